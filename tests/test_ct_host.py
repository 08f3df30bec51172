"""Continuous-time Gaussian diffusion, host logic, no GPU: the step and training tables against the scalars recorded from the
running reference BIT FOR BIT (the kernels only multiply / add / divide / clamp by them), the CPU restatement of the
kernels' arithmetic (tests/ct_oracle.py) against the reference's recorded ``p_sample`` steps and ``sample()`` outputs, the
mirrored surface, the refusals, the struct bindings and the order of draws.  Fixture: tests/golden/make_golden_ct.py."""
import ctypes
import inspect
import math
import os
import re
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import continuous as K
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo

import ct_oracle as co
from conftest import ROOT, load_golden, rel_l2

STEP_TOL = 1e-4  # the project's ceiling for one forward
LOOP_TOL = 1e-3  # the project's ceiling for a sampling loop
CLASSES = {"noise": dm.ContinuousTimeGaussianDiffusion, "v": dm.VParamContinuousTimeGaussianDiffusion}
OBJ = {"noise": co.NOISE, "v": co.V}


@pytest.fixture(scope="module")
def golden():
    return load_golden("ct.pt")


def _sched(kind, kw):
    return "cosine" if kind == "v" else kw.get("noise_schedule", "linear")


def _check_rows(tab, rec, names, tag):
    """Every table column against the recorded scalar of the same p_mean_variance call, bit for bit."""
    col = {n: j for j, n in enumerate(names)}
    assert tab.shape[0] == rec.shape[0] and tab.dtype == torch.float32
    for i in range(tab.shape[0]):
        want = {K.LOG_SNR: "log_snr", K.ALPHA: "alpha", K.SIGMA: "sigma", K.ALPHA_NEXT: "alpha_next", K.C_: "c"}
        for j, name in want.items():
            assert float(tab[i, j]) == float(rec[i, col[name]]), (tag, i, name, float(tab[i, j]), float(rec[i, col[name]]))
        sv = float(rec[i, col["sqrt_var"]])
        if math.isnan(sv):  # p_sample took no square root: time_next == 0, the mean is returned
            assert i == tab.shape[0] - 1 and float(tab[i, K.SQRT_VAR]) == 0.0, (tag, i)
        else:
            assert float(tab[i, K.SQRT_VAR]) == sv != 0.0, (tag, i)
            # sqrt(posterior_variance) of the recorded fp32 variance is what p_sample multiplies the noise by
            assert sv == float(torch.tensor(float(rec[i, col["posterior_variance"]]), dtype=torch.float32).sqrt())
        # the three derived entries are 0-dim fp32 expressions of recorded values (the reference forms them inline)
        f32 = lambda name: torch.tensor(float(rec[i, col[name]]), dtype=torch.float32)  # noqa: E731
        assert float(tab[i, K.ONE_M_C]) == float(1 - f32("c"))
        assert float(tab[i, K.AN_OVER_A]) == float(f32("alpha_next") / f32("alpha"))
        assert float(tab[i, K.C_SIGMA]) == float(f32("c") * f32("sigma"))
        assert not bool(tab[i, K.LOSS_W:].any())


def test_step_tables_bitwise(golden):
    names = golden["names"]
    for n, steps in golden["steps"].items():
        assert torch.equal(torch.linspace(1., 0., n + 1), steps)
        for sched in ("linear", "cosine"):
            _check_rows(dm.ct_step_table(n, sched), golden["scalars"][f"{sched}_{n}"], names, (sched, n))
    _check_rows(dm.ct_step_table(12, "cosine"), golden["scalars"]["v_12"], names, "v_12")
    for key, c in golden["loops"].items():
        _check_rows(dm.ct_step_table(c["n"], _sched(c["kind"], c["ct_kw"])), c["scalars"], names, key)


def test_cosine_t1_row_is_the_references_rounding_artefact(golden):
    """At t = 1 cos(pi / 2) is not 0 in fp32: log-SNR ~ -33.9 and alpha ~ 4e-8 are what the reference computes, and the
    table holds exactly them -- a 'cleaner' (fp64, or clamped) formula would not."""
    rec = golden["scalars"]["cosine_8"][0]
    row = dm.ct_step_table(8, "cosine")[0]
    assert float(row[K.LOG_SNR]) == float(rec[0]) and -34.5 < float(row[K.LOG_SNR]) < -33.0
    assert float(row[K.ALPHA]) == float(rec[3]) and 3e-8 < float(row[K.ALPHA]) < 6e-8
    exact = float(dm.alpha_cosine_log_snr(torch.tensor(1.0, dtype=torch.float64)))
    assert abs(exact - float(row[K.LOG_SNR])) > 1.0  # the fp64 value is another number altogether
    assert torch.isfinite(dm.ct_step_table(500, "cosine")).all() and torch.isfinite(dm.ct_step_table(500, "linear")).all()


def test_train_table_matches_q_sample_scalars(golden):
    q = golden["q_sample"]
    for key, sched in (("noise_linear", "linear"), ("noise_cosine", "cosine"), ("v", "cosine")):
        tab = dm.ct_train_table(q["times"], sched)
        assert torch.equal(tab[:, K.LOG_SNR], q[key][1]), key
        assert bool((tab[:, K.LOSS_W] == 1).all())
    v = q["v"]
    tab = dm.ct_train_table(q["times"], "cosine")
    assert torch.equal(tab[:, K.ALPHA], v[2].reshape(-1)) and torch.equal(tab[:, K.SIGMA], v[3].reshape(-1))
    # min-SNR: snr on both sides of gamma, the weight the reference's expression gives
    c = golden["train"]["noise_cos_minsnr"]
    snr = c["snr"]
    assert bool((snr > 5).any()) and bool((snr < 5).any())
    tab = dm.ct_train_table(c["times"][0], "cosine", True, 5)
    assert torch.equal(tab[:, K.LOSS_W], snr.clamp(min=5) / snr)
    assert torch.equal(tab[:, K.LOG_SNR].exp(), snr)


def _fwd(ukw, salt):
    cfg = UnetConfig(channels=3, **ukw)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt)
    return lambda x, t: uo.unet_forward(sd, cfg, x, t)


def test_restated_p_sample_reproduces_the_reference(golden):
    for key, g in golden["steps_single"].items():
        fwd = _fwd(g["unet_kw"], g["salt"])
        sched = _sched(g["kind"], g["ct_kw"])
        clip = g["ct_kw"].get("clip_sample_denoised", True)
        for st in g["steps"]:
            row = K.ct_step_row(sched, st["time"], st["time_next"])
            last = float(st["time_next"]) == 0
            assert (float(row[K.SQRT_VAR]) == 0) == last
            eps = None if last else so.NoiseStream(st["noise_seed"])(g["x"].shape)
            with torch.inference_mode():
                got = co.p_sample(fwd, g["x"], row, eps, OBJ[g["kind"]], clip)
            err = rel_l2(got, st["y"])
            print(f"restated p_sample {key} step {st['i']}: {err:.3e}")
            assert err <= STEP_TOL, (key, st["i"], err)


@pytest.mark.parametrize("key", ["v_n8", "v_n8_noclip", "lin_n8", "cos_n12", "v_d64_n6", "v_rff_n8"])
def test_restated_loop_reproduces_the_reference(golden, key):
    c = golden["loops"][key]
    share = float(((c["sample"] == 0) | (c["sample"] == 1)).float().mean())
    assert share <= 0.5, (key, share)  # the comparison is not carried by the final clamp
    shape = (c["batch"], 3, c["image_size"], c["image_size"])
    tab = dm.ct_step_table(c["n"], _sched(c["kind"], c["ct_kw"]))
    with torch.inference_mode():
        got = co.sample(_fwd(c["unet_kw"], c["salt"]), tab, shape, so.NoiseStream(c["noise_seed"]), OBJ[c["kind"]],
                        c["ct_kw"].get("clip_sample_denoised", True))
    err = rel_l2(got, c["sample"])
    print(f"restated loop {key} (N = {c['n']}, {share:.0%} of the pixels on the final clamp): {err:.3e}")
    assert err <= LOOP_TOL


def test_restated_training_passes_agree_with_autograd_in_fp64():
    g = torch.Generator().manual_seed(9)
    B, shape = 5, (5, 3, 8, 8)
    times = torch.tensor([0.0, 0.2, 0.5, 0.9, 1.0])
    for objective, sched, minsnr in ((co.NOISE, "linear", False), (co.NOISE, "cosine", True), (co.V, "cosine", False)):
        tab = dm.ct_train_table(times, sched, minsnr, 5).double()
        img = torch.rand(shape, generator=g, dtype=torch.float64)
        eps = torch.randn(shape, generator=g, dtype=torch.float64)
        F = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
        pad = lambda col: tab[:, col].reshape(B, 1, 1, 1)  # noqa: E731
        x0 = img * 2 - 1
        x = x0 * pad(K.ALPHA) + eps * pad(K.SIGMA)
        target = eps if objective == co.NOISE else pad(K.ALPHA) * eps - pad(K.SIGMA) * x0
        losses = torch.nn.functional.mse_loss(F, target, reduction="none").reshape(B, -1).mean(dim=1) * tab[:, K.LOSS_W]
        loss = losses.mean() * 0.5
        loss.backward()
        rx, rt = co.noise_in(img, eps, tab, objective)
        assert torch.equal(rx, x) and torch.equal(rt, target)
        rloss, rdF = co.loss_and_dF(F.detach(), rt, tab, loss_scale=0.5)
        assert abs(float(rloss) - float(loss.detach())) <= 1e-14 * abs(float(loss.detach()))
        assert float((rdF - F.grad).norm() / F.grad.norm()) <= 1e-14
        if objective == co.V:  # F.mse_loss over the whole batch is the same quantity with w = 1
            whole = torch.nn.functional.mse_loss(F.detach(), target) * 0.5
            assert abs(float(rloss) - float(whole)) <= 1e-14 * float(whole)


@pytest.mark.parametrize("key", ["noise_lin", "noise_cos_minsnr", "v_learned", "v_random", "noise_lin_accumulate2"])
def test_restatement_reproduces_the_reference_loss(golden, key):
    c = golden["train"][key]
    fwd = _fwd(c["unet_kw"], c["salt"])
    kw = c["ct_kw"]
    total = 0.0
    with torch.inference_mode():
        for img, t, noise in zip(c["imgs"], c["times"], c["noises"]):
            tab = dm.ct_train_table(t, _sched(c["kind"], kw), kw.get("min_snr_loss_weight", False), kw.get("min_snr_gamma", 5))
            total += float(co.ct_loss(fwd, img, noise, tab, OBJ[c["kind"]], loss_scale=1.0 / c["micro"]))
    err = abs(total - c["loss"]) / abs(c["loss"])
    print(key, "restated loss", total, "reference", c["loss"], "rel", err)
    assert err <= 1e-5
    assert 0 <= c["ref_err_loss"] < 1e-5 and 0 <= c["ref_err_grad_max"] < 1e-4


# ---- interface ------------------------------------------------------------------------------------------------------
def _stub_net(**kw):
    base = dict(random_or_learned_sinusoidal_cond=True, self_condition=False, text_condition=False, out_dim=3, channels=3,
                cfg=types.SimpleNamespace(cond_channels=0), device="cpu", downsample_factor=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("kind", ["noise", "v"])
def test_surface_matches_the_reference(golden, kind):
    cls, s = CLASSES[kind], golden["surface"][kind]
    sig = inspect.signature(cls.__init__)
    ours = [(p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name)
            for p in sig.parameters.values() if p.name != "self"]
    want = [tuple(v) for v in s["init_params"]]
    assert ours[:len(want)] == want
    assert [n for n, _, _ in ours[len(want):]] == ["use_graph"]
    assert all(k == "KEYWORD_ONLY" for _, _, k in ours[len(want):])  # extensions never shift a reference argument
    for name, params in s["methods"].items():
        got = list(inspect.signature(getattr(cls, name)).parameters.values())[1:]
        assert [p.name for p in got[:len(params)]] == params, name
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in got[len(params):]), name
    for name in s["properties"]:
        assert isinstance(getattr(cls, name), property)
    for name in ("eval", "parameters", "sample_shape", "train", "state_dict", "load_state_dict", "forward"):
        assert callable(getattr(cls, name))
    assert cls.__call__ is cls.forward
    fwd = list(inspect.signature(cls.forward).parameters.values())[1:]
    assert [p.name for p in fwd] == ["img", "times", "noise", "loss_scale", "accumulate", "sync"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in fwd[1:])
    pl = list(inspect.signature(cls.p_losses).parameters.values())[1:]
    assert [p.name for p in pl] == ["x_start", "times", "noise", "loss_scale", "accumulate", "sync"]
    cfg = UnetConfig(channels=3, **golden["state_dict_unet_kw"])
    assert golden["state_dict_keys"][kind] == ["model." + n for n, _ in dm.unet_param_spec(cfg)]
    obj = cls(_stub_net(state_dict=lambda: {"a.b": torch.zeros(1)}), image_size=16)
    assert list(obj.state_dict()) == ["model.a.b"] and obj.sample_shape() == (3, 16, 16) and obj.num_sample_steps == 500
    assert obj.eval() is obj and obj.device == "cpu"
    t = torch.tensor([0.0, 0.3, 1.0])
    want_fn = dm.beta_linear_log_snr if kind == "noise" else dm.alpha_cosine_log_snr
    assert torch.equal(obj.log_snr(t), want_fn(t))


def test_refusals():
    for cls in CLASSES.values():
        with pytest.raises(AssertionError):
            cls(_stub_net(random_or_learned_sinusoidal_cond=False), image_size=16)
        with pytest.raises(AssertionError):
            cls(_stub_net(self_condition=True), image_size=16)
        with pytest.raises(NotImplementedError, match="text-conditional"):
            cls(_stub_net(text_condition=True), image_size=16)
        with pytest.raises(NotImplementedError, match="image-conditional"):
            cls(_stub_net(cfg=types.SimpleNamespace(cond_channels=3)), image_size=16)
        with pytest.raises(ValueError, match="learned variance"):
            cls(_stub_net(out_dim=6), image_size=16)
        obj = cls(_stub_net(), image_size=16)
        # a net that is not a library Unet: refused before any tensor or the device is touched
        with pytest.raises(NotImplementedError, match="train"):
            obj(torch.zeros(1, 3, 16, 16))
        with pytest.raises(NotImplementedError, match="train"):
            obj.p_losses(torch.zeros(1, 3, 16, 16), torch.zeros(1))
        with pytest.raises(NotImplementedError, match="train"):
            obj.train()
        assert obj.train(False) is obj
        # train_step keeps the three kinds of injected draws apart
        for bad in (dict(t=[torch.zeros(1, dtype=torch.long)]), dict(sigmas=[torch.ones(1)]), dict(text_mask=[None])):
            with pytest.raises(ValueError, match="times="):
                dm.train_step(obj, [torch.zeros(1, 3, 16, 16)], **bad)
    with pytest.raises(NotImplementedError, match="learned"):
        dm.ContinuousTimeGaussianDiffusion(_stub_net(), image_size=16, noise_schedule="learned")
    with pytest.raises(ValueError, match="unknown noise schedule"):
        dm.ContinuousTimeGaussianDiffusion(_stub_net(), image_size=16, noise_schedule="sigmoid")
    assert dm.ContinuousTimeGaussianDiffusion(_stub_net(), image_size=16, noise_schedule="cosine").log_snr is dm.alpha_cosine_log_snr
    edm = dm.ElucidatedDiffusion(_stub_net(), image_size=16)
    with pytest.raises(ValueError, match="times="):
        dm.train_step(edm, [torch.zeros(1, 3, 16, 16)], times=[torch.zeros(1)])
    sig = inspect.signature(dm.train_step).parameters
    assert sig["times"].kind is inspect.Parameter.KEYWORD_ONLY and sig["times"].default is None


def _declared(struct):
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    declared = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*([\w\s,]+)", decl)
        assert m, decl
        for name in (n.strip() for n in m.group(4).split(",")):
            declared.append((name, "pointer" if m.group(3) else ctype[m.group(2)]))
    return declared, src


@pytest.mark.parametrize("struct,binding,size", [("dm_ct_args", "CtArgs", 88), ("dm_ct_train_args", "CtTrainArgs", 72)])
def test_struct_bindings_match_the_header(struct, binding, size):
    """The bindings are written by hand: field names, order, C types and offsets are those of the header's declaration
    under natural alignment (LP64: pointers and uint64 are 8 bytes, the rest 4)."""
    declared, src = _declared(struct)
    cls = getattr(_lib, binding)
    bound = []
    for name, t in cls._fields_:
        is_ptr = t is ctypes.c_void_p or isinstance(t, type(ctypes.POINTER(ctypes.c_float)))
        bound.append((name, "pointer" if is_ptr else t))
    assert bound == declared
    off, offsets = 0, {}
    for name, t in declared:
        sz = 8 if t == "pointer" else ctypes.sizeof(t)
        off = (off + sz - 1) // sz * sz
        offsets[name] = off
        off += sz
    assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == offsets
    assert ctypes.sizeof(cls) == (off + 7) // 8 * 8 == size
    assert _lib.DM_CT_COEFS == int(re.search(r"#define DM_CT_COEFS (\d+)", src).group(1)) == K.COLS
    assert (_lib.CT_PRED_NOISE, _lib.CT_PRED_V) == (int(re.search(r"#define DM_CT_PRED_NOISE (\d+)", src).group(1)),
                                                    int(re.search(r"#define DM_CT_PRED_V (\d+)", src).group(1)))
    assert K.LOSS_W == 9 < K.COLS
    # additions only: the EDM structs keep their sizes and the ABI version its value
    assert ctypes.sizeof(_lib.EdmArgs) == 88 and ctypes.sizeof(_lib.EdmTrainArgs) == 72 and _lib.ABI_VERSION == 9


def _shell_net():
    """A handle-less ``Unet`` shell marked as armed: nothing reaches the library or a device."""
    from diffusion_models_amd.unet import Unet

    net = object.__new__(Unet)  # no constructor: no handle is created, __del__ finds none to destroy
    net.__dict__.update(_stub_net(cfg=types.SimpleNamespace(cond_channels=0, downsample_factor=2)).__dict__, _training=True,
                        _loaded=True)
    net._handle = ctypes.c_void_p(1)
    return net


@pytest.mark.parametrize("kind", ["noise", "v"])
def test_forward_draws_times_before_the_noise(kind):
    class _Stop(Exception):
        pass

    net = _shell_net()
    try:
        obj = CLASSES[kind](net, image_size=16)
        calls, drawn = [], []
        real = obj._draw_times
        obj._draw_times = lambda n: calls.append(("times", n)) or drawn.append(real(n)) or drawn[-1]

        def randn(shape, *a, **k):
            calls.append(("noise", tuple(shape)))
            raise _Stop

        obj._randn = randn
        torch.manual_seed(77)
        with pytest.raises(_Stop):
            obj(torch.zeros(6, 3, 16, 16))
        assert calls == [("times", 6), ("noise", (6, 3, 16, 16))]
        torch.manual_seed(77)
        want = torch.zeros((6,)).float().uniform_(0, 1)  # the reference's draw, from torch's global generator
        assert torch.equal(drawn[0], want) and float(want.min()) >= 0 and float(want.max()) < 1
        calls.clear()
        with pytest.raises(RuntimeError, match="times has 5 entries"):
            obj(torch.zeros(6, 3, 16, 16), times=torch.ones(5) * 0.5, noise=torch.zeros(6, 3, 16, 16))
        assert calls == []
    finally:
        net._handle = ctypes.c_void_p()  # nothing for __del__ to hand to the library


def test_sampling_draw_order_of_an_injected_noise_source():
    """One call for the start image, then one per step except the last -- the reference's order (randn in p_sample_loop,
    randn_like in every p_sample whose time_next != 0).  The run stops where it would ask for the stream: nothing reaches
    the library or a device."""
    class _Stop(Exception):
        pass

    def stop():
        raise _Stop

    net = _shell_net()
    try:
        for kind, n in (("v", 5), ("noise", 1)):
            obj = CLASSES[kind](net, image_size=16, num_sample_steps=n)
            obj._stream = stop
            calls = []
            with pytest.raises(_Stop):
                obj.sample(batch_size=2, noise=lambda shape: calls.append(tuple(shape)) or torch.zeros(shape))
            assert calls == [(2, 3, 16, 16)] * n  # the start image + n - 1 of the n steps
    finally:
        net._handle = ctypes.c_void_p()
