"""Bits-per-dim evaluation without a GPU (fixture: tests/golden/make_golden_bpd.py): the step rows against the schedule
buffers and the scalars recorded from the running reference, bit for bit; ``times`` handling; every refusal, on stub nets;
the additions to the C ABI (declared, bound, exported, the struct's size, ABI version 9); and the CPU restatement
(tests/bpd_oracle.py) over the oracle U-Net against the reference's fp64 arrays, which ties the row layout and the kernels'
formulas to the reference."""
import ctypes as C
import inspect
import os
import re
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import bpd as Bp
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo

import bpd_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(GOLDEN, "bpd.pt"), weights_only=True)


@pytest.fixture(scope="module")
def learned_scalars():
    return torch.load(os.path.join(GOLDEN, "learned.pt"), weights_only=True)["scalars"]


def _stub_net(**kw):
    base = dict(random_or_learned_sinusoidal_cond=False, self_condition=False, text_condition=False, out_dim=3, channels=3,
                cfg=types.SimpleNamespace(cond_channels=0), device="cpu", downsample_factor=2, seq1d=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


# ---- the step rows -----------------------------------------------------------------------------------------------------
SCHEDULES = {"linear_50": ("linear", 50), "cosine_24": ("cosine", 24), "linear_1000": ("linear", 1000)}
BUFFERS = ((Bp.RECIP, "sqrt_recip_alphas_cumprod"), (Bp.RECIPM1, "sqrt_recipm1_alphas_cumprod"),
           (Bp.COEF1, "posterior_mean_coef1"), (Bp.COEF2, "posterior_mean_coef2"),
           (Bp.POST_LOG, "posterior_log_variance_clipped"), (Bp.SQRT_AC, "sqrt_alphas_cumprod"),
           (Bp.SQRT_1M_AC, "sqrt_one_minus_alphas_cumprod"))


@pytest.mark.parametrize("key", list(SCHEDULES))
def test_step_rows_equal_the_schedule_bit_for_bit(learned_scalars, key):
    name, T = SCHEDULES[key]
    sched = dm.make_schedule(T, name)
    times, tab = dm.bpd_step_table(sched)
    assert times == list(reversed(range(T))) and tab.shape == (T, Bp.COLS) and tab.dtype == torch.float32
    assert Bp.COLS == _lib.DM_BPD_COEFS == 16
    idx = torch.tensor(times)
    for col, buf in BUFFERS:
        assert sched[buf].dtype == torch.float32 and torch.equal(tab[:, col], sched[buf][idx]), buf
    # min_log / max_log as the reference's `extract` returned them at every t (recorded by make_golden_learned.py)
    rec = learned_scalars[key]
    assert torch.equal(tab[:, Bp.POST_LOG].double(), rec[idx, 0]) and torch.equal(tab[:, Bp.MAX_LOG].double(), rec[idx, 1])
    assert torch.equal(tab[:, Bp.T0], (idx == 0).float()) and int(tab[:, Bp.T0].sum()) == 1 and not bool(tab[:, 9:].any())
    # columns 0..4, 6, 7 sit where ddpm_step_table has its own (the kernels read both with ddpm_coefs)
    from diffusion_models_amd.spec import ddpm_step_table

    _, ddpm = ddpm_step_table(sched)
    assert torch.equal(tab[:, :4], ddpm[:, :4]) and torch.equal(tab[:, 6:8], ddpm[:, 6:8])
    # a subset keeps the caller's order
    sub_t, sub = dm.bpd_step_table(sched, (T - 1, 3, 0, 7))
    assert sub_t == [T - 1, 3, 0, 7] and torch.equal(sub, tab[[0, T - 1 - 3, T - 1, T - 1 - 7]])
    a, lv = Bp.prior_scalars(sched)
    assert a == float(sched["sqrt_alphas_cumprod"][T - 1]) and lv == float(sched["log_one_minus_alphas_cumprod"][T - 1])


@pytest.mark.parametrize("key,name,T", [("linear", "linear", 1000), ("cosine", "cosine", 1000), ("sigmoid", "sigmoid", 1000),
                                        ("linear250", "linear", 250)])
def test_step_rows_equal_the_schedule_goldens_bit_for_bit(key, name, T):
    """Against the buffers recorded from the reference (tests/golden/schedule.pt), not against make_schedule."""
    ref = torch.load(os.path.join(GOLDEN, "schedule.pt"), weights_only=True)["sched"][key]
    times, tab = dm.bpd_step_table(dm.make_schedule(T, name))
    idx = torch.tensor(times)
    assert times == list(reversed(range(T))) and int(ref["betas"].shape[0]) == T
    for col, buf in BUFFERS:
        assert torch.equal(tab[:, col], ref[buf][idx]), buf
    assert torch.equal(tab[:, Bp.MAX_LOG], torch.log(ref["betas"])[idx])
    sub = dm.bpd_step_table(dm.make_schedule(T, name), (T - 1, 37, 1, 0))[1]
    for col, buf in BUFFERS:
        assert torch.equal(sub[:, col], ref[buf][torch.tensor([T - 1, 37, 1, 0])]), buf
    a, lv = Bp.prior_scalars(dm.make_schedule(T, name))
    assert a == float(ref["sqrt_alphas_cumprod"][T - 1]) and lv == float(ref["log_one_minus_alphas_cumprod"][T - 1])


def test_times_handling():
    assert Bp.bpd_times(5) == ([4, 3, 2, 1, 0], True)
    assert Bp.bpd_times(5, range(5)) == ([0, 1, 2, 3, 4], True)  # all of them in any order is the whole bound
    assert Bp.bpd_times(5, (4, 0)) == ([4, 0], False)
    assert Bp.bpd_times(1000, torch.tensor([999, 500, 37, 1, 0])) == ([999, 500, 37, 1, 0], False)
    for bad, msg in (((), "empty"), ((5,), "lie in"), ((-1, 2), "lie in"), ((3, 3), "twice")):
        with pytest.raises(ValueError, match=msg):
            Bp.bpd_times(5, bad)


class _FakeLib:
    """Stands where libdm_hip.so is called: fills the outputs of dm_eval_bpd with recognisable values."""

    def __init__(self):
        self.calls = []

    def dm_eval_bpd(self, handle, args):
        a = args._obj
        self.calls.append({f: getattr(a, f) for f, _ in _lib.BpdArgs._fields_ if f not in ("times_host", "table_host")})
        self.calls[-1]["times"] = [a.times_host[i] for i in range(a.n_steps)]
        self.calls[-1]["table"] = [a.table_host[i] for i in range(a.n_steps * _lib.DM_BPD_COEFS)]
        n = a.n_steps * a.B * 3
        (C.c_float * n).from_address(a.terms_out)[:] = [float(i) for i in range(n)]
        (C.c_float * a.B).from_address(a.prior_out)[:] = [0.5] * a.B
        return 0


def test_total_is_none_on_a_subset_and_the_columns_follow_times():
    obj = dm.DenoisingDiffusion(_stub_net(), image_size=16, timesteps=50, objective="pred_v")
    obj._lib = _FakeLib()
    obj._stream = lambda: None
    obj.model._handle = None
    img = torch.rand(2, 3, 16, 16)
    calls = []

    def noise(shape):
        calls.append(tuple(shape))
        return torch.zeros(shape)

    out = obj.calc_bpd_loop(img, False, times=(49, 7, 0), noise=noise, sample_offset=4)
    assert out["total_bpd"] is None and out["times"] == [49, 7, 0] and calls == [(2, 3, 16, 16)] * 3
    assert set(out) == {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse", "times"}
    a = obj._lib.calls[0]
    assert (a["learned"], a["objective"], a["clip_denoised"], a["n_steps"], a["B"], a["H"], a["W"]) == (0, 2, 0, 3, 2, 16, 16)
    assert a["times"] == [49, 7, 0] and a["sample_offset"] == 4 and a["noise"] and not a["ctx"] and not a["cond"]
    assert a["table"] == dm.bpd_step_table(obj._sched, (49, 7, 0))[1].reshape(-1).tolist()
    assert (a["prior_sqrt_ac"], a["prior_logvar"]) == tuple(torch.tensor(Bp.prior_scalars(obj._sched)).tolist())
    # terms_out is (n, B, 3): column k of image b is entry (k, b)
    want = torch.arange(3 * 2 * 3, dtype=torch.float32).reshape(3, 2, 3).permute(1, 0, 2)
    for i, k in enumerate(("vb", "xstart_mse", "mse")):
        assert out[k].shape == (2, 3) and torch.equal(out[k], want[:, :, i])
    assert torch.equal(out["prior_bpd"], torch.full((2,), 0.5))
    full = obj.calc_bpd_loop(img, seed=3)
    assert full["times"] == list(reversed(range(50))) and full["vb"].shape == (2, 50)
    assert torch.equal(full["total_bpd"], (full["vb"].double().sum(1) + 0.5).float())
    b = obj._lib.calls[1]
    assert b["seed"] == 3 and not b["noise"] and b["clip_denoised"] == 1
    with pytest.raises(AssertionError, match="height and width"):
        obj.calc_bpd_loop(torch.rand(2, 3, 8, 8))
    with pytest.raises(ValueError, match="twice"):
        obj.calc_bpd_loop(img, times=(1, 1))
    lv = dm.LearnedGaussianDiffusion(_stub_net(out_dim=6), image_size=16, timesteps=50, objective="pred_x0")
    lv._lib, lv._stream, lv.model._handle = _FakeLib(), (lambda: None), None
    lv.calc_bpd_loop(img, times=(3,))
    assert (lv._lib.calls[0]["learned"], lv._lib.calls[0]["objective"]) == (1, 0)  # the first half is noise whatever it says


def test_bpd_global_passes_the_normalised_times():
    obj = dm.DenoisingDiffusion(_stub_net(), image_size=16, timesteps=50)
    obj._lib, obj._stream, obj.model._handle = _FakeLib(), (lambda: None), None
    img = torch.rand(3, 3, 16, 16)
    # a tensor as long as the batch is not a per-image keyword, and a one-shot iterator is read once
    for times in (torch.tensor([49, 7, 0]), iter((49, 7, 0))):
        out = dm.bpd_global(obj, img, seed=5, times=times)
        assert out["times"] == [49, 7, 0] and out["vb"].shape == (3, 3) and out["total_bpd"] is None
        assert obj._lib.calls[-1]["times"] == [49, 7, 0] and obj._lib.calls[-1]["seed"] == 5
    full = dm.bpd_global(obj, img, seed=5)
    assert full["times"] == list(reversed(range(50))) and full["total_bpd"].shape == (3,)


def test_signatures():
    for cls, extra in ((dm.DenoisingDiffusion, ()), (dm.LearnedGaussianDiffusion, ()),
                       (dm.TextConditionalDenoisingDiffusion, ("text_emb",)),
                       (dm.ImageConditionalDenoisingDiffusion, ("cond",))):
        p = inspect.signature(cls.calc_bpd_loop).parameters
        assert list(p)[:3] == ["self", "img", "clip_denoised"] and p["clip_denoised"].default is True
        kwonly = {k for k, v in p.items() if v.kind is inspect.Parameter.KEYWORD_ONLY}
        assert kwonly == {"times", "noise", "seed", "sample_offset"} | set(extra), cls
        assert p["sample_offset"].default == 0 and all(p[k].default is None for k in kwonly - {"sample_offset"})
    g = inspect.signature(dm.bpd_global).parameters
    assert list(g)[:4] == ["diffusion", "img", "seed", "group"]
    for name in ("bpd_global", "bpd_step_table", "bpd_times"):
        assert name in dm.__all__ and hasattr(dm, name)


# ---- refusals ----------------------------------------------------------------------------------------------------------
REFUSING = (dm.LatentDiffusion, dm.TextConditionalLatentDiffusion, dm.ImageConditionalLatentDiffusion,
            dm.DenoisingDiffusion1D, dm.RePaintGaussianDiffusion, dm.WeightedObjectiveGaussianDiffusion,
            dm.ClassifierGuidedGaussianDiffusion)


@pytest.mark.parametrize("cls", REFUSING, ids=lambda c: c.__name__)
def test_classes_without_a_bound_refuse_with_a_reason(cls):
    obj = cls.__new__(cls)  # the refusal comes before anything of the object is read
    assert isinstance(cls._bpd_refusal, str) and len(cls._bpd_refusal) > 20
    with pytest.raises(NotImplementedError, match=re.escape(cls._bpd_refusal[:30])):
        obj.calc_bpd_loop(torch.rand(1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match=cls.__name__):
        dm.bpd_global(obj, torch.rand(1, 3, 16, 16), seed=1)
    if "Latent" in cls.__name__:
        assert "8-bit" in cls._bpd_refusal


def test_self_condition_refuses_and_the_four_classes_do_not():
    for cls in (dm.DenoisingDiffusion, dm.TextConditionalDenoisingDiffusion, dm.ImageConditionalDenoisingDiffusion,
                dm.LearnedGaussianDiffusion):
        assert cls._bpd_refusal is None
    obj = dm.DenoisingDiffusion(_stub_net(self_condition=True), image_size=16, timesteps=50)
    with pytest.raises(NotImplementedError, match="self_condition"):
        obj.calc_bpd_loop(torch.rand(1, 3, 16, 16))
    ic = dm.ImageConditionalDenoisingDiffusion(_stub_net(cfg=types.SimpleNamespace(cond_channels=3)), image_size=16, timesteps=50)
    with pytest.raises(AssertionError, match="cond="):
        ic.calc_bpd_loop(torch.rand(1, 3, 16, 16))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
NEW = ("dm_eval_bpd", "dm_op_bpd_step_in", "dm_op_bpd_terms", "dm_op_bpd_prior")


def test_abi_additions_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "dm_hip.h")) as f:
        src = f.read()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 9 and lib.dm_abi_version() == 9  # additions only
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, src), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"#define DM_BPD_COEFS 16\b", src) and re.search(r"#define DM_BPD_CHUNK %d\b" % _lib.DM_BPD_CHUNK, src)
    # the struct, field by field, against the header's declaration
    body = re.search(r"typedef struct dm_bpd_args \{(.*?)\} dm_bpd_args;", src, re.S).group(1)
    declared = []
    for line in body.split(";"):
        line = line.strip()
        if line:
            names = line.replace("*", " ").split()
            declared += [n.strip(",") for n in (names[-3:] if line.startswith("int32_t B") else names[-1:])]
    assert declared == [f for f, _ in _lib.BpdArgs._fields_]
    assert C.sizeof(_lib.BpdArgs) == 136  # csrc/dm_bpd.inc asserts the same of the C struct
    assert _lib.BpdArgs.stream.offset == 128 and _lib.BpdArgs.terms_out.offset == 96


# ---- the restatement against the reference's fp64 arrays ---------------------------------------------------------------
def _model(golden, case):
    kw = golden["unet_kw"][case["kind"]]
    cfg = UnetConfig(**kw)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=golden["salt"])
    extra = case["extra"]
    if case["kind"] == "text":
        return lambda x, t: uo.unet_forward(sd, cfg, x, t, text_emb=extra)
    if case["kind"] == "imgcond":
        return lambda x, t: uo.unet_forward(sd, cfg, x, t, cond=extra)
    return lambda x, t: uo.unet_forward(sd, cfg, x, t)


@pytest.mark.parametrize("key", ["learned_cosine24", "v_sigmoid24", "x0_cosine24_noclip", "noise_linear1000_subset"])
def test_restated_loop_matches_the_reference(golden, key):
    c = golden["cases"][key]
    img = golden["image_u8"].float() / 255.0
    sched = dm.make_schedule(c["timesteps"], c["beta_schedule"])
    with torch.inference_mode():
        got = O.loop(_model(golden, c), sched, img, c["times"], so.NoiseStream(c["noise_seed"]), c["kind"] == "learned",
                     _lib.OBJECTIVES[c["objective"]], c["clip_denoised"])
    assert (got["total_bpd"] is None) == (c["times"] is not None)
    for name, want in c["want"].items():
        rel = (got[name].double() - want).abs() / want.abs()
        exc = c["excepted"].get(name)
        if exc:  # the column the reference's fp32 run loses to cancellation: its absolute error, in bits
            cols = [got["times"].index(t) for t in exc["times"]]
            abs_err = float((got[name].double() - want)[:, cols].abs().max())
            print(f"{key} {name} at t in {exc['times']}: restatement vs reference fp64 {abs_err:.2e} bits "
                  f"(reference fp32 {exc['ref_abs_err']:.2e} bits)")
            assert abs_err <= 4 * exc["ref_abs_err"]
            rel = rel[:, [k for k in range(rel.shape[1]) if k not in cols]]
        err = float(rel.max())
        # fp32 torch arithmetic on both sides (the U-Net is the oracle's, not the reference module): the reference's own
        # fp32 error, with room for the other U-Net code
        lim = max(16 * c["ref_err"][name], 1e-4)
        print(f"{key} {name}: restatement vs reference fp64 {err:.2e} (reference fp32 {c['ref_err'][name]:.2e})")
        assert got[name].shape == want.shape and err <= lim, (name, err, lim)
