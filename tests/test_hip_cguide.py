"""Classifier-guided DDPM sampling on the GPU (fixture: tests/golden/make_golden_classifier_guidance.py, from the reference).

* ``dm_op_cg_mean`` / ``dm_op_cg_finish`` against the same expressions in fp64 torch (tests/cguide_oracle.py).  The bound
  is elementwise and derived from the operand magnitudes: with contraction off every product and every sum rounds once
  (relative error <= 2^-24), so the first-order error of ``mean = c2 clamp(c0 x - c1 e) + c3 x`` is at most
  ``2^-23 (|c2| (|c0 x| + |c1 e|) + |c2 x0| + |c3 x|)`` and that of ``(mean + c8 g) + c4 z`` at most
  ``2^-23 (|mean| + |c8 g| + |c4 z|)``; the limit is twice that (second-order terms, the clamp edge).
* single ``p_sample`` steps at the three recorded times, <= 1e-4 (the project's bar for one step);
* the three recorded loops on identical noise, every frame of ``return_all_timesteps``: <= max(1e-4, 4 x the reference's
  own fp32-vs-fp64 distance of that loop).  Measured on an MI355X: see DESIGN.md 7j.
* equivalences that must hold bit for bit, graph reuse, and host errors.
Measured errors are printed (run with -s to see them)."""
import numpy as np
import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import classifier_guidance as G
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import cguide_oracle as CO
import philox_ref
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_TOL = LOOP_TOL = 1e-4
ULP1 = 2.0 ** -23
POISON = float("nan")


@pytest.fixture(scope="module")
def golden():
    return load_golden("classifier_guidance.pt")


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


_NETS = {}


def _net(c):
    key = (c["channels"], c["self_condition"], c["salt"])
    if key not in _NETS:
        kw = dict(channels=c["channels"], self_condition=c["self_condition"], **c["unet_kw"])
        u = dm.Unet(device=DEV, **kw)
        u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(**kw)), salt=c["salt"]))
        _NETS[key] = u
    return _NETS[key]


def _obj(c, **kw):
    return dm.ClassifierGuidedGaussianDiffusion(_net(c), image_size=c["image_size"], timesteps=c["timesteps"],
                                                beta_schedule=c["beta_schedule"], objective=c["objective"], **kw)


def _guide(c, scale=None, labels=None, calls=None):
    cond_fn = CO.make_cond_fn(c["classifier"], c["timesteps"], device=DEV, calls=calls)
    kw = dict(y=torch.tensor(c["labels"] if labels is None else labels, device=DEV), scale=c["scale"] if scale is None else scale)
    return cond_fn, kw


def _zero_fn(calls=None):
    def cond_fn(x, t, **kw):
        if calls is not None:
            calls.append(int(t[0]))
        return torch.zeros_like(x)
    return cond_fn


# ---- the two kernels ---------------------------------------------------------------------------------------------------------
def _rows():
    """A noisy row (t = 25) and the t = 0 row (c[5] = 0, c[8] = 0) of the linear T = 50 schedule."""
    _, tab = dm.cg_step_table(dm.make_schedule(50, "linear", ddpm=False), [25, 0])
    assert tab[:, G.NOISE].tolist() == [1, 0] and float(tab[0, G.VARIANCE]) > 0 and float(tab[1, G.VARIANCE]) == 0
    return tab.contiguous()


def _guarded(n):
    """A poisoned device buffer of n + 8 floats and its first n as the tensor a kernel may write."""
    buf = torch.full((n + 8,), POISON, device=DEV)
    return buf, buf[:n]


SHAPES = [(2, 1, 2, 2), (3, 3, 16, 16)]  # per = 4 in one partial workgroup; 2304 floats = 576 threads: 3 workgroups, the last partial


@pytest.mark.parametrize("objective", [0, 1, 2], ids=["pred_noise", "pred_x0", "pred_v"])
@pytest.mark.parametrize("shape", SHAPES, ids=["per4-one-partial-block", "three-blocks-last-partial"])
def test_op_mean_vs_fp64(shape, objective):
    lib = _lib.load()
    B, per, n = shape[0], int(np.prod(shape[1:])), int(np.prod(shape))
    for i, row in enumerate(_rows()):
        x, e = _randn(shape, 10 + i), _randn(shape, 20 + i, 1.5)  # 1.5: part of x_0 leaves [-1, 1] and is clamped
        xd, ed = x.to(DEV).contiguous(), e.to(DEV).contiguous()
        for want_xs in (True, False):
            mbuf, mean = _guarded(n)
            xbuf, xs = _guarded(n)
            _lib.check(lib.dm_op_cg_mean(_lib.ptr(xd), _lib.ptr(ed), _lib.fptr(row.contiguous()), objective, _lib.ptr(mean),
                                         _lib.ptr(xs) if want_xs else None, B, per, None))
            assert bool(torch.isnan(mbuf[n:]).all()) and bool(torch.isnan(xbuf[n:]).all()), "wrote past n"
            assert bool(torch.isfinite(mean).all())
            assert bool(torch.isfinite(xs).all()) if want_xs else bool(torch.isnan(xs).all())  # only what was asked for
            if want_xs:
                got_m, got_xs = mean.cpu().view(shape).double(), xs.cpu().view(shape).double()
            else:
                assert torch.equal(mean.cpu().view(shape).double(), got_m)
        ref_m, ref_xs = CO.cg_mean(x, e, row, objective, torch.float64)
        c = row.double()
        xa, ea = x.double().abs(), e.double().abs()
        raw = {0: c[0].abs() * xa + c[1].abs() * ea, 1: torch.zeros_like(xa), 2: c[6].abs() * xa + c[7].abs() * ea}[objective]
        lim_xs = 2 * ULP1 * raw
        lim_m = 2 * ULP1 * (c[2].abs() * raw + (c[2] * ref_xs).abs() + c[3].abs() * xa)
        err_m = (got_m - ref_m).abs()
        err_xs = (got_xs - ref_xs).abs()
        clamped = float((ref_xs.abs() == 1).double().mean())
        print(f"op cg_mean {shape} objective {objective} row {i}: mean err {float(err_m.max()):.3e} (limit up to "
              f"{float(lim_m.max()):.3e}), x_start err {float(err_xs.max()):.3e}, clamped share {clamped:.2f}")
        assert bool((err_m <= lim_m).all()) and bool((err_xs <= lim_xs).all())
        if objective != 1 and n >= 48:
            assert 0.0 < clamped < 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=["per4-one-partial-block", "three-blocks-last-partial"])
def test_op_finish_vs_fp64_injected_noise_in_place_and_poison(shape):
    lib = _lib.load()
    B, per, n = shape[0], int(np.prod(shape[1:])), int(np.prod(shape))
    for i, row in enumerate(_rows()):
        noisy = float(row[G.NOISE]) != 0
        m, g, z = _randn(shape, 30 + i), _randn(shape, 40 + i, 20.0), _randn(shape, 50 + i)
        zin = z if noisy else torch.full_like(z, POISON)  # the t = 0 row must not read its noise
        md, gd, zd = (t.to(DEV).contiguous() for t in (m, g, zin))
        obuf, out = _guarded(n)
        gbuf, guided = _guarded(n)
        _lib.check(lib.dm_op_cg_finish(_lib.ptr(md), _lib.ptr(gd), _lib.ptr(zd), _lib.fptr(row.contiguous()), 0, 1, 0,
                                       _lib.ptr(out), _lib.ptr(guided), B, per, None))
        assert bool(torch.isnan(obuf[n:]).all()) and bool(torch.isnan(gbuf[n:]).all()), "wrote past n"
        ref_o, ref_g = CO.cg_finish(m, g, z, row, torch.float64)
        c = row.double()
        lim_g = 2 * ULP1 * (m.double().abs() + (c[8] * g.double()).abs())
        lim_o = lim_g + 2 * ULP1 * ((c[4] * z.double()).abs() if noisy else 0.0)
        err_o = (out.cpu().view(shape).double() - ref_o).abs()
        err_g = (guided.cpu().view(shape).double() - ref_g).abs()
        print(f"op cg_finish {shape} row {i}: out err {float(err_o.max()):.3e} (limit up to {float(lim_o.max()):.3e}), "
              f"guided mean err {float(err_g.max()):.3e}, shift {float((c[8] * g.double()).abs().max()):.3e}")
        assert bool((err_o <= lim_o).all()) and bool((err_g <= lim_g).all())
        if not noisy:
            assert torch.equal(out, guided) and torch.equal(guided.cpu().view(shape), m)  # c[8] = 0: the gradient has no effect
        # without the optional output: it stays poisoned; in place (out = mean): the same bits
        gbuf2, guided2 = _guarded(n)
        inplace = md.clone()
        _lib.check(lib.dm_op_cg_finish(_lib.ptr(inplace), _lib.ptr(gd), _lib.ptr(zd), _lib.fptr(row.contiguous()), 0, 1, 0,
                                       _lib.ptr(inplace), None, B, per, None))
        assert bool(torch.isnan(gbuf2).all()) and torch.equal(inplace.view(-1), out)


def _box_muller64(words):
    """The kernel's transform of (N, 4) Philox words (csrc/philox.h) with its own fp32 uniforms, evaluated in fp64 / fp32."""
    f32 = np.float32
    inv = f32(2.0 ** -32)
    u1 = np.minimum((words[:, 0::2].astype(f32) + f32(1.0)) * inv, f32(1.0))
    ang = f32(6.2831853) * (words[:, 1::2].astype(f32) * inv)
    out = []
    for t in (np.float64, np.float32):
        rad = np.sqrt(t(-2.0) * np.log(u1.astype(t)))
        out.append(np.stack([rad * np.cos(ang.astype(t)), rad * np.sin(ang.astype(t))], axis=2).reshape(words.shape[0], 4))
    return out


def test_op_finish_philox_draw_vs_philox_ref():
    lib = _lib.load()
    shape = SHAPES[1]
    B, per, n = shape[0], int(np.prod(shape[1:])), int(np.prod(shape))
    row = _rows()[0]
    m, g = _randn(shape, 60), _randn(shape, 61, 20.0)
    md, gd = m.to(DEV).contiguous(), g.to(DEV).contiguous()
    seed, draw, off = 0x9E3779B97F4A7C15, 7, 4 * 100
    out = torch.full((n,), POISON, device=DEV)
    _lib.check(lib.dm_op_cg_finish(_lib.ptr(md), _lib.ptr(gd), None, _lib.fptr(row.contiguous()), seed, draw, off,
                                   _lib.ptr(out), None, B, per, None))
    z64, z32 = _box_muller64(philox_ref.stream(seed, draw, off // 4, n // 4))
    z = torch.from_numpy(z64.reshape(shape))
    ref_o, _ = CO.cg_finish(m, g, z, row, torch.float64)
    c = row.double()
    z_err = 4 * float(np.abs(z32 - z64).max())  # the bar of dm_randn itself (tests/test_hip_step_ops.py)
    lim = 2 * ULP1 * (m.double().abs() + (c[8] * g.double()).abs() + (c[4] * z).abs()) + float(c[4]) * z_err
    err = (out.cpu().view(shape).double() - ref_o).abs()
    print(f"op cg_finish Philox draw {draw}: err {float(err.max()):.3e} (limit up to {float(lim.max()):.3e})")
    assert bool((err <= lim).all())
    # the same draw as dm_randn's: injected, bit for bit
    zd = torch.empty((n,), device=DEV)
    _lib.check(lib.dm_randn(_lib.ptr(zd), n, seed, draw, off, None))
    inj = torch.empty((n,), device=DEV)
    _lib.check(lib.dm_op_cg_finish(_lib.ptr(md), _lib.ptr(gd), _lib.ptr(zd), _lib.fptr(row.contiguous()), 0, 1, 0,
                                   _lib.ptr(inj), None, B, per, None))
    assert torch.equal(inj, out)
    with pytest.raises(RuntimeError, match="draw 0"):
        _lib.check(lib.dm_op_cg_finish(_lib.ptr(md), _lib.ptr(gd), None, _lib.fptr(row.contiguous()), seed, 0, 0, _lib.ptr(inj),
                                       None, B, per, None))


# ---- single steps ------------------------------------------------------------------------------------------------------------
def test_p_sample_vs_reference(golden):
    c = golden["loops"]["a"]
    d = _obj(c)
    cond_fn, kw = _guide(c)
    x = golden["steps_single"]["x"]
    for s in golden["steps_single"]["steps"]:
        out, xs, mean, guided = d._guided_step(x, s["t"], None, cond_fn, kw, so.NoiseStream(s["noise_seed"]))
        errs = dict(y=rel_l2(out.cpu(), s["y"]), x_start=rel_l2(xs.cpu(), s["x_start"]), mean=rel_l2(mean.cpu(), s["mean"]),
                    guided_mean=rel_l2(guided.cpu(), s["guided_mean"]))
        print(f"p_sample t = {s['t']}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        assert max(errs.values()) <= STEP_TOL, (s["t"], errs)
        y2, xs2 = d.p_sample(x, s["t"], None, cond_fn, kw, noise=so.NoiseStream(s["noise_seed"]))
        assert torch.equal(y2, out) and torch.equal(xs2, xs)
        cm = d.condition_mean(cond_fn, mean, d.posterior_variance[s["t"]].reshape(1, 1, 1, 1).expand(x.shape[0], 1, 1, 1), x,
                              torch.full((x.shape[0],), s["t"]), kw)
        assert torch.equal(cm, guided)
        if s["t"] > 0:
            assert rel_l2(guided.cpu(), mean.cpu()) > 1e-3  # the guidance moved the mean
    # t == 0: posterior_variance[0] == 0, so two different gradients give the same bits
    a = d.p_sample(x, 0, None, *_guide(c, scale=50.0, labels=[0, 1]))
    b = d.p_sample(x, 0, None, *_guide(c, scale=-7.0, labels=[4, 2]))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- whole loops -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["a", "b", "c"])
def test_loop_vs_reference(golden, key):
    c = golden["loops"][key]
    d = _obj(c)
    calls = []
    cond_fn, kw = _guide(c, calls=calls)
    y = d.sample(batch_size=c["batch"], return_all_timesteps=True, cond_fn=cond_fn, guidance_kwargs=kw,
                 noise=so.NoiseStream(c["noise_seed"])).cpu()
    ref = c["frames"]
    assert y.shape == ref.shape and bool(torch.isfinite(y).all())
    limit = max(LOOP_TOL, 4 * c["ref_err"])
    per_frame = [rel_l2(y[:, f], ref[:, f]) for f in range(ref.shape[1])]
    whole = rel_l2(y, ref)
    print(f"guided loop {key}: all frames {whole:.3e}, worst frame {max(per_frame):.3e} (frame {int(np.argmax(per_frame))}), "
          f"final {per_frame[-1]:.3e}; limit {limit:.3e} (reference fp32-vs-fp64 {c['ref_err']:.3e})")
    assert whole <= limit and max(per_frame) <= limit
    T = c["timesteps"]
    assert [int(t[0]) for _, t in calls] == list(reversed(range(T)))  # once per step, t == 0 included
    assert all(t.dtype == torch.int64 and tuple(t.shape) == (c["batch"],) and t.is_cuda for _, t in calls)
    if key == "a":
        away = rel_l2(y[:, -1], c["unguided_final"])
        print(f"guided loop a vs the unguided run: {away:.4f} (recorded {c['guided_vs_unguided']:.4f})")
        assert away >= 0.5 * c["guided_vs_unguided"]  # an ignored gradient fails here
        final = d.sample(batch_size=c["batch"], cond_fn=cond_fn, guidance_kwargs=kw, noise=so.NoiseStream(c["noise_seed"]))
        assert torch.equal(final.cpu(), y[:, -1])


# ---- equivalences, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["a", "b"])
def test_zero_gradient_is_the_plain_ddpm_loop(golden, key):
    c = golden["loops"][key]
    d = _obj(c)
    plain = dm.DenoisingDiffusion(_net(c), image_size=c["image_size"], timesteps=c["timesteps"], beta_schedule=c["beta_schedule"],
                                  objective=c["objective"])
    B = c["batch"]
    for mk in (lambda: dict(seed=4242), lambda: dict(noise=so.NoiseStream(77))):  # a Philox seed; injected noise
        want = plain.sample(batch_size=B, return_all_timesteps=True, **mk())
        calls = []
        got = d.sample(batch_size=B, return_all_timesteps=True, cond_fn=_zero_fn(calls), guidance_kwargs={}, **mk())
        assert len(calls) == c["timesteps"] and torch.equal(got, want), key
        assert torch.equal(d.sample(batch_size=B, cond_fn=_zero_fn(), guidance_kwargs={}, **mk()), plain.sample(batch_size=B, **mk()))


def test_without_guidance_kwargs_it_is_the_parents_loop(golden):
    c = golden["loops"]["a"]
    d = _obj(c)
    calls = []
    want = d.sample(batch_size=2, seed=11)
    assert torch.equal(d.sample(batch_size=2, cond_fn=_zero_fn(calls), guidance_kwargs=None, seed=11), want)
    assert torch.equal(d.sample(batch_size=2, cond_fn=None, guidance_kwargs={}, seed=11), want)
    x = golden["steps_single"]["x"]
    a = d.p_sample(x, 7, None, _zero_fn(calls), None, noise=so.NoiseStream(5))
    b = dm.DenoisingDiffusion.p_sample(d, x, 7, noise=so.NoiseStream(5))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and calls == []


def test_graph_equals_eager_and_ddim_ignores_guidance(golden):
    c = golden["loops"]["b"]  # self-conditioning
    cond_fn, kw = _guide(c)
    run = lambda d: d.sample(batch_size=2, return_all_timesteps=True, cond_fn=cond_fn, guidance_kwargs=kw, seed=5)  # noqa: E731
    assert torch.equal(run(_obj(c, use_graph=True)), run(_obj(c, use_graph=False)))
    d = _obj(c, sampling_timesteps=6)
    calls = []
    assert d.is_ddim_sampling
    got = d.sample(batch_size=2, cond_fn=_zero_fn(calls), guidance_kwargs=kw, seed=9)
    assert torch.equal(got, d.sample(batch_size=2, seed=9)) and calls == []
    shape = (2, c["channels"], 16, 16)
    assert torch.equal(d.ddim_sample(shape, cond_fn=_zero_fn(calls), guidance_kwargs=kw, seed=9), got) and calls == []


# ---- graph reuse -------------------------------------------------------------------------------------------------------------
def test_two_graphs_captured_once_and_reused(golden):
    c = golden["loops"]["a"]
    net = _net(c)
    d = _obj(c)
    plain_before = d.sample(batch_size=2, seed=3)  # the slot holds the plain DDPM step
    n0 = net.graph_captures
    first = d.sample(batch_size=2, cond_fn=_guide(c)[0], guidance_kwargs=_guide(c)[1], seed=1)
    assert net.graph_captures == n0 + 2  # the two halves
    other = d.sample(batch_size=2, cond_fn=_guide(c)[0], guidance_kwargs=_guide(c, scale=5.0, labels=[4, 0])[1], seed=2)
    assert net.graph_captures == n0 + 2 and not torch.equal(first, other)
    assert torch.equal(d.sample(batch_size=2, cond_fn=_guide(c)[0], guidance_kwargs=_guide(c)[1], seed=1), first)
    assert net.graph_captures == n0 + 2
    assert torch.equal(d.sample(batch_size=2, seed=3), plain_before)  # the plain loop re-captures and is still right
    assert net.graph_captures == n0 + 3


# ---- host errors -------------------------------------------------------------------------------------------------------------
def test_cond_fn_errors_surface_and_the_handle_stays_usable(golden):
    c = golden["loops"]["a"]
    d = _obj(c)
    cond_fn, kw = _guide(c)
    good = d.sample(batch_size=2, cond_fn=cond_fn, guidance_kwargs=kw, seed=21)
    seen = []

    def raising(x, t, **k):
        seen.append(int(t[0]))
        if len(seen) == 4:  # step 3
            raise ValueError("the classifier gave up")
        return cond_fn(x, t, **k)

    for use_graph in (True, False):
        d.use_graph = use_graph
        seen.clear()
        with pytest.raises(ValueError, match="the classifier gave up"):
            d.sample(batch_size=2, cond_fn=raising, guidance_kwargs=kw, seed=21)
        assert seen == [49, 48, 47, 46]  # nothing ran after the step that raised
        assert torch.equal(d.sample(batch_size=2, cond_fn=cond_fn, guidance_kwargs=kw, seed=21), good)
    d.use_graph = True

    grad = d._cg_buffers[1]
    before = grad.clone()
    with pytest.raises(ValueError, match="must return a tensor of the mean's shape"):
        d.sample(batch_size=2, cond_fn=lambda x, t, **k: torch.ones_like(x)[:, :1], guidance_kwargs=kw, seed=21)
    assert torch.equal(grad, before)  # raised before anything was copied
    with pytest.raises(ValueError, match="must return a tensor"):
        d.sample(batch_size=2, cond_fn=lambda x, t, **k: None, guidance_kwargs=kw, seed=21)
    with pytest.raises(TypeError, match="unexpected keyword"):
        d.sample(batch_size=2, cond_fn=cond_fn, guidance_kwargs=kw, seed=21, text_emb=torch.zeros(2, 512))
    assert torch.equal(d.sample(batch_size=2, cond_fn=cond_fn, guidance_kwargs=kw, seed=21), good)


def test_conditional_unets_are_refused():
    calls = []
    for kw, msg in ((dict(text_condition=True), "no text-conditional U-Net"), (dict(cond_channels=3), "no image condition")):
        kw = dict(dim=32, dim_mults=(1, 2), channels=3, **kw)
        u = dm.Unet(device=DEV, **kw)
        u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(**kw)), salt=7))
        d = dm.ClassifierGuidedGaussianDiffusion(u, image_size=16, timesteps=50, beta_schedule="linear")
        with pytest.raises(RuntimeError, match=msg):
            d.sample(batch_size=2, cond_fn=_zero_fn(calls), guidance_kwargs={}, seed=1)
    assert calls == []
