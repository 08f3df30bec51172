"""LearnedGaussianDiffusion sampling on the GPU (fixture: tests/golden/make_golden_learned.py, from the reference).

* ``Unet(learned_variance=True).forward`` (final_conv with 2, 6 and 8 outputs through the one-pixel-per-thread kernel)
  against the reference's output: rel-L2 <= 1e-4, the project's bar for one forward;
* ``dm_op_lv_step`` against the fp64 restatement (tests/learned_oracle.py): error <= max(1e-6, 4 x the fp32 restatement's
  own error against fp64);
* single ``p_sample`` steps and the two whole loops against the reference: <= 1e-4;
* ``return_all_timesteps``, graph == eager bit for bit and graph caching, sharding with ``sample_offset``, and NaN-poisoned
  ``out`` / ``all_steps`` that must come back fully written.
Measured errors are printed (run with -s to see them)."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import learned as L
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import learned_oracle as O
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = STEP_TOL = LOOP_TOL = 1e-4
OP_TOL = 1e-6


@pytest.fixture(scope="module")
def golden():
    return load_golden("learned.pt")


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _net(channels, ukw, salt):
    cfg = UnetConfig(channels=channels, learned_variance=True, **ukw)
    u = dm.Unet(channels=channels, learned_variance=True, device=DEV, **ukw)
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt))
    return u


def _loop_obj(c, **kw):
    return dm.LearnedGaussianDiffusion(_net(c["channels"], c["unet_kw"], c["salt"]), image_size=c["image_size"],
                                       timesteps=c["timesteps"], beta_schedule=c["beta_schedule"], **kw)


# ---- the U-Net with 2 C outputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["c3_d32", "c1_d32", "c4_d64"])
def test_unet_forward_vs_reference(golden, key):
    c = golden["unet"][key]
    u = _net(c["channels"], c["unet_kw"], c["salt"])
    assert u.out_dim == 2 * c["channels"]
    y = u(c["x"].to(DEV), c["t"].to(DEV)).cpu()
    err = rel_l2(y, c["y"])
    halves = [rel_l2(h, w) for h, w in zip(y.chunk(2, dim=1), c["y"].chunk(2, dim=1))]
    print(f"Unet(learned_variance=True) {key}: {err:.3e} (noise half {halves[0]:.3e}, variance half {halves[1]:.3e})")
    assert y.shape == c["y"].shape and err <= FWD_TOL and max(halves) <= FWD_TOL


# ---- the step kernel -------------------------------------------------------------------------------------------------------
def _step_rows():
    """Rows with and without the noise flag: t = T - 1, a middle row, t = 1 and t = 0 of the linear T = 1000 schedule."""
    _, tab = dm.lv_step_table(dm.make_schedule(1000, "linear"))
    rows = tab[[0, 500, 998, 999]].contiguous()
    assert rows[:, L.NOISE].tolist() == [1, 1, 1, 0]
    return rows


def _run_step(x, mo, z, row, seed=0, draw=1, off=0):
    lib = _lib.load()
    B, per = x.shape[0], x[0].numel()
    xd, md = x.to(DEV).contiguous(), mo.to(DEV).contiguous()
    zd = z.to(DEV).contiguous() if z is not None else None
    outs = [torch.full_like(xd, float("nan")) for _ in range(4)]
    _lib.check(lib.dm_op_lv_step(_lib.ptr(xd), _lib.ptr(md), _lib.ptr(zd), _lib.fptr(row.contiguous()), seed, draw, off,
                                 *[_lib.ptr(o) for o in outs], B, per, None))
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("B,shape", [(2, (3, 4, 4)), (1, (1, 2, 2)), (3, (3, 20, 20))],
                         ids=["per48", "per4-smallest", "several-blocks"])
def test_op_step_vs_fp64(B, shape):
    rows = _step_rows()
    C_ = shape[0]
    for i in range(rows.shape[0]):
        x, z = _randn((B,) + shape, 10 + i), _randn((B,) + shape, 30 + i)
        mo = _randn((B, 2 * C_) + shape[1:], 20 + i)
        mo[:, C_:] *= 1.5  # the interpolation weight (v + 1) / 2 leaves [0, 1] on both sides
        frac = (mo[:, C_:] + 1) * 0.5
        if frac.numel() >= 48:
            assert float(frac.min()) < 0 and float(frac.max()) > 1
        noisy = float(rows[i, L.NOISE]) != 0
        zin = z if noisy else torch.full_like(z, float("nan"))  # the t = 0 row must not read its noise
        got = _run_step(x, mo, zin, rows[i])
        ref = O.step(x, mo, z, rows[i], torch.float64)
        r32 = O.step(x, mo, z, rows[i], torch.float32)
        for name, g, w, w32 in zip(("out", "mean", "logvar", "x_start"), got, ref, r32):
            err, e32 = rel_l2(g, w), rel_l2(w32, w)
            limit = max(OP_TOL, 4 * e32)
            print(f"op lv_step row {i} B={B} {shape} {name}: kernel {err:.3e} limit {limit:.3e} torch fp32 {e32:.3e}")
            assert bool(torch.isfinite(g).all()) and err <= limit, (i, name, err, limit)
        if not noisy:
            assert torch.equal(got[0], got[1])  # mean + exp(0.5 logvar) * 0


def test_op_step_philox_is_the_dm_randn_stream_and_refusals():
    lib = _lib.load()
    rows = _step_rows()
    B, shape = 3, (3, 16, 16)
    x, mo = _randn((B,) + shape, 50), _randn((B, 6, 16, 16), 51)
    seed, draw, off = 1234, 7, 4 * 100
    z = torch.empty((B,) + shape, device=DEV)
    _lib.check(lib.dm_randn(_lib.ptr(z), z.numel(), seed, draw, off, None))
    a = _run_step(x, mo, z.cpu(), rows[1])[0]
    b = _run_step(x, mo, None, rows[1], seed, draw, off)[0]
    assert torch.equal(a, b)
    c = _run_step(x, mo, None, rows[3], seed, draw, off)[0]  # t = 0: no draw
    d = _run_step(x, mo, None, rows[3], seed + 1, draw + 1, 0)[0]
    assert torch.equal(c, d) and not torch.equal(a, c)
    xd = x.to(DEV)
    out = torch.empty_like(xd)
    bad = torch.empty((1, 6), device=DEV)
    rc = lib.dm_op_lv_step(_lib.ptr(bad), _lib.ptr(bad), None, _lib.fptr(rows[0].contiguous()), 0, 1, 0, _lib.ptr(bad), None, None,
                           None, 1, 6, None)
    assert rc != 0 and b"multiple of 4" in lib.dm_last_error()
    rc = lib.dm_op_lv_step(_lib.ptr(xd), _lib.ptr(xd), None, _lib.fptr(rows[0].contiguous()), 0, 0, 0, _lib.ptr(out), None, None,
                           None, B, 768, None)
    assert rc != 0 and b"draw 0" in lib.dm_last_error()


# ---- p_sample, p_mean_variance and the loops against the reference -------------------------------------------------------
def test_p_sample_and_p_mean_variance_vs_reference(golden):
    s = golden["steps_single"]
    obj = dm.LearnedGaussianDiffusion(_net(s["channels"], s["unet_kw"], s["salt"]), image_size=16, timesteps=s["timesteps"],
                                      beta_schedule=s["beta_schedule"])
    for row in s["steps"]:
        t = row["t"]
        got, x_start = obj.p_sample(s["x"], t, noise=so.NoiseStream(row["noise_seed"]))
        err = (rel_l2(got.cpu(), row["y"]), rel_l2(x_start.cpu(), row["x_start"]))
        print(f"p_sample t = {t}: pred_img {err[0]:.3e} x_start {err[1]:.3e}")
        assert max(err) <= STEP_TOL
    # p_mean_variance with per-image timesteps: each image equals its own single-t call; exp(logvar) is the variance
    t = torch.tensor([500, 0])
    mo = obj.model(s["x"].to(DEV), t.to(DEV))
    mean, var, logvar, xs = obj.p_mean_variance(x=s["x"], t=t, clip_denoised=True, model_output=mo)
    for b in range(2):
        m1, v1, l1, x1 = obj.p_mean_variance(x=s["x"][b:b + 1], t=int(t[b]), clip_denoised=True, model_output=mo[b:b + 1])
        assert torch.equal(mean[b:b + 1], m1) and torch.equal(logvar[b:b + 1], l1) and torch.equal(xs[b:b + 1], x1)
    assert torch.equal(var, logvar.exp()) and float(xs.abs().max()) <= 1.0
    _, tab = dm.lv_step_table(obj._sched)
    want = O.step(s["x"][:1], mo[:1].cpu(), None, tab[999 - 500].clone().index_fill_(0, torch.tensor([L.NOISE]), 0.0))
    assert rel_l2(mean[:1].cpu(), want[1]) <= OP_TOL * 10 and rel_l2(logvar[:1].cpu(), want[2]) <= OP_TOL * 10
    unclipped = obj.p_mean_variance(x=s["x"], t=t, clip_denoised=False, model_output=mo)[3]
    assert float(unclipped.abs().max()) > 1.0 and torch.equal(unclipped.clamp(-1, 1), xs)


@pytest.mark.parametrize("key", ["lin50_c3", "cos24_c4_d64"])
def test_sample_vs_reference_graph_and_eager(golden, key):
    c = golden["loops"][key]
    obj = _loop_obj(c)
    outs = {}
    for use_graph in (True, False):
        obj.use_graph = use_graph
        got = obj.sample(batch_size=c["batch"], noise=so.NoiseStream(c["noise_seed"])).cpu()
        err = rel_l2(got, c["sample"])
        print(f"sample {key} {'graph' if use_graph else 'eager'} (T = {c['timesteps']}, frac {c['frac_range']}): {err:.3e}")
        assert got.shape == c["sample"].shape and err <= LOOP_TOL
        outs[use_graph] = got
    assert torch.equal(outs[True], outs[False])
    obj.use_graph = True
    frames = obj.sample(batch_size=c["batch"], return_all_timesteps=True, noise=so.NoiseStream(c["noise_seed"])).cpu()
    assert frames.shape == (c["batch"], c["timesteps"] + 1) + tuple(c["sample"].shape[1:])
    assert torch.equal(frames[:, -1], outs[True])
    x_T = so.NoiseStream(c["noise_seed"])(c["sample"].shape)
    assert torch.equal(frames[:, 0], (x_T + 1) * 0.5)


def test_graph_caching_sharding_and_seeds(golden):
    c = golden["loops"]["lin50_c3"]
    obj = _loop_obj(c)
    net = obj.model
    assert net.graph_captures == 0
    a = obj.sample(batch_size=4, seed=77)
    assert net.graph_captures == 1
    assert torch.equal(a, obj.sample(batch_size=4, seed=77)) and net.graph_captures == 1
    assert not torch.equal(a, obj.sample(batch_size=4, seed=78)) and net.graph_captures == 1  # the seed is device data
    halves = torch.cat((obj.sample(batch_size=2, seed=77), obj.sample(batch_size=2, seed=77, sample_offset=2)))
    assert torch.equal(a, halves) and net.graph_captures == 2  # one more capture for the new shape, none for the offset
    assert 0.0 <= float(a.min()) and float(a.max()) <= 1.0 and float(a.std()) > 0.01
    obj.use_graph = False
    assert torch.equal(a, obj.sample(batch_size=4, seed=77))
    short = obj.p_sample_loop((2, 3, 16, 16), seed=5, max_steps=3)
    assert short.shape == (2, 3, 16, 16) and bool(torch.isfinite(short).all())


def test_poisoned_outputs_come_back_fully_written(golden):
    c = golden["loops"]["lin50_c3"]
    obj = _loop_obj(c)
    lib = _lib.load()
    B, T = 2, c["timesteps"]
    shape = (B, 3, 16, 16)
    times, coefs = dm.lv_step_table(obj._sched)
    x_T = _randn(shape, 3).to(DEV)
    for use_graph in (1, 0):
        out = torch.full(shape, float("nan"), device=DEV)
        frames = torch.full((T + 1,) + shape, float("nan"), device=DEV)
        times_arr = (C.c_int64 * T)(*times)
        a = _lib.LvArgs()
        a.n_steps, a.times_host, a.table_host = T, C.cast(times_arr, C.POINTER(C.c_int64)), _lib.fptr(coefs)
        a.x_T, a.noise, a.seed, a.sample_offset = _lib.ptr(x_T), None, 9, 0
        a.out, a.all_steps, a.B, a.H, a.W = _lib.ptr(out), _lib.ptr(frames), B, 16, 16
        a.unnormalize, a.use_graph, a.stream = 1, use_graph, torch.cuda.current_stream(DEV).cuda_stream
        _lib.check(lib.dm_sample_lv(obj.model._handle, C.byref(a)))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(frames).all())
        assert torch.equal(frames[0], x_T) and torch.equal(out, (frames[-1] + 1) * 0.5)
    # the plain sampler and the plain loss keep refusing such a U-Net; the new loop refuses a plain one
    plain = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    plain.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(dim=32, dim_mults=(1, 2), channels=3)), salt=1))
    assert lib.dm_sample_lv(plain._handle, C.byref(a)) != 0 and b"2 * channels" in lib.dm_last_error()
    with pytest.raises(AssertionError):
        dm.DenoisingDiffusion(obj.model, image_size=16)
