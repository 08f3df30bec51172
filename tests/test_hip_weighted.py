"""WeightedObjectiveGaussianDiffusion sampling on the GPU (fixture: tests/golden/make_golden_weighted.py, from the
reference).

* ``dm_op_wo_step`` against the fp64 restatement (tests/weighted_oracle.py) on (B, C, HxW) = (1, 1, 2x2) (one thread, the
  smallest), (3, 3, 6x10) (HW not a power of two, several channels) and (2, 2, 16x16), each at a t > 0 row and the t = 0
  row with given noise: error <= max(1e-6, 4 x the fp32 restatement's own error against fp64); NaN-filled outputs must come
  back fully written; the Philox form equals ``dm_randn`` at the same seed / draw / offset bit for bit;
* ``Unet(out_dim = 2 C + 2).forward`` (final_conv with 8, 6 and 4 outputs), ``p_mean_variance``, single ``p_sample`` steps
  and the two whole loops against the reference: rel-L2 <= 1e-4;
* graph == eager bit for bit, a second call of one shape reuses the captured graph, two batch shards with
  ``sample_offset`` equal the unsharded run, NaN-poisoned ``out`` / ``all_steps`` come back fully written.
Measured errors are printed (run with -s to see them)."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import weighted as Wm
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import weighted_oracle as O
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = STEP_TOL = LOOP_TOL = 1e-4
OP_TOL = 1e-6
SHAPES = [(1, 1, 2, 2), (3, 3, 6, 10), (2, 2, 16, 16)]
SHAPE_IDS = ["one-thread", "hw60-3ch", "16x16-2ch"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("weighted.pt")


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _net(channels, ukw, salt):
    cfg = UnetConfig(channels=channels, out_dim=2 * channels + 2, **ukw)
    u = dm.Unet(channels=channels, out_dim=2 * channels + 2, device=DEV, **ukw)
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt))
    return u


def _obj(c, **kw):
    return dm.WeightedObjectiveGaussianDiffusion(_net(c["channels"], c["unet_kw"], c["salt"]), image_size=c.get("image_size", 16),
                                                 timesteps=c["timesteps"], beta_schedule=c["beta_schedule"], **kw)


# ---- the U-Net with 2 C + 2 outputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["c3", "c2", "c1"])
def test_unet_forward_vs_reference(golden, key):
    c = golden["unet"][key]
    ch = c["channels"]
    u = _net(ch, c["unet_kw"], c["salt"])
    assert u.out_dim == 2 * ch + 2
    y = u(c["x"].to(DEV), c["t"].to(DEV)).cpu()
    err = rel_l2(y, c["y"])
    groups = [rel_l2(h, w) for h, w in zip(O.split(y), O.split(c["y"]))]
    print(f"Unet(out_dim={2 * ch + 2}) {key}: {err:.3e} (noise {groups[0]:.3e}, x_start {groups[1]:.3e}, weights {groups[2]:.3e})")
    assert y.shape == c["y"].shape and err <= FWD_TOL and max(groups) <= FWD_TOL


# ---- the step kernel -------------------------------------------------------------------------------------------------------
def _step_rows():
    """A row that adds noise (t = 500) and the t = 0 row of the linear T = 1000 schedule."""
    _, tab = dm.wo_step_table(dm.make_schedule(1000, "linear"))
    rows = tab[[499, 999]].contiguous()
    assert rows[:, Wm.NOISE].tolist() == [1, 0]
    return rows


def _run_step(x, mo, z, row, clip=1, seed=0, draw=1, off=0):
    lib = _lib.load()
    B, Cc, HW = x.shape[0], x.shape[1], x[0, 0].numel()
    xd, md = x.to(DEV).contiguous(), mo.to(DEV).contiguous()
    zd = z.to(DEV).contiguous() if z is not None else None
    outs = [torch.full_like(xd, float("nan")) for _ in range(3)]
    _lib.check(lib.dm_op_wo_step(_lib.ptr(xd), _lib.ptr(md), _lib.ptr(zd), _lib.fptr(row.contiguous()), clip, seed, draw, off,
                                 *[_lib.ptr(o) for o in outs], B, Cc, HW, None))
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_op_step_vs_fp64(shape):
    rows = _step_rows()
    B, Cc, H, W = shape
    for i in range(rows.shape[0]):
        x, z = _randn(shape, 10 + i), _randn(shape, 30 + i)
        mo = _randn((B, 2 * Cc + 2, H, W), 20 + i)
        mo[:, 2 * Cc:] *= 2.0  # softmax weights from near 0 to near 1
        noisy = float(rows[i, Wm.NOISE]) != 0
        zin = z if noisy else torch.full_like(z, float("nan"))  # the t = 0 row must not read its noise
        for clip in (1, 0):
            got = _run_step(x, mo, zin, rows[i], clip)
            ref = O.step(x, mo, z, rows[i], bool(clip), torch.float64)
            r32 = O.step(x, mo, z, rows[i], bool(clip), torch.float32)
            for name, g, w, w32 in zip(("out", "mean", "x_start"), got, ref, r32):
                err, e32 = rel_l2(g, w), rel_l2(w32, w)
                limit = max(OP_TOL, 4 * e32)
                print(f"op wo_step row {i} clip {clip} {shape} {name}: kernel {err:.3e} limit {limit:.3e} torch fp32 {e32:.3e}")
                assert bool(torch.isfinite(g).all()) and err <= limit, (i, name, err, limit)
            if clip:
                assert float(got[2].abs().max()) <= 1.0
                if got[2].numel() >= 180:  # the clamp is active somewhere, and inactive somewhere
                    assert bool((got[2].abs() == 1.0).any()) and bool((got[2].abs() < 1.0).any())
            if not noisy:
                assert torch.equal(got[0], got[1])  # mean + exp(0.5 logvar) * 0


def test_op_step_philox_is_the_dm_randn_stream_and_refusals():
    lib = _lib.load()
    rows = _step_rows()
    shape = (3, 3, 6, 10)  # the counter of element b C HW + c HW + p: the flat index of the (B, C, H, W) tensor
    x, mo = _randn(shape, 50), _randn((3, 8, 6, 10), 51)
    seed, draw, off = 1234, 7, 4 * 100
    z = torch.empty(shape, device=DEV)
    _lib.check(lib.dm_randn(_lib.ptr(z), z.numel(), seed, draw, off, None))
    a = _run_step(x, mo, z.cpu(), rows[0])
    b = _run_step(x, mo, None, rows[0], 1, seed, draw, off)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    c = _run_step(x, mo, None, rows[1], 1, seed, draw, off)[0]  # t = 0: no draw
    d = _run_step(x, mo, None, rows[1], 1, seed + 1, draw + 1, 0)[0]
    assert torch.equal(c, d) and not torch.equal(a[0], c)
    xd = x.to(DEV)
    out = torch.empty_like(xd)
    bad = torch.empty((1, 4, 6), device=DEV)
    rc = lib.dm_op_wo_step(_lib.ptr(bad), _lib.ptr(bad), None, _lib.fptr(rows[0].contiguous()), 1, 0, 1, 0, _lib.ptr(bad), None, None,
                           1, 1, 6, None)
    assert rc != 0 and b"multiple of 4" in lib.dm_last_error()
    rc = lib.dm_op_wo_step(_lib.ptr(xd), _lib.ptr(xd), None, _lib.fptr(rows[0].contiguous()), 1, 0, 0, 0, _lib.ptr(out), None, None,
                           3, 3, 60, None)
    assert rc != 0 and b"draw 0" in lib.dm_last_error()


# ---- p_mean_variance, p_sample and the loops against the reference --------------------------------------------------------
def test_p_mean_variance_and_p_sample_vs_reference(golden):
    p, s = golden["pmv"], golden["steps_single"]
    obj = _obj(p)
    for row in p["rows"]:
        t = torch.full((2,), row["t"], dtype=torch.long)
        mean, var, logvar = obj.p_mean_variance(x=p["x"], t=t, clip_denoised=True)
        raw = obj.p_mean_variance(x=p["x"], t=t, clip_denoised=False)[0]
        err = (rel_l2(mean.cpu(), row["mean"]), rel_l2(raw.cpu(), row["mean_unclipped"]))
        print(f"p_mean_variance t = {row['t']}: mean {err[0]:.3e} unclipped {err[1]:.3e}")
        assert max(err) <= STEP_TOL and tuple(var.shape) == (2, 1, 1, 1) and tuple(logvar.shape) == (2, 1, 1, 1)
        assert torch.equal(var.cpu(), row["variance"]) and torch.equal(logvar.cpu(), row["log_variance"])
    # per-image timesteps in one call; a passed model_output is ignored, as in the reference
    m = p["mixed"]
    junk = torch.full((2, 8, 16, 16), float("nan"), device=DEV)
    mean, var, logvar = obj.p_mean_variance(x=p["x"], t=m["t"], clip_denoised=True, model_output=junk)
    assert rel_l2(mean.cpu(), m["mean"]) <= STEP_TOL and torch.equal(logvar.cpu(), m["log_variance"])
    assert torch.equal(var.cpu(), m["variance"])
    for row in s["steps"]:
        t = row["t"]
        got, x_start = obj.p_sample(s["x"], t, noise=so.NoiseStream(row["noise_seed"]))
        err = (rel_l2(got.cpu(), row["y"]), rel_l2(x_start.cpu(), row["x_start"]))
        print(f"p_sample t = {t}: pred_img {err[0]:.3e} x_start {err[1]:.3e}")
        assert max(err) <= STEP_TOL and float(x_start.abs().max()) <= 1.0


@pytest.mark.parametrize("key", ["lin50_c3", "cos24_c1"])
def test_sample_vs_reference_graph_and_eager(golden, key):
    c = golden["loops"][key]
    obj = _obj(c)
    outs = {}
    for use_graph in (True, False):
        obj.use_graph = use_graph
        got = obj.sample(batch_size=c["batch"], noise=so.NoiseStream(c["noise_seed"])).cpu()
        err = rel_l2(got, c["sample"])
        print(f"sample {key} {'graph' if use_graph else 'eager'} (T = {c['timesteps']}): {err:.3e}")
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
    obj = _obj(c)
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


def test_poisoned_outputs_come_back_fully_written_and_refusals(golden):
    c = golden["loops"]["lin50_c3"]
    obj = _obj(c)
    lib = _lib.load()
    B, T = 2, c["timesteps"]
    shape = (B, 3, 16, 16)
    times, coefs = dm.wo_step_table(obj._sched)
    x_T = _randn(shape, 3).to(DEV)
    for use_graph in (1, 0):
        out = torch.full(shape, float("nan"), device=DEV)
        frames = torch.full((T + 1,) + shape, float("nan"), device=DEV)
        times_arr = (C.c_int64 * T)(*times)
        a = _lib.WoArgs()
        a.n_steps, a.times_host, a.table_host = T, C.cast(times_arr, C.POINTER(C.c_int64)), _lib.fptr(coefs)
        a.x_T, a.noise, a.seed, a.sample_offset = _lib.ptr(x_T), None, 9, 0
        a.out, a.all_steps, a.B, a.H, a.W = _lib.ptr(out), _lib.ptr(frames), B, 16, 16
        a.unnormalize, a.use_graph, a.stream = 1, use_graph, torch.cuda.current_stream(DEV).cuda_stream
        _lib.check(lib.dm_sample_wo(obj.model._handle, C.byref(a)))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(frames).all())
        assert torch.equal(frames[0], x_T) and torch.equal(out, (frames[-1] + 1) * 0.5)
    # the new loop refuses a plain U-Net and a learned-variance one; the plain class refuses this U-Net
    plain = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    plain.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(dim=32, dim_mults=(1, 2), channels=3)), salt=1))
    assert lib.dm_sample_wo(plain._handle, C.byref(a)) != 0 and b"2 * channels + 2" in lib.dm_last_error()
    with pytest.raises(AssertionError):
        dm.DenoisingDiffusion(obj.model, image_size=16)
