"""RePaint inpainting on the GPU (fixture: tests/golden/make_golden_repaint.py, from the reference).

* ``dm_op_repaint_step`` on plain buffers, every mode, BIT-EXACT against the same expression in torch fp32 on the CPU
  (tests/repaint_oracle.py): the kernel only multiplies, adds, subtracts and clamps, with contraction off;
* its Philox path against injected tensors made by ``dm_randn`` at the documented draw ids (bitwise), and those ids against
  tests/philox_ref.py;
* ``sample()`` / ``p_sample`` against the reference's recorded outputs: relative L2 <= max(1e-4, 4 x the reference's own
  fp32-vs-fp64 error of the case); the known region bitwise;
* graph == eager == the row-by-row composition of ``p_sample``, bitwise; graph reuse; sharding; refusals.
Measured errors are printed (run with -s to see them)."""
import ctypes as C

import numpy as np
import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import repaint as R
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import philox_ref
import repaint_oracle as ro
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLE_TOL = 1e-4  # the project's sample tolerance (README, test_hip_configs.py)
OBJ = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}


def limit(ref_err):
    return max(SAMPLE_TOL, 4.0 * ref_err)


@pytest.fixture(scope="module")
def golden():
    return load_golden("repaint.pt")


@pytest.fixture(scope="module")
def net(golden):
    cfg = UnetConfig(channels=3, **golden["unet_kw"])
    u = dm.Unet(channels=3, device=DEV, **golden["unet_kw"])
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=golden["salt"]))
    return u


def _fp(t):
    assert t.dtype == torch.float32 and t.is_contiguous()
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


TABLE = dm.repaint_step_table(dm.make_schedule(20, "cosine"), True, 2, 3, 4)
# (row, mode, unnormalize): a plain row, a row whose successor opens a resample iteration (jump), an inner row, the last row
OP_CASES = [(0, R.BLEND, 0), (4, R.BLEND, 0), (0, R.STEP, 0), (49, R.STEP, 0), (0, R.STEP_NEXT, 0), (3, R.STEP_NEXT, 0),
            (4, R.STEP_NEXT, 0), (49, R.LAST, 0), (49, R.LAST, 1)]


def _op(mode, objective, x, eps, gt, mask, zj, zk, zs, rows, unnorm, B, Cc, HW, seed=0, row=0, off=0, want_xs=True):
    lib = _lib.load()
    dev = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    xd, ed, gd, md, zjd, zkd, zsd = (dev(t) for t in (x, eps, gt, mask, zj, zk, zs))
    out = torch.full((x.numel() + 8,), 7.0, device=DEV)
    xs = torch.empty_like(xd) if (want_xs and mode != R.BLEND) else None
    _lib.check(lib.dm_op_repaint_step(mode, objective, _lib.ptr(xd), _lib.ptr(ed), _lib.ptr(gd), _lib.ptr(md), mask.shape[1],
                                      _lib.ptr(zjd), _lib.ptr(zkd), _lib.ptr(zsd), _fp(rows), unnorm, seed, row, off,
                                      _lib.ptr(out), _lib.ptr(xs), B, Cc, HW, None))
    out = out.cpu()
    assert bool((out[x.numel():] == 7.0).all()), "wrote past the tensor"
    return out[:x.numel()].reshape(x.shape), (None if xs is None else xs.cpu())


def _want(mode, objective, x, eps, gt, mask, zj, zk, zs, row, nxt, unnorm):
    if mode == R.BLEND:
        return ro.blend(x, gt, mask, row, zk), None
    pred, x0 = ro.update(x, eps, row, zs, objective)
    if mode == R.STEP:
        return pred, x0
    if mode == R.LAST:
        return ro.last(pred, gt, mask, unnorm), x0
    return ro.step_next(x, eps, gt, mask, row, nxt, zs, zj, zk, objective)[0], x0


def _check_ops(B, Cc, HW, Cm):
    shape = (B, Cc, HW)
    g = torch.Generator().manual_seed(B * 1000 + Cc * 100 + HW + Cm)
    x, eps, zj, zk, zs = (torch.randn(shape, generator=g) for _ in range(5))
    gt = torch.rand(shape, generator=g)
    mask = torch.tensor([0.0, 0.25, 1.0, 0.7])[torch.randint(0, 4, (B, Cm, HW), generator=g)]  # not binary
    for r, mode, unnorm in OP_CASES:
        rows = TABLE.coefs[r:r + 2].contiguous() if mode == R.STEP_NEXT else TABLE.coefs[r:r + 1].contiguous()
        row, nxt = rows[0], rows[-1]
        assert (mode != R.STEP_NEXT) or bool(nxt[R.JUMP]) == (r == 3)
        no_step = float(row[5]) == 0.0
        zs_in = torch.full(shape, float("nan")) if no_step else zs  # t == 0 must not read its step noise
        for objective in (0, 1, 2):
            got, xs = _op(mode, objective, x, eps, gt, mask, zj, zk, zs_in, rows, unnorm, B, Cc, HW)
            want, want_xs = _want(mode, objective, x, eps, gt, mask, zj, zk, zs, row, nxt, unnorm)
            assert torch.equal(got, want), (r, mode, unnorm, objective, float((got - want).abs().max()))
            if xs is not None:
                assert torch.equal(xs, want_xs), (r, mode, objective)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 1025])  # the tail, more than one workgroup (1024 elements), the image boundary
def test_op_bit_exact(n, B):
    _check_ops(B, 1, n, 1)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Cm", [1, 3])
def test_op_mask_channels_bit_exact(Cm, B):
    _check_ops(B, 3, 5, Cm)  # Cm == 1: the kernel broadcasts the plane over the channels


def test_op_refusals():
    lib = _lib.load()
    x = torch.zeros((1, 3, 4), device=DEV)
    row = TABLE.coefs[:2].contiguous()
    args = lambda mode, cm, zk: (mode, 0, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), cm, None, zk, None, _fp(row), 0, 0,  # noqa: E731
                                 0, 0, _lib.ptr(x), None, 1, 3, 4, None)
    assert lib.dm_op_repaint_step(*args(R.BLEND, 2, None)) != 0 and b"1 or C channels" in lib.dm_last_error()
    assert lib.dm_op_repaint_step(*args(0, 1, None)) != 0 and b"explicit modes" in lib.dm_last_error()
    # injected noise without the draw the row reads (row 0: t = 19 > 0 takes step noise)
    assert lib.dm_op_repaint_step(*args(R.STEP, 1, _lib.ptr(x))) != 0 and b"every draw" in lib.dm_last_error()


def _box_muller64(c):
    f32 = np.float32
    u1 = np.minimum((c[:, 0::2].astype(f32) + f32(1.0)) * f32(2.0 ** -32), f32(1.0)).astype(np.float64)
    ang = (f32(6.2831853) * (c[:, 1::2].astype(f32) * f32(2.0 ** -32))).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=2).reshape(-1)


def test_philox_path_is_dm_randn_at_the_documented_ids():
    lib = _lib.load()
    B, Cc, HW = 3, 3, 1025 // 5 * 4  # per % 4 == 0 so that an element offset is a counter offset
    shape = (B, Cc, HW)
    n = B * Cc * HW
    seed, off = 0x9E3779B97F4A7C15, 4 * 100
    x, eps, gt = _randn(shape, 1), _randn(shape, 2), torch.rand(shape, generator=torch.Generator().manual_seed(3))
    mask = torch.full((B, 1, HW), 0.25)

    def randn(draw):
        z = torch.empty(shape, device=DEV)
        _lib.check(lib.dm_randn(_lib.ptr(z), n, seed, draw, off, None))
        return z.cpu()

    # the ids: jump 3r + 1, known 3r + 2, step 3r + 3 -- and dm_randn at such an id is the reference Philox stream
    assert R.draw_ids(3) == (10, 11, 12)
    z64 = _box_muller64(philox_ref.stream(seed, R.draw_ids(4)[0], off // 4, n // 4))
    assert float(np.abs(randn(13).numpy().reshape(-1) - z64).max()) < 1e-5
    for r, mode in ((0, R.BLEND), (4, R.BLEND), (0, R.STEP), (0, R.STEP_NEXT), (3, R.STEP_NEXT), (49, R.LAST)):
        rows = TABLE.coefs[r:r + 2].contiguous() if mode == R.STEP_NEXT else TABLE.coefs[r:r + 1].contiguous()
        b = r if mode == R.BLEND else r + 1  # the row whose jump and blend the launch does
        zj, zk, zs = randn(R.draw_ids(b)[0]), randn(R.draw_ids(b)[1]), randn(R.draw_ids(r)[2])
        inj, _ = _op(mode, 2, x, eps, gt, mask, zj, zk, zs, rows, 0, B, Cc, HW)
        phi, _ = _op(mode, 2, x, eps, gt, mask, None, None, None, rows, 0, B, Cc, HW, seed=seed, row=r, off=off)
        assert torch.equal(inj, phi), (r, mode)
        if mode != R.LAST:
            other, _ = _op(mode, 2, x, eps, gt, mask, None, None, None, rows, 0, B, Cc, HW, seed=seed, row=r + 1, off=off)
            assert not torch.equal(other, phi)  # another row draws other noise


# ---- the loop ---------------------------------------------------------------------------------------------------------
def _diffusion(net, ckw, **kw):
    return dm.RePaintGaussianDiffusion(net, image_size=16, timesteps=20, **ckw, **kw)


def _sample_kw(c):
    return dict(c["sample_kw"])


@pytest.mark.parametrize("key", ["a", "b", "c", "d"])
def test_sample_vs_golden(golden, net, key):
    c = golden["loops"][key]
    d = _diffusion(net, c["diffusion_kw"])
    got = d.sample(gt=golden["gt"], mask=c["mask"], noise=so.NoiseStream(golden["noise_seed"]), **_sample_kw(c)).cpu()
    err = rel_l2(got, c["sample"])
    print(f"repaint sample {key}: rel-L2 {err:.3e} (limit {limit(c['ref_err']):.1e}, reference fp32-vs-fp64 {c['ref_err']:.2e})")
    assert got.shape == c["sample"].shape and err <= limit(c["ref_err"]), (key, err)
    known = c["mask"].expand(got.shape) == 1
    assert torch.equal(got[known], c["sample"][known])  # pred drops out where mask == 1
    if key == "d":  # auto_normalize=False: the known region is 2 gt - 1
        assert torch.equal(got[known], (golden["gt"] * 2 - 1)[known])


def test_all_timesteps_vs_golden(golden, net):
    c = golden["loops"]["e"]
    d = _diffusion(net, c["diffusion_kw"])
    got = d.sample(gt=golden["gt"], mask=c["mask"], noise=so.NoiseStream(golden["noise_seed"]), **_sample_kw(c)).cpu()
    assert tuple(got.shape) == tuple(c["shape"])
    err = rel_l2(got[:, -c["n_last"]:], c["last_frames"])
    print(f"repaint frames: rel-L2 {err:.3e}")
    assert err <= limit(c["ref_err"])
    kw = {k: v for k, v in c["sample_kw"].items() if k != "return_all_timesteps"}
    one = d.sample(gt=golden["gt"], mask=c["mask"], noise=so.NoiseStream(golden["noise_seed"]), **kw).cpu()
    assert torch.equal(got[:, -1], one) and torch.equal(got[:, 0], (so.NoiseStream(golden["noise_seed"])(one.shape) + 1) * 0.5)


def test_p_sample_vs_golden(golden, net):
    p = golden["p_sample"]
    for objective, case in p["steps"].items():
        d = _diffusion(net, case["diffusion_kw"])
        for st in case["steps"]:
            y, xs = d.p_sample(p["x"], st["t"], gt=golden["gt"], mask=p["mask"], noise=so.NoiseStream(st["noise_seed"]))
            e1, e2 = rel_l2(y.cpu(), st["y"]), rel_l2(xs.cpu(), st["x_start"])
            print(f"repaint p_sample {objective} t={st['t']}: {e1:.3e} x_start {e2:.3e} (limit {limit(st['ref_err']):.1e})")
            assert e1 <= limit(st["ref_err"]) and e2 <= limit(st["ref_err"]), (objective, st["t"], e1, e2)


def test_no_mask_is_the_parent(golden, net):
    c = golden["loops"]["g"]
    d = _diffusion(net, c["diffusion_kw"])
    got = d.sample(batch_size=2, noise=so.NoiseStream(golden["noise_seed"]))
    err = rel_l2(got.cpu(), c["sample"])
    print(f"repaint no mask: rel-L2 {err:.3e}")
    assert err <= limit(c["ref_err"])
    parent = dm.DenoisingDiffusion(net, image_size=16, timesteps=20, objective="pred_noise", beta_schedule="cosine")
    assert torch.equal(got, parent.p_sample_loop((2, 3, 16, 16), noise=so.NoiseStream(golden["noise_seed"])))
    # sampling_timesteps < timesteps: still the DDPM loop, never DDIM
    ddim = _diffusion(net, c["diffusion_kw"], sampling_timesteps=5)
    assert ddim.is_ddim_sampling and torch.equal(ddim.sample(batch_size=2, noise=so.NoiseStream(golden["noise_seed"])), got)


@pytest.mark.parametrize("key", ["a", "b"])
def test_graph_equals_eager_equals_p_sample_composition(golden, net, key):
    c = golden["loops"][key]
    d = _diffusion(net, c["diffusion_kw"])
    gt, mask, kw = golden["gt"], c["mask"], _sample_kw(c)
    graph = d.sample(gt=gt, mask=mask, noise=so.NoiseStream(7), **kw)
    d.use_graph = False
    eager = d.sample(gt=gt, mask=mask, noise=so.NoiseStream(7), **kw)
    d.use_graph = True
    assert torch.equal(graph, eager)
    seeded = [d.sample(gt=gt, mask=mask, seed=99, **kw) for _ in range(2)]
    d.use_graph = False
    assert torch.equal(seeded[0], seeded[1]) and torch.equal(seeded[0], d.sample(gt=gt, mask=mask, seed=99, **kw))
    assert not torch.equal(seeded[0], graph)
    # row by row: the jump between the rows, then p_sample with the mask
    tab = dm.repaint_step_table(d._sched, **kw)
    noise = so.NoiseStream(7)
    x = noise(graph.shape).to(DEV)
    for r, t in enumerate(tab.times):
        row = tab.coefs[r]
        if float(row[R.JUMP]) != 0:
            x = float(row[R.JUMP_X]) * x + float(row[R.JUMP_Z]) * noise(x.shape).to(DEV)
        x, _ = d.p_sample(x, t, gt=gt, mask=mask, noise=noise)
    assert torch.equal(d.unnormalize(x), graph)


def test_graph_is_reused_across_calls(golden, net):
    lib = _lib.load()
    c = golden["loops"]["a"]
    d = _diffusion(net, c["diffusion_kw"])
    gt, mask = golden["gt"], c["mask"]
    first = d.sample(gt=gt, mask=mask, seed=1, **_sample_kw(c))
    n = lib.dm_unet_graph_captures(net._handle)
    other = d.sample(gt=1 - gt, mask=mask * 0.5, seed=2, **_sample_kw(c))
    assert lib.dm_unet_graph_captures(net._handle) == n and not torch.equal(first, other)
    kw = dict(_sample_kw(c), resample_iter=3)  # another row count
    more = d.sample(gt=gt, mask=mask, seed=1, **kw)
    assert lib.dm_unet_graph_captures(net._handle) == n
    d.use_graph = False
    assert torch.equal(more, d.sample(gt=gt, mask=mask, seed=1, **kw))
    assert torch.equal(first, d.sample(gt=gt, mask=mask, seed=1, **_sample_kw(c)))


def test_shards_reproduce_the_batch(golden, net):
    c = golden["loops"]["b"]
    d = _diffusion(net, c["diffusion_kw"])
    g = torch.Generator().manual_seed(11)
    gt = torch.rand((4, 3, 16, 16), generator=g)
    mask = (torch.rand((4, 3, 16, 16), generator=g) > 0.5).float()
    kw = _sample_kw(c)
    whole = d.sample(gt=gt, mask=mask, seed=5, **kw)
    halves = [d.sample(gt=gt[o:o + 2], mask=mask[o:o + 2], seed=5, sample_offset=o, **kw) for o in (0, 2)]
    assert torch.equal(whole, torch.cat(halves, dim=0))


def test_self_conditioning_with_a_mask_is_refused(golden):
    u = dm.Unet(channels=3, device=DEV, self_condition=True, **golden["unet_kw"])
    d = dm.RePaintGaussianDiffusion(u, image_size=16, timesteps=20)
    with pytest.raises(NotImplementedError):
        d.sample(gt=golden["gt"], mask=golden["loops"]["a"]["mask"])
