"""The three input-gradient kernels on their own (dm_op_conv7_dgrad, dm_op_sinusoid_ft_tgrad, dm_op_ct_sched_reduce) against
an fp64 torch restatement (tests/ct_learned_oracle.py).

Two measures per output, as in tests/test_hip_attn_cores.py: whole-tensor rel-L2, and the worst row -- the error norm of one
row (conv: one (image, channel, y) line of W values; the per-image kernels: one image) over the RMS row norm of the
reference.  The limit of both is max(5e-5, 4 x the error of the same restatement run in fp32 against fp64), computed at run
time and never from the kernel's result.  Every case prints the kernel's value next to the restatement's (run with -s).

conv7_dgrad also: outputs pre-filled with NaN between canaries, two runs bit-identical, an image's result independent of the
batch it is in, and a dY that is non-zero in one corner pixel only (every tap that reaches it is a border tap)."""
import math

import pytest
import torch

from diffusion_models_amd import _lib

import ct_learned_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR, FACTOR = 5e-5, 4.0
CANARY, CANARY_VALUE = 64, -7.25


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _measures(got, want64, rows):
    """(rel-L2, worst row) of `got` against the fp64 `want64`, both viewed as (rows, -1)."""
    e = (got.double().cpu() - want64).reshape(rows, -1)
    w = want64.reshape(rows, -1)
    rms = float(w.norm(dim=1).pow(2).mean().sqrt().clamp_min(1e-300))
    return float(e.norm() / w.norm().clamp_min(1e-300)), float(e.norm(dim=1).max()) / rms


def _check(tag, got, want64, want32, rows):
    k, r = _measures(got, want64, rows), _measures(want32, want64, rows)
    lim = [max(FLOOR, FACTOR * v) for v in r]
    print(f"{tag}: rel-L2 {k[0]:.2e} | {r[0]:.2e} (limit {lim[0]:.1e})  worst row {k[1]:.2e} | {r[1]:.2e} (limit {lim[1]:.1e})")
    assert bool(torch.isfinite(got).all()), tag
    assert k[0] <= lim[0] and k[1] <= lim[1], (tag, k, lim)


def _guarded(shape):
    """A NaN-filled device tensor of `shape` between two canary spans: (whole buffer, the view)."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * CANARY,), CANARY_VALUE, device=DEV)
    buf[CANARY:CANARY + n] = float("nan")
    return buf, buf[CANARY:CANARY + n].view(shape)


def _canaries_intact(buf):
    return bool((buf[:CANARY] == CANARY_VALUE).all()) and bool((buf[-CANARY:] == CANARY_VALUE).all())


def _conv7(dy, w):
    B, Cout, H, W = dy.shape
    C = w.shape[1]
    buf, dx = _guarded((B, C, H, W))
    _lib.check(_lib.load().dm_op_conv7_dgrad(_lib.ptr(dy), _lib.ptr(w), _lib.ptr(dx), B, H, W, Cout, C, _stream()))
    torch.cuda.synchronize()
    assert _canaries_intact(buf)
    return dx.clone()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(8, 8), (16, 16), (24, 40)])
@pytest.mark.parametrize("init_dim", [32, 64])
@pytest.mark.parametrize("C", [3, 4, 8])
def test_conv7_dgrad_vs_fp64(C, init_dim, hw, B):
    H, W = hw
    g = torch.Generator().manual_seed(1000 * C + init_dim + H + B)
    dy = torch.randn((B, init_dim, H, W), generator=g)
    w = torch.randn((init_dim, C, 7, 7), generator=g) / math.sqrt(49 * C)
    want64, want32 = lo.conv7_dgrad(dy.double(), w.double()), lo.conv7_dgrad(dy, w)
    dyd, wd = dy.to(DEV), w.to(DEV)
    got = _conv7(dyd, wd)
    _check(f"conv7_dgrad C={C} init_dim={init_dim} {H}x{W} B={B}", got, want64, want32, B * C * H)
    assert torch.equal(got, _conv7(dyd, wd))  # fixed accumulation order: bit-identical runs
    if B > 1:  # an image's result does not depend on the batch it is in
        for b in range(B):
            assert torch.equal(got[b:b + 1], _conv7(dyd[b:b + 1].contiguous(), wd)), b


@pytest.mark.parametrize("corner", [(0, 0), (0, -1), (-1, 0), (-1, -1)])
@pytest.mark.parametrize("C,init_dim,hw", [(3, 32, (8, 8)), (8, 64, (24, 40))])
def test_conv7_dgrad_of_one_corner_pixel(C, init_dim, hw, corner):
    H, W = hw
    g = torch.Generator().manual_seed(77)
    dy = torch.zeros((2, init_dim, H, W))
    dy[:, :, corner[0], corner[1]] = torch.randn((2, init_dim), generator=g)
    w = torch.randn((init_dim, C, 7, 7), generator=g) / math.sqrt(49 * C)
    want64 = lo.conv7_dgrad(dy.double(), w.double())
    got = _conv7(dy.to(DEV), w.to(DEV))
    _check(f"conv7_dgrad corner {corner} C={C} init_dim={init_dim} {H}x{W}", got, want64, lo.conv7_dgrad(dy, w), 2 * C * H)
    # the gradient lives in the 4 x 4 pixels the corner's window reaches inside the image, and is exactly zero elsewhere
    ys = slice(0, 4) if corner[0] == 0 else slice(H - 4, H)
    xs = slice(0, 4) if corner[1] == 0 else slice(W - 4, W)
    rest = got.clone()
    rest[:, :, ys, xs] = 0
    assert not bool(rest.any()) and bool(got[:, :, ys, xs].abs().min() > 0)


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("half", [1, 8, 17])
def test_sinusoid_ft_tgrad_vs_fp64(half, B):
    g = torch.Generator().manual_seed(10 * half + B)
    t = torch.linspace(-10.0, 10.0, B) if B > 1 else torch.tensor([-10.0])  # the log-SNR range of the linear schedule
    freqs = torch.randn(half, generator=g)
    ang = t.double()[:, None] * freqs.double()[None, :] * 2 * math.pi
    e0 = torch.cat((t.double()[:, None], ang.sin(), ang.cos()), dim=1).float()  # the taped rows are fp32
    de0 = torch.randn((B, 2 * half + 1), generator=g)
    want64 = lo.sinusoid_ft_tgrad(de0.double(), e0.double(), freqs.double())
    want32 = lo.sinusoid_ft_tgrad(de0, e0, freqs)
    buf, dt = _guarded((B,))
    dev = [v.to(DEV) for v in (de0, e0, freqs)]  # (kept alive over the call)
    _lib.check(_lib.load().dm_op_sinusoid_ft_tgrad(*[_lib.ptr(v) for v in dev], _lib.ptr(dt), B, half, _stream()))
    assert _canaries_intact(buf)
    _check(f"sinusoid_ft_tgrad half={half} B={B}", dt, want64, want32, B)


@pytest.mark.parametrize("with_dt", [True, False])
@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("shape", [(3, 8, 8), (4, 16, 16)])
def test_ct_sched_reduce_vs_fp64(shape, normalize, with_dt):
    B = 3
    g = torch.Generator().manual_seed(sum(shape) + normalize)
    full = (B,) + shape
    dx, eps, Fo, target = (torch.randn(full, generator=g) for _ in range(4))
    images = torch.rand(full, generator=g)
    dt = torch.randn(B, generator=g) if with_dt else None
    args64 = [v.double() if v is not None else None for v in (dx, images, eps, Fo, target, dt)]
    want64 = lo.sched_reduce(*args64, normalize)
    want32 = lo.sched_reduce(dx, images, eps, Fo, target, dt, normalize)
    buf, out = _guarded((B, 4))
    dev = [v.to(DEV) if v is not None else None for v in (dx, images, eps, Fo, target, dt)]
    _lib.check(_lib.load().dm_op_ct_sched_reduce(*[_lib.ptr(v) for v in dev], normalize, _lib.ptr(out), B, math.prod(shape),
                                                 _stream()))
    assert _canaries_intact(buf)
    for j, name in enumerate(("sum dx x0", "sum dx eps", "dt", "mean (F - target)^2")):
        if name == "dt":  # passed through (or zero): exact
            assert torch.equal(out[:, j].cpu(), dt if with_dt else torch.zeros(B))
            continue
        _check(f"ct_sched_reduce per={math.prod(shape)} normalize={normalize} {name}", out[:, j], want64[:, j], want32[:, j], B)
