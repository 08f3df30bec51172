"""GPU parity of CrossAttention as the text-conditional U-Net runs it, one operator at a time, forward and backward
(dm_op_cross_attention: run_cross; dm_op_cross_attention_bwd: t_cross then t_cross_bwd), against
``oracle.unet_oracle.cross_attention`` evaluated in fp64 on the CPU on the same fp32 inputs, gradients by autograd in fp64.

The models of the suite reach this layer with 16 (once 1024) queries and 1 or 3 context tokens only.  The cases here take
every form of every step at shapes with ``nq != nk``: the LDS-resident and the tiled attention core with ragged 64-key
tiles, the three backward forms (pair-per-thread with its score cache, thread-per-query, tiled) on either side of their
thresholds, the three forms of the context projections (MFMA rows GEMM, groups of 8 rows, fewer than 8 rows), the 1x1
convolutions around the core on and off the MFMA grids, ``dim_head`` 64, the one-token algebra against the general path, and
the per-image text mask.

Limits.  Unit-scale ``randn`` inputs: rel-L2 <= 2e-5 forward (``TOL`` of tests/test_hip_ops.py) and <= 5e-5 per gradient
tensor (``TOL`` of tests/test_hip_train_ops.py).  Every other input family: the same oracle is run in fp32 on the CPU and
measured against the fp64 result inside the test, and the kernel may be ``max(that bound, 4 x the fp32 error)`` off (the rule
of tests/test_hip_vae_ops.py; the factor 4 allows for another summation order between two correct fp32 implementations).
Every case prints ``case, tensor, kernel error, fp32 error, limit`` before it asserts (run with -s; DESIGN.md holds the
table)."""
import pytest
import torch

from diffusion_models_amd import _lib
from oracle import unet_oracle as uo

from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL_FWD = 2e-5
TOL_BWD = 5e-5
DEV = "cuda:0"
PARAMS = ("to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight", "to_out.0.bias", "to_out.1.g")


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def make_inputs(case, family):
    """x, ctx, dy and the six parameters of the layer (fp32, CPU).
    randn:  unit-scale x and ctx, weights scaled by fan_in ** -0.5.
    peaked: to_q and to_k times 6: the scores grow 36-fold, softmax rows are nearly one-hot, __expf runs far from 0.
    padded: the last two thirds of the tokens of every caption are one identical row (equal scores across the 64-key tile
            boundaries); the first third differs, so that dx and the to_q / to_k gradients are not identically zero."""
    B, C, H, W, m, E, dh = case
    inner = 4 * dh
    x = seeded((B, C, H, W), 1)
    ctx = seeded((B, m, E), 2)
    dy = seeded((B, C, H, W), 3)
    sd = {
        "c.to_q.weight": seeded((inner, C), 4, C ** -0.5),
        "c.to_k.weight": seeded((inner, E), 5, E ** -0.5),
        "c.to_v.weight": seeded((inner, E), 6, E ** -0.5),
        "c.to_out.0.weight": seeded((C, inner), 7, inner ** -0.5),
        "c.to_out.0.bias": seeded((C,), 8, 0.1),
        "c.to_out.1.g": 1 + 0.3 * seeded((1, C), 9),
    }
    if family == "peaked":
        sd["c.to_q.weight"] = sd["c.to_q.weight"] * 6
        sd["c.to_k.weight"] = sd["c.to_k.weight"] * 6
    elif family == "padded":
        assert m >= 3
        ctx[:, m // 3:, :] = ctx[:, m // 3:m // 3 + 1, :].clone()
    else:
        assert family == "randn"
    return x, ctx, dy, sd


def oracle(x, ctx, dy, sd, dtype):
    """The layer on (B, C, H, W) maps in `dtype` on the CPU: (out, dx, {parameter: gradient})."""
    B, C, H, W = x.shape
    xg = x.to(dtype).requires_grad_(True)
    p = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    flat = xg.reshape(B, C, H * W).permute(0, 2, 1)
    out = uo.cross_attention(p, "c", flat, ctx.to(dtype)).permute(0, 2, 1).reshape(B, C, H, W)
    names = list(p)
    grads = torch.autograd.grad(out, [xg] + [p[k] for k in names], dy.to(dtype))
    return out.detach(), grads[0], {k[2:]: g for k, g in zip(names, grads[1:])}


def hip_forward(case, x, ctx, sd, mask):
    B, C, H, W, m, E, dh = case
    a = [dev(t) for t in (x, ctx, sd["c.to_q.weight"], sd["c.to_k.weight"], sd["c.to_v.weight"], sd["c.to_out.0.weight"],
                          sd["c.to_out.0.bias"], sd["c.to_out.1.g"])]
    mk = None if mask is None else torch.tensor(mask, dtype=torch.int32, device=DEV)
    out = torch.full((B, C, H, W), float("nan"), device=DEV)
    _lib.check(_lib.load().dm_op_cross_attention(*[_lib.ptr(t) for t in a], _lib.ptr(mk), _lib.ptr(out), B, C, H, W, m, E, dh,
                                                 None))
    return out.cpu()


def hip_backward(case, x, ctx, dy, sd, mask):
    """(y_out, dx, {parameter: gradient}) of dm_op_cross_attention_bwd; every output starts as NaN."""
    B, C, H, W, m, E, dh = case
    a = [dev(t) for t in (x, ctx, sd["c.to_q.weight"], sd["c.to_k.weight"], sd["c.to_v.weight"], sd["c.to_out.0.weight"],
                          sd["c.to_out.0.bias"], sd["c.to_out.1.g"])]
    mk = None if mask is None else torch.tensor(mask, dtype=torch.int32, device=DEV)
    y = torch.full((B, C, H, W), float("nan"), device=DEV)
    dx = torch.full((B, C, H, W), float("nan"), device=DEV)
    outs = [torch.full(sd["c." + n].shape, float("nan"), device=DEV) for n in PARAMS]
    _lib.check(_lib.load().dm_op_cross_attention_bwd(*[_lib.ptr(t) for t in a], _lib.ptr(mk), _lib.ptr(dev(dy)), _lib.ptr(y),
                                                     _lib.ptr(dx), *[_lib.ptr(t) for t in outs], B, C, H, W, m, E, dh, None))
    return y.cpu(), dx.cpu(), {n: t.cpu() for n, t in zip(PARAMS, outs)}


def limit_for(family, bound, err32):
    return bound if family == "randn" else max(bound, 4.0 * err32)


def check(label, family, tensor, got, ref64, ref32, bound):
    """Print, then assert, one tensor against the fp64 reference; the fp32 error is the oracle's own, never the kernel's."""
    err = rel_l2(got, ref64)
    err32 = rel_l2(ref32, ref64)
    lim = limit_for(family, bound, err32)
    print(f"cross_attention {label} {tensor}: kernel {err:.3g}  fp32 {err32:.3g}  limit {lim:.3g}")
    assert torch.isfinite(got).all(), (label, tensor)
    assert err <= lim, (label, tensor, err, lim)


# (B, C, H, W, m, E, dim_head)
ONE_TOKEN = (2, 64, 4, 4, 1, 512, 32)        # one-token algebra; fused-norm to_out in the general path
PAIRS_77 = (2, 256, 4, 4, 77, 512, 32)       # pairs kernel, two key tiles (64 + 13)
UNCACHED_300 = (1, 64, 4, 4, 300, 512, 32)   # uncached LDS kernel, more keys than the 256 threads of its key phase
TILED_BWD = (1, 32, 23, 25, 130, 64, 32)     # odd map, ragged last query tile, three key tiles: tiled backward
TILED_FWD = (1, 32, 8, 8, 330, 64, 32)       # over 320 keys: tiled forward
CASES = [
    ONE_TOKEN,
    (3, 128, 4, 4, 3, 512, 32),      # today's model shape; 9 context rows (ragged group of 8)
    (1, 64, 4, 4, 5, 512, 32),       # fewer than 8 context rows: linear_rows_kernel
    PAIRS_77,
    (2, 64, 8, 8, 64, 512, 32),      # nq * m = 4096: the last shape with the score cache
    (2, 64, 8, 8, 65, 512, 32),      # nq * m = 4160: the first without
    UNCACHED_300,
    (2, 64, 1, 1, 77, 512, 32),      # one query
    (1, 32, 24, 24, 77, 64, 32),     # nq = 576: tiled backward (9 query tiles x 2 key tiles); LDS-resident forward, query split
    TILED_BWD,
    TILED_FWD,
    (2, 36, 5, 7, 65, 48, 32),       # channels and E off every MFMA grid: direct / VALU kernels
    (1, 64, 8, 8, 130, 512, 64),     # dim_head 64, three key tiles
    (2, 128, 4, 4, 3, 512, 64),      # dim_head 64 at the model's shape
]
# the hard families on one shape per backward form (pairs, uncached, tiled) and per forward form (resident, tiled)
HARD_SHAPES = [PAIRS_77, UNCACHED_300, TILED_BWD, TILED_FWD]
# the text mask on a pairs shape and on a tiled shape, B = 3
MASK_SHAPES = [(3, 256, 4, 4, 77, 512, 32), (3, 32, 24, 24, 77, 64, 32)]
MASKS = [(1, 0, 1), (1, 1, 1), (0, 0, 0)]
RUNS = ([("randn", c, None) for c in CASES] + [(f, c, None) for f in ("peaked", "padded") for c in HARD_SHAPES] +
        [("randn", c, k) for c in MASK_SHAPES for k in MASKS])


def run_id(run):
    family, case, mask = run
    return "-".join([family] + [str(v) for v in case] + (["mask" + "".join(str(v) for v in mask)] if mask else []))


@pytest.mark.parametrize("run", RUNS, ids=[run_id(r) for r in RUNS])
def test_cross_attention(run):
    family, case, mask = run
    B, C, H, W, m, E, dh = case
    label = run_id(run)
    x, ctx, dy, sd = make_inputs(case, family)
    out = hip_forward(case, x, ctx, sd, mask)
    y_out, dx, grads = hip_backward(case, x, ctx, dy, sd, mask)

    keep = [b for b in range(B) if mask is None or mask[b]]
    drop = [b for b in range(B) if b not in keep]
    if drop:
        # the layer is skipped for these images: its result is its input, the gradient passes through untouched
        assert torch.equal(out[drop], x[drop]), (label, "out of the masked rows is not x")
        assert torch.equal(y_out[drop], x[drop]), (label, "y_out of the masked rows is not x")
        assert torch.equal(dx[drop], dy[drop]), (label, "dx of the masked rows is not dy")
    if not keep:
        for n in PARAMS:
            assert torch.count_nonzero(grads[n]) == 0, (label, n, "gradient of an all-dropped batch is not exactly 0")
        print(f"cross_attention {label}: out == x, dx == dy, every parameter gradient exactly 0")
        return

    # the reference sees the kept rows only
    r64 = oracle(x[keep], ctx[keep], dy[keep], sd, torch.float64)
    r32 = oracle(x[keep], ctx[keep], dy[keep], sd, torch.float32)
    check(label, family, "out", out[keep], r64[0], r32[0], TOL_FWD)
    check(label, family, "y_out", y_out[keep], r64[0], r32[0], TOL_FWD)
    zero = ("to_q.weight", "to_k.weight") if m == 1 else ()
    if m == 1:
        # softmax over one key is 1 whatever q and k are: nothing reaches x, to_q or to_k.  rel_l2 would divide by zero
        assert torch.count_nonzero(r64[1]) == 0 and all(torch.count_nonzero(r64[2][n]) == 0 for n in zero)
        assert torch.count_nonzero(dx[keep]) == 0, (label, "dx is not exactly 0 with one context token")
        for n in zero:
            assert torch.count_nonzero(grads[n]) == 0, (label, n, "not exactly 0 with one context token")
        # the one-token algebra (forward op; the general path under DM_NO_CROSS1) against the general path of t_cross
        err = rel_l2(out, y_out)
        print(f"cross_attention {label} out vs y_out: {err:.3g}  limit {TOL_FWD:.3g}")
        assert err <= TOL_FWD, (label, "one-token forward vs general path", err)
    else:
        check(label, family, "dx", dx[keep], r64[1], r32[1], TOL_BWD)
    for n in PARAMS:
        if n not in zero:
            check(label, family, n, grads[n], r64[2][n], r32[2][n], TOL_BWD)
