"""tests/conv_restate.py in fp64 against ``F.conv2d`` and its autograd in fp64: every restatement (forward families, the
input gradient through each of them, both weight-gradient forms, the bias sums) at one shape per class, to 1e-12.  Only then
is its fp32 error the floor of an algorithm and not of a mistake."""
import pytest
import torch
import torch.nn.functional as F

import conv_restate as cr
from conftest import rel_l2

TOL = 1e-12


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# (B, C, c0, H, W, Cout, k, up2, fwd, dgrad per source, wgrad)
CASES = [
    (2, 20, 12, 7, 9, 12, 3, False, "direct", ("direct", "direct"), "direct"),   # odd map, two sources, chunks of 4
    (2, 32, 32, 5, 6, 8, 1, False, "direct", ("direct",), "direct"),             # 1x1, chunks of 16
    (1, 6, 6, 8, 8, 8, 7, False, "direct", ("direct",), "direct"),               # 7x7
    (3, 16, 8, 6, 10, 8, 3, False, "wino", ("wino", "wino"), "wino"),            # F(2x2): ragged tiles in neither direction
    (2, 8, 8, 6, 2, 8, 3, False, "wino", ("wino",), "direct"),                   # image narrower than a tile row
    (2, 8, 8, 4, 4, 8, 3, False, "wino4", ("wino4",), "wino"),                   # F(4x4), one tile per image
    (1, 8, 8, 16, 32, 8, 3, False, "wino4", ("wino4",), "wino"),                 # 4 x 8 tiles
    (1, 8, 8, 10, 6, 8, 3, False, "wino4", ("wino",), "wino"),                   # F(4x4) on a size that is no multiple of 4
    (2, 8, 8, 4, 4, 8, 3, True, "upwino", ("wino4",), "wino"),                   # nearest x2: source-grid algorithm
    (2, 8, 8, 3, 5, 8, 3, True, "upfold", ("direct",), "direct"),                # nearest x2: four parity convolutions
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[8]}-{c[10]}-{c[3]}x{c[4]}-k{c[6]}{'-up' if c[7] else ''}" for c in CASES])
def test_restatement_in_fp64_matches_conv2d(case):
    B, C, c0, H, W, Cout, k, up2, fwd, dgrad, wgrad = case
    x = seeded((B, C, H, W), 1).requires_grad_(True)
    w = (seeded((Cout, C, k, k), 2) / (k * C ** 0.5)).requires_grad_(True)
    b = seeded((Cout,), 3).requires_grad_(True)
    ref = F.conv2d(cr.upsample2(x) if up2 else x, w, b, padding=k // 2)
    dy = seeded(tuple(ref.shape), 4)
    want = torch.autograd.grad(ref, (x, w, b), dy)
    spec = dict(k=k, up2=up2, c0=c0, fwd=fwd, dgrad=dgrad, wgrad=wgrad)
    got_y = cr.conv(x, w, b, spec)
    got = torch.autograd.grad(got_y, (x, w, b), dy)
    errs = dict(y=rel_l2(got_y, ref), dx=rel_l2(got[0], want[0]), dw=rel_l2(got[1], want[1]), db=rel_l2(got[2], want[2]))
    print(case, errs)
    assert max(errs.values()) < TOL, errs


def test_space_to_depth_is_the_downsample_rearrangement():
    from oracle import unet_oracle as uo
    x = seeded((2, 4, 6, 10), 1)
    sd = {"d.1.weight": seeded((8, 16, 1, 1), 2), "d.1.bias": seeded((8,), 3)}
    got = cr.direct(cr.space_to_depth(x), sd["d.1.weight"]) + sd["d.1.bias"][None, :, None, None]
    assert rel_l2(got, uo.downsample(sd, "d", x)) < TOL
