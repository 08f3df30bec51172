"""GPU parity of every convolution kernel family, one operator at a time through the C ABI (dm_op_conv2d, dm_op_downsample,
dm_op_block and their backward operators), against ``F.conv2d`` / ``oracle.unet_oracle`` evaluated in fp64 on the CPU on
the same fp32 inputs, gradients by autograd in fp64.

Asserted dispatch.  Every case names, in the table and never from the library's plan functions, the kernel family its
convolution must reach (conv_mfma, wino_mfma, wino4_mfma, upwino_mfma, pw_mfma, init7_mfma), for the backward operators also
the family of each input-gradient convolution and the mode of the weight gradient (direct, 1x1, space-to-depth, Winograd
domain), and where the case is about it, a K split > 1 and the tile form (q: 32-cout workgroups of F(2x2); r: 16-pixel row
tiles per wave of the 1x1 GEMM).  The call is bracketed with the library's profile rows (detail mode: one row per layer
shape) and the named row must be there.  The dispatch thresholds are read once per process, so the table holds one
expectation per set of switches; tests/test_hip_forced_dispatch.py runs this file again in two children:
  forced   DM_WINO4_MIN_WGS = DM_WINO4_MIN_K = DM_UPWINO_MIN_WGS = DM_UPWINO_MIN_K = 1: F(4x4) and the upsample kernel
  alt      DM_WINO_Q_TARGET_WGS = DM_PW_RT_TARGET_WGS = 1, DM_WGRAD_NO_WINO = 1: the 64-cout form of F(2x2) (q2), the
           64-pixel wave tiles of the 1x1 GEMM (r4) -- small grids take q1 / r1 by default -- and the direct 3x3 weight gradient
The naive weight-gradient kernel (first and last convolution of the U-Net) has no operator entry point: its case is skipped
by name; tests/test_hip_train.py reaches it through the model.

Limits.  Per tensor two metrics: whole-tensor rel-L2 and max|got - ref| / rms(ref).  The floor of each is the fp32
restatement (tests/conv_restate.py) of the algorithm of the family that the table names, measured against the fp64 reference
inside the test and never taken from the kernel's output; the kernel may be 4 x the floor off (another summation order
between two correct fp32 implementations).  The ``randn`` family must additionally stay under the limits of
tests/test_hip_ops.py / tests/test_hip_train_ops.py (2e-5 forward, 5e-5 per gradient tensor).  Every output is finite:
run_op poisons the operator workspace and the gradient slots with NaNs.
Every case prints ``case tensor kernel: kernel error, floor, limit`` for both metrics before it asserts (run with -s;
DESIGN.md holds the table); the module prints the number of cases per family and mode at the end."""
import collections
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_checks
import conv_restate as cr
from conv_checks import dev, family_input, nans, profiled_call, seeded
from diffusion_models_amd import _lib
from oracle import unet_oracle as uo

pytestmark = pytest.mark.gpu
TOL_FWD = 2e-5
TOL_BWD = 5e-5


def config():
    e = os.environ
    if e.get("DM_WINO4_MIN_WGS") == "1" and e.get("DM_UPWINO_MIN_WGS") == "1":
        return "forced"
    if e.get("DM_WINO_Q_TARGET_WGS") == "1" and e.get("DM_PW_RT_TARGET_WGS") == "1" and e.get("DM_WGRAD_NO_WINO") == "1":
        return "alt"
    return "default"


CFG = config()
WGRAD_MODE = {"direct": 0, "1x1": 1, "s2d": 2, "wino": 3}
COUNTS = collections.Counter()


@pytest.fixture(scope="module", autouse=True)
def profiled():
    _lib.profile_enable(True, detail=True)
    _lib.profile_read()
    yield
    _lib.profile_read()
    _lib.profile_enable(False)
    print(f"\nconv families [{CFG}]: cases per family / weight-gradient mode")
    for name, n in sorted(COUNTS.items()):
        print(f"  {name}: {n}")


def expected(exp):
    """The expectation of a case under the switches of this process: 'family [q1|q2|r1|r4] [k>1]' -> (family, tokens).
    The alt child keeps the family of the default process and takes the large-tile forms."""
    s = exp.get(CFG, exp["default"])
    if CFG == "alt" and "alt" not in exp:
        s = s.replace(" q1", " q2").replace(" r1", " r4")
    parts = s.split()
    return parts[0], parts[1:]


def runs_here(exp, wgrad=None):
    """Children run the cases they change: another family (forced), another tile form or weight-gradient mode (alt)."""
    if CFG == "default":
        return True
    if CFG == "forced":
        return "forced" in exp
    return any(t in exp["default"] for t in (" q1", " r1")) or wgrad == "wino"


def assert_row(label, rows, family, shape, tokens=()):
    return conv_checks.assert_row(COUNTS, label, rows, family, shape, tokens)


def assert_wgrad_row(label, rows, mode, shape, split):
    hits = [r for r in rows if r.startswith(f"wgrad m{WGRAD_MODE[mode]} ") and shape in r]
    assert hits, (label, f"no wgrad_mfma row of mode {mode} with '{shape}'", rows)
    if split:
        k = [int(m.group(1)) for r in hits for m in [re.search(r" k(\d+)", r)] if m]
        assert k and max(k) > 1, (label, "no pixel split", hits)
    COUNTS[f"wgrad_mfma {mode}"] += 1
    return hits[0]


class Checker(conv_checks.Checker):
    def __init__(self, label, family, bound):
        super().__init__(f"conv_families[{CFG}]", COUNTS, label, family, bound)


RESTATE = {"conv": "direct", "pw": "direct", "init7": "direct", "wino": "wino", "wino4": "wino4", "upwino": "upwino"}


def restate_family(family, up2=False):
    return "upfold" if (up2 and family == "conv") else RESTATE[family]


def direct_ck(family):
    return 1 if family == "init7" else None  # the first conv runs its K index channel-major: c * 49 + tap


# ---- dm_op_conv2d ---------------------------------------------------------------------------------------------------------
# (B, C0, C1, H, W, Cout, k, up2, bias, residual, {switches: expectation}, input families beyond randn)
HARD = ("offset", "wide", "flat")
W2_W4 = dict(default="wino q1", forced="wino4")
CONV_CASES = [
    # F(4x4) (forced child; F(2x2) in the default process): 4x4, 8x8 and multiples of 16
    (5, 64, 0, 4, 4, 64, 3, False, True, False, W2_W4, HARD),           # 16 images per workgroup, ragged last group
    (3, 64, 0, 8, 8, 64, 3, False, True, False, W2_W4, ()),             # 4 images per workgroup, ragged
    (2, 16, 0, 16, 16, 64, 3, False, True, False, W2_W4, HARD),         # one image per workgroup
    (1, 16, 0, 16, 32, 64, 3, False, False, False, W2_W4, ()),          # two workgroups across
    (2, 8, 0, 8, 8, 64, 3, False, True, False, W2_W4, ()),              # a single chunk
    (3, 24, 8, 8, 8, 64, 3, False, True, True, W2_W4, ()),              # two sources 24 + 8, residual
    (2, 32, 0, 4, 4, 128, 3, False, True, False, W2_W4, ()),            # two cout tiles
    (2, 1024, 0, 4, 4, 64, 3, False, True, False, dict(default="wino q1 k>1", forced="wino4 k>1"), ()),  # K split + finalize
    (37, 64, 0, 4, 4, 128, 3, False, False, False, W2_W4, ()),          # F(2x2): 8 images per workgroup, ragged batch
    # F(2x2) under every set of switches: even sizes outside the F(4x4) classes
    (2, 8, 0, 6, 2, 64, 3, False, True, False, dict(default="wino q1"), ()),       # image narrower than a tile row
    (3, 72, 8, 12, 20, 64, 3, False, True, True, dict(default="wino q1"), HARD),   # masked tiles, two sources, residual
    (1, 16, 0, 18, 34, 64, 3, False, False, False, dict(default="wino q1"), ()),   # ragged blocks in both directions
    # direct implicit GEMM: odd sizes, channels off the Winograd grids, 7x7 away from the first-conv kernel, tiny maps
    (2, 64, 64, 7, 9, 64, 3, False, True, True, dict(default="conv"), HARD),       # two sources, residual
    (3, 256, 0, 5, 5, 256, 3, False, True, False, dict(default="conv k>1"), ()),   # K split
    (300, 192, 0, 1, 1, 44, 3, False, True, False, dict(default="conv"), ()),      # 1x1 maps, ragged batch
    (70, 40, 24, 2, 2, 100, 3, False, True, True, dict(default="conv"), ()),       # 2x2 maps, two sources
    (2, 20, 12, 7, 9, 36, 3, False, True, False, dict(default="conv"), ()),        # channels that are multiples of 4 only
    (1, 6, 0, 8, 8, 32, 7, False, True, False, dict(default="conv"), ()),          # 7x7 with 6 channels, 32 couts
    (1, 1024, 0, 2, 2, 64, 3, False, True, False, dict(default="conv k>1"), ()),   # window too large for F(2x2)
    (1, 8, 0, 2, 2, 64, 1, False, True, False, dict(default="conv"), ()),          # 1x1 with 8 channels: not a 1x1 GEMM chunk
    # 1x1 GEMM (channels in chunks of 16, couts in tiles of 64)
    (3, 64, 64, 10, 6, 64, 1, False, True, True, dict(default="pw r1"), HARD),     # two sources, ragged last rows, residual
    (1, 16, 0, 2, 2, 64, 1, False, True, False, dict(default="pw r1"), ()),        # one chunk, four pixels
    (2, 64, 0, 8, 8, 192, 1, False, True, False, dict(default="pw r1"), ()),       # 192 couts
    (5, 32, 0, 8, 8, 384, 1, False, False, False, dict(default="pw r1"), ()),      # 384 couts, no bias
    (2, 512, 256, 4, 4, 512, 1, False, True, True, dict(default="pw r1 k>1"), ()),  # K split, two sources
    # nearest x2 + 3x3: the upsample kernel (forced child), the folded direct kernel by default
    (5, 64, 0, 4, 4, 128, 3, True, True, False, dict(default="conv", forced="upwino"), ()),      # four 4x4 images per workgroup, ragged
    (2, 64, 0, 8, 8, 64, 3, True, True, False, dict(default="conv", forced="upwino"), HARD),     # one 8x8 block per image
    (1, 16, 0, 8, 24, 64, 3, True, False, False, dict(default="conv", forced="upwino"), ()),     # non-square source
    (2, 512, 0, 4, 4, 64, 3, True, True, False, dict(default="conv", forced="upwino k>1"), ()),  # K split
    (3, 32, 0, 8, 8, 128, 3, True, True, True, dict(default="conv", forced="upwino"), ()),       # residual, two cout tiles
    # on either side of the production thresholds (default process): F(4x4) from 200 workgroups and 12 chunks per workgroup
    # on, the upsample kernel from 128 workgroups and 8 chunks on
    (50, 96, 0, 16, 16, 256, 3, False, True, False, dict(default="wino4"), ()),                   # 200 workgroups, 12 chunks
    (50, 88, 0, 16, 16, 256, 3, False, True, False, dict(default="wino q1"), ()),                 # 11 chunks
    (49, 96, 0, 16, 16, 256, 3, False, True, False, dict(default="wino q1"), ()),                 # 196 workgroups
    (32, 64, 0, 8, 8, 256, 3, True, True, False, dict(default="upwino"), ()),                     # 128 workgroups, 8 chunks
    (32, 56, 0, 8, 8, 256, 3, True, True, False, dict(default="conv"), ()),                       # 7 chunks
    (31, 64, 0, 8, 8, 256, 3, True, True, False, dict(default="conv"), ()),                       # 124 workgroups
    # first conv
    (3, 4, 0, 20, 28, 64, 7, False, True, False, dict(default="init7"), HARD),     # ragged 16x16 blocks
    (1, 6, 0, 8, 8, 64, 7, False, False, False, dict(default="init7"), ()),        # image smaller than a block
    (2, 3, 0, 8, 8, 64, 7, False, True, False, dict(default="init7"), ()),
    (2, 8, 0, 20, 28, 64, 7, False, True, False, dict(default="init7"), ()),
]
CONV_RUNS = [(c, f) for c in CONV_CASES if runs_here(c[10]) for f in ("randn",) + c[11]]


def conv_shape(family, C0, C1, Cout, H, W, up2):
    """The layer as the row of `family` prints it (the folded direct kernel names its source grid)."""
    if family == "upwino":
        return f" {C0}->{Cout} @{2 * H}x{2 * W} "
    if family == "init7":
        return f" {C0}->64 @{H}x{W} "
    return f" {C0}+{C1}->{Cout} @{H}x{W} " + ("upfold " if up2 else "")


def run_id(run):
    case, family = run
    return family + "-" + "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in case if not isinstance(v, (dict, tuple)))


@pytest.mark.parametrize("run", CONV_RUNS, ids=[run_id(r) for r in CONV_RUNS])
def test_conv2d(run):
    (B, C0, C1, H, W, Cout, k, up2, bias, residual, exp, _), fam = run
    label = "conv2d " + run_id(run)
    kern, tokens = expected(exp)
    pad = k // 2
    x = family_input(torch.cat((seeded((B, C0, H, W), 1), seeded((B, C1, H, W), 2)), 1), fam, 7)
    w = seeded((Cout, C0 + C1, k, k), 3, (C0 + C1) ** -0.5 / k)
    b = seeded((Cout,), 4) if bias else None
    s = 2 if up2 else 1
    res = seeded((B, Cout, s * H, s * W), 5) if residual else None

    def ref(dt):
        y = F.conv2d(cr.upsample2(x.to(dt)) if up2 else x.to(dt), w.to(dt), None if b is None else b.to(dt), padding=pad)
        return y if res is None else y + res.to(dt)

    floor = cr.forward(x, w, restate_family(kern, up2), k, up2, direct_ck(kern))
    if b is not None:
        floor = floor + b[None, :, None, None]
    if res is not None:
        floor = floor + res
    out = nans(B, Cout, s * H, s * W)
    a = [dev(t) for t in (x[:, :C0], x[:, C0:] if C1 else None, w, b, res)]
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_conv2d(
        _lib.ptr(a[0]), C0, _lib.ptr(a[1]), C1, _lib.ptr(a[2]), _lib.ptr(a[3]), _lib.ptr(a[4]), _lib.ptr(out), B, H, W, Cout, k,
        pad, int(up2), None)))
    row = assert_row(label, rows, kern, conv_shape(kern, C0, C1, Cout, H, W, up2), tokens)
    chk = Checker(label, fam, TOL_FWD)
    chk("out", row, out.cpu(), ref(torch.float64), floor)
    chk.done()


# ---- dm_op_downsample -----------------------------------------------------------------------------------------------------
# (B, C, H, W, Cout, expectation, input families beyond randn): space-to-depth, then a 1x1 convolution over 4 C channels
DOWN_CASES = [
    (2, 32, 16, 16, 64, dict(default="pw r1"), HARD),
    (3, 64, 8, 8, 128, dict(default="pw r1"), ()),             # ragged pixel block
    (2, 128, 4, 4, 256, dict(default="pw r1 k>1"), ()),        # K split
    (1, 16, 6, 10, 16, dict(default="conv"), ()),              # 16 couts: direct kernel
    (2, 48, 8, 8, 64, dict(default="conv"), ()),               # three chunks per sub-pixel (no power of two): direct kernel
]
DOWN_RUNS = [(c, f) for c in DOWN_CASES if runs_here(c[5]) for f in ("randn",) + c[6]]


@pytest.mark.parametrize("run", DOWN_RUNS, ids=[run_id(r) for r in DOWN_RUNS])
def test_downsample(run):
    (B, C, H, W, Cout, exp, _), fam = run
    label = "downsample " + run_id(run)
    kern, tokens = expected(exp)
    x = family_input(seeded((B, C, H, W), 1), fam, 7)
    sd = {"d.1.weight": seeded((Cout, 4 * C, 1, 1), 2, (4 * C) ** -0.5), "d.1.bias": seeded((Cout,), 3)}
    ref = uo.downsample({n: t.double() for n, t in sd.items()}, "d", x.double())
    floor = cr.direct(cr.space_to_depth(x), sd["d.1.weight"]) + sd["d.1.bias"][None, :, None, None]
    out = nans(*ref.shape)
    a = [dev(x), dev(sd["d.1.weight"]), dev(sd["d.1.bias"])]
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_downsample(
        _lib.ptr(a[0]), C, _lib.ptr(a[1]), _lib.ptr(a[2]), _lib.ptr(out), B, H, W, Cout, None)))
    row = assert_row(label, rows, kern, f" {C}+0->{Cout} @{H // 2}x{W // 2} s2d", tokens)
    chk = Checker(label, fam, TOL_FWD)
    chk("out", row, out.cpu(), ref, floor)
    chk.done()


# ---- dm_op_block ----------------------------------------------------------------------------------------------------------
# (B, Cin, Cout, H, W, scale_shift, expectation, input families beyond randn)
BLOCK_CASES = [
    (5, 64, 64, 4, 4, True, dict(default="wino q2", forced="wino4"), HARD),   # fused epilogue; scale_shift rows of 5 images in one tile
    (2, 768, 512, 4, 4, True, W2_W4, ()),                                      # Cout > 256: separate norm
    (2, 64, 128, 16, 16, False, W2_W4, ()),                                    # two cout tiles: landing pass
    (3, 64, 64, 12, 10, True, dict(default="wino q2"), ()),                    # F(2x2) fused epilogue on masked tiles
    (2, 64, 64, 7, 9, True, dict(default="conv"), HARD),                       # direct kernel
    (2, 32, 48, 8, 8, True, dict(default="conv"), ()),                         # 48 couts
    (2, 64, 320, 5, 5, True, dict(default="conv"), ()),                        # direct kernel, Cout > 256: separate norm
]
BLOCK_RUNS = [(c, f) for c in BLOCK_CASES if runs_here(c[6]) for f in ("randn",) + c[7]]


def block_tail(y, g, scale, shift):
    y = uo.rms_norm(y, g)
    if scale is not None:
        y = y * (scale + 1) + shift
    return F.silu(y)


def block_inputs(B, Cin, Cout, H, W, ss, fam):
    x = family_input(seeded((B, Cin, H, W), 1), fam, 7)
    w = seeded((Cout, Cin, 3, 3), 2, (9 * Cin) ** -0.5)
    b = seeded((Cout,), 3, 0.1)
    g = 1 + 0.3 * seeded((1, Cout, 1, 1), 4)
    scale = seeded((B, Cout, 1, 1), 5, 0.5) if ss else None
    shift = seeded((B, Cout, 1, 1), 6, 0.5) if ss else None
    return x, w, b, g, scale, shift


@pytest.mark.parametrize("run", BLOCK_RUNS, ids=[run_id(r) for r in BLOCK_RUNS])
def test_block(run):
    (B, Cin, Cout, H, W, ss, exp, _), fam = run
    label = "block " + run_id(run)
    kern, tokens = expected(exp)
    x, w, b, g, scale, shift = block_inputs(B, Cin, Cout, H, W, ss, fam)
    d = [None if t is None else t.double() for t in (x, w, b, g, scale, shift)]
    ref = block_tail(F.conv2d(d[0], d[1], d[2], padding=1), d[3], d[4], d[5])
    floor = block_tail(cr.forward(x, w, restate_family(kern), 3) + b[None, :, None, None], g, scale, shift)
    out = nans(B, Cout, H, W)
    a = [dev(t) for t in (x, w, b, g, None if scale is None else scale.reshape(B, Cout),
                          None if shift is None else shift.reshape(B, Cout))]
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_block(
        _lib.ptr(a[0]), Cin, _lib.ptr(a[1]), _lib.ptr(a[2]), _lib.ptr(a[3]), _lib.ptr(a[4]), _lib.ptr(a[5]), _lib.ptr(out), B, H, W,
        Cout, None)))
    row = assert_row(label, rows, kern, conv_shape(kern, Cin, 0, Cout, H, W, False), tokens)
    chk = Checker(label, fam, TOL_FWD)
    chk("out", row, out.cpu(), ref, floor)
    chk.done()


# ---- dm_op_conv2d_bwd -----------------------------------------------------------------------------------------------------
# (B, C0, C1, H, W, Cout, k, up2, weight-gradient mode, pixel split, {switches: input-gradient family per source}, families)
# The input gradient of source i is a k x k convolution Cout -> Ci with the rotated, transposed weights, at the size of dy
# (with up2: at the upsampled size, followed by the 2x2 sums).
D_W2_W4 = dict(default="wino", forced="wino4")
CONV_BWD_CASES = [
    (3, 64, 64, 16, 16, 64, 3, False, "wino", True, D_W2_W4, HARD),                  # two sources
    (5, 256, 0, 4, 4, 256, 3, False, "wino", False, D_W2_W4, ()),                    # whole small images per block, ragged batch
    (1, 64, 0, 64, 64, 64, 3, False, "wino", True, D_W2_W4, ()),                     # one row per pixel block
    (2, 128, 0, 8, 8, 64, 3, True, "wino", True, D_W2_W4, HARD),                     # up2: Upsample 128 -> 64
    (2, 32, 0, 8, 8, 16, 3, True, "wino", True, dict(default="conv"), ()),           # up2, thin channels
    (2, 20, 12, 7, 9, 36, 3, False, "direct", True, dict(default="conv"), HARD),     # odd size, two sources, multiples of 4
    (2, 64, 0, 7, 9, 64, 3, False, "direct", True, dict(default="conv"), ()),        # odd size, whole tiles of channels
    (5, 64, 0, 5, 5, 128, 3, False, "direct", False, dict(default="conv"), ()),      # whole small images per block, ragged batch
    (2, 64, 0, 16, 16, 384, 1, False, "1x1", True, dict(default="pw"), HARD),        # to_qkv
    (2, 128, 64, 8, 8, 64, 1, False, "1x1", False, dict(default="pw"), ()),          # two sources
    (3, 24, 0, 5, 6, 40, 1, False, "1x1", False, dict(default="conv"), ()),          # odd everything, ragged batch
]
CONV_BWD_RUNS = [(c, f) for c in CONV_BWD_CASES if runs_here(c[10], c[8]) for f in ("randn",) + c[11]]


def wgrad_mode_here(mode):
    return "direct" if (mode == "wino" and CFG == "alt") else mode


@pytest.mark.parametrize("run", CONV_BWD_RUNS, ids=[run_id(r) for r in CONV_BWD_RUNS])
def test_conv2d_bwd(run):
    (B, C0, C1, H, W, Cout, k, up2, mode, split, exp, _), fam = run
    label = "conv2d_bwd " + run_id(run)
    dkern, _ = expected(exp)
    mode = wgrad_mode_here(mode)
    pad, s = k // 2, (2 if up2 else 1)
    Ho, Wo = s * H, s * W
    x = family_input(torch.cat((seeded((B, C0, H, W), 1), seeded((B, C1, H, W), 2)), 1), fam, 7)
    w = seeded((Cout, C0 + C1, k, k), 3, 1.0 / (k * (C0 + C1) ** 0.5))
    b = seeded((Cout,), 4, 0.1)
    dy = family_input(seeded((B, Cout, Ho, Wo), 5), fam, 8)

    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = torch.autograd.grad(F.conv2d(cr.upsample2(xd) if up2 else xd, wd, bd, padding=pad), (xd, wd, bd), dy.double())
    spec = dict(k=k, up2=up2, c0=C0, fwd="upfold" if up2 else "direct", dgrad=(restate_family(dkern),) * 2,
                wgrad="wino" if mode == "wino" else "direct")
    xf, wf, bf = (t.clone().requires_grad_(True) for t in (x, w, b))
    floor = torch.autograd.grad(cr.conv(xf, wf, bf, spec), (xf, wf, bf), dy)

    d0, d1 = nans(B, C0, H, W), (nans(B, C1, H, W) if C1 else None)
    dw, db = nans(Cout, C0 + C1, k, k), nans(Cout)
    a = [dev(t) for t in (x[:, :C0], x[:, C0:] if C1 else None, w, dy)]
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_conv2d_bwd(
        _lib.ptr(a[0]), C0, _lib.ptr(a[1]), C1, _lib.ptr(a[2]), _lib.ptr(a[3]), _lib.ptr(d0), _lib.ptr(d1), _lib.ptr(dw),
        _lib.ptr(db), B, H, W, Cout, k, pad, int(up2), None)))
    wrow = assert_wgrad_row(label, rows, mode, f" {C0}+{C1}->{Cout} @{Ho}x{Wo}" + (" up" if up2 else ""), split)
    r0 = assert_row(label, rows, dkern, conv_shape(dkern, Cout, 0, C0, Ho, Wo, False))
    chk = Checker(label, fam, TOL_BWD)
    chk("dx0", r0, d0.cpu(), ref[0][:, :C0], floor[0][:, :C0])
    if C1:
        r1 = assert_row(label, rows, dkern, conv_shape(dkern, Cout, 0, C1, Ho, Wo, False))
        chk("dx1", r1, d1.cpu(), ref[0][:, C0:], floor[0][:, C0:])
    chk("dw", wrow, dw.cpu(), ref[1], floor[1])
    chk("db", "colsum", db.cpu(), ref[2], floor[2])
    chk.done()


# ---- dm_op_downsample_bwd -------------------------------------------------------------------------------------------------
# (B, C, H, W, Cout, pixel split, {switches: family of the 1x1 input-gradient convolution Cout -> 4 C}, families)
DOWN_BWD_CASES = [
    (3, 64, 16, 16, 128, True, dict(default="pw"), HARD),
    (2, 32, 8, 12, 48, False, dict(default="pw"), ()),        # 48 couts: three chunks of the input gradient
    (5, 16, 4, 4, 20, False, dict(default="conv"), ()),       # whole small images per block, ragged batch, multiples of 4
    (2, 64, 32, 32, 64, True, dict(default="pw"), ()),
]
DOWN_BWD_RUNS = [(c, f) for c in DOWN_BWD_CASES if runs_here(c[6]) for f in ("randn",) + c[7]]


@pytest.mark.parametrize("run", DOWN_BWD_RUNS, ids=[run_id(r) for r in DOWN_BWD_RUNS])
def test_downsample_bwd(run):
    (B, C, H, W, Cout, split, exp, _), fam = run
    label = "downsample_bwd " + run_id(run)
    dkern, _ = expected(exp)
    x = family_input(seeded((B, C, H, W), 1), fam, 7)
    w = seeded((Cout, 4 * C, 1, 1), 2, 0.05)
    b = seeded((Cout,), 3, 0.1)
    dy = family_input(seeded((B, Cout, H // 2, W // 2), 4), fam, 8)

    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = torch.autograd.grad(uo.downsample({"d.1.weight": wd, "d.1.bias": bd}, "d", xd), (xd, wd, bd), dy.double())
    spec = dict(k=1, fwd="direct", dgrad=("direct",), wgrad="direct")
    xf, wf, bf = (t.clone().requires_grad_(True) for t in (x, w, b))
    floor = torch.autograd.grad(cr.conv(cr.space_to_depth(xf), wf, bf, spec), (xf, wf, bf), dy)

    dx, dw, db = nans(B, C, H, W), nans(Cout, 4 * C, 1, 1), nans(Cout)
    a = [dev(x), dev(w), dev(dy)]
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_downsample_bwd(
        _lib.ptr(a[0]), C, _lib.ptr(a[1]), _lib.ptr(a[2]), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), B, H, W, Cout, None)))
    wrow = assert_wgrad_row(label, rows, "s2d", f" {C}+0->{Cout} @{H // 2}x{W // 2}", split)
    drow = assert_row(label, rows, dkern, f" {Cout}+0->{4 * C} @{H // 2}x{W // 2} ")
    chk = Checker(label, fam, TOL_BWD)
    chk("dx", drow, dx.cpu(), ref[0], floor[0])
    chk("dw", wrow, dw.cpu(), ref[1], floor[1])
    chk("db", "colsum", db.cpu(), ref[2], floor[2])
    chk.done()


# ---- dm_op_block_bwd ------------------------------------------------------------------------------------------------------
# (B, Cin, Cout, H, W, scale_shift, weight-gradient mode, pixel split, {switches: family of the forward convolution and of the
# input-gradient convolution}); Cin != Cout, so that the two rows differ
BLOCK_BWD_CASES = [
    (2, 64, 128, 16, 16, True, "wino", True, D_W2_W4),
    (5, 128, 64, 4, 4, True, "wino", False, D_W2_W4),                # scale_shift rows of several images in one tile, ragged
    (2, 64, 320, 4, 4, True, "wino", False, D_W2_W4),                # Cout > 256
    (2, 24, 40, 7, 5, True, "direct", False, dict(default="conv")),  # odd size, multiples of 4
    (2, 128, 64, 7, 9, False, "direct", True, dict(default="conv")),
]
BLOCK_BWD_RUNS = [(c, "randn") for c in BLOCK_BWD_CASES if runs_here(c[8], c[6])]


@pytest.mark.parametrize("run", BLOCK_BWD_RUNS, ids=[run_id(r) for r in BLOCK_BWD_RUNS])
def test_block_bwd(run):
    (B, Cin, Cout, H, W, ss, mode, split, exp), fam = run
    label = "block_bwd " + run_id(run)
    kern, _ = expected(exp)
    mode = wgrad_mode_here(mode)
    ins = block_inputs(B, Cin, Cout, H, W, ss, fam)
    dy = seeded((B, Cout, H, W), 7)
    names = ["dx", "dw", "db", "dg"] + (["dscale", "dshift"] if ss else [])

    def grads(dt, conv):
        t = [None if v is None else v.to(dt).requires_grad_(True) for v in ins]
        y = block_tail(conv(t[0], t[1], t[2]), t[3], t[4], t[5])
        return torch.autograd.grad(y, [v for v in t if v is not None], dy.to(dt))

    ref = grads(torch.float64, lambda x, w, b: F.conv2d(x, w, b, padding=1))
    spec = dict(k=3, fwd=restate_family(kern), dgrad=(restate_family(kern),), wgrad="wino" if mode == "wino" else "direct")
    floor = grads(torch.float32, lambda x, w, b: cr.conv(x, w, b, spec))

    outs = dict(dx=nans(B, Cin, H, W), dw=nans(Cout, Cin, 3, 3), db=nans(Cout), dg=nans(Cout),
                dscale=nans(B, Cout) if ss else None, dshift=nans(B, Cout) if ss else None)
    x, w, b, g, scale, shift = ins
    a = [dev(t) for t in (x, w, b, g, None if scale is None else scale.reshape(B, Cout),
                          None if shift is None else shift.reshape(B, Cout), dy)]
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_block_bwd(
        _lib.ptr(a[0]), Cin, *[_lib.ptr(t) for t in a[1:]], *[_lib.ptr(outs[n]) for n in ("dx", "dw", "db", "dg", "dscale", "dshift")], B, H, W, Cout,
        None)))
    frow = assert_row(label, rows, kern, conv_shape(kern, Cin, 0, Cout, H, W, False))
    drow = assert_row(label, rows, kern, conv_shape(kern, Cout, 0, Cin, H, W, False))
    wrow = assert_wgrad_row(label, rows, mode, f" {Cin}+0->{Cout} @{H}x{W}", split)
    chk = Checker(label, fam, TOL_BWD)
    for n, r64, f32 in zip(names, ref, floor):
        kernel = {"dx": drow, "dw": wrow}.get(n, f"norm_act_bwd behind {frow}")
        chk(n, kernel, outs[n].cpu().reshape(r64.shape), r64, f32)
    chk.done()


def test_naive_weight_gradient_has_no_operator():
    pytest.skip("wgrad_naive_kernel (7x7 first conv over the NCHW image, final_conv with 3 outputs): dm_op_conv2d_bwd takes "
                "3x3 and 1x1 only, so no operator reaches it; tests/test_hip_train.py does through the model")


def test_every_family_and_mode_got_its_cases():
    """Runs last: the cases above must have reached every family and mode that the switches of this process allow."""
    want = {"default": ["conv_mfma", "wino_mfma", "pw_mfma", "init7_mfma", "wgrad_mfma direct", "wgrad_mfma 1x1",
                        "wgrad_mfma s2d", "wgrad_mfma wino"],
            "forced": ["wino4_mfma", "upwino_mfma", "wgrad_mfma wino"],
            "alt": ["wino_mfma", "pw_mfma", "wgrad_mfma direct"]}[CFG]
    print(f"conv families [{CFG}]: " + ", ".join(f"{n} {COUNTS[n]}" for n in sorted(COUNTS)))
    total = sum(len(r) for r in (CONV_RUNS, DOWN_RUNS, BLOCK_RUNS, CONV_BWD_RUNS, DOWN_BWD_RUNS, BLOCK_BWD_RUNS))
    if COUNTS["cases run"] != total:
        pytest.skip(f"only {COUNTS['cases run']} of {total} cases were selected: the counts say nothing")
    short = {n: COUNTS[n] for n in want if COUNTS[n] < 3}
    assert not short, short
