"""GPU parity of the convolution forms and blocks of the first-stage models (csrc/dm_vae.inc: VQ decoder, VQ encoder,
AutoencoderKL), one trunk node at a time through the C ABI (dm_op_vae_conv, dm_op_vae_resblock, dm_op_vae_attn_block: the code
the trunk runs for the node), against the plain definition evaluated in fp64 on the CPU on the same fp32 inputs.  These are the
forms that dm_op_conv2d / dm_op_downsample / dm_op_block (tests/test_hip_conv_families.py) cannot express:
  s2        3x3, stride 2, pad 0, one more row and column of zeros below and right (encoder.down.N.downsample.conv)
  nchw_in   1x1 / 3x3 reading an NCHW tensor of 3, 4 or 8 channels (post_quant_conv, encoder.conv_in)
  nchw_out  3x3 writing NCHW with a handful of output channels (decoder.conv_out)
  scalar    NHWC with input or output channels that are no multiple of 4 (encoder.conv_out, quant_conv)
  thin      1x1, NHWC in, NCHW out, 1..8 output channels: pointwise_small_kernel, the U-Net's final_conv
  up        nearest x2 + 3x3 as the trunk calls it (decoder.up.N.upsample.conv)
  res       GroupNorm + swish, 3x3, GroupNorm + swish, 3x3 with the residual; with nin_shortcut the residual rides on the 1x1
  attn      GroupNorm, q / k / v 1x1, the attention core, proj_out with the residual

Reference.  Convolutions: F.conv2d in fp64; the stride-2 form with F.pad(x, (0, 1, 0, 1)) in front, as the model this was ported
from does.  Blocks: the composition of F.group_norm(., 32, eps=1e-6), x * sigmoid(x), F.conv2d and the softmax with scale
C ** -0.5 over the tokens.

Limits.  Convolutions: the two metrics of conv_checks.Checker (rel-L2 and max|d| / rms); the floor is conv_restate.direct (the
folded nearest-x2 form: conv_restate.upfold) in fp32 against fp64 with the zero row and column added to the input beforehand;
the kernel may be 4 x the floor off and ``randn`` inputs also stay under 2e-5.  Every conv case also judges three slices on
their own by the same rule -- the last output row, the last output column and the first row of image 1 -- in the ``offset``
family (t + 4) as well: a pad that reads the neighbouring image's row instead of a zero is far above the floor there.
Blocks: rel-L2; the floor is the same composition in fp32 on the CPU; the limit is max(2e-5, 4 x floor), the rule of
tests/test_hip_vae_ops.py.  No limit comes from the kernel's output.  Every output tensor starts as NaNs and must end finite
(run_op fills the operator workspace with NaNs as well).

Dispatch.  Every case names in the table, never from the library's plan functions, the kernel family of its convolutions and
asserts it from the detail profile rows around the call.  pointwise_small_kernel records no row: its cases assert that the
call left no conv<, pw< or wino row.  The attention core records none either: the table states the kernel by the condition
of vae_attn_mfma_ok (n % 32 == 0 and C in 64, 128, 256: the MFMA kernel; else one row per wavefront).
Every case prints ``case tensor kernel: kernel error, floor, limit`` before it asserts (run with -s; DESIGN.md holds the
table); the last test counts the cases that reached each form."""
import collections

import pytest
import torch
import torch.nn.functional as F

import conv_checks
import conv_restate as cr
from conv_checks import dev, family_input, nans, profiled_call, seeded
from diffusion_models_amd import _lib

pytestmark = pytest.mark.gpu
TOL = 2e-5
FACTOR = 4.0
COUNTS = collections.Counter()
TAG = "vae_conv_ops"


@pytest.fixture(scope="module", autouse=True)
def profiled():
    _lib.profile_enable(True, detail=True)
    _lib.profile_read()
    yield
    _lib.profile_read()
    _lib.profile_enable(False)
    print(f"\n{TAG}: cases per form")
    for name, n in sorted(COUNTS.items()):
        print(f"  {name}: {n}")


def case_id(case):
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in case if not isinstance(v, (dict, tuple)))


# ---- dm_op_vae_conv -------------------------------------------------------------------------------------------------------
def conv_case(form, B, C, H, W, Cout, k=3, stride=1, pad=1, pad_hi=0, up=False, in_nchw=False, out_nchw=False, bias=True,
              expect="conv", families=("randn", "offset")):
    return (form, B, C, H, W, Cout, k, stride, pad, pad_hi, up, in_nchw, out_nchw, bias, expect, families)


def s2(B, C, H, W, Cout, expect="conv", families=("randn", "offset")):
    return conv_case("s2", B, C, H, W, Cout, 3, 2, 0, 1, expect=expect, families=families)


CONV_CASES = [
    # 3x3 / stride 2 / pad_hi 1: the direct kernel.  Out = (H + 1 - 3) // 2 + 1
    s2(2, 32, 8, 8, 32),
    s2(3, 64, 6, 10, 64),                                   # non-square, ragged tiles
    s2(2, 32, 5, 7, 32),                                    # odd sizes: the added row is not read, the last window ends at it
    s2(5, 32, 2, 2, 32),                                    # 1x1 output, ragged batch
    s2(2, 20, 4, 6, 36),                                    # CK = 4
    s2(1, 256, 4, 4, 256, expect="conv k>1"),               # K split that lands through norm_act
    s2(2, 64, 16, 16, 64, families=("randn", "offset", "wide")),
    # NCHW source, 1x1 (post_quant_conv)
    *[conv_case("nchw_in", 3, C, H, W, Cout, 1, 1, 0, in_nchw=True)
      for C in (3, 4, 8) for Cout in (3, 4) for H, W in ((4, 4), (5, 3))],
    # NCHW source, 3x3 / pad 1 (encoder.conv_in)
    *[conv_case("nchw_in", 3, 3, H, W, Cout, in_nchw=True) for Cout in (32, 64) for H, W in ((8, 8), (7, 9))],
    conv_case("nchw_in", 3, 4, 4, 4, 128, in_nchw=True),
    # NCHW output, 3x3 / pad 1 (decoder.conv_out); B = 3: the image index of the store off zero
    *[conv_case("nchw_out", 3, C, H, W, 3, out_nchw=True) for C in (32, 64, 128) for H, W in ((8, 8), (7, 5))],
    *[conv_case("nchw_out", 3, 64, 6, 6, Cout, out_nchw=True) for Cout in (1, 4, 6)],
    conv_case("nchw_out", 3, 256, 4, 4, 4, out_nchw=True, expect="conv k1"),  # its NHWC twin splits K; NCHW output never does
    # NHWC with channel counts off the multiples of 4 (encoder.conv_out, quant_conv)
    *[conv_case("scalar", 2, 64, H, H, Cout) for Cout in (3, 6, 8) for H in (4, 5)],
    *[conv_case("scalar", 70, C, 4, 4, Cout, 1, 1, 0) for C, Cout in ((3, 3), (6, 4), (8, 8), (4, 8))],  # one ragged pixel tile
    # thin pointwise: k = 1, NHWC in, NCHW out, 1..8 couts (pointwise_small_kernel<1..8>): no profile row
    *[conv_case("thin", 2, 64, 4, 4, Cout, 1, 1, 0, out_nchw=True, bias=Cout % 2 == 1, expect="thin") for Cout in range(1, 9)],
    conv_case("thin", 2, 4, 4, 4, 3, 1, 1, 0, out_nchw=True, expect="thin"),
    conv_case("thin", 2, 36, 4, 4, 3, 1, 1, 0, out_nchw=True, bias=False, expect="thin"),
    conv_case("thin", 2, 512, 4, 4, 8, 1, 1, 0, out_nchw=True, expect="thin"),
    conv_case("thin", 1, 64, 15, 17, 3, 1, 1, 0, out_nchw=True, expect="thin"),               # 255 pixels
    conv_case("thin", 1, 64, 16, 16, 3, 1, 1, 0, out_nchw=True, bias=False, expect="thin"),   # 256: exactly one block
    conv_case("thin", 1, 64, 257, 1, 3, 1, 1, 0, out_nchw=True, expect="thin"),               # 257: one thread in the second
    conv_case("thin", 3, 64, 5, 7, 5, 1, 1, 0, out_nchw=True, expect="thin"),
    # nearest x2 + 3x3 as the trunk calls it (the families themselves: tests/test_hip_conv_families.py)
    conv_case("up", 2, 64, 4, 4, 64, up=True),
    conv_case("up", 1, 32, 3, 5, 32, up=True),
]
CONV_RUNS = [(c, f) for c in CONV_CASES for f in c[15]]


def conv_out_size(H, W, k, stride, pad, pad_hi, up):
    s = 2 if up else 1
    return (s * H + 2 * pad + pad_hi - k) // stride + 1, (s * W + 2 * pad + pad_hi - k) // stride + 1


def conv_reference(x, w, b, stride, pad, pad_hi, up, dt):
    xd = cr.upsample2(x.to(dt)) if up else x.to(dt)
    if pad_hi:
        xd = F.pad(xd, (0, pad_hi, 0, pad_hi))
    return F.conv2d(xd, w.to(dt), None if b is None else b.to(dt), stride=stride, padding=pad)


def conv_floor(x, w, b, stride, pad, pad_hi, up):
    if up:
        y = cr.upfold(x, w)
    else:
        y = cr.direct(F.pad(x, (0, pad_hi, 0, pad_hi)) if pad_hi else x, w, pad=pad, stride=stride)
    return y if b is None else y + b[None, :, None, None]


def conv_inputs(case, fam):
    _, B, C, H, W, Cout, k, _, _, _, _, _, _, bias, _, _ = case
    x = family_input(seeded((B, C, H, W), 1), fam, 7)
    w = seeded((Cout, C, k, k), 3, C ** -0.5 / k)
    b = seeded((Cout,), 4) if bias else None
    return x, w, b


def hip_vae_conv(x, w, b, case):
    """x (B, C, H, W) on the host -> the operator's output as (B, Cout, Ho, Wo) on the host, and the profile rows of the call."""
    _, B, C, H, W, Cout, k, stride, pad, pad_hi, up, in_nchw, out_nchw, _, _, _ = case
    Ho, Wo = conv_out_size(H, W, k, stride, pad, pad_hi, up)
    a = [dev(x if in_nchw else x.permute(0, 2, 3, 1)), dev(w), dev(b)]
    out = nans(B, Cout, Ho, Wo) if out_nchw else nans(B, Ho, Wo, Cout)
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_vae_conv(
        _lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), _lib.ptr(out), B, H, W, C, Cout, k, stride, pad, pad_hi, int(up),
        int(in_nchw), int(out_nchw), None)))
    got = out.cpu()
    return (got if out_nchw else got.permute(0, 3, 1, 2).contiguous()), rows


def assert_conv_dispatch(label, rows, case):
    form, _, C, H, W, Cout, k, stride, pad, pad_hi, up, _, _, _, expect, _ = case
    if expect == "thin":
        stray = [r for r in rows if r.startswith(("conv<", "pw<", "wino"))]
        assert not stray, (label, "pointwise_small_kernel records no row, yet", stray)
        return "pointwise_small"
    family, *tokens = expect.split()
    Ho, Wo = conv_out_size(H, W, k, stride, pad, pad_hi, up)
    # the folded direct kernel names its source grid and its four 2x2 parity convolutions
    shape = f" {C}+0->{Cout} @{H}x{W} upfold " if up else f" {k}x{k} s{stride} {C}+0->{Cout} @{Ho}x{Wo} "
    return conv_checks.assert_row(COUNTS, label, rows, family, shape, tokens)


@pytest.mark.parametrize("run", CONV_RUNS, ids=[f"{f}-{case_id(c)}" for c, f in CONV_RUNS])
def test_vae_conv(run):
    case, fam = run
    form, B = case[0], case[1]
    stride, pad, pad_hi, up = case[7:11]
    label = f"conv {fam}-{case_id(case)}"
    x, w, b = conv_inputs(case, fam)
    ref = conv_reference(x, w, b, stride, pad, pad_hi, up, torch.float64)
    floor = conv_floor(x, w, b, stride, pad, pad_hi, up)
    got, rows = hip_vae_conv(x, w, b, case)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    row = assert_conv_dispatch(label, rows, case)
    chk = conv_checks.Checker(TAG, COUNTS, label, fam, TOL)
    chk("out", row, got, ref, floor)
    edges = [("last row", (slice(None), slice(None), -1)), ("last column", (slice(None), slice(None), slice(None), -1))]
    if B > 1:
        edges.append(("first row of image 1", (1, slice(None), 0)))
    for name, sl in edges:
        chk(f"out[{name}]", row, got[sl], ref[sl], floor[sl])
    COUNTS[form] += 1
    chk.done()


# ---- the two blocks -------------------------------------------------------------------------------------------------------
def swish(x):
    return x * torch.sigmoid(x)


def group_means(x, mean):
    """`mean` times +-1 (alternating, +-10 % from group to group) added to each of the 32 channel groups of x (B, C, H, W)."""
    C = x.shape[1]
    g = torch.Generator().manual_seed(7)
    gm = mean * (1 + 0.1 * (2 * torch.rand(32, generator=g) - 1)) * (1 - 2.0 * (torch.arange(32) % 2))
    return x + gm.repeat_interleave(C // 32)[None, :, None, None]


def block_check(label, got, ref, floor32, what):
    e, f = conv_checks.metrics(got, ref), conv_checks.metrics(floor32, ref)
    lim = max(TOL, FACTOR * f[0])
    print(f"{TAG} {label} out {what}: rel-L2 kernel {e[0]:.3g} floor {f[0]:.3g} limit {lim:.3g} | max/rms kernel {e[1]:.3g} "
          f"floor {f[1]:.3g}")
    assert torch.isfinite(got).all(), (label, "not finite", int((~torch.isfinite(got)).sum()))
    assert e[0] <= lim, (label, e, lim)


def rows_of(x):
    return x.permute(0, 2, 3, 1).contiguous()


# (B, cin, cout, H, W, family of the two 3x3 convolutions, family of nin_shortcut, input family)
RES_CASES = [
    (2, 32, 32, 4, 4, "conv", None, "randn"),      # 32 couts: off the 64-cout tiles of F(2x2)
    (2, 32, 64, 4, 4, "wino", "pw", "randn"),
    (3, 64, 64, 5, 7, "conv", None, "randn"),      # odd sizes
    (1, 128, 256, 8, 8, "wino", "pw", "randn"),
    (2, 64, 32, 6, 6, "conv", "conv", "randn"),    # nin_shortcut to 32 couts: not a 1x1 GEMM tile
    (2, 64, 32, 6, 6, "conv", "conv", "mean30"),   # every group of the input at mean +-30, std 1
    (3, 64, 64, 5, 7, "conv", None, "mean30"),
]


def res_params(cin, cout):
    P = dict(n1w=1 + 0.3 * seeded((cin,), 2), n1b=seeded((cin,), 3, 0.5), c1w=seeded((cout, cin, 3, 3), 4, (9 * cin) ** -0.5),
             c1b=seeded((cout,), 5, 0.1), n2w=1 + 0.3 * seeded((cout,), 6), n2b=seeded((cout,), 7, 0.5),
             c2w=seeded((cout, cout, 3, 3), 8, (9 * cout) ** -0.5), c2b=seeded((cout,), 9, 0.1))
    if cin != cout:
        P.update(ninw=seeded((cout, cin, 1, 1), 10, cin ** -0.5), ninb=seeded((cout,), 11, 0.1))
    return P


def res_reference(x, P, dt):
    p = {n: t.to(dt) for n, t in P.items()}
    x = x.to(dt)
    h = F.conv2d(swish(F.group_norm(x, 32, p["n1w"], p["n1b"], eps=1e-6)), p["c1w"], p["c1b"], padding=1)
    h = F.conv2d(swish(F.group_norm(h, 32, p["n2w"], p["n2b"], eps=1e-6)), p["c2w"], p["c2b"], padding=1)
    if "ninw" in p:
        x = F.conv2d(x, p["ninw"], p["ninb"])
    return x + h


RES_ORDER = ("n1w", "n1b", "c1w", "c1b", "n2w", "n2b", "c2w", "c2b", "ninw", "ninb")


@pytest.mark.parametrize("case", RES_CASES, ids=[case_id(c) for c in RES_CASES])
def test_vae_resblock(case):
    B, cin, cout, H, W, k3, nin, fam = case
    label = f"resblock {case_id(case)}"
    x = seeded((B, cin, H, W), 1)
    if fam == "mean30":
        x = group_means(x, 30.0)
    P = res_params(cin, cout)
    ref = res_reference(x, P, torch.float64)
    floor = res_reference(x, P, torch.float32)
    a = [dev(rows_of(x))] + [dev(P.get(n)) for n in RES_ORDER]
    out = nans(B, H, W, cout)
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_vae_resblock(
        *[_lib.ptr(t) for t in a], _lib.ptr(out), B, H, W, cin, cout, None)))
    r1 = conv_checks.assert_row(COUNTS, label, rows, k3, f" 3x3 s1 {cin}+0->{cout} @{H}x{W} ")
    conv_checks.assert_row(COUNTS, label, rows, k3, f" 3x3 s1 {cout}+0->{cout} @{H}x{W} ")
    if nin:
        conv_checks.assert_row(COUNTS, label, rows, nin, f" 1x1 {cin}+0->{cout} @{H}x{W} " if nin == "pw" else
                               f" 1x1 s1 {cin}+0->{cout} @{H}x{W} ")
    COUNTS["res nin" if nin else "res"] += 1
    block_check(label, out.cpu().permute(0, 3, 1, 2), ref, floor, r1)


# (B, C, H, W, family of the four 1x1 convolutions, attention kernel by vae_attn_mfma_ok: n % 32 == 0 and C in 64, 128, 256)
ATTN_CASES = [
    (1, 32, 4, 4, "conv", "rows"),      # C = 32: the row kernel at any n; 32 couts: the direct kernel
    (3, 32, 8, 8, "conv", "rows"),
    (3, 64, 4, 4, "pw", "rows"),        # n = 16
    (1, 64, 3, 5, "pw", "rows"),        # n = 15
    (3, 64, 8, 8, "pw", "mfma"),        # n = 64
    (1, 128, 8, 8, "pw", "mfma"),
    (3, 128, 3, 5, "pw", "rows"),
    (3, 128, 4, 4, "pw", "rows"),
    (1, 64, 16, 16, "pw", "mfma"),      # n = 256: two query blocks of 128 per image
]


def attn_params(C):
    P = dict(nw=1 + 0.3 * seeded((C,), 2), nb=seeded((C,), 3, 0.5))
    for i, n in enumerate(("q", "k", "v", "proj")):
        P[n + "w"] = seeded((C, C, 1, 1), 4 + 2 * i, C ** -0.5)
        P[n + "b"] = seeded((C,), 5 + 2 * i, 0.1)
    return P


def attn_reference(x, P, dt):
    p = {n: t.to(dt) for n, t in P.items()}
    x = x.to(dt)
    B, C, H, W = x.shape
    h = F.group_norm(x, 32, p["nw"], p["nb"], eps=1e-6)
    q, k, v = (F.conv2d(h, p[n + "w"], p[n + "b"]).reshape(B, C, H * W) for n in ("q", "k", "v"))
    a = torch.softmax(torch.bmm(q.permute(0, 2, 1), k) * C ** -0.5, dim=2)   # (B, query token, key token)
    h = torch.bmm(v, a.permute(0, 2, 1)).reshape(B, C, H, W)
    return x + F.conv2d(h, p["projw"], p["projb"])


ATTN_ORDER = ("nw", "nb", "qw", "qb", "kw", "kb", "vw", "vb", "projw", "projb")


@pytest.mark.parametrize("case", ATTN_CASES, ids=[case_id(c) for c in ATTN_CASES])
def test_vae_attn_block(case):
    B, C, H, W, k1, core = case
    assert (core == "mfma") == ((H * W) % 32 == 0 and C in (64, 128, 256)), "the table misstates the condition of the kernels"
    label = f"attn_block {case_id(case)}"
    x = seeded((B, C, H, W), 1)
    P = attn_params(C)
    ref = attn_reference(x, P, torch.float64)
    floor = attn_reference(x, P, torch.float32)
    a = [dev(rows_of(x))] + [dev(P[n]) for n in ATTN_ORDER]
    out = nans(B, H, W, C)
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_vae_attn_block(
        *[_lib.ptr(t) for t in a], _lib.ptr(out), B, H, W, C, None)))
    r = conv_checks.assert_row(COUNTS, label, rows, k1, f" 1x1 {C}+0->{C} @{H}x{W} " if k1 == "pw" else
                               f" 1x1 s1 {C}+0->{C} @{H}x{W} ")
    COUNTS[f"attn {core}"] += 1
    block_check(label, out.cpu().permute(0, 3, 1, 2), ref, floor, f"{r} / attention {core}")


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    """What the trunk's code refuses comes back as the library's error, and nothing is written."""
    lib = _lib.load()
    B, C, H, W = 2, 64, 4, 4
    x, w, b = dev(seeded((B, H, W, C), 1)), dev(seeded((3, C, 3, 3), 2, 0.05)), dev(seeded((3,), 3))
    # NCHW output asked of a call whose plan leaves partial sums for a landing pass, which writes NHWC.  A plain convolution
    # never gets there (conv_plan takes no K split under NCHW output: the `conv k1` case above); nearest x2 in front does
    # (four parity convolutions into one landing), and is refused before anything runs
    out = nans(B, 3, 2 * H, 2 * W)
    with pytest.raises(RuntimeError, match="folded upsample conv is NHWC"):
        _lib.check(lib.dm_op_vae_conv(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), B, H, W, C, 3, 3, 1, 1, 0, 1, 0, 1,
                                      None))
    assert torch.isnan(out).all()
    # null pointers
    out = nans(B, 3, H, W)
    for args in ((None, w, b, out), (x, None, b, out), (x, w, b, None)):
        with pytest.raises(RuntimeError, match="null argument"):
            _lib.check(lib.dm_op_vae_conv(*[_lib.ptr(t) for t in args], B, H, W, C, 3, 3, 1, 1, 0, 0, 0, 1, None))
    assert torch.isnan(out).all()
    assert lib.dm_op_vae_conv(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), 0, H, W, C, 3, 3, 1, 1, 0, 0, 0, 1, None) != 0
    assert lib.dm_op_vae_conv(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), B, 1, 1, C, 3, 3, 2, 0, 1, 0, 0, 1, None) != 0

    P = {n: dev(t) for n, t in res_params(C, C).items()}
    nin = {n: dev(t) for n, t in res_params(32, C).items() if n.startswith("nin")}
    out = nans(B, H, W, C)

    def res(params, cin, cout):
        return lib.dm_op_vae_resblock(_lib.ptr(x), *[_lib.ptr(params.get(n)) for n in RES_ORDER], _lib.ptr(out), B, H, W, cin,
                                      cout, None)

    with pytest.raises(RuntimeError, match="nin_shortcut"):
        _lib.check(res({**P, **nin}, C, C))                 # nin_shortcut given with cin == cout
    with pytest.raises(RuntimeError, match="nin_shortcut"):
        _lib.check(res(res_params_dev(32, C, drop=("ninw", "ninb")), 32, C))   # and missing with cin != cout
    with pytest.raises(RuntimeError, match="nin_shortcut"):
        _lib.check(res({**P, "ninw": nin["ninw"]}, C, C))   # one of the two
    with pytest.raises(RuntimeError, match="null argument"):
        _lib.check(res({**P, "n2b": None}, C, C))
    A = {n: dev(t) for n, t in attn_params(C).items()}
    with pytest.raises(RuntimeError, match="null argument"):
        _lib.check(lib.dm_op_vae_attn_block(_lib.ptr(x), *[_lib.ptr({**A, "kb": None}[n]) for n in ATTN_ORDER], _lib.ptr(out), B,
                                            H, W, C, None))
    with pytest.raises(RuntimeError, match="null argument"):
        _lib.check(lib.dm_op_vae_attn_block(None, *[_lib.ptr(A[n]) for n in ATTN_ORDER], _lib.ptr(out), B, H, W, C, None))
    assert torch.isnan(out).all()


def res_params_dev(cin, cout, drop=()):
    return {n: dev(t) for n, t in res_params(cin, cout).items() if n not in drop}


def test_every_form_got_its_cases():
    """Runs last: the cases above must have reached every form at least three times."""
    want = ["s2", "nchw_in", "nchw_out", "scalar", "thin", "up", "res", "res nin", "attn rows", "attn mfma"]
    print(f"{TAG}: " + ", ".join(f"{n} {COUNTS[n]}" for n in sorted(COUNTS)))
    total = len(CONV_RUNS)
    blocks = len(RES_CASES) + len(ATTN_CASES)
    ran = COUNTS["cases run"] + sum(COUNTS[n] for n in ("res", "res nin", "attn rows", "attn mfma"))
    if ran != total + blocks:
        pytest.skip(f"only {ran} of {total + blocks} cases were selected: the counts say nothing")
    short = {n: COUNTS[n] for n in want if COUNTS[n] < 3}
    assert not short, short
