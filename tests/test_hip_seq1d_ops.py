"""GPU parity of the sequence model's operators, one at a time through the C ABI (dm_op_conv1d, dm_op_block1d, the two
attention layers with mem_kv = NULL, dm_op_sampler_update_ex), against fp64 on the CPU on the same fp32 inputs.

Asserted dispatch.  Every convolution case names in its table the kernel family it must reach (conv: the direct implicit
GEMM; pw: the 1x1 GEMM) and, where the case is about it, a K split; the call is bracketed with the library's profile rows
(detail mode) and the named row, with the layer's shape in it, must be there.  The plan functions are never asked.  The
Winograd F(4,3) kernel that was measured against the direct family lost at every layer and is not in the library
(experimental/wino1d_mfma.hip): the cases that were chosen to break it -- several sequences per tile group, a
partial last group, one K chunk, L % 4 != 0 -- stay, on the family that runs them.

Limits, as in tests/test_hip_conv_families.py.  Per tensor two metrics: whole-tensor rel-L2 and max|got - ref| / rms(ref).
The floor of each is the fp32 restatement of the operator (tests/conv1d_restate.py) measured against the fp64 reference
inside the test; the kernel may be 4 x the floor off.  The inputs are ``randn``, so rel-L2 must also stay under that file's
TOL_FWD = 2e-5.  Outputs are poisoned with NaN before the call, and run_op poisons the operator workspace.  Every case prints
``case: kernel error, floor, limit`` for both metrics before it asserts (run with -s).  The DDIM update is compared bit for
bit with a torch restatement of the reference's expression tree."""
import ctypes as C
import re

import pytest
import torch
import torch.nn.functional as F

import conv1d_restate as c1
from diffusion_models_amd import _lib

pytestmark = pytest.mark.gpu
TOL_FWD = 2e-5
FACTOR = 4.0
DEV = "cuda:0"
W1, W1K = "conv", "conv k>1"  # K = 3, C % 8 == 0, Cout % 64 == 0, L % 4 == 0: the shapes an F(4,3) family would take


def expected(exp):
    return exp.split()[0], "k>1" in exp


@pytest.fixture(scope="module", autouse=True)
def profiled():
    _lib.profile_enable(True, detail=True)
    _lib.profile_read()
    yield
    _lib.profile_read()
    _lib.profile_enable(False)


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def profiled_call(fn):
    _lib.profile_read()
    fn()
    return [r["kernel"] for r in _lib.profile_read()]


def metrics(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d = got - ref
    return (float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.pow(2).mean().sqrt().clamp_min(1e-300)))


def check(label, got, ref64, floor32):
    e, f = metrics(got, ref64), metrics(floor32, ref64)
    lim = (min(FACTOR * f[0], TOL_FWD), FACTOR * f[1])
    print(f"seq1d_ops {label}: rel-L2 kernel {e[0]:.3g} floor {f[0]:.3g} limit {lim[0]:.3g} | max/rms kernel {e[1]:.3g} "
          f"floor {f[1]:.3g} limit {lim[1]:.3g}")
    assert torch.isfinite(got).all(), (label, "not finite", int((~torch.isfinite(got)).sum()))
    assert e[0] <= lim[0] and e[1] <= lim[1], (label, e, lim)


def assert_row(label, rows, family, shape, split):
    prefix = {"conv": "conv<", "pw": "pw<"}[family]
    hits = [r for r in rows if r.startswith(prefix) and shape in r]
    assert hits, (label, f"no {family} row with '{shape}'", rows)
    if split:
        k = [int(m.group(1)) for r in hits for m in [re.search(r" k(\d+)", r)] if m]
        assert k and max(k) > 1, (label, "no K split", hits)


# ---- dm_op_conv1d ---------------------------------------------------------------------------------------------------------------
# (B, C0, C1, L, Cout, K, stride, pad, up2, bias, residual, family [k>1])
CONV_CASES = [
    # K = 3 blocks: tiles of several sequences share a workgroup, the last group is partial
    (3, 64, 0, 4, 64, 3, 1, 1, False, True, False, W1),
    (3, 64, 0, 12, 64, 3, 1, 1, False, True, True, W1),
    (3, 64, 0, 20, 64, 3, 1, 1, False, False, False, W1),
    (3, 64, 32, 12, 64, 3, 1, 1, False, True, False, W1),            # the skip concatenation, C0 != C1
    (3, 64, 64, 20, 128, 3, 1, 1, False, True, True, W1),            # two cout tiles
    (1, 512, 0, 4, 64, 3, 1, 1, False, True, False, W1K),            # K split
    (35, 8, 0, 8, 64, 3, 1, 1, False, True, True, W1),               # 70 tiles: two tile groups, the second partial; one chunk
    (2, 64, 0, 6, 64, 3, 1, 1, False, True, False, "conv"),          # L % 4 != 0: not an F(4,3) shape
    (2, 36, 0, 12, 64, 3, 1, 1, False, True, False, "conv"),         # a width no chunked family takes
    (3, 1, 0, 33, 32, 3, 1, 1, False, True, False, "conv"),          # odd length, one channel
    # Upsample: nearest x2 + K = 3 as one convolution with 2 Cout channels on the source grid
    (3, 64, 0, 12, 32, 3, 1, 1, True, True, False, W1),              # 64 doubled channels
    (2, 128, 0, 8, 64, 3, 1, 1, True, True, False, W1),
    (1, 8, 0, 1, 4, 3, 1, 1, True, False, False, "conv"),            # one position: both halves read only padding beside it
    # init_conv: K = 7 from (B, C, L) as stored
    (3, 1, 0, 20, 32, 7, 1, 3, False, True, False, "conv"),
    (2, 2, 0, 32, 64, 7, 1, 3, False, True, False, "conv"),
    (2, 3, 0, 5, 32, 7, 1, 3, False, False, False, "conv"),          # shorter than the kernel
    # Downsample: Conv1d(4, 2, 1)
    (3, 64, 0, 6, 128, 4, 2, 1, False, True, False, "conv"),
    (2, 32, 0, 16, 64, 4, 2, 1, False, True, False, "conv"),
    # K = 1: to_qkv / to_out / res_conv
    (3, 64, 0, 12, 384, 1, 1, 0, False, False, False, "pw"),
    (2, 64, 32, 20, 64, 1, 1, 0, False, True, True, "pw"),
    (2, 24, 0, 12, 40, 1, 1, 0, False, True, False, "conv"),
]


def conv_id(c):
    return f"B{c[0]}_{c[1]}+{c[2]}_L{c[3]}_{c[4]}_k{c[5]}s{c[6]}" + ("_up" if c[8] else "") + ("_res" if c[10] else "")


@pytest.mark.parametrize("case", CONV_CASES, ids=conv_id)
def test_conv1d(case):
    B, C0, C1, L, Cout, K, stride, pad, up2, bias, residual, exp = case
    family, split = expected(exp)
    Cin = C0 + C1
    x0, x1 = seeded((B, C0, L), 1), (seeded((B, C1, L), 2) if C1 else None)
    w = seeded((Cout, Cin, K), 3, (K * Cin) ** -0.5)
    b = seeded((Cout,), 4, 0.1) if bias else None
    Lo = 2 * L if up2 else (L + 2 * pad - K) // stride + 1
    r = seeded((B, Cout, Lo), 5) if residual else None
    x = x0 if x1 is None else torch.cat([x0, x1], dim=1)

    def ref(dt):
        xx, ww, bb = x.to(dt), w.to(dt), None if b is None else b.to(dt)
        if up2:  # fp64: the layer as the reference runs it; fp32: the packing the library runs, on the family's algorithm
            y = c1.upsample_reference(xx, ww, bb) if dt == torch.float64 else c1.upsample_conv(xx, ww, bb)
        else:
            y = F.conv1d(xx, ww, bb, stride=stride, padding=pad)
        return y if r is None else y + r.to(dt)

    out = nans(B, Cout, Lo)
    a = [dev(t) for t in (x0, x1, w, b, r)]
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_conv1d(
        _lib.ptr(a[0]), C0, _lib.ptr(a[1]), C1, _lib.ptr(a[2]), _lib.ptr(a[3]), _lib.ptr(a[4]), _lib.ptr(out), B, L, Cout, K,
        stride, pad, int(up2), None)))
    kc, ko = (3, 2 * Cout) if up2 else (K, Cout)
    shape = (f"1x1 {C0}+{C1}->{ko} @1x{Lo if not up2 else L}" if family == "pw"
             else f"1x{kc} s{stride} {C0}+{C1}->{ko} @1x{L if up2 else Lo}")
    assert_row(conv_id(case), rows, family, shape, split)
    check(conv_id(case), out.cpu(), ref(torch.float64), ref(torch.float32))


# ---- dm_op_block1d ----------------------------------------------------------------------------------------------------------------
# (B, C0, C1, L, Cout, scale-shift, residual, family)
BLOCK_CASES = [
    (3, 64, 0, 12, 64, True, False, W1),
    (3, 64, 0, 20, 64, False, True, W1),
    (3, 64, 32, 12, 64, True, True, W1),      # ResnetBlock.block1 of the up path
    (2, 128, 0, 4, 128, False, False, W1),    # two cout tiles under one RMSNorm
    (1, 512, 0, 4, 256, True, False, W1K),    # K split: the landing pass runs the epilogue
    (2, 36, 0, 9, 20, True, True, "conv"),
]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: f"B{c[0]}_{c[1]}+{c[2]}_L{c[3]}_{c[4]}_ss{int(c[5])}_res{int(c[6])}")
def test_block1d(case):
    B, C0, C1, L, Cout, ss, res, exp = case
    family, split = expected(exp)
    Cin = C0 + C1
    x0, x1 = seeded((B, C0, L), 11), (seeded((B, C1, L), 12) if C1 else None)
    w, b = seeded((Cout, Cin, 3), 13, (3 * Cin) ** -0.5), seeded((Cout,), 14, 0.1)
    g = 1 + 0.3 * seeded((Cout,), 15)
    scale, shift = (seeded((B, Cout), 16, 0.5), seeded((B, Cout), 17, 0.5)) if ss else (None, None)
    r = seeded((B, Cout, L), 18) if res else None
    x = x0 if x1 is None else torch.cat([x0, x1], dim=1)

    def ref(dt):
        cv = lambda t: None if t is None else t.to(dt)
        return c1.block(cv(x), cv(w), cv(b), cv(g), cv(scale), cv(shift), cv(r))

    out = nans(B, Cout, L)
    a = [dev(t) for t in (x0, x1, w, b, g, scale, shift, r)]
    rows = profiled_call(lambda: _lib.check(_lib.load().dm_op_block1d(
        _lib.ptr(a[0]), C0, _lib.ptr(a[1]), C1, *[_lib.ptr(t) for t in a[2:]], _lib.ptr(out), B, L, Cout, None)))
    assert_row(str(case), rows, family, f"1x3 s1 {C0}+{C1}->{Cout} @1x{L}", split)
    check(f"block1d {case[:7]} {family}", out.cpu(), ref(torch.float64), ref(torch.float32))


# ---- attention without memory key / values ---------------------------------------------------------------------------------------
def attn_weights(C_, heads, dh, full, seed):
    hid = heads * dh
    return dict(norm_g=1 + 0.3 * seeded((C_,), seed), w_qkv=seeded((3 * hid, C_, 1), seed + 1, C_ ** -0.5),
                w_out=seeded((C_, hid, 1), seed + 2, hid ** -0.5), b_out=seeded((C_,), seed + 3, 0.1),
                out_g=None if full else 1 + 0.3 * seeded((C_,), seed + 4))


@pytest.mark.parametrize("n", [3, 16, 320])
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("full", [False, True], ids=["linear", "full"])
def test_attention_without_memory(full, dh, n):
    B, C_, heads = 3, 64, 4 if dh == 32 else 2
    x = seeded((B, C_, n), 21)
    p = attn_weights(C_, heads, dh, full, 22)

    def ref(dt):
        q = {k: (None if v is None else v.to(dt)) for k, v in p.items()}
        if full:
            return c1.attention(x.to(dt), q["norm_g"], q["w_qkv"], q["w_out"], q["b_out"], heads, dh)
        return c1.linear_attention(x.to(dt), q["norm_g"], q["w_qkv"], q["w_out"], q["b_out"], q["out_g"], heads, dh)

    out = nans(B, C_, n)
    d = {k: dev(v) for k, v in p.items()}
    lib, xd = _lib.load(), dev(x)
    if full:
        call = lambda: _lib.check(lib.dm_op_attention(_lib.ptr(xd), _lib.ptr(d["norm_g"]), None, _lib.ptr(d["w_qkv"]),
                                                      _lib.ptr(d["w_out"]), _lib.ptr(d["b_out"]), _lib.ptr(out), B, C_, 1, n,
                                                      heads, dh, None))
    else:
        call = lambda: _lib.check(lib.dm_op_linear_attention(_lib.ptr(xd), _lib.ptr(d["norm_g"]), None, _lib.ptr(d["w_qkv"]),
                                                             _lib.ptr(d["w_out"]), _lib.ptr(d["b_out"]), _lib.ptr(d["out_g"]),
                                                             _lib.ptr(out), B, C_, 1, n, heads, dh, None))
    rows = profiled_call(call)
    if full:
        assert any(r.startswith("attention_core") and f"<{dh}>" in r for r in rows), rows
    else:  # the memory-free instantiation of the context kernel, never the fused kernels (they bake the memory rows in)
        assert any(r.startswith("linattn_ctx_mfma_kernel<") and r.endswith(f",{dh},0>") for r in rows), rows
        assert not any("fused" in r for r in rows), rows
    check(f"{'attention' if full else 'linear_attention'} dh{dh} n{n}", out.cpu(), ref(torch.float64), ref(torch.float32))


# ---- the DDIM update with its two switches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1, 2, 3], ids=["clamp_rederive", "noclamp_rederive", "clamp_raw", "noclamp_raw"])
def test_ddim_update_switches_bit_exact(flags):
    """flags 0 is the image classes' update (dm_op_sampler_update gives the same bits); DM_DDIM_NO_CLAMP (bit 1) leaves x_start
    as predicted, DM_DDIM_RAW_NOISE (bit 2) takes the model output as pred_noise under pred_noise
    (denoising_diffusion_1d.py:503-526 with clip_x_start = clip_denoised and no rederive_pred_noise, :577)."""
    n = 3 * 2 * 32 + 3  # not a multiple of 4
    x, eps, z = seeded((n,), 1), seeded((n,), 2, 3.0), seeded((n,), 3)
    lib = _lib.load()
    a = [dev(x), dev(eps), dev(z)]
    for obj in (0, 1, 2):
        for c in ([3.5, 3.4, 0.9, 0.43, 0.1, 1.0, 0.28, 0.96], [1.2, 0.6, 0, 0, 0, 0.0, 0.83, 0.55]):
            ct = torch.tensor(c, dtype=torch.float32)
            x0 = (ct[0] * x - ct[1] * eps, eps, ct[6] * x - ct[7] * eps)[obj]
            x0 = x0 if flags & 1 else x0.clamp(-1.0, 1.0)
            e2 = eps if (flags & 2 and obj == 0) else (ct[0] * x - x0) / ct[1]
            ref = (x0 * ct[2] + ct[3] * e2) + ct[4] * z if c[5] else x0
            out, xs = nans(n), nans(n)
            carr = (C.c_float * 8)(*c)
            _lib.check(lib.dm_op_sampler_update_ex(1, obj, flags, _lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), carr,
                                                   _lib.ptr(out), _lib.ptr(xs), n, None))
            assert torch.equal(out.cpu(), ref) and torch.equal(xs.cpu(), x0), (obj, flags, c)
            if flags == 0:
                out2 = nans(n)
                _lib.check(lib.dm_op_sampler_update(1, obj, _lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), carr,
                                                    _lib.ptr(out2), None, n, None))
                assert torch.equal(out2, out)
    # the switches belong to the DDIM update
    out = nans(n)
    carr = (C.c_float * 8)(*[1.0] * 8)
    assert lib.dm_op_sampler_update_ex(0, 0, 1, _lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), carr, _lib.ptr(out), None, n,
                                       None) != 0
    assert lib.dm_op_sampler_update_ex(1, 0, 4, _lib.ptr(a[0]), _lib.ptr(a[1]), _lib.ptr(a[2]), carr, _lib.ptr(out), None, n,
                                       None) != 0
