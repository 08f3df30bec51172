"""GPU parity of the code AROUND the U-Net in a training step, one operator at a time through the C ABI: the Philox noise
stream and the dropout masks, the elementwise ops of q_sample / predict_* / the immiscible assignment, the DDPM loss kernel,
gradient clipping + Adam, the EMA lerp.  Each against a plain restatement at higher precision (numpy Philox from the paper,
torch fp64 on the CPU), at shapes the whole-model tests never produce: tails, sample boundaries inside a block, counters
with non-zero high words, more blocks than the grid-stride cap.

Limits come from the fp32 error of the same expression in numpy / torch against the fp64 reference, times 4 (another libm,
another summation order), computed here and printed next to the kernel's error; integer and contraction-free fp32
expressions are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_ref
from diffusion_models_amd import _lib

from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 5e-5
DEV = "cuda:0"
ULP1 = 2.0 ** -23


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=gen(seed)) * scale


def dev(t):
    return t.to(DEV).contiguous()


def fptr(t):
    """float* of a contiguous fp32 CPU tensor."""
    assert t.dtype == torch.float32 and t.is_contiguous()
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


# ---------------------------------------------------------------------------------------------------------------------
# 1. Philox
# ---------------------------------------------------------------------------------------------------------------------
RANDN_CASES = [
    # (seed, draw, element_offset, n)
    (0, 0, 0, 4096),
    (0x9E3779B97F4A7C15, 3, 0, 4096),            # seed with a non-zero high word
    (1234, (1 << 32) + 5, 0, 4096),              # draw >= 2^32
    (1234, 7, (1 << 34) + 8, 4096),              # element offset >= 2^34: idx4 >= 2^32
    (77, 1, 4 * 300, 4099),                      # n % 4 != 0, n % 1024 != 0
    (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF00000001, (1 << 36) - 4, 1030),  # idx4 carries from the low word into the high one
]


def _box_muller(c):
    """(fp64 reference, the same formula in numpy fp32) of the kernel's transform of (N, 4) Philox words: uniforms with the
    kernel's own fp32 roundings, Box-Muller evaluated in fp64 / fp32."""
    f32 = np.float32
    inv = f32(2.0 ** -32)
    u1 = np.minimum((c[:, 0::2].astype(f32) + f32(1.0)) * inv, f32(1.0))   # (0, 1]
    u2 = c[:, 1::2].astype(f32) * inv
    ang = f32(6.2831853) * u2
    assert u1.dtype == f32 and ang.dtype == f32
    out = []
    for t in (np.float64, np.float32):
        rad = np.sqrt(t(-2.0) * np.log(u1.astype(t)))
        z = np.stack([rad * np.cos(ang.astype(t)), rad * np.sin(ang.astype(t))], axis=2)  # (N, pair, cos / sin)
        assert z.dtype == t
        out.append(z.reshape(c.shape[0], 4))
    return out


@pytest.mark.parametrize("case", RANDN_CASES)
def test_randn_is_philox4x32_10_box_muller(case):
    seed, draw, off, n = case
    lib = _lib.load()
    z = torch.full((n + 8,), 7.0, device=DEV)
    _lib.check(lib.dm_randn(_lib.ptr(z), n, seed, draw, off, None))
    torch.cuda.synchronize()
    z = z.cpu().numpy()
    assert np.all(z[n:] == 7.0), "wrote past n"
    words = philox_ref.stream(seed, draw, off // 4, (n + 3) // 4)
    z64, z32 = (a.reshape(-1)[:n] for a in _box_muller(words))
    limit = 4 * float(np.abs(z32 - z64).max())
    err = float(np.abs(z[:n] - z64).max())
    print(f"dm_randn {case}: kernel {err:.3e} limit {limit:.3e} (numpy fp32 {limit / 4:.3e}), max |z| {np.abs(z64).max():.2f}")
    assert err <= limit, (err, limit)


def test_randn_reference_fp32_error_over_2_16_counters():
    """The figure DESIGN.md quotes: kernel and numpy-fp32 error over 2^16 counters (2^18 normals)."""
    lib = _lib.load()
    n = 4 << 16
    z = torch.empty((n,), device=DEV)
    _lib.check(lib.dm_randn(_lib.ptr(z), n, 2024, 0, 0, None))
    torch.cuda.synchronize()
    z64, z32 = (a.reshape(-1) for a in _box_muller(philox_ref.stream(2024, 0, 0, n // 4)))
    limit = 4 * float(np.abs(z32 - z64).max())
    err = float(np.abs(z.cpu().numpy() - z64).max())
    print(f"dm_randn 2^16 counters: kernel {err:.3e} limit {limit:.3e} (numpy fp32 {limit / 4:.3e}), max |z| {np.abs(z64).max():.2f}")
    assert err <= limit, (err, limit)


DROPOUT_KEYS = [
    # (seed, call, block_index)
    (0, 0, 0),
    (0xDEADBEEF12345678, 3, 17),        # seed with a non-zero high word
    (42, (1 << 16) + 5, 2),             # call << 16 reaches the high counter word
    (0x8000000000000001, (1 << 40) | 9, 0),  # the call numbers of the gradient-free self-conditioning pass
]


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("key", DROPOUT_KEYS)
def test_dropout_mask_is_the_same_philox(key, p):
    seed, call, blk = key
    lib = _lib.load()
    f32 = np.float32
    for n in (420, 4 * 256 * 3 + 40):  # a partly filled 256-thread block; several blocks and a tail
        m = torch.full((n + 4,), 7.0, device=DEV)
        _lib.check(lib.dm_op_dropout_mask(_lib.ptr(m), n, p, C.c_uint64(seed), C.c_uint64(call), blk, None))
        torch.cuda.synchronize()
        m = m.cpu().numpy()
        assert np.all(m[n:] == 7.0), "wrote past n"
        words = philox_ref.stream(seed, ((call << 16) | (blk + 1)) & 0xFFFFFFFFFFFFFFFF, 0, n // 4).reshape(-1)
        u = words.astype(f32) * f32(2.0 ** -32)
        want = np.where(u >= f32(p), f32(1.0) / (f32(1.0) - f32(p)), f32(0.0)).astype(f32)
        diff = int((m[:n].view(np.int32) != want.view(np.int32)).sum())
        print(f"dropout_mask key {key} p {p} n {n}: {diff} differing elements (limit 0), kept {float((want > 0).mean()):.3f}")
        assert diff == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. Elementwise ops of the training step: bit-exact against the same expression tree in torch fp32
# ---------------------------------------------------------------------------------------------------------------------
PER = 3 * 5 * 7  # sample boundaries fall inside a 256-thread block; B * PER is no multiple of 256


def _bits_differ(a, b):
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


@pytest.mark.parametrize("B", [1, 5])
def test_q_sample_bit_exact(B):
    lib = _lib.load()
    x, nz = randn((B, PER), 1), randn((B, PER), 2)
    coef = torch.zeros((B, 12))
    coef[:, 0] = torch.rand(B, generator=gen(3))
    coef[:, 1] = (1 - coef[:, 0] ** 2).sqrt()
    coef[:, 2:] = randn((B, 10), 4)  # the other columns must not matter
    out = torch.full((B * PER + 3,), 7.0, device=DEV)
    xd, nd = dev(x), dev(nz)  # named: a temporary would be freed, and its memory reused, before the call
    _lib.check(lib.dm_op_q_sample(_lib.ptr(xd), _lib.ptr(nd), fptr(coef), _lib.ptr(out), B, PER, None))
    want = coef[:, 0:1] * x + coef[:, 1:2] * nz
    got = out.cpu()
    d = _bits_differ(got[: B * PER].reshape(B, PER), want)
    print(f"q_sample B {B}: {d} differing elements (limit 0)")
    assert d == 0 and bool((got[B * PER:] == 7.0).all())


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("clamp", [0, 1])
def test_lincomb_bit_exact(B, mode, clamp):
    lib = _lib.load()
    x, y = randn((B, PER), 5, 1.5), randn((B, PER), 6, 1.5)
    coef = 0.25 + torch.rand((B, 2), generator=gen(7)) * 2
    coef[0] = 0.5  # sample 0: (0.5, 0.5), so that the values below land exactly on +-1 or just past them
    if mode == 0:   # 0.5 x + 0.5 y
        x[0, :6] = torch.tensor([1.0, -1.0, 1.5, -1.5, 1.0 + ULP1, -1.0 - ULP1])
        y[0, :6] = x[0, :6]
    else:           # (0.5 x - y) / 0.5
        x[0, :6] = torch.tensor([4.0, 2.0, 4.0, 2.0, 4.0, 2.0])
        y[0, :6] = torch.tensor([1.5, 1.5, 1.25, 1.75, 1.5 - ULP1, 1.5 + ULP1])
    out = torch.full((B * PER + 3,), 7.0, device=DEV)
    xd, yd = dev(x), dev(y)
    _lib.check(lib.dm_op_lincomb(_lib.ptr(xd), _lib.ptr(yd), fptr(coef), _lib.ptr(out), B, PER, mode, clamp, None))
    c0, c1 = coef[:, 0:1], coef[:, 1:2]
    want = c0 * x + c1 * y if mode == 0 else (c0 * x - y) / c1
    assert want[0, 0] == 1.0 and want[0, 1] == -1.0 and want[0, 2] > 1.0 and want[0, 3] < -1.0
    assert (want[0, 4] > 1.0 and want[0, 5] < -1.0) if mode == 0 else (want[0, 4] > 1.0 and want[0, 5] < 1.0)
    if clamp:
        want = want.clamp(-1.0, 1.0)
    got = out.cpu()
    d = _bits_differ(got[: B * PER].reshape(B, PER), want)
    print(f"lincomb B {B} mode {mode} clamp {clamp}: {d} differing elements (limit 0)")
    assert d == 0 and bool((got[B * PER:] == 7.0).all())


@pytest.mark.parametrize("B", [1, 5])
def test_mask_mix_bit_exact(B):
    lib = _lib.load()
    n = B * PER
    a, b = randn((n,), 8), randn((n,), 9)
    mask = torch.rand((n,), generator=gen(10))
    mask[::7] = 0.0
    mask[3::7] = 1.0
    out = torch.full((n + 3,), 7.0, device=DEV)
    ad, bd, md = dev(a), dev(b), dev(mask)
    _lib.check(lib.dm_op_mask_mix(_lib.ptr(ad), _lib.ptr(bd), _lib.ptr(md), _lib.ptr(out), n, None))
    want = a * mask + b * (1.0 - mask)
    got = out.cpu()
    d = _bits_differ(got[:n], want)
    print(f"mask_mix n {n}: {d} differing elements (limit 0)")
    assert d == 0 and bool((got[n:] == 7.0).all())


def test_offset_noise_bit_exact():
    lib = _lib.load()
    BC, HW = 7, 35
    noise, offset = randn((BC, HW), 11), randn((BC,), 12)
    buf = torch.full((BC * HW + 3,), 7.0, device=DEV)
    buf[: BC * HW] = dev(noise).reshape(-1)
    od = dev(offset)
    _lib.check(lib.dm_op_offset_noise(_lib.ptr(buf), _lib.ptr(od), 0.1, BC, HW, None))
    want = noise + torch.tensor(0.1, dtype=torch.float32) * offset[:, None]
    got = buf.cpu()
    d = _bits_differ(got[: BC * HW].reshape(BC, HW), want)
    print(f"offset_noise: {d} differing elements (limit 0)")
    assert d == 0 and bool((got[BC * HW:] == 7.0).all())


@pytest.mark.parametrize("D", [1, 255, 257, 3 * 16 * 16 + 1])
def test_cdist_vs_fp64(D):
    """Against torch.cdist in fp64.  Rows 1 / 2 are identical (distance exactly 0); rows 3 / 4 sit at +1000 with unit-scale
    differences, which |x|^2 + |y|^2 - 2 x.y would lose in fp32."""
    lib = _lib.load()
    n, m = 5, 7
    x, y = randn((n, D), 13), randn((m, D), 14)
    y[2] = x[1]
    x[3] += 1000.0
    y[4] += 1000.0
    out = torch.full((n * m + 3,), 7.0, device=DEV)
    xd, yd = dev(x), dev(y)
    _lib.check(lib.dm_op_cdist(_lib.ptr(xd), _lib.ptr(yd), _lib.ptr(out), n, m, D, None))
    got = out.cpu()
    ref = torch.cdist(x.double(), y.double(), compute_mode="donot_use_mm_for_euclid_dist")
    direct = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1).sqrt()
    assert direct.dtype == torch.float32
    limit = 4 * float((direct.double() - ref).abs().max())
    err = float((got[: n * m].reshape(n, m).double() - ref).abs().max())
    print(f"cdist D {D}: kernel {err:.3e} limit {limit:.3e} (torch fp32 direct {limit / 4:.3e}), 1000-offset pair {float(ref[3, 4]):.4f}")
    assert float(got[1 * m + 2]) == 0.0 and float(ref[1, 2]) == 0.0
    assert err <= limit and bool((got[n * m:] == 7.0).all())


def test_gather_rows():
    lib = _lib.load()
    n, D = 6, PER
    src = randn((n, D), 15)
    sd = dev(src)
    for idx in ([3, 0, 5, 1, 4, 2], list(range(n)), [2, 2, 0, 5, 2, 5]):
        dst = torch.full((n * D + 3,), 7.0, device=DEV)
        _lib.check(lib.dm_op_gather_rows(_lib.ptr(sd), (C.c_int64 * n)(*idx), _lib.ptr(dst), n, D, None))
        torch.cuda.synchronize()
        got = dst.cpu()
        d = _bits_differ(got[: n * D].reshape(n, D), src[idx])
        print(f"gather_rows {idx}: {d} differing elements (limit 0)")
        assert d == 0 and bool((got[n * D:] == 7.0).all())
    dst = torch.empty((n, D), device=DEV)
    for bad in ([0, 1, 2, 3, 4, n], [0, -1, 2, 3, 4, 5]):
        with pytest.raises(RuntimeError, match="out of range"):
            _lib.check(lib.dm_op_gather_rows(_lib.ptr(sd), (C.c_int64 * n)(*bad), _lib.ptr(dst), n, D, None))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 3. The DDPM loss kernel
# ---------------------------------------------------------------------------------------------------------------------
def _schedule_rows(t):
    """The 12 per-sample scalars of the loss kernel (rows as dm_train_args documents them) for timesteps t of a 1000-step
    linear schedule, from the DDPM definitions in fp64, rounded to fp32 as the reference's registered buffers are."""
    betas = torch.linspace(1e-4, 0.02, 1000, dtype=torch.float64)
    ac = torch.cumprod(1 - betas, 0)
    ac_prev = torch.cat([torch.ones(1, dtype=torch.float64), ac[:-1]])
    pv = betas * (1 - ac_prev) / (1 - ac)
    snr = ac / (1 - ac)
    tab = torch.zeros((1000, 12), dtype=torch.float64)
    tab[:, 0], tab[:, 1] = ac.sqrt(), (1 - ac).sqrt()
    tab[:, 2] = snr.clamp(max=5.0) / snr  # min-SNR weights: not all 1
    tab[:, 3] = (torch.arange(1000) > 0).double()
    tab[:, 4], tab[:, 5] = (1 / ac).sqrt(), (1 / ac - 1).sqrt()
    tab[:, 8] = betas * ac_prev.sqrt() / (1 - ac)
    tab[:, 9] = (1 - ac_prev) * (1 - betas).sqrt() / (1 - ac)
    tab[:, 10] = pv
    tab[:, 11] = pv.clamp(min=1e-20).log()
    return tab[torch.as_tensor(t)].float().contiguous()


def _pred_x_start(o, xq, c, objective):
    if objective == 0:
        return c[:, 4:5] * xq - c[:, 5:6] * o
    if objective == 1:
        return o
    return c[:, 0:1] * xq - c[:, 1:2] * o


def _loss_ref(out, x_start, noise, xq, coef, objective, terms, loss_scale, kl_weight, dtype):
    """p_losses after the U-Net, as the comment above mse_loss_kernel states it, in torch autograd at `dtype`.
    Returns loss, d loss / d out, the per-sample weighted MSE and masked KL means, pred_x_start."""
    o = out.detach().to(dtype).clone().requires_grad_(True)
    xs, nz, xq, c = x_start.to(dtype), noise.to(dtype), xq.to(dtype), coef.to(dtype)
    tgt = nz if objective == 0 else xs if objective == 1 else c[:, 0:1] * nz - c[:, 1:2] * xs
    part = ((o - tgt) ** 2).mean(1) * c[:, 2]
    total = part.mean() if terms & 1 else torch.zeros((), dtype=dtype)
    x0 = _pred_x_start(o, xq, c, objective)
    mm = c[:, 8:9] * x0.clamp(-1.0, 1.0) + c[:, 9:10] * xq
    pm = c[:, 8:9] * xs + c[:, 9:10] * xq
    mlv = c[:, 11:12].expand_as(o)
    kl = 0.5 * (mlv - mlv + (mlv.exp() + (mm - pm) ** 2) / c[:, 10:11] - 1.0)
    klpart = kl.mean(1) * c[:, 3]
    if terms & 2:
        total = total + kl_weight * klpart.sum() / (c[:, 3].sum() + 1e-8)
    total = total * loss_scale
    total.backward()
    return total.detach(), o.grad, part.detach(), klpart.detach(), x0.detach()


def _run_loss(out, x_start, noise, xq, coef, objective, terms, loss_scale, kl_weight):
    lib = _lib.load()
    B, per = out.shape
    dout = torch.full((B * per + 3,), 7.0, device=DEV)
    part, klpart = torch.full((B,), 7.0, device=DEV), torch.full((B,), 7.0, device=DEV)
    loss = C.c_float(0.0)
    ins = [dev(t) for t in (out, x_start, noise, xq)]
    _lib.check(lib.dm_op_mse_loss(*[_lib.ptr(t) for t in ins],
                                  fptr(coef), objective, terms, loss_scale, kl_weight, _lib.ptr(dout), C.byref(loss),
                                  _lib.ptr(part), _lib.ptr(klpart), B, per, None))
    dout = dout.cpu()
    assert bool((dout[B * per:] == 7.0).all()), "wrote past the end"
    return torch.tensor(loss.value), dout[: B * per].reshape(B, per), part.cpu(), klpart.cpu()


def _loss_errors(got, ref):
    """loss: relative; dout: the worst per-sample rel-L2 (one sample's large KL gradient must not hide another's);
    part / klpart (when given): worst error against the largest entry -- they are summed into the loss, and the KL mean of a
    late timestep is (1 + d) - 1 with d ~ 1e-7, noise in any fp32 evaluation."""
    e = {"loss": float((got[0].double() - ref[0].double()).abs() / ref[0].double().abs())}
    e["dout"] = max(rel_l2(got[1][b], ref[1][b]) for b in range(got[1].shape[0]))
    for k, name in ((2, "part"), (3, "klpart")):
        if got[k] is not None:
            e[name] = float((got[k].double() - ref[k].double()).abs().max() / ref[k].double().abs().max())
    return e


def _loss_inputs(B):
    t = [250] if B == 1 else [1, 10, 250, 600, 999]
    coef = _schedule_rows(t)
    x_start, noise = randn((B, PER), 20).clamp(-1, 1), randn((B, PER), 21)
    xq = coef[:, 0:1] * x_start + coef[:, 1:2] * noise
    return coef, x_start, noise, xq


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("objective", [0, 1, 2])
def test_mse_loss_vs_fp64_autograd(B, objective):
    coef, x_start, noise, xq = _loss_inputs(B)
    tgt = noise if objective == 0 else x_start if objective == 1 else coef[:, 0:1] * noise - coef[:, 1:2] * x_start
    out = tgt + randn((B, PER), 22, 0.3)  # a model that is roughly right: pred_x_start lands on both sides of +-1
    for terms in (1, 2, 3):
        for loss_scale in (1.0, 0.5):
            ref = _loss_ref(out, x_start, noise, xq, coef, objective, terms, loss_scale, 0.001, torch.float64)
            r32 = _loss_ref(out, x_start, noise, xq, coef, objective, terms, loss_scale, 0.001, torch.float32)
            got = _run_loss(out, x_start, noise, xq, coef, objective, terms, loss_scale, 0.001)
            # elements whose fp64 pred_x_start is within 8 fp32 ulps of +-1 may be clamped differently in fp32
            near = ((ref[4].abs() - 1.0).abs() < 8 * ULP1)
            assert float(near.double().mean()) < 0.01
            keep = ~near
            e32 = _loss_errors((r32[0], r32[1] * keep, r32[2], r32[3]), (ref[0], ref[1] * keep, ref[2], ref[3]))
            err = _loss_errors((got[0], got[1] * keep, got[2], got[3]), (ref[0], ref[1] * keep, ref[2], ref[3]))
            if not terms & 1:
                assert bool((got[2] == 0).all())
                err.pop("part")
            if not terms & 2:
                err.pop("klpart")
            limit = {k: max(4 * e32.get(k, 0.0), TOL) for k in err}
            print(f"mse_loss B {B} objective {objective} terms {terms} scale {loss_scale}: kernel {err} limit {limit} torch fp32 {e32}")
            assert all(err[k] <= limit[k] for k in err), (err, limit)
            inside = (ref[4].abs() <= 1.0)
            if terms & 2:
                assert 0.02 < float(inside.double().mean()) < 0.98  # both branches of the clamp are exercised


@pytest.mark.parametrize("objective", [0, 1, 2])
def test_mse_loss_kl_gradient_at_the_clamp_edges(objective):
    """Model outputs chosen so that pred_x_start lands a few ulps on either side of +-1: the KL gradient is exactly zero
    outside the closed interval [-1, 1] and non-zero inside (clamp_ passes the gradient on the closed interval)."""
    B = 5
    coef = _schedule_rows([100, 200, 300, 400, 500])
    x_start = randn((B, PER), 30).clamp(-0.9, 0.9)
    noise = randn((B, PER), 31)
    xq = randn((B, PER), 32, 0.1)  # small: c * xq rounds far below one ulp of 1
    steps = torch.tensor([10, 12, 16, 24, 32, -10, -12, -16, -24, -32], dtype=torch.float64)
    target = (1.0 + steps * ULP1).repeat(PER * B // 10 + 1)[: B * PER].reshape(B, PER)
    target = target * torch.where(torch.rand((B, PER), generator=gen(33)) < 0.5, -1.0, 1.0).double()
    c = coef.double()
    if objective == 0:
        out = (c[:, 4:5] * xq.double() - target) / c[:, 5:6]
    elif objective == 1:
        out = target.clone()
        # exact in both precisions: the ends of the closed interval and their neighbours
        out[0, :6] = torch.tensor([1.0, -1.0, 1.0 + ULP1, -1.0 - ULP1, 1.0 - ULP1 / 2, -1.0 + ULP1 / 2], dtype=torch.float64)
    else:
        out = (c[:, 0:1] * xq.double() - target) / c[:, 1:2]
    out = out.float()
    for terms in (2, 3):
        ref = _loss_ref(out, x_start, noise, xq, coef, objective, terms, 1.0, 0.001, torch.float64)
        r32 = _loss_ref(out, x_start, noise, xq, coef, objective, terms, 1.0, 0.001, torch.float32)
        got = _run_loss(out, x_start, noise, xq, coef, objective, terms, 1.0, 0.001)
        x0 = ref[4]
        near = (x0.abs() - 1.0).abs() < 8 * ULP1
        if objective == 1:
            near[0, :6] = False  # pred_x_start is the output itself: nothing is rounded
        share = float(near.double().mean())
        keep = ~near
        inside = (x0.abs() <= 1.0)
        assert share < 0.01 and 0.3 < float(inside.double().mean()) < 0.7, share
        assert float((x0.abs() - 1.0).abs().max()) < 64 * ULP1  # every element sits within a few ulps of an edge
        if terms == 2:
            g = got[1]
            assert bool((g[keep & ~inside] == 0).all()) and bool((ref[1][~inside] == 0).all())
            assert bool((g[keep & inside] != 0).all()) and bool((ref[1][inside] != 0).all())
        e32 = _loss_errors((r32[0], r32[1] * keep, r32[2], r32[3]), (ref[0], ref[1] * keep, ref[2], ref[3]))
        err = _loss_errors((got[0], got[1] * keep, got[2], got[3]), (ref[0], ref[1] * keep, ref[2], ref[3]))
        if terms == 2:
            err.pop("part")
        limit = {k: max(4 * e32.get(k, 0.0), TOL) for k in err}
        print(f"mse_loss clamp edges objective {objective} terms {terms}: kernel {err} limit {limit}, masked share {share:.4f} (limit 0.01)")
        assert all(err[k] <= limit[k] for k in err), (err, limit)


def test_mse_loss_t0_is_nan_as_in_the_reference():
    """A t = 0 sample with the KL term: posterior_variance[0] = 0 is divided by before the mask multiplies (inf * 0).  The
    reference's loss is NaN and so is the gradient of that sample wherever pred_x_start is inside the clamp; the NaN pattern
    and every finite value have to agree."""
    B = 5
    coef = _schedule_rows([0, 10, 250, 600, 999])
    assert coef[0, 10] == 0.0 and coef[0, 3] == 0.0
    x_start, noise = randn((B, PER), 40).clamp(-1, 1), randn((B, PER), 41)
    xq = coef[:, 0:1] * x_start + coef[:, 1:2] * noise
    out = noise + randn((B, PER), 42, 0.3)
    for terms in (2, 3):
        ref = _loss_ref(out, x_start, noise, xq, coef, 0, terms, 1.0, 0.001, torch.float64)
        r32 = _loss_ref(out, x_start, noise, xq, coef, 0, terms, 1.0, 0.001, torch.float32)
        got = _run_loss(out, x_start, noise, xq, coef, 0, terms, 1.0, 0.001)
        inside0 = ref[4][0].abs() <= 1.0  # clamp's backward selects: outside the interval the KL gradient is 0, not NaN
        assert 0.1 < float(inside0.double().mean()) < 0.9
        assert bool(ref[0].isnan()) and torch.equal(ref[1][0].isnan(), inside0) and not bool(ref[1][1:].isnan().any())
        nan_diff = int((got[1].isnan() != ref[1].isnan()).sum())
        err = max(rel_l2(got[1][b], ref[1][b]) for b in range(1, B))
        # mm - pm cancels to ~1e-4 of its terms at t = 999: the fp32 expression itself is only good to ~1e-3 there
        limit = max(4 * max(rel_l2(r32[1][b], ref[1][b]) for b in range(1, B)), TOL)
        print(f"mse_loss t=0 terms {terms}: loss {float(got[0])}, NaN pattern differs at {nan_diff} elements (limit 0), "
              f"finite samples' dout rel-L2 {err:.3e} limit {limit:.3e} (torch fp32 {limit / 4:.3e})")
        fin = ~ref[1][0].isnan()
        err0 = rel_l2(got[1][0][fin], ref[1][0][fin]) if terms & 1 else float(got[1][0][fin].abs().max())
        assert bool(got[0].isnan()) and nan_diff == 0 and err <= limit and err0 <= TOL, (nan_diff, err, err0)
        assert bool(got[3][0].isnan()) and bool(ref[3][0].isnan())


def test_mse_loss_kl_factor_is_the_one_training_passes():
    """dm_op_mse_loss forms kl_weight / (n_pos + 1e-8) in C; the training call receives the factor from
    diffusion.hybrid_kl_scale.  With the KL term alone and loss_scale 1 the loss is the single fp32 product of that factor
    and the in-order fp32 sum of klpart, so the two formulas are compared bit for bit.  Rows with t = 0 carry the mask of
    t = 0 on the scalars of a later timestep (at t = 0 itself the loss is NaN, see above)."""
    from diffusion_models_amd.diffusion import hybrid_kl_scale
    for t in ([250], [1, 10, 250, 600, 999], [7, 0, 250, 0, 999], [0, 0, 0, 40, 0]):
        B = len(t)
        coef = _schedule_rows([v if v > 0 else 500 for v in t])
        coef[:, 3] = (torch.tensor(t) > 0).float()
        x_start, noise = randn((B, PER), 50).clamp(-1, 1), randn((B, PER), 51)
        xq = coef[:, 0:1] * x_start + coef[:, 1:2] * noise
        got = _run_loss(noise + randn((B, PER), 52, 0.3), x_start, noise, xq, coef, 0, 2, 1.0, 0.001)
        k = np.float32(0.0)
        for b in range(B):
            k = np.float32(k + got[3][b].numpy())
        want = np.float32(hybrid_kl_scale(torch.tensor(t))) * k
        assert want.dtype == np.float32 and np.isfinite(want) and want != 0
        print(f"mse_loss KL factor t {t}: loss {float(got[0])!r}, diffusion.hybrid_kl_scale x sum(klpart) {float(want)!r} (limit: equal)")
        assert np.float32(got[0].item()).tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 4. Clip + Adam, EMA
# ---------------------------------------------------------------------------------------------------------------------
LR, EPS = 1e-3, 1e-8


def _adam_inputs(n, step, scale_to, seed, zero_block=False):
    """|g| log-uniform in [1e-3, 1] with random signs (sqrt(v) well conditioned), scaled so that the norm is `scale_to`
    when given; m, v of a run in progress (same sign as g: no cancellation in the moments) unless step == 1; p zero on the
    first half -- there (p_new - p_old) / lr is the update itself, not the update rounded to an ulp of p."""
    gn = gen(seed)
    g = 10.0 ** (-3.0 * torch.rand((n,), generator=gn, dtype=torch.float64))
    g = g * torch.where(torch.rand((n,), generator=gn) < 0.5, -1.0, 1.0).double()
    if scale_to is not None:
        g = g * (scale_to / g.norm())
    g = g.float()
    m = (g.double() * (0.5 + torch.rand((n,), generator=gn, dtype=torch.float64))).float()
    v = (g.double() ** 2 * (0.5 + torch.rand((n,), generator=gn, dtype=torch.float64))).float()
    if step == 1:
        m.zero_()
        v.zero_()
    if zero_block:
        g[n // 4: n // 2] = 0.0
        g[3 * n // 4:] = 0.0
    p = randn((n,), seed + 1, 0.02)
    p[: (n + 1) // 2] = 0.0
    return p, g, m, v


def _torch_adam(p, g, m, v, step, betas, max_norm, dtype):
    """clip_grad_norm_ + torch.optim.Adam on the CPU at `dtype`, the optimiser's state preset to step - 1."""
    q = torch.nn.Parameter(p.to(dtype).clone())
    q.grad = g.to(dtype).clone()
    opt = torch.optim.Adam([q], lr=LR, betas=betas, eps=EPS)
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.to(dtype).clone(), "exp_avg_sq": v.to(dtype).clone()}
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_([q], max_norm)
    opt.step()
    st = opt.state[q]
    assert float(st["step"]) == step
    return q.detach(), st["exp_avg"], st["exp_avg_sq"]


def _hip_adam(p, g, m, v, step, betas, max_norm):
    lib = _lib.load()
    n = p.numel()
    bufs = [torch.full((n + 3,), 7.0, device=DEV) for _ in range(4)]
    for b, t in zip(bufs, (p, g, m, v)):
        b[:n] = t.to(DEV)
    nc = (C.c_float * 2)(0.0, 0.0)
    _lib.check(lib.dm_op_adam_step(*[_lib.ptr(b) for b in bufs], n, LR, betas[0], betas[1], EPS, step, max_norm, nc, None))
    out = [b.cpu() for b in bufs]
    assert all(bool((o[n:] == 7.0).all()) for o in out), "wrote past n"
    assert _bits_differ(out[1][:n], g) == 0, "the gradient buffer is an input"
    return out[0][:n], out[2][:n], out[3][:n], float(nc[0]), float(nc[1])


def _relerr(a, ref):
    """Worst elementwise relative error; where the reference is exactly 0 the value must be too."""
    a, ref = a.double(), ref.double()
    zero = ref == 0
    assert bool((a[zero] == 0).all()), "non-zero where the reference is exactly 0"
    if bool(zero.all()):
        return 0.0
    return float(((a - ref).abs()[~zero] / ref.abs()[~zero]).max())


def _adam_errors(new, old_p, ref, ref_old_p):
    """update = (p_new - p_old) / lr on the half with p_old == 0 and on the other half, m, v."""
    n = old_p.numel()
    h = (n + 1) // 2
    upd = (new[0].double() - old_p.double()) / LR
    rupd = (ref[0].double() - ref_old_p.double()) / LR
    e = {"update_p0": _relerr(upd[:h], rupd[:h]), "m": _relerr(new[1], ref[1]), "v": _relerr(new[2], ref[2])}
    if n > h:
        e["update"] = _relerr(upd[h:], rupd[h:])
    return e


CLIP_MODES = ["below", "above", "off"]


@pytest.mark.parametrize("n", [1, 3, 4, 1023, 4 * 256 * 1024 + 7])
@pytest.mark.parametrize("clip", CLIP_MODES)
def test_clip_adam_vs_fp64_torch(n, clip):
    """n: tail only, no tail, one partial block, and more than 1024 blocks of float4 so that the grid-stride loop of the norm
    kernel and its tail meet.  clip: norm 0.5 (coefficient exactly 1), norm 3 (clipped to 1), max_grad_norm = 0 (off).
    The kernel evaluates the step in double and rounds m, v and p once each, so each stored value is the float nearest to
    the fp64 reference: no fp32 evaluation, torch's included, is closer on any element, whatever the host's CPU kernels do."""
    scale_to, max_norm = {"below": (0.5, 1.0), "above": (3.0, 1.0), "off": (None, 0.0)}[clip]
    worst, worst32 = {}, {}
    for step in (1, 2, 1000):
        for betas in ((0.9, 0.99), (0.9, 0.999)):
            p, g, m, v = _adam_inputs(n, step, scale_to, 100 + step, zero_block=False)
            ref = _torch_adam(p, g, m, v, step, betas, max_norm, torch.float64)
            r32 = _torch_adam(p, g, m, v, step, betas, max_norm, torch.float32)
            got = _hip_adam(p, g, m, v, step, betas, max_norm)
            norm = float(g.double().norm())
            assert abs(got[3] - norm) <= 1e-6 * norm, (got[3], norm)
            if clip == "above":
                assert abs(got[4] - max_norm / (norm + 1e-6)) <= 1e-6 * got[4] and got[4] < 0.5
            else:
                assert got[4] == 1.0, got[4]
            err, e32 = _adam_errors(got, p, ref, p), _adam_errors(r32, p, ref, p)
            assert all(err[k] <= 4 * e32[k] for k in err), (step, betas, err, e32)
            for k in err:
                worst[k], worst32[k] = max(worst.get(k, 0.0), err[k]), max(worst32.get(k, 0.0), e32[k])
    print(f"clip+adam n {n} clip {clip}: kernel {worst} limit 4 x torch fp32 {worst32} (each case against its own limit)")


@pytest.mark.parametrize("step", [1, 2])
def test_adam_zero_gradient_block(step):
    """A block of exactly-zero gradients: at step 1 (m = v = 0) parameter and moments stay exactly as they were; later the
    moments decay (m * beta1, v * beta2) and the update follows the old moments."""
    n, betas = 1023, (0.9, 0.99)
    p, g, m, v = _adam_inputs(n, step, None, 300, zero_block=True)
    zero = g == 0
    assert 400 < int(zero.sum()) < 600
    ref = _torch_adam(p, g, m, v, step, betas, 1.0, torch.float64)
    r32 = _torch_adam(p, g, m, v, step, betas, 1.0, torch.float32)
    got = _hip_adam(p, g, m, v, step, betas, 1.0)
    if step == 1:
        assert torch.equal(got[0][zero], p[zero]) and bool((got[1][zero] == 0).all()) and bool((got[2][zero] == 0).all())
    else:
        assert rel_l2(got[1][zero], m[zero].double() * betas[0]) < 1e-6 and rel_l2(got[2][zero], v[zero].double() * betas[1]) < 1e-6
    err, e32 = _adam_errors(got, p, ref, p), _adam_errors(r32, p, ref, p)
    print(f"adam zero-gradient block step {step}: kernel {err} limit 4 x torch fp32 {e32}")
    assert all(err[k] <= 4 * e32[k] for k in err), (err, e32)


def test_clip_propagates_a_nan_gradient_and_zeroes_at_inf():
    """clip_grad_norm_ multiplies every gradient by max_norm / (norm + 1e-6): one NaN gradient makes that NaN and with it every
    parameter; one inf gradient makes it 0 (the clamp keeps 0), so only inf * 0 = NaN at that element."""
    n, betas = 1023, (0.9, 0.99)
    for bad in (float("nan"), float("inf")):
        p, g, m, v = _adam_inputs(n, 1, None, 400)
        g[517] = bad
        ref = _torch_adam(p, g, m, v, 1, betas, 1.0, torch.float64)
        got = _hip_adam(p, g, m, v, 1, betas, 1.0)
        nan_diff = [int((a.isnan() != b.isnan()).sum()) for a, b in zip(got[:3], ref)]
        print(f"clip with one {bad} gradient: norm {got[3]} coefficient {got[4]}, NaN pattern of p / m / v differs at {nan_diff} "
              f"elements (limit 0), reference NaN parameters {int(ref[0].isnan().sum())} of {n}")
        assert nan_diff == [0, 0, 0]
        if bad != bad:
            assert bool(ref[0].isnan().all()) and bool(got[0].isnan().all()) and got[3] != got[3] and got[4] != got[4]
        else:
            assert int(ref[0].isnan().sum()) == 1 and got[3] == float("inf") and got[4] == 0.0
            ok = ~ref[0].isnan()
            assert torch.equal(got[0][ok], p[ok]) and torch.equal(got[0][ok].double(), ref[0][ok])
    # without clipping a NaN stays where it is, in torch and here
    p, g, m, v = _adam_inputs(n, 1, None, 400)
    g[517] = float("nan")
    ref = _torch_adam(p, g, m, v, 1, betas, 0.0, torch.float64)
    got = _hip_adam(p, g, m, v, 1, betas, 0.0)
    assert int(got[0].isnan().sum()) == 1 and int(ref[0].isnan().sum()) == 1 and bool(got[0][517].isnan())


@pytest.mark.parametrize("decay", [0.5, 0.995, 0.9999])
@pytest.mark.parametrize("n", [3, 1025])
def test_ema_lerp_increment_vs_fp64(decay, n):
    """The increment ema_new - ema_old against e.lerp_(p, 1 - decay) in fp64.  |ema| is small against |p - ema| so that the
    rounding of ema_new to an ulp of ema stays below the error of the weight: 1.0f - 0.9999f is 1.7e-4 off."""
    lib = _lib.load()
    e, p = randn((n,), 50, 1e-3), randn((n,), 51)
    ref = e.double().clone().lerp_(p.double(), 1 - decay) - e.double()
    r32 = e.clone().lerp_(p, 1 - decay).double() - e.double()
    buf = torch.full((n + 3,), 7.0, device=DEV)
    buf[:n] = e.to(DEV)
    pd = dev(p)
    _lib.check(lib.dm_op_ema_lerp(_lib.ptr(buf), _lib.ptr(pd), n, decay, None))
    got = buf.cpu()
    scale = float(ref.abs().max())
    err = float((got[:n].double() - e.double() - ref).abs().max()) / scale
    limit = 4 * float((r32 - ref).abs().max()) / scale
    print(f"ema_lerp decay {decay} n {n}: kernel {err:.3e} limit {limit:.3e} (torch fp32 lerp_ {limit / 4:.3e}), of the largest increment")
    assert err <= limit and bool((got[n:] == 7.0).all())
