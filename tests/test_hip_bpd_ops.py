"""The bits-per-dim kernels on their own (csrc/bpd.hip through ``dm_op_bpd_terms`` / ``dm_op_bpd_step_in`` / ``dm_op_bpd_prior``)
against the fp64 restatement of tests/bpd_oracle.py on the same fp32 inputs.

Limit, per image and quantity: ``|got - want| <= max(4 x the fp32 restatement's own error, 2e-5) * |want|``, the rule of
test_hip_seq1d_ops.py.  Shapes: ``per`` = 4 (one vector), one chunk of the term kernel minus / plus one vector, the chunk
itself, and 3 * 16 * 16; B = 1 and 3.  An image evaluated alone gives the bits it gives inside a batch; the step-in kernel
gives the bits of ``q_sample``.  Measured errors are printed (run with -s to see them)."""
import ctypes as C
import math

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import bpd as Bp

import bpd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2e-5
CHUNK = _lib.DM_BPD_CHUNK
PERS = [4, CHUNK - 4, CHUNK, CHUNK + 4, 3 * 16 * 16]
NAMES = ("vb", "xstart_mse", "mse")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grid(shape, g, ends=0.0):
    """Normalised 8-bit images; ``ends``: the share of pixels set to exactly -1 and to exactly +1, in runs."""
    x = torch.randint(0, 256, shape, generator=g).float() / 255.0 * 2 - 1
    flat = x.reshape(shape[0], -1)
    n = int(flat.shape[1] * ends)
    if n:
        flat[:, :n] = -1.0
        flat[:, -n:] = 1.0
    return x


def _terms(mo, x0, x_t, z, row, learned, objective, clip):
    lib = _lib.load()
    B, per = x0.shape[0], x0[0].numel()
    out = (C.c_float * (3 * B))()
    dev = [t.to(DEV).contiguous() for t in (mo, x0, x_t, z)]
    _lib.check(lib.dm_op_bpd_terms(*[_lib.ptr(t) for t in dev], _lib.fptr(row.contiguous()), int(learned), objective, int(clip),
                                   out, B, per, None))
    return torch.tensor(list(out), dtype=torch.float32).reshape(B, 3)


def _check(tag, got, mo, x0, x_t, z, row, learned, objective, clip):
    want = O.terms(mo, x0, x_t, z, row, learned, objective, clip, torch.float64)
    w32 = O.terms(mo, x0, x_t, z, row, learned, objective, clip, torch.float32)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all())
    for b in range(got.shape[0]):
        for q, name in enumerate(NAMES):
            w = float(want[b, q])
            err = abs(float(got[b, q]) - w) / abs(w)
            e32 = abs(float(w32[b, q]) - w) / abs(w)
            lim = max(4 * e32, FLOOR)
            print(f"{tag} image {b} {name}: kernel {err:.3e} limit {lim:.3e} torch fp32 {e32:.3e} (value {w:.4g})")
            assert err <= lim, (tag, b, name, err, lim)


# ---- the decoder term --------------------------------------------------------------------------------------------------
def _decoder_case(B, per, seed):
    """A t == 0 row (coef1 = 1, coef2 = 0 as at t = 0) with min_log / max_log chosen so that sigma = exp(0.5 logvar) spans
    1/510 .. 1/64, and a model output whose mean is x0 + delta * sigma: delta uniform in (-2, 2), one run at 12 (on the
    clamp of log)."""
    g = _gen(seed)
    x0 = _grid((B, 1, 1, per), g, ends=0.1 if per >= 40 else 0.25)
    row = torch.zeros(Bp.COLS)
    row[Bp.RECIP], row[Bp.RECIPM1], row[Bp.COEF1], row[Bp.COEF2], row[Bp.T0] = 1.0, 1.0, 1.0, 0.0, 1.0
    row[Bp.SQRT_AC], row[Bp.SQRT_1M_AC] = 0.99, 0.14
    row[Bp.POST_LOG], row[Bp.MAX_LOG] = 2 * math.log(1 / 510), 2 * math.log(1 / 64)
    v = torch.rand((B, 1, 1, per), generator=g) * 2 - 1
    frac = (v + 1) * 0.5
    sigma = torch.exp(0.5 * (frac * row[Bp.MAX_LOG] + (1 - frac) * row[Bp.POST_LOG]))
    delta = torch.rand((B, 1, 1, per), generator=g) * 4 - 2
    n = max(per // 25, 1)
    delta[..., per // 2:per // 2 + n] = 12.0  # 4 % of the pixels
    z = torch.randn((B, 1, 1, per), generator=g)
    x_t = row[Bp.SQRT_AC] * x0 + row[Bp.SQRT_1M_AC] * z
    eps = x_t - (x0 + delta * sigma)  # x_start = 1 * x_t - 1 * eps = the mean
    return torch.cat((eps, v), dim=1), x0, x_t, z, row


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", PERS)
def test_decoder_term_vs_fp64(B, per):
    mo, x0, x_t, z, row = _decoder_case(B, per, 100 + per + B)
    want, term = O.terms(mo, x0, x_t, z, row, True, 0, False, torch.float64, parts=True)
    if per >= 40:  # all three branches and the clamp are hit
        share = [float((x0 < -0.999).float().mean()), float((x0 > 0.999).float().mean())]
        clamped = float((term >= -math.log(1e-15) - 1e-9).float().mean())
        print(f"decoder per={per} B={B}: branch shares low {share[0]:.3f} high {share[1]:.3f}, on the clamp {clamped:.3f}")
        assert min(share) >= 0.05 and 1 - sum(share) >= 0.5 and 0.01 <= clamped <= 0.10
    got = _terms(mo, x0, x_t, z, row, True, 0, False)
    _check(f"decoder per={per} B={B}", got, mo, x0, x_t, z, row, True, 0, False)


# ---- the KL term -------------------------------------------------------------------------------------------------------
def _kl_case(B, per, t, learned, seed, T=1000):
    g = _gen(seed)
    sched = dm.make_schedule(T, "linear")
    row = dm.bpd_step_table(sched, (t,))[1][0].contiguous()
    x0 = _grid((B, 1, 1, per), g)
    z = torch.randn((B, 1, 1, per), generator=g)
    x_t = row[Bp.SQRT_AC] * x0 + row[Bp.SQRT_1M_AC] * z
    mo = torch.randn((B, 2 if learned else 1, 1, per), generator=g)
    if learned:
        mo[:, 1:] *= 1.5  # the interpolation weight leaves [0, 1] on both sides
    return mo, x0, x_t, z, row


@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
@pytest.mark.parametrize("learned,objective", [(False, 0), (False, 1), (False, 2), (True, 0)],
                         ids=["pred_noise", "pred_x0", "pred_v", "learned"])
def test_kl_term_vs_fp64(learned, objective, clip):
    for t in (500, 1):
        mo, x0, x_t, z, row = _kl_case(3, 3 * 16 * 16, t, learned, 300 + 10 * objective + t + int(learned))
        assert float(row[Bp.T0]) == 0.0
        got = _terms(mo, x0, x_t, z, row, learned, objective, clip)
        _check(f"kl t={t} {'learned' if learned else 'fixed'} objective {objective} clip {clip}", got, mo, x0, x_t, z, row,
               learned, objective, clip)
    if clip:  # the flag reaches the kernel
        other = _terms(mo, x0, x_t, z, row, learned, objective, False)
        assert not torch.equal(other, got)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("per", PERS)
def test_kl_term_shapes_vs_fp64(B, per):
    for learned in (False, True):
        mo, x0, x_t, z, row = _kl_case(B, per, 37, learned, 500 + per + B)
        got = _terms(mo, x0, x_t, z, row, learned, 0, True)
        _check(f"kl per={per} B={B} {'learned' if learned else 'fixed'}", got, mo, x0, x_t, z, row, learned, 0, True)


def test_real_t0_row_fixed_variance_vs_fp64():
    """The row of t = 0 as the schedule has it, with the fixed variance log(1e-20): the decoder term of DenoisingDiffusion."""
    g = _gen(7)
    row = dm.bpd_step_table(dm.make_schedule(1000, "linear"), (0,))[1][0].contiguous()
    assert float(row[Bp.T0]) == 1.0
    x0 = _grid((2, 1, 1, 768), g, ends=0.1)
    z = torch.randn(x0.shape, generator=g)
    x_t = row[Bp.SQRT_AC] * x0 + row[Bp.SQRT_1M_AC] * z
    mo = z + 5.0 * torch.randn(x0.shape, generator=g)  # x_start = x0 + 0.05 r: inside the pixel's bin for 6 % of the pixels
    got = _terms(mo, x0, x_t, z, row, False, 0, True)
    _check("t = 0 row, fixed variance", got, mo, x0, x_t, z, row, False, 0, True)


# ---- by image ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [CHUNK + 4, 3 * 16 * 16])
def test_an_image_alone_gives_the_bits_it_gives_in_a_batch(per):
    for case in (_decoder_case(3, per, 900 + per), _kl_case(3, per, 500, True, 901 + per), _kl_case(3, per, 1, False, 902 + per)):
        mo, x0, x_t, z, row = case
        learned = mo.shape[1] == 2
        whole = _terms(mo, x0, x_t, z, row, learned, 0, False)
        for b in range(3):
            alone = _terms(mo[b:b + 1], x0[b:b + 1], x_t[b:b + 1], z[b:b + 1], row, learned, 0, False)
            assert torch.equal(alone[0], whole[b]), (per, b)


# ---- step-in and prior -------------------------------------------------------------------------------------------------
def _step_in(x0, z, row, seed=0, draw=1, off=0):
    lib = _lib.load()
    B, per = x0.shape[0], x0[0].numel()
    xd = x0.to(DEV).contiguous()
    zd = z.to(DEV).contiguous() if z is not None else None
    out = torch.full_like(xd, float("nan"))
    _lib.check(lib.dm_op_bpd_step_in(_lib.ptr(xd), _lib.ptr(zd), _lib.fptr(row.contiguous()), seed, draw, off, _lib.ptr(out), B,
                                     per, None))
    return out.cpu()


@pytest.mark.parametrize("B,per", [(1, 4), (3, CHUNK + 4), (3, 768)])
def test_step_in_is_q_sample_bit_for_bit(B, per):
    lib = _lib.load()
    sched = dm.make_schedule(1000, "linear")
    g = _gen(40 + per)
    x0, z = _grid((B, 1, 1, per), g), torch.randn((B, 1, 1, per), generator=g)
    for t in (999, 500, 0):
        row = dm.bpd_step_table(sched, (t,))[1][0]
        got = _step_in(x0, z, row)
        coef = torch.zeros(B, 12)
        coef[:, 0], coef[:, 1] = sched["sqrt_alphas_cumprod"][t], sched["sqrt_one_minus_alphas_cumprod"][t]
        xd, zd = x0.to(DEV).contiguous(), z.to(DEV).contiguous()
        want = torch.empty_like(xd)
        _lib.check(lib.dm_op_q_sample(_lib.ptr(xd), _lib.ptr(zd), _lib.fptr(coef.contiguous()), _lib.ptr(want), B, per, None))
        torch.cuda.synchronize()
        assert torch.equal(got, want.cpu()), t
        assert torch.equal(got, O.step_in(x0, z, row, torch.float32))  # and torch's fp32 q_sample


def test_step_in_philox_is_the_dm_randn_stream_and_refusals():
    lib = _lib.load()
    row = dm.bpd_step_table(dm.make_schedule(1000, "linear"), (500,))[1][0].contiguous()
    B, per = 3, 768
    x0 = _grid((B, 1, 1, per), _gen(60))
    seed, draw, off = 4321, 6, 4 * 50
    z = torch.empty((B, 1, 1, per), device=DEV)
    _lib.check(lib.dm_randn(_lib.ptr(z), z.numel(), seed, draw, off, None))
    torch.cuda.synchronize()
    assert torch.equal(_step_in(x0, z.cpu(), row), _step_in(x0, None, row, seed, draw, off))
    assert not torch.equal(_step_in(x0, None, row, seed, draw + 1, off), _step_in(x0, None, row, seed, draw, off))
    xd = x0.to(DEV)
    out = torch.empty_like(xd)
    rc = lib.dm_op_bpd_step_in(_lib.ptr(xd), None, _lib.fptr(row), 0, 0, 0, _lib.ptr(out), B, per, None)
    assert rc != 0 and b"draw 0" in lib.dm_last_error()
    bad = torch.empty((1, 6), device=DEV)
    host = (C.c_float * 3)()
    rc = lib.dm_op_bpd_terms(_lib.ptr(bad), _lib.ptr(bad), _lib.ptr(bad), _lib.ptr(bad), _lib.fptr(row), 0, 0, 1, host, 1, 6, None)
    assert rc != 0 and b"multiple of 4" in lib.dm_last_error()
    rc = lib.dm_op_bpd_terms(_lib.ptr(xd), _lib.ptr(xd), _lib.ptr(xd), _lib.ptr(xd), _lib.fptr(row), 1, 2, 1, host, 1, per, None)
    assert rc != 0 and b"first half as noise" in lib.dm_last_error()


@pytest.mark.parametrize("B,per", [(1, 4), (3, CHUNK + 4), (3, 768)])
def test_prior_vs_fp64(B, per):
    lib = _lib.load()
    x0 = _grid((B, 1, 1, per), _gen(80 + per))
    for name, T in (("linear", 1000), ("cosine", 24)):
        a, lv = Bp.prior_scalars(dm.make_schedule(T, name))
        xd = x0.to(DEV).contiguous()
        out = torch.full((B,), float("nan"), device=DEV)
        _lib.check(lib.dm_op_bpd_prior(_lib.ptr(xd), a, lv, _lib.ptr(out), B, per, None))
        torch.cuda.synchronize()
        got, want, w32 = out.cpu().double(), O.prior(x0, a, lv), O.prior(x0, a, lv, torch.float32).double()
        for b in range(B):
            err, e32 = abs(float(got[b] - want[b])) / float(want[b]), abs(float(w32[b] - want[b])) / float(want[b])
            lim = max(4 * e32, FLOOR)
            print(f"prior {name} T={T} per={per} image {b}: kernel {err:.3e} limit {lim:.3e} torch fp32 {e32:.3e}")
            assert err <= lim
