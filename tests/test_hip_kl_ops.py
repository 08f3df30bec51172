"""GPU parity of the kernels of the KL first stage and of the codebook lookups next to it, one operator at a time:
``dm_op_kl_posterior`` (kl_posterior_kernel + kl_finish_kernel), ``dm_op_embed_code`` (embed_code_kernel) and
``dm_op_vq_nearest_nchw`` (vq_nearest_kernel<true>).

The posterior is compared with the reference's formulas (distributions.py:27-36, 44-46; tests/kl_oracle.py) evaluated in
fp64 on the same fp32 inputs.  Limit, per output, the rule of tests/test_hip_step_ops.py: ``rel_l2 <= max(4 x e32, 5e-5)``
with ``e32`` the error of the same formulas in fp32 torch on the CPU against that fp64.  Every case prints its figures
before it asserts.  The gathers are exact: compared bit for bit."""
import ctypes as C

import pytest
import torch

from diffusion_models_amd import _lib

import kl_oracle as ko
from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 5e-5
DEV = "cuda:0"
POISON = -7.25e11  # no output of any case comes near it


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return t.to(DEV).contiguous()


def make_moments(B, E, hw):
    """(B, 2E, hw) NCHW.  Log-variances of std 3 with -40, -30, 20 and 30 planted (both clamp edges, both far sides);
    means of unit scale with every fifth at scale 1e3."""
    mean = seeded((B, E, hw), 1)
    big = torch.arange(mean.numel()).view(B, E, hw) % 5 == 0
    mean = torch.where(big, mean * 1e3, mean)
    lv = seeded((B, E, hw), 2, 3.0).flatten()
    for i, v in enumerate((-40.0, -30.0, 20.0, 30.0, -30.0, 20.0)):
        lv[(i * 7 + 1) % lv.numel()] = v
    lv = lv.view(B, E, hw)
    assert {-40.0, -30.0, 20.0, 30.0} <= set(lv.flatten().tolist()) and float(mean.abs().max()) >= 1e3
    return torch.cat([mean, lv], dim=1).contiguous()


def as_layout(m, rows):
    """The kernel's view of the NCHW moments: as they are, or as pixel rows (B * hw, 2E)."""
    return m.permute(0, 2, 1).contiguous() if rows else m


def padded(shape, head):
    """A poisoned device buffer with `head` floats in front of and 64 behind the tensor of `shape` (view returned too)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((head + n + 64,), POISON, device=DEV)
    return buf, buf[head:head + n].view(shape)


def posterior(m_dev, rows, B, E, hw, *, eps=None, philox=None, sample=1, want=("z", "moments", "kl"), head=4):
    """One dm_op_kl_posterior call into poisoned buffers; returns {name: (whole buffer, view)} of the requested outputs."""
    out = {}
    if "z" in want:
        out["z"] = padded((B, E, hw), head)
    if "moments" in want:
        out["moments"] = padded((B, 2 * E, hw), head)
    if "kl" in want:
        out["kl"] = padded((B,), head)
    seed, draw, off = philox if philox else (0, 0, 0)
    p = lambda k: _lib.ptr(out[k][1]) if k in out else None  # noqa: E731
    rc = _lib.load().dm_op_kl_posterior(_lib.ptr(m_dev), _lib.KL_ROWS if rows else _lib.KL_NCHW, _lib.ptr(eps),
                                        C.c_uint64(seed), C.c_uint64(draw), C.c_uint64(off), sample, p("z"), p("moments"),
                                        p("kl"), B, E, hw, None)
    _lib.check(rc)
    for name, (buf, view) in out.items():
        head_, tail = buf[:head], buf[head + view.numel():]
        assert bool((head_ == POISON).all()) and bool((tail == POISON).all()), f"{name}: written outside the tensor"
    return out


# (B, E, hw)
SHAPES = [
    (3, 3, 4),      # rows of 6 floats: not 16-byte aligned
    (2, 1, 8),      # one latent channel
    (65, 4, 16),    # more than one workgroup
    (2, 4, 1024),   # the KL sum spans several wavefronts and blocks
    (3, 8, 1),      # one pixel; injected noise only
    (2, 3, 5),      # E * hw % 4 != 0: a quad crosses channels and the image's end (injected noise only)
    (1, 4, 20000),  # more quads than 64 blocks x 256 threads: the strided loop
]


@pytest.fixture(scope="module")
def refs():
    """Per shape: moments, eps and the fp64 / fp32 evaluations of the reference formulas (computed once, not modified)."""
    out = {}
    for B, E, hw in SHAPES:
        m = make_moments(B, E, hw)
        eps = seeded((B, E, hw), 3)
        p64, p32 = ko.Posterior(m.unsqueeze(-1), torch.float64), ko.Posterior(m.unsqueeze(-1))
        e4 = eps.unsqueeze(-1)
        out[(B, E, hw)] = dict(m=m, eps=eps, z=p64.sample(e4).squeeze(-1), kl=p64.kl(), mean=m[:, :E].clone(),
                               z32=p32.sample(e4).squeeze(-1), kl32=p32.kl())
    return out


@pytest.mark.parametrize("rows", [0, 1], ids=["nchw", "rows"])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_kl_posterior_vs_fp64(refs, shape, rows):
    B, E, hw = shape
    r = refs[shape]
    m_dev = dev(as_layout(r["m"], rows))
    got = posterior(m_dev, rows, B, E, hw, eps=dev(r["eps"]))
    z, mo, kl = (got[k][1].cpu() for k in ("z", "moments", "kl"))
    errs = dict(z=rel_l2(z, r["z"]), kl=rel_l2(kl, r["kl"]))
    e32 = dict(z=rel_l2(r["z32"], r["z"]), kl=rel_l2(r["kl32"], r["kl"]))
    lim = {k: max(4 * e32[k], TOL) for k in errs}
    print(f"kl_posterior {shape} {'rows' if rows else 'nchw'}: kernel {errs}  torch fp32 {e32}  limit {lim}")
    assert torch.isfinite(z).all() and torch.isfinite(kl).all()
    assert all(errs[k] <= lim[k] for k in errs)
    assert torch.equal(mo, r["m"])  # parameters in NCHW, log-variance unclamped


@pytest.mark.parametrize("rows", [0, 1], ids=["nchw", "rows"])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_kl_posterior_mode_repeat_and_optional_outputs(refs, shape, rows):
    B, E, hw = shape
    r = refs[shape]
    m_dev, eps = dev(as_layout(r["m"], rows)), dev(r["eps"])
    full = posterior(m_dev, rows, B, E, hw, eps=eps)
    again = posterior(m_dev, rows, B, E, hw, eps=eps)
    for k in ("z", "moments", "kl"):  # a fixed-order reduction: the same bits
        assert torch.equal(full[k][1], again[k][1]), k
    # sample = 0: the mode is the mean, bit for bit, with or without a noise pointer
    assert torch.equal(posterior(m_dev, rows, B, E, hw, sample=0, want=("z",))["z"][1].cpu(), r["mean"])
    assert torch.equal(posterior(m_dev, rows, B, E, hw, eps=eps, sample=0, want=("z",))["z"][1].cpu(), r["mean"])
    # each output on its own equals the one of the full call; `padded` has checked that nothing else was written
    for k in ("z", "moments", "kl"):
        assert torch.equal(posterior(m_dev, rows, B, E, hw, eps=eps, want=(k,))[k][1], full[k][1]), k
    # outputs that start 4 bytes off a 16-byte boundary: the element-by-element stores
    off = posterior(m_dev, rows, B, E, hw, eps=eps, head=1)
    for k in ("z", "moments", "kl"):
        assert torch.equal(off[k][1], full[k][1]), k


PHILOX = [s for s in SHAPES if s[1] * s[2] % 4 == 0 and s != (3, 8, 1)]


@pytest.mark.parametrize("rows", [0, 1], ids=["nchw", "rows"])
@pytest.mark.parametrize("shape", PHILOX, ids=[str(s) for s in PHILOX])
def test_kl_posterior_philox_equals_injected_dm_randn(refs, shape, rows):
    B, E, hw = shape
    m_dev = dev(as_layout(refs[shape]["m"], rows))
    lib = _lib.load()
    for seed, draw, off in ((1234567, 0, 0), (2 ** 40 + 17, 3, 8)):
        eps = torch.empty((B, E, hw), device=DEV)
        _lib.check(lib.dm_randn(_lib.ptr(eps), eps.numel(), C.c_uint64(seed), C.c_uint64(draw), C.c_uint64(off), None))
        a = posterior(m_dev, rows, B, E, hw, philox=(seed, draw, off), want=("z", "kl"))
        b = posterior(m_dev, rows, B, E, hw, eps=eps, want=("z", "kl"))
        assert torch.equal(a["z"][1], b["z"][1]) and torch.equal(a["kl"][1], b["kl"][1])
        assert not torch.equal(a["z"][1].cpu(), refs[shape]["mean"])  # noise was drawn


def test_kl_posterior_refusals():
    lib = _lib.load()
    m = torch.zeros(4096, device=DEV)
    z = torch.empty(4096, device=DEV)
    p = _lib.ptr
    u = C.c_uint64
    assert lib.dm_op_kl_posterior(p(m), 0, None, u(1), u(0), u(0), 1, p(z), None, None, 2, 3, 5, None) != 0   # Philox, 15 % 4
    assert b"% 4" in lib.dm_last_error()
    assert lib.dm_op_kl_posterior(p(m), 0, None, u(1), u(0), u(2), 1, p(z), None, None, 2, 4, 4, None) != 0   # offset % 4
    assert lib.dm_op_kl_posterior(p(m), 2, None, u(1), u(0), u(0), 0, p(z), None, None, 2, 4, 4, None) != 0   # no such layout
    assert lib.dm_op_kl_posterior(p(m), 0, None, u(1), u(0), u(0), 0, None, None, None, 2, 4, 4, None) != 0   # no output
    assert lib.dm_op_kl_posterior(None, 0, None, u(1), u(0), u(0), 0, p(z), None, None, 2, 4, 4, None) != 0
    assert lib.dm_op_kl_posterior(p(m), 0, None, u(1), u(0), u(0), 0, p(z), None, None, 0, 4, 4, None) != 0
    assert lib.dm_op_kl_posterior(p(m), 0, None, u(1), u(0), u(0), 0, p(z), None, None, 65536, 1, 1, None) != 0
    # the same shape with injected noise, or as the mode, is fine
    _lib.check(lib.dm_op_kl_posterior(p(m), 0, p(m), u(0), u(0), u(0), 1, p(z), None, None, 2, 3, 5, None))
    _lib.check(lib.dm_op_kl_posterior(p(m), 0, None, u(0), u(0), u(0), 0, p(z), None, None, 2, 3, 5, None))


# =====================================================================================================================
# embed_code_kernel: quantize.embed_code + "b h w c -> b c h w"
# =====================================================================================================================

GATHER = [(2, 3, 5, 3, 7), (1, 8, 8, 4, 8192)]  # (B, h, w, E, n_embed)


def embed_code(idx, e_dev, B, hw, E, n_embed):
    buf, out = padded((B, E, hw), 4)
    rc = _lib.load().dm_op_embed_code(_lib.ptr(idx), idx.element_size(), _lib.ptr(e_dev), _lib.ptr(out), B * hw, E, n_embed,
                                      hw, None)
    assert bool((buf[:4] == POISON).all()) and bool((buf[4 + out.numel():] == POISON).all())
    return rc, out


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("case", GATHER, ids=[str(c) for c in GATHER])
def test_embed_code(case, dtype):
    B, h, w, E, n_embed = case
    e = seeded((n_embed, E), 5)
    idx = torch.randint(0, n_embed, (B * h * w,), generator=torch.Generator().manual_seed(6))
    idx[0], idx[-1] = 0, n_embed - 1  # both ends of the codebook
    rc, out = embed_code(dev(idx.to(dtype)), dev(e), B, h * w, E, n_embed)
    _lib.check(rc)
    want = e[idx].view(B, h, w, E).permute(0, 3, 1, 2).reshape(B, E, h * w)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("bad", [-1, 7, 2 ** 31 - 1], ids=["minus1", "n_embed", "int32max"])
def test_embed_code_refuses_an_index_outside_the_codebook(bad, dtype):
    """An error from the host wrapper; the kernel does not use such an index as an address (the run goes on)."""
    B, h, w, E, n_embed = GATHER[0]
    e_dev = dev(seeded((n_embed, E), 5))
    idx = torch.randint(0, n_embed, (B * h * w,), generator=torch.Generator().manual_seed(6))
    idx[11] = bad
    rc, _ = embed_code(dev(idx.to(dtype)), e_dev, B, h * w, E, n_embed)
    assert rc != 0 and b"outside" in _lib.load().dm_last_error()
    idx[11] = 3
    rc, out = embed_code(dev(idx.to(dtype)), e_dev, B, h * w, E, n_embed)  # the flag does not stick
    _lib.check(rc)
    assert torch.equal(out.cpu(), e_dev.cpu()[idx].view(B, h * w, E).permute(0, 2, 1))
    lib = _lib.load()
    assert lib.dm_op_embed_code(_lib.ptr(dev(idx)), 2, _lib.ptr(e_dev), _lib.ptr(out), B * h * w, E, n_embed, h * w, None) != 0
    assert lib.dm_op_embed_code(_lib.ptr(dev(idx)), 8, _lib.ptr(e_dev), _lib.ptr(out), B * h * w, E, n_embed, 4, None) != 0


# =====================================================================================================================
# vq_nearest_kernel<true>: the codebook search on NCHW latents
# =====================================================================================================================

SEARCH = [(2, 3, 5, 3, 7), (3, 8, 8, 4, 1000), (1, 33, 31, 3, 8192)]  # (B, h, w, E, n_embed)


@pytest.mark.parametrize("case", SEARCH, ids=[str(c) for c in SEARCH])
def test_vq_nearest_nchw(case):
    """Inputs are codebook rows moved by 1e-3 of the smallest distance between two codes, so every winner is known and no
    pixel is left out: the indices are the planted ones, and zq is, bit for bit, what the row-layout kernel
    (dm_op_vq_nearest, unchanged) returns on the transposed input.  The planted codes are those whose nearest neighbour is
    far enough for fp32 to tell the two apart (checked in fp64 below); the whole codebook is searched."""
    B, h, w, E, n_embed = case
    hw, pixels = h * w, B * h * w
    e = seeded((n_embed, E), 8)
    d = torch.cdist(e.double(), e.double())
    d.fill_diagonal_(float("inf"))
    nn = d.min(dim=1).values
    dmin = float(nn.min())
    clear = torch.nonzero(nn ** 2 > 1e-3 * 2 * (e.double() ** 2).sum(1)).flatten()
    assert len(clear) >= n_embed // 2
    g = torch.Generator().manual_seed(9)
    idx = clear[torch.randint(0, len(clear), (pixels,), generator=g)]
    step = torch.randn((pixels, E), generator=g)
    z_rows = (e[idx] + (1e-3 * dmin) * step / step.norm(dim=1, keepdim=True)).contiguous()
    # precondition, in fp64: the planted code wins every pixel by more than fp32 can blur
    dz = torch.cdist(z_rows.double(), e.double()) ** 2
    best = dz.argmin(dim=1)
    gap = dz.scatter(1, best[:, None], float("inf")).min(dim=1).values - dz.gather(1, best[:, None])[:, 0]
    assert torch.equal(best, idx) and bool((gap > 1e-4 * ((z_rows.double() ** 2).sum(1) + (e[idx].double() ** 2).sum(1))).all())
    z_nchw = z_rows.view(B, hw, E).permute(0, 2, 1).contiguous()
    lib = _lib.load()
    e_dev = dev(e)
    outs = []
    for fn, z in ((lib.dm_op_vq_nearest_nchw, z_nchw), (lib.dm_op_vq_nearest, z_rows)):
        buf, zq = padded((B, E, hw), 4)
        got_idx = torch.full((pixels,), -1, dtype=torch.int32, device=DEV)
        _lib.check(fn(_lib.ptr(dev(z)), _lib.ptr(e_dev), _lib.ptr(zq), _lib.ptr(got_idx), pixels, E, n_embed, hw, None))
        assert bool((buf[:4] == POISON).all()) and bool((buf[4 + zq.numel():] == POISON).all())
        outs.append((zq.cpu(), got_idx.cpu().long()))
    (zq_n, idx_n), (zq_r, idx_r) = outs
    assert torch.equal(idx_n, idx) and torch.equal(idx_r, idx)
    assert torch.equal(zq_n, zq_r)
    assert torch.equal(zq_n, (z_rows + (e[idx] - z_rows)).view(B, hw, E).permute(0, 2, 1))
    # without the index output
    _, zq2 = padded((B, E, hw), 4)
    _lib.check(lib.dm_op_vq_nearest_nchw(_lib.ptr(dev(z_nchw)), _lib.ptr(e_dev), _lib.ptr(zq2), None, pixels, E, n_embed, hw, None))
    assert torch.equal(zq2.cpu(), zq_n)


def test_vq_nearest_nchw_refusals():
    lib = _lib.load()
    t = torch.zeros(4096, device=DEV)
    p = [_lib.ptr(t), _lib.ptr(t), _lib.ptr(torch.empty_like(t)), None]
    assert lib.dm_op_vq_nearest_nchw(*p, 10, 4, 16, 4, None) != 0  # pixels is not a whole number of images
    assert lib.dm_op_vq_nearest_nchw(*p, 0, 4, 16, 4, None) != 0
    assert lib.dm_op_vq_nearest_nchw(None, p[1], p[2], None, 8, 4, 16, 4, None) != 0
