"""Dynamic thresholding on the GPU, operator by operator: the select (dm_op_dyn_threshold) and the two thresholded updates
(dm_op_sampler_update_dyn, dm_op_dpmpp_update_dyn) bit for bit against the fp32 restatement (tests/dynthresh_oracle.py).

Sizes: per = 1, 2 and 5 (fewer values than a wave), 255 / 256 / 257 (around the 256 bins and half a workgroup), 3072 and
12292 (several strides of the 512 threads, 12292 with a remainder), 49152 (more than any LDS staging would hold); B = 1 and 3."""
import ctypes as C

import pytest
import torch

from diffusion_models_amd import _lib

import dynthresh_oracle as dy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PERCENTILES = (0.5, 0.95, 0.995, 1.0)
ROW = [1.7, 1.3, 0.83, 0.31, 0.45, 1.0, 0.59, 0.81]


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _row(row):
    return (C.c_float * 8)(*[float(v) for v in row])


def _select(objective, x, out, p, row=ROW):
    b, per = x.shape
    xd, od = x.to(DEV).contiguous(), out.to(DEV).contiguous()
    s = torch.full((b,), -7.0, device=DEV)
    _lib.check(_lib.load().dm_op_dyn_threshold(objective, _lib.ptr(xd), _lib.ptr(od), _row(row), b, per, float(p), _lib.ptr(s),
                                               None))
    return s.cpu()


def _want(objective, x, out, p, row=ROW):
    return dy.threshold(dy.do.x_start(torch.tensor(row), objective, x, out, clamp=False), p)


def _same_bits(a, b):
    """Equal bit for bit, any NaN counting as equal to any NaN."""
    nan = torch.isnan(a) & torch.isnan(b)
    return bool(torch.all(nan | (a.view(torch.int32) == b.view(torch.int32))))


@pytest.mark.parametrize("per", [1, 2, 5, 255, 256, 257, 3072, 12292, 49152])
def test_select_bit_exact(per):
    for b in (1, 3):
        x, out = seeded((b, per), 10 + per), seeded((b, per), 20 + per, 2.0)
        for objective in (0, 1, 2):
            for p in PERCENTILES:
                got, want = _select(objective, x, out, p), _want(objective, x, out, p)
                assert _same_bits(got, want), (b, per, objective, p, got, want)
    assert float(want.max()) > 1.0 or per <= 2  # the inputs do leave [-1, 1]


def _check(vals, ps=PERCENTILES):
    """objective pred_x0: x_start_raw is the model output itself."""
    out = torch.as_tensor(vals, dtype=torch.float32).reshape(1, -1)
    for p in ps:
        got, want = _select(1, torch.zeros_like(out), out, p), dy.threshold(out, p)
        assert _same_bits(got, want), (p, got, want)
    return got


def test_select_ties_and_edges():
    g = torch.Generator().manual_seed(5)
    # all elements equal
    for n in (1, 7, 512, 3073):
        assert float(_check(torch.full((n,), -2.5))) == 2.5
    # v_lo and v_hi inside one run of duplicates: 100 values, ranks 40..79 hold 3.0; p = 0.5 -> pos 49.5
    vals = torch.cat([torch.linspace(0.1, 2.9, 40), torch.full((40,), 3.0), torch.linspace(3.5, 9.0, 20)])
    vals = vals[torch.randperm(100, generator=g)] * torch.where(torch.rand(100, generator=g) < 0.5, -1.0, 1.0)
    assert float(_check(vals, (0.5,))) == 3.0
    # v_lo the last of a run: pos = 79.2 at p = 0.8 -> v_lo = 3.0 (rank 79), v_hi = 3.5 (rank 80)
    got = _check(vals, (0.8,))
    assert 3.0 < float(got) < 3.5
    # ... and the first of a run, and the run at the very top
    _check(vals, (40 / 99, 39.5 / 99))
    _check(torch.cat([vals, torch.full((30,), 9.0)]))
    # signed zeros, alone and under a few large values
    _check([0.0, -0.0, -0.0, 0.0, 0.0])
    _check([0.0, -0.0, 4.0, -0.0, -6.0, 0.0, -0.0])
    # denormals
    _check([1e-40, -3e-41, 0.0, 5.0, -1e-39, 2e-45, -7.0])
    _check([1e-40, -3e-41, 1e-39, 2e-45])
    # one inf: finite below it, inf - inf = NaN at the top
    inf = [0.5, -2.0, float("inf"), 3.0, -1.0, 4.0, 2.5, -3.5, 0.25]
    _check(inf)
    assert torch.isnan(dy.threshold(torch.tensor([inf]), 1.0)).all() and float(dy.threshold(torch.tensor([inf]), 0.5)) == 2.5
    _check([0.5, -2.0, float("-inf"), 3.0])
    # every |v| < 1: s == 1
    small = torch.rand(3072, generator=g) * 1.98 - 0.99
    assert float(_check(small)) == 1.0
    # a NaN makes its own image NaN, whatever its rank, and no other image
    x = seeded((3, 700), 9, 3.0)
    x[1, 123] = float("nan")
    for p in PERCENTILES:
        got = _select(1, torch.zeros_like(x), x, p)
        assert torch.isnan(got[1]) and _same_bits(got, dy.threshold(x, p)) and not torch.isnan(got[[0, 2]]).any()


def test_select_is_deterministic():
    x, out = seeded((3, 12292), 1), seeded((3, 12292), 2, 2.0)
    first = _select(0, x, out, 0.95)
    for _ in range(5):
        assert torch.equal(_select(0, x, out, 0.95), first)


# ---- the updates ------------------------------------------------------------------------------------------------------------
def _sampler(kind, objective, x, out, z, row, s=None):
    """dm_op_sampler_update_dyn (s given) or dm_op_sampler_update: (x_next, x_start); outputs start as NaN."""
    b, per = x.shape
    xd, od, zd = (v.to(DEV).contiguous() for v in (x, out, z))
    res, x0 = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    lib = _lib.load()
    if s is None:
        _lib.check(lib.dm_op_sampler_update(kind, objective, _lib.ptr(xd), _lib.ptr(od), _lib.ptr(zd), _row(row), _lib.ptr(res),
                                            _lib.ptr(x0), b * per, None))
    else:
        sd = s.to(DEV).contiguous()
        _lib.check(lib.dm_op_sampler_update_dyn(kind, objective, _lib.ptr(xd), _lib.ptr(od), _lib.ptr(zd), _row(row),
                                                _lib.ptr(sd), b, per, _lib.ptr(res), _lib.ptr(x0), None))
    return res.cpu(), x0.cpu()


def _dpmpp(objective, x, out, hist, row, s=None):
    b, per = x.shape
    xd, od, hd = (v.to(DEV).contiguous() for v in (x, out, hist))
    res = torch.full_like(xd, float("nan"))
    lib = _lib.load()
    if s is None:
        _lib.check(lib.dm_op_dpmpp_update(objective, _lib.ptr(xd), _lib.ptr(od), _lib.ptr(hd), _row(row), _lib.ptr(res), b * per,
                                          None))
    else:
        sd = s.to(DEV).contiguous()
        _lib.check(lib.dm_op_dpmpp_update_dyn(objective, _lib.ptr(xd), _lib.ptr(od), _lib.ptr(hd), _row(row), _lib.ptr(sd), b, per,
                                              _lib.ptr(res), None))
    return res.cpu(), hd.cpu()


@pytest.mark.parametrize("b, per", [(3, 85), (2, 768)])
def test_updates_bit_exact(b, per):
    """(3, 85): 255 elements, a scalar tail, and threads whose four elements lie in two images; (2, 768): two blocks."""
    x, out, z = seeded((b, per), 1), seeded((b, per), 2, 3.0), seeded((b, per), 3)
    hist = seeded((b, per), 4).clamp(-1, 1)
    one = torch.ones(b)
    for objective in (0, 1, 2):
        for flag in (0.0, 1.0):
            for g in (0.0, 0.45):
                row = torch.tensor(ROW[:4] + [g, flag] + ROW[6:])
                s = dy.threshold(dy.do.x_start(row, objective, x, out, clamp=False), 0.95)
                assert float(s.min()) > 1.0 and len(set(s.tolist())) == b  # every image has its own threshold
                for kind in (0, 1):
                    want = dy.sampler_update(kind, row, objective, x, out, z, s)
                    got = _sampler(kind, objective, x, out, z, row, s)
                    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (kind, objective, flag, g)
                    # s == 1 is the static clamp, bit for bit
                    got1, plain = _sampler(kind, objective, x, out, z, row, one), _sampler(kind, objective, x, out, z, row)
                    assert torch.equal(got1[0], plain[0]) and torch.equal(got1[1], plain[1]), (kind, objective, flag, g)
                want = dy.dpmpp_update(row, objective, x, out, hist, s)
                got = _dpmpp(objective, x, out, hist, row, s)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (objective, flag, g)
                got1, plain = _dpmpp(objective, x, out, hist, row, one), _dpmpp(objective, x, out, hist, row)
                assert torch.equal(got1[0], plain[0]) and torch.equal(got1[1], plain[1]), (objective, flag, g)
    # a NaN threshold gives a NaN image and leaves the others alone
    s = torch.tensor([2.0, float("nan"), 3.0][:b])
    got = _sampler(1, 1, x, out, z, torch.tensor(ROW), s)
    want = dy.sampler_update(1, torch.tensor(ROW), 1, x, out, z, s)
    assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1])
    if b == 3:
        assert torch.isnan(got[1][1]).all() and not torch.isnan(got[1][[0, 2]]).any()


def test_select_then_update_is_the_rule():
    """The two operators chained, as the loop chains them: x_start is clamp(raw, -s, s) / s with s from the device."""
    x, out = seeded((3, 3072), 7), seeded((3, 3072), 8, 2.0)
    row = torch.tensor(ROW[:5] + [0.0] + ROW[6:])  # a last DDIM step: x_next = x_start
    for objective in (0, 1, 2):
        s = _select(objective, x, out, 0.95, row.tolist())
        raw = dy.do.x_start(row, objective, x, out, clamp=False)
        got = _sampler(1, objective, x, out, torch.zeros_like(x), row, s)
        assert torch.equal(got[1], dy.apply(raw, s)) and torch.equal(got[0], got[1])
        assert float(got[1].abs().max()) == 1.0 and float((raw.abs() > 1).float().mean()) > 0.2


def test_argument_checks():
    lib = _lib.load()
    x = torch.zeros(8, device=DEV)
    s = torch.ones(2, device=DEV)
    for p in (0.0, 1.5, -1.0):
        assert lib.dm_op_dyn_threshold(0, _lib.ptr(x), _lib.ptr(x), _row(ROW), 2, 4, p, _lib.ptr(s), None) != 0
    assert lib.dm_op_dyn_threshold(3, _lib.ptr(x), _lib.ptr(x), _row(ROW), 2, 4, 0.5, _lib.ptr(s), None) != 0
    assert lib.dm_op_dyn_threshold(0, _lib.ptr(x), _lib.ptr(x), _row(ROW), 0, 4, 0.5, _lib.ptr(s), None) != 0
    assert lib.dm_op_sampler_update_dyn(2, 0, _lib.ptr(x), _lib.ptr(x), None, _row(ROW), _lib.ptr(s), 2, 4, _lib.ptr(x), None,
                                        None) != 0
    assert lib.dm_op_sampler_update_dyn(0, 0, _lib.ptr(x), _lib.ptr(x), None, _row(ROW), None, 2, 4, _lib.ptr(x), None, None) != 0
