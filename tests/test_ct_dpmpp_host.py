"""DPM-Solver++ (2M) for the continuous-time classes, no GPU: the step table against the solver's identities and a float64
restatement written from the paper's formulas (tests/ct_dpmpp_oracle.py), the grids, the order of accuracy on a Gaussian
data model whose probability-flow solution is known in closed form -- which is what chose the default grid -- the
argument checks, the dispatch of ``sample(solver=)`` and the binding."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import continuous as K

import ct_dpmpp_oracle as do
from conftest import ROOT, load_golden, rel_l2

SCHEDULES = ("linear", "cosine")
STEPS = (10, 20, 40, 80)
NEW = [c for c in range(K.COLS) if c not in (K.LOG_SNR, K.ALPHA, K.SIGMA, K.DPM_CX, K.DPM_CD, K.DPM_G)]


def _close(got, want, tol):
    return abs(float(got) - float(want)) <= tol * abs(float(want))


@pytest.mark.parametrize("spacing", K.SPACINGS)
@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("order", [1, 2])
def test_identities_on_rows_and_table(sched, spacing, order):
    """c_D + c_x alpha_i = alpha_next and c_x sigma_i = sigma_next: with g == 0 the step is alpha_next x0 + sigma_next eps.
    1e-12 on the float64 rows; 1e-6 on the fp32 table, three casts of 6e-8 each."""
    for n in (1, 6, 20):
        nodes = dm.ct_dpmpp_nodes(n, sched, spacing)
        rows, want, tab = K.ct_dpmpp_rows(nodes, order), do.rows_f64(nodes, order), dm.ct_dpmpp_table(n, sched, order, spacing)
        assert tab.shape == (n, K.COLS) and tab.dtype == torch.float32 and rows.dtype == torch.float64
        assert bool(torch.isfinite(tab).all()) and bool((tab[:, NEW] == 0).all())
        assert torch.equal(tab, rows.to(torch.float32))  # rounded once
        assert torch.equal(tab[:, K.LOG_SNR], nodes[:-1])
        assert rel_l2(rows, want) <= 1e-12
        for i in range(n):
            a_n, s_n = do.alpha_sigma(float(nodes[i + 1]))
            for r, tol in ((rows[i], 1e-12), (tab[i].double(), 1e-6)):
                assert _close(r[K.DPM_CD] + r[K.DPM_CX] * r[K.ALPHA], a_n, tol), (n, i, tol)
                assert _close(r[K.DPM_CX] * r[K.SIGMA], s_n, tol), (n, i, tol)
                assert _close(r[K.DPM_G], want[i, K.DPM_G], tol) or float(want[i, K.DPM_G]) == 0.0
        assert float(tab[0, K.DPM_G]) == 0.0
        assert bool((tab[1:, K.DPM_G] > 0).all()) if order == 2 else bool((tab[:, K.DPM_G] == 0).all())
        keep = [c for c in range(K.COLS) if c != K.DPM_G]
        assert torch.equal(tab[:, keep], dm.ct_dpmpp_table(n, sched, 3 - order, spacing)[:, keep])  # the order changes g alone


def test_step_with_g0_is_ddim():
    """x_next = alpha_next x0 + sigma_next eps_hat on the float64 rows, both objectives."""
    nodes = dm.ct_dpmpp_nodes(5, "linear")
    rows = K.ct_dpmpp_rows(nodes, 1)
    g = torch.Generator().manual_seed(3)
    x, F = (torch.randn((2, 3, 4, 4), generator=g, dtype=torch.float64) for _ in range(2))
    for i, row in enumerate(rows):
        a, s = float(row[K.ALPHA]), float(row[K.SIGMA])
        a_n, s_n = do.alpha_sigma(float(nodes[i + 1]))
        for objective in (do.NOISE, do.V):
            got, x0 = do.update(x, F, None, row, objective, False)
            eps = F if objective == do.NOISE else s * x + a * F
            assert rel_l2(x0, (x - s * eps) / a) <= 1e-12
            assert rel_l2(got, a_n * x0 + s_n * eps) <= 1e-12


@pytest.mark.parametrize("sched", SCHEDULES)
def test_grids(sched):
    f = K.SCHEDULES[sched]
    first, last = f(torch.tensor(1.)), f(torch.tensor(0.))
    for n in (1, 7, 20):
        nodes = dm.ct_dpmpp_nodes(n, sched)
        assert nodes.dtype == torch.float32 and nodes.shape == (n + 1,)
        assert float(nodes[0]) == float(first) and float(nodes[-1]) == float(last)  # exactly the schedule's fp32 values
        steps = (nodes[1:] - nodes[:-1]).double()
        assert float(steps.max() / steps.min()) - 1 <= 1e-5  # uniform up to the fp32 rounding of the nodes
        timed = dm.ct_dpmpp_nodes(n, sched, "time")
        assert torch.equal(timed[:-1], dm.ct_step_table(n, sched)[:, K.LOG_SNR]) and float(timed[-1]) == float(last)
    floor = dm.ct_dpmpp_nodes(10, sched, log_snr_min=-15.0)
    assert float(floor[0]) == max(float(first), -15.0) and float(floor[-1]) == float(last)
    assert torch.equal(dm.ct_dpmpp_nodes(10, sched, log_snr_min=-1e3), dm.ct_dpmpp_nodes(10, sched))
    assert float(dm.ct_dpmpp_table(10, sched, 2, "logsnr", -15.0)[0, K.LOG_SNR]) == max(float(first), -15.0)


def test_learned_schedule_nodes_come_from_the_module():
    torch.manual_seed(0)
    sched = dm.learned_noise_schedule(log_snr_max=9.0, log_snr_min=-9.0, hidden_dim=16)
    nodes = dm.ct_dpmpp_nodes(4, sched)
    assert not nodes.requires_grad
    with torch.no_grad():
        assert float(nodes[0]) == float(sched(torch.tensor(1.))) and float(nodes[-1]) == float(sched(torch.tensor(0.)))
        timed = dm.ct_dpmpp_nodes(4, sched, "time")
        assert float(timed[2]) == float(sched(torch.tensor(0.5)))
    assert dm.ct_dpmpp_table(4, sched).shape == (4, K.COLS)


@pytest.mark.parametrize("sched", SCHEDULES)
def test_order_of_accuracy_on_gaussian_data(sched):
    """Float64, optimal denoiser for x0 ~ N(0, 0.5^2), clamp off, nodes from the fp32 schedule.  On the default grid the 2M
    error is at most half the first-order error at every N (smallest measured ratio 3.70: cosine at N = 10), and 2M at
    N = 20 beats both orders on the time grid at N = 20 -- the reason the solver ships with its own grid."""
    for n in STEPS:
        e1, e2 = (do.gaussian_error(dm.ct_dpmpp_nodes(n, sched), order) for order in (1, 2))
        print(f"{sched} N={n} logsnr grid: first order {e1:.3e}  2M {e2:.3e}  ratio {e1 / e2:.2f}")
        assert e1 / e2 >= 2.0, (sched, n, e1, e2)
    ours = do.gaussian_error(dm.ct_dpmpp_nodes(20, sched), 2)
    t1, t2 = (do.gaussian_error(dm.ct_dpmpp_nodes(20, sched, "time"), order) for order in (1, 2))
    print(f"{sched} N=20: 2M on the logsnr grid {ours:.3e}; time grid first order {t1:.3e}  2M {t2:.3e}")
    assert ours < t1 and ours < t2
    # the v objective is the same solver: x_start is formed from another output
    assert abs(do.gaussian_error(dm.ct_dpmpp_nodes(20, sched), 2, do.V) / ours - 1) <= 1e-9


def test_restatement_fp32_against_float64():
    """The fp32 restatement of the update lies within 8 * 2^-24 * (sum of the magnitudes of its terms) of the float64 value
    on the same fp32 row: two roundings for x_start (v; the noise form's division is a third), three for D, three for the
    result."""
    U = 2.0 ** -24
    g = torch.Generator().manual_seed(11)
    for sched in SCHEDULES:
        for row in dm.ct_dpmpp_table(8, sched):
            x, F, hist = (torch.randn((2, 3, 4, 4), generator=g) for _ in range(3))
            for objective in (do.NOISE, do.V):
                got, x0 = do.update32(x, F, hist, row, objective, False)
                want, x0w = do.update(x.double(), F.double(), hist.double(), row.double(), objective, False)
                c = [abs(float(v)) for v in row]
                m0 = (c[K.ALPHA] * x.abs() + c[K.SIGMA] * F.abs() if objective == do.V
                      else (x.abs() + c[K.SIGMA] * F.abs()) / c[K.ALPHA]).double()
                mag = c[K.DPM_CX] * x.abs().double() + c[K.DPM_CD] * (m0 + c[K.DPM_G] * (m0 + hist.abs().double()))
                assert float(((x0.double() - x0w).abs() / (U * m0)).max()) <= 3.0
                assert float(((got.double() - want).abs() / (U * mag)).max()) <= 8.0


def test_golden_is_what_the_generator_promises():
    cases = load_golden("ct_solver.pt")["cases"]
    assert sorted(c["order"] for c in cases.values()).count(1) == 2
    assert {(c["kind"], c["order"]) for c in cases.values()} == {("v", 1), ("v", 2), ("noise", 1), ("noise", 2)}
    for key, c in cases.items():
        assert c["ref_err"] < 1e-4 and c["n"] == 6, key
        assert c["compare"] == ("sample" if c["kind"] == "v" else "x")
        assert c["compare"] != "sample" or c["clamp_share"] <= 0.5, key
        assert torch.equal(c["sample64"], (c["x64"].clamp(-1, 1) + 1) * 0.5)
    assert rel_l2(cases["v_o1"]["sample64"], cases["v_o2"]["sample64"]) > 1e-2
    assert rel_l2(cases["lin_o1_noclip"]["x64"], cases["lin_o2_noclip"]["x64"]) > 1e-2


def _stub_net(**kw):
    base = dict(random_or_learned_sinusoidal_cond=True, self_condition=False, text_condition=False, out_dim=3, channels=3,
                cfg=types.SimpleNamespace(cond_channels=0), device="cuda:0", downsample_factor=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


CLASSES = (dm.ContinuousTimeGaussianDiffusion, dm.VParamContinuousTimeGaussianDiffusion)


@pytest.mark.parametrize("cls", CLASSES)
def test_sample_dispatch(cls, monkeypatch):
    calls = []
    sig = inspect.signature(cls.dpm_solver_sample)
    monkeypatch.setattr(cls, "dpm_solver_sample", lambda self, shape, *a, **k: calls.append(("dpmpp", tuple(shape), a, k)))
    monkeypatch.setattr(cls, "p_sample_loop", lambda self, shape, **k: calls.append(("ancestral", tuple(shape), (), k)))
    d = cls(_stub_net(), image_size=16)
    d.sample(batch_size=2, seed=4)  # solver=None: today's call
    assert calls.pop() == ("ancestral", (2, 3, 16, 16), (), dict(noise=None, seed=4, sample_offset=0))
    d.sample(batch_size=2, solver="dpmpp", seed=4, sample_offset=6)
    kind, shape, a, k = calls.pop()
    assert (kind, shape, a) == ("dpmpp", (2, 3, 16, 16), (20, 2)) and d.num_sample_steps == 500  # 20, never the constructor's
    assert k == dict(spacing="logsnr", log_snr_min=None, noise=None, seed=4, sample_offset=6)
    d.sample(batch_size=1, solver="dpmpp", order=1, num_sample_steps=7, spacing="time")
    assert calls.pop()[2:] == ((7, 1), dict(spacing="time", log_snr_min=None, noise=None, seed=None, sample_offset=0))
    with pytest.raises(ValueError, match="solver"):
        d.sample(batch_size=1, solver="heun")
    with pytest.raises(ValueError, match="num_sample_steps"):
        d.sample(batch_size=1, num_sample_steps=7)
    assert not calls
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:4]] == [
        ("shape", inspect.Parameter.empty), ("num_sample_steps", 20), ("order", 2)]
    assert [p.name for p in sig.parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY] == [
        "spacing", "log_snr_min", "noise", "seed", "sample_offset", "unnormalize"]


def test_argument_checks():
    for order in (0, 3, None, 2.5, True):
        with pytest.raises(ValueError, match="order"):
            dm.ct_dpmpp_table(20, "linear", order)
    for n in (0, -1, 2.0, None):
        with pytest.raises(ValueError, match="num_sample_steps"):
            dm.ct_dpmpp_table(n, "linear")
    with pytest.raises(ValueError, match="spacing"):
        dm.ct_dpmpp_table(20, "linear", 2, "uniform")
    with pytest.raises(ValueError, match="log_snr_min"):
        dm.ct_dpmpp_table(20, "linear", 2, "logsnr", 10.0)  # above log_snr(0): no grid left
    with pytest.raises(ValueError, match="log_snr_min"):
        dm.ct_dpmpp_table(20, "linear", 2, "time", -12.0)
    with pytest.raises(ValueError, match="unknown noise schedule"):
        dm.ct_dpmpp_table(20, "sigmoid")
    for cls in CLASSES:  # the checks come before anything touches the device
        d = cls(_stub_net(), image_size=16)
        with pytest.raises(ValueError, match="order"):
            d.dpm_solver_sample((1, 3, 16, 16), order=3)
        with pytest.raises(ValueError, match="spacing"):
            d.dpm_solver_sample((1, 3, 16, 16), spacing="karras")
        with pytest.raises(ValueError, match="order"):
            d.sample(batch_size=1, solver="dpmpp", order=0)


def test_symbols_in_header_binding_and_library():
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dm_sample_ct_dpmpp", "dm_op_ct_dpmpp_step"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert re.search(r"int dm_op_ct_dpmpp_step\(const float\* x, const float\* F, float\* hist, const float\* c_host, int rows, "
                     r"int objective, int clip,\s*float\* out, int B, int64_t per, void\* stream\);", code)
    # the struct of the binding, field for field
    body = re.search(r"typedef struct dm_ct_dpmpp_args \{(.*?)\} dm_ct_dpmpp_args;", code, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.CtDpmppArgs._fields_]
    ct_h = open(os.path.join(ROOT, "diffusion-models_amd", "csrc", "ct.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"\b(CT_[A-Z_]+) = (\d+),", ct_h)}
    assert (enum["CT_DPM_CX"], enum["CT_DPM_CD"], enum["CT_DPM_G"]) == (K.DPM_CX, K.DPM_CD, K.DPM_G) == (10, 11, 12)
    lib.dm_abi_version.restype = ctypes.c_int
    assert lib.dm_abi_version() == _lib.ABI_VERSION == 9
