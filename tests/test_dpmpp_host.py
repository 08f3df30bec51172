"""DPM-Solver++ (2M) for the integer-time classes, no GPU: the step table against the closed form of DDIM (eta = 0) and
against a float64 recomputation of h / (2 h_last), the fp32 restatement of the kernel (tests/dpmpp_oracle.py) against
float64, the order of accuracy on a Gaussian data model whose probability-flow solution is known in closed form, and
the binding, the argument checks and the refusals."""
import math
import os
import re
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.spec import DM_COEFS, ddim_step_table, ddim_time_pairs, dpmpp_step_table, make_schedule

import dpmpp_oracle as do
from conftest import ROOT, rel_l2

SCHEDULES = ("linear", "cosine", "sigmoid")
CAST_TOL = 1e-6  # one fp32 cast costs 6e-8 relative: a safe multiple of it
U = 2.0 ** -24   # unit roundoff of fp32


def _f64_schedule(sched):
    """alpha, sigma, lambda in float64 from the betas the table is built from."""
    ac = torch.cumprod(1.0 - sched["betas"].double(), dim=0)
    alpha, sigma = ac.sqrt(), (1.0 - ac).sqrt()
    return ac, alpha, sigma, torch.log(alpha / sigma)


def _close(got, want, tol=CAST_TOL):
    return abs(float(got) - float(want)) <= tol * abs(float(want))


@pytest.mark.parametrize("name", SCHEDULES)
@pytest.mark.parametrize("S", [5, 20, 50])
def test_order1_table_is_ddim_eta0(name, S):
    """c3 + c2 alpha_t = alpha_next and c2 sigma_t = sigma_next: x_next = alpha_next x0 + sigma_next eps, DDIM at eta = 0."""
    sched = make_schedule(1000, name)
    times, tab = dpmpp_step_table(sched, S, 1)
    pairs = ddim_time_pairs(1000, S)
    assert times == [p[0] for p in pairs] and tab.shape == (S, DM_COEFS) and tab.dtype == torch.float32
    _, alpha, sigma, _ = _f64_schedule(sched)
    _, ddim = ddim_step_table(sched, S, 0.0)
    for i, (t, tn) in enumerate(pairs):
        a_n, s_n = (float(alpha[tn]), float(sigma[tn])) if tn >= 0 else (1.0, 0.0)
        c = tab[i].double()
        assert _close(c[3] + c[2] * alpha[t], a_n), (name, S, i)
        assert abs(float(c[2] * sigma[t]) - s_n) <= CAST_TOL * s_n, (name, S, i)
        for col in (0, 1, 6, 7):
            assert float(tab[i, col]) == float(ddim[i, col])
    assert bool((tab[:, 4] == 0).all())
    assert tab[:, 5].tolist() == [1.0] * (S - 1) + [0.0]
    assert bool(torch.isfinite(tab).all())


@pytest.mark.parametrize("name", SCHEDULES)
@pytest.mark.parametrize("S", [5, 20, 50])
def test_order2_table(name, S):
    sched = make_schedule(1000, name)
    _, tab = dpmpp_step_table(sched, S, 2)
    _, first = dpmpp_step_table(sched, S, 1)
    _, _, _, lam = _f64_schedule(sched)
    pairs = ddim_time_pairs(1000, S)
    h = [float(lam[tn] - lam[t]) for t, tn in pairs[:-1]]
    assert float(tab[0, 4]) == 0.0 and float(tab[-1, 4]) == 0.0
    for i in range(1, S - 1):
        assert _close(tab[i, 4], h[i] / (2.0 * h[i - 1])), (name, S, i)
        assert float(tab[i, 4]) > 0
    keep = [c for c in range(DM_COEFS) if c != 4]
    assert torch.equal(tab[:, keep], first[:, keep])  # the order changes c4 alone


@pytest.mark.parametrize("objective", [0, 1, 2])
@pytest.mark.parametrize("order", [1, 2])
def test_restatement_against_float64(objective, order):
    """Every element of the fp32 restatement lies within 8 * 2^-24 * (sum of the magnitudes of its terms) of the float64
    value of the same fp32 row: at most eight roundings between the inputs and the result (dpmpp_oracle.update_f64)."""
    _, tab = dpmpp_step_table(make_schedule(1000, "cosine"), 10, order)
    g = torch.Generator().manual_seed(100 + 10 * objective + order)
    worst = 0.0
    for row in tab:
        x, out = torch.randn((2, 3, 5, 5), generator=g), torch.randn((2, 3, 5, 5), generator=g)
        hist = torch.rand((2, 3, 5, 5), generator=g) * 2 - 1
        for clamp in (True, False):
            got, x0 = do.update(row, objective, x, out, hist, clamp)
            want, mag = do.update_f64(row, objective, x, out, hist, clamp)
            ratio = float(((got.double() - want).abs() / (U * mag)).max())
            worst = max(worst, ratio)
            assert ratio <= 8.0, (objective, order, clamp, ratio)
            assert torch.equal(x0, do.x_start(row, objective, x, out, clamp))
    print(f"objective {objective} order {order}: worst error {worst:.2f} x 2^-24 x sum|terms| (bound 8)")


def _gaussian_case(name, S, order, c=0.5):
    """The fp32 oracle loop on data x0 ~ N(0, c^2): the optimal noise predictor is eps*(x, t) = sigma_t x / (alpha_t^2 c^2 +
    sigma_t^2), and the probability-flow solution scales as sqrt(alpha_t^2 c^2 + sigma_t^2).  Returns the iterate in front
    of the final x0 step, its exact value, and the float64 solver's iterate."""
    sched = make_schedule(1000, name)
    ac, alpha, sigma, _ = _f64_schedule(sched)
    var = alpha ** 2 * c * c + sigma ** 2
    times, tab = dpmpp_step_table(sched, S, order)
    shape = (1, 1, 8, 8)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(7))

    def eps32(x, bt):
        t = int(bt[0])
        return torch.tensor(float(sigma[t] / var[t]), dtype=torch.float32) * x

    frames = do.dpmpp_sample(eps32, times, tab, shape, lambda s: x_T, clamp=False, unnormalize=False,
                             return_all_timesteps=True)
    t_last = times[-1]
    exact = x_T.double() * math.sqrt(float(var[t_last]) / float(var[times[0]]))
    f64 = do.dpmpp_sample_f64(lambda x, t: float(sigma[t] / var[t]) * x, ac, ddim_time_pairs(1000, S), order, x_T,
                              clamp=False)
    return frames[:, S - 1].double(), exact, f64[S - 1]


@pytest.mark.parametrize("name", SCHEDULES)
def test_order_of_accuracy_on_gaussian_data(name):
    """The 2M error is at most half the first-order error at S = 10, 20, 40, 80 (float64 numpy gives 3.6x at the least,
    linear at S = 40).  The fp32 table-driven loop also follows the float64 solver written from alphas_cumprod: at most 80
    steps of about ten fp32 roundings each, 80 * 10 * 6e-8 = 5e-5 if they all added up, so 1e-4."""
    for S in (10, 20, 40, 80):
        errs = {}
        for order in (1, 2):
            got, exact, f64 = _gaussian_case(name, S, order)
            errs[order] = rel_l2(got, exact)
            drift = rel_l2(got, f64)
            assert drift <= 1e-4, (name, S, order, drift)
        print(f"{name} S={S}: first order {errs[1]:.3e}  2M {errs[2]:.3e}  ratio {errs[1] / errs[2]:.2f}")
        assert errs[2] <= 0.5 * errs[1], (name, S, errs)


def test_binding_matches_the_header():
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    assert re.search(r"int dm_op_dpmpp_update\(int objective, const float\* x, const float\* model_out, float\* x0_hist,\s*"
                     r"const float\* coef_host,\s*float\* out, int64_t n, void\* stream\);", src)
    assert "dm_op_dpmpp_update" in _lib.EXPORTS
    assert int(re.search(r"#define DM_SAMPLER_DPMPP (\d+)", src).group(1)) == dm.diffusion.DPMPP == 2
    assert int(re.search(r"#define DM_COEFS (\d+)", src).group(1)) == DM_COEFS == 8
    assert _lib.ABI_VERSION == 9


def _stub_net(**kw):
    base = dict(random_or_learned_sinusoidal_cond=False, self_condition=False, text_condition=False, out_dim=3, channels=3,
                cfg=types.SimpleNamespace(cond_channels=0), device="cuda:0", downsample_factor=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_sample_dispatch_on_the_six_classes(monkeypatch):
    """``sample(solver='dpmpp', order=k, sampling_timesteps=S)`` reaches the loop with kind DM_SAMPLER_DPMPP and the
    (S, order) table, with each class's own condition; the latent classes decode what the loop returns."""
    calls = []

    def fake_run(self, kind, shape, times, coefs, takes_noise, return_all_timesteps, noise, seed, text_emb=None,
                 max_steps=None, cond=None, sample_offset=0, x_init=None, unnormalize=None, guidance=None):
        calls.append(dict(kind=kind, shape=tuple(shape), S=len(times), second=bool((coefs[:, 4] != 0).any()),
                          takes=list(takes_noise), text=text_emb, cond=cond, guidance=guidance))
        return torch.zeros(shape)

    monkeypatch.setattr(dm.DenoisingDiffusion, "_run", fake_run)
    vae = types.SimpleNamespace(decode=lambda z: z + 1.0, encode=lambda img: img * 0.5)
    inet = _stub_net(cfg=types.SimpleNamespace(cond_channels=3))
    emb, cond = torch.ones(2, 512), torch.full((2, 3, 16, 16), 0.25)
    cases = [
        (dm.DenoisingDiffusion(_stub_net(), image_size=16), {}, False),
        (dm.TextConditionalDenoisingDiffusion(model=_stub_net(), image_size=16), dict(text_emb=emb, cond_scale=1.0), False),
        (dm.ImageConditionalDenoisingDiffusion(inet, image_size=16), dict(cond=cond), False),
        (dm.LatentDiffusion(_stub_net(), vae, (3, 16, 16)), {}, True),
        (dm.TextConditionalLatentDiffusion(_stub_net(), vae, (3, 16, 16)), dict(text_emb=emb), True),
        (dm.ImageConditionalLatentDiffusion(inet, vae, (3, 16, 16), 16), dict(cond=cond), True),
    ]
    for d, kw, latent in cases:
        for order in (1, 2):
            calls.clear()
            y = d.sample(batch_size=2, solver="dpmpp", order=order, sampling_timesteps=7, **kw)
            (c,) = calls
            assert c["kind"] == 2 and c["shape"] == (2, 3, 16, 16) and c["S"] == 7 and c["takes"] == [], type(d).__name__
            assert c["second"] == (order == 2) and c["guidance"] is None
            assert (c["text"] is emb) == ("text_emb" in kw)
            if "cond" in kw:
                assert torch.equal(c["cond"], cond * 0.5 if latent else cond)
            assert float(y.flatten()[0]) == (1.0 if latent else 0.0), type(d).__name__
        calls.clear()
        d.sample(batch_size=2, **kw)  # solver=None: the dispatch it always was (DDPM here)
        assert calls[0]["kind"] == 0 and calls[0]["S"] == 1000
    got = cases[2][0].sample(batch_size=2, return_condition_image=True, solver="dpmpp", cond=cond)
    assert got[0] is cond and calls[-1]["S"] == 20  # sampling_timesteps: 20 when the constructor selects DDPM


def test_argument_checks_and_refusals():
    sched = make_schedule(1000, "linear")
    for order in (0, 3, None, 2.5):
        with pytest.raises(ValueError, match="order"):
            dpmpp_step_table(sched, 20, order)
    for S in (0, -1, 1001, 2.0, None):
        with pytest.raises(ValueError, match="sampling_timesteps"):
            dpmpp_step_table(sched, S, 2)
    assert dpmpp_step_table(sched, 1, 2)[1].shape == (1, DM_COEFS) and len(dpmpp_step_table(sched, 1000, 2)[0]) == 1000
    d = dm.DenoisingDiffusion(_stub_net(), image_size=16)
    with pytest.raises(ValueError, match="order"):
        d.dpm_solver_sample((1, 3, 16, 16), order=3)
    with pytest.raises(ValueError, match="sampling_timesteps"):
        d.dpm_solver_sample((1, 3, 16, 16), sampling_timesteps=1001)
    with pytest.raises(ValueError, match="solver"):
        d.sample(batch_size=1, solver="heun")
    # sampling_timesteps: the constructor's when it selects DDIM sampling, else 20
    assert len(d._dpmpp_tables(None, 2)[0]) == 20
    assert len(dm.DenoisingDiffusion(_stub_net(), image_size=16, sampling_timesteps=50)._dpmpp_tables(None, 2)[0]) == 50
    text = dm.TextConditionalDenoisingDiffusion(model=_stub_net(), image_size=16)
    with pytest.raises(ValueError, match="solver"):
        text.sample(batch_size=1, solver="ddim", text_emb=torch.zeros(1, 512))
    img = dm.ImageConditionalDenoisingDiffusion(_stub_net(cfg=types.SimpleNamespace(cond_channels=3)), image_size=16)
    with pytest.raises(ValueError, match="solver"):
        img.sample(batch_size=1, solver="ddim", cond=torch.zeros(1, 3, 16, 16))
    lv = dm.LearnedGaussianDiffusion(_stub_net(out_dim=6), image_size=16)
    with pytest.raises(NotImplementedError, match="dpm_solver_sample"):
        lv.dpm_solver_sample((1, 3, 16, 16))
    wo = dm.WeightedObjectiveGaussianDiffusion(_stub_net(out_dim=8), image_size=16)
    with pytest.raises(NotImplementedError, match="dpm_solver_sample"):
        wo.dpm_solver_sample((1, 3, 16, 16))
