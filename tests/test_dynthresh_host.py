"""Dynamic thresholding, host side (no GPU): the fp32 restatement of the rule (tests/dynthresh_oracle.py) against
torch.quantile, the restated loops with s forced to 1 against the existing oracle loops, the keyword's surface, errors and
refusals, and the C ABI additions."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.spec import ddim_time_pairs, dpmpp_step_table, make_schedule
from oracle import sampler_oracle as so

import dpmpp_oracle as do
import dynthresh_oracle as dy
from conftest import ROOT

PERCENTILES = (0.5, 0.95, 0.995, 1.0)


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the rule -------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """Distance in fp32 steps between two positive finite fp32 tensors."""
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs()


@pytest.mark.parametrize("p", PERCENTILES)
@pytest.mark.parametrize("per", [1, 2, 5, 257, 3072])
def test_restatement_agrees_with_torch_quantile(p, per):
    """q of the restatement is torch.quantile(|x|, p) within 2 ulp of q.  torch.quantile is given |x| in float64 (the same
    values, exactly) and its result is rounded to fp32: it forms pos = p (n - 1) in the dtype of its input, and the rule
    forms pos in float64 on the host.  Given |x| in fp32, torch.quantile rounds p and pos to fp32, so its weight is off by
    up to n * 2^-24 and its own result moves by that times (v_hi - v_lo): 3 ulp from the restatement at (per 257, p 0.995)
    on the first input below, printed here and not asserted.  The restatement's own error against the exact value is the
    rounding of frac to fp32 and three fp32 operations, under 2 ulp of q while v_hi - v_lo <= q."""
    raw = seeded((3, per), 100 + per, 2.5)
    ties = raw.clone()
    ties[:, : per // 2] = 1.75      # one long run of duplicates, above 1
    ties[:, per // 2:] = ties[:, per // 2:].round()  # and many short ones
    for x in (raw, ties):
        want = torch.quantile(x.abs().double(), p, dim=1).float()
        s = dy.threshold(x, p)
        assert s.dtype == torch.float32 and s.shape == (3,)
        big = want > 1
        assert torch.all(s[~big] == 1.0)
        fp32 = torch.quantile(x.abs(), p, dim=1)
        print(f"per {per} p {p}: ulps vs float64 torch.quantile {_ulps(s[big], want[big]).tolist()}  "
              f"vs fp32 torch.quantile {_ulps(s[big], fp32[big]).tolist()}")
        assert torch.all(_ulps(s[big], want[big]) <= 2), (p, per, s, want)


def test_rule_edges():
    lo, hi, frac = dy.quantile_params(1.0, 7)
    assert (lo, hi, frac) == (6, 6, 0.0)
    assert dy.quantile_params(0.5, 2) == (0, 1, 0.5)
    assert dy.quantile_params(0.95, 1) == (0, 0, 0.0)
    x = torch.tensor([[0.5, -0.25, 0.75, -1.0]])
    assert torch.equal(dy.threshold(x, 1.0), torch.ones(1))           # every |v| <= 1: the static clamp
    assert torch.equal(dy.apply(x * 3, torch.ones(1)), (x * 3).clamp(-1, 1))
    x = torch.tensor([[0.5, float("nan"), 0.75, 3.0]])
    assert torch.isnan(dy.threshold(x, 0.5)).all()                    # as torch.quantile
    assert torch.isnan(torch.quantile(x.abs(), 0.5, dim=1)).all()
    x = torch.tensor([[4.0, -2.0, 1.0, 0.5]])
    s = dy.threshold(x, 1.0)
    assert float(s) == 4.0 and torch.equal(dy.apply(x, s), torch.tensor([[1.0, -0.5, 0.25, 0.125]]))


# ---- the loops with s forced to 1 are the existing oracle loops -----------------------------------------------------------------
def _toy(x, bt, sc=None):
    """A cheap stand-in for the network with large outputs, so that x_start leaves [-1, 1]."""
    y = torch.tanh(x * 1.3) * 2.0 + 0.001 * bt.reshape(-1, 1, 1, 1).to(x.dtype)
    return y if sc is None else y - 0.5 * sc


SHAPE = (2, 3, 8, 8)


@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0", "pred_v"])
@pytest.mark.parametrize("self_condition", [False, True])
def test_forced_one_is_the_static_clamp(objective, self_condition):
    fwd = _toy if self_condition else (lambda x, bt: _toy(x, bt))
    sched = make_schedule(12, "cosine")
    want = so.p_sample_loop(fwd, sched, SHAPE, so.NoiseStream(3), objective=objective, self_condition=self_condition)
    got = dy.p_sample_loop(fwd, sched, SHAPE, so.NoiseStream(3), 0.95, objective, self_condition, force_one=True)
    assert torch.equal(got, want)
    sched = make_schedule(1000, "linear")
    want = so.ddim_sample(fwd, sched, SHAPE, so.NoiseStream(4), 6, eta=0.5, objective=objective, self_condition=self_condition)
    got = dy.ddim_sample(fwd, sched, SHAPE, so.NoiseStream(4), 6, 0.95, 0.5, objective, self_condition, force_one=True)
    assert torch.equal(got, want)
    times, tab = dpmpp_step_table(sched, 6, 2)
    want = do.dpmpp_sample(fwd, times, tab, SHAPE, so.NoiseStream(5), objective, self_condition)
    got = dy.dpmpp_sample(fwd, times, tab, SHAPE, so.NoiseStream(5), 0.95, objective, self_condition, force_one=True)
    assert torch.equal(got, want)
    if not self_condition:
        x_T = seeded(SHAPE, 6)
        model = lambda x, t: _toy(x, torch.full((2,), t))  # noqa: E731
        pairs = ddim_time_pairs(1000, 6)
        want = do.dpmpp_sample_f64(model, sched["alphas_cumprod"], pairs, 2, x_T, objective)
        got = dy.dpmpp_sample_f64(model, sched["alphas_cumprod"], pairs, 2, x_T, 0.95, objective, force_one=True)
        assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_the_threshold_changes_the_loops_and_float64_follows():
    """With the toy network x_start leaves [-1, 1]: s > 1 at most steps, the result moves away from the static clamp, and
    the fp32 loop follows its float64 twin."""
    sched = make_schedule(1000, "linear")
    fwd = lambda x, bt: _toy(x, bt)  # noqa: E731
    log = []
    got = dy.ddim_sample(fwd, sched, SHAPE, so.NoiseStream(4), 6, 0.95, 0.5, "pred_x0", log=log)
    static = so.ddim_sample(fwd, sched, SHAPE, so.NoiseStream(4), 6, eta=0.5, objective="pred_x0")
    s = torch.stack(log)
    assert s.shape == (6, 2) and float((s > 1).float().mean()) >= 0.5
    assert float((got - static).norm() / static.norm()) > 1e-2
    f64 = dy.ddim_sample(fwd, sched, SHAPE, lambda sh, n=so.NoiseStream(4): n(sh).double(), 6, 0.95, 0.5, "pred_x0")
    assert f64.dtype == torch.float64 and float((got.double() - f64).norm() / f64.norm()) < 1e-5


# ---- the keyword --------------------------------------------------------------------------------------------------------------
METHODS = ("sample", "p_sample_loop", "ddim_sample", "dpm_solver_sample", "p_sample", "p_mean_variance", "model_predictions")


@pytest.mark.parametrize("cls", [dm.DenoisingDiffusion, dm.TextConditionalDenoisingDiffusion,
                                 dm.ImageConditionalDenoisingDiffusion])
def test_keyword_surface(cls):
    for name in METHODS:
        p = inspect.signature(getattr(cls, name)).parameters["dynamic_threshold"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None, (cls.__name__, name)


def _stub_net(**kw):
    base = dict(random_or_learned_sinusoidal_cond=False, self_condition=False, text_condition=False, out_dim=3, channels=3,
                cfg=types.SimpleNamespace(cond_channels=0), device="cuda:0", downsample_factor=2, seq1d=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_values_outside_the_interval_are_refused(monkeypatch):
    monkeypatch.setattr(dm.DenoisingDiffusion, "_run", lambda self, *a, **k: k.get("dynamic_threshold"))
    d = dm.DenoisingDiffusion(_stub_net(), image_size=16)
    for bad in (0.0, -0.1, 1.0001, 2, float("nan"), "0.95", True):
        for call in (lambda v: d.sample(batch_size=1, dynamic_threshold=v),
                     lambda v: d.p_sample_loop((1, 3, 16, 16), dynamic_threshold=v),
                     lambda v: d.ddim_sample((1, 3, 16, 16), 5, dynamic_threshold=v),
                     lambda v: d.dpm_solver_sample((1, 3, 16, 16), 5, dynamic_threshold=v),
                     lambda v: d.p_sample(torch.zeros(1, 3, 16, 16), 3, dynamic_threshold=v)):
            with pytest.raises(ValueError, match="dynamic_threshold"):
                call(bad)
    # what is accepted reaches the loop as a float; None does not reach it at all
    assert d.sample(batch_size=1, dynamic_threshold=0.95) == 0.95
    assert d.sample(batch_size=1, solver="dpmpp", dynamic_threshold=1) == 1.0
    assert d.ddim_sample((1, 3, 16, 16), 5, dynamic_threshold=0.995) == 0.995
    assert d.sample(batch_size=1) is None and d.sample(batch_size=1, dynamic_threshold=None) is None
    t = dm.TextConditionalDenoisingDiffusion(model=_stub_net(), image_size=16)
    emb = torch.ones(1, 512)
    assert t.sample(batch_size=1, text_emb=emb, dynamic_threshold=0.9) == 0.9
    assert t.sample(batch_size=1, text_emb=emb, solver="dpmpp", dynamic_threshold=0.9) == 0.9
    with pytest.raises(ValueError, match="dynamic_threshold"):
        t.sample(batch_size=1, text_emb=emb, dynamic_threshold=1.5)
    i = dm.ImageConditionalDenoisingDiffusion(_stub_net(cfg=types.SimpleNamespace(cond_channels=3)), image_size=16)
    cond = torch.zeros(1, 3, 16, 16)
    for solver in (None, "dpmpp"):
        assert i.sample(batch_size=1, cond=cond, solver=solver, dynamic_threshold=0.9) == 0.9
    with pytest.raises(ValueError, match="dynamic_threshold"):
        i.sample(batch_size=1, cond=cond, dynamic_threshold=0.0)


def test_latent_classes_refuse_with_value_error():
    vae = types.SimpleNamespace(decode=lambda z: z, encode=lambda img: img)
    inet = _stub_net(cfg=types.SimpleNamespace(cond_channels=3))
    emb, cond = torch.ones(1, 512), torch.zeros(1, 3, 16, 16)
    cases = [(dm.LatentDiffusion(_stub_net(), vae, (3, 16, 16)), {}),
             (dm.TextConditionalLatentDiffusion(_stub_net(), vae, (3, 16, 16)), dict(text_emb=emb)),
             (dm.ImageConditionalLatentDiffusion(inet, vae, (3, 16, 16), 16), dict(cond=cond))]
    for d, kw in cases:
        for solver in (None, "dpmpp"):
            with pytest.raises(ValueError, match="latents"):
                d.sample(batch_size=1, solver=solver, dynamic_threshold=0.95, **kw)


def test_other_classes_refuse_with_not_implemented():
    seq = _stub_net(seq1d=True, channels=2, out_dim=2)
    cases = [
        (dm.DenoisingDiffusion1D(seq, seq_length=16), {}),
        (dm.RePaintGaussianDiffusion(_stub_net(), image_size=16, timesteps=20), {}),
        (dm.RePaintGaussianDiffusion(_stub_net(), image_size=16, timesteps=20),
         dict(gt=torch.zeros(1, 3, 16, 16), mask=torch.ones(1, 1, 16, 16))),
        (dm.LearnedGaussianDiffusion(_stub_net(out_dim=6), image_size=16, timesteps=20), {}),
        (dm.WeightedObjectiveGaussianDiffusion(_stub_net(out_dim=8), image_size=16, timesteps=20), {}),
        (dm.ClassifierGuidedGaussianDiffusion(_stub_net(), image_size=16, timesteps=20), {}),
        (dm.ClassifierGuidedGaussianDiffusion(_stub_net(), image_size=16, timesteps=20),
         dict(cond_fn=lambda x, t: x, guidance_kwargs={})),
    ]
    for d, kw in cases:
        with pytest.raises(NotImplementedError, match="dynamic_threshold"):
            d.sample(batch_size=1, dynamic_threshold=0.95, **kw)
        with pytest.raises(ValueError, match="dynamic_threshold"):  # the value is checked first
            d.sample(batch_size=1, dynamic_threshold=7, **kw)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_additions():
    """dm_sample_args keeps its layout (tests/test_seq1d_host.py and tests/test_cfg_host.py pin it): the two fields ride in
    dm_sample_dyn_args behind it, and the ABI version stays 9."""
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    body = re.search(r"typedef struct dm_sample_dyn_args \{(.*?)\} dm_sample_dyn_args;", src, flags=re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls == ["int32_t dyn_threshold", "float dyn_percentile"]
    assert [(n, t) for n, t in _lib.SampleDynArgs._fields_] == [("dyn_threshold", ctypes.c_int32),
                                                              ("dyn_percentile", ctypes.c_float)]
    assert ctypes.sizeof(_lib.SampleDynArgs) == 8           # int32_t + float, as the header lays them out
    z = _lib.SampleDynArgs()
    assert z.dyn_threshold == 0 and z.dyn_percentile == 0.0  # the zero-initialised struct is the loop as it was
    assert ctypes.sizeof(_lib.SampleArgs) == 160 and _lib.ABI_VERSION == 9
    new = ("dm_sample_ex_dyn", "dm_op_dyn_threshold", "dm_op_sampler_update_dyn", "dm_op_dpmpp_update_dyn")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in new:
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, src), name
    assert re.search(r"int dm_sample_ex_dyn\(dm_unet\* u, const dm_sample_args\* args, const dm_sample_dyn_args\* dyn\);", src)
