"""Dynamic thresholding through the sampling loops on the GPU: the golden loops of tests/golden/dynthresh.pt (the restated
loops of tests/dynthresh_oracle.py over the reference U-Nets), and what the handle does with the keyword: eager == graph,
one capture per shape for any percentile, a separate graph without the keyword, shards, the percentile that never
thresholds, the single-step methods.

Small nets: dim 32, dim_mults (1, 2), 16x16, B = 2, synthetic weights.  Loops: rel-L2 < 1e-3, the project's loop contract."""
import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo

import dynthresh_oracle as dy
from conftest import load_golden, rel_l2
from test_hip_model import LOOP_TOL, build_unet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (2, 3, 16, 16)


@pytest.fixture(scope="module")
def golden():
    g = load_golden("dynthresh.pt")
    assert g["tol"] == LOOP_TOL and tuple(g["shape"]) == SHAPE
    return g


@pytest.fixture(scope="module")
def plain(golden):
    return build_unet(salt=1, **golden["small"])


def _margins_hold(e, active=True):
    m = e["margins"]
    assert m["finite"] and m["vs_f64"] < LOOP_TOL / 10
    if active:
        assert m["active"] >= 0.5 and m["vs_static"] >= 10 * LOOP_TOL
    else:
        assert m["active"] == 0.0


def _check(name, got, e):
    err = rel_l2(got, e["y"])
    print(f"{name}: {err:.3e}  (golden: s > 1 in {e['margins']['active']:.2f} of the steps, {e['margins']['vs_static']:.2e} from "
          f"the static clamp, fp32 vs float64 {e['margins']['vs_f64']:.1e})")
    assert torch.isfinite(got).all() and err < LOOP_TOL, (name, err)


@pytest.mark.parametrize("use_graph", [False, True])
def test_golden_loops(golden, plain, use_graph):
    e = golden["ddpm50"]
    _margins_hold(e)
    d = dm.DenoisingDiffusion(plain, image_size=16, timesteps=e["T"], beta_schedule=e["schedule"], objective=e["objective"],
                              use_graph=use_graph)
    ddpm = d.p_sample_loop(SHAPE, noise=so.NoiseStream(e["seed"]), dynamic_threshold=e["p"]).cpu()
    _check("ddpm50", ddpm, e)
    assert torch.equal(d.sample(batch_size=2, noise=so.NoiseStream(e["seed"]), dynamic_threshold=e["p"]).cpu(), ddpm)

    e = golden["ddim8_v"]
    _margins_hold(e)
    d = dm.DenoisingDiffusion(plain, image_size=16, timesteps=e["T"], sampling_timesteps=e["S"], ddim_sampling_eta=e["eta"],
                              beta_schedule=e["schedule"], objective=e["objective"], use_graph=use_graph)
    ddim = d.ddim_sample(SHAPE, noise=so.NoiseStream(e["seed"]), dynamic_threshold=e["p"]).cpu()
    _check("ddim8_v", ddim, e)
    assert torch.equal(d.sample(batch_size=2, noise=so.NoiseStream(e["seed"]), dynamic_threshold=e["p"]).cpu(), ddim)

    e = golden["dpmpp8"]
    _margins_hold(e)
    d = dm.DenoisingDiffusion(plain, image_size=16, timesteps=e["T"], beta_schedule=e["schedule"], objective=e["objective"],
                              use_graph=use_graph)
    got = d.dpm_solver_sample(SHAPE, e["S"], e["order"], noise=so.NoiseStream(e["seed"]), dynamic_threshold=e["p"]).cpu()
    _check("dpmpp8", got, e)
    via = d.sample(batch_size=2, solver="dpmpp", order=e["order"], sampling_timesteps=e["S"], noise=so.NoiseStream(e["seed"]),
                   dynamic_threshold=e["p"]).cpu()
    assert torch.equal(via, got)
    static = d.dpm_solver_sample(SHAPE, e["S"], e["order"], noise=so.NoiseStream(e["seed"])).cpu()
    assert rel_l2(got, static) >= 10 * LOOP_TOL  # the threshold reached the update


def test_golden_self_conditioned(golden):
    e = golden["selfcond"]
    _margins_hold(e)
    u = build_unet(salt=e["salt"], self_condition=True, **golden["small"])
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=e["T"], sampling_timesteps=e["S"], ddim_sampling_eta=e["eta"],
                              beta_schedule=e["schedule"], objective=e["objective"])
    _check("selfcond", d.ddim_sample(SHAPE, noise=so.NoiseStream(e["seed"]), dynamic_threshold=e["p"]).cpu(), e)


def test_golden_text_conditional_guided(golden):
    e = golden["text_ddim"]
    _margins_hold(e)
    kw = dict(e["kwargs"])
    u = dm.Unet(device=DEV, **kw)
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(**kw)), salt=e["salt"]))
    d = dm.TextConditionalDenoisingDiffusion(model=u, image_size=16, timesteps=e["T"], sampling_timesteps=e["S"],
                                             ddim_sampling_eta=e["eta"], beta_schedule=e["schedule"], objective=e["objective"])
    scale, phi, remove, keep = e["case"]
    guide = dict(cond_scale=scale, rescaled_phi=phi, remove_parallel_component=remove, keep_parallel_frac=keep)
    got = d.ddim_sample(SHAPE, text_emb=e["ctx"], noise=so.NoiseStream(e["seed"]), dynamic_threshold=e["p"], **guide).cpu()
    _check("text_ddim", got, e)
    via = d.sample(batch_size=2, text_emb=e["ctx"], noise=so.NoiseStream(e["seed"]), dynamic_threshold=e["p"], **guide).cpu()
    assert torch.equal(via, got)


def test_image_conditional(golden):
    """The condition rides behind x; the threshold is taken over the image channels alone.  Against the restated loop over
    the oracle U-Net."""
    kw = dict(golden["small"], cond_channels=3)
    cfg = UnetConfig(**kw)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=34)
    u = dm.Unet(device=DEV, **kw)
    u.load_state_dict(sd)
    d = dm.ImageConditionalDenoisingDiffusion(u, image_size=16, timesteps=1000, sampling_timesteps=6)
    cond = torch.rand((2, 3, 16, 16), generator=torch.Generator().manual_seed(43))
    log = []
    want = dy.ddim_sample(lambda x, t: uo.unet_forward(sd, cfg, x, t, cond=cond), d._sched, SHAPE, so.NoiseStream(44), 6, 0.95,
                          log=log)
    got = d.ddim_sample(SHAPE, None, cond, noise=so.NoiseStream(44), dynamic_threshold=0.95).cpu()
    err = rel_l2(got, want)
    print(f"image-conditional: {err:.3e}; s > 1 in {float((torch.stack(log) > 1).float().mean()):.2f} of the steps")
    assert err < LOOP_TOL and float((torch.stack(log) > 1).float().mean()) >= 0.5
    assert torch.equal(d.sample(batch_size=2, cond=cond, noise=so.NoiseStream(44), dynamic_threshold=0.95).cpu(), got)


# ---- what the handle does ----------------------------------------------------------------------------------------------------
def test_graph_is_eager_and_one_capture_serves_every_percentile(golden):
    u = build_unet(salt=1, **golden["small"])
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=1000, sampling_timesteps=6)
    eager = dm.DenoisingDiffusion(u, image_size=16, timesteps=1000, sampling_timesteps=6, use_graph=False)
    n0 = u.graph_captures
    a = d.ddim_sample(SHAPE, seed=5, dynamic_threshold=0.95).cpu()
    assert u.graph_captures == n0 + 1
    b = d.ddim_sample(SHAPE, seed=5, dynamic_threshold=0.5).cpu()
    assert u.graph_captures == n0 + 1                 # the percentile is device data of the captured step
    assert not torch.equal(a, b)
    assert torch.equal(d.ddim_sample(SHAPE, seed=5, dynamic_threshold=0.95).cpu(), a)
    assert u.graph_captures == n0 + 1
    assert torch.equal(eager.ddim_sample(SHAPE, seed=5, dynamic_threshold=0.95).cpu(), a)
    assert torch.equal(eager.ddim_sample(SHAPE, seed=5, dynamic_threshold=0.5).cpu(), b)
    none = d.ddim_sample(SHAPE, seed=5).cpu()
    assert u.graph_captures == n0 + 2                 # without the keyword the step is another graph: one kernel fewer
    assert not torch.equal(none, a)
    fresh = build_unet(salt=1, **golden["small"])
    want = dm.DenoisingDiffusion(fresh, image_size=16, timesteps=1000, sampling_timesteps=6).ddim_sample(SHAPE, seed=5).cpu()
    assert torch.equal(none, want)                    # None is the loop of a handle that never thresholded
    # the other two kinds, graph against eager
    for fn in ("p_sample_loop", "dpm_solver_sample"):
        kw = dict(max_steps=6) if fn == "p_sample_loop" else {}
        g = getattr(d, fn)(SHAPE, seed=7, dynamic_threshold=0.9, **kw).cpu()
        assert torch.equal(getattr(eager, fn)(SHAPE, seed=7, dynamic_threshold=0.9, **kw).cpu(), g), fn
        assert not torch.equal(getattr(d, fn)(SHAPE, seed=7, **kw).cpu(), g), fn


def test_shards_are_the_whole_batch(golden, plain):
    d = dm.DenoisingDiffusion(plain, image_size=16, timesteps=1000, sampling_timesteps=6)
    whole = d.sample(batch_size=3, seed=11, dynamic_threshold=0.95).cpu()
    shards = [d.sample(batch_size=hi - lo, seed=11, sample_offset=lo, dynamic_threshold=0.95).cpu() for lo, hi in ((0, 1), (1, 3))]
    assert torch.equal(torch.cat(shards), whole)
    from diffusion_models_amd.dist import sample_global
    assert torch.equal(sample_global(d, 3, seed=11, dynamic_threshold=0.95).cpu(), whole)
    assert not torch.equal(sample_global(d, 3, seed=11).cpu(), whole)


def test_a_percentile_that_never_thresholds_is_the_static_clamp(golden, plain):
    e = golden["static"]
    _margins_hold(e, active=False)  # the generator checked q <= 1 for every image and step
    for use_graph in (False, True):
        d = dm.DenoisingDiffusion(plain, image_size=16, timesteps=e["T"], beta_schedule=e["schedule"], objective=e["objective"],
                                  use_graph=use_graph)
        none = d.dpm_solver_sample(SHAPE, e["S"], e["order"], noise=so.NoiseStream(e["seed"])).cpu()
        got = d.dpm_solver_sample(SHAPE, e["S"], e["order"], noise=so.NoiseStream(e["seed"]), dynamic_threshold=e["p"]).cpu()
        assert torch.equal(got, none)
        assert rel_l2(got, e["y"]) < LOOP_TOL


def test_none_has_the_launches_it_had_and_the_keyword_adds_one(plain):
    def profiled(fn):
        _lib.profile_enable(True)
        try:
            fn()
            rows = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
        return {r["kernel"]: r["launches"] for r in rows}

    d = dm.DenoisingDiffusion(plain, image_size=16, timesteps=1000, use_graph=False)
    base = profiled(lambda: d.ddim_sample(SHAPE, 2, seed=3))
    none = profiled(lambda: d.ddim_sample(SHAPE, 2, seed=3, dynamic_threshold=None))
    dyn = profiled(lambda: d.ddim_sample(SHAPE, 2, seed=3, dynamic_threshold=0.95))
    assert base and none == base and "dyn_threshold_kernel" not in base
    assert dyn == dict(base, dyn_threshold_kernel=2), (dyn, base)


# ---- the single-step methods -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [999, 250])
def test_p_sample_and_p_mean_variance(golden, t):
    kw = dict(golden["small"])
    cfg = UnetConfig(**kw)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=1)
    u = dm.Unet(device=DEV, **kw)
    u.load_state_dict(sd)
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=1000)
    x = torch.randn(SHAPE, generator=torch.Generator().manual_seed(60 + t))
    z = torch.randn(SHAPE, generator=torch.Generator().manual_seed(61 + t))
    fwd = lambda xx, tt: uo.unet_forward(sd, cfg, xx, tt)  # noqa: E731
    log = []
    with torch.inference_mode():
        want, want_x0 = dy.p_sample(fwd, d._sched, x, t, z, 0.95, log=log)
        static_x0 = so.p_sample(fwd, d._sched, x, t, z)[1]
    assert float(log[0].min()) > 1.0  # both images are thresholded at this time
    got, got_x0 = d.p_sample(x, t, noise=lambda shape: z, dynamic_threshold=0.95)
    print(f"p_sample t={t}: x {rel_l2(got, want):.3e}  x_start {rel_l2(got_x0, want_x0):.3e}  s {log[0].tolist()}")
    assert rel_l2(got, want) < 1e-4 and rel_l2(got_x0, want_x0) < 1e-4
    assert rel_l2(want_x0, static_x0) > 1e-2
    mean, var, logvar, x0 = d.p_mean_variance(x, t, dynamic_threshold=0.95)
    want_mean = d._sched["posterior_mean_coef1"][t] * want_x0 + d._sched["posterior_mean_coef2"][t] * x
    assert rel_l2(x0, want_x0) < 1e-4 and rel_l2(mean, want_mean) < 1e-4
    pred = d.model_predictions(x, t, clip_x_start=True, dynamic_threshold=0.95)
    assert torch.equal(pred.pred_x_start, x0)
    # honoured only with clip_x_start
    raw = d.model_predictions(x, t, clip_x_start=False, dynamic_threshold=0.95).pred_x_start
    assert torch.equal(raw, d.model_predictions(x, t, clip_x_start=False).pred_x_start)
    assert float(raw.abs().max()) > 1.0


def test_library_refusals(plain):
    d = dm.DenoisingDiffusion(plain, image_size=16, timesteps=1000, sampling_timesteps=4)
    with pytest.raises(RuntimeError, match="ddim_flags"):
        d._run(dm.diffusion.DDIM, SHAPE, *d._ddim_tables(4), [True] * 4, False, None, 1, ddim_flags=_lib.DDIM_RAW_NOISE,
               dynamic_threshold=0.95)
