"""GPU parity of the sequence model (Unet1D / DenoisingDiffusion1D, through dm_unet_forward / dm_sample_ex on a seq1d handle)
against the goldens generated from the reference (tests/golden/seq1d.pt).

Tolerances are those of tests/test_hip_model.py (rel-L2, fp32): one U-Net forward <= 1e-4, whole loops <= 1e-3.  Every golden
carries the reference's own fp32-vs-fp64 error, which must be at most a tenth of the limit it is used with.  Measured values
are printed with -s."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from oracle import sampler_oracle as so

from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 1e-4
LOOP_TOL = 1e-3


@pytest.fixture(scope="module")
def golden():
    return load_golden("seq1d.pt")


_UNETS = {}


def unet(golden, key):
    """One handle per golden configuration, shared by the tests of this module."""
    if key not in _UNETS:
        g = golden["unet"][key]
        u = dm.Unet1D(device=DEV, **g["unet_kw"])
        u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=g["salt"]))
        _UNETS[key] = u
    return _UNETS[key]


def diffusion(golden, key, use_graph=True):
    g = golden["loops"][key]
    return dm.DenoisingDiffusion1D(unet(golden, g["unet"]), seq_length=g["L"], use_graph=use_graph, **g["diffusion_kw"])


def run_loop(golden, key, use_graph=True, **kw):
    g = golden["loops"][key]
    d = diffusion(golden, key, use_graph)
    if g["method"] == "sample":
        return d.sample(batch_size=g["batch"], **kw)
    return getattr(d, g["method"])((g["batch"], d.channels, g["L"]), **g["method_kw"], **kw)


@pytest.mark.parametrize("key", ["d32_c2", "d64_c1", "selfcond", "dh64"])
def test_unet1d_forward(golden, key):
    g = golden["unet"][key]
    assert g["ref_err"] <= FWD_TOL / 10
    u = unet(golden, key)
    y = u(g["x"].to(DEV), g["t"].to(DEV), g["x_self_cond"]).cpu()
    err = rel_l2(y, g["y"])
    print("unet1d", key, "rel-L2", err, "reference fp32-vs-fp64", g["ref_err"])
    assert y.shape == g["y"].shape and torch.isfinite(y).all() and err < FWD_TOL
    assert u.workspace_bytes > 0


def test_unet1d_surface(golden):
    u = unet(golden, "d32_c2")
    sd = u.state_dict()
    want = dm.synth_state_dict(u.param_spec(), salt=golden["unet"]["d32_c2"]["salt"])
    assert list(sd.keys()) == [k for k, _ in u.param_spec()] and all(torch.equal(sd[k].cpu(), want[k]) for k in want)
    assert sum(p.numel() for p in u.parameters()) == sum(v.numel() for v in want.values())
    assert u.to(DEV) is u and u.cuda() is u and u.eval() is u
    with pytest.raises(RuntimeError):
        u(torch.zeros(1, 2, 31), torch.zeros(1, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        u.train()
    # a second load refreshes the weights in place (every layer is re-packed, the Upsample packing included): other values
    # give what a fresh handle gives with them, and the first values give the first output again
    g = golden["unet"]["d32_c2"]
    y0 = u(g["x"], g["t"])
    other = dm.synth_state_dict(u.param_spec(), salt=77)
    fresh = dm.Unet1D(device=DEV, **g["unet_kw"])
    fresh.load_state_dict(other)
    u.load_state_dict(other)
    y1 = u(g["x"], g["t"])
    assert torch.equal(y1, fresh(g["x"], g["t"])) and not torch.equal(y1, y0)
    u.load_state_dict(want)
    assert torch.equal(u(g["x"], g["t"]), y0)
    for name in ("grads", "optimizer_step", "sync", "ema_update"):
        with pytest.raises(NotImplementedError):
            getattr(u, name)()


def test_train_enable_is_refused_and_leaves_the_handle_usable(golden):
    u = unet(golden, "d32_c2")
    g = golden["unet"]["d32_c2"]
    y0 = u(g["x"], g["t"])
    lib = _lib.load()
    assert lib.dm_unet_train_enable(u._handle) != 0
    assert "sequence model" in lib.dm_last_error().decode()
    assert lib.dm_unet_train_enable_ft(u._handle, 0) != 0
    assert torch.equal(u(g["x"], g["t"]), y0)


def test_forward_rejects_an_image_shape(golden):
    u = unet(golden, "d32_c2")
    lib = _lib.load()
    x = torch.zeros(1, 2, 2, 16, device=DEV)
    t = torch.zeros(1, dtype=torch.long, device=DEV)
    out = torch.empty(1, 2, 2, 16, device=DEV)
    assert lib.dm_unet_forward(u._handle, _lib.ptr(x), _lib.ptr(t), None, 0, _lib.ptr(out), 1, 2, 16, None) != 0
    assert lib.dm_unet_forward(u._handle, _lib.ptr(x), _lib.ptr(t), None, 0, _lib.ptr(out), 1, 1, 31, None) != 0
    assert "divisible by 2" in lib.dm_last_error().decode()


def test_learned_sinusoidal_unet1d_runs_forward_only():
    u = dm.Unet1D(dim=32, dim_mults=(1, 2), channels=2, learned_sinusoidal_cond=True, device=DEV)
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=9))
    y = u(torch.zeros(2, 2, 8), torch.tensor([1, 5]))
    assert y.shape == (2, 2, 8) and torch.isfinite(y).all()
    with pytest.raises(NotImplementedError):
        dm.DenoisingDiffusion1D(u, seq_length=8)


def test_p_mean_variance(golden):
    g = golden["p_mean_variance"]
    d = dm.DenoisingDiffusion1D(unet(golden, g["unet"]), seq_length=g["x"].shape[-1], timesteps=g["timesteps"])
    for row in g["rows"]:
        t = torch.full((g["x"].shape[0],), row["t"], dtype=torch.long)
        mean, var, logvar, x_start = d.p_mean_variance(g["x"], t)
        errs = (rel_l2(mean, row["mean"]), rel_l2(x_start, row["x_start"]))
        print("p_mean_variance t", row["t"], errs)
        assert max(errs) < FWD_TOL
        assert torch.equal(var.reshape(-1).cpu(), row["var"]) and torch.equal(logvar.reshape(-1).cpu(), row["logvar"])
        mp = d.model_predictions(g["x"], t, clip_x_start=True)
        assert rel_l2(mp.pred_x_start, row["x_start"]) < FWD_TOL


@pytest.mark.parametrize("key", ["ddpm50", "ddim8_clip", "ddim8_noclip", "ddim8_v", "ddim6_selfcond", "ddpm24_d64"])
def test_loops(golden, key):
    g = golden["loops"][key]
    assert g["ref_err"] <= LOOP_TOL / 10
    y = run_loop(golden, key, noise=so.NoiseStream(g["noise_seed"])).cpu()
    err = rel_l2(y, g["sample"])
    print("loop", key, "rel-L2", err, "reference fp32-vs-fp64", g["ref_err"])
    assert y.shape == g["sample"].shape and torch.isfinite(y).all() and err < LOOP_TOL


def test_ddim_does_not_rederive(golden):
    """The goldens can tell the sequence class's DDIM from the image class's: the generator asserted the margins."""
    m = golden["margins"]
    assert min(m["rederive"], m["clip"]) >= 10 * LOOP_TOL
    y = run_loop(golden, "ddim8_clip", noise=so.NoiseStream(golden["loops"]["ddim8_clip"]["noise_seed"])).cpu()
    assert rel_l2(y, m["rederived_sample"]) > 100 * LOOP_TOL > rel_l2(y, golden["loops"]["ddim8_clip"]["sample"])


def test_interpolate(golden):
    g = golden["interpolate"]
    assert g["ref_err"] <= LOOP_TOL / 10
    d = dm.DenoisingDiffusion1D(unet(golden, g["unet"]), seq_length=g["x1"].shape[-1], timesteps=g["timesteps"])
    y = d.interpolate(g["x1"], g["x2"], t=g["t"], lam=g["lam"], noise=so.NoiseStream(g["noise_seed"])).cpu()
    err = rel_l2(y, g["y"])
    print("interpolate rel-L2", err)
    assert y.shape == g["y"].shape and err < LOOP_TOL


@pytest.mark.parametrize("key", ["ddim8_clip", "ddpm50"])
def test_graph_replay_equals_eager_and_captures_once(golden, key):
    u = unet(golden, golden["loops"][key]["unet"])
    eager = run_loop(golden, key, use_graph=False, seed=5)
    n0 = u.graph_captures
    a = run_loop(golden, key, use_graph=True, seed=5)
    n1 = u.graph_captures
    b = run_loop(golden, key, use_graph=True, seed=5)
    c = run_loop(golden, key, use_graph=True, seed=6)
    assert torch.equal(a, eager) and torch.equal(a, b) and not torch.equal(a, c)
    assert n1 - n0 <= 1 and u.graph_captures == n1, "one capture per shape"


def test_clip_settings_do_not_share_a_graph(golden):
    """clip_denoised is a kernel argument of the captured update: the two settings are two graphs, each right."""
    u = unet(golden, "d32_c2")
    ga, gb = golden["loops"]["ddim8_clip"], golden["loops"]["ddim8_noclip"]
    a = run_loop(golden, "ddim8_clip", noise=so.NoiseStream(ga["noise_seed"])).cpu()
    b = run_loop(golden, "ddim8_noclip", noise=so.NoiseStream(gb["noise_seed"])).cpu()
    a2 = run_loop(golden, "ddim8_clip", noise=so.NoiseStream(ga["noise_seed"])).cpu()
    assert rel_l2(a, ga["sample"]) < LOOP_TOL and rel_l2(b, gb["sample"]) < LOOP_TOL and torch.equal(a, a2)
    assert u.graph_captures >= 2


def test_sharded_equals_whole_batch(golden):
    d = diffusion(golden, "ddim8_v")  # eta = 0.5: every step draws device noise
    whole = d.sample(batch_size=4, seed=11)
    parts = [d.sample(batch_size=2, seed=11, sample_offset=off) for off in (0, 2)]
    assert torch.equal(torch.cat(parts), whole)
    assert d.sample_shape() == (2, 32) and whole.shape == (4, 2, 32)


def test_return_all_timesteps(golden):
    d = diffusion(golden, "ddim8_clip")
    frames = d.sample(batch_size=2, return_all_timesteps=True, seed=3)
    last = d.sample(batch_size=2, seed=3)
    assert frames.shape == (2, 9, 2, 32) and torch.equal(frames[:, -1], last)


def test_diffusion_state_dict_round_trip(golden):
    d = diffusion(golden, "ddpm50")
    sd = d.state_dict()
    assert list(sd.keys()) == golden["state_dict_keys"]
    d.load_state_dict({k: v.cpu() for k, v in sd.items()})
    g = golden["loops"]["ddpm50"]
    assert rel_l2(run_loop(golden, "ddpm50", noise=so.NoiseStream(g["noise_seed"])), g["sample"]) < LOOP_TOL


def test_library_refuses_the_unpinned_solver(golden):
    """DenoisingDiffusion1D refuses DPM-Solver++ in Python; a caller that reaches the loop anyway is refused by the library,
    and the handle stays usable."""
    d = diffusion(golden, "ddim8_clip")
    with pytest.raises(NotImplementedError):
        d.dpm_solver_sample((2, 2, 32))
    with pytest.raises(RuntimeError, match="DPM-Solver"):
        dm.DenoisingDiffusion.dpm_solver_sample(d, (2, 2, 32), sampling_timesteps=4, seed=1)
    g = golden["loops"]["ddim8_clip"]
    assert rel_l2(run_loop(golden, "ddim8_clip", noise=so.NoiseStream(g["noise_seed"])), g["sample"]) < LOOP_TOL
