"""DPM-Solver++ (2M) for the integer-time classes on the GPU: the update operator (dm_op_dpmpp_update) bit for bit against
the fp32 restatement (tests/dpmpp_oracle.py), order 1 against the reference's own recorded ``ddim_sample`` (first-order
DPM-Solver++ is DDIM with eta = 0), order 2 against the CPU oracle loop over ``oracle.unet_oracle.unet_forward`` -- every
objective, self-conditioning, all frames, the text- / image-conditional and latent wrappers -- and what the handle does:
one capture per shape, eager == graph, DDIM unaffected, shards, launches.

Small nets: dim 32, dim_mults (1, 2), 16x16, B = 2, synthetic weights.  Loops: rel-L2 < 1e-3, the project's loop contract."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.spec import (DecoderConfig, EncoderConfig, UnetConfig, dpmpp_step_table, encoder_param_spec,
                                       make_schedule)
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo
from oracle import vae_oracle as vo

import dpmpp_oracle as do
from conftest import load_golden, rel_l2
from test_cfg_host import guided_f64
from test_hip_model import LOOP_TOL, build_unet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPE = (2, 3, 16, 16)
SMALL = dict(dim=32, dim_mults=(1, 2), channels=3)


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _net(salt, **kw):
    """(handle, state dict, config) of a small U-Net with synthetic weights."""
    kw = dict(SMALL, **kw)
    cfg = UnetConfig(**kw)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt)
    u = dm.Unet(device=DEV, **kw)
    u.load_state_dict(sd)
    return u, sd, cfg


# ---- 1. the operator ---------------------------------------------------------------------------------------------------
def _op(objective, x, out, hist, row):
    """dm_op_dpmpp_update on device copies: (x_next, history afterwards); the output starts as NaN."""
    n = x.numel()
    xd, od, hd = (v.to(DEV).contiguous() for v in (x, out, hist))
    res = torch.full((n,), float("nan"), device=DEV)
    _lib.check(_lib.load().dm_op_dpmpp_update(objective, _lib.ptr(xd), _lib.ptr(od), _lib.ptr(hd),
                                              (C.c_float * 8)(*[float(v) for v in row]), _lib.ptr(res), n, None))
    return res.cpu(), hd.cpu()


@pytest.mark.parametrize("n", [2 * 3 * 5 * 5, 1536])
def test_operator_bit_exact(n):
    """n = 150 ends in a scalar tail (150 = 4 * 37 + 2); 1536 = 4 * 384 spans two blocks of 256 threads."""
    x, out, hist = seeded((n,), 1), seeded((n,), 2, 3.0), seeded((n,), 3).clamp(-1, 1)
    nan = torch.full((n,), float("nan"))
    for obj in (0, 1, 2):
        for g in (0.0, 0.7):
            for flag in (0.0, 1.0):
                row = torch.tensor([1.7, 1.3, 0.83, 0.31, g, flag, 0.59, 0.81], dtype=torch.float32)
                want, want_x0 = do.update(row, obj, x, out, hist)
                got, got_hist = _op(obj, x, out, hist, row)
                assert torch.equal(got, want), (n, obj, g, flag)  # no NaN left: every element was written
                assert torch.equal(got_hist, want_x0), (n, obj, g, flag)
                if g == 0.0:  # the history is not read: a NaN buffer gives the same result and is overwritten
                    got, got_hist = _op(obj, x, out, nan, row)
                    assert torch.equal(got, want) and torch.equal(got_hist, want_x0), (n, obj, flag)
    # rows of a real table, the last one (flag 0, c2 = 0, c3 = 1) included
    _, tab = dpmpp_step_table(make_schedule(1000, "linear"), 5, 2)
    for row in tab:
        want, want_x0 = do.update(row, 0, x, out, hist)
        got, got_hist = _op(0, x, out, hist, row)
        assert torch.equal(got, want) and torch.equal(got_hist, want_x0)


# ---- 2. the tie to the reference -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_unet():
    return build_unet(salt=1, **SMALL)


@pytest.mark.parametrize("use_graph", [False, True])
def test_order1_is_the_reference_ddim(golden_samplers, small_unet, use_graph):
    b = golden_samplers["small_ddim50"]  # the reference's own ddim_sample, eta = 0, S = 50
    assert b["eta"] == 0.0 and tuple(b["shape"]) == SHAPE
    d = dm.DenoisingDiffusion(small_unet, image_size=16, timesteps=1000, use_graph=use_graph)
    y = d.dpm_solver_sample(b["shape"], sampling_timesteps=b["S"], order=1, noise=so.NoiseStream(b["seed"])).cpu()
    err = rel_l2(y, b["y"])
    ours = d.ddim_sample(b["shape"], sampling_timesteps=b["S"], noise=so.NoiseStream(b["seed"])).cpu()
    err_ours = rel_l2(y, ours)
    print(f"order 1 vs reference ddim_sample (graph {use_graph}): {err:.3e}   vs this library's ddim_sample: {err_ours:.3e}")
    assert err < LOOP_TOL and err_ours < LOOP_TOL


# ---- 3. order 2 against the CPU oracle loop --------------------------------------------------------------------------------
def _oracle(fwd, sched, S, order, seed, **kw):
    times, tab = dpmpp_step_table(sched, S, order)
    return do.dpmpp_sample(fwd, times, tab, SHAPE, so.NoiseStream(seed), **kw)


@pytest.fixture(scope="module")
def plain():
    return _net(1)


@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0", "pred_v"])
def test_order2_objectives(plain, objective):
    u, sd, cfg = plain
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=8, beta_schedule="cosine", objective=objective)
    got = d.dpm_solver_sample(SHAPE, 6, 2, return_all_timesteps=True, noise=so.NoiseStream(31)).cpu()
    want = _oracle(lambda x, t: uo.unet_forward(sd, cfg, x, t), d._sched, 6, 2, 31, objective=objective,
                   return_all_timesteps=True)
    assert got.shape == want.shape == (2, 7, 3, 16, 16)
    err, first = rel_l2(got, want), rel_l2(got[:, 1], want[:, 1])
    print(f"order 2 {objective}: all frames {err:.3e}  first iterate {first:.3e}  final {rel_l2(got[:, -1], want[:, -1]):.3e}")
    assert torch.equal(got[:, 0], want[:, 0])  # x_T
    assert err < LOOP_TOL and first < 1e-4
    final = d.dpm_solver_sample(SHAPE, 6, 2, noise=so.NoiseStream(31)).cpu()
    assert torch.equal(final, got[:, -1])


def test_order2_self_conditioning():
    """One buffer: the x_start the solver extrapolates from is the x_start the U-Net is fed."""
    u, sd, cfg = _net(32, self_condition=True)
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=8, beta_schedule="cosine")
    got = d.dpm_solver_sample(SHAPE, 6, 2, noise=so.NoiseStream(33)).cpu()
    want = _oracle(lambda x, t, sc: uo.unet_forward(sd, cfg, x, t, sc), d._sched, 6, 2, 33, self_condition=True)
    err = rel_l2(got, want)
    print(f"order 2 self-conditioning: {err:.3e}")
    assert err < LOOP_TOL


# ---- 4. the wrappers ---------------------------------------------------------------------------------------------------
def test_text_conditional_guided():
    m = load_golden("cfg_text.pt")["models"]["concat"]  # the small text configuration of tests/test_hip_cfg.py
    kw = dict(m["kwargs"])
    cfg = UnetConfig(**kw)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=m["salt"])
    u = dm.Unet(device=DEV, **kw)
    u.load_state_dict(sd)
    d = dm.TextConditionalDenoisingDiffusion(model=u, image_size=16, timesteps=1000)
    ctx = seeded((2, 512), 41)
    case = (3.0, 0.7, True, 0.0)

    def fwd(x, t):
        cond, null = uo.unet_forward(sd, cfg, x, t, text_emb=ctx), uo.unet_forward(sd, cfg, x, t)
        return guided_f64(cond, null, *case).float()

    want = _oracle(fwd, d._sched, 6, 2, 42)
    got = d.dpm_solver_sample(SHAPE, None, 6, 2, text_emb=ctx, noise=so.NoiseStream(42), cond_scale=3.0, rescaled_phi=0.7).cpu()
    err = rel_l2(got, want)
    print(f"text-conditional, cond_scale 3, rescaled_phi 0.7: {err:.3e}")
    assert err < LOOP_TOL
    via_sample = d.sample(batch_size=2, solver="dpmpp", sampling_timesteps=6, text_emb=ctx, noise=so.NoiseStream(42),
                          cond_scale=3.0, rescaled_phi=0.7).cpu()
    assert torch.equal(via_sample, got)
    plain = d.dpm_solver_sample(SHAPE, None, 6, 2, text_emb=ctx, noise=so.NoiseStream(42)).cpu()
    assert rel_l2(plain, got) > 1e-3  # the guidance reached the update


def test_image_conditional():
    u, sd, cfg = _net(34, cond_channels=3)
    d = dm.ImageConditionalDenoisingDiffusion(u, image_size=16, timesteps=1000)
    cond = torch.rand((2, 3, 16, 16), generator=torch.Generator().manual_seed(43))
    want = _oracle(lambda x, t: uo.unet_forward(sd, cfg, x, t, cond=cond), d._sched, 6, 2, 44)
    back, got = d.dpm_solver_sample(SHAPE, 6, 2, cond, True, noise=so.NoiseStream(44))
    err = rel_l2(got.cpu(), want)
    print(f"image-conditional: {err:.3e}")
    assert err < LOOP_TOL and back is cond
    via_sample = d.sample(batch_size=2, solver="dpmpp", sampling_timesteps=6, cond=cond, noise=so.NoiseStream(44))
    assert torch.equal(via_sample, got)


def test_latent_diffusion(plain):
    u, sd, cfg = plain
    vsd = dm.synth_state_dict(encoder_param_spec(EncoderConfig(n_embed=8192)) + dm.decoder_param_spec(DecoderConfig()), salt=21)
    vae = dm.VQModel(dict(ch=64, out_ch=3, in_channels=3, ch_mult=(1, 2), num_res_blocks=2, attn_resolutions=(),
                          resolution=32, z_channels=3, double_z=False), n_embed=8192, embed_dim=3, device=DEV)
    vae.load_state_dict(vsd)
    ld = dm.LatentDiffusion(u, vae, latent_shape=(3, 16, 16), timesteps=1000)
    lat = _oracle(lambda x, t: uo.unet_forward(sd, cfg, x, t), ld._sched, 6, 2, 45, unnormalize=False)
    with torch.inference_mode():
        want = vo.vq_decode(vsd, DecoderConfig(), lat)
    got = ld.sample(batch_size=2, solver="dpmpp", order=2, sampling_timesteps=6, noise=so.NoiseStream(45)).cpu()
    err = rel_l2(got, want)
    print(f"LatentDiffusion (decoded): {err:.3e}")
    assert got.shape == (2, 3, 32, 32) and err < LOOP_TOL


# ---- 5. what the handle does ---------------------------------------------------------------------------------------------
def test_one_graph_serves_every_table_and_ddim_is_untouched():
    u, _, _ = _net(1)
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=1000)
    n0 = u.graph_captures
    a = d.dpm_solver_sample(SHAPE, 6, 2, seed=5).cpu()
    assert u.graph_captures == n0 + 1
    others = [d.dpm_solver_sample(SHAPE, 4, 2, seed=5).cpu(), d.dpm_solver_sample(SHAPE, 6, 1, seed=5).cpu(),
              d.dpm_solver_sample(SHAPE, 6, 2, seed=6).cpu()]
    assert u.graph_captures == n0 + 1
    assert all(not torch.equal(a, o) for o in others)
    assert torch.equal(d.dpm_solver_sample(SHAPE, 6, 2, seed=5).cpu(), a)
    # More steps than the handle's device tables have ever held: the tables are reallocated (grow_tables,
    # csrc/dm_sampler.inc) and the graph, which reads them, is captured once more -- as for DDIM; after that none again.
    d.dpm_solver_sample(SHAPE, 9, 2, seed=5)
    assert u.graph_captures == n0 + 2
    assert torch.equal(d.dpm_solver_sample(SHAPE, 6, 2, seed=5).cpu(), a)
    d.dpm_solver_sample(SHAPE, 8, 1, seed=7)
    assert u.graph_captures == n0 + 2
    eager = dm.DenoisingDiffusion(u, image_size=16, timesteps=1000, use_graph=False)
    assert torch.equal(eager.dpm_solver_sample(SHAPE, 6, 2, seed=5).cpu(), a)
    assert torch.equal(eager.dpm_solver_sample(SHAPE, 6, 1, seed=5).cpu(), others[1])
    # DDIM on this handle, after the solver, against DDIM on a handle that never ran it
    fresh, _, _ = _net(1)
    want = dm.DenoisingDiffusion(fresh, image_size=16, timesteps=1000).ddim_sample(SHAPE, 6, seed=5).cpu()
    assert torch.equal(d.ddim_sample(SHAPE, 6, seed=5).cpu(), want)
    assert torch.equal(d.dpm_solver_sample(SHAPE, 6, 2, seed=5).cpu(), a)
    # two shards of one global batch
    one = (1,) + SHAPE[1:]
    shards = [d.dpm_solver_sample(one, 6, 2, seed=5, sample_offset=k).cpu() for k in (0, 1)]
    assert torch.equal(torch.cat(shards), a)


# ---- 6. launches -------------------------------------------------------------------------------------------------------
def _profiled(fn):
    _lib.profile_enable(True)
    try:
        fn()
        rows = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return {r["kernel"]: r["launches"] for r in rows}


def test_a_step_has_the_launches_of_a_ddim_step():
    u, _, _ = _net(1)
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=1000, use_graph=False)
    ddim = _profiled(lambda: d.ddim_sample(SHAPE, 2, seed=3))
    ours = _profiled(lambda: d.dpm_solver_sample(SHAPE, 2, 2, seed=3))
    assert ddim and len(ours) == len(ddim)
    assert ours == ddim, (ours, ddim)
