"""Classifier-free guidance on the GPU: the combine operator (dm_op_cfg_combine), the masked 2B forward
(dm_unet_forward_masked), Unet.forward_with_cond_scale and the guided DDIM / DDPM loops against the reference's goldens
(tests/golden/make_golden_cfg.py -> cfg_text.pt), the unguided path at cond_scale == 1, graph reuse across guidance scales,
batch and shard invariance, sampling after caption-dropout training, the refusals, and the unfused attention routes in a
child process."""
import os
import subprocess
import sys

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.spec import UnetConfig
from diffusion_models_amd.unet import cfg_combine
from oracle import sampler_oracle as so

from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.abspath(__file__))
OP_TOL = 1e-5     # the combine against the reference / the float64 restatement (fp32 output)
FWD_TOL = 1e-5    # model forward against the reference
LOOP_TOL = 2e-5   # DDIM / DDPM loops
GRID = [(s, p, r, 0.0) for s in (3.0, 6.0) for p in (0.0, 0.7) for r in (True, False)] + [(6.0, 0.7, True, 0.5),
                                                                                          (0.0, 0.0, True, 0.0)]


@pytest.fixture(scope="module")
def golden():
    return load_golden("cfg_text.pt")


def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def guided_f64(cond, null, cond_scale, rescaled_phi, remove_parallel_component, keep_parallel_frac):
    """Unet.forward_with_cond_scale's combine (DD/classifier_free_guidance.py:355-369, project :49-60), all in float64."""
    c = cond.double().flatten(1)
    update = (cond - null).double().flatten(1)
    if remove_parallel_component:
        unit = c / c.norm(dim=1, keepdim=True).clamp_min(1e-12)
        parallel = (update * unit).sum(dim=1, keepdim=True) * unit
        update = (update - parallel) + parallel * keep_parallel_frac
    scaled = c + update * (cond_scale - 1.0)
    if rescaled_phi != 0.0:
        ratio = c.std(dim=1, keepdim=True) / scaled.std(dim=1, keepdim=True)
        scaled = scaled * ratio * rescaled_phi + scaled * (1.0 - rescaled_phi)
    return scaled.reshape(cond.shape)


_UNETS = {}


def text_unet(golden, name):
    """The golden's text U-Net (synthetic weights of the recorded salt), one handle per model."""
    if name not in _UNETS:
        m = golden["models"][name]
        kw = dict(m["kwargs"])
        u = dm.Unet(device=DEV, **kw)
        u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(**kw)), salt=m["salt"]))
        _UNETS[name] = u
    return _UNETS[name]


def fwd_inputs(golden, b):
    m = golden["models"][b["model"]]["tokens"]
    side = b["side"]
    return seeded((3, 3, side, side), b["x_seed"]), b["t"], seeded((3, m, 512), b["ctx_seed"])


def masked_forward(u, x, t, ctx, mask):
    B, _, H, W = x.shape
    x, t, ctx = (v.to(DEV).contiguous() for v in (x, t, ctx))
    mask = torch.tensor(mask, dtype=torch.int32, device=DEV)
    out = torch.empty((B, u.out_dim, H, W), device=DEV)
    _lib.check(_lib.load().dm_unet_forward_masked(u._handle, _lib.ptr(x), _lib.ptr(t), _lib.ptr(ctx), ctx.shape[1],
                                                  _lib.ptr(mask), _lib.ptr(out), B, H, W, None))
    torch.cuda.synchronize()
    return out.cpu()


# ---- the combine operator ----------------------------------------------------------------------------------------------
def test_combine_op_against_golden(golden):
    for key, b in golden["fwd"].items():
        for case, want in zip(b["cases"], b["guided"]):
            got = cfg_combine(b["cond"].to(DEV), b["null"].to(DEV), *case).cpu()
            err = rel_l2(got, want)
            print(key, case, f"{err:.2e}")
            assert err < OP_TOL, (key, case, err)


@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 4, 13, 11), (1, 1, 1, 2), (3, 3, 128, 128), (2, 4, 64, 64),
                                   (5, 3, 33, 17)])
def test_combine_op_odd_sizes(shape):
    """C x H x W not a multiple of 64 (or of the workgroup), B = 1, and the largest pixel / latent images."""
    g = torch.Generator().manual_seed(sum(shape))
    cond = torch.randn(shape, generator=g)
    null = cond * 0.8 + 0.3 * torch.randn(shape, generator=g) + 0.05
    for case in GRID:
        got = cfg_combine(cond.to(DEV), null.to(DEV), *case).cpu()
        err = rel_l2(got, guided_f64(cond, null, *case))
        assert err < OP_TOL, (shape, case, err)
    # per image: image 0 of the batch alone gives the same row, bit for bit
    one = cfg_combine(cond[:1].to(DEV), null[:1].to(DEV), 6.0, 0.7, True, 0.5).cpu()
    full = cfg_combine(cond.to(DEV), null.to(DEV), 6.0, 0.7, True, 0.5).cpu()
    assert torch.equal(one[0], full[0])


# ---- the masked forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["concat_16", "cross1_16", "cross3_16", "concat_32", "cross1_32"])
def test_masked_forward_halves(golden, key):
    """[x | x] with the mask [1.. | 0..]: the conditioned half equals the B forward with text_emb, the null half the B forward
    without; a mixed mask selects per image."""
    b = golden["fwd"][key]
    u = text_unet(golden, b["model"])
    x, t, ctx = fwd_inputs(golden, b)
    B = x.shape[0]
    out2 = masked_forward(u, torch.cat((x, x)), torch.cat((t, t)), torch.cat((ctx, ctx)), [1] * B + [0] * B)
    cond = u(x.to(DEV), t.to(DEV), text_emb=ctx.to(DEV)).cpu()
    null = u(x.to(DEV), t.to(DEV)).cpu()
    ec, en = rel_l2(out2[:B], cond), rel_l2(out2[B:], null)
    print(key, f"cond {ec:.2e} (bitwise {torch.equal(out2[:B], cond)})  null {en:.2e} (bitwise {torch.equal(out2[B:], null)})")
    assert ec < 1e-6 and en < 1e-6
    assert rel_l2(cond, b["cond"]) < FWD_TOL and rel_l2(null, b["null"]) < FWD_TOL
    mixed = masked_forward(u, x, t, ctx, [0, 1, 0])
    for i, want in enumerate((null[0], cond[1], null[2])):
        assert rel_l2(mixed[i], want) < 1e-6, (key, i)


def test_forward_with_cond_scale_against_golden(golden):
    for key, b in golden["fwd"].items():
        u = text_unet(golden, b["model"])
        x, t, ctx = fwd_inputs(golden, b)
        for case, want in zip(b["cases"], b["guided"]):
            s, p, r, k = case
            g, null = u.forward_with_cond_scale(x, t, ctx, cond_scale=s, rescaled_phi=p, remove_parallel_component=r,
                                                keep_parallel_frac=k)
            eg, en = rel_l2(g.cpu(), want), rel_l2(null.cpu(), b["null"])
            print(key, case, f"guided {eg:.2e} null {en:.2e}")
            assert eg < FWD_TOL and en < FWD_TOL, (key, case)
        plain = u.forward_with_cond_scale(x, t, ctx)
        assert torch.is_tensor(plain) and torch.equal(plain.cpu(), u(x, t, text_emb=ctx).cpu())


# ---- the guided loops ------------------------------------------------------------------------------------------------
def _diffusion(golden, b, use_graph):
    u = text_unet(golden, b["model"])
    return dm.TextConditionalDenoisingDiffusion(model=u, image_size=16, timesteps=b["T"], sampling_timesteps=b["S"] or b["T"],
                                                objective=b["objective"], use_graph=use_graph)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("key", ["ddim20", "ddpm50", "ddim20_v"])
def test_guided_loops_against_golden(golden, key, use_graph):
    b = golden[key]
    d = _diffusion(golden, b, use_graph)
    s, p, r, k = b["case"]
    fn = d.ddim_sample if b["S"] else d.p_sample_loop
    y = fn(b["shape"], text_emb=b["ctx"], noise=so.NoiseStream(b["seed"]), cond_scale=s, rescaled_phi=p,
           remove_parallel_component=r, keep_parallel_frac=k).cpu()
    err = rel_l2(y, b["y"])
    print(key, use_graph, f"{err:.3e}")
    assert err < LOOP_TOL


def test_guided_p_sample_and_model_predictions(golden):
    """The callable step methods take the same keywords: one guided DDPM step equals the first step of the loop."""
    b = golden["ddpm50"]
    d = _diffusion(golden, b, False)
    s, p, r, k = b["case"]
    kw = dict(cond_scale=s, rescaled_phi=p, remove_parallel_component=r, keep_parallel_frac=k)
    noise = so.NoiseStream(b["seed"])
    x_T, z = noise(b["shape"]), noise(b["shape"])
    T = b["T"]
    img, x_start = d.p_sample(x_T, T - 1, b["ctx"], noise=lambda shape: z, **kw)
    one = d._run(dm.diffusion.DDPM, b["shape"], *[v[:1] for v in d._ddpm_tables()], [True], False,
                 _SeqNoise([x_T, z]), None, text_emb=b["ctx"], unnormalize=False, guidance=(s, p, r, k))
    assert rel_l2(img.cpu(), one.cpu()) < 1e-6
    pred = d.model_predictions(x_T, T - 1, b["ctx"], clip_x_start=True, **kw)
    assert rel_l2(pred.pred_x_start.cpu(), x_start.cpu()) < 1e-6
    unguided = d.model_predictions(x_T, T - 1, b["ctx"], clip_x_start=True)
    assert rel_l2(unguided.pred_x_start.cpu(), x_start.cpu()) > 1e-3
    mean, _, _, xs = d.p_mean_variance(x_T, T - 1, b["ctx"], **kw)
    assert rel_l2(xs.cpu(), x_start.cpu()) < 1e-6 and bool(torch.isfinite(mean).all())


class _SeqNoise:
    def __init__(self, tensors):
        self.t = list(tensors)

    def __call__(self, shape):
        return self.t.pop(0)


# ---- cond_scale == 1, graph reuse, invariance -----------------------------------------------------------------------
def _profile_run(fn):
    _lib.profile_enable(True)
    try:
        y = fn()
        rows = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return y, {r["kernel"]: (r["launches"], r["total_flops"]) for r in rows}


@pytest.mark.parametrize("cross", [False, True])
def test_cond_scale_one_is_the_unguided_path(golden, cross):
    """Bit for bit the call without the keywords, and the same launches: no null forward, no combine."""
    u = text_unet(golden, "cross1" if cross else "concat")
    d = dm.TextConditionalDenoisingDiffusion(model=u, image_size=16, timesteps=1000, sampling_timesteps=4, use_graph=False)
    ctx = seeded((2, 512), 90)
    a, pa = _profile_run(lambda: d.sample(batch_size=2, text_emb=ctx, seed=5).cpu())
    b, pb = _profile_run(lambda: d.sample(batch_size=2, text_emb=ctx, seed=5, cond_scale=1.0, rescaled_phi=0.7,
                                          remove_parallel_component=False, keep_parallel_frac=0.5).cpu())
    g, pg = _profile_run(lambda: d.sample(batch_size=2, text_emb=ctx, seed=5, cond_scale=3.0).cpu())
    assert torch.equal(a, b)
    assert pa == pb and pa, (pa, pb)
    assert "cfg_combine_kernel" not in pa and pg["cfg_combine_kernel"][0] == 4
    flops = lambda prof: sum(f for k, (n, f) in prof.items() if k != "cfg_combine_kernel")  # noqa: E731
    # one forward at 2B per step (with one context token the unguided cross model skips its bottleneck, the guided one
    # cannot: its null half needs it)
    ratio = flops(pg) / flops(pa)
    assert abs(ratio - 2.0) < 1e-9 if not cross else ratio >= 2.0, ratio
    assert not torch.equal(a, g)


def test_one_capture_across_guidance_scales(golden):
    u = text_unet(golden, "cross1")
    d = dm.TextConditionalDenoisingDiffusion(model=u, image_size=16, timesteps=1000, sampling_timesteps=5)
    ctx = seeded((3, 1, 512), 91)
    n0 = u.graph_captures
    a = d.sample(batch_size=3, text_emb=ctx, seed=9, cond_scale=3.0).cpu()
    assert u.graph_captures == n0 + 1
    b = d.sample(batch_size=3, text_emb=ctx, seed=9, cond_scale=7.5, rescaled_phi=0.7, remove_parallel_component=False).cpu()
    c = d.sample(batch_size=3, text_emb=ctx, seed=9, cond_scale=3.0).cpu()
    assert u.graph_captures == n0 + 1
    assert torch.equal(a, c) and not torch.equal(a, b)
    eager = dm.TextConditionalDenoisingDiffusion(model=u, image_size=16, timesteps=1000, sampling_timesteps=5,
                                                 use_graph=False)
    e = eager.sample(batch_size=3, text_emb=ctx, seed=9, cond_scale=7.5, rescaled_phi=0.7,
                     remove_parallel_component=False).cpu()
    assert torch.equal(e, b)


@pytest.mark.parametrize("name", ["concat", "cross1", "cross3"])
def test_guided_batch_and_shard_invariance(golden, name):
    """Guidance is per image: the first images of a larger seeded run, and the shards of a batch (sample_offset, what
    dist.sample_global passes), equal the whole run -- bit for bit where the U-Net forward is batch invariant.  The
    cross-attention core with 3 context tokens is not (its B-row and 2B-row forwards differ by ~5e-7 relative, see
    test_masked_forward_halves[cross3_16]); 4 guided steps at cond_scale 4 amplify that, so that model is held to the model
    files' 1e-4."""
    u = text_unet(golden, name)
    m = golden["models"][name]["tokens"]
    d = dm.TextConditionalDenoisingDiffusion(model=u, image_size=16, timesteps=1000, sampling_timesteps=4)
    ctx = seeded((4, m, 512), 92)
    kw = dict(cond_scale=4.0, rescaled_phi=0.5)
    whole = d.sample(batch_size=4, text_emb=ctx, seed=21, **kw).cpu()
    head = d.sample(batch_size=2, text_emb=ctx[:2], seed=21, **kw).cpu()
    tail = d.sample(batch_size=2, text_emb=ctx[2:], seed=21, sample_offset=2, **kw).cpu()
    e_head, e_tail = rel_l2(head, whole[:2]), rel_l2(tail, whole[2:])
    print(name, f"head {e_head:.2e} tail {e_tail:.2e}")
    glob = dm.sample_global(d, 4, seed=21, text_emb=ctx, **kw).cpu()
    if m == 1:
        assert torch.equal(whole[:2], head) and torch.equal(whole[2:], tail)
        assert torch.equal(glob, whole)
    else:
        assert e_head < 1e-4 and e_tail < 1e-4
        assert rel_l2(glob, whole) < 1e-4


# ---- training meets sampling -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", [False, True])
def test_guided_sampling_after_caption_dropout_training(cross):
    """A few steps trained with captions and with them dropped (text_emb=None), then guided sampling from the trained
    handle: its guided prediction is the combine of its own conditioned and null forwards."""
    kw = dict(dim=32, dim_mults=(1, 2), channels=3, text_condition=True, use_cross_attn=cross)
    u = dm.Unet(device=DEV, **kw)
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(**kw)), salt=93))
    d = dm.TextConditionalDenoisingDiffusion(model=u, image_size=16, timesteps=1000, sampling_timesteps=5).train()
    g = torch.Generator().manual_seed(94)
    emb = torch.randn((4, 512), generator=g)
    for it in range(4):
        x_start = torch.rand((4, 3, 16, 16), generator=g) * 2 - 1
        t = torch.randint(0, 1000, (4,), generator=g)
        d.p_losses(x_start, t, emb if it % 2 == 0 else None)
        u.optimizer_step(lr=1e-3)
    u.sync()
    d.eval()
    x = seeded((4, 3, 16, 16), 95)
    t = torch.tensor([3, 250, 600, 999])
    guided, null = u.forward_with_cond_scale(x, t, emb, cond_scale=5.0, rescaled_phi=0.7)
    cond = u(x, t, text_emb=emb).cpu()
    assert rel_l2(null.cpu(), u(x, t).cpu()) < 1e-6
    assert rel_l2(guided.cpu(), guided_f64(cond, null.cpu(), 5.0, 0.7, True, 0.0)) < 1e-5
    y = d.sample(batch_size=4, text_emb=emb, seed=3, cond_scale=5.0, rescaled_phi=0.7).cpu()
    y1 = d.sample(batch_size=4, text_emb=emb, seed=3).cpu()
    assert bool(torch.isfinite(y).all()) and not torch.equal(y, y1)


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals(golden):
    plain = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    plain.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(dim=32, dim_mults=(1, 2), channels=3)), salt=1))
    d = dm.TextConditionalDenoisingDiffusion(model=plain, image_size=16, timesteps=1000, sampling_timesteps=2)
    ctx = seeded((2, 512), 96)
    with pytest.raises(ValueError, match="text-conditional"):
        d.sample(batch_size=2, text_emb=ctx, cond_scale=3.0)
    with pytest.raises(ValueError, match="text-conditional"):
        plain.forward_with_cond_scale(seeded((2, 3, 16, 16), 1), torch.tensor([1, 2]), ctx, cond_scale=3.0)
    assert d.sample(batch_size=2, text_emb=ctx, seed=1, cond_scale=1.0).shape == (2, 3, 16, 16)
    x = seeded((2, 3, 16, 16), 1).to(DEV)
    with pytest.raises(RuntimeError, match="text-conditional"):
        masked_forward(plain, x, torch.tensor([1, 2]), ctx[:, None], [1, 0])
    kw = dict(dim=32, dim_mults=(1, 2), channels=3, text_condition=True, self_condition=True)
    sc = dm.Unet(device=DEV, **kw)
    sc.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(**kw)), salt=2))
    dsc = dm.TextConditionalDenoisingDiffusion(model=sc, image_size=16, timesteps=1000, sampling_timesteps=2)
    with pytest.raises(NotImplementedError, match="self_condition"):
        dsc.sample(batch_size=2, text_emb=ctx, cond_scale=3.0)
    with pytest.raises(NotImplementedError, match="self_condition"):
        dsc.model_predictions(x, 5, ctx, cond_scale=3.0)
    u = text_unet(golden, "cross1")
    with pytest.raises(ValueError, match="text_emb"):
        u.forward_with_cond_scale(x, torch.tensor([1, 2]), None, cond_scale=3.0)
    # the library refuses what the Python layer would: guidance on a handle without text conditioning
    a = _lib.SampleArgs()
    times = (torch.tensor([10], dtype=torch.int64))
    coefs = torch.zeros((1, _lib.DM_COEFS))
    out = torch.empty((2, 3, 16, 16), device=DEV)
    a.kind, a.n_steps, a.B, a.H, a.W = 1, 1, 2, 16, 16
    a.times_host = _ptr64(times)
    a.coefs_host = _ptrf(coefs)
    a.x_T, a.out = _lib.ptr(x), _lib.ptr(out)
    a.cfg, a.cfg_scale = 1, 3.0
    rc = _lib.load().dm_sample_ex(plain._handle, a)
    assert rc != 0 and "text-conditional" in _lib.load().dm_last_error().decode()


def _ptr64(t):
    import ctypes
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int64))


def _ptrf(t):
    import ctypes
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def test_unfused_attention_routes():
    """The operator, masked-forward and golden cases with the fused LinearAttention and attn16 kernels switched off, in a
    child process (the switches are read once per process)."""
    env = dict(os.environ, DM_NO_FUSED_LINATTN="1", DM_NO_ATTN16="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "combine_op or masked_forward or forward_with_cond_scale or loops_against_golden", "-p",
                        "no:cacheprovider"], cwd=os.path.dirname(ROOT), env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
