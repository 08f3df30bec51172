"""Per-image caption dropout in one training batch (``p_losses(text_mask=...)`` / ``cond_drop_prob``,
dm_unet_loss_backward_masked) on the GPU: a mixed mask against the reference's golden (tests/golden/make_golden_cfg_train.py
-> cfg_train.pt), the all-ones / all-zeros masks against the unmasked calls bit for bit, per-image independence, the
unmasked path's launches, self-conditioning and the hybrid loss, train -> guided sampling end to end, the refusals."""
import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.spec import UnetConfig

from conftest import check_grad_digest, load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_TOL = 2e-4  # the constant of tests/test_hip_train.py


@pytest.fixture(scope="module")
def golden():
    return load_golden("cfg_train.pt")


def is_text(name):
    return name.startswith(("text_", "cross_attn"))


def text_model(cross, salt=None, **kw):
    """The small text U-Net of tests/test_hip_train.py in training mode (keywords: Unet's, then the diffusion class's)."""
    ukw = dict(dim=32, dim_mults=(1, 2), channels=3, text_condition=True, use_cross_attn=cross)
    for k in ("self_condition", "dropout"):
        if k in kw:
            ukw[k] = kw.pop(k)
    cfg = UnetConfig(**{k: v for k, v in ukw.items() if k != "dropout"})
    u = dm.Unet(device=DEV, **ukw)
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=(2 if cross else 3) if salt is None else salt))
    kw.setdefault("timesteps", 1000)
    return dm.TextConditionalDenoisingDiffusion(model=u, image_size=16, **kw).train()


def batch(B, seed, tokens=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 3, 16, 16), generator=g) * 2 - 1
    t = torch.randint(1, 1000, (B,), generator=g)  # no t = 0: the hybrid loss is NaN there, as in the reference
    noise = torch.randn((B, 3, 16, 16), generator=g)
    emb = torch.randn((B, tokens, 512), generator=g) if tokens > 1 else torch.randn((B, 512), generator=g)
    return x, t, noise, emb


def grads_of(d):
    return {k: v.cpu() for k, v in d.model.grads().items()}


def same_bits(a, b, names=None):
    for k in (names if names is not None else a):
        assert torch.equal(a[k], b[k]), k


# ---- 1. the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["concat", "cross1", "cross3"])
def test_mixed_mask_vs_reference_golden(golden, case):
    """Loss and every gradient of a batch with mask [1, 0, 1, 1, 0] against the reference's own p_losses(...).backward()
    on the kept sub-batch (with captions) and the dropped one (text_emb=None), combined per image.  ``cross3`` has three
    context tokens: the CrossAttention's own input gradient is non-zero for the kept rows."""
    b = golden[case]
    d = text_model(b["kwargs"]["use_cross_attn"], salt=b["salt"], timesteps=b["T"])
    loss = float(d.p_losses(b["img"] * 2 - 1, b["t"], b["emb"], b["noise"], text_mask=b["mask"]))
    print(case, "loss", loss, b["loss"], "all captions", b["loss_all_captions"])
    assert abs(loss - b["loss"]) <= 1e-5 * abs(b["loss"])
    assert abs(b["loss"] - b["loss_all_captions"]) > 1e-4 * abs(b["loss"])  # the mask matters in this golden
    grads = grads_of(d)
    assert set(grads) == set(b["grads"])
    scale = max(dg["norm"] for dg in b["grads"].values())
    for name, dg in b["grads"].items():
        if dg["norm"] < 1e-9 * scale:  # exact zeros in the reference (to_q / to_k with a single context token)
            assert float(grads[name].norm()) < 1e-6 * scale, name
        else:
            check_grad_digest(name, grads[name], dg, GRAD_TOL)


# ---- 2., 3. the two uniform masks, plain / self-conditioned / hybrid (6.) -------------------------------------------------
MODES = {
    "plain": {},
    "self_cond": dict(self_condition=True),
    "hybrid": dict(hybrid_loss=True),
    "hybrid_dropout": dict(hybrid_loss=True, dropout=0.1),
}


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_uniform_masks_are_the_unmasked_calls_bitwise(cross, mode):
    """A mask of ones is the call without a mask; a mask of zeros is the text_emb=None call with exactly zero text
    gradients -- loss and gradients bit for bit.  For self-conditioning (the gradient-free pass forced on) and the hybrid
    loss these invariances are the check: oracle.train_oracle's gradient-free pass takes no text_emb, and the KL
    normaliser couples the batch, so neither composes over sub-batches.  With dropout the handle's mask counter advances per
    call, so every compared call starts from a fresh handle with the same dropout seed."""
    kw = dict(MODES[mode])
    B = 4
    x, t, noise, emb = batch(B, 71, tokens=3 if cross else 1)
    call_kw = dict(self_cond=True) if mode == "self_cond" else {}

    def run(text, mask):
        d = text_model(cross, **dict(kw))
        if "dropout" in kw:
            d.model.set_dropout_seed(1234)
        loss = float(d.p_losses(x, t, text, noise, text_mask=mask, **call_kw))
        return loss, grads_of(d)

    l_text, g_text = run(emb, None)
    l_ones, g_ones = run(emb, torch.ones(B, dtype=torch.int32))
    assert l_ones == l_text and l_text == l_text
    same_bits(g_text, g_ones)
    l_none, g_none = run(None, None)
    l_zero, g_zero = run(emb, torch.zeros(B, dtype=torch.bool))
    assert l_zero == l_none and l_none != l_text
    same_bits(g_none, g_zero, [k for k in g_none if not is_text(k)])
    text_names = [k for k in g_zero if is_text(k)]
    assert text_names
    for k in text_names:
        assert float(g_zero[k].abs().sum()) == 0.0, k
    # a mixed mask: finite, and neither of the two
    l_mix, g_mix = run(emb, torch.tensor([1, 0, 0, 1]))
    assert l_mix == l_mix and l_mix not in (l_text, l_none)
    assert all(bool(torch.isfinite(v).all()) for v in g_mix.values())


# ---- 4. per-image independence -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["concat", "cross_m1", "cross_m3", "hybrid_mse_part"])
def test_mixed_batch_is_the_sum_of_its_sub_batches(variant):
    """Plain MSE loss: the gradient of a mixed batch equals the accumulate=True sum of the kept sub-batch with captions and
    the dropped sub-batch with text_emb=None, each with loss_scale = n / B.  ``hybrid_mse_part``: the same for the MSE part
    (loss_terms = 1) of a hybrid_loss model's call, taken through the C ABI."""
    import ctypes as C

    cross = variant != "concat"
    B = 6
    x, t, noise, emb = batch(B, 72, tokens=3 if variant == "cross_m3" else 1)
    mask = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.bool)
    d = text_model(cross)
    if variant == "hybrid_mse_part":
        # what p_losses of a hybrid_loss model passes, with loss_terms forced to 1
        lib = _lib.load()
        xs, ns, ctx = x.to(DEV).contiguous(), noise.to(DEV).contiguous(), emb[:, None].to(DEV).contiguous()
        coef = d._tcoef(t)
        loss = C.c_float(0.0)
        a = _lib.TrainArgs()
        a.x_start, a.noise, a.ctx = _lib.ptr(xs), _lib.ptr(ns), _lib.ptr(ctx)
        t_arr = (C.c_int64 * B)(*t.tolist())
        a.t_host = C.cast(t_arr, C.POINTER(C.c_int64))
        a.coef_host, a.coef_stride = C.cast(coef.data_ptr(), C.POINTER(C.c_float)), int(coef.shape[1])
        a.ctx_tokens, a.objective, a.loss_scale, a.loss_terms = 1, d._objective_id, 1.0, 1
        a.loss_out_host, a.B, a.H, a.W = C.pointer(loss), B, 16, 16
        m_arr = (C.c_int32 * B)(*[int(v) for v in mask.tolist()])
        _lib.check(lib.dm_unet_loss_backward_masked(d.model._handle, C.byref(a), m_arr))
        l_mix = loss.value
    else:
        l_mix = float(d.p_losses(x, t, emb, noise, text_mask=mask))
    g_mix = grads_of(d)
    k, dr = mask, ~mask
    n_k, n_d = int(k.sum()), int(dr.sum())
    l_sum = float(d.p_losses(x[k], t[k], emb[k], noise[k], loss_scale=n_k / B))
    l_sum += float(d.p_losses(x[dr], t[dr], None, noise[dr], loss_scale=n_d / B, accumulate=True))
    g_sum = grads_of(d)
    print(variant, "loss", l_mix, l_sum)
    assert abs(l_mix - l_sum) <= 1e-5 * abs(l_sum)
    scale = max(float(v.norm()) for v in g_sum.values())
    for name, w in g_sum.items():
        if float(w.norm()) < 1e-9 * scale:
            assert float(g_mix[name].norm()) < 1e-6 * scale, name
        else:
            assert rel_l2(g_mix[name], w) < GRAD_TOL, (name, rel_l2(g_mix[name], w))


# ---- 5. no mask, no change -------------------------------------------------------------------------------------------------
def _profile_run(fn):
    _lib.profile_enable(True)
    try:
        y = fn()
        rows = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    return y, {r["kernel"]: r["launches"] for r in rows}


@pytest.mark.parametrize("cross", [False, True])
def test_no_mask_is_the_unmasked_path(cross):
    """An unmasked p_losses -- no keyword, or cond_drop_prob = 0 spelled out -- runs no routing launch and the same profiled
    launches as before; the masked call adds two routing launches (concat) or six (cross) and nothing else.  Image-only
    train_step iterations on a model built with cond_drop_prob > 0 are bit for bit those of one built without."""
    d = text_model(cross)
    x, t, noise, emb = batch(4, 73)
    (l0, g0), p0 = _profile_run(lambda: (float(d.p_losses(x, t, emb, noise)), grads_of(d)))
    (l1, g1), p1 = _profile_run(lambda: (float(d.p_losses(x, t, emb, noise, cond_drop_prob=0.0)), grads_of(d)))
    (_, _), pm = _profile_run(lambda: (float(d.p_losses(x, t, emb, noise, text_mask=[1, 0, 1, 0])), grads_of(d)))
    assert p0 and p0 == p1 and "route_rows_kernel" not in p0
    assert l0 == l1
    same_bits(g0, g1)
    assert pm.pop("route_rows_kernel") == (6 if cross else 2)
    assert pm == p0
    imgs = [torch.rand((4, 3, 16, 16), generator=torch.Generator().manual_seed(s)) for s in (1, 2)]
    ts = [torch.tensor([5, 300, 600, 900]), torch.tensor([7, 100, 500, 990])]
    ns = [batch(4, 80 + s)[2] for s in (1, 2)]
    out = []
    for p in (0.0, 0.5):
        dd = text_model(cross, cond_drop_prob=p)
        res = [dm.train_step(dd, [imgs[i]], lr=1e-3, t=[ts[i]], noise=[ns[i]]) for i in range(2)]
        out.append((res, {k: v.cpu() for k, v in dd.model.state_dict().items()}))
    assert out[0][0] == out[1][0]
    same_bits(out[0][1], out[1][1])


# ---- 7. end to end -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", [False, True])
def test_guided_sampling_after_per_image_caption_dropout_training(cross):
    """A few train_step iterations on (images, text_emb) micro-batches with cond_drop_prob = 0.5 under a fixed seed, EMA
    on, then guided sampling from the trained weights: finite, in range, different from cond_scale = 1, and reproducible."""
    def run():
        d = text_model(cross, salt=93, cond_drop_prob=0.5, sampling_timesteps=5)
        ema = dm.EMA(d, beta=0.995, update_every=1, update_after_step=1)
        torch.manual_seed(11)
        g = torch.Generator().manual_seed(94)
        emb = torch.randn((8, 512), generator=g)
        losses = []
        for _ in range(4):
            img = torch.rand((8, 3, 16, 16), generator=g)
            loss, norm = dm.train_step(d, [(img[:4], emb[:4]), (img[4:], emb[4:])], lr=1e-3, ema=ema)
            assert loss == loss and norm == norm and loss > 0
            losses.append(loss)
        return d, ema, emb, losses

    d, ema, emb, losses = run()
    d2, _, _, losses2 = run()
    assert losses == losses2  # torch.manual_seed fixes timesteps, noise seeds and the caption masks
    d.model.sync()
    y3 = d.sample(batch_size=4, text_emb=emb[:4], seed=3, cond_scale=3.0).cpu()
    y1 = d.sample(batch_size=4, text_emb=emb[:4], seed=3).cpu()
    assert bool(torch.isfinite(y3).all()) and float(y3.min()) >= 0.0 and float(y3.max()) <= 1.0
    assert not torch.equal(y3, y1)
    e3 = ema.ema_model.sample(batch_size=4, text_emb=emb[:4], seed=3, cond_scale=3.0).cpu()
    assert bool(torch.isfinite(e3).all()) and float(e3.min()) >= 0.0 and float(e3.max()) <= 1.0


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals():
    d = text_model(False)
    x, t, noise, emb = batch(4, 74)
    with pytest.raises(ValueError, match="text_emb"):
        d.p_losses(x, t, None, noise, text_mask=[1, 0, 1, 0])
    with pytest.raises(RuntimeError, match="entries"):
        d.p_losses(x, t, emb, noise, text_mask=[1, 0, 1])
    with pytest.raises(ValueError, match="cond_drop_prob"):
        d.p_losses(x, t, emb, noise, cond_drop_prob=1.5)
    with pytest.raises(ValueError, match="cond_drop_prob"):
        text_model(False, cond_drop_prob=-0.1)
    plain = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    plain.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(dim=32, dim_mults=(1, 2), channels=3)), salt=1))
    dp = dm.TextConditionalDenoisingDiffusion(model=plain, image_size=16, timesteps=1000).train()
    with pytest.raises(ValueError, match="text-conditional"):
        dp.p_losses(x, t, emb, noise, text_mask=[1, 0, 1, 0])
    with pytest.raises(ValueError, match="micro-batches"):
        dm.train_step(d, [(x, emb)], text_mask=[[1, 0, 1, 0], [1, 1, 1, 1]])
    with pytest.raises(ValueError, match="without text_emb"):
        dm.train_step(d, [x], text_mask=[[1, 0, 1, 0]])
    # cond_drop_prob = 1 drops every caption: the text_emb=None call
    l_all = float(d.p_losses(x, t, emb, noise, cond_drop_prob=1.0))
    g_all = grads_of(d)
    assert l_all == float(d.p_losses(x, t, None, noise))
    same_bits(g_all, grads_of(d), [k for k in g_all if not is_text(k)])
