"""Per-image caption dropout without a device: the mask draw, train_step's argument handling on a stub diffusion object,
and the golden (tests/golden/make_golden_cfg_train.py -> cfg_train.pt) recomputed with oracle.train_oracle on sub-batches."""
import math

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.diffusion import prob_mask_like
from diffusion_models_amd.spec import UnetConfig

from conftest import check_grad_digest, load_golden


# ---- the mask draw -----------------------------------------------------------------------------------------------------------
def test_mask_draw_edges_seed_and_rate():
    assert prob_mask_like((7,), 1).dtype == torch.bool and bool(prob_mask_like((7,), 1).all())
    assert prob_mask_like((7,), 1.0).shape == (7,) and not bool(prob_mask_like((7,), 0).any())
    # the edge cases draw nothing from the generator, as in the reference (classifier_free_guidance.py:41-47)
    torch.manual_seed(3)
    a = torch.rand(4)
    torch.manual_seed(3)
    prob_mask_like((9,), 1), prob_mask_like((9,), 0)
    assert torch.equal(a, torch.rand(4))
    torch.manual_seed(5)
    m1 = prob_mask_like((64,), 0.5)
    torch.manual_seed(5)
    m2 = prob_mask_like((64,), 0.5)
    assert torch.equal(m1, m2) and bool(m1.any()) and not bool(m1.all())
    # the draw is uniform_(0, 1) < prob of the global CPU generator
    torch.manual_seed(5)
    assert torch.equal(m1, torch.zeros((64,)).float().uniform_(0, 1) < 0.5)
    # keep rate of a large draw: binomial(n, p), bound of 6 standard deviations (a false alarm has probability ~2e-9)
    n, p = 200_000, 0.7
    torch.manual_seed(7)
    k = int(prob_mask_like((n,), p).sum())
    assert abs(k - n * p) <= 6.0 * math.sqrt(n * p * (1 - p)), k


# ---- train_step ------------------------------------------------------------------------------------------------------------
class _StubUnet:
    def optimizer_step(self, **kw):
        return 1.0


class _StubDiffusion:
    """Records what train_step passes to p_losses."""
    device = "cpu"
    num_timesteps = 1000

    def __init__(self):
        self.model = _StubUnet()
        self.calls = []

    def normalize(self, x):
        return x * 2 - 1

    def p_losses(self, x, t, **kw):
        self.calls.append(dict(kw, x=x, t=t))
        return torch.tensor(0.5)


def test_train_step_micro_batches_and_masks():
    img, emb = torch.rand(4, 3, 8, 8), torch.randn(4, 512)
    d = _StubDiffusion()
    dm.train_step(d, [img, img])  # image tensors, as before: nothing new reaches p_losses
    assert [sorted(c) for c in d.calls] == [["accumulate", "loss_scale", "noise", "t", "x"]] * 2
    assert [c["accumulate"] for c in d.calls] == [False, True] and d.calls[0]["loss_scale"] == 0.5
    d = _StubDiffusion()
    mask = torch.tensor([1, 0, 1, 1])
    total, norm = dm.train_step(d, [(img, emb), img, [img, emb]], text_mask=[mask, None, None])
    assert total == 1.5 and norm == 1.0
    assert d.calls[0]["text_emb"] is emb and d.calls[0]["text_mask"] is mask
    assert "text_emb" not in d.calls[1] and "text_mask" not in d.calls[1]
    assert d.calls[2]["text_emb"] is emb and "text_mask" not in d.calls[2]
    assert torch.equal(d.calls[0]["x"], img * 2 - 1)
    with pytest.raises(ValueError, match="micro-batches"):
        dm.train_step(_StubDiffusion(), [(img, emb)], text_mask=[mask, mask])
    with pytest.raises(ValueError, match="without text_emb"):
        dm.train_step(_StubDiffusion(), [img], text_mask=[mask])
    with pytest.raises(ValueError, match="pair"):
        dm.train_step(_StubDiffusion(), [(img, emb, emb)])


def test_binding_keeps_the_struct_and_adds_the_masked_call():
    """dm_train_args is what it was (an unmasked caller passes the same bytes); the mask travels as an argument of a new
    entry point."""
    assert [f[0] for f in _lib.TrainArgs._fields_][-2:] == ["loss_terms", "kl_scale"]
    assert "dm_unet_loss_backward_masked" in _lib.EXPORTS


# ---- the golden ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["concat", "cross1", "cross3"])
def test_golden_is_the_composition_of_sub_batches(case):
    """oracle.train_oracle on the kept sub-batch (with captions) and the dropped one (text_emb=None), combined per image,
    reproduces the reference's golden within the oracle's usual agreement (tests/test_oracle_golden.py: loss 1e-5,
    digests 2e-5)."""
    from oracle import train_oracle as to

    b = load_golden("cfg_train.pt")[case]
    cfg = UnetConfig(**b["kwargs"])
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=b["salt"])
    sched = dm.make_schedule(b["T"], "linear")
    mask = b["mask"].bool()
    B, n_k, n_d = mask.numel(), int(mask.sum()), int((~mask).sum())
    assert n_k >= 2 and n_d >= 2 and b["emb"].shape[0] == B and (b["emb"].dim() == 3) == (b["tokens"] > 1)
    x_start = b["img"] * 2 - 1
    torch.set_num_threads(8)
    k, d = mask, ~mask
    lk, gk = to.loss_and_grads(sd, cfg, sched, x_start[k], b["t"][k], b["noise"][k], text_emb=b["emb"][k])
    ld, gd = to.loss_and_grads(sd, cfg, sched, x_start[d], b["t"][d], b["noise"][d])
    loss = (n_k * lk + n_d * ld) / B
    assert abs(loss - b["loss"]) <= 1e-5 * abs(b["loss"]), (loss, b["loss"])
    assert set(gk) == set(b["grads"])
    scale = max(dg["norm"] for dg in b["grads"].values())
    for name, dg in b["grads"].items():
        g = (n_k * gk[name].double() + n_d * gd[name].double()) / B
        if dg["norm"] < 1e-9 * scale:  # exact zeros in the reference (single context token)
            assert float(g.norm()) < 1e-6 * scale, name
        else:
            check_grad_digest(name, g, dg, 2e-5)
    if case == "cross3":  # with three tokens the CrossAttention's query path carries gradient
        assert b["grads"]["cross_attn.to_q.weight"]["norm"] > 1e-6 * scale
