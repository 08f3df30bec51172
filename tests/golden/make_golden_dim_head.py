#!/usr/bin/env python3
"""64-wide attention heads, goldens from the REFERENCE (build container only):
``python tests/golden/make_golden_dim_head.py`` -> ``dim_head.pt``.

Every model here is built with ``attn_dim_head=64``, which the reference passes to every LinearAttention, Attention, mid_attn
and CrossAttention (DD/denoising_diffusion.py:248,295,318,324,335, DD/denoising_diffusion_text_conditional.py:97,123-125):

* ``unet_a16`` / ``unet_a32``: ``Unet(dim=32, dim_mults=(1, 2, 4))`` forward at 16x16 and 32x32, B = 3 (LinearAttention at
  1024 / 256 / 64 tokens, full attention on 4x4 / 8x8 maps);
* ``unet_bench``: the benchmark architecture ``Unet(dim=64, dim_mults=(1, 2, 4, 8))`` at 32x32, B = 2;
* ``stage_heads``: ``attn_heads=(2, 4, 8)`` with width 64: forward, ``p_losses`` + ``backward()`` (loss and a digest of every
  parameter gradient: its norm, the 8 random projections of train.pt / r4.pt and its first 64 elements, packed into one
  tensor per field -- see ``pack``);
* ``train_a16``: ``p_losses`` + ``backward()`` of the ``unet_a16`` model;
* ``text_cross`` / ``text_cross_m3`` / ``text_concat``: the text-conditional U-Net with cross-attention (1 and 3 context
  tokens) and the concat variant, forward; ``train_text_cross``: loss and gradient digests of the cross-attention model
  (3 context tokens);
* ``ddim20`` / ``ddpm50``: a DDIM-20 loop and a T = 50 DDPM loop of the ``unet_a16`` model on injected noise.
Only DATA is written."""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, patched_noise, save, seeded  # noqa: E402
from make_golden_train import digest  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402
from diffusion_models_amd.spec import UnetConfig  # noqa: E402

DH = 64
HEAD = 64  # leading elements of each gradient kept in the digest


def pack(grads: dict) -> dict:
    """Gradient digests of one model as a few tensors (one file entry per field, not three per parameter):
    ``names``, ``norm`` (P,), ``proj`` (P, 8), and the first ``HEAD`` elements of every gradient concatenated in ``head`` with
    their counts in ``head_len``.  tests/test_hip_dim_head.py unpacks them into check_grad_digest's dicts."""
    names = list(grads)
    heads = [grads[k]["head"][:HEAD] for k in names]
    return dict(names=names, norm=torch.tensor([grads[k]["norm"] for k in names], dtype=torch.float64),
                proj=torch.stack([grads[k]["proj"] for k in names]), head=torch.cat(heads),
                head_len=torch.tensor([h.numel() for h in heads], dtype=torch.int64))


def _train(dd, net, side, seed, text_emb=None, text_p_losses=None):
    diff = dd.DenoisingDiffusion(net, image_size=side, timesteps=1000).train()
    img = torch.rand((3, 3, side, side), generator=torch.Generator().manual_seed(seed))
    tt = torch.tensor([0, 500, 999])
    noise = seeded((3, 3, side, side), seed + 1)
    if text_p_losses is None:
        loss = diff.p_losses(diff.normalize(img), tt, noise=noise.clone())
    else:  # the text-conditional p_losses (its own positional order: x_start, t, text_emb, noise)
        loss = text_p_losses(diff, diff.normalize(img), tt, text_emb=text_emb, noise=noise.clone())
    loss.backward()
    return dict(img=img, tt=tt, noise=noise, loss=float(loss),
                grads=pack({k: digest(k, p.grad) for k, p in net.named_parameters()}))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    dd, ddt, _ = import_reference()
    out = {"dim_head": DH}

    cfg = UnetConfig(dim=32, dim_mults=(1, 2, 4), channels=3, attn_dim_head=DH)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=61)
    net = dd.Unet(dim=32, dim_mults=(1, 2, 4), channels=3, attn_dim_head=DH)
    net.load_state_dict(sd, strict=True)
    net.eval()
    t = torch.tensor([0, 417, 999])
    for side, seed in ((16, 160), (32, 161)):
        x = seeded((3, 3, side, side), seed)
        with torch.inference_mode():
            y = net(x, t)
        out[f"unet_a{side}"] = dict(x=x, t=t, y=y, salt=61)
        print(f"unet_a{side}", float(y.abs().mean()))
    diff = dd.DenoisingDiffusion(net, image_size=16, timesteps=1000).eval()
    with patched_noise(dd, 162), torch.inference_mode():
        out["ddim20"] = dict(seed=162, shape=(2, 3, 16, 16), S=20,
                             y=diff.ddim_sample((2, 3, 16, 16), sampling_timesteps=20))
    diff50 = dd.DenoisingDiffusion(net, image_size=16, timesteps=50).eval()
    with patched_noise(dd, 163), torch.inference_mode():
        out["ddpm50"] = dict(seed=163, shape=(2, 3, 16, 16), T=50, y=diff50.p_sample_loop((2, 3, 16, 16)))
    print("loops", float(out["ddim20"]["y"].abs().mean()), float(out["ddpm50"]["y"].abs().mean()))
    out["train_a16"] = _train(dd, net, 16, 164)
    print("train_a16", out["train_a16"]["loss"])

    bcfg = UnetConfig(dim=64, dim_mults=(1, 2, 4, 8), channels=3, attn_dim_head=DH)
    bnet = dd.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, attn_dim_head=DH).eval()
    bnet.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(bcfg), salt=62), strict=True)
    x = seeded((2, 3, 32, 32), 165)
    tb = torch.tensor([5, 760])
    with torch.inference_mode():
        out["unet_bench"] = dict(x=x, t=tb, y=bnet(x, tb), salt=62)
    print("unet_bench", float(out["unet_bench"]["y"].abs().mean()))

    heads = (2, 4, 8)
    hcfg = UnetConfig(dim=32, dim_mults=(1, 2, 4), channels=3, attn_heads=heads, attn_dim_head=DH)
    hnet = dd.Unet(dim=32, dim_mults=(1, 2, 4), channels=3, attn_heads=heads, attn_dim_head=DH)
    hnet.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(hcfg), salt=63), strict=True)
    x = seeded((2, 3, 16, 16), 166)
    th = torch.tensor([3, 871])
    with torch.inference_mode():
        y = hnet.eval()(x, th)
    out["stage_heads"] = dict(x=x, t=th, y=y, heads=heads, salt=63, **_train(dd, hnet, 16, 167))
    print("stage_heads", float(y.abs().mean()), out["stage_heads"]["loss"])

    tcfg = UnetConfig(dim=32, dim_mults=(1, 2), channels=3, text_condition=True, use_cross_attn=True, attn_dim_head=DH)
    tnet = ddt.Unet(dim=32, dim_mults=(1, 2), channels=3, text_condition=True, use_cross_attn=True, attn_dim_head=DH).eval()
    tnet.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(tcfg), salt=64), strict=True)
    ccfg = UnetConfig(dim=32, dim_mults=(1, 2), channels=3, text_condition=True, use_cross_attn=False, attn_dim_head=DH)
    cnet = ddt.Unet(dim=32, dim_mults=(1, 2), channels=3, text_condition=True, use_cross_attn=False, attn_dim_head=DH).eval()
    cnet.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(ccfg), salt=65), strict=True)
    x = seeded((2, 3, 16, 16), 168)
    tt = torch.tensor([11, 640])
    ctx1, ctx3 = seeded((2, 1, 512), 169), seeded((2, 3, 512), 170)
    with torch.inference_mode():
        out["text_cross"] = dict(x=x, t=tt, ctx=ctx1, y=tnet(x, tt, text_emb=ctx1), salt=64)
        out["text_cross_m3"] = dict(x=x, t=tt, ctx=ctx3, y=tnet(x, tt, text_emb=ctx3), salt=64)
        out["text_concat"] = dict(x=x, t=tt, ctx=ctx1, y=cnet(x, tt, text_emb=ctx1), salt=65)
    emb = seeded((3, 3, 512), 171)  # 3 context tokens: with one, the gradients of to_k are exactly zero
    out["train_text_cross"] = dict(ctx=emb, **_train(dd, tnet.train(), 16, 172, text_emb=emb,
                                                     text_p_losses=ddt.TextConditionalDenoisingDiffusion.p_losses))
    print("text", float(out["text_cross"]["y"].abs().mean()), out["train_text_cross"]["loss"])
    save("dim_head.pt", out)


if __name__ == "__main__":
    main()
