#!/usr/bin/env python3
"""Cost of per-image caption dropout in one training iteration (loss + backward, clip, Adam), one process.

  python tools/cfg_train_time.py [--iters 20] [--reps 5] [--json OUT]

Two text-conditional models: the benchmark architecture (dim 64, mults (1, 2, 4, 8), 32x32) as a concat text model at
B = 64, and config 5's shape (the same U-Net with cross-attention at 64x64, one context token) at B = 32.  For each:
ms per iteration unmasked (cond_drop_prob = 0) and masked (cond_drop_prob = 0.5), as the median over --reps windows of
--iters back-to-back iterations, the two alternating; the spread of the windows is reported as the noise.  The new
routing kernel's time comes from dm_profile brackets of one masked loss + backward (kernel execution time).  Running the
same script on the parent commit gives the parent's unmasked figure (its masked leg is skipped: no cond_drop_prob).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402
from diffusion_models_amd import _lib  # noqa: E402

DEV = "cuda:0"


def build(cross, side, drop):
    u = dm.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, text_condition=True, use_cross_attn=cross, device=DEV)
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
    kw = {"cond_drop_prob": drop} if drop else {}
    return dm.TextConditionalDenoisingDiffusion(model=u, image_size=side, timesteps=1000, **kw).train()


def iteration(d, img, emb, **kw):
    """What train_step does with one (images, text_emb) micro-batch, spelled out so that the parent commit runs it too."""
    t = torch.randint(0, d.num_timesteps, (img.shape[0],)).long()
    d.p_losses(d.normalize(img), t, emb, **kw)
    d.model.optimizer_step(lr=2e-4, **kw)


def window_ms(d, img, emb, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        iteration(d, img, emb, sync=False)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def measure(name, cross, side, batch, iters, reps, masked_ok):
    g = torch.Generator().manual_seed(0)
    img = torch.rand((batch, 3, side, side), generator=g).to(DEV)
    emb = torch.randn((batch, 512), generator=g).to(DEV)
    legs = {"unmasked": build(cross, side, 0.0)}
    if masked_ok:
        legs["masked"] = build(cross, side, 0.5)
    torch.manual_seed(0)
    for d in legs.values():  # warm-up: workspace sizing (both masks shapes), re-pack, clocks
        for _ in range(3):
            iteration(d, img, emb)
    res = {k: [] for k in legs}
    for _ in range(reps):
        for k, d in legs.items():
            res[k].append(window_ms(d, img, emb, iters))
    out = {"config": dict(model=name, cross_attn=cross, size=side, batch=batch, dim=64, dim_mults=[1, 2, 4, 8],
                          iters_per_window=iters, windows=reps)}
    for k, v in res.items():
        out[f"{k}_ms"] = statistics.median(v)
        out[f"{k}_windows_ms"] = [round(x, 3) for x in v]
        out[f"{k}_spread"] = (max(v) - min(v)) / statistics.median(v)
    if masked_ok:
        out["masked_over_unmasked"] = out["masked_ms"] / out["unmasked_ms"]
        d = legs["masked"]
        t = torch.randint(1, 1000, (batch,))
        mask = torch.arange(batch) % 2
        d.p_losses(d.normalize(img), t, emb, text_mask=mask)
        _lib.profile_enable(True)
        try:
            d.p_losses(d.normalize(img), t, emb, text_mask=mask)
            rows = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
        r = [r for r in rows if r["kernel"] == "route_rows_kernel"][0]
        out["route_rows_launches"] = r["launches"]
        out["route_rows_total_ms"] = r["total_ms"]
        out["route_rows_share_of_masked_iteration"] = r["total_ms"] / out["masked_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", help="write the results here")
    a = ap.parse_args()
    import inspect
    masked_ok = "cond_drop_prob" in inspect.signature(dm.TextConditionalDenoisingDiffusion.__init__).parameters
    out = {"bench_arch_concat_32x32_b64": measure("bench_concat", False, 32, 64, a.iters, a.reps, masked_ok),
           "config5_cross_64x64_b32": measure("config5", True, 64, 32, a.iters, a.reps, masked_ok)}
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
