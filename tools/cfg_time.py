#!/usr/bin/env python3
"""Classifier-free guidance step time (graph-replayed DDIM steps, after warm-up, in one process).

  python tools/cfg_time.py [--steps 20] [--json OUT]

Two text-conditional models:
  * config 5: Unet(dim=64, dim_mults=(1, 2, 4, 8), text_condition=True, use_cross_attn=True) at 64x64, B = 32, one context
    token (the reference's sampler passes pooled (B, 512) embeddings);
  * the benchmark architecture (dim 64, mults (1, 2, 4, 8), 32x32) as a concat text model, B = 256.
For each: ms per step unguided at B, unguided at 2B, guided at B (cond_scale 3, rescaled_phi 0.7: the combine's three-pass
form), and the combine kernel alone (dm_profile brackets of an eager run: kernel execution time).  The expectation is
guided at B ~= unguided at 2B, and the combine <= ~1 % of a guided step.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402
from diffusion_models_amd import _lib  # noqa: E402

GUIDE = dict(cond_scale=3.0, rescaled_phi=0.7)


def build(cross):
    u = dm.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, text_condition=True, use_cross_attn=cross, device="cuda:0")
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
    return u


def step_ms(d, batch, emb, steps, warmup, **kw):
    for i in range(warmup):
        d.sample(batch_size=batch, text_emb=emb[:batch], seed=1 + i, **kw)
    torch.cuda.synchronize()
    reps = 3
    t0 = time.perf_counter()
    for i in range(reps):
        d.sample(batch_size=batch, text_emb=emb[:batch], seed=100 + i, **kw)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / (reps * steps)


def combine_ms(u, side, batch, emb):
    """Kernel time of cfg_combine_kernel per step from an eager 4-step guided run under dm_profile."""
    d = dm.TextConditionalDenoisingDiffusion(model=u, image_size=side, timesteps=1000, sampling_timesteps=4, use_graph=False)
    d.sample(batch_size=batch, text_emb=emb[:batch], seed=1, **GUIDE)
    _lib.profile_enable(True)
    try:
        d.sample(batch_size=batch, text_emb=emb[:batch], seed=2, **GUIDE)
        rows = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    r = [r for r in rows if r["kernel"] == "cfg_combine_kernel"][0]
    return r["total_ms"] / r["launches"]


def measure(name, cross, side, batch, steps, warmup):
    u = build(cross)
    emb = torch.randn((2 * batch, 512), generator=torch.Generator().manual_seed(0)).to("cuda:0")
    d = dm.TextConditionalDenoisingDiffusion(model=u, image_size=side, timesteps=1000, sampling_timesteps=steps)
    res = {}
    for _ in range(2):  # interleaved twice: clocks ramp over the first launches of a process
        for key, b, kw in (("unguided_B", batch, {}), ("unguided_2B", 2 * batch, {}), ("guided_B", batch, GUIDE)):
            res.setdefault(key, []).append(step_ms(d, b, emb, steps, warmup, **kw))
    out = {f"{k}_step_ms": min(v) for k, v in res.items()}
    out["combine_kernel_ms"] = combine_ms(u, side, batch, emb)
    out["guided_over_unguided_2B"] = out["guided_B_step_ms"] / out["unguided_2B_step_ms"]
    out["combine_share_of_guided_step"] = out["combine_kernel_ms"] / out["guided_B_step_ms"]
    out["config"] = dict(model=name, cross_attn=cross, size=side, batch=batch, dim=64, dim_mults=[1, 2, 4, 8],
                         ddim_steps=steps, graph=True, guidance=GUIDE)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", help="write the results here")
    a = ap.parse_args()
    out = {"config5_cross_64x64_b32": measure("config5", True, 64, 32, a.steps, a.warmup),
           "bench_arch_concat_32x32_b256": measure("bench_concat", False, 32, 256, a.steps, a.warmup)}
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
