#!/usr/bin/env python3
"""Dynamic thresholding step time (graph-replayed DDIM steps, after warm-up, in one process).

  python tools/dynthresh_time.py [--steps 20] [--reps 5] [--none-only] [--json OUT]

The benchmark architecture (dim 64, mults (1, 2, 4, 8), synthetic weights) at B = 256, 32x32 and at B = 8, 64x64.  For each:
ms per step with ``dynamic_threshold=None`` and with 0.95, the two alternating ``--reps`` times (min, median and max over
the repetitions: the spread says what a difference means), and the selection kernel alone (dm_profile brackets of an eager
run: kernel execution time) at (B, C*H*W) = (256, 3072) and (8, 12288).  ``--none-only`` times only the loop without the
keyword: it runs on a tree from before the keyword too, which gives the parent's step in the same call.
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

P = 0.95


def build():
    u = dm.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, device="cuda:0")
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
    return u


def step_ms(d, batch, steps, seed, **kw):
    calls = 3
    # the handle holds one step graph: the first call after the other leg captures again (another key), untimed here
    d.sample(batch_size=batch, seed=seed - 1, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        d.sample(batch_size=batch, seed=seed + i, **kw)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / (calls * steps)


def select_ms(u, side, batch):
    """Kernel time of dyn_threshold_kernel per step from an eager 4-step run under dm_profile."""
    d = dm.DenoisingDiffusion(u, image_size=side, timesteps=1000, sampling_timesteps=4, use_graph=False)
    d.sample(batch_size=batch, seed=1, dynamic_threshold=P)
    _lib.profile_enable(True)
    try:
        d.sample(batch_size=batch, seed=2, dynamic_threshold=P)
        rows = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    r = [r for r in rows if r["kernel"] == "dyn_threshold_kernel"][0]
    return r["total_ms"] / r["launches"]


def measure(u, side, batch, steps, reps, none_only):
    d = dm.DenoisingDiffusion(u, image_size=side, timesteps=1000, sampling_timesteps=steps)
    legs = [("none", {})] if none_only else [("none", {}), ("dyn", dict(dynamic_threshold=P))]
    for _, kw in legs:  # warm-up: both graphs captured, clocks up
        for i in range(2):
            d.sample(batch_size=batch, seed=1 + i, **kw)
    res = {k: [] for k, _ in legs}
    for r in range(reps):
        for key, kw in legs:
            res[key].append(step_ms(d, batch, steps, 100 + 10 * r, **kw))
    out = {}
    for key, v in res.items():
        out[f"{key}_step_ms"] = dict(min=min(v), median=statistics.median(v), max=max(v), all=v)
    if not none_only:
        out["dyn_over_none_median"] = out["dyn_step_ms"]["median"] / out["none_step_ms"]["median"]
        out["select_kernel_ms"] = select_ms(u, side, batch)
        out["select_share_of_dyn_step"] = out["select_kernel_ms"] / out["dyn_step_ms"]["median"]
    out["config"] = dict(size=side, batch=batch, per=3 * side * side, dim=64, dim_mults=[1, 2, 4, 8], ddim_steps=steps, graph=True,
                         percentile=P, calls_per_repetition=3, repetitions=reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--none-only", action="store_true")
    ap.add_argument("--json", help="write the results here")
    a = ap.parse_args()
    u = build()
    out = {"b256_32x32": measure(u, 32, 256, a.steps, a.reps, a.none_only),
           "b8_64x64": measure(u, 64, 8, a.steps, a.reps, a.none_only)}
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
