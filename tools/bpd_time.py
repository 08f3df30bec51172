#!/usr/bin/env python3
"""Bits-per-dim loop step time beside a p_sample_loop step of the same model and shape (graph replay, after warm-up, in
one process).

  python tools/bpd_time.py [--steps 20] [--reps 5] [--json OUT]

The benchmark architecture (dim 64, mults (1, 2, 4, 8), synthetic weights) at B = 256, 32x32 and at B = 8, 64x64.  For each:
ms per step of ``calc_bpd_loop`` over ``--steps`` timesteps and of ``p_sample_loop(max_steps=--steps)``, the two alternating
``--reps`` times (min, median and max over the repetitions: the spread says what a difference means), for
``DenoisingDiffusion`` and for ``LearnedGaussianDiffusion``; and the step-in, term and finishing kernels alone: dm_profile
brackets of an eager 4-step run, for which the library parks the GPU while the host enqueues.  These are event intervals
around single launches, good to about a microsecond, not durations from a kernel trace.
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

KERNELS = ("bpd_step_in_kernel", "bpd_terms_kernel", "bpd_finish_kernel")


def build(learned):
    u = dm.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, learned_variance=learned, device="cuda:0")
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
    return u


def timed(fn, steps, calls=3):
    fn(0)  # the handle holds one step graph: the first call after the other leg captures again (another key), untimed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        fn(1 + i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / (calls * steps)


def kernel_ms(d, img, times):
    """Event interval per launch of the loop's own kernels, from an eager 4-step run under dm_profile."""
    d.use_graph = False
    try:
        d.calc_bpd_loop(img, seed=1, times=times[:4])
        _lib.profile_enable(True)
        try:
            d.calc_bpd_loop(img, seed=2, times=times[:4])
            rows = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
    finally:
        d.use_graph = True
    by = {r["kernel"]: r for r in rows}
    return {k: by[k]["total_ms"] / by[k]["launches"] for k in KERNELS}


def measure(learned, side, batch, steps, reps):
    u = build(learned)
    cls = dm.LearnedGaussianDiffusion if learned else dm.DenoisingDiffusion
    d = cls(u, image_size=side, timesteps=1000)
    img = torch.randint(0, 256, (batch, 3, side, side), generator=torch.Generator().manual_seed(3)).float().div(255).to("cuda:0")
    times = list(range(999, 999 - steps, -1))
    shape = (batch, 3, side, side)
    legs = [("bpd", lambda s: d.calc_bpd_loop(img, seed=100 + s, times=times)),
            ("ddpm", lambda s: d.p_sample_loop(shape, seed=100 + s, max_steps=steps))]
    for _, fn in legs:  # warm-up: clocks up, workspace grown
        for i in range(2):
            fn(50 + i)
    res = {k: [] for k, _ in legs}
    for _ in range(reps):
        for key, fn in legs:
            res[key].append(timed(fn, steps))
    out = {f"{k}_step_ms": dict(min=min(v), median=statistics.median(v), max=max(v), all=v) for k, v in res.items()}
    out["bpd_over_ddpm_median"] = out["bpd_step_ms"]["median"] / out["ddpm_step_ms"]["median"]
    out["kernel_ms"] = kernel_ms(d, img, times)
    out["kernels_share_of_bpd_step"] = sum(out["kernel_ms"].values()) / out["bpd_step_ms"]["median"]
    out["config"] = dict(size=side, batch=batch, per=3 * side * side, dim=64, dim_mults=[1, 2, 4, 8], steps=steps, graph=True,
                         learned_variance=learned, calls_per_repetition=3, repetitions=reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", help="write the results here")
    a = ap.parse_args()
    out = {}
    for learned in (False, True):
        tag = "learned" if learned else "fixed"
        out[f"{tag}_b256_32x32"] = measure(learned, 32, 256, a.steps, a.reps)
        out[f"{tag}_b8_64x64"] = measure(learned, 64, 8, a.steps, a.reps)
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
