#!/usr/bin/env python3
"""RePaint row time against the plain DDPM step time at the benchmark shape (graph-replayed, after warm-up, one process).

  python tools/repaint_time.py [--timesteps 300] [--json OUT]

Unet(dim=64, dim_mults=(1, 2, 4, 8)) at 32x32, B = 256 under RePaintGaussianDiffusion.  The masked loop (resample_every =
T / 3, resample_iter = 2, resample_jump = 10: a bounded number of rows) is timed per row, the loop without a mask -- the
parent's p_sample_loop, the path bench.py's DDPM mode measures -- per step.  A masked row is the same U-Net forward and one
elementwise launch that reads gt and the mask on top of what the plain update reads, so the expectation is a ratio inside
the run-to-run spread of the plain step.  That spread is measured here by timing the plain loop three times, around and
between the two timings of the masked one; the ratio is reported, not asserted.

The clock is the host's around whole sample() calls ending in a device synchronise.  A masked call also pays, once per
call and not per row, for what the plain one does not have: the unrolling of the row table in Python, three
device-to-device copies (gt, mask, result) and the blend in front of row 0.  That is inside the masked figure and biases the
ratio upward, the more the fewer rows a call has.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402

BATCH, SIDE = 256, 32


def call_ms(fn, warmup, reps):
    for i in range(warmup):
        fn(seed=1 + i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(seed=100 + i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timesteps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", help="write the results here")
    a = ap.parse_args()
    T = a.timesteps
    u = dm.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, device="cuda:0")
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
    d = dm.RePaintGaussianDiffusion(u, image_size=SIDE, timesteps=T)
    kw = dict(resample=True, resample_iter=2, resample_jump=10, resample_every=T // 3)
    rows = len(dm.repaint_step_table(d._sched, **kw).times)
    g = torch.Generator().manual_seed(0)
    gt = torch.rand((BATCH, 3, SIDE, SIDE), generator=g).to("cuda:0")
    mask = torch.zeros((BATCH, 1, SIDE, SIDE), device="cuda:0")
    mask[..., SIDE // 2:] = 1.0
    plain = lambda seed: d.sample(batch_size=BATCH, seed=seed)  # noqa: E731
    masked = lambda seed: d.sample(gt=gt, mask=mask, seed=seed, **kw)  # noqa: E731
    res = {"plain": [], "masked": []}
    for _ in range(2):  # plain, masked, plain, masked, plain: the plain loop brackets the masked one
        res["plain"].append(call_ms(plain, a.warmup, a.reps) / T)
        res["masked"].append(call_ms(masked, a.warmup, a.reps) / rows)
    res["plain"].append(call_ms(plain, a.warmup, a.reps) / T)
    p, m = res["plain"], res["masked"]
    out = {
        "plain_step_ms": p, "masked_row_ms": m,
        "plain_step_ms_min": min(p), "masked_row_ms_min": min(m),
        "plain_spread": (max(p) - min(p)) / min(p),
        "masked_row_over_plain_step": min(m) / min(p),
        "config": dict(dim=64, dim_mults=[1, 2, 4, 8], size=SIDE, batch=BATCH, timesteps=T, rows=rows, graph=True,
                       mask_channels=1, reps=a.reps, **kw),
    }
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
