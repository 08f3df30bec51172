#!/usr/bin/env python3
"""Classifier-guided step time against the plain DDPM step time at the benchmark shape (graph-replayed, after warm-up, one
process).

  python tools/cguide_time.py [--timesteps 100] [--json OUT]

Unet(dim=64, dim_mults=(1, 2, 4, 8)) at 32x32, B = 256 under ClassifierGuidedGaussianDiffusion.  Three loops are timed per
step: the plain one (no cond_fn: the parent's p_sample_loop, the path bench.py's DDPM mode measures), the guided one with a
no-op cond_fn that returns a held zero tensor (the split step alone: one more launch, one write and one read of the mean,
one read of the gradient, two graph launches instead of one and the host round trip -- a stream synchronisation, a ctypes
callback, a ``fill_`` of t, a device copy into ``grad`` and a second synchronisation), and the guided one with a 10-class
linear classifier on the flattened image (``log_softmax`` and ``autograd.grad`` in torch, tests/cguide_oracle.py's form).
The plain loop is timed three times, around and between the guided timings, and its spread is reported next to the
ratios.  These are measurements, not thresholds.

The clock is the host's around whole sample() calls ending in a device synchronise; a guided call cannot run ahead of the
host, so its figure is the wall time per step, idle GPU time of the round trip included.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402

BATCH, SIDE, CLASSES = 256, 32, 10
DEV = "cuda:0"


def call_ms(fn, warmup, reps):
    for i in range(warmup):
        fn(seed=1 + i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(seed=100 + i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def linear_classifier(T):
    g = torch.Generator().manual_seed(0)
    W = (torch.randn((CLASSES, 3 * SIDE * SIDE), generator=g) * 0.05).to(DEV)
    u = (torch.randn((CLASSES,), generator=g) * 0.05).to(DEV)

    def cond_fn(x, t, y=None, scale=1.0):
        with torch.enable_grad():
            xin = x.detach().requires_grad_(True)
            logp = torch.log_softmax(xin.flatten(1) @ W.T + (t.float() / T)[:, None] * u, dim=-1)
            return torch.autograd.grad(logp[torch.arange(xin.shape[0], device=DEV), y].sum(), xin)[0] * scale

    return cond_fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timesteps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", help="write the results here")
    a = ap.parse_args()
    T = a.timesteps
    u = dm.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, device=DEV)
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
    d = dm.ClassifierGuidedGaussianDiffusion(u, image_size=SIDE, timesteps=T, beta_schedule="linear")
    zeros = torch.zeros((BATCH, 3, SIDE, SIDE), device=DEV)
    y = torch.randint(0, CLASSES, (BATCH,), generator=torch.Generator().manual_seed(1)).to(DEV)
    clf = linear_classifier(T)
    plain = lambda seed: d.sample(batch_size=BATCH, seed=seed)  # noqa: E731
    noop = lambda seed: d.sample(batch_size=BATCH, cond_fn=lambda x, t: zeros, guidance_kwargs={}, seed=seed)  # noqa: E731
    linear = lambda seed: d.sample(batch_size=BATCH, cond_fn=clf, guidance_kwargs=dict(y=y, scale=10.0), seed=seed)  # noqa: E731
    res = {"plain": [], "noop": [], "linear": []}
    res["plain"].append(call_ms(plain, a.warmup, a.reps) / T)
    res["noop"].append(call_ms(noop, a.warmup, a.reps) / T)
    res["plain"].append(call_ms(plain, a.warmup, a.reps) / T)
    res["linear"].append(call_ms(linear, a.warmup, a.reps) / T)
    res["plain"].append(call_ms(plain, a.warmup, a.reps) / T)
    p = res["plain"]
    out = {
        "plain_step_ms": p, "guided_noop_step_ms": res["noop"], "guided_linear_step_ms": res["linear"],
        "plain_step_ms_min": min(p), "plain_spread": (max(p) - min(p)) / min(p),
        "noop_over_plain": min(res["noop"]) / min(p), "linear_over_plain": min(res["linear"]) / min(p),
        "noop_extra_ms_per_step": min(res["noop"]) - min(p), "linear_extra_ms_per_step": min(res["linear"]) - min(p),
        "config": dict(dim=64, dim_mults=[1, 2, 4, 8], size=SIDE, batch=BATCH, timesteps=T, classes=CLASSES, graph=True,
                       reps=a.reps),
    }
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
