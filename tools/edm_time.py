#!/usr/bin/env python3
"""ElucidatedDiffusion step time at the benchmark shape (graph-replayed steps, after warm-up, in one process).

  python tools/edm_time.py [--steps 18] [--json OUT]

Unet(dim=64, dim_mults=(1, 2, 4, 8)) at 32x32, B = 256, twice: with learned_sinusoidal_cond=True under ElucidatedDiffusion
(Heun, two forwards per step but the last; DPM-Solver++, one forward per step) and as the plain U-Net under DDIM, the
path bench.py measures.  A Heun step is two forwards plus three elementwise passes over a 3-channel image, so the
expectation is ~2x the DDIM step; the ratio is reported, not asserted.
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


def build(**kw):
    u = dm.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, device="cuda:0", **kw)
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
    return u


def call_ms(fn, warmup, reps=3):
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
    ap.add_argument("--steps", type=int, default=18)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", help="write the results here")
    a = ap.parse_args()
    n = a.steps
    edm = dm.ElucidatedDiffusion(build(learned_sinusoidal_cond=True), image_size=SIDE, num_sample_steps=n)
    ddim = dm.DenoisingDiffusion(build(), image_size=SIDE, timesteps=1000, sampling_timesteps=n)
    res = {}
    for _ in range(2):  # interleaved twice: clocks ramp over the first launches of a process
        for key, fn in (("ddim", lambda seed: ddim.sample(batch_size=BATCH, seed=seed)),
                        ("heun", lambda seed: edm.sample(batch_size=BATCH, seed=seed)),
                        ("dpmpp", lambda seed: edm.sample_using_dpmpp(batch_size=BATCH, seed=seed))):
            res.setdefault(key, []).append(call_ms(fn, a.warmup))
    call = {k: min(v) for k, v in res.items()}
    forwards = {"ddim": n, "heun": 2 * n - 1, "dpmpp": n}
    out = {
        "ddim_step_ms": call["ddim"] / n,
        "heun_step_ms": call["heun"] / (n - 0.5),  # a call is n - 1 two-forward steps and one single-forward step
        "dpmpp_step_ms": call["dpmpp"] / n,
        "call_ms": call,
        "ms_per_forward": {k: call[k] / forwards[k] for k in call},
    }
    out["heun_step_over_2x_ddim_step"] = out["heun_step_ms"] / (2 * out["ddim_step_ms"])
    out["dpmpp_step_over_ddim_step"] = out["dpmpp_step_ms"] / out["ddim_step_ms"]
    out["config"] = dict(dim=64, dim_mults=[1, 2, 4, 8], size=SIDE, batch=BATCH, steps=n, graph=True,
                         edm_unet="learned_sinusoidal_cond=True", ddim_unet="plain")
    print(json.dumps(out, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
