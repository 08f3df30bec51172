#!/usr/bin/env python3
"""attn_dim_head = 32 vs 64 at the benchmark configuration (32x32, dim 64, mults (1, 2, 4, 8), B = 256).

  python tools/dim_head_time.py [--batch 256] [--steps 20] [--warmup 2] [--json OUT]
      ms per graph-replayed DDIM denoise step at both widths, measured in the same process after warm-up.
  rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/dim_head_time.py --layers [--batch 256]
      one eager forward and one training iteration (B = 16) per width, for per-kernel forward / backward times from the
      trace (the attention kernels carry the linattn_ / att prefixes).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402


def build(dh):
    u = dm.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, attn_dim_head=dh, device="cuda:0")
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
    return u


def step_ms(dh, batch, steps, warmup):
    d = dm.DenoisingDiffusion(build(dh), image_size=32, timesteps=1000, sampling_timesteps=steps)
    for i in range(warmup):
        d.sample(batch_size=batch, seed=1 + i)
    torch.cuda.synchronize()
    reps = 3
    t0 = time.perf_counter()
    for i in range(reps):
        d.sample(batch_size=batch, seed=100 + i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / (reps * steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", action="store_true", help="one forward + one training iteration per width (under rocprofv3)")
    ap.add_argument("--json", help="write the step times here")
    a = ap.parse_args()
    if a.layers:
        for dh in (32, 64):
            u = build(dh)
            x = torch.randn((a.batch, 3, 32, 32), device="cuda:0")
            t = torch.randint(0, 1000, (a.batch,), device="cuda:0")
            u(x, t)
            d = dm.DenoisingDiffusion(u, image_size=32, timesteps=1000)
            dm.train_step(d, [torch.rand((16, 3, 32, 32))], lr=1e-4)
            torch.cuda.synchronize()
        return
    res = {}
    for _ in range(2):  # interleaved twice: clocks ramp over the first launches of a process
        for dh in (32, 64):
            res.setdefault(dh, []).append(step_ms(dh, a.batch, a.steps, a.warmup))
    out = {f"dh{dh}_step_ms": min(v) for dh, v in res.items()}
    out["ratio_64_over_32"] = out["dh64_step_ms"] / out["dh32_step_ms"]
    out["config"] = dict(batch=a.batch, size=32, dim=64, dim_mults=[1, 2, 4, 8], ddim_steps=a.steps, graph=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
