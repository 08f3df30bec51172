#!/usr/bin/env python3
"""The sequence model's denoise step: ms per hipGraph-replayed DDIM step of ``Unet1D(dim=64, dim_mults=(1, 2, 4, 8))`` and the
time of every kernel of one step, per layer shape.

    python tools/seq1d_time.py [--shapes 64x128,16x1024] [--steps 20] [--repeats 5] [--out FILE]

The library has one family for each layer form of the sequence model, so there is nothing to switch between; the run that
compared the K = 3 layers on the direct family and on the Winograd F(4,3) kernel of experimental/ used this tool's two
figures on two builds (profiles/seq1d_wino1d_vs_direct.jsonl).  The two figures come from two regimes and are
not to be subtracted from one another: the step time is graph replay, the per-layer times are an eager run with an event
pair around every launch.

Step time: every window is a host clock around one ``sample()`` of ``steps`` graph replays that ends in a device
synchronise, after a warm-up call of the same shape; the median, the fastest and the slowest of ``repeats`` windows are
reported, the spread being (max - min) / median.  Per-layer time: one eager run of 8 steps under the library's profile rows
in detail mode (event pairs around every launch, bracket overhead subtracted), summed per family: the K = 3 convolutions, the
other convolutions, the attention cores, and what is left (norms, elementwise, the update).  One JSON line per shape."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="64x128,16x1024")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402
from diffusion_models_amd import _lib  # noqa: E402

assert torch.cuda.is_available(), "seq1d_time.py measures on the GPU; there is nothing to fall back to"
DEV = "cuda:0"
PROFILE_STEPS = 8


def profile_rows():
    rows = (_lib.ProfileRow * 512)()
    n = C.c_int(0)
    _lib.check(_lib.load().dm_profile_read(rows, 512, C.byref(n)))
    return [dict(kernel=rows[i].kernel.decode(), launches=int(rows[i].launches), ms=float(rows[i].total_ms),
                 flops=float(rows[i].total_flops)) for i in range(n.value)]


def family(kernel):
    if kernel.startswith(("conv<", "pw<", "wino", "upwino", "init7")):  # "wino1d ..." rows name their 1x3 shape too
        return "conv_k3" if " 1x3 " in kernel else "conv_other"
    if "attn" in kernel or "attention" in kernel:
        return "attention_cores"
    return "other"


u = dm.Unet1D(dim=64, dim_mults=(1, 2, 4, 8), channels=2, device=DEV)
u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
lines = []
for shape in args.shapes.split(","):
    B, L = (int(v) for v in shape.split("x"))
    d = dm.DenoisingDiffusion1D(u, seq_length=L, timesteps=1000, sampling_timesteps=args.steps)
    d.sample(batch_size=B, seed=1)
    torch.cuda.synchronize()
    windows = []
    for i in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.sample(batch_size=B, seed=2 + i)
        torch.cuda.synchronize()
        windows.append(1e3 * (time.perf_counter() - t0) / args.steps)
    med = statistics.median(windows)
    # per-layer: an eager run short enough for the library to park the GPU while the host enqueues
    e = dm.DenoisingDiffusion1D(u, seq_length=L, timesteps=1000, sampling_timesteps=PROFILE_STEPS, use_graph=False)
    e.sample(batch_size=B, seed=1)
    _lib.profile_enable(True, detail=True)
    profile_rows()
    e.sample(batch_size=B, seed=1)
    rows = profile_rows()
    _lib.profile_enable(False)
    fam = {}
    for r in rows:
        f = fam.setdefault(family(r["kernel"]), dict(ms_per_step=0.0, launches_per_step=0.0, flops_per_step=0.0))
        f["ms_per_step"] += r["ms"] / PROFILE_STEPS
        f["launches_per_step"] += r["launches"] / PROFILE_STEPS
        f["flops_per_step"] += r["flops"] / PROFILE_STEPS
    for f in fam.values():
        f["tflops"] = round(f["flops_per_step"] / max(f["ms_per_step"], 1e-9) / 1e9, 2)
        f["ms_per_step"], f["launches_per_step"] = round(f["ms_per_step"], 4), round(f["launches_per_step"], 1)
        del f["flops_per_step"]
    layers = sorted(({"kernel": r["kernel"], "launches_per_step": r["launches"] / PROFILE_STEPS,
                      "us_per_launch": round(1e3 * r["ms"] / max(r["launches"], 1), 2),
                      "tflops": round(r["flops"] / max(r["ms"], 1e-9) / 1e9, 2)} for r in rows),
                    key=lambda r: -r["us_per_launch"] * r["launches_per_step"])
    lines.append(json.dumps(dict(what="Unet1D(dim=64, dim_mults=(1,2,4,8)) DDIM step, graph replay", B=B, L=L, steps=args.steps,
                                 ms_per_step_median=round(med, 4), ms_min=round(min(windows), 4), ms_max=round(max(windows), 4),
                                 spread=round((max(windows) - min(windows)) / med, 4),
                                 kernel_ms_per_step=round(sum(r["ms"] for r in rows) / PROFILE_STEPS, 4),
                                 launches_per_step=round(sum(r["launches"] for r in rows) / PROFILE_STEPS, 1),
                                 families=fam, layers=layers)))
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
