#!/usr/bin/env python3
"""KarrasUnet's denoise step under ElucidatedDiffusion: ms per hipGraph-replayed DPM-Solver++ step and Heun step of the default
constructor (``dim=192, channels=4``, three downsamples, four blocks per stage) at ``image_size=64``, the same forward through
the project's torch restatement (tests/karras_oracle.py, fp32, eager PyTorch-ROCm) on the same GPU in the same call, and the
time of every kernel of one forward.

    python tools/karras_time.py [--batch 64] [--image-size 64] [--dim 192] [--steps 8] [--repeats 5] [--out FILE]

Step time: every window is a host clock around one sampling call of ``steps`` graph replays that ends in a device
synchronise, after a warm-up call of the same shape; the median, the fastest and the slowest of ``repeats`` windows are
reported, the spread being (max - min) / median.  A Heun step holds two forwards (the last step one).  Eager baseline: the
median of ``repeats`` forwards of the restatement between device synchronisations, after one warm-up.  Per-kernel time: one
eager float-time forward under the library's profile rows in detail mode (event pairs around every launch, bracket overhead
subtracted), summed per family -- 3x3 convolutions, 1x1 convolutions, the attention cores, each kunet_* kernel, the head's
Linear layers -- with the launches per forward; for the kunet_* rows the bytes moved (from the shapes) over the kernel time are
set against the HBM bandwidth of MI355X_MICROARCH.md.  The figures come from different regimes (graph replay, eager torch,
bracketed eager launches) and are not to be subtracted from one another.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--image-size", type=int, default=64)
ap.add_argument("--dim", type=int, default=192)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402
import karras_oracle as ko  # noqa: E402
from diffusion_models_amd import _lib  # noqa: E402

assert torch.cuda.is_available(), "karras_time.py measures on the GPU; there is nothing to fall back to"
DEV = "cuda:0"
HBM_TBS = 8.0  # peak HBM3E bandwidth of one MI355X, TB/s


def profile_rows():
    rows = (_lib.ProfileRow * 512)()
    n = C.c_int(0)
    _lib.check(_lib.load().dm_profile_read(rows, 512, C.byref(n)))
    return [dict(kernel=rows[i].kernel.decode(), launches=int(rows[i].launches), ms=float(rows[i].total_ms),
                 bytes=float(rows[i].total_bytes)) for i in range(n.value)]


def family(kernel):
    if kernel.startswith("kunet_"):
        return kernel
    if kernel.startswith(("conv<", "pw<", "wino", "upwino", "init7")):
        return "conv_3x3" if " 3x3 " in kernel else "conv_1x1"
    if "attn" in kernel or "attention" in kernel:
        return "attention_cores"
    return "other"


def windows_of(fn, per):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / per)
    med = statistics.median(out)
    return dict(median=round(med, 4), min=round(min(out), 4), max=round(max(out), 4), spread=round((max(out) - min(out)) / med, 4))


def to_dev(v):
    if torch.is_tensor(v):
        return v.to(DEV)
    if isinstance(v, dict):
        return {k: to_dev(x) for k, x in v.items()}
    if isinstance(v, list):
        return [to_dev(x) for x in v]
    return v


B, S = args.batch, args.image_size
u = dm.KarrasUnet(image_size=S, dim=args.dim, dim_max=4 * args.dim, device=DEV)
sd = dm.synth_state_dict(u.param_spec(), salt=0)
u.load_state_dict(sd)
edm = dm.ElucidatedDiffusion(u, image_size=S, channels=u.channels, num_sample_steps=args.steps)
dpmpp = windows_of(lambda: edm.sample_using_dpmpp(batch_size=B, seed=1), args.steps)
heun = windows_of(lambda: edm.sample(batch_size=B, seed=1), args.steps)

x = torch.randn(B, u.channels, S, S, device=DEV)
t = torch.linspace(-1.5, 1.0, B, device=DEV)
fwd = windows_of(lambda: u(x, t), 1)
P = to_dev(ko.fold(sd, u.cfg, torch.float32))
with torch.inference_mode():
    eager = windows_of(lambda: ko.forward(P, x, t), 1)
    err = float((u(x, t).double() - ko.forward(P, x, t).double()).norm() / ko.forward(P, x, t).double().norm())

u(x, t)
_lib.profile_enable(True, detail=True)
profile_rows()
u(x, t)
rows = profile_rows()
_lib.profile_enable(False)
fam = {}
for r in rows:
    f = fam.setdefault(family(r["kernel"]), dict(ms=0.0, launches=0, bytes=0.0))
    f["ms"] += r["ms"]
    f["launches"] += r["launches"]
    f["bytes"] += r["bytes"]
for name, f in fam.items():
    if name.startswith("kunet_"):
        f["tb_per_s"] = round(f["bytes"] / max(f["ms"], 1e-9) / 1e9, 3)
        f["fraction_of_hbm_peak"] = round(f["tb_per_s"] / HBM_TBS, 3)
    f["ms"] = round(f["ms"], 4)
    del f["bytes"]
line = json.dumps(dict(what=f"KarrasUnet(dim={args.dim}, 3 downsamples, 4 blocks per stage) under ElucidatedDiffusion", B=B,
                       image_size=S, steps=args.steps, params=sum(v.numel() for v in sd.values()),
                       dpmpp_ms_per_step=dpmpp, heun_ms_per_step=heun, forward_ms=fwd, eager_restatement_forward_ms=eager,
                       forward_vs_restatement_rel_l2=err, kernel_ms_per_forward=round(sum(r["ms"] for r in rows), 4),
                       launches_per_forward=sum(r["launches"] for r in rows), families=fam))
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
