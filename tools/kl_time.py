#!/usr/bin/env python3
"""ms per ``AutoencoderKL.encode_sample`` and per ``VQModel.encode`` of the same ddconfig at the config-4 encoder shape
(B = 128, 3x64x64 images -> 4x32x32 latents), the two legs alternating in one process.

    python tools/kl_time.py [--B 128] [--iters 100] [--repeats 5] [--legs kl,vq] [--root DIR] [--out FILE]

``--root DIR`` imports the package from another checkout (the parent commit, for its VQ leg: ``--legs vq``).  Every window
is a host clock around ``iters`` calls that ends in a device synchronise, after a warm-up of the same shape.  One JSON line
per leg: the median, the fastest and the slowest window.  The posterior kernel's own time comes from a kernel trace of
``--legs kl`` (``rocprofv3 --kernel-trace --stats -- python tools/kl_time.py --legs kl --iters 20 --repeats 1``)."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=128)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--legs", default="kl,vq")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402
from diffusion_models_amd.spec import DecoderConfig, EncoderConfig, decoder_param_spec, encoder_param_spec  # noqa: E402

assert torch.cuda.is_available(), "kl_time.py measures on the GPU; there is nothing to fall back to"
DEV = "cuda:0"
DD = dict(ch=64, out_ch=3, in_channels=3, ch_mult=(1, 2), num_res_blocks=2, attn_resolutions=(), resolution=64, z_channels=4,
          double_z=True)
KW = dict(ch=64, ch_mult=(1, 2), num_res_blocks=2, attn_resolutions=(), resolution=64, z_channels=4, embed_dim=4)
legs = args.legs.split(",")
x = torch.rand((args.B, 3, 64, 64), generator=torch.Generator().manual_seed(1)).to(DEV) * 2 - 1
calls = {}
if "kl" in legs:
    ecfg = EncoderConfig(n_embed=0, double_z=True, **KW)
    kl = dm.AutoencoderKL(DD, None, 4, device=DEV)
    kl.load_state_dict(dm.synth_state_dict(encoder_param_spec(ecfg) + decoder_param_spec(DecoderConfig(**KW)), salt=4))
    calls["kl"] = lambda: kl.encode_sample(x, seed=7)
if "vq" in legs:
    ecfg = EncoderConfig(n_embed=8192, double_z=True, **KW)
    vq = dm.VQModel(DD, None, 8192, 4, device=DEV)
    vq.load_state_dict(dm.synth_state_dict(encoder_param_spec(ecfg) + decoder_param_spec(DecoderConfig(**KW)), salt=4))
    calls["vq"] = lambda: vq.encode(x)

for fn in calls.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
windows = {k: [] for k in calls}
for _ in range(args.repeats):
    for name, fn in calls.items():  # alternating: both legs see the same neighbours on a shared host
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        windows[name].append(1e3 * (time.perf_counter() - t0) / args.iters)
lines = []
for name, w in windows.items():
    lines.append(json.dumps(dict(leg=name, what="AutoencoderKL.encode_sample" if name == "kl" else "VQModel.encode", B=args.B,
                                 image=[3, 64, 64], latent=[4, 32, 32], iters=args.iters, ms_median=round(statistics.median(w), 4),
                                 ms_min=round(min(w), 4), ms_max=round(max(w), 4), windows_ms=[round(v, 4) for v in w],
                                 root=os.path.abspath(args.root) == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
                                 and "this checkout" or "other checkout")))
print("\n".join(lines))
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
