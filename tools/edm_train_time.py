#!/usr/bin/env python3
"""One ElucidatedDiffusion training iteration against one DDPM training iteration at the benchmark's training shape.

  python tools/edm_train_time.py [--iters 20] [--rounds 5] [--json profiles/edm_train_time.json]

Unet(dim=64, dim_mults=(1, 2, 4, 8)) at 32x32, B = 64 and B = 16, twice: with learned_sinusoidal_cond=True under
ElucidatedDiffusion (``train_step``: forward + backward + clip + Adam) and as the plain U-Net under DenoisingDiffusion, the
iteration bench.py's training mode measures.  Both in one process, interleaved round by round after a warm-up of every
shape; an iteration is enqueued with ``sync=False`` and the window of ``iters`` iterations ends in a device synchronise.
Reported per batch: the median and the spread (max - min over the rounds, relative to the median) of each, and the ratio
of the medians.  The ratio is reported, not asserted: from the code the EDM iteration is the DDPM one plus the noise-in
and loss passes over a 3-channel image, two small launches behind time_mlp.1 and the 17-wide (odd) time_mlp.1 taking the
scalar linear kernels.
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

SIDE = 32


def build(**kw):
    u = dm.Unet(dim=64, dim_mults=(1, 2, 4, 8), channels=3, device="cuda:0", **kw)
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=0))
    return u


def window_ms(model, imgs, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        dm.train_step(model, [imgs], lr=1e-4, sync=False)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", help="write the results here")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    torch.manual_seed(0)
    edm = dm.ElucidatedDiffusion(build(learned_sinusoidal_cond=True), image_size=SIDE).train()
    ddpm = dm.DenoisingDiffusion(build(), image_size=SIDE, timesteps=1000).train()
    out = {"shape": "Unet(dim=64, dim_mults=(1,2,4,8)) 32x32", "iters_per_window": a.iters, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0)}
    for B in (64, 16):
        imgs = torch.rand((B, 3, SIDE, SIDE), generator=torch.Generator().manual_seed(B)).to("cuda:0")
        for m in (ddpm, edm):
            window_ms(m, imgs, a.warmup)
        t = {"ddpm": [], "edm": []}
        for _ in range(a.rounds):
            t["ddpm"].append(window_ms(ddpm, imgs, a.iters))
            t["edm"].append(window_ms(edm, imgs, a.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        out[f"b{B}"] = {
            "ddpm_iter_ms": med["ddpm"], "edm_iter_ms": med["edm"],
            "ddpm_rounds_ms": t["ddpm"], "edm_rounds_ms": t["edm"],
            "ddpm_spread": (max(t["ddpm"]) - min(t["ddpm"])) / med["ddpm"],
            "edm_spread": (max(t["edm"]) - min(t["edm"])) / med["edm"],
            "edm_over_ddpm": med["edm"] / med["ddpm"],
        }
        print(f"B={B}: DDPM {med['ddpm']:.3f} ms  EDM {med['edm']:.3f} ms  ratio {med['edm'] / med['ddpm']:.4f}  "
              f"(DDPM spread {out[f'b{B}']['ddpm_spread']:.3%})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
