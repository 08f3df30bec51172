"""Time of the kernels of one fused LinearAttention layer per (batch, C, tokens), from the library's own event rows:
the context pass (blocked kernel + reduce, or the per-image kernel, whichever launch_c selects in the library that is
loaded), and the output kernel.  Development aid behind the dispatch rule of launch_c (linattn_fused.hip):

    python tools/linattn_ctx_time.py [--reps 20] [--json FILE]

To compare the two forms at every shape, build the library twice with la_image_form returning true / false and point
DM_LIB at each build in turn; the rows of both runs side by side are the table in profiles/."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffusion_models_amd import _lib  # noqa: E402

SHAPES = [(64, 32, 32), (64, 16, 16), (128, 16, 16), (128, 8, 8)]  # the five fused layers of the 32x32 benchmark U-Net
BATCHES = [32, 64, 128, 256]


def seeded(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to("cuda:0").contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json")
    args = ap.parse_args()
    lib = _lib.load()
    out = []
    _lib.profile_enable(True)
    try:
        for Cc, H, W in SHAPES:
            w = [1 + 0.3 * seeded((1, Cc, 1, 1), 10), seeded((2, 4, 32, 4), 11), seeded((384, Cc, 1, 1), 12, Cc ** -0.5),
                 seeded((Cc, 128, 1, 1), 13, 128 ** -0.5), seeded((Cc,), 14, 0.1), 1 + 0.3 * seeded((1, Cc, 1, 1), 15)]
            for B in BATCHES:
                x = seeded((B, Cc, H, W), 1)
                y = torch.empty_like(x)

                def call():
                    _lib.check(lib.dm_op_linear_attention(_lib.ptr(x), *[_lib.ptr(t) for t in w], _lib.ptr(y), B, Cc, H, W,
                                                          4, 32, None))

                call()
                _lib.profile_read()
                for _ in range(args.reps):
                    call()
                us = {r["kernel"]: 1e3 * r["total_ms"] / r["launches"] for r in _lib.profile_read()
                      if r["kernel"].startswith("linattn_")}
                ctx = sum(v for k, v in us.items() if k.startswith("linattn_ctx_"))
                row = {"B": B, "C": Cc, "tokens": H * W, "ctx_pass_us": round(ctx, 2),
                       "rows_us": {k: round(v, 2) for k, v in sorted(us.items())}}
                out.append(row)
                print(json.dumps(row), flush=True)
    finally:
        _lib.profile_enable(False)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"lib": os.path.basename(os.path.dirname(_lib.LIB_PATH)), "reps": args.reps, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
