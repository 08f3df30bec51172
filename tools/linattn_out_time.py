"""Time of the output kernel (kernel 2) of one fused LinearAttention layer per (batch, C, tokens), from the library's
own event rows: whichever form launch_c selects in the library that is loaded.  Development aid behind the dispatch
rule la_out_headsum_form (linattn_fused.hip):

    python tools/linattn_out_time.py [--reps 20] [--json FILE]

To compare the two forms at every shape, build linattn_fused.hip twice with -DDM_LA_OUT_FORM=0 / =1 (every layer on
the (token block, image) kernel / on the head-sum kernel) and point DM_LIB at each build in turn; the rows of both runs
side by side are profiles/linattn_out_dispatch_table.json."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffusion_models_amd import _lib  # noqa: E402

# the five fused layers of the 32x32 benchmark U-Net (four shapes) and the full-resolution layers of the 64x64 configs
SHAPES = [(64, 32, 32), (64, 16, 16), (128, 16, 16), (128, 8, 8), (64, 64, 64)]
BATCHES = [8, 32, 64, 128, 256]


def seeded(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to("cuda:0").contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=2, help="independent timings of every (shape, batch)")
    ap.add_argument("--json")
    args = ap.parse_args()
    lib = _lib.load()
    out = []
    _lib.profile_enable(True)
    try:
        for run in range(args.runs):
            for Cc, H, W in SHAPES:
                w = [1 + 0.3 * seeded((1, Cc, 1, 1), 10), seeded((2, 4, 32, 4), 11),
                     seeded((384, Cc, 1, 1), 12, Cc ** -0.5), seeded((Cc, 128, 1, 1), 13, 128 ** -0.5),
                     seeded((Cc,), 14, 0.1), 1 + 0.3 * seeded((1, Cc, 1, 1), 15)]
                for B in BATCHES:
                    x = seeded((B, Cc, H, W), 1)
                    y = torch.empty_like(x)

                    def call():
                        _lib.check(lib.dm_op_linear_attention(_lib.ptr(x), *[_lib.ptr(t) for t in w], _lib.ptr(y), B, Cc,
                                                              H, W, 4, 32, None))

                    call()
                    _lib.profile_read()
                    for _ in range(args.reps):
                        call()
                    us = {r["kernel"]: 1e3 * r["total_ms"] / r["launches"] for r in _lib.profile_read()
                          if r["kernel"].startswith("linattn_out_")}
                    assert len(us) == 1, us
                    (kernel, t), = us.items()
                    row = {"run": run, "B": B, "C": Cc, "tokens": H * W, "kernel": kernel, "out_us": round(t, 2)}
                    out.append(row)
                    print(json.dumps(row), flush=True)
                    del x, y
    finally:
        _lib.profile_enable(False)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"lib": os.path.basename(_lib.LIB_PATH), "reps": args.reps, "rows": out}, f, indent=1)


if __name__ == "__main__":
    main()
