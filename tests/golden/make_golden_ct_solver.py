#!/usr/bin/env python3
"""DPM-Solver++ goldens for the continuous-time classes (build container only):
``python tests/golden/make_golden_ct_solver.py`` -> ``ct_solver.pt``.

The reference has no such sampler, so the loop is the CPU oracle's (tests/ct_dpmpp_oracle.py) over the REFERENCE U-Net on
the name-seeded synthetic weights of make_golden_ct.py: once in fp32, as the library runs it, and once in float64 on the
same fp32 step table.  Stored per case: ``x_T``, the float64 final iterate, the float64 finalized sample, and the
fp32-vs-float64 error of what the case compares.  Only DATA is written.

What a case compares:
* v objective: the finalized sample (the share of its pixels on the final clamp is printed and must be at most 0.5);
* noise objective: the raw final iterate.  With synthetic weights a noise-objective run ends with most pixels outside
  [-1, 1], so the finalized image would be carried by the clamp.
Asserted here: every case's own fp32-vs-float64 error is below a tenth of the loop tolerance (1e-3), the clamp shares, and
that the order-1 and order-2 runs of one case differ by more than 1e-2 (a test that passed on the wrong order would show
nothing)."""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import import_reference, save, seeded  # noqa: E402
from make_golden_ct import D32, ref_net  # noqa: E402

import ct_dpmpp_oracle as do  # noqa: E402
import diffusion_models_amd as dm  # noqa: E402

LOOP_TOL = 1e-3
RFF = dict(dim=32, dim_mults=(1, 2), random_fourier_features=True)
CASES = {
    # key: (class, unet kwargs, schedule, clip, N, order, salt, x_T seed, what is compared)
    "v_o2": ("v", D32, "cosine", True, 6, 2, 81, 701, "sample"),
    "v_o2_noclip": ("v", D32, "cosine", False, 6, 2, 82, 702, "sample"),
    "v_o2_rff": ("v", RFF, "cosine", True, 6, 2, 84, 703, "sample"),
    "v_o1": ("v", D32, "cosine", True, 6, 1, 81, 701, "sample"),
    "lin_o2_noclip": ("noise", D32, "linear", False, 6, 2, 81, 704, "x"),
    "cos_o2_noclip": ("noise", D32, "cosine", False, 6, 2, 82, 705, "x"),
    "lin_o2_clip": ("noise", D32, "linear", True, 6, 2, 81, 706, "x"),
    "lin_o1_noclip": ("noise", D32, "linear", False, 6, 1, 81, 704, "x"),
}
ORDER_PAIRS = (("v_o1", "v_o2"), ("lin_o1_noclip", "lin_o2_noclip"))
SHAPE = (2, 3, 16, 16)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    dd, _, _ = import_reference()
    out = {"cases": {}}
    for key, (kind, ukw, sched, clip, n, order, salt, seed, what) in CASES.items():
        objective = do.V if kind == "v" else do.NOISE
        table = dm.ct_dpmpp_table(n, sched, order)
        x_T = seeded(SHAPE, seed)
        res, x_starts = {}, []
        with torch.inference_mode():
            for dtype in (torch.float32, torch.float64):
                net, _ = ref_net(dd, ukw, salt, dtype)
                net.eval()
                res[dtype] = do.sample(lambda x, t: net(x, t), table.to(dtype), x_T.to(dtype), objective, clip,
                                       x_starts if dtype is torch.float64 else None)
        # the share of x_start values on the clamp over the float64 run
        on_clamp = float(torch.stack(x_starts).abs().eq(1).double().mean()) if clip else None
        (x32, y32), (x64, y64) = res[torch.float32], res[torch.float64]
        share = float(((y64 == 0) | (y64 == 1)).double().mean())
        err = rel(y32, y64) if what == "sample" else rel(x32, x64)
        print(f"{key}: fp32 vs float64 on {what} {err:.3e}; final clamp share {share:.2f}; x_start on the clamp {on_clamp}")
        assert err < LOOP_TOL / 10, (key, err)
        assert what != "sample" or share <= 0.5, (key, share)
        out["cases"][key] = dict(kind=kind, unet_kw=ukw, schedule=sched, clip=clip, n=n, order=order, salt=salt, compare=what,
                                 x_T=x_T, x64=x64, sample64=y64, ref_err=err, clamp_share=share, x_start_clamp_share=on_clamp)
    for a, b in ORDER_PAIRS:
        ca, cb = out["cases"][a], out["cases"][b]
        what = "sample64" if ca["compare"] == "sample" else "x64"
        d = rel(ca[what], cb[what])
        print(f"{a} vs {b}: {d:.3e}")
        assert d > 1e-2, (a, b, d)
    save("ct_solver.pt", out)


if __name__ == "__main__":
    main()
