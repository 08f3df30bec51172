"""CPU restatement of the two ElucidatedDiffusion loops as the HIP path runs them: driven by the host step tables
(``edm_heun_table`` / ``edm_dpmpp_table``), with exactly the arithmetic of the kernels in csrc/edm.hip on fp32 CPU tensors
and ``oracle.unet_oracle.unet_forward`` as the network.  Test helper only: the product never imports it.

It is what ties the table layout and the kernel formulas to the reference on a machine without a GPU: its outputs are
compared with the reference's recorded ``sample()`` / ``sample_using_dpmpp()`` results (tests/golden/edm.pt)."""
from __future__ import annotations

import torch

from diffusion_models_amd import elucidated as E


def _f(v):
    return torch.tensor(float(v), dtype=torch.float32)


def churn_in(x, eps, row):
    """edm_churn_in_kernel: (xhat, xin)."""
    xhat = x if float(row[E.CHURN]) == 0.0 else x + _f(row[E.CHURN]) * (_f(row[E.S_NOISE]) * eps)
    return xhat, _f(row[E.C_IN]) * xhat


def euler(xhat, F, row, clamp):
    """edm_euler_kernel: (D, d, xnext, xin2)."""
    D = _f(row[E.C_SKIP]) * xhat + _f(row[E.C_OUT]) * F
    if clamp:
        D = D.clamp(-1.0, 1.0)
    d = (xhat - D) / _f(row[E.SIGMA])
    xnext = xhat + _f(row[E.DT]) * d
    return D, d, xnext, _f(row[E.C_IN2]) * xnext


def heun(xhat, d, xnext, F2, row, clamp):
    """edm_heun_kernel."""
    D = _f(row[E.C_SKIP2]) * xnext + _f(row[E.C_OUT2]) * F2
    if clamp:
        D = D.clamp(-1.0, 1.0)
    d2 = (xnext - D) / _f(row[E.SIGMA2])
    return xhat + _f(row[E.HALF_DT]) * (d + d2)


def dpmpp(x, F, d_old, row):
    """edm_dpmpp_kernel: (x_next, D)."""
    D = _f(row[E.C_SKIP]) * x + _f(row[E.C_OUT]) * F
    dd = D if float(row[E.G]) == 0.0 else _f(row[E.OMG]) * D + _f(row[E.G]) * d_old
    return _f(row[E.A]) * x - _f(row[E.B_]) * dd, D


def finalize(x):
    return (x.clamp(-1.0, 1.0) + 1.0) * 0.5


def heun_sample(fwd, table, sigma_init, shape, noise, clamp=True):
    """``fwd(x, t)``: the U-Net on a (B,) float time.  ``noise``: draw 0 = start image, then one draw per step."""
    b = shape[0]
    x = _f(sigma_init) * noise(shape)
    for row in table:
        eps = noise(shape)
        xhat, xin = churn_in(x, eps, row)
        F = fwd(xin, torch.full((b,), float(row[E.C_NOISE])))
        _, d, x, xin2 = euler(xhat, F, row, clamp)
        if float(row[E.SIGMA2]) != 0.0:
            F2 = fwd(xin2, torch.full((b,), float(row[E.C_NOISE2])))
            x = heun(xhat, d, x, F2, row, clamp)
    return finalize(x)


def dpmpp_sample(fwd, table, sigma_init, shape, noise):
    b = shape[0]
    x = _f(sigma_init) * noise(shape)
    d_old = torch.zeros(shape)
    for row in table:
        _, xin = churn_in(x, None, row)
        F = fwd(xin, torch.full((b,), float(row[E.C_NOISE])))
        x, d_old = dpmpp(x, F, d_old, row)
    return finalize(x)
