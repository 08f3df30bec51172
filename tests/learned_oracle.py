"""CPU restatement of the learned-variance passes as the HIP path runs them: driven by the host tables (``lv_step_table`` /
``lv_train_table``), with the arithmetic of the kernels in csrc/learned.hip on CPU tensors, in the dtype asked for (fp32 as
the kernels, or fp64 as the yardstick).  The loss gradient comes from autograd, not from the kernels' hand-derived
formulas.  Test helper only: the product never imports it."""
from __future__ import annotations

import math

import torch

from diffusion_models_amd import learned as L

NAT = 1.0 / math.log(2.0)
BIN = 1.0 / 255.0
EPS = 1e-15


def _c(tab, col, dtype, ndim):
    """Column `col` of a (rows, cols) table as a broadcastable tensor: one row for every image, or row b for image b."""
    return tab[:, col].to(dtype).reshape(-1, *([1] * (ndim - 1)))


def logvar(v, min_log, max_log):
    frac = (v + 1) * 0.5
    return frac * max_log + (1 - frac) * min_log


def step(x, model_out, z, row, dtype=torch.float32):
    """lv_step_kernel on one table row: (out, mean, logvar, x_start).  ``z`` is not touched where the row adds no noise."""
    row = row.reshape(1, -1)
    x, model_out = x.to(dtype), model_out.to(dtype)
    eps, v = model_out.chunk(2, dim=1)
    recip, recipm1, coef1, coef2, min_log, max_log = (
        _c(row, j, dtype, x.dim()) for j in (L.RECIP, L.RECIPM1, L.COEF1, L.COEF2, L.MIN_LOG, L.MAX_LOG))
    lv = logvar(v, min_log, max_log)
    x_start = (recip * x - recipm1 * eps).clamp(-1.0, 1.0)
    mean = coef1 * x_start + coef2 * x
    if float(row[0, L.NOISE]) == 0.0:
        return mean + (0.5 * lv).exp() * 0.0, mean, lv, x_start
    return mean + (0.5 * lv).exp() * z.to(dtype), mean, lv, x_start


def _cdf(x):
    return 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * (x * x * x))))


def _log(t):
    return torch.log(t.clamp(min=EPS))


def vb_terms(x_start, x_t, pred, v, tab, clip, dtype):
    """The per-element vb term (nats) of every image: the decoder NLL where the row's t == 0 flag is set, else the KL.
    Both branches are evaluated and selected per image (as the reference does); the model mean is detached."""
    nd = x_start.dim()
    recip, recipm1, coef1, coef2, min_log, true_log, max_log, t0 = (
        _c(tab, j, dtype, nd) for j in (L.T_RECIP, L.T_RECIPM1, L.T_COEF1, L.T_COEF2, L.T_MIN_LOG, L.T_TRUE_LOG, L.T_MAX_LOG,
                                        L.T_T0))
    lv = logvar(v, min_log, max_log)
    x0 = recip * x_t - recipm1 * pred
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    model_mean = (coef1 * x0 + coef2 * x_t).detach()
    true_mean = coef1 * x_start + coef2 * x_t
    kl = 0.5 * (-1.0 + lv - true_log + torch.exp(true_log - lv) + ((true_mean - model_mean) ** 2) * torch.exp(-lv))
    centered = x_start - model_mean
    inv_stdv = torch.exp(-(0.5 * lv))
    cdf_plus, cdf_min = _cdf(inv_stdv * (centered + BIN)), _cdf(inv_stdv * (centered - BIN))
    delta = cdf_plus - cdf_min
    log_probs = torch.where(x_start < -0.999, _log(cdf_plus), torch.where(x_start > 0.999, _log(1.0 - cdf_min), _log(delta)))
    return torch.where((t0 != 0).expand_as(kl), -log_probs, kl), lv, delta


def loss(model_out, x_start, noise, x_t, tab, vb_loss_weight, clip=False, loss_scale=1.0, dtype=torch.float32):
    """lv_loss_kernel: (loss, dout, mse_part, vb_part); dout = d loss / d model_out from autograd."""
    mo = model_out.to(dtype).clone().requires_grad_(True)
    x_start, noise, x_t = x_start.to(dtype), noise.to(dtype), x_t.to(dtype)
    pred, v = mo.chunk(2, dim=1)
    B = mo.shape[0]
    term, _, _ = vb_terms(x_start, x_t, pred, v, tab, clip, dtype)
    vb_part = term.reshape(B, -1).mean(dim=1) * NAT
    mse_part = ((pred - noise) ** 2).reshape(B, -1).mean(dim=1)
    total = (mse_part.mean() + vb_part.mean() * vb_loss_weight) * loss_scale
    total.backward()
    return total.detach(), mo.grad.detach(), mse_part.detach(), vb_part.detach()


def p_sample(fwd, x, t, row, z):
    out = fwd(x, torch.full((x.shape[0],), int(t), dtype=torch.long))
    return step(x, out, z, row)


def sample(fwd, times, table, shape, noise, unnormalize=True):
    """``fwd(x, t)``: the U-Net on a (B,) integer time.  ``noise``: draw 0 = start image, then one draw per step with t > 0."""
    x = noise(shape)
    for t, row in zip(times, table):
        z = noise(shape) if t > 0 else None
        x = p_sample(fwd, x, t, row, z)[0]
    return (x + 1) * 0.5 if unnormalize else x
