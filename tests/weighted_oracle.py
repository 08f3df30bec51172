"""CPU restatement of the weighted-objective passes as the HIP path runs them: driven by the host tables (``wo_step_table``
/ ``wo_train_table``), in plain torch on CPU tensors, in the dtype asked for (fp32 as the kernels, or fp64 as the
yardstick).  The softmax is torch's; the loss gradient comes from autograd, not from the kernels' hand-derived formulas.
Test helper only: the product never imports it."""
from __future__ import annotations

import torch

from diffusion_models_amd import weighted as Wm


def _c(tab, col, dtype, ndim):
    """Column `col` of a (rows, cols) table as a broadcastable tensor: one row for every image, or row b for image b."""
    return tab[:, col].to(dtype).reshape(-1, *([1] * (ndim - 1)))


def split(model_out):
    """(pred_noise, pred_x_start, weights) of a (B, 2C + 2, ...) model output."""
    c = (model_out.shape[1] - 2) // 2
    return model_out.split((c, c, 2), dim=1)


def step(x, model_out, z, row, clip=True, dtype=torch.float32):
    """wo_step_kernel on one table row: (out, mean, x_start).  ``z`` is not touched where the row adds no noise."""
    row = row.reshape(1, -1)
    x, model_out = x.to(dtype), model_out.to(dtype)
    eps, px, w = split(model_out)
    recip, recipm1, coef1, coef2, logvar = (
        _c(row, j, dtype, x.dim()) for j in (Wm.RECIP, Wm.RECIPM1, Wm.COEF1, Wm.COEF2, Wm.LOGVAR))
    s = w.softmax(dim=1)
    x_start = s[:, :1] * (recip * x - recipm1 * eps) + s[:, 1:] * px
    if clip:
        x_start = x_start.clamp(-1.0, 1.0)
    mean = coef1 * x_start + coef2 * x
    sd = (0.5 * logvar).exp()
    if float(row[0, Wm.NOISE]) == 0.0:
        return mean + sd * 0.0, mean, x_start
    return mean + sd * z.to(dtype), mean, x_start


def loss(model_out, x_start, noise, x_t, tab, noise_w, x_start_w, loss_scale=1.0, dtype=torch.float32):
    """wo_loss_kernel: (loss, dout, weighted_part, x_start_part, noise_part, xs); dout = d loss / d model_out from
    autograd; xs = predict_start_from_noise before the clamp at +-2 (the tests look at where it falls)."""
    mo = model_out.to(dtype).clone().requires_grad_(True)
    x_start, noise, x_t = x_start.to(dtype), noise.to(dtype), x_t.to(dtype)
    pn, px, w = split(mo)
    B = mo.shape[0]
    recip, recipm1 = (_c(tab, j, dtype, x_t.dim()) for j in (Wm.T_RECIP, Wm.T_RECIPM1))
    xs = recip * x_t - recipm1 * pn
    s = w.softmax(dim=1)
    wx = s[:, :1] * xs.clamp(-2.0, 2.0) + s[:, 1:] * px
    w_part = ((x_start - wx) ** 2).reshape(B, -1).mean(dim=1)
    x_part = ((x_start - px) ** 2).reshape(B, -1).mean(dim=1)
    n_part = ((noise - pn) ** 2).reshape(B, -1).mean(dim=1)
    total = (w_part.mean() + x_part.mean() * x_start_w + n_part.mean() * noise_w) * loss_scale
    total.backward()
    return total.detach(), mo.grad.detach(), w_part.detach(), x_part.detach(), n_part.detach(), xs.detach()


def p_mean_variance(fwd, x, t, row, clip=True):
    """(model_mean, x_start) at one time ``t`` for the whole batch."""
    out = fwd(x, torch.full((x.shape[0],), int(t), dtype=torch.long))
    _, mean, x_start = step(x, out, None, row.clone().index_fill_(0, torch.tensor([Wm.NOISE]), 0.0), clip)
    return mean, x_start


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
