"""CPU restatement of the bits-per-dim kernels (csrc/bpd.hip) in torch, at a chosen dtype: the expression trees of the
reference's functions (``q_sample``, ``p_mean_variance``, ``q_posterior``, ``normal_kl``,
``discretized_gaussian_log_likelihood``, ``predict_noise_from_start``) on one row of ``bpd_step_table``.  In fp64 it is what
the operator tests compare the kernels with; in fp32 its own distance to fp64 sets their limit."""
from math import log as ln
from math import pi, sqrt

import torch

from diffusion_models_amd import bpd as Bp

NAT = 1.0 / ln(2)


def _row(row, dtype):
    return row.to(dtype)


def step_in(x0, z, row, dtype=torch.float64):
    c = _row(row, dtype)
    return c[Bp.SQRT_AC] * x0.to(dtype) + c[Bp.SQRT_1M_AC] * z.to(dtype)


def _cdf(x):
    return 0.5 * (1.0 + torch.tanh(sqrt(2.0 / pi) * (x + 0.044715 * (x ** 3))))


def _log(t, eps=1e-15):
    return torch.log(t.clamp(min=eps))


def nll(x, means, log_scales, thres=0.999):
    centered = x - means
    inv_stdv = torch.exp(-log_scales)
    cdf_plus = _cdf(inv_stdv * (centered + 1.0 / 255.0))
    cdf_min = _cdf(inv_stdv * (centered - 1.0 / 255.0))
    return -torch.where(x < -thres, _log(cdf_plus), torch.where(x > thres, _log(1.0 - cdf_min), _log(cdf_plus - cdf_min)))


def normal_kl(mean1, logvar1, mean2, logvar2):
    return 0.5 * (-1.0 + logvar2 - logvar1 + torch.exp(logvar1 - logvar2) + ((mean1 - mean2) ** 2) * torch.exp(-logvar2))


def x_start(model_out, x_t, c, objective, clip):
    if objective == 0:
        xs = c[Bp.RECIP] * x_t - c[Bp.RECIPM1] * model_out
    elif objective == 1:
        xs = model_out
    else:
        xs = c[Bp.SQRT_AC] * x_t - c[Bp.SQRT_1M_AC] * model_out
    return xs.clamp(-1.0, 1.0) if clip else xs


def terms(model_out, x0, x_t, z, row, learned, objective, clip, dtype=torch.float64, parts=False):
    """(B, 3): [vb in bits, mean((pred - x0)^2), mean((eps - z)^2)] per image.  ``parts``: also the per-element decoder
    argument statistics of a t == 0 row (the share of clamped pixels)."""
    c = _row(row, dtype)
    mo, x0, x_t, z = (v.to(dtype) for v in (model_out, x0, x_t, z))
    C = x0.shape[1]
    post_log = c[Bp.POST_LOG]
    if learned:
        mo, v = mo[:, :C], mo[:, C:]
        frac = (v + 1) * 0.5
        logvar = frac * c[Bp.MAX_LOG] + (1 - frac) * post_log
    else:
        logvar = post_log.expand_as(x0)
    pred = x_start(mo, x_t, c, 0 if learned else objective, clip)
    mean = c[Bp.COEF1] * pred + c[Bp.COEF2] * x_t
    true_mean = c[Bp.COEF1] * x0 + c[Bp.COEF2] * x_t
    if float(row[Bp.T0]) != 0.0:
        term = nll(x0, mean, 0.5 * logvar)
    else:
        term = normal_kl(true_mean, post_log.expand_as(x0), mean, logvar)
    eps = (c[Bp.RECIP] * x_t - pred) / c[Bp.RECIPM1]
    flat = lambda t: t.flatten(1).mean(1)  # noqa: E731
    out = torch.stack([flat(term) * NAT, flat((pred - x0) ** 2), flat((eps - z) ** 2)], dim=1)
    return (out, term) if parts else out


def prior(x0, sqrt_ac, logvar, dtype=torch.float64):
    x0 = x0.to(dtype)
    zero = torch.zeros_like(x0)
    lv = torch.full_like(x0, logvar)
    return normal_kl(torch.tensor(sqrt_ac, dtype=dtype) * x0, lv, zero, zero).flatten(1).mean(1) * NAT


def loop(model, sched, img, times, noise, learned, objective, clip, dtype=torch.float32):
    """``calc_bpd_loop`` over ``model(x_t, t_batch) -> model output``: the dict of bpd.calc_bpd_loop on the CPU."""
    times, full = Bp.bpd_times(int(sched["betas"].shape[0]), times)
    _, tab = Bp.bpd_step_table(sched, times)
    x0 = (img * 2 - 1).to(dtype)
    rows = []
    for k, t in enumerate(times):
        z = noise(tuple(x0.shape)).to(dtype)
        x_t = step_in(x0, z, tab[k], dtype)
        mo = model(x_t, torch.full((x0.shape[0],), t, dtype=torch.long))
        rows.append(terms(mo, x0, x_t, z, tab[k], learned, objective, clip, dtype))
    r = torch.stack(rows, dim=1)  # (B, n, 3)
    out = {k: r[:, :, i] for i, k in enumerate(Bp.KEYS)}
    out["prior_bpd"] = prior(x0, *Bp.prior_scalars(sched), dtype=dtype)
    out["total_bpd"] = out["vb"].sum(1) + out["prior_bpd"] if full else None
    out["times"] = times
    return out
