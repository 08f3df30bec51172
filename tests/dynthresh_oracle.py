"""CPU restatement of dynamic thresholding (Imagen, arXiv 2205.11487, section 2.3) as the HIP path runs it.  Test helper
only: the product never imports it.

The rule, per image b:  s_b = max(1, quantile_p(|x_start_raw| over (C, H, W))),  x_start = clamp(x_start_raw, -s_b, s_b) / s_b.
The quantile is torch.quantile's with linear interpolation, written out with a sort: pos = p (n - 1), lo = floor(pos),
hi = min(lo + 1, n - 1), frac = float(pos - lo) -- all formed in float64 on the host -- and q = v_lo + frac * (v_hi - v_lo)
in the dtype of the data, one rounding per operation (what ``dyn_threshold_kernel`` computes in fp32, csrc/dynthresh.hip).
An image that holds a NaN has s = NaN.

Two kinds of restatement:
* fp32, operation for operation what the kernels do (``threshold``, ``x_start_dyn``, ``sampler_update``, ``dpmpp_update``):
  the operator tests compare bit for bit;
* the three loops with the threshold (``p_sample_loop``, ``ddim_sample``, ``dpmpp_sample`` on the step table, and
  ``dpmpp_sample_f64`` from alphas_cumprod alone), in the dtype of what ``noise`` returns: fp32 for the goldens, float64 for
  their twins.  With ``force_one`` every s is 1 and the loops are the existing oracle loops (oracle/sampler_oracle.py,
  tests/dpmpp_oracle.py), static clamp and all."""
from __future__ import annotations

import math

import numpy as np
import torch

import dpmpp_oracle as do
from oracle import sampler_oracle as so

OBJECTIVES = do.OBJECTIVES


def quantile_params(p: float, n: int):
    """(lo, hi, frac) of the quantile p over n values; frac rounded to fp32 as the library uploads it."""
    pos = np.float64(p) * np.float64(n - 1)
    lo = int(np.floor(pos))
    hi = min(lo + 1, n - 1)
    return lo, hi, float(np.float32(pos - np.float64(lo)))


def threshold(raw: torch.Tensor, p: float, force_one: bool = False) -> torch.Tensor:
    """s (B,) of a batch of unclamped x_start estimates (B, ...), in raw's dtype."""
    b = raw.shape[0]
    a = raw.abs().reshape(b, -1)
    if force_one:
        return torch.ones((b,), dtype=raw.dtype)
    lo, hi, frac = quantile_params(p, a.shape[1])
    v = torch.sort(a, dim=1).values  # NaNs sort last
    v_lo, v_hi = v[:, lo], v[:, hi]
    q = v_lo + torch.tensor(frac, dtype=raw.dtype) * (v_hi - v_lo)
    s = torch.where(q <= 1, torch.ones_like(q), q)
    return torch.where(torch.isnan(a).any(dim=1), torch.full_like(s, float("nan")), s)


def apply(raw: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """clamp(raw, -s_b, s_b) / s_b."""
    sb = s.reshape((-1,) + (1,) * (raw.dim() - 1))
    return torch.minimum(torch.maximum(raw, -sb), sb) / sb


# ---- fp32, as the kernels compute ----------------------------------------------------------------------------------------
def _f(v):
    return torch.tensor(float(v), dtype=torch.float32)


def x_start_dyn(row, objective: int, x, out, s):
    """ddpm_x_start_dyn (csrc/step_device.h) on (B, ...) tensors."""
    return apply(do.x_start(row, objective, x, out, clamp=False), s)


def sampler_update(kind: int, row, objective: int, x, out, z, s=None):
    """sampler_update_kernel (csrc/elementwise.hip), kind 0 DDPM / 1 DDIM: (x_next, x_start).  s = None: the static clamp."""
    x0 = do.x_start(row, objective, x, out, clamp=True) if s is None else x_start_dyn(row, objective, x, out, s)
    noisy = float(row[5]) != 0.0
    zz = z if noisy and z is not None else torch.zeros_like(x)
    if kind == 0:
        mean = _f(row[2]) * x0 + _f(row[3]) * x
        return mean + _f(row[4]) * zz, x0
    if not noisy:
        return x0, x0
    e2 = (_f(row[0]) * x - x0) / _f(row[1])
    return (x0 * _f(row[2]) + _f(row[3]) * e2) + _f(row[4]) * zz, x0


def dpmpp_update(row, objective: int, x, out, hist, s=None):
    """dpmpp_update_kernel: (x_next, x_start)."""
    x0 = do.x_start(row, objective, x, out, clamp=True) if s is None else x_start_dyn(row, objective, x, out, s)
    d = x0 if float(row[4]) == 0.0 else x0 + _f(row[4]) * (x0 - hist)
    if float(row[5]) == 0.0:
        return x0, x0
    return _f(row[2]) * x + _f(row[3]) * d, x0


# ---- the loops, in the dtype of the noise ----------------------------------------------------------------------------------
def _sched(sched, dtype):
    return {k: v.to(dtype) if torch.is_floating_point(v) else v for k, v in sched.items()}


def _x_start(fwd, sched, x, t, objective, sc, p, force_one, log):
    raw = so.model_x_start(fwd, sched, x, t, objective, sc)
    s = threshold(raw, p, force_one)
    if log is not None:
        log.append(s.clone())
    return apply(raw, s)


@torch.inference_mode()
def p_sample(fwd, sched, x, t: int, z, p, objective="pred_noise", x_self_cond=None, force_one=False, log=None):
    """oracle.sampler_oracle.p_sample with the thresholded x_start: (x_next, x_start)."""
    x0 = _x_start(fwd, sched, x, t, objective, x_self_cond, p, force_one, log)
    mean = sched["posterior_mean_coef1"][t] * x0 + sched["posterior_mean_coef2"][t] * x
    std = (0.5 * sched["posterior_log_variance_clipped"][t]).exp()
    return (mean + std * z if t > 0 else mean + std * 0.0), x0


@torch.inference_mode()
def p_sample_loop(fwd, sched, shape, noise, p, objective="pred_noise", self_condition=False, unnormalize=True,
                  force_one=False, log=None):
    """oracle.sampler_oracle.p_sample_loop with the threshold.  ``log`` (a list) receives s of every step."""
    img = noise(shape)
    sched = _sched(sched, img.dtype)
    x_start = None
    for t in reversed(range(sched["betas"].shape[0])):
        z = noise(shape) if t > 0 else None
        sc = (x_start if x_start is not None else torch.zeros_like(img)) if self_condition else None
        img, x_start = p_sample(fwd, sched, img, t, z, p, objective, sc, force_one, log)
    return (img + 1) * 0.5 if unnormalize else img


@torch.inference_mode()
def ddim_sample(fwd, sched, shape, noise, sampling_timesteps, p, eta=0.0, objective="pred_noise", self_condition=False,
                unnormalize=True, force_one=False, log=None):
    """oracle.sampler_oracle.ddim_sample with the threshold: pred_noise is re-derived from the thresholded x_start."""
    img = noise(shape)
    sched = _sched(sched, img.dtype)
    ac = sched["alphas_cumprod"]
    x0 = None
    for t, t_next in so.ddim_pairs(sched["betas"].shape[0], sampling_timesteps):
        sc = (x0 if x0 is not None else torch.zeros_like(img)) if self_condition else None
        x0 = _x_start(fwd, sched, img, t, objective, sc, p, force_one, log)
        eps = so.predict_noise_from_start(sched, img, t, x0)
        if t_next < 0:
            img = x0
            continue
        alpha, alpha_next = ac[t], ac[t_next]
        sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        c = (1 - alpha_next - sigma ** 2).sqrt()
        z = noise(shape)
        img = x0 * alpha_next.sqrt() + c * eps + sigma * z
    return (img + 1) * 0.5 if unnormalize else img


@torch.inference_mode()
def dpmpp_sample(fwd, times, table, shape, noise, p, objective="pred_noise", self_condition=False, unnormalize=True,
                 force_one=False, log=None):
    """tests/dpmpp_oracle.dpmpp_sample (fp32, on the host step table) with the threshold."""
    obj = OBJECTIVES[objective]
    x = noise(shape)
    hist = torch.zeros(shape)
    for t, row in zip(times, table):
        bt = torch.full((shape[0],), int(t), dtype=torch.long)
        out = fwd(x, bt, hist) if self_condition else fwd(x, bt)
        s = threshold(do.x_start(row, obj, x, out, clamp=False), p, force_one)
        if log is not None:
            log.append(s.clone())
        x, hist = dpmpp_update(row, obj, x, out, hist, s)
    return (x + 1) * 0.5 if unnormalize else x


@torch.inference_mode()
def dpmpp_sample_f64(model, alphas_cumprod, pairs, order, x_T, p, objective="pred_noise", force_one=False, log=None):
    """tests/dpmpp_oracle.dpmpp_sample_f64 (Algorithm 2 of arXiv 2211.01095 from alphas_cumprod alone) with the threshold.
    ``model(x, t)``: the float64 network output at integer time t.  Returns every iterate, x_T first."""
    ac = alphas_cumprod.double()
    x = x_T.double()
    xs = [x]
    x0_prev, h_last = None, None
    for t, tn in pairs:
        a_t, s_t = math.sqrt(float(ac[t])), math.sqrt(1.0 - float(ac[t]))
        out = model(x, t)
        if objective == "pred_noise":
            raw = (x - s_t * out) / a_t
        elif objective == "pred_x0":
            raw = out
        else:
            raw = a_t * x - s_t * out
        s = threshold(raw, p, force_one)
        if log is not None:
            log.append(s.clone())
        x0 = apply(raw, s)
        if tn < 0:
            x = x0
        else:
            a_n, s_n = math.sqrt(float(ac[tn])), math.sqrt(1.0 - float(ac[tn]))
            h = math.log(a_n / s_n) - math.log(a_t / s_t)
            d = x0
            if order == 2 and x0_prev is not None:
                d = x0 + h / (2.0 * h_last) * (x0 - x0_prev)
            x = (s_n / s_t) * x - a_n * math.expm1(-h) * d
            h_last = h
        x0_prev = x0
        xs.append(x)
    return xs
