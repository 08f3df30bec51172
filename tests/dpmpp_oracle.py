"""CPU restatement of DenoisingDiffusion.dpm_solver_sample as the HIP path runs it: driven by the host step table
(``spec.dpmpp_step_table``), with exactly the arithmetic of ``dpmpp_update_kernel`` (csrc/elementwise.hip) on fp32 CPU
tensors -- the same expression tree, one rounding per tensor op, no contraction.  Test helper only: the product never
imports it.

Next to it, two float64 forms: the kernel's expression on one fp32 row (``update_f64`` with the magnitude of its terms,
for a rounding bound), and the solver of Lu et al. (arXiv 2211.01095, Algorithm 2) written straight from alphas_cumprod,
which never sees the table (``dpmpp_sample_f64``)."""
from __future__ import annotations

import math

import torch

OBJECTIVES = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}


def _f(v):
    return torch.tensor(float(v), dtype=torch.float32)


def x_start(row, objective: int, x, out, clamp=True):
    """ddpm_x_start (csrc/step_device.h): x_0 from the model output by objective, clamped."""
    if objective == 0:
        x0 = _f(row[0]) * x - _f(row[1]) * out
    elif objective == 1:
        x0 = out
    else:
        x0 = _f(row[6]) * x - _f(row[7]) * out
    return x0.clamp(-1.0, 1.0) if clamp else x0


def update(row, objective: int, x, out, hist, clamp=True):
    """dpmpp_update_kernel: (x_next, x0).  ``hist`` is not touched when row[4] == 0."""
    x0 = x_start(row, objective, x, out, clamp)
    d = x0 if float(row[4]) == 0.0 else x0 + _f(row[4]) * (x0 - hist)
    if float(row[5]) == 0.0:
        return x0, x0
    return _f(row[2]) * x + _f(row[3]) * d, x0


def update_f64(row, objective: int, x, out, hist, clamp=True):
    """The same expression in float64 on the fp32 row and fp32 inputs: (x_next, sum of the magnitudes of its terms).
    Every input reaches the result through at most seven rounded fp32 operations of ``update`` (two for x0, three for D,
    two for the result), so ``update`` lies within 8 * 2^-24 * magnitude of this value."""
    c = [float(v) for v in row]
    x, out, hist = x.double(), out.double(), hist.double()
    if objective == 0:
        x0, mag0 = c[0] * x - c[1] * out, abs(c[0]) * x.abs() + abs(c[1]) * out.abs()
    elif objective == 1:
        x0, mag0 = out, out.abs()
    else:
        x0, mag0 = c[6] * x - c[7] * out, abs(c[6]) * x.abs() + abs(c[7]) * out.abs()
    if clamp:
        x0 = x0.clamp(-1.0, 1.0)
    d, magd = x0, mag0
    if c[4] != 0.0:
        d, magd = x0 + c[4] * (x0 - hist), mag0 + abs(c[4]) * (mag0 + hist.abs())
    if c[5] == 0.0:
        return x0, mag0
    return c[2] * x + c[3] * d, abs(c[2]) * x.abs() + abs(c[3]) * magd


@torch.inference_mode()
def dpmpp_sample(fwd, times, table, shape, noise, objective="pred_noise", self_condition=False, clamp=True,
                 unnormalize=True, return_all_timesteps=False):
    """The loop of sample_impl (csrc/dm_sampler.inc) with kind DM_SAMPLER_DPMPP.  ``fwd(x, t)`` (``fwd(x, t, x_self_cond)``
    with ``self_condition``): the network on a (B,) int64 time.  ``noise`` is called once, for x_T.  The history buffer
    starts as zeros and is what self-conditioning feeds back."""
    obj = OBJECTIVES[objective]
    x = noise(shape)
    hist = torch.zeros(shape)
    frames = [x]
    for t, row in zip(times, table):
        bt = torch.full((shape[0],), int(t), dtype=torch.long)
        out = fwd(x, bt, hist) if self_condition else fwd(x, bt)
        x, hist = update(row, obj, x, out, hist, clamp)
        frames.append(x)
    ret = torch.stack(frames, dim=1) if return_all_timesteps else x
    return (ret + 1) * 0.5 if unnormalize else ret


def dpmpp_sample_f64(model, alphas_cumprod, pairs, order, x_T, objective="pred_noise", clamp=True):
    """Algorithm 2 of arXiv 2211.01095 (multistep, data prediction) in float64, from alphas_cumprod alone:
    x_next = (sigma_next / sigma_t) x - alpha_next expm1(-h) D,  D = x0 + h / (2 h_last) (x0 - x0_prev) at order 2 from the
    second step on, x_next = x0 when t_next < 0.  ``model(x, t)``: the float64 network output at integer time t.
    Returns every iterate, x_T first."""
    ac = alphas_cumprod.double()
    x = x_T.double()
    xs = [x]
    x0_prev, h_last = None, None
    for t, tn in pairs:
        a_t, s_t = math.sqrt(float(ac[t])), math.sqrt(1.0 - float(ac[t]))
        out = model(x, t)
        if objective == "pred_noise":
            x0 = (x - s_t * out) / a_t
        elif objective == "pred_x0":
            x0 = out
        else:
            x0 = a_t * x - s_t * out
        if clamp:
            x0 = x0.clamp(-1.0, 1.0)
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
