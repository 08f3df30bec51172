"""CPU restatement of DPM-Solver++ (2M) for the continuous-time classes as the HIP path runs it.  Test helper only: the
product never imports it.

* ``rows_f64``: the step rows from the log-SNR nodes in float64 Python scalars (``math``), written from the formulas of
  arXiv 2211.01095 (Algorithm 2) and never from ``continuous.ct_dpmpp_rows``;
* ``update``: exactly the arithmetic of ``ct_dpmpp_step_kernel`` (csrc/ct.hip) on CPU tensors in the dtype of its inputs,
  one rounding per tensor op, no contraction: on float64 inputs the reference value, on fp32 inputs (``update32``) the
  restatement a kernel output can be compared with;
* ``sample``: the loop of ``dm_sample_ct_dpmpp`` over any ``fwd(x, log_snr)``;
* ``gaussian_error``: the solver on data x0 ~ N(0, c^2), whose optimal denoiser and probability-flow solution are known
  in closed form."""
from __future__ import annotations

import math

import torch

from diffusion_models_amd import continuous as K

NOISE, V = 0, 1


def alpha_sigma(l: float):
    """alpha = sqrt(sigmoid(l)), sigma = sqrt(sigmoid(-l)) without overflow at either end."""
    sig = lambda v: 1.0 / (1.0 + math.exp(-v)) if v >= 0 else math.exp(v) / (1.0 + math.exp(v))  # noqa: E731
    return math.sqrt(sig(l)), math.sqrt(sig(-l))


def rows_f64(nodes, order=2) -> torch.Tensor:
    """(N, COLS) float64 rows on the N + 1 nodes: lambda = l / 2, h = lambda_next - lambda."""
    l = [float(v) for v in nodes]
    rows = torch.zeros((len(l) - 1, K.COLS), dtype=torch.float64)
    h_last = None
    for i in range(len(l) - 1):
        (a, s), (an, sn) = alpha_sigma(l[i]), alpha_sigma(l[i + 1])
        h = l[i + 1] / 2 - l[i] / 2
        rows[i, K.LOG_SNR], rows[i, K.ALPHA], rows[i, K.SIGMA] = l[i], a, s
        rows[i, K.DPM_CX], rows[i, K.DPM_CD] = sn / s, -an * math.expm1(-h)
        rows[i, K.DPM_G] = h / (2 * h_last) if order == 2 and h_last is not None else 0.0
        h_last = h
    return rows


def _col(tab, col, like):
    """Column `col` of a (rows, COLS) table in the dtype of `like`: one row for every image, or row b for image b."""
    tab = tab.reshape(-1, K.COLS)
    return tab[:, col].to(like.dtype).reshape(-1, *([1] * (like.dim() - 1)))


def x_start(x, F, tab, objective, clip):
    alpha, sigma = _col(tab, K.ALPHA, x), _col(tab, K.SIGMA, x)
    xs = alpha * x - sigma * F if objective == V else (x - sigma * F) / alpha
    return xs.clamp(-1.0, 1.0) if clip else xs


def update(x, F, hist, tab, objective, clip):
    """ct_dpmpp_step_kernel: (x_next, x_start).  Where g == 0 ``hist`` does not enter, whatever it holds."""
    c_x, c_d, g = (_col(tab, j, x) for j in (K.DPM_CX, K.DPM_CD, K.DPM_G))
    xs = x_start(x, F, tab, objective, clip)
    second = (g != 0).expand_as(xs)
    D = xs if hist is None else torch.where(second, xs + g * (xs - torch.nan_to_num(hist)), xs)
    assert hist is not None or not bool(second.any())
    return c_x * x + c_d * D, xs


def update32(x, F, hist, tab, objective, clip):
    """The fp32 restatement: fp32 tensors, the row's scalars rounded to fp32."""
    return update(x.float(), F.float(), None if hist is None else hist.float(), tab.float(), objective, clip)


def sample(fwd, table, x_T, objective, clip, x_starts=None):
    """(final iterate, finalized sample) in the dtype of ``x_T``; ``fwd(x, t)``: the network on a (B,) log-SNR.
    ``x_starts``: a list that receives every step's x_start."""
    x, hist = x_T, None
    for row in table:
        F = fwd(x, torch.full((x.shape[0],), float(row[K.LOG_SNR]), dtype=x.dtype))
        x, hist = update(x, F, hist, row, objective, clip)
        if x_starts is not None:
            x_starts.append(hist)
    return x, (x.clamp(-1.0, 1.0) + 1.0) * 0.5


def gaussian_error(nodes, order, objective=NOISE, c=0.5):
    """Relative L2 error of the float64 solver's final iterate on data x0 ~ N(0, c^2) against the exact probability-flow
    solution.  With var(l) = alpha^2 c^2 + sigma^2 the optimal predictions are x0* = alpha c^2 x / var and
    eps* = sigma x / var (v* = alpha eps* - sigma x0*), and the exact solution scales as sqrt(var)."""
    nodes = [float(v) for v in nodes]
    var = {l: alpha_sigma(l)[0] ** 2 * c * c + alpha_sigma(l)[1] ** 2 for l in nodes}

    def fwd(x, t):
        l = float(t[0])
        a, s = alpha_sigma(l)
        eps, x0 = s / var[l] * x, a * c * c / var[l] * x
        return a * eps - s * x0 if objective == V else eps

    x_T = torch.randn((1, 1, 8, 8), generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    got, _ = sample(fwd, rows_f64(nodes, order), x_T, objective, False)
    want = x_T * math.sqrt(var[nodes[-1]] / var[nodes[0]])
    return float((got - want).norm() / want.norm())
