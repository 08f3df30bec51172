"""Bits-per-dim evaluation: the variational bound of a batch of real images, term by term (Improved DDPM, arXiv
2102.09672: ``calc_bpd_loop`` / ``_vb_terms_bpd`` / ``_prior_bpd``), written with the reference's own functions --
``q_sample``, the class's ``p_mean_variance``, ``q_posterior``, and ``normal_kl`` / ``discretized_gaussian_log_likelihood`` /
``meanflat`` / ``NAT`` of ``denoising_diffusion/learned_gaussian_diffusion.py``.  Not in the reference.

The loop runs in the library (``dm_eval_bpd``: one captured step graph per shape around the U-Net; kernels in
csrc/bpd.hip).  ``DenoisingDiffusion``, its text- and image-conditional classes and ``LearnedGaussianDiffusion`` have the
method ``calc_bpd_loop``; the other subclasses refuse it with a reason (``_bpd_refusal``).

This is not the ``hybrid_loss`` term of ``DenoisingDiffusion.p_losses``, which divides by ``posterior_variance[0] == 0`` and
is NaN at ``t == 0`` by design of the reference.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib, _loop

COLS = _lib.DM_BPD_COEFS
RECIP, RECIPM1, COEF1, COEF2, POST_LOG, T0, SQRT_AC, SQRT_1M_AC, MAX_LOG = range(9)  # BpdCol of csrc/bpd.h
KEYS = ("vb", "xstart_mse", "mse")  # the three columns of a result row


def bpd_times(num_timesteps: int, times=None) -> Tuple[List[int], bool]:
    """(the timesteps to evaluate, whether they are all of them).  ``times``: an iterable of distinct timesteps in
    [0, T); None: every timestep, descending (the order of ``calc_bpd_loop``)."""
    T = int(num_timesteps)
    if times is None:
        return list(reversed(range(T))), True
    times = [int(t) for t in times]
    if not times:
        raise ValueError("times is empty: nothing to evaluate")
    if min(times) < 0 or max(times) >= T:
        raise ValueError(f"times must lie in [0, {T}), got {min(times)} .. {max(times)}")
    if len(set(times)) != len(times):
        raise ValueError("times holds a timestep twice: a term of the bound is evaluated once")
    return times, len(times) == T


def bpd_step_table(sched: Dict[str, torch.Tensor], times=None) -> Tuple[List[int], torch.Tensor]:
    """Per-step scalars of the loop, gathered in fp32 as ``extract`` does.  Row i (time t):
    [sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, posterior_log_variance_clipped, t == 0, sqrt_ac, sqrt_1m_ac,
    log(betas), 0...]."""
    times, _ = bpd_times(int(sched["betas"].shape[0]), times)
    idx = torch.tensor(times, dtype=torch.long)
    c = torch.zeros(len(times), COLS, dtype=torch.float32)
    c[:, RECIP] = sched["sqrt_recip_alphas_cumprod"][idx]
    c[:, RECIPM1] = sched["sqrt_recipm1_alphas_cumprod"][idx]
    c[:, COEF1] = sched["posterior_mean_coef1"][idx]
    c[:, COEF2] = sched["posterior_mean_coef2"][idx]
    c[:, POST_LOG] = sched["posterior_log_variance_clipped"][idx]
    c[:, T0] = (idx == 0).to(torch.float32)
    c[:, SQRT_AC] = sched["sqrt_alphas_cumprod"][idx]
    c[:, SQRT_1M_AC] = sched["sqrt_one_minus_alphas_cumprod"][idx]
    c[:, MAX_LOG] = torch.log(sched["betas"])[idx]
    return times, c


def prior_scalars(sched: Dict[str, torch.Tensor]) -> Tuple[float, float]:
    """(sqrt_alphas_cumprod[T - 1], log(1 - alphas_cumprod[T - 1])) of the prior term, fp32 buffers of the schedule."""
    return float(sched["sqrt_alphas_cumprod"][-1]), float(sched["log_one_minus_alphas_cumprod"][-1])


def refuse(diff) -> None:
    """Raise ``NotImplementedError`` with the class's reason, or for a self-conditioned U-Net."""
    reason = getattr(diff, "_bpd_refusal", None)
    if reason is not None:
        raise NotImplementedError(f"{type(diff).__name__} has no calc_bpd_loop: {reason}")
    if getattr(diff, "self_condition", False):
        raise NotImplementedError("calc_bpd_loop is not built for Unet(self_condition=True): the bound's terms are "
                                  "p_mean_variance at one noised image each, with no previous step to condition on")


def calc_bpd_loop(diff, img, clip_denoised=True, *, times=None, noise=None, seed=None, sample_offset=0, text_emb=None,
                  cond=None, learned=False) -> Dict[str, Optional[torch.Tensor]]:
    """The loop behind the classes' ``calc_bpd_loop``.  ``img`` is what ``forward`` takes (``diff.normalize`` is applied).
    Returns Improved DDPM's dict: ``total_bpd`` (B,) (None when ``times`` is a proper subset), ``prior_bpd`` (B,), ``vb`` /
    ``xstart_mse`` / ``mse`` (B, n_times) with column k for ``times[k]``, and ``times``."""
    refuse(diff)
    times, full = bpd_times(diff.num_timesteps, times)
    img = img.to(diff.device, torch.float32)
    assert img.dim() == 4 and tuple(img.shape[2:]) == tuple(diff.image_size), (
        f"height and width of image must be {diff.image_size}")
    shape = _loop.checked_shape(diff, img.shape)
    B, _, H, W = shape
    x0 = diff.normalize(img).contiguous()
    _, table = bpd_step_table(diff._sched, times)
    n = len(times)
    if seed is None:
        seed = _lib.default_seed()
    rows = None
    if noise is not None:  # one draw per evaluated step, in loop order
        rows = torch.stack([noise(shape).to(torch.float32) for _ in times], dim=0)
        assert tuple(rows.shape[1:]) == shape, "noise() must return tensors of the image's shape"
        rows = rows.to(diff.device).contiguous()
    terms = torch.empty((n, B, 3), device=diff.device, dtype=torch.float32)
    prior = torch.empty((B,), device=diff.device, dtype=torch.float32)
    times_arr = (C.c_int64 * n)(*times)
    a = _lib.BpdArgs()
    a.learned, a.objective = int(bool(learned)), 0 if learned else diff._objective_id
    a.clip_denoised, a.n_steps = int(bool(clip_denoised)), n
    a.times_host, a.table_host = C.cast(times_arr, C.POINTER(C.c_int64)), _lib.fptr(table)
    a.x0, a.noise, a.seed, a.sample_offset = _lib.ptr(x0), _lib.ptr(rows), int(seed), int(sample_offset)
    if text_emb is not None:
        ctx, m = diff.model._ctx(text_emb, B)
        a.ctx, a.ctx_tokens = _lib.ptr(ctx), m
    if cond is not None:
        cond = cond.to(diff.device, torch.float32).contiguous()
        assert cond.shape[0] == B and tuple(cond.shape[2:]) == (H, W), "batch / size mismatch between img and cond"
        a.cond, a.cond_channels = _lib.ptr(cond), int(cond.shape[1])
    a.prior_sqrt_ac, a.prior_logvar = prior_scalars(diff._sched)
    a.terms_out, a.prior_out = _lib.ptr(terms), _lib.ptr(prior)
    a.B, a.H, a.W = B, H, W
    a.use_graph, a.stream = 1 if diff.use_graph else 0, diff._stream()
    _lib.check(diff._lib.dm_eval_bpd(diff.model._handle, C.byref(a)))
    per_image = terms.permute(1, 0, 2)  # (B, n, 3)
    out = {k: per_image[:, :, i].contiguous() for i, k in enumerate(KEYS)}
    out["prior_bpd"] = prior
    # summed in double: the total then does not depend on how a reduction of this shape happens to be ordered
    out["total_bpd"] = (out["vb"].double().sum(dim=1) + prior.double()).float() if full else None
    out["times"] = list(times)
    return out
