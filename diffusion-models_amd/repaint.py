"""RePaint inpainting (arXiv 2201.09865) as the reference has it: ``denoising_diffusion/repaint.py``.

``GaussianDiffusion`` is ``DenoisingDiffusion`` with the reference's other defaults (``objective='pred_v'``,
``beta_schedule='sigmoid'``, the loss weight always derived from the SNR) and a ``sample()`` that always runs the DDPM
loop.  Given a ground-truth image ``gt`` in [0, 1] and a ``mask`` (1 = keep), ``sample`` / ``p_sample_loop`` /
``p_sample`` keep the masked pixels and generate the rest (:614-681).  Without a mask every method is the parent's.

The loop is unrolled on the host (``repaint_step_table``) into one flat list of rows, one U-Net evaluation each, and run by
``dm_sample_repaint``: one captured step graph replayed per row, whose single elementwise kernel does the DDPM update of
the row and the jump / known-region blend in front of the next one (csrc/repaint.hip).

Quirks of the reference that are kept: ``gt`` is normalised with ``2 gt - 1`` whatever ``auto_normalize``
is; the known region gets fresh noise in every ``p_sample`` call, ``t == 0`` included; the jump of a resample iteration is
ONE forward step with ``betas[resample_jump]``, followed by ``resample_jump`` steps that all run at the constant time
``resample_jump``; ``sample()`` defaults to ``resample_jump=10`` and ``p_sample_loop`` to 3.  Not mirrored: a mask with
``Unet(self_condition=True)`` raises ``NotImplementedError`` (the reference's inner resample calls drop ``x_self_cond``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple

import torch

from . import _lib, _loop
from .diffusion import DenoisingDiffusion
from .spec import ddpm_step_table

COLS = _lib.DM_REPAINT_COEFS
KNOWN_GT, KNOWN_Z, JUMP_X, JUMP_Z, JUMP, SLOT = 8, 9, 10, 11, 12, 13
BLEND, STEP, STEP_NEXT, LAST = 1, 2, 3, 4  # DM_REPAINT_* of include/dm_hip.h


def draw_ids(row: int):
    """Philox draw ids of row ``row`` (draw 0 is x_T): (jump in front of the row, known-region noise, step noise)."""
    return 3 * row + 1, 3 * row + 2, 3 * row + 3


class RepaintTable(NamedTuple):
    times: List[int]     # the integer time of every row
    coefs: torch.Tensor  # (rows, 16) fp32: DM_REPAINT_COEFS columns of include/dm_hip.h
    n_frames: int        # entries of the reference's ``imgs`` list: 1 + T + resample events


def repaint_step_table(sched: Dict[str, torch.Tensor], resample=True, resample_iter=10, resample_jump=10,
                       resample_every=50) -> RepaintTable:
    """The masked ``p_sample_loop`` of repaint.py:644-681 as a flat list of rows, one per U-Net evaluation.

    Row columns: 0..7 the DDPM coefficients of ``ddpm_step_table`` at the row's time; 8, 9 the known-region weights
    ``sqrt(ac[t])``, ``sqrt(1 - ac[t])``; 10, 11 the jump pair ``sqrt(1 - betas[j])``, ``sqrt(betas[j])`` and 12 = 1 on a row
    that opens a resample iteration (else 1, 0, 0); 13 the ``imgs`` entry the row's result becomes, or -1.  The scalars are
    the reference's own fp32 tensor expressions on the registered fp32 buffers."""
    T = int(sched["betas"].shape[0])
    does = resample is True  # the reference tests `resample is True`
    if does:
        if isinstance(resample_jump, bool) or not isinstance(resample_jump, int) or not 1 <= resample_jump <= T - 1:
            raise ValueError(f"resample_jump must be an integer in [1, {T - 1}] (it indexes betas and is a time), got "
                             f"{resample_jump!r}")
        if isinstance(resample_iter, bool) or not isinstance(resample_iter, int) or resample_iter < 1:
            raise ValueError(f"resample_iter must be a positive integer (pass resample=False for none), got {resample_iter!r}")
        if isinstance(resample_every, bool) or not isinstance(resample_every, int) or resample_every < 1:
            raise ValueError(f"resample_every must be a positive integer, got {resample_every!r}")
    _, ddpm = ddpm_step_table(sched)  # row i is t = T - 1 - i
    ac, betas = sched["alphas_cumprod"], sched["betas"]
    times: List[int] = []
    jumps: List[bool] = []
    slots: List[int] = []
    frame = 0  # imgs[0] is x_T
    for t in reversed(range(T)):
        frame += 1
        times.append(t)
        jumps.append(False)
        slots.append(frame)
        if does and t > 0 and (t % resample_every == 0 or t == 1):
            frame += 1  # one more entry after the whole block: the last inner row's result
            for it in range(resample_iter):
                for j in range(resample_jump):
                    times.append(resample_jump)
                    jumps.append(j == 0)
                    slots.append(frame if (it == resample_iter - 1 and j == resample_jump - 1) else -1)
    idx = torch.tensor(times)
    c = torch.zeros(len(times), COLS, dtype=torch.float32)
    c[:, :8] = ddpm[T - 1 - idx]
    c[:, KNOWN_GT] = torch.sqrt(ac[idx])
    c[:, KNOWN_Z] = torch.sqrt(1 - ac[idx])
    c[:, JUMP_X] = 1.0
    if any(jumps):
        beta = betas[resample_jump]
        jm = torch.tensor(jumps)
        c[jm, JUMP_X] = torch.sqrt(1 - beta)
        c[jm, JUMP_Z] = torch.sqrt(beta)
        c[jm, JUMP] = 1.0
    c[:, SLOT] = torch.tensor(slots, dtype=torch.float32)
    return RepaintTable(times, c, frame + 1)


class GaussianDiffusion(DenoisingDiffusion):
    """``repaint.GaussianDiffusion`` (repaint.py:423-840): the reference's constructor signature and defaults, plus
    ``use_graph``.  ``dpm_solver_sample`` is the parent's, inherited as ``ddim_sample`` is: it takes no ``gt`` / ``mask``
    and samples unmasked; inpainting is the DDPM loop only."""

    def __init__(
        self,
        model,
        *,
        image_size,
        timesteps=1000,
        sampling_timesteps=None,
        objective="pred_v",
        beta_schedule="sigmoid",
        schedule_fn_kwargs=dict(),
        ddim_sampling_eta=0.0,
        auto_normalize=True,
        offset_noise_strength=0.0,
        min_snr_loss_weight=False,
        min_snr_gamma=5,
        use_graph=True,
    ):
        assert not (type(self) == GaussianDiffusion and model.channels != model.out_dim)
        super().__init__(model, image_size=image_size, timesteps=timesteps, sampling_timesteps=sampling_timesteps,
                         objective=objective, beta_schedule=beta_schedule, schedule_fn_kwargs=schedule_fn_kwargs,
                         ddim_sampling_eta=ddim_sampling_eta, auto_normalize=auto_normalize, use_graph=use_graph,
                         offset_noise_strength=offset_noise_strength, min_snr_loss_weight=min_snr_loss_weight,
                         min_snr_gamma=min_snr_gamma, ddpm=False)  # the loss weight always comes from the SNR (:522-535)

    # -- helpers ----------------------------------------------------------------------------------------------------------
    def _masked_inputs(self, shape, gt, mask):
        if self.self_condition:
            raise NotImplementedError("RePaint with Unet(self_condition=True) is not supported: the reference's inner "
                                      "resample calls drop x_self_cond, which is not mirrored")
        B, Cc, H, W = shape
        if gt is None:
            raise ValueError("a mask needs the ground-truth image gt")
        mask = mask.to(self.device, torch.float32).contiguous()
        gt = gt.to(self.device, torch.float32).contiguous()
        if tuple(gt.shape) != tuple(shape):
            raise ValueError(f"gt {tuple(gt.shape)} does not match the sampled shape {tuple(shape)}")
        if mask.dim() != 4 or mask.shape[0] != B or tuple(mask.shape[2:]) != (H, W) or mask.shape[1] not in (1, Cc):
            raise ValueError(f"mask {tuple(mask.shape)} must be ({B}, 1 or {Cc}, {H}, {W})")
        return gt, mask

    _dyn_refusal = NotImplementedError  # dynamic_threshold: this class's loop has its own update kernel
    _bpd_refusal = ("RePaint is an inpainting sampler over a mask and a known image; it defines no bound on "
                    "data")

    # -- the loop ---------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def p_sample_loop(self, shape, return_all_timesteps=False, gt=None, mask=None, resample=True, resample_iter=10,
                      resample_jump=3, resample_every=50, *, noise=None, seed=None, sample_offset=0, **kw):
        """:644-681.  ``noise`` (a callable ``shape -> cpu tensor``) is called in the reference's draw order: x_T, then per
        row [z_jump], z_known, [z_step]."""
        self._dyn(kw.get("dynamic_threshold"))
        if mask is None:
            return super().p_sample_loop(shape, return_all_timesteps, noise=noise, seed=seed, sample_offset=sample_offset, **kw)
        if kw:
            raise TypeError(f"unexpected keyword arguments with a mask: {sorted(kw)}")
        shape = _loop.checked_shape(self, shape)
        gt, mask = self._masked_inputs(shape, gt, mask)
        tab = repaint_step_table(self._sched, resample, resample_iter, resample_jump, resample_every)
        slots = torch.stack([tab.coefs[:, JUMP] != 0, torch.ones(len(tab.times), dtype=torch.bool), tab.coefs[:, 5] != 0], dim=1)
        start = _loop.loop_start(self, shape, noise, seed, sample_offset, slots)
        a = _lib.RepaintArgs()
        a.objective, a.n_rows, a.n_frames = self._objective_id, len(tab.times), tab.n_frames
        a.gt, a.mask, a.mask_channels = _lib.ptr(gt), _lib.ptr(mask), int(mask.shape[1])
        # unnormalize=False with all frames: they are unnormalised together after the call
        return _loop.loop_call(self, a, self._lib.dm_sample_repaint, shape, start, sample_offset, tab.times, tab.coefs,
                               "table_host", tab.n_frames, return_all_timesteps,
                               unnormalize=False if return_all_timesteps else None)

    @torch.inference_mode()
    def sample(self, batch_size=16, return_all_timesteps=False, gt=None, mask=None, resample=True, resample_iter=10,
               resample_jump=10, resample_every=50, *, noise=None, seed=None, sample_offset=0, **kw):
        """:725-748: always the DDPM loop, whatever ``sampling_timesteps`` says; the batch size is the mask's."""
        (h, w), channels = self.image_size, self.channels
        batch_size = mask.shape[0] if mask is not None else batch_size
        return self.p_sample_loop((batch_size, channels, h, w), return_all_timesteps=return_all_timesteps, gt=gt, mask=mask,
                                  resample=resample, resample_iter=resample_iter, resample_jump=resample_jump,
                                  resample_every=resample_every, noise=noise, seed=seed, sample_offset=sample_offset, **kw)

    @torch.inference_mode()
    def p_sample(self, x, t: int, x_self_cond=None, gt=None, mask=None, *, noise=None):
        """:614-642.  Returns (pred_img, x_start).  ``noise`` draws z_known, then z_step when t > 0."""
        if mask is None:
            return super().p_sample(x, t, x_self_cond, noise=noise)
        t = int(t)
        x = x.to(self.device, torch.float32).contiguous()
        shape = tuple(x.shape)
        b, c, h, w = shape
        gt, mask = self._masked_inputs(shape, gt, mask)
        assert x_self_cond is None, "the model was built without self_condition"
        s = self._sched
        row = torch.zeros(COLS, dtype=torch.float32)
        row[:8] = ddpm_step_table(s)[1][self.num_timesteps - 1 - t]
        row[KNOWN_GT], row[KNOWN_Z] = torch.sqrt(s["alphas_cumprod"][t]), torch.sqrt(1 - s["alphas_cumprod"][t])
        row[JUMP_X], row[SLOT] = 1.0, -1.0
        coef = _lib.fptr(row)
        if noise is not None:
            z_known = noise(shape).to(self.device, torch.float32).contiguous()
            z_step = noise(shape).to(self.device, torch.float32).contiguous() if t > 0 else None
            seed = 0
        else:
            z_known = z_step = None
            seed = _lib.default_seed()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        mc = int(mask.shape[1])

        def op(mode, xin, eps, out, xs):
            _lib.check(self._lib.dm_op_repaint_step(mode, self._objective_id, _lib.ptr(xin), _lib.ptr(eps), _lib.ptr(gt),
                                                    _lib.ptr(mask), mc, None, _lib.ptr(z_known), _lib.ptr(z_step), coef, 0,
                                                    C.c_uint64(seed), C.c_uint64(0), C.c_uint64(0), _lib.ptr(out),
                                                    _lib.ptr(xs), b, c, h * w, stream))

        xb = torch.empty_like(x)
        op(BLEND, x, None, xb, None)
        eps = self._eps(xb, torch.full((b,), t, device=self.device, dtype=torch.long))
        out, x_start = torch.empty_like(x), torch.empty_like(x)
        op(LAST if t == 0 else STEP, xb, eps, out, x_start)
        return out, x_start
