"""Weighted-objective Gaussian diffusion as the reference has it:
``denoising_diffusion/weighted_objective_gaussian_diffusion.py``.

``Unet(out_dim = 2 * channels + 2)`` predicts the noise, x_start and two weight maps.  The softmax over the two weights at a
pixel blends the x_start derived from the predicted noise with the predicted x_start; the reverse step runs on that blend
(``dm_sample_wo``: one captured step graph whose single elementwise kernel is ``wo_step_kernel``, csrc/weighted.hip), and
training regresses the blend on x_start and adds the two plain MSE terms, each with its weight
(``dm_unet_loss_backward_wo``: ``wo_loss_kernel`` writes the loss and its gradient in one pass).

Kept from the reference: ``objective``, ``offset_noise_strength``, ``min_snr_loss_weight`` and
``hybrid_loss`` are accepted and have NO effect; ``clip_denoised`` of ``p_losses`` is accepted and unused;
``p_mean_variance`` ignores a passed ``model_output`` and always calls the model; DDIM is refused by the constructor.  The
reference's file calls ``F.mse_loss`` without importing ``F``: training is built here as the file is written, ``F`` being
``torch.nn.functional`` as in the base module.

ONE STATED DEVIATION: in the reference ``sample()`` raises ``TypeError`` -- the base ``p_sample``
(denoising_diffusion.py:638-645) passes ``x_self_cond=`` to ``p_mean_variance`` and unpacks four values, which this class's
``p_mean_variance`` neither accepts nor returns.  ``p_sample`` / ``p_sample_loop`` / ``sample`` here are the base class's
DDPM loop with the single adaptation that call needs: ``p_mean_variance(x=, t=, clip_denoised=True)`` without
``x_self_cond``, three values, and the clamped weighted x_start as ``x_start``.

``channels > 3`` (``out_dim > 8``, beyond the thin-output ``final_conv`` kernels) and ``immiscible=True`` raise
``NotImplementedError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import torch

from . import _lib, _loop
from .diffusion import DenoisingDiffusion

COLS = _lib.DM_WO_COEFS
RECIP, RECIPM1, COEF1, COEF2, LOGVAR, NOISE = range(6)  # WoCol of csrc/weighted.h
TRAIN_COLS = _lib.DM_WO_TRAIN_COEFS
T_SQRT_AC, T_SQRT_1M_AC, T_RECIP, T_RECIPM1 = range(4)  # WoTrainCol of csrc/weighted.h

_NO_DDIM = ("WeightedObjectiveGaussianDiffusion has no {}: the constructor asserts 'ddim sampling cannot be used' "
            "(weighted_objective_gaussian_diffusion.py:27) and p_mean_variance is the only prediction path")


def wo_step_table(sched: Dict[str, torch.Tensor], times=None) -> Tuple[List[int], torch.Tensor]:
    """Per-step scalars of ``p_sample_loop`` over ``p_mean_variance`` (:33-49), gathered in fp32 as ``extract`` does.
    Row i (t = T-1-i): [sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, posterior_log_variance_clipped, t > 0, 0...] -- the
    columns the learned-variance step table shares.  ``times``: the rows to build, when not the whole loop."""
    if times is None:
        times = reversed(range(int(sched["betas"].shape[0])))
    times = [int(t) for t in times]
    idx = torch.tensor(times, dtype=torch.long)
    c = torch.zeros(len(times), COLS, dtype=torch.float32)
    c[:, RECIP] = sched["sqrt_recip_alphas_cumprod"][idx]
    c[:, RECIPM1] = sched["sqrt_recipm1_alphas_cumprod"][idx]
    c[:, COEF1] = sched["posterior_mean_coef1"][idx]
    c[:, COEF2] = sched["posterior_mean_coef2"][idx]
    c[:, LOGVAR] = sched["posterior_log_variance_clipped"][idx]
    c[:, NOISE] = (idx > 0).to(torch.float32)
    return times, c


def wo_train_table(sched: Dict[str, torch.Tensor], t: torch.Tensor) -> torch.Tensor:
    """(B, 12): what ``extract`` gathers at each image's timestep for ``q_sample`` (columns 0, 1) and
    ``predict_start_from_noise`` (columns 2, 3); the rest 0."""
    t = t.detach().to("cpu", torch.long).reshape(-1)
    c = torch.zeros(t.shape[0], TRAIN_COLS, dtype=torch.float32)
    c[:, T_SQRT_AC] = sched["sqrt_alphas_cumprod"][t]
    c[:, T_SQRT_1M_AC] = sched["sqrt_one_minus_alphas_cumprod"][t]
    c[:, T_RECIP] = sched["sqrt_recip_alphas_cumprod"][t]
    c[:, T_RECIPM1] = sched["sqrt_recipm1_alphas_cumprod"][t]
    return c


class WeightedObjectiveGaussianDiffusion(DenoisingDiffusion):
    """``WeightedObjectiveGaussianDiffusion`` (weighted_objective_gaussian_diffusion.py:14-74): the reference's signature --
    the two loss weights are keyword-only, the rest is ``DenoisingDiffusion``'s."""

    def __init__(self, model, *args, pred_noise_loss_weight=0.1, pred_x_start_loss_weight=0.1, **kwargs):
        super().__init__(model, *args, **kwargs)
        channels = model.channels
        assert model.out_dim == (channels * 2 + 2), (
            "dimension out (out_dim) of unet must be twice the number of channels + 2 (for the softmax weighted sum) - for "
            "channels of 3, this should be (3 * 2) + 2 = 8")
        assert not model.self_condition, "not supported yet"
        assert not self.is_ddim_sampling, "ddim sampling cannot be used"
        if self.immiscible:
            raise NotImplementedError("immiscible=True is not built for WeightedObjectiveGaussianDiffusion")
        if channels > 3:
            raise NotImplementedError(f"channels={channels} gives out_dim={2 * channels + 2} > 8: the thin-output final_conv "
                                      "kernels stop at 8 outputs, so WeightedObjectiveGaussianDiffusion is built for channels <= 3")
        self.split_dims = (channels, channels, 2)
        self.pred_noise_loss_weight = pred_noise_loss_weight
        self.pred_x_start_loss_weight = pred_x_start_loss_weight

    # -- what the class does not have --------------------------------------------------------------------------------------
    def model_predictions(self, *args, **kwargs):
        raise NotImplementedError(_NO_DDIM.format("model_predictions"))

    def ddim_sample(self, *args, **kwargs):
        raise NotImplementedError(_NO_DDIM.format("ddim_sample"))

    def ddim_sample_guided(self, *args, **kwargs):
        raise NotImplementedError(_NO_DDIM.format("ddim_sample_guided"))

    def dpm_solver_sample(self, *args, **kwargs):
        raise NotImplementedError(_NO_DDIM.format("dpm_solver_sample (the model output is a softmax blend of two predictions, "
                                                  "not the plain prediction DPM-Solver++ steps on)"))

    _dyn_refusal = NotImplementedError  # dynamic_threshold: this class's loop has its own update kernel
    _bpd_refusal = ("the weighted-objective p_mean_variance blends two predictions per pixel; Improved DDPM's "
                    "bound is not defined for it here")

    # -- sampling ---------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def p_sample_loop(self, shape, return_all_timesteps=False, *, noise=None, seed=None, max_steps=None, sample_offset=0,
                      dynamic_threshold=None):
        """denoising_diffusion.py:647-664 over the p_mean_variance of :33-49 (the module docstring's deviation).  ``noise``
        (a callable ``shape -> cpu tensor``) is called in the reference's draw order: x_T, then one per step with t > 0."""
        self._dyn(dynamic_threshold)
        shape = _loop.checked_shape(self, shape)
        times = list(reversed(range(self.num_timesteps)))
        if max_steps is not None:  # bounded run: the first `max_steps` iterations only
            times = times[:max(int(max_steps), 0)]
        times, coefs = wo_step_table(self._sched, times)
        start = _loop.loop_start(self, shape, noise, seed, sample_offset, [t > 0 for t in times])
        a = _lib.WoArgs()
        a.n_steps = len(times)
        return _loop.loop_call(self, a, self._lib.dm_sample_wo, shape, start, sample_offset, times, coefs, "table_host",
                               len(times) + 1, return_all_timesteps)

    @torch.inference_mode()
    def sample(self, batch_size=16, return_all_timesteps=False, **kw):
        """denoising_diffusion.py:779-783; the constructor has refused DDIM, so this is always the DDPM loop."""
        (h, w), channels = self.image_size, self.channels
        return self.p_sample_loop((batch_size, channels, h, w), return_all_timesteps=return_all_timesteps, **kw)

    def _step(self, x, t, z, clip, seed=0):
        """The model at the per-call time ``t`` (an int) and ``dm_op_wo_step``: (pred_img, model_mean, x_start)."""
        t = int(t)
        x = x.to(self.device, torch.float32).contiguous()
        b, c = x.shape[0], x.shape[1]
        model_output = self.model(x, torch.full((b,), t, device=self.device, dtype=torch.long))
        model_output = model_output.to(self.device, torch.float32).contiguous()
        assert tuple(model_output.shape) == (b, 2 * c + 2) + tuple(x.shape[2:]), "the model output is (B, 2C + 2, H, W)"
        row = wo_step_table(self._sched, [t])[1][0].contiguous()
        outs = [torch.empty_like(x) for _ in range(3)]
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_op_wo_step(_lib.ptr(x), _lib.ptr(model_output), _lib.ptr(z), _lib.fptr(row), int(bool(clip)),
                                           C.c_uint64(seed), C.c_uint64(1), C.c_uint64(0), *[_lib.ptr(o) for o in outs], b, c,
                                           x[0, 0].numel(), stream))
        return outs

    @torch.inference_mode()
    def p_mean_variance(self, *, x, t, clip_denoised, model_output=None):
        """:33-49: (model_mean, posterior_variance, posterior_log_variance_clipped), the last two shaped (B, 1, 1, 1) as
        ``extract`` returns them.  ``model_output`` is IGNORED and the model is always called, as in the reference (:34).
        ``t`` is the reference's (B,) tensor (or an int); the images are grouped by their timestep, one model call and one
        kernel launch per distinct value."""
        x = x.to(self.device, torch.float32).contiguous()
        bt = self._bt(t, x.shape[0])
        mean = torch.empty_like(x)
        for tv in sorted(set(bt.tolist())):
            sel = (bt == tv).nonzero().reshape(-1).to(self.device)
            mean[sel] = self._step(x[sel], tv, None, clip_denoised)[1]  # (the step's own draw goes into the unused pred_img)
        return mean, self._ext("posterior_variance", bt, x), self._ext("posterior_log_variance_clipped", bt, x)

    @torch.inference_mode()
    def p_sample(self, x, t: int, x_self_cond=None, *, noise=None):
        """denoising_diffusion.py:638-645 over :33-49, adapted as the module docstring says.  Returns (pred_img, x_start),
        x_start being the clamped weighted one; ``noise`` draws once when t > 0."""
        assert x_self_cond is None, "the model was built without self_condition"
        t = int(t)
        z, seed = None, 0
        if t > 0:
            if noise is not None:
                z = noise(tuple(x.shape)).to(self.device, torch.float32).contiguous()
            else:
                seed = _lib.default_seed()
        out, _, x_start = self._step(x, t, z, True, seed)
        return out, x_start

    # -- training ---------------------------------------------------------------------------------------------------------
    def p_losses(self, x_start, t, noise=None, clip_denoised=False, *, loss_scale=1.0, accumulate=False, sync=True,
                 return_model_out=False):
        """:51-74: ``mse(x_start, weighted) + w_x mse(x_start, pred_x_start) + w_n mse(noise, pred_noise)`` and every
        parameter gradient, in one call of the library (the gradients stay on the model: ``self.model.grad(name)``).
        ``clip_denoised`` is accepted and unused, as in the reference.  ``loss_scale`` / ``accumulate`` are the micro-batch
        loop of ``Trainer.train``; ``sync=False`` returns the loss as a 0-dim DEVICE tensor without waiting for the GPU.
        ``noise`` defaults to a draw of the device Philox stream."""
        if not getattr(self.model, "_training", False):
            self.model.train()
        x_start, noise = _loop.loss_inputs(self, x_start, t, noise)
        b, c, h, w = x_start.shape
        t_cpu = t.detach().to("cpu", torch.long).contiguous()
        coef = wo_train_table(self._sched, t_cpu)
        out = torch.empty((b, 2 * c + 2, h, w), device=self.device, dtype=torch.float32) if return_model_out else None
        t_arr = (C.c_int64 * b)(*[int(v) for v in t_cpu.tolist()])
        a = _lib.WoTrainArgs()
        a.x_start, a.noise = _lib.ptr(x_start), _lib.ptr(noise)
        a.t_host = C.cast(t_arr, C.POINTER(C.c_int64))
        a.coef_host, a.coef_stride = _lib.fptr(coef), int(coef.shape[1])
        a.pred_noise_loss_weight = float(self.pred_noise_loss_weight)
        a.pred_x_start_loss_weight = float(self.pred_x_start_loss_weight)
        a.loss_scale, a.accumulate = float(loss_scale), int(bool(accumulate))
        a.model_out, a.B, a.H, a.W = _lib.ptr(out), b, h, w
        val = _loop.loss_call(self, self.model._handle, self._lib.dm_unet_loss_backward_wo, a, sync)
        return (val, out) if return_model_out else val

    def forward(self, img, *args, **kwargs):
        """denoising_diffusion.py:892-899: random timesteps (torch's CPU generator), normalise, p_losses."""
        b, c, h, w = img.shape
        assert (h, w) == tuple(self.image_size), f"height and width of image must be {self.image_size}"
        t = torch.randint(0, self.num_timesteps, (b,)).long()
        return self.p_losses(self.normalize(img.to(self.device, torch.float32)), t, *args, **kwargs)

    __call__ = forward
