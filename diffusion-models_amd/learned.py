"""Learned-variance Gaussian diffusion (Improved DDPM, arXiv 2102.09672) as the reference has it:
``denoising_diffusion/learned_gaussian_diffusion.py``.

``Unet(learned_variance=True)`` predicts ``2 * channels`` maps: the noise and a per-pixel weight that interpolates between
the two extreme posterior log-variances (``posterior_log_variance_clipped[t]`` and ``log(betas)[t]``).  The reverse step
draws with that variance (``dm_sample_lv``: one captured step graph whose single elementwise kernel is ``lv_step_kernel``,
csrc/learned.hip); training adds ``vb_loss_weight`` times the variational-bound term -- the KL between the true and the
predicted posterior, or the discretised decoder NLL on images with ``t == 0`` -- to the plain noise MSE
(``dm_unet_loss_backward_lv``).  The model mean is detached in the vb term, so its gradient reaches only the variance half
of the model output.

Quirks of the reference that are kept: the first half of the model output is read as noise whatever
``objective`` says; ``objective``, ``offset_noise_strength``, ``min_snr_loss_weight`` and ``hybrid_loss`` are accepted and
have NO effect on ``sample`` / ``p_losses`` (the MSE is a plain mean over all elements, without ``loss_weight``).  The
reference's file lacks three imports: ``F`` in ``p_losses`` (training is built here as the file is written, ``F`` being
``torch.nn.functional`` as in the base module), and ``partial`` / ``identity`` in ``model_predictions``, so
``model_predictions`` and with it DDIM sampling (``sampling_timesteps < timesteps``) raise there -- here they raise
``NotImplementedError``.  ``immiscible=True`` raises ``NotImplementedError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import torch

from . import _lib, _loop, bpd as _bpd
from .diffusion import DenoisingDiffusion

COLS = _lib.DM_LV_COEFS
RECIP, RECIPM1, COEF1, COEF2, MIN_LOG, NOISE, MAX_LOG = range(7)  # LvCol of csrc/learned.h
TRAIN_COLS = _lib.DM_LV_TRAIN_COEFS
(T_SQRT_AC, T_SQRT_1M_AC, T_RECIP, T_RECIPM1, T_COEF1, T_COEF2, T_MIN_LOG, T_TRUE_LOG, T_MAX_LOG,
 T_T0) = range(10)  # LvTrainCol of csrc/learned.h

_NO_PATH = ("the reference's {} does not run (learned_gaussian_diffusion.py:75-91 uses `partial` and `identity` without "
            "importing them); only the DDPM loop (sampling_timesteps == timesteps) is built")


def lv_step_table(sched: Dict[str, torch.Tensor], times=None) -> Tuple[List[int], torch.Tensor]:
    """Per-step scalars of ``p_sample_loop`` over ``p_mean_variance`` (:93-111), gathered in fp32 as ``extract`` does.
    Row i (t = T-1-i): [sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2, min_log, t > 0, max_log, 0...] with
    ``min_log = posterior_log_variance_clipped[t]`` and ``max_log = torch.log(betas)[t]`` (:97-98).  ``times``: the rows to
    build, when not the whole loop (a bounded run; one ``p_sample`` step)."""
    if times is None:
        times = reversed(range(int(sched["betas"].shape[0])))
    times = [int(t) for t in times]
    idx = torch.tensor(times, dtype=torch.long)
    c = torch.zeros(len(times), COLS, dtype=torch.float32)
    c[:, RECIP] = sched["sqrt_recip_alphas_cumprod"][idx]
    c[:, RECIPM1] = sched["sqrt_recipm1_alphas_cumprod"][idx]
    c[:, COEF1] = sched["posterior_mean_coef1"][idx]
    c[:, COEF2] = sched["posterior_mean_coef2"][idx]
    c[:, MIN_LOG] = sched["posterior_log_variance_clipped"][idx]
    c[:, NOISE] = (idx > 0).to(torch.float32)
    c[:, MAX_LOG] = torch.log(sched["betas"])[idx]
    return times, c


def lv_train_table(sched: Dict[str, torch.Tensor], t: torch.Tensor) -> torch.Tensor:
    """(B, 12): what ``extract`` gathers at each image's timestep for ``q_sample``, ``predict_start_from_noise``,
    ``q_posterior`` (mean coefficients; the log variance twice: as ``min_log`` and as the true log variance), ``max_log`` and
    the ``t == 0`` flag that selects the decoder NLL (:138)."""
    t = t.detach().to("cpu", torch.long).reshape(-1)
    c = torch.zeros(t.shape[0], TRAIN_COLS, dtype=torch.float32)
    c[:, T_SQRT_AC] = sched["sqrt_alphas_cumprod"][t]
    c[:, T_SQRT_1M_AC] = sched["sqrt_one_minus_alphas_cumprod"][t]
    c[:, T_RECIP] = sched["sqrt_recip_alphas_cumprod"][t]
    c[:, T_RECIPM1] = sched["sqrt_recipm1_alphas_cumprod"][t]
    c[:, T_COEF1] = sched["posterior_mean_coef1"][t]
    c[:, T_COEF2] = sched["posterior_mean_coef2"][t]
    c[:, T_MIN_LOG] = sched["posterior_log_variance_clipped"][t]
    c[:, T_TRUE_LOG] = sched["posterior_log_variance_clipped"][t]
    c[:, T_MAX_LOG] = torch.log(sched["betas"])[t]
    c[:, T_T0] = (t == 0).to(torch.float32)
    return c


class LearnedGaussianDiffusion(DenoisingDiffusion):
    """``LearnedGaussianDiffusion`` (learned_gaussian_diffusion.py:61-146): the reference's signature --
    ``vb_loss_weight`` is the second positional parameter, the rest is ``DenoisingDiffusion``'s."""

    def __init__(self, model, vb_loss_weight=0.001, *args, **kwargs):  # lambda was 0.001 in the paper
        super().__init__(model, *args, **kwargs)
        assert model.out_dim == (model.channels * 2), (
            "dimension out of unet must be twice the number of channels for learned variance - you can also set the "
            "`learned_variance` keyword argument on the Unet to be `True`")
        assert not model.self_condition, "not supported yet"
        if self.immiscible:
            raise NotImplementedError("immiscible=True is not built for LearnedGaussianDiffusion")
        self.vb_loss_weight = vb_loss_weight

    # -- what the reference cannot run ------------------------------------------------------------------------------------
    def model_predictions(self, *args, **kwargs):
        raise NotImplementedError(_NO_PATH.format("model_predictions"))

    def ddim_sample(self, *args, **kwargs):
        raise NotImplementedError(_NO_PATH.format("ddim_sample (it calls model_predictions)"))

    def ddim_sample_guided(self, *args, **kwargs):
        raise NotImplementedError(_NO_PATH.format("ddim_sample_guided (it calls model_predictions)"))

    def dpm_solver_sample(self, *args, **kwargs):
        raise NotImplementedError("LearnedGaussianDiffusion has no dpm_solver_sample: the model output is (prediction, "
                                  "variance interpolation), not the plain prediction DPM-Solver++ steps on, and the class has "
                                  "no model_predictions")

    _dyn_refusal = NotImplementedError  # dynamic_threshold: this class's loop has its own update kernel

    # -- sampling ---------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def p_sample_loop(self, shape, return_all_timesteps=False, *, noise=None, seed=None, max_steps=None, sample_offset=0,
                      dynamic_threshold=None):
        """denoising_diffusion.py:647-664 over the p_mean_variance of :93-111.  ``noise`` (a callable ``shape -> cpu
        tensor``) is called in the reference's draw order: x_T, then one per step with t > 0."""
        self._dyn(dynamic_threshold)
        shape = _loop.checked_shape(self, shape)
        times = list(reversed(range(self.num_timesteps)))
        if max_steps is not None:  # bounded run: the first `max_steps` iterations only
            times = times[:max(int(max_steps), 0)]
        times, coefs = lv_step_table(self._sched, times)
        start = _loop.loop_start(self, shape, noise, seed, sample_offset, [t > 0 for t in times])
        a = _lib.LvArgs()
        a.n_steps = len(times)
        return _loop.loop_call(self, a, self._lib.dm_sample_lv, shape, start, sample_offset, times, coefs, "table_host",
                               len(times) + 1, return_all_timesteps)

    @torch.inference_mode()
    def sample(self, batch_size=16, return_all_timesteps=False, **kw):
        """denoising_diffusion.py:779-783.  With ``sampling_timesteps < timesteps`` the reference takes its DDIM path, which
        does not run."""
        if self.is_ddim_sampling:
            raise NotImplementedError(_NO_PATH.format("DDIM path (sampling_timesteps < timesteps)"))
        (h, w), channels = self.image_size, self.channels
        return self.p_sample_loop((batch_size, channels, h, w), return_all_timesteps=return_all_timesteps, **kw)

    def _step(self, x, t, model_output, z, seed=0):
        """``dm_op_lv_step`` at per-call time ``t`` (an int): (pred_img, model_mean, model_log_variance, x_start)."""
        t = int(t)
        x = x.to(self.device, torch.float32).contiguous()
        b = x.shape[0]
        if model_output is None:
            model_output = self.model(x, torch.full((b,), t, device=self.device, dtype=torch.long))
        model_output = model_output.to(self.device, torch.float32).contiguous()
        assert tuple(model_output.shape) == (b, 2 * x.shape[1]) + tuple(x.shape[2:]), "model_output is (B, 2C, H, W)"
        row = lv_step_table(self._sched, [t])[1][0].contiguous()
        outs = [torch.empty_like(x) for _ in range(4)]
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_op_lv_step(_lib.ptr(x), _lib.ptr(model_output), _lib.ptr(z), _lib.fptr(row), C.c_uint64(seed),
                                           C.c_uint64(1), C.c_uint64(0), *[_lib.ptr(o) for o in outs], b, x[0].numel(),
                                           stream))
        return outs

    @torch.inference_mode()
    def p_mean_variance(self, *, x, t, clip_denoised, model_output=None, **kwargs):
        """:93-111: (model_mean, model_variance, model_log_variance, x_start).  ``t`` is the reference's (B,) tensor (or an
        int); the images are grouped by their timestep, one kernel launch per distinct value."""
        x = x.to(self.device, torch.float32).contiguous()
        b = x.shape[0]
        bt = self._bt(t, b)
        if model_output is None:
            model_output = self.model(x, bt.to(self.device))
        model_output = model_output.to(self.device, torch.float32)
        mean, logvar, x_start = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        for tv in sorted(set(bt.tolist())):
            sel = (bt == tv).nonzero().reshape(-1).to(self.device)
            _, m, lv, xs = self._step(x[sel], tv, model_output[sel].contiguous(), None)
            if not clip_denoised:  # the kernel clamps (p_sample always does): the unclamped x_start and its mean
                xs = self.predict_start_from_noise(x[sel], tv, model_output[sel, :x.shape[1]])
                m = self.q_posterior(xs, x[sel], tv)[0]
            mean[sel], logvar[sel], x_start[sel] = m, lv, xs
        return mean, logvar.exp(), logvar, x_start

    @torch.inference_mode()
    def p_sample(self, x, t: int, x_self_cond=None, *, noise=None):
        """denoising_diffusion.py:638-645 over :93-111.  Returns (pred_img, x_start); ``noise`` draws once when t > 0."""
        assert x_self_cond is None, "the model was built without self_condition"
        t = int(t)
        z, seed = None, 0
        if t > 0:
            if noise is not None:
                z = noise(tuple(x.shape)).to(self.device, torch.float32).contiguous()
            else:
                seed = _lib.default_seed()
        out, _, _, x_start = self._step(x, t, None, z, seed)
        return out, x_start

    @torch.inference_mode()
    def calc_bpd_loop(self, img, clip_denoised=True, *, times=None, noise=None, seed=None, sample_offset=0):
        """The variational bound of the images, term by term, in bits per dimension (bpd.py) with this class's
        ``p_mean_variance`` (:93-111): the variance the model predicts, and the first half of its output read as noise.
        The ``vb`` column of a timestep is the quantity ``p_losses`` weighs with ``vb_loss_weight``, at every t."""
        return _bpd.calc_bpd_loop(self, img, clip_denoised, times=times, noise=noise, seed=seed, sample_offset=sample_offset,
                                  learned=True)

    # -- training ---------------------------------------------------------------------------------------------------------
    def p_losses(self, x_start, t, noise=None, clip_denoised=False, *, loss_scale=1.0, accumulate=False, sync=True,
                 return_model_out=False):
        """:113-146: ``mse_loss(pred_noise, noise) + vb_losses.mean() * vb_loss_weight`` and every parameter gradient, in
        one call of the library (the gradients stay on the model: ``self.model.grad(name)``).  ``loss_scale`` /
        ``accumulate`` are the micro-batch loop of ``Trainer.train``; ``sync=False`` returns the loss as a 0-dim DEVICE
        tensor without waiting for the GPU.  ``noise`` defaults to a draw of the device Philox stream."""
        if not getattr(self.model, "_training", False):
            self.model.train()
        x_start, noise = _loop.loss_inputs(self, x_start, t, noise)
        b, c, h, w = x_start.shape
        t_cpu = t.detach().to("cpu", torch.long).contiguous()
        coef = lv_train_table(self._sched, t_cpu)
        out = torch.empty((b, 2 * c, h, w), device=self.device, dtype=torch.float32) if return_model_out else None
        t_arr = (C.c_int64 * b)(*[int(v) for v in t_cpu.tolist()])
        a = _lib.LvTrainArgs()
        a.x_start, a.noise = _lib.ptr(x_start), _lib.ptr(noise)
        a.t_host = C.cast(t_arr, C.POINTER(C.c_int64))
        a.coef_host, a.coef_stride = _lib.fptr(coef), int(coef.shape[1])
        a.vb_loss_weight, a.clip_denoised = float(self.vb_loss_weight), int(bool(clip_denoised))
        a.loss_scale, a.accumulate = float(loss_scale), int(bool(accumulate))
        a.model_out, a.B, a.H, a.W = _lib.ptr(out), b, h, w
        val = _loop.loss_call(self, self.model._handle, self._lib.dm_unet_loss_backward_lv, a, sync)
        return (val, out) if return_model_out else val

    def forward(self, img, *args, **kwargs):
        """denoising_diffusion.py:892-899: random timesteps (torch's CPU generator), normalise, p_losses."""
        b, c, h, w = img.shape
        assert (h, w) == tuple(self.image_size), f"height and width of image must be {self.image_size}"
        t = torch.randint(0, self.num_timesteps, (b,)).long()
        return self.p_losses(self.normalize(img.to(self.device, torch.float32)), t, *args, **kwargs)

    __call__ = forward
