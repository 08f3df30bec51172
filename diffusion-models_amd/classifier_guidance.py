"""Classifier-guided DDPM sampling (Sohl-Dickstein et al. 2015; Dhariwal & Nichol, arXiv 2105.05233) as the reference has
it: ``denoising_diffusion/guided_diffusion.py``.

``ClassifierGuidedGaussianDiffusion`` is ``DenoisingDiffusion`` with that file's defaults (``beta_schedule='sigmoid'``, the
loss weight always derived from the SNR) and a DDPM loop that takes ``cond_fn`` and ``guidance_kwargs``.  After the U-Net
has produced the posterior mean of a step, ``cond_fn(mean, t, **guidance_kwargs)`` returns the gradient of
``log p(y | x)`` AT THAT MEAN (the file's stated fix of the OpenAI code, :561-563); the mean is shifted by
``posterior_variance[t] * gradient`` and the noise is added after that (:553-584).

``cond_fn`` is Python, so this is the one loop whose step leaves the GPU in the middle.  ``dm_sample_classifier_guided``
runs a step as two captured halves -- the U-Net forward with ``cg_mean_kernel``, and ``cg_finish_kernel`` with the step
counter (csrc/cguide.hip) -- and calls back into this module between them.  ``mean`` and ``grad`` are two tensors
allocated once, outside any inference mode, and reused by every step; the object keeps the pair for the next call of
the same shape, because their addresses are arguments of the captured kernels.

Kept from the reference: guidance is applied only when BOTH ``cond_fn`` and ``guidance_kwargs`` are given
(:579), otherwise every method is the parent's and ``cond_fn`` is never called; the gradient is multiplied by the UNCLIPPED
``posterior_variance[t]``, which is 0 at ``t == 0``, so the last step calls ``cond_fn`` and its result has no effect; the
returned ``x_start`` and the self-conditioning input of the next step are the unguided clamped estimate; ``ddim_sample``
accepts ``cond_fn`` / ``guidance_kwargs`` and ignores them (:606-644 never uses them).  Not mirrored: the per-step
``print("gradient: ", ...)`` of :568.

The guided loop runs under ``torch.no_grad()``, not ``torch.inference_mode()``: a ``cond_fn`` does
``x.detach().requires_grad_(True)`` under ``torch.enable_grad()``, which an inference tensor refuses.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import torch

from . import _lib, _loop
from .diffusion import DenoisingDiffusion
from .spec import ddpm_step_table

COLS = _lib.DM_CG_COEFS
SIGMA, NOISE, VARIANCE = 4, 5, 8  # CgCol of csrc/cguide.h


def cg_step_table(sched: Dict[str, torch.Tensor], times=None) -> Tuple[List[int], torch.Tensor]:
    """Per-step scalars of the guided ``p_sample`` (:573-584).  Row i (t = T-1-i): columns 0..7 the DDPM row of
    ``ddpm_step_table`` as it is, column 8 ``posterior_variance[t]`` (the registered fp32 buffer, unclipped: 0 at t == 0),
    the rest 0.  ``times``: the rows to build, when not the whole loop (one ``p_sample`` step)."""
    all_times, ddpm = ddpm_step_table(sched)  # row i is t = T - 1 - i
    T = len(all_times)
    times = all_times if times is None else [int(t) for t in times]
    idx = torch.tensor(times, dtype=torch.long)
    c = torch.zeros(len(times), COLS, dtype=torch.float32)
    c[:, :8] = ddpm[T - 1 - idx]
    c[:, VARIANCE] = sched["posterior_variance"][idx]
    return times, c


class ClassifierGuidedGaussianDiffusion(DenoisingDiffusion):
    """``guided_diffusion.GaussianDiffusion`` (guided_diffusion.py:380-727): the reference's constructor signature and
    defaults, plus ``use_graph``.  Training (``p_losses``, ``forward``) is the base class's.  So is ``dpm_solver_sample``:
    it takes no ``cond_fn`` and samples unguided, as this class's ``ddim_sample`` does."""

    def __init__(
        self,
        model,
        *,
        image_size,
        timesteps=1000,
        sampling_timesteps=None,
        objective="pred_noise",
        beta_schedule="sigmoid",
        schedule_fn_kwargs=dict(),
        ddim_sampling_eta=0.0,
        auto_normalize=True,
        min_snr_loss_weight=False,
        min_snr_gamma=5,
        use_graph=True,
    ):
        assert not (type(self) == ClassifierGuidedGaussianDiffusion and model.channels != model.out_dim)
        super().__init__(model, image_size=image_size, timesteps=timesteps, sampling_timesteps=sampling_timesteps,
                         objective=objective, beta_schedule=beta_schedule, schedule_fn_kwargs=schedule_fn_kwargs,
                         ddim_sampling_eta=ddim_sampling_eta, auto_normalize=auto_normalize, use_graph=use_graph,
                         min_snr_loss_weight=min_snr_loss_weight, min_snr_gamma=min_snr_gamma,
                         ddpm=False)  # the loss weight always comes from the SNR (:468-481)

    # -- the callback's Python side -----------------------------------------------------------------------------------------
    @staticmethod
    def _gradient(cond_fn, mean, t, guidance_kwargs, grad):
        """``cond_fn(mean, t, **guidance_kwargs)`` (:564) checked and copied as fp32 into ``grad``."""
        g = cond_fn(mean, t, **guidance_kwargs)
        if not isinstance(g, torch.Tensor) or tuple(g.shape) != tuple(mean.shape):
            got = tuple(g.shape) if isinstance(g, torch.Tensor) else type(g).__name__
            raise ValueError(f"cond_fn must return a tensor of the mean's shape {tuple(mean.shape)}, got {got}")
        grad.copy_(g.detach().float())
        return grad

    _dyn_refusal = NotImplementedError  # dynamic_threshold: this class's loop has its own update kernel
    _bpd_refusal = ("the guided reverse step shifts the mean by a classifier's gradient, which is no "
                    "normalised posterior to bound with")

    # -- the loop -----------------------------------------------------------------------------------------------------------
    def p_sample_loop(self, shape, return_all_timesteps=False, cond_fn=None, guidance_kwargs=None, *, noise=None, seed=None,
                      sample_offset=0, **kw):
        """:586-603.  Without ``cond_fn`` or without ``guidance_kwargs`` this is the parent's loop.  ``noise`` (a callable
        ``shape -> cpu tensor``) is called in the reference's draw order: x_T, then one per step with t > 0.  ``cond_fn``
        receives the (B, C, H, W) fp32 device mean and ``t`` as a (B,) int64 device tensor; both are reused by every step,
        so a ``cond_fn`` that keeps them clones them."""
        self._dyn(kw.get("dynamic_threshold"))
        if cond_fn is None or guidance_kwargs is None:
            return super().p_sample_loop(shape, return_all_timesteps, noise=noise, seed=seed, sample_offset=sample_offset, **kw)
        if kw:
            raise TypeError(f"unexpected keyword arguments with classifier guidance: {sorted(kw)}")
        with torch.no_grad():
            return self._guided_loop(shape, return_all_timesteps, cond_fn, guidance_kwargs, noise, seed, sample_offset)

    def _guided_loop(self, shape, return_all_timesteps, cond_fn, guidance_kwargs, noise, seed, sample_offset):
        shape = _loop.checked_shape(self, shape)
        times, coefs = cg_step_table(self._sched)
        start = _loop.loop_start(self, shape, noise, seed, sample_offset, [t > 0 for t in times])
        # what cond_fn sees and what it returns into: allocated once, outside any inference mode, reused by every step
        mean, grad = self._guide_buffers(shape)
        t_dev = torch.zeros((shape[0],), device=self.device, dtype=torch.long)
        stream = torch.cuda.current_stream(self.device)
        raised: List[BaseException] = []

        def callback(_user, _step, t):
            try:
                t_dev.fill_(int(t))
                self._gradient(cond_fn, mean, t_dev, guidance_kwargs, grad)
                stream.synchronize()  # grad is complete before the second half of the step reads it
                return 0
            except BaseException as e:  # nothing may propagate through the C frames: re-raised after the call returns
                raised.append(e)
                return 1

        def entry(handle, args):  # what the callback caught goes first: the library's own error only says that it returned 1
            rc = self._lib.dm_sample_classifier_guided(handle, args)
            if raised:
                raise raised[0]
            return rc

        cb = _lib.CondCallback(callback)
        a = _lib.CguideArgs()
        a.objective, a.self_condition, a.n_steps = self._objective_id, int(bool(self.self_condition)), len(times)
        a.mean, a.grad, a.cond_cb, a.user = _lib.ptr(mean), _lib.ptr(grad), cb, None
        return _loop.loop_call(self, a, entry, shape, start, sample_offset, times, coefs, "table_host", len(times) + 1,
                               return_all_timesteps)

    def _guide_buffers(self, shape):
        """(mean, grad) of ``shape``, kept between calls: their addresses are kernel arguments of the captured halves, so a
        second call of the same shape replays the graphs of the first."""
        held = getattr(self, "_cg_buffers", None)
        if held is None or tuple(held[0].shape) != tuple(shape):
            held = (torch.zeros(shape, device=self.device, dtype=torch.float32),
                    torch.zeros(shape, device=self.device, dtype=torch.float32))
            self._cg_buffers = held
        return held

    def sample(self, batch_size=16, return_all_timesteps=False, cond_fn=None, guidance_kwargs=None, *, noise=None, seed=None,
               sample_offset=0, **kw):
        """:646-650."""
        (h, w), channels = self.image_size, self.channels
        shape = (batch_size, channels, h, w)
        if not self.is_ddim_sampling:
            return self.p_sample_loop(shape, return_all_timesteps, cond_fn, guidance_kwargs, noise=noise, seed=seed,
                                      sample_offset=sample_offset, **kw)
        return self.ddim_sample(shape, return_all_timesteps=return_all_timesteps, cond_fn=cond_fn,
                                guidance_kwargs=guidance_kwargs, noise=noise, seed=seed, sample_offset=sample_offset, **kw)

    def ddim_sample(self, shape, sampling_timesteps=None, return_all_timesteps=False, cond_fn=None, guidance_kwargs=None, **kw):
        """:606-644.  ``cond_fn`` and ``guidance_kwargs`` are accepted and IGNORED: the reference's DDIM loop takes both and
        never uses them, so DDIM sampling is unguided and ``cond_fn`` is never called.  This is the parent's ``ddim_sample``."""
        return super().ddim_sample(shape, sampling_timesteps, return_all_timesteps, **kw)

    # -- one step -----------------------------------------------------------------------------------------------------------
    def _row(self, t: int) -> torch.Tensor:
        return cg_step_table(self._sched, [int(t)])[1][0].contiguous()

    def _finish(self, mean, grad, row, z, seed=0):
        """``dm_op_cg_finish``: (mean + row[8] grad) + row[4] z and the guided mean."""
        out, guided = torch.empty_like(mean), torch.empty_like(mean)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_op_cg_finish(_lib.ptr(mean), _lib.ptr(grad), _lib.ptr(z), _lib.fptr(row), C.c_uint64(seed),
                                             C.c_uint64(1), C.c_uint64(0), _lib.ptr(out), _lib.ptr(guided), mean.shape[0],
                                             mean[0].numel(), stream))
        return out, guided

    def condition_mean(self, cond_fn, mean, variance, x, t, guidance_kwargs=None):
        """:553-569: ``mean.float() + variance * cond_fn(mean, t, **guidance_kwargs).float()``.  ``variance`` is what
        ``extract(posterior_variance, t, x.shape)`` gives: a (B, 1, 1, 1) tensor (or a (B,) tensor, or one number).  ``x`` is
        unused, as in the reference."""
        with torch.no_grad():
            mean = mean.detach().to(self.device, torch.float32).contiguous()
            b = mean.shape[0]
            bt = self._bt(t, b).to(self.device)
            grad = self._gradient(cond_fn, mean, bt, guidance_kwargs, torch.empty_like(mean))
            var = torch.as_tensor(variance, dtype=torch.float32).detach().to("cpu").reshape(-1)
            assert var.numel() in (1, b), "variance holds one value, or one per image"
            var = var.expand(b)
            row = torch.zeros(COLS, dtype=torch.float32)
            out = torch.empty_like(mean)
            for v in sorted(set(var.tolist())):  # one launch per distinct value (a p_sample batch has one)
                sel = (var == v).nonzero().reshape(-1).to(self.device)
                row[VARIANCE] = v
                out[sel] = self._finish(mean[sel].contiguous(), grad[sel].contiguous(), row, None)[1]
            return out

    def _guided_step(self, x, t, x_self_cond, cond_fn, guidance_kwargs, noise):
        """One guided reverse step as its four tensors: (pred_img, x_start, model_mean, guided_mean)."""
        t = int(t)
        x = x.detach().to(self.device, torch.float32).contiguous()
        b = x.shape[0]
        bt = torch.full((b,), t, device=self.device, dtype=torch.long)
        if self.self_condition:
            cond_kw = dict(x_self_cond=x_self_cond)
        else:
            assert x_self_cond is None, "the model was built without self_condition"
            cond_kw = {}
        model_out = self._eps(x, bt, **cond_kw).contiguous()
        row = self._row(t)
        mean, x_start = torch.empty_like(x), torch.empty_like(x)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_op_cg_mean(_lib.ptr(x), _lib.ptr(model_out), _lib.fptr(row), self._objective_id, _lib.ptr(mean),
                                           _lib.ptr(x_start), b, x[0].numel(), stream))
        grad = self._gradient(cond_fn, mean, bt, guidance_kwargs, torch.empty_like(x))
        z, seed = None, 0
        if t > 0:
            if noise is not None:
                z = noise(tuple(x.shape)).to(self.device, torch.float32).contiguous()
            else:
                seed = _lib.default_seed()
        out, guided = self._finish(mean, grad, row, z, seed)
        return out, x_start, mean, guided

    def p_sample(self, x, t: int, x_self_cond=None, cond_fn=None, guidance_kwargs=None, *, noise=None):
        """:573-584.  Returns (pred_img, x_start); ``x_start`` is the unguided clamped estimate.  ``noise`` draws once when
        t > 0."""
        if cond_fn is None or guidance_kwargs is None:
            return super().p_sample(x, t, x_self_cond, noise=noise)
        with torch.no_grad():
            return self._guided_step(x, t, x_self_cond, cond_fn, guidance_kwargs, noise)[:2]
