"""Host-side mirror of the reference's sequence model: ``Unet1D`` and ``DenoisingDiffusion1D`` over tensors (B, C, L)
(denoising-diffusion-pytorch/denoising_diffusion/denoising_diffusion_1d.py:219-349, :376-677).

Sampling and inference only.  The library sees a sequence as a one-row image: activations are (B, L, C) = NHWC with
H = 1, the convolutions run as 1 x K, and the handle is a ``dm_unet`` created with ``seq1d = 1``.  Both classes reuse what
the image classes have -- the handle surface of ``Unet``, the schedule, loops and elementwise helpers of
``DenoisingDiffusion`` -- and restate only what the reference's 1D file does differently:

* ``DenoisingDiffusion1D.ddim_sample(shape, clip_denoised=True)`` calls ``model_predictions(img, t, self_cond,
  clip_x_start=clip_denoised)`` WITHOUT ``rederive_pred_noise`` (:577).  Under ``objective='pred_noise'`` the update takes the
  raw network output as ``pred_noise`` next to the clamped ``x_start``; with ``clip_denoised=False`` nothing is clamped; the
  other objectives derive the noise from the (possibly clamped) ``x_start``.  The image class re-derives and always clamps.
* ``loss_weight`` has no min-SNR clamp (:454-463); ``beta_schedule`` is ``linear`` or ``cosine``, default ``cosine``.
* every stage's attention is ``LinearAttention(dim)`` with its default four 32-wide heads, ``mid_attn`` alone takes
  ``attn_heads`` / ``attn_dim_head`` (:285, :291, :300); no layer has memory key / values.

Restrictions (each raises): training (``train(True)``, ``p_losses``, ``forward``) and DPM-Solver++ are not pinned for this
class yet; a ``Unet1D`` with ``learned_sinusoidal_cond`` / ``random_fourier_features`` serves ``Unet1D.forward`` alone, as
the 2D model does (the reference does not assert this away; we restrict it); ``out_dim != channels`` is refused by
``DenoisingDiffusion1D``.
"""
from __future__ import annotations

import torch

from . import _lib
from .diffusion import DDIM, DenoisingDiffusion
from .spec import Unet1DConfig, ddim_step_table, unet1d_param_spec
from .unet import Unet

TRAINING_FOLLOW_UP = ("training the sequence model (p_losses, the backward pass, Trainer1D) is the follow-up to the sampling "
                      "path: this class samples and runs inference only")


class Unet1D(Unet):
    """``Unet1D(dim, dim_mults=..., channels=...)`` -- drop-in for the reference class at inference: ``forward(x, time,
    x_self_cond=None)`` on (B, C, L), ``load_state_dict`` / ``state_dict`` with the reference's key names."""

    seq1d = True

    def __init__(self, dim, init_dim=None, out_dim=None, dim_mults=(1, 2, 4, 8), channels=3, dropout=0.0,
                 self_condition=False, learned_variance=False, learned_sinusoidal_cond=False, random_fourier_features=False,
                 learned_sinusoidal_dim=16, sinusoidal_pos_emb_theta=10000, attn_dim_head=32, attn_heads=4, device="cuda:0"):
        if isinstance(attn_dim_head, (tuple, list)) or isinstance(attn_heads, (tuple, list)):
            raise ValueError("Unet1D takes one attn_dim_head and one attn_heads: they shape mid_attn alone")
        self.cfg = Unet1DConfig(
            dim=dim, init_dim=init_dim, out_dim=out_dim, dim_mults=tuple(dim_mults), channels=channels, dropout=float(dropout),
            self_condition=bool(self_condition), learned_variance=bool(learned_variance),
            learned_sinusoidal_cond=bool(learned_sinusoidal_cond), random_fourier_features=bool(random_fourier_features),
            learned_sinusoidal_dim=int(learned_sinusoidal_dim), sinusoidal_pos_emb_theta=float(sinusoidal_pos_emb_theta),
            attn_dim_head=int(attn_dim_head), attn_heads=int(attn_heads))
        c = self._attach(self.cfg, dropout, device)
        c.attn_heads, c.attn_dim_head = self.cfg.attn_heads, self.cfg.attn_dim_head
        c.text_mode, c.text_emb_dim, c.seq1d = 0, 0, 1
        self._create(c)

    def param_spec(self):
        return unet1d_param_spec(self.cfg)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(TRAINING_FOLLOW_UP)
        return self

    def forward(self, x, time, x_self_cond=None):
        """denoising_diffusion_1d.py:310-349 on (B, C, L).  ``L`` must be divisible by ``2 ** (len(dim_mults) - 1)``: the
        reference itself fails on the skip concatenation for other lengths."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() must be called before forward()")
        if x.dim() != 3:
            raise RuntimeError(f"Unet1D takes (B, C, L), got {tuple(x.shape)}")
        f = self.downsample_factor
        if x.shape[-1] % f != 0:
            raise RuntimeError(f"your sequence length {x.shape[-1]} needs to be divisible by {f}, given the unet")
        x = x.to(device=self.device, dtype=torch.float32)
        if self.self_condition:
            if x_self_cond is None:
                x_self_cond = torch.zeros_like(x)
            x = torch.cat((x_self_cond.to(x), x), dim=1)
        else:
            assert x_self_cond is None, "the model was built without self_condition"
        x = x.contiguous()
        B, Cin, L = x.shape
        if Cin != self.cfg.input_channels:
            raise RuntimeError(f"expected {self.cfg.input_channels} input channels, got {Cin}")
        float_time = self.random_or_learned_sinusoidal_cond and torch.is_tensor(time) and time.is_floating_point()
        t = time.to(device=self.device, dtype=torch.float32 if float_time else torch.int64).reshape(-1)
        if t.numel() == 1 and B > 1:
            t = t.expand(B)
        if t.numel() != B:
            raise RuntimeError(f"time has {t.numel()} entries for a batch of {B}")
        t = t.contiguous()
        out = torch.empty((B, self.out_dim, L), device=self.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        fwd = self._lib.dm_unet_forward_ft if float_time else self._lib.dm_unet_forward
        _lib.check(fwd(self._handle, _lib.ptr(x), _lib.ptr(t), None, 0, _lib.ptr(out), B, 1, L, stream))
        return out

    __call__ = forward

    def forward_with_cond_scale(self, *a, **k):
        raise NotImplementedError("Unet1D has no text condition")


def _refused(name):
    def method(self, *a, **k):
        raise NotImplementedError(f"Unet1D.{name}: {TRAINING_FOLLOW_UP}")
    method.__name__ = name
    return method


# the training surface Unet1D inherits from Unet: refused as train() is, not left to fail inside the library
for _name in ("set_dropout_seed", "grad", "grads", "grads_flat", "grad_buckets", "bucket_wait", "optimizer_step", "ema_update",
              "optimizer_state_dict", "load_optimizer_state_dict", "load_ema_state_dict", "sync", "check_device_pack"):
    assert hasattr(Unet, _name), _name
    setattr(Unet1D, _name, _refused(_name))


class DenoisingDiffusion1D(DenoisingDiffusion):
    """``DenoisingDiffusion1D(model, *, seq_length, ...)`` (denoising_diffusion_1d.py:376-468): sampling over (B, C, L).  The
    loops are the image class's, called on the (B, C, 1, L) view; ``noise=``, ``seed=``, ``sample_offset=`` and
    ``return_all_timesteps=`` are the keyword extensions of this code base."""

    def __init__(self, model, *, seq_length, timesteps=1000, sampling_timesteps=None, objective="pred_noise",
                 beta_schedule="cosine", ddim_sampling_eta=0.0, auto_normalize=True, use_graph=True):
        if not getattr(model, "seq1d", False):
            raise TypeError("DenoisingDiffusion1D needs a Unet1D")
        if getattr(model, "random_or_learned_sinusoidal_cond", False):
            raise NotImplementedError("a Unet1D with learned_sinusoidal_cond / random_fourier_features serves Unet1D.forward "
                                      "alone: the sampling loops take the integer-time embedding, as the image classes do")
        if model.channels != model.out_dim:
            raise NotImplementedError("DenoisingDiffusion1D needs out_dim == channels (no learned variance)")
        if beta_schedule not in ("linear", "cosine"):
            raise ValueError(f"unknown beta schedule {beta_schedule}")
        if objective not in ("pred_noise", "pred_x0", "pred_v"):
            raise ValueError("objective must be pred_noise, pred_x0 or pred_v")
        # loss_weight from the float64 SNR without a min-SNR clamp (:454-463): make_schedule(ddpm=False)
        super().__init__(model, image_size=(1, int(seq_length)), timesteps=timesteps, sampling_timesteps=sampling_timesteps,
                         objective=objective, beta_schedule=beta_schedule, ddim_sampling_eta=ddim_sampling_eta,
                         auto_normalize=auto_normalize, use_graph=use_graph, ddpm=False, min_snr_loss_weight=False)
        self.seq_length = int(seq_length)

    def sample_shape(self):
        return (self.channels, self.seq_length)

    _dyn_refusal = NotImplementedError  # dynamic_threshold: this class's loop has its own update kernel
    _bpd_refusal = ("the decoder term's 1/255 bins are those of 8-bit images, and the sequence model runs only "
                    "its pinned DDPM / DDIM loops")

    # -- the loops: (B, C, L) at the surface, (B, C, 1, L) at the ABI -------------------------------------------------
    def _run(self, kind, shape, times, coefs, takes_noise, return_all_timesteps, noise, seed, text_emb=None, max_steps=None,
             cond=None, sample_offset=0, x_init=None, unnormalize=None, guidance=None, ddim_flags=0, dynamic_threshold=None):
        self._dyn(dynamic_threshold)
        assert text_emb is None and cond is None and guidance is None, "the sequence model is unconditional"
        shape = tuple(int(v) for v in shape)
        assert len(shape) == 3, f"shape {shape}: (batch, channels, seq_length)"
        B, Cc, L = shape
        f = self.model.downsample_factor
        assert L % f == 0, f"shape {shape}: the sequence length must be divisible by {f}"
        noise4 = (lambda s4: noise(shape).reshape(s4)) if noise is not None else None
        x4 = x_init.reshape(B, Cc, 1, L) if x_init is not None else None
        out = super()._run(kind, (B, Cc, 1, L), times, coefs, takes_noise, return_all_timesteps, noise4, seed,
                           max_steps=max_steps, sample_offset=sample_offset, x_init=x4, unnormalize=unnormalize,
                           ddim_flags=ddim_flags)
        return out.squeeze(-2)

    @torch.inference_mode()
    def p_sample_loop(self, shape, return_all_timesteps=False, *, noise=None, seed=None, max_steps=None, sample_offset=0,
                      dynamic_threshold=None):
        """:547-560."""
        return super().p_sample_loop(shape, return_all_timesteps, noise=noise, seed=seed, max_steps=max_steps,
                                     sample_offset=sample_offset, dynamic_threshold=dynamic_threshold)

    @torch.inference_mode()
    def ddim_sample(self, shape, clip_denoised=True, return_all_timesteps=False, *, noise=None, seed=None, max_steps=None,
                    sample_offset=0, dynamic_threshold=None):
        """:562-596: ``model_predictions(img, t, self_cond, clip_x_start=clip_denoised)`` without ``rederive_pred_noise``."""
        self._dyn(dynamic_threshold)
        times, coefs = ddim_step_table(self._sched, self.sampling_timesteps, self.ddim_sampling_eta)
        takes = [bool(c[5] != 0) for c in coefs]
        flags = _lib.DDIM_RAW_NOISE | (0 if clip_denoised else _lib.DDIM_NO_CLAMP)
        return self._run(DDIM, shape, times, coefs, takes, return_all_timesteps, noise, seed, max_steps=max_steps,
                         sample_offset=sample_offset, ddim_flags=flags)

    @torch.inference_mode()
    def sample(self, batch_size=16, return_all_timesteps=False, *, solver=None, **kw):
        """:598-602."""
        if solver is not None:
            raise NotImplementedError("DPM-Solver++ is not pinned for DenoisingDiffusion1D yet (solver=None only)")
        sample_fn = self.p_sample_loop if not self.is_ddim_sampling else self.ddim_sample
        return sample_fn((batch_size, self.channels, self.seq_length), return_all_timesteps=return_all_timesteps, **kw)

    def dpm_solver_sample(self, *a, **k):
        raise NotImplementedError("DPM-Solver++ is not pinned for DenoisingDiffusion1D yet")

    def ddim_sample_guided(self, *a, **k):
        raise NotImplementedError("the reference's sequence class has no guided DDIM loop")

    @torch.inference_mode()
    def p_mean_variance(self, x, t, x_self_cond=None, clip_denoised=True):
        """:528-536: ``model_predictions`` WITHOUT clipping, then ``x_start.clamp_(-1, 1)`` -- the same values as clipping
        inside (the posterior reads x_start alone)."""
        return super().p_mean_variance(x, t, x_self_cond, clip_denoised)

    @torch.inference_mode()
    def p_sample(self, x, t: int, x_self_cond=None, clip_denoised=True, *, noise=None):
        """:538-545.  Returns (pred_img, x_start).  The update kernel is the image class's, which clamps x_start: the
        reference's own loops never pass ``clip_denoised=False``, and neither does this path."""
        if not clip_denoised:
            raise NotImplementedError("p_sample(clip_denoised=False): the DDPM update kernel clamps x_start")
        return self._p_sample(x, t, noise, {}, x_self_cond)

    # -- training: the follow-up --------------------------------------------------------------------------------------
    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(TRAINING_FOLLOW_UP)
        return self

    def p_losses(self, *a, **k):
        raise NotImplementedError(TRAINING_FOLLOW_UP)

    def forward(self, *a, **k):
        raise NotImplementedError(TRAINING_FOLLOW_UP)

    __call__ = forward
