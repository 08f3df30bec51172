"""What the diffusion classes with a real-valued U-Net time share: ``ElucidatedDiffusion`` (time = c_noise(sigma)) and the
two continuous-time classes (time = log-SNR).  The base holds the module-like surface over the U-Net, the constructor's
U-Net checks, ``train()``, the start image and injected noise rows of a sampling loop, and the tail of a loss call.  A
subclass names its U-Net field (also its ``state_dict`` prefix) and its training entry of libdm_hip.so.
"""
from __future__ import annotations

import torch

from . import _lib, _loop


class FloatTimeDiffusion:
    _unet_attr = "model"  # the U-Net's field, and the prefix of its keys in state_dict(): "net" / "model" as in the reference
    _train_entry = ""     # dm_unet_loss_backward_edm / dm_unet_loss_backward_ct

    def _init_unet(self, unet, image_size, channels, use_graph, calls):
        """The U-Net checks of both constructors.  ``calls``: the class's sentence on how it calls the U-Net."""
        assert unet.random_or_learned_sinusoidal_cond
        self._refuse_self_condition(unet)
        if getattr(unet, "text_condition", False) or getattr(getattr(unet, "cfg", None), "cond_channels", 0):
            raise NotImplementedError(f"{calls}: a text-conditional or image-conditional U-Net has no place for its condition")
        if unet.out_dim != channels or unet.channels != channels:
            raise ValueError(f"the U-Net maps {unet.channels} to {unet.out_dim} channels, the sampler needs {channels} -> "
                             f"{channels} (no learned variance)")
        setattr(self, self._unet_attr, unet)
        self.channels = channels
        self.image_size = image_size
        self.use_graph = use_graph
        self._lib = _lib.load()

    @property
    def _unet(self):
        return getattr(self, self._unet_attr)

    # -- module-ish surface ------------------------------------------------------------------------
    @property
    def device(self):
        return self._unet.device

    def eval(self):
        return self

    def parameters(self):
        return self._unet.parameters()

    def sample_shape(self):
        """(C, H, W) of one sample (``dist.sample_global`` builds empty shards from it)."""
        return (self.channels, self.image_size, self.image_size)

    def state_dict(self):
        """The reference modules have no buffers: the prefix + the U-Net's keys."""
        return {f"{self._unet_attr}.{k}": v for k, v in self._unet.state_dict().items()}

    def load_state_dict(self, state_dict, strict=True):
        pre = self._unet_attr + "."
        other = [k for k in state_dict if not k.startswith(pre)]
        if strict and other:
            raise RuntimeError(f"Error(s) in loading state_dict: unexpected {other[:5]}")
        self._unet.load_state_dict({k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}, strict=strict)
        return self

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _randn(self, shape, seed, draw, sample_offset):
        return _lib.randn(self._lib, self.device, shape, seed, draw, sample_offset)

    # -- sampling ----------------------------------------------------------------------------------
    def _start(self, shape, noise, noise_rows, seed, sample_offset):
        """(seed, start image, noise rows or None) of a sampling loop.  An injected ``noise`` callable is called once for
        the start image, then ``noise_rows`` times, the reference's order of draws; without one the start image is Philox
        draw 0 and the loop draws its rows on the device."""
        return _loop.loop_start(self, shape, noise, seed, sample_offset, [True] * noise_rows)

    # -- training ----------------------------------------------------------------------------------
    def _trainable(self):
        """The library ``Unet`` behind the object; anything else (no handle, or a library without the float-time training
        entry) cannot be trained.  Touches neither a tensor nor the device."""
        from .unet import Unet

        unet = self._unet
        if (not isinstance(unet, Unet) or not unet.float_time_training or getattr(unet, "_handle", None) is None
                or not hasattr(self._lib, self._train_entry)):
            raise NotImplementedError(f"{type(self).__name__} can train a library Unet only (dm_unet_train_enable_ft arms its "
                                      f"handle for the float-time training loss); got {type(unet).__name__}")
        return unet

    def train(self, mode: bool = True):
        """``model.train()``: arm the U-Net for float-time training (gradient buffers, input-gradient convolutions; once)."""
        if mode:
            unet = self._trainable()
            if not unet._loaded:
                raise RuntimeError("load_state_dict() must be called before train()")
            # random_fourier_features: the reference builds time_mlp.0.weights with requires_grad = False
            _lib.check(self._lib.dm_unet_train_enable_ft(unet._handle, int(bool(unet.cfg.random_fourier_features))))
            if not getattr(unet, "_training", False):
                unet.set_dropout_seed(_lib.default_seed())
            unet._training = True
        return self

    def _loss_inputs(self, images, noise):
        """The batch and its noise on the device; the noise defaults to a device Philox draw under a fresh seed."""
        images = images.to(self.device, torch.float32).contiguous()
        noise = (noise.to(self.device, torch.float32).contiguous() if noise is not None
                 else self._randn(images.shape, _lib.default_seed(), 0, 0))
        if noise.shape != images.shape:
            raise RuntimeError(f"noise {tuple(noise.shape)} does not match images {tuple(images.shape)}")
        return images, noise

    def _loss_call(self, args, sync):
        """Run the training entry on ``args`` (``loss_out_host`` and ``stream`` are set here): the loss as a 0-dim CPU
        tensor, or with ``sync=False`` a 0-dim device tensor (nothing waited for)."""
        return _loop.loss_call(self, self._unet._handle, getattr(self._lib, self._train_entry), args, sync)
