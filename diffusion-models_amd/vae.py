"""Host-side mirror of the first-stage models of latent-diffusion/ldm/models/autoencoder.py: ``VQModel`` (:14-121),
``VQModelInterface`` (:318-336) and ``AutoencoderKL`` (:339-396) with its ``DiagonalGaussianDistribution``
(ldm/modules/distributions/distributions.py:24-62).  ``decode`` = ``post_quant_conv`` -> ``Decoder``
(ldm/modules/diffusionmodules/model.py:476-585) is ``dm_decoder_forward`` in libdm_hip.so, ``encode`` = ``Encoder`` ->
``quant_conv`` -> quantiser or posterior is ``dm_encoder_forward`` / ``dm_encoder_forward_kl``."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict

import torch

from . import _lib
from .spec import (DecoderConfig, EncoderConfig, autoencoder_kl_param_spec, decoder_param_spec,  # noqa: F401
                   encoder_param_spec)
from .unet import _device_index


class _Net:
    """What ``VQDecoder`` and ``VQEncoder`` share: one handle of libdm_hip.so, made from the ddconfig fields that both
    networks have and filled by ``load_state_dict``.  A subclass names its cfg struct and its four library functions."""

    _Cfg = _create = _destroy = _set_param = _finalize = None

    def _open(self, cfg, device, **own):
        """``own``: the fields of the cfg struct that only this network has."""
        self.cfg = cfg
        self.device = torch.device(device)
        self._lib = _lib.load()
        self._handle = C.c_void_p()
        self._loaded = False
        c = self._Cfg()
        c.ch, c.n_levels = cfg.ch, cfg.num_resolutions
        for i, m in enumerate(cfg.ch_mult):
            c.ch_mult[i] = m
        c.num_res_blocks = cfg.num_res_blocks
        c.n_attn_res = len(cfg.attn_resolutions)
        for i, r in enumerate(cfg.attn_resolutions):
            c.attn_resolutions[i] = r
        c.resolution, c.z_channels, c.embed_dim = cfg.resolution, cfg.z_channels, cfg.embed_dim
        for k, v in own.items():
            setattr(c, k, v)
        _lib.check(getattr(self._lib, self._create)(C.byref(c), _device_index(device), C.byref(self._handle)))

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            getattr(self._lib, self._destroy)(h)
            h.value = None

    def eval(self):
        return self

    def parameters(self):
        return iter(())

    def load_state_dict(self, state_dict, strict: bool = True):
        spec = dict(self.param_spec())
        missing = [k for k in spec if k not in state_dict]
        if missing:
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing[:5]}")
        set_param = getattr(self._lib, self._set_param)
        for name, shape in spec.items():
            t = state_dict[name].detach().to(device="cpu", dtype=torch.float32).contiguous()
            if tuple(t.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {name}: {tuple(t.shape)} vs {tuple(shape)}")
            shp = (C.c_int64 * t.dim())(*t.shape)
            _lib.check(set_param(self._handle, name.encode(), t.data_ptr(), shp, t.dim()))
        _lib.check(getattr(self._lib, self._finalize)(self._handle))
        self._loaded = True
        return self


class VQDecoder(_Net):
    """``vae = VQDecoder(ddconfig, embed_dim); vae.load_state_dict(vqmodel_state_dict); vae.decode(z)``.

    ``load_state_dict`` takes the ``state_dict`` of the reference ``VQModel`` (or a Lightning
    checkpoint's ``state_dict``) and uses the ``post_quant_conv.*`` and ``decoder.*`` entries."""

    _Cfg = _lib.DecoderCfg
    _create, _destroy = "dm_decoder_create", "dm_decoder_destroy"
    _set_param, _finalize = "dm_decoder_set_param", "dm_decoder_finalize"

    def __init__(self, ddconfig: Dict, embed_dim: int, device="cuda:0"):
        cfg = DecoderConfig(
            ch=ddconfig["ch"], out_ch=ddconfig["out_ch"], ch_mult=tuple(ddconfig["ch_mult"]),
            num_res_blocks=ddconfig["num_res_blocks"], attn_resolutions=tuple(ddconfig.get("attn_resolutions", ())),
            resolution=ddconfig["resolution"], z_channels=ddconfig["z_channels"], embed_dim=embed_dim,
        )
        self._open(cfg, device, out_ch=cfg.out_ch)

    def param_spec(self):
        return decoder_param_spec(self.cfg)

    def decoded_shape(self, latent_chw):
        """(C, H, W) of ``decode`` for one latent of shape (embed_dim, h, w)."""
        f = 2 ** (self.cfg.num_resolutions - 1)
        return (self.cfg.out_ch, int(latent_chw[1]) * f, int(latent_chw[2]) * f)

    @torch.inference_mode()
    def decode(self, quant):
        if not self._loaded:
            raise RuntimeError("load_state_dict() must be called before decode()")
        z = quant.to(device=self.device, dtype=torch.float32).contiguous()
        B, Cz, h, w = z.shape
        if Cz != self.cfg.embed_dim:
            raise RuntimeError(f"expected {self.cfg.embed_dim} latent channels, got {Cz}")
        f = 2 ** (self.cfg.num_resolutions - 1)
        out = torch.empty((B, self.cfg.out_ch, h * f, w * f), device=self.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_decoder_forward(self._handle, _lib.ptr(z), _lib.ptr(out), B, h, w, stream))
        return out


class VQEncoder(_Net):
    """Mirror of ``VQModel.encode`` / ``encode_to_prequant`` (autoencoder.py:102-111): ``Encoder`` -> ``quant_conv`` ->
    nearest-codebook quantisation, executed by ``dm_encoder_forward``.  ``load_state_dict`` takes the ``VQModel``
    state dict and uses its ``encoder.*``, ``quant_conv.*`` and ``quantize.embedding.weight`` entries."""

    _Cfg = _lib.EncoderCfg
    _create, _destroy = "dm_encoder_create", "dm_encoder_destroy"
    _set_param, _finalize = "dm_encoder_set_param", "dm_encoder_finalize"

    def __init__(self, ddconfig: Dict, embed_dim: int, n_embed: int, device="cuda:0"):
        cfg = EncoderConfig(
            ch=ddconfig["ch"], in_channels=ddconfig.get("in_channels", 3), ch_mult=tuple(ddconfig["ch_mult"]),
            num_res_blocks=ddconfig["num_res_blocks"], attn_resolutions=tuple(ddconfig.get("attn_resolutions", ())),
            resolution=ddconfig["resolution"], z_channels=ddconfig["z_channels"], embed_dim=embed_dim, n_embed=n_embed,
            double_z=bool(ddconfig.get("double_z", False)),
        )
        self._open(cfg, device, in_channels=cfg.in_channels, n_embed=cfg.n_embed, double_z=int(cfg.double_z))

    def param_spec(self):
        return encoder_param_spec(self.cfg)

    def _run(self, x, want_quant: bool):
        if not self._loaded:
            raise RuntimeError("load_state_dict() must be called before encode()")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        B, Cin, H, W = x.shape
        if Cin != self.cfg.in_channels:
            raise RuntimeError(f"expected {self.cfg.in_channels} image channels, got {Cin}")
        f = 2 ** (self.cfg.num_resolutions - 1)
        shape = (B, self.cfg.embed_dim, H // f, W // f)
        pre = torch.empty(shape, device=self.device, dtype=torch.float32)
        zq = torch.empty(shape, device=self.device, dtype=torch.float32) if want_quant else None
        idx = torch.empty((B * shape[2] * shape[3],), device=self.device, dtype=torch.int32) if want_quant else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_encoder_forward(self._handle, _lib.ptr(x), _lib.ptr(zq), _lib.ptr(pre), _lib.ptr(idx), B, H,
                                                W, stream))
        return zq, pre, idx

    @torch.inference_mode()
    def encode(self, x):
        """(quant, emb_loss, (perplexity, min_encodings, indices)) like ``VQModel.encode``; the loss terms are training
        quantities and come back as ``None``."""
        zq, _, idx = self._run(x, True)
        return zq, None, (None, None, idx.to(torch.int64))

    @torch.inference_mode()
    def encode_to_prequant(self, x):
        return self._run(x, False)[1]

    def _latent(self, t, dtype, what):
        if not self._loaded:
            raise RuntimeError(f"load_state_dict() must be called before {what}()")
        return t.to(device=self.device, dtype=dtype).contiguous()

    @torch.inference_mode()
    def quantize(self, h):
        """``VectorQuantizer.forward`` on a pre-quantisation latent (B, embed_dim, h, w) -> (quant, indices): the codebook
        search of ``encode`` reading NCHW (``dm_encoder_quantize``)."""
        h = self._latent(h, torch.float32, "quantize")
        B, E, hh, ww = h.shape
        if E != self.cfg.embed_dim:
            raise RuntimeError(f"expected {self.cfg.embed_dim} latent channels, got {E}")
        zq = torch.empty_like(h)
        idx = torch.empty((B * hh * ww,), device=self.device, dtype=torch.int32)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_encoder_quantize(self._handle, _lib.ptr(h), _lib.ptr(zq), _lib.ptr(idx), B, hh, ww, stream))
        return zq, idx.to(torch.int64)

    @torch.inference_mode()
    def embed_code(self, code_b):
        """``quantize.embed_code`` + ``b h w c -> b c h w`` (autoencoder.py:118-120): codes (B, h, w) -> (B, embed_dim, h, w)
        (``dm_encoder_embed_code``).  A code outside the codebook raises."""
        if code_b.dim() != 3:
            raise RuntimeError(f"expected codes of shape (B, h, w), got {tuple(code_b.shape)}")
        code = self._latent(code_b, torch.int64, "embed_code")
        B, hh, ww = code.shape
        out = torch.empty((B, self.cfg.embed_dim, hh, ww), device=self.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_encoder_embed_code(self._handle, _lib.ptr(code), _lib.ptr(out), B, hh, ww, stream))
        return out


class KLEncoder(VQEncoder):
    """``AutoencoderKL.encode`` (autoencoder.py:374-378): ``Encoder`` -> ``quant_conv`` -> posterior, executed by
    ``dm_encoder_forward_kl`` on an encoder handle without a codebook (``n_embed = 0``).  ``load_state_dict`` uses the
    ``encoder.*`` and ``quant_conv.*`` entries."""

    def __init__(self, ddconfig: Dict, embed_dim: int, device="cuda:0"):
        assert ddconfig["double_z"], "AutoencoderKL needs ddconfig['double_z']"
        super().__init__(ddconfig, embed_dim, 0, device=device)

    @torch.inference_mode()
    def forward_kl(self, x, *, want_moments=False, want_z=False, want_kl=False, sample=True, noise=None, seed=None):
        """(moments, z, kl), each ``None`` unless asked for: one ``dm_encoder_forward_kl`` call."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() must be called before encode()")
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        B, Cin, H, W = x.shape
        if Cin != self.cfg.in_channels:
            raise RuntimeError(f"expected {self.cfg.in_channels} image channels, got {Cin}")
        f = 2 ** (self.cfg.num_resolutions - 1)
        E, h, w = self.cfg.embed_dim, H // f, W // f
        new = lambda *shape: torch.empty(shape, device=self.device, dtype=torch.float32)  # noqa: E731
        moments = new(B, 2 * E, h, w) if want_moments else None
        z = new(B, E, h, w) if want_z else None
        kl = new(B) if want_kl else None
        eps = None
        if want_z and sample:
            if noise is not None:
                eps = noise.to(device=self.device, dtype=torch.float32).contiguous()
                if tuple(eps.shape) != (B, E, h, w):
                    raise RuntimeError(f"noise must have the latent's shape {(B, E, h, w)}, got {tuple(eps.shape)}")
            elif seed is None:
                seed = _lib.default_seed()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_encoder_forward_kl(self._handle, _lib.ptr(x), _lib.ptr(moments), _lib.ptr(z), _lib.ptr(kl),
                                                   _lib.ptr(eps), C.c_uint64(int(seed or 0)), C.c_uint64(0), C.c_uint64(0),
                                                   int(bool(sample)), B, H, W, stream))
        return moments, z, kl

    def encode(self, x):
        return DiagonalGaussianDistribution(self.forward_kl(x, want_moments=True)[0])

    def encode_to_prequant(self, x):
        raise RuntimeError("a KL first stage has no quantiser")

    quantize = embed_code = encode_to_prequant


class DiagonalGaussianDistribution:
    """distributions.py:24-62 on device tensors.  ``sample`` / ``mode`` / ``kl()`` run the library's posterior kernel
    (``dm_op_kl_posterior``); ``kl(other)`` and ``nll`` are the reference's expressions in torch (they train the VAE and are
    on no hot path here).  Deviation: the reference draws ``torch.randn`` on the CPU; here the draw is the library's
    Philox stream on the device (``dm_randn`` of the latent's shape, draw 0) under ``seed`` -- taken from torch's global
    generator when none is given, as elsewhere in the package -- and ``noise=`` injects the draw."""

    def __init__(self, parameters, deterministic=False):
        if not (torch.is_tensor(parameters) and parameters.is_cuda):
            raise RuntimeError("DiagonalGaussianDistribution takes a tensor on the GPU (there is no CPU path)")
        if parameters.dim() != 4 or parameters.shape[1] % 2 != 0:
            raise RuntimeError(f"parameters must be (B, 2E, h, w), got {tuple(parameters.shape)}")
        self.parameters = parameters.to(torch.float32).contiguous()
        self.deterministic = deterministic
        self.mean, logvar = torch.chunk(self.parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        if deterministic:
            self.var = self.std = torch.zeros_like(self.mean)
        else:
            self.std = torch.exp(0.5 * self.logvar)
            self.var = torch.exp(self.logvar)

    def _posterior(self, *, want_z=False, want_kl=False, sample=False, noise=None, seed=None):
        p = self.parameters
        B, E2, h, w = p.shape
        E = E2 // 2
        z = torch.empty((B, E, h, w), device=p.device, dtype=torch.float32) if want_z else None
        kl = torch.empty((B,), device=p.device, dtype=torch.float32) if want_kl else None
        eps = None
        if noise is not None:
            eps = noise.to(device=p.device, dtype=torch.float32).contiguous()
            if tuple(eps.shape) != (B, E, h, w):
                raise RuntimeError(f"noise must have the latent's shape {(B, E, h, w)}, got {tuple(eps.shape)}")
        with torch.cuda.device(p.device):
            stream = torch.cuda.current_stream(p.device).cuda_stream
            _lib.check(_lib.load().dm_op_kl_posterior(_lib.ptr(p), _lib.KL_NCHW, _lib.ptr(eps), C.c_uint64(int(seed or 0)),
                                                      C.c_uint64(0), C.c_uint64(0), int(bool(sample)), _lib.ptr(z), None,
                                                      _lib.ptr(kl), B, E, h * w, stream))
        return z, kl

    @torch.inference_mode()
    def sample(self, *, noise=None, seed=None):
        if self.deterministic:  # std = 0 (:32-33): the sample is the mean
            return self.mode()
        if noise is None and seed is None:
            seed = _lib.default_seed()
        return self._posterior(want_z=True, sample=True, noise=noise, seed=seed)[0]

    @torch.inference_mode()
    def mode(self):
        return self._posterior(want_z=True)[0]

    @torch.inference_mode()
    def kl(self, other=None):
        if self.deterministic:
            return torch.Tensor([0.])
        if other is None:
            return self._posterior(want_kl=True)[1]
        return 0.5 * torch.sum(torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0 - self.logvar
                               + other.logvar, dim=[1, 2, 3])

    @torch.inference_mode()
    def nll(self, sample, dims=[1, 2, 3]):
        if self.deterministic:
            return torch.Tensor([0.])
        logtwopi = math.log(2.0 * math.pi)
        sample = sample.to(device=self.mean.device, dtype=torch.float32)
        return 0.5 * torch.sum(logtwopi + self.logvar + torch.pow(sample - self.mean, 2) / self.var, dim=dims)


class _FirstStage:
    """What ``VQModel`` and ``AutoencoderKL`` share: an encoder and a ``VQDecoder`` over one ``state_dict``."""

    def _open(self, encoder, ddconfig, embed_dim, device, image_key, ckpt_path, ignore_keys):
        self.image_key = image_key
        self.encoder = encoder
        self.decoder = VQDecoder(ddconfig, embed_dim, device=device)
        self.device = torch.device(device)
        if ckpt_path is not None:
            self.init_from_ckpt(ckpt_path, ignore_keys=ignore_keys)

    def init_from_ckpt(self, path, ignore_keys=()):
        """autoencoder.py:78-91 / :363-372 through the safe loader of checkpoint.py."""
        from .checkpoint import load_vae_checkpoint

        sd = {k: v for k, v in load_vae_checkpoint(path).items() if not any(k.startswith(ik) for ik in ignore_keys)}
        self.load_state_dict(sd, strict=False)
        return self

    def eval(self):
        return self

    def parameters(self):
        return iter(())

    def load_state_dict(self, state_dict, strict: bool = True):
        self.encoder.load_state_dict(state_dict, strict)
        self.decoder.load_state_dict(state_dict, strict)
        return self

    def encode(self, x):
        return self.encoder.encode(x)

    def decode(self, quant):
        return self.decoder.decode(quant)

    def decoded_shape(self, latent_chw):
        return self.decoder.decoded_shape(latent_chw)


class VQModel(_FirstStage):
    """``VQModel`` of the reference restricted to inference: ``encode`` / ``encode_to_prequant`` / ``decode`` over one
    ``state_dict`` (autoencoder.py:14-121)."""

    def __init__(self, ddconfig: Dict, lossconfig=None, n_embed: int = None, embed_dim: int = None, ckpt_path=None,
                 ignore_keys=(), image_key="image", colorize_nlabels=None, monitor=None, batch_resize_range=None,
                 scheduler_config=None, lr_g_factor=1.0, remap=None, sane_index_shape=False, use_ema=False, *,
                 device="cuda:0"):
        """The reference's positional order (autoencoder.py:15-31: ddconfig, lossconfig, n_embed, embed_dim, ...).  The loss
        network, the Lightning / EMA / scheduler options are training-only and ignored; ``ckpt_path`` loads the state dict
        (``load_vae_checkpoint``: ``weights_only=True``) minus the keys that start with one of ``ignore_keys``."""
        assert n_embed is not None and embed_dim is not None, "n_embed and embed_dim are required"
        assert remap is None and not sane_index_shape, "remap / sane_index_shape are not on the HIP path"
        self._open(VQEncoder(ddconfig, embed_dim, n_embed, device=device), ddconfig, embed_dim, device, image_key, ckpt_path,
                   ignore_keys)

    def param_spec(self):
        return self.encoder.param_spec() + self.decoder.param_spec()

    def encode_to_prequant(self, x):
        return self.encoder.encode_to_prequant(x)

    def decode_code(self, code_b):
        """autoencoder.py:118-121: codes (B, h, w) -> their codebook rows as a latent -> ``decode``."""
        return self.decode(self.encoder.embed_code(code_b))

    def forward(self, input, return_pred_indices=False):
        """autoencoder.py:123-128: encode, quantize, decode -> (dec, diff[, indices]); the commitment loss ``diff`` is a
        training quantity and comes back as ``None``."""
        quant, diff, (_, _, ind) = self.encode(input)
        dec = self.decode(quant)
        return (dec, diff, ind) if return_pred_indices else (dec, diff)

    __call__ = forward


class VQModelInterface(VQModel):
    """``VQModelInterface`` (autoencoder.py:318-336): diffusion runs on the pre-quantisation latents, and ``decode``
    quantises first."""

    def __init__(self, embed_dim, *args, **kwargs):
        super().__init__(*args, embed_dim=embed_dim, **kwargs)
        self.embed_dim = embed_dim

    def encode(self, x):
        return self.encoder.encode_to_prequant(x)

    def decode(self, h, force_not_quantize=False):
        quant = h if force_not_quantize else self.encoder.quantize(h)[0]
        return self.decoder.decode(quant)

    def forward(self, input, return_pred_indices=False):
        """``VQModel.forward`` unpacks a triple that this class's ``encode`` does not return (the reference's own
        ``VQModelInterface.forward`` raises for that reason): encode, then the quantising decode."""
        h = self.encode(input)
        quant, ind = self.encoder.quantize(h)
        dec = self.decoder.decode(quant)
        return (dec, None, ind) if return_pred_indices else (dec, None)

    __call__ = forward


class AutoencoderKL(_FirstStage):
    """``AutoencoderKL`` of the reference restricted to inference (autoencoder.py:339-396): ``encode`` returns the
    posterior, ``decode`` is ``post_quant_conv`` -> ``Decoder`` (the ``VQDecoder`` of this module), ``forward`` returns
    ``(dec, posterior)``.  ``encode_sample`` is the latent in one library call, the form the latent-diffusion classes
    use.  State-dict keys are the reference's (``encoder.*``, ``decoder.*``, ``quant_conv.*``, ``post_quant_conv.*``);
    ``loss.*`` entries are ignored."""

    def __init__(self, ddconfig: Dict, lossconfig=None, embed_dim: int = None, ckpt_path=None, ignore_keys=(),
                 image_key="image", colorize_nlabels=None, monitor=None, *, device="cuda:0"):
        """The reference's positional order (:340-349).  The loss network, ``colorize_nlabels`` and ``monitor`` belong to
        training and logging and are ignored; ``ckpt_path`` loads the state dict (``load_vae_checkpoint``:
        ``weights_only=True``) minus the keys that start with one of ``ignore_keys``."""
        assert embed_dim is not None, "embed_dim is required"
        assert ddconfig["double_z"]
        self.embed_dim = embed_dim
        if monitor is not None:
            self.monitor = monitor
        self._open(KLEncoder(ddconfig, embed_dim, device=device), ddconfig, embed_dim, device, image_key, ckpt_path,
                   ignore_keys)

    def param_spec(self):
        """``state_dict()`` order of the reference: encoder, decoder, quant_conv, post_quant_conv."""
        return autoencoder_kl_param_spec(self.encoder.cfg, self.decoder.cfg)

    def encode_sample(self, x, *, sample_posterior=True, noise=None, seed=None, return_kl=False):
        """``encode(x).sample()`` (``.mode()`` with ``sample_posterior=False``) without the round trip through the moments:
        encoder, ``quant_conv`` and the posterior in one ``dm_encoder_forward_kl`` call.  ``return_kl``: ``(z, kl)``."""
        _, z, kl = self.encoder.forward_kl(x, want_z=True, want_kl=return_kl, sample=sample_posterior, noise=noise, seed=seed)
        return (z, kl) if return_kl else z

    def forward(self, input, sample_posterior=True):
        posterior = self.encode(input)
        z = posterior.sample() if sample_posterior else posterior.mode()
        return self.decode(z), posterior

    __call__ = forward
