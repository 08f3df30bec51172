"""Host-side mirror of the reference's ``KarrasUnet``, the EDM2 magnitude-preserving U-Net (Karras et al., arXiv 2312.02696,
config G; denoising-diffusion-pytorch/denoising_diffusion/karras_unet.py:374-595) in front of a ``dm_kunet_create`` handle.

Inference and sampling only.  Same keyword-only constructor, ``forward(x, time, self_cond=None, class_labels=None)`` and
``state_dict`` keys as the reference.  The handle is a ``dm_unet``: loading, refreshing and reading parameters, the workspace
and the step-graph cache are those of ``Unet``, which this class inherits them from.  Every magnitude-preserving constant is
folded into the packed weights when they are loaded (csrc/dm_kunet.inc).

``ElucidatedDiffusion(KarrasUnet(...))`` samples with both of its loops.  That is a stated deviation: the reference's class
raises ``AttributeError`` on ``net.random_or_learned_sinusoidal_cond``, which this class carries as ``True`` (its time
embedding is a random Fourier feature of a real-valued time).  A network with ``num_classes`` samples with
``class_labels=``.

Restrictions (each raises): ``train(True)`` and the training surface of ``Unet`` (the reference's training forward rewrites
the weights in place: a follow-up); ``attn_dim_head`` other than 32 or 64; an integer-time forward (the time is real-valued).
``attn_flash`` is accepted (same arithmetic), ``dropout`` is accepted and acts in training only.
"""
from __future__ import annotations

import ctypes as C
from math import sqrt

import torch
import torch.nn.functional as F

from . import _lib
from .spec import KarrasUnetConfig, karras_unet_param_spec
from .unet import Unet, _device_index

TRAINING_FOLLOW_UP = ("training KarrasUnet (forced weight normalisation in the training forward, the backward of its operators) "
                      "is a follow-up: this class samples and runs inference only")


class KarrasUnet(Unet):
    """``KarrasUnet(image_size=..., dim=192, ...)`` -- drop-in for the reference class at inference."""

    random_or_learned_sinusoidal_cond = True  # a random Fourier feature of a real-valued time (ElucidatedDiffusion asserts it)
    text_condition = False
    use_cross_attn = False
    float_time_training = False  # ElucidatedDiffusion.train() / forward(images) refuse this network

    def __init__(self, *, image_size, dim=192, dim_max=768, num_classes=None, channels=4, num_downsamples=3,
                 num_blocks_per_stage=4, attn_res=(16, 8), fourier_dim=16, attn_dim_head=64, attn_flash=False, mp_cat_t=0.5,
                 mp_add_emb_t=0.5, attn_res_mp_add_t=0.3, resnet_mp_add_t=0.3, dropout=0.1, self_condition=False,
                 device="cuda:0"):
        if attn_dim_head not in (32, 64):
            raise NotImplementedError("attn_dim_head: the HIP attention kernels support head widths 32 and 64")
        assert num_blocks_per_stage >= 1
        assert fourier_dim % 2 == 0
        attn_res = tuple(attn_res) if isinstance(attn_res, (tuple, list, set, frozenset)) else (attn_res,)
        if len(attn_res) > _lib.DM_MAX_STAGES or num_downsamples >= _lib.DM_MAX_STAGES:
            raise ValueError(f"at most {_lib.DM_MAX_STAGES} attention resolutions and {_lib.DM_MAX_STAGES - 1} downsamples")
        self.cfg = cfg = KarrasUnetConfig(
            image_size=int(image_size), dim=int(dim), dim_max=int(dim_max), num_classes=None if num_classes is None else int(num_classes),
            channels=int(channels), num_downsamples=int(num_downsamples), num_blocks_per_stage=int(num_blocks_per_stage),
            attn_res=tuple(int(r) for r in attn_res), fourier_dim=int(fourier_dim), attn_dim_head=int(attn_dim_head),
            attn_flash=bool(attn_flash), mp_cat_t=float(mp_cat_t), mp_add_emb_t=float(mp_add_emb_t),
            attn_res_mp_add_t=float(attn_res_mp_add_t), resnet_mp_add_t=float(resnet_mp_add_t), dropout=float(dropout),
            self_condition=bool(self_condition))
        self.channels = cfg.channels
        self.image_size = cfg.image_size
        self.self_condition = cfg.self_condition
        self.out_dim = cfg.channels
        self.num_classes = cfg.num_classes
        self.needs_class_labels = cfg.num_classes is not None
        self.num_downsamples = cfg.num_downsamples
        self.dropout = cfg.dropout
        self.device = torch.device(device)
        self._dev_index = _device_index(device)
        self._lib = _lib.load()
        self._handle = C.c_void_p()
        self._loaded = False
        c = _lib.KunetCfg()
        c.image_size, c.dim, c.dim_max, c.num_classes = cfg.image_size, cfg.dim, cfg.dim_max, cfg.num_classes or 0
        c.channels, c.input_channels = cfg.channels, cfg.input_channels
        c.num_downsamples, c.num_blocks_per_stage = cfg.num_downsamples, cfg.num_blocks_per_stage
        c.n_attn_res = len(cfg.attn_res)
        for i, r in enumerate(cfg.attn_res):
            c.attn_res[i] = r
        c.fourier_dim, c.attn_dim_head = cfg.fourier_dim, cfg.attn_dim_head
        c.mp_cat_t, c.mp_add_emb_t = cfg.mp_cat_t, cfg.mp_add_emb_t
        c.attn_res_mp_add_t, c.resnet_mp_add_t = cfg.attn_res_mp_add_t, cfg.resnet_mp_add_t
        _lib.check(self._lib.dm_kunet_create(C.byref(c), self._dev_index, C.byref(self._handle)))

    def param_spec(self):
        return karras_unet_param_spec(self.cfg)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(TRAINING_FOLLOW_UP)
        return self

    # -- class labels --------------------------------------------------------------------------------------------------------
    def class_rows(self, class_labels, batch):
        """Integer, one-hot or soft labels as the (B, num_classes) fp32 matrix the conditioning head reads, already times
        ``sqrt(num_classes)`` (karras_unet.py:548-553)."""
        nc = self.cfg.num_classes
        labels = torch.as_tensor(class_labels)
        if labels.dtype in (torch.int, torch.long):
            labels = F.one_hot(labels.long(), nc)
        assert labels.shape[-1] == nc
        if labels.shape[0] != batch:
            raise RuntimeError(f"class_labels has {labels.shape[0]} rows for a batch of {batch}")
        return labels.float() * sqrt(nc)

    def set_class_labels(self, class_labels, batch):
        """Hand the labels of the next calls with this batch size to the handle (``dm_kunet_set_class_labels``).  They are
        device data of the conditioning head: a captured step graph serves any labels."""
        assert not ((class_labels is not None) ^ (self.cfg.num_classes is not None)), \
            "class_labels are required by a network with num_classes and refused by one without"
        if class_labels is None:
            return
        rows = self.class_rows(class_labels, batch).to(self.device).contiguous()
        _lib.check(self._lib.dm_kunet_set_class_labels(self._handle, _lib.ptr(rows), int(batch)))

    # -- forward -------------------------------------------------------------------------------------------------------------
    def forward(self, x, time, self_cond=None, class_labels=None):
        """karras_unet.py:521-595.  ``time``: one real value per image (or one for the batch)."""
        cfg = self.cfg
        assert tuple(x.shape[1:]) == (cfg.channels, cfg.image_size, cfg.image_size), \
            f"input {tuple(x.shape[1:])}, the network takes {(cfg.channels, cfg.image_size, cfg.image_size)}"
        assert cfg.self_condition or self_cond is None, "the model was built without self_condition"
        assert not ((class_labels is not None) ^ (cfg.num_classes is not None)), \
            "class_labels are required by a network with num_classes and refused by one without"
        if not self._loaded:
            raise RuntimeError("load_state_dict() must be called before forward()")
        x = x.to(device=self.device, dtype=torch.float32)
        if cfg.self_condition:
            if self_cond is None:
                self_cond = torch.zeros_like(x)
            x = torch.cat((self_cond.to(x), x), dim=1)
        x = x.contiguous()
        B, _, H, W = x.shape
        t = torch.as_tensor(time).to(device=self.device, dtype=torch.float32).reshape(-1)
        if t.numel() == 1 and B > 1:
            t = t.expand(B)
        if t.numel() != B:
            raise RuntimeError(f"time has {t.numel()} entries for a batch of {B}")
        t = t.contiguous()
        self.set_class_labels(class_labels, B)
        out = torch.empty((B, cfg.channels, H, W), device=self.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_unet_forward_ft(self._handle, _lib.ptr(x), _lib.ptr(t), None, 0, _lib.ptr(out), B, H, W, stream))
        return out

    __call__ = forward

    def forward_with_cond_scale(self, *a, **k):
        raise NotImplementedError("KarrasUnet has no text condition")


def _refused(name):
    def method(self, *a, **k):
        raise NotImplementedError(f"KarrasUnet.{name}: {TRAINING_FOLLOW_UP}")
    method.__name__ = name
    return method


# the training surface KarrasUnet inherits from Unet: refused as train() is, not left to fail inside the library
for _name in ("set_dropout_seed", "grad", "grads", "grads_flat", "grad_buckets", "bucket_wait", "optimizer_step", "ema_update",
              "optimizer_state_dict", "load_optimizer_state_dict", "load_ema_state_dict", "sync", "check_device_pack"):
    assert hasattr(Unet, _name), _name
    setattr(KarrasUnet, _name, _refused(_name))
