"""KarrasUnet (the EDM2 magnitude-preserving U-Net) restated in torch from the FOLDED form the HIP path runs: weights
normalised once, every magnitude-preserving constant folded into a weight or into the constant of an elementwise pass, the
downsample as a 2x2 mean in front of its 1x1 convolution, the upsample as the separable 0.25 / 0.75 filter.  dtype-generic
(fp64 for the references, fp32 for the floors of the operator tests).  What is pinned here is the folding algebra itself:
tests/test_karras_host.py compares this file with the reference's own outputs (tests/golden/karras.pt).

``fold`` is the host-side pack of csrc/dm_kunet.inc in the same order and with the same names; ``forward`` is its
``kunet_forward_impl``.  Tensors are NCHW here."""
from __future__ import annotations

from math import pi, sqrt

import torch
import torch.nn.functional as F

from diffusion_models_amd.spec import MP_SILU_GAIN, KarrasUnetConfig, karras_blocks

EPS = 1e-4  # PixelNorm and normalize_weight (karras_unet.py:78, :91)


# ---- constants ------------------------------------------------------------------------------------------------------------------
def mp_add_consts(t):
    """MPAdd(t): out = a x + b res."""
    den = sqrt((1 - t) ** 2 + t ** 2)
    return (1 - t) / den, t / den


def mp_cat_consts(t, na, nb):
    """MPCat(t): out = cat(ca a, cb b)."""
    c = sqrt((na + nb) / ((1 - t) ** 2 + t ** 2))
    return c * (1 - t) / sqrt(na), c * t / sqrt(nb)


def normalize_weight(w, fan_in=None):
    """``normalize_weight(w, eps) / sqrt(fan_in)`` per output row, in the dtype of ``w``.  ``fan_in`` differs from the row's
    element count for ``input_block`` alone, whose row counts the ones channel and whose fan_in does not."""
    rows = w.reshape(w.shape[0], -1)
    numel = rows.shape[1]
    n = rows.norm(dim=1, keepdim=True).clamp_min(EPS)
    return (rows / n * (sqrt(numel) / sqrt(fan_in if fan_in is not None else numel))).reshape(w.shape)


# ---- operators ------------------------------------------------------------------------------------------------------------------
def pixel_norm(x, dim=1):
    return x / x.norm(dim=dim, keepdim=True).clamp_min(EPS) * sqrt(x.shape[dim])


def pixelnorm_op(x, res_scale):
    """kunet_pixelnorm: (pn * res_scale, silu(pn))."""
    pn = pixel_norm(x, 1)
    return pn * res_scale, F.silu(pn)


def avgpool2(x):
    b, c, h, w = x.shape
    return x.reshape(b, c, h // 2, 2, w // 2, 2).mean(dim=(3, 5))


def _up2_axis(x, dim):
    n = x.shape[dim]
    idx = torch.arange(n, device=x.device)
    lo, hi = x.index_select(dim, (idx - 1).clamp_min(0)), x.index_select(dim, (idx + 1).clamp_max(n - 1))
    even, odd = 0.25 * lo + 0.75 * x, 0.75 * x + 0.25 * hi
    out = torch.stack((even, odd), dim=dim + 1)
    shape = list(x.shape)
    shape[dim] = 2 * n
    return out.reshape(shape)


def bilinear_up2(x):
    """F.interpolate(x, (2h, 2w), mode='bilinear'): output 2i = 0.25 x[i-1] + 0.75 x[i], output 2i+1 = 0.75 x[i] + 0.25 x[i+1],
    indices clamped to the edge, along each axis."""
    return _up2_axis(_up2_axis(x, 2), 3)


def up2_op(x, res_scale):
    """kunet_bilinear_up2: (x_up, silu(x_up), x_up * res_scale)."""
    u = bilinear_up2(x)
    return u, F.silu(u), u * res_scale


def act_op(a, ca, b=None, cb=1.0, copy_scale=None):
    """kunet_act: silu(ca a) [cat silu(cb b)] and optionally the scaled copy of ``a``."""
    y = F.silu(a * ca)
    if b is not None:
        y = torch.cat((y, F.silu(b * cb)), dim=1)
    return y, (a * copy_scale if copy_scale is not None else None)


def qkv_norm_op(qkv, heads, dh):
    """kunet_qkv_norm on (B, 3 heads dh, H, W): every head's q, k and v pixel-normed along dh."""
    b, c, h, w = qkv.shape
    t = qkv.reshape(b, 3 * heads, dh, h, w)
    return pixel_norm(t, 2).reshape(b, c, h, w)


def attention_core(qkv, mem_kv, heads, dh):
    """softmax(q k^T dh^-0.5) v with the (already normalised) memory rows in front of the keys / values."""
    b, _, h, w = qkv.shape
    q, k, v = (t.reshape(b, heads, dh, h * w).transpose(2, 3) for t in qkv.chunk(3, dim=1))
    mk, mv = (m.unsqueeze(0).expand(b, -1, -1, -1) for m in mem_kv)
    k, v = torch.cat((mk, k), dim=2), torch.cat((mv, v), dim=2)
    p = (q @ k.transpose(2, 3) * dh ** -0.5).softmax(dim=-1)
    return (p @ v).transpose(2, 3).reshape(b, heads * dh, h, w)


def fourier(time, weights):
    f = (time[:, None] * weights[None, :]) * (2 * pi)
    return torch.cat((f.sin(), f.cos()), dim=-1) * sqrt(2)


def head_op(P, time, labels=None):
    """The conditioning head: Fourier features [| labels sqrt(num_classes)] -> one Linear (MPAdd folded in) -> silu -> the
    concatenated to_emb matrix (gain and 1 / 0.596 folded in).  (B, ss_total): per block dout scale columns, then dout zeros."""
    e = fourier(time.to(P["fourier_w"].dtype), P["fourier_w"])
    if labels is not None:
        e = torch.cat((e, labels.to(e.dtype)), dim=-1)
    return F.silu(e @ P["emb_w"].t()) @ P["ss_w"].t()


def class_rows(class_labels, num_classes, dtype):
    """Integer, one-hot or soft labels as the (B, num_classes) matrix the head reads: already times sqrt(num_classes)."""
    if not class_labels.is_floating_point():
        class_labels = F.one_hot(class_labels.long(), num_classes)
    assert class_labels.shape[-1] == num_classes
    return class_labels.to(dtype) * sqrt(num_classes)


# ---- the pack ---------------------------------------------------------------------------------------------------------------------
def fold_block(sd, b, cfg: KarrasUnetConfig, ss_off):
    """Folded weights of one Encoder / Decoder (csrc/dm_kunet.inc: build_kblock)."""
    p = b.name
    a, r = mp_add_consts(cfg.resnet_mp_add_t)
    K = dict(block=b, ss_off=ss_off, res_scale=r, ca=1.0, cb=1.0)
    if b.down:
        K["down_w"] = normalize_weight(sd[f"{p}.downsample_conv.weight"])
    K["w1"] = normalize_weight(sd[f"{p}.block1.1.weight"]) * MP_SILU_GAIN
    K["w2"] = normalize_weight(sd[f"{p}.block2.2.weight"]) * (MP_SILU_GAIN * a)
    if b.skip:
        na = b.din - b.dout  # the width of x; the skip has the rest
        K["na"] = na
        K["ca"], K["cb"] = mp_cat_consts(cfg.mp_cat_t, na, b.din - na)
    if b.res_conv:
        w = normalize_weight(sd[f"{p}.res_conv.weight"]) * r
        if b.skip:
            w = torch.cat((w[:, :K["na"]] * K["ca"], w[:, K["na"]:] * K["cb"]), dim=1)
        K["res_w"] = w
    if b.attn:
        aa, ar = mp_add_consts(cfg.attn_res_mp_add_t)
        K["heads"] = cfg.heads(b.dout)
        K["attn_res_scale"] = ar
        K["qkv_w"] = normalize_weight(sd[f"{p}.attn.to_qkv.weight"])
        K["out_w"] = normalize_weight(sd[f"{p}.attn.to_out.weight"]) * aa
        K["mem_kv"] = pixel_norm(sd[f"{p}.attn.mem_kv"], -1)
    return K


def fold(sd, cfg: KarrasUnetConfig, dtype=torch.float64):
    """Every packed buffer of the handle from a state dict, formed in double and rounded once to ``dtype``."""
    sd = {k: v.double() for k, v in sd.items()}
    P = dict(cfg=cfg)
    cin = cfg.input_channels
    P["in_w"] = normalize_weight(sd["input_block.weight"], fan_in=cin * 9)
    P["out_w"] = normalize_weight(sd["output_block.0.weight"]) * sd["output_block.1.gain"]
    P["fourier_w"] = sd["to_time_emb.0.weights"]
    wt = normalize_weight(sd["to_time_emb.1.weight"])
    if cfg.num_classes is not None:
        a, r = mp_add_consts(cfg.mp_add_emb_t)
        wt = torch.cat((wt * a, normalize_weight(sd["to_class_emb.weight"]) * r), dim=1)
    P["emb_w"] = wt
    blocks = karras_blocks(cfg)
    ss, off = [], 0
    for group in ("downs", "mids", "ups"):
        P[group] = []
        for b in blocks[group]:
            P[group].append(fold_block(sd, b, cfg, off))
            w = normalize_weight(sd[f"{b.name}.to_emb.0.weight"]) * (sd[f"{b.name}.to_emb.1.gain"] * MP_SILU_GAIN)
            ss += [w, torch.zeros_like(w)]  # the shift rows of EPI_SCALE_SHIFT: zero
            off += 2 * b.dout
    P["ss_w"] = torch.cat(ss, dim=0)

    def cast(v):
        if torch.is_tensor(v):
            return v.to(dtype)
        if isinstance(v, dict):
            return {k: cast(x) for k, x in v.items()}
        if isinstance(v, list):
            return [cast(x) for x in v]
        return v

    return cast(P)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------
def conv(x, w):
    return F.conv2d(x, w, padding=w.shape[-1] // 2)


def scale_of(K, ss):
    return 1 + ss[:, K["ss_off"]:K["ss_off"] + K["block"].dout, None, None]


def attention(K, x, cfg):
    heads, dh = K["heads"], cfg.attn_dim_head
    qkv = qkv_norm_op(conv(x, K["qkv_w"]), heads, dh)
    o = attention_core(qkv, K["mem_kv"], heads, dh)
    return conv(o, K["out_w"]) + x * K["attn_res_scale"]


def encoder(K, x, ss, cfg):
    if K["block"].down:
        x = conv(avgpool2(x), K["down_w"])
    res, act = pixelnorm_op(x, K["res_scale"])
    h = F.silu(conv(act, K["w1"]) * scale_of(K, ss))
    y = conv(h, K["w2"]) + res
    return attention(K, y, cfg) if K["block"].attn else y


def decoder(K, x, skip, ss, cfg):
    b = K["block"]
    if b.up:
        xu, act, res = up2_op(x, K["res_scale"])
        if b.res_conv:
            res = conv(xu, K["res_w"])
    elif b.skip:
        act, _ = act_op(x, K["ca"], skip, K["cb"])
        res = conv(torch.cat((x, skip), dim=1), K["res_w"])
    else:
        act, res = act_op(x, 1.0, copy_scale=K["res_scale"])
        if b.res_conv:
            res = conv(x, K["res_w"])
    h = F.silu(conv(act, K["w1"]) * scale_of(K, ss))
    y = conv(h, K["w2"]) + res
    return attention(K, y, cfg) if b.attn else y


def input_block(P, x):
    return conv(torch.cat((torch.ones_like(x[:, :1]), x), dim=1), P["in_w"])


def forward(P, x, time, self_cond=None, class_labels=None):
    """KarrasUnet.forward (karras_unet.py:521-595) on the folded weights ``P = fold(sd, cfg, dtype)``."""
    cfg = P["cfg"]
    dtype = P["in_w"].dtype
    x = x.to(dtype)
    assert x.shape[1:] == (cfg.channels, cfg.image_size, cfg.image_size)
    if cfg.self_condition:
        x = torch.cat((torch.zeros_like(x) if self_cond is None else self_cond.to(dtype), x), dim=1)
    else:
        assert self_cond is None
    assert (class_labels is not None) == (cfg.num_classes is not None)
    labels = class_rows(class_labels, cfg.num_classes, dtype) if class_labels is not None else None
    ss = head_op(P, time.to(dtype), labels)
    x = input_block(P, x)
    skips = [x]
    for K in P["downs"]:
        x = encoder(K, x, ss, cfg)
        skips.append(x)
    for K in P["mids"]:
        x = decoder(K, x, None, ss, cfg)
    for K in P["ups"]:
        x = decoder(K, x, skips.pop() if K["block"].skip else None, ss, cfg)
    return conv(x, P["out_w"])
