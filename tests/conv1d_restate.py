"""fp32 restatements of the sequence model's convolution forms, for the floors of tests/test_hip_seq1d_ops.py and for the
CPU tests of the packers (tests/test_seq1d_host.py).  Each mirrors what the library does on the host or in a kernel; none
of them calls it.

* ``upsample1d_pack``: nearest x2 + Conv1d(3, padding 1) as one K = 3 convolution with 2 Cout channels on the source grid
  (make_upsample1d, csrc/dm_api.hip).
* ``direct``: the K-tap sum in fp32.
"""
import torch
import torch.nn.functional as F


def upsample1d_pack(w, b=None):
    """w (Cout, Cin, 3) -> (2 Cout, Cin, 3): rows [0, Cout) hold the taps {w0, w1 + w2, 0} of the even outputs, rows
    [Cout, 2 Cout) hold {0, w0 + w1, w2} of the odd ones; the bias twice.  Sums in the dtype of ``w``."""
    even = torch.stack([w[..., 0], w[..., 1] + w[..., 2], torch.zeros_like(w[..., 0])], dim=-1)
    odd = torch.stack([torch.zeros_like(w[..., 0]), w[..., 0] + w[..., 1], w[..., 2]], dim=-1)
    return torch.cat([even, odd], dim=0), (None if b is None else torch.cat([b, b], dim=0))


def unpack_upsampled(y2, cout):
    """(B, 2 Cout, L) of the packed convolution -> (B, Cout, 2L): channel p * Cout + o at position i is output o at 2i + p."""
    B, _, L = y2.shape
    return y2.reshape(B, 2, cout, L).permute(0, 2, 3, 1).reshape(B, cout, 2 * L)


def upsample_conv(x, w, b=None):
    """The layer through the packing, in the dtype of the arguments."""
    w2, b2 = upsample1d_pack(w, b)
    return unpack_upsampled(F.conv1d(x, w2, b2, padding=1), w.shape[0])


def upsample_reference(x, w, b=None):
    """The layer as the reference runs it (denoising_diffusion_1d.py:56-60), in the dtype of the arguments."""
    return F.conv1d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)


def direct(x, w, b=None, stride=1, pad=0):
    """The K-tap sum in fp32 (the direct family, the 1x1 GEMM and the thin kernel sum in another order of the same terms)."""
    return F.conv1d(x.float(), w.float(), None if b is None else b.float(), stride=stride, padding=pad)


def rms_norm(x, g):
    """RMSNorm over the channels of (B, C, L) (denoising_diffusion_1d.py:65-71)."""
    return F.normalize(x, dim=1) * g.reshape(1, -1, 1) * (x.shape[1] ** 0.5)


def block(x, w, b, g, scale=None, shift=None, residual=None, conv=None):
    """Block.forward (:127-136) with an optional residual behind the SiLU, in the dtype of the arguments; ``conv``: the
    restatement of the convolution (default: F.conv1d)."""
    h = conv(x, w, b) if conv is not None else F.conv1d(x, w, b, padding=1)
    h = rms_norm(h, g)
    if scale is not None:
        h = h * (scale[:, :, None] + 1) + shift[:, :, None]
    h = F.silu(h)
    return h if residual is None else h + residual


def linear_attention(x, norm_g, w_qkv, w_out, b_out, out_g, heads, dim_head):
    """PreNorm + LinearAttention without memory key / values (:164-191), without the outer residual."""
    B, C, n = x.shape
    xn = rms_norm(x, norm_g)
    q, k, v = F.conv1d(xn, w_qkv).chunk(3, dim=1)
    q, k, v = (t.reshape(B, heads, dim_head, n) for t in (q, k, v))
    q = q.softmax(dim=-2) * dim_head ** -0.5
    k = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, heads * dim_head, n)
    return rms_norm(F.conv1d(out, w_out, b_out), out_g)


def attention(x, norm_g, w_qkv, w_out, b_out, heads, dim_head):
    """PreNorm + Attention without memory key / values (:193-215), without the outer residual."""
    B, C, n = x.shape
    xn = rms_norm(x, norm_g)
    q, k, v = F.conv1d(xn, w_qkv).chunk(3, dim=1)
    q, k, v = (t.reshape(B, heads, dim_head, n) for t in (q, k, v))
    sim = torch.einsum("bhdi,bhdj->bhij", q * dim_head ** -0.5, k)
    out = torch.einsum("bhij,bhdj->bhid", sim.softmax(dim=-1), v)
    out = out.permute(0, 1, 3, 2).reshape(B, heads * dim_head, n)
    return F.conv1d(out, w_out, b_out)


# ---- Winograd F(4,3) (experimental/wino1d_mfma.hip: measured, not in the library) ---------------------------------------------------------------------------------
# Lavin & Gray (arXiv 1509.09308), points 0, +-1, +-2, inf: Y = A^T [(G g) . (B^T d)], d = 6 positions, Y = 4 outputs
WINO_BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
           [0, 4, 0, -5, 0, 1]]
WINO_G = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
          [0, 0, 1]]
WINO_AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]


def wino1d_pack(w):
    """(Cout, Cin, 3) -> U = G g (Cout, Cin, 6): transformed in float64 and rounded once to the dtype of ``w``, as the host
    packer does (the kernel layout is a permutation of these values)."""
    return torch.einsum("xk,ock->ocx", torch.tensor(WINO_G, dtype=torch.float64), w.double()).to(w.dtype)


def wino1d(x, w, b=None):
    """Conv1d(3, padding 1) over (B, C, L), L % 4 == 0, as F(4,3) in the dtype of ``x``: tiles of 4 outputs read 6 positions
    of their own sequence, zeros outside it."""
    B, C, L = x.shape
    assert L % 4 == 0
    U = wino1d_pack(w)
    d = F.pad(x, (1, 1)).unfold(2, 6, 4)  # (B, C, L / 4, 6)
    V = torch.einsum("xp,bctp->bctx", torch.tensor(WINO_BT, dtype=x.dtype), d)
    M = torch.einsum("bctx,ocx->botx", V, U)
    Y = torch.einsum("mx,botx->botm", torch.tensor(WINO_AT, dtype=x.dtype), M).reshape(B, w.shape[0], L)
    return Y if b is None else Y + b[None, :, None]
