"""Plain torch restatements of the convolution algorithms of the HIP kernels, one per kernel family, in the dtype of their
inputs.  In fp32 they are the rounding FLOOR of the family (tests/test_hip_conv_families.py measures them against an fp64
convolution and allows the kernel 4 x that error); in fp64 they must reproduce ``F.conv2d`` and its autograd to 1e-12
(tests/test_conv_restate.py), which is what makes them restatements.

Every reduction is the longest serial chain a kernel could legitimately form: one rounded product per rounded add, starting
from zero.
  direct     conv_mfma / pw_mfma / init7_mfma: running sum over (channel chunk, tap, channel of the chunk).
  upfold     conv_mfma on a nearest-x2 source: four 2x2 parity convolutions on the source grid, their taps summed in the
             working precision as the host packer does (make_conv), each a `direct` sum.
  wino       winograd_mfma.hip F(2x2,3x3), wino4: wino4_mfma.hip F(4x4,3x3), upwino: upwino_mfma.hip (nearest x2 + 3x3 on
             the source grid): the filter transform G g G^T in double, rounded once (the host packers); input and output
             transforms in the working precision; the running sum over input channels in the transform domain.
  weight gradients: the running sum goes over images and pixels (direct, 1x1, space-to-depth) or over images and 2x2 tiles
             in the Winograd domain (wgrad_mfma.hip mode 3: dW = G^T [sum (A dY A^T) (.) (B^T X B)] G).
The matrices are the ones in the headers of those files."""
import torch
import torch.nn.functional as F

BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
G2 = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]
BT4 = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
       [0, 4, 0, -5, 0, 1]]
G4 = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
      [0, 0, 1]]
AT4 = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]
TU = [[1, -1, 0], [0, 1, 0], [0, -1, 1]]
GU = [[1, 0, 0], [1, 1, 1], [0, 0, 1]]
ATU = [[1, 1, 0], [0, 1, 1]]
AW = [[1, 0], [1, 1], [1, -1], [0, -1]]  # wgrad, Winograd domain: dY tile (2x2) -> 4x4


def _m(rows, dtype):
    return torch.tensor(rows, dtype=dtype)


def _both_sides(mat, t):
    """mat . t . mat^T on the two axes after (batch, channel) of t (b, c, j, k, n)."""
    return torch.einsum("ij,bcjkn,lk->bciln", mat, t, mat)


def filter_transform(w, G):
    """G g G^T in double, rounded to the working precision once (what the host packers store)."""
    Gd = _m(G, torch.float64)
    return torch.einsum("ia,ocab,jb->ocij", Gd, w.double(), Gd).to(w.dtype)


def upsample2(x):
    return x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def direct(x, w, pad=0, stride=1, ck=None):
    """x (B, C, H, W), w (Cout, C, kh, kw): running sum over channel chunks of `ck`, taps, channels of the chunk."""
    B, C, H, W = x.shape
    Cout, _, kh, kw = w.shape
    ck = ck or (16 if C % 16 == 0 else 4)
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    cols = F.unfold(x, (kh, kw), padding=pad, stride=stride).reshape(B, C, kh * kw, Ho * Wo)
    wf = w.reshape(Cout, C, kh * kw)
    acc = torch.zeros(B, Cout, Ho * Wo, dtype=x.dtype)
    for c0 in range(0, C, ck):
        for t in range(kh * kw):
            for c in range(c0, min(c0 + ck, C)):
                acc = acc + wf[None, :, c, t, None] * cols[:, None, c, t, :]
    return acc.reshape(B, Cout, Ho, Wo)


def upfold(x, w, ck=None):
    """nearest x2 then 3x3 / pad 1 as one 2x2 convolution per output parity on the source grid x (B, C, H, W)."""
    B, C, H, W = x.shape
    Cout = w.shape[0]
    taps = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}  # (parity, a) -> summed taps of the 3x3 kernel
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(B, Cout, 2 * H, 2 * W, dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            w2 = torch.zeros(Cout, C, 2, 2, dtype=x.dtype)
            for a in range(2):
                for b in range(2):
                    s = torch.zeros(Cout, C, dtype=x.dtype)
                    for dy in taps[(py, a)]:
                        for dx in taps[(px, b)]:
                            s = s + w[:, :, dy, dx]
                    w2[:, :, a, b] = s
            full = direct(xp, w2, ck=ck)  # (H + 1, W + 1): window rows (i - 1, i) at index i
            out[:, :, py::2, px::2] = full[:, :, py:py + H, px:px + W]
    return out


def _transform_domain_sum(U, V):
    """M[b, o, i, j, n] = sum_c U[o, c, i, j] V[b, c, i, j, n], serially over c."""
    B, C = V.shape[:2]
    M = torch.zeros((B, U.shape[0]) + tuple(V.shape[2:]), dtype=V.dtype)
    for c in range(C):
        M = M + U[None, :, c, :, :, None] * V[:, None, c]
    return M


def _winograd(x, w, BT, G, AT, m):
    B, C, H, W = x.shape
    Cout = w.shape[0]
    a = m + 2
    th, tw = -(-H // m), -(-W // m)
    xp = F.pad(x, (1, tw * m + 1 - W, 1, th * m + 1 - H))
    d = F.unfold(xp, (a, a), stride=m).reshape(B, C, a, a, th * tw)
    V = _both_sides(_m(BT, x.dtype), d)
    M = _transform_domain_sum(filter_transform(w, G), V)
    Y = _both_sides(_m(AT, x.dtype), M)  # (B, Cout, m, m, tiles)
    out = F.fold(Y.reshape(B, Cout * m * m, th * tw), (th * m, tw * m), (m, m), stride=m)
    return out[:, :, :H, :W]


def wino(x, w):
    """F(2x2, 3x3), pad 1."""
    return _winograd(x, w, BT2, G2, AT2, 2)


def wino4(x, w):
    """F(4x4, 3x3), pad 1."""
    return _winograd(x, w, BT4, G4, AT4, 4)


def upwino(x, w):
    """nearest x2 then 3x3 / pad 1, nine products per source pixel of x (B, C, H, W)."""
    B, C, H, W = x.shape
    Cout = w.shape[0]
    d = F.unfold(F.pad(x, (1, 1, 1, 1)), (3, 3)).reshape(B, C, 3, 3, H * W)
    V = _both_sides(_m(TU, x.dtype), d)
    M = _transform_domain_sum(filter_transform(w, GU), V)
    Y = _both_sides(_m(ATU, x.dtype), M)  # (B, Cout, 2, 2, H W)
    return F.fold(Y.reshape(B, Cout * 4, H * W), (2 * H, 2 * W), (2, 2), stride=2)


FORWARD = {"direct": direct, "wino": wino, "wino4": wino4}


def forward(x, w, family, k, up2=False, ck=None):
    """The convolution of a (B, C, H, W) source: `family` in direct / wino / wino4, and upfold / upwino with up2."""
    if up2:
        assert family in ("upfold", "upwino") and k == 3
        return upfold(x, w, ck) if family == "upfold" else upwino(x, w)
    if family == "direct":
        return direct(x, w, pad=k // 2, ck=ck)
    assert k == 3
    return FORWARD[family](x, w)


def bias_grad(dy):
    """Column sums of dy (B, Cout, H, W), serially over images and pixels."""
    B, Cout = dy.shape[:2]
    f = dy.reshape(B, Cout, -1)
    acc = torch.zeros(Cout, dtype=dy.dtype)
    for b in range(B):
        for p in range(f.shape[2]):
            acc = acc + f[b, :, p]
    return acc


def wgrad_direct(x, dy, k):
    """dW (Cout, C, k, k) of a k x k / pad k // 2 convolution of x (B, C, H, W): running sum over images and pixels."""
    B, C, H, W = x.shape
    Cout = dy.shape[1]
    cols = F.unfold(x, (k, k), padding=k // 2)  # (B, C k k, L)
    f = dy.reshape(B, Cout, -1)
    acc = torch.zeros(Cout, C * k * k, dtype=x.dtype)
    for b in range(B):
        for p in range(f.shape[2]):
            acc = acc + f[b, :, p, None] * cols[b, None, :, p]
    return acc.reshape(Cout, C, k, k)


def wgrad_wino(x, dy):
    """dW of the 3x3 / pad 1 convolution in the Winograd domain F(3x3, 2x2); even image sizes."""
    B, C, H, W = x.shape
    Cout = dy.shape[1]
    assert H % 2 == 0 and W % 2 == 0
    n = (H // 2) * (W // 2)
    Xt = _both_sides(_m(BT2, x.dtype), F.unfold(F.pad(x, (1, 1, 1, 1)), (4, 4), stride=2).reshape(B, C, 4, 4, n))
    Yt = _both_sides(_m(AW, x.dtype), F.unfold(dy, (2, 2), stride=2).reshape(B, Cout, 2, 2, n))
    acc = torch.zeros(Cout, C, 4, 4, dtype=x.dtype)
    for b in range(B):
        for t in range(n):
            acc = acc + Yt[b, :, None, :, :, t] * Xt[b, None, :, :, :, t]
    Gm = _m(G2, x.dtype)
    return torch.einsum("ia,ocij,jb->ocab", Gm, acc, Gm)


class Conv(torch.autograd.Function):
    """y = conv(x, w) + b through the restatements: ``spec`` names the family of the forward convolution, of the
    input-gradient convolution of each source (the layer of rotated, transposed weights that build_conv_bwd packs) and the
    mode of the weight gradient.  spec: k, up2, c0 (channels of the first source), fwd, dgrad (one family per source),
    wgrad ("direct" or "wino"), ck (optional chunk of the direct forward)."""

    @staticmethod
    def forward(ctx, x, w, b, spec):
        ctx.save_for_backward(x, w)
        ctx.spec = spec
        y = forward(x, w, spec["fwd"], spec["k"], spec.get("up2", False), spec.get("ck"))
        return y if b is None else y + b[None, :, None, None]

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        spec = ctx.spec
        k, up2 = spec["k"], spec.get("up2", False)
        xin = upsample2(x) if up2 else x
        dw = wgrad_wino(xin, dy) if spec["wgrad"] == "wino" else wgrad_direct(xin, dy, k)
        db = bias_grad(dy) if ctx.needs_input_grad[2] else None
        wr = w.flip(2, 3).transpose(0, 1)  # (C, Cout, k, k): the input gradient is a convolution of dy with these
        c0 = spec.get("c0", x.shape[1])
        halves = [(0, c0)] + ([(c0, x.shape[1])] if c0 < x.shape[1] else [])
        dx = torch.cat([forward(dy, wr[lo:hi].contiguous(), fam, k) for (lo, hi), fam in zip(halves, spec["dgrad"])], 1)
        if up2:  # the gradient at the upsampled size, then the 2x2 sums
            B, C, H2, W2 = dx.shape
            dx = dx.reshape(B, C, H2 // 2, 2, W2 // 2, 2).sum((3, 5))
        return dx, dw, db, None


def conv(x, w, b, spec):
    return Conv.apply(x, w, b, spec)


def space_to_depth(x):
    """'b c (h 2) (w 2) -> b (c 2 2) h w' of Downsample."""
    b, c, hh, ww = x.shape
    return x.reshape(b, c, hh // 2, 2, ww // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(b, c * 4, hh // 2, ww // 2)
