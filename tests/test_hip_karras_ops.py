"""GPU parity of KarrasUnet's own kernels and blocks, one at a time through the C ABI (dm_op_kunet_*), against the fp64 torch
restatement of the folded network (tests/karras_oracle.py) on the same fp32 inputs.

Limits, as in tests/test_hip_seq1d_ops.py.  Per tensor two metrics: whole-tensor rel-L2 and max|got - ref| / rms(ref).  The
floor of each is the same operator restated in fp32 torch (the oracle run in fp32), measured against the fp64 reference inside
the test; the kernel may be 4 x the floor off, and rel-L2 must also stay under 2e-5.  Outputs are poisoned with NaN before the
call.  Every case prints ``case: kernel error, floor, limit`` for both metrics before it asserts (run with -s)."""
import ctypes as C
from math import sqrt

import pytest
import torch
import torch.nn.functional as F

import karras_oracle as ko
from diffusion_models_amd import _lib
from diffusion_models_amd.spec import MP_SILU_GAIN, KarrasBlock, KarrasUnetConfig

pytestmark = pytest.mark.gpu
TOL_FWD = 2e-5
FACTOR = 4.0
DEV = "cuda:0"
T_RES, T_ATTN, T_CAT = 0.3, 0.3, 0.5


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


_KEEP = []  # device copies made by dev() stay alive until the test ends: their addresses are passed as plain integers


def dev(t):
    if t is None:
        return None
    _KEEP.append(t.to(DEV).contiguous())
    return _KEEP[-1]


@pytest.fixture(autouse=True)
def keep_device_inputs():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def metrics(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d = got - ref
    return (float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.pow(2).mean().sqrt().clamp_min(1e-300)))


def check(label, got, ref64, floor32):
    assert got.shape == ref64.shape, (label, got.shape, ref64.shape)
    e, f = metrics(got, ref64), metrics(floor32, ref64)
    lim = (min(FACTOR * f[0], TOL_FWD), FACTOR * f[1])
    print(f"karras_ops {label}: rel-L2 kernel {e[0]:.3g} floor {f[0]:.3g} limit {lim[0]:.3g} | max/rms kernel {e[1]:.3g} "
          f"floor {f[1]:.3g} limit {lim[1]:.3g}")
    assert torch.isfinite(got).all(), (label, "not finite", int((~torch.isfinite(got)).sum()))
    assert e[0] <= lim[0] and e[1] <= lim[1], (label, e, lim)


def both(fn, *tensors):
    """fn on the fp64 and on the fp32 copies of the tensors: (reference, floor)."""
    return fn(*[None if t is None else t.double() for t in tensors]), fn(*[None if t is None else t.float() for t in tensors])


# ---- kunet_pixelnorm --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 48, 192, 768])
def test_pixelnorm(C):
    lib = _lib.load()
    x = seeded((2, C, 5, 7), 100 + C)
    x[0, :, 0, 0] = 0.0                                  # an all-zero pixel
    x[1, :, 4, 6] = 0.0
    x[1, 3, 4, 6] = 1e-6                                 # a pixel of norm 1e-6: both take the eps branch
    rows = nhwc(x)
    res, act = nans(*rows.shape), nans(*rows.shape)
    _lib.check(lib.dm_op_kunet_pixelnorm(_lib.ptr(dev(rows)), _lib.ptr(res), _lib.ptr(act), 2 * 5 * 7, C, 0.39, stream()))
    (r64, a64), (r32, a32) = both(lambda t: ko.pixelnorm_op(t, 0.39), x)
    check(f"pixelnorm C={C} res", nchw(res.cpu()), r64, r32)
    check(f"pixelnorm C={C} act", nchw(act.cpu()), a64, a32)
    # the eps branch is exactly what max(||x||, 1e-4) gives: x / 1e-4 * sqrt(C) in fp32, whatever the order of the sum
    res_c, act_c = nchw(res.cpu()), nchw(act.cpu())
    assert torch.equal(res_c[0, :, 0, 0], torch.zeros(C)) and torch.equal(act_c[0, :, 0, 0], torch.zeros(C))
    want = torch.tensor(1e-6) / torch.tensor(1e-4) * torch.tensor(sqrt(C), dtype=torch.float32)
    assert float(res_c[1, 3, 4, 6]) == float(want * torch.tensor(0.39)) and float(res_c[1, 0, 4, 6]) == 0.0
    assert abs(float(act_c[1, 3, 4, 6]) - float(F.silu(want))) <= 2e-7 * float(F.silu(want))
    # one output at a time
    only = nans(*rows.shape)
    _lib.check(lib.dm_op_kunet_pixelnorm(_lib.ptr(dev(rows)), None, _lib.ptr(only), 2 * 5 * 7, C, 1.0, stream()))
    assert torch.equal(only, act)


# ---- kunet_avgpool2 ----------------------------------------------------------------------------------------------------------------
def test_avgpool2():
    lib = _lib.load()
    x = seeded((2, 32, 6, 4), 111)  # non-square on purpose
    y = nans(2, 3, 2, 32)
    _lib.check(lib.dm_op_kunet_avgpool2(_lib.ptr(dev(nhwc(x))), _lib.ptr(y), 2, 6, 4, 32, stream()))
    ref, floor = both(ko.avgpool2, x)
    check("avgpool2 2x32x6x4", nchw(y.cpu()), ref, floor)
    assert lib.dm_op_kunet_avgpool2(_lib.ptr(dev(nhwc(x))), _lib.ptr(y), 2, 5, 4, 32, stream()) != 0  # odd H is refused


# ---- kunet_bilinear_up2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W", [(2, 32, 1, 1), (2, 32, 3, 5), (1, 48, 3, 5)])
def test_bilinear_up2(B, C, H, W):
    lib = _lib.load()
    x = seeded((B, C, H, W), 120 + C + H)
    outs = [nans(B, 2 * H, 2 * W, C) for _ in range(3)]
    _lib.check(lib.dm_op_kunet_bilinear_up2(_lib.ptr(dev(nhwc(x))), *[_lib.ptr(o) for o in outs], B, H, W, C, 0.39, stream()))
    ref, floor = both(lambda t: ko.up2_op(t, 0.39), x)
    for name, o, r, f in zip(("up", "act", "res"), outs, ref, floor):
        check(f"bilinear_up2 {B}x{C}x{H}x{W} {name}", nchw(o.cpu()), r, f)
    # the identity-res_conv form: no x_up
    act, res = nans(B, 2 * H, 2 * W, C), nans(B, 2 * H, 2 * W, C)
    _lib.check(lib.dm_op_kunet_bilinear_up2(_lib.ptr(dev(nhwc(x))), None, _lib.ptr(act), _lib.ptr(res), B, H, W, C, 0.39, stream()))
    assert torch.equal(act, outs[1]) and torch.equal(res, outs[2])


# ---- kunet_act ---------------------------------------------------------------------------------------------------------------------
def test_act_two_sources():
    lib = _lib.load()
    a, b = seeded((2, 64, 3, 5), 131), seeded((2, 32, 3, 5), 132)
    ca, cb = ko.mp_cat_consts(T_CAT, 64, 32)
    assert abs(ca - cb) > 0.1
    act, copy = nans(2, 3, 5, 96), nans(2, 3, 5, 64)
    _lib.check(lib.dm_op_kunet_act(_lib.ptr(dev(nhwc(a))), 64, ca, _lib.ptr(dev(nhwc(b))), 32, cb, _lib.ptr(act), _lib.ptr(copy),
                                   0.39, 2 * 3 * 5, stream()))
    ref, floor = both(lambda p, q: ko.act_op(p, ca, q, cb, copy_scale=0.39), a, b)
    check("act 64+32 act", nchw(act.cpu()), ref[0], floor[0])
    check("act 64+32 copy", nchw(copy.cpu()), ref[1], floor[1])


def test_act_one_source_with_and_without_the_activation():
    lib = _lib.load()
    a = seeded((2, 48, 4, 4), 133)
    act, copy = nans(2, 4, 4, 48), nans(2, 4, 4, 48)
    _lib.check(lib.dm_op_kunet_act(_lib.ptr(dev(nhwc(a))), 48, 1.0, None, 0, 1.0, _lib.ptr(act), _lib.ptr(copy), 0.39, 32, stream()))
    ref, floor = both(lambda p: ko.act_op(p, 1.0, copy_scale=0.39), a)
    check("act 48 act", nchw(act.cpu()), ref[0], floor[0])
    check("act 48 copy", nchw(copy.cpu()), ref[1], floor[1])
    only = nans(2, 4, 4, 48)  # the scaled copy in front of an attention layer
    _lib.check(lib.dm_op_kunet_act(_lib.ptr(dev(nhwc(a))), 48, 1.0, None, 0, 1.0, None, _lib.ptr(only), 0.39, 32, stream()))
    assert torch.equal(only, copy)


# ---- kunet_qkv_norm + the attention core --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,heads,dh", [(16, 2, 32), (64, 3, 64), (256, 2, 64)])
def test_qkv_norm_and_attention_core(n, heads, dh):
    lib = _lib.load()
    side = int(sqrt(n))
    qkv = seeded((2, 3 * heads * dh, side, side), 140 + n)
    mem = seeded((2, heads, 4, dh), 141 + n)
    out = nans(2, n, heads * dh)
    _lib.check(lib.dm_op_kunet_attention(_lib.ptr(dev(nhwc(qkv))), _lib.ptr(dev(mem)), _lib.ptr(out), 2, n, heads, dh, stream()))

    def op(q, m):
        return ko.attention_core(ko.qkv_norm_op(q, heads, dh), ko.pixel_norm(m, -1), heads, dh)

    ref, floor = both(op, qkv, mem)
    check(f"attention n={n} heads={heads} dh={dh}", nchw(out.cpu().reshape(2, side, side, heads * dh)), ref, floor)
    # the memory rows matter
    no_mem = op(qkv.double(), mem.double() * 0 + 1e-9)
    assert metrics(no_mem, ref)[0] > 1e-3


# ---- the head ----------------------------------------------------------------------------------------------------------------------
def head_case(B, classes, label_kind, seed):
    dim, fourier_dim, douts = 32, 16, (32, 64, 48)
    E = 4 * dim
    sd = {"to_time_emb.0.weights": seeded((fourier_dim // 2,), seed), "to_time_emb.1.weight": seeded((E, fourier_dim), seed + 1)}
    if classes:
        sd["to_class_emb.weight"] = seeded((E, classes), seed + 2)
    to_emb = [seeded((d, E), seed + 3 + i) for i, d in enumerate(douts)]
    gains = [0.8, 0.55, 0.95]
    time = torch.tensor([-1.55, 0.0, 1.1])[:B]
    labels = None
    if classes:
        idx = torch.tensor([4, 0, 2])[:B]
        labels = {"int": idx, "onehot": F.one_hot(idx, classes).float(),
                  "soft": torch.softmax(seeded((B, classes), seed + 9), dim=-1)}[label_kind]
    return dict(dim=dim, fourier_dim=fourier_dim, douts=douts, E=E, sd=sd, to_emb=to_emb, gains=gains, time=time, labels=labels)


def head_oracle(c, dtype, classes):
    P = {"fourier_w": c["sd"]["to_time_emb.0.weights"].double()}
    wt = ko.normalize_weight(c["sd"]["to_time_emb.1.weight"].double())
    rows = None
    if classes:
        a, r = ko.mp_add_consts(0.5)
        wt = torch.cat((wt * a, ko.normalize_weight(c["sd"]["to_class_emb.weight"].double()) * r), dim=1)
        rows = ko.class_rows(c["labels"], classes, dtype)
    ss = []
    for w, g in zip(c["to_emb"], c["gains"]):
        wn = ko.normalize_weight(w.double()) * (g * MP_SILU_GAIN)
        ss += [wn, torch.zeros_like(wn)]
    P["emb_w"], P["ss_w"] = wt, torch.cat(ss, dim=0)
    P = {k: v.to(dtype) for k, v in P.items()}
    return ko.head_op(P, c["time"].to(dtype), rows)


@pytest.mark.parametrize("B,classes,label_kind", [(1, 0, None), (3, 0, None), (1, 5, "int"), (3, 5, "int"), (3, 5, "onehot"),
                                                  (3, 5, "soft")])
def test_head(B, classes, label_kind):
    lib = _lib.load()
    c = head_case(B, classes, label_kind, 150 + B + classes)
    rows = dev(ko.class_rows(c["labels"], classes, torch.float32)) if classes else None
    total = 2 * sum(c["douts"])
    out = nans(B, total)
    douts = (C.c_int32 * 3)(*c["douts"])
    gains = (C.c_float * 3)(*c["gains"])
    _lib.check(lib.dm_op_kunet_head(_lib.ptr(dev(c["time"])), _lib.ptr(rows), _lib.ptr(dev(c["sd"]["to_time_emb.0.weights"])),
                                    _lib.ptr(dev(c["sd"]["to_time_emb.1.weight"])),
                                    _lib.ptr(dev(c["sd"]["to_class_emb.weight"])) if classes else None,
                                    _lib.ptr(dev(torch.cat(c["to_emb"], dim=0))), douts, gains, 3, c["fourier_dim"], c["E"], classes,
                                    0.5, _lib.ptr(out), B, stream()))
    ref, floor = head_oracle(c, torch.float64, classes), head_oracle(c, torch.float32, classes)
    got = out.cpu()
    off = 0
    for d in c["douts"]:  # the shift half of every block is exactly zero
        assert torch.equal(got[:, off + d:off + 2 * d], torch.zeros(B, d))
        off += 2 * d
    check(f"head B={B} classes={classes} {label_kind}", got, ref, floor)
    if label_kind == "onehot":  # integer and one-hot labels are one path
        ci = head_case(B, classes, "int", 150 + B + classes)
        assert torch.equal(ko.class_rows(ci["labels"], classes, torch.float32), rows.cpu())


# ---- input and output block ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin", [3, 8])
def test_input_block(Cin):
    lib = _lib.load()
    dim = 32
    x, w = seeded((2, Cin, 8, 8), 160 + Cin), seeded((dim, Cin + 1, 3, 3), 161 + Cin)
    out = nans(2, dim, 8, 8)
    _lib.check(lib.dm_op_kunet_input_block(_lib.ptr(dev(x)), _lib.ptr(dev(w)), _lib.ptr(out), 2, Cin, 8, 8, dim, stream()))

    def op(xx, ww):
        return ko.input_block({"in_w": ko.normalize_weight(ww.double(), fan_in=Cin * 9).to(ww.dtype)}, xx)

    ref, floor = both(op, x, w)
    got = out.cpu()
    check(f"input_block C={Cin}", got, ref, floor)
    border = torch.ones(8, 8, dtype=torch.bool)
    border[1:-1, 1:-1] = False  # the zero padding reaches the ones channel: what tells it from a bias
    check(f"input_block C={Cin} border", got[..., border], ref[..., border], floor[..., border])
    wn = ko.normalize_weight(w.double(), fan_in=Cin * 9)
    as_bias = F.conv2d(x.double(), wn[:, 1:], padding=1) + wn[:, 0].sum(dim=(1, 2))[None, :, None, None]
    assert metrics(as_bias[..., border], ref[..., border])[0] > 1e-2 and metrics(as_bias[..., ~border], ref[..., ~border])[0] < 1e-12


def test_output_block():
    lib = _lib.load()
    dim, ch, gain = 32, 3, 0.7
    x, w = seeded((2, dim, 8, 8), 170), seeded((ch, dim, 3, 3), 171)
    out = nans(2, ch, 8, 8)
    _lib.check(lib.dm_op_kunet_output_block(_lib.ptr(dev(x)), _lib.ptr(dev(w)), gain, _lib.ptr(out), 2, dim, 8, 8, ch, stream()))
    ref, floor = both(lambda xx, ww: ko.conv(xx, (ko.normalize_weight(ww.double()) * gain).to(ww.dtype)), x, w)
    check("output_block", out.cpu(), ref, floor)
    zero = nans(2, ch, 8, 8)
    _lib.check(lib.dm_op_kunet_output_block(_lib.ptr(dev(x)), _lib.ptr(dev(w)), 0.0, _lib.ptr(zero), 2, dim, 8, 8, ch, stream()))
    assert torch.equal(zero.cpu(), torch.zeros(2, ch, 8, 8))  # the gain is in the weights


# ---- one Encoder and one Decoder of each form ---------------------------------------------------------------------------------------
BLOCKS = {
    # name: (KarrasBlock, dh)
    "encoder": (KarrasBlock("b", False, 32, 32), 32),
    "encoder_down": (KarrasBlock("b", False, 32, 64, down=True), 32),
    "encoder_attn": (KarrasBlock("b", False, 64, 64, attn=True), 32),
    "decoder_mid": (KarrasBlock("b", True, 64, 64), 32),
    "decoder_up_identity": (KarrasBlock("b", True, 64, 64, up=True), 32),
    "decoder_up_conv": (KarrasBlock("b", True, 64, 32, up=True), 32),
    "decoder_skip": (KarrasBlock("b", True, 64, 32, skip=True), 32),
    "decoder_skip_attn": (KarrasBlock("b", True, 128, 64, attn=True, skip=True), 64),
}


@pytest.mark.parametrize("name", list(BLOCKS))
def test_block(name):
    lib = _lib.load()
    b, dh = BLOCKS[name]
    B, H = 2, 8
    cfg = KarrasUnetConfig(image_size=H, attn_dim_head=dh, mp_cat_t=T_CAT, attn_res_mp_add_t=T_ATTN, resnet_mp_add_t=T_RES)
    seed = 200 + 10 * list(BLOCKS).index(name)
    xc = b.din - b.dout if b.skip else b.din
    x = seeded((B, xc, H, H), seed)
    skip = seeded((B, b.dout, H, H), seed + 1) if b.skip else None
    emb_scale = seeded((B, b.dout), seed + 2, 0.5)
    sd = {"b.block1.1.weight": seeded((b.dout, b.dout if b.down else b.din, 3, 3), seed + 3),
          "b.block2.2.weight": seeded((b.dout, b.dout, 3, 3), seed + 4)}
    if b.down:
        sd["b.downsample_conv.weight"] = seeded((b.dout, b.din, 1, 1), seed + 5)
    if b.res_conv:
        sd["b.res_conv.weight"] = seeded((b.dout, b.din, 1, 1), seed + 6)
    heads = cfg.heads(b.dout)
    if b.attn:
        sd["b.attn.mem_kv"] = seeded((2, heads, 4, dh), seed + 7)
        sd["b.attn.to_qkv.weight"] = seeded((3 * heads * dh, b.dout, 1, 1), seed + 8)
        sd["b.attn.to_out.weight"] = seeded((b.dout, heads * dh, 1, 1), seed + 9)
    Ho = H // 2 if b.down else 2 * H if b.up else H
    out = nans(B, b.dout, Ho, Ho)
    keep = {k: dev(v) for k, v in sd.items()}
    xd, sk, es = dev(x), dev(skip), dev(emb_scale)
    a = _lib.KunetBlockOp()
    a.decoder, a.down, a.up, a.skip, a.attn = int(b.decoder), int(b.down), int(b.up), int(b.skip), int(b.attn)
    a.din, a.dout, a.skip_channels, a.dh = b.din, b.dout, b.dout if b.skip else 0, dh
    a.mp_cat_t, a.attn_res_mp_add_t, a.resnet_mp_add_t = T_CAT, T_ATTN, T_RES
    a.x, a.skip_x, a.emb_scale = _lib.ptr(xd), _lib.ptr(sk), _lib.ptr(es)
    a.down_w, a.w1, a.w2 = _lib.ptr(keep.get("b.downsample_conv.weight")), _lib.ptr(keep["b.block1.1.weight"]), _lib.ptr(keep["b.block2.2.weight"])
    a.res_w, a.mem_kv = _lib.ptr(keep.get("b.res_conv.weight")), _lib.ptr(keep.get("b.attn.mem_kv"))
    a.qkv_w, a.out_w = _lib.ptr(keep.get("b.attn.to_qkv.weight")), _lib.ptr(keep.get("b.attn.to_out.weight"))
    a.out, a.B, a.H, a.W = _lib.ptr(out), B, H, H
    _lib.check(lib.dm_op_kunet_block(C.byref(a), stream()))

    def op(dtype):
        K = ko.fold_block({k: v.double() for k, v in sd.items()}, b, cfg, 0)
        K = {k: v.to(dtype) if torch.is_tensor(v) else v for k, v in K.items()}
        ss = torch.cat((emb_scale, torch.zeros_like(emb_scale)), dim=1).to(dtype)
        if b.decoder:
            return ko.decoder(K, x.to(dtype), None if skip is None else skip.to(dtype), ss, cfg)
        return ko.encoder(K, x.to(dtype), ss, cfg)

    check(f"block {name}", out.cpu(), op(torch.float64), op(torch.float32))
