"""KarrasUnet on the host: spec, the folded torch restatement against the reference's fp64 outputs, every folding identity,
the two resampling identities, the constructor surface, refusals, ABI.  No GPU.  Goldens: tests/golden/karras.pt
(tests/golden/make_golden_karras.py, from the reference)."""
import ctypes
import inspect
import os
import re
from math import sqrt

import pytest
import torch
import torch.nn.functional as F

import diffusion_models_amd as dm
import karras_oracle as ko
from diffusion_models_amd import _lib, karras
from diffusion_models_amd.spec import MP_SILU_GAIN, KarrasUnetConfig, karras_blocks, karras_unet_param_spec

from conftest import ROOT, load_golden, rel_l2

ORACLE_TOL = 1e-10
FOLD_TOL = 1e-12
TINY = dict(image_size=16, dim=32, dim_max=64, channels=3, num_downsamples=2, num_blocks_per_stage=1, attn_res=(8, 4),
            attn_dim_head=32, num_classes=5)


@pytest.fixture(scope="module")
def golden():
    return load_golden("karras.pt")


def seeded(shape, seed, dtype=torch.float64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def maxdiff(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ---- spec -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["a", "b"])
def test_param_spec_equals_reference_state_dict(golden, key):
    g = golden["keys"][key]
    spec = karras_unet_param_spec(KarrasUnetConfig(**g["unet_kw"]))
    assert [(k, tuple(s)) for k, s in spec] == [(k, tuple(s)) for k, s in g["entries"]]


def test_param_spec_structure():
    cfg = KarrasUnetConfig(**TINY)
    spec = karras_unet_param_spec(cfg)
    names = dict(spec)
    assert len(spec) == 108 and sum(torch.Size(s).numel() for _, s in spec) == 1_401_976
    assert spec[0] == ("input_block.weight", (32, 4, 3, 3)) and names["output_block.1.gain"] == ()
    assert names["to_time_emb.0.weights"] == (8,) and names["to_class_emb.weight"] == (128, 5)
    assert names["downs.1.downsample_conv.weight"] == (64, 32, 1, 1) and names["downs.1.attn.mem_kv"] == (2, 2, 4, 32)
    order = [k for k, _ in spec]
    assert order.index("ups.0.to_emb.0.weight") < order.index("mids.0.to_emb.0.weight")  # downs, ups, then the mids
    b = karras_blocks(cfg)
    assert [len(b[k]) for k in ("downs", "mids", "ups")] == [5, 2, 8]
    ups = b["ups"]
    assert [u.up for u in ups] == [False, False, True, False, False, True, False, False]
    assert all(u.skip != u.up for u in ups) and not any(m.skip or m.up for m in b["mids"])
    # dim_max caps both sides of the last upsampling decoder: its res_conv is the identity
    assert not ups[2].res_conv and ups[5].res_conv and cfg.heads(64) == 2 and cfg.heads(192) == 6
    wide = KarrasUnetConfig(image_size=64)
    assert wide.heads(768) == 12 and wide.emb_dim == 768 and wide.downsample_factor == 8 and wide.input_channels == 4


def test_synth_gains_are_away_from_zero():
    sd = dm.synth_state_dict(karras_unet_param_spec(KarrasUnetConfig(**TINY)), salt=3)
    gains = [v for k, v in sd.items() if k.endswith(".gain")]
    assert len(gains) == 16 and all(g.shape == () and 0.5 <= float(g) < 1.0 for g in gains)


# ---- the folded restatement against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["a_plain", "a_soft", "b_plain", "b_self_cond", "c_plain"])
def test_oracle_equals_reference_fp64(golden, key):
    f = golden["forward"][key]
    cfg = KarrasUnetConfig(**f["unet_kw"])
    sd = dm.synth_state_dict(karras_unet_param_spec(cfg), salt=f["salt"])
    y = ko.forward(ko.fold(sd, cfg, torch.float64), f["x"], f["t"], f["self_cond"], f["labels"])
    err = rel_l2(y, f["y64"])
    print("karras oracle", key, "vs reference fp64", err, "| reference fp32-vs-fp64", f["ref_err"])
    assert err < ORACLE_TOL and f["ref_err"] < 1e-5
    y32 = ko.forward(ko.fold(sd, cfg, torch.float32), f["x"], f["t"], f["self_cond"], f["labels"])
    assert y32.dtype == torch.float32 and rel_l2(y32, f["y64"]) < 1e-5


def test_golden_margins(golden):
    m = golden["margins"]
    for k in ("a_time", "a_labels", "b_time", "b_self_cond", "c_time", "a_ones_channel"):
        assert m[k] >= 1e-3, k
    for f in golden["forward"].values():
        assert torch.isfinite(f["y"]).all() and float(f["y"].pow(2).mean().sqrt()) > 0.1 and f["ref_err"] < 1e-5
    for L in golden["loops"].values():
        assert torch.isfinite(L["sample"]).all() and float(L["sample"].pow(2).mean().sqrt()) > 0.1 and L["ref_err"] < 1e-4
    # the oracle tells the ones channel from a bias too
    f = golden["forward"]["a_plain"]
    assert rel_l2(m["a_ones_channel_output"], f["y"]) == pytest.approx(m["a_ones_channel"])


# ---- folding identities, fp64 --------------------------------------------------------------------------------------------------------
def ref_normalize_weight(w, eps=1e-4):
    """karras_unet.py:91-95."""
    flat = w.reshape(w.shape[0], -1)
    return (F.normalize(flat, dim=-1, eps=eps) * sqrt(flat.numel() / flat.shape[0])).reshape(w.shape)


def ref_mp_add(x, res, t):
    return (x * (1. - t) + res * t) / sqrt((1 - t) ** 2 + t ** 2)


def ref_mp_cat(a, b, t):
    na, nb = a.shape[1], b.shape[1]
    c = sqrt((na + nb) / ((1. - t) ** 2 + t ** 2))
    return c * torch.cat((a * (1. - t) / sqrt(na), b * t / sqrt(nb)), dim=1)


def ref_mp_silu(x):
    return F.silu(x) / 0.596


def test_weight_normalisation_with_the_fan_in_quirk():
    w = seeded((8, 5, 3, 3), 1)
    w[3] *= 1e-7  # a row under eps keeps its direction and the eps denominator
    got = ko.normalize_weight(w)
    assert maxdiff(got, ref_normalize_weight(w) / sqrt(5 * 9)) < FOLD_TOL
    assert maxdiff(got[3], w[3] / 1e-4) < FOLD_TOL and float(got[3].norm()) < 1e-2 and abs(float(got[0].norm()) - 1.0) < 1e-12
    # input_block: the row counts the ones channel (5 * 9 elements), fan_in does not (4 * 9)
    quirk = ko.normalize_weight(w, fan_in=4 * 9)
    assert maxdiff(quirk, ref_normalize_weight(w) / sqrt(4 * 9)) < FOLD_TOL
    assert abs(float(quirk[0].norm()) - sqrt(5 / 4)) < 1e-12
    lin = seeded((6, 16), 2)
    assert maxdiff(ko.normalize_weight(lin), ref_normalize_weight(lin) / sqrt(16)) < FOLD_TOL


@pytest.mark.parametrize("t", [0.3, 0.5, 0.0, 0.9])
def test_mp_add_folds_into_the_producer_and_the_residual(t):
    x, w, res = seeded((2, 8, 5, 5), 3), seeded((8, 8, 3, 3), 4), seeded((2, 8, 5, 5), 5)
    a, b = ko.mp_add_consts(t)
    want = ref_mp_add(F.conv2d(x, w, padding=1), res, t)
    assert maxdiff(F.conv2d(x, w * a, padding=1) + res * b, want) < FOLD_TOL
    assert abs(a * a + b * b - 1.0) < 1e-15


@pytest.mark.parametrize("na,nb,t", [(8, 8, 0.5), (8, 4, 0.3)])
def test_mp_cat_folds_into_res_conv_and_the_activation_pass(na, nb, t):
    x, skip, w = seeded((2, na, 4, 4), 6), seeded((2, nb, 4, 4), 7), seeded((6, na + nb, 1, 1), 8)
    ca, cb = ko.mp_cat_consts(t, na, nb)
    cat = ref_mp_cat(x, skip, t)
    wf = torch.cat((w[:, :na] * ca, w[:, na:] * cb), dim=1)
    assert maxdiff(F.conv2d(torch.cat((x, skip), dim=1), wf), F.conv2d(cat, w)) < FOLD_TOL
    act, copy = ko.act_op(x, ca, skip, cb)
    assert copy is None and maxdiff(act, F.silu(cat)) < FOLD_TOL


def test_gain_and_mp_silu_fold_into_the_consumer():
    x, w, gain = seeded((2, 8, 5, 5), 9), seeded((4, 8, 3, 3), 10), 0.73
    assert maxdiff(F.conv2d(F.silu(x), w * MP_SILU_GAIN, padding=1), F.conv2d(ref_mp_silu(x), w, padding=1)) < FOLD_TOL
    assert maxdiff(F.conv2d(x, w * gain, padding=1), F.conv2d(x, w, padding=1) * gain) < FOLD_TOL
    emb, lin = seeded((3, 16), 11), seeded((8, 16), 12)
    assert maxdiff(F.silu(emb) @ (lin * (gain * MP_SILU_GAIN)).t(), (ref_mp_silu(emb) @ lin.t()) * gain) < FOLD_TOL
    assert MP_SILU_GAIN == 1.0 / 0.596


def test_head_layout_and_class_rows():
    cfg = KarrasUnetConfig(**TINY)
    sd = dm.synth_state_dict(karras_unet_param_spec(cfg), salt=5)
    P = ko.fold(sd, cfg)
    blocks = [K for g in ("downs", "mids", "ups") for K in P[g]]
    assert P["ss_w"].shape == (2 * sum(K["block"].dout for K in blocks), cfg.emb_dim)
    assert [K["ss_off"] for K in blocks[:3]] == [0, 64, 192]
    labels = torch.tensor([1, 4, 0])
    rows = ko.class_rows(labels, 5, torch.float64)
    ss = ko.head_op(P, torch.tensor([0.3, -1.2, 2.0], dtype=torch.float64), rows)
    for K in blocks:  # dout scales, then dout zeros: the shift of EPI_SCALE_SHIFT
        o, d = K["ss_off"], K["block"].dout
        assert float(ss[:, o:o + d].abs().min()) > 0 and float(ss[:, o + d:o + 2 * d].abs().max()) == 0
    assert torch.equal(rows, F.one_hot(labels, 5).double() * sqrt(5))
    soft = torch.softmax(seeded((3, 5), 13), dim=-1)
    assert torch.equal(ko.class_rows(soft, 5, torch.float64), soft * sqrt(5))
    # mem_kv is normalised at pack time
    K = next(K for K in blocks if K["block"].attn)
    assert maxdiff(K["mem_kv"].norm(dim=-1), torch.full((2, 2, 4), sqrt(32), dtype=torch.float64)) < 1e-12


# ---- resampling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 6, 4), (1, 2, 2, 2), (1, 1, 8, 16)])
def test_bilinear_downsample_is_the_2x2_mean(shape):
    x = seeded(shape, 14)
    want = F.interpolate(x, (shape[2] // 2, shape[3] // 2), mode="bilinear")
    assert float((ko.avgpool2(x) - want).abs().max()) <= 1e-15


@pytest.mark.parametrize("shape", [(2, 3, 3, 5), (1, 2, 1, 1), (1, 1, 1, 4), (1, 2, 8, 8)])
def test_bilinear_upsample_is_the_quarter_three_quarter_filter(shape):
    x = seeded(shape, 15)
    want = F.interpolate(x, (2 * shape[2], 2 * shape[3]), mode="bilinear")
    assert float((ko.bilinear_up2(x) - want).abs().max()) <= 4e-16 * max(1.0, float(x.abs().max()))
    u, act, res = ko.up2_op(x, 0.4)
    assert torch.equal(u, ko.bilinear_up2(x)) and torch.equal(act, F.silu(u)) and torch.equal(res, u * 0.4)


# ---- surface and refusals (no handle is needed to be refused) ----------------------------------------------------------------------
def test_constructor_and_forward_signatures(golden):
    s = golden["surface"]
    sig = inspect.signature(dm.KarrasUnet.__init__)
    ours = [(p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name)
            for p in sig.parameters.values() if p.name != "self"]
    want = [tuple(v) for v in s["__init__"]]
    assert ours[:len(want)] == want and ours[len(want):] == [("device", "cuda:0", "KEYWORD_ONLY")]
    fwd = [(p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name)
           for p in inspect.signature(dm.KarrasUnet.forward).parameters.values() if p.name != "self"]
    assert fwd == [tuple(v) for v in s["forward"]]
    assert {"KarrasUnet", "KarrasUnetConfig", "karras_unet_param_spec"} <= set(dm.__all__)


def bare(**kw):
    u = dm.KarrasUnet.__new__(dm.KarrasUnet)
    u._handle = None
    u._loaded = True
    u.cfg = KarrasUnetConfig(**{**TINY, **kw})
    return u


def test_refusals():
    u = bare()
    with pytest.raises(NotImplementedError, match="follow-up"):
        u.train()
    assert u.train(False) is u and u.eval() is u
    for name in ("grads", "optimizer_step", "sync", "ema_update"):
        with pytest.raises(NotImplementedError):
            getattr(u, name)()
    with pytest.raises(NotImplementedError, match="32 and 64"):
        dm.KarrasUnet(image_size=16, attn_dim_head=48)
    x, t = torch.zeros(2, 3, 16, 16), torch.zeros(2)
    with pytest.raises(AssertionError, match="class_labels"):  # a class-conditional network without labels
        u.forward(x, t)
    with pytest.raises(AssertionError, match="class_labels"):  # and the reverse
        bare(num_classes=None).forward(x, t, class_labels=torch.tensor([0, 1]))
    with pytest.raises(AssertionError, match="the network takes"):  # a wrong image size
        u.forward(torch.zeros(2, 3, 8, 8), t, class_labels=torch.tensor([0, 1]))
    with pytest.raises(AssertionError, match="the network takes"):
        u.forward(torch.zeros(2, 4, 16, 16), t, class_labels=torch.tensor([0, 1]))
    with pytest.raises(AssertionError, match="self_condition"):
        u.forward(x, t, self_cond=x, class_labels=torch.tensor([0, 1]))
    assert u.random_or_learned_sinusoidal_cond is True and u.downsample_factor == 4
    assert torch.equal(u.class_rows(torch.tensor([3, 0]), 2), F.one_hot(torch.tensor([3, 0]), 5).float() * sqrt(5))
    with pytest.raises(RuntimeError, match="rows for a batch"):
        u.class_rows(torch.tensor([3, 0]), 3)


class _Net:
    """What ElucidatedDiffusion reads of a KarrasUnet, without a handle."""
    random_or_learned_sinusoidal_cond, self_condition, text_condition = True, False, False
    channels = out_dim = 3
    float_time_training = False
    downsample_factor, device = 4, "cpu"

    def __init__(self):
        self.labels = []

    def set_class_labels(self, class_labels, batch):
        self.labels.append((class_labels, batch))
        assert class_labels is not None, "class_labels are required by a network with num_classes and refused by one without"


def test_elucidated_diffusion_over_a_karras_unet_refuses_training_and_needs_labels():
    ed = dm.ElucidatedDiffusion(_Net(), image_size=16, channels=3)
    with pytest.raises(NotImplementedError):
        ed.train()
    with pytest.raises(NotImplementedError):
        ed(torch.zeros(2, 3, 16, 16))
    with pytest.raises(AssertionError, match="class_labels"):
        ed.sample(batch_size=2, num_sample_steps=4)
    net = _Net()
    net.self_condition = True
    with pytest.raises(NotImplementedError):
        dm.ElucidatedDiffusion(net, image_size=16, channels=3)
    for name in ("sample", "sample_using_dpmpp", "preconditioned_network_forward"):
        p = inspect.signature(getattr(dm.ElucidatedDiffusion, name)).parameters["class_labels"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert karras.KarrasUnet.float_time_training is False and dm.Unet.float_time_training is True


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def _struct_fields(name):
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        for d in decl.split(","):
            m = re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", d.strip())
            if m:
                names.append(m.group(1))
    return names


NEW_SYMBOLS = ("dm_kunet_create", "dm_kunet_set_class_labels", "dm_op_kunet_pixelnorm", "dm_op_kunet_avgpool2",
               "dm_op_kunet_bilinear_up2", "dm_op_kunet_act", "dm_op_kunet_attention", "dm_op_kunet_head",
               "dm_op_kunet_input_block", "dm_op_kunet_output_block", "dm_op_kunet_block")


def test_abi_additions():
    assert _struct_fields("dm_kunet_cfg") == [f[0] for f in _lib.KunetCfg._fields_]
    assert ctypes.sizeof(_lib.KunetCfg) == (9 + _lib.DM_MAX_STAGES + 2 + 4) * 4
    assert _struct_fields("dm_kunet_block_op") == [f[0] for f in _lib.KunetBlockOp._fields_]
    assert ctypes.sizeof(_lib.KunetBlockOp) == 12 * 4 + 11 * 8 + 4 * 4  # 3 ints and the tail padding behind the pointers
    # additions only: the image U-Net's configuration and the version stay
    assert _struct_fields("dm_unet_cfg")[-1] == "seq1d" and ctypes.sizeof(_lib.UnetCfg) == 37 * 4 and _lib.ABI_VERSION == 9
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.dm_abi_version() == 9
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, src), name
