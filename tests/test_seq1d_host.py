"""The sequence model (Unet1D / DenoisingDiffusion1D) on the host: spec, schedule, packers, refusals, checkpoint, ABI.
No GPU.  Goldens: tests/golden/seq1d.pt (tests/golden/make_golden_seq1d.py, from the reference)."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv1d_restate as c1
import diffusion_models_amd as dm
from diffusion_models_amd import _lib, seq1d
from diffusion_models_amd.spec import SCHEDULE_BUFFERS, Unet1DConfig, make_schedule, unet1d_param_spec

from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def golden():
    return load_golden("seq1d.pt")


def seeded(shape, seed, dtype=torch.float64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ---- spec ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["d32_c2", "d64_c1"])
def test_param_spec_equals_reference_state_dict(golden, key):
    g = golden["keys"][key]
    spec = unet1d_param_spec(Unet1DConfig(**g["unet_kw"]))
    assert [(k, tuple(s)) for k, s in spec] == [(k, tuple(s)) for k, s in g["entries"]]


def test_param_spec_structure():
    spec = unet1d_param_spec(Unet1DConfig(dim=32, dim_mults=(1, 2), channels=2))
    names = dict(spec)
    assert len(spec) == 138 and spec[0] == ("init_conv.weight", (32, 2, 7))
    assert not any("mem_kv" in k for k in names)
    assert names["downs.0.2.fn.norm.g"] == (1, 32, 1) and names["mid_attn.fn.norm.g"] == (1, 64, 1)
    assert names["downs.0.2.fn.fn.to_qkv.weight"] == (384, 32, 1) and names["downs.0.2.fn.fn.to_out.1.g"] == (1, 32, 1)
    assert names["mid_attn.fn.fn.to_out.weight"] == (64, 128, 1) and "mid_attn.fn.fn.to_out.1.g" not in names
    assert names["downs.0.3.weight"] == (32, 32, 4) and names["downs.1.3.weight"] == (64, 32, 3)
    assert names["ups.0.3.1.weight"] == (32, 64, 3) and names["ups.1.3.weight"] == (32, 32, 3)
    order = [k for k, _ in spec]
    assert order.index("ups.1.3.bias") < order.index("mid_block1.mlp.1.weight")  # downs, ups, then the mid blocks
    # attn_dim_head / attn_heads shape mid_attn alone
    wide = dict(unet1d_param_spec(Unet1DConfig(dim=32, dim_mults=(1, 2), channels=2, attn_dim_head=64, attn_heads=2)))
    assert wide["mid_attn.fn.fn.to_qkv.weight"] == (384, 64, 1) and wide["downs.0.2.fn.fn.to_qkv.weight"] == (384, 32, 1)
    sc = dict(unet1d_param_spec(Unet1DConfig(dim=32, dim_mults=(1, 2), channels=2, self_condition=True, learned_variance=True)))
    assert sc["init_conv.weight"] == (32, 4, 7) and sc["final_conv.weight"] == (4, 32, 1)


# ---- schedule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["linear", "cosine"])
@pytest.mark.parametrize("objective", ["pred_noise", "pred_x0", "pred_v"])
def test_schedule_and_loss_weight(golden, name, objective):
    """The 13 buffers as DenoisingDiffusion1D builds them: make_schedule(ddpm=False) without min-SNR, bit for bit."""
    want = golden["sched"][f"{name}_{objective}"]
    got = make_schedule(1000, name, ddpm=False, objective=objective, min_snr_loss_weight=False)
    assert list(want.keys()) == list(SCHEDULE_BUFFERS)
    for k in SCHEDULE_BUFFERS:
        assert got[k].dtype == torch.float32 and torch.equal(got[k], want[k]), k


def test_schedule_250(golden):
    got = make_schedule(250, "cosine", ddpm=False, objective="pred_noise")
    for k, v in golden["sched"]["cosine250_pred_noise"].items():
        assert torch.equal(got[k], v), k


# ---- the Upsample packing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,L,B", [(64, 32, 12, 3), (8, 64, 1, 2), (5, 3, 7, 1)])
def test_upsample_packing_is_exact(cin, cout, L, B):
    """nearest x2 + Conv1d(3, padding 1) == one K = 3 convolution with 2 Cout channels on the source grid: fp64 agreement at
    rounding level (the packing adds two taps before the products instead of after)."""
    x, w, b = seeded((B, cin, L), 1), seeded((cout, cin, 3), 2) / (3 * cin) ** 0.5, seeded((cout,), 3)
    ref = c1.upsample_reference(x, w, b)
    got = c1.upsample_conv(x, w, b)
    assert got.shape == ref.shape == (B, cout, 2 * L)
    assert float((got - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max()))
    w2, b2 = c1.upsample1d_pack(w, b)
    assert w2.shape == (2 * cout, cin, 3) and torch.equal(b2, torch.cat([b, b]))
    assert torch.equal(w2[:cout, :, 2], torch.zeros(cout, cin, dtype=w.dtype)) and torch.equal(w2[cout:, :, 0], w2[:cout, :, 2])
    assert torch.equal(w2[:cout, :, 0], w[:, :, 0]) and torch.equal(w2[cout:, :, 2], w[:, :, 2])
    # fp32 packing: within fp32 rounding of the fp64 layer
    got32 = c1.upsample_conv(x.float(), w.float(), b.float())
    assert float((got32.double() - ref).norm() / ref.norm()) < 2e-6


# ---- refusals (no handle is needed to be refused) ----------------------------------------------------------------------------------
class _Model:
    seq1d, channels, out_dim, self_condition, random_or_learned_sinusoidal_cond, downsample_factor = True, 2, 2, False, False, 2
    device = "cpu"


def _diffusion(**kw):
    return dm.DenoisingDiffusion1D(_Model(), seq_length=16, **kw)


def test_constructor_defaults_and_shape():
    d = _diffusion()
    assert d.sample_shape() == (2, 16) and d.seq_length == 16 and d.num_timesteps == 1000 and not d.is_ddim_sampling
    assert torch.equal(d.loss_weight, make_schedule(1000, "cosine", ddpm=False)["loss_weight"])
    sd = d.state_dict()
    assert list(sd.keys()) == list(SCHEDULE_BUFFERS)


def test_refusals():
    with pytest.raises(ValueError):
        _diffusion(beta_schedule="sigmoid")
    with pytest.raises(ValueError):
        _diffusion(objective="pred_eps")
    m = _Model()
    m.random_or_learned_sinusoidal_cond = True
    with pytest.raises(NotImplementedError):
        dm.DenoisingDiffusion1D(m, seq_length=16)
    m = _Model()
    m.out_dim = 4
    with pytest.raises(NotImplementedError):
        dm.DenoisingDiffusion1D(m, seq_length=16)
    m = _Model()
    m.seq1d = False
    with pytest.raises(TypeError):
        dm.DenoisingDiffusion1D(m, seq_length=16)
    d = _diffusion(sampling_timesteps=8)
    x = torch.zeros(2, 2, 16)
    for call in (lambda: d.p_losses(x, torch.zeros(2, dtype=torch.long)), lambda: d.forward(x), lambda: d(x),
                 lambda: d.train(), lambda: d.dpm_solver_sample((2, 2, 16)), lambda: d.sample(2, solver="dpmpp"),
                 lambda: d.p_sample(x, 3, clip_denoised=False)):
        with pytest.raises(NotImplementedError):
            call()
    assert d.train(False) is d
    with pytest.raises(AssertionError):  # the length must be divisible by 2 ** (stages - 1), before any launch
        d.ddim_sample((2, 2, 15))


def test_unet1d_refusals_need_no_handle():
    u = dm.Unet1D.__new__(dm.Unet1D)
    u._handle = None
    with pytest.raises(NotImplementedError, match="follow-up"):
        u.train()
    assert u.train(False) is u
    u._loaded, u.cfg = True, Unet1DConfig(dim=32, dim_mults=(1, 2, 4), channels=2)
    with pytest.raises(RuntimeError, match="divisible by 4"):
        u.forward(torch.zeros(1, 2, 10), torch.zeros(1, dtype=torch.long))
    with pytest.raises(RuntimeError):
        u.forward(torch.zeros(1, 2, 1, 8), torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError):
        dm.Unet1D(32, attn_heads=(4, 4))


# ---- surface ----------------------------------------------------------------------------------------------------------------------
def test_surface_follows_the_reference(golden):
    s = golden["surface"]
    ref_init = [p[0] for p in s["unet"]["init_params"]]
    ours = [p for p in inspect.signature(dm.Unet1D.__init__).parameters if p != "self"]
    assert ours[:len(ref_init)] == ref_init and ours[len(ref_init):] == ["device"]
    for name, default, _ in s["unet"]["init_params"]:
        if default is not None:
            assert inspect.signature(dm.Unet1D.__init__).parameters[name].default == default, name
    assert [p[0] for p in s["unet"]["methods"]["forward"]] == [p for p in inspect.signature(dm.Unet1D.forward).parameters
                                                               if p != "self"]
    sig = inspect.signature(dm.DenoisingDiffusion1D.__init__)
    ours = [p for p in sig.parameters if p != "self"]
    ref_init = s["diffusion"]["init_params"]
    assert ours[:len(ref_init)] == [p[0] for p in ref_init] and ours[len(ref_init):] == ["use_graph"]
    for name, default, kind in ref_init:
        assert sig.parameters[name].kind.name == kind, name
        if name not in ("model", "seq_length"):
            assert sig.parameters[name].default == default, name
    for name, params in s["diffusion"]["methods"].items():
        ref_pos = [p[0] for p in params if p[1] == "POSITIONAL_OR_KEYWORD"]
        have = [p for p, v in inspect.signature(getattr(dm.DenoisingDiffusion1D, name)).parameters.items()
                if p != "self" and v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
        if name in ("p_losses", "forward"):
            continue  # refused: the follow-up
        assert have[:len(ref_pos)] == ref_pos, (name, have, ref_pos)


def test_state_dict_keys(golden):
    spec = unet1d_param_spec(Unet1DConfig(dim=32, dim_mults=(1, 2), channels=2))
    assert golden["state_dict_keys"] == list(SCHEDULE_BUFFERS) + ["model." + k for k, _ in spec]


# ---- checkpoint -------------------------------------------------------------------------------------------------------------------
def test_load_trainer1d_checkpoint(tmp_path, golden):
    """Trainer1D.save writes step / model / opt / ema / scaler / version (denoising_diffusion_1d.py:768-781)."""
    spec = unet1d_param_spec(Unet1DConfig(dim=32, dim_mults=(1, 2), channels=2))
    sched = make_schedule(1000, "cosine", ddpm=False)
    raw = {**sched, **{"model." + k: v for k, v in dm.synth_state_dict(spec, salt=1).items()}}
    ema = {**sched, **{"model." + k: v for k, v in dm.synth_state_dict(spec, salt=2).items()}}
    data = {"step": 7, "model": raw, "opt": {}, "ema": {"initted": torch.tensor(True), "step": torch.tensor(7),
                                                        **{"ema_model." + k: v for k, v in ema.items()},
                                                        **{"online_model." + k: v for k, v in raw.items()}},
            "scaler": None, "version": "2.0.0"}
    path = os.path.join(tmp_path, "model-1.pt")
    torch.save(data, path)
    sd = dm.load_trainer_checkpoint(path)
    assert list(sd.keys()) == golden["state_dict_keys"]
    assert torch.equal(sd["model.init_conv.weight"], ema["model.init_conv.weight"])
    sd = dm.load_trainer_checkpoint(path, prefer_ema=False)
    assert torch.equal(sd["model.init_conv.weight"], raw["model.init_conv.weight"])
    d = _diffusion()
    d.model.load_state_dict = lambda model_sd, strict=True: setattr(d.model, "got", model_sd)
    d.load_state_dict(sd)
    assert list(d.model.got.keys()) == [k for k, _ in spec] and d.model.got["init_conv.weight"].shape == (32, 2, 7)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def _struct_fields(name):
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):  # "int32_t B, H, W" / "const float* x_T" / "int32_t dim_mults[DM_MAX_STAGES]"
        for d in decl.split(","):
            m = re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", d.strip())
            if m:
                names.append(m.group(1))
    return names


def test_abi_additions():
    assert _struct_fields("dm_unet_cfg") == [f[0] for f in _lib.UnetCfg._fields_]
    assert _struct_fields("dm_unet_cfg")[-1] == "seq1d" and ctypes.sizeof(_lib.UnetCfg) == 37 * 4
    assert _lib.UnetCfg().seq1d == 0  # the zero-initialised struct is the image U-Net
    assert _struct_fields("dm_sample_args") == [f[0] for f in _lib.SampleArgs._fields_]
    assert ctypes.sizeof(_lib.SampleArgs) == 160 and _lib.SampleArgs().ddim_flags == 0
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    assert int(re.search(r"#define DM_DDIM_NO_CLAMP (\d+)", src).group(1)) == _lib.DDIM_NO_CLAMP == 1
    assert int(re.search(r"#define DM_DDIM_RAW_NOISE (\d+)", src).group(1)) == _lib.DDIM_RAW_NOISE == 2
    assert {"dm_op_conv1d", "dm_op_block1d", "dm_op_sampler_update_ex"} <= set(_lib.EXPORTS)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dm_op_conv1d", "dm_op_block1d", "dm_op_sampler_update_ex"):
        assert hasattr(lib, name), name
    assert seq1d.TRAINING_FOLLOW_UP


# ---- Winograd F(4,3): packer and fp32 restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,L,B,limit", [(64, 64, 32, 2, 1.5e-6), (512, 512, 16, 2, 3e-6), (8, 64, 4, 3, 1.5e-6)])
def test_wino1d_restatement(cin, cout, L, B, limit):
    """F(4,3) is exact in fp64 and, in fp32 on randn inputs with weights scaled by 1 / sqrt(3 C), a few times the direct sum's
    error (5.0e-7 at 64 -> 64, L = 32 and 9.9e-7 at 512 -> 512, L = 16; the direct sum: 1.3e-7, 1.6e-7): far inside the
    operator limit of 2e-5.  ``limit`` is three times those figures."""
    x, w, b = seeded((B, cin, L), 41), seeded((cout, cin, 3), 42) / (3 * cin) ** 0.5, seeded((cout,), 43)
    ref = F.conv1d(x, w, b, padding=1)
    exact = c1.wino1d(x, w, b)
    assert float((exact - ref).norm() / ref.norm()) < 1e-13
    got = c1.wino1d(x.float(), w.float(), b.float())
    err = float((got.double() - ref).norm() / ref.norm())
    direct = float((c1.direct(x, w, b, pad=1).double() - ref).norm() / ref.norm())
    print(f"wino1d {cin}->{cout} L={L}: F(4,3) fp32 {err:.2e}, direct fp32 {direct:.2e}")
    assert direct < err < limit
    U = c1.wino1d_pack(w.float())
    assert U.shape == (cout, cin, 6) and torch.equal(U[..., 5], w.float()[..., 2]) and torch.equal(U[..., 0], w.float()[..., 0] / 4)


def test_wino1d_never_reads_the_neighbouring_sequence():
    """Tiles at the ends of a sequence read zeros, not the next sequence's rows: the batch is independent."""
    x, w = seeded((3, 8, 8), 44), seeded((64, 8, 3), 45)
    whole = c1.wino1d(x, w)
    for i in range(3):
        assert torch.equal(c1.wino1d(x[i:i + 1], w), whole[i:i + 1])
