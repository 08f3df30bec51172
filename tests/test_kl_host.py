"""CPU checks of the KL first stage: the parameter spec against the reference's ``state_dict()`` key list, the CPU
restatement (tests/kl_oracle.py) against the reference's outputs (tests/golden/kl.pt, tests/golden/make_golden_kl.py), the
ABI version, and the helper through which the latent classes read a first stage's ``encode``."""
import importlib.util
import os

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import diffusion as D

import kl_oracle as ko
from conftest import GOLDEN, load_golden, rel_l2

# fp32 on the CPU against the reference's fp32 on the CPU: the same torch operators in the same order
ORACLE_TOL = 1e-6


def _generator():
    """The generator's case table and config builder (it touches the reference inside main() only)."""
    spec = importlib.util.spec_from_file_location("make_golden_kl", os.path.join(GOLDEN, "make_golden_kl.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CASES, mod.configs


@pytest.fixture(scope="module")
def golden_kl():
    return load_golden("kl.pt")


@pytest.fixture(scope="module")
def cases():
    table, configs = _generator()
    out = {}
    for name, (ddconfig, embed_dim, salt, shape, _) in table.items():
        ecfg, dcfg = configs(ddconfig, embed_dim)
        out[name] = (ecfg, dcfg, salt, shape)
    return out


def test_cases_match_the_fixture(golden_kl, cases):
    assert sorted(golden_kl) == sorted(cases)
    for name, (ecfg, dcfg, _, shape) in cases.items():
        g = golden_kl[name]
        f = 2 ** (ecfg.num_resolutions - 1)
        assert tuple(g["x"].shape) == shape
        assert tuple(g["moments"].shape) == (shape[0], 2 * ecfg.embed_dim, shape[2] // f, shape[3] // f)
        assert tuple(g["z"].shape) == tuple(g["eps"].shape) == tuple(g["mode"].shape)
        raw = g["moments"][:, ecfg.embed_dim:]
        assert float(((raw > -30) & (raw < 20)).double().mean()) >= 0.9


def test_param_spec_is_the_reference_state_dict_order(golden_kl, cases):
    for name, (ecfg, dcfg, _, _) in cases.items():
        spec = dm.autoencoder_kl_param_spec(ecfg, dcfg)
        assert [n for n, _ in spec] == golden_kl[name]["keys"], name
        shapes = dict(spec)
        assert shapes["quant_conv.weight"] == (2 * ecfg.embed_dim, 2 * ecfg.z_channels, 1, 1)  # autoencoder.py:356
        assert shapes["post_quant_conv.weight"] == (ecfg.z_channels, ecfg.embed_dim, 1, 1)
        assert not any(n.startswith("quantize.") for n in shapes)


def test_vq_spec_is_unchanged_by_the_kl_branch():
    cfg = dm.EncoderConfig()
    names = [n for n, _ in dm.encoder_param_spec(cfg)]
    assert names[-3:] == ["quant_conv.weight", "quant_conv.bias", "quantize.embedding.weight"]
    assert dict(dm.encoder_param_spec(cfg))["quant_conv.weight"] == (cfg.embed_dim, cfg.z_channels, 1, 1)
    with pytest.raises(AssertionError):
        dm.encoder_param_spec(dm.EncoderConfig(n_embed=0, double_z=False))


def test_oracle_matches_the_reference(golden_kl, cases):
    torch.set_num_threads(8)
    for name, (ecfg, dcfg, salt, _) in cases.items():
        g = golden_kl[name]
        sd = dm.synth_state_dict(dm.autoencoder_kl_param_spec(ecfg, dcfg), salt=salt)
        with torch.inference_mode():
            post = ko.kl_encode(sd, ecfg, g["x"])
            errs = dict(moments=rel_l2(post.parameters, g["moments"]), mode=rel_l2(post.mode(), g["mode"]),
                        z=rel_l2(post.sample(g["eps"]), g["z"]), kl=rel_l2(post.kl(), g["kl"]),
                        nll=rel_l2(post.nll(g["z"]), g["nll"]), dec=rel_l2(ko.kl_decode(sd, dcfg, g["z"]), g["dec"]),
                        dec_mode=rel_l2(ko.kl_forward(sd, ecfg, dcfg, g["x"])[0], g["dec_mode"]))
        print(name, {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) <= ORACLE_TOL, (name, errs)


def test_oracle_clamp_and_kl_other():
    """What kl.pt does not reach: both clamp edges, and kl(other) against the closed form for equal distributions."""
    lv = torch.tensor([-40.0, -30.0, 0.5, 20.0, 30.0], dtype=torch.float64).view(1, 5, 1, 1)
    p = ko.Posterior(torch.cat([torch.zeros_like(lv), lv], dim=1))
    assert p.logvar.flatten().tolist() == [-30.0, -30.0, 0.5, 20.0, 20.0]
    assert torch.equal(p.parameters[:, 5:], lv)  # parameters stay raw
    assert float(p.kl(p)) == 0.0
    unit = ko.Posterior(torch.zeros(1, 10, 1, 1, dtype=torch.float64))
    assert float((p.kl(unit) - p.kl()).abs()) <= 1e-9 * float(p.kl())


def test_abi_version_stays_9():
    assert _lib.ABI_VERSION == 9
    for name in ("dm_encoder_forward_kl", "dm_encoder_quantize", "dm_encoder_embed_code", "dm_op_kl_posterior",
                 "dm_op_embed_code", "dm_op_vq_nearest_nchw"):
        assert name in _lib.EXPORTS


def test_public_surface():
    for name in ("AutoencoderKL", "DiagonalGaussianDistribution", "VQModelInterface"):
        assert name in dm.__all__ and hasattr(dm, name)
    assert issubclass(dm.VQModelInterface, dm.VQModel) and hasattr(dm.VQModel, "decode_code")
    for m in ("encode", "decode", "forward", "encode_sample", "init_from_ckpt", "load_state_dict", "param_spec",
              "decoded_shape", "eval", "parameters"):
        assert hasattr(dm.AutoencoderKL, m), m
    for m in ("sample", "mode", "kl", "nll"):
        assert hasattr(dm.DiagonalGaussianDistribution, m), m
    with pytest.raises(RuntimeError):
        dm.DiagonalGaussianDistribution(torch.zeros(1, 2, 2, 2))  # a CPU tensor: there is no CPU path


def test_checkpoint_filter_keeps_the_kl_keys_and_drops_the_loss():
    from diffusion_models_amd.checkpoint import vae_state_dict_from_checkpoint

    sd = {k: torch.zeros(1) for k in ("encoder.conv_in.weight", "decoder.conv_in.weight", "quant_conv.weight",
                                      "post_quant_conv.bias", "loss.logvar", "loss.discriminator.main.0.weight")}
    assert sorted(vae_state_dict_from_checkpoint({"state_dict": sd})) == [
        "decoder.conv_in.weight", "encoder.conv_in.weight", "post_quant_conv.bias", "quant_conv.weight"]


class _Vae:
    def __init__(self, ret):
        self.ret, self.calls = ret, []

    def encode(self, images):
        self.calls.append("encode")
        return self.ret


class _Posterior:
    def __init__(self, z):
        self.z = z

    def sample(self):
        return self.z


class _KlVae(_Vae):
    def encode_sample(self, images):
        self.calls.append("encode_sample")
        return self.ret


def test_latent_helper_keeps_tensors_and_tuples_and_samples_posteriors():
    z = torch.arange(6.0).view(1, 1, 2, 3)
    x = torch.zeros(1, 3, 4, 6)
    assert D._first_stage_latents(_Vae(z), x) is z                       # VQModelInterface: a tensor
    assert D._first_stage_latents(_Vae((z, None, (None, None, None))), x) is z  # VQModel: the head of the tuple
    assert D._first_stage_latents(_Vae(_Posterior(z)), x) is z           # a posterior of a foreign VAE: its sample
    v = _KlVae(z)
    assert D._first_stage_latents(v, x) is z and v.calls == ["encode_sample"]  # AutoencoderKL: the one-call route


@pytest.mark.parametrize("cls", ["LatentDiffusion", "TextConditionalLatentDiffusion", "ImageConditionalLatentDiffusion"])
def test_latent_classes_encode_through_the_helper(cls):
    """``encode`` of the three latent classes on an object that has nothing but the attributes it reads."""
    z = torch.ones(1, 1, 2, 2)
    for ret in (z, (z, None, None), _Posterior(z)):
        obj = object.__new__(getattr(dm, cls))
        obj.vae = _Vae(ret)
        obj.cond_vae = _Vae((2 * z,))
        assert obj.encode(torch.zeros(1, 3, 4, 4)) is z
    if cls == "ImageConditionalLatentDiffusion":
        assert torch.equal(obj.encode(torch.zeros(1, 3, 4, 4), cond=True), 2 * z)
