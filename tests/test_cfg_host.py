"""Classifier-free guidance without a device: the golden (tests/golden/make_golden_cfg.py -> cfg_text.pt) against an in-test
float64 restatement of the reference formula, the argument checks, and the C ABI struct that carries the guidance."""
import ctypes
import inspect
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.unet import check_guidance

from conftest import load_golden, rel_l2

KEYWORDS = dict(cond_scale=1.0, rescaled_phi=0.0, remove_parallel_component=True, keep_parallel_frac=0.0)


def guided_f64(cond, null, cond_scale, rescaled_phi, remove_parallel_component, keep_parallel_frac):
    """Unet.forward_with_cond_scale's combine (DD/classifier_free_guidance.py:355-369, project :49-60), all in float64."""
    c = cond.double().flatten(1)
    update = (cond - null).double().flatten(1)
    if remove_parallel_component:
        unit = c / c.norm(dim=1, keepdim=True).clamp_min(1e-12)
        parallel = (update * unit).sum(dim=1, keepdim=True) * unit
        update = (update - parallel) + parallel * keep_parallel_frac
    scaled = c + update * (cond_scale - 1.0)
    if rescaled_phi != 0.0:
        ratio = c.std(dim=1, keepdim=True) / scaled.std(dim=1, keepdim=True)
        scaled = scaled * ratio * rescaled_phi + scaled * (1.0 - rescaled_phi)
    return scaled.reshape(cond.shape)


@pytest.fixture(scope="module")
def golden():
    return load_golden("cfg_text.pt")


def test_golden_is_the_formula(golden):
    n = 0
    for key, b in golden["fwd"].items():
        assert b["guided"].shape == (len(b["cases"]),) + tuple(b["cond"].shape), key
        assert not torch.equal(b["cond"], b["null"]), key  # the text really reaches the output
        for case, g in zip(b["cases"], b["guided"]):
            err = rel_l2(g, guided_f64(b["cond"], b["null"], *case))
            assert err < 1e-6, (key, case, err)
            n += 1
    assert n == 9 + 4 + 4 + 1 + 1
    grid = {tuple(c) for c in golden["fwd"]["cross1_16"]["cases"]}
    assert {c[0] for c in grid} == {3.0, 6.0} and {c[1] for c in grid} == {0.0, 0.7} and {c[2] for c in grid} == {True, False}
    assert any(c[3] == 0.5 for c in grid)
    for key in ("ddim20", "ddpm50", "ddim20_v"):
        assert golden[key]["case"][0] != 1.0 and bool(torch.isfinite(golden[key]["y"]).all())
    assert golden["ddim20_v"]["objective"] == "pred_v"


def test_cond_scale_one_is_the_conditioned_output():
    g = torch.Generator().manual_seed(1)
    cond, null = torch.randn((2, 3, 5, 7), generator=g), torch.randn((2, 3, 5, 7), generator=g)
    for case in ((1.0, 0.0, True, 0.0), (1.0, 0.7, False, 0.0), (1.0, 0.7, True, 0.5)):
        assert rel_l2(guided_f64(cond, null, *case), cond) < 1e-15


def test_guidance_argument_checks():
    text = types.SimpleNamespace(text_condition=True, self_condition=False)
    assert check_guidance(text, 1.0, 0.0, True, 0.0) is False
    assert check_guidance(text, 1, 0.7, False, 0.5) is False  # cond_scale == 1: no guidance, whatever the rest says
    assert check_guidance(text, 3.0, 0.7, True, 0.5) is True
    assert check_guidance(text, 0.0, 0.0, False, 0.0) is True
    with pytest.raises(ValueError, match="text-conditional"):
        check_guidance(types.SimpleNamespace(text_condition=False, self_condition=False), 3.0, 0.0, True, 0.0)
    with pytest.raises(NotImplementedError, match="self_condition"):
        check_guidance(types.SimpleNamespace(text_condition=True, self_condition=True), 3.0, 0.0, True, 0.0)
    for bad in (dict(cond_scale="3"), dict(cond_scale=float("nan")), dict(rescaled_phi=None), dict(keep_parallel_frac=True)):
        kw = dict(KEYWORDS, cond_scale=3.0)
        kw.update(bad)
        with pytest.raises(TypeError):
            check_guidance(text, **kw)
    with pytest.raises(TypeError, match="remove_parallel_component"):
        check_guidance(text, 3.0, 0.0, 1, 0.0)


@pytest.mark.parametrize("cls, methods", [
    (dm.TextConditionalDenoisingDiffusion, ("sample", "p_sample_loop", "ddim_sample", "model_predictions", "p_mean_variance",
                                            "p_sample")),
    (dm.TextConditionalLatentDiffusion, ("sample",)),
    (dm.Unet, ("forward_with_cond_scale",)),
])
def test_guidance_keywords(cls, methods):
    """Keyword-only, with the reference's defaults; the existing parameters keep their positional order."""
    for name in methods:
        params = inspect.signature(getattr(cls, name)).parameters
        for k, v in KEYWORDS.items():
            assert params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default == v, (cls, name, k)
    pos = [p for p, v in inspect.signature(dm.TextConditionalDenoisingDiffusion.model_predictions).parameters.items()
           if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert pos == ["self", "x", "t", "text_emb", "x_self_cond", "clip_x_start", "rederive_pred_noise"]
    pos = [p for p, v in inspect.signature(dm.Unet.forward_with_cond_scale).parameters.items()
           if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert pos == ["self", "x", "time", "text_emb"]


def test_sample_args_guidance_fields():
    """dm_sample_args (since ABI 6) ends with the guidance fields; the zero-initialised struct means no guidance."""
    names = [f[0] for f in _lib.SampleArgs._fields_]
    assert names[-6:] == ["cfg", "cfg_scale", "cfg_rescaled_phi", "cfg_keep_parallel_frac", "cfg_remove_parallel",
                          "cfg_reserved_"]
    a = _lib.SampleArgs()
    assert a.cfg == 0 and a.cfg_scale == 0.0
    assert ctypes.sizeof(_lib.SampleArgs) % 8 == 0
    assert _lib.ABI_VERSION == 9
    assert {"dm_unet_forward_masked", "dm_op_cfg_combine"} <= set(_lib.EXPORTS)
