"""ElucidatedDiffusion training, host logic, no GPU: the per-image coefficient rows against the scalars recorded from the
running reference BIT FOR BIT, the sigma draw and the order of the two draws, the hand-written struct binding against the
header, the surface and the refusals, and the plain-torch restatement of the three training kernels
(tests/edm_train_oracle.py) against autograd in fp64 and against the reference's recorded loss.
Fixture: tests/golden/make_golden_edm_train.py."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import elucidated as E
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo

import edm_train_oracle as eto
from conftest import ROOT, load_golden


@pytest.fixture(scope="module")
def golden():
    return load_golden("edm_train.pt")


def _stub_net(**kw):
    base = dict(random_or_learned_sinusoidal_cond=True, self_condition=False, text_condition=False, out_dim=3, channels=3,
                cfg=types.SimpleNamespace(cond_channels=0), device="cpu", downsample_factor=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_fixture_holds_the_cases_the_feature_is_specified_on(golden):
    c = golden["cases"]
    assert set(c) == {"d32_learned", "d64_learned", "d32_random", "d32_lsd8", "d32_sigma_range", "d32_accumulate2"}
    assert (c["d32_learned"]["B"], c["d32_learned"]["image_size"]) == (6, 16)
    assert (c["d64_learned"]["B"], c["d64_learned"]["image_size"], tuple(c["d64_learned"]["unet_kw"]["dim_mults"])) == (4, 32, (1, 2, 4))
    assert c["d32_random"]["unet_kw"]["random_fourier_features"] and c["d32_random"]["frozen"] == ["time_mlp.0.weights"]
    assert c["d32_lsd8"]["unet_kw"]["learned_sinusoidal_dim"] == 8
    assert [round(float(v), 6) for v in c["d32_sigma_range"]["sigmas"][0]] == [0.002, 0.05, 0.5, 3.0, 20.0, 80.0]
    assert c["d32_accumulate2"]["micro"] == 2
    for case in c.values():
        assert 0 <= case["ref_err_loss"] < 1e-5 and 0 < case["ref_err_grad_max"] < 1e-4


def test_coefficient_rows_bitwise(golden):
    for key, c in golden["cases"].items():
        for sig, rec in zip(c["sigmas"], c["scalars"]):
            tab = dm.edm_train_table(sig, 0.5)
            assert tab.shape == (c["B"], E.COLS) and tab.dtype == torch.float32
            assert torch.equal(tab[:, E.SIGMA], sig), key
            for col, name in ((E.C_IN, "c_in"), (E.C_NOISE, "c_noise"), (E.C_SKIP, "c_skip"), (E.C_OUT, "c_out"),
                              (E.LOSS_W, "loss_weight")):
                assert torch.equal(tab[:, col], rec[name]), (key, name)
            used = {E.C_IN, E.C_NOISE, E.C_SKIP, E.C_OUT, E.SIGMA, E.LOSS_W}
            assert all(bool((tab[:, j] == 0).all()) for j in range(E.COLS) if j not in used)
    # the methods of the object are the same expressions
    edm = dm.ElucidatedDiffusion(_stub_net(), image_size=16)
    sig = golden["cases"]["d32_sigma_range"]["sigmas"][0]
    assert torch.equal(edm.loss_weight(sig), dm.edm_train_table(sig)[:, E.LOSS_W])


def test_noise_distribution_draw_is_the_references(golden):
    g = golden["noise_distribution"]
    edm = dm.ElucidatedDiffusion(_stub_net(), image_size=16)
    torch.manual_seed(g["seed"])
    got = edm.noise_distribution(g["B"])
    assert got.dtype == torch.float32 and torch.equal(got, g["sigmas"])


def test_draw_order_is_sigma_then_noise(golden):
    """The reference asked its (redirected) generator for the (B,) sigma draw first and the image-shaped noise second, per
    micro-batch: the recorded tensors are reproduced by one NoiseStream read in that order."""
    for key, c in golden["cases"].items():
        if key == "d32_sigma_range":
            continue
        stream = so.NoiseStream(c["seed"])
        for sig, noise in zip(c["sigmas"], c["noises"]):
            assert torch.equal((-1.2 + 1.2 * stream((c["B"],))).exp(), sig), key
            assert torch.equal(stream(noise.shape), noise), key



def test_forward_draws_sigma_before_the_noise(golden):
    """forward() itself, run on the CPU up to its second draw: a handle-less ``Unet`` shell marked as armed, the two draw
    methods recorded, the noise draw stops the call (nothing reaches the library or a device)."""
    from diffusion_models_amd.unet import Unet

    class _Stop(Exception):
        pass

    net = object.__new__(Unet)  # no constructor: no handle is created, __del__ finds none to destroy
    net.__dict__.update(_stub_net().__dict__, _training=True, _loaded=True)
    net._handle = ctypes.c_void_p(1)
    try:
        edm = dm.ElucidatedDiffusion(net, image_size=16)
        calls = []
        real = edm._draw_sigmas
        drawn = []
        edm._draw_sigmas = lambda n: calls.append(("sigma", n)) or drawn.append(real(n)) or drawn[-1]

        def randn(shape, *a, **k):
            calls.append(("noise", tuple(shape)))
            raise _Stop

        edm._randn = randn
        g = golden["noise_distribution"]
        torch.manual_seed(g["seed"])
        with pytest.raises(_Stop):
            edm(torch.zeros(g["B"], 3, 16, 16))
        assert calls == [("sigma", g["B"]), ("noise", (g["B"], 3, 16, 16))]
        assert torch.equal(drawn[0], g["sigmas"])  # the first consumer of the global CPU generator, as in the reference
        # injected draws: neither method is called
        calls.clear()
        with pytest.raises(RuntimeError, match="sigmas has 5 entries"):
            edm(torch.zeros(6, 3, 16, 16), sigmas=torch.ones(5), noise=torch.zeros(6, 3, 16, 16))
        assert calls == []
    finally:
        net._handle = ctypes.c_void_p()  # nothing for __del__ to hand to the library


def test_train_args_binding_matches_the_header():
    """``_lib.EdmTrainArgs`` is written by hand: field names, order, C types and offsets are those of ``dm_edm_train_args``."""
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    body = re.search(r"typedef struct dm_edm_train_args \{(.*?)\} dm_edm_train_args;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    declared = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*([\w\s,]+)", decl)
        assert m, decl
        for name in (n.strip() for n in m.group(4).split(",")):
            declared.append((name, "pointer" if m.group(3) else ctype[m.group(2)]))
    bound = []
    for name, t in _lib.EdmTrainArgs._fields_:
        is_ptr = t is ctypes.c_void_p or isinstance(t, type(ctypes.POINTER(ctypes.c_float)))
        bound.append((name, "pointer" if is_ptr else t))
    assert bound == declared
    off, offsets = 0, {}
    for name, t in declared:
        size = 8 if t == "pointer" else ctypes.sizeof(t)
        off = (off + size - 1) // size * size
        offsets[name] = off
        off += size
    assert {n: getattr(_lib.EdmTrainArgs, n).offset for n, _ in _lib.EdmTrainArgs._fields_} == offsets
    assert ctypes.sizeof(_lib.EdmTrainArgs) == (off + 7) // 8 * 8 == 72
    assert {"images", "noise", "coef_host", "coef_stride", "loss_scale", "accumulate", "loss_out_host", "denoised_out", "B", "H",
            "W", "stream"} == {n for n, _ in declared}
    assert E.LOSS_W == 14 < _lib.DM_EDM_COEFS
    assert {"dm_unet_train_enable_ft", "dm_unet_loss_backward_edm", "dm_op_edm_noise_in", "dm_op_edm_loss",
            "dm_op_sinusoid_ft_bwd"} <= set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 9


def test_surface_and_refusals():
    params = list(inspect.signature(dm.ElucidatedDiffusion.forward).parameters.values())[1:]
    assert [p.name for p in params] == ["images", "sigmas", "noise", "loss_scale", "accumulate", "sync", "return_denoised"]
    assert params[0].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[1:])
    assert [p.default for p in params[1:]] == [None, None, 1.0, False, True, False]
    assert dm.ElucidatedDiffusion.__call__ is dm.ElucidatedDiffusion.forward
    assert list(inspect.signature(dm.ElucidatedDiffusion.train).parameters)[1:] == ["mode"]
    edm = dm.ElucidatedDiffusion(_stub_net(), image_size=16)
    # a net that is not a library Unet: refused before any tensor or the device is touched
    with pytest.raises(NotImplementedError, match="train"):
        edm(torch.zeros(1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match="train"):
        edm.train()
    assert edm.train(False) is edm
    with pytest.raises(NotImplementedError, match="self_condition"):
        dm.ElucidatedDiffusion(_stub_net(self_condition=True), image_size=16)
    with pytest.raises(NotImplementedError, match="text-conditional"):
        dm.ElucidatedDiffusion(_stub_net(text_condition=True), image_size=16)
    with pytest.raises(ValueError, match="learned variance"):
        dm.ElucidatedDiffusion(_stub_net(out_dim=6), image_size=16)
    # train_step keeps the two kinds of injected draws apart
    with pytest.raises(ValueError, match="sigmas"):
        dm.train_step(edm, [torch.zeros(1, 3, 16, 16)], t=[torch.zeros(1, dtype=torch.long)])
    sig = inspect.signature(dm.train_step).parameters
    assert sig["sigmas"].kind is inspect.Parameter.KEYWORD_ONLY and sig["sigmas"].default is None


def test_restated_passes_agree_with_autograd_in_fp64():
    g = torch.Generator().manual_seed(9)
    B, shape = 5, (5, 3, 8, 8)
    sig = torch.tensor([0.002, 0.3, 1.7, 20.0, 80.0])
    tab = dm.edm_train_table(sig).double()
    img = torch.rand(shape, generator=g, dtype=torch.float64)
    eps = torch.randn(shape, generator=g, dtype=torch.float64)
    F = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True)
    pad = lambda col: tab[:, col].reshape(B, 1, 1, 1)  # noqa: E731
    # the reference's expressions (:240-264)
    x0 = img * 2 - 1
    noised = x0 + pad(E.SIGMA) * eps
    D = pad(E.C_SKIP) * noised + pad(E.C_OUT) * F
    losses = torch.nn.functional.mse_loss(D, x0, reduction="none").reshape(B, -1).mean(dim=1) * tab[:, E.LOSS_W]
    loss = losses.mean() * 0.5
    loss.backward()
    rx0, rnoised, rxin = eto.noise_in(img, eps, tab)
    assert torch.equal(rx0, x0) and torch.equal(rnoised, noised) and torch.equal(rxin, pad(E.C_IN) * noised)
    rloss, rdF, rD = eto.loss_and_dF(rnoised, F.detach(), rx0, tab, loss_scale=0.5)
    assert torch.allclose(rD, D.detach(), rtol=0, atol=0)
    assert abs(float(rloss) - float(loss.detach())) <= 1e-14 * abs(float(loss.detach()))
    assert float((rdF - F.grad).norm() / F.grad.norm()) <= 1e-14
    # the learned embedding (DD/denoising_diffusion.py:96-101)
    for half in (8, 4):
        w = torch.randn(half, generator=g, dtype=torch.float64, requires_grad=True)
        t = tab[:, E.C_NOISE]
        freqs = t[:, None] * w[None, :] * 2 * torch.pi
        e0 = torch.cat((t[:, None], freqs.sin(), freqs.cos()), dim=-1)
        de0 = torch.randn(e0.shape, generator=g, dtype=torch.float64)
        (e0 * de0).sum().backward()
        got = eto.sinusoid_ft_bwd(de0, e0.detach(), half)
        assert float((got - w.grad).norm() / w.grad.norm()) <= 1e-13
        assert torch.equal(eto.sinusoid_ft_bwd(de0, e0.detach(), half, learned=False), torch.zeros(half, dtype=torch.float64))


@pytest.mark.parametrize("key", ["d32_learned", "d32_random", "d32_lsd8", "d32_sigma_range", "d32_accumulate2"])
def test_restatement_reproduces_the_reference_loss(golden, key):
    """The restated passes around the CPU oracle U-Net give the reference's loss (fp32 on the same CPU; the reductions are
    ordered differently, so the bound is the project's loss tolerance, 1e-5)."""
    c = golden["cases"][key]
    cfg = UnetConfig(channels=3, **c["unet_kw"])
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=c["salt"])
    total = 0.0
    with torch.inference_mode():
        for img, sig, noise in zip(c["imgs"], c["sigmas"], c["noises"]):
            total += float(eto.edm_loss(lambda x, t: uo.unet_forward(sd, cfg, x, t), img, noise, dm.edm_train_table(sig),
                                        loss_scale=1.0 / c["micro"]))
    err = abs(total - c["loss"]) / abs(c["loss"])
    print(key, "restated loss", total, "reference", c["loss"], "rel", err)
    assert err <= 1e-5


def test_digests_unpack_to_the_form_the_checker_reads(golden):
    from conftest import check_grad_digest
    from oracle.train_oracle import directions

    c = golden["cases"]["d32_lsd8"]
    spec = dm.unet_param_spec(UnetConfig(channels=3, **c["unet_kw"]))
    dg = eto.unpack_digests(c, spec)
    assert list(dg) == [n for n, _ in spec]
    w = dg["time_mlp.0.weights"]
    assert tuple(w["full"].shape) == (4,) and w["norm"] > 0
    check_grad_digest("time_mlp.0.weights", w["full"], w, 1e-6)  # a stored tensor satisfies its own digest
    assert torch.allclose(directions("time_mlp.0.weights", 4) @ w["full"].double().reshape(-1), w["proj"], rtol=1e-6)
    r = golden["cases"]["d32_random"]
    rd = eto.unpack_digests(r, dm.unet_param_spec(UnetConfig(channels=3, **r["unet_kw"])))
    assert rd["time_mlp.0.weights"]["norm"] == 0.0 and not bool(rd["time_mlp.0.weights"]["full"].any())
