"""GPU tests of continuous-time Gaussian diffusion training on the HIP path (fixture: tests/golden/make_golden_ct.py).

Loss and gradients against the reference's own ``p_losses(...).backward()``: the tolerances of tests/test_hip_edm_train.py --
1e-4 relative on the loss, every gradient digest within max(2e-4, 4 x the reference's stored fp32-vs-fp64 error of the
case).  Then a short training run, the checkpoint round trip, and the other training paths left as they were.
Measured errors are printed (run with -s to see them)."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import continuous as K
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import edm_train_oracle as eto
from conftest import check_grad_digest, load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL, GRAD_TOL = 1e-4, 2e-4
CASES = ["noise_lin", "noise_cos_minsnr", "v_learned", "v_random", "noise_lin_accumulate2"]
CLASSES = {"noise": dm.ContinuousTimeGaussianDiffusion, "v": dm.VParamContinuousTimeGaussianDiffusion}
NAME = "time_mlp.0.weights"


@pytest.fixture(scope="module")
def golden():
    return load_golden("ct.pt")


def _fp(t):
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _obj(c, **kw):
    cfg = UnetConfig(channels=3, **c["unet_kw"])
    u = dm.Unet(channels=3, device=DEV, **c["unet_kw"])
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=c["salt"]))
    return CLASSES[c["kind"]](u, image_size=c["image_size"], **c["ct_kw"], **kw), cfg


def _run_case(c, obj):
    total = 0.0
    for i in range(c["micro"]):
        total += float(obj(c["imgs"][i], times=c["times"][i], noise=c["noises"][i], loss_scale=1.0 / c["micro"],
                           accumulate=i > 0))
    return total


@pytest.mark.parametrize("case", CASES)
def test_loss_and_all_gradients_vs_reference_autograd(golden, case):
    c = golden["train"][case]
    assert c["micro"] == (2 if case.endswith("accumulate2") else 1)
    obj, cfg = _obj(c)
    obj.train()
    loss = _run_case(c, obj)
    spec = dm.unet_param_spec(cfg)
    want = eto.unpack_digests(c, spec)
    grads = obj.model.grads()
    assert set(grads) == set(want)
    tol = max(GRAD_TOL, 4 * c["ref_err_grad_max"])
    loss_err = abs(loss - c["loss"]) / abs(c["loss"])
    worst = ("", 0.0)
    for name, dg in want.items():
        if dg["norm"] > 0:
            worst = max(worst, (name, abs(float(grads[name].double().norm()) - dg["norm"]) / dg["norm"]), key=lambda v: v[1])
    print(f"{case}: loss vs reference {loss_err:.3e} (gate {LOSS_TOL:.0e}); worst gradient norm ({worst[0]}) {worst[1]:.3e} "
          f"(gate {tol:.1e}); the reference's own fp32-vs-fp64 worst gradient {c['ref_err_grad_max']:.3e}")
    assert loss_err <= LOSS_TOL
    for name, dg in want.items():
        check_grad_digest(name, grads[name].cpu(), dg, tol)
    # the embedding's weights: a gradient when learned, exact zeros when random (requires_grad = False in the reference)
    g = grads[NAME]
    if c["unet_kw"].get("random_fourier_features"):
        assert c["frozen"] == [NAME] and not bool(g.any())
    else:
        assert c["frozen"] == [] and want[NAME]["norm"] > 0
        assert rel_l2(g.cpu(), want[NAME]["full"]) <= tol


def test_p_losses_on_normalised_images_is_forward_and_the_async_form(golden):
    c = golden["train"]["v_learned"]
    obj, _ = _obj(c)
    obj.train()
    kw = dict(times=c["times"][0], noise=c["noises"][0])
    a = obj(c["imgs"][0], **kw)
    g1 = {k: v.clone() for k, v in obj.model.grads().items()}
    b = obj.p_losses(c["imgs"][0] * 2 - 1, c["times"][0], noise=c["noises"][0])
    assert float(a) == float(b) and all(torch.equal(g1[k], v) for k, v in obj.model.grads().items())
    d = obj(c["imgs"][0], sync=False, **kw)
    assert d.device.type == "cuda" and d.dim() == 0 and float(d) == float(a)
    # without injection: times from torch's global CPU generator first, the noise from the device Philox stream
    torch.manual_seed(5)
    l1 = float(obj(c["imgs"][0]))
    torch.manual_seed(5)
    assert float(obj(c["imgs"][0])) == l1 and 0.0 < l1 < 100.0


def _smooth_images(n=8):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 16), torch.linspace(0, 1, 16), indexing="ij")
    g = torch.Generator().manual_seed(3)
    return torch.stack([torch.stack([(yy * a + xx * (1 - a)), (yy * xx) ** b, (1 - yy) * a]) for a, b in
                        zip(torch.rand(n, generator=g).tolist(), (torch.rand(n, generator=g) + 0.5).tolist())]).float()


@pytest.mark.parametrize("case", ["v_learned", "noise_lin"])
def test_training_lowers_the_loss_then_the_handle_samples(golden, case):
    c = golden["train"][case]
    obj, cfg = _obj(c, num_sample_steps=6)
    obj.train()
    imgs = _smooth_images()
    g = torch.Generator().manual_seed(4)
    times = 0.02 + 0.96 * torch.rand(8, generator=g)
    noise = torch.randn(imgs.shape, generator=g)
    ema = dm.EMA(obj, beta=0.99, update_every=2, update_after_step=4)
    losses = [dm.train_step(obj, [imgs], lr=1e-3, ema=ema, times=[times], noise=[noise])[0] for _ in range(40)]
    print(case, "loss", losses[0], "->", losses[-1])
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    with pytest.raises(RuntimeError, match="dm_unet_train_sync"):
        obj.sample(batch_size=2, noise=so.NoiseStream(8))
    obj.model.sync()
    a = obj.sample(batch_size=2, noise=so.NoiseStream(8))
    fresh = dm.Unet(channels=3, device=DEV, **c["unet_kw"])
    fresh.load_state_dict(obj.model.state_dict())
    assert [k for k in obj.state_dict()] == ["model." + n for n, _ in dm.unet_param_spec(cfg)]
    b = CLASSES[c["kind"]](fresh, image_size=16, num_sample_steps=6, **c["ct_kw"]).sample(batch_size=2, noise=so.NoiseStream(8))
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    e = ema.ema_model.sample(batch_size=2, noise=so.NoiseStream(8))
    assert e.shape == a.shape and bool(torch.isfinite(e).all())
    assert ema.ema_model.model.cfg.learned_sinusoidal_cond and ema.ema_model.model is not obj.model


def test_checkpoint_round_trip_continues_bit_for_bit(golden, tmp_path):
    c = golden["train"]["noise_cos_minsnr"]
    g = torch.Generator().manual_seed(12)
    batches = [torch.rand((4, 3, 16, 16), generator=g) for _ in range(3)]
    times = [torch.rand(4, generator=g) for _ in range(3)]
    noises = [torch.randn((4, 3, 16, 16), generator=g) for _ in range(3)]

    def fresh():
        obj, _ = _obj(c)
        return obj.train(), dm.EMA(obj, beta=0.995, update_every=1, update_after_step=0)

    def step(obj, ema, s):
        return dm.train_step(obj, [batches[s]], lr=1e-3, ema=ema, times=[times[s]], noise=[noises[s]])

    d, ema = fresh()
    for s in range(2):
        step(d, ema, s)
    path = tmp_path / "ct-1.pt"
    dm.save_checkpoint(path, d, step=2, ema=ema, lr=1e-3)
    data = torch.load(str(path), map_location="cpu", weights_only=True)
    names = [n for n, _ in d.model.param_spec()]
    assert list(data["model"]) == ["model." + n for n in names]  # the reference module has no buffers
    assert "ema_model.model." + names[0] in data["ema"] and "online_model.model." + names[0] in data["ema"]
    step(d, ema, 2)
    d2, ema2 = fresh()
    at, hyper = dm.load_checkpoint(path, d2, ema=ema2)
    assert at == 2 and abs(hyper["lr"] - 1e-3) < 1e-12 and ema2.step == 2
    step(d2, ema2, 2)
    for which, a, b in (("param", d.model.state_dict(), d2.model.state_dict()),
                        ("ema", d.model.state_dict(ema=True), d2.model.state_dict(ema=True)),
                        ("exp_avg", d.model._train_tensors(2), d2.model._train_tensors(2)),
                        ("exp_avg_sq", d.model._train_tensors(3), d2.model._train_tensors(3))):
        diff = [k for k in a if not torch.equal(a[k], b[k])]
        assert not diff, (which, diff[:3])


def test_other_paths_are_untouched_and_an_unarmed_handle_is_refused(golden):
    """An EDM training call and an integer-time DDPM call on other handles give the same loss and gradients bit for bit
    before and after a continuous-time call; a handle that dm_unet_train_enable_ft has not armed is refused by name."""
    edm_c = load_golden("edm_train.pt")["cases"]["d32_learned"]
    ecfg = UnetConfig(channels=3, **edm_c["unet_kw"])
    eu = dm.Unet(channels=3, device=DEV, **edm_c["unet_kw"])
    eu.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(ecfg), salt=edm_c["salt"]))
    edm = dm.ElucidatedDiffusion(eu, image_size=16).train()
    pcfg = UnetConfig(dim=32, dim_mults=(1, 2), channels=3)
    pu = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    pu.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(pcfg), salt=41))
    ddpm = dm.DenoisingDiffusion(pu, image_size=16, timesteps=1000).train()
    g = torch.Generator().manual_seed(14)
    x = torch.rand((4, 3, 16, 16), generator=g) * 2 - 1
    t, nz = torch.tensor([3, 250, 600, 999]), torch.randn((4, 3, 16, 16), generator=g)

    def both():
        le = float(edm(edm_c["imgs"][0], sigmas=edm_c["sigmas"][0], noise=edm_c["noises"][0]))
        ge = {k: v.clone() for k, v in eu.grads().items()}
        lp = float(ddpm.p_losses(x, t, noise=nz))
        gp = {k: v.clone() for k, v in pu.grads().items()}
        return le, ge, lp, gp

    le1, ge1, lp1, gp1 = both()
    c = golden["train"]["noise_cos_minsnr"]
    obj, _ = _obj(c)
    _run_case(c, obj.train())
    obj.model.optimizer_step(lr=1e-3)
    le2, ge2, lp2, gp2 = both()
    assert le1 == le2 and lp1 == lp2
    assert all(torch.equal(ge1[k], ge2[k]) for k in ge1) and all(torch.equal(gp1[k], gp2[k]) for k in gp1)
    # the EDM-armed handle also takes a continuous-time call (the same arming), and goes back to EDM unchanged
    v = dm.VParamContinuousTimeGaussianDiffusion(eu, image_size=16)
    assert float(v(c["imgs"][0], times=c["times"][0], noise=c["noises"][0])) > 0
    le3 = float(edm(edm_c["imgs"][0], sigmas=edm_c["sigmas"][0], noise=edm_c["noises"][0]))
    assert le3 == le1 and all(torch.equal(ge1[k], v_) for k, v_ in eu.grads().items())
    # not armed: refused with a message that names the call that arms
    lib = _lib.load()
    fresh, _ = _obj(c)
    xz = torch.zeros((2, 3, 16, 16), device=DEV)
    tab = dm.ct_train_table(torch.tensor([0.3, 0.6]), "cosine").contiguous()
    a = _lib.CtTrainArgs()
    a.images, a.noise, a.coef_host, a.coef_stride = _lib.ptr(xz), _lib.ptr(xz), _fp(tab), K.COLS
    a.objective, a.loss_scale, a.B, a.H, a.W, a.normalize, a.stream = 0, 1.0, 2, 16, 16, 1, _stream()
    assert lib.dm_unet_loss_backward_ct(fresh.model._handle, C.byref(a)) != 0
    assert b"dm_unet_train_enable_ft" in lib.dm_last_error()
    assert lib.dm_unet_loss_backward_ct(pu._handle, C.byref(a)) != 0  # armed for integer time only
    assert b"dm_unet_train_enable_ft" in lib.dm_last_error()
    # and sampling refuses a U-Net without the float-time embedding
    s = _lib.CtArgs()
    step_tab = dm.ct_step_table(2, "cosine").contiguous()
    out = torch.empty_like(xz)
    s.objective, s.clip, s.n_steps, s.table_host, s.x_init, s.out = 1, 1, 2, _fp(step_tab), _lib.ptr(xz), _lib.ptr(out)
    s.B, s.H, s.W, s.use_graph, s.stream = 2, 16, 16, 0, _stream()
    assert lib.dm_sample_ct(pu._handle, C.byref(s)) != 0
    with pytest.raises(AssertionError):
        dm.ContinuousTimeGaussianDiffusion(pu, image_size=16)
