"""GPU tests of ElucidatedDiffusion training on the HIP path (fixture: tests/golden/make_golden_edm_train.py).

Operators: each of the three new passes against the same arithmetic in fp64 on the same inputs, including sigma = 0.002
and sigma = 80 and a batch that is not a multiple of 4.  Bounds from the formats: an fp32 expression of k roundings is
within k * 2^-24 of the exact value per element, so the elementwise outputs (k <= 5) and the loss (double accumulation,
k <= 8) are held to 1e-6 relative; the embedding gradient is a sum over B terms whose two products may cancel, so it is
held to B * 4 * 2^-24 with a factor 8 for cancellation: 1e-5 of the gradient's norm.

Loss and gradients: the reference's own ``forward`` + ``backward()``; the project's tolerances (1e-4 relative on the loss,
2e-4 on every gradient digest, as tests/test_hip_train.py), the limit of a case being max(2e-4, 4 x the reference's stored
fp32-vs-fp64 error on that case) -- with the stored errors (<= 5.1e-6) that is 2e-4 for every case.
Measured errors are written to profiles/edm_train_parity_errors.txt: the file is emptied once per run of this module and
every operator and case check appends its line, so the committed file is one run's record."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import elucidated as E
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import edm_train_oracle as eto
from conftest import ROOT, check_grad_digest, load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL, GRAD_TOL = 1e-4, 2e-4
CASES = ["d32_learned", "d64_learned", "d32_random", "d32_lsd8", "d32_sigma_range", "d32_accumulate2"]
ERRORS = os.path.join(ROOT, "profiles", "edm_train_parity_errors.txt")


def _log(name, err, gate):
    print(f"{name}: {err:.3e} (gate {gate:.0e})")
    with open(ERRORS, "a") as f:
        f.write(f"{name}\t{err:.3e}\tgate {gate:.0e}\n")


@pytest.fixture(scope="module", autouse=True)
def _fresh_error_record():
    """One run, one record: a second run does not duplicate the lines of the first."""
    open(ERRORS, "w").close()


@pytest.fixture(scope="module")
def golden():
    return load_golden("edm_train.pt")


def _fp(t):
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


def _edm(c, **kw):
    cfg = UnetConfig(channels=3, **c["unet_kw"])
    u = dm.Unet(channels=3, device=DEV, **c["unet_kw"])
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=c["salt"]))
    return dm.ElucidatedDiffusion(u, image_size=c["image_size"], **kw), cfg


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ---- operators ----------------------------------------------------------------------------------------------------
SIGMAS5 = torch.tensor([0.002, 0.3, 1.7, 20.0, 80.0])


@pytest.mark.parametrize("B,shape", [(5, (3, 8, 8)), (1, (3, 16, 16)), (7, (1, 2, 2))])
def test_op_noise_in_vs_fp64(B, shape):
    lib = _lib.load()
    g = torch.Generator().manual_seed(31)
    sig = SIGMAS5.repeat(2)[:B].contiguous()
    tab = dm.edm_train_table(sig).contiguous()
    img, eps = torch.rand((B, *shape), generator=g), torch.randn((B, *shape), generator=g)
    per = img[0].numel()
    outs = [torch.empty((B, *shape), device=DEV) for _ in range(3)]
    img_d, eps_d = img.to(DEV), eps.to(DEV)
    _lib.check(lib.dm_op_edm_noise_in(_lib.ptr(img_d), _lib.ptr(eps_d), _fp(tab), B, *[_lib.ptr(o) for o in outs], B, per,
                                      _stream()))
    want = eto.noise_in(img.double(), eps.double(), tab.double())
    for name, got, w in zip(("x0", "noised", "xin"), outs, want):
        err = rel_l2(got.cpu(), w)
        _log(f"op noise_in B={B} {shape} {name} vs fp64", err, 1e-6)
        assert err <= 1e-6
    # per row: the sigma = 0.002 image stays within fp32 rounding of x0, the sigma = 80 image is dominated by the noise
    assert rel_l2(outs[1][0].cpu(), want[1][0]) <= 1e-6 and (B < 5 or rel_l2(outs[1][4].cpu(), want[1][4]) <= 1e-6)


@pytest.mark.parametrize("B,shape,with_D", [(5, (3, 8, 8), True), (3, (3, 32, 32), False), (7, (1, 2, 2), True)])
def test_op_loss_vs_fp64(B, shape, with_D):
    lib = _lib.load()
    g = torch.Generator().manual_seed(32)
    sig = SIGMAS5.repeat(2)[:B].contiguous()
    tab = dm.edm_train_table(sig).contiguous()
    noised, F, x0 = (torch.randn((B, *shape), generator=g) for _ in range(3))
    per = x0[0].numel()
    dF = torch.empty((B, *shape), device=DEV)
    D = torch.empty((B, *shape), device=DEV) if with_D else None
    loss = C.c_float(0.0)
    dev = [v.to(DEV) for v in (noised, F, x0)]
    _lib.check(lib.dm_op_edm_loss(*[_lib.ptr(v) for v in dev], _fp(tab), 0.5, _lib.ptr(dF), _lib.ptr(D), C.byref(loss), B, per,
                                  _stream()))
    wl, wdF, wD = eto.loss_and_dF(noised.double(), F.double(), x0.double(), tab.double(), loss_scale=0.5)
    el, eg = abs(loss.value - float(wl)) / abs(float(wl)), rel_l2(dF.cpu(), wdF)
    _log(f"op loss B={B} {shape} loss vs fp64", el, 1e-6)
    _log(f"op loss B={B} {shape} dF vs fp64", eg, 1e-6)
    assert el <= 1e-6 and eg <= 1e-6
    for b in range(B):  # every image on its own scale: loss_weight spans 4 .. 250000
        assert rel_l2(dF[b].cpu(), wdF[b]) <= 1e-6, b
    if with_D:
        _log(f"op loss B={B} {shape} D vs fp64", rel_l2(D.cpu(), wD), 1e-6)
        assert rel_l2(D.cpu(), wD) <= 1e-6


@pytest.mark.parametrize("B,half", [(5, 8), (6, 4), (1, 8), (64, 8)])
def test_op_sinusoid_ft_bwd_vs_fp64(B, half):
    lib = _lib.load()
    g = torch.Generator().manual_seed(33)
    t = dm.edm_train_table(SIGMAS5.repeat(13)[:B])[:, E.C_NOISE]
    w = torch.randn(half, generator=g)
    a = (t[:, None] * w[None, :]) * (2 * torch.pi)
    e0 = torch.cat((t[:, None], a.sin(), a.cos()), dim=-1).contiguous()
    de0 = torch.randn(e0.shape, generator=g)
    dw = torch.full((half,), 7.0, device=DEV)
    de0_d, e0_d = de0.to(DEV), e0.to(DEV)
    args = (_lib.ptr(de0_d), _lib.ptr(e0_d), _lib.ptr(dw), B, half)
    _lib.check(lib.dm_op_sinusoid_ft_bwd(*args, 1, 0, _stream()))
    want = eto.sinusoid_ft_bwd(de0.double(), e0.double(), half)
    err = rel_l2(dw.cpu(), want)
    _log(f"op sinusoid_ft_bwd B={B} half={half} vs fp64", err, 1e-5)
    assert err <= 1e-5
    _lib.check(lib.dm_op_sinusoid_ft_bwd(*args, 1, 1, _stream()))  # accumulate: twice the gradient
    assert rel_l2(dw.cpu(), 2 * want) <= 1e-5
    _lib.check(lib.dm_op_sinusoid_ft_bwd(*args, 0, 0, _stream()))  # random_fourier_features: exact zeros
    assert not bool(dw.any())


# ---- loss and gradients against the reference ----------------------------------------------------------------------
def _run_case(c, edm):
    total = 0.0
    for i in range(c["micro"]):
        total += float(edm(c["imgs"][i], sigmas=c["sigmas"][i], noise=c["noises"][i], loss_scale=1.0 / c["micro"],
                           accumulate=i > 0))
    return total


@pytest.mark.parametrize("case", CASES)
def test_loss_and_all_gradients_vs_reference_autograd(golden, case):
    c = golden["cases"][case]
    edm, cfg = _edm(c)
    edm.train()
    loss = _run_case(c, edm)
    spec = dm.unet_param_spec(cfg)
    want = eto.unpack_digests(c, spec)
    grads = edm.net.grads()
    assert set(grads) == set(want)
    tol = max(GRAD_TOL, 4 * c["ref_err_grad_max"])
    loss_err = abs(loss - c["loss"]) / abs(c["loss"])
    worst, worst_norm = ("", 0.0), ("", 0.0)
    for name, dg in want.items():
        gcpu = grads[name].cpu()
        if "full" in dg and dg["norm"] > 0:
            worst = max(worst, (name, rel_l2(gcpu, dg["full"])), key=lambda v: v[1])
        if dg["norm"] > 0:
            worst_norm = max(worst_norm, (name, abs(float(gcpu.double().norm()) - dg["norm"]) / dg["norm"]), key=lambda v: v[1])
    _log(f"{case} loss vs reference", loss_err, max(LOSS_TOL, 4 * c["ref_err_loss"]))
    _log(f"{case} worst fully stored gradient ({worst[0]}) vs reference", worst[1], tol)
    _log(f"{case} worst gradient norm ({worst_norm[0]}) vs reference", worst_norm[1], tol)
    _log(f"{case} the reference's own fp32-vs-fp64 worst gradient", c["ref_err_grad_max"], tol)
    assert loss_err <= max(LOSS_TOL, 4 * c["ref_err_loss"])
    for name, dg in want.items():
        check_grad_digest(name, grads[name].cpu(), dg, tol)


def test_time_weights_gradient_learned_and_frozen(golden):
    """time_mlp.0.weights: the learned embedding's gradient is the reference's; the random one's is exact zeros and an
    optimiser step leaves the parameter bit for bit where it was (the reference: requires_grad = False)."""
    name = "time_mlp.0.weights"
    for case in ("d32_learned", "d32_lsd8"):
        c = golden["cases"][case]
        edm, cfg = _edm(c)
        _run_case(c, edm.train())
        dg = eto.unpack_digests(c, dm.unet_param_spec(cfg))[name]
        err = rel_l2(edm.net.grad(name).cpu(), dg["full"])
        _log(f"{case} {name} vs reference", err, GRAD_TOL)
        assert dg["norm"] > 0 and err <= GRAD_TOL
    c = golden["cases"]["d32_random"]
    edm, cfg = _edm(c)
    _run_case(c, edm.train())
    g = edm.net.grad(name)
    assert not bool(g.any()) and g.shape == (8,)
    before = {k: v.clone() for k, v in edm.net.state_dict().items()}
    edm.net.optimizer_step(lr=1e-2)
    after = edm.net.state_dict()
    assert torch.equal(after[name], before[name])
    assert torch.equal(after[name].cpu(), dm.synth_state_dict(dm.unet_param_spec(cfg), salt=c["salt"])[name])
    assert not torch.equal(after["time_mlp.1.weight"], before["time_mlp.1.weight"])
    # a second call that accumulates keeps the zeros
    edm(c["imgs"][0], sigmas=c["sigmas"][0], noise=c["noises"][0], accumulate=True)
    assert not bool(edm.net.grad(name).any())


def test_async_loss_denoised_and_draws(golden):
    c = golden["cases"]["d32_learned"]
    edm, cfg = _edm(c)
    edm.train()
    kw = dict(sigmas=c["sigmas"][0], noise=c["noises"][0])
    a = edm(c["imgs"][0], **kw)
    g1 = edm.net.grads()
    b = edm(c["imgs"][0], sync=False, **kw)
    assert b.device.type == "cuda" and b.dim() == 0 and float(b) == float(a)
    assert all(torch.equal(g1[k], v) for k, v in edm.net.grads().items())
    l3, den = edm(c["imgs"][0], return_denoised=True, **kw)
    assert float(l3) == float(a) and den.shape == c["imgs"][0].shape
    # the returned image is D: the loss recomputed from it in fp64
    x0 = c["imgs"][0].double() * 2 - 1
    per_img = ((den.cpu().double() - x0) ** 2).reshape(x0.shape[0], -1).mean(dim=1)
    want = float((per_img * dm.edm_train_table(c["sigmas"][0])[:, E.LOSS_W].double()).mean())
    assert abs(float(a) - want) <= 1e-5 * want
    # without injection: sigma from torch's global CPU generator first, the noise from the device Philox stream
    torch.manual_seed(5)
    l1 = float(edm(c["imgs"][0]))
    torch.manual_seed(5)
    l2 = float(edm(c["imgs"][0]))
    assert l1 == l2 and 0.0 < l1 < 100.0
    calls = []
    real_sig, real_randn = edm._draw_sigmas, edm._randn
    edm._draw_sigmas = lambda n: calls.append("sigma") or real_sig(n)
    edm._randn = lambda *a_, **k_: calls.append("noise") or real_randn(*a_, **k_)
    edm(c["imgs"][0])
    assert calls == ["sigma", "noise"]


def _smooth_images(n=8):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 16), torch.linspace(0, 1, 16), indexing="ij")
    g = torch.Generator().manual_seed(3)
    return torch.stack([torch.stack([(yy * a + xx * (1 - a)), (yy * xx) ** b, (1 - yy) * a]) for a, b in
                        zip(torch.rand(n, generator=g).tolist(), (torch.rand(n, generator=g) + 0.5).tolist())]).float()


def test_training_lowers_the_loss_then_the_handle_samples(golden):
    c = golden["cases"]["d32_learned"]
    edm, cfg = _edm(c, num_sample_steps=6)
    edm.train()
    imgs = _smooth_images()
    g = torch.Generator().manual_seed(4)
    sig = (-1.2 + 1.2 * torch.randn(8, generator=g)).exp()
    noise = torch.randn(imgs.shape, generator=g)
    ema = dm.EMA(edm, beta=0.99, update_every=2, update_after_step=4)
    losses = [dm.train_step(edm, [imgs], lr=1e-3, ema=ema, sigmas=[sig], noise=[noise])[0] for _ in range(40)]
    print("EDM loss", losses[0], "->", losses[-1])
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    with pytest.raises(RuntimeError, match="dm_unet_train_sync"):
        edm.sample(batch_size=2, noise=so.NoiseStream(8))
    edm.net.sync()
    a = edm.sample(batch_size=2, noise=so.NoiseStream(8))
    fresh = dm.Unet(channels=3, device=DEV, **c["unet_kw"])
    fresh.load_state_dict(edm.net.state_dict())
    assert [k for k in edm.state_dict()] == ["net." + n for n, _ in dm.unet_param_spec(cfg)]
    b = dm.ElucidatedDiffusion(fresh, image_size=16, num_sample_steps=6).sample(batch_size=2, noise=so.NoiseStream(8))
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    e = ema.ema_model.sample_using_dpmpp(batch_size=2, noise=so.NoiseStream(8))
    assert e.shape == a.shape and bool(torch.isfinite(e).all())
    assert ema.ema_model.net.cfg.learned_sinusoidal_cond and ema.ema_model.net is not edm.net


def test_checkpoint_round_trip_continues_bit_for_bit(golden, tmp_path):
    c = golden["cases"]["d32_lsd8"]
    g = torch.Generator().manual_seed(12)
    batches = [torch.rand((4, 3, 16, 16), generator=g) for _ in range(3)]
    sigs = [(-1.2 + 1.2 * torch.randn(4, generator=g)).exp() for _ in range(3)]
    noises = [torch.randn((4, 3, 16, 16), generator=g) for _ in range(3)]

    def fresh():
        edm, _ = _edm(c)
        return edm.train(), dm.EMA(edm, beta=0.995, update_every=1, update_after_step=0)

    def step(edm, ema, s):
        return dm.train_step(edm, [batches[s]], lr=1e-3, ema=ema, sigmas=[sigs[s]], noise=[noises[s]])

    d, ema = fresh()
    for s in range(2):
        step(d, ema, s)
    path = tmp_path / "edm-1.pt"
    dm.save_checkpoint(path, d, step=2, ema=ema, lr=1e-3)
    data = torch.load(str(path), map_location="cpu", weights_only=True)
    names = [n for n, _ in d.net.param_spec()]
    assert list(data["model"]) == ["net." + n for n in names]  # the reference module has no buffers
    assert "ema_model.net." + names[0] in data["ema"] and "online_model.net." + names[0] in data["ema"]
    step(d, ema, 2)
    d2, ema2 = fresh()
    at, hyper = dm.load_checkpoint(path, d2, ema=ema2)
    assert at == 2 and abs(hyper["lr"] - 1e-3) < 1e-12 and ema2.step == 2
    step(d2, ema2, 2)
    for which, a, b in (("param", d.net.state_dict(), d2.net.state_dict()),
                        ("ema", d.net.state_dict(ema=True), d2.net.state_dict(ema=True)),
                        ("exp_avg", d.net._train_tensors(2), d2.net._train_tensors(2)),
                        ("exp_avg_sq", d.net._train_tensors(3), d2.net._train_tensors(3))):
        diff = [k for k in a if not torch.equal(a[k], b[k])]
        assert not diff, (which, diff[:3])
    assert d2.net._lib.dm_unet_adam_step(d2.net._handle, -1) == 3


CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["DM_ROOT"])
import torch
import torch.distributed as dist
import diffusion_models_amd as dm
from diffusion_models_amd.spec import UnetConfig

torch.cuda.set_device(0)
kw = dict(dim=64, dim_mults=(1, 2), learned_sinusoidal_cond=True)
sd = dm.synth_state_dict(dm.unet_param_spec(UnetConfig(channels=3, **kw)), salt=71)
def model():
    u = dm.Unet(channels=3, device="cuda:0", **kw)
    u.load_state_dict(sd)
    return dm.ElucidatedDiffusion(u, image_size=16).train()
g = torch.Generator().manual_seed(7)
img = torch.rand((6, 3, 16, 16), generator=g)
sig = (-1.2 + 1.2 * torch.randn(6, generator=g)).exp()
nz = torch.randn((6, 3, 16, 16), generator=g)
ref = model()
want_loss, want_norm = dm.train_step(ref, [img], lr=1e-3, sigmas=[sig], noise=[nz])
want = ref.net.state_dict()
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
try:
    d = model()
    bucketed = os.environ.get("DM_TEST_BUCKETED") == "1"
    if bucketed:
        assert len(d.net.grad_buckets()) >= 2, d.net.grad_buckets()  # DM_TRAIN_BUCKET_MB=1: several buckets on this net
    loss, norm = dm.train_step(d, [img], lr=1e-3, sigmas=[sig], noise=[nz], bucketed=bucketed)
    assert d.net._bucketed == bucketed
    got = d.net.state_dict()
    assert loss == want_loss and norm == want_norm, (loss, want_loss, norm, want_norm)
    bad = [k for k in want if not torch.equal(got[k], want[k])]
    assert not bad, bad[:3]
    print("EDM_DP_OK")
finally:
    dist.destroy_process_group()
"""


@pytest.mark.parametrize("bucketed", [False, True])
def test_train_step_under_a_world_size_1_process_group_is_the_same_step(bucketed):
    """Also with the gradient buffer all-reduced bucket by bucket on a second stream (1 MB buckets: the last bucket's event
    follows the embedding's backward launches)."""
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, DM_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1",
               LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if bucketed:
        env.update(DM_TEST_BUCKETED="1", DM_TRAIN_BUCKET_MB="1")
    p = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "EDM_DP_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]


def test_plain_unet_training_is_untouched_by_an_edm_call(golden):
    """p_losses of a plain U-Net before and after an EDM training call on another handle: the same gradients bit for bit
    and the same kernels launched the same number of times (the integer-time path issues what it always issued)."""
    cfg = UnetConfig(dim=32, dim_mults=(1, 2), channels=3)
    u = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=41))
    d = dm.DenoisingDiffusion(u, image_size=16, timesteps=1000).train()
    g = torch.Generator().manual_seed(14)
    x = torch.rand((4, 3, 16, 16), generator=g) * 2 - 1
    t, nz = torch.tensor([3, 250, 600, 999]), torch.randn((4, 3, 16, 16), generator=g)

    def launches():
        float(d.p_losses(x, t, noise=nz))  # (warm: the workspace dry run and first-use packs are not part of the list)
        _lib.profile_enable(True)
        try:
            _lib.profile_read()
            loss = float(d.p_losses(x, t, noise=nz))
            rows = _lib.profile_read()
        finally:
            _lib.profile_enable(False)
        return loss, {k: v.clone() for k, v in d.model.grads().items()}, sorted((r["kernel"], r["launches"]) for r in rows)

    l1, g1, k1 = launches()
    c = golden["cases"]["d32_learned"]
    edm, _ = _edm(c)
    _run_case(c, edm.train())
    edm.net.optimizer_step(lr=1e-3)
    l2, g2, k2 = launches()
    assert l1 == l2 and k1 == k2 and len(k1) > 5
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    assert not any("edm" in name or "sinusoid_ft" in name for name, _ in k1)


def test_integer_time_entries_still_refuse(golden):
    c = golden["cases"]["d32_learned"]
    edm, cfg = _edm(c)
    lib = _lib.load()
    with pytest.raises(RuntimeError):
        edm.net.train()
    with pytest.raises(AssertionError):
        dm.DenoisingDiffusion(edm.net, image_size=16)
    edm.train()
    with pytest.raises(RuntimeError):  # still, on an armed handle
        edm.net.train()
    # the integer-time loss entries refuse a handle armed for float time
    x = torch.zeros((2, 3, 16, 16), device=DEV)
    t_arr = (C.c_int64 * 2)(1, 2)
    coef = torch.zeros((2, 8))
    loss = C.c_float(0.0)
    rc = lib.dm_unet_loss_backward(edm.net._handle, _lib.ptr(x), t_arr, _fp(coef), _lib.ptr(x), None, None, 0, None, 0, 0, 0,
                                   1.0, 0, C.byref(loss), None, 2, 16, 16, _stream())
    assert rc != 0 and b"dm_unet_loss_backward_edm" in lib.dm_last_error()
    a = _lib.TrainArgs()
    a.x_start, a.noise, a.t_host, a.coef_host, a.coef_stride = _lib.ptr(x), _lib.ptr(x), C.cast(t_arr, C.POINTER(C.c_int64)), _fp(coef), 8
    a.loss_scale, a.B, a.H, a.W, a.loss_terms, a.stream = 1.0, 2, 16, 16, 1, _stream()
    assert lib.dm_unet_loss_backward_ex(edm.net._handle, C.byref(a)) != 0
    mask = (C.c_int32 * 2)(1, 0)
    assert lib.dm_unet_loss_backward_masked(edm.net._handle, C.byref(a), mask) != 0
    # and the float-time entries refuse every other U-Net
    plain = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    plain.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(dim=32, dim_mults=(1, 2), channels=3)), salt=41))
    assert lib.dm_unet_train_enable_ft(plain._handle, 0) != 0
    plain.train()
    e = _lib.EdmTrainArgs()
    tab = dm.edm_train_table(torch.tensor([0.5, 1.0])).contiguous()
    e.images, e.noise, e.coef_host, e.coef_stride = _lib.ptr(x), _lib.ptr(x), _fp(tab), E.COLS
    e.loss_scale, e.B, e.H, e.W, e.stream = 1.0, 2, 16, 16, _stream()
    assert lib.dm_unet_loss_backward_edm(plain._handle, C.byref(e)) != 0
    assert b"dm_unet_train_enable_ft" in lib.dm_last_error()
    with pytest.raises(NotImplementedError, match="train"):  # a net that is not a library Unet, now with a GPU present
        _refuse_stub()


def _refuse_stub():
    import types

    stub = types.SimpleNamespace(random_or_learned_sinusoidal_cond=True, self_condition=False, text_condition=False,
                                 out_dim=3, channels=3, cfg=types.SimpleNamespace(cond_channels=0), device=DEV,
                                 downsample_factor=2)
    dm.ElucidatedDiffusion(stub, image_size=16)(torch.zeros(1, 3, 16, 16))
