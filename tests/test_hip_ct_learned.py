"""GPU tests of the learned noise schedule and of the U-Net's input gradients on the HIP path (fixture:
tests/golden/make_golden_ct_learned.py).

* Input gradients alone: ``p_losses_input_grads`` of a linear-schedule and of a v / cosine object against fp64 autograd of the
  oracle U-Net, gate max(2e-4, 4 x the error of the same restatement in fp32); loss and parameter gradients of that call are
  bit for bit those of a plain ``p_losses`` on a fresh handle.
* Reference parity, every fixture case: loss within 1e-4; the U-Net gradient digests and the six schedule gradients within
  max(2e-4, 4 x the case's recorded fp32-vs-fp64 error) -- the gates of tests/test_hip_ct_train.py; a schedule gradient's
  error is relative to the norm of all six, the measure the fixture records (the last bias cancels in the normalisation: its
  own gradient is rounding noise around zero).
* The N = 8 sample within 1e-4 rel-L2 of the recording, graph and eager.
* A few ``train_step``s, the EMA's own schedule, the checkpoint round trip, and the plain entry left as it was.
Measured errors are printed (run with -s to see them)."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import continuous as K
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import ct_learned_oracle as lo
import ct_oracle as co
import edm_train_oracle as eto
from conftest import check_grad_digest, load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_TOL, GRAD_TOL, SAMPLE_TOL = 1e-4, 2e-4, 1e-4
CASES = ["learned", "learned_h1024", "learned_minsnr", "learned_frac025", "learned_rff", "learned_accumulate2"]
NAME = "time_mlp.0.weights"
D32 = dict(dim=32, dim_mults=(1, 2), learned_sinusoidal_cond=True)


@pytest.fixture(scope="module")
def golden():
    return load_golden("ct_learned.pt")


def _unet(ukw, salt):
    cfg = UnetConfig(channels=3, **ukw)
    u = dm.Unet(channels=3, device=DEV, **ukw)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt)
    u.load_state_dict(sd)
    return u, cfg, sd


def _obj(c, **kw):
    u, cfg, _ = _unet(c["unet_kw"], c["salt"])
    obj = dm.ContinuousTimeGaussianDiffusion(u, image_size=c["image_size"], noise_schedule="learned", **c["ct_kw"], **kw)
    obj.log_snr.load_state_dict(c["sched"])
    return obj, cfg


def _run_case(c, obj):
    total = 0.0
    for i in range(c["micro"]):
        total += float(obj(c["imgs"][i], times=c["times"][i], noise=c["noises"][i], loss_scale=1.0 / c["micro"], accumulate=i > 0))
    return total


@pytest.mark.parametrize("kind", ["noise_linear", "v_cosine"])
def test_input_gradients_vs_fp64_autograd_and_the_plain_call_unchanged(kind):
    cls, objective, sched = ((dm.ContinuousTimeGaussianDiffusion, co.NOISE, "linear") if kind == "noise_linear" else
                             (dm.VParamContinuousTimeGaussianDiffusion, co.V, "cosine"))
    g = torch.Generator().manual_seed(21)
    x0 = torch.rand((4, 3, 16, 16), generator=g) * 2 - 1
    times = torch.tensor([0.05, 0.3, 0.6, 0.9])
    noise = torch.randn((4, 3, 16, 16), generator=g)
    u, cfg, sd = _unet(D32, 55)
    obj = cls(u, image_size=16).train()
    loss, dx, dt = obj.p_losses_input_grads(x0, times, noise=noise)
    assert dx.shape == x0.shape and dt.shape == (4,) and dx.is_cuda and dt.is_cuda
    grads = {k: v.clone() for k, v in u.grads().items()}
    tab = dm.ct_train_table(times, sched)
    want = lo.input_grads(sd, cfg, x0, noise, tab, objective, False, torch.float64)
    restated = lo.input_grads(sd, cfg, x0, noise, tab, objective, False, torch.float32)
    for name, got, key in (("dL/dx", dx, "dx"), ("dL/dtime", dt, "dtime")):
        err, own = rel_l2(got, want[key]), rel_l2(restated[key], want[key])
        tol = max(GRAD_TOL, 4 * own)
        print(f"{kind} {name}: vs fp64 autograd {err:.3e} (gate {tol:.1e}); the fp32 restatement {own:.3e}")
        assert err <= tol and float(want[key].norm()) > 0
    assert abs(float(loss) - float(want["loss"])) <= LOSS_TOL * abs(float(want["loss"]))
    # the same inputs through the plain entry on a fresh handle: loss and every parameter gradient bit for bit
    u2, _, _ = _unet(D32, 55)
    plain = cls(u2, image_size=16).train()
    loss2 = plain.p_losses(x0, times, noise=noise)
    assert float(loss) == float(loss2)
    diff = [k for k, v in u2.grads().items() if not torch.equal(v, grads[k])]
    assert not diff, diff[:3]
    # forward on [0, 1] images is p_losses on the normalised ones
    l3, dx3, dt3 = obj.forward_input_grads((x0 + 1) / 2, times=times, noise=noise)
    assert rel_l2(dx3, dx) <= 1e-5 and rel_l2(dt3, dt) <= 1e-5


@pytest.mark.parametrize("case", CASES)
def test_loss_and_all_gradients_vs_reference_autograd(golden, case):
    c = golden["cases"][case]
    assert c["micro"] == (2 if case.endswith("accumulate2") else 1)
    obj, cfg = _obj(c)
    obj.train()
    loss = _run_case(c, obj)
    spec = dm.unet_param_spec(cfg)
    want = eto.unpack_digests(c, spec)
    grads = obj.model.grads()
    tol = max(GRAD_TOL, 4 * c["ref_err_grad_max"])
    loss_err = abs(loss - c["loss"]) / abs(c["loss"])
    worst = ("", 0.0)
    for name, dg in want.items():
        if dg["norm"] > 0:
            worst = max(worst, (name, abs(float(grads[name].double().norm()) - dg["norm"]) / dg["norm"]), key=lambda v: v[1])
    snorm = torch.cat([v.reshape(-1) for v in c["sched_grads64"].values()]).norm()
    stol = max(GRAD_TOL, 4 * c["ref_err_sched_grad_max"])
    sgot = dict(obj.log_snr.named_parameters())
    serr = {k: float((sgot[k].grad.double() - v.double()).norm() / snorm) for k, v in c["sched_grads"].items()}
    print(f"{case}: loss vs reference {loss_err:.3e} (gate {LOSS_TOL:.0e}); worst U-Net gradient norm ({worst[0]}) {worst[1]:.3e} "
          f"(gate {tol:.1e}; reference fp32-vs-fp64 {c['ref_err_grad_max']:.3e}); worst schedule gradient "
          f"{max(serr.values()):.3e} (gate {stol:.1e}; reference fp32-vs-fp64 {c['ref_err_sched_grad_max']:.3e})")
    assert loss_err <= LOSS_TOL
    for name, dg in want.items():
        check_grad_digest(name, grads[name].cpu(), dg, tol)
    assert max(serr.values()) <= stol, serr
    assert float(snorm) > 0 and all(p.grad is not None for p in sgot.values())
    if case == "learned_rff":  # frozen embedding weights: exact zeros there, and the schedule still gets its gradient
        assert c["frozen"] == [NAME] and not bool(grads[NAME].any())
        assert float(torch.cat([p.grad.reshape(-1) for p in sgot.values()]).norm()) > 0
    else:
        assert c["frozen"] == [] and want[NAME]["norm"] > 0
    if case == "learned_frac025":  # the same case at frac_gradient 1: the U-Net's gradients as they were, the schedule's 4 x
        full, _ = _obj(golden["cases"]["learned"])
        full.train()
        _run_case(golden["cases"]["learned"], full)
        for k, p in full.log_snr.named_parameters():
            assert torch.allclose(sgot[k].grad, 0.25 * p.grad, rtol=1e-5, atol=1e-7 * float(snorm)), k
        assert all(torch.equal(v, grads[k]) for k, v in full.model.grads().items())


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("case", ["learned", "learned_h1024", "learned_minsnr"])
def test_sample_vs_reference(golden, case, use_graph):
    c = golden["cases"][case]
    obj, _ = _obj(c, num_sample_steps=c["n"], use_graph=use_graph)
    y = obj.sample(batch_size=2, noise=so.NoiseStream(c["sample_noise_seed"]))
    err = rel_l2(y, c["sample"])
    print(f"{case} N={c['n']} {'graph' if use_graph else 'eager'}: sample vs reference {err:.3e} (gate {SAMPLE_TOL:.0e}); on the "
          f"final clamp {c['clamp_share']:.3f}")
    assert err <= SAMPLE_TOL and c["clamp_share"] <= 0.5
    # the other sampling entries run on the module too
    x = torch.randn((2, 3, 16, 16), generator=torch.Generator().manual_seed(1))
    mean, var = obj.p_mean_variance(x, 0.5, 0.375)
    assert bool(torch.isfinite(mean).all()) and float(var) > 0
    xq, log_snr = obj.q_sample(x.clamp(-1, 1), torch.tensor([0.2, 0.7]), noise=x)
    with torch.no_grad():
        assert torch.equal(log_snr.cpu(), obj.log_snr(torch.tensor([0.2, 0.7])))


def _smooth_images(n=8):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 16), torch.linspace(0, 1, 16), indexing="ij")
    g = torch.Generator().manual_seed(3)
    return torch.stack([torch.stack([(yy * a + xx * (1 - a)), (yy * xx) ** b, (1 - yy) * a]) for a, b in
                        zip(torch.rand(n, generator=g).tolist(), (torch.rand(n, generator=g) + 0.5).tolist())]).float()


def test_training_moves_the_schedule_and_the_ema_keeps_its_own(golden):
    c = golden["cases"]["learned"]
    obj, cfg = _obj(c, num_sample_steps=6)
    obj.train()
    imgs = _smooth_images()
    g = torch.Generator().manual_seed(4)
    times = 0.02 + 0.96 * torch.rand(8, generator=g)
    noise = torch.randn(imgs.shape, generator=g)
    before = [p.detach().clone() for p in obj.log_snr.parameters()]
    ema = dm.EMA(obj, beta=0.99, update_every=2, update_after_step=4)
    out = [dm.train_step(obj, [imgs], lr=1e-3, ema=ema, times=[times], noise=[noise]) for _ in range(40)]
    losses = [o[0] for o in out]
    print("learned: loss", losses[0], "->", losses[-1], "combined gradient norm of the first step", out[0][1])
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    after = list(obj.log_snr.parameters())
    assert sum(not torch.equal(a, b) for a, b in zip(after, before)) >= 5  # (the last bias has a zero gradient)
    assert [k for k in obj.state_dict()] == c["state_dict_keys"] and len(list(obj.parameters())) == len(c["parameter_names"])
    # the EMA's own schedule: the averages, neither the online module nor its values
    em = ema.ema_model
    assert em.log_snr is not obj.log_snr and isinstance(em.log_snr, K.learned_noise_schedule)
    avg = list(em.log_snr.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(avg, after)) and any(not torch.equal(a, b) for a, b in zip(avg, before))
    e1 = em.sample(batch_size=2, noise=so.NoiseStream(8))
    saved = [p.detach().clone() for p in after]
    with torch.no_grad():
        for p in after:
            p.mul_(1.5)
    e2 = ema.ema_model.sample(batch_size=2, noise=so.NoiseStream(8))
    assert torch.equal(e1, e2) and bool(torch.isfinite(e1).all())  # changing the online schedule does not reach it
    with torch.no_grad():
        for p, v in zip(after, saved):
            p.copy_(v)
    sd = ema.state_dict()
    for k in c["sched"]:
        assert torch.equal(sd["ema_model.log_snr." + k], dict(em.log_snr.state_dict())[k])
        assert torch.equal(sd["online_model.log_snr." + k], dict(obj.log_snr.state_dict())[k])
    # one shared clip: the combined norm is the root of the two squared norms
    obj(imgs, times=times, noise=noise)
    unet_sq = float(obj.model.grads_flat().double().pow(2).sum())
    sched_sq = float(sum(p.grad.double().pow(2).sum() for p in obj.log_snr.parameters()))
    norm = obj.model.optimizer_step(lr=0.0, extra_sq_norm=sched_sq)
    assert abs(norm - (unet_sq + sched_sq) ** 0.5) <= 1e-5 * norm and sched_sq > 0


def test_checkpoint_round_trip_continues_bit_for_bit(golden, tmp_path):
    c = golden["cases"]["learned_minsnr"]
    g = torch.Generator().manual_seed(12)
    batches = [torch.rand((4, 3, 16, 16), generator=g) for _ in range(3)]
    times = [0.05 + 0.6 * torch.rand(4, generator=g) for _ in range(3)]
    noises = [torch.randn((4, 3, 16, 16), generator=g) for _ in range(3)]

    def fresh():
        obj, _ = _obj(c)
        return obj.train(), dm.EMA(obj, beta=0.995, update_every=1, update_after_step=0)

    def step(obj, ema, s):
        return dm.train_step(obj, [batches[s]], lr=1e-3, ema=ema, times=[times[s]], noise=[noises[s]])

    d, ema = fresh()
    for s in range(2):
        step(d, ema, s)
    path = tmp_path / "ct-learned.pt"
    dm.save_checkpoint(path, d, step=2, ema=ema, lr=1e-3)
    data = torch.load(str(path), map_location="cpu", weights_only=True)
    assert list(data["model"]) == c["state_dict_keys"]
    n = len(d.model.param_spec())
    assert data["opt"]["param_groups"][0]["params"] == list(range(n + 6)) and set(data["opt"]["state"]) == set(range(n + 6))
    assert all(float(data["opt"]["state"][n + i]["step"]) == 2.0 for i in range(6))
    assert "ema_model.log_snr.net.1.net.weight" in data["ema"] and "online_model.log_snr.net.1.net.weight" in data["ema"]
    l1 = step(d, ema, 2)
    d2, ema2 = fresh()
    at, hyper = dm.load_checkpoint(path, d2, ema=ema2)
    assert at == 2 and abs(hyper["lr"] - 1e-3) < 1e-12 and ema2.step == 2
    l2 = step(d2, ema2, 2)
    assert l1 == l2
    for which, a, b in (("param", d.model.state_dict(), d2.model.state_dict()),
                        ("ema", d.model.state_dict(ema=True), d2.model.state_dict(ema=True)),
                        ("exp_avg", d.model._train_tensors(2), d2.model._train_tensors(2)),
                        ("schedule", d.log_snr.state_dict(), d2.log_snr.state_dict()),
                        ("schedule ema", ema.ema_model.log_snr.state_dict(), ema2.ema_model.log_snr.state_dict())):
        diff = [k for k in a if not torch.equal(a[k], b[k])]
        assert not diff, (which, diff[:3])
    sa, sb = d._sched_opt.state_dict()["state"], d2._sched_opt.state_dict()["state"]
    assert all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in ("step", "exp_avg", "exp_avg_sq"))


def test_the_plain_entry_is_untouched_by_a_learned_call_in_between(golden):
    """One handle: dm_unet_loss_backward_ct, then a learned-schedule call through the input-gradient entry, then the first
    call again -- loss and two gradients bit for bit."""
    c = golden["cases"]["learned"]
    obj, _ = _obj(c)
    obj.train()
    lin = dm.ContinuousTimeGaussianDiffusion(obj.model, image_size=16, noise_schedule="linear")
    kw = dict(times=c["times"][0], noise=c["noises"][0])

    def plain():
        loss = float(lin(c["imgs"][0], **kw))
        return loss, obj.model.grad("init_conv.weight").clone(), obj.model.grad(NAME).clone()

    l1, a1, b1 = plain()
    assert float(obj(c["imgs"][0], **kw)) > 0
    assert float(obj.p_losses_input_grads(c["imgs"][0] * 2 - 1, c["times"][0], noise=c["noises"][0])[0]) > 0
    l2, a2, b2 = plain()
    assert l1 == l2 and torch.equal(a1, a2) and torch.equal(b1, b2)
    # an unarmed handle is refused by the new entry too, by the name of the call that arms
    fresh, _, _ = _unet(D32, 7)
    xz = torch.zeros((2, 3, 16, 16), device=DEV)
    tab = dm.ct_train_table(torch.tensor([0.3, 0.6]), "cosine").contiguous()
    a = _lib.CtTrainIgArgs()
    a.images, a.noise, a.coef_host, a.coef_stride = _lib.ptr(xz), _lib.ptr(xz), _lib.fptr(tab), K.COLS
    a.objective, a.loss_scale, a.B, a.H, a.W, a.normalize = 0, 1.0, 2, 16, 16, 1
    a.stream = torch.cuda.current_stream(DEV).cuda_stream
    lib = _lib.load()
    assert lib.dm_unet_loss_backward_ct_ig(fresh._handle, C.byref(a)) != 0
    assert b"dm_unet_train_enable_ft" in lib.dm_last_error()
