"""WeightedObjectiveGaussianDiffusion training on the GPU (fixture: tests/golden/make_golden_weighted.py, from the
reference).

* ``dm_op_wo_loss`` against the fp64 restatement with autograd (tests/weighted_oracle.py) on (B, C, HxW) = (1, 1, 2x2),
  (3, 3, 6x10), (2, 2, 16x16), with inputs built so that all three regions of ``xs`` (below -2, inside, above 2) are
  populated and no pixel is within 1e-4 of a bound: the loss, the three per-image parts and ``dout`` per image and per
  channel group (noise / x_start / weights) within max(1e-6, 4 x the fp32 restatement's own error against fp64);
  ``dout[:, 2C + 1] == -dout[:, 2C]`` bit for bit; where ``|xs| > 2`` the noise group equals the bare noise-MSE term to
  1e-6; with both loss weights 0 the result is the weighted term alone;
* every training case of the fixture against the reference's own ``p_losses(...).backward()``: loss within max(1e-4, 4 x
  the case's stored reference fp32-vs-fp64 loss error), every gradient digest within max(2e-4, 4 x the case's stored worst
  gradient error) -- the gates of tests/test_hip_learned_train.py -- with ``final_conv.weight`` / ``.bias`` compared in full
  for out_dim 4, 6 and 8 (both instances of the thin-output backward kernels on this layout);
* accumulation, ``forward`` == ``p_losses``, the asynchronous form, a 5-step training run, EMA, the checkpoint round trip,
  and the refusals of the C entry points.
Measured errors are printed (run with -s to see them)."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import weighted as Wm
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import edm_train_oracle as eto
import weighted_oracle as O
from conftest import check_grad_digest, load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OP_TOL, LOSS_TOL, GRAD_TOL = 1e-6, 1e-4, 2e-4
CASES = ["hand_t", "random_t", "accumulate2", "c1", "c2", "weights"]
SHAPES = [(1, 1, 2, 2), (3, 3, 6, 10), (2, 2, 16, 16)]
SHAPE_IDS = ["one-thread", "hw60-3ch", "16x16-2ch"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("weighted.pt")


def _obj(c, **kw):
    ch = c["channels"]
    cfg = UnetConfig(channels=ch, out_dim=2 * ch + 2, **c["unet_kw"])
    u = dm.Unet(channels=ch, out_dim=2 * ch + 2, device=DEV, **c["unet_kw"])
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=c["salt"]))
    kw.setdefault("timesteps", c["timesteps"])
    kw.setdefault("beta_schedule", c["beta_schedule"])
    kw.setdefault("pred_noise_loss_weight", c["pred_noise_loss_weight"])
    kw.setdefault("pred_x_start_loss_weight", c["pred_x_start_loss_weight"])
    return dm.WeightedObjectiveGaussianDiffusion(u, image_size=c["image_size"], **kw), cfg


def _run_case(c, obj):
    total = 0.0
    for i in range(c["micro"]):
        total += float(obj.p_losses(c["imgs"][i] * 2 - 1, c["t"][i], noise=c["noises"][i], loss_scale=1.0 / c["micro"],
                                    accumulate=i > 0))
    return total


# ---- the loss kernel -------------------------------------------------------------------------------------------------------
TARGETS = (-3.1, 0.6, 2.7, -0.9, 1.6, -2.4, 2.2, -1.7)  # xs of consecutive pixels: below -2, inside, above 2; none near a bound


def _loss_inputs(shape, seed):
    """Images at t = 500, 0, 999 (in that order).  ``xs = recip x_t - recipm1 pn`` is steered onto TARGETS (plus a jitter of
    +-0.05) through ``pn`` where recipm1 is large, through ``x_t`` on the t = 0 image (recipm1 = 0.01)."""
    B, C_, H, W = shape
    sched = dm.make_schedule(1000, "linear")
    tab = dm.wo_train_table(sched, torch.tensor([500, 0, 999][:B])).contiguous()
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1
    noise = torch.randn(shape, generator=g, dtype=torch.float64)
    target = torch.tensor(TARGETS, dtype=torch.float64).repeat(x0.numel() // len(TARGETS) + 1)[:x0.numel()].reshape(shape)
    target = target + (torch.rand(shape, generator=g, dtype=torch.float64) - 0.5) * 0.1
    recip = tab[:, Wm.T_RECIP].double().reshape(-1, 1, 1, 1)
    recipm1 = tab[:, Wm.T_RECIPM1].double().reshape(-1, 1, 1, 1)
    x_t = torch.randn(shape, generator=g, dtype=torch.float64)
    pn = noise + 0.3 * torch.randn(shape, generator=g, dtype=torch.float64)
    by_pn = (recipm1 > 0.5).expand(shape)
    pn = torch.where(by_pn, (recip * x_t - target) / recipm1, pn)
    x_t = torch.where(by_pn, x_t, (target + recipm1 * pn) / recip)
    px = x0 + 0.3 * torch.randn(shape, generator=g, dtype=torch.float64)
    w = torch.randn((B, 2, H, W), generator=g, dtype=torch.float64) * 1.5
    mo = torch.cat((pn, px, w), dim=1).float().contiguous()
    return tab, x0.float(), noise.float(), x_t.float(), mo


def _run_loss(mo, x0, noise, x_t, tab, w_n, w_x, scale):
    lib = _lib.load()
    B, C_, HW = x0.shape[0], x0.shape[1], x0[0, 0].numel()
    d = [t.to(DEV).contiguous() for t in (mo, x0, noise, x_t)]
    dout = torch.full_like(d[0], float("nan"))
    loss = C.c_float(0.0)
    parts = [(C.c_float * B)() for _ in range(3)]
    _lib.check(lib.dm_op_wo_loss(*[_lib.ptr(t) for t in d], _lib.fptr(tab), w_n, w_x, scale, _lib.ptr(dout), C.byref(loss),
                                 *parts, B, C_, HW, None))
    return (torch.tensor(loss.value), dout.cpu()) + tuple(torch.tensor(list(p)) for p in parts)


def _loss_errors(got, ref, C_):
    """loss: relative; dout: every image and channel group on its own scale; the per-image parts: worst error against the
    largest entry."""
    e = {"loss": float((got[0].double() - ref[0].double()).abs() / ref[0].double().abs())}
    for b in range(got[1].shape[0]):
        for name, sl in (("noise", slice(0, C_)), ("x_start", slice(C_, 2 * C_)), ("weights", slice(2 * C_, 2 * C_ + 2))):
            e[f"dout_{name}[{b}]"] = rel_l2(got[1][b, sl], ref[1][b, sl])
    for j, name in ((2, "weighted_part"), (3, "x_start_part"), (4, "noise_part")):
        e[name] = float((got[j].double() - ref[j].double()).abs().max() / ref[j].double().abs().max())
    return e


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_op_loss_vs_fp64_autograd(shape):
    B, C_, H, W = shape
    tab, x0, noise, x_t, mo = _loss_inputs(shape, 60 + B)
    for w_n, w_x, scale in ((0.1, 0.1, 1.0), (0.5, 0.25, 0.5), (0.0, 0.0, 1.0)):
        got = _run_loss(mo, x0, noise, x_t, tab, w_n, w_x, scale)
        ref = O.loss(mo, x0, noise, x_t, tab, w_n, w_x, scale, torch.float64)
        r32 = O.loss(mo, x0, noise, x_t, tab, w_n, w_x, scale, torch.float32)
        # all three regions of xs, in fp64 and in fp32 alike, and no pixel within 1e-4 of a bound
        for xs in (ref[5], r32[5].double()):
            assert bool((xs < -2).any()) and bool((xs.abs() < 2).any()) and bool((xs > 2).any())
            assert float((xs.abs() - 2).abs().min()) >= 1e-4
        assert torch.equal(ref[5] > 2, r32[5] > 2) and torch.equal(ref[5] < -2, r32[5] < -2)
        err, e32 = _loss_errors(got, ref, C_), _loss_errors(r32, ref, C_)
        limit = {k: max(4 * e32[k], OP_TOL) for k in err}
        k = max(err, key=lambda k: err[k] / limit[k])  # the figure closest to its limit; the largest error
        m = max(err, key=lambda k: err[k])
        print(f"op wo_loss {shape} w_n={w_n} w_x={w_x} scale={scale}: closest to its limit {k} kernel {err[k]:.3e} limit "
              f"{limit[k]:.3e} torch fp32 {e32[k]:.3e}; largest {m} kernel {err[m]:.3e} limit {limit[m]:.3e}")
        assert bool(torch.isfinite(got[1]).all()) and all(err[k] <= limit[k] for k in err), (err, limit)
        # softmax sees only w0 - w1
        assert torch.equal(got[1][:, 2 * C_ + 1], -got[1][:, 2 * C_]) and bool(got[1][:, 2 * C_].any())
        # outside the clamp the weighted term does not reach the noise group: the bare noise-MSE term is left
        outside = ref[5].abs() > 2
        n_all = float(x0.numel())
        bare = (scale * 2.0 / n_all * w_n) * (mo[:, :C_].double() - noise.double())
        g_out, b_out = got[1][:, :C_].double()[outside], bare[outside]
        if w_n > 0:
            pin = float((g_out - b_out).norm() / b_out.norm())
            print(f"  noise group where |xs| > 2 vs the bare noise-MSE term: {pin:.3e}")
            assert pin <= 1e-6
        else:
            assert not bool(g_out.any()) and bool(got[1][:, :C_][~outside].any())
    # both weights 0: the weighted term alone -- the same parts bit for bit, and the loss is their mean
    a = _run_loss(mo, x0, noise, x_t, tab, 0.1, 0.1, 1.0)
    z = _run_loss(mo, x0, noise, x_t, tab, 0.0, 0.0, 1.0)
    assert all(torch.equal(a[j], z[j]) for j in (2, 3, 4)) and torch.equal(a[1][:, 2 * C_:], z[1][:, 2 * C_:])
    assert abs(float(z[0]) - float(z[2].double().mean())) <= 1e-6 * float(z[0])
    assert float(a[0]) > float(z[0])


# ---- the reference's own loss and gradients ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_loss_and_all_gradients_vs_reference_autograd(golden, case):
    c = golden["train"][case]
    ch = c["channels"]
    assert c["micro"] == (2 if case == "accumulate2" else 1) and ch == {"c1": 1, "c2": 2}.get(case, 3)
    obj, cfg = _obj(c)
    obj.train()
    loss = _run_case(c, obj)
    spec = dm.unet_param_spec(cfg)
    want = eto.unpack_digests(c, spec)
    grads = obj.model.grads()
    assert set(grads) == set(want)
    loss_tol = max(LOSS_TOL, 4 * c["ref_err_loss"])
    tol = max(GRAD_TOL, 4 * c["ref_err_grad_max"])
    loss_err = abs(loss - c["loss"]) / abs(c["loss"])
    worst = ("", 0.0)
    for name, dg in want.items():
        if dg["norm"] > 0:
            worst = max(worst, (name, abs(float(grads[name].double().norm()) - dg["norm"]) / dg["norm"]), key=lambda v: v[1])
    fw = rel_l2(grads["final_conv.weight"].cpu(), c["final_conv_weight_grad"])
    fb = rel_l2(grads["final_conv.bias"].cpu(), c["final_conv_bias_grad"])
    rows = [rel_l2(grads["final_conv.weight"][r].cpu(), c["final_conv_weight_grad"][r]) for r in range(2 * ch + 2)]
    print(f"{case}: loss vs reference {loss_err:.3e} (gate {loss_tol:.1e}); worst gradient norm ({worst[0]}) {worst[1]:.3e} "
          f"(gate {tol:.1e}); final_conv.weight {fw:.3e} (worst row {max(rows):.3e}) final_conv.bias {fb:.3e}; the reference's "
          f"own fp32-vs-fp64: loss {c['ref_err_loss']:.3e}, worst gradient {c['ref_err_grad_max']:.3e}")
    assert loss_err <= loss_tol
    for name, dg in want.items():
        check_grad_digest(name, grads[name].cpu(), dg, tol)
    assert grads["final_conv.weight"].shape[0] == 2 * ch + 2 and max(fw, fb) <= tol and max(rows) <= tol


def test_forward_is_p_losses_and_the_async_form(golden):
    c = golden["train"]["random_t"]
    obj, _ = _obj(c)
    obj.train()
    img, t, noise = c["imgs"][0], c["t"][0], c["noises"][0]
    a = obj.p_losses(img * 2 - 1, t, noise=noise)
    g1 = {k: v.clone() for k, v in obj.model.grads().items()}
    torch.manual_seed(5)
    t_drawn = torch.randint(0, obj.num_timesteps, (img.shape[0],)).long()
    torch.manual_seed(5)
    b = obj(img, noise=noise)
    c2 = obj.p_losses(img * 2 - 1, t_drawn, noise=noise)
    assert float(b) == float(c2)  # forward: random t from torch's CPU generator, normalise, p_losses
    d = obj.p_losses(img * 2 - 1, t, noise=noise, sync=False)
    assert d.device.type == "cuda" and d.dim() == 0 and float(d) == float(a)
    assert all(torch.equal(g1[k], v) for k, v in obj.model.grads().items())
    val, out = obj.p_losses(img * 2 - 1, t, noise=noise, return_model_out=True)
    assert out.shape == (img.shape[0], 8, 16, 16) and float(val) == float(a)
    # clip_denoised is accepted and unused
    assert float(obj.p_losses(img * 2 - 1, t, noise=noise, clip_denoised=True)) == float(a)
    # accumulation: two half-scaled calls add up to the gradients of one call, to rounding
    obj.p_losses(img * 2 - 1, t, noise=noise, loss_scale=0.5)
    obj.p_losses(img * 2 - 1, t, noise=noise, loss_scale=0.5, accumulate=True)
    acc = obj.model.grads()
    assert max(rel_l2(acc[k], g1[k]) for k in g1 if float(g1[k].norm()) > 0) <= 1e-5
    # without injection: t from torch's global CPU generator first, the noise from the device Philox stream
    torch.manual_seed(6)
    l1 = float(obj(img))
    torch.manual_seed(6)
    assert float(obj(img)) == l1 and 0.0 < l1 < 100.0
    # objective and the other accepted keywords have no effect
    other, _ = _obj(c, objective="pred_x0", offset_noise_strength=0.3, min_snr_loss_weight=True, hybrid_loss=True)
    assert float(other.train().p_losses(img * 2 - 1, t, noise=noise)) == float(a)


def _smooth_images(n=8):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 16), torch.linspace(0, 1, 16), indexing="ij")
    g = torch.Generator().manual_seed(3)
    return torch.stack([torch.stack([(yy * a + xx * (1 - a)), (yy * xx) ** b, (1 - yy) * a]) for a, b in
                        zip(torch.rand(n, generator=g).tolist(), (torch.rand(n, generator=g) + 0.5).tolist())]).float()


def test_five_training_steps_lower_the_loss_then_the_handle_samples(golden):
    c = golden["train"]["random_t"]
    obj, cfg = _obj(c, timesteps=50)
    obj.train()
    imgs = _smooth_images()
    g = torch.Generator().manual_seed(4)
    t = torch.randint(0, 50, (8,), generator=g)
    noise = torch.randn(imgs.shape, generator=g)
    ema = dm.EMA(obj, beta=0.99, update_every=2, update_after_step=1)
    losses = [dm.train_step(obj, [imgs], lr=1e-3, ema=ema, t=[t], noise=[noise])[0] for _ in range(5)]
    print("weighted objective: loss", losses)
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    with pytest.raises(RuntimeError, match="dm_unet_train_sync"):
        obj.sample(batch_size=2, noise=so.NoiseStream(8))
    obj.model.sync()
    a = obj.sample(batch_size=2, noise=so.NoiseStream(8))
    fresh = dm.Unet(channels=3, out_dim=8, device=DEV, **c["unet_kw"])
    fresh.load_state_dict(obj.model.state_dict())
    b = dm.WeightedObjectiveGaussianDiffusion(fresh, image_size=16, timesteps=50).sample(batch_size=2, noise=so.NoiseStream(8))
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    e = ema.ema_model.sample(batch_size=2, noise=so.NoiseStream(8))
    assert e.shape == a.shape and bool(torch.isfinite(e).all())
    assert isinstance(ema.ema_model, dm.WeightedObjectiveGaussianDiffusion) and ema.ema_model.model.out_dim == 8
    assert list(dm.diffusion_state_dict(obj)) == golden["state_dict_keys"]


def test_checkpoint_round_trip_continues_bit_for_bit(golden, tmp_path):
    c = golden["train"]["hand_t"]
    g = torch.Generator().manual_seed(12)
    batches = [torch.rand((4, 3, 16, 16), generator=g) for _ in range(3)]
    ts = [torch.randint(0, 1000, (4,), generator=g) for _ in range(3)]
    noises = [torch.randn((4, 3, 16, 16), generator=g) for _ in range(3)]

    def fresh():
        obj, _ = _obj(c, pred_noise_loss_weight=0.2)
        return obj.train(), dm.EMA(obj, beta=0.995, update_every=1, update_after_step=0)

    def step(obj, ema, s):
        return dm.train_step(obj, [batches[s]], lr=1e-3, ema=ema, t=[ts[s]], noise=[noises[s]])

    d, ema = fresh()
    for s in range(2):
        step(d, ema, s)
    path = tmp_path / "wo-1.pt"
    dm.save_checkpoint(path, d, step=2, ema=ema, lr=1e-3)
    data = torch.load(str(path), map_location="cpu", weights_only=True)
    assert list(data["model"]) == golden["state_dict_keys"]
    assert list(dm.load_trainer_checkpoint(str(path))) == golden["state_dict_keys"]
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
    d2.model.sync()
    y = d2.p_sample_loop((2, 3, 16, 16), seed=3, max_steps=4)
    assert bool(torch.isfinite(y).all())


def test_c_entry_points_refuse_the_wrong_handle(golden):
    c = golden["train"]["hand_t"]
    lib = _lib.load()
    obj, _ = _obj(c)
    obj.train()
    B = 2
    x = torch.zeros((B, 3, 16, 16), device=DEV)
    t_arr = (C.c_int64 * B)(3, 500)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    # the plain loss entry refuses the weighted-objective handle and names the new call
    coef = obj._tcoef(torch.tensor([3, 500]))
    a = _lib.TrainArgs()
    a.x_start, a.noise, a.t_host = _lib.ptr(x), _lib.ptr(x), C.cast(t_arr, C.POINTER(C.c_int64))
    a.coef_host, a.coef_stride, a.loss_scale, a.B, a.H, a.W, a.stream, a.loss_terms = _lib.fptr(coef), 12, 1.0, B, 16, 16, stream, 1
    assert lib.dm_unet_loss_backward_ex(obj.model._handle, C.byref(a)) != 0
    assert b"dm_unet_loss_backward_wo" in lib.dm_last_error()
    tab = dm.wo_train_table(obj._sched, torch.tensor([3, 500])).contiguous()
    v = _lib.WoTrainArgs()
    v.x_start, v.noise, v.t_host, v.coef_host, v.coef_stride = _lib.ptr(x), _lib.ptr(x), a.t_host, _lib.fptr(tab), 12
    v.pred_noise_loss_weight, v.pred_x_start_loss_weight, v.loss_scale = 0.1, 0.1, 1.0
    v.B, v.H, v.W, v.stream = B, 16, 16, stream
    # a plain U-Net (out_dim == channels)
    plain = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    plain.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(dim=32, dim_mults=(1, 2), channels=3)), salt=1))
    plain.train()
    assert lib.dm_unet_loss_backward_wo(plain._handle, C.byref(v)) != 0 and b"2 * channels + 2" in lib.dm_last_error()
    # out_dim 10 (channels 4): beyond the thin-output kernels, in C as in the constructor
    cfg10 = UnetConfig(dim=32, dim_mults=(1, 2), channels=4, out_dim=10)
    wide = dm.Unet(dim=32, dim_mults=(1, 2), channels=4, out_dim=10, device=DEV)
    wide.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg10), salt=2))
    with pytest.raises(NotImplementedError, match="channels <= 3"):
        dm.WeightedObjectiveGaussianDiffusion(wide, image_size=16)
    s = _lib.WoArgs()
    times, coefs = dm.wo_step_table(obj._sched, [5, 4])
    times_arr = (C.c_int64 * 2)(*times)
    x4 = torch.zeros((B, 4, 16, 16), device=DEV)
    s.n_steps, s.times_host, s.table_host = 2, C.cast(times_arr, C.POINTER(C.c_int64)), _lib.fptr(coefs)
    s.x_T, s.out, s.B, s.H, s.W, s.seed, s.stream = _lib.ptr(x4), _lib.ptr(x4), B, 16, 16, 1, stream
    assert lib.dm_sample_wo(wide._handle, C.byref(s)) != 0 and b"at most 8" in lib.dm_last_error()
    # a handle armed for float-time training
    ft = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, learned_sinusoidal_cond=True, device=DEV)
    ft.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(
        UnetConfig(dim=32, dim_mults=(1, 2), channels=3, learned_sinusoidal_cond=True)), salt=3))
    dm.ElucidatedDiffusion(ft, image_size=16).train()
    assert lib.dm_unet_loss_backward_wo(ft._handle, C.byref(v)) != 0 and b"float-time" in lib.dm_last_error()
    # one that is not armed at all; then the armed one runs
    unarmed, _ = _obj(c)
    assert lib.dm_unet_loss_backward_wo(unarmed.model._handle, C.byref(v)) != 0
    assert b"dm_unet_train_enable" in lib.dm_last_error()
    loss = C.c_float(0.0)
    v.loss_out_host = C.pointer(loss)
    assert lib.dm_unet_loss_backward_wo(obj.model._handle, C.byref(v)) == 0 and loss.value > 0
