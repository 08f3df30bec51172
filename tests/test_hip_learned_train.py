"""LearnedGaussianDiffusion training on the GPU (fixture: tests/golden/make_golden_learned.py, from the reference).

* ``dm_op_lv_loss`` against the fp64 restatement with autograd (tests/learned_oracle.py): the loss, both per-image parts
  and ``dout`` within max(1e-6, 4 x the fp32 restatement's own error against fp64); the variance half of ``dout`` exactly
  zero for ``vb_loss_weight = 0`` and the noise half independent of the weight bit for bit; the t = 0 image's variance-half
  ``dout`` (all three NLL branches, zero on the clamp) and NLL part pinned against fp32 autograd at 1e-4;
* every training case of the fixture against the reference's own ``p_losses(...).backward()``: loss within max(1e-4, 4 x
  the case's stored reference fp32-vs-fp64 loss error), every gradient digest within max(2e-4, 4 x the case's stored worst
  gradient error) -- the gates of tests/test_hip_ct_train.py -- with ``final_conv.weight`` / ``.bias`` (6 and 8 outputs: the
  wide instance of the thin-output backward kernels) compared in full;
* accumulation, ``forward`` == ``p_losses``, the asynchronous form, a short training run, the checkpoint round trip, and
  the refusals of the C entry points.
Measured errors are printed (run with -s to see them)."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import learned as L
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import edm_train_oracle as eto
import learned_oracle as O
from conftest import check_grad_digest, load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OP_TOL, LOSS_TOL, GRAD_TOL = 1e-6, 1e-4, 2e-4
# The decoder NLL against torch's fp32 autograd of the SAME expression tree: what differs is expf / tanhf / logf (a few ulps
# each), amplified where 1 - tanh^2 cancels; the kernel's arithmetic run on the host differs from torch fp32 by 2e-5 on the
# fixture's t = 0 image.  The fp64 yardstick cannot pin this branch (fp32 itself is 0.7 .. 0.9 away from it).
NLL_PIN_TOL = 1e-4
CASES = ["hand_t", "random_t", "clip", "accumulate2", "c4"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("learned.pt")


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _obj(c, **kw):
    ch = c["channels"]
    cfg = UnetConfig(channels=ch, learned_variance=True, **c["unet_kw"])
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=c["salt"])
    sd["final_conv.bias"][ch:] += c["var_bias"]  # as the fixture's generator builds the training networks
    u = dm.Unet(channels=ch, learned_variance=True, device=DEV, **c["unet_kw"])
    u.load_state_dict(sd)
    kw.setdefault("timesteps", c["timesteps"])
    kw.setdefault("beta_schedule", c["beta_schedule"])
    return dm.LearnedGaussianDiffusion(u, image_size=c["image_size"], **kw), cfg


def _run_case(c, obj):
    total = 0.0
    for i in range(c["micro"]):
        total += float(obj.p_losses(c["imgs"][i] * 2 - 1, c["t"][i], noise=c["noises"][i], clip_denoised=c["clip_denoised"],
                                    loss_scale=1.0 / c["micro"], accumulate=i > 0))
    return total


# ---- the loss kernel -------------------------------------------------------------------------------------------------------
def _loss_inputs(B, C_, hw, seed):
    """A model that is roughly right, images with exact -1 / +1 pixels, image 0 at t = 0 (the decoder NLL)."""
    sched = dm.make_schedule(1000, "linear")
    t = torch.tensor([0, 1, 500, 999, 250][:B])
    tab = dm.lv_train_table(sched, t).contiguous()
    g = torch.Generator().manual_seed(seed)
    shape = (B, C_, hw, hw)
    img, r = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    img[r < 0.1], img[r > 0.9] = 0.0, 1.0
    x0, noise = img * 2 - 1, torch.randn(shape, generator=g)
    x_t = tab[:, L.T_SQRT_AC].reshape(-1, 1, 1, 1) * x0 + tab[:, L.T_SQRT_1M_AC].reshape(-1, 1, 1, 1) * noise
    pred = noise + 0.3 * torch.randn(shape, generator=g)
    v = 0.8 + 0.5 * torch.randn(shape, generator=g)  # the interpolation weight around 0.9, beyond 1 and below 0.5
    return tab, x0, noise, x_t, torch.cat((pred, v), dim=1).contiguous()


def _run_loss(mo, x0, noise, x_t, tab, w, clip, scale):
    lib = _lib.load()
    B, per = x0.shape[0], x0[0].numel()
    d = [t.to(DEV).contiguous() for t in (mo, x0, noise, x_t)]
    dout = torch.full_like(d[0], float("nan"))
    loss = C.c_float(0.0)
    mse, vb = (C.c_float * B)(), (C.c_float * B)()
    _lib.check(lib.dm_op_lv_loss(*[_lib.ptr(t) for t in d], _lib.fptr(tab), w, int(clip), scale, _lib.ptr(dout), C.byref(loss),
                                 mse, vb, B, per, None))
    return torch.tensor(loss.value), dout.cpu(), torch.tensor(list(mse)), torch.tensor(list(vb))


def _loss_errors(got, ref, C_, t0):
    """loss: relative; dout: every image and half on its own scale; the per-image parts as tests/test_hip_step_ops.py
    measures them -- worst error against the largest entry: the KL mean of a middle timestep, where min_log ~ max_log, is
    (-1 + d) + exp(-d) with d ~ 1e-3, noise in any fp32 evaluation.  The t = 0 image (`t0`: the flag column) is kept apart
    from the KL images: its decoder NLL is ill-conditioned in fp32 (tanh saturates) and must not lend them its error."""
    e = {"loss": float((got[0].double() - ref[0].double()).abs() / ref[0].double().abs())}
    for b in range(got[1].shape[0]):
        e[f"dout_noise[{b}]"] = rel_l2(got[1][b, :C_], ref[1][b, :C_])
        e[f"dout_var[{b}]"] = rel_l2(got[1][b, C_:], ref[1][b, C_:])
    e["mse_part"] = float((got[2].double() - ref[2].double()).abs().max() / ref[2].double().abs().max())
    for name, sel in (("vb_part_nll", t0 != 0), ("vb_part_kl", t0 == 0)):
        if bool(sel.any()):
            e[name] = float((got[3][sel].double() - ref[3][sel].double()).abs().max() / ref[3][sel].double().abs().max())
    return e


@pytest.mark.parametrize("B,C_,hw", [(4, 3, 16), (1, 1, 2), (5, 4, 20)], ids=["B4-one-t0", "per4-smallest", "C4-several-strides"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
def test_op_loss_vs_fp64_autograd(B, C_, hw, clip):
    tab, x0, noise, x_t, mo = _loss_inputs(B, C_, hw, 60 + B)
    assert tab[:, L.T_T0].tolist() == [1.0] + [0.0] * (B - 1)
    for w, scale in ((0.001, 1.0), (0.05, 0.5)):
        got = _run_loss(mo, x0, noise, x_t, tab, w, clip, scale)
        ref = O.loss(mo, x0, noise, x_t, tab, w, clip, scale, torch.float64)
        r32 = O.loss(mo, x0, noise, x_t, tab, w, clip, scale, torch.float32)
        err, e32 = _loss_errors(got, ref, C_, tab[:, L.T_T0]), _loss_errors(r32, ref, C_, tab[:, L.T_T0])
        limit = {k: max(4 * e32[k], OP_TOL) for k in err}
        print(f"op lv_loss B={B} C={C_} {hw}x{hw} clip={clip} w={w} scale={scale}: kernel {err} limit {limit} torch fp32 {e32}")
        assert bool(torch.isfinite(got[1]).all()) and all(err[k] <= limit[k] for k in err), (err, limit)
        if B > 1:  # the hand-derived NLL derivative of the t = 0 image, pinned against fp32 autograd
            xs0, g32, gk = x0[0], r32[1][0, C_:], got[1][0, C_:]
            low, high = xs0 < -0.999, xs0 > 0.999
            mid, on_clamp = ~(low | high), g32 == 0  # (no gradient in fp32 autograd)
            share = {k: float(m.float().mean()) for k, m in (("low", low), ("high", high), ("mid", mid), ("clamp", on_clamp))}
            assert min(share["low"], share["high"], share["mid"]) >= 0.01 and 0.01 <= share["clamp"] <= 0.5, share
            pin = {k: rel_l2(gk[m & ~on_clamp], g32[m & ~on_clamp]) for k, m in (("low", low), ("high", high), ("mid", mid))}
            pin["all"] = rel_l2(gk, g32)
            pin["nll_part"] = rel_l2(got[3][0], r32[3][0])
            print(f"  t = 0 image vs torch fp32 autograd: {pin} (gate {NLL_PIN_TOL:.0e}); shares {share}")
            assert all(v <= NLL_PIN_TOL for v in pin.values()), pin
            # nothing where fp32 autograd has exactly 0 (log's clamp at 1e-15 active, or tanh saturated on both sides): tanhf
            # may saturate an ulp later on the device, so the measure is the magnitude left there, not a count of zeros
            assert float(gk[on_clamp].double().norm()) <= NLL_PIN_TOL * float(g32.double().norm())
    # the vb term reaches only the variance half; the MSE only the noise half
    a = _run_loss(mo, x0, noise, x_t, tab, 0.0, clip, 1.0)
    b = _run_loss(mo, x0, noise, x_t, tab, 0.001, clip, 1.0)
    c = _run_loss(mo, x0, noise, x_t, tab, 0.7, clip, 1.0)
    assert not bool(a[1][:, C_:].any()) and bool(b[1][:, C_:].any())
    assert torch.equal(a[1][:, :C_], b[1][:, :C_]) and torch.equal(a[1][:, :C_], c[1][:, :C_])
    assert torch.equal(a[2], b[2]) and torch.equal(b[3], c[3])
    if B > 1:  # an image evaluates only the branch its t selects: the t = 0 image's parts do not move with the others' rows
        tab2 = tab.clone()
        tab2[1:, L.T_T0] = 1.0
        d = _run_loss(mo, x0, noise, x_t, tab2, 0.001, clip, 1.0)
        assert torch.equal(d[3][0], b[3][0]) and torch.equal(d[1][0], b[1][0]) and not torch.equal(d[3][1:], b[3][1:])


# ---- the reference's own loss and gradients ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_loss_and_all_gradients_vs_reference_autograd(golden, case):
    c = golden["train"][case]
    assert c["micro"] == (2 if case == "accumulate2" else 1) and c["channels"] == (4 if case == "c4" else 3)
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
    ch = c["channels"]
    fv = rel_l2(grads["final_conv.weight"][ch:].cpu(), c["final_conv_weight_grad"][ch:])
    print(f"{case}: loss vs reference {loss_err:.3e} (gate {loss_tol:.1e}); worst gradient norm ({worst[0]}) {worst[1]:.3e} "
          f"(gate {tol:.1e}); final_conv.weight {fw:.3e} (variance half {fv:.3e}) final_conv.bias {fb:.3e}; the reference's "
          f"own fp32-vs-fp64: loss {c['ref_err_loss']:.3e}, worst gradient {c['ref_err_grad_max']:.3e}")
    assert loss_err <= loss_tol
    for name, dg in want.items():
        check_grad_digest(name, grads[name].cpu(), dg, tol)
    assert grads["final_conv.weight"].shape[0] == 2 * ch and max(fw, fb) <= tol
    # the variance half of final_conv.weight carries only the vb term (KL and, with a t = 0 image, the NLL derivative): held to
    # the project's gradient floor against the reference's own fp32 autograd, not to the fp64-derived gate above
    assert fv <= GRAD_TOL, (case, fv)
    assert float(c["final_conv_weight_grad"][ch:].norm()) > 0  # the vb term reaches the variance half


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
    assert out.shape == (img.shape[0], 6, 16, 16) and float(val) == float(a)
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


def test_training_lowers_the_loss_then_the_handle_samples(golden):
    c = golden["train"]["random_t"]
    obj, cfg = _obj(c, timesteps=50)
    obj.train()
    imgs = _smooth_images()
    g = torch.Generator().manual_seed(4)
    t = torch.randint(0, 50, (8,), generator=g)
    t[0] = 0  # one image on the decoder NLL
    noise = torch.randn(imgs.shape, generator=g)
    ema = dm.EMA(obj, beta=0.99, update_every=2, update_after_step=4)
    losses = [dm.train_step(obj, [imgs], lr=1e-3, ema=ema, t=[t], noise=[noise])[0] for _ in range(30)]
    print("learned variance: loss", losses[0], "->", losses[-1])
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    with pytest.raises(RuntimeError, match="dm_unet_train_sync"):
        obj.sample(batch_size=2, noise=so.NoiseStream(8))
    obj.model.sync()
    a = obj.sample(batch_size=2, noise=so.NoiseStream(8))
    fresh = dm.Unet(channels=3, learned_variance=True, device=DEV, **c["unet_kw"])
    fresh.load_state_dict(obj.model.state_dict())
    b = dm.LearnedGaussianDiffusion(fresh, image_size=16, timesteps=50).sample(batch_size=2, noise=so.NoiseStream(8))
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    e = ema.ema_model.sample(batch_size=2, noise=so.NoiseStream(8))
    assert e.shape == a.shape and bool(torch.isfinite(e).all()) and isinstance(ema.ema_model, dm.LearnedGaussianDiffusion)
    assert list(dm.diffusion_state_dict(obj)) == golden["state_dict_keys"]


def test_checkpoint_round_trip_continues_bit_for_bit(golden, tmp_path):
    c = golden["train"]["hand_t"]
    g = torch.Generator().manual_seed(12)
    batches = [torch.rand((4, 3, 16, 16), generator=g) for _ in range(3)]
    ts = [torch.randint(0, 1000, (4,), generator=g) for _ in range(3)]
    noises = [torch.randn((4, 3, 16, 16), generator=g) for _ in range(3)]

    def fresh():
        obj, _ = _obj(c, vb_loss_weight=0.01)
        return obj.train(), dm.EMA(obj, beta=0.995, update_every=1, update_after_step=0)

    def step(obj, ema, s):
        return dm.train_step(obj, [batches[s]], lr=1e-3, ema=ema, t=[ts[s]], noise=[noises[s]])

    d, ema = fresh()
    for s in range(2):
        step(d, ema, s)
    path = tmp_path / "lv-1.pt"
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
    # the plain loss entries refuse the learned-variance handle and name the new call
    coef = obj._tcoef(torch.tensor([3, 500]))
    a = _lib.TrainArgs()
    a.x_start, a.noise, a.t_host = _lib.ptr(x), _lib.ptr(x), C.cast(t_arr, C.POINTER(C.c_int64))
    a.coef_host, a.coef_stride, a.loss_scale, a.B, a.H, a.W, a.stream, a.loss_terms = _lib.fptr(coef), 12, 1.0, B, 16, 16, stream, 1
    assert lib.dm_unet_loss_backward_ex(obj.model._handle, C.byref(a)) != 0
    assert b"dm_unet_loss_backward_lv" in lib.dm_last_error()
    mask = (C.c_int32 * B)(1, 1)
    assert lib.dm_unet_loss_backward_masked(obj.model._handle, C.byref(a), mask) != 0
    assert b"dm_unet_loss_backward_lv" in lib.dm_last_error()
    rc = lib.dm_unet_loss_backward(obj.model._handle, _lib.ptr(x), a.t_host, a.coef_host, _lib.ptr(x), None, None, 0, None, 0, 0, 0,
                                   1.0, 0, None, None, B, 16, 16, stream)
    assert rc != 0 and b"dm_unet_loss_backward_lv" in lib.dm_last_error()
    # the new entry refuses a handle whose out_dim == channels, and one that is not armed
    plain = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    plain.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(dim=32, dim_mults=(1, 2), channels=3)), salt=1))
    plain.train()
    tab = dm.lv_train_table(obj._sched, torch.tensor([3, 500])).contiguous()
    v = _lib.LvTrainArgs()
    v.x_start, v.noise, v.t_host, v.coef_host, v.coef_stride = _lib.ptr(x), _lib.ptr(x), a.t_host, _lib.fptr(tab), 12
    v.vb_loss_weight, v.loss_scale, v.B, v.H, v.W, v.stream = 0.001, 1.0, B, 16, 16, stream
    assert lib.dm_unet_loss_backward_lv(plain._handle, C.byref(v)) != 0 and b"2 * channels" in lib.dm_last_error()
    unarmed, _ = _obj(c)
    assert lib.dm_unet_loss_backward_lv(unarmed.model._handle, C.byref(v)) != 0
    assert b"dm_unet_train_enable" in lib.dm_last_error()
    loss = C.c_float(0.0)
    v.loss_out_host = C.pointer(loss)
    assert lib.dm_unet_loss_backward_lv(obj.model._handle, C.byref(v)) == 0 and loss.value > 0
