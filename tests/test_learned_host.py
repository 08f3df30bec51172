"""LearnedGaussianDiffusion without a GPU (fixture: tests/golden/make_golden_learned.py): the host tables against the
scalars recorded from the running reference, bit for bit; the constructor / method surface and the state-dict keys; the
reference's asserts and every refusal, on stub nets; the CPU restatement (tests/learned_oracle.py) against the reference's
recorded p_sample steps, loops and losses, which ties the table layout and the kernels' formulas to the reference."""
import inspect
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import learned as L
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo

import learned_oracle as O
from conftest import load_golden, rel_l2


@pytest.fixture(scope="module")
def golden():
    return load_golden("learned.pt")


SCHEDULES = {"linear_50": ("linear", 50), "cosine_24": ("cosine", 24), "linear_1000": ("linear", 1000)}


@pytest.mark.parametrize("key", list(SCHEDULES))
def test_tables_equal_the_recorded_scalars_bit_for_bit(golden, key):
    name, T = SCHEDULES[key]
    sched = dm.make_schedule(T, name)
    rec = golden["scalars"][key]  # row t: [min_log, max_log] as the reference's `extract` returned them
    assert rec.shape == (T, 2) and bool(torch.isfinite(rec).all())
    times, tab = dm.lv_step_table(sched)
    assert times == list(reversed(range(T))) and tab.shape == (T, L.COLS) and tab.dtype == torch.float32
    idx = torch.tensor(times)
    assert torch.equal(tab[:, L.MIN_LOG].double(), rec[idx, 0]) and torch.equal(tab[:, L.MAX_LOG].double(), rec[idx, 1])
    assert torch.equal(tab[:, L.NOISE], (idx > 0).float()) and not bool(tab[:, 7:].any())
    for col, buf in ((L.RECIP, "sqrt_recip_alphas_cumprod"), (L.RECIPM1, "sqrt_recipm1_alphas_cumprod"),
                     (L.COEF1, "posterior_mean_coef1"), (L.COEF2, "posterior_mean_coef2")):
        assert torch.equal(tab[:, col], sched[buf][idx])
    t = torch.tensor([0, 1, T // 2, T - 1, 0])
    tt = dm.lv_train_table(sched, t)
    assert tt.shape == (5, L.TRAIN_COLS) and tt.dtype == torch.float32
    assert torch.equal(tt[:, L.T_MIN_LOG].double(), rec[t, 0]) and torch.equal(tt[:, L.T_TRUE_LOG], tt[:, L.T_MIN_LOG])
    assert torch.equal(tt[:, L.T_MAX_LOG].double(), rec[t, 1]) and tt[:, L.T_T0].tolist() == [1, 0, 0, 0, 1]
    for col, buf in ((L.T_SQRT_AC, "sqrt_alphas_cumprod"), (L.T_SQRT_1M_AC, "sqrt_one_minus_alphas_cumprod"),
                     (L.T_RECIP, "sqrt_recip_alphas_cumprod"), (L.T_RECIPM1, "sqrt_recipm1_alphas_cumprod"),
                     (L.T_COEF1, "posterior_mean_coef1"), (L.T_COEF2, "posterior_mean_coef2")):
        assert torch.equal(tt[:, col], sched[buf][t])
    assert not bool(tt[:, 10:].any())


def test_the_linear_schedule_trap_and_the_objective():
    # beta_schedule='linear' scales betas by 1000 / timesteps: 8 steps give betas >= 1 and a NaN table, 50 are fine
    assert not bool(torch.isfinite(dm.lv_step_table(dm.make_schedule(8, "linear"))[1]).all())
    assert bool(torch.isfinite(dm.lv_step_table(dm.make_schedule(50, "linear"))[1]).all())
    a = L.LearnedGaussianDiffusion(_stub_net(), image_size=16, timesteps=50, objective="pred_noise")
    b = L.LearnedGaussianDiffusion(_stub_net(), image_size=16, timesteps=50, objective="pred_x0")
    assert torch.equal(dm.lv_step_table(a._sched)[1], dm.lv_step_table(b._sched)[1])


def _stub_net(**kw):
    base = dict(random_or_learned_sinusoidal_cond=False, self_condition=False, text_condition=False, out_dim=6, channels=3,
                cfg=types.SimpleNamespace(cond_channels=0), device="cpu", downsample_factor=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_surface_and_state_dict_keys_match_the_reference(golden):
    cls, s = dm.LearnedGaussianDiffusion, golden["surface"]
    sig = inspect.signature(cls.__init__)
    ours = [(p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name)
            for p in sig.parameters.values() if p.name != "self"]
    assert ours == [tuple(v) for v in s["init_params"]]
    assert ours[:2] == [("model", None, "POSITIONAL_OR_KEYWORD"), ("vb_loss_weight", 0.001, "POSITIONAL_OR_KEYWORD")]
    for name, params in s["methods"].items():
        got = list(inspect.signature(getattr(cls, name)).parameters.values())[1:]
        if name == "model_predictions":  # refused whatever it is given
            continue
        want = [(n, k) for n, k in (tuple(p) for p in params) if k != "VAR_KEYWORD"]
        ref = [(p.name, p.kind.name) for p in got[:len(want)]]
        assert ref == want, (name, ref, want)
        rest = [p for p in got[len(want):] if p.kind is not inspect.Parameter.VAR_POSITIONAL]
        assert all(p.kind in (inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.VAR_KEYWORD) for p in rest), name
    assert issubclass(cls, dm.DenoisingDiffusion) and cls.__call__ is cls.forward
    pl = inspect.signature(cls.p_losses).parameters
    assert list(pl)[1:5] == ["x_start", "t", "noise", "clip_denoised"] and pl["clip_denoised"].default is False
    assert all(pl[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("loss_scale", "accumulate", "sync"))
    loop = inspect.signature(cls.p_sample_loop).parameters
    assert all(loop[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("noise", "seed", "max_steps", "sample_offset"))
    cfg = UnetConfig(**golden["state_dict_unet_kw"])
    from diffusion_models_amd.spec import SCHEDULE_BUFFERS
    assert golden["state_dict_keys"] == list(SCHEDULE_BUFFERS) + ["model." + n for n, _ in dm.unet_param_spec(cfg)]
    net = _stub_net(state_dict=lambda: {"a.b": torch.zeros(1)}, _loaded=True)
    obj = cls(net, image_size=16, timesteps=50)
    assert list(obj.state_dict()) == list(SCHEDULE_BUFFERS) + ["model.a.b"]
    assert obj.vb_loss_weight == 0.001 and cls(net, 0.01, image_size=16).vb_loss_weight == 0.01
    assert obj.sample_shape() == (3, 16, 16) and obj.num_timesteps == 50 and not obj.is_ddim_sampling
    for name in ("LearnedGaussianDiffusion", "lv_step_table", "lv_train_table"):
        assert name in dm.__all__ and hasattr(dm, name)


def test_asserts_and_refusals():
    cls = dm.LearnedGaussianDiffusion
    with pytest.raises(AssertionError, match="twice the number of channels"):
        cls(_stub_net(out_dim=3), image_size=16)
    with pytest.raises(AssertionError, match="not supported yet"):
        cls(_stub_net(self_condition=True), image_size=16)
    with pytest.raises(AssertionError):
        cls(_stub_net(random_or_learned_sinusoidal_cond=True), image_size=16)
    with pytest.raises(NotImplementedError, match="immiscible"):
        cls(_stub_net(), image_size=16, immiscible=True)
    # accepted and without effect, as in the reference
    obj = cls(_stub_net(), image_size=16, timesteps=50, objective="pred_v", offset_noise_strength=0.1,
              min_snr_loss_weight=True, hybrid_loss=True)
    assert obj.objective == "pred_v"
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="does not run"):
        obj.model_predictions(x, torch.zeros(1, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="does not run"):
        obj.ddim_sample((1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match="does not run"):
        obj.ddim_sample_guided((1, 3, 16, 16))
    ddim = cls(_stub_net(), image_size=16, timesteps=50, sampling_timesteps=10)
    assert ddim.is_ddim_sampling
    with pytest.raises(NotImplementedError, match="sampling_timesteps < timesteps"):
        ddim.sample(batch_size=1)
    # the plain class still refuses such a U-Net
    with pytest.raises(AssertionError):
        dm.DenoisingDiffusion(_stub_net(), image_size=16)


# ---- the restatement against the reference's recorded results ----------------------------------------------------------
def _weights(channels, ukw, salt, var_bias=0.0):
    cfg = UnetConfig(channels=channels, learned_variance=True, **ukw)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt)
    sd["final_conv.bias"][channels:] += var_bias
    return cfg, sd


def test_restated_p_sample_steps_match_the_reference(golden):
    s = golden["steps_single"]
    cfg, sd = _weights(s["channels"], s["unet_kw"], s["salt"])
    times, tab = dm.lv_step_table(dm.make_schedule(s["timesteps"], s["beta_schedule"]))
    with torch.inference_mode():
        for row in s["steps"]:
            t = row["t"]
            z = so.NoiseStream(row["noise_seed"])(s["x"].shape) if t > 0 else None
            out, _, _, x_start = O.p_sample(lambda x, tt: uo.unet_forward(sd, cfg, x, tt), s["x"], t, tab[s["timesteps"] - 1 - t], z)
            err = (rel_l2(out, row["y"]), rel_l2(x_start, row["x_start"]))
            print("p_sample t", t, "restatement vs reference", err, "frac", row["frac_range"])
            assert max(err) <= 1e-5


def test_restated_loop_matches_the_reference(golden):
    c = golden["loops"]["lin50_c3"]
    cfg, sd = _weights(c["channels"], c["unet_kw"], c["salt"])
    times, tab = dm.lv_step_table(dm.make_schedule(c["timesteps"], c["beta_schedule"]))
    shape = (c["batch"], c["channels"], c["image_size"], c["image_size"])
    with torch.inference_mode():
        y = O.sample(lambda x, tt: uo.unet_forward(sd, cfg, x, tt), times, tab, shape, so.NoiseStream(c["noise_seed"]))
    err = rel_l2(y, c["sample"])
    print("loop lin50_c3 restatement vs reference", err, "frac", c["frac_range"])
    assert err <= 1e-4 and c["frac_range"][0] < 0 and c["frac_range"][1] > 1


@pytest.mark.parametrize("case", ["hand_t", "clip", "c4"])
def test_restated_loss_matches_the_reference(golden, case):
    c = golden["train"][case]
    ch = c["channels"]
    cfg, sd = _weights(ch, c["unet_kw"], c["salt"], c["var_bias"])
    sched = dm.make_schedule(c["timesteps"], c["beta_schedule"])
    t, x0, noise = c["t"][0], c["imgs"][0] * 2 - 1, c["noises"][0]
    assert t.tolist() == [0, 1, c["timesteps"] // 2, c["timesteps"] - 1]
    tab = dm.lv_train_table(sched, t)
    x_t = tab[:, L.T_SQRT_AC].reshape(-1, 1, 1, 1) * x0 + tab[:, L.T_SQRT_1M_AC].reshape(-1, 1, 1, 1) * noise
    with torch.inference_mode():
        mo = uo.unet_forward(sd, cfg, x_t, t)
    loss, dout, mse, vb = O.loss(mo, x0, noise, x_t, tab, c["vb_loss_weight"], clip=c["clip_denoised"])
    err = dict(loss=abs(float(loss) - c["loss"]) / abs(c["loss"]), mse=rel_l2(mse, c["parts"][0]["mse"]),
               vb=rel_l2(vb, c["parts"][0]["vb"]))
    print(case, "restatement vs reference", err, "reference fp32-vs-fp64 loss", c["ref_err_loss"])
    # the same fp32 torch arithmetic on both sides (the U-Net is the oracle's, not the reference module)
    assert err["loss"] <= 1e-5 and err["mse"] <= 1e-5 and err["vb"] <= 1e-4
    # the vb term reaches only the variance half, the MSE only the noise half
    _, d0, _, _ = O.loss(mo, x0, noise, x_t, tab, 0.0, clip=c["clip_denoised"])
    assert not bool(d0[:, ch:].any()) and torch.equal(d0[:, :ch], dout[:, :ch]) and bool(dout[:, ch:].any())
    assert c["t0_var_grad_norm"] > 0 and 0 <= c["ref_err_loss"] < 1e-3
