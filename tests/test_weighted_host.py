"""WeightedObjectiveGaussianDiffusion without a GPU (fixture: tests/golden/make_golden_weighted.py): the host tables against
the scalars ``extract`` gave the running reference, bit for bit; the constructor / method surface and the state-dict keys;
the reference's asserts and every refusal, on stub nets; the CPU restatement (tests/weighted_oracle.py) against the
reference's recorded p_mean_variance, p_sample steps, loops and losses, which ties the table layout and the kernels'
formulas to the reference; and the conditions the fixture's generator asserted, read back from the stored values."""
import inspect
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import weighted as Wm
from diffusion_models_amd.spec import SCHEDULE_BUFFERS, UnetConfig
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo

import weighted_oracle as O
from conftest import load_golden, rel_l2

TRAIN_CASES = ["hand_t", "random_t", "accumulate2", "c1", "c2", "weights"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("weighted.pt")


def _stub_net(**kw):
    base = dict(random_or_learned_sinusoidal_cond=False, self_condition=False, text_condition=False, out_dim=8, channels=3,
                cfg=types.SimpleNamespace(cond_channels=0), device="cpu", downsample_factor=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _weights(channels, ukw, salt):
    cfg = UnetConfig(channels=channels, out_dim=2 * channels + 2, **ukw)
    return cfg, dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt)


def test_tables_equal_what_extract_gave_the_reference(golden):
    p = golden["pmv"]
    sched = dm.make_schedule(p["timesteps"], p["beta_schedule"])
    T = p["timesteps"]
    times, tab = dm.wo_step_table(sched)
    assert times == list(reversed(range(T))) and tab.shape == (T, Wm.COLS) and tab.dtype == torch.float32
    assert (Wm.COLS, Wm.TRAIN_COLS) == (16, 12) and not bool(tab[:, 6:].any())
    idx = torch.tensor(times)
    assert torch.equal(tab[:, Wm.NOISE], (idx > 0).float())
    for row in p["rows"]:
        t, ext = row["t"], row["extract"]
        r = tab[T - 1 - t]
        got = dict(sqrt_recip_alphas_cumprod=r[Wm.RECIP], sqrt_recipm1_alphas_cumprod=r[Wm.RECIPM1],
                   posterior_mean_coef1=r[Wm.COEF1], posterior_mean_coef2=r[Wm.COEF2],
                   posterior_log_variance_clipped=r[Wm.LOGVAR])
        tt = dm.wo_train_table(sched, torch.tensor([t]))[0]
        got.update(sqrt_alphas_cumprod=tt[Wm.T_SQRT_AC], sqrt_one_minus_alphas_cumprod=tt[Wm.T_SQRT_1M_AC])
        for k, v in got.items():
            assert float(v) == ext[k], (t, k)
        assert float(tt[Wm.T_RECIP]) == ext["sqrt_recip_alphas_cumprod"] and float(tt[Wm.T_RECIPM1]) == ext["sqrt_recipm1_alphas_cumprod"]
        assert not bool(tt[4:].any())
        # the variance and log variance the reference returned are those scalars, shaped (B, 1, 1, 1)
        assert tuple(row["variance"].shape) == (2, 1, 1, 1) and tuple(row["log_variance"].shape) == (2, 1, 1, 1)
        assert float(row["log_variance"][0]) == float(r[Wm.LOGVAR])
        assert float(row["variance"][0]) == float(sched["posterior_variance"][t])
    # a bounded table, and per-image training rows
    times3, tab3 = dm.wo_step_table(sched, [5, 0])
    assert times3 == [5, 0] and torch.equal(tab3[0], tab[T - 6]) and torch.equal(tab3[1], tab[T - 1])
    tt = dm.wo_train_table(sched, torch.tensor([0, 1, T // 2, T - 1]))
    assert tt.shape == (4, 12) and torch.equal(tt[:, Wm.T_SQRT_AC], sched["sqrt_alphas_cumprod"][[0, 1, T // 2, T - 1]])


def test_surface_and_state_dict_keys_match_the_reference(golden):
    cls, s = dm.WeightedObjectiveGaussianDiffusion, golden["surface"]
    sig = inspect.signature(cls.__init__)
    ours = [(p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name)
            for p in sig.parameters.values() if p.name != "self"]
    assert ours == [tuple(v) for v in s["init_params"]]
    assert ours == [("model", None, "POSITIONAL_OR_KEYWORD"), ("args", None, "VAR_POSITIONAL"),
                    ("pred_noise_loss_weight", 0.1, "KEYWORD_ONLY"), ("pred_x_start_loss_weight", 0.1, "KEYWORD_ONLY"),
                    ("kwargs", None, "VAR_KEYWORD")]
    for name, params in s["methods"].items():
        got = list(inspect.signature(getattr(cls, name)).parameters.values())[1:]
        want = [(n, k) for n, k in (tuple(p) for p in params) if k != "VAR_KEYWORD"]
        ref = [(p.name, p.kind.name) for p in got[:len(want)]]
        assert ref == want, (name, ref, want)
        rest = [p for p in got[len(want):] if p.kind is not inspect.Parameter.VAR_POSITIONAL]
        assert all(p.kind in (inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.VAR_KEYWORD) for p in rest), name
    assert [p for p in inspect.signature(cls.p_mean_variance).parameters][1:] == ["x", "t", "clip_denoised", "model_output"]
    assert issubclass(cls, dm.DenoisingDiffusion) and cls.__call__ is cls.forward
    pl = inspect.signature(cls.p_losses).parameters
    assert list(pl)[1:5] == ["x_start", "t", "noise", "clip_denoised"] and pl["clip_denoised"].default is False
    assert all(pl[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("loss_scale", "accumulate", "sync", "return_model_out"))
    loop = inspect.signature(cls.p_sample_loop).parameters
    assert all(loop[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("noise", "seed", "max_steps", "sample_offset"))
    cfg = UnetConfig(**golden["state_dict_unet_kw"])
    assert golden["state_dict_keys"] == list(SCHEDULE_BUFFERS) + ["model." + n for n, _ in dm.unet_param_spec(cfg)]
    net = _stub_net(state_dict=lambda: {"a.b": torch.zeros(1)}, _loaded=True)
    obj = cls(net, image_size=16, timesteps=50)
    assert list(obj.state_dict()) == list(SCHEDULE_BUFFERS) + ["model.a.b"]
    assert (obj.pred_noise_loss_weight, obj.pred_x_start_loss_weight, obj.split_dims) == (0.1, 0.1, (3, 3, 2))
    other = cls(_stub_net(out_dim=4, channels=1), image_size=16, pred_noise_loss_weight=0.5, pred_x_start_loss_weight=0.25)
    assert (other.pred_noise_loss_weight, other.pred_x_start_loss_weight, other.split_dims) == (0.5, 0.25, (1, 1, 2))
    assert obj.sample_shape() == (3, 16, 16) and obj.num_timesteps == 50 and not obj.is_ddim_sampling
    for name in ("WeightedObjectiveGaussianDiffusion", "wo_step_table", "wo_train_table"):
        assert name in dm.__all__ and hasattr(dm, name)
    assert golden["reference_sample_raises"] == "TypeError"  # the deviation: the reference trains but cannot sample


def test_asserts_and_refusals():
    cls = dm.WeightedObjectiveGaussianDiffusion
    with pytest.raises(AssertionError, match="twice the number of channels \\+ 2"):
        cls(_stub_net(out_dim=6), image_size=16)
    with pytest.raises(AssertionError, match="not supported yet"):
        cls(_stub_net(self_condition=True), image_size=16)
    with pytest.raises(AssertionError, match="ddim sampling cannot be used"):
        cls(_stub_net(), image_size=16, timesteps=50, sampling_timesteps=10)
    with pytest.raises(AssertionError):
        cls(_stub_net(random_or_learned_sinusoidal_cond=True), image_size=16)
    with pytest.raises(NotImplementedError, match="immiscible"):
        cls(_stub_net(), image_size=16, immiscible=True)
    with pytest.raises(NotImplementedError, match="channels <= 3"):
        cls(_stub_net(out_dim=10, channels=4), image_size=16)
    # accepted and without effect, as in the reference
    obj = cls(_stub_net(), image_size=16, timesteps=50, objective="pred_v", offset_noise_strength=0.1,
              min_snr_loss_weight=True, hybrid_loss=True)
    plain = cls(_stub_net(), image_size=16, timesteps=50)
    assert obj.objective == "pred_v"
    assert torch.equal(dm.wo_step_table(obj._sched)[1], dm.wo_step_table(plain._sched)[1])
    t = torch.tensor([0, 7, 49])
    assert torch.equal(dm.wo_train_table(obj._sched, t), dm.wo_train_table(plain._sched, t))
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match="ddim sampling cannot be used"):
        obj.model_predictions(x, torch.zeros(1, dtype=torch.long))
    with pytest.raises(NotImplementedError, match="ddim sampling cannot be used"):
        obj.ddim_sample((1, 3, 16, 16))
    with pytest.raises(NotImplementedError, match="ddim sampling cannot be used"):
        obj.ddim_sample_guided((1, 3, 16, 16))
    # the plain class still refuses such a U-Net
    with pytest.raises(AssertionError):
        dm.DenoisingDiffusion(_stub_net(), image_size=16)


# ---- the restatement against the reference's recorded results ----------------------------------------------------------
def test_restated_p_mean_variance_matches_the_reference(golden):
    p = golden["pmv"]
    cfg, sd = _weights(p["channels"], p["unet_kw"], p["salt"])
    T = p["timesteps"]
    _, tab = dm.wo_step_table(dm.make_schedule(T, p["beta_schedule"]))
    fwd = lambda x, tt: uo.unet_forward(sd, cfg, x, tt)  # noqa: E731
    with torch.inference_mode():
        for row in p["rows"]:
            t = row["t"]
            mean, x_start = O.p_mean_variance(fwd, p["x"], t, tab[T - 1 - t])
            raw, _ = O.p_mean_variance(fwd, p["x"], t, tab[T - 1 - t], clip=False)
            err = (rel_l2(mean, row["mean"]), rel_l2(raw, row["mean_unclipped"]))
            print("p_mean_variance t", t, "restatement vs reference (clipped, unclipped)", err)
            assert max(err) <= 1e-5 and float(x_start.abs().max()) <= 1.0
        m = p["mixed"]
        for b, t in enumerate(m["t"].tolist()):
            mean, _ = O.p_mean_variance(fwd, p["x"][b:b + 1], t, tab[T - 1 - t])
            assert rel_l2(mean, m["mean"][b:b + 1]) <= 1e-5
            assert float(m["log_variance"][b]) == float(tab[T - 1 - t, Wm.LOGVAR])


def test_restated_p_sample_steps_match_the_reference(golden):
    s = golden["steps_single"]
    cfg, sd = _weights(s["channels"], s["unet_kw"], s["salt"])
    _, tab = dm.wo_step_table(dm.make_schedule(s["timesteps"], s["beta_schedule"]))
    with torch.inference_mode():
        for row in s["steps"]:
            t = row["t"]
            z = so.NoiseStream(row["noise_seed"])(s["x"].shape) if t > 0 else None
            out, _, x_start = O.p_sample(lambda x, tt: uo.unet_forward(sd, cfg, x, tt), s["x"], t, tab[s["timesteps"] - 1 - t], z)
            err = (rel_l2(out, row["y"]), rel_l2(x_start, row["x_start"]))
            print("p_sample t", t, "restatement vs reference", err)
            assert max(err) <= 1e-5


@pytest.mark.parametrize("key", ["lin50_c3", "cos24_c1"])
def test_restated_loop_matches_the_reference(golden, key):
    c = golden["loops"][key]
    cfg, sd = _weights(c["channels"], c["unet_kw"], c["salt"])
    times, tab = dm.wo_step_table(dm.make_schedule(c["timesteps"], c["beta_schedule"]))
    shape = (c["batch"], c["channels"], c["image_size"], c["image_size"])
    with torch.inference_mode():
        y = O.sample(lambda x, tt: uo.unet_forward(sd, cfg, x, tt), times, tab, shape, so.NoiseStream(c["noise_seed"]))
    err = rel_l2(y, c["sample"])
    print("loop", key, "restatement vs reference", err)
    assert err <= 1e-4


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_restated_loss_matches_the_reference(golden, case):
    c = golden["train"][case]
    ch, T = c["channels"], c["timesteps"]
    cfg, sd = _weights(ch, c["unet_kw"], c["salt"])
    sched = dm.make_schedule(T, c["beta_schedule"])
    total = 0.0
    for i in range(c["micro"]):
        t, x0, noise = c["t"][i], c["imgs"][i] * 2 - 1, c["noises"][i]
        tab = dm.wo_train_table(sched, t)
        x_t = tab[:, Wm.T_SQRT_AC].reshape(-1, 1, 1, 1) * x0 + tab[:, Wm.T_SQRT_1M_AC].reshape(-1, 1, 1, 1) * noise
        with torch.inference_mode():
            mo = uo.unet_forward(sd, cfg, x_t, t)
        loss, dout, wp, xp, npart, xs = O.loss(mo, x0, noise, x_t, tab, c["pred_noise_loss_weight"], c["pred_x_start_loss_weight"],
                                               1.0 / c["micro"])
        total += float(loss)
        err = dict(weighted=rel_l2(wp, c["parts"][i]["weighted"]), x_start=rel_l2(xp, c["parts"][i]["x_start"]),
                   noise=rel_l2(npart, c["parts"][i]["noise"]))
        print(case, i, "per-image parts, restatement vs reference", err)
        assert max(err.values()) <= 1e-4
        # d w1 = -d w0: the softmax sees only the difference of the two weight maps
        assert rel_l2(dout[:, 2 * ch + 1], -dout[:, 2 * ch]) <= 1e-6 and bool(dout[:, 2 * ch].any())
        # outside the clamp the weighted term does not reach the noise half
        _, d0, *_ = O.loss(mo, x0, noise, x_t, tab, 0.0, 0.0, 1.0 / c["micro"])
        out_of_gate = (xs.abs() > 2)
        assert bool(out_of_gate.any()) and not bool(d0[:, :ch][out_of_gate].any()) and bool(d0[:, :ch][~out_of_gate].any())
    err = abs(total - c["loss"]) / abs(c["loss"])
    print(case, "loss restatement vs reference", err, "reference fp32-vs-fp64", c["ref_err_loss"])
    # the same fp32 torch arithmetic on both sides (the U-Net is the oracle's, not the reference module)
    assert err <= 1e-5 and 0 <= c["ref_err_loss"] < 1e-3


@pytest.mark.parametrize("case", TRAIN_CASES)
def test_fixture_conditions_hold(golden, case):
    c = golden["train"][case]
    ch, T = c["channels"], c["timesteps"]
    assert c["micro"] == (2 if case == "accumulate2" else 1) and ch == {"c1": 1, "c2": 2}.get(case, 3)
    assert (c["pred_noise_loss_weight"], c["pred_x_start_loss_weight"]) == ((0.5, 0.25) if case == "weights" else (0.1, 0.1))
    assert c["clamp_margin"] >= 1e-3 and c["s0_range"][0] <= 0.35 and c["s0_range"][1] >= 0.65
    if case != "random_t":
        assert c["t"][0].tolist() == [0, 1, T // 2, T - 1]
        lo, _, mid, hi = c["clamp_share"][0]
        assert lo == 0.0 and 0.1 <= mid <= 0.9 and hi >= 0.9
    rows = c["final_conv_row_norms"]
    assert rows.numel() == 2 * ch + 2 and bool((rows > 0).all())
    assert abs(float(rows[-1]) - float(rows[-2])) <= 1e-5 * float(rows[-1])
    assert bool(torch.isfinite(c["final_conv_weight_grad"]).all()) and bool(torch.isfinite(c["ref_err_grads"]).all())
