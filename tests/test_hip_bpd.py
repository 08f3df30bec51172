"""Bits-per-dim evaluation on the GPU (fixture: tests/golden/make_golden_bpd.py, Improved DDPM's loop composed from the
reference's functions, run in fp64).

Every golden case runs through ``calc_bpd_loop`` with the injected noise.  Per entry ``|got - want| <= lim * |want|`` with
``lim = max(4 x the array's stored reference fp32 error, 2e-5)``; the measured worst of every array is printed (run with -s
to see them).  One column is held apart, named by the generator (``excepted``): ``vb`` at t = 999 of the T = 1000 case is
8e-7 bits left over after the O(1) terms of ``normal_kl`` cancel, and the reference's own fp32 run is 22 % off there.  Its
limit is the same rule in absolute form, ``|got - want| <= 4 x the reference's absolute fp32 error`` in that column
(6.9e-7 bits); ``ref_err`` and the relative limit cover the array's other columns.  Graph replay gives
the bits of the eager loop; one capture per shape serves different ``times``; on the Philox path two shards with
``sample_offset`` give the bits of the whole batch, ``bpd_global`` at world size 1 likewise, and the same seed gives the
same result twice."""
import os

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2e-5
ARRAYS = ("vb", "xstart_mse", "mse", "prior_bpd", "total_bpd")
CASES = ["learned_cosine24", "noise_linear24", "v_sigmoid24", "x0_cosine24_noclip", "text_linear24", "imgcond_linear24",
         "noise_linear1000_subset"]


@pytest.fixture(scope="module")
def golden():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bpd.pt")
    return torch.load(path, weights_only=True)


def _obj(golden, case, **kw):
    ukw = golden["unet_kw"][case["kind"]]
    net = dm.Unet(device=DEV, **ukw)
    net.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(UnetConfig(**ukw)), salt=golden["salt"]))
    dkw = dict(image_size=golden["image_size"], timesteps=case["timesteps"], beta_schedule=case["beta_schedule"],
               objective=case["objective"], **kw)
    if case["kind"] == "learned":
        return dm.LearnedGaussianDiffusion(net, **dkw)
    if case["kind"] == "text":
        return dm.TextConditionalDenoisingDiffusion(model=net, **dkw)
    if case["kind"] == "imgcond":
        return dm.ImageConditionalDenoisingDiffusion(net, **dkw)
    return dm.DenoisingDiffusion(net, **dkw)


def _extra(case):
    return {"text": {"text_emb": case["extra"]}, "imgcond": {"cond": case["extra"]}}.get(case["kind"], {})


def _run(obj, golden, case, **kw):
    img = golden["image_u8"].float() / 255.0
    return obj.calc_bpd_loop(img, case["clip_denoised"], times=case["times"], **_extra(case), **kw)


def _same(a, b):
    assert a["times"] == b["times"] and (a["total_bpd"] is None) == (b["total_bpd"] is None)
    return all(torch.equal(a[k], b[k]) for k in ARRAYS if a[k] is not None)


@pytest.mark.parametrize("key", CASES)
def test_loop_vs_reference_graph_and_eager(golden, key):
    case = golden["cases"][key]
    obj = _obj(golden, case)
    outs = {}
    for use_graph in (True, False):
        obj.use_graph = use_graph
        outs[use_graph] = _run(obj, golden, case, noise=so.NoiseStream(case["noise_seed"]))
    got = outs[True]
    T = case["timesteps"]
    assert got["times"] == (case["times"] if case["times"] is not None else list(reversed(range(T))))
    assert (got["total_bpd"] is None) == (case["times"] is not None) and set(case["want"]) == {k for k in ARRAYS if got[k] is not None}
    worst = {}
    for name, want in case["want"].items():
        g = got[name].cpu().double()
        assert g.shape == want.shape and bool(torch.isfinite(g).all()), name
        err = (g - want).abs() / want.abs()
        exc = case["excepted"].get(name)
        if exc:  # the named columns against their own absolute limit, the others against the relative one
            cols = [got["times"].index(t) for t in exc["times"]]
            abs_err, abs_lim = float((g - want)[:, cols].abs().max()), 4 * exc["ref_abs_err"]
            print(f"calc_bpd_loop {key} {name} at t in {exc['times']}: worst entry {abs_err:.3e} bits limit {abs_lim:.3e} bits "
                  f"(reference fp32 {exc['ref_abs_err']:.3e} bits; relative {float(err[:, cols].max()):.3e})")
            worst[f"{name} excepted"] = (abs_err, abs_lim)
            err = err[:, [k for k in range(err.shape[1]) if k not in cols]]
        lim = max(4 * case["ref_err"][name], FLOOR)
        worst[name] = (float(err.max()), lim)
        print(f"calc_bpd_loop {key} {name}: worst entry {float(err.max()):.3e} limit {lim:.3e} "
              f"(reference fp32 {case['ref_err'][name]:.3e})")
    for name, (err, lim) in worst.items():
        assert err <= lim, (key, name, err, lim)
    assert _same(outs[True], outs[False])  # graph replay is the eager loop bit for bit
    if got["total_bpd"] is not None:
        assert torch.equal(got["total_bpd"], (got["vb"].double().sum(1) + got["prior_bpd"].double()).float())


def test_one_capture_per_shape_serves_any_times(golden):
    case = golden["cases"]["noise_linear24"]
    obj = _obj(golden, case)
    net = obj.model
    img = golden["image_u8"].float() / 255.0
    assert net.graph_captures == 0
    full = obj.calc_bpd_loop(img, seed=11)
    assert net.graph_captures == 1 and full["vb"].shape == (3, 24)
    sub = obj.calc_bpd_loop(img, seed=11, times=(23, 5, 0))
    assert net.graph_captures == 1 and sub["total_bpd"] is None and sub["vb"].shape == (3, 3)
    # step k draws k + 1 whatever its time: the first column sees the same noise in both calls, the others do not
    assert torch.equal(sub["vb"][:, 0], full["vb"][:, 0]) and torch.equal(sub["prior_bpd"], full["prior_bpd"])
    rev = obj.calc_bpd_loop(img, seed=12, times=range(24))
    assert net.graph_captures == 1 and rev["total_bpd"] is not None and rev["times"] == list(range(24))
    obj.calc_bpd_loop(img, False, seed=11)  # clip_denoised is an argument of the captured term kernel
    assert net.graph_captures == 2
    obj.calc_bpd_loop(img[:2], False, seed=11)
    assert net.graph_captures == 3


@pytest.mark.parametrize("key", ["learned_cosine24", "text_linear24", "imgcond_linear24"])
def test_philox_shards_equal_the_whole_batch(golden, key):
    case = golden["cases"][key]
    obj = _obj(golden, case)
    img = golden["image_u8"].float() / 255.0
    extra = _extra(case)
    whole = obj.calc_bpd_loop(img, seed=77, **extra)
    again = obj.calc_bpd_loop(img, seed=77, **extra)
    assert _same(whole, again)  # the same seed, the same result
    other = obj.calc_bpd_loop(img, seed=78, **extra)
    assert not torch.equal(whole["vb"], other["vb"]) and torch.equal(whole["prior_bpd"], other["prior_bpd"])
    parts = [obj.calc_bpd_loop(img[lo:hi], seed=77, sample_offset=lo, **{k: v[lo:hi] for k, v in extra.items()})
             for lo, hi in ((0, 1), (1, 3))]
    for name in ARRAYS:
        assert torch.equal(torch.cat([p[name] for p in parts]), whole[name]), name
    glob = dm.bpd_global(obj, img, seed=77, **extra)  # world size 1
    assert _same(glob, whole)
    obj.use_graph = False
    assert _same(obj.calc_bpd_loop(img, seed=77, **extra), whole)
    assert bool(torch.isfinite(whole["total_bpd"]).all()) and float(whole["total_bpd"].min()) > 0


def test_a_batch_whose_results_fill_several_workgroups(golden):
    """3 B > 256: the finishing pass runs in several workgroups, and the last of them advances the step.  A loop over
    three times gives, column by column, the bits of three one-step loops on the same noise rows and the same batch."""
    case = golden["cases"]["noise_linear24"]
    obj = _obj(golden, case)
    B = 90
    img = (golden["image_u8"].float() / 255.0).repeat(B // 3, 1, 1, 1)
    img = img.roll(1, dims=3) * torch.linspace(0.5, 1.0, B).reshape(B, 1, 1, 1)  # the images differ
    times = (23, 5, 0)
    rows = [so.NoiseStream(900 + k)(img.shape) for k in range(3)]
    it = iter(rows)
    whole = obj.calc_bpd_loop(img, times=times, noise=lambda shape: next(it))
    assert whole["vb"].shape == (B, 3) and all(bool(torch.isfinite(whole[k]).all()) for k in ("vb", "xstart_mse", "mse", "prior_bpd"))
    for k, t in enumerate(times):
        one = obj.calc_bpd_loop(img, times=(t,), noise=lambda shape, k=k: rows[k])
        for name in ("vb", "xstart_mse", "mse"):
            assert torch.equal(one[name][:, 0], whole[name][:, k]), (name, t)
    assert len({float(v) for v in whole["vb"][:, 1]}) == B  # one result per image
    assert float(whole["vb"][:, 2].min()) > 30 * float(whole["vb"][:, 0].max())  # t = 0 against t = 23: the columns are the steps'


def test_refusals_of_the_library(golden):
    import ctypes as C

    from diffusion_models_amd import _lib

    case = golden["cases"]["noise_linear24"]
    obj = _obj(golden, case)
    lib = _lib.load()
    img = golden["image_u8"].float() / 255.0
    lv = dm.LearnedGaussianDiffusion.__new__(dm.LearnedGaussianDiffusion)
    lv.__dict__.update(obj.__dict__)  # the learned loop on a plain U-Net: the library names what it needs
    with pytest.raises(RuntimeError, match="2 \\* channels"):
        lv.calc_bpd_loop(img, times=(3,))
    a = _lib.BpdArgs()
    assert lib.dm_eval_bpd(obj.model._handle, C.byref(a)) != 0 and b"null argument" in lib.dm_last_error()
    out = obj.calc_bpd_loop(img, times=(3,), seed=1)  # the handle stays usable
    assert bool(torch.isfinite(out["vb"]).all())
