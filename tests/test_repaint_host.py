"""RePaint inpainting, host logic, no GPU: the flattened row table against the ``p_sample`` call sequence, frame count and
schedule buffers recorded from the running reference, the CPU restatement of the kernel's arithmetic (tests/repaint_oracle.py)
against the reference's recorded ``sample()`` / ``p_sample`` outputs, the mirrored surface, the refusals and the C ABI
additions.  Fixture: tests/golden/make_golden_repaint.py."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import repaint as R
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so
from oracle import unet_oracle as uo

import repaint_oracle as ro
from conftest import ROOT, load_golden, rel_l2

SAMPLE_TOL = 1e-4  # the project's sample tolerance (README, test_hip_configs.py)
OBJ = {"pred_noise": 0, "pred_x0": 1, "pred_v": 2}


def limit(ref_err):
    """relative L2 <= max(1e-4, 4 x the reference's own fp32-vs-fp64 error of the case)."""
    return max(SAMPLE_TOL, 4.0 * ref_err)


@pytest.fixture(scope="module")
def golden():
    return load_golden("repaint.pt")


def _table(g, key):
    c = g["loops"][key]
    kw = {k: v for k, v in c["sample_kw"].items() if k != "return_all_timesteps"}
    kw.setdefault("resample_jump", 10)  # sample()'s own default
    sched = dm.make_schedule(g["timesteps"], c["diffusion_kw"]["beta_schedule"])
    return c, sched, dm.repaint_step_table(sched, **kw)


def test_table_reproduces_the_recorded_call_sequence(golden):
    for key in ("a", "b", "c", "d", "e"):
        c, _, tab = _table(golden, key)
        assert [(t, True) for t in tab.times] == [tuple(v) for v in c["calls"]], key
        assert tab.coefs.shape == (len(tab.times), _lib.DM_REPAINT_COEFS) and tab.coefs.dtype == torch.float32
    c, _, tab = _table(golden, "e")
    assert tab.n_frames == c["shape"][1]
    slots = [int(s) for s in tab.coefs[:, R.SLOT] if s >= 0]
    assert slots == list(range(1, tab.n_frames))  # every frame but x_T is written once, in order
    c, _, tab = _table(golden, "c")
    assert tab.times == list(reversed(range(20))) and not bool(tab.coefs[:, R.JUMP].any())
    # without a mask the reference's loop is the plain DDPM loop
    assert [tuple(v) for v in golden["loops"]["g"]["calls"]] == [(t, False) for t in reversed(range(20))]


@pytest.mark.parametrize("T,kw,events", [
    (1000, {}, 20),  # the defaults: t = 950, 900, ..., 50 and t = 1
    (20, dict(resample_iter=2, resample_jump=3, resample_every=4), 5),
    (20, dict(resample_iter=3, resample_jump=19, resample_every=7), 3),
    (20, dict(resample_iter=1, resample_jump=1, resample_every=1), 19),  # t == 1 is an event once, not twice
    (20, dict(resample=False), 0),
    (20, dict(resample=1), 0),  # the reference tests `resample is True`
])
def test_row_count(T, kw, events):
    tab = dm.repaint_step_table(dm.make_schedule(T, "sigmoid"), **kw)
    it, jump = kw.get("resample_iter", 10), kw.get("resample_jump", 10)
    assert len(tab.times) == T + events * it * jump
    assert tab.n_frames == 1 + T + events
    assert int(tab.coefs[:, R.JUMP].sum()) == events * it
    if T == 1000:
        assert len(tab.times) == 3000


def test_scalars_equal_the_reference_buffers_bitwise(golden):
    for name in ("cosine", "sigmoid"):
        buf = golden["buffers"][name]
        sched = dm.make_schedule(golden["timesteps"], name)
        assert torch.equal(sched["betas"], buf["betas"]) and torch.equal(sched["alphas_cumprod"], buf["alphas_cumprod"])
        tab = dm.repaint_step_table(sched, True, 2, 3, 4)
        _, ddpm = dm.spec.ddpm_step_table(sched)
        for r, t in enumerate(tab.times):
            row = tab.coefs[r]
            ac = buf["alphas_cumprod"][t]
            assert torch.equal(row[:8], ddpm[golden["timesteps"] - 1 - t])
            assert float(row[R.KNOWN_GT]) == float(torch.sqrt(ac)) and float(row[R.KNOWN_Z]) == float(torch.sqrt(1 - ac))
            if float(row[R.JUMP]) != 0:
                beta = buf["betas"][3]  # indexed by resample_jump, not by t
                assert float(row[R.JUMP_X]) == float(torch.sqrt(1 - beta)) and float(row[R.JUMP_Z]) == float(torch.sqrt(beta))
                assert t == 3
            else:
                assert float(row[R.JUMP_X]) == 1.0 and float(row[R.JUMP_Z]) == 0.0
            assert not bool(row[14:].any())


def test_bad_resampling_settings_are_refused():
    sched = dm.make_schedule(20, "cosine")
    for bad in (0, -1, 20, 25, 2.0, True):
        with pytest.raises(ValueError):
            dm.repaint_step_table(sched, True, 2, bad, 4)
    dm.repaint_step_table(sched, True, 2, 19, 4)
    dm.repaint_step_table(sched, False, 2, 99, 4)  # nothing resamples: the reference never reads the setting
    for bad_iter in (0, -2):
        with pytest.raises(ValueError):
            dm.repaint_step_table(sched, True, bad_iter, 3, 4)
    with pytest.raises(ValueError):
        dm.repaint_step_table(sched, True, 2, 3, 0)


def _fwd(g):
    cfg = UnetConfig(channels=3, **g["unet_kw"])
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=g["salt"])
    return lambda x, t: uo.unet_forward(sd, cfg, x, t)


@pytest.mark.parametrize("key", ["a", "b", "c", "d"])
def test_restated_loop_reproduces_the_reference(golden, key):
    c, _, tab = _table(golden, key)
    shape = tuple(c["sample"].shape)
    with torch.inference_mode():
        got = ro.sample(_fwd(golden), tab, shape, golden["gt"], c["mask"], so.NoiseStream(golden["noise_seed"]),
                        OBJ[c["diffusion_kw"]["objective"]], unnormalize=c["diffusion_kw"].get("auto_normalize", True))
    err = rel_l2(got, c["sample"])
    print(f"repaint oracle loop {key}: rel-L2 {err:.3e} (limit {limit(c['ref_err']):.1e}, reference fp32-vs-fp64 {c['ref_err']:.2e})")
    assert err <= limit(c["ref_err"]), (key, err)
    known = c["mask"].expand(shape) == 1
    want = golden["gt"] * 2 - 1
    want = (want + 1) * 0.5 if c["diffusion_kw"].get("auto_normalize", True) else want
    assert torch.equal(c["sample"][known], want[known])  # pred drops out of the known region
    assert torch.equal(got[known], c["sample"][known])


def test_restated_loop_frames(golden):
    c, _, tab = _table(golden, "e")
    with torch.inference_mode():
        got = ro.sample(_fwd(golden), tab, (2, 3, 16, 16), golden["gt"], c["mask"], so.NoiseStream(golden["noise_seed"]), 0,
                        return_all_timesteps=True)
    assert tuple(got.shape) == tuple(c["shape"])
    assert rel_l2(got[:, -c["n_last"]:], c["last_frames"]) <= limit(c["ref_err"])


def test_restated_p_sample_reproduces_the_reference(golden):
    p = golden["p_sample"]
    fwd = _fwd(golden)
    for objective, case in p["steps"].items():
        sched = dm.make_schedule(golden["timesteps"], case["diffusion_kw"]["beta_schedule"])
        for st in case["steps"]:
            with torch.inference_mode():
                y, xs = ro.p_sample(fwd, sched, p["x"], st["t"], golden["gt"], p["mask"], so.NoiseStream(st["noise_seed"]),
                                    OBJ[objective])
            assert rel_l2(y, st["y"]) <= limit(st["ref_err"]), (objective, st["t"], rel_l2(y, st["y"]))
            assert rel_l2(xs, st["x_start"]) <= limit(st["ref_err"]), (objective, st["t"])


def _fake_model(self_condition=False):
    return types.SimpleNamespace(channels=3, out_dim=3, self_condition=self_condition, device="cpu", downsample_factor=2)


def test_surface_matches_the_reference(golden):
    s = golden["surface"]
    cls = dm.RePaintGaussianDiffusion
    assert cls is R.GaussianDiffusion and issubclass(cls, dm.DenoisingDiffusion)
    ours = inspect.signature(cls.__init__).parameters
    for name, default, kind in s["init_params"]:
        assert name in ours, name
        assert ours[name].kind.name == kind, name
        if default is None and name in ("model", "image_size"):
            assert ours[name].default is inspect.Parameter.empty
        else:
            assert ours[name].default == default, (name, ours[name].default, default)
    assert set(ours) - {n for n, _, _ in s["init_params"]} == {"self", "use_graph"}
    assert not {"hybrid_loss", "immiscible", "ddpm"} & set(ours)
    for meth, params in s["methods"].items():
        mine = [p for p in inspect.signature(getattr(cls, meth)).parameters.values() if p.name != "self"]
        head = [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in mine[:len(params)]]
        assert head == [tuple(p) for p in params], meth  # the reference's positional order and defaults
        assert all(p.kind in (p.KEYWORD_ONLY, p.VAR_KEYWORD) for p in mine[len(params):]), meth
    assert dict(s["methods"]["sample"])["resample_jump"] == 10 and dict(s["methods"]["p_sample_loop"])["resample_jump"] == 3
    assert not set(s["names"]) - set(dir(cls)), sorted(set(s["names"]) - set(dir(cls)))
    d = cls(_fake_model(), image_size=16, timesteps=20)
    assert d.objective == "pred_v" and d.num_timesteps == 20 and not d.is_ddim_sampling
    want = dm.make_schedule(20, "sigmoid", ddpm=False, objective="pred_v")
    assert all(torch.equal(getattr(d, k), v) for k, v in want.items())


def test_self_conditioning_with_a_mask_is_refused():
    d = dm.RePaintGaussianDiffusion(_fake_model(self_condition=True), image_size=16, timesteps=20)
    gt, mask = torch.zeros(2, 3, 16, 16), torch.ones(2, 1, 16, 16)
    with pytest.raises(NotImplementedError):
        d.sample(gt=gt, mask=mask)
    with pytest.raises(NotImplementedError):
        d.p_sample(torch.zeros(2, 3, 16, 16), 3, gt=gt, mask=mask)


def test_draw_ids_do_not_collide():
    ids = [i for r in range(3000) for i in R.draw_ids(r)]
    assert len(set(ids)) == len(ids) and min(ids) == 1  # draw 0 is x_T
    assert R.draw_ids(0) == (1, 2, 3) and R.draw_ids(7) == (22, 23, 24)
    src = open(os.path.join(ROOT, "diffusion-models_amd", "csrc", "repaint.h")).read()
    for name, k in (("jump", 1), ("known", 2), ("step", 3)):
        assert re.search(rf"repaint_draw_{name}\(uint64_t r\) \{{ return 3 \* r \+ {k}; \}}", src), name


def test_abi_additions():
    header = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("dm_sample_repaint", "dm_op_repaint_step"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    lib.dm_abi_version.restype = ctypes.c_int
    assert lib.dm_abi_version() == _lib.ABI_VERSION == 9
    assert int(re.search(r"#define DM_REPAINT_COEFS (\d+)", header).group(1)) == _lib.DM_REPAINT_COEFS == R.COLS
    for name, val in (("BLEND", R.BLEND), ("STEP", R.STEP), ("STEP_NEXT", R.STEP_NEXT), ("LAST", R.LAST)):
        assert int(re.search(rf"#define DM_REPAINT_{name} (\d+)", header).group(1)) == val
    # dm_repaint_args: the binding lists the header's fields in order
    body = re.search(r"typedef struct dm_repaint_args \{(.*?)\} dm_repaint_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip(" *") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.RepaintArgs._fields_]
