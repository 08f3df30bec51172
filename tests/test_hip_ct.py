"""Continuous-time Gaussian diffusion on the GPU (fixture: tests/golden/make_golden_ct.py, from the reference).

* every dm_op_ct_* pass against an fp64 evaluation of its formula on the same fp32 inputs and table scalars (first, middle
  and last row of a real schedule, and the cosine t = 1 row with alpha ~ 4e-8): rel-L2 <= 1e-6 on what the pass writes --
  each output is a handful of fp32 roundings of its inputs;
* ``p_sample`` against the reference's recorded steps: <= 1e-4 (the project's ceiling for one forward);
* ``sample()`` against every recorded loop, hipGraph replay and eager: <= 1e-3 (the ceiling for a loop), graph == eager bit
  for bit;
* the seeded Philox path (reproducible, shardable) and graph caching.
Measured errors are printed (run with -s to see them)."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import continuous as K
from diffusion_models_amd.spec import UnetConfig
from oracle import sampler_oracle as so

import ct_oracle as co
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OP_TOL = 1e-6
STEP_TOL = 1e-4
LOOP_TOL = 1e-3
CLASSES = {"noise": dm.ContinuousTimeGaussianDiffusion, "v": dm.VParamContinuousTimeGaussianDiffusion}
OBJ = {"noise": co.NOISE, "v": co.V}
SHAPES = [(B, shape) for B in (1, 3, 5) for shape in ((1, 4, 4), (3, 8, 8), (3, 16, 16))]  # per = 16: one float4 group per block edge


@pytest.fixture(scope="module")
def golden():
    return load_golden("ct.pt")


def _fp(t):
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rows():
    """First, middle and last (sqrt_var == 0) row of the linear schedule and the cosine t = 1 row (alpha ~ 4e-8)."""
    lin, cos = dm.ct_step_table(8, "linear"), dm.ct_step_table(8, "cosine")
    rows = torch.stack([lin[0], lin[4], lin[7], cos[0]]).contiguous()
    assert float(rows[2, K.SQRT_VAR]) == 0 and all(float(rows[i, K.SQRT_VAR]) != 0 for i in (0, 1, 3))
    assert float(rows[3, K.ALPHA]) < 1e-7
    return rows


def _net(ukw, salt):
    cfg = UnetConfig(channels=3, **ukw)
    u = dm.Unet(channels=3, device=DEV, **ukw)
    u.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt))
    return u


def _obj(kind, ukw, salt, **kw):
    return CLASSES[kind](_net(ukw, salt), **kw)


# ---- operators ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective,clip", [(co.V, 1), (co.V, 0), (co.NOISE, 1), (co.NOISE, 0)],
                         ids=["v-clip", "v-noclip", "noise-clip", "noise-noclip"])
@pytest.mark.parametrize("B,shape", SHAPES)
def test_op_step_vs_fp64(objective, clip, B, shape):
    lib = _lib.load()
    rows = _rows()
    per = shape[0] * shape[1] * shape[2]
    has_xs = not (objective == co.NOISE and not clip)

    def run(tab, x, F, eps):
        out = torch.empty((B, per), device=DEV)
        xs = torch.empty((B, per), device=DEV) if has_xs else None
        xd, Fd, ed = x.to(DEV), F.to(DEV), eps.to(DEV)
        _lib.check(lib.dm_op_ct_step(_lib.ptr(xd), _lib.ptr(Fd), _lib.ptr(ed), _fp(tab), tab.shape[0], objective, clip, 0, 1, 0,
                                     _lib.ptr(out), _lib.ptr(xs), B, per, None))
        return out.cpu(), (xs.cpu() if has_xs else None)

    def check(tag, tab, x, F, eps):
        out, xs = run(tab, x, F, eps)
        want, want_xs = co.step(x.double(), F.double(), eps.double(), tab.double(), objective, clip)
        err = rel_l2(out, want)
        print(f"op ct_step {tag} B={B} {shape} out: {err:.3e}")
        assert err <= OP_TOL and bool(torch.isfinite(out).all())
        if has_xs:
            e2 = rel_l2(xs, want_xs)
            print(f"op ct_step {tag} B={B} {shape} x_start: {e2:.3e}")
            assert e2 <= OP_TOL

    for i in range(rows.shape[0]):  # rows == 1: one row for every image
        x, F, eps = _randn((B, per), 10 + i), _randn((B, per), 20 + i), _randn((B, per), 30 + i)
        if float(rows[i, K.SQRT_VAR]) == 0:
            eps = torch.full((B, per), float("nan"))  # the last step must not read its noise
        check(f"row {i}", rows[i:i + 1].contiguous(), x, F, eps)
    if B > 1:  # rows == B: row b for image b; the images on the sqrt_var == 0 row get NaN noise
        tab = rows[torch.arange(B) % rows.shape[0]].contiguous()
        x, F, eps = _randn((B, per), 41), _randn((B, per), 42), _randn((B, per), 43)
        eps[tab[:, K.SQRT_VAR] == 0] = float("nan")
        check("rows == B", tab, x, F, eps)


def test_op_step_x_start_is_refused_where_none_is_formed():
    lib = _lib.load()
    row = _rows()[:1].contiguous()
    x = _randn((2, 16), 1).to(DEV)
    out, xs = torch.empty_like(x), torch.empty_like(x)
    rc = lib.dm_op_ct_step(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _fp(row), 1, co.NOISE, 0, 0, 1, 0, _lib.ptr(out), _lib.ptr(xs),
                           2, 16, None)
    assert rc != 0 and b"x_start" in lib.dm_last_error()
    rc = lib.dm_op_ct_step(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _fp(row), 1, 7, 0, 0, 1, 0, _lib.ptr(out), None, 2, 16, None)
    assert rc != 0 and b"objective" in lib.dm_last_error()
    rc = lib.dm_op_ct_step(_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _fp(row), 1, co.V, 0, 0, 1, 0, _lib.ptr(out), None, 1, 6, None)
    assert rc != 0 and b"multiple of 4" in lib.dm_last_error()  # 6 floats: no whole float4 groups


def test_op_step_philox_is_the_dm_randn_stream():
    lib = _lib.load()
    row = _rows()[1:2].contiguous()
    B, per = 3, 3 * 16 * 16
    x, F = _randn((B, per), 50).to(DEV), _randn((B, per), 51).to(DEV)
    seed, draw, off = 1234, 7, 4 * 100
    z = torch.empty_like(x)
    _lib.check(lib.dm_randn(_lib.ptr(z), z.numel(), seed, draw, off, None))
    outs = []
    for eps in (z, None):
        out = torch.empty_like(x)
        _lib.check(lib.dm_op_ct_step(_lib.ptr(x), _lib.ptr(F), _lib.ptr(eps), _fp(row), 1, co.V, 1, seed, draw, off,
                                     _lib.ptr(out), None, B, per, None))
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    last = _rows()[2:3].contiguous()  # sqrt_var == 0: no draw either
    a, b = torch.empty_like(x), torch.empty_like(x)
    _lib.check(lib.dm_op_ct_step(_lib.ptr(x), _lib.ptr(F), None, _fp(last), 1, co.V, 1, seed, draw, off, _lib.ptr(a), None, B, per, None))
    _lib.check(lib.dm_op_ct_step(_lib.ptr(x), _lib.ptr(F), None, _fp(last), 1, co.V, 1, seed + 1, draw + 1, 0, _lib.ptr(b), None, B, per, None))
    assert torch.equal(a, b) and not torch.equal(a, outs[0])


@pytest.mark.parametrize("objective", [co.NOISE, co.V], ids=["noise", "v"])
@pytest.mark.parametrize("B,shape", SHAPES)
def test_op_noise_in_vs_fp64(objective, B, shape):
    lib = _lib.load()
    g = torch.Generator().manual_seed(61)
    per = shape[0] * shape[1] * shape[2]
    times = torch.tensor([0.0, 0.3, 0.7, 1.0, 0.5])
    for rows, sched in ((B, "cosine"), (1, "linear")):
        tab = dm.ct_train_table(times[:rows] if rows > 1 else times[1:2], sched).contiguous()
        img, eps = torch.rand((B, per), generator=g), torch.randn((B, per), generator=g)
        for normalize in (1, 0):
            src = img if normalize else img * 2 - 1
            x, target = torch.empty((B, per), device=DEV), torch.empty((B, per), device=DEV)
            sd, ed = src.to(DEV), eps.to(DEV)
            _lib.check(lib.dm_op_ct_noise_in(_lib.ptr(sd), _lib.ptr(ed), _fp(tab), tab.shape[0], objective, normalize,
                                             _lib.ptr(x), _lib.ptr(target), B, per, None))
            wx, wt = co.noise_in(src.double(), eps.double(), tab.double(), objective, bool(normalize))
            ex, et = rel_l2(x.cpu(), wx), rel_l2(target.cpu(), wt)
            print(f"op ct_noise_in B={B} {shape} rows={rows} normalize={normalize}: x {ex:.3e} target {et:.3e}")
            assert ex <= OP_TOL and et <= OP_TOL
            if objective == co.NOISE:
                assert torch.equal(target.cpu(), eps)


@pytest.mark.parametrize("mixed", [False, True], ids=["w1", "mixed"])
@pytest.mark.parametrize("B,shape", SHAPES)
def test_op_loss_vs_fp64(mixed, B, shape):
    lib = _lib.load()
    g = torch.Generator().manual_seed(62)
    per = shape[0] * shape[1] * shape[2]
    times = torch.tensor([0.05, 0.2, 0.5, 0.9, 0.7])[:B]
    tab = dm.ct_train_table(times, "cosine", mixed, 5).contiguous()
    if mixed and B > 1:
        assert bool((tab[:, K.LOSS_W] == 1).any()) and bool((tab[:, K.LOSS_W] > 1).any())
    F, target = torch.randn((B, per), generator=g), torch.randn((B, per), generator=g)
    dF = torch.empty((B, per), device=DEV)
    loss = C.c_float(0.0)
    Fd, td = F.to(DEV), target.to(DEV)
    _lib.check(lib.dm_op_ct_loss(_lib.ptr(Fd), _lib.ptr(td), _fp(tab), 0.5, _lib.ptr(dF), C.byref(loss), B, per, None))
    wl, wdF = co.loss_and_dF(F.double(), target.double(), tab.double(), loss_scale=0.5)
    el, eg = abs(loss.value - float(wl)) / abs(float(wl)), rel_l2(dF.cpu(), wdF)
    print(f"op ct_loss B={B} {shape} mixed={mixed}: loss {el:.3e} dF {eg:.3e}")
    assert el <= OP_TOL and eg <= OP_TOL
    for b in range(B):  # every image on its own scale
        assert rel_l2(dF[b].cpu(), wdF[b]) <= OP_TOL, b


# ---- p_sample and q_sample against the reference --------------------------------------------------------------------------
def test_p_sample_vs_reference(golden):
    for key, g in golden["steps_single"].items():
        obj = _obj(g["kind"], g["unet_kw"], g["salt"], image_size=16, **g["ct_kw"])
        for st in g["steps"]:
            last = float(st["time_next"]) == 0
            eps = None if last else so.NoiseStream(st["noise_seed"])(g["x"].shape)
            got = obj.p_sample(g["x"], st["time"], st["time_next"], noise=eps).cpu()
            err = rel_l2(got, st["y"])
            print(f"p_sample {key} step {st['i']}: {err:.3e}")
            assert err <= STEP_TOL, (key, st["i"], err)
        st = g["steps"][1]
        mean, var = obj.p_mean_variance(g["x"], st["time"], st["time_next"])
        names = golden["names"]
        assert float(var) == float(st["scalars"][0, names.index("posterior_variance")])
        noisy = obj.p_sample(g["x"], st["time"], st["time_next"], noise=torch.zeros_like(g["x"]))
        assert torch.equal(mean, noisy)  # mean + sqrt_var * 0


def test_q_sample_vs_reference(golden):
    q = golden["q_sample"]
    net = _net(golden["state_dict_unet_kw"], 85)
    for key, kind, kw in (("noise_linear", "noise", dict(noise_schedule="linear")),
                          ("noise_cosine", "noise", dict(noise_schedule="cosine")), ("v", "v", {})):
        obj = CLASSES[kind](net, image_size=16, **kw)
        got = obj.q_sample(q["x_start"], q["times"], noise=q["noise"])
        assert len(got) == len(q[key]) == (2 if kind == "noise" else 4)
        err = rel_l2(got[0].cpu(), q[key][0])
        print(f"q_sample {key}: {err:.3e}")
        assert err <= OP_TOL
        for a, b in zip(got[1:], q[key][1:]):
            assert a.shape == b.shape and torch.equal(a.cpu(), b)
    assert list(obj.state_dict().keys()) == golden["state_dict_keys"]["v"]


# ---- loops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["v_n8", "v_n8_noclip", "lin_n8", "cos_n12", "v_d64_n6", "v_rff_n8"])
def test_sample_vs_reference(golden, key):
    c = golden["loops"][key]
    want = c["sample"]
    share = float(((want == 0) | (want == 1)).float().mean())
    assert share <= 0.5, (key, share)  # the comparison is not carried by the final clamp
    obj = _obj(c["kind"], c["unet_kw"], c["salt"], image_size=c["image_size"], num_sample_steps=c["n"], **c["ct_kw"])
    outs = {}
    for use_graph in (True, False):
        obj.use_graph = use_graph
        got = obj.sample(batch_size=c["batch"], noise=so.NoiseStream(c["noise_seed"])).cpu()
        assert got.shape == want.shape
        err = rel_l2(got, want)
        print(f"sample {key} {'graph' if use_graph else 'eager'} (N = {c['n']}, {share:.0%} on the final clamp): {err:.3e}")
        assert err <= LOOP_TOL
        outs[use_graph] = got
    assert torch.equal(outs[True], outs[False])


def test_seeded_sampling_is_reproducible_and_shardable(golden):
    c = golden["loops"]["v_n8"]
    for kind, kw in (("v", {}), ("noise", dict(noise_schedule="linear"))):
        obj = _obj(kind, c["unet_kw"], c["salt"], image_size=16, num_sample_steps=6, **kw)
        a = obj.sample(batch_size=4, seed=77)
        assert torch.equal(a, obj.sample(batch_size=4, seed=77))
        assert not torch.equal(a, obj.sample(batch_size=4, seed=78))
        halves = torch.cat((obj.sample(batch_size=2, seed=77), obj.sample(batch_size=2, seed=77, sample_offset=2)))
        assert torch.equal(a, halves)
        assert 0.0 <= float(a.min()) and float(a.max()) <= 1.0 and float(a.std()) > 0.01
        assert torch.equal(dm.sample_global(obj, 4, seed=77), a)


def test_graph_caching(golden):
    c = golden["loops"]["v_n8"]
    obj = _obj("v", c["unet_kw"], c["salt"], image_size=16, num_sample_steps=8)
    net = obj.model
    assert net.graph_captures == 0
    a = obj.sample(batch_size=2, seed=5)
    assert net.graph_captures == 1  # every step, the last included, is the same graph
    assert torch.equal(a, obj.sample(batch_size=2, seed=5)) and net.graph_captures == 1
    obj.num_sample_steps = 5  # a sampling-time choice: same graph, another table
    obj.sample(batch_size=2, seed=6)
    assert net.graph_captures == 1
    obj.clip_sample_denoised = False  # a kernel argument of the captured step
    obj.sample(batch_size=2, seed=6)
    assert net.graph_captures == 2
    noise_obj = dm.ContinuousTimeGaussianDiffusion(net, image_size=16, noise_schedule="cosine", num_sample_steps=5)
    noise_obj.sample(batch_size=2, seed=6)
    assert net.graph_captures == 3
    noise_obj.sample(batch_size=3, seed=6)
    assert net.graph_captures == 4
    # the EDM loops on the same handle keep their own graphs apart
    edm = dm.ElucidatedDiffusion(net, image_size=16, num_sample_steps=6)
    e1 = edm.sample_using_dpmpp(batch_size=3, seed=9)
    assert net.graph_captures == 5
    noise_obj.sample(batch_size=3, seed=6)
    assert net.graph_captures == 6
    assert torch.equal(e1, edm.sample_using_dpmpp(batch_size=3, seed=9))
