"""DPM-Solver++ (2M) for the continuous-time classes on the GPU (fixture: tests/golden/make_golden_ct_solver.py, the CPU
oracle loop over the reference U-Net in float64).

* ``dm_op_ct_dpmpp_step`` against a float64 evaluation of its formula on the same fp32 inputs and row: rel-L2 <= 1e-6 on
  the new x and on the history (each is a handful of fp32 roundings of its inputs), and bit for bit against the fp32
  restatement (contraction is off in the kernel and fp32 division is correctly rounded, so the same IEEE operations in
  the same order give the same bits);
* ``dpm_solver_sample`` against every recorded loop, hipGraph replay and eager: <= 1e-3 (the project's ceiling for a
  loop), graph == eager bit for bit;
* what the handle does: one capture for any N, order and spacing; the ancestral loop untouched; seeds, shards,
  ``sample_global``; the loop composed by hand from ``Unet.forward`` and the operator; a learned schedule; refusals.
Measured errors are printed (run with -s to see them)."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import continuous as K
from diffusion_models_amd.spec import UnetConfig

import ct_dpmpp_oracle as do
from conftest import load_golden, rel_l2
from test_hip_ct import LOOP_TOL, OP_TOL, SHAPES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = {"noise": dm.ContinuousTimeGaussianDiffusion, "v": dm.VParamContinuousTimeGaussianDiffusion}
D32 = dict(dim=32, dim_mults=(1, 2), learned_sinusoidal_cond=True)
SHAPE = (2, 3, 16, 16)


@pytest.fixture(scope="module")
def golden():
    return load_golden("ct_solver.pt")["cases"]


def _fp(t):
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _net(ukw, salt, cls=dm.Unet, **kw):
    u = cls(device=DEV, **dict(ukw, **kw))
    u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=salt))
    return u


def _obj(kind, ukw, salt, **kw):
    return CLASSES[kind](_net(ukw, salt, channels=3), image_size=16, **kw)


def _case_obj(c, **kw):
    ckw = dict(clip_sample_denoised=c["clip"])
    if c["kind"] == "noise":
        ckw["noise_schedule"] = c["schedule"]
    return _obj(c["kind"], c["unet_kw"], c["salt"], **ckw, **kw)


# ---- the operator ---------------------------------------------------------------------------------------------------
def _rows():
    """First and middle row of the linear table, the last row of the cosine one, and the cosine first node (alpha ~ 4e-8),
    each with g = 0 and g = 0.7."""
    lin, cos = dm.ct_dpmpp_table(8, "linear"), dm.ct_dpmpp_table(8, "cosine")
    base = torch.stack([lin[0], lin[4], cos[7], cos[0]])
    assert float(base[3, K.ALPHA]) < 1e-7
    rows = base.repeat_interleave(2, dim=0).contiguous()
    rows[0::2, K.DPM_G], rows[1::2, K.DPM_G] = 0.0, 0.7
    return rows


def _op(x, F, hist, tab, objective, clip):
    """dm_op_ct_dpmpp_step on device copies: (x_next, history afterwards); the output starts as NaN."""
    B, per = x.shape
    xd, Fd, hd = (v.to(DEV).contiguous() for v in (x, F, hist))
    out = torch.full((B, per), float("nan"), device=DEV)
    _lib.check(_lib.load().dm_op_ct_dpmpp_step(_lib.ptr(xd), _lib.ptr(Fd), _lib.ptr(hd), _fp(tab), tab.shape[0], objective,
                                               clip, _lib.ptr(out), B, per, None))
    return out.cpu(), hd.cpu()


@pytest.mark.parametrize("objective,clip", [(do.V, 1), (do.V, 0), (do.NOISE, 1), (do.NOISE, 0)],
                         ids=["v-clip", "v-noclip", "noise-clip", "noise-noclip"])
@pytest.mark.parametrize("B,shape", SHAPES)
def test_op_step_vs_fp64(objective, clip, B, shape):
    rows = _rows()
    per = shape[0] * shape[1] * shape[2]

    def check(tag, tab, x, F, hist):
        out, new_hist = _op(x, F, hist, tab, objective, clip)
        want, want_xs = do.update(x.double(), F.double(), hist.double(), tab.double(), objective, clip)
        e_out, e_xs = rel_l2(out, want), rel_l2(new_hist, want_xs)
        print(f"op ct_dpmpp_step {tag} B={B} {shape}: out {e_out:.3e}  x_start {e_xs:.3e}")
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(new_hist).all())  # every element was written
        assert e_out <= OP_TOL and e_xs <= OP_TOL
        out32, xs32 = do.update32(x, F, hist, tab, objective, clip)
        assert torch.equal(out, out32) and torch.equal(new_hist, xs32), tag

    for i in range(rows.shape[0]):  # rows == 1: one row for every image
        x, F, hist = _randn((B, per), 10 + i), _randn((B, per), 20 + i), _randn((B, per), 30 + i).clamp(-1, 1)
        if float(rows[i, K.DPM_G]) == 0:
            hist = torch.full((B, per), float("nan"))  # the first step runs over an uninitialised buffer
        check(f"row {i}", rows[i:i + 1].contiguous(), x, F, hist)
    if B > 1:  # rows == B: row b for image b; the images on a g == 0 row get a NaN history
        tab = rows[torch.arange(B) % rows.shape[0]].contiguous()
        x, F, hist = _randn((B, per), 41), _randn((B, per), 42), _randn((B, per), 43).clamp(-1, 1)
        hist[tab[:, K.DPM_G] == 0] = float("nan")
        check("rows == B", tab, x, F, hist)


def test_op_step_refusals():
    lib = _lib.load()
    row = _rows()[:1].contiguous()
    x = _randn((2, 16), 1).to(DEV)
    out, hist = torch.empty_like(x), torch.empty_like(x)
    call = lambda *a: lib.dm_op_ct_dpmpp_step(*a)  # noqa: E731
    assert call(_lib.ptr(x), _lib.ptr(x), _lib.ptr(hist), _fp(row), 1, 7, 0, _lib.ptr(out), 2, 16, None) != 0
    assert b"objective" in lib.dm_last_error()
    assert call(_lib.ptr(x), _lib.ptr(x), _lib.ptr(hist), _fp(row), 1, do.V, 0, _lib.ptr(out), 1, 6, None) != 0
    assert b"multiple of 4" in lib.dm_last_error()  # 6 floats: no whole float4 groups
    assert call(_lib.ptr(x), _lib.ptr(x), None, _fp(row), 1, do.V, 0, _lib.ptr(out), 2, 16, None) != 0
    assert call(_lib.ptr(x), _lib.ptr(x), _lib.ptr(out), _fp(row), 1, do.V, 0, _lib.ptr(out), 2, 16, None) != 0
    assert b"aliases" in lib.dm_last_error()
    two = _rows()[:2].contiguous()
    assert call(_lib.ptr(x), _lib.ptr(x), _lib.ptr(hist), _fp(two), 2, do.V, 0, _lib.ptr(out), 4, 8, None) != 0  # rows: 1 or B


# ---- loops against the float64 oracle over the reference U-Net ---------------------------------------------------------------
@pytest.mark.parametrize("key", ["v_o2", "v_o2_noclip", "v_o2_rff", "v_o1", "lin_o2_noclip", "cos_o2_noclip", "lin_o2_clip",
                                 "lin_o1_noclip"])
def test_loop_vs_float64_oracle(golden, key):
    """v cases compare the finalized sample (at most half of its pixels on the final clamp); noise cases compare the raw
    iterate, since with synthetic weights a noise-objective run ends almost entirely outside [-1, 1].  lin_o2_clip: 96 % of
    its x_start values sit on the clamp (recorded in the fixture), so it shows that the clamped loop runs and agrees, while
    the clamp's own arithmetic is what test_op_step_vs_fp64 covers."""
    c = golden[key]
    raw = c["compare"] == "x"
    want = c["x64"] if raw else c["sample64"]
    assert raw or c["clamp_share"] <= 0.5
    obj = _case_obj(c)
    outs = {}
    for use_graph in (True, False):
        obj.use_graph = use_graph
        got = obj.dpm_solver_sample(SHAPE, c["n"], c["order"], noise=lambda shape: c["x_T"], unnormalize=not raw).cpu()
        err = rel_l2(got, want)
        print(f"dpm_solver_sample {key} {'graph' if use_graph else 'eager'} ({'x' if raw else 'sample'}; the oracle's own "
              f"fp32 vs float64 {c['ref_err']:.1e}): {err:.3e}")
        assert got.shape == want.shape and err <= LOOP_TOL
        outs[use_graph] = got
    assert torch.equal(outs[True], outs[False])


# ---- what the handle does ---------------------------------------------------------------------------------------------------
def test_one_capture_serves_every_table_and_the_ancestral_loop_is_untouched(golden):
    c = golden["v_o2"]
    obj = _case_obj(c, num_sample_steps=5)
    net = obj.model
    assert net.graph_captures == 0
    a = obj.dpm_solver_sample(SHAPE, 8, 2, seed=5)  # the longest table first: a longer one would move the device table
    assert net.graph_captures == 1
    others = [obj.dpm_solver_sample(SHAPE, 6, 2, seed=5), obj.dpm_solver_sample(SHAPE, 8, 1, seed=5),
              obj.dpm_solver_sample(SHAPE, 8, 2, spacing="time", seed=5),
              obj.dpm_solver_sample(SHAPE, 8, 2, log_snr_min=-15.0, seed=5), obj.dpm_solver_sample(SHAPE, 8, 2, seed=6)]
    assert net.graph_captures == 1
    assert all(not torch.equal(a, o) for o in others)
    assert torch.equal(obj.dpm_solver_sample(SHAPE, 8, 2, seed=5), a)
    obj.clip_sample_denoised = False  # a kernel argument of the captured step
    b = obj.dpm_solver_sample(SHAPE, 8, 2, seed=5)
    assert net.graph_captures == 2 and not torch.equal(a, b)
    obj.clip_sample_denoised = True
    eager = CLASSES["v"](net, image_size=16, use_graph=False)
    assert torch.equal(eager.dpm_solver_sample(SHAPE, 8, 2, seed=5), a)
    # sample() on this handle, after the solver, against sample() on a handle that never ran it
    fresh = _case_obj(c, num_sample_steps=5)
    assert torch.equal(obj.sample(batch_size=2, seed=9), fresh.sample(batch_size=2, seed=9))
    assert torch.equal(obj.dpm_solver_sample(SHAPE, 8, 2, seed=5), a)


def test_seeded_sampling_is_reproducible_and_shardable(golden):
    c = golden["v_o2"]
    for kind, kw in (("v", {}), ("noise", dict(noise_schedule="linear"))):
        obj = _obj(kind, c["unet_kw"], c["salt"], **kw)
        a = obj.sample(batch_size=4, solver="dpmpp", num_sample_steps=6, seed=77)
        assert torch.equal(a, obj.dpm_solver_sample((4, 3, 16, 16), 6, 2, seed=77))
        assert not torch.equal(a, obj.sample(batch_size=4, solver="dpmpp", num_sample_steps=6, seed=78))
        halves = [obj.sample(batch_size=2, solver="dpmpp", num_sample_steps=6, seed=77, sample_offset=k) for k in (0, 2)]
        assert torch.equal(a, torch.cat(halves))
        assert 0.0 <= float(a.min()) and float(a.max()) <= 1.0 and float(a.std()) > 0.01
        assert torch.equal(dm.sample_global(obj, 4, seed=77, solver="dpmpp", num_sample_steps=6), a)
        calls = []

        def noise(shape):
            calls.append(tuple(shape))
            return _randn(shape, 3)

        obj.dpm_solver_sample(SHAPE, 3, 2, noise=noise)
        assert calls == [SHAPE]  # an injected noise is called once: nothing is drawn after x_T


def _by_hand(obj, table, x_T):
    """The loop from ``Unet.forward`` and ``dm_op_ct_dpmpp_step``; the history starts as NaN."""
    lib = _lib.load()
    x = x_T.to(DEV).contiguous()
    B, per = x.shape[0], x[0].numel()
    hist = torch.full_like(x, float("nan"))
    for row in table:
        row = row.reshape(1, K.COLS).contiguous()
        F = obj.model(x, row[0, K.LOG_SNR].expand(B).contiguous().to(DEV))
        nxt = torch.empty_like(x)
        _lib.check(lib.dm_op_ct_dpmpp_step(_lib.ptr(x), _lib.ptr(F), _lib.ptr(hist), _fp(row), 1, obj._objective,
                                           int(bool(obj.clip_sample_denoised)), _lib.ptr(nxt), B, per, None))
        x = nxt
    return x


@pytest.mark.parametrize("key", ["v_o2", "lin_o2_clip"])
def test_loop_is_the_composition_of_forward_and_operator(golden, key):
    c = golden[key]
    obj = _case_obj(c)
    got = obj.dpm_solver_sample(SHAPE, 5, 2, noise=lambda shape: c["x_T"], unnormalize=False)
    want = _by_hand(obj, dm.ct_dpmpp_table(5, c["schedule"], 2), c["x_T"])
    assert torch.equal(got, want)
    final = obj.dpm_solver_sample(SHAPE, 5, 2, noise=lambda shape: c["x_T"])
    assert torch.equal(final, (got.clamp(-1, 1) + 1) * 0.5)


def test_learned_schedule_samples_on_its_own_nodes(golden):
    c = golden["lin_o2_noclip"]
    torch.manual_seed(0)
    net = _net(c["unet_kw"], c["salt"], channels=3)
    obj = dm.ContinuousTimeGaussianDiffusion(net, image_size=16, noise_schedule="learned", learned_schedule_net_hidden_dim=16)
    # the default grid takes its two ends from the module, the time grid every node
    with torch.no_grad():
        ends = [float(obj.log_snr(torch.tensor(t))) for t in (1., 0.)]
    nodes = dm.ct_dpmpp_nodes(5, obj.log_snr)
    assert [float(nodes[0]), float(nodes[-1])] == ends
    got = obj.dpm_solver_sample(SHAPE, 5, 2, noise=lambda shape: c["x_T"], unnormalize=False)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, _by_hand(obj, dm.ct_dpmpp_table(5, obj.log_snr, 2), c["x_T"]))
    table, linear = (dm.ct_dpmpp_table(5, s, 2, "time") for s in (obj.log_snr, "linear"))
    assert float((table[1:, K.LOG_SNR] - linear[1:, K.LOG_SNR]).abs().min()) > 1e-2  # not the linear schedule's nodes
    timed = obj.dpm_solver_sample(SHAPE, 5, 2, spacing="time", noise=lambda shape: c["x_T"], unnormalize=False)
    assert torch.equal(timed, _by_hand(obj, table, c["x_T"]))
    assert not torch.equal(timed, _by_hand(obj, linear, c["x_T"])) and not torch.equal(timed, got)


def test_entry_refuses_other_handles():
    """As dm_sample_ct: no sequence model, no text or image condition, a float-time U-Net only; and row 0 must have g == 0."""
    lib = _lib.load()
    table = dm.ct_dpmpp_table(2, "cosine").contiguous()
    x = _randn(SHAPE, 1).to(DEV)
    out = torch.empty_like(x)

    def call(handle, tab=table, shape=SHAPE):
        a = _lib.CtDpmppArgs()
        a.objective, a.clip, a.n_steps, a.table_host = do.V, 1, tab.shape[0], _fp(tab)
        a.x_init, a.out, a.x_out = _lib.ptr(x), _lib.ptr(out), None
        a.B, a.H, a.W = shape[0], shape[2], shape[3]
        a.use_graph, a.stream = 0, torch.cuda.current_stream(DEV).cuda_stream
        rc = lib.dm_sample_ct_dpmpp(handle, C.byref(a))
        return rc, lib.dm_last_error()

    seq = _net(dict(dim=32, dim_mults=(1, 2), channels=3, learned_sinusoidal_cond=True), 1, cls=dm.Unet1D)
    rc, msg = call(seq._handle, shape=(2, 3, 1, 256))
    assert rc != 0 and b"seq1d" in msg
    text = _net(dict(D32, channels=3, text_condition=True), 1)
    rc, msg = call(text._handle)
    assert rc != 0 and b"text-conditional" in msg
    img = _net(dict(D32, channels=3, cond_channels=3), 1)
    rc, msg = call(img._handle)
    assert rc != 0 and b"image" in msg
    plain = _net(dict(dim=32, dim_mults=(1, 2), channels=3), 1)
    rc, msg = call(plain._handle)
    assert rc != 0 and b"sinusoidal" in msg
    ok = _net(dict(D32, channels=3), 1)
    bad = table.clone()
    bad[0, K.DPM_G] = 0.5
    rc, msg = call(ok._handle, tab=bad)
    assert rc != 0 and b"c[12]" in msg
    assert call(ok._handle)[0] == 0
