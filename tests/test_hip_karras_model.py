"""GPU parity of KarrasUnet (through dm_unet_forward_ft on a dm_kunet_create handle) and of ElucidatedDiffusion's two loops
over it (dm_sample_edm) against the goldens generated from the reference (tests/golden/karras.pt).

Tolerances are those of tests/test_hip_seq1d_model.py (rel-L2, fp32): one forward <= 1e-4, whole loops <= 1e-3.  Every golden
carries the reference's own fp32-vs-fp64 error, which must be at most a tenth of the limit it is used with.  Measured values
are printed with -s."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from oracle import sampler_oracle as so

from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = 1e-4
LOOP_TOL = 1e-3


@pytest.fixture(scope="module")
def golden():
    return load_golden("karras.pt")


_UNETS = {}


def unet(golden, key):
    """One handle per golden configuration, shared by the tests of this module."""
    if key not in _UNETS:
        f = golden["forward"][f"{key}_plain"]
        u = dm.KarrasUnet(device=DEV, **f["unet_kw"])
        u.load_state_dict(dm.synth_state_dict(u.param_spec(), salt=f["salt"]))
        _UNETS[key] = u
    return _UNETS[key]


def edm(golden, key, use_graph=True, steps=None):
    L = golden["loops"][key]
    u = unet(golden, L["config"])
    return dm.ElucidatedDiffusion(u, image_size=u.image_size, channels=u.channels, num_sample_steps=steps or L["steps"],
                                  use_graph=use_graph)


def run_loop(golden, key, use_graph=True, steps=None, labels="golden", batch=None, **kw):
    L = golden["loops"][key]
    labels = L["labels"] if isinstance(labels, str) else labels
    if labels is not None:
        kw["class_labels"] = labels
    return getattr(edm(golden, key, use_graph, steps), L["method"])(batch_size=batch or L["batch"], **kw)


@pytest.mark.parametrize("key", ["a_plain", "a_soft", "b_plain", "b_self_cond", "c_plain"])
def test_forward(golden, key):
    f = golden["forward"][key]
    assert f["ref_err"] <= FWD_TOL / 10
    u = unet(golden, f["config"])
    y = u(f["x"].to(DEV), f["t"].to(DEV), f["self_cond"], f["labels"]).cpu()
    err = rel_l2(y, f["y"])
    print("karras forward", key, "rel-L2", err, "reference fp32-vs-fp64", f["ref_err"])
    assert y.shape == f["y"].shape and torch.isfinite(y).all() and err < FWD_TOL
    assert u.workspace_bytes > 0


def test_forward_sees_the_ones_channel_and_the_labels(golden):
    """The goldens can tell the ones channel of input_block from a bias, and one label set from another."""
    m, f = golden["margins"], golden["forward"]["a_plain"]
    assert min(m["a_ones_channel"], m["a_labels"], m["a_time"]) >= 10 * FWD_TOL
    u = unet(golden, "a")
    y = u(f["x"], f["t"], None, f["labels"]).cpu()
    assert rel_l2(y, m["a_ones_channel_output"]) > 100 * FWD_TOL > rel_l2(y, f["y"])
    other = u(f["x"], f["t"], None, (f["labels"] + 1) % 5).cpu()
    assert abs(rel_l2(other, f["y"]) - m["a_labels"]) < 10 * FWD_TOL
    onehot = torch.nn.functional.one_hot(f["labels"], 5).float()
    assert torch.equal(u(f["x"], f["t"], None, onehot).cpu(), y)  # integer and one-hot labels are one path
    assert torch.equal(u(f["x"], f["t"], None, f["labels"]).cpu(), y)  # the label buffer was restored


def test_surface_and_refresh(golden):
    u = unet(golden, "c")
    f = golden["forward"]["c_plain"]
    sd = u.state_dict()
    want = dm.synth_state_dict(u.param_spec(), salt=f["salt"])
    assert list(sd.keys()) == [k for k, _ in u.param_spec()] and all(torch.equal(sd[k].cpu(), want[k]) for k in want)
    assert sum(p.numel() for p in u.parameters()) == sum(v.numel() for v in want.values())
    assert u.to(DEV) is u and u.eval() is u and u.out_dim == u.channels == 4 and u.downsample_factor == 2
    # a second load refreshes the weights in place: other values give what a fresh handle gives with them, and the first
    # values give the first output again, bit for bit
    y0 = u(f["x"], f["t"])
    other = dm.synth_state_dict(u.param_spec(), salt=77)
    fresh = dm.KarrasUnet(device=DEV, **f["unet_kw"])
    fresh.load_state_dict(other)
    u.load_state_dict(other)
    y1 = u(f["x"], f["t"])
    assert torch.equal(y1, fresh(f["x"], f["t"])) and not torch.equal(y1, y0)
    # one changed parameter re-packs only its consumers: the head matrix for a to_emb gain, the output convolution for its own
    # gain, one block for a weight (permuted: the forced weight normalisation makes a rescaled weight the same weight)
    qkv = next(k for k in other if k.endswith(".attn.to_qkv.weight"))
    for name, changed in (("mids.1.to_emb.1.gain", other["mids.1.to_emb.1.gain"] * 1.5),
                          ("output_block.1.gain", other["output_block.1.gain"] * 1.5), (qkv, other[qkv].flip(1).contiguous())):
        part = dict(other)
        part[name] = changed
        u.load_state_dict(part)
        fresh.load_state_dict(part)
        assert torch.equal(u(f["x"], f["t"]), fresh(f["x"], f["t"])), name
        assert not torch.equal(u(f["x"], f["t"]), y1), name
    scaled = dict(other)
    scaled[qkv] = other[qkv] * 3.0  # ... and a rescaled weight is indeed the same weight, up to the rounding of the norm
    u.load_state_dict(scaled)
    assert rel_l2(u(f["x"], f["t"]), y1) < 1e-5
    u.load_state_dict(want)
    assert torch.equal(u(f["x"], f["t"]), y0)


@pytest.mark.parametrize("key", ["a_heun", "a_dpmpp", "c_heun", "c_dpmpp"])
def test_loops(golden, key):
    L = golden["loops"][key]
    assert L["ref_err"] <= LOOP_TOL / 10
    y = run_loop(golden, key, noise=so.NoiseStream(L["noise_seed"])).cpu()
    err = rel_l2(y, L["sample"])
    print("karras loop", key, "rel-L2", err, "reference fp32-vs-fp64", L["ref_err"])
    assert y.shape == L["sample"].shape and torch.isfinite(y).all() and err < LOOP_TOL


@pytest.mark.parametrize("key", ["a_heun", "c_dpmpp"])
def test_graph_replay_equals_the_eager_loop(golden, key):
    eager = run_loop(golden, key, use_graph=False, seed=5)
    a = run_loop(golden, key, use_graph=True, seed=5)
    b = run_loop(golden, key, use_graph=True, seed=5)
    c = run_loop(golden, key, use_graph=True, seed=6)
    assert torch.equal(a, eager) and torch.equal(a, b) and not torch.equal(a, c)


def test_one_graph_capture_per_shape_across_labels_and_step_counts(golden):
    """The labels are device data of the conditioning head and the step count is data of the step table: a captured DPM-Solver++
    step serves two label sets and two step counts."""
    u = unet(golden, "a")
    longer0 = run_loop(golden, "a_dpmpp", seed=9, steps=8)  # the step table grows to its largest size here: growing drops the graph
    n0 = u.graph_captures
    first = run_loop(golden, "a_dpmpp", seed=9)
    other_labels = run_loop(golden, "a_dpmpp", seed=9, labels=torch.tensor([0, 2]))
    longer = run_loop(golden, "a_dpmpp", seed=9, steps=8)
    again = run_loop(golden, "a_dpmpp", seed=9)
    assert u.graph_captures == n0, "one capture per shape"
    assert torch.equal(again, first) and torch.equal(longer, longer0)
    assert not torch.equal(other_labels, first) and not torch.equal(longer, first)
    eager = run_loop(golden, "a_dpmpp", use_graph=False, seed=9, labels=torch.tensor([0, 2]))
    assert torch.equal(eager, other_labels)
    soft = torch.softmax(torch.randn(2, 5, generator=torch.Generator().manual_seed(1)), dim=-1)
    assert torch.isfinite(run_loop(golden, "a_dpmpp", seed=9, labels=soft)).all() and u.graph_captures == n0


def test_sharded_equals_whole_batch(golden):
    d = edm(golden, "a_heun")  # S_churn > 0: every Heun step draws device noise
    labels = torch.tensor([1, 3, 0, 4])
    whole = d.sample(batch_size=4, seed=11, class_labels=labels)
    parts = [d.sample(batch_size=2, seed=11, sample_offset=off, class_labels=labels[off:off + 2]) for off in (0, 2)]
    assert torch.equal(torch.cat(parts), whole)
    assert d.sample_shape() == (3, 16, 16) and whole.shape == (4, 3, 16, 16)


def test_labels_are_required_and_refused(golden):
    with pytest.raises(AssertionError, match="class_labels"):
        run_loop(golden, "a_dpmpp", labels=None, seed=1)
    with pytest.raises(AssertionError, match="class_labels"):
        run_loop(golden, "c_dpmpp", labels=torch.tensor([0, 1]), seed=1)
    d = edm(golden, "c_dpmpp")
    with pytest.raises(NotImplementedError):
        d.train()
    with pytest.raises(NotImplementedError):
        d(torch.zeros(2, 4, 16, 16))
    with pytest.raises(NotImplementedError):
        dm.ElucidatedDiffusion(unet(golden, "b"), image_size=16, channels=4)  # self-conditioned sampling stays refused


def test_refused_entries_leave_the_handle_usable(golden):
    u = unet(golden, "c")
    f = golden["forward"]["c_plain"]
    y0 = u(f["x"], f["t"])
    lib = _lib.load()
    x, out = f["x"].to(DEV).contiguous(), torch.empty(1, 4, 16, 16, device=DEV)
    ti = torch.zeros(1, dtype=torch.long, device=DEV)

    def refused(rc, word="KarrasUnet"):
        assert rc != 0 and word in lib.dm_last_error().decode(), lib.dm_last_error().decode()

    refused(lib.dm_unet_forward(u._handle, _lib.ptr(x), _lib.ptr(ti), None, 0, _lib.ptr(out), 1, 16, 16, None))
    refused(lib.dm_unet_train_enable(u._handle), "forward-only")  # the integer-time training entry refuses a Fourier time
    refused(lib.dm_unet_train_enable_ft(u._handle, 1))
    # every other loop of the library, each with arguments that pass its own null checks
    times = torch.zeros(4, dtype=torch.int64)
    table = torch.zeros(4, 16)
    bufs = {k: torch.zeros(1, 4, 16, 16, device=DEV) for k in ("x_T", "x_init", "x0", "out", "terms_out", "gt", "mask", "mean", "grad")}
    cb = _lib.CondCallback(lambda user, step, t: 0)
    loops = [(lib.dm_sample_ex, _lib.SampleArgs), (lib.dm_sample_ct, _lib.CtArgs), (lib.dm_sample_ct_dpmpp, _lib.CtDpmppArgs),
             (lib.dm_sample_repaint, _lib.RepaintArgs), (lib.dm_sample_lv, _lib.LvArgs), (lib.dm_sample_wo, _lib.WoArgs),
             (lib.dm_sample_classifier_guided, _lib.CguideArgs), (lib.dm_eval_bpd, _lib.BpdArgs)]
    for fn, Args in loops:
        a = Args()
        names = {f[0] for f in Args._fields_}
        for k, v in bufs.items():
            if k in names:
                setattr(a, k, _lib.ptr(v))
        for k, v in (("times_host", C.cast(times.data_ptr(), C.POINTER(C.c_int64))), ("table_host", _lib.fptr(table)),
                     ("coefs_host", _lib.fptr(table)), ("n_steps", 1), ("n_rows", 1), ("B", 1), ("H", 16), ("W", 16),
                     ("mask_channels", 1), ("cond_cb", cb)):
            if k in names:
                setattr(a, k, v)
        refused(fn(u._handle, C.byref(a)))
    # a wrong size is refused by the library too
    big = torch.zeros(1, 4, 32, 32, device=DEV)
    tf = torch.zeros(1, device=DEV)
    refused(lib.dm_unet_forward_ft(u._handle, _lib.ptr(big), _lib.ptr(tf), None, 0, _lib.ptr(torch.empty_like(big)), 1, 32, 32, None),
            "image_size")
    assert torch.equal(u(f["x"], f["t"]), y0)


def test_attn_dim_head_is_refused_at_creation():
    lib = _lib.load()
    c = _lib.KunetCfg()
    c.image_size, c.dim, c.dim_max, c.channels, c.input_channels = 16, 32, 64, 3, 3
    c.num_downsamples, c.num_blocks_per_stage, c.fourier_dim, c.attn_dim_head = 1, 1, 16, 48
    c.mp_cat_t = c.mp_add_emb_t = 0.5
    c.attn_res_mp_add_t = c.resnet_mp_add_t = 0.3
    h = C.c_void_p()
    assert lib.dm_kunet_create(C.byref(c), 0, C.byref(h)) != 0 and "32 and 64" in lib.dm_last_error().decode()
    c.attn_dim_head = 32
    assert lib.dm_kunet_create(C.byref(c), 0, C.byref(h)) == 0 and lib.dm_unet_missing_params(h) > 0
    assert "missing parameter" in lib.dm_last_error().decode()
    lib.dm_unet_destroy(h)


def test_an_image_unet_is_untouched_by_a_karras_unet_in_the_same_process(golden):
    cfg = dm.UnetConfig(dim=32, dim_mults=(1, 2), channels=3)
    img = dm.Unet(dim=32, dim_mults=(1, 2), channels=3, device=DEV)
    img.load_state_dict(dm.synth_state_dict(dm.unet_param_spec(cfg), salt=4))
    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(2))
    t = torch.tensor([3, 500])
    before = img(x, t)
    f = golden["forward"]["a_plain"]
    k = dm.KarrasUnet(device=DEV, **f["unet_kw"])
    k.load_state_dict(dm.synth_state_dict(k.param_spec(), salt=f["salt"]))
    assert rel_l2(k(f["x"], f["t"], None, f["labels"]), f["y"]) < FWD_TOL
    assert torch.equal(img(x, t), before)
