"""CPU tests of ``ContinuousTimeGaussianDiffusion(noise_schedule='learned')`` (fixture: tests/golden/make_golden_ct_learned.py):
the package's schedule module and the step table it feeds against the scalars recorded from the reference, the state-dict and
``parameters()`` surface, the host surrogate against the reference's schedule gradients (fed with per-image rows from fp64
autograd of the oracle U-Net), the C struct of the new entry, and the refusals.

Gates.  A recorded scalar: 4 x the reference's own fp32-vs-fp64 difference of that scalar, with a floor of one fp32 ulp of
its value (the reduction over the hidden width is a threaded F.linear: never bit-exact by contract).  A schedule gradient:
max(2e-4, 4 x the case's recorded fp32-vs-fp64 error), relative to the norm of all six, the measure the fixture records."""
import ctypes
import os
import re
import types

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import continuous as K
from diffusion_models_amd.spec import UnetConfig

import ct_learned_oracle as lo
import ct_oracle as co
from conftest import ROOT, load_golden

CASES = ["learned", "learned_h1024", "learned_minsnr", "learned_frac025", "learned_rff", "learned_accumulate2"]
SCHED_KEYS = ["net.1.net.weight", "net.1.net.bias", "net.2.fn.0.net.weight", "net.2.fn.0.net.bias", "net.2.fn.2.net.weight",
              "net.2.fn.2.net.bias"]
GRAD_TOL = 2e-4


@pytest.fixture(scope="module")
def golden():
    return load_golden("ct_learned.pt")


def _module(c):
    kw = c["ct_kw"]
    lo_, hi = [K.beta_linear_log_snr(torch.tensor([t])).item() for t in (1., 0.)]
    m = K.learned_noise_schedule(log_snr_max=hi, log_snr_min=lo_, hidden_dim=kw.get("learned_schedule_net_hidden_dim", 1024),
                                 frac_gradient=kw.get("learned_noise_schedule_frac_gradient", 1.))
    m.load_state_dict(c["sched"])
    return m


def _ulp(v):
    a = v.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def _gate(want32, want64):
    return torch.maximum(4 * (want32.double() - want64.double()).abs(), _ulp(want32))


class _HandleUnet(dm.Unet):
    """A library ``Unet`` as far as the constructors look (class, a handle) that never touches the device."""

    def __init__(self, ukw):
        self.cfg = UnetConfig(channels=3, **ukw)
        self.channels, self.out_dim, self.self_condition, self.text_condition = 3, 3, False, False
        self.random_or_learned_sinusoidal_cond = True
        self.device = torch.device("cpu")
        self._handle, self._loaded = object(), True

    def __del__(self):
        pass

    def state_dict(self, ema=False):
        return {n: torch.zeros(tuple(s)) for n, s in dm.unet_param_spec(self.cfg)}


@pytest.mark.parametrize("case", CASES)
def test_schedule_module_reproduces_the_recorded_log_snr(golden, case):
    c = golden["cases"][case]
    m = _module(c)
    assert list(m.state_dict()) == SCHED_KEYS and all(not p.is_cuda for p in m.parameters())
    for t, want, want64 in zip(c["times"], c["log_snr"], c["log_snr64"]):
        with torch.no_grad():
            got = m(t)
        err, gate = (got.double() - want.double()).abs(), _gate(want, want64)
        print(case, "log_snr |ours - reference|", err.tolist(), "gate", gate.tolist())
        assert got.dtype == torch.float32 and bool((err <= gate).all())
    # t = 0 / 1 map to the ends of the linear schedule whatever the parameters are
    with torch.no_grad():
        ends = m(torch.tensor([0., 1.]))
    assert torch.allclose(ends, torch.tensor([m.intercept, m.intercept + m.slope]), rtol=1e-6, atol=0)


@pytest.mark.parametrize("case", CASES)
def test_step_table_reproduces_the_recorded_scalars(golden, case):
    c, names = golden["cases"][case], golden["names"]
    tab = dm.ct_step_table(c["n"], _module(c))
    rec, rec64 = c["scalars"], c["scalars64"]
    assert tab.shape == (c["n"], K.COLS) and tab.dtype == torch.float32 and not tab.requires_grad
    cols = {"log_snr": K.LOG_SNR, "c": K.C_, "alpha": K.ALPHA, "sigma": K.SIGMA, "alpha_next": K.ALPHA_NEXT, "sqrt_var": K.SQRT_VAR}
    for name, col in cols.items():
        j = names.index(name)
        want, want64 = rec[:, j].clone(), rec64[:, j].clone()
        if name == "sqrt_var":  # the last step takes no square root: the table holds 0 there
            assert bool(torch.isnan(want[-1])) and float(tab[-1, col]) == 0.0
            want, want64, got = want[:-1], want64[:-1], tab[:-1, col]
        else:
            got = tab[:, col]
        err, gate = (got.double() - want).abs(), _gate(want.float(), want64)
        print(case, name, "worst |ours - reference|", float(err.max()), "its gate", float(gate[err.argmax()]))
        assert bool((err <= gate).all()), (name, err.tolist(), gate.tolist())


def test_state_dict_and_parameters_follow_the_reference(golden):
    c = golden["cases"]["learned"]
    obj = dm.ContinuousTimeGaussianDiffusion(_HandleUnet(c["unet_kw"]), image_size=16, noise_schedule="learned", **c["ct_kw"])
    assert isinstance(obj.log_snr, K.learned_noise_schedule) and obj.learned_schedule is obj.log_snr
    sd = obj.state_dict()
    assert list(sd) == c["state_dict_keys"]
    for k in SCHED_KEYS:
        assert tuple(sd["log_snr." + k].shape) == tuple(c["sched"][k].shape)
    params = list(obj.parameters())
    spec = dm.unet_param_spec(obj.model.cfg)
    assert c["parameter_names"] == ["model." + n for n, _ in spec] + ["log_snr." + k for k in SCHED_KEYS]
    assert len(params) == len(c["parameter_names"])
    assert [tuple(p.shape) for p in params[-6:]] == [tuple(c["sched"][k].shape) for k in SCHED_KEYS]
    assert all(a is b for a, b in zip(params[-6:], obj.log_snr.parameters()))
    # default hidden width, initialisation in the reference's construction order (same seed, same values)
    torch.manual_seed(3)
    a = dm.ContinuousTimeGaussianDiffusion(_HandleUnet(c["unet_kw"]), image_size=16, noise_schedule="learned")
    torch.manual_seed(3)
    lin = [torch.nn.Linear(1, 1), torch.nn.Linear(1, 1024), torch.nn.Linear(1024, 1)]
    got = list(a.log_snr.parameters())
    assert all(torch.equal(g, w) for g, w in zip(got, [p for l in lin for p in (l.weight, l.bias)]))
    assert a.log_snr.frac_gradient == 1.0
    # load_state_dict: the six keys are required when the schedule is learned and unexpected otherwise
    full = {k: v for k, v in sd.items()}
    loaded = {}
    obj.model.load_state_dict = lambda d, strict=True: loaded.update(d)
    full["log_snr." + SCHED_KEYS[0]] = torch.full((1, 1), 0.75)
    obj.load_state_dict(full)
    assert float(obj.log_snr.net[1].net.weight.detach()) == 0.75 and set(loaded) == {n for n, _ in spec}
    with pytest.raises(RuntimeError, match="Missing key"):
        obj.load_state_dict({k: v for k, v in full.items() if k != "log_snr." + SCHED_KEYS[3]})
    fixed = dm.ContinuousTimeGaussianDiffusion(_HandleUnet(c["unet_kw"]), image_size=16)
    fixed.model.load_state_dict = lambda d, strict=True: None
    assert list(fixed.state_dict()) == ["model." + n for n, _ in spec] and fixed.learned_schedule is None
    with pytest.raises(RuntimeError, match="unexpected"):
        fixed.load_state_dict(full)


@pytest.mark.parametrize("case", CASES)
def test_surrogate_on_fp64_rows_gives_the_recorded_schedule_gradients(golden, case):
    c = golden["cases"][case]
    kw = c["ct_kw"]
    cfg = UnetConfig(channels=3, **c["unet_kw"])
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=c["salt"])
    m = _module(c)
    scale = 1.0 / c["micro"]
    for img, t, noise in zip(c["imgs"], c["times"], c["noises"]):
        terms, tab = K.learned_train_terms(m, t, kw.get("min_snr_loss_weight", False), kw.get("min_snr_gamma", 5))
        rows = lo.input_grads(sd, cfg, img, noise, tab, co.NOISE, True, torch.float64, loss_scale=scale)["rows"]
        K.schedule_surrogate(terms, rows, scale).backward()
    want = c["sched_grads"]
    norm = torch.cat([v.reshape(-1) for v in c["sched_grads64"].values()]).norm()
    tol = max(GRAD_TOL, 4 * c["ref_err_sched_grad_max"])
    worst = 0.0
    for k, p in m.named_parameters():
        err = float((p.grad.double() - want[k].double()).norm() / norm)
        worst = max(worst, err)
        assert err <= tol, (k, err, tol)
    print(f"{case}: schedule gradients vs reference, worst {worst:.3e} (gate {tol:.1e}; the reference's own fp32-vs-fp64 "
          f"{c['ref_err_sched_grad_max']:.3e})")
    assert float(norm) > 0
    if case == "learned_frac025":  # frac_gradient scales the gradient that goes back, nothing else
        full = golden["cases"]["learned"]["sched_grads"]
        for k in want:
            assert torch.allclose(want[k], 0.25 * full[k], rtol=1e-5, atol=1e-7 * float(norm))


def _declared(struct):
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    declared = []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        m = re.fullmatch(r"(const\s+)?(\w+)\s*(\*?)\s*([\w\s,]+)", decl)
        assert m, decl
        for name in (n.strip() for n in m.group(4).split(",")):
            declared.append((name, "pointer" if m.group(3) else ctype[m.group(2)]))
    return declared, src


def test_ig_struct_binding_matches_the_header_and_extends_the_plain_one():
    declared, src = _declared("dm_ct_train_ig_args")
    bound = []
    for name, t in _lib.CtTrainIgArgs._fields_:
        is_ptr = t is ctypes.c_void_p or isinstance(t, type(ctypes.POINTER(ctypes.c_float)))
        bound.append((name, "pointer" if is_ptr else t))
    assert bound == declared
    off, offsets = 0, {}
    for name, t in declared:
        size = 8 if t == "pointer" else ctypes.sizeof(t)
        off = (off + size - 1) // size * size
        offsets[name] = off
        off += size
    assert {n: getattr(_lib.CtTrainIgArgs, n).offset for n, _ in declared} == offsets
    assert ctypes.sizeof(_lib.CtTrainIgArgs) == (off + 7) // 8 * 8 == 96
    # the first 13 fields are dm_ct_train_args, field for field, at the same offsets; its size is unchanged
    plain, _ = _declared("dm_ct_train_args")
    assert declared[:len(plain)] == plain and ctypes.sizeof(_lib.CtTrainArgs) == 72
    assert all(getattr(_lib.CtTrainArgs, n).offset == offsets[n] for n, _ in plain)
    assert [n for n, _ in declared[len(plain):]] == ["sched_out_host", "dx_out", "dtime_out"]
    new = {"dm_unet_loss_backward_ct_ig", "dm_op_conv7_dgrad", "dm_op_sinusoid_ft_tgrad", "dm_op_ct_sched_reduce",
           "dm_unet_optimizer_step_ex"}
    assert new <= set(_lib.EXPORTS) and all(re.search(r"\bint %s\(" % s, src) for s in new)
    assert _lib.ABI_VERSION == 9  # additions only


def _stub_net(**kw):
    base = dict(random_or_learned_sinusoidal_cond=True, self_condition=False, text_condition=False, out_dim=3, channels=3,
                cfg=types.SimpleNamespace(cond_channels=0), device="cpu", downsample_factor=2)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_refusals(golden, monkeypatch):
    with pytest.raises(NotImplementedError, match="learned noise schedule.*input-gradient"):
        dm.ContinuousTimeGaussianDiffusion(_stub_net(), image_size=16, noise_schedule="learned")
    c = golden["cases"]["learned"]
    obj = dm.ContinuousTimeGaussianDiffusion(_HandleUnet(c["unet_kw"]), image_size=16, noise_schedule="learned", **c["ct_kw"])
    # the per-image rows have to come back: refused before a tensor or the device is touched
    with pytest.raises(ValueError, match="sync=False"):
        obj(c["imgs"][0], times=c["times"][0], noise=c["noises"][0], sync=False)
    with pytest.raises(ValueError, match="sync=False"):
        obj.p_losses(c["imgs"][0], c["times"][0], sync=False)
    # more than one rank: averaging the six host gradients is not built
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        dm.train_step(obj, [c["imgs"][0]], times=[c["times"][0]], noise=[c["noises"][0]])
    # the v class has no schedule argument; the fixed schedules have no module
    assert dm.VParamContinuousTimeGaussianDiffusion(_stub_net(), image_size=16).learned_schedule is None
