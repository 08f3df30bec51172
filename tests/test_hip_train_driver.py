"""What the training-call driver (run_train, csrc/dm_train.inc) owns, for all four loss + backward entries -- DDPM,
learned variance, ElucidatedDiffusion, continuous time -- and the table_op scaffold of the three stand-alone loss operators.

The library has no atomics on this path and training is run-to-run bit equal, so every comparison between two handles, or
between two calls, is ``torch.equal``:
* shape changes on one handle (workspace and per-image rows regrown, a smaller shape's workspace key hit after a larger
  one, the key's optional-output flag) give what a fresh handle gives for the same single call;
* a call the entry refuses in its argument checks leaves the handle as it was: the dropout call counter does not move;
* the loss operators called twice in a row (B = 1, then B = 5) do not depend on the first call, and stay within the bounds
  of their own per-operator tests, whose helpers are imported."""
import ctypes as C

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd import learned as L
from diffusion_models_amd.spec import UnetConfig

import ct_oracle as co
import edm_train_oracle as eto
import learned_oracle as LO
from conftest import rel_l2
from test_hip_edm_train import SIGMAS5
from test_hip_learned_train import OP_TOL as LV_OP_TOL
from test_hip_learned_train import _loss_errors, _loss_inputs, _run_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRIES = ["ddpm", "lv", "edm", "ct"]
UNET_KW = {
    "ddpm": dict(dim=32, dim_mults=(1, 2)),
    "lv": dict(dim=32, dim_mults=(1, 2), learned_variance=True),
    "edm": dict(dim=32, dim_mults=(1, 2), learned_sinusoidal_cond=True),
    "ct": dict(dim=32, dim_mults=(1, 2), learned_sinusoidal_cond=True),
}
_SD = {}


def _unet(entry, **kw):
    """A fresh handle with the entry's synthetic weights (the state dict is built once per entry and never changed)."""
    if entry not in _SD:
        _SD[entry] = dm.synth_state_dict(dm.unet_param_spec(UnetConfig(channels=3, **UNET_KW[entry])), salt=41)
    u = dm.Unet(channels=3, device=DEV, **UNET_KW[entry], **kw)
    u.load_state_dict(_SD[entry])
    return u


def _call(entry, u, B, hw, extra=False):
    """One loss + backward call on ``u`` with injected t / sigmas / times and noise, a function of (B, hw) alone.
    Returns (loss, gradients, the optional output or None); ``extra`` asks for the entry's optional output."""
    g = torch.Generator().manual_seed(100 * B + hw)
    img = torch.rand((B, 3, hw, hw), generator=g)
    noise = torch.randn((B, 3, hw, hw), generator=g)
    t = torch.tensor([3, 500, 999][:B])
    u01 = torch.tensor([0.1, 0.5, 0.9][:B])
    out = None
    if entry == "ddpm":
        r = dm.DenoisingDiffusion(u, image_size=hw, timesteps=1000).p_losses(img * 2 - 1, t, noise=noise, return_model_out=extra)
    elif entry == "lv":
        r = dm.LearnedGaussianDiffusion(u, image_size=hw, timesteps=1000).p_losses(img * 2 - 1, t, noise=noise,
                                                                                     return_model_out=extra)
    elif entry == "edm":
        r = dm.ElucidatedDiffusion(u, image_size=hw)(img, sigmas=(4 * u01 - 2).exp(), noise=noise, return_denoised=extra)
    else:
        assert not extra
        r = dm.ContinuousTimeGaussianDiffusion(u, image_size=hw).p_losses(img * 2 - 1, u01, noise=noise)
    if extra:
        r, out = r
    loss = r.clone()
    assert bool(torch.isfinite(loss))
    return loss, u.grads_flat().clone(), out


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and (a[2] is None) == (b[2] is None) and (
        a[2] is None or torch.equal(a[2], b[2]))


@pytest.mark.parametrize("entry", ENTRIES)
def test_shape_changes_on_one_handle_equal_fresh_handles(entry):
    calls = [(2, 8, False), (3, 16, False), (2, 8, False)] + ([(2, 8, True)] if entry != "ct" else [])
    fresh = {}
    for c in set(calls):
        fresh[c] = _call(entry, _unet(entry), *c)
    assert float(fresh[(2, 8, False)][1].abs().sum()) > 0 and not torch.equal(fresh[(2, 8, False)][0], fresh[(3, 16, False)][0])
    one = _unet(entry)
    for i, c in enumerate(calls):
        got = _call(entry, one, *c)
        assert _same(got, fresh[c]), (entry, i, c, float(got[0]), float(fresh[c][0]))
    if entry != "ct":  # the optional output changes nothing else
        assert torch.equal(fresh[(2, 8, True)][1], fresh[(2, 8, False)][1]) and fresh[(2, 8, True)][2] is not None


def _refused_call(entry, u):
    """A call that fails the entry's own argument checks in the library (never a device fault): an odd image side, which
    check_hw rejects, or -- where the Python class would catch that first -- a condition image on a plain U-Net."""
    x = torch.zeros((2, 3, 9, 9))
    if entry == "ddpm":
        with pytest.raises(RuntimeError, match="input channels"):
            dm.DenoisingDiffusion(u, image_size=16, timesteps=1000).p_losses(
                torch.zeros((2, 3, 16, 16)), torch.tensor([3, 500]), noise=torch.zeros((2, 3, 16, 16)), cond=torch.zeros((2, 3, 16, 16)))
    elif entry == "lv":
        lib = _lib.load()
        xd = torch.zeros((2, 3, 16, 16), device=DEV)
        t_arr = (C.c_int64 * 2)(3, 500)
        tab = dm.lv_train_table(dm.make_schedule(1000, "linear"), torch.tensor([3, 500])).contiguous()
        v = _lib.LvTrainArgs()
        v.x_start, v.noise, v.t_host = _lib.ptr(xd), _lib.ptr(xd), C.cast(t_arr, C.POINTER(C.c_int64))
        v.coef_host, v.coef_stride, v.vb_loss_weight, v.loss_scale = _lib.fptr(tab), 12, 0.001, 1.0
        v.B, v.H, v.W, v.stream = 2, 9, 9, torch.cuda.current_stream(DEV).cuda_stream
        assert lib.dm_unet_loss_backward_lv(u._handle, C.byref(v)) != 0 and b"divisible by 2" in lib.dm_last_error()
    elif entry == "edm":
        with pytest.raises(RuntimeError, match="divisible by 2"):
            dm.ElucidatedDiffusion(u, image_size=9)(x, sigmas=torch.tensor([0.5, 1.0]), noise=x)
    else:
        with pytest.raises(RuntimeError, match="divisible by 2"):
            dm.ContinuousTimeGaussianDiffusion(u, image_size=9).p_losses(x, torch.tensor([0.3, 0.6]), noise=x)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_refused_call_leaves_the_handle_as_it_was(entry):
    def handle():
        u = _unet(entry, dropout=0.1)
        _call(entry, u, 2, 16)  # arms the handle (and draws a dropout seed) ...
        return u.set_dropout_seed(7)  # ... which is fixed here: the call counter starts at 0 on both handles

    a, b = handle(), handle()
    first = _call(entry, a, 2, 16)
    _refused_call(entry, a)
    second_a = _call(entry, a, 3, 16)
    assert _same(first, _call(entry, b, 2, 16))
    second_b = _call(entry, b, 3, 16)
    assert _same(second_a, second_b), (entry, float(second_a[0]), float(second_b[0]))
    # the masks do depend on the counter: the same call made first on a handle gives another result
    c = handle()
    assert not torch.equal(_call(entry, c, 3, 16)[1], second_b[1])


# ---- the stand-alone loss operators ----------------------------------------------------------------------------------------
def _edm_loss(B):
    lib = _lib.load()
    g = torch.Generator().manual_seed(32 + B)
    shape = (3, 8, 8) if B > 1 else (1, 2, 2)
    tab = dm.edm_train_table(SIGMAS5[:B].contiguous()).contiguous()
    noised, F, x0 = (torch.randn((B, *shape), generator=g) for _ in range(3))
    dev = [v.to(DEV) for v in (noised, F, x0)]

    def run():
        dF, D, loss = torch.full((B, *shape), float("nan"), device=DEV), torch.empty((B, *shape), device=DEV), C.c_float(0.0)
        _lib.check(lib.dm_op_edm_loss(*[_lib.ptr(v) for v in dev], _lib.fptr(tab), 0.5, _lib.ptr(dF), _lib.ptr(D), C.byref(loss), B,
                                      x0[0].numel(), None))
        return torch.tensor(loss.value), dF.cpu(), D.cpu()

    wl, wdF, wD = eto.loss_and_dF(noised.double(), F.double(), x0.double(), tab.double(), loss_scale=0.5)

    def errors(got):  # the bound of tests/test_hip_edm_train.py::test_op_loss_vs_fp64
        return [abs(float(got[0]) - float(wl)) / abs(float(wl)), rel_l2(got[2], wD)] + [rel_l2(got[1][b], wdF[b]) for b in range(B)], 1e-6

    return run, errors


def _ct_loss(B):
    lib = _lib.load()
    g = torch.Generator().manual_seed(62 + B)
    per = 192 if B > 1 else 16
    tab = dm.ct_train_table(torch.tensor([0.05, 0.2, 0.5, 0.9, 0.7])[:B], "cosine", True, 5).contiguous()
    F, target = torch.randn((B, per), generator=g), torch.randn((B, per), generator=g)
    Fd, td = F.to(DEV), target.to(DEV)

    def run():
        dF, loss = torch.full((B, per), float("nan"), device=DEV), C.c_float(0.0)
        _lib.check(lib.dm_op_ct_loss(_lib.ptr(Fd), _lib.ptr(td), _lib.fptr(tab), 0.5, _lib.ptr(dF), C.byref(loss), B, per, None))
        return torch.tensor(loss.value), dF.cpu()

    wl, wdF = co.loss_and_dF(F.double(), target.double(), tab.double(), loss_scale=0.5)

    def errors(got):  # the bound of tests/test_hip_ct.py::test_op_loss_vs_fp64
        return [abs(float(got[0]) - float(wl)) / abs(float(wl))] + [rel_l2(got[1][b], wdF[b]) for b in range(B)], 1e-6

    return run, errors


def _lv_loss(B):
    C_, hw = (4, 20) if B > 1 else (1, 2)  # B = 1: `per4-smallest` of tests/test_hip_learned_train.py
    tab, x0, noise, x_t, mo = _loss_inputs(B, C_, hw, 60 + B)
    args = (mo, x0, noise, x_t, tab, 0.05, False, 0.5)

    def run():
        return _run_loss(*args)

    ref, r32 = LO.loss(*args, torch.float64), LO.loss(*args, torch.float32)
    e32 = _loss_errors(r32, ref, C_, tab[:, L.T_T0])

    def errors(got):  # the bound of tests/test_hip_learned_train.py::test_op_loss_vs_fp64_autograd, key by key
        err = _loss_errors(got, ref, C_, tab[:, L.T_T0])
        return [err[k] / max(4 * e32[k], LV_OP_TOL) for k in err], 1.0

    return run, errors


@pytest.mark.parametrize("op", [_edm_loss, _ct_loss, _lv_loss], ids=["edm", "ct", "lv"])
def test_loss_operators_do_not_depend_on_the_previous_call(op):
    results = {}
    for B in (1, 5):
        run, errors = op(B)
        results[B] = (run(), run(), errors)
    run1, _ = op(1)
    again = run1()  # B = 1 after B = 5: a smaller table behind a larger one
    for B, (first, second, errors) in results.items():
        assert all(torch.equal(p, q) for p, q in zip(first, second)), B
        err, bound = errors(second)
        print(f"{op.__name__} B={B}: worst {max(err):.3e} (bound {bound:.0e})")
        assert all(bool(torch.isfinite(p).all()) for p in second) and max(err) <= bound, (B, err)
    assert all(torch.equal(p, q) for p, q in zip(again, results[1][0]))
