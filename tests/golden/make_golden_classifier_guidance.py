#!/usr/bin/env python3
"""Classifier-guidance goldens from the REFERENCE (build container only):
``python tests/golden/make_golden_classifier_guidance.py`` -> ``classifier_guidance.pt``.

``denoising_diffusion/guided_diffusion.py`` (``GaussianDiffusion`` with ``cond_fn`` / ``guidance_kwargs``) runs over
``denoising_diffusion.Unet`` with name-seeded synthetic weights; the module's ``from utils import ...`` is served by
aliasing ``utils`` to ``denoising_diffusion.utils`` and ``accelerate`` by an inert stub, next to the stubs of
``make_golden.import_reference``.  ``torch.randn`` / ``randn_like`` as the module sees them are redirected to a seeded
NoiseStream; the module's per-step ``print`` goes to a swallowed stdout.

The classifier and its ``cond_fn`` are this project's (tests/cguide_oracle.py): a linear map of the flattened image plus a
time term, ``log_softmax`` and ``autograd.grad``.  Its weights are stored, so the GPU tests rebuild the identical function.

RECORDED: ``posterior_variance`` and the DDPM row scalars of every t of three schedules (read from the module's buffers as
its ``p_sample`` uses them); constructor signature and method names; single ``p_sample`` steps at t = T-1, a middle t and
t = 0 with mean, guided mean, x_start and output (``condition_mean`` wrapped); whole loops with ``return_all_timesteps``
(a: c3 linear-50 pred_noise guided, its unguided run a0 as the final sample, b: c3 self-conditioning cosine-24 pred_v,
c: c1 pred_x0 linear-50); for each loop the same run by an fp64 twin of module, network and classifier and the
reference's own fp32-vs-fp64 relative L2.  Conditions asserted below, on the reference alone: every value is finite; loop
(a) differs from (a0) by at least 0.05 relative L2; the scale-0 run and the ``guidance_kwargs=None`` run equal (a0)
exactly.  Only DATA is written."""
from __future__ import annotations

import contextlib
import inspect
import io
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import _stub, import_reference, save, seeded  # noqa: E402

import cguide_oracle as CO  # noqa: E402
import diffusion_models_amd as dm  # noqa: E402
from diffusion_models_amd.spec import UnetConfig  # noqa: E402
from oracle.sampler_oracle import NoiseStream  # noqa: E402

D32 = dict(dim=32, dim_mults=(1, 2))
SCHEDULES = {"linear_50": ("linear", 50), "cosine_24": ("cosine", 24), "sigmoid_1000": ("sigmoid", 1000)}
N_CLASSES = 5
LOOPS = {
    # key: (channels, self_condition, schedule, T, objective, B, salt, noise seed, classifier seed, labels, scale)
    "a": (3, False, "linear", 50, "pred_noise", 2, 131, 811, 821, [1, 3], 50.0),
    "b": (3, True, "cosine", 24, "pred_v", 2, 132, 812, 822, [0, 4], 50.0),
    "c": (1, False, "linear", 50, "pred_x0", 2, 133, 813, 823, [2, 2], 50.0),
}
SIZE = 16


def import_guided():
    dd, _, _ = import_reference()
    import denoising_diffusion.utils as ref_utils

    sys.modules["utils"] = ref_utils

    class _Dummy:
        def __init__(self, *a, **k):
            pass

    _stub("accelerate", Accelerator=_Dummy)
    import denoising_diffusion.guided_diffusion as gd

    return dd, gd


class noise_as:
    """randn / randn_like as one module sees them -> a NoiseStream whose fp32 draws are cast to ``dtype``."""

    def __init__(self, module, seed, dtype=torch.float32):
        self.module, self.stream, self.dtype = module, NoiseStream(seed), dtype

    def __enter__(self):
        real, stream, dtype = self.module.torch, self.stream, self.dtype

        class _T:
            def __getattr__(_, k):
                if k == "randn":
                    return lambda shape, device=None, **kw: stream(shape).to(dtype)
                if k == "randn_like":
                    return lambda x, **kw: stream(x.shape).to(dtype)
                return getattr(real, k)

        self._real = real
        self.module.torch = _T()
        return self

    def __exit__(self, *exc):
        self.module.torch = self._real


def ref_net(dd, channels, self_condition, salt, dtype=torch.float32):
    cfg = UnetConfig(channels=channels, self_condition=self_condition, **D32)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=salt)
    net = dd.Unet(channels=channels, self_condition=self_condition, **D32).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    return net.eval()


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def schedule_scalars(gd, dd, sched, T):
    """(T, 9) fp32, row t: the DDPM row of p_sample at t -- [sqrt_recip_ac, sqrt_recipm1_ac, coef1, coef2,
    exp(0.5 posterior_log_variance_clipped), t > 0, sqrt_ac, sqrt_1m_ac] -- and posterior_variance[t]."""
    obj = gd.GaussianDiffusion(dd.Unet(dim=8, dim_mults=(1,), channels=1), image_size=4, timesteps=T, beta_schedule=sched)
    t = torch.arange(T)
    return torch.stack([obj.sqrt_recip_alphas_cumprod, obj.sqrt_recipm1_alphas_cumprod, obj.posterior_mean_coef1,
                        obj.posterior_mean_coef2, (0.5 * obj.posterior_log_variance_clipped).exp(), (t > 0).float(),
                        obj.sqrt_alphas_cumprod, obj.sqrt_one_minus_alphas_cumprod, obj.posterior_variance], dim=1).float()


def run_loop(gd, dd, key, dtype, cond=True, scale=None, kwargs_none=False):
    ch, sc, sched, T, objective, B, salt, nseed, cseed, labels, scale0 = LOOPS[key]
    net = ref_net(dd, ch, sc, salt, dtype)
    obj = gd.GaussianDiffusion(net, image_size=SIZE, timesteps=T, beta_schedule=sched, objective=objective).to(dtype)
    clf = CO.make_classifier(N_CLASSES, ch * SIZE * SIZE, cseed)
    cond_fn = CO.make_cond_fn(clf, T, dtype=dtype)
    kw = dict(y=torch.tensor(labels), scale=scale0 if scale is None else scale)
    # the sinusoidal embedding of an integer t takes its dtype from torch's default
    torch.set_default_dtype(dtype)
    try:
        with noise_as(gd, nseed, dtype):
            y = quiet(obj.sample, batch_size=B, return_all_timesteps=True, cond_fn=cond_fn if cond else None,
                      guidance_kwargs=None if kwargs_none else kw)
    finally:
        torch.set_default_dtype(torch.float32)
    return y, clf


def surface(cls):
    sig = inspect.signature(cls.__init__)
    init = [(p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name)
            for p in sig.parameters.values() if p.name != "self"]
    methods = {name: [(p.name, p.kind.name) for p in inspect.signature(getattr(cls, name)).parameters.values()
                      if p.name != "self"]
               for name in ("condition_mean", "p_sample", "p_sample_loop", "ddim_sample", "sample", "model_predictions",
                            "p_mean_variance", "q_sample", "p_losses", "forward")}
    return dict(init_params=init, methods=methods)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    dd, gd = import_guided()
    out = {}

    out["scalars"] = {k: schedule_scalars(gd, dd, s, T) for k, (s, T) in SCHEDULES.items()}
    for k, v in out["scalars"].items():
        assert torch.isfinite(v).all(), k
    out["surface"] = surface(gd.GaussianDiffusion)

    out["loops"] = {}
    for key, (ch, sc, sched, T, objective, B, salt, nseed, cseed, labels, scale) in LOOPS.items():
        y, clf = run_loop(gd, dd, key, torch.float32)
        y64, _ = run_loop(gd, dd, key, torch.float64)
        assert y.dtype == torch.float32 and y64.dtype == torch.float64 and y.shape == (B, T + 1, ch, SIZE, SIZE)
        assert torch.isfinite(y).all() and torch.isfinite(y64).all(), key
        err = rel_l2(y, y64)
        print(f"loop {key}: mean {float(y[:, -1].mean()):.4f}  reference fp32-vs-fp64 rel-L2 {err:.3e} (all frames), "
              f"{rel_l2(y[:, -1], y64[:, -1]):.3e} (final)")
        out["loops"][key] = dict(channels=ch, self_condition=sc, unet_kw=D32, image_size=SIZE, beta_schedule=sched, timesteps=T,
                                 objective=objective, batch=B, salt=salt, noise_seed=nseed, classifier=clf, labels=labels,
                                 scale=scale, frames=y, ref_err=err)
    a0, _ = run_loop(gd, dd, "a", torch.float32, cond=False)
    zero, _ = run_loop(gd, dd, "a", torch.float32, scale=0.0)
    nokw, _ = run_loop(gd, dd, "a", torch.float32, kwargs_none=True)
    a = out["loops"]["a"]["frames"]
    dist = rel_l2(a[:, -1], a0[:, -1])
    print(f"loop a vs a0 (final sample): {dist:.4f}; scale 0 equal: {torch.equal(zero, a0)}; kwargs None equal: "
          f"{torch.equal(nokw, a0)}")
    assert torch.isfinite(a0).all() and dist >= 0.05 and torch.equal(zero, a0) and torch.equal(nokw, a0)
    out["loops"]["a"]["unguided_final"] = a0[:, -1].clone()
    out["loops"]["a"]["guided_vs_unguided"] = dist

    # single p_sample steps of loop a's network: condition_mean wrapped to keep its input and output
    ch, sc, sched, T, objective, B, salt, nseed, cseed, labels, scale = LOOPS["a"]
    obj = gd.GaussianDiffusion(ref_net(dd, ch, sc, salt), image_size=SIZE, timesteps=T, beta_schedule=sched, objective=objective)
    clf = CO.make_classifier(N_CLASSES, ch * SIZE * SIZE, cseed)
    cond_fn = CO.make_cond_fn(clf, T)
    kw = dict(y=torch.tensor(labels), scale=scale)
    x = seeded((B, ch, SIZE, SIZE), 830)
    rows = []
    for t in (T - 1, T // 2, 0):
        kept = {}
        real = obj.condition_mean

        def wrapped(cond_fn_, mean, variance, x_, t_, guidance_kwargs=None, _real=real, _kept=kept):
            _kept["mean"] = mean.detach().clone()
            _kept["guided"] = _real(cond_fn_, mean, variance, x_, t_, guidance_kwargs).detach().clone()
            return _kept["guided"]

        obj.condition_mean = wrapped
        try:
            with noise_as(gd, 840 + t):
                y, xs = quiet(obj.p_sample, x, t, None, cond_fn, kw)
        finally:
            obj.condition_mean = real
        assert all(torch.isfinite(v).all() for v in (y, xs, kept["mean"], kept["guided"])), t
        rows.append(dict(t=t, noise_seed=840 + t, y=y, x_start=xs, mean=kept["mean"], guided_mean=kept["guided"]))
    out["steps_single"] = dict(loop="a", x=x, steps=rows)
    save("classifier_guidance.pt", out)


if __name__ == "__main__":
    main()
