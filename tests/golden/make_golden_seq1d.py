#!/usr/bin/env python3
"""Unet1D / DenoisingDiffusion1D goldens from the REFERENCE (build container only):
``python tests/golden/make_golden_seq1d.py`` -> ``seq1d.pt``.

``denoising_diffusion/denoising_diffusion_1d.py`` runs on name-seeded synthetic weights (``synth_state_dict`` over
``unet1d_param_spec``, loaded ``strict=True``: the spec equals the reference's ``state_dict()``).  ``torch.randn`` /
``randn_like`` as the module sees them are redirected to a seeded NoiseStream.  Every forward and every loop is stored with
the reference's own fp32-vs-fp64 error, from an fp64 twin of the network and the wrapper on the same weights and noise.

Stored: state-dict keys and shapes of two configurations; ``Unet1D`` forward outputs of four; ``p_mean_variance`` at four
times; whole loops (DDPM, DDIM under pred_noise with and without clipping, DDIM under pred_v with eta > 0, a self-conditioned
DDIM loop); ``interpolate``; the schedule buffers of both schedules and ``loss_weight`` of every objective; the constructor and
method signatures.

Conditions asserted here on the reference alone (values stored under ``margins``): everything is finite; the clipped
pred_noise DDIM loop differs from the same loop with ``rederive_pred_noise=True`` (a subclass below that adds the one
keyword) by at least 10 x the loop tolerance of the tests, or the tests could not see that the sequence class does not
re-derive; the unclipped loop differs from the clipped one by at least as much.  Only DATA is written."""
from __future__ import annotations

import inspect
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, save, seeded  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402
from diffusion_models_amd.spec import Unet1DConfig, unet1d_param_spec  # noqa: E402
from oracle.sampler_oracle import NoiseStream  # noqa: E402

LOOP_TOL = 1e-3  # tests/test_hip_model.py
MARGIN = 10 * LOOP_TOL

UNETS = {
    # key: (Unet1D kwargs, L, B, salt, input seed)
    "d32_c2": (dict(dim=32, dim_mults=(1, 2), channels=2), 32, 2, 201, 801),
    # reaches 64-wide and 256-wide layers, two cout tiles, an odd batch, L / 4 not a power of two
    "d64_c1": (dict(dim=64, dim_mults=(1, 2, 4), channels=1), 24, 3, 202, 802),
    "selfcond": (dict(dim=32, dim_mults=(1, 2), channels=2, self_condition=True), 16, 2, 203, 803),
    "dh64": (dict(dim=32, dim_mults=(1, 2), channels=3, attn_dim_head=64, attn_heads=2), 16, 2, 204, 804),
}
LOOPS = {
    # key: (unet key, diffusion kwargs, method, method kwargs, noise seed)
    "ddpm50": ("d32_c2", dict(timesteps=50), "sample", {}, 811),
    "ddim8_clip": ("d32_c2", dict(timesteps=1000, sampling_timesteps=8), "ddim_sample", dict(clip_denoised=True), 812),
    "ddim8_noclip": ("d32_c2", dict(timesteps=1000, sampling_timesteps=8), "ddim_sample", dict(clip_denoised=False), 812),
    "ddim8_v": ("d32_c2", dict(timesteps=1000, sampling_timesteps=8, objective="pred_v", ddim_sampling_eta=0.5,
                               beta_schedule="linear"), "sample", {}, 813),
    "ddim6_selfcond": ("selfcond", dict(timesteps=1000, sampling_timesteps=6), "sample", {}, 814),
    "ddpm24_d64": ("d64_c1", dict(timesteps=24, objective="pred_x0"), "sample", {}, 815),
}


class patched_noise:
    """randn / randn_like as the 1D module sees them -> one NoiseStream, cast to ``dtype``."""

    def __init__(self, module, seed, dtype=torch.float32):
        self.module, self.stream, self.dtype = module, NoiseStream(seed), dtype

    def __enter__(self):
        real, stream, dtype = self.module.torch, self.stream, self.dtype

        class _T:
            def __getattr__(_, k):
                if k == "randn":
                    return lambda shape, device=None, **kw: stream(tuple(shape)).to(dtype)
                if k == "randn_like":
                    return lambda x, **kw: stream(tuple(x.shape)).to(dtype)
                return getattr(real, k)

        self._real = real
        self.module.torch = _T()
        return self

    def __exit__(self, *exc):
        self.module.torch = self._real


class fp64_default:
    """The sinusoidal embedding of an integer t takes its dtype from torch's default: fp64 while a twin RUNS."""

    def __enter__(self):
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.set_default_dtype(torch.float32)


def ref_net(d1, ukw, salt, dtype=torch.float32):
    spec = unet1d_param_spec(Unet1DConfig(**ukw))
    sd = dm.synth_state_dict(spec, salt=salt)
    net = d1.Unet1D(**ukw).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(s)) for k, s in spec]
    return net.eval(), spec


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def run_loop(d1, cls, net, L, B, dkw, method, mkw, nseed, dtype=torch.float32):
    obj = cls(net, seq_length=L, **dkw)
    if dtype == torch.float64:
        obj = obj.double()
    ch = net.channels
    with patched_noise(d1, nseed, dtype):
        if method == "sample":
            return obj.sample(batch_size=B)
        return getattr(obj, method)((B, ch, L), **mkw)


def surface(cls, names):
    sig = inspect.signature(cls.__init__)
    init = [(p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name)
            for p in sig.parameters.values() if p.name != "self"]
    methods = {n: [(p.name, p.kind.name) for p in inspect.signature(getattr(cls, n)).parameters.values() if p.name != "self"]
               for n in names}
    return dict(init_params=init, methods=methods)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import_reference()
    import denoising_diffusion.denoising_diffusion_1d as d1

    d1.tqdm = lambda it, **kw: it  # no progress bars in the log
    out = {"loop_tol": LOOP_TOL}

    # ---- state-dict keys and shapes --------------------------------------------------------------------------------------
    out["keys"] = {}
    for key in ("d32_c2", "d64_c1"):
        ukw = UNETS[key][0]
        net = d1.Unet1D(**ukw)
        out["keys"][key] = dict(unet_kw=ukw, entries=[(k, tuple(v.shape)) for k, v in net.state_dict().items()])
    assert len(out["keys"]["d32_c2"]["entries"]) == 138
    assert out["keys"]["d32_c2"]["entries"][0] == ("init_conv.weight", (32, 2, 7))

    # ---- Unet1D.forward ---------------------------------------------------------------------------------------------------
    out["unet"] = {}
    for key, (ukw, L, B, salt, seed) in UNETS.items():
        net, _ = ref_net(d1, ukw, salt)
        ch = ukw["channels"]
        x, t = seeded((B, ch, L), seed), torch.tensor([3, 987, 412][:B])
        xsc = seeded((B, ch, L), seed + 50) if ukw.get("self_condition") else None
        with torch.inference_mode():
            y = net(x, t, xsc)
        net64, _ = ref_net(d1, ukw, salt, torch.float64)
        with torch.inference_mode(), fp64_default():
            y64 = net64(x.double(), t, xsc.double() if xsc is not None else None)
        err = rel(y, y64)
        print(f"unet {key}: out {tuple(y.shape)} rms {float(y.pow(2).mean().sqrt()):.3f} reference fp32-vs-fp64 {err:.2e}")
        assert torch.isfinite(y).all()
        out["unet"][key] = dict(unet_kw=ukw, L=L, salt=salt, x=x, t=t, x_self_cond=xsc, y=y, ref_err=err)

    # ---- p_mean_variance ------------------------------------------------------------------------------------------------------
    ukw, L, B, salt, seed = UNETS["d32_c2"]
    net, _ = ref_net(d1, ukw, salt)
    T = 1000
    obj = d1.DenoisingDiffusion1D(net, seq_length=L, timesteps=T)
    x = seeded((B, ukw["channels"], L), 820)
    rows = []
    with torch.inference_mode():
        for t in (T - 1, T // 2, 1, 0):
            mean, var, logvar, x_start = obj.p_mean_variance(x, torch.full((B,), t, dtype=torch.long))
            assert all(torch.isfinite(v).all() for v in (mean, var, logvar, x_start))
            rows.append(dict(t=t, mean=mean, var=var.reshape(-1), logvar=logvar.reshape(-1), x_start=x_start.clone()))
    out["p_mean_variance"] = dict(unet="d32_c2", timesteps=T, beta_schedule="cosine", x=x, rows=rows)

    # ---- whole loops -----------------------------------------------------------------------------------------------------------
    out["loops"] = {}
    for key, (ukey, dkw, method, mkw, nseed) in LOOPS.items():
        ukw, L, B, salt, _ = UNETS[ukey]
        net, _ = ref_net(d1, ukw, salt)
        y = run_loop(d1, d1.DenoisingDiffusion1D, net, L, B, dkw, method, mkw, nseed)
        net64, _ = ref_net(d1, ukw, salt, torch.float64)
        with fp64_default():
            y64 = run_loop(d1, d1.DenoisingDiffusion1D, net64, L, B, dkw, method, mkw, nseed, torch.float64)
        err = rel(y, y64)
        print(f"loop {key}: mean {float(y.mean()):.4f} reference fp32-vs-fp64 {err:.2e}")
        assert torch.isfinite(y).all()
        out["loops"][key] = dict(unet=ukey, L=L, batch=B, diffusion_kw=dkw, method=method, method_kw=mkw, noise_seed=nseed,
                                 sample=y, ref_err=err)

    # the 1D quirk must be visible: against a loop that re-derives, and against the other clip setting
    class Rederive(d1.DenoisingDiffusion1D):
        def model_predictions(self, x, t, x_self_cond=None, clip_x_start=False, rederive_pred_noise=False):
            return super().model_predictions(x, t, x_self_cond, clip_x_start=clip_x_start, rederive_pred_noise=True)

    ukey, dkw, method, mkw, nseed = LOOPS["ddim8_clip"]
    ukw, L, B, salt, _ = UNETS[ukey]
    net, _ = ref_net(d1, ukw, salt)
    y_re = run_loop(d1, Rederive, net, L, B, dkw, method, mkw, nseed)
    m_re = rel(out["loops"]["ddim8_clip"]["sample"], y_re)
    m_clip = rel(out["loops"]["ddim8_noclip"]["sample"], out["loops"]["ddim8_clip"]["sample"])
    print(f"margins: raw vs re-derived pred_noise {m_re:.3e}, unclipped vs clipped {m_clip:.3e} (needed: {MARGIN:.0e})")
    assert m_re >= MARGIN and m_clip >= MARGIN, (m_re, m_clip)
    out["margins"] = dict(rederive=m_re, clip=m_clip, rederived_sample=y_re)

    # ---- interpolate ------------------------------------------------------------------------------------------------------------
    ukw, L, B, salt, _ = UNETS["d32_c2"]
    net, _ = ref_net(d1, ukw, salt)
    obj = d1.DenoisingDiffusion1D(net, seq_length=L, timesteps=50)
    x1, x2 = seeded((B, ukw["channels"], L), 831).clamp(-1, 1), seeded((B, ukw["channels"], L), 832).clamp(-1, 1)
    with patched_noise(d1, 833):
        y = obj.interpolate(x1, x2, t=20, lam=0.3)
    net64, _ = ref_net(d1, ukw, salt, torch.float64)
    obj64 = d1.DenoisingDiffusion1D(net64, seq_length=L, timesteps=50).double()
    with patched_noise(d1, 833, torch.float64), fp64_default():
        y64 = obj64.interpolate(x1.double(), x2.double(), t=20, lam=0.3)
    assert torch.isfinite(y).all()
    out["interpolate"] = dict(unet="d32_c2", timesteps=50, t=20, lam=0.3, x1=x1, x2=x2, noise_seed=833, y=y, ref_err=rel(y, y64))
    print(f"interpolate: reference fp32-vs-fp64 {out['interpolate']['ref_err']:.2e}")

    # ---- schedule buffers ----------------------------------------------------------------------------------------------------
    tiny = d1.Unet1D(dim=8, dim_mults=(1,), channels=1)
    out["sched"] = {}
    for name in ("linear", "cosine"):
        for objective in ("pred_noise", "pred_x0", "pred_v"):
            obj = d1.DenoisingDiffusion1D(tiny, seq_length=8, timesteps=1000, beta_schedule=name, objective=objective)
            out["sched"][f"{name}_{objective}"] = {k: v.clone() for k, v in obj.state_dict().items() if not k.startswith("model.")}
    obj = d1.DenoisingDiffusion1D(tiny, seq_length=8, timesteps=250, beta_schedule="cosine")
    out["sched"]["cosine250_pred_noise"] = {k: v.clone() for k, v in obj.state_dict().items() if not k.startswith("model.")}
    for k, bufs in out["sched"].items():
        assert len(bufs) == 13 and all(torch.isfinite(v).all() for v in bufs.values()), k
    out["state_dict_keys"] = list(d1.DenoisingDiffusion1D(d1.Unet1D(**UNETS["d32_c2"][0]), seq_length=32).state_dict().keys())

    # ---- surface --------------------------------------------------------------------------------------------------------------
    out["surface"] = dict(
        unet=surface(d1.Unet1D, ("forward",)),
        diffusion=surface(d1.DenoisingDiffusion1D, (
            "predict_start_from_noise", "predict_noise_from_start", "predict_v", "predict_start_from_v", "q_posterior",
            "model_predictions", "p_mean_variance", "p_sample", "p_sample_loop", "ddim_sample", "sample", "interpolate",
            "q_sample", "p_losses", "forward")))
    save("seq1d.pt", out)


if __name__ == "__main__":
    main()
