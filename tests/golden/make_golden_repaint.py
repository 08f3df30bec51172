#!/usr/bin/env python3
"""RePaint inpainting goldens from the REFERENCE (build container only):
``python tests/golden/make_golden_repaint.py`` -> ``repaint.pt``.

``repaint.GaussianDiffusion`` runs on name-seeded synthetic weights (dim 32, mults (1, 2), 16x16, B = 2, 20 timesteps) with
``torch.randn`` / ``randn_like`` redirected to a seeded NoiseStream.  Stored per loop case: the settings, ``gt``, ``mask``,
the output (for ``return_all_timesteps`` its shape and the last frames only), the RECORDED sequence of ``(t, had mask)``
calls of ``p_sample``, the share of unknown-region output pixels on the final clamp (asserted <= 0.5) and the reference's own
fp32-vs-fp64 discrepancy: the same module in float64 on the same noise.  Besides: single ``p_sample`` calls, the schedule
buffers the loop's scalars come from, and the class's surface.  Only DATA is written."""
from __future__ import annotations

import inspect
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, import_reference, patched_noise, save, seeded  # noqa: E402

import diffusion_models_amd as dm  # noqa: E402
from diffusion_models_amd.spec import UnetConfig  # noqa: E402

UKW = dict(dim=32, dim_mults=(1, 2))
SIZE, B, T, SALT, NOISE_SEED, GT_SEED = 16, 2, 20, 31, 360, 5
RS = dict(resample=True, resample_iter=2, resample_jump=3, resample_every=4)
KEEP_FRAMES = 4


def masks():
    half = torch.zeros(B, 1, SIZE, SIZE)
    half[..., SIZE // 2:] = 1.0  # keep the right half
    per = torch.zeros(B, 3, SIZE, SIZE)  # different per image and per channel
    per[0, 0, :8], per[0, 1, :, :8], per[0, 2, 4:12, 4:12] = 1.0, 1.0, 1.0
    per[1, 0, 8:], per[1, 1, :, 8:], per[1, 2, ::2] = 1.0, 1.0, 1.0
    return half, per


def cases():
    half, per = masks()
    return {
        # key: (class kwargs, mask, sample kwargs)
        "a": (dict(objective="pred_noise", beta_schedule="cosine"), half, dict(RS)),
        "b": (dict(objective="pred_v", beta_schedule="sigmoid"), per, dict(RS)),
        "c": (dict(objective="pred_x0", beta_schedule="cosine"), half, dict(resample=False)),
        "d": (dict(objective="pred_noise", beta_schedule="cosine", auto_normalize=False), half, dict(RS)),
        "e": (dict(objective="pred_noise", beta_schedule="cosine"), half, dict(RS, return_all_timesteps=True)),
        "g": (dict(objective="pred_noise", beta_schedule="cosine"), None, {}),
    }


def import_repaint():
    import_reference()

    class _Dummy:
        def __init__(self, *a, **k):
            pass

    for name in ("pytorch_fid", "pytorch_fid.inception", "pytorch_fid.fid_score"):
        m = types.ModuleType(name)
        m.__path__ = []
        m.InceptionV3, m.calculate_frechet_distance = _Dummy, None
        sys.modules[name] = m
    sys.path.insert(0, os.path.join(REF, "denoising-diffusion-pytorch", "denoising_diffusion"))  # its `from utils import *`
    import denoising_diffusion.repaint as rp

    return rp


def ref_obj(rp, ckw, dtype=torch.float32):
    spec = dm.unet_param_spec(UnetConfig(channels=3, **UKW))
    sd = dm.synth_state_dict(spec, salt=SALT)
    net = rp.Unet(channels=3, **UKW).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True)
    obj = rp.GaussianDiffusion(net.eval(), image_size=SIZE, timesteps=T, **ckw)
    return obj.to(dtype) if dtype != torch.float32 else obj


class noise_as(patched_noise):
    """patched_noise whose draws come in another dtype (the float64 twin reads the SAME values).  While it is active
    torch's default dtype is that dtype too: the reference's sinusoidal embedding builds its frequencies in the default
    dtype, which a float64 module must match."""

    def __init__(self, module, seed, dtype):
        super().__init__(module, seed)
        base = self.stream
        self.dtype = dtype
        self.stream = lambda shape: base(shape).to(dtype)

    def __enter__(self):
        self._default = torch.get_default_dtype()
        torch.set_default_dtype(self.dtype)
        return super().__enter__()

    def __exit__(self, *exc):
        torch.set_default_dtype(self._default)
        return super().__exit__(*exc)


def run_loop(rp, ckw, gt, mask, skw, dtype=torch.float32):
    obj = ref_obj(rp, ckw, dtype)
    calls = []
    real = obj.p_sample

    def p_sample(x, t, x_self_cond=None, gt=None, mask=None):
        calls.append((int(t), mask is not None))
        return real(x=x, t=t, x_self_cond=x_self_cond, gt=gt, mask=mask)

    obj.p_sample = p_sample
    with noise_as(rp, NOISE_SEED, dtype):
        y = obj.sample(batch_size=B, gt=None if gt is None else gt.to(dtype), mask=None if mask is None else mask.to(dtype),
                       **skw)
    return y, calls


def surface(cls):
    sig = inspect.signature(cls.__init__)
    init = [(p.name, None if p.default is inspect.Parameter.empty else p.default, p.kind.name)
            for p in sig.parameters.values() if p.name != "self"]
    methods = {}
    for name in ("p_sample", "p_sample_loop", "sample"):
        methods[name] = [(p.name, None if p.default is inspect.Parameter.empty else p.default)
                         for p in inspect.signature(getattr(cls, name)).parameters.values() if p.name != "self"]
    public = sorted(n for n, v in vars(cls).items() if not n.startswith("_") and (callable(v) or isinstance(v, property)))
    return dict(init_params=init, methods=methods, names=public)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rp = import_repaint()
    gt = torch.rand((B, 3, SIZE, SIZE), generator=torch.Generator().manual_seed(GT_SEED))
    out = dict(unet_kw=UKW, image_size=SIZE, batch=B, timesteps=T, salt=SALT, noise_seed=NOISE_SEED, gt=gt, loops={})

    for key, (ckw, mask, skw) in cases().items():
        y, calls = run_loop(rp, ckw, gt if mask is not None else None, mask, skw)
        y64, calls64 = run_loop(rp, ckw, gt if mask is not None else None, mask, skw, torch.float64)
        assert calls == calls64 and y64.dtype == torch.float64
        final = y[:, -1] if skw.get("return_all_timesteps") else y
        final64 = y64[:, -1] if skw.get("return_all_timesteps") else y64
        ref_err = float((final.double() - final64).norm() / final64.norm())
        unknown = (torch.ones_like(final) if mask is None else (1 - mask).expand_as(final)) > 0
        lo, hi = (0.0, 1.0) if ckw.get("auto_normalize", True) else (-1.0, 1.0)
        share = float(((final == lo) | (final == hi))[unknown].float().mean())
        print(key, "mean", float(final.mean()), "unknown pixels on the final clamp:", share, "fp32-vs-fp64:", ref_err)
        assert share <= 0.5, (key, share)
        c = dict(diffusion_kw=ckw, mask=mask, sample_kw=skw, calls=calls, clamp_share=share, ref_err=ref_err)
        if skw.get("return_all_timesteps"):
            c.update(shape=tuple(y.shape), last_frames=y[:, -KEEP_FRAMES:].clone(), n_last=KEEP_FRAMES)
        else:
            c["sample"] = y
        out["loops"][key] = c

    # (f) single p_sample calls; the draws of one call: z_known, then z_step when t > 0
    half, _ = masks()
    x = seeded((B, 3, SIZE, SIZE), 370)
    out["p_sample"] = dict(x=x, mask=half, steps={})
    for objective, sched in (("pred_noise", "cosine"), ("pred_x0", "cosine"), ("pred_v", "sigmoid")):
        ckw = dict(objective=objective, beta_schedule=sched)
        obj, obj64 = ref_obj(rp, ckw), ref_obj(rp, ckw, torch.float64)
        rows = []
        for t in (0, 3, 19):
            with patched_noise(rp, 380 + t):
                y, xs = obj.p_sample(x, t, gt=gt, mask=half)
            with noise_as(rp, 380 + t, torch.float64):
                y64, _ = obj64.p_sample(x.double(), t, gt=gt.double(), mask=half.double())
            rows.append(dict(t=t, noise_seed=380 + t, y=y, x_start=xs,
                             ref_err=float((y.double() - y64).norm() / y64.norm())))
        out["p_sample"]["steps"][objective] = dict(diffusion_kw=ckw, steps=rows)

    # the fp32 buffers the loop's scalars are taken from, and the defaults' row structure
    out["buffers"] = {}
    for sched in ("cosine", "sigmoid"):
        obj = ref_obj(rp, dict(beta_schedule=sched))
        out["buffers"][sched] = {k: getattr(obj, k).clone() for k in ("betas", "alphas_cumprod")}
    out["surface"] = surface(rp.GaussianDiffusion)
    save("repaint.pt", out)


if __name__ == "__main__":
    main()
