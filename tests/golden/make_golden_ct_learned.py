#!/usr/bin/env python3
"""Goldens for ``ContinuousTimeGaussianDiffusion(noise_schedule='learned')`` from the REFERENCE (build container only):
``python tests/golden/make_golden_ct_learned.py`` -> ``ct_learned.pt``.

The reference class with its ``learned_noise_schedule`` runs on name-seeded synthetic U-Nets (dim 32, mults (1, 2), 16x16,
B = 4).  Per case the file stores

* the schedule's state dict (perturbed away from its initialisation where the case says so), the times, ``log_snr(times)``
  from the fp32 module and from its fp64 twin;
* loss + ``backward()``: the U-Net gradient digests (packed as make_golden_edm_train packs them) and the six schedule
  gradients in full, each with the reference's own fp32-vs-fp64 error;
* dL/dx and dL/dtime of the U-Net's two inputs from autograd (a pass-through module around the U-Net clones both inputs and
  retains their gradients: the clone of log_snr collects the U-Net's share alone), with their fp32-vs-fp64 error;
* the N = 8 ``sample()`` output with injected noise and the scalars of every ``p_mean_variance`` call (log_snr recorded by
  a forward hook on the schedule module; c, alpha, sigma, alpha_next, the variance as make_golden_ct records them).  The
  share of output pixels on the final clamp is printed and must be at most 0.5.  The fp64 twin's scalars are stored beside
  them (p_mean_variance alone; the square root p_sample takes is restated there).
Only DATA is written."""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import import_reference, patched_noise, save  # noqa: E402
from make_golden_ct import NAMES, ref_net  # noqa: E402
from make_golden_edm_train import pack  # noqa: E402

D32 = dict(dim=32, dim_mults=(1, 2), learned_sinusoidal_cond=True)
RFF = dict(dim=32, dim_mults=(1, 2), random_fourier_features=True)
HAND = (0.05, 0.2, 0.5, 0.9)
B, SIZE, N_SAMPLE = 4, 16, 8
CASES = {
    # key: (unet kwargs, class kwargs, micro-batches, salt, draw seed, schedule seed, perturb, hand-set times, sample noise seed)
    "learned": (D32, dict(learned_schedule_net_hidden_dim=16), 1, 101, 701, 801, False, None, 901),
    "learned_h1024": (D32, dict(), 1, 102, 702, 802, True, None, 902),
    "learned_minsnr": (D32, dict(learned_schedule_net_hidden_dim=16, min_snr_loss_weight=True), 1, 103, 703, 803, True, HAND, 903),
    # the inputs, weights and schedule of `learned`: only frac_gradient differs
    "learned_frac025": (D32, dict(learned_schedule_net_hidden_dim=16, learned_noise_schedule_frac_gradient=0.25), 1, 101, 701,
                        801, False, None, 901),
    "learned_rff": (RFF, dict(learned_schedule_net_hidden_dim=16), 1, 105, 705, 805, True, None, 905),
    "learned_accumulate2": (D32, dict(learned_schedule_net_hidden_dim=16), 2, 106, 706, 806, True, None, 906),
}


class Tap(torch.nn.Module):
    """The U-Net behind clones of its two inputs whose gradients are retained."""

    self_condition = False

    def __init__(self, net):
        super().__init__()
        self.net = net
        self.random_or_learned_sinusoidal_cond = net.random_or_learned_sinusoidal_cond
        self.seen = []

    def forward(self, x, t):
        x, t = x.clone(), t.clone()
        if x.requires_grad:
            x.retain_grad()
            t.retain_grad()
            self.seen.append((x, t))
        return self.net(x, t)


class StepRecorder:
    """make_golden_ct.Recorder for a schedule that is a module: log_snr comes from a forward hook."""

    def __init__(self, mod, obj):
        self.mod, self.obj, self.calls = mod, obj, []

    def __enter__(self):
        rec, mod, obj = self, self.mod, self.obj
        self._expm1, self._sqrt = mod.expm1, mod.sqrt
        real_pmv = obj.p_mean_variance

        def hook(_m, _inp, out):
            if rec.calls and out.dim() == 0:
                cur = rec.calls[-1]
                cur["log_snr_next" if "log_snr" in cur else "log_snr"] = float(out)

        def expm1(v):
            out = rec._expm1(v)
            if rec.calls and out.dim() == 0:
                rec.calls[-1]["c"] = float(-out)
            return out

        def sqrt(v):
            out = rec._sqrt(v)
            if rec.calls and out.dim() == 0:
                cur = rec.calls[-1]
                for name in ("alpha", "sigma", "alpha_next", "sqrt_var"):
                    if name not in cur:
                        cur[name] = float(out)
                        break
            return out

        def pmv(*a, **k):
            rec.calls.append({})
            mean, var = real_pmv(*a, **k)
            rec.calls[-1]["posterior_variance"] = float(var)
            return mean, var

        self._hook = obj.log_snr.register_forward_hook(hook)
        mod.expm1, mod.sqrt, obj.p_mean_variance = expm1, sqrt, pmv
        return self

    def __exit__(self, *exc):
        self._hook.remove()
        self.mod.expm1, self.mod.sqrt = self._expm1, self._sqrt
        del self.obj.p_mean_variance

    def table(self):
        return torch.tensor([[c.get(n, float("nan")) for n in NAMES] for c in self.calls], dtype=torch.float64)


def build(dd, ctm, ukw, ckw, salt, sched_seed, perturb, dtype):
    net, spec = ref_net(dd, ukw, salt, dtype)
    torch.manual_seed(sched_seed)
    obj = ctm.ContinuousTimeGaussianDiffusion(Tap(net), image_size=SIZE, noise_schedule="learned", num_sample_steps=N_SAMPLE,
                                              **ckw)
    if perturb:
        g = torch.Generator().manual_seed(sched_seed + 1)
        with torch.no_grad():
            for p in obj.log_snr.parameters():
                p.mul_(1 + 0.3 * torch.randn(p.shape, generator=g)).add_(0.05 * torch.randn(p.shape, generator=g))
    obj.log_snr.to(dtype)
    return net, spec, obj


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def run(obj, net, imgs, times, noises, dtype):
    micro = len(imgs)
    total = 0.0
    for i in range(micro):
        loss = obj.p_losses(imgs[i].to(dtype) * 2 - 1, times[i].to(dtype), noise=noises[i].to(dtype).clone()) / micro
        loss.backward()
        total += float(loss)
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in net.named_parameters()}
    sgrads = {k: p.grad.clone() for k, p in obj.log_snr.named_parameters()}
    dx = [x.grad.clone() for x, _ in obj.model.seen]
    dt = [t.grad.clone() for _, t in obj.model.seen]
    return total, grads, sgrads, dx, dt


def case(dd, ctm, ukw, ckw, micro, salt, seed, sched_seed, perturb, hand, nseed):
    net, spec, obj = build(dd, ctm, ukw, ckw, salt, sched_seed, perturb, torch.float32)
    obj.train()
    sched_sd = {k: v.clone() for k, v in obj.log_snr.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    imgs = [torch.rand((B, 3, SIZE, SIZE), generator=g) for _ in range(micro)]
    times = [torch.tensor(hand) if hand is not None else 0.02 + 0.93 * torch.rand((B,), generator=g) for _ in range(micro)]
    noises = [torch.randn((B, 3, SIZE, SIZE), generator=g) for _ in range(micro)]
    total, grads, sgrads, dx, dt = run(obj, net, imgs, times, noises, torch.float32)
    frozen = [k for k, p in net.named_parameters() if not p.requires_grad]
    net64, _, obj64 = build(dd, ctm, ukw, ckw, salt, sched_seed, perturb, torch.float64)
    obj64.train()
    total64, g64, s64, dx64, dt64 = run(obj64, net64, imgs, times, noises, torch.float64)
    err = {k: rel(grads[k], g64[k]) for k, _ in spec}
    # a schedule gradient's error is taken relative to the norm of all six: the last bias cancels in the normalisation, so
    # its own gradient is rounding noise around an exact zero
    snorm = torch.cat([v.reshape(-1) for v in s64.values()]).norm()
    serr = {k: float((sgrads[k].double() - s64[k]).norm() / snorm) for k in sgrads}
    with torch.no_grad():
        log_snr = [obj.log_snr(t) for t in times]
        log_snr64 = [obj64.log_snr(t.double()) for t in times]
    # sampling (eval mode, the reference's own loop), then the scalars of its eight p_mean_variance calls
    obj.eval()
    with patched_noise(ctm, nseed), StepRecorder(ctm, obj) as rec:
        y = obj.sample(batch_size=2)
    share = float(((y == 0) | (y == 1)).float().mean())
    assert share <= 0.5, share
    # the same scalars from the fp64 twin (the image does not enter them)
    steps = torch.linspace(1., 0., N_SAMPLE + 1)
    obj64.eval()
    with torch.no_grad(), StepRecorder(ctm, obj64) as rec64:
        for i in range(N_SAMPLE):
            obj64.p_mean_variance(torch.zeros((1, 3, SIZE, SIZE), dtype=torch.float64), steps[i].double(), steps[i + 1].double())
            (rec64.calls[-1].__setitem__("sqrt_var", rec64.calls[-1]["posterior_variance"] ** 0.5) if i < N_SAMPLE - 1 else None)
    unwrap = lambda k: k.replace("model.net.", "model.", 1)  # the pass-through module is not part of the reference's names
    names = [unwrap(k) for k, _ in obj.named_parameters()]
    return dict(unet_kw=ukw, ct_kw=ckw, image_size=SIZE, B=B, micro=micro, salt=salt, imgs=imgs, times=times, noises=noises,
                sched=sched_sd, log_snr=log_snr, log_snr64=log_snr64,
                ref_err_log_snr=[(a.double() - b).abs() for a, b in zip(log_snr, log_snr64)],
                loss=total, loss64=total64, ref_err_loss=abs(total - total64) / abs(total64),
                grads=pack(spec, grads), frozen=frozen, ref_err_grads=torch.tensor([err[k] for k, _ in spec]),
                ref_err_grad_max=max(err.values()),
                sched_grads=sgrads, sched_grads64=s64, ref_err_sched_grads=serr, ref_err_sched_grad_max=max(serr.values()),
                dx=dx, dtime=dt, dtime64=dt64, ref_err_dx=[rel(a, b) for a, b in zip(dx, dx64)],
                ref_err_dtime=[rel(a, b) for a, b in zip(dt, dt64)],
                sample=y, sample_noise_seed=nseed, n=N_SAMPLE, scalars=rec.table(), scalars64=rec64.table(),
                clamp_share=share, steps=steps, parameter_names=names,
                state_dict_keys=[unwrap(k) for k in obj.state_dict().keys()]), share


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    dd, _, _ = import_reference()
    import denoising_diffusion.continuous_time_gaussian_diffusion as ctm

    out = {"names": list(NAMES), "cases": {}}
    for key, args in CASES.items():
        c, share = case(dd, ctm, *args)
        out["cases"][key] = c
        print(key, "loss", c["loss"], "fp64", c["loss64"], "reference fp32-vs-fp64: loss", c["ref_err_loss"], "worst U-Net gradient",
              c["ref_err_grad_max"], "schedule gradients", c["ref_err_sched_grad_max"], "dx", max(c["ref_err_dx"]),
              "dtime", max(c["ref_err_dtime"]), "log_snr", [round(v, 3) for v in c["log_snr"][0].tolist()],
              "on the final clamp:", share)
    save("ct_learned.pt", out)


if __name__ == "__main__":
    main()
