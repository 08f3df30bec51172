"""What the per-operator convolution suites share (tests/test_hip_conv_families.py, tests/test_hip_vae_conv_ops.py): seeded
inputs and their families, the bracket that reads the library's detail profile rows around one call, the assertion that a
row of the named kernel family is among them, the two metrics, and the Checker that prints and judges every tensor of a case
against 4 x the fp32 floor.  Each suite passes its own Counter and the tag of its printed lines."""
import re

import torch

from diffusion_models_amd import _lib

FACTOR = 4.0
DEV = "cuda:0"
PREFIX = {"conv": "conv<", "wino": "wino ", "wino4": "wino4<", "upwino": "upwino<", "pw": "pw<", "init7": "init7 "}
KERNEL = {"conv": "conv_mfma", "wino": "wino_mfma", "wino4": "wino4_mfma", "upwino": "upwino_mfma", "pw": "pw_mfma",
          "init7": "init7_mfma"}


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def family_input(t, family, seed):
    """randn: t as drawn.  offset: t + 4 (activations behind SiLU).  wide: channel c times exp(u_c), u spread evenly over
    [-4.6, 4.6] and shuffled.  flat: 4 + 0.01 t (the F(4x4) input transform cancels)."""
    if family == "randn":
        return t
    if family == "offset":
        return t + 4
    if family == "flat":
        return 4 + 0.01 * t
    assert family == "wide"
    C = t.shape[1]
    u = torch.linspace(-4.6, 4.6, C)[torch.randperm(C, generator=torch.Generator().manual_seed(seed))]
    return t * torch.exp(u)[None, :, None, None]


def profiled_call(fn):
    _lib.profile_read()
    fn()
    return [r["kernel"] for r in _lib.profile_read()]


def assert_row(counts, label, rows, family, shape, tokens=()):
    """A row of `family` (PREFIX) with the layer `shape` in its name; tokens: q1 / q2 / r1 / r4 literally, 'k>1' a K split."""
    hits = [r for r in rows if r.startswith(PREFIX[family]) and shape in r]
    assert hits, (label, f"no {KERNEL[family]} row with '{shape}'", rows)
    for tok in tokens:
        if tok == "k>1":
            k = [int(m.group(1)) for r in hits for m in [re.search(r" k(\d+)", r)] if m]
            assert k and max(k) > 1, (label, "no K split", hits)
        else:
            assert any(f" {tok}" in r for r in hits), (label, f"no row with {tok}", hits)
    counts[KERNEL[family]] += 1
    return hits[0]


def metrics(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d = got - ref
    return (float(d.norm() / ref.norm().clamp_min(1e-300)),
            float(d.abs().max() / ref.pow(2).mean().sqrt().clamp_min(1e-300)))


class Checker:
    """Prints, then asserts at the end, every tensor of one case: no tensor hides behind the first failure."""

    def __init__(self, tag, counts, label, family, bound):
        self.tag, self.counts, self.label, self.family, self.bound, self.bad = tag, counts, label, family, bound, []

    def __call__(self, tensor, kernel, got, ref64, floor32):
        e = metrics(got, ref64)
        f = metrics(floor32, ref64)
        lim = [FACTOR * f[0], FACTOR * f[1]]
        if self.family == "randn":
            lim[0] = min(lim[0], self.bound)
        print(f"{self.tag} {self.label} {tensor} {kernel}: rel-L2 kernel {e[0]:.3g} floor {f[0]:.3g} limit "
              f"{lim[0]:.3g} | max/rms kernel {e[1]:.3g} floor {f[1]:.3g} limit {lim[1]:.3g}")
        if not torch.isfinite(got).all():
            self.bad.append((tensor, "not finite", int((~torch.isfinite(got)).sum())))
        elif e[0] > lim[0] or e[1] > lim[1]:
            self.bad.append((tensor, kernel, e, lim))

    def done(self):
        self.counts["cases run"] += 1
        assert not self.bad, (self.label, self.bad)
