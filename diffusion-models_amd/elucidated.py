"""Host-side mirror of the reference ``ElucidatedDiffusion`` (Karras et al., "Elucidating the Design Space of
Diffusion-Based Generative Models") in front of ``dm_sample_edm`` in libdm_hip.so.

Same constructor arguments, method names and ``state_dict`` keys as
  denoising-diffusion-pytorch/denoising_diffusion/elucidated_diffusion.py:22-264
for sampling -- the Heun loop (``sample``) and DPM-Solver++(2M) (``sample_using_dpmpp``) -- and for training (``forward``,
the weighted denoising loss of :228-264 with its backward pass).  The per-step and per-image scalars are computed here
the way the reference computes them -- preconditioning terms as fp32 tensor arithmetic, the churn terms as Python doubles
rounded to fp32 once -- and handed to the library as a table; the kernels hold no schedule logic.

Over a ``KarrasUnet`` (karras.py) both loops run too -- a stated deviation: the reference's constructor raises
``AttributeError`` on that network -- and ``class_labels=`` carries the labels of a class-conditional one.

Extensions (keyword-only, as on the other samplers): ``noise`` injects a source of N(0,1) draws called in the
reference's order (the start image, then one draw per Heun step); ``seed`` / ``sample_offset`` select the device Philox
stream and the index of the call's first sample in a global batch.

Training: ``train()`` arms the U-Net through ``dm_unet_train_enable_ft`` (``Unet.train()`` keeps refusing a learned /
random sinusoidal U-Net: it arms the integer-time ``p_losses`` path, which would truncate ``c_noise(sigma)``);
``forward(images)`` is then one ``dm_unet_loss_backward_edm`` call -- loss and every parameter gradient, no autograd graph.
Its keyword-only extensions: ``sigmas`` / ``noise`` inject the two draws (without them sigma comes from torch's global CPU
generator, drawn first as in the reference, and the noise from the device Philox stream), ``loss_scale`` / ``accumulate``
are the micro-batch loop of ``Trainer.train``, ``sync=False`` leaves the loss on the device, ``return_denoised`` also
returns the denoised images.  ``train_step`` / ``EMA`` / ``save_checkpoint`` of train.py take the object as they take a
``DenoisingDiffusion``.
"""
from __future__ import annotations

import ctypes as C
from math import sqrt
from typing import Optional

import torch

from . import _lib
from ._floattime import FloatTimeDiffusion
from ._lib import fptr as _fptr

COLS = _lib.DM_EDM_COEFS
# columns of a step-table row (csrc/edm.h)
CHURN, S_NOISE, C_IN, C_NOISE, C_SKIP, C_OUT, SIGMA, DT, C_IN2, C_NOISE2, C_SKIP2, C_OUT2, SIGMA2, HALF_DT = range(14)
LOSS_W = 14  # training rows only
A, B_, G, OMG = C_IN2, C_NOISE2, C_SKIP2, C_OUT2  # DPM-Solver++ reuses the second preconditioning block


def edm_sigmas(num_sample_steps, sigma_min=0.002, sigma_max=80, rho=7) -> torch.Tensor:
    """``sample_schedule`` (:117-127, equation 5): N fp32 noise levels from sigma_max down to sigma_min, then 0."""
    n = int(num_sample_steps)
    inv_rho = 1 / rho
    steps = torch.arange(n, dtype=torch.float32)
    sigmas = (sigma_max ** inv_rho + steps / (n - 1) * (sigma_min ** inv_rho - sigma_max ** inv_rho)) ** rho
    return torch.cat((sigmas, sigmas.new_zeros(1)))


def edm_precond(sigma: torch.Tensor, sigma_data=0.5):
    """(c_in, c_noise, c_skip, c_out) of an fp32 sigma tensor (:76-86, Table 1), in the reference's tensor arithmetic."""
    c_skip = (sigma_data ** 2) / (sigma ** 2 + sigma_data ** 2)
    c_out = sigma * sigma_data * (sigma_data ** 2 + sigma ** 2) ** -0.5
    c_in = 1 * (sigma ** 2 + sigma_data ** 2) ** -0.5
    c_noise = torch.log(sigma.clamp(min=1e-20)) * 0.25
    return c_in, c_noise, c_skip, c_out


def _precond_of_float(sigma: float, sigma_data):
    """The four terms for a Python-float sigma: the reference builds ``torch.full((batch,), sigma)`` (fp32) first (:94-95)."""
    return tuple(float(v) for v in edm_precond(torch.full((1,), float(sigma)), sigma_data))


def edm_heun_table(num_sample_steps, sigma_min=0.002, sigma_max=80, sigma_data=0.5, rho=7, S_churn=80, S_tmin=0.05,
                   S_tmax=50, S_noise=1.003) -> torch.Tensor:
    """(N, DM_EDM_COEFS) fp32 step table of ``sample`` (:137-181); the layout is documented in include/dm_hip.h."""
    n = int(num_sample_steps)
    sigmas = edm_sigmas(n, sigma_min, sigma_max, rho)
    gammas = torch.where((sigmas >= S_tmin) & (sigmas <= S_tmax), min(S_churn / n, sqrt(2) - 1), 0.0)
    tab = torch.zeros((n, COLS), dtype=torch.float64)
    for i in range(n):
        sigma, sigma_next, gamma = sigmas[i].item(), sigmas[i + 1].item(), gammas[i].item()
        sigma_hat = sigma + gamma * sigma
        row = tab[i]
        row[CHURN] = sqrt(sigma_hat ** 2 - sigma ** 2)
        row[S_NOISE] = S_noise
        row[C_IN], row[C_NOISE], row[C_SKIP], row[C_OUT] = _precond_of_float(sigma_hat, sigma_data)
        row[SIGMA] = sigma_hat
        row[DT] = sigma_next - sigma_hat
        row[C_IN2], row[C_NOISE2], row[C_SKIP2], row[C_OUT2] = _precond_of_float(sigma_next, sigma_data)
        row[SIGMA2] = sigma_next
        row[HALF_DT] = 0.5 * (sigma_next - sigma_hat)
    return tab.to(torch.float32)  # doubles are rounded once, where they meet an fp32 tensor; fp32 values pass unchanged


def edm_dpmpp_table(num_sample_steps, sigma_min=0.002, sigma_max=80, sigma_data=0.5, rho=7) -> torch.Tensor:
    """(N, DM_EDM_COEFS) fp32 step table of ``sample_using_dpmpp`` (:198-221): a, expm1(-h) and gamma are 0-dim fp32
    tensor expressions in the reference, and so they are here."""
    n = int(num_sample_steps)
    sigmas = edm_sigmas(n, sigma_min, sigma_max, rho)

    def sigma_fn(t):
        return t.neg().exp()

    def t_fn(sigma):
        return sigma.log().neg()

    tab = torch.zeros((n, COLS), dtype=torch.float32)
    for i in range(n):
        row = tab[i]
        row[C_IN], row[C_NOISE], row[C_SKIP], row[C_OUT] = _precond_of_float(sigmas[i].item(), sigma_data)
        row[SIGMA] = sigmas[i]
        row[SIGMA2] = sigmas[i + 1]
        t, t_next = t_fn(sigmas[i]), t_fn(sigmas[i + 1])
        h = t_next - t
        row[A] = sigma_fn(t_next) / sigma_fn(t)
        row[B_] = (-h).expm1()
        if i == 0 or sigmas[i + 1] == 0:
            row[G], row[OMG] = 0.0, 1.0  # denoised_d = denoised
        else:
            h_last = t - t_fn(sigmas[i - 1])
            r = h_last / h
            gamma = -1 / (2 * r)
            row[G], row[OMG] = gamma, 1 - gamma
    return tab


def edm_loss_weight(sigma: torch.Tensor, sigma_data=0.5) -> torch.Tensor:
    """``loss_weight`` (:228-229) of an fp32 sigma tensor."""
    return (sigma ** 2 + sigma_data ** 2) * (sigma * sigma_data) ** -2


def edm_train_table(sigmas: torch.Tensor, sigma_data=0.5) -> torch.Tensor:
    """(B, DM_EDM_COEFS) fp32 rows of ``forward`` (:234-264), one per image: the preconditioning terms and sigma in their
    step-table columns, ``loss_weight(sigma)`` in column 14 -- fp32 tensor expressions on the (B,) sigma tensor, as
    ``preconditioned_network_forward`` and ``loss_weight`` evaluate them."""
    sig = sigmas.detach().to("cpu", torch.float32).reshape(-1)
    tab = torch.zeros((sig.numel(), COLS), dtype=torch.float32)
    tab[:, C_IN], tab[:, C_NOISE], tab[:, C_SKIP], tab[:, C_OUT] = edm_precond(sig, sigma_data)
    tab[:, SIGMA] = sig
    tab[:, LOSS_W] = edm_loss_weight(sig, sigma_data)
    return tab


class ElucidatedDiffusion(FloatTimeDiffusion):
    """``ElucidatedDiffusion(net, image_size=...)`` -- drop-in for the reference class: training loss and samplers."""

    _unet_attr = "net"
    _train_entry = "dm_unet_loss_backward_edm"

    def __init__(
        self,
        net,
        *,
        image_size,
        channels=3,
        num_sample_steps=32,
        sigma_min=0.002,
        sigma_max=80,
        sigma_data=0.5,
        rho=7,
        P_mean=-1.2,
        P_std=1.2,
        S_churn=80,
        S_tmin=0.05,
        S_tmax=50,
        S_noise=1.003,
        use_graph=True,
    ):
        self._init_unet(net, image_size, channels, use_graph, "ElucidatedDiffusion calls net(x, t, self_cond) only")
        self.self_condition = net.self_condition
        self.sigma_min = sigma_min
        self.sigma_max = sigma_max
        self.sigma_data = sigma_data
        self.rho = rho
        self.P_mean = P_mean
        self.P_std = P_std
        self.num_sample_steps = num_sample_steps
        self.S_churn = S_churn
        self.S_tmin = S_tmin
        self.S_tmax = S_tmax
        self.S_noise = S_noise

    @staticmethod
    def _refuse_self_condition(net):
        if getattr(net, "self_condition", False):
            raise NotImplementedError("ElucidatedDiffusion with a self_condition U-Net is not built on the HIP path")

    # -- Table 1 -----------------------------------------------------------------------------------
    def c_skip(self, sigma):
        return (self.sigma_data ** 2) / (sigma ** 2 + self.sigma_data ** 2)

    def c_out(self, sigma):
        return sigma * self.sigma_data * (self.sigma_data ** 2 + sigma ** 2) ** -0.5

    def c_in(self, sigma):
        return 1 * (sigma ** 2 + self.sigma_data ** 2) ** -0.5

    def c_noise(self, sigma):
        return torch.log(sigma.clamp(min=1e-20)) * 0.25

    def loss_weight(self, sigma):
        return edm_loss_weight(sigma, self.sigma_data)

    def _draw_sigmas(self, batch_size):
        return (self.P_mean + self.P_std * torch.randn((batch_size,))).exp()

    def noise_distribution(self, batch_size):
        """:231-232; the (batch_size,) draw comes from torch's global CPU generator."""
        return self._draw_sigmas(batch_size).to(self.device)

    def sample_schedule(self, num_sample_steps=None):
        n = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        return edm_sigmas(n, self.sigma_min, self.sigma_max, self.rho).to(self.device)

    # -- equation 7 --------------------------------------------------------------------------------
    def preconditioned_network_forward(self, noised_images, sigma, self_cond=None, clamp=False, *, class_labels=None):
        """:91-110.  ``sigma``: a float or a (B,) tensor.  The scalings run in dm_op_edm_churn_in / dm_op_edm_euler, the
        network through the float-time forward.  ``class_labels``: for a class-conditional network (``_labels``)."""
        if self_cond is not None:
            raise NotImplementedError("self-conditioning is not built on the HIP ElucidatedDiffusion path")
        x = noised_images.to(self.device, torch.float32).contiguous()
        b, per = x.shape[0], x[0].numel()
        if isinstance(sigma, float):
            sig = torch.full((1,), sigma)
        else:
            sig = sigma.detach().to("cpu", torch.float32).reshape(-1)
            if sig.numel() != b:
                raise RuntimeError(f"sigma has {sig.numel()} entries for a batch of {b}")
        rows = sig.numel()
        tab = torch.zeros((rows, COLS), dtype=torch.float32)
        tab[:, C_IN], tab[:, C_NOISE], tab[:, C_SKIP], tab[:, C_OUT] = edm_precond(sig, self.sigma_data)
        tab[:, SIGMA] = sig
        stream = self._stream()
        xin = torch.empty_like(x)
        _lib.check(self._lib.dm_op_edm_churn_in(_lib.ptr(x), None, _fptr(tab), rows, 0, 1, 0, None, _lib.ptr(xin), b, per,
                                                stream))
        self._labels(class_labels, b)
        kw = {} if class_labels is None else dict(class_labels=class_labels)
        net_out = self.net(xin, tab[:, C_NOISE].expand(b).contiguous().to(self.device), **kw)
        out = torch.empty_like(x)
        _lib.check(self._lib.dm_op_edm_euler(_lib.ptr(x), _lib.ptr(net_out), _fptr(tab), rows, int(bool(clamp)),
                                             _lib.ptr(out), None, None, None, b, per, stream))
        return out

    # -- sampling ----------------------------------------------------------------------------------
    def _labels(self, class_labels, batch):
        """The keyword extension ``class_labels=`` of the loops: required by a network with ``num_classes``
        (``KarrasUnet``), refused by every other, as the network's own assert does.  The labels become device data of the
        handle's conditioning head, so the captured step graph serves any labels."""
        net = self.net
        if not hasattr(net, "set_class_labels"):
            assert class_labels is None, "class_labels= needs a class-conditional network (KarrasUnet(num_classes=...))"
            return
        net.set_class_labels(class_labels, batch)

    def _run(self, kind, table, sigma_init, batch_size, clamp, noise, noise_rows, seed, sample_offset, class_labels=None):
        shape = (int(batch_size), self.channels, self.image_size, self.image_size)
        self._labels(class_labels, shape[0])
        f = self.net.downsample_factor
        assert shape[0] > 0 and self.image_size % f == 0, f"shape {shape}: the sides must be divisible by {f}"
        seed, x_init, noise_dev = self._start(shape, noise, noise_rows, seed, sample_offset)
        table = table.contiguous()
        out = torch.empty(shape, device=self.device, dtype=torch.float32)
        a = _lib.EdmArgs()
        a.kind, a.n_steps, a.table_host = kind, table.shape[0], _fptr(table)
        a.x_init, a.noise, a.seed, a.sample_offset = _lib.ptr(x_init), _lib.ptr(noise_dev), seed, int(sample_offset)
        a.out, a.sigma_init, a.clamp = _lib.ptr(out), float(sigma_init), int(bool(clamp))
        a.B, a.H, a.W = shape[0], shape[2], shape[3]
        a.use_graph, a.stream = 1 if self.use_graph else 0, self._stream()
        _lib.check(self._lib.dm_sample_edm(self.net._handle, C.byref(a)))
        return out

    def sample(self, batch_size=16, num_sample_steps=None, clamp=True, *, noise=None, seed=None, sample_offset=0,
               class_labels=None):
        """:129-187, the stochastic Heun sampler (Algorithm 2).  The reference draws the churn noise at every step, so an
        injected ``noise`` source is called once per step whatever gamma is."""
        n = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        table = edm_heun_table(n, self.sigma_min, self.sigma_max, self.sigma_data, self.rho, self.S_churn, self.S_tmin,
                               self.S_tmax, self.S_noise)
        sigma_init = edm_sigmas(n, self.sigma_min, self.sigma_max, self.rho)[0].item()
        return self._run(_lib.EDM_HEUN, table, sigma_init, batch_size, clamp, noise, n, seed, sample_offset, class_labels)

    def sample_using_dpmpp(self, batch_size=16, num_sample_steps=None, *, noise=None, seed=None, sample_offset=0,
                           class_labels=None):
        """:189-224, DPM-Solver++(2M): one network evaluation per step, one draw (the start image)."""
        n = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        table = edm_dpmpp_table(n, self.sigma_min, self.sigma_max, self.sigma_data, self.rho)
        sigma_init = edm_sigmas(n, self.sigma_min, self.sigma_max, self.rho)[0].item()
        return self._run(_lib.EDM_DPMPP, table, sigma_init, batch_size, False, noise, 0, seed, sample_offset, class_labels)

    # -- training ----------------------------------------------------------------------------------
    def forward(self, images, *, sigmas=None, noise=None, loss_scale=1.0, accumulate=False, sync=True,
                return_denoised=False):
        """:234-264: the loss (0-dim CPU tensor; ``sync=False``: a 0-dim device tensor, nothing waited for); the parameter
        gradients stay on the U-Net (``self.net.grad(name)`` / ``.grads()``).  ``images`` in [0, 1]."""
        net = self._trainable()
        b, c, h, w = images.shape
        assert h == self.image_size and w == self.image_size, f"height and width of image must be {self.image_size}"
        assert c == self.channels, "mismatch of image channels"
        if not getattr(net, "_training", False):
            self.train()
        # the reference's order of draws: sigma (:242), then the noise (:245)
        sig = self._draw_sigmas(b) if sigmas is None else sigmas.detach().to("cpu", torch.float32).reshape(-1)
        if sig.numel() != b:
            raise RuntimeError(f"sigmas has {sig.numel()} entries for a batch of {b}")
        images, noise = self._loss_inputs(images, noise)
        tab = edm_train_table(sig, self.sigma_data).contiguous()
        den = torch.empty_like(images) if return_denoised else None
        a = _lib.EdmTrainArgs()
        a.images, a.noise, a.coef_host, a.coef_stride = _lib.ptr(images), _lib.ptr(noise), _fptr(tab), COLS
        a.loss_scale, a.accumulate = float(loss_scale), int(bool(accumulate))
        a.B, a.H, a.W = b, h, w
        a.denoised_out = _lib.ptr(den)
        val = self._loss_call(a, sync)
        return (val, den) if return_denoised else val

    __call__ = forward
