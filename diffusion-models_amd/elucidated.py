"""Host-side mirror of the reference ``ElucidatedDiffusion`` (Karras et al., "Elucidating the Design Space of
Diffusion-Based Generative Models") in front of ``dm_sample_edm`` in libdm_hip.so.

Same constructor arguments, method names and ``state_dict`` keys as
  denoising-diffusion-pytorch/denoising_diffusion/elucidated_diffusion.py:22-264
for sampling -- the Heun loop (``sample``) and DPM-Solver++(2M) (``sample_using_dpmpp``) -- and for training (``forward``,
the weighted denoising loss of :228-264 with its backward pass).  The per-step and per-image scalars are computed here
the way the reference computes them -- preconditioning terms as fp32 tensor arithmetic, the churn terms as Python doubles
rounded to fp32 once -- and handed to the library as a table; the kernels hold no schedule logic.

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


def _default_seed() -> int:
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _fptr(t: torch.Tensor):
    return C.cast(t.data_ptr(), C.POINTER(C.c_float))


class ElucidatedDiffusion:
    """``ElucidatedDiffusion(net, image_size=...)`` -- drop-in for the reference class: training loss and samplers."""

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
        assert net.random_or_learned_sinusoidal_cond
        if getattr(net, "self_condition", False):
            raise NotImplementedError("ElucidatedDiffusion with a self_condition U-Net is not built on the HIP path")
        if getattr(net, "text_condition", False) or getattr(getattr(net, "cfg", None), "cond_channels", 0):
            raise NotImplementedError("ElucidatedDiffusion calls net(x, t, self_cond) only: a text-conditional or "
                                      "image-conditional U-Net has no place for its condition")
        if net.out_dim != channels or net.channels != channels:
            raise ValueError(f"the U-Net maps {net.channels} to {net.out_dim} channels, the sampler needs {channels} -> "
                             f"{channels} (no learned variance)")
        self.self_condition = net.self_condition
        self.net = net
        self.channels = channels
        self.image_size = image_size
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
        self.use_graph = use_graph
        self._lib = _lib.load()

    # -- module-ish surface ------------------------------------------------------------------------
    @property
    def device(self):
        return self.net.device

    def eval(self):
        return self

    def parameters(self):
        return self.net.parameters()

    def sample_shape(self):
        """(C, H, W) of one sample (``dist.sample_global`` builds empty shards from it)."""
        return (self.channels, self.image_size, self.image_size)

    def state_dict(self):
        """The reference module has no buffers: ``net.`` + the U-Net's keys."""
        return {"net." + k: v for k, v in self.net.state_dict().items()}

    def load_state_dict(self, state_dict, strict=True):
        other = [k for k in state_dict if not k.startswith("net.")]
        if strict and other:
            raise RuntimeError(f"Error(s) in loading state_dict: unexpected {other[:5]}")
        self.net.load_state_dict({k[len("net."):]: v for k, v in state_dict.items() if k.startswith("net.")}, strict=strict)
        return self

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
    def preconditioned_network_forward(self, noised_images, sigma, self_cond=None, clamp=False):
        """:91-110.  ``sigma``: a float or a (B,) tensor.  The scalings run in dm_op_edm_churn_in / dm_op_edm_euler, the
        network through the float-time forward."""
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
        stream = torch.cuda.current_stream(self.device).cuda_stream
        xin = torch.empty_like(x)
        _lib.check(self._lib.dm_op_edm_churn_in(_lib.ptr(x), None, _fptr(tab), rows, 0, 1, 0, None, _lib.ptr(xin), b, per,
                                                stream))
        net_out = self.net(xin, tab[:, C_NOISE].expand(b).contiguous().to(self.device))
        out = torch.empty_like(x)
        _lib.check(self._lib.dm_op_edm_euler(_lib.ptr(x), _lib.ptr(net_out), _fptr(tab), rows, int(bool(clamp)),
                                             _lib.ptr(out), None, None, None, b, per, stream))
        return out

    # -- sampling ----------------------------------------------------------------------------------
    def _randn(self, shape, seed, draw, sample_offset):
        out = torch.empty(tuple(shape), device=self.device, dtype=torch.float32)
        per = out.numel() // max(int(shape[0]), 1)
        _lib.check(self._lib.dm_randn(_lib.ptr(out), out.numel(), C.c_uint64(seed), C.c_uint64(draw),
                                      C.c_uint64(int(sample_offset) * per), torch.cuda.current_stream(self.device).cuda_stream))
        return out

    def _run(self, kind, table, sigma_init, batch_size, clamp, noise, noise_rows, seed, sample_offset):
        shape = (int(batch_size), self.channels, self.image_size, self.image_size)
        f = self.net.downsample_factor
        assert shape[0] > 0 and self.image_size % f == 0, f"shape {shape}: the sides must be divisible by {f}"
        if seed is None:
            seed = _default_seed()
        n_steps = table.shape[0]
        if noise is not None:
            x_init = noise(shape).to(self.device, torch.float32).contiguous()
            noise_dev = (torch.stack([noise(shape).to(torch.float32) for _ in range(noise_rows)], dim=0)
                         .to(self.device).contiguous() if noise_rows else None)
        else:
            x_init = self._randn(shape, seed, 0, sample_offset)
            noise_dev = None
        assert tuple(x_init.shape) == shape, "noise() must return tensors of the sampled shape"
        table = table.contiguous()
        out = torch.empty(shape, device=self.device, dtype=torch.float32)
        a = _lib.EdmArgs()
        a.kind, a.n_steps, a.table_host = kind, n_steps, _fptr(table)
        a.x_init, a.noise, a.seed, a.sample_offset = _lib.ptr(x_init), _lib.ptr(noise_dev), seed, int(sample_offset)
        a.out, a.sigma_init, a.clamp = _lib.ptr(out), float(sigma_init), int(bool(clamp))
        a.B, a.H, a.W = shape[0], shape[2], shape[3]
        a.use_graph, a.stream = 1 if self.use_graph else 0, torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._lib.dm_sample_edm(self.net._handle, C.byref(a)))
        return out

    def sample(self, batch_size=16, num_sample_steps=None, clamp=True, *, noise=None, seed=None, sample_offset=0):
        """:129-187, the stochastic Heun sampler (Algorithm 2).  The reference draws the churn noise at every step, so an
        injected ``noise`` source is called once per step whatever gamma is."""
        n = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        table = edm_heun_table(n, self.sigma_min, self.sigma_max, self.sigma_data, self.rho, self.S_churn, self.S_tmin,
                               self.S_tmax, self.S_noise)
        sigma_init = edm_sigmas(n, self.sigma_min, self.sigma_max, self.rho)[0].item()
        return self._run(_lib.EDM_HEUN, table, sigma_init, batch_size, clamp, noise, n, seed, sample_offset)

    def sample_using_dpmpp(self, batch_size=16, num_sample_steps=None, *, noise=None, seed=None, sample_offset=0):
        """:189-224, DPM-Solver++(2M): one network evaluation per step, one draw (the start image)."""
        n = self.num_sample_steps if num_sample_steps is None else num_sample_steps
        table = edm_dpmpp_table(n, self.sigma_min, self.sigma_max, self.sigma_data, self.rho)
        sigma_init = edm_sigmas(n, self.sigma_min, self.sigma_max, self.rho)[0].item()
        return self._run(_lib.EDM_DPMPP, table, sigma_init, batch_size, False, noise, 0, seed, sample_offset)

    # -- training ----------------------------------------------------------------------------------
    def _trainable_net(self):
        """The library ``Unet`` behind ``net``; anything else (no handle, or a library without the float-time training
        entry) cannot be trained.  Touches neither a tensor nor the device."""
        from .unet import Unet

        net = self.net
        if not isinstance(net, Unet) or getattr(net, "_handle", None) is None or not hasattr(self._lib, "dm_unet_loss_backward_edm"):
            raise NotImplementedError("ElucidatedDiffusion can train a library Unet only (dm_unet_train_enable_ft arms its "
                                      f"handle for the float-time training loss); got {type(net).__name__}")
        return net

    def train(self, mode: bool = True):
        """``model.train()``: arm the U-Net for float-time training (gradient buffers, input-gradient convolutions; once)."""
        if mode:
            net = self._trainable_net()
            if not net._loaded:
                raise RuntimeError("load_state_dict() must be called before train()")
            # random_fourier_features: the reference builds time_mlp.0.weights with requires_grad = False
            _lib.check(self._lib.dm_unet_train_enable_ft(net._handle, int(bool(net.cfg.random_fourier_features))))
            if not getattr(net, "_training", False):
                net.set_dropout_seed(int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item()))
            net._training = True
        return self

    def forward(self, images, *, sigmas=None, noise=None, loss_scale=1.0, accumulate=False, sync=True,
                return_denoised=False):
        """:234-264: the loss (0-dim CPU tensor; ``sync=False``: a 0-dim device tensor, nothing waited for); the parameter
        gradients stay on the U-Net (``self.net.grad(name)`` / ``.grads()``).  ``images`` in [0, 1]."""
        net = self._trainable_net()
        b, c, h, w = images.shape
        assert h == self.image_size and w == self.image_size, f"height and width of image must be {self.image_size}"
        assert c == self.channels, "mismatch of image channels"
        if not getattr(net, "_training", False):
            self.train()
        # the reference's order of draws: sigma (:242), then the noise (:245)
        sig = self._draw_sigmas(b) if sigmas is None else sigmas.detach().to("cpu", torch.float32).reshape(-1)
        if sig.numel() != b:
            raise RuntimeError(f"sigmas has {sig.numel()} entries for a batch of {b}")
        images = images.to(self.device, torch.float32).contiguous()
        noise = (noise.to(self.device, torch.float32).contiguous() if noise is not None
                 else self._randn(images.shape, _default_seed(), 0, 0))
        if noise.shape != images.shape:
            raise RuntimeError(f"noise {tuple(noise.shape)} does not match images {tuple(images.shape)}")
        tab = edm_train_table(sig, self.sigma_data).contiguous()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        loss = C.c_float(0.0)
        den = torch.empty_like(images) if return_denoised else None
        a = _lib.EdmTrainArgs()
        a.images, a.noise, a.coef_host, a.coef_stride = _lib.ptr(images), _lib.ptr(noise), _fptr(tab), COLS
        a.loss_scale, a.accumulate = float(loss_scale), int(bool(accumulate))
        a.B, a.H, a.W = b, h, w
        a.loss_out_host = C.pointer(loss) if sync else None
        a.denoised_out, a.stream = _lib.ptr(den), stream
        _lib.check(self._lib.dm_unet_loss_backward_edm(net._handle, C.byref(a)))
        if sync:
            val = torch.tensor(loss.value, dtype=torch.float32)
        else:
            val = torch.empty((), device=self.device, dtype=torch.float32)
            _lib.check(self._lib.dm_unet_train_scalar(net._handle, 0, _lib.ptr(val), stream))
        return (val, den) if return_denoised else val

    __call__ = forward
