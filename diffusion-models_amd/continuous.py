"""Host-side mirrors of the reference's two continuous-time classes in front of ``dm_sample_ct`` /
``dm_unet_loss_backward_ct`` in libdm_hip.so:

  ``ContinuousTimeGaussianDiffusion``        denoising-diffusion-pytorch/denoising_diffusion/continuous_time_gaussian_diffusion.py:97-259
  ``VParamContinuousTimeGaussianDiffusion``  denoising-diffusion-pytorch/denoising_diffusion/v_param_continuous_time_gaussian_diffusion.py:32-170

Same constructor arguments, method names and ``state_dict`` keys.  The U-Net's time is ``log_snr(t)``, a float, so both
need the learned / random sinusoidal U-Net (the reference asserts it).  ``num_sample_steps`` is a sampling-time choice: no
table is tied to training.

The per-step and per-image scalars are computed HERE, as the same fp32 torch expressions in the same order as the
reference (0-dim tensors for a sampling step, (B,) tensors for a training batch), and handed to the library as a table;
the kernels hold no schedule logic.  This is deliberate: the cosine schedule's own samples move by 4e-3 .. 2e-2 (rel-L2)
when the same expressions are evaluated in fp64 -- at t = 1, ``cos(pi / 2) ** -2`` makes log-SNR ~ -33.9 a pure fp32
rounding artefact -- so parity is with the reference's fp32 scalars, never with a cleaner formula.

``noise_schedule='learned'`` (``learned_noise_schedule``: a monotonic MLP t -> log-SNR trained with the U-Net) keeps its six
parameters on the host as a torch module, where B scalars through 1 -> 1 and 1 -> H -> 1 cost nothing.  Its gradient needs
the loss differentiated with respect to the U-Net's INPUTS, which ``dm_unet_loss_backward_ct_ig`` returns reduced per image:
``ga_b = sum dL/dx x0``, ``gs_b = sum dL/dx eps``, ``dt_b = dL/dtime_b`` and the unweighted ``l_b``.  With ``lambda =
log_snr(times)`` under autograd and alpha, sigma, w the reference's expressions of it, the host back-propagates the surrogate

    sum_b (ga_b alpha_b + gs_b sigma_b + dt_b lambda_b) + loss_scale * mean_b(l_b w_b)

whose gradient is the loss's: x = alpha x0 + sigma eps gives dL/dalpha_b = ga_b and dL/dsigma_b = gs_b, the U-Net's time
is lambda_b itself, and the loss weight multiplies l_b.  Every chain-rule factor (sqrt . sigmoid, clamp, the normalisation by
net(0) / net(1), frac_gradient) is then torch's own.  ``p_losses_input_grads`` / ``forward_input_grads`` return dL/dx and
dL/dtime next to the loss, for any schedule.

Extensions (keyword-only): ``noise`` injects a source of N(0,1) draws called in the reference's order (the start image,
then one draw per step except the last); ``seed`` / ``sample_offset`` select the device Philox stream and the index of the
call's first sample in a global batch.  ``dpm_solver_sample`` / ``sample(solver='dpmpp')`` is DPM-Solver++ (2M) in front of
``dm_sample_ct_dpmpp``: the solver's lambda is ``log_snr / 2``, so its nodes are log-SNR values the U-Net is fed as they
are, uniform in log-SNR by default (``ct_dpmpp_nodes``); its coefficients are float64 on those fp32 nodes, rounded once
(``ct_dpmpp_table``) -- there is no reference expression to follow.  Training: ``train()`` arms the U-Net through ``dm_unet_train_enable_ft``;
``p_losses`` / ``forward`` are one ``dm_unet_loss_backward_ct`` call -- loss and every parameter gradient; ``times`` /
``noise`` inject the two draws, ``loss_scale`` / ``accumulate`` / ``sync`` are as on ``ElucidatedDiffusion.forward``.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import sqrt
from torch.special import expm1

from . import _lib, _loop
from ._floattime import FloatTimeDiffusion
from ._lib import default_seed as _default_seed, fptr as _fptr

from torch import nn
import torch.nn.functional as F

COLS = _lib.DM_CT_COEFS
# columns of a table row (csrc/ct.h)
LOG_SNR, ALPHA, SIGMA, ALPHA_NEXT, C_, ONE_M_C, SQRT_VAR, AN_OVER_A, C_SIGMA, LOSS_W = range(10)
DPM_CX, DPM_CD, DPM_G = 10, 11, 12  # rows of ct_dpmpp_table only
SPACINGS = ("logsnr", "time")


def _log(t, eps=1e-20):
    return torch.log(t.clamp(min=eps))


def beta_linear_log_snr(t):
    """log(snr) that approximates the original linear schedule (continuous_time_gaussian_diffusion.py:51-52)."""
    return -_log(expm1(1e-4 + 10 * (t ** 2)))


def alpha_cosine_log_snr(t, s=0.008):
    """:54-55 (and the v class, :29-30)."""
    return -_log((torch.cos((t + s) / (1 + s) * math.pi * 0.5) ** -2) - 1, eps=1e-5)


SCHEDULES = {"linear": beta_linear_log_snr, "cosine": alpha_cosine_log_snr}


class MonotonicLinear(nn.Module):
    """:33-39: a Linear whose weight and bias enter as absolute values."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.net = nn.Linear(*args, **kwargs)

    def forward(self, x):
        return F.linear(x, self.net.weight.abs(), self.net.bias.abs())


class _Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return x + self.fn(x)


class _LastDim(nn.Module):
    """'... -> ... 1' (add) and '... 1 -> ...' (drop): the two Rearrange layers of the reference's net; they hold no
    parameter and keep the Sequential's indices, hence the state_dict keys net.1 / net.2."""

    def __init__(self, add):
        super().__init__()
        self.add = add

    def forward(self, x):
        return x.unsqueeze(-1) if self.add else x.squeeze(-1)


class learned_noise_schedule(nn.Module):
    """:57-95 (sections H and I.2 of the Variational Diffusion Models supplement): a monotonic t -> log-SNR net, normalised
    so that t = 0 / 1 map to log_snr_max / log_snr_min; ``frac_gradient`` of the gradient goes back.  A CPU module: same
    construction order as the reference, so the same seed gives the same initialisation."""

    def __init__(self, *, log_snr_max, log_snr_min, hidden_dim=1024, frac_gradient=1.):
        super().__init__()
        self.slope = log_snr_min - log_snr_max
        self.intercept = log_snr_max
        self.net = nn.Sequential(
            _LastDim(True),
            MonotonicLinear(1, 1),
            _Residual(nn.Sequential(MonotonicLinear(1, hidden_dim), nn.Sigmoid(), MonotonicLinear(hidden_dim, 1))),
            _LastDim(False),
        )
        self.frac_gradient = frac_gradient

    def forward(self, x):
        frac_gradient = self.frac_gradient
        out_zero = self.net(torch.zeros_like(x))
        out_one = self.net(torch.ones_like(x))
        x = self.net(x)
        normed = self.slope * ((x - out_zero) / (out_one - out_zero)) + self.intercept
        return normed * frac_gradient + normed.detach() * (1 - frac_gradient)


class _NoGrad:
    """A schedule module as the plain function of t the step tables take."""

    def __init__(self, module):
        self.module = module

    def __call__(self, t):
        with torch.no_grad():
            return self.module(t)


def _schedule(schedule):
    if isinstance(schedule, nn.Module):
        return _NoGrad(schedule)
    if callable(schedule):
        return schedule
    if schedule == "learned":
        raise ValueError("noise_schedule='learned' names a module the diffusion object owns: pass that module "
                         "(ContinuousTimeGaussianDiffusion(...).log_snr)")
    if schedule not in SCHEDULES:
        raise ValueError(f"unknown noise schedule {schedule}")
    return SCHEDULES[schedule]


def ct_step_row(schedule, time: torch.Tensor, time_next: torch.Tensor) -> torch.Tensor:
    """One DM_CT_COEFS row of ``p_mean_variance`` (:155-183) + ``p_sample`` (:188-197) for 0-dim fp32 ``time`` /
    ``time_next``: every entry is the reference's own 0-dim tensor expression."""
    f = _schedule(schedule)
    log_snr = f(time)
    log_snr_next = f(time_next)
    c = -expm1(log_snr - log_snr_next)
    squared_alpha, squared_alpha_next = log_snr.sigmoid(), log_snr_next.sigmoid()
    squared_sigma, squared_sigma_next = (-log_snr).sigmoid(), (-log_snr_next).sigmoid()
    alpha, sigma, alpha_next = map(sqrt, (squared_alpha, squared_sigma, squared_alpha_next))
    posterior_variance = squared_sigma_next * c
    row = torch.zeros(COLS, dtype=torch.float32)
    row[LOG_SNR], row[ALPHA], row[SIGMA], row[ALPHA_NEXT] = log_snr, alpha, sigma, alpha_next
    row[C_], row[ONE_M_C] = c, 1 - c
    row[SQRT_VAR] = 0.0 if time_next == 0 else sqrt(posterior_variance)  # p_sample returns the mean when time_next == 0
    row[AN_OVER_A], row[C_SIGMA] = alpha_next / alpha, c * sigma
    return row


def ct_step_table(num_sample_steps, schedule="linear") -> torch.Tensor:
    """(N, DM_CT_COEFS) fp32 step table of ``p_sample_loop`` (:200-213): ``steps = linspace(1, 0, N + 1)``, row i from
    the 0-dim ``steps[i]`` / ``steps[i + 1]``; the layout is documented in include/dm_hip.h."""
    n = int(num_sample_steps)
    steps = torch.linspace(1., 0., n + 1)
    return torch.stack([ct_step_row(schedule, steps[i], steps[i + 1]) for i in range(n)])


def ct_dpmpp_nodes(num_sample_steps, schedule="linear", spacing="logsnr", log_snr_min=None) -> torch.Tensor:
    """The N + 1 fp32 log-SNR nodes ``l_0 < ... < l_N`` of the DPM-Solver++ loop; the U-Net is fed ``l_i`` itself.

    ``spacing='logsnr'``: uniform in log-SNR (so in the solver's lambda = log_snr / 2) between the schedule's own fp32
    ``log_snr(1.)`` and ``log_snr(0.)``, which the end nodes equal exactly; ``log_snr_min`` raises the first node to
    ``max(log_snr(1.), log_snr_min)`` (the cosine schedule's ~ -33.9 is an fp32 rounding artefact: a floor of -12 .. -20
    spends the steps where the signal is).  ``spacing='time'``: ``log_snr(linspace(1, 0, N + 1)[i])``, the nodes of
    ``p_sample_loop`` -- kept for comparison; its lambda steps at both ends are many times their neighbours, which makes
    the second-order method worse than the first up to about 40 steps (DESIGN, the grid table)."""
    n = num_sample_steps
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"num_sample_steps must be a positive integer, got {n!r}")
    if spacing not in SPACINGS:
        raise ValueError(f"unknown spacing {spacing!r}: one of {SPACINGS}")
    f = _schedule(schedule)
    if spacing == "time":
        steps = torch.linspace(1., 0., n + 1)
        nodes = torch.stack([f(steps[i]).reshape(()) for i in range(n + 1)]).to(torch.float32)
        if log_snr_min is not None:
            raise ValueError("log_snr_min belongs to spacing='logsnr': the time grid starts at log_snr(1.)")
    else:
        first, last = (f(torch.tensor(t)).to(torch.float32).reshape(()) for t in (1., 0.))
        if log_snr_min is not None:
            first = torch.maximum(first, torch.tensor(float(log_snr_min), dtype=torch.float32))
        nodes = torch.linspace(float(first), float(last), n + 1, dtype=torch.float64).to(torch.float32)
        nodes[0], nodes[-1] = first, last
    if not bool((nodes[1:] > nodes[:-1]).all()):
        raise ValueError(f"the log-SNR nodes must increase strictly from {float(nodes[0])} to {float(nodes[-1])}"
                         + (f" (log_snr_min = {log_snr_min})" if log_snr_min is not None else ""))
    return nodes


def ct_dpmpp_rows(nodes: torch.Tensor, order=2) -> torch.Tensor:
    """(N, DM_CT_COEFS) float64 rows of DPM-Solver++ (2M; arXiv 2211.01095, Algorithm 2) on N + 1 log-SNR nodes, with
    lambda = l / 2, alpha = sqrt(sigmoid(l)), sigma = sqrt(sigmoid(-l)), h_i = lambda_{i+1} - lambda_i:
    ``c_x = sigma_{i+1} / sigma_i``, ``c_D = -alpha_{i+1} expm1(-h_i)``, ``g = h_i / (2 h_{i-1})`` (0 on row 0 and at
    order 1), so that ``c_D + c_x alpha_i = alpha_{i+1}`` and ``c_x sigma_i = sigma_{i+1}``."""
    if isinstance(order, bool) or not isinstance(order, int) or order not in (1, 2):
        raise ValueError(f"order must be 1 or 2, got {order!r}")
    l = nodes.detach().to("cpu", torch.float64).reshape(-1)
    alpha, sigma = sqrt(l.sigmoid()), sqrt((-l).sigmoid())
    h = (l[1:] - l[:-1]) / 2
    rows = torch.zeros((l.numel() - 1, COLS), dtype=torch.float64)
    rows[:, LOG_SNR], rows[:, ALPHA], rows[:, SIGMA] = l[:-1], alpha[:-1], sigma[:-1]
    rows[:, DPM_CX] = sigma[1:] / sigma[:-1]
    rows[:, DPM_CD] = -alpha[1:] * expm1(-h)
    if order == 2:
        rows[1:, DPM_G] = h[1:] / (2 * h[:-1])
    return rows


def ct_dpmpp_table(num_sample_steps, schedule="linear", order=2, spacing="logsnr", log_snr_min=None) -> torch.Tensor:
    """(N, DM_CT_COEFS) fp32 step table of ``dpm_solver_sample`` (``dm_sample_ct_dpmpp``): the nodes of
    ``ct_dpmpp_nodes``, every coefficient evaluated in float64 on them (``ct_dpmpp_rows``) and rounded to fp32 once;
    the layout is documented in include/dm_hip.h."""
    return ct_dpmpp_rows(ct_dpmpp_nodes(num_sample_steps, schedule, spacing, log_snr_min), order).to(torch.float32)


def ct_train_table(times: torch.Tensor, schedule="linear", min_snr_loss_weight=False, min_snr_gamma=5) -> torch.Tensor:
    """(B, DM_CT_COEFS) fp32 rows of ``q_sample`` / ``p_losses`` (:222-251), one per image: log_snr, alpha, sigma as
    tensor expressions on the (B,) ``times``; column 9 the loss weight (1, or ``snr.clamp(min = gamma) / snr``)."""
    f = _schedule(schedule)
    t = times.detach().to("cpu", torch.float32).reshape(-1)
    log_snr = f(t)
    tab = torch.zeros((t.numel(), COLS), dtype=torch.float32)
    tab[:, LOG_SNR] = log_snr
    tab[:, ALPHA], tab[:, SIGMA] = sqrt(log_snr.sigmoid()), sqrt((-log_snr).sigmoid())
    if min_snr_loss_weight:
        snr = log_snr.exp()
        tab[:, LOSS_W] = snr.clamp(min=min_snr_gamma) / snr
    else:
        tab[:, LOSS_W] = 1.0
    return tab


def learned_train_terms(sched, times, min_snr_loss_weight=False, min_snr_gamma=5):
    """(lambda, alpha, sigma, w) of ``q_sample`` / ``p_losses`` (:225-228, :247-248) for a schedule MODULE, as (B,) fp32
    tensor expressions of ``lambda = sched(times)`` that carry its autograd graph, and the (B, DM_CT_COEFS) table of their
    values the library reads."""
    t = torch.as_tensor(times).detach().to("cpu", torch.float32).reshape(-1)
    lam = sched(t)
    alpha, sigma = sqrt(lam.sigmoid()), sqrt((-lam).sigmoid())
    if min_snr_loss_weight:
        snr = lam.exp()
        weight = snr.clamp(min=min_snr_gamma) / snr
    else:
        weight = torch.ones_like(lam)
    tab = torch.zeros((t.numel(), COLS), dtype=torch.float32)
    tab[:, LOG_SNR], tab[:, ALPHA], tab[:, SIGMA], tab[:, LOSS_W] = lam.detach(), alpha.detach(), sigma.detach(), weight.detach()
    return (lam, alpha, sigma, weight), tab


def schedule_surrogate(terms, rows, loss_scale=1.0):
    """The scalar whose gradient with respect to the schedule's parameters is the loss's: ``terms`` from
    ``learned_train_terms``, ``rows`` the (B, 4) [ga, gs, dt, l] of ``dm_unet_loss_backward_ct_ig`` (constants here)."""
    lam, alpha, sigma, weight = terms
    ga, gs, dt, l = rows.detach().to(lam.dtype).unbind(dim=1)
    return (ga * alpha + gs * sigma + dt * lam).sum() + float(loss_scale) * (l * weight).mean()


class _ContinuousTimeBase(FloatTimeDiffusion):
    """What the two classes share; ``_objective`` and the schedule tell them apart."""

    _unet_attr = "model"
    _train_entry = "dm_unet_loss_backward_ct"
    _objective = _lib.CT_PRED_NOISE
    min_snr_loss_weight = False
    min_snr_gamma = 5

    def _init(self, model, image_size, channels, schedule, num_sample_steps, clip_sample_denoised, use_graph):
        self._init_unet(model, image_size, channels, use_graph, f"{type(self).__name__} calls model(x, log_snr) only")
        self.log_snr = _schedule(schedule) if not isinstance(schedule, nn.Module) else schedule
        self.num_sample_steps = num_sample_steps
        self.clip_sample_denoised = clip_sample_denoised

    @staticmethod
    def _refuse_self_condition(model):
        assert not model.self_condition, 'not supported yet'

    # -- sampling ----------------------------------------------------------------------------------
    def _step_op(self, x, row, eps, want_x_start=False):
        """``dm_op_ct_step`` on one table row: the U-Net at log_snr, then the elementwise step."""
        x = x.to(self.device, torch.float32).contiguous()
        b, per = x.shape[0], x[0].numel()
        row = row.reshape(1, COLS).contiguous()
        F = self.model(x, row[0, LOG_SNR].expand(b).contiguous().to(self.device))
        out = torch.empty_like(x)
        x_start = torch.empty_like(x) if want_x_start else None
        if eps is not None:
            eps = eps.to(self.device, torch.float32).contiguous()
            assert eps.shape == x.shape, "noise must have the shape of x"
        _lib.check(self._lib.dm_op_ct_step(_lib.ptr(x), _lib.ptr(F), _lib.ptr(eps), _fptr(row), 1, self._objective,
                                           int(bool(self.clip_sample_denoised)), 0, 1, 0, _lib.ptr(out), _lib.ptr(x_start),
                                           b, per, self._stream()))
        return out, x_start

    @staticmethod
    def _t0(v):
        return torch.as_tensor(v, dtype=torch.float32).detach().cpu().reshape(())

    def p_mean_variance(self, x, time, time_next):
        """:155-183: (model_mean, posterior_variance) for 0-dim ``time`` / ``time_next``."""
        time, time_next = self._t0(time), self._t0(time_next)
        row = ct_step_row(self.log_snr, time, time_next)
        row[SQRT_VAR] = 0.0
        mean, _ = self._step_op(x, row, None)
        f = _schedule(self.log_snr)
        log_snr, log_snr_next = f(time), f(time_next)
        return mean, ((-log_snr_next).sigmoid() * -expm1(log_snr - log_snr_next)).to(self.device)

    def p_sample(self, x, time, time_next, *, noise=None):
        """:188-197.  ``noise``: the step's N(0,1) tensor (default: a device Philox draw); unused when time_next == 0."""
        time, time_next = self._t0(time), self._t0(time_next)
        row = ct_step_row(self.log_snr, time, time_next)
        if float(row[SQRT_VAR]) != 0.0 and noise is None:
            noise = self._randn(x.shape, _default_seed(), 0, 0)
        return self._step_op(x, row, noise if float(row[SQRT_VAR]) != 0.0 else None)[0]

    def p_sample_loop(self, shape, *, noise=None, seed=None, sample_offset=0):
        """:200-213.  An injected ``noise`` callable is called once for the start image and once per step except the
        last, the reference's order of draws."""
        shape = tuple(int(v) for v in shape)
        f = self.model.downsample_factor
        assert shape[0] > 0 and shape[2] % f == 0 and shape[3] % f == 0, f"shape {shape}: the sides must be divisible by {f}"
        table = ct_step_table(self.num_sample_steps, self.log_snr).contiguous()
        n_steps = table.shape[0]
        # (a one-step loop draws nothing after the start image: its only row has c[6] == 0)
        seed, x_init, noise_dev = self._start(shape, noise, n_steps - 1, seed, sample_offset)
        out = torch.empty(shape, device=self.device, dtype=torch.float32)
        a = _lib.CtArgs()
        a.objective, a.clip, a.n_steps, a.table_host = self._objective, int(bool(self.clip_sample_denoised)), n_steps, _fptr(table)
        a.x_init, a.noise, a.seed, a.sample_offset = _lib.ptr(x_init), _lib.ptr(noise_dev), seed, int(sample_offset)
        a.out = _lib.ptr(out)
        a.B, a.H, a.W = shape[0], shape[2], shape[3]
        a.use_graph, a.stream = 1 if self.use_graph else 0, self._stream()
        _lib.check(self._lib.dm_sample_ct(self.model._handle, C.byref(a)))
        return out

    def dpm_solver_sample(self, shape, num_sample_steps=20, order=2, *, spacing='logsnr', log_snr_min=None, noise=None,
                          seed=None, sample_offset=0, unnormalize=True):
        """An extension: DPM-Solver++ (2M; ``order=1``: DDIM at eta = 0) on ``num_sample_steps`` U-Net evaluations, one
        ``dm_sample_ct_dpmpp`` call over ``ct_dpmpp_table`` (grid: ``ct_dpmpp_nodes``).  Deterministic after the start
        image, which ``noise`` / ``seed`` / ``sample_offset`` choose exactly as in ``p_sample_loop`` (an injected
        ``noise`` is called once).  ``unnormalize=False`` returns the final iterate as it is: no clamp, no map to [0, 1]."""
        shape = tuple(int(v) for v in shape)
        f = self.model.downsample_factor
        assert shape[0] > 0 and shape[2] % f == 0 and shape[3] % f == 0, f"shape {shape}: the sides must be divisible by {f}"
        table = ct_dpmpp_table(num_sample_steps, self.log_snr, order, spacing, log_snr_min).contiguous()
        _, x_init, _ = self._start(shape, noise, 0, seed, sample_offset)
        out = torch.empty(shape, device=self.device, dtype=torch.float32)
        x_out = None if unnormalize else torch.empty_like(out)
        a = _lib.CtDpmppArgs()
        a.objective, a.clip = self._objective, int(bool(self.clip_sample_denoised))
        a.n_steps, a.table_host = table.shape[0], _fptr(table)
        a.x_init, a.out, a.x_out = _lib.ptr(x_init), _lib.ptr(out), _lib.ptr(x_out)
        a.B, a.H, a.W = shape[0], shape[2], shape[3]
        a.use_graph, a.stream = 1 if self.use_graph else 0, self._stream()
        _lib.check(self._lib.dm_sample_ct_dpmpp(self.model._handle, C.byref(a)))
        return out if unnormalize else x_out

    def sample(self, batch_size=16, *, solver=None, order=2, num_sample_steps=None, spacing='logsnr', log_snr_min=None,
               noise=None, seed=None, sample_offset=0):
        """:216-217.  ``solver='dpmpp'`` (an extension) samples with ``dpm_solver_sample`` at ``order`` on
        ``num_sample_steps`` steps -- 20 unless given, never the constructor's 500, which is the ancestral loop's."""
        shape = (batch_size, self.channels, self.image_size, self.image_size)
        if solver == "dpmpp":
            return self.dpm_solver_sample(shape, 20 if num_sample_steps is None else num_sample_steps, order, spacing=spacing,
                                          log_snr_min=log_snr_min, noise=noise, seed=seed, sample_offset=sample_offset)
        if solver is not None:
            raise ValueError(f"unknown solver {solver!r}: None (the ancestral p_sample_loop) or 'dpmpp'")
        if num_sample_steps is not None:
            raise ValueError("num_sample_steps= belongs to solver='dpmpp': p_sample_loop runs the object's num_sample_steps")
        return self.p_sample_loop(shape, noise=noise, seed=seed, sample_offset=sample_offset)

    # -- training ----------------------------------------------------------------------------------
    def _q_sample(self, x_start, times, noise):
        x_start = x_start.to(self.device, torch.float32).contiguous()
        noise = (noise.to(self.device, torch.float32).contiguous() if noise is not None
                 else self._randn(x_start.shape, _default_seed(), 0, 0))
        tab = ct_train_table(times, self.log_snr)
        b = x_start.shape[0]
        if tab.shape[0] != b:
            raise RuntimeError(f"times has {tab.shape[0]} entries for a batch of {b}")
        coef = tab[:, [ALPHA, SIGMA]].contiguous()
        out = torch.empty_like(x_start)
        _lib.check(self._lib.dm_op_lincomb(_lib.ptr(x_start), _lib.ptr(noise), _fptr(coef), _lib.ptr(out), b,
                                           x_start[0].numel(), 0, 0, self._stream()))
        pad = (b,) + (1,) * (x_start.dim() - 1)
        return out, tab[:, LOG_SNR].to(self.device), tab[:, ALPHA].reshape(pad).to(self.device), tab[:, SIGMA].reshape(pad).to(self.device)

    def _draw_times(self, batch_size):
        return torch.zeros((batch_size,)).float().uniform_(0, 1)

    def random_times(self, batch_size):
        """:233-235: uniform on [0, 1); the (batch_size,) draw comes from torch's global CPU generator."""
        return self._draw_times(batch_size).to(self.device)

    @property
    def learned_schedule(self):
        """The schedule module when the schedule is trained, else None."""
        return self.log_snr if isinstance(self.log_snr, nn.Module) else None

    def _loss(self, images, times, noise, normalize, loss_scale, accumulate, sync, return_input_grads=False):
        model = self._trainable()
        b, c, h, w = images.shape
        assert c == self.channels, "mismatch of image channels"
        sched = self.learned_schedule
        if sched is not None and not sync:
            raise ValueError("sync=False cannot serve a learned noise schedule: the per-image gradient rows have to come back "
                             "to the host before its backward pass")
        if not getattr(model, "_training", False):
            self.train()
        if sched is None:
            tab = ct_train_table(times, self.log_snr, self.min_snr_loss_weight, self.min_snr_gamma).contiguous()
        else:
            terms, tab = learned_train_terms(sched, times, self.min_snr_loss_weight, self.min_snr_gamma)
        if tab.shape[0] != b:
            raise RuntimeError(f"times has {tab.shape[0]} entries for a batch of {b}")
        images, noise = self._loss_inputs(images, noise)
        ig = sched is not None or return_input_grads
        a = _lib.CtTrainIgArgs() if ig else _lib.CtTrainArgs()
        a.images, a.noise, a.coef_host, a.coef_stride = _lib.ptr(images), _lib.ptr(noise), _fptr(tab), COLS
        a.objective, a.loss_scale, a.accumulate = self._objective, float(loss_scale), int(bool(accumulate))
        a.B, a.H, a.W, a.normalize = b, h, w, int(bool(normalize))
        if not ig:
            return self._loss_call(a, sync)
        if not hasattr(self._lib, "dm_unet_loss_backward_ct_ig"):
            raise NotImplementedError("this libdm_hip.so has no input-gradient entry (dm_unet_loss_backward_ct_ig)")
        rows = torch.zeros((b, 4), dtype=torch.float32) if sched is not None else None
        dx = torch.empty_like(images) if return_input_grads else None
        dtime = torch.empty((b,), device=self.device, dtype=torch.float32) if return_input_grads else None
        a.sched_out_host = _fptr(rows) if rows is not None else None
        a.dx_out, a.dtime_out = _lib.ptr(dx), _lib.ptr(dtime)
        loss = _loop.loss_call(self, model._handle, self._lib.dm_unet_loss_backward_ct_ig, a, sync)
        if sched is not None:
            if not accumulate:
                for p in sched.parameters():
                    p.grad = None
            schedule_surrogate(terms, rows, loss_scale).backward()
        return (loss, dx, dtime) if return_input_grads else loss

    def p_losses(self, x_start, times, noise=None, *, loss_scale=1.0, accumulate=False, sync=True):
        """:237-251 (v: :152-162) on ``x_start`` in [-1, 1]: the loss (0-dim CPU tensor; ``sync=False``: a 0-dim device
        tensor, nothing waited for); the parameter gradients stay on the U-Net (``self.model.grad(name)`` / ``.grads()``),
        those of a learned schedule land in ``.grad`` of its six host parameters (``accumulate=False`` clears them first)."""
        return self._loss(x_start, times, noise, False, loss_scale, accumulate, sync)

    def forward(self, img, *, times=None, noise=None, loss_scale=1.0, accumulate=False, sync=True):
        """:253-259 on ``img`` in [0, 1]: the draw of ``times`` comes first, as in the reference, then the noise."""
        self._trainable()
        b, c, h, w = img.shape
        assert h == self.image_size and w == self.image_size, f'height and width of image must be {self.image_size}'
        times = self._draw_times(b) if times is None else times
        return self._loss(img, times, noise, True, loss_scale, accumulate, sync)

    def p_losses_input_grads(self, x_start, times, noise=None, *, loss_scale=1.0, accumulate=False):
        """``p_losses`` on the same arguments, returning ``(loss, dL/dx, dL/dtime)``: the last two are device tensors
        (B, C, H, W) and (B,), the gradient with respect to the noised image and to the log-SNR the U-Net was called with
        (any schedule, both classes).  Loss and parameter gradients are those of ``p_losses``."""
        return self._loss(x_start, times, noise, False, loss_scale, accumulate, True, return_input_grads=True)

    def forward_input_grads(self, img, *, times=None, noise=None, loss_scale=1.0, accumulate=False):
        """``forward`` returning ``(loss, dL/dx, dL/dtime)`` as ``p_losses_input_grads`` does."""
        self._trainable()
        b, c, h, w = img.shape
        assert h == self.image_size and w == self.image_size, f'height and width of image must be {self.image_size}'
        times = self._draw_times(b) if times is None else times
        return self._loss(img, times, noise, True, loss_scale, accumulate, True, return_input_grads=True)

    def _schedule_optimizer(self, lr, betas, eps):
        """The ``torch.optim.Adam`` over the six host parameters of a learned schedule (made on first use), set to the
        call's hyper-parameters: ``train_step`` steps it beside the library's Adam, the checkpoints carry its state."""
        opt = self.__dict__.get("_sched_opt")
        if opt is None:
            opt = self._sched_opt = torch.optim.Adam(list(self.learned_schedule.parameters()), lr=lr, betas=tuple(betas), eps=eps)
        g = opt.param_groups[0]
        g["lr"], g["betas"], g["eps"] = lr, tuple(betas), eps
        return opt

    # -- module-ish surface with a trained schedule: the U-Net's parameters, then the six (the reference's registration order)
    def parameters(self):
        yield from self._unet.parameters()
        if self.learned_schedule is not None:
            yield from self.learned_schedule.parameters()

    def state_dict(self):
        sd = super().state_dict()
        if self.learned_schedule is not None:
            sd.update({f"log_snr.{k}": v.detach().clone() for k, v in self.learned_schedule.state_dict().items()})
        return sd

    def load_state_dict(self, state_dict, strict=True):
        sched = self.learned_schedule
        own = {k[len("log_snr."):]: v for k, v in state_dict.items() if k.startswith("log_snr.")}
        if sched is None:
            return super().load_state_dict(state_dict, strict=strict)  # log_snr.* keys are unexpected there
        super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("log_snr.")}, strict=strict)
        sched.load_state_dict(own, strict=strict)
        return self

    __call__ = forward


class ContinuousTimeGaussianDiffusion(_ContinuousTimeBase):
    """``ContinuousTimeGaussianDiffusion(model, image_size=...)`` -- drop-in for the reference class (noise prediction,
    linear or cosine log-SNR schedule, optional min-SNR loss weight)."""

    _objective = _lib.CT_PRED_NOISE

    def __init__(
        self,
        model,
        *,
        image_size,
        channels=3,
        noise_schedule='linear',
        num_sample_steps=500,
        clip_sample_denoised=True,
        learned_schedule_net_hidden_dim=1024,
        learned_noise_schedule_frac_gradient=1.,
        min_snr_loss_weight=False,
        min_snr_gamma=5,
        use_graph=True,
    ):
        if not isinstance(noise_schedule, str):
            raise ValueError(f'unknown noise schedule {noise_schedule}')
        if noise_schedule == 'learned':
            self._unet_for_learned(model)
            log_snr_max, log_snr_min = [beta_linear_log_snr(torch.tensor([time])).item() for time in (0., 1.)]
            noise_schedule = learned_noise_schedule(log_snr_max=log_snr_max, log_snr_min=log_snr_min,
                                                    hidden_dim=learned_schedule_net_hidden_dim,
                                                    frac_gradient=learned_noise_schedule_frac_gradient)
        self._init(model, image_size, channels, noise_schedule, num_sample_steps, clip_sample_denoised, use_graph)
        self.min_snr_loss_weight = min_snr_loss_weight
        self.min_snr_gamma = min_snr_gamma

    @staticmethod
    def _unet_for_learned(model):
        """The learned schedule trains through the library's input-gradient entry: what ``_trainable()`` would refuse is
        refused at construction."""
        from .unet import Unet

        if not isinstance(model, Unet) or getattr(model, "_handle", None) is None:
            raise NotImplementedError("noise_schedule='learned': the learned noise schedule needs the library's input-gradient "
                                      "entry (dm_unet_loss_backward_ct_ig), hence a library Unet with a handle; got "
                                      f"{type(model).__name__}")

    def q_sample(self, x_start, times, noise=None):
        """:222-231: (x_noised, log_snr)."""
        return self._q_sample(x_start, times, noise)[:2]


class VParamContinuousTimeGaussianDiffusion(_ContinuousTimeBase):
    """``VParamContinuousTimeGaussianDiffusion(model, image_size=...)`` -- drop-in for the reference class (v prediction,
    cosine log-SNR schedule)."""

    _objective = _lib.CT_PRED_V

    def __init__(
        self,
        model,
        *,
        image_size,
        channels=3,
        num_sample_steps=500,
        clip_sample_denoised=True,
        use_graph=True,
    ):
        self._init(model, image_size, channels, "cosine", num_sample_steps, clip_sample_denoised, use_graph)

    def q_sample(self, x_start, times, noise=None):
        """:138-147: (x_noised, log_snr, alpha, sigma), the last two padded to ``x_start``'s rank."""
        return self._q_sample(x_start, times, noise)
