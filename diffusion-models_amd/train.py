"""Host-side mirror of one iteration of ``Trainer.train`` (denoising-diffusion-pytorch/denoising_diffusion/
denoising_diffusion.py:1162-1190) on the HIP training step: the micro-batch loop with ``loss / gradient_accumulate_every``,
``clip_grad_norm_(max_grad_norm)``, ``Adam.step()``, ``ema.update()`` -- every FLOP in libdm_hip.so, the parameters, Adam
moments and the EMA copy resident on the device.

``EMA`` restates the schedule of ``ema_pytorch.EMA`` as the reference configures it (``EMA(diffusion_model, beta=ema_decay,
update_every=ema_update_every)``, :1017): ema-pytorch is not in the reference tree nor in this image, so the schedule is
restated from its published source (ema-pytorch 0.7.x: ``update_after_step=100``, ``inv_gamma=1``, ``power=2/3``,
``min_value=0``) -- parity unpinned, the arithmetic itself (copy / lerp) is tested against torch.

The reference's ``Trainer`` (datasets, accelerate, checkpoints, tensorboard, FID hooks) is outside the scope of this
package; INTEGRATION.md shows the three lines its loop changes.
"""
from __future__ import annotations

from typing import Iterable, Optional

import torch


def _schedule_of(diffusion):
    """The learned noise-schedule module of a continuous-time object (six host parameters), else None."""
    return getattr(diffusion, "learned_schedule", None)


def _unet_of(diffusion):
    """The U-Net of a diffusion object and its state-dict prefix: ``model`` (DenoisingDiffusion and its variants, the
    continuous-time classes) or ``net`` (ElucidatedDiffusion)."""
    attr = getattr(diffusion, "_unet_attr", "model")
    return getattr(diffusion, attr), attr


class EMA:
    """``ema = EMA(diffusion, beta=0.995, update_every=10); ema.update(); ema.ema_model.sample(...)``."""

    def __init__(self, model, beta=0.9999, update_after_step=100, update_every=10, inv_gamma=1.0, power=2 / 3,
                 min_value=0.0):
        self.online_model = model
        self.beta, self.update_after_step, self.update_every = beta, update_after_step, update_every
        self.inv_gamma, self.power, self.min_value = inv_gamma, power, min_value
        self.step = 0
        self.initted = False
        self._ema_model = None
        self._ema_model_step = -1
        # a learned noise schedule is averaged on the host by the same rules, in a module of the EMA's own
        self._ema_sched = None
        if _schedule_of(model) is not None:
            import copy

            self._ema_sched = copy.deepcopy(_schedule_of(model)).requires_grad_(False)

    def get_current_decay(self) -> float:
        epoch = max(self.step - self.update_after_step - 1, 0)
        if epoch <= 0:
            return 0.0
        value = 1 - (1 + epoch / self.inv_gamma) ** -self.power
        return min(max(value, self.min_value), self.beta)

    def update(self):
        step = self.step
        self.step += 1
        if step % self.update_every != 0:
            return
        unet = _unet_of(self.online_model)[0]
        if step <= self.update_after_step or not self.initted:
            unet.ema_update(0.0, copy=True)
            self._update_schedule(None)
            self.initted = self.initted or step > self.update_after_step
            return
        unet.ema_update(self.get_current_decay(), copy=False)
        self._update_schedule(self.get_current_decay())

    @torch.no_grad()
    def _update_schedule(self, decay):
        """The six tensors of a learned schedule: a copy (``decay`` None), else ``ema.lerp_(online, 1 - decay)``."""
        if self._ema_sched is None:
            return
        for avg, cur in zip(self._ema_sched.parameters(), _schedule_of(self.online_model).parameters()):
            if decay is None:
                avg.copy_(cur)
            else:
                avg.lerp_(cur, 1.0 - decay)

    def state_dict(self):
        """``ema_pytorch.EMA.state_dict()`` as ``Trainer.save`` stores it under ``'ema'`` (:1108): the averaged copy under
        ``ema_model.`` (the prefix the reference's sampling scripts strip, denoising-diffusion-pytorch/sampling.py:157-159),
        the online model under ``online_model.``, and the ``initted`` / ``step`` buffers (names from ema-pytorch's
        published source; parity unpinned beyond the ``ema_model.`` prefix)."""
        d = self.online_model
        out = {"initted": torch.tensor(bool(self.initted)), "step": torch.tensor(int(self.step))}
        online = diffusion_state_dict(d)
        out.update({"online_model." + k: v for k, v in online.items()})
        averaged = diffusion_state_dict(d, ema=True) if self.step > 0 else online
        if self._ema_sched is not None and self.step > 0:
            averaged.update({"log_snr." + k: v.detach().clone() for k, v in self._ema_sched.state_dict().items()})
        out.update({"ema_model." + k: v for k, v in averaged.items()})
        return out

    def load_state_dict(self, sd):
        """``ema.load_state_dict(data['ema'])`` as ``Trainer.load`` (:1127) and the sampling scripts
        (denoising-diffusion-pytorch/sampling.py:157-159) call it.  On a model in training mode the averaged parameters go
        into the device-resident EMA state; on an inference-only model (the sampling scripts) they go straight into
        ``ema_model``, which is then ready to sample."""
        self.initted = bool(sd["initted"]) if "initted" in sd else True
        self.step = int(sd["step"]) if "step" in sd else 1
        online, attr = _unet_of(self.online_model)
        pre = f"ema_model.{attr}."
        averaged = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        if not averaged:
            raise KeyError(f"state dict has no '{pre}*' entries")
        if self._ema_sched is not None:
            spre = "ema_model.log_snr."
            self._ema_sched.load_state_dict({k[len(spre):]: v for k, v in sd.items() if k.startswith(spre)})
        if getattr(online, "_training", False):
            if self.step > 0:
                online.load_ema_state_dict(averaged)
            self._ema_model_step = -1
        else:
            _unet_of(self._make_ema_model())[0].load_state_dict(averaged)
            self._ema_model_step = self.step
        return self

    def _make_ema_model(self):
        """A shallow copy of the online diffusion object (same class, schedule, VAE, options) around a second U-Net handle
        of the same variant -- what ``copy.deepcopy(model)`` is to ``ema_pytorch.EMA``."""
        import copy

        from .unet import Unet

        d = self.online_model
        if self._ema_model is None:
            online, attr = _unet_of(d)
            cfg = online.cfg
            unet = Unet(dim=cfg.dim, init_dim=cfg.init_dim, out_dim=cfg.out_dim_, dim_mults=cfg.dim_mults, channels=cfg.channels,
                        self_condition=cfg.self_condition, sinusoidal_pos_emb_theta=cfg.sinusoidal_pos_emb_theta,
                        attn_dim_head=cfg.attn_dim_head, attn_heads=cfg.attn_heads, full_attn=cfg.full_attn,
                        text_condition=cfg.text_condition, text_emb_dim=cfg.text_emb_dim, use_cross_attn=cfg.use_cross_attn,
                        cond_channels=cfg.cond_channels, learned_sinusoidal_cond=cfg.learned_sinusoidal_cond,
                        random_fourier_features=cfg.random_fourier_features,
                        learned_sinusoidal_dim=cfg.learned_sinusoidal_dim, device=d.device)
            self._ema_model = copy.copy(d)
            setattr(self._ema_model, attr, unet)
            if self._ema_sched is not None:
                self._ema_model.log_snr = self._ema_sched  # its own schedule: the averages, not the online module
        return self._ema_model

    @property
    def ema_model(self):
        """A sampler holding the EMA weights (a second U-Net handle, refreshed when the EMA state has moved on)."""
        d = self.online_model
        self._make_ema_model()
        if self._ema_model_step != self.step:
            if self.step == 0:
                raise RuntimeError("EMA.update() has not run yet")
            _unet_of(self._ema_model)[0].load_state_dict(_unet_of(d)[0].state_dict(ema=True))
            self._ema_model_step = self.step
        return self._ema_model


def diffusion_state_dict(diffusion, ema: bool = False):
    """``DenoisingDiffusion.state_dict()`` of the reference module: the 13 schedule buffers + ``model.*`` (the online
    parameters of the device-resident training state, or its EMA copy).  ``ElucidatedDiffusion.state_dict()`` has no
    buffers and the prefix ``net.``."""
    out = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in diffusion.state_dict().items()}
    if ema:
        unet, attr = _unet_of(diffusion)
        out.update({f"{attr}." + k: v.cpu() for k, v in unet.state_dict(ema=True).items()})
    return out


def save_checkpoint(path, diffusion, *, step: int, ema: Optional[EMA] = None, lr=1e-4, betas=(0.9, 0.99), eps=1e-8,
                    version: str = "dm_hip"):
    """``Trainer.save`` (:1100-1113): ``{'step', 'model', 'opt', 'ema', 'scaler', 'version'}`` in the reference's layouts
    (``model``: ``DenoisingDiffusion.state_dict()``; ``opt``: ``torch.optim.Adam.state_dict()``; ``ema``:
    ``ema_pytorch.EMA.state_dict()``), so that the reference's ``Trainer.load`` / sampling scripts -- and
    ``load_checkpoint`` below -- read it back.  Tensors are written on the CPU."""
    opt = _unet_of(diffusion)[0].optimizer_state_dict(lr=lr, betas=betas, eps=eps)
    for st in opt["state"].values():
        st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].cpu(), st["exp_avg_sq"].cpu()
    if _schedule_of(diffusion) is not None:
        # the six schedule parameters follow the U-Net's in parameters(): their Adam state takes the next indices
        n = len(opt["param_groups"][0]["params"])
        own = diffusion._schedule_optimizer(lr, betas, eps).state_dict()
        for i, st in own["state"].items():
            opt["state"][n + i] = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
        opt["param_groups"][0]["params"] = list(range(n + len(own["param_groups"][0]["params"])))
    data = {"step": int(step), "model": diffusion_state_dict(diffusion), "opt": opt,
            "ema": ema.state_dict() if ema is not None else None, "scaler": None, "version": version}
    torch.save(data, str(path))
    return data


def load_checkpoint(path, diffusion, *, ema: Optional[EMA] = None):
    """``Trainer.load`` (:1115-1133) into a diffusion object in training mode: the online parameters, Adam's moments and
    step counter, the EMA copy and its counters.  Returns ``(step, adam_hyper_parameters)``.  The file is opened with
    ``weights_only=True`` (nothing from it is executed)."""
    data = torch.load(str(path), map_location="cpu", weights_only=True)
    diffusion.load_state_dict(data["model"])
    diffusion.train()
    opt = data["opt"]
    if _schedule_of(diffusion) is not None:
        group = dict(opt["param_groups"][0])
        n = len(group["params"]) - len(list(_schedule_of(diffusion).parameters()))
        own = diffusion._schedule_optimizer(group["lr"], group["betas"], group["eps"])
        mine = own.state_dict()
        mine["state"] = {i - n: st for i, st in opt["state"].items() if i >= n}
        own.load_state_dict(mine)
        group["params"] = group["params"][:n]
        opt = {"state": {i: st for i, st in opt["state"].items() if i < n}, "param_groups": [group]}
    hyper = _unet_of(diffusion)[0].load_optimizer_state_dict(opt)
    if ema is not None and data.get("ema") is not None:
        ema.load_state_dict(data["ema"])
    return int(data["step"]), hyper


def train_step(diffusion, micro_batches: Iterable[torch.Tensor], *, lr=1e-4, betas=(0.9, 0.99), eps=1e-8,
               max_grad_norm=1.0, ema: Optional[EMA] = None, t=None, noise=None, group=None, sync=True,
               timing: Optional[dict] = None, bucketed: Optional[bool] = None, text_mask=None, sigmas=None, times=None):
    """One iteration of ``Trainer.train`` (:1164-1190).  ``micro_batches``: the ``gradient_accumulate_every`` image batches
    (in [0, 1]) of the iteration; for a text-conditional model a micro-batch may be a pair ``(images, text_emb)``, whose
    captions ``p_losses`` then drops per image with the model's ``cond_drop_prob``.  ``t`` / ``noise`` / ``text_mask``
    (lists, one entry per micro-batch) inject the random draws for tests.  An ``ElucidatedDiffusion`` takes the same
    iteration through its ``forward``; its injection lists are ``sigmas`` / ``noise``.  So does a continuous-time object
    (``ContinuousTimeGaussianDiffusion`` / ``VParamContinuousTimeGaussianDiffusion``, told by ``random_times``); its lists
    are ``times`` / ``noise``.
    Under ``torch.distributed`` (one process per GPU, as ``accelerate`` runs the reference's Trainer under DDP) every rank
    computes the gradients of ITS micro-batches and the flat gradient buffer is averaged over the ranks in place (RCCL over
    xGMI) before the optimiser step; every rank then takes the same step.  With more than one rank (``bucketed=True`` forces
    it, ``False`` forbids it) the buffer is all-reduced BUCKET BY BUCKET on a second stream, each bucket as soon as the
    backward pass has completed it -- DDP's overlap of communication with the backward pass (``Unet.grad_buckets``);
    otherwise as one collective.
    Returns (total_loss of this rank, grad_norm): floats, or with ``sync=False`` 0-dim device tensors -- the iteration is
    then only ENQUEUED when the call returns (no host round trip: the reference's loop runs ahead of the GPU the same way
    until ``loss.item()``), so back-to-back iterations leave no idle gaps on the GPU.  ``timing`` (a dict): HIP event pairs
    around the gradient all-reduce are appended to ``timing["allreduce_events"]`` (bench.py reports its share)."""
    import torch.distributed as dist

    batches = list(micro_batches)
    k = len(batches)
    total = 0.0
    lazy = {} if sync else {"sync": False}  # only the asynchronous form asks the diffusion object for anything new
    parallel = dist.is_available() and dist.is_initialized()  # also at world size 1: the collectives are the same code path
    unet = _unet_of(diffusion)[0]
    edm = not hasattr(diffusion, "p_losses")  # ElucidatedDiffusion: the loss is forward(images), the draws sigma and noise
    ct = hasattr(diffusion, "random_times")  # continuous time: the loss is forward(images), the draws times and noise
    if ct and (t is not None or sigmas is not None or text_mask is not None):
        raise ValueError("a continuous-time diffusion has real-valued times and no captions: inject times= / noise=")
    if times is not None and not ct:
        raise ValueError("times= is the draw of a continuous-time diffusion; this object takes t= or sigmas=")
    if edm and (t is not None or text_mask is not None):
        raise ValueError("an ElucidatedDiffusion has no timesteps or captions: inject sigmas= / noise=")
    if sigmas is not None and not edm:
        raise ValueError("sigmas= is the draw of an ElucidatedDiffusion; this object takes t=")
    # by default on RCCL with more than one rank (gloo stages every collective through pinned host memory: nothing to overlap)
    sched = _schedule_of(diffusion)
    if sched is not None and parallel and dist.get_world_size(group) > 1:
        raise NotImplementedError("a learned noise schedule under more than one rank: averaging its six host gradients "
                                  "across the ranks is not built")
    overlap = parallel and bucketed is not False and hasattr(unet, "grad_buckets") and (
        bucketed or (dist.get_world_size(group) > 1 and dist.get_backend(group) == "nccl"))
    if overlap != getattr(unet, "_bucketed", False) and hasattr(unet, "grad_buckets"):
        unet.grad_buckets(enable=overlap)
    if text_mask is not None and len(text_mask) != k:
        raise ValueError(f"text_mask has {len(text_mask)} entries for {k} micro-batches")
    for i, data in enumerate(batches):
        if ct:
            loss = diffusion(data, times=times[i] if times is not None else None,
                             noise=noise[i] if noise is not None else None, loss_scale=1.0 / k, accumulate=i > 0, **lazy)
            total = (total + float(loss)) if sync else (loss if i == 0 else total + loss)
            continue
        if edm:
            loss = diffusion(data, sigmas=sigmas[i] if sigmas is not None else None,
                             noise=noise[i] if noise is not None else None, loss_scale=1.0 / k, accumulate=i > 0, **lazy)
            total = (total + float(loss)) if sync else (loss if i == 0 else total + loss)
            continue
        text = {}  # only a micro-batch with captions asks the diffusion object for anything new
        if isinstance(data, (tuple, list)):
            if len(data) != 2:
                raise ValueError("a micro-batch is an image tensor or a pair (images, text_emb)")
            data, emb = data
            text = {"text_emb": emb}
        if text_mask is not None and text_mask[i] is not None:
            if not text:
                raise ValueError(f"text_mask[{i}] given for a micro-batch without text_emb")
            text["text_mask"] = text_mask[i]
        x = diffusion.normalize(data.to(diffusion.device, torch.float32))
        ti = t[i] if t is not None else torch.randint(0, diffusion.num_timesteps, (x.shape[0],)).long()
        ni = noise[i] if noise is not None else None
        loss = diffusion.p_losses(x, ti, noise=ni, loss_scale=1.0 / k, accumulate=i > 0, **text, **lazy)
        total = (total + float(loss)) if sync else (loss if i == 0 else total + loss)
    if parallel:
        # DDP averages the gradients over the ranks.  The buffer is the library's own (a zero-copy view); no host
        # synchronisation anywhere: each collective is ordered behind the kernels that complete its span, and the optimiser
        # step behind the collectives.
        flat, world = unet.grads_flat(), dist.get_world_size(group)
        ev = None
        if timing is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        if overlap:
            # bucket by bucket, on a second stream: a bucket's all-reduce starts when the backward pass (still running --
            # the call above only enqueued it) has completed that bucket, and runs beside the rest of the pass
            main = torch.cuda.current_stream(diffusion.device)
            if unet._comm_stream is None:
                unet._comm_stream = torch.cuda.Stream(device=diffusion.device)
            side = unet._comm_stream
            for b, (off, n) in enumerate(unet.grad_buckets()):
                unet.bucket_wait(b, side)
                with torch.cuda.stream(side):
                    span = flat[off:off + n]
                    dist.all_reduce(span, op=dist.ReduceOp.SUM, group=group)
                    span.div_(world)
            main.wait_stream(side)
        else:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
            flat.div_(world)
        if ev is not None:
            ev[1].record()
            timing.setdefault("allreduce_events", []).append(ev)
    if sched is not None:
        # the six host parameters share the clip: their squared norm joins the library's, the host applies the same
        # coefficient (clip_grad_norm_: max_norm / (total + 1e-6), capped at 1) and takes the same Adam step
        grads = [p.grad for p in sched.parameters() if p.grad is not None]
        sq = float(sum(float(g.double().pow(2).sum()) for g in grads))
        norm = unet.optimizer_step(lr=lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, extra_sq_norm=sq)
        if max_grad_norm:
            coef = min(1.0, max_grad_norm / (norm + 1e-6))
            for g in grads:
                g.mul_(coef)
        diffusion._schedule_optimizer(lr, betas, eps).step()
        if ema is not None:
            ema.update()
        return total, norm
    norm = unet.optimizer_step(lr=lr, betas=betas, eps=eps, max_grad_norm=max_grad_norm, **lazy)
    if ema is not None:
        ema.update()
    return total, norm
