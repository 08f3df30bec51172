"""The host side of a sampling loop and of a loss call, as every diffusion class runs them: the shape check, the start
image with the injected noise rows, the argument fields the loop entries of libdm_hip.so share, and the tail of a training
call.  Plain functions over the object, which supplies ``device``, ``_randn``, ``_stream`` and ``_lib`` (and, for an
integer-time loop, ``model``, ``channels``, ``use_graph`` and the unnormalise pair): ``DenoisingDiffusion`` with its
subclasses and ``FloatTimeDiffusion`` share them without inheriting from one another.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def checked_shape(diff, shape):
    """``shape`` as a tuple of ints that the model can sample."""
    shape = tuple(int(v) for v in shape)
    B, Cc, H, W = shape
    assert Cc == diff.channels, f"shape has {Cc} channels, the model {diff.channels}"
    f = diff.model.downsample_factor
    if getattr(diff.model, "seq1d", False):  # a sequence (B, C, L) arrives as its one-row view (B, C, 1, L)
        assert B > 0 and H == 1 and W % f == 0, f"shape {shape}: one row, its length divisible by {f}"
        return shape
    assert B > 0 and H % f == 0 and W % f == 0, f"shape {shape}: the sides must be divisible by {f}"
    return shape


def loop_start(diff, shape, noise, seed, sample_offset, slots, x_init=None):
    """(seed, start image, noise rows or None) of a sampling loop.  ``slots``: a bool array (n_rows,) or (n_rows, k), one
    entry per noise slot of the loop's noise tensor.  An injected ``noise`` callable is called once for the start image
    (not when ``x_init`` gives it), then once per True slot, row-major: the reference's order of draws.  The slots it is
    not called for are zeros; the rows are (n_rows[, k], *shape) fp32 on the device, None when there is no slot.  Without
    a callable the start image is Philox draw 0 at ``sample_offset`` and the loop draws its rows on the device."""
    if seed is None:
        seed = _lib.default_seed()
    rows = None
    if noise is not None:
        x_T = noise(shape) if x_init is None else x_init
        slots = torch.as_tensor(slots, dtype=torch.bool)
        zero = torch.zeros(shape, dtype=torch.float32)
        drawn = [noise(shape).to(torch.float32) if flag else zero for flag in slots.reshape(-1).tolist()]
        rows = torch.stack(drawn, dim=0) if drawn else None
    else:
        x_T = diff._randn(shape, seed, 0, int(sample_offset)) if x_init is None else x_init
    x_T = x_T.to(diff.device, torch.float32).contiguous()
    assert tuple(x_T.shape) == shape, f"initial state {tuple(x_T.shape)} does not match {shape}"
    if rows is None:
        return seed, x_T, None
    assert tuple(rows.shape[1:]) == shape, "noise() must return tensors of the sampled shape"
    return seed, x_T, rows.reshape(tuple(slots.shape) + shape).to(diff.device).contiguous()


def loop_call(diff, args, entry, shape, start, sample_offset, times, table, table_field, n_frames, return_all_timesteps,
              unnormalize=None):
    """Run the loop ``entry(handle, args)`` of libdm_hip.so.  ``args`` holds the class's own fields; the common ones are
    set here: the times and the step table (``table_field``: ``coefs_host`` or ``table_host``), ``start`` (what
    ``loop_start`` returned), the outputs, the shape and the flags.  Returns the final image, or with
    ``return_all_timesteps`` the ``n_frames`` frames as (B, n_frames, C, H, W) like ``torch.stack(imgs, dim=1)``."""
    seed, x_T, noise_dev = start
    B, _, H, W = shape
    out = torch.empty(shape, device=diff.device, dtype=torch.float32)
    all_steps = torch.empty((n_frames,) + shape, device=diff.device, dtype=torch.float32) if return_all_timesteps else None
    times_arr = (C.c_int64 * len(times))(*[int(t) for t in times])
    table = table.contiguous()
    args.times_host = C.cast(times_arr, C.POINTER(C.c_int64))
    setattr(args, table_field, _lib.fptr(table))
    args.x_T, args.noise, args.seed, args.sample_offset = _lib.ptr(x_T), _lib.ptr(noise_dev), seed, int(sample_offset)
    args.out, args.all_steps = _lib.ptr(out), _lib.ptr(all_steps)
    args.B, args.H, args.W = B, H, W
    args.unnormalize = diff._unnormalize_flag if unnormalize is None else int(bool(unnormalize))
    args.use_graph, args.stream = 1 if diff.use_graph else 0, diff._stream()
    _lib.check(entry(diff.model._handle, C.byref(args)))
    if not return_all_timesteps:
        return out
    return diff.unnormalize(all_steps.permute(1, 0, 2, 3, 4).contiguous())


def loss_inputs(diff, x_start, t, noise):
    """The batch and its noise on the device, checked against the model and ``t``; the noise defaults to a device Philox
    draw under a fresh seed."""
    x_start = x_start.to(diff.device, torch.float32).contiguous()
    b, c, h, w = x_start.shape
    f = diff.model.downsample_factor
    if c != diff.channels or h % f or w % f:
        raise RuntimeError(f"x_start {tuple(x_start.shape)}: expected {diff.channels} channels and sides divisible by {f}")
    noise = (noise.to(diff.device, torch.float32).contiguous() if noise is not None
             else diff._randn(x_start.shape, _lib.default_seed(), 0, 0))
    if noise.shape != x_start.shape or t.numel() != b:
        raise RuntimeError(f"noise {tuple(noise.shape)} / t ({t.numel()} entries) do not match x_start {tuple(x_start.shape)}")
    return x_start, noise


def loss_call(diff, handle, entry, args, sync):
    """Run the training entry ``entry(handle, args)`` (``loss_out_host`` and ``stream`` are set here): the loss as a 0-dim
    CPU tensor, or with ``sync=False`` a 0-dim device tensor (nothing waited for)."""
    loss = C.c_float(0.0)
    args.loss_out_host = C.pointer(loss) if sync else None
    args.stream = diff._stream()
    _lib.check(entry(handle, C.byref(args)))
    if sync:
        return torch.tensor(loss.value, dtype=torch.float32)
    val = torch.empty((), device=diff.device, dtype=torch.float32)
    _lib.check(diff._lib.dm_unet_train_scalar(handle, 0, _lib.ptr(val), args.stream))
    return val
