"""The noisy classifier of the classifier-guidance fixtures and tests, and fp64 restatements of the two guidance passes.

The classifier is a linear map of the flattened image plus a time term:
``logits = x.flatten(1) @ W.T + b + (t / T) * u``.  ``cond_fn`` returns ``scale * d log_softmax(logits)[y] / d x`` through
``torch.autograd.grad``.  ``tests/golden/make_golden_classifier_guidance.py`` draws the weights, runs the reference with
this ``cond_fn`` and stores the weights in the fixture; the GPU tests rebuild the identical function from them."""
import torch


def make_classifier(n_classes, numel, seed, std=0.05):
    g = torch.Generator().manual_seed(seed)
    return dict(W=torch.randn((n_classes, numel), generator=g) * std, b=torch.randn((n_classes,), generator=g) * std,
                u=torch.randn((n_classes,), generator=g) * std)


def make_cond_fn(clf, timesteps, device=None, dtype=torch.float32, calls=None):
    """``cond_fn(x, t, y=, scale=)``.  ``calls`` (a list) receives a clone of every x and t the function is called with."""
    W, b, u = (clf[k].to(device=device, dtype=dtype) for k in ("W", "b", "u"))

    def cond_fn(x, t, y=None, scale=1.0):
        if calls is not None:
            calls.append((x.detach().clone(), t.detach().clone()))
        with torch.enable_grad():
            xin = x.detach().to(dtype).requires_grad_(True)
            logits = xin.flatten(1) @ W.T + b + (t.to(dtype) / timesteps)[:, None] * u
            logp = torch.log_softmax(logits, dim=-1)
            picked = logp[torch.arange(xin.shape[0], device=xin.device), y.to(xin.device)]
            return torch.autograd.grad(picked.sum(), xin)[0] * scale

    return cond_fn


def x_start(x, model_out, row, objective, dtype):
    """``ddpm_x_start`` of csrc/step_device.h in ``dtype``: the clamped x_0 estimate by objective (0, 1, 2)."""
    x, e, c = x.to(dtype), model_out.to(dtype), row.to(dtype)
    if objective == 0:
        x0 = c[0] * x - c[1] * e
    elif objective == 1:
        x0 = e
    else:
        x0 = c[6] * x - c[7] * e
    return x0.clamp(-1.0, 1.0)


def cg_mean(x, model_out, row, objective, dtype):
    """(mean, x_start) of ``cg_mean_kernel``."""
    xs = x_start(x, model_out, row, objective, dtype)
    c = row.to(dtype)
    return c[2] * xs + c[3] * x.to(dtype), xs


def cg_finish(mean, grad, z, row, dtype):
    """(out, guided mean) of ``cg_finish_kernel``; a row with ``row[5] == 0`` reads no noise."""
    c = row.to(dtype)
    m = mean.to(dtype) + c[8] * grad.to(dtype)
    if float(row[5]) != 0:
        return m + c[4] * z.to(dtype), m
    return m + c[4] * 0.0, m
