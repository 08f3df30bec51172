"""GPU parity of the conditioning head of the U-Net and of the deferred reduction tables of the training backward pass,
each on its own through the C ABI (dm_unet_cond_forward, dm_unet_cond_backward, dm_op_deferred_reduce), against fp64 on the CPU
on the same fp32 inputs.  The entry points call the functions the walks call (cond_forward, cond_train_forward,
cond_backward, flush_deferred_reductions), so what runs here is what the models run.

The head.  time [+ pooled caption] -> e0 (sinusoid) -> h1pre (time_mlp.1) -> h1 (GELU) -> temb (time_mlp.3) -> [te0pre
(text_proj.0) -> te0 (GELU) -> cat = (temb | text_proj.2(te0)) -> tfinal = text_concat_proj(cat), masked rows = temb] -> tact
(SiLU) -> ss = every ResnetBlock.mlp.1.  Forward checks are stage-local: a stage is compared with the fp64 restatement of
that stage alone (the lines of oracle.unet_oracle.time_mlp / unet_forward) applied to the GPU's own input of the stage, so a
failure names the kernel; then ss end to end.  The sinusoid reference is sin / cos in fp64 of the argument as the oracle
forms it in fp32 (``float(t) * freqs``; learned: ``(t * w) * 2 pi``).  Gradients are fp64 autograd of sum(ss * dss).

Which kernel takes a (rows R, inputs I, outputs O, leading dimensions) Linear, by the predicates of small_gemm.hip and the
launchers (td = 128, fdim = 32 or 17, E = 48, ss_total = 960 for `small`, 4032 for `wide`; no profile row exists for these
kernels, so this table is documentation; the DM_NO_SMALL_GEMM child of tests/test_hip_forced_dispatch.py puts the VALU
kernels on every shape):

  forward  launch_linear_rows        act_in / act_out != 0 (inference walk: e0->h1, ctx->te0, tfinal->ss): VALU always
                                     R < 8: linear_rows_kernel; R >= 8: linear_rows8_kernel (B = 9, 20: ragged last group)
                                     else rows_gemm_nt when R >= 16, I % 16 == 0, O % 16 == 0, ldx % 4 == 0:
                                       B = 20: h1->temb, te0->cat+td (ldy = 2 td), cat->tfinal (I = ldx = 2 td), tact->ss;
                                       e0->h1pre only for fdim = 32 (fdim = 17: rows8, odd rows); ctx->te0pre (I = E = 48)
                                     B = 1, 3: linear_rows_kernel; B = 9: linear_rows8_kernel
  dW       launch_mlp_rows_wgrad     rows_gemm_tn (row-pointer table) when R >= 4, I % 64 == 0, O % 64 == 0: B = 9, 20;
                                     B = 1, 3: mlp_rows_wgrad_kernel (B = 3: the 4-row group ragged)
           launch_linear_wgrad       rows_gemm_tn under the same predicate: B = 9, 20 for I = 128, 256; time_mlp.1 (I = fdim) and
                                     text_proj.0 (I = 48): linear_wgrad_kernel at every B
  dx       launch_linear_dgrad       rows_gemm_nn when R >= 16, I % 64 == 0, O % 16 == 0: B = 20 (dss->dtf0: shares =
                                     ceil(O / 16 / SG_NN_CH) > 1 for `wide`; dcat+td with ldy = 2 td; dtc->dcat I = 2 td);
                                     else linear_dgrad_kernel, with 16 shares + linear_dgrad_sum_kernel when O >= 2048 (`wide`,
                                     B = 3); dh1pre->de0 (I = 17, odd): linear_dgrad_kernel at every B
  `odd` (dim 24: td = 96, fdim = 24): I % 64 != 0, so mlp_rows_wgrad_kernel, linear_wgrad_kernel and linear_dgrad_kernel take
  B = 9 and 20 in the default process too; rows_gemm_nt still takes the forward at B = 20 (I % 16 == 0)
  colsum   launch_colsum             colsum_lanes_kernel (B <= 512 rows), on the strided half row of dcat for text_proj.2.bias
                                     and time_mlp.3.bias with a caption

Limits (the rule of tests/test_hip_conv_families.py).  Per tensor rel-L2 and max|got - ref| / rms(ref); the floor of each is
the fp32 restatement of the same stage (torch fp32 on the CPU) against the fp64 reference, measured here and never taken
from the kernel; the kernel may be FACTOR = 4 times the floor off.  `randn` cases also stay under 2e-5 (forward) / 5e-5 (per
gradient tensor).  sin / cos: max absolute error <= 4 * max(floor, 2^-24).  Every output is finite: the workspace and the
gradient slots start as NaNs.  Every case prints ``case tensor: kernel error, floor, limit`` before it asserts (run with
-s; DESIGN.md holds the table)."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from oracle import unet_oracle as uo

pytestmark = pytest.mark.gpu
TOL_FWD = 2e-5
TOL_BWD = 5e-5
FACTOR = 4.0
DEV = "cuda:0"

KINDS = {
    "small": dict(dim=32, dim_mults=(1, 2)),
    "wide": dict(dim=32, dim_mults=(1, 2, 4, 8)),
    "odd": dict(dim=24, dim_mults=(1, 2)),  # td = 96: no 64-wide tile of rows_gemm_tn / nn, so their VALU forms at every B
    "learned": dict(dim=32, dim_mults=(1, 2), learned_sinusoidal_cond=True, learned_sinusoidal_dim=16),
    "fourier": dict(dim=32, dim_mults=(1, 2), random_fourier_features=True, learned_sinusoidal_dim=16),
    "text": dict(dim=32, dim_mults=(1, 2), text_condition=True, text_emb_dim=48),
}
SALT = {"small": 21, "wide": 22, "odd": 26, "learned": 23, "fourier": 24, "text": 25}
E_TEXT = 48
# the ends of EDM's c_noise(sigma) = ln(sigma) / 4 over sigma in [0.002, 80], and 0
T_FLOAT = (0.25 * math.log(0.002), 0.25 * math.log(80.0), 0.0)
T_INT = (0, 1, 999)


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def block_names(cfg):
    """The ResnetBlocks in the order of their slices of the (B, ss_total) scale / shift rows."""
    n = len(cfg.dim_mults)
    return ([f"downs.{i}.{j}" for i in range(n) for j in (0, 1)] + ["mid_block1", "mid_block2"] +
            [f"ups.{i}.{j}" for i in range(n) for j in (0, 1)] + ["final_res_block"])


class Net:
    """One U-Net handle with seeded parameters; hot: time_mlp.1.weight and text_proj.0.weight times 8."""

    def __init__(self, kind, family):
        self.kind, self.family = kind, family
        self.u = dm.Unet(channels=3, device=DEV, **KINDS[kind])
        self.cfg = cfg = self.u.cfg
        sd = dm.synth_state_dict(self.u.param_spec(), salt=SALT[kind])
        if family == "hot":
            sd["time_mlp.1.weight"] = sd["time_mlp.1.weight"] * 8
            if "text_proj.0.weight" in sd:
                sd["text_proj.0.weight"] = sd["text_proj.0.weight"] * 8
        self.u.load_state_dict(sd)
        self.blocks = block_names(cfg)
        self.lsd = cfg.learned_sinusoidal_dim if cfg.random_or_learned_sinusoidal_cond else 0
        self.text = bool(cfg.text_condition)
        self.td = 4 * cfg.dim
        self.head_names = (["time_mlp.1.weight", "time_mlp.1.bias", "time_mlp.3.weight", "time_mlp.3.bias"] +
                           [f"{b}.mlp.1.{w}" for b in self.blocks for w in ("weight", "bias")] +
                           (["time_mlp.0.weights"] if self.lsd else []) +
                           ([f"text_proj.{i}.{w}" for i in (0, 2) for w in ("weight", "bias")] +
                            ["text_concat_proj.weight", "text_concat_proj.bias"] if self.text else []))
        self.sd = {k: sd[k] for k in self.head_names}
        self.ss_total = sum(sd[f"{b}.mlp.1.bias"].numel() for b in self.blocks)
        self.armed = False

    def params(self, dtype, grad=False):
        return {k: v.to(dtype).clone().requires_grad_(grad) for k, v in self.sd.items()}

    def arm(self):
        if not self.armed:
            if self.lsd:
                _lib.check(self.u._lib.dm_unet_train_enable_ft(self.u._handle, int(self.cfg.random_fourier_features)))
            else:
                _lib.check(self.u._lib.dm_unet_train_enable(self.u._handle))
            self.armed = True
        return self


@functools.lru_cache(maxsize=None)
def net(kind, family):
    return Net(kind, family)


# ---- the reference: the lines of oracle.unet_oracle (time_mlp :54-62, the text-concat branch of unet_forward :222-229,
# resnet_block's mlp :81-82) one stage at a time, in the dtype of their arguments -------------------------------------------
def sin_arg32(N, t):
    """The argument of sin / cos as the oracle forms it in fp32, (R, half).  The frequency table of the fixed sinusoid is
    exp(i * -k) rounded to fp32 (exp in fp64, then rounded): torch's vectorised fp32 exp is one ulp off that value at some
    indices (i = 4 at dim 24, i = 24 at dim 64 on the CPUs this was written on), which t = 999 turns into 3e-6 of sin --
    a property of that exp, not of the embedding, so the reference does not inherit it."""
    if N.lsd:
        x = t.to(torch.float32)[:, None]
        return (x * N.sd["time_mlp.0.weights"][None, :]) * torch.tensor(2 * math.pi, dtype=torch.float32)
    half = N.cfg.dim // 2
    k = math.log(N.cfg.sinusoidal_pos_emb_theta) / (half - 1)
    a = torch.arange(half) * -k
    assert a.dtype == torch.float32
    freqs = torch.exp(a.double()).to(torch.float32)
    assert float(((freqs - torch.exp(a)) / freqs).abs().max()) <= 2.0 ** -23  # the oracle's table, to an ulp
    return t.to(torch.float32)[:, None] * freqs[None, :]


def e0_of(N, t, dtype):
    """sin / cos of the fp32 argument, in fp64 (the reference) or in fp32 (its floor); the learned row leads with t."""
    t32 = t.to(torch.float32)
    a = sin_arg32(N, t).to(dtype)
    e = torch.cat((a.sin(), a.cos()), dim=-1)
    e = torch.cat((t32.to(dtype)[:, None], e), dim=-1) if N.lsd else e
    own = (uo.learned_sinusoidal_pos_emb(t32, N.sd["time_mlp.0.weights"]) if N.lsd
           else uo.sinusoidal_pos_emb(t32, N.cfg.dim, N.cfg.sinusoidal_pos_emb_theta))
    assert float((e - own.to(dtype)).abs().max()) < 1e-5  # the restatement is the oracle's embedding (to that ulp times t)
    return e


def ss_matrix(N, P):
    return (torch.cat([P[f"{b}.mlp.1.weight"] for b in N.blocks]), torch.cat([P[f"{b}.mlp.1.bias"] for b in N.blocks]))


STAGES = {
    "h1pre": lambda N, P, e0: F.linear(e0, P["time_mlp.1.weight"], P["time_mlp.1.bias"]),
    "gelu": lambda N, P, x: F.gelu(x),
    "h1_fused": lambda N, P, e0: F.gelu(F.linear(e0, P["time_mlp.1.weight"], P["time_mlp.1.bias"])),
    "temb": lambda N, P, h1: F.linear(h1, P["time_mlp.3.weight"], P["time_mlp.3.bias"]),
    "te0pre": lambda N, P, c: F.linear(c, P["text_proj.0.weight"], P["text_proj.0.bias"]),
    "te0_fused": lambda N, P, c: F.gelu(F.linear(c, P["text_proj.0.weight"], P["text_proj.0.bias"])),
    "cat_right": lambda N, P, te0: F.linear(te0, P["text_proj.2.weight"], P["text_proj.2.bias"]),
    "t2": lambda N, P, cat: F.linear(cat, P["text_concat_proj.weight"], P["text_concat_proj.bias"]),
    "silu": lambda N, P, x: F.silu(x),
    "ss": lambda N, P, tact: F.linear(tact, *ss_matrix(N, P)),
    "ss_fused": lambda N, P, tf: F.linear(F.silu(tf), *ss_matrix(N, P)),
}


def chain(N, P, e0, ctx, mask):
    """e0 -> ss, every intermediate; differentiable in P (and in e0).  ctx None: no caption."""
    o = {"e0": e0}
    o["h1pre"] = STAGES["h1pre"](N, P, e0)
    o["h1"] = F.gelu(o["h1pre"])
    o["temb"] = STAGES["temb"](N, P, o["h1"])
    o["tfinal"] = o["temb"]
    if ctx is not None:
        B = ctx.shape[0]
        o["te0pre"] = STAGES["te0pre"](N, P, ctx)
        o["te0"] = F.gelu(o["te0pre"])
        temb = o["temb"].expand(B, -1)
        o["cat"] = torch.cat((temb, STAGES["cat_right"](N, P, o["te0"])), dim=1)
        t2 = STAGES["t2"](N, P, o["cat"])
        o["tfinal"] = t2 if mask is None else torch.where(mask[:, None] != 0, t2, temb)
    o["tact"] = F.silu(o["tfinal"])
    o["ss"] = STAGES["ss"](N, P, o["tact"])
    return o


# ---- limits ------------------------------------------------------------------------------------------------------------------
def metrics(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    d = got - ref
    return (float(d.norm() / ref.norm().clamp_min(1e-300)),
            float(d.abs().max() / ref.pow(2).mean().sqrt().clamp_min(1e-300)))


class Checker:
    """Prints, then asserts at the end, every tensor of one case: no tensor hides behind the first failure."""

    def __init__(self, label, family, bound):
        self.label, self.family, self.bound, self.bad = label, family, bound, []

    def finite(self, tensor, got):
        if not bool(torch.isfinite(got).all()):
            self.bad.append((tensor, "not finite", int((~torch.isfinite(got)).sum())))
            return False
        return True

    def __call__(self, tensor, got, ref64, floor32):
        e = metrics(got, ref64)
        f = metrics(floor32, ref64)
        lim = [FACTOR * f[0], FACTOR * f[1]]
        if self.family == "randn":
            lim[0] = min(lim[0], self.bound)
        print(f"cond_ops {self.label} {tensor}: rel-L2 kernel {e[0]:.3g} floor {f[0]:.3g} limit {lim[0]:.3g} | "
              f"max/rms kernel {e[1]:.3g} floor {f[1]:.3g} limit {lim[1]:.3g}")
        if self.finite(tensor, got) and (e[0] > lim[0] or e[1] > lim[1]):
            self.bad.append((tensor, e, lim))

    def sincos(self, tensor, got, ref64, floor32):
        e = float((got.double().cpu() - ref64).abs().max())
        f = float((floor32.double() - ref64).abs().max())
        lim = FACTOR * max(f, 2.0 ** -24)
        print(f"cond_ops {self.label} {tensor}: max abs kernel {e:.3g} floor {f:.3g} limit {lim:.3g}")
        if self.finite(tensor, got) and e > lim:
            self.bad.append((tensor, e, lim))

    def exact(self, tensor, got, want):
        ok = torch.equal(got.cpu(), want.cpu())
        print(f"cond_ops {self.label} {tensor}: bitwise {'equal' if ok else 'DIFFERENT'}")
        if not ok:
            self.bad.append((tensor, "not bitwise equal", float((got.cpu().double() - want.cpu().double()).abs().max())))

    def stage(self, tensor, N, name, got, *inputs):
        """`got` against stage `name` of the reference applied to the GPU's own inputs of the stage."""
        ref = STAGES[name](N, N.params(torch.float64), *[x.detach().double().cpu() for x in inputs])
        floor = STAGES[name](N, N.params(torch.float32), *[x.detach().float().cpu() for x in inputs])
        self(tensor, got, ref, floor)

    def done(self):
        assert not self.bad, (self.label, self.bad)


# ---- calls -------------------------------------------------------------------------------------------------------------------
TIME_KIND = {("int", False): _lib.COND_TIME_INT, ("float", False): _lib.COND_TIME_FLOAT,
             ("int", True): _lib.COND_TIME_INT_SHARED, ("float", True): _lib.COND_TIME_FLOAT_SHARED}


def cond_forward(N, walk, t, ctx, mask, B, shared=False):
    """Every intermediate the walk forms, as device tensors that started as NaNs."""
    train = walk == "train"
    is_float = t.is_floating_point()
    R = 1 if shared else B
    Bs = 1 if (shared and ctx is None) else B
    td, fdim = N.td, (N.lsd + 1 if N.lsd else N.cfg.dim)
    out = {"e0": nans(R, fdim), "h1": nans(R, td), "temb": nans(R, td), "ss": nans(Bs, N.ss_total),
           "tfinal": nans(B if ctx is not None else R, td)}
    if ctx is not None:
        out.update(te0=nans(B, td), cat=nans(B, 2 * td))
    if train:
        out.update(h1pre=nans(R, td), tact=nans(B, td))
        if ctx is not None:
            out["te0pre"] = nans(B, td)
    bufs = _lib.CondBufs(**{k: _lib.ptr(v) for k, v in out.items()})
    t_dev = t.to(DEV, torch.float32 if is_float else torch.int64).contiguous()
    ctx_dev = None if ctx is None else ctx.to(DEV).contiguous()
    mask_dev = None if mask is None else mask.to(DEV, torch.int32).contiguous()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(N.u._lib.dm_unet_cond_forward(N.u._handle, _lib.COND_WALK_TRAIN if train else _lib.COND_WALK_INFER,
                                             TIME_KIND["float" if is_float else "int", shared], _lib.ptr(t_dev),
                                             _lib.ptr(ctx_dev), _lib.ptr(mask_dev), C.byref(bufs), B, stream))
    torch.cuda.synchronize()
    return out, ctx_dev, mask_dev


def cond_backward(N, tape, ctx_dev, mask_dev, dss, B, accumulate, want_dt):
    bufs = _lib.CondBufs(**{k: _lib.ptr(v) for k, v in tape.items()})
    dt = nans(B) if want_dt else None
    dss_dev = dss.to(DEV).contiguous()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(N.u._lib.dm_unet_cond_backward(N.u._handle, C.byref(bufs), _lib.ptr(ctx_dev), _lib.ptr(mask_dev),
                                              _lib.ptr(dss_dev), _lib.ptr(dt), B, accumulate, stream))
    torch.cuda.synchronize()
    return {k: N.u.grad(k).cpu() for k in N.head_names}, (None if dt is None else dt.cpu())


def times(kind, B, seed):
    """Integer times with 0, 1, 999 in front; float times with the ends of the c_noise range and 0.0 in front."""
    g = torch.Generator().manual_seed(seed)
    if kind == "int":
        t = torch.randint(0, 1000, (B,), generator=g)
        head = torch.tensor(T_INT)
    else:
        t = torch.rand((B,), generator=g) * (T_FLOAT[1] - T_FLOAT[0]) + T_FLOAT[0]
        head = torch.tensor(T_FLOAT, dtype=torch.float32)
    n = min(B, 3)
    # one row: the largest argument (999, or the far end of the c_noise range)
    t[:n] = head[:n] if B > 1 else head[2 if kind == "int" else 0:][:1]
    return t


def text_mask(which, B):
    if which is None:
        return None
    if which == "ones":
        return torch.ones(B, dtype=torch.int32)
    if which == "zeros":
        return torch.zeros(B, dtype=torch.int32)
    m = (torch.arange(B) % 3 != 1).to(torch.int32)  # mixed: 1 0 1 1 0 1 ...
    assert 0 < int(m.sum()) < B
    return m


# ---- forward -------------------------------------------------------------------------------------------------------------
def fwd_cases():
    c = []
    for B in (1, 3, 9, 20):
        for walk in ("infer", "train"):
            c.append(("small", "randn", walk, "int", B, None, False))
            c.append(("learned", "randn", walk, "float", B, None, False))
        c.append(("learned", "randn", "infer", "int", B, None, False))  # the learned row of sinusoid_kernel
    for kind, tk in (("small", "int"), ("learned", "float"), ("learned", "int")):
        c.append((kind, "randn", "infer", tk, 3, None, True))  # the samplers' shared time: one row
    for walk in ("infer", "train"):
        c.append(("small", "hot", walk, "int", 9, None, False))
        c.append(("learned", "hot", walk, "float", 20, None, False))
        c.append(("fourier", "randn", walk, "float", 9, None, False))
        for B in (3, 20):
            c.append(("wide", "randn", walk, "int", B, None, False))
        for B in (9, 20):
            c.append(("odd", "randn", walk, "int", B, None, False))
        for B in (3, 9, 20):
            for m in (None, "ones", "zeros", "mixed"):
                c.append(("text", "randn", walk, "int", B, m, False))
        c.append(("text", "hot", walk, "int", 9, "mixed", False))
    for m in (None, "ones", "zeros", "mixed"):
        c.append(("text", "randn", "infer", "int", 9, m, True))  # select_rows with x_ld = 0, broadcast_rows
    c.append(("text", "randn", "infer", "int", 20, "mixed", True))
    return c


def case_id(c):
    return "-".join(str(x) for x in c)


@pytest.mark.parametrize("case", fwd_cases(), ids=case_id)
def test_cond_forward_stage_by_stage(case):
    kind, family, walk, tk, B, mk, shared = case
    N = net(kind, family)
    assert kind != "wide" or N.ss_total >= 2048, N.ss_total
    ck = Checker(case_id(case), family, TOL_FWD)
    if shared:  # one row: each of the values the per-image cases put in front
        head = torch.tensor(T_INT) if tk == "int" else torch.tensor(T_FLOAT, dtype=torch.float32)
        for v in head:
            check_forward(ck, N, case, v.reshape(1))
    else:
        check_forward(ck, N, case, times(tk, B, seed=B))
    ck.done()


def check_forward(ck, N, case, t):
    kind, family, walk, tk, B, mk, shared = case
    ctx = seeded((B, E_TEXT), 100 + B) if N.text else None
    mask = text_mask(mk, B)
    G, _, _ = cond_forward(N, walk, t, ctx, mask, B, shared)
    train = walk == "train"
    # the embedding: sin / cos of the fp32 argument; the leading column of the learned row is the time itself
    e64, e32 = e0_of(N, t, torch.float64), e0_of(N, t, torch.float32)
    ck.sincos("e0", G["e0"], e64, e32)
    if N.lsd:
        ck.exact("e0[:, 0]", G["e0"][:, 0], t.to(torch.float32))
    if train:
        ck.stage("h1pre", N, "h1pre", G["h1pre"], G["e0"])
        ck.stage("h1", N, "gelu", G["h1"], G["h1pre"])
        if family == "hot":  # the hot family reaches the tails (by the reference, not by the kernel): about 12 with these weights
            hot = float(chain(N, N.params(torch.float64), e64, None, None)["h1pre"].abs().max())
            print(f"cond_ops {ck.label} max |h1pre| of the reference: {hot:.3g}")
            assert hot > 8
    else:
        ck.stage("h1", N, "h1_fused", G["h1"], G["e0"])
    ck.stage("temb", N, "temb", G["temb"], G["h1"])
    if ctx is not None:
        if train:
            ck.stage("te0pre", N, "te0pre", G["te0pre"], ctx)
            ck.stage("te0", N, "gelu", G["te0"], G["te0pre"])
        else:
            ck.stage("te0", N, "te0_fused", G["te0"], ctx)
        ck.exact("cat[:, :td]", G["cat"][:, :N.td], G["temb"].expand(B, -1))
        ck.stage("cat[:, td:]", N, "cat_right", G["cat"][:, N.td:], G["te0"])
        if mask is None or int(mask.sum()) > 0:
            keep = torch.ones(B, dtype=torch.bool) if mask is None else mask.bool()
            ck.stage("tfinal[kept]", N, "t2", G["tfinal"][keep.to(DEV)], G["cat"][keep.to(DEV)])
        if mask is not None and int(mask.sum()) < B:
            drop = ~mask.bool()
            ck.exact("tfinal[dropped]", G["tfinal"][drop.to(DEV)], G["temb"].expand(B, -1)[drop.to(DEV)])
    else:
        ck.exact("tfinal", G["tfinal"], G["temb"])
    if train:
        ck.stage("tact", N, "silu", G["tact"], G["tfinal"])
        ck.stage("ss", N, "ss", G["ss"], G["tact"])
    else:
        ck.stage("ss", N, "ss_fused", G["ss"], G["tfinal"])
    # end to end against the whole chain
    want = chain(N, N.params(torch.float64), e64, None if ctx is None else ctx.double(), mask)
    floor = chain(N, N.params(torch.float32), e32, ctx, mask)
    ck("ss end-to-end", G["ss"], want["ss"], floor["ss"])
    assert G["ss"].shape[0] == (1 if (shared and ctx is None) else B)


# ---- backward -------------------------------------------------------------------------------------------------------------
def dss_of(N, family, B, seed):
    d = seeded((B, N.ss_total), seed)
    if family == "wide":  # every ResnetBlock's slice times exp(u), u spread over [-4.6, 4.6] and shuffled
        n = len(N.blocks)
        u = torch.linspace(-4.6, 4.6, n)[torch.randperm(n, generator=torch.Generator().manual_seed(seed))]
        off = 0
        for b, ub in zip(N.blocks, u):
            w = N.sd[f"{b}.mlp.1.bias"].numel()
            d[:, off:off + w] *= math.exp(float(ub))
            off += w
    return d


def bwd_cases():
    c = []
    for B in (1, 3, 9, 20):
        c.append(("small", "randn", B, None, "randn"))
        c.append(("learned", "randn", B, None, "randn"))
    c.append(("small", "hot", 9, None, "randn"))
    c.append(("learned", "hot", 20, None, "randn"))
    c.append(("fourier", "randn", 9, None, "randn"))
    for B in (3, 20):
        for df in ("randn", "wide"):
            c.append(("wide", "randn", B, None, df))
    for B in (9, 20):  # mlp_rows_wgrad_kernel with full and ragged 4-row groups, linear_wgrad_kernel / linear_dgrad_kernel
        c.append(("odd", "randn", B, None, "randn"))
    for B in (3, 9, 20):
        for m in (None, "ones", "zeros", "mixed"):
            c.append(("text", "randn", B, m, "randn"))
    c.append(("text", "hot", 9, "mixed", "randn"))
    return c


def autograd_grads(N, dtype, t, ctx, mask, dss, want_dt):
    P = N.params(dtype, grad=True)
    tt = None
    if N.lsd:  # differentiable in the weights and in t
        tt = t.to(dtype).clone().requires_grad_(True)
        e0 = uo.learned_sinusoidal_pos_emb(tt, P["time_mlp.0.weights"])
    else:
        e0 = e0_of(N, t, dtype)
    ss = chain(N, P, e0, None if ctx is None else ctx.to(dtype), mask)["ss"]
    (ss * dss.to(dtype)).sum().backward()
    g = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items()}
    return g, (tt.grad if want_dt else None)


@pytest.mark.parametrize("case", bwd_cases(), ids=case_id)
def test_cond_backward_every_gradient(case):
    kind, family, B, mk, dfam = case
    N = net(kind, family).arm()
    tk = "float" if N.lsd else "int"
    t = times(tk, B, seed=50 + B)
    ctx = seeded((B, E_TEXT), 200 + B) if N.text else None
    mask = text_mask(mk, B)
    dss = dss_of(N, dfam, B, 300 + B)
    tape, ctx_dev, mask_dev = cond_forward(N, "train", t, ctx, mask, B)
    fam = "randn" if (family, dfam) == ("randn", "randn") else "other"
    ck = Checker(case_id(case), fam, TOL_BWD)
    want, want_dt = autograd_grads(N, torch.float64, t, ctx, mask, dss, bool(N.lsd))
    floor, floor_dt = autograd_grads(N, torch.float32, t, ctx, mask, dss, bool(N.lsd))
    N.u.grads_flat().fill_(float("nan"))
    torch.cuda.synchronize()
    for acc, k in ((0, 1), (1, 2)):  # overwrite the NaNs, then accumulate on top: k times the gradient
        got, dt = cond_backward(N, tape, ctx_dev, mask_dev, dss, B, acc, bool(N.lsd))
        for name in N.head_names:
            label = f"{name} x{k}"
            frozen = name == "time_mlp.0.weights" and N.cfg.random_fourier_features
            text_off = mask is not None and int(mask.sum()) == 0 and name.startswith("text_")
            if frozen or text_off:  # exact zeros, which the code promises
                ck.exact(label, got[name], torch.zeros_like(got[name]))
                if text_off:
                    assert not bool(want[name].any())
            else:
                ck(label, got[name], k * want[name], k * floor[name])
        if dt is not None:
            ck("dt", dt, want_dt, floor_dt)
    ck.done()


def test_all_zero_mask_is_the_uncaptioned_pass_bitwise():
    """Rows with mask 0 take dtf itself as time_mlp's gradient: with every row dropped, each gradient outside the text branch
    is bit for bit that of the same pass without a caption (the strided left half of dcat against the contiguous dtf)."""
    N = net("text", "randn").arm()
    for B in (3, 9, 20):
        t, ctx, dss = times("int", B, 60 + B), seeded((B, E_TEXT), 210 + B), dss_of(N, "randn", B, 310 + B)
        ck = Checker(f"zero-mask-B{B}", "randn", TOL_BWD)
        tape0, c0, m0 = cond_forward(N, "train", t, ctx, text_mask("zeros", B), B)
        tape1, _, _ = cond_forward(N, "train", t, None, None, B)
        ck.exact("ss", tape0["ss"], tape1["ss"])
        N.u.grads_flat().fill_(float("nan"))
        g0, _ = cond_backward(N, tape0, c0, m0, dss, B, 0, False)
        N.u.grads_flat().fill_(float("nan"))
        g1, _ = cond_backward(N, tape1, None, None, dss, B, 0, False)
        for name in N.head_names:
            if not name.startswith("text_"):
                ck.exact(name, g0[name], g1[name])
        ck.done()


def test_refusals_that_need_a_handle():
    N = net("small", "randn")
    B = 3
    stream = torch.cuda.current_stream(DEV).cuda_stream
    lib = N.u._lib
    mask = torch.ones(B, dtype=torch.int32, device=DEV)
    t = times("int", B, 1).to(DEV)
    out = _lib.CondBufs(ss=_lib.ptr(nans(B, N.ss_total)))
    # a text mask without text conditioning: no caption, and a caption on a U-Net built without text
    assert lib.dm_unet_cond_forward(N.u._handle, 0, 0, _lib.ptr(t), None, _lib.ptr(mask), C.byref(out), B, stream) != 0
    assert b"text mask" in lib.dm_last_error()
    ctx = seeded((B, E_TEXT), 1).to(DEV)
    assert lib.dm_unet_cond_forward(N.u._handle, 0, 0, _lib.ptr(t), _lib.ptr(ctx), _lib.ptr(mask), C.byref(out), B, stream) != 0
    assert b"without text conditioning" in lib.dm_last_error()
    # the intermediates the inference walk fuses away, a shared time in the training walk, a float time on a fixed sinusoid
    bad = _lib.CondBufs(tact=_lib.ptr(nans(B, N.td)))
    assert lib.dm_unet_cond_forward(N.u._handle, 0, 0, _lib.ptr(t), None, None, C.byref(bad), B, stream) != 0
    assert lib.dm_unet_cond_forward(N.u._handle, 1, 2, _lib.ptr(t), None, None, C.byref(out), B, stream) != 0
    assert lib.dm_unet_cond_forward(N.u._handle, 0, 1, _lib.ptr(t), None, None, C.byref(out), B, stream) != 0


def test_unarmed_handle_refuses_the_backward():
    fresh = Net("small", "randn")
    B = 3
    tape, _, _ = cond_forward(fresh, "train", times("int", B, 1), None, None, B)
    bufs = _lib.CondBufs(**{k: _lib.ptr(v) for k, v in tape.items()})
    dss = torch.zeros(B, fresh.ss_total, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    assert fresh.u._lib.dm_unet_cond_backward(fresh.u._handle, C.byref(bufs), None, None, _lib.ptr(dss), None, B, 0, stream) != 0
    assert b"train_enable" in fresh.u._lib.dm_last_error()


# ==============================================================================================================================
# The deferred reduction tables
# ==============================================================================================================================
NORM_C = (36, 64, 96, 256, 1024)   # ragged last 64-channel blocks, every NV template (LPR = min(64, pow2ceil(C / 4)))
NORM_PIX = (16, 64, 176, 256)      # at C = 64: 1, 4, 11 and 16 chunks -- the 8-unrolled loop, its tail, both
COL_ROWS = (5, 4096, 512, 513)     # small and large alternate; the partial pass begins above 512 rows
COL_C = (4, 64, 80)


def norm_layer(C_, pix, B, with_ss, with_dbias, seed):
    L = dict(kind="norm", C=C_, pix=pix, silu=1, with_ss=with_ss, with_dbias=with_dbias)
    L["dy"], L["u"] = seeded((B * pix, C_), seed), seeded((B * pix, C_), seed + 1)
    L["g"] = 1 + 0.1 * seeded((C_,), seed + 2)
    if with_ss:  # the layer's slice of a wider row, as in the (B, ss_total) rows of the walk
        L["ss_stride"] = 2 * C_ + 8
        L["ss"] = torch.full((B, L["ss_stride"]), float("nan"))
        L["ss"][:, :2 * C_] = 0.5 * seeded((B, 2 * C_), seed + 3)
    return L


def col_layer(rows, C_, half, seed):
    L = dict(kind="col", C=C_, rows=rows, half=half)
    L["xfull"] = seeded((rows, 2 * C_ if half else C_), seed)
    return L


def norm_reference(L, B, dtype):
    C_, pix = L["C"], L["pix"]
    u = L["u"].to(dtype).reshape(B, pix, C_).clone().requires_grad_(True)
    g = L["g"].to(dtype).clone().requires_grad_(True)
    w = F.normalize(u, dim=-1) * g * math.sqrt(C_)
    ss = None
    if L["with_ss"]:
        ss = L["ss"][:, :2 * C_].to(dtype).clone().requires_grad_(True)
        w = w * (ss[:, None, :C_] + 1) + ss[:, None, C_:]
    (F.silu(w) * L["dy"].to(dtype).reshape(B, pix, C_)).sum().backward()
    o = {"du": u.grad.reshape(B * pix, C_), "dg": g.grad}
    if L["with_dbias"]:
        o["dbias"] = u.grad.sum((0, 1))
    if ss is not None:
        o["dss"] = ss.grad
    return o


def col_reference(L, dtype):
    x = L["xfull"].to(dtype)
    return {"out": (x[:, L["C"]:] if L["half"] else x).sum(0)}


def run_reduce(layers, B, deferred, accumulate, outs=None):
    """One dm_op_deferred_reduce call; outs: the output tensors of an earlier call (accumulate on top), else NaNs."""
    arr = (_lib.ReduceLayer * len(layers))()
    keep, res = [], []
    for i, L in enumerate(layers):
        R, C_ = arr[i], L["C"]
        R.C = C_
        o = {} if outs is None else outs[i]
        if L["kind"] == "norm":
            R.kind, R.silu, R.rows = _lib.REDUCE_NORM_BWD, L["silu"], L["pix"]
            d = {k: L[k].to(DEV).contiguous() for k in ("dy", "u", "g")}
            o.setdefault("du", nans(B * L["pix"], C_))
            o.setdefault("dg", nans(C_))
            if L["with_dbias"]:
                o.setdefault("dbias", nans(C_))
            if L["with_ss"]:
                d["ss"] = L["ss"].to(DEV).contiguous()
                o.setdefault("dss", nans(B, L["ss_stride"]))
                R.ss_stride = R.dss_stride = L["ss_stride"]
            for k, v in list(d.items()) + list(o.items()):
                setattr(R, k, _lib.ptr(v))
            keep.append(d)
        else:
            R.kind, R.rows = _lib.REDUCE_COLSUM, L["rows"]
            x = L["xfull"].to(DEV).contiguous()
            R.row_stride, R.col_stride = x.shape[1], 1
            R.x = _lib.ptr(x) + (4 * C_ if L["half"] else 0)
            o.setdefault("out", nans(C_))
            R.out = _lib.ptr(o["out"])
            keep.append(x)
        res.append(o)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(_lib.load().dm_op_deferred_reduce(arr, len(layers), B, deferred, accumulate, stream))
    torch.cuda.synchronize()
    return res


def check_table(label, layers, B):
    """The table against each layer alone on the immediate path (bitwise: both add the same terms in the same fixed order),
    accumulate 0 on NaNs then 1 on top, and against fp64."""
    ck = Checker(label, "randn", TOL_BWD)
    got = run_reduce(layers, B, 1, 0)
    alone2 = [run_reduce([L], B, 0, 0)[0] for L in layers]
    first, alone = ([{k: v.clone() for k, v in o.items()} for o in outs] for outs in (got, alone2))
    got2 = run_reduce(layers, B, 1, 1, got)  # (accumulates into the tensors of the first call)
    for L, o in zip(layers, alone2):
        run_reduce([L], B, 0, 1, [o])
    for i, L in enumerate(layers):
        name = (f"[{i}] norm C{L['C']} pix{L['pix']} ss{int(L['with_ss'])} db{int(L['with_dbias'])}" if L["kind"] == "norm"
                else f"[{i}] colsum rows{L['rows']} C{L['C']} half{int(L['half'])}")
        ref = norm_reference(L, B, torch.float64) if L["kind"] == "norm" else col_reference(L, torch.float64)
        flo = norm_reference(L, B, torch.float32) if L["kind"] == "norm" else col_reference(L, torch.float32)
        for k in ref:
            g1, g2 = first[i][k], got2[i][k]
            if k == "dss":  # the columns beside the layer's slice are nobody's: still NaN
                assert bool(torch.isnan(g1[:, 2 * L["C"]:]).all()), (name, "dss: a column outside the slice was written")
                g1, g2 = g1[:, :2 * L["C"]], g2[:, :2 * L["C"]]
                a1, a2 = alone[i][k][:, :2 * L["C"]], alone2[i][k][:, :2 * L["C"]]
            else:
                a1, a2 = alone[i][k], alone2[i][k]
            ck.exact(f"{name} {k} table == alone", g1, a1)
            ck.exact(f"{name} {k} table == alone, accumulated", g2, a2)
            ck(f"{name} {k}", g1, ref[k], flo[k])
            times_k = 1 if k in ("du", "dss") else 2  # du and dss are overwritten, dg / dbias / out accumulate
            ck(f"{name} {k} accumulated", g2, times_k * ref[k], times_k * flo[k])
    ck.done()


def big_table(B):
    """Every (C, pixels) norm layer -- the four (scale/shift, dbias) combinations spread so that each C and each pixel count
    meets all of them -- interleaved with every column sum: small and large ones alternate, so the stable sort that puts
    the partial-pass jobs first reorders the table; the widest layer (C = 1024) is neither first nor last."""
    norms = [norm_layer(C_, pix, B, bool((i + j) & 1), bool((i + j) & 2), 1000 + 10 * (4 * i + j))
             for i, C_ in enumerate(NORM_C) for j, pix in enumerate(NORM_PIX)]
    norms = norms[4:] + norms[:4]  # C = 36 last, C = 1024 in the middle
    cols = [col_layer(rows, C_, half, 2000 + 7 * n)
            for n, (C_, half, rows) in enumerate((C_, half, rows) for C_ in COL_C for half in (False, True) for rows in COL_ROWS)]
    cols.insert(10, col_layer(B, 1024, False, 2999))  # mem_kv-shaped: one row per image, 2 * heads * dim_head * 4 columns
    layers = []
    for i in range(max(len(norms), len(cols))):
        layers += cols[i:i + 1] + norms[i:i + 1]
    assert sum(L["kind"] == "col" for L in layers) >= 12 and layers[0]["C"] != 1024 != layers[-1]["C"]
    return layers


@pytest.mark.parametrize("B", [1, 5, 9])
def test_deferred_tables_every_shape(B):
    check_table(f"table-B{B}", big_table(B), B)


@pytest.mark.parametrize("B", [1, 5, 9])
def test_deferred_tables_of_one_and_two_jobs(B):
    n = norm_layer(96, 176, B, True, True, 11)
    for rows in (5, 513):
        c = col_layer(rows, 80, True, 12)
        check_table(f"one-colsum-rows{rows}-B{B}", [c], B)
        check_table(f"one-of-each-rows{rows}-B{B}", [n, c], B)
        check_table(f"one-of-each-reversed-rows{rows}-B{B}", [c, n], B)
    check_table(f"one-norm-B{B}", [n], B)
    check_table(f"one-norm-plain-B{B}", [norm_layer(36, 16, B, False, False, 13)], B)
