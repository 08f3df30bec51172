"""The two attention cores of the training step alone, forward and backward, through dm_op_linear_attention_core_bwd and
dm_op_attention_core_bwd: the three training-forward kernels of attention.hip and the seven backward kernels of attn_bwd.hip
with nothing in front of or behind them (no norm, no projection, no weight-gradient GEMM that averages over the tokens).

Reference.  ``linear_core`` / ``full_core`` below restate the cores in plain torch on token rows; they run in fp64 with
autograd on the same fp32 qkv / mem_kv / dout.  Checked per case: out, ctx (linear), dq, dk, dv (the column blocks of dqkv),
d_mem_k, d_mem_v, and the key statistics the backward starts from (linear: kstats[..., 0, :] is the fp64 column maximum
exactly, kstats[..., 1, :] the column sum of exp(k - max)).

Two measures per quantity: whole-tensor rel-L2, and the worst row: the error norm of one (image, head, token) row -- for ctx
one (image, head, d) row -- over the RMS row norm of the quantity in the reference.  The limit of both is the rule of
tests/test_hip_ops.py::_hard_limit with the floor of tests/test_hip_train_ops.py: max(5e-5, 4 x the error of the same torch
restatement run in fp32 against fp64), computed at run time and never from the kernel's result; every hard-input case also
asserts that the fp32 restatement itself stays within 1e-4 on every quantity (rel-L2), so that no limit goes vacuous.  Every
case prints the kernel's value next to the restatement's (run with -s).

Asserted dispatch.  The tables name, per case, the kernels the call must bracket in the profile rows (and no others): the
forward form and the backward form of full attention, the wave count of the LinearAttention context kernel.  The switches
are read once per process, so the tables carry one expectation per set of switches;
tests/test_hip_forced_dispatch.py::test_attention_backward_tiled_form_on_every_shape runs this file in two children:
  nocache  DM_ATTN_BWD_NO_CACHE = 1: the thread-per-query kernel where the score cache would be used
  tiled    DM_ATTN_BWD_TILED = DM_ATTN_TILED = 1: the tiled forward kernel and the tiled backward pair on every shape

Which case pins which kernel (default process; heads in {1, 4, 8} spread over the cases):
  attention_core_kernel<32>          n = 1, 15, 62, 63, 301, 302      attention_core_kernel<64>        n = 62, 153, 154
  attention_core_tiled_kernel<32>    n = 579 (over 320 keys)          attention_core_tiled_kernel<64>  tiled child, every n
  attn_bwd_pairs_kernel<32>          n = 1, 15, 62 (62 * 66 <= 4096)  attn_bwd_pairs_kernel<64>        n = 62
  attn_bwd_kernel<32>                n = 63, 301 (<= 160 KB of LDS)   attn_bwd_kernel<64>              n = 153
  attn_bwd_q_tiled / kv_tiled<32>    n = 302, 579 (ragged tiles)      attn_bwd_q_tiled / kv_tiled<64>  n = 154
  linattn_ctx_mfma_kernel<4, DH>     n = 1, 3, 63, 64, 65, 255        (waves 1-3 empty at n = 1, 3; one half-wave empty)
  linattn_ctx_mfma_kernel<8, DH>     n = 256, 324, 1023               (1023: the last wave is odd)
  linattn_ctx_mfma_kernel<16, DH>    n = 1024
  linattn_out_mfma / bwd_q_mfma / bwd_stats / bwd_kv_mfma<DH>: every linear case; 324 tokens are 6 blocks, so the share sum
  of linattn_bwd_stats_kernel runs its 4-way unrolled loop and its tail loop in one call (1 block at n <= 64, 2 at 65,
  4 at 255 / 256, 16 at 1023 / 1024).

Invariants: the same call twice is bit-identical on every output; the per-image outputs of images 0..B-1 of a (B + 2)-image
call equal the B-image call bit for bit and d_mem_kv is the sum of the kernel's own dmem_part to fp32 rounding; every output
is allocated with 64 canary floats on either side of a NaN payload, and after the call the payload holds no NaN and the
canaries are untouched (asserted in every case; the ragged shapes 63, 65, 302 and 1023 have a test of their own).

Measured on MI355X (worst quantity of the case: kernel | fp32 restatement, rel-L2 and worst row):
  full   (3, 1, 4, 32)     plain      rel-L2 1.7e-07 | 2.2e-07  worst row 3.3e-07 | 5.2e-07
  full   (3, 15, 8, 32)    plain      rel-L2 1.8e-07 | 1.8e-07  worst row 7.7e-07 | 7.3e-07
  full   (3, 62, 4, 32)    plain      rel-L2 2.5e-07 | 2.6e-07  worst row 1.5e-06 | 1.2e-06
  full   (3, 63, 1, 32)    plain      rel-L2 2.8e-07 | 2.8e-07  worst row 1.8e-06 | 2e-06
  full   (3, 301, 4, 32)   plain      rel-L2   4e-07 | 3.3e-07  worst row 2.5e-06 | 2.2e-06
  full   (3, 302, 8, 32)   plain      rel-L2 4.2e-07 | 3.4e-07  worst row 3.6e-06 | 3.6e-06
  full   (1, 579, 4, 32)   plain      rel-L2 6.1e-07 | 3.6e-07  worst row 2.7e-06 | 1.7e-06
  full   (3, 62, 8, 64)    plain      rel-L2   3e-07 | 3e-07    worst row 1.4e-06 | 1.6e-06
  full   (3, 153, 1, 64)   plain      rel-L2 4.1e-07 | 4.2e-07  worst row 1.4e-06 | 1.4e-06
  full   (3, 154, 4, 64)   plain      rel-L2 3.9e-07 | 3.8e-07  worst row 1.8e-06 | 1.7e-06
  linear (3, 1, 4, 32)     plain      rel-L2 2.4e-07 | 1.8e-07  worst row 6.6e-07 | 3.2e-07
  linear (3, 3, 8, 32)     plain      rel-L2 2.4e-07 | 3e-07    worst row 7.3e-07 | 1.2e-06
  linear (3, 63, 1, 32)    plain      rel-L2 2.3e-07 | 3e-07    worst row 8.6e-07 | 9.7e-07
  linear (3, 64, 4, 32)    plain      rel-L2 2.3e-07 | 2.9e-07  worst row   1e-06 | 9.9e-07
  linear (3, 65, 8, 32)    plain      rel-L2 2.3e-07 | 2.9e-07  worst row 9.7e-07 | 1.3e-06
  linear (3, 255, 1, 32)   plain      rel-L2 2.9e-07 | 3.5e-07  worst row 1.1e-06 | 9.6e-07
  linear (3, 256, 4, 32)   plain      rel-L2 2.6e-07 | 3.5e-07  worst row 1.3e-06 | 1.5e-06
  linear (3, 324, 4, 32)   plain      rel-L2 2.7e-07 | 3.8e-07  worst row 1.6e-06 | 2.1e-06
  linear (1, 1023, 8, 32)  plain      rel-L2 3.4e-07 | 3.9e-07  worst row 1.9e-06 | 2.6e-06
  linear (1, 1024, 1, 32)  plain      rel-L2 2.9e-07 | 3.9e-07  worst row 2.2e-06 | 2.5e-06
  linear (3, 1, 8, 64)     plain      rel-L2 2.9e-07 | 3e-07    worst row 6.6e-07 | 5.6e-07
  linear (3, 3, 1, 64)     plain      rel-L2 3.6e-07 | 2.5e-07  worst row 5.5e-07 | 3.7e-07
  linear (3, 63, 4, 64)    plain      rel-L2 2.6e-07 | 3.4e-07  worst row   9e-07 | 1.1e-06
  linear (3, 64, 8, 64)    plain      rel-L2 2.6e-07 | 3.3e-07  worst row 1.6e-06 | 1.4e-06
  linear (3, 65, 1, 64)    plain      rel-L2 3.1e-07 | 3.8e-07  worst row 1.5e-06 | 1.3e-06
  linear (3, 255, 4, 64)   plain      rel-L2   3e-07 | 3.8e-07  worst row 1.6e-06 | 1.8e-06
  linear (3, 256, 8, 64)   plain      rel-L2 2.8e-07 | 3.8e-07  worst row 1.4e-06 | 1.9e-06
  linear (3, 324, 1, 64)   plain      rel-L2   3e-07 | 4.3e-07  worst row 1.1e-06 | 1.6e-06
  linear (1, 1023, 1, 64)  plain      rel-L2 3.7e-07 | 4.3e-07  worst row 1.5e-06 | 1.7e-06
  linear (1, 1024, 4, 64)  plain      rel-L2 3.2e-07 | 4.2e-07  worst row 2.2e-06 | 2.1e-06
  full   (3, 62, 4, 32)    saturated  rel-L2 7.4e-06 | 7.4e-06  worst row 6.8e-05 | 6.9e-05
  full   (3, 62, 4, 32)    shift      rel-L2 1.5e-05 | 1.6e-05  worst row 6.2e-05 | 5.9e-05
  full   (3, 62, 4, 32)    dominant   rel-L2 8.1e-07 | 9.2e-07  worst row 1.3e-05 | 1.3e-05
  full   (3, 63, 1, 32)    saturated  rel-L2 7.2e-06 | 7.1e-06  worst row 6.2e-05 | 6.2e-05
  full   (3, 63, 1, 32)    shift      rel-L2 1.5e-05 | 1.6e-05  worst row 3.9e-05 | 4.4e-05
  full   (3, 63, 1, 32)    dominant   rel-L2 5.4e-07 | 7.4e-07  worst row 2.6e-06 | 3.8e-06
  full   (3, 302, 8, 32)   saturated  rel-L2   1e-05 | 1e-05    worst row 0.00019 | 0.00019
  full   (3, 302, 8, 32)   shift      rel-L2 2.3e-05 | 2.5e-05  worst row 8.7e-05 | 9.6e-05
  full   (3, 302, 8, 32)   dominant   rel-L2 8.3e-07 | 1.8e-06  worst row 1.8e-05 | 6.4e-05
  full   (3, 62, 8, 64)    saturated  rel-L2   1e-05 | 1e-05    worst row 0.00016 | 0.00016
  full   (3, 62, 8, 64)    shift      rel-L2 1.8e-05 | 1.8e-05  worst row  0.0001 | 0.0001
  full   (3, 62, 8, 64)    dominant   rel-L2 9.7e-07 | 1.1e-06  worst row   2e-05 | 2e-05
  full   (3, 153, 1, 64)   saturated  rel-L2   4e-05 | 4e-05    worst row 0.00029 | 0.00029
  full   (3, 153, 1, 64)   shift      rel-L2 2.1e-05 | 2.2e-05  worst row 6.2e-05 | 7.2e-05
  full   (3, 153, 1, 64)   dominant   rel-L2 6.3e-07 | 1.1e-06  worst row 5.9e-06 | 1.2e-05
  full   (3, 154, 4, 64)   saturated  rel-L2 1.3e-05 | 1.3e-05  worst row  0.0002 | 0.0002
  full   (3, 154, 4, 64)   shift      rel-L2 2.1e-05 | 2.2e-05  worst row 8.5e-05 | 7.8e-05
  full   (3, 154, 4, 64)   dominant   rel-L2 6.8e-07 | 8.1e-07  worst row 9.1e-06 | 1.1e-05
  linear (3, 324, 4, 32)   saturated  rel-L2 5.5e-07 | 4.3e-07  worst row 7.3e-06 | 5.5e-06
  linear (3, 324, 4, 32)   shift      rel-L2 2.6e-07 | 3.7e-07  worst row 1.3e-06 | 1.9e-06
  linear (3, 324, 4, 32)   dominant   rel-L2 3.9e-07 | 2.8e-07  worst row 1.3e-05 | 6.1e-06
  linear (3, 65, 1, 64)    saturated  rel-L2 6.1e-07 | 4.6e-07  worst row 2.5e-06 | 2.1e-06
  linear (3, 65, 1, 64)    shift      rel-L2 2.7e-07 | 3.6e-07  worst row 6.8e-07 | 1e-06
  linear (3, 65, 1, 64)    dominant   rel-L2 6.9e-07 | 3.2e-07  worst row 5.6e-06 | 1.7e-06
Before the row statistics of the full-attention backward became compensated sums the worst dq row stood at 2.4e-4 (63
tokens, shift), 3.6e-4 (302, shift) and 4.8e-4 (302, dominant), 4 to 8 times the fp32 restatement; the module-level hard-input
cases of tests/test_hip_train_ops.py (all under 1e-6) did not see it."""
import functools
import os

import pytest
import torch

from diffusion_models_amd import _lib

pytestmark = pytest.mark.gpu
FLOOR = 5e-5      # tests/test_hip_train_ops.py: fp32, another summation order
FACTOR = 4.0      # tests/test_hip_ops.py::_hard_limit
RESTATE_MAX = 1e-4
DEV = "cuda:0"
CANARY = 64
CANARY_VALUE = -7.25


def config():
    e = os.environ
    if e.get("DM_ATTN_BWD_TILED") == "1" and e.get("DM_ATTN_TILED") == "1":
        return "tiled"
    if e.get("DM_ATTN_BWD_NO_CACHE") == "1":
        return "nocache"
    return "default"


CFG = config()

# ---- the expected kernels --------------------------------------------------------------------------------------------------
# full attention: 'forward backward' per set of switches; forward: core | tiled, backward: pairs | query | tiled
FWD_ROWS = {"core": ["attention_core_kernel"], "tiled": ["attention_core_tiled_kernel"]}
BWD_ROWS = {"pairs": ["attn_bwd_pairs_kernel"], "query": ["attn_bwd_kernel"],
            "tiled": ["attn_bwd_q_tiled_kernel", "attn_bwd_kv_tiled_kernel"]}
PAIRS = dict(default="core pairs", nocache="core query", tiled="tiled tiled")
QUERY = dict(default="core query", nocache="core query", tiled="tiled tiled")
TILED = dict(default="core tiled", nocache="core tiled", tiled="tiled tiled")
LONG = dict(default="tiled tiled", nocache="tiled tiled", tiled="tiled tiled")
FULL_CASES = {
    # (B, n, heads, dh): expectation
    (3, 1, 4, 32): PAIRS,      # one query, five keys
    (3, 15, 8, 32): PAIRS,
    (3, 62, 4, 32): PAIRS,     # 62 * 66 = 4092: the last cached size
    (3, 63, 1, 32): QUERY,     # 63 * 67 = 4221: the first uncached one
    (3, 301, 4, 32): QUERY,    # 163 596 B of LDS: the last resident size
    (3, 302, 8, 32): TILED,    # 164 136 B: the first tiled one; 302 = 4 * 64 + 46 queries, 306 = 4 * 64 + 50 keys
    (1, 579, 4, 32): LONG,     # ragged query (579 = 9 * 64 + 3) and key (583 = 9 * 64 + 7) tiles
    (3, 62, 8, 64): PAIRS,
    (3, 153, 1, 64): QUERY,    # 163 036 B
    (3, 154, 4, 64): TILED,    # 164 088 B
}
# LinearAttention: waves of the context kernel (by n alone, no switch changes it)
LINEAR_CASES = {
    (3, 1, 4, 32): 4, (3, 3, 8, 32): 4, (3, 63, 1, 32): 4, (3, 64, 4, 32): 4, (3, 65, 8, 32): 4, (3, 255, 1, 32): 4,
    (3, 256, 4, 32): 8, (3, 324, 4, 32): 8, (1, 1023, 8, 32): 8, (1, 1024, 1, 32): 16,
    (3, 1, 8, 64): 4, (3, 3, 1, 64): 4, (3, 63, 4, 64): 4, (3, 64, 8, 64): 4, (3, 65, 1, 64): 4, (3, 255, 4, 64): 4,
    (3, 256, 8, 64): 8, (3, 324, 1, 64): 8, (1, 1023, 1, 64): 8, (1, 1024, 4, 64): 16,
}
# hard inputs: one shape per backward form and head width
FULL_HARD = [(3, 62, 4, 32), (3, 63, 1, 32), (3, 302, 8, 32), (3, 62, 8, 64), (3, 153, 1, 64), (3, 154, 4, 64)]
LINEAR_HARD = [(3, 324, 4, 32), (3, 65, 1, 64)]
FAMILIES = ("saturated", "shift", "dominant")
RAGGED_FULL = [(3, 63, 1, 32), (3, 302, 8, 32)]
RAGGED_LINEAR = [(3, 63, 1, 32), (3, 65, 8, 32), (3, 65, 1, 64), (1, 1023, 8, 32), (1, 1023, 1, 64)]
INVARIANT_FULL = (1, 579, 4, 32)     # tiled forward, tiled backward pair
INVARIANT_LINEAR = (3, 324, 4, 32)   # six token blocks


def expected_rows(kind, case):
    dh = case[3]
    if kind == "linear":
        names = [f"linattn_ctx_mfma_kernel<{LINEAR_CASES[case]},{dh}>"]
        names += [f"{k}<{dh}>" for k in ("linattn_out_mfma_kernel", "linattn_bwd_q_mfma_kernel", "linattn_bwd_stats_kernel",
                                         "linattn_bwd_kv_mfma_kernel")]
        return sorted(names)
    fwd, bwd = FULL_CASES[case][CFG].split()
    return sorted(f"{k}<{dh}>" for k in FWD_ROWS[fwd] + BWD_ROWS[bwd])


@pytest.fixture(scope="module", autouse=True)
def profiled():
    _lib.profile_enable(True)
    _lib.profile_read()
    yield
    _lib.profile_read()
    _lib.profile_enable(False)


# ---- the cores in plain torch ------------------------------------------------------------------------------------------------
def linear_core(qkv, mem_kv, heads, dh):
    """qkv (B, n, 3 heads dh) token rows, mem_kv (2, heads, dh, 4) -> out (B, n, heads dh), ctx (B, heads, dh, dh),
    the keys with the memory tokens in front (B, heads, dh, 4 + n)"""
    B, n, _ = qkv.shape
    q, k, v = (t.reshape(B, n, heads, dh).permute(0, 2, 3, 1) for t in qkv.chunk(3, dim=-1))
    k = torch.cat((mem_kv[0].expand(B, -1, -1, -1), k), dim=-1)
    v = torch.cat((mem_kv[1].expand(B, -1, -1, -1), v), dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", k.softmax(dim=-1), v)
    out = torch.einsum("bhde,bhdn->bhen", ctx, q.softmax(dim=-2) * dh ** -0.5)
    return out.permute(0, 3, 1, 2).reshape(B, n, heads * dh), ctx, k


def full_core(qkv, mem_kv, heads, dh):
    """qkv (B, n, 3 heads dh) token rows, mem_kv (2, heads, 4, dh) -> out (B, n, heads dh); the memory rows come first"""
    B, n, _ = qkv.shape
    q, k, v = (t.reshape(B, n, heads, dh).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    k = torch.cat((mem_kv[0].expand(B, -1, -1, -1), k), dim=-2)
    v = torch.cat((mem_kv[1].expand(B, -1, -1, -1), v), dim=-2)
    attn = (torch.einsum("bhid,bhjd->bhij", q, k) * dh ** -0.5).softmax(dim=-1)
    return torch.einsum("bhij,bhjd->bhid", attn, v).transpose(1, 2).reshape(B, n, heads * dh)


def restate(kind, qkv, mem_kv, dout, heads, dh, dtype):
    """Every checked quantity of one core from the torch restatement in `dtype`, gradients by autograd."""
    qkv = qkv.detach().to(dtype, copy=True).requires_grad_(True)
    mem_kv = mem_kv.detach().to(dtype, copy=True).requires_grad_(True)
    res = {}
    if kind == "linear":
        out, ctx, k = linear_core(qkv, mem_kv, heads, dh)
        res["ctx"] = ctx.detach()
        kmax = k.detach().amax(dim=-1)
        res["kmax"], res["ksum"] = kmax, (k.detach() - kmax[..., None]).exp().sum(dim=-1)
    else:
        out = full_core(qkv, mem_kv, heads, dh)
    out.backward(dout.to(dtype))
    hid = heads * dh
    res["out"] = out.detach()
    res["dq"], res["dk"], res["dv"] = (qkv.grad[..., i * hid:(i + 1) * hid] for i in range(3))
    res["d_mem_k"], res["d_mem_v"] = mem_kv.grad[0], mem_kv.grad[1]
    return res


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def seeded(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def make_inputs(kind, case, family, seed=1):
    """plain: unit-scale randn.  saturated: q and k x 8, mem_kv x 4.  shift: k + 100 on every token and memory key (the
    softmax must not change; a recomputation that forgets the maximum overflows).  dominant: +30 on the columns d < dh / 2 of
    head 0 of k at token n / 2 and of q at token n / 3 (not on every d: a constant shift of a whole k row cancels in dq)."""
    B, n, heads, dh = case
    hid = heads * dh
    qkv = seeded((B, n, 3 * hid), seed)
    mem = seeded((2, heads, dh, 4) if kind == "linear" else (2, heads, 4, dh), seed + 1)
    dout = seeded((B, n, hid), seed + 2)
    if family == "saturated":
        qkv[..., :2 * hid] *= 8
        mem *= 4
    elif family == "shift":
        qkv[..., hid:2 * hid] += 100
        mem[0] += 100
    elif family == "dominant":
        qkv[:, n // 2, hid:hid + dh // 2] += 30
        qkv[:, n // 3, :dh // 2] += 30
    else:
        assert family == "plain"
    return qkv, mem, dout


# ---- the call --------------------------------------------------------------------------------------------------------------------
class Guarded:
    """A device output with CANARY floats before and after a NaN payload."""

    def __init__(self, shape):
        self.shape = tuple(shape)
        self.n = int(torch.Size(self.shape).numel())
        self.buf = torch.full((self.n + 2 * CANARY,), CANARY_VALUE, device=DEV)
        self.buf[CANARY:CANARY + self.n] = float("nan")

    def ptr(self):
        return self.buf.data_ptr() + 4 * CANARY

    def read(self):
        """(payload on the CPU, canaries intact)"""
        h = self.buf.cpu()
        ok = bool((h[:CANARY] == CANARY_VALUE).all() and (h[CANARY + self.n:] == CANARY_VALUE).all())
        return h[CANARY:CANARY + self.n].reshape(self.shape).clone(), ok


def run_core(kind, qkv, mem_kv, dout, heads, dh):
    """-> ({name: CPU tensor} of every output of the operator, canaries intact, sorted profile rows of the call)"""
    B, n, _ = qkv.shape
    hid = heads * dh
    mem_shape = tuple(mem_kv.shape)
    outs = {"out": Guarded((B, n, hid))}
    if kind == "linear":
        outs["ctx"] = Guarded((B, heads, dh, dh))
        outs["kstats"] = Guarded((B, heads, 2, dh))
    outs["dqkv"] = Guarded((B, n, 3 * hid))
    outs["dmem_part"] = Guarded((B,) + mem_shape)
    outs["d_mem_kv"] = Guarded(mem_shape)
    ins = [t.to(DEV).contiguous() for t in (qkv, mem_kv, dout)]
    lib = _lib.load()
    fn = lib.dm_op_linear_attention_core_bwd if kind == "linear" else lib.dm_op_attention_core_bwd
    _lib.profile_read()
    _lib.check(fn(*[_lib.ptr(t) for t in ins], *[g.ptr() for g in outs.values()], B, n, heads, dh, None))
    rows = sorted(r["kernel"] for r in _lib.profile_read())
    got, intact = {}, True
    for name, g in outs.items():
        got[name], ok = g.read()
        intact = intact and ok
    return got, intact, rows


def quantities(kind, got, heads, dh):
    """The checked quantities out of the operator's outputs, named as restate() names them."""
    hid = heads * dh
    q = {"out": got["out"], "d_mem_k": got["d_mem_kv"][0], "d_mem_v": got["d_mem_kv"][1]}
    q["dq"], q["dk"], q["dv"] = (got["dqkv"][..., i * hid:(i + 1) * hid] for i in range(3))
    if kind == "linear":
        q["ctx"], q["kmax"], q["ksum"] = got["ctx"], got["kstats"][:, :, 0], got["kstats"][:, :, 1]
    return q


def as_rows(kind, name, t, dh):
    """(rows, dh): one row per (image, head, token); ctx: per (image, head, d); the statistics: per (image, head)"""
    if kind == "linear" and name in ("d_mem_k", "d_mem_v"):
        t = t.transpose(-1, -2)  # (heads, dh, 4) -> (heads, 4, dh)
    return t.reshape(-1, dh)


def measures(kind, name, got, ref, dh):
    """(whole-tensor rel-L2, worst row error norm / RMS row norm of the reference)"""
    g, r = as_rows(kind, name, got.double(), dh), as_rows(kind, name, ref.double(), dh)
    d = g - r
    rms_row = r.pow(2).sum(dim=1).mean().sqrt().clamp_min(1e-300)
    return float(d.norm() / r.norm().clamp_min(1e-300)), float(d.pow(2).sum(dim=1).sqrt().max() / rms_row)


@functools.lru_cache(maxsize=None)
def case_result(kind, case, family):
    """(inputs, fp64 reference, fp32 restatement, operator outputs, canaries intact, profile rows), computed once"""
    _, _, heads, dh = case
    ins = make_inputs(kind, case, family)
    ref64 = restate(kind, *ins, heads, dh, torch.float64)
    ref32 = restate(kind, *ins, heads, dh, torch.float32)
    got, intact, rows = run_core(kind, *ins, heads, dh)
    return ins, ref64, ref32, got, intact, rows


def check_case(kind, case, family):
    _, _, heads, dh = case
    _, ref64, ref32, got, intact, rows = case_result(kind, case, family)
    label = f"attn_cores[{CFG}] {kind} {case} {family}"
    assert rows == expected_rows(kind, case), (label, rows)
    assert intact, (label, "a canary was overwritten")
    bad = [(name, int(torch.isnan(t).sum())) for name, t in got.items() if not torch.isfinite(t).all()]
    assert not bad, (label, "not finite (an unwritten or poisoned element)", bad)
    q = quantities(kind, got, heads, dh)
    fails, worst = [], [0.0, 0.0, 0.0, 0.0]
    for name in sorted(ref64):
        if name == "kmax":
            if not torch.equal(q["kmax"].double(), ref64["kmax"]):
                fails.append(("kmax", "not the exact column maximum"))
            continue
        e = measures(kind, name, q[name], ref64[name], dh)
        f = measures(kind, name, ref32[name], ref64[name], dh)
        lim = [max(FLOOR, FACTOR * f[0]), max(FLOOR, FACTOR * f[1])]
        print(f"{label} {name}: rel-L2 kernel {e[0]:.3g} fp32 {f[0]:.3g} limit {lim[0]:.3g} | worst row kernel {e[1]:.3g} "
              f"fp32 {f[1]:.3g} limit {lim[1]:.3g}")
        worst = [max(a, b) for a, b in zip(worst, (e[0], f[0], e[1], f[1]))]
        if family != "plain" and f[0] > RESTATE_MAX:
            fails.append((name, "the fp32 restatement itself is off", f))
        if not (e[0] <= lim[0] and e[1] <= lim[1]):
            fails.append((name, e, lim))
    print(f"{label} WORST: rel-L2 kernel {worst[0]:.2g} | fp32 {worst[1]:.2g}; worst row kernel {worst[2]:.2g} | fp32 {worst[3]:.2g}")
    assert not fails, (label, fails)


@pytest.mark.parametrize("case", list(FULL_CASES))
def test_attention_core(case):
    check_case("full", case, "plain")


@pytest.mark.parametrize("case", list(LINEAR_CASES))
def test_linear_attention_core(case):
    check_case("linear", case, "plain")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", FULL_HARD)
def test_attention_core_hard_inputs(case, family):
    check_case("full", case, family)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", LINEAR_HARD)
def test_linear_attention_core_hard_inputs(case, family):
    check_case("linear", case, family)


# ---- invariants ------------------------------------------------------------------------------------------------------------------
INVARIANTS = [("full", INVARIANT_FULL), ("linear", INVARIANT_LINEAR)]


@pytest.mark.parametrize("kind,case", INVARIANTS)
def test_same_call_twice_is_bitwise_identical(kind, case):
    """attn_bwd.hip: 'a fixed summation order (no atomics)'."""
    ins, _, _, got, _, rows = case_result(kind, case, "plain")
    again, intact, rows2 = run_core(kind, *ins, case[2], case[3])
    assert intact and rows2 == rows == expected_rows(kind, case)
    for name in got:
        assert torch.equal(again[name], got[name]), name


@pytest.mark.parametrize("kind,case", INVARIANTS)
def test_image_does_not_depend_on_the_batch_around_it(kind, case):
    """Images 0..B-1 of a (B + 2)-image call equal the B-image call bit for bit on every per-image output, and d_mem_kv is
    the sum of the kernel's own per-image shares: B fp32 additions, each within 2^-24 of the running sum."""
    B, n, heads, dh = case
    (qkv, mem, dout), _, _, got, _, _ = case_result(kind, case, "plain")
    extra = make_inputs(kind, (2, n, heads, dh), "plain", seed=7)
    more, intact, rows = run_core(kind, torch.cat([qkv, extra[0]]), mem, torch.cat([dout, extra[2]]), heads, dh)
    assert intact and rows == expected_rows(kind, case)
    for name in got:
        if name != "d_mem_kv":
            assert torch.equal(more[name][:B], got[name]), name
    for res, nb in ((got, B), (more, B + 2)):
        part = res["dmem_part"].double()
        bound = nb * 2.0 ** -24 * part.abs().sum(dim=0)
        assert bool(((res["d_mem_kv"].double() - part.sum(dim=0)).abs() <= bound).all()), nb


@pytest.mark.parametrize("kind,case", [("full", c) for c in RAGGED_FULL] + [("linear", c) for c in RAGGED_LINEAR])
def test_written_exactly_once_nowhere_else(kind, case):
    """Ragged token counts (63, 65, 302, 1023): every element of every output is written -- the payload was NaN -- and the
    64 floats on either side of every output are untouched."""
    _, _, _, got, intact, _ = case_result(kind, case, "plain")
    assert intact
    for name, t in got.items():
        assert not torch.isnan(t).any(), name


def test_every_kernel_is_pinned_by_a_case():
    """Every training kernel of attention.hip and attn_bwd.hip stands in the expectation of at least one case of the tables
    under the default switches."""
    names = set()
    for kind, table in (("full", FULL_CASES), ("linear", LINEAR_CASES)):
        for case in table:
            if kind == "linear":
                names |= set(expected_rows(kind, case))
            else:
                fwd, bwd = table[case]["default"].split()
                names |= {f"{k}<{case[3]}>" for k in FWD_ROWS[fwd] + BWD_ROWS[bwd]}
    want = {f"linattn_ctx_mfma_kernel<{w},{dh}>" for w in (4, 8, 16) for dh in (32, 64)}
    want |= {f"{k}<{dh}>" for dh in (32, 64) for k in (
        "linattn_out_mfma_kernel", "linattn_bwd_q_mfma_kernel", "linattn_bwd_stats_kernel", "linattn_bwd_kv_mfma_kernel",
        "attention_core_kernel", "attn_bwd_pairs_kernel", "attn_bwd_kernel", "attn_bwd_q_tiled_kernel",
        "attn_bwd_kv_tiled_kernel")}
    want.add("attention_core_tiled_kernel<32>")
    assert want <= names, sorted(want - names)
