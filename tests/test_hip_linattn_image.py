"""The per-image form of the fused LinearAttention context kernel (linattn_fused.hip, linattn_ctx_image_kernel): one
workgroup walks all tokens of its image, W_v is applied to the accumulated P^T once per image, and the same workgroup
finishes the image (halves combined, memory tokens, denominators, M = W_out ctx^T), so no reduce launch follows.

Called through dm_op_linear_attention like tests/test_hip_ops.py::test_linear_attention and compared with
oracle.unet_oracle.linear_attention at that file's limit (fp32, another summation order: rel-L2 < 2e-5).  Every case
reads the profile rows back and asserts which form of kernel 1 ran.

Shapes, for the ways this kernel can go wrong (token windows are 128 rows, tiles 32 tokens, wave = (head, token half)):
  (64, 2x2)    4 tokens: one partial tile, the second token half empty, the memory tokens dominate
  (64, 6x10)   60 tokens, ragged inside one window
  (128, 9x13)  117 tokens, ragged, four column tiles
  (128, 15x20) 300 tokens: three windows, the last one ragged
  (64, 24x24)  576 tokens: five windows (an odd count), both LDS windows reused
  (64, 16x16)  256 tokens, an exact multiple"""
import functools

import pytest
import torch

from diffusion_models_amd import _lib
from oracle import unet_oracle as uo

from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 2e-5
DEV = "cuda:0"
B_IMAGE = 256  # the dispatch rule of launch_c selects the per-image form at this batch for every shape below
SHAPES = [(64, 2, 2), (64, 6, 10), (128, 9, 13), (128, 15, 20), (64, 24, 24), (64, 16, 16)]
IMAGE, BLOCKED, REDUCE = "linattn_ctx_image_kernel", "linattn_ctx_fused_kernel", "linattn_ctx_reduce_kernel"


@pytest.fixture(scope="module", autouse=True)
def profiled():
    _lib.profile_enable(True)
    _lib.profile_read()
    yield
    _lib.profile_read()
    _lib.profile_enable(False)


def seeded(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def attn_sd(Cc, seed=10):
    hid = 128
    return {
        "a.norm.g": 1 + 0.3 * seeded((1, Cc, 1, 1), seed),
        "a.mem_kv": seeded((2, 4, 32, 4), seed + 1),
        "a.to_qkv.weight": seeded((3 * hid, Cc, 1, 1), seed + 2, Cc ** -0.5),
        "a.to_out.0.weight": seeded((Cc, hid, 1, 1), seed + 3, hid ** -0.5),
        "a.to_out.0.bias": seeded((Cc,), seed + 4, 0.1),
        "a.to_out.1.g": 1 + 0.3 * seeded((1, Cc, 1, 1), seed + 5),
    }


def run(sd, x):
    """(output on the CPU, names of the profile rows of this call)"""
    B, Cc, H, W = x.shape
    out = torch.empty(x.shape, device=DEV)
    a = [sd[k].to(DEV).contiguous() for k in ("a.norm.g", "a.mem_kv", "a.to_qkv.weight", "a.to_out.0.weight",
                                              "a.to_out.0.bias", "a.to_out.1.g")]
    xd = x.to(DEV).contiguous()
    _lib.profile_read()
    _lib.check(_lib.load().dm_op_linear_attention(_lib.ptr(xd), *[_lib.ptr(t) for t in a], _lib.ptr(out), B, Cc, H, W,
                                                  4, 32, None))
    rows = [r["kernel"] for r in _lib.profile_read()]
    return out.cpu(), rows


def assert_image_form(rows):
    assert IMAGE in rows and REDUCE not in rows and BLOCKED not in rows, rows


@functools.lru_cache(maxsize=None)
def case(shape):
    """(state dict, x, oracle output, kernel output, profile rows) of one shape at B_IMAGE, computed once"""
    Cc, H, W = shape
    sd = attn_sd(Cc)
    x = seeded((B_IMAGE, Cc, H, W), 1)
    ref = uo.linear_attention(sd, "a", x, 4, 32)
    out, rows = run(sd, x)
    return sd, x, ref, out, rows


@pytest.mark.parametrize("shape", SHAPES)
def test_image_form_matches_oracle(shape):
    _, _, ref, out, rows = case(shape)
    assert_image_form(rows)
    err = rel_l2(out, ref)
    print(f"linattn image {shape}: rel-L2 {err:.3g}")
    assert err < TOL


# x scaled by 8, mem_kv by 4 (test_hip_ops.py::test_linear_attention_hard_inputs): the fp64 oracle is the reference and
# the limit is that test's rule, max(TOL, 4 x the fp32 oracle's own error against fp64).  One shape per C.
@pytest.mark.parametrize("shape", [(64, 6, 10), (128, 9, 13)])
def test_image_form_hard_inputs(shape):
    Cc, H, W = shape
    sd = attn_sd(Cc)
    sd["a.mem_kv"] = sd["a.mem_kv"] * 4
    x = seeded((B_IMAGE, Cc, H, W), 1, 8.0)
    ref = uo.linear_attention({k: v.double() for k, v in sd.items()}, "a", x.double(), 4, 32)
    lim = max(TOL, 4 * rel_l2(uo.linear_attention(sd, "a", x, 4, 32), ref))
    out, rows = run(sd, x)
    assert_image_form(rows)
    err = rel_l2(out, ref)
    print(f"linattn image hard {shape}: kernel {err:.3g}  limit {lim:.3g}")
    assert err <= lim


@pytest.mark.parametrize("shape", [(64, 24, 24), (128, 9, 13)])
def test_same_call_twice_is_bitwise_identical(shape):
    sd, x, _, out, _ = case(shape)
    again, rows = run(sd, x)
    assert_image_form(rows)
    assert torch.equal(again, out)


@pytest.mark.parametrize("shape", [(64, 24, 24), (128, 9, 13)])
def test_image_does_not_depend_on_the_batch_around_it(shape):
    """The first 256 images of a 260-image call equal the 256-image call bit for bit."""
    Cc, H, W = shape
    sd, x, _, out, _ = case(shape)
    more = torch.cat([x, seeded((4, Cc, H, W), 2)])
    out260, rows = run(sd, more)
    assert_image_form(rows)
    assert torch.equal(out260[:B_IMAGE], out)


def test_small_batch_keeps_the_blocked_kernel_and_the_reduce():
    sd = attn_sd(64)
    x = seeded((2, 64, 16, 16), 1)
    out, rows = run(sd, x)
    assert BLOCKED in rows and REDUCE in rows and IMAGE not in rows, rows
    assert rel_l2(out, uo.linear_attention(sd, "a", x, 4, 32)) < TOL
