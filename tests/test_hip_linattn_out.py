"""The head-sum form of the fused LinearAttention output kernel (linattn_fused.hip, linattn_out_headsum_kernel): the
waves exchange the softmaxed queries p through LDS, the sum over heads z = sum_h M_h p_h runs as one MFMA chain per
output column tile, and a workgroup walks a run of token windows of one image with its operands in registers.

Called through dm_op_linear_attention like tests/test_hip_linattn_image.py and compared with
oracle.unet_oracle.linear_attention at that file's limit (fp32, another summation order: rel-L2 < 2e-5).  Every case
reads the profile rows back and asserts which form of kernel 2 ran.

Shapes, for the ways this kernel can go wrong (windows are 64 tokens at C = 64 and 32 at C = 128, tiles 32 tokens; at
the batch of these tests an image is cut into two runs of ceil(windows / 2) windows):
  (64, 2x2)    4 tokens: one partial tile, the second tile of the window empty
  (64, 3x11)   33 tokens: a full tile plus one token
  (64, 6x10)   60 tokens, ragged inside one window
  (128, 8x8)   64 tokens, exact
  (128, 9x13)  117 tokens, ragged, four column tiles
  (128, 15x20) 300 tokens: ten windows, the last one ragged
  (64, 24x24)  576 tokens = 9 windows (an odd count): both LDS windows reused, the run boundary inside the image
  (64, 3x43)   129 tokens: one token past the first run, the second workgroup of an image owns that token alone
  (128, 3x11)  33 tokens: the same at C = 128"""
import functools

import pytest
import torch

import diffusion_models_amd as dm
from diffusion_models_amd import _lib
from diffusion_models_amd.spec import UnetConfig
from oracle import unet_oracle as uo

from conftest import rel_l2

pytestmark = pytest.mark.gpu
TOL = 2e-5
FWD_TOL = 1e-4  # the forward limit of tests/test_hip_model.py
DEV = "cuda:0"
B_NEW = 256  # the dispatch rule of launch_c selects the head-sum form from B = 32 on, for every shape
SHAPES = [(64, 2, 2), (64, 3, 11), (64, 6, 10), (128, 8, 8), (128, 9, 13), (128, 15, 20), (64, 24, 24), (64, 3, 43),
          (128, 3, 11)]
HEADSUM, BLOCKED = "linattn_out_headsum_kernel", "linattn_out_fused_kernel"


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


def assert_headsum_form(rows):
    assert HEADSUM in rows and BLOCKED not in rows, rows


@functools.lru_cache(maxsize=None)
def case(shape):
    """(state dict, x, oracle output, kernel output, profile rows) of one shape at B_NEW, computed once"""
    Cc, H, W = shape
    sd = attn_sd(Cc)
    x = seeded((B_NEW, Cc, H, W), 1)
    ref = uo.linear_attention(sd, "a", x, 4, 32)
    out, rows = run(sd, x)
    return sd, x, ref, out, rows


@pytest.mark.parametrize("shape", SHAPES)
def test_headsum_form_matches_oracle(shape):
    _, _, ref, out, rows = case(shape)
    assert_headsum_form(rows)
    err = rel_l2(out, ref)
    print(f"linattn out {shape}: rel-L2 {err:.3g}")
    assert err < TOL


# x scaled by 8, mem_kv by 4 (test_hip_ops.py::test_linear_attention_hard_inputs): the fp64 oracle is the reference and
# the limit is that test's rule, max(TOL, 4 x the fp32 oracle's own error against fp64).  One shape per C.
@pytest.mark.parametrize("shape", [(64, 6, 10), (128, 9, 13)])
def test_headsum_form_hard_inputs(shape):
    Cc, H, W = shape
    sd = attn_sd(Cc)
    sd["a.mem_kv"] = sd["a.mem_kv"] * 4
    x = seeded((B_NEW, Cc, H, W), 1, 8.0)
    ref = uo.linear_attention({k: v.double() for k, v in sd.items()}, "a", x.double(), 4, 32)
    lim = max(TOL, 4 * rel_l2(uo.linear_attention(sd, "a", x, 4, 32), ref))
    out, rows = run(sd, x)
    assert_headsum_form(rows)
    err = rel_l2(out, ref)
    print(f"linattn out hard {shape}: kernel {err:.3g}  limit {lim:.3g}")
    assert err <= lim


@pytest.mark.parametrize("shape", [(64, 24, 24), (128, 9, 13)])
def test_same_call_twice_is_bitwise_identical(shape):
    sd, x, _, out, _ = case(shape)
    again, rows = run(sd, x)
    assert_headsum_form(rows)
    assert torch.equal(again, out)


@pytest.mark.parametrize("shape", [(64, 24, 24), (128, 9, 13)])
def test_image_does_not_depend_on_the_batch_around_it(shape):
    """The first 256 images of a 260-image call equal the 256-image call bit for bit (both batches are on the head-sum
    form's side of the rule)."""
    Cc, H, W = shape
    sd, x, _, out, _ = case(shape)
    more = torch.cat([x, seeded((4, Cc, H, W), 2)])
    out260, rows = run(sd, more)
    assert_headsum_form(rows)
    assert torch.equal(out260[:B_NEW], out)


@pytest.mark.parametrize("shape", [(64, 16, 16), (128, 9, 13)])
def test_small_batch_keeps_the_blocked_kernel(shape):
    Cc, H, W = shape
    sd = attn_sd(Cc)
    x = seeded((2, Cc, H, W), 1)
    out, rows = run(sd, x)
    assert BLOCKED in rows and HEADSUM not in rows, rows
    assert rel_l2(out, uo.linear_attention(sd, "a", x, 4, 32)) < TOL


def test_unet_forward_adds_the_residual():
    """dm_op_linear_attention calls the layer with add_x = 0; inside the U-Net it runs as attn(x) + x.  One forward of
    a small U-Net whose LinearAttention stages have C = 64 and C = 128 (8x8 and 4x4 maps), against the oracle."""
    cfg = UnetConfig(dim=64, dim_mults=(1, 2), channels=3)
    sd = dm.synth_state_dict(dm.unet_param_spec(cfg), salt=1)
    unet = dm.Unet(dim=64, dim_mults=(1, 2), channels=3, device=DEV)
    unet.load_state_dict(sd)
    x = seeded((B_NEW, 3, 8, 8), 3)
    t = torch.randint(0, 1000, (B_NEW,), generator=torch.Generator().manual_seed(4))
    _lib.profile_read()
    y = unet(x.to(DEV), t.to(DEV)).cpu()
    rows = [r["kernel"] for r in _lib.profile_read()]
    assert_headsum_form(rows)
    with torch.inference_mode():
        ref = uo.unet_forward(sd, cfg, x, t)
    err = rel_l2(y, ref)
    print(f"unet forward with the head-sum form: rel-L2 {err:.3g}")
    assert err < FWD_TOL
