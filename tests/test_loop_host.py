"""The host helpers every sampling loop and loss call goes through (diffusion_models_amd/_loop.py), on CPU stubs and without
the library: which noise slots an injected ``noise`` callable is called for, in which order and where its tensors land; the
Philox start image when there is no callable; the tail of a loss call; the two shape-mismatch errors of its input half."""
import ctypes as C
import types

import pytest
import torch

from diffusion_models_amd import _lib, _loop

SHAPE = (2, 3, 4, 4)
STREAM = 0x5EED


class Recorder:
    """``noise(shape)``: call k returns a tensor filled with k + 1."""

    def __init__(self):
        self.calls = 0

    def __call__(self, shape):
        self.calls += 1
        return torch.full(shape, float(self.calls))


class Stub:
    """What the helpers read from a diffusion object."""
    device = "cpu"
    channels = 3
    model = types.SimpleNamespace(downsample_factor=2, _handle=None)

    def __init__(self):
        self.randn_calls = []

    def _randn(self, shape, seed, draw, sample_offset):
        self.randn_calls.append((tuple(shape), seed, draw, sample_offset))
        return torch.full(tuple(shape), -1.0)

    def _stream(self):
        return STREAM


def test_flag_vector_draws_in_order_and_leaves_zeros():
    noise = Recorder()
    seed, x_T, rows = _loop.loop_start(Stub(), SHAPE, noise, 7, 0, [True, True, False])
    assert seed == 7 and noise.calls == 3
    assert torch.equal(x_T, torch.full(SHAPE, 1.0))  # the first call is the start image
    assert rows.shape == (3,) + SHAPE and rows.dtype == torch.float32 and rows.is_contiguous()
    assert torch.equal(rows[0], torch.full(SHAPE, 2.0)) and torch.equal(rows[1], torch.full(SHAPE, 3.0))
    assert torch.equal(rows[2], torch.zeros(SHAPE))


def test_slot_array_is_walked_row_major():
    slots = torch.tensor([[False, True, True], [True, False, True], [True, True, False]])  # rows of [jump, known, step]
    noise = Recorder()
    _, x_T, rows = _loop.loop_start(Stub(), SHAPE, noise, 7, 0, slots)
    assert noise.calls == 1 + int(slots.sum()) and torch.equal(x_T, torch.full(SHAPE, 1.0))
    assert rows.shape == (3, 3) + SHAPE and rows.dtype == torch.float32
    # every slot holds one value: the number of the call that filled it, 0 where there was none
    filled = [[rows[r, k].unique().item() for k in range(3)] for r in range(3)]
    assert filled == [[0.0, 2.0, 3.0], [4.0, 0.0, 5.0], [6.0, 7.0, 0.0]]
    for r in range(3):
        for k in range(3):
            if not slots[r, k]:
                assert torch.equal(rows[r, k], torch.zeros(SHAPE))


def test_float_time_form_without_rows_gives_none():
    noise = Recorder()
    _, x_T, rows = _loop.loop_start(Stub(), SHAPE, noise, 7, 0, [True] * 0)
    assert noise.calls == 1 and rows is None and torch.equal(x_T, torch.full(SHAPE, 1.0))
    noise = Recorder()
    _, _, rows = _loop.loop_start(Stub(), SHAPE, noise, 7, 0, [True] * 2)  # unconditional draws
    assert noise.calls == 3 and rows.shape == (2,) + SHAPE
    assert torch.equal(rows[0], torch.full(SHAPE, 2.0)) and torch.equal(rows[1], torch.full(SHAPE, 3.0))


def test_given_start_image_is_not_drawn():
    noise = Recorder()
    x_init = torch.full(SHAPE, 9.0, dtype=torch.float64)
    _, x_T, rows = _loop.loop_start(Stub(), SHAPE, noise, 7, 0, [True, False], x_init=x_init)
    assert noise.calls == 1 and x_T.dtype == torch.float32 and torch.equal(x_T, torch.full(SHAPE, 9.0))
    assert torch.equal(rows[0], torch.full(SHAPE, 1.0)) and torch.equal(rows[1], torch.zeros(SHAPE))
    stub = Stub()
    _, x_T, rows = _loop.loop_start(stub, SHAPE, None, 7, 0, [True, False], x_init=x_init)
    assert stub.randn_calls == [] and rows is None and torch.equal(x_T, torch.full(SHAPE, 9.0))


def test_without_a_callable_the_start_image_is_philox_draw_0():
    stub = Stub()
    seed, x_T, rows = _loop.loop_start(stub, SHAPE, None, 7, 5, [True, True, False])
    assert stub.randn_calls == [(SHAPE, 7, 0, 5)]  # draw index 0 at the passed sample_offset
    assert seed == 7 and rows is None and torch.equal(x_T, torch.full(SHAPE, -1.0))
    torch.manual_seed(3)
    want = _lib.default_seed()
    torch.manual_seed(3)
    assert _loop.loop_start(stub, SHAPE, None, None, 0, [])[0] == want  # seed=None: torch's global CPU generator


def test_loop_start_shape_asserts():
    with pytest.raises(AssertionError, match="initial state .* does not match"):
        _loop.loop_start(Stub(), SHAPE, None, 7, 0, [], x_init=torch.zeros(2, 3, 4, 2))
    calls = iter([SHAPE, (2, 3, 4, 2), (2, 3, 4, 2)])
    with pytest.raises(AssertionError, match=r"noise\(\) must return tensors of the sampled shape"):
        _loop.loop_start(Stub(), SHAPE, lambda shape: torch.zeros(next(calls)), 7, 0, [True, True])


def test_checked_shape():
    assert _loop.checked_shape(Stub(), [2, 3, torch.tensor(4), 6]) == (2, 3, 4, 6)
    with pytest.raises(AssertionError, match="shape has 4 channels, the model 3"):
        _loop.checked_shape(Stub(), (2, 4, 4, 4))
    with pytest.raises(AssertionError, match="the sides must be divisible by 2"):
        _loop.checked_shape(Stub(), (2, 3, 4, 5))


def test_loss_call_sync_returns_the_host_value_and_sets_the_stream():
    seen = []

    def entry(handle, ref):
        a = ref._obj
        seen.append((handle, a.stream, bool(a.loss_out_host)))
        a.loss_out_host[0] = 1.5
        return 0

    val = _loop.loss_call(Stub(), 0xABC, entry, _lib.LvTrainArgs(), True)
    assert seen == [(0xABC, STREAM, True)]
    assert val.device.type == "cpu" and val.dim() == 0 and val.dtype == torch.float32 and float(val) == 1.5


def test_loss_call_without_sync_reads_the_device_scalar():
    stub, seen = Stub(), []

    def entry(handle, ref):
        seen.append(bool(ref._obj.loss_out_host))
        return 0

    def train_scalar(handle, which, out_ptr, stream):
        seen.append((handle, which, stream))
        C.c_float.from_address(out_ptr).value = 2.5
        return 0

    stub._lib = types.SimpleNamespace(dm_unet_train_scalar=train_scalar)
    val = _loop.loss_call(stub, 0xABC, entry, _lib.WoTrainArgs(), False)
    assert seen == [False, (0xABC, 0, STREAM)]  # no host pointer; the scalar is read on the stream the helper set
    assert val.dim() == 0 and val.dtype == torch.float32 and float(val) == 2.5


def test_loss_inputs_defaults_and_mismatch_errors():
    stub = Stub()
    x = torch.zeros(SHAPE, dtype=torch.float64)
    t = torch.zeros(2, dtype=torch.long)
    xs, noise = _loop.loss_inputs(stub, x, t, None)
    assert xs.dtype == torch.float32 and torch.equal(noise, torch.full(SHAPE, -1.0))
    assert len(stub.randn_calls) == 1 and stub.randn_calls[0][0] == SHAPE and stub.randn_calls[0][2:] == (0, 0)
    given = torch.ones(SHAPE)
    assert torch.equal(_loop.loss_inputs(stub, x, t, given)[1], given) and len(stub.randn_calls) == 1
    with pytest.raises(RuntimeError, match=r"x_start \(2, 4, 4, 4\): expected 3 channels and sides divisible by 2"):
        _loop.loss_inputs(stub, torch.zeros(2, 4, 4, 4), t, None)
    with pytest.raises(RuntimeError, match=r"noise \(2, 3, 4, 2\) / t \(2 entries\) do not match x_start \(2, 3, 4, 4\)"):
        _loop.loss_inputs(stub, x, t, torch.zeros(2, 3, 4, 2))
    with pytest.raises(RuntimeError, match=r"noise \(2, 3, 4, 4\) / t \(3 entries\) do not match x_start \(2, 3, 4, 4\)"):
        _loop.loss_inputs(stub, x, torch.zeros(3, dtype=torch.long), given)
