"""The conditioning-head and deferred-reduction entry points on the host: declared, bound, and refusing bad arguments before
anything touches a device (no GPU here; the refusals that need a handle are in tests/test_hip_cond_ops.py)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
from diffusion_models_amd import _lib

NEW = ("dm_unet_cond_forward", "dm_unet_cond_backward", "dm_op_deferred_reduce")


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_new_exports_are_declared_and_bound_with_the_header_arity():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == len(_prototype(name)), name


def test_struct_layouts_match_the_header():
    # dm_cond_bufs: ten pointers; dm_reduce_layer: six int32, three int64, ten pointers, no padding
    assert C.sizeof(_lib.CondBufs) == 10 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.ReduceLayer) == 6 * 4 + 3 * 8 + 10 * C.sizeof(C.c_void_p)
    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    body = re.search(r"typedef struct dm_cond_bufs \{(.*?)\} dm_cond_bufs;", src, flags=re.S).group(1)
    assert re.findall(r"\*(\w+)", body) == [n for n, _ in _lib.CondBufs._fields_]
    body = re.search(r"typedef struct dm_reduce_layer \{(.*?)\} dm_reduce_layer;", src, flags=re.S).group(1)
    assert re.findall(r"[\s*](\w+)[,;]", body) == [n for n, _ in _lib.ReduceLayer._fields_]


def _refused(rc, *words):
    msg = _lib.load().dm_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def test_null_handle_and_null_arguments_are_refused():
    lib = _lib.load()
    bufs = _lib.CondBufs()
    t = (C.c_int64 * 2)(1, 2)
    _refused(lib.dm_unet_cond_forward(None, 0, 0, C.addressof(t), None, None, C.byref(bufs), 2, None), "null")
    _refused(lib.dm_unet_cond_backward(None, C.byref(bufs), None, None, C.addressof(t), None, 2, 0, None), "null")
    _refused(lib.dm_op_deferred_reduce(None, 1, 2, 1, 0, None), "bad argument")


@pytest.mark.parametrize("C_", [0, 6, 63, 1028])
def test_norm_layer_widths_the_kernel_cannot_take_are_refused(C_):
    lib = _lib.load()
    x = (C.c_float * 4)()
    p = C.addressof(x)  # never dereferenced: the arguments are checked before the first device call
    L = _lib.ReduceLayer(kind=_lib.REDUCE_NORM_BWD, C=C_, silu=1, rows=4, dy=p, u=p, g=p, du=p, dg=p)
    _refused(lib.dm_op_deferred_reduce(C.byref(L), 1, 2, 1, 0, None), "multiple of 4")


def test_other_layer_refusals():
    lib = _lib.load()
    x = (C.c_float * 4)()
    p = C.addressof(x)
    L = _lib.ReduceLayer(kind=_lib.REDUCE_NORM_BWD, C=8, silu=1, rows=4, dy=p, u=p, g=p, du=p, dg=p, ss=p)
    _refused(lib.dm_op_deferred_reduce(C.byref(L), 1, 2, 1, 0, None), "ss and dss come together")
    L = _lib.ReduceLayer(kind=7, C=8)
    _refused(lib.dm_op_deferred_reduce(C.byref(L), 1, 2, 1, 0, None), "unknown layer kind")
    L = _lib.ReduceLayer(kind=_lib.REDUCE_COLSUM, C=8, rows=4, row_stride=8, col_stride=1, x=p)
    _refused(lib.dm_op_deferred_reduce(C.byref(L), 1, 2, 1, 0, None), "column sum")
