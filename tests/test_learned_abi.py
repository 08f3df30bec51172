"""The learned-variance additions to the C ABI: the new symbols are declared in include/dm_hip.h, bound in _lib.EXPORTS and
exported by the built library; the two ctypes structs have the sizes and offsets the C compiler gives the header's
declarations (an ``offsetof`` dump compiled for the host); the column indices of the Python tables are those of the kernels'
enums.  No compute calls (no GPU here)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("dm_sample_lv", "dm_unet_loss_backward_lv", "dm_op_lv_step", "dm_op_lv_loss")
STRUCTS = {"dm_lv_args": "LvArgs", "dm_lv_train_args": "LvTrainArgs"}


def test_symbols_defines_and_columns():
    from diffusion_models_amd import _lib
    from diffusion_models_amd import learned as L

    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    defines = sorted((k[len("DM_LV_"):], int(v)) for k, v in re.findall(r"#define (DM_LV_[A-Z_]+) (\d+)", code))
    assert defines == [("COEFS", 16), ("TRAIN_COEFS", 12)]
    assert (_lib.DM_LV_COEFS, _lib.DM_LV_TRAIN_COEFS) == (16, 12) and (L.COLS, L.TRAIN_COLS) == (16, 12)
    for s in STRUCTS:
        assert "typedef struct %s" % s in code
    h = open(os.path.join(ROOT, "diffusion-models_amd", "csrc", "learned.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"\b(LVT?_[A-Z0-9_]+) = (\d+),", h)}
    want = dict(LV_RECIP=L.RECIP, LV_RECIPM1=L.RECIPM1, LV_COEF1=L.COEF1, LV_COEF2=L.COEF2, LV_MIN_LOG=L.MIN_LOG,
                LV_NOISE=L.NOISE, LV_MAX_LOG=L.MAX_LOG, LV_NCOLS=L.COLS, LVT_SQRT_AC=L.T_SQRT_AC, LVT_SQRT_1M_AC=L.T_SQRT_1M_AC,
                LVT_RECIP=L.T_RECIP, LVT_RECIPM1=L.T_RECIPM1, LVT_COEF1=L.T_COEF1, LVT_COEF2=L.T_COEF2,
                LVT_MIN_LOG=L.T_MIN_LOG, LVT_TRUE_LOG=L.T_TRUE_LOG, LVT_MAX_LOG=L.T_MAX_LOG, LVT_T0=L.T_T0,
                LVT_NCOLS=L.TRAIN_COLS)
    assert {k: enum[k] for k in want} == want
    lib.dm_abi_version.restype = ctypes.c_int
    assert lib.dm_abi_version() == _lib.ABI_VERSION  # additions only: the version keeps its value


def test_struct_layouts_match_the_compiler(tmp_path):
    from diffusion_models_amd import _lib

    cxx = os.environ.get("HIPCC") or shutil.which("hipcc") or shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no C++ compiler found (the build needs hipcc)")
    lines = ['#include "dm_hip.h"', "#include <cstddef>", "#include <cstdio>", "int main() {"]
    for s, b in STRUCTS.items():
        lines.append('    std::printf("%s size %%zu\\n", sizeof(%s));' % (s, s))
        for name, _ in getattr(_lib, b)._fields_:
            lines.append('    std::printf("%s %s %%zu\\n", offsetof(%s, %s));' % (s, name, s, name))
    lines += ["    return 0;", "}"]
    src = tmp_path / "lv_offsets.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "lv_offsets"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        s, name, v = line.split()
        got.setdefault(s, {})[name] = int(v)
    for s, b in STRUCTS.items():
        cls = getattr(_lib, b)
        ours = {name: getattr(cls, name).offset for name, _ in cls._fields_}
        ours["size"] = ctypes.sizeof(cls)
        assert got[s] == ours, s
    assert got["dm_lv_args"]["size"] == 104 and got["dm_lv_train_args"]["size"] == 96
