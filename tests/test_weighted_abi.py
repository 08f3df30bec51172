"""The weighted-objective additions to the C ABI: the new symbols are declared in include/dm_hip.h, bound in _lib.EXPORTS and
exported by the built library; the two ctypes structs have the sizes and offsets the C compiler gives the header's
declarations (an ``offsetof`` dump compiled for the host); the column indices of the Python tables are those of the kernels'
enums and sit where the learned-variance tables have the shared columns.  No compute calls (no GPU here)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("dm_sample_wo", "dm_unet_loss_backward_wo", "dm_op_wo_step", "dm_op_wo_loss")
STRUCTS = {"dm_wo_args": "WoArgs", "dm_wo_train_args": "WoTrainArgs"}


def test_symbols_defines_and_columns():
    from diffusion_models_amd import _lib
    from diffusion_models_amd import learned as L
    from diffusion_models_amd import weighted as Wm

    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    defines = sorted((k[len("DM_WO_"):], int(v)) for k, v in re.findall(r"#define (DM_WO_[A-Z_]+) (\d+)", code))
    assert defines == [("COEFS", 16), ("TRAIN_COEFS", 12)]
    assert (_lib.DM_WO_COEFS, _lib.DM_WO_TRAIN_COEFS) == (16, 12) and (Wm.COLS, Wm.TRAIN_COLS) == (16, 12)
    # the row widths and the shared columns are the learned-variance tables': the handle's table buffers serve unchanged
    assert (_lib.DM_WO_COEFS, _lib.DM_WO_TRAIN_COEFS) == (_lib.DM_LV_COEFS, _lib.DM_LV_TRAIN_COEFS)
    assert (Wm.RECIP, Wm.RECIPM1, Wm.COEF1, Wm.COEF2, Wm.LOGVAR, Wm.NOISE) == (L.RECIP, L.RECIPM1, L.COEF1, L.COEF2, L.MIN_LOG,
                                                                              L.NOISE)
    assert (Wm.T_SQRT_AC, Wm.T_SQRT_1M_AC, Wm.T_RECIP, Wm.T_RECIPM1) == (L.T_SQRT_AC, L.T_SQRT_1M_AC, L.T_RECIP, L.T_RECIPM1)
    for s in STRUCTS:
        assert "typedef struct %s" % s in code
    h = open(os.path.join(ROOT, "diffusion-models_amd", "csrc", "weighted.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"\b(WOT?_[A-Z0-9_]+) = (\d+),", h)}
    want = dict(WO_RECIP=Wm.RECIP, WO_RECIPM1=Wm.RECIPM1, WO_COEF1=Wm.COEF1, WO_COEF2=Wm.COEF2, WO_LOGVAR=Wm.LOGVAR,
                WO_NOISE=Wm.NOISE, WO_NCOLS=Wm.COLS, WOT_SQRT_AC=Wm.T_SQRT_AC, WOT_SQRT_1M_AC=Wm.T_SQRT_1M_AC,
                WOT_RECIP=Wm.T_RECIP, WOT_RECIPM1=Wm.T_RECIPM1, WOT_NCOLS=Wm.TRAIN_COLS)
    assert {k: enum[k] for k in want} == want
    lib.dm_abi_version.restype = ctypes.c_int
    assert lib.dm_abi_version() == _lib.ABI_VERSION  # additions only: the version keeps its value
    mk = open(os.path.join(ROOT, "diffusion-models_amd", "csrc", "Makefile")).read()
    assert "weighted.hip" in mk and "dm_weighted.inc" in mk


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
    src = tmp_path / "wo_offsets.cpp"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "wo_offsets"
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
    assert got["dm_wo_args"]["size"] == 104 and got["dm_wo_train_args"]["size"] == 96
