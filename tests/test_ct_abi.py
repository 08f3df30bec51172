"""The continuous-time additions to the C ABI: the new symbols are declared in include/dm_hip.h, bound in _lib.EXPORTS and
exported by the built library, and the DM_CT_* defines have the values the binding and the kernels' table layout use.
No compute calls (no GPU here)."""
import ctypes
import os
import re

from conftest import ROOT

SYMBOLS = ("dm_sample_ct", "dm_unet_loss_backward_ct", "dm_op_ct_step", "dm_op_ct_noise_in", "dm_op_ct_loss")


def test_symbols_and_defines_exist_in_header_binding_and_library():
    from diffusion_models_amd import _lib
    from diffusion_models_amd import continuous as K

    src = open(os.path.join(ROOT, "include", "dm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    defines = sorted((k[len("DM_CT_"):], int(v)) for k, v in re.findall(r"#define (DM_CT_[A-Z_]+) (\d+)", code))
    assert defines == [("COEFS", 16), ("PRED_NOISE", 0), ("PRED_V", 1)]
    assert (_lib.DM_CT_COEFS, _lib.CT_PRED_NOISE, _lib.CT_PRED_V) == (16, 0, 1) and K.COLS == 16
    assert "typedef struct dm_ct_args" in code and "typedef struct dm_ct_train_args" in code
    # the column indices of the Python tables are those of the kernels' enum (csrc/ct.h)
    ct_h = open(os.path.join(ROOT, "diffusion-models_amd", "csrc", "ct.h")).read()
    enum = {k: int(v) for k, v in re.findall(r"\b(CT_[A-Z_]+) = (\d+),", ct_h)}
    want = dict(CT_LOG_SNR=K.LOG_SNR, CT_ALPHA=K.ALPHA, CT_SIGMA=K.SIGMA, CT_ALPHA_NEXT=K.ALPHA_NEXT, CT_C=K.C_,
                CT_ONE_M_C=K.ONE_M_C, CT_SQRT_VAR=K.SQRT_VAR, CT_AN_OVER_A=K.AN_OVER_A, CT_C_SIGMA=K.C_SIGMA,
                CT_LOSS_W=K.LOSS_W, CT_NCOLS=K.COLS)
    assert {k: enum[k] for k in want} == want
    # additions only
    lib.dm_abi_version.restype = ctypes.c_int
    assert lib.dm_abi_version() == _lib.ABI_VERSION == 9
