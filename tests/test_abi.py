"""The C-ABI library: builds, loads, and exports exactly what include/dm_hip.h declares.
No compute calls (no GPU here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "dm_hip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dm_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_agree():
    from diffusion_models_amd import _lib

    assert sorted(_lib.EXPORTS) == _declared()


def test_library_loads_and_exports_every_symbol():
    from diffusion_models_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _declared():
        assert hasattr(lib, name), name
    lib.dm_abi_version.restype = ctypes.c_int
    assert lib.dm_abi_version() == _lib.ABI_VERSION


def test_no_cpu_fallback_without_gpu():
    import torch

    import diffusion_models_amd as dm

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        dm.Unet(dim=32, dim_mults=(1, 2))  # handle creation needs a HIP device; nothing falls back to the CPU
    with pytest.raises(RuntimeError):
        dm.Unet(dim=32, dim_mults=(1, 2), device="cpu")


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "diffusion-models_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".inc")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f


def _sources(top, exts):
    for dirpath, _, files in os.walk(top):
        for f in files:
            if f.endswith(exts):
                path = os.path.join(dirpath, f)
                yield path, open(path).read()


def test_every_switch_a_test_sets_is_read():
    """A child test that sets a DM_* variable nothing reads silently runs the default path.  Every name a test under tests/
    sets must be read by the library (env_int / env_flag, once per name) or by a Python file of the package or the tests;
    the library reads its environment in dm_common.h only."""
    csrc = os.path.join(ROOT, "diffusion-models_amd", "csrc")
    lib_reads = []
    for path, text in _sources(csrc, (".hip", ".h", ".inc", ".cpp")):
        if os.path.basename(path) != "dm_common.h":
            assert "getenv" not in text, f"{path}: read the environment through env_int / env_flag (dm_common.h)"
        lib_reads += re.findall(r'\benv_(?:int|flag)\(\s*"(DM_[A-Z0-9_]+)"', text)
    dup = sorted({n for n in lib_reads if lib_reads.count(n) > 1})
    assert not dup, f"read at more than one site: {dup}"
    read = set(lib_reads)
    tests = list(_sources(os.path.join(ROOT, "tests"), (".py",)))
    for _, text in list(_sources(os.path.join(ROOT, "diffusion-models_amd"), (".py",))) + tests:
        read |= set(re.findall(r'(?:environ\.get|getenv)\(\s*["\'](DM_[A-Z0-9_]+)["\']', text))
        read |= set(re.findall(r'environ\[\s*["\'](DM_[A-Z0-9_]+)["\']\s*\](?!\s*=[^=])', text))
    set_by_tests = set()
    for _, text in tests:
        set_by_tests |= set(re.findall(r'\b(DM_[A-Z0-9_]+)\s*=(?!=)', text))  # keyword arguments
        set_by_tests |= set(re.findall(r'["\'](DM_[A-Z0-9_]+)["\']\s*(?::|\]\s*=(?!=))', text))  # dict keys, item assignment
        set_by_tests |= set(re.findall(r'setenv\(\s*["\'](DM_[A-Z0-9_]+)["\']', text))
    assert {"DM_NO_WINOGRAD", "DM_ATTN_TILED"} <= set_by_tests & read  # the patterns still see the tests' switches
    unread = sorted(set_by_tests - read)
    assert not unread, f"set by tests but read by nothing: {unread}"
