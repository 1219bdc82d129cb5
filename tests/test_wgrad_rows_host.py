"""CPU-side checks of the indexed-rows weight gradient's C-ABI: the header declares the three names, the binding table carries them with the
header's argument types, the built library exports them, and the host wrappers exist and refuse CPU tensors."""

import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dfol_vqa.h")
NAMES = ("dfol_linear_wgrad_rows_supported", "dfol_linear_wgrad_bias_rows_f32", "dfol_linear_wgrad_bias_rows_bf16")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dfol_vqa_amd import _lib
    return _lib


def header_arguments(name):
    """The C argument types of `name`'s prototype, as ctypes types (pointers of every kind are c_void_p in the binding table)."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, "%s is not declared in include/dfol_vqa.h" % name
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        if "*" in arg:
            out.append(ctypes.c_void_p)
        elif arg.startswith("int64_t"):
            out.append(ctypes.c_int64)
        elif arg.startswith("int32_t"):
            out.append(ctypes.c_int32)
        else:
            raise AssertionError("unexpected argument %r of %s" % (arg, name))
    return out


def test_names_are_declared_bound_and_exported(lib):
    handle = ctypes.CDLL(lib.LIB_PATH)
    for name in NAMES:
        assert name in lib.SIGNATURES, name
        assert lib.SIGNATURES[name] == header_arguments(name), name
        assert hasattr(handle, name), "libdfolvqa.so does not export %s" % name
    # the two entry points take the matrix form's arguments with the index after the table's stride
    matrix = lib.SIGNATURES["dfol_linear_wgrad_bias_f32"]
    for name in NAMES[1:]:
        assert lib.SIGNATURES[name] == matrix[:4] + [ctypes.c_void_p] + matrix[4:], name
    assert lib.SIGNATURES[NAMES[1]] == lib.SIGNATURES[NAMES[2]]


def test_predicate_needs_no_gpu(lib, monkeypatch):
    monkeypatch.delenv("DFOL_WGRAD_MATH", raising=False)
    assert lib.linear_wgrad_rows_supported(512, 2048, 512, 2048) is True
    assert lib.linear_wgrad_rows_supported(512, 2046, 512, 2048) is False      # K % 4
    assert lib.linear_wgrad_rows_supported(510, 2048, 512, 2048) is False      # N % 4
    assert lib.linear_wgrad_rows_supported(512, 2048, 514, 2048) is False      # ld_dy % 4
    assert lib.linear_wgrad_rows_supported(512, 2048, 512, 2044) is False      # ld_table < K
    assert lib.linear_wgrad_rows_supported(512, 2048, 512, 1 << 25) is False   # 16 rows beyond a buffer descriptor's reach
    monkeypatch.setenv("DFOL_WGRAD_MATH", "f32")
    assert lib.linear_wgrad_rows_supported(512, 2048, 512, 2048) is False      # the fp32 matrix pipe has no indexed form


def test_host_wrapper_refuses_cpu_tensors(lib):
    import torch
    dy, table, idx = torch.zeros(4, 8), torch.zeros(40, 16), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(lib.DfolError):
        lib.linear_wgrad_rows(dy, table, idx)
