"""CPU-side checks of the one-posterior Relate of the ungated train step (DFOL_RELATE_TRAIN=1): the two entry points at the C-ABI boundary, the
switch, the autograd front and the refusal of CPU tensors."""

import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dfol_vqa.h")
ENTRY_POINTS = {"dfol_relate_keep_fwd_f32": 15, "dfol_relate_keep_bwd_f32": 18}
C_TYPES = {"const float*": "c_void_p", "float*": "c_void_p", "const int32_t*": "c_void_p", "const uint8_t*": "c_void_p", "void*": "c_void_p",
           "int32_t": "c_int"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dfol_vqa_amd import _lib
    return _lib


def test_entry_points_in_header_and_table(lib):
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    handle = lib.load()
    for name, count in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert m, name + " is not declared in include/dfol_vqa.h"
        args = [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]
        assert len(args) == count == len(lib.SIGNATURES[name]), (name, len(args), len(lib.SIGNATURES[name]))
        assert args[-1] == "void* stream"
        for a, ct in zip(args, lib.SIGNATURES[name]):                 # the table's ctypes, argument for argument
            ctype = a.rsplit(" ", 1)[0]
            assert C_TYPES[ctype] == ct.__name__, (name, a, ct)
        assert hasattr(handle, name)
        comment = raw[:raw.index("int " + name)].rsplit("/*", 1)[1]  # the header cites the reference lines each replaces
        assert "batch_gqa_ops.py:364-371" in comment and "batch_base_ops.py" in comment, name
    assert handle.dfol_abi_version() == 4 == lib.ABI_VERSION
    assert re.search(r"#define\s+DFOL_ABI_VERSION\s+4\b", raw)
    version_note = raw[:raw.index("#define DFOL_ABI_VERSION")].rsplit("/*", 1)[1]
    assert all(name in version_note for name in ENTRY_POINTS)


def test_argument_errors_without_a_device(lib):
    h = lib.load()
    assert h.dfol_relate_keep_fwd_f32(None, None, None, None, None, None, None, None, 0, None, 2, 6, 0, None, None) != 0
    assert b"relate_keep_fwd" in h.dfol_last_error()
    assert h.dfol_relate_keep_fwd_f32(None, None, None, None, None, None, None, None, 0, None, 2, 8, 0, None, None) != 0
    assert b"null pointer" in h.dfol_last_error()
    assert h.dfol_relate_keep_bwd_f32(*([None] * 9), 0, None, 2, 2052, 0, None, None, None, None) != 0
    assert b"relate_keep_bwd" in h.dfol_last_error() and b"2048" in h.dfol_last_error()
    assert lib.RELATE_KEEP_BWD_MAX_NS == 2048


def test_relate_train_reads_the_switch_per_call(lib, monkeypatch):
    monkeypatch.delenv("DFOL_RELATE_TRAIN", raising=False)
    assert lib.relate_train() is False
    monkeypatch.setenv("DFOL_RELATE_TRAIN", "1")                  # read when asked, not cached at import
    assert lib.relate_train() is True
    monkeypatch.setenv("DFOL_RELATE_TRAIN", "0")
    assert lib.relate_train() is False
    monkeypatch.setenv("DFOL_GATE_TRAIN", "1")                    # the gated model's switch is another switch
    assert lib.relate_train() is False and lib.gate_train() is True
    from dfol_vqa_amd import ops
    assert ops.relate_train is lib.relate_train


def test_no_cpu_fallback(lib):
    import torch
    from dfol_vqa_amd import ops
    assert callable(ops.relate_keep)
    P, NS = 2, 4
    x, prev, tile = torch.zeros(P, NS), torch.zeros(P, NS), torch.zeros(P, NS, NS)
    pq, n = torch.arange(P, dtype=torch.int32), torch.full((P,), 3, dtype=torch.int32)
    quant, flag = torch.ones(P), torch.ones(P, dtype=torch.uint8)
    with pytest.raises(lib.DfolError, match="no CPU fallback"):
        lib.relate_keep_fwd(x, prev, tile, pq, n, quant, flag)
    with pytest.raises(lib.DfolError, match="no CPU fallback"):
        lib.relate_keep_bwd(x, x, prev, tile, pq, n, quant, flag, None, None, False, identity=True)
    with pytest.raises(lib.DfolError, match="no CPU fallback"):
        ops.relate_keep(x.clone().requires_grad_(True), prev, tile, pq, n, quant, flag)
    with pytest.raises(lib.DfolError, match="no CPU fallback"):
        with torch.no_grad():
            ops.relate_keep(x, prev, tile, pq, n, quant, flag)
    with pytest.raises(lib.DfolError, match="fp32 tiles"):           # shape and dtype refusals come before anything touches a device
        lib.relate_keep_fwd(x, prev, tile.to(torch.bfloat16), pq, n, quant, flag)
    with pytest.raises(lib.DfolError, match="subject flags"):
        lib.relate_keep_fwd(x, prev, tile, pq, n, quant, flag[:1])
    with pytest.raises(lib.DfolError, match="do not match"):
        lib.relate_keep_fwd(x[:, :3], prev, tile, pq, n, quant, flag)
