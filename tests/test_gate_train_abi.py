"""CPU-side checks of the one-posterior gated Relate of the train step (DFOL_GATE_TRAIN=1): the two entry points at the C-ABI boundary, the
switch, and the refusal of CPU tensors."""

import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dfol_vqa.h")
ENTRY_POINTS = {"dfol_relate_keep_gate_fwd_f32": 17, "dfol_relate_keep_gate_bwd_f32": 23}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from dfol_vqa_amd import _lib
    return _lib


def test_entry_points_in_header_and_table(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    handle = lib.load()
    for name, count in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
        assert m, name + " is not declared in include/dfol_vqa.h"
        args = [a for a in m.group(1).split(",") if a.strip()]
        assert len(args) == count == len(lib.SIGNATURES[name]), (name, len(args), len(lib.SIGNATURES[name]))
        assert args[-1].strip() == "void* stream"
        assert hasattr(handle, name)
    assert handle.dfol_abi_version() == 4 == lib.ABI_VERSION
    # the header cites the reference lines each replaces
    raw = open(HEADER).read()
    for name in ENTRY_POINTS:
        comment = raw[:raw.index("int " + name)].rsplit("/*", 1)[1]
        assert "batch_gqa_ops.py:364-371" in comment and "batch_base_ops.py" in comment, name


def test_argument_errors_without_a_device(lib):
    h = lib.load()
    assert h.dfol_relate_keep_gate_fwd_f32(None, None, None, None, None, None, None, None, 0, None, 2, 6, 0, None, None, None, None) != 0
    assert b"relate_keep_gate_fwd" in h.dfol_last_error()
    assert h.dfol_relate_keep_gate_bwd_f32(*([None] * 9), 0, None, 2, 1028, 0, *([None] * 9)) != 0
    assert b"relate_keep_gate_bwd" in h.dfol_last_error() and b"1024" in h.dfol_last_error()


def test_gate_train_reads_the_switch(lib, monkeypatch):
    monkeypatch.delenv("DFOL_GATE_TRAIN", raising=False)
    assert lib.gate_train() is False
    monkeypatch.setenv("DFOL_GATE_TRAIN", "1")
    assert lib.gate_train() is True
    monkeypatch.setenv("DFOL_GATE_TRAIN", "0")
    assert lib.gate_train() is False
    monkeypatch.setenv("DFOL_GATE_NATIVE", "1")                    # the inference switch is another switch
    assert lib.gate_train() is False and lib.gate_native() is True


def test_no_cpu_fallback(lib):
    import torch
    from dfol_vqa_amd import ops
    P, NS = 2, 4
    x, prev, tile = torch.zeros(P, NS), torch.zeros(P, NS), torch.zeros(P, NS, NS)
    pq, n = torch.arange(P, dtype=torch.int32), torch.full((P,), 3, dtype=torch.int32)
    quant, flag = torch.ones(P), torch.ones(P, dtype=torch.uint8)
    w, b = torch.zeros(6, 2), torch.zeros(6)
    gate = lib.gate_params(w, b)
    with pytest.raises(lib.DfolError, match="no CPU fallback"):
        lib.relate_keep_gate_fwd(x, prev, tile, pq, n, quant, flag, gate, gate)
    with pytest.raises(lib.DfolError, match="no CPU fallback"):
        lib.relate_keep_gate_bwd(x, x, prev, tile, pq, n, quant, flag, gate, gate, None, None, False, identity=True)
    with pytest.raises(lib.DfolError, match="no CPU fallback"):
        ops.relate_keep_gate(x, prev, tile, pq, n, quant, flag, w.requires_grad_(True), b, w, b)
    with pytest.raises(lib.DfolError, match="no CPU fallback"):
        with torch.no_grad():
            ops.relate_keep_gate(x, prev, tile, pq, n, quant, flag, w, b, w, b)
