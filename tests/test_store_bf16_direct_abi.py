"""CPU tests of the default arithmetic's in-place route over a bf16 feature store (DFOL_STORE_BF16_DIRECT=1): the new entry points in the header
and the binding table, the size predicate, the predicate the routes share (`interpreter.store_layers_of`) with the switch unset and set, and the
wrapper's refusals, which come before any call into the library."""

import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _program_inputs as PI  # noqa: E402
from dfol_vqa_amd import _lib  # noqa: E402
from dfol_vqa_amd.interpreter import store_layers_of  # noqa: E402
from dfol_vqa_amd.visual_oracle import RegularMLP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dfol_linear_wide_rows_bf16t_h2_f32", "dfol_linear_wide_rows_bf16t_supported", "dfol_store_bf16_is_f16", "dfol_linear_wide_rows_bf16t_f16_h2_f32")
CTYPE = {"int32_t": "_i32", "int64_t": "_i64", "float": "_f"}


def test_binding_table_names_the_new_entry_points_with_the_headers_signatures():
    with open(os.path.join(ROOT, "include", "dfol_vqa.h")) as f:
        header = f.read()
    kinds = {id(_lib._p): "_p", id(_lib._i32): "_i32", id(_lib._i64): "_i64", id(_lib._f): "_f"}
    for name in NEW:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            arg = " ".join(arg.split())
            want.append("_p" if "*" in arg else CTYPE[arg.replace("const ", "").split(" ")[0]])
        assert name in _lib.SIGNATURES and [kinds[id(t)] for t in _lib.SIGNATURES[name]] == want, name
    # the product's arguments are dfol_linear_wide_rows_h2_f32's (the table's element type aside); the route's two forms stand beside their siblings
    assert len(_lib.SIGNATURES["dfol_linear_wide_rows_bf16t_h2_f32"]) == len(_lib.SIGNATURES["dfol_linear_wide_rows_h2_f32"]) == 12
    PI.assert_forms_and_layout()                                  # DFOL_FEATURES_ROWS_BF16_H2 and DFOL_FEATURES_ROWS_BF16_H2_F16, in the scene struct
    assert "dfol_linear_wide_rows_bf16t_supported and dfol_linear_wide_rows_bf16t_h2_f32" in header       # the "added under 3" list
    assert "dfol_store_bf16_is_f16 and dfol_linear_wide_rows_bf16t_f16_h2_f32" in header
    assert _lib.ABI_VERSION == 4 and "#define DFOL_ABI_VERSION 4" in header


def test_the_size_predicate_is_reachable_without_a_device():
    import __graft_entry__ as g
    g.build()
    M = 25600
    if os.environ.get("DFOL_DENSE_WIDE") == "0":
        assert not _lib.linear_wide_rows_bf16t_supported(M, 512, 2048, 2048)
        return
    assert _lib.linear_wide_supported(M, 512, 2048) and _lib.linear_wide_rows_bf16t_supported(M, 512, 2048, 2048)
    assert _lib.linear_wide_rows_bf16t_supported(M, 512, 2048, 2052)                    # 8-byte rows: the two 8-byte loads
    assert not _lib.linear_wide_rows_bf16t_supported(M, 512, 2048, 2050)                # rows that are not 8-byte aligned
    assert not _lib.linear_wide_rows_bf16t_supported(M, 512, 2048, 2044)                # a stride below K
    assert not _lib.linear_wide_rows_bf16t_supported(M, 256, 2048, 2048)                # what dfol_linear_wide_supported refuses stays refused
    assert not _lib.linear_wide_rows_bf16t_supported(M, 512, 96, 96)
    h = _lib.load()
    # refusals before any launch: no device is touched here
    assert h.dfol_linear_wide_rows_bf16t_h2_f32(8, 2048, None, 16, None, 8, 512, 4, 512, 2048, 0, None) != 0 and b"null pointer" in h.dfol_last_error()
    assert h.dfol_linear_wide_rows_bf16t_h2_f32(8, 2050, 8, 16, None, 8, 512, 4, 512, 2048, 0, None) != 0 and b"multiple of 4" in h.dfol_last_error()
    assert h.dfol_linear_wide_rows_bf16t_h2_f32(8, 2044, 8, 16, None, 8, 512, 4, 512, 2048, 0, None) != 0 and b"bad sizes" in h.dfol_last_error()
    assert h.dfol_linear_wide_rows_bf16t_h2_f32(12, 2048, 8, 16, None, 8, 512, 4, 512, 2048, 0, None) != 0 and b"8-byte" in h.dfol_last_error()
    for name in ("ROWS_BF16_H2", "ROWS_BF16_H2_F16", "ROWS_BF16"):
        form = getattr(PI.native_exec, "FEATURES_" + name)
        rc, err = PI.run_empty(feature_form=form, src_row=8)       # (an empty program: nothing is launched)
        assert rc != 0 and b"src_row" in err and b"box6" in err and ("(DFOL_FEATURES_%s," % name).encode() in err, (form, err)
        rc, err = PI.run_empty(feature_form=form)
        assert rc != 0 and b"src_row" in err, (form, err)
        assert PI.run_empty(feature_form=form, src_row=8, box6=8)[0] == 0 and PI.run_empty()[0] == 0


def test_the_shared_predicate_follows_the_switch(monkeypatch):
    monkeypatch.delenv("DFOL_DENSE_MATH", raising=False)
    net = RegularMLP(2048, 512, [], 0.0)
    M = 25600
    if os.environ.get("DFOL_DENSE_WIDE") == "0":                                                # (read once by the library: no wide kernel, no route)
        monkeypatch.setenv("DFOL_STORE_BF16_DIRECT", "1")
        with torch.no_grad():
            assert store_layers_of(net, 2048, M, bf16_ld=2048)[0] is None
        return
    with torch.no_grad():
        monkeypatch.delenv("DFOL_STORE_BF16_DIRECT", raising=False)
        assert not _lib.store_bf16_direct()
        layers, why = store_layers_of(net, 2048, M, bf16_ld=2048)
        assert layers is None and "'f16x2', not 'bf16'" in why                                  # as ever: the question is the bf16 mode's
        assert store_layers_of(net, 2048, M)[0] is not None                                     # (an fp32 table: the wide kernel's, unchanged)
        monkeypatch.setenv("DFOL_STORE_BF16_DIRECT", "0")
        assert store_layers_of(net, 2048, M, bf16_ld=2048)[0] is None
        monkeypatch.setenv("DFOL_STORE_BF16_DIRECT", "1")
        assert _lib.store_bf16_direct()
        layers, why = store_layers_of(net, 2048, M, bf16_ld=2048)
        assert why is None and [(lin.out_features, act) for lin, act in layers] == [(512, _lib.ACT_SIGMOID)]
        assert store_layers_of(net, 2048, M, bf16_ld=2052)[0] is not None
        for bad_net, F, rows, ld, word in ((net, 2048, M, 2050, "row stride 2050"), (net, 2048, 40, 2048, "over 40 rows"), (net, 2052, M, 2052, "2052"),
                                           (RegularMLP(64, 512, [], 0.0), 64, M, 64, "wide kernel")):
            layers, why = store_layers_of(bad_net, F, rows, bf16_ld=ld)
            assert layers is None and word in why, why
        with _lib.dense_math("bf16"):                                                           # the bf16 mode keeps its own question, any M
            assert store_layers_of(net, 2048, 40, bf16_ld=2048)[0] is not None
        with _lib.dense_math("bf16x3"):
            layers, why = store_layers_of(net, 2048, M, bf16_ld=2048)
            assert layers is None and "bf16x3" in why
    # a featurizer that trains keeps today's answer: the inference route only
    assert store_layers_of(net, 2048, M, bf16_ld=2048)[0] is None


def test_the_wrapper_refuses_before_any_call(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", no_call)
    idx = torch.arange(4, dtype=torch.int32)
    W = torch.zeros(512, 128)
    with pytest.raises(_lib.DfolError, match="bfloat16"):
        _lib.linear_wide_rows_bf16t(torch.zeros(8, 128), idx, W, None, 0)                        # an fp32 table is linear_wide_rows'
    with pytest.raises(_lib.DfolError, match="bfloat16"):
        _lib.linear_wide_rows_bf16t(torch.zeros(8, 128, dtype=torch.float16), idx, W, None, 0)
    with pytest.raises(_lib.DfolError, match=r"weight \[N, 132\]"):
        _lib.linear_wide_rows_bf16t(torch.zeros(8, 132, dtype=torch.bfloat16), idx, W, None, 0)  # a weight of another width
    with pytest.raises(_lib.DfolError, match="unit column stride"):
        _lib.linear_wide_rows_bf16t(torch.zeros(8, 256, dtype=torch.bfloat16)[:, ::2], idx, W, None, 0)
