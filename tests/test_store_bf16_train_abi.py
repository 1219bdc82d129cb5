"""CPU tests of the default arithmetic's train route over a bf16 feature store (DFOL_STORE_BF16_TRAIN=1): the weight gradient's two entry points
in the header and the binding table, its size predicate - DFOL_WGRAD_MATH=f32 included, which the library reads per call - the switch reader, and
what the shared predicate `interpreter.store_layers_of` answers a featurizer that trains with the switch unset and set."""

import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import _lib  # noqa: E402
from dfol_vqa_amd.interpreter import store_layers_of  # noqa: E402
from dfol_vqa_amd.visual_oracle import RegularMLP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dfol_linear_wgrad_rows_bf16t_x3_supported", "dfol_linear_wgrad_bias_rows_bf16t_x3")
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
    # the arguments are the bf16 mode's entry points' over the same table
    assert _lib.SIGNATURES["dfol_linear_wgrad_bias_rows_bf16t_x3"] == _lib.SIGNATURES["dfol_linear_wgrad_bias_rows_bf16t"]
    assert _lib.SIGNATURES["dfol_linear_wgrad_rows_bf16t_x3_supported"] == _lib.SIGNATURES["dfol_linear_wgrad_rows_bf16t_supported"]
    assert "dfol_linear_wgrad_rows_bf16t_x3_supported and dfol_linear_wgrad_bias_rows_bf16t_x3" in header      # the "added under 3" list
    assert _lib.ABI_VERSION == 4 and "#define DFOL_ABI_VERSION 4" in header


def test_the_size_predicate(monkeypatch):
    import __graft_entry__ as g
    g.build()
    monkeypatch.delenv("DFOL_WGRAD_MATH", raising=False)
    ok = _lib.linear_wgrad_rows_bf16t_x3_supported
    assert ok(512, 2048, 512, 2048) and ok(512, 2048, 516, 2052)
    assert not ok(512, 2048, 512, 2050)                                   # ld_table % 4 != 0: rows that are not 8-byte aligned
    assert not ok(512, 2046, 512, 2048) and not ok(510, 2048, 512, 2048)  # K % 4 != 0, N % 4 != 0
    assert not ok(512, 2048, 508, 2048)                                   # ld_dy < N
    assert not ok(512, 2048, 512, 2044)                                   # a stride below K
    monkeypatch.setenv("DFOL_WGRAD_MATH", "f32")                          # the fp32 pipe has no indexed form
    assert not ok(512, 2048, 512, 2048)
    assert _lib.linear_wgrad_rows_supported(512, 2048, 512, 2048, bf16_table=True)       # (the bf16 mode does not read that switch)
    h = _lib.load()
    assert h.dfol_linear_wgrad_bias_rows_bf16t_x3(16, 512, 8, 2048, 8, 4, 512, 2048, 16, 16, None, None) != 0 and b"DFOL_WGRAD_MATH=f32" in h.dfol_last_error()
    monkeypatch.delenv("DFOL_WGRAD_MATH")
    assert ok(512, 2048, 512, 2048)
    # refusals before any launch: no device is touched here
    assert h.dfol_linear_wgrad_bias_rows_bf16t_x3(16, 512, None, 2048, 8, 4, 512, 2048, 16, 16, None, None) != 0 and b"null pointer" in h.dfol_last_error()
    assert h.dfol_linear_wgrad_bias_rows_bf16t_x3(16, 512, 8, 2050, 8, 4, 512, 2048, 16, 16, None, None) != 0 and b"ld_table % 4" in h.dfol_last_error()
    assert h.dfol_linear_wgrad_bias_rows_bf16t_x3(16, 512, 8, 2048, 8, 0, 512, 2048, 16, 16, None, None) != 0 and b"bad sizes" in h.dfol_last_error()
    assert h.dfol_linear_wgrad_bias_rows_bf16t_x3(24, 512, 8, 2048, 8, 4, 512, 2048, 16, 16, None, None) != 0 and b"16-byte" in h.dfol_last_error()
    assert h.dfol_linear_wgrad_bias_rows_bf16t_x3(16, 512, 12, 2048, 8, 4, 512, 2048, 16, 16, None, None) != 0 and b"8-byte" in h.dfol_last_error()


def test_the_switch_reader(monkeypatch):
    monkeypatch.delenv("DFOL_STORE_BF16_TRAIN", raising=False)
    assert _lib.store_bf16_train() is False
    monkeypatch.setenv("DFOL_STORE_BF16_TRAIN", "0")
    assert _lib.store_bf16_train() is False
    monkeypatch.setenv("DFOL_STORE_BF16_TRAIN", "1")
    assert _lib.store_bf16_train() is True
    monkeypatch.setenv("DFOL_STORE_BF16_DIRECT", "1")                     # the inference switch is another one
    monkeypatch.delenv("DFOL_STORE_BF16_TRAIN")
    assert _lib.store_bf16_train() is False and _lib.store_bf16_direct()


def test_the_shared_predicate_admits_a_training_featurizer_under_its_own_switch_only(monkeypatch):
    for k in ("DFOL_DENSE_MATH", "DFOL_STORE_BF16_DIRECT", "DFOL_STORE_BF16_TRAIN"):
        monkeypatch.delenv(k, raising=False)
    net = RegularMLP(2048, 512, [], 0.0)
    M = 25600
    assert torch.is_grad_enabled() and any(p.requires_grad for p in net.parameters())
    if os.environ.get("DFOL_DENSE_WIDE") == "0":                          # (read once by the library: no wide kernel, no route)
        monkeypatch.setenv("DFOL_STORE_BF16_TRAIN", "1")
        assert store_layers_of(net, 2048, M, bf16_ld=2048)[0] is None
        return
    layers, why = store_layers_of(net, 2048, M, bf16_ld=2048)
    assert layers is None and "'f16x2', not 'bf16'" in why                # as ever
    monkeypatch.setenv("DFOL_STORE_BF16_DIRECT", "1")                     # the inference switch does not move a train step
    assert store_layers_of(net, 2048, M, bf16_ld=2048)[0] is None
    monkeypatch.delenv("DFOL_STORE_BF16_DIRECT")
    monkeypatch.setenv("DFOL_STORE_BF16_TRAIN", "1")
    layers, why = store_layers_of(net, 2048, M, bf16_ld=2048)
    assert why is None and [(lin.out_features, act) for lin, act in layers] == [(512, _lib.ACT_SIGMOID)]
    assert store_layers_of(net, 2048, M, bf16_ld=2050)[0] is None and store_layers_of(net, 2048, 40, bf16_ld=2048)[0] is None
    with torch.no_grad():                                                 # ... and the train switch does not move inference
        assert store_layers_of(net, 2048, M, bf16_ld=2048)[0] is None
    with _lib.dense_math("bf16"):                                         # the bf16 mode keeps its own question
        assert store_layers_of(net, 2048, 40, bf16_ld=2048)[0] is not None
    with _lib.dense_math("bf16x3"):
        layers, why = store_layers_of(net, 2048, M, bf16_ld=2048)
        assert layers is None and "bf16x3" in why
