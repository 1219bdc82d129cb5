"""CPU tests of the feature store's cached form (`DeviceFeatureStore(..., featurized=True)`): the binding table against the header, the
entry points' size guards, the cache's key and its release_raw state machine (`feature_store.FeaturizedRows`: no device call) and the
predicate the cache builder shares with the direct route (`interpreter.store_layers_of`)."""

import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _program_inputs as PI  # noqa: E402
from dfol_vqa_amd import _lib, feature_store  # noqa: E402
from dfol_vqa_amd.interpreter import BatchGQABoxFeaturizer, featurizer_trains, store_layers_of  # noqa: E402
from dfol_vqa_amd.visual_oracle import RegularMLP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dfol_store_objects_f32",)
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
        assert [kinds[id(t)] for t in _lib.SIGNATURES[name]] == want, name
    assert "its cached form: dfol_store_objects_f32" in header                      # the "added under 3" list
    PI.assert_forms_and_layout()                                                    # the cached form travels in the scene struct: DFOL_FEATURES_CACHED
    assert _lib.ABI_VERSION == 4 and "#define DFOL_ABI_VERSION 4" in header         # (the structs grew: a layout change moves the version)


def test_entry_points_validate_their_sizes_without_a_device():
    import __graft_entry__ as g
    g.build()
    h = _lib.load()
    assert h.dfol_store_objects_f32(None, 512, None, None, 0, 512, None, 516, None) == 0          # O == 0: nothing to do, no launch
    for O, W, ld_cache, ld_out in ((-1, 512, 512, 516), (0, 0, 512, 516), (0, 512, 511, 516), (0, 512, 512, 515), (0, 1, 1, 4), (1, 512, 512, 516)):
        assert h.dfol_store_objects_f32(None, ld_cache, None, None, O, W, None, ld_out, None) != 0, (O, W, ld_cache, ld_out)
        assert b"store_objects" in h.dfol_last_error()                                            # (the last: null pointers with O > 0)
    assert h.dfol_store_objects_f32(None, 512, None, None, 0, 512, None, 515, None) != 0 and b"ld_out" in h.dfol_last_error()
    # the scene's cached form, on an empty program (nothing is launched)
    C = PI.native_exec.FEATURES_CACHED
    assert PI.run_empty()[0] == 0
    rc, err = PI.run_empty(feature_form=C, cache=8, ld_cache=512, cache_cols=512)                  # a cache without src_row and box6
    assert rc != 0 and b"src_row" in err and b"DFOL_FEATURES_CACHED" in err, err
    rc, err = PI.run_empty(feature_form=C, src_row=8, box6=8, ld_cache=512, cache_cols=512)        # src_row and box6 without a cache
    assert rc != 0 and b"scene->cache" in err, err
    rc, err = PI.run_empty(cache=8, ld_cache=512, cache_cols=512)                                  # a stray cache in the matrix form
    assert rc != 0 and b"scene->cache" in err and b"DFOL_FEATURES_MATRIX" in err, err
    rc, err = PI.run_empty(feature_form=C, cache=8, src_row=8, box6=8, ld_cache=511, cache_cols=512)
    assert rc != 0 and b"cache_cols=512" in err and b"ld_cache=511" in err, err
    rc, err = PI.run_empty(feature_form=C, cache=8, src_row=8, box6=8, ld_cache=512, cache_cols=0)  # (cache_cols is the struct's LAST field: the
    assert rc != 0 and b"cache_cols=0" in err, err                                                 # ctypes layout and the C layout agree)
    assert PI.run_empty(feature_form=C, cache=8, src_row=8, box6=8, ld_cache=512, cache_cols=512)[0] == 0
    assert PI.run_empty(feature_form=C, cache=8, src_row=8, box6=8, ld_cache=516, cache_cols=512)[0] == 0 and PI.run_empty()[0] == 0


def test_cache_key_follows_weight_versions_and_the_arithmetic():
    net = RegularMLP(2048, 512, [], 0.0)
    cache = feature_store.FeaturizedRows()
    assert not cache.valid_for(net) and cache.rows is None and cache.builds == 0
    rows = torch.zeros(4, 512)
    assert cache.set(net, rows) is rows and cache.valid_for(net) and cache.builds == 1
    key = feature_store.featurizer_key(net)
    assert len(key[0]) == 2 and key[1] == _lib._dense_math()                    # weight and bias; the dense arithmetic
    with torch.no_grad():
        net._network[1].bias.add_(1.0)                                          # an in-place update: what an optimizer step does
    assert not cache.valid_for(net) and feature_store.featurizer_key(net) != key
    cache.set(net, rows)
    assert cache.valid_for(net) and cache.builds == 2
    with _lib.dense_math("bf16x3"):                                             # another arithmetic: other rows
        assert not cache.valid_for(net)
    assert cache.valid_for(net)
    net.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})    # the same values, copied in place: a new version all the same
    assert not cache.valid_for(net)
    assert not cache.valid_for(RegularMLP(2048, 512, [], 0.0))                  # another network


def test_release_raw_state_machine():
    net = RegularMLP(2048, 512, [], 0.0)
    cache = feature_store.FeaturizedRows()
    cache.need_raw("gather")                                                    # the raw features are there: nothing to say
    with pytest.raises(_lib.DfolError, match="featurize"):
        cache.release_raw()                                                     # no cache yet: nothing could serve a batch afterwards
    assert not cache.raw_released
    cache.set(net, torch.zeros(4, 512))
    cache.release_raw()
    assert cache.raw_released and cache.valid_for(net)
    for what in ("gather", "StoreRows.materialize()", "featurize() for new featurizer weights"):
        with pytest.raises(_lib.DfolError, match="release_raw") as e:
            cache.need_raw(what)
        assert what in str(e.value)
    cache.release_raw()                                                         # again: no harm


def test_the_predicate_shared_with_the_direct_route():
    net = RegularMLP(2048, 512, [], 0.0)
    M = feature_store.FEATURIZE_BLOCK_ROWS
    layers, why = store_layers_of(net, 2048, M)
    if os.environ.get("DFOL_DENSE_WIDE") != "0" and os.environ.get("DFOL_DENSE_MATH", "f16x2") == "f16x2":
        assert why is None and [(lin.out_features, act) for lin, act in layers] == [(512, _lib.ACT_SIGMOID)]     # the block size pays by default
        two = store_layers_of(RegularMLP(2048, 512, [448], 0.0), 2048, M)[0]
        assert [(lin.in_features, lin.out_features, act) for lin, act in two] == [(2048, 448, _lib.ACT_ELU), (448, 512, _lib.ACT_SIGMOID)]
    for bad, F, word in ((None, 2048, "no network"), (RegularMLP(2048, 512, None, 0.0), 2048, "no network"), (net, 2052, "2052"),
                         (RegularMLP(64, 512, [], 0.0), 64, "wide kernel")):
        layers, why = store_layers_of(bad, F, M)
        assert layers is None and word in why, (F, why)
    with _lib.dense_math("bf16x3"):
        layers, why = store_layers_of(net, 2048, M)
        assert layers is None and "bf16x3" in why

    class Rows(object):                                                         # what _store_layers reads of a StoreRows
        class store(object):
            F = 2048
        O = M
    feat = BatchGQABoxFeaturizer(net)
    assert featurizer_trains(net) and feat._store_layers(Rows) is None          # a gradient reaches the weights: not the direct route's
    with torch.no_grad():
        assert not featurizer_trains(net)
        assert (feat._store_layers(Rows) is None) == (store_layers_of(net, 2048, M)[0] is None)
    for p in net.parameters():
        p.requires_grad_(False)
    assert not featurizer_trains(net)                                           # frozen: grad mode or not
    Rows.O = 0
    assert feat._store_layers(Rows) is None
