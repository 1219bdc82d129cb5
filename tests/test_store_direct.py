"""CPU tests of the feature store's index form: the binding table against the header, the host restatement of the row expansion
(`ObjectFeatureRef.source_rows`, the expected value of the GPU tests) and the guard on stores of 2^31 rows or more."""

import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _program_inputs as PI  # noqa: E402
from dfol_vqa_amd import _lib, feature_store  # noqa: E402
from dfol_vqa_amd.feature_store import ObjectFeatureRef  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dfol_store_rows_f32", "dfol_linear_wide_rows_h2_f32")
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
    assert "dfol_store_rows_f32 and dfol_linear_wide_rows_h2_f32" in header                              # the "added under 3" list
    PI.assert_forms_and_layout()                                  # the index form travels in the scene struct: DFOL_FEATURES_ROWS_F32
    assert _lib.ABI_VERSION == 4 and "#define DFOL_ABI_VERSION 4" in header


MAX_OBJ = 40


def restated(slots, counts, max_obj):
    return np.array([s * max_obj + j for s, n in zip(slots, counts) for j in range(min(n, max_obj))], np.int64)


@pytest.mark.parametrize("slots,counts", [([3, 0, 5, 5, 2, 1, 3], [40, 0, 37, 1, 40, 13, 7]), ([5], [40]), ([4, 4, 4], [1, 40, 1]), ([2, 0, 2], [0, 0, 0]), ([], [])],
                         ids=["ragged", "last", "repeated", "zeros", "none"])
def test_source_rows(slots, counts):
    ref = ObjectFeatureRef("s", slots, counts)
    got = ref.source_rows(MAX_OBJ)
    assert got.dtype == np.int32 and got.shape == (sum(counts),)
    assert np.array_equal(got, restated(slots, counts, MAX_OBJ))
    off = ref.index_array()[len(slots):]
    for i, (s, n) in enumerate(zip(slots, counts)):              # the kernel's own statement: src_row[obj_off[i] + j] = slot[i] * max_obj + j
        assert got[off[i]:off[i + 1]].tolist() == [s * MAX_OBJ + j for j in range(n)]


def test_source_rows_stop_at_max_obj():
    assert ObjectFeatureRef("s", [1, 0], [5, 2]).source_rows(3).tolist() == [3, 4, 5, 0, 1]


def test_row_space_guard():
    feature_store.check_row_space(2 ** 31 // 128 - 1, 128)
    feature_store.check_row_space(21474836, 100)                  # 2_147_483_600 rows
    for S, max_obj in ((2 ** 31 // 128, 128), (21474837, 100), (2 ** 31, 1)):
        with pytest.raises(_lib.DfolError):
            feature_store.check_row_space(S, max_obj)
    with pytest.raises(_lib.DfolError):
        ObjectFeatureRef("s", [2 ** 24], [1]).source_rows(128)


def test_entry_points_validate_their_sizes_without_a_device():
    import __graft_entry__ as g
    g.build()
    h = _lib.load()
    assert h.dfol_store_rows_f32(None, None, None, None, 0, 6, 40, None, None, None) == 0                # I == 0: nothing to do, no launch
    assert h.dfol_store_rows_f32(None, None, None, None, 0, 2 ** 24, 128, None, None, None) != 0          # S * max_obj = 2^31
    assert b"store_rows" in h.dfol_last_error() and b"2^31" in h.dfol_last_error()
    assert h.dfol_store_rows_f32(None, None, None, None, 0, 2 ** 24 - 1, 128, None, None, None) == 0
    for I, S, max_obj in ((-1, 6, 40), (1, 0, 40), (1, 6, 0), (1, 6, 40)):                                  # bad sizes; null pointers with I > 0
        assert h.dfol_store_rows_f32(None, None, None, None, I, S, max_obj, None, None, None) != 0
        assert b"store_rows" in h.dfol_last_error()
    assert h.dfol_linear_wide_rows_h2_f32(None, 128, None, None, None, None, 512, 1, 512, 128, 0, None) != 0
    assert b"linear_wide_rows_h2" in h.dfol_last_error()
    # the scene's index form, on an empty program (nothing is launched): the fields are checked before anything else happens
    F = PI.native_exec.FEATURES_ROWS_F32
    assert PI.run_empty()[0] == 0                                                                          # a zeroed tail: the matrix form
    assert PI.run_empty(feature_form=F, src_row=8, box6=8)[0] == 0
    for fields in (dict(feature_form=F, src_row=8), dict(feature_form=F, box6=8), dict(feature_form=F), dict(src_row=8, box6=8), dict(src_row=8)):
        rc, err = PI.run_empty(**fields)                                                                   # one without the other; a rows form
        assert rc != 0 and b"src_row" in err and b"box6" in err, (fields, err)                             # without them; the matrix form with a stray one
    assert b"DFOL_FEATURES_ROWS_F32" in PI.run_empty(feature_form=F, src_row=8)[1] and b"DFOL_FEATURES_MATRIX" in PI.run_empty(src_row=8)[1]
    for bad in (-1, 6, 2 ** 31 - 1):
        rc, err = PI.run_empty(feature_form=bad, src_row=8, box6=8)
        assert rc != 0 and b"feature_form" in err and str(bad).encode() in err, (bad, err)
    # the model's gate table likewise (n_gates is the struct's LAST field: its refusals show that the ctypes layout and the C layout agree)
    assert PI.run_empty(model=dict(gates=8, n_gates=3))[0] == 0
    for fields in (dict(n_gates=-1), dict(gates=8, n_gates=-1), dict(gates=8, n_gates=0), dict(n_gates=2)):
        rc, err = PI.run_empty(model=fields)
        assert rc != 0 and b"n_gates" in err and ("%d gates" % fields["n_gates"]).encode() in err, (fields, err)
