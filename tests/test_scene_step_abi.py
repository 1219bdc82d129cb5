"""CPU-side checks of the listed pairs' kernels of the scene-graph step: the two entry points at the C-ABI boundary (header against the table,
argument for argument), their argument errors without a device, the registered operators' fake-tensor shapes, and the tensor-op route that CPU
tensors take."""

import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dfol_vqa.h")
ENTRY_POINTS = {"dfol_scene_pair_rows_f32": 10, "dfol_scene_pair_rows_bwd_f32": 10}
C_TYPES = {"const float*": "c_void_p", "float*": "c_void_p", "const int32_t*": "c_void_p", "void*": "c_void_p", "int32_t": "c_int", "int64_t": "c_long"}


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
        for a, ct in zip(args, lib.SIGNATURES[name]):
            assert C_TYPES[a.rsplit(" ", 1)[0]] == ct.__name__, (name, a, ct)
        assert hasattr(handle, name)
        comment = raw[:raw.index("int " + name)].rsplit("/*", 1)[1]   # the header cites the reference lines the kernels replace
        assert "batch_gqa_boxfeatures_pipeline.py:225-279" in comment and "No atomics" in comment, name
    assert handle.dfol_abi_version() == 4 == lib.ABI_VERSION           # (the entry points themselves were pure additions under 3)
    version_note = raw[:raw.index("#define DFOL_ABI_VERSION")].rsplit("/*", 1)[1]
    assert all(name in version_note for name in ENTRY_POINTS)
    assert "dfol_scene_pairs.hip" in open(os.path.join(ROOT, "dfol_vqa_amd", "csrc", "Makefile")).read()


def test_argument_errors_without_a_device(lib):
    h = lib.load()
    assert h.dfol_scene_pair_rows_f32(None, 8, 3, 8, None, None, 0, None, 20, None) == 0            # P = 0 launches nothing and asks for nothing
    assert h.dfol_scene_pair_rows_f32(None, 8, 3, 8, None, None, 2, None, 20, None) != 0
    assert b"scene_pair_rows" in h.dfol_last_error() and b"null pointer" in h.dfol_last_error()
    assert h.dfol_scene_pair_rows_f32(None, 8, 3, 8, None, None, 2, None, 19, None) != 0            # a row of 2 D + 4 does not fit
    assert b"bad sizes" in h.dfol_last_error()
    assert h.dfol_scene_pair_rows_f32(None, 8, 3, 3, None, None, 2, None, 20, None) != 0            # no room for the box columns
    assert h.dfol_scene_pair_rows_f32(None, 8, 0, 8, None, None, 2, None, 20, None) != 0
    assert b"no object" in h.dfol_last_error()
    assert h.dfol_scene_pair_rows_bwd_f32(None, 20, 2, 8, None, None, 0, None, 8, None) == 0        # no object row: nothing to write
    assert h.dfol_scene_pair_rows_bwd_f32(None, 20, 2, 8, None, None, 3, None, 8, None) != 0
    assert b"scene_pair_rows_bwd" in h.dfol_last_error() and b"null pointer" in h.dfol_last_error()
    assert h.dfol_scene_pair_rows_bwd_f32(None, 15, 2, 8, None, None, 3, None, 8, None) != 0
    assert b"bad sizes" in h.dfol_last_error()


def test_registered_ops_have_fake_formulas(lib):
    from dfol_vqa_amd import torch_ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        obj = torch.empty(7, 12)
        i32 = lambda n: torch.empty(n, dtype=torch.int32)
        rows = torch.ops.dfol.scene_pair_rows(obj, i32(5), i32(5), i32(8), i32(10))
        assert tuple(rows.shape) == (5, 28)
        d = torch.ops.dfol.scene_pair_rows_bwd(rows, i32(8), i32(10), 7, 12)
        assert tuple(d.shape) == (7, 12)


def test_cpu_tensors_take_the_tensor_op_expression(lib):
    from dfol_vqa_amd import data, ops
    rng = np.random.RandomState(0)
    # (values on a 2^-6 grid: every sum of the centre differences is exact, so a pair of one object with itself has distance exactly 0)
    obj = torch.as_tensor((rng.randint(0, 65, size=(6, 10)) / 64.0).astype(np.float32)).requires_grad_(True)
    s, o = np.asarray([0, 5, 2, 2], np.int32), np.asarray([1, 2, 2, 0], np.int32)
    csr = tuple(torch.from_numpy(a) for a in data.scene_pair_csr(s, o, 6))
    before = ops.PATH_COUNTS["scene_pair_rows_torch"]
    rows = ops.scene_pair_rows(obj, torch.from_numpy(s), torch.from_numpy(o), csr)
    assert ops.PATH_COUNTS["scene_pair_rows_torch"] == before + 1 and tuple(rows.shape) == (4, 24)
    want = ops.scene_pair_rows_reference(obj, torch.from_numpy(s.astype(np.int64)), torch.from_numpy(o.astype(np.int64)))
    assert torch.equal(rows, want)
    assert torch.equal(rows[2, 20:], torch.zeros(4))                   # s == o: distance 0, angle 0, sides 0
    rows.sum().backward()
    assert obj.grad[:, :6].sum().item() == 2 * 4 * 6                    # every pair row holds two object rows (the box columns also feed the geometry)
    assert tuple(ops.scene_pair_rows(obj, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), csr).shape) == (0, 24)
    with pytest.raises(lib.DfolError, match="no CPU fallback"):        # the raw kernels have none
        lib.scene_pair_rows(obj.detach(), torch.from_numpy(s), torch.from_numpy(o))
