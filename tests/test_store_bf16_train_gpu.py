"""GPU tests of the DEFAULT arithmetic's weight gradient over the indexed rows of a bf16 table: dfol_linear_wgrad_bias_rows_bf16t_x3
(csrc/dfol_dense_wgrad.hip: dY in three bf16 pieces, a table value its own one piece, three of the six piece products) against
dfol_linear_wgrad_bias_f32 over `table.float()[src_row]`, the kernel that splits both operands and issues all six.  Every comparison is bit
equality: the three products left out multiply by a zero piece, and an accumulator that starts at +0 stays what it was under +-0.

That argument is what these inputs are after: dY and the table hold +0 and -0 beside values of both signs, dY has one row of -0 only, and a third
of dY's columns is scaled by 2^12, a third by 2^-12, so that the h, m and l pieces of dY all carry bits.  Inputs are finite.  Every table row
the index does not name, the table's padding, the gathered matrix's six extra columns, the workspace and the results hold NaN before the call."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfol_vqa_amd as D  # noqa: E402,F401
from dfol_vqa_amd import _lib  # noqa: E402
from test_wgrad_rows_gpu import PATTERNS, SHAPES, first_growth, index_of  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
BF16 = torch.bfloat16
# test_wgrad_rows_gpu's shapes (the narrow last row block, the K tail, one or two blocks in the last group) and a last row block of 44 rows
ALL_SHAPES = SHAPES + [(300, 260), (512, 2048)]


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def signed_zeros(t, g, every):
    """About one entry in `every` of t becomes +0 and as many -0 (in place) -> t."""
    r = torch.randint(0, every, t.shape, generator=g)
    t[r == 0] = 0.0
    t[r == 1] = -0.0
    return t


def inputs(M, N, K, pattern, seed):
    """-> dY [M, N] fp32, table [R, ld] bf16 (NaN outside the named rows' first K columns), src_row [M], the gathered matrix [M, K + 6]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    R, ld = 8 * M + 3, K + 12
    idx = index_of(pattern, M, R, g)
    named = torch.unique(idx.long())
    table = torch.full((R, ld), NAN, dtype=BF16)
    table[named, :K] = signed_zeros(torch.randn(named.numel(), K, generator=g), g, 7).to(BF16)
    dy = torch.randn(M, N, generator=g) * 0.1
    col = torch.arange(N) % 3
    dy[:, col == 1] *= 2.0 ** 12
    dy[:, col == 2] *= 2.0 ** -12
    signed_zeros(dy, g, 9)
    if M > 1 or seed % 2 == 0:                                            # one row of -0 only (M = 1: it is all of dY, so every other case)
        dy[M // 2] = -0.0
    dy, table, idx = dy.to(DEV), table.to(DEV), idx.to(DEV)
    mat = torch.full((M, K + 6), NAN, device=DEV)
    mat[:, :K] = table.float()[idx.long(), :K]
    return dy, table, idx, mat, ld


def wgrad_case(M, N, K, pattern, want_db, seed):
    dy, table, idx, mat, ld = inputs(M, N, K, pattern, seed)
    where = (M, N, K, pattern, want_db)
    assert bool(torch.isfinite(dy).all()) and bool(torch.isfinite(mat[:, :K]).all()), where
    if M > 1:                                                            # (-0 and +0 are there wherever the sizes leave no doubt)
        assert bool((bits(dy[M // 2]) == 0x80000000).all()), where
    if M * N >= 512:
        assert bool((bits(dy) == 0).any()), where
    if M * K >= 512 and pattern != "all_equal":
        assert bool((bits(mat[:, :K]) == 0x80000000).any()) and bool((bits(mat[:, :K]) == 0).any()), where
    lib, out = _lib.load(), []
    assert _lib.linear_wgrad_rows_bf16t_x3_supported(N, K, N, ld), where
    for rows_form in (False, True):
        ws = torch.full((lib.dfol_linear_wgrad_workspace(M, N, K),), NAN, device=DEV)
        dw = torch.full((N, K), NAN, device=DEV)
        db = torch.full((N,), NAN, device=DEV) if want_db else None
        tail = (M, N, K, ws.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(), _lib._stream())
        if rows_form:
            _lib.call("dfol_linear_wgrad_bias_rows_bf16t_x3", dy.data_ptr(), N, table.data_ptr(), ld, idx.data_ptr(), *tail)
        else:
            _lib.call("dfol_linear_wgrad_bias_f32", dy.data_ptr(), N, mat.data_ptr(), K + 6, *tail)
        out.append((dw, db))
    (dw0, db0), (dw1, db1) = out
    assert bool(torch.isfinite(dw0).all()) and bool(torch.isfinite(dw1).all()), where
    diff = bits(dw0) != bits(dw1)
    assert not diff.any(), (where, int(diff.sum()), bits(dw0)[diff][:4], bits(dw1)[diff][:4])
    if want_db:
        assert bool(torch.isfinite(db0).all()) and bool(torch.isfinite(db1).all()) and np.array_equal(bits(db0), bits(db1)), where


@pytest.fixture(autouse=True)
def default_arithmetic(monkeypatch):
    for k in ("DFOL_WGRAD_MATH", "DFOL_DENSE_MATH"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_three_products_over_the_table_equal_six_over_the_widened_rows(shape):
    N, K = shape
    # around the 16-row MFMA step; 20 and 27: the range ends inside the eight rows of a lane of the first / second half; more slabs than one row gets
    Ms = (257,) if shape == (512, 2048) else (1, 15, 16, 17, 20, 27, 257, first_growth(N, K) + 2)
    for M in Ms:
        for p, pattern in enumerate(PATTERNS):
            wgrad_case(M, N, K, pattern, (M + p) % 2 == 0, 1000 * M + p)


def test_host_wrapper():
    M, N, K = 300, 256, 260
    dy, table, idx, mat, ld = inputs(M, N, K, "repeats", 9)
    with _lib.dense_math("f16x2"):
        dw0, db0 = _lib.linear_wgrad(dy, table.float()[idx.long(), :K], bias=True)
        dw1, db1 = _lib.linear_wgrad_rows_bf16t_x3(dy, table[:, :K], idx, bias=True)
        only_dw = _lib.linear_wgrad_rows_bf16t_x3(dy, table[:, :K], idx)
    assert bool(torch.isfinite(dw0).all()) and np.array_equal(bits(dw0), bits(dw1)) and np.array_equal(bits(db0), bits(db1))
    assert np.array_equal(bits(only_dw), bits(dw0))
    with pytest.raises(_lib.DfolError, match="bfloat16 GPU table"):       # an fp32 table is linear_wgrad_rows'
        _lib.linear_wgrad_rows_bf16t_x3(dy, table.float()[:, :K], idx)
    with pytest.raises(_lib.DfolError, match="src_row has"):
        _lib.linear_wgrad_rows_bf16t_x3(dy, table[:, :K], idx[:-1])
    with pytest.raises(_lib.DfolError, match="bf16 mode applies"):        # the bf16 mode's form is linear_wgrad_rows over the same table
        with _lib.dense_math("bf16"):
            _lib.linear_wgrad_rows_bf16t_x3(dy, table[:, :K], idx)


def test_no_rows_no_launch(monkeypatch):
    N, K = 256, 260
    table = torch.full((8, K), NAN, dtype=BF16, device=DEV)
    dy, idx = torch.zeros(0, N, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "call", no_call)
    dw, db = _lib.linear_wgrad_rows_bf16t_x3(dy, table, idx, bias=True)
    assert tuple(dw.shape) == (N, K) and tuple(db.shape) == (N,) and not bool(dw.any()) and not bool(db.any())


def test_refusals_name_their_reason(monkeypatch):
    M, N, K = 20, 256, 260
    dy, table, idx, mat, ld = inputs(M, N, K, "ascending", 3)
    ws = torch.full((_lib.load().dfol_linear_wgrad_workspace(M, N, K),), NAN, device=DEV)
    dw = torch.full((N, K), -7.5, device=DEV)
    tail = (M, N, K, ws.data_ptr(), dw.data_ptr(), None, _lib._stream())
    with pytest.raises(_lib.DfolError, match=r"linear_wgrad_rows_bf16t_x3: .*ld_table % 4"):
        _lib.call("dfol_linear_wgrad_bias_rows_bf16t_x3", dy.data_ptr(), N, table.data_ptr(), K + 2, idx.data_ptr(), *tail)
    assert not _lib.linear_wgrad_rows_bf16t_x3_supported(N, K, N, K + 2) and not _lib.linear_wgrad_rows_bf16t_x3_supported(N, 258, N, 260)
    monkeypatch.setenv("DFOL_WGRAD_MATH", "f32")
    assert not _lib.linear_wgrad_rows_bf16t_x3_supported(N, K, N, ld)
    with pytest.raises(_lib.DfolError, match="DFOL_WGRAD_MATH=f32"):
        _lib.call("dfol_linear_wgrad_bias_rows_bf16t_x3", dy.data_ptr(), N, table.data_ptr(), ld, idx.data_ptr(), *tail)
    torch.cuda.synchronize()
    assert bool((dw == -7.5).all())                                       # nothing was launched
