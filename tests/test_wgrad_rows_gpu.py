"""GPU tests of the weight gradient over indexed rows (csrc/dfol_dense_wgrad.hip, ROWS: dfol_linear_wgrad_bias_rows_f32 / _bf16) against the
matrix kernel over the gathered matrix.  Every comparison is bit equality: only the address of an X row differs between the two forms.

Every table row the index does not name, the table's padding columns, the gathered matrix's six extra columns and the workspace hold NaN: a
read past M, outside the index or of an unwritten partial shows in dW / db.

The row counts: 1, 15, 16, 17 (around the 16-row MFMA step), 257, and one where the rows are cut into more slabs than a single row gets.
dfol_linear_wgrad_slabs never returns 2 (the fp32-pipe kernel's four wavefront slabs are its floor), so that count is the first M at which
the library's answer grows beyond its answer for M = 1, asked of the library, plus two rows (a second slab shorter than the first)."""

import numpy as np
import pytest
import torch

import dfol_vqa_amd as D  # noqa: F401
from dfol_vqa_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
# (N, K): one block; one block with a full k-step; 2 x 3 blocks with a boundary inside a 128-block both ways (a last group of two blocks that
# split their rows, a narrow last row block); two blocks (nb % 4 == 2); five blocks (a full group and a last group of one: nb % 4 == 1)
SHAPES = [(4, 4), (8, 128), (132, 260), (8, 256), (12, 516)]
FLAGSHIP = (512, 2048)                                      # the workload's featurizer, at M = 257 only
PATTERNS = ("ascending", "descending", "repeats", "all_equal", "first_last")


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def first_growth(N, K):
    """The smallest M at which dfol_linear_wgrad_slabs(M, N, K) exceeds its value at M = 1 (the library cuts the rows into more slabs)."""
    lib = _lib.load()
    base, hi = lib.dfol_linear_wgrad_slabs(1, N, K), 2
    while lib.dfol_linear_wgrad_slabs(hi, N, K) == base:
        hi *= 2
        assert hi < (1 << 24), "the slab count never grows"
    lo = hi // 2                                            # slabs(lo) == base < slabs(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.dfol_linear_wgrad_slabs(mid, N, K) == base else (lo, mid)
    return hi


def index_of(pattern, M, R, g):
    if pattern == "ascending":
        idx = torch.sort(torch.randperm(R, generator=g)[:M]).values
    elif pattern == "descending":
        idx = torch.sort(torch.randperm(R, generator=g)[:M], descending=True).values
    elif pattern == "repeats":                              # shared scenes: runs of rows named twice, out of order
        idx = torch.randint(0, R, ((M + 2) // 3,), generator=g).repeat(3)[:M]
    elif pattern == "all_equal":
        idx = torch.full((M,), int(torch.randint(0, R, (1,), generator=g)))
    else:                                                   # the table's first and last row, wherever M allows both
        idx = torch.randint(0, R, (M,), generator=g)
        idx[0] = R - 1
        idx[-1] = 0 if M > 1 else R - 1
    return idx.to(torch.int32)


def operands(M, N, K, pattern, seed):
    """dY [M, N]; a NaN table [R >= 8 M, K + 10] with the named rows' first K columns filled; src_row; the gathered matrix [M, K + 6] (NaN beyond K)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    R, ld = 8 * M + 3, K + 10
    idx = index_of(pattern, M, R, g)
    table = torch.full((R, ld), NAN)
    named = torch.unique(idx.long())
    table[named, :K] = torch.randn(named.numel(), K, generator=g)
    dy = torch.randn(M, N, generator=g) * 0.1
    mat = torch.full((M, K + 6), NAN)
    mat[:, :K] = table[idx.long(), :K]
    return dy.to(DEV), table.to(DEV), idx.to(DEV), mat.to(DEV)


def run(name, dy, x, ld_x, src_row, M, N, K, want_db):
    """One call of a wgrad entry point (src_row None: the matrix form) with a NaN workspace and NaN results -> (dW, db or None)."""
    lib = _lib.load()
    ws = torch.full((lib.dfol_linear_wgrad_workspace(M, N, K),), NAN, device=DEV)
    dw = torch.full((N, K), NAN, device=DEV)
    db = torch.full((N,), NAN, device=DEV) if want_db else None
    tail = (M, N, K, ws.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(), _lib._stream())
    if src_row is None:
        _lib.call(name, dy.data_ptr(), dy.stride(0), x.data_ptr(), ld_x, *tail)
    else:
        _lib.call(name, dy.data_ptr(), dy.stride(0), x.data_ptr(), ld_x, src_row.data_ptr(), *tail)
    return dw, db


def check(M, N, K, mode, pattern, want_db, seed):
    dy, table, idx, mat = operands(M, N, K, pattern, seed)
    where = (M, N, K, mode, pattern, want_db)
    assert _lib.linear_wgrad_rows_supported(N, K, dy.stride(0), table.stride(0)), where
    dw0, db0 = run("dfol_linear_wgrad_bias_" + mode, dy, mat, mat.stride(0), None, M, N, K, want_db)
    dw1, db1 = run("dfol_linear_wgrad_bias_rows_" + mode, dy, table, table.stride(0), idx, M, N, K, want_db)
    assert bool(torch.isfinite(dw0).all()) and bool(torch.isfinite(dw1).all()), where
    assert np.array_equal(bits(dw0), bits(dw1)), where
    if want_db:
        assert bool(torch.isfinite(db1).all()) and np.array_equal(bits(db0), bits(db1)), where
    return dw1


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_rows_form_equals_matrix_form(shape, mode):
    N, K = shape
    grown = first_growth(N, K)
    assert _lib.load().dfol_linear_wgrad_slabs(grown, N, K) > _lib.load().dfol_linear_wgrad_slabs(grown - 1, N, K)
    for M in (1, 15, 16, 17, 257, grown + 2):
        for p, pattern in enumerate(PATTERNS):
            check(M, N, K, mode, pattern, want_db=(M + p) % 2 == 0, seed=1000 * M + p)     # (db == NULL on every other case)
    # ... and the product is the right one: against float64, within the worst case of the arithmetic relative to max sum |dy| |x| - 257 fp32
    # additions (257 x 2^-24 < 2^-15, the split pieces' own error is below that), in the bf16 mode two operands rounded to 8 bits (2 x 2^-9) on top
    dy, table, idx, mat = operands(257, N, K, "repeats", 5)
    dw, _ = run("dfol_linear_wgrad_bias_rows_" + mode, dy, table, table.stride(0), idx, 257, N, K, False)
    ref = dy.double().t() @ mat[:, :K].double()
    scale = float((dy.double().abs().t() @ mat[:, :K].double().abs()).max())
    assert float((dw.double() - ref).abs().max()) <= (2.0 ** -7 if mode == "bf16" else 2.0 ** -15) * scale


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_rows_form_at_the_featurizer_shape(mode):
    N, K = FLAGSHIP
    for p, pattern in enumerate(PATTERNS):
        check(257, N, K, mode, pattern, want_db=p % 2 == 0, seed=70 + p)


def test_host_wrapper_equals_linear_wgrad():
    """_lib.linear_wgrad_rows against _lib.linear_wgrad over the gathered matrix, in both dense arithmetics (the wrappers' own mode choice)."""
    M, N, K = 300, 256, 260                                 # (a weight of SPLIT_MIN_WEIGHT elements or more: the bf16 mode applies to it)
    assert N * K >= _lib.SPLIT_MIN_WEIGHT
    dy, table, idx, mat = operands(M, N, K, "repeats", 9)
    for math in ("f16x2", "bf16"):
        with _lib.dense_math(math):
            dw0, db0 = _lib.linear_wgrad(dy, mat[:, :K], bias=True)
            dw1, db1 = _lib.linear_wgrad_rows(dy, table[:, :K], idx, bias=True)
            dw2 = _lib.linear_wgrad_rows(dy, table[:, :K], idx)
        assert np.array_equal(bits(dw0), bits(dw1)) and np.array_equal(bits(db0), bits(db1)) and np.array_equal(bits(dw1), bits(dw2)), math
    with _lib.dense_math("f16x2"):
        a = _lib.linear_wgrad_rows(dy, table[:, :K], idx)
    with _lib.dense_math("bf16"):
        b = _lib.linear_wgrad_rows(dy, table[:, :K], idx)
    assert not np.array_equal(bits(a), bits(b))              # the modes differ
    dw, db = _lib.linear_wgrad_rows(dy[:0], table[:, :K], idx[:0], bias=True)
    assert tuple(dw.shape) == (N, K) and not bool(dw.any()) and not bool(db.any())


def test_refusals(monkeypatch):
    """Everything outside the bf16-pipe kernel's conditions raises DfolError before any launch (dW keeps its sentinel), and the predicate
    says so for what it can see (sizes and strides; pointers and M are the entry point's)."""
    M, N, K = 17, 8, 128
    dy, table, idx, _ = operands(M, N, K, "ascending", 3)
    ld_t = table.stride(0)
    lib = _lib.load()
    ws = torch.full((lib.dfol_linear_wgrad_workspace(64, 16, 256),), NAN, device=DEV)
    dw = torch.full((16 * 256,), -7.5, device=DEV)
    wide_dy = torch.zeros(M, N + 2, device=DEV)
    off_dy = torch.zeros(M * N + 4, device=DEV)[1:]         # 4 bytes past a 16-byte boundary

    def refused(mode, dy_ptr, ld_dy, tab_ptr, ld_table, idx_ptr, m, n, k, what):
        with pytest.raises(_lib.DfolError, match=what):
            _lib.call("dfol_linear_wgrad_bias_rows_" + mode, dy_ptr, ld_dy, tab_ptr, ld_table, idx_ptr, m, n, k, ws.data_ptr(), dw.data_ptr(), None,
                      _lib._stream())

    for mode in ("f32", "bf16"):
        p = (dy.data_ptr(), N, table.data_ptr(), ld_t, idx.data_ptr())
        refused(mode, *p, M, 6, K, "multiples of 4")
        refused(mode, *p, M, N, 126, "multiples of 4")
        refused(mode, wide_dy.data_ptr(), N + 2, *p[2:], M, N, K, "16-byte aligned")
        refused(mode, off_dy.data_ptr(), N, *p[2:], M, N, K, "16-byte aligned")
        refused(mode, p[0], p[1], p[2], K - 4, p[4], M, N, K, "shorter than K")
        refused(mode, p[0], p[1], p[2], p[3], None, M, N, K, "null pointer")
        refused(mode, *p, 1 << 31, N, K, "bad sizes")
        refused(mode, *p, 0, N, K, "bad sizes")
        refused(mode, p[0], p[1], p[2], 1 << 25, p[4], M, N, K, "row stride too large")
    assert not _lib.linear_wgrad_rows_supported(6, K, 8, ld_t) and not _lib.linear_wgrad_rows_supported(N, 126, N, ld_t)
    assert not _lib.linear_wgrad_rows_supported(N, K, N + 2, ld_t) and not _lib.linear_wgrad_rows_supported(N, K, N, K - 4)
    assert not _lib.linear_wgrad_rows_supported(N, K, N, 1 << 25) and _lib.linear_wgrad_rows_supported(N, K, N, ld_t)
    monkeypatch.setenv("DFOL_WGRAD_MATH", "f32")            # the fp32 matrix pipe has no indexed form, in either mode
    assert not _lib.linear_wgrad_rows_supported(N, K, N, ld_t)
    for mode in ("f32", "bf16"):
        refused(mode, dy.data_ptr(), N, table.data_ptr(), ld_t, idx.data_ptr(), M, N, K, "DFOL_WGRAD_MATH=f32")
    monkeypatch.delenv("DFOL_WGRAD_MATH")
    assert _lib.linear_wgrad_rows_supported(N, K, N, ld_t)
    torch.cuda.synchronize()
    assert bool((dw == -7.5).all())                          # nothing was launched
