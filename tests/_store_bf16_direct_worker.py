"""Child process of tests/test_store_bf16_direct_gpu.py: dfol_linear_wide_rows_bf16t_h2_f32 (csrc/dfol_dense_wide.hip, BF16T) against the code that
existed before it - `_lib.linear_wide` (dfol_linear_wide_h2_f32) over `table.float()[src_row]` - as uint32 bit patterns, no tolerance.  The library
reads DFOL_DENSE_WIDE once per process; the parent sets it to 2.

Tables hold NaN wherever the index does not point - unnamed rows, the padding of a row stride beyond K, the elements in front of an offset base -
so a read outside the named rows shows in the result.

usage: python tests/_store_bf16_direct_worker.py      prints one JSON line {section: {"cases": n, "failures": [...]}}."""
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from dfol_vqa_amd import _lib  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
NAN = float("nan")
ACTS = (_lib.ACT_NONE, _lib.ACT_SIGMOID, _lib.ACT_ELU, _lib.ACT_LOGSIGMOID)
MS, NS, KS = (1, 127, 128, 129, 300), (257, 300, 512), (128, 132, 164, 2048)
PATTERNS = ("identity", "reversed", "one_row")


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def index_of(pattern, M, R):
    if pattern == "identity":
        idx = torch.arange(M)
    elif pattern == "reversed":
        idx = torch.arange(R - 1, R - 1 - M, -1)                         # (names the table's last row)
    else:
        idx = torch.full((M,), R // 2)
    return idx.to(torch.int32)


def values(kind, n, K, g):
    """kind: "random" (bf16 normals with zeros and -0 planted), "tiny" (magnitudes near 2^-20: a non-zero low fp16 piece), "big" (one 2^17),
    "f16" (drawn from {0, +-[2^-10, 2^10]}: every value an fp16 value)."""
    v = torch.randn(n, K, generator=g)
    if kind == "f16":
        mag = torch.exp2(torch.rand(n, K, generator=g) * 20.0 - 10.0).clamp(2.0 ** -10, 2.0 ** 10)
        mag = mag.to(BF16).float().clamp(2.0 ** -10, 2.0 ** 10)           # (rounded first: the clamp's bounds are bf16 values)
        v = torch.where(v < 0, -mag, mag)
    if kind == "tiny":
        v = v * 2.0 ** -20
    v = v.to(BF16)
    flat = v.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    if kind == "big":
        flat[(n * K) // 2 + 1] = 2.0 ** 17
    return v


def table_of(R, K, ld, off, named, kind, g):
    """-> ([R, K] view of row stride ld whose first element lies `off` elements into a 256-byte aligned buffer, the buffer)."""
    buf = torch.full((off + R * ld,), NAN, dtype=BF16)
    view = buf[off:].view(R, ld)
    view[named, :K] = values(kind, named.numel(), K, g)
    buf = buf.to(DEV)
    return buf[off:].view(R, ld)[:, :K], buf


_WEIGHTS = {}


def weights_of(N, K):
    if (N, K) not in _WEIGHTS:
        g = torch.Generator(device="cpu").manual_seed(1000 * N + K)
        _WEIGHTS[N, K] = ((torch.randn(N, K, generator=g) / K ** 0.5).to(DEV), torch.randn(N, generator=g).to(DEV))
    return _WEIGHTS[N, K]


_WORD = None


def with_range_word(fn):
    """-> (fn(), the range status word its launches left)."""
    global _WORD
    if _WORD is None:
        _WORD = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    _WORD.zero_()
    lib.dfol_set_range_status(_WORD.data_ptr())
    try:
        out = fn()
    finally:
        lib.dfol_set_range_status(None)
    return out, int(_WORD.item())


class Store(object):
    """What linear_wide_rows_bf16t reads of a DeviceFeatureStore: its certificate."""

    def __init__(self, f16_exact):
        self.f16_exact = f16_exact


def case(M, N, K, ld, off, pattern, act, use_bias, kind, seed, sliced=False, store=None):
    """One comparison -> None or a description of what differs."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    R = M + 3
    idx = index_of(pattern, M, R)
    table, _keep = table_of(R, K, ld, off, torch.unique(idx.long()), kind, g)
    idx = idx.to(DEV)
    W, b = weights_of(N, K)
    b = b if use_bias else None
    where = dict(M=M, N=N, K=K, ld=ld, off=off, pattern=pattern, act=act, bias=use_bias, kind=kind, sliced=sliced,
                 store=None if store is None else store.f16_exact)
    kw = {} if store is None else {"store": store}
    if store is not None and store.f16_exact and not _lib.store_bf16_is_f16(_keep[off:].view(R, ld)[torch.unique(idx.long()).to(DEV), :K].contiguous()):
        return dict(where, what="the case's own table does not certify")
    if table.data_ptr() % 16 != (8 if off % 8 else 0):
        return dict(where, what="the table's base is not aligned as the case says")
    want, word0 = with_range_word(lambda: _lib.linear_wide(table.float()[idx.long()].contiguous(), W, b, act))
    if sliced:
        wide = torch.full((M, N + 5), -12345.5, device=DEV)
        _, word1 = with_range_word(lambda: _lib.linear_wide_rows_bf16t(table, idx, W, b, act, out=wide[:, 2:2 + N], **kw))
        got = wide[:, 2:2 + N]
        if not bool((wide[:, :2] == -12345.5).all()) or not bool((wide[:, 2 + N:] == -12345.5).all()):
            return dict(where, what="columns beside the out= slice were written")
    else:
        got, word1 = with_range_word(lambda: _lib.linear_wide_rows_bf16t(table, idx, W, b, act, **kw))
    if tuple(got.shape) != (M, N) or not np.array_equal(bits(got), bits(want)):
        return dict(where, what="outputs differ")
    if word0 != word1:
        return dict(where, what="range words differ: %d (yardstick) and %d" % (word0, word1))
    if kind == "big":
        # (ELU's fmaxf drops a NaN argument: there the flag alone tells)
        if not (word1 & _lib.RANGE_X_OVERFLOW) or not (act == _lib.ACT_ELU or bool(torch.isnan(want).any())):
            return dict(where, what="a table holding 2^17 must raise the flag and give NaN on both routes")
    elif word1 or not bool(torch.isfinite(want).all()):
        return dict(where, what="an in-range table gave flags %d or a non-finite yardstick" % word1)
    return None


def section(report, name, cases):
    fails, n = [], 0
    for c in cases:
        r = case(*c[0], **c[1]) if isinstance(c, tuple) and len(c) == 2 and isinstance(c[1], dict) else case(*c)
        n += 1
        if r is not None:
            fails.append(r)
    report[name] = {"cases": n, "failures": fails[:5], "failed": len(fails)}


def main():
    assert os.environ.get("DFOL_DENSE_WIDE") == "2"
    report = {}
    # every M x N x K x row stride x base offset; activations, bias and index patterns take turns
    grid = []
    for p, (M, N, K, pad, off) in enumerate(itertools.product(MS, NS, KS, (0, 4), (0, 4))):
        grid.append((M, N, K, K + pad, off, PATTERNS[p % 3], ACTS[(p // 3) % 4], p % 2 == 0, "random", p))
    section(report, "shapes", grid)
    # all four activations x bias x out= slice x index pattern on one shape of each load width, tail included
    combos = []
    for p, (act, use_bias, sliced, pattern) in enumerate(itertools.product(ACTS, (True, False), (False, True), PATTERNS)):
        for K, ld, off in ((128, 128, 0), (132, 136, 4), (164, 164, 0)):
            combos.append(((129, 300, K, ld, off, pattern, act, use_bias, "random", 5000 + p), dict(sliced=sliced)))
    section(report, "activations", combos)
    # values: a non-zero low piece everywhere; a value beyond fp16's range (the range word and the NaN bits)
    vals = []
    for p, (kind, (K, ld, off), M) in enumerate(itertools.product(("tiny", "big"), ((128, 128, 0), (132, 136, 4), (2048, 2048, 0), (2048, 2052, 4)), (1, 129, 300))):
        vals.append((M, 512 if p % 2 else 257, K, ld, off, PATTERNS[p % 2], ACTS[p % 4], True, kind, 9000 + p))
    section(report, "values", vals)
    # Part B.  The certificate: true for a table of fp16 values, false after one planted element that is not - a low piece fp16 cannot hold,
    # a value beyond its range, inf, NaN - at the first and at the last element
    g = torch.Generator(device="cpu").manual_seed(77)
    cert = values("f16", 301, 132, g).to(DEV)
    planted = {"clean": _lib.store_bf16_is_f16(cert), "empty": _lib.store_bf16_is_f16(cert[:0])}
    for name, bad in (("low_bits", 2.0 ** -20 * (1 + 2.0 ** -7)), ("beyond_range", 2.0 ** 17), ("inf", float("inf")), ("nan", NAN)):
        for where_, (r, c) in (("first", (0, 0)), ("last", (300, 131))):
            t = cert.clone()
            t[r, c] = bad
            assert float(t[r, c]) == bad or bad != bad, name                # (each planted value is a bf16 value)
            planted["%s_%s" % (name, where_)] = _lib.store_bf16_is_f16(t)
    report["certificate"] = planted
    # the two-product launch on certified tables over the whole shape list, and with every activation / slice / pattern
    section(report, "two_products", [(c[:8] + ("f16", c[9]), dict(store=Store(True))) for c in grid])
    section(report, "two_products_activations", [(c[0][:8] + ("f16", c[0][9]), dict(c[1], store=Store(True))) for c in combos])
    # a request for two products on an uncertified store runs three: tables whose low piece is not zero must still give the yardstick's bits
    # and a table holding 2^17: NaN and the range flag as the yardstick's
    section(report, "uncertified_request", [(c, dict(store=Store(False))) for c in vals])
    # more 128-row blocks than CUs: a workgroup goes on to a second block and reads src_row again at the transition
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    M, N, K, R = 128 * (cus + 1) + 5, 257, 128, 61
    g = torch.Generator(device="cpu").manual_seed(3)
    idx = torch.randint(0, R, (M,), generator=g).to(torch.int32)
    table, _keep = table_of(R, K, K + 4, 4, torch.unique(idx.long()), "random", g)
    W, b = weights_of(N, K)
    idx = idx.to(DEV)
    want = _lib.linear_wide(table.float()[idx.long()].contiguous(), W, b, _lib.ACT_SIGMOID)
    got = _lib.linear_wide_rows_bf16t(table, idx, W, b, _lib.ACT_SIGMOID)
    report["blocks"] = {"M": M, "equal": bool(np.array_equal(bits(got), bits(want))), "finite": bool(torch.isfinite(want).all())}
    del want, got
    # table rows beyond a 4 GB byte offset
    K = 2048
    R = (1 << 32) // (2 * K) + 9
    table = torch.empty((R, K), dtype=BF16, device=DEV)                   # uninitialised: only the named rows are written
    idx = torch.tensor([R - 1, 5, R - 3, 5, R - 1, 0, R - 2], dtype=torch.int32)
    named = torch.unique(idx.long())
    table[named.to(DEV)] = values("random", named.numel(), K, g).to(DEV)
    W, b = weights_of(257, K)
    idx = idx.to(DEV)
    want = _lib.linear_wide(table[idx.long()].float(), W, b, _lib.ACT_SIGMOID)
    got = _lib.linear_wide_rows_bf16t(table, idx, W, b, _lib.ACT_SIGMOID)
    report["beyond_4gb"] = {"past": bool((R - 3) * 2 * K >= 1 << 32), "equal": bool(np.array_equal(bits(got), bits(want))),
                            "finite": bool(torch.isfinite(want).all())}
    del table, want, got
    # refusals: before any launch, with a message
    K, N, M = 128, 300, 4
    tab = torch.zeros(16, 136, dtype=BF16, device=DEV)
    W, b = weights_of(N, K)
    packed = _lib.linear_pack_w_split(W, False, 2)
    idx = torch.arange(M, dtype=torch.int32, device=DEV)
    y = torch.full((M, N), -7.5, device=DEV)
    st = _lib._stream()
    refused = {}
    for name, (tp, ld, ip, wp, yp, k, word) in {
            "null_table": (None, 136, idx.data_ptr(), packed.data_ptr(), y.data_ptr(), K, "null pointer"),
            "null_index": (tab.data_ptr(), 136, None, packed.data_ptr(), y.data_ptr(), K, "null pointer"),
            "null_weight": (tab.data_ptr(), 136, idx.data_ptr(), None, y.data_ptr(), K, "null pointer"),
            "null_output": (tab.data_ptr(), 136, idx.data_ptr(), packed.data_ptr(), None, K, "null pointer"),
            "stride_not_4": (tab.data_ptr(), 134, idx.data_ptr(), packed.data_ptr(), y.data_ptr(), K, "multiple of 4"),
            "stride_below_K": (tab.data_ptr(), 124, idx.data_ptr(), packed.data_ptr(), y.data_ptr(), K, "bad sizes"),
            "K_not_4": (tab.data_ptr(), 136, idx.data_ptr(), packed.data_ptr(), y.data_ptr(), 130, "bad sizes"),
            "K_small": (tab.data_ptr(), 136, idx.data_ptr(), packed.data_ptr(), y.data_ptr(), 96, "bad sizes"),
            "table_not_8_byte": (tab.data_ptr() + 4, 136, idx.data_ptr(), packed.data_ptr(), y.data_ptr(), K, "8-byte")}.items():
        try:
            _lib.call("dfol_linear_wide_rows_bf16t_h2_f32", tp, ld, ip, wp, None, yp, N, M, N, k, 0, st)
            refused[name] = "not refused"
        except _lib.DfolError as e:
            refused[name] = True if word in str(e) else str(e)
    try:
        _lib.call("dfol_linear_wide_rows_bf16t_h2_f32", tab.data_ptr(), 136, idx.data_ptr(), packed.data_ptr(), None, y.data_ptr(), N, 0, N, K, 0, st)
        refused["M_zero"] = "not refused"
    except _lib.DfolError as e:
        refused["M_zero"] = True if "bad sizes" in str(e) else str(e)
    torch.cuda.synchronize()
    refused["nothing_launched"] = bool((y == -7.5).all())
    report["refusals"] = refused
    report["supported"] = [_lib.linear_wide_rows_bf16t_supported(300, 512, 2048, 2048), _lib.linear_wide_rows_bf16t_supported(300, 512, 2048, 2052),
                           _lib.linear_wide_rows_bf16t_supported(300, 512, 2048, 2050), _lib.linear_wide_rows_bf16t_supported(300, 512, 2048, 2044),
                           _lib.linear_wide_rows_bf16t_supported(300, 256, 2048, 2048), _lib.linear_wide_supported(300, 512, 2048)]
    print(json.dumps(report))


if __name__ == "__main__":
    main()
