"""The fused pair weight gradient's two SUMS forms (csrc/dfol_pair_wgrad.hip: pair_wgrad_fused_kernel<3, true> behind dfol_pair_wgrad_fused_sums_f32,
pair_wgrad_fused_kernel<4, true, true> behind dfol_pair_wgrad_fused_sums_bf16, and pair_sums_reduce_kernel) off the shapes they were born at:
more than 65 536 rows (row slabs WITHOUT rows), narrow and odd widths, a predicate boundary in every position of an octet, of a 32-row step and
of a slab, predicates without rows, dx = 0, dbe = NULL, a strided dE, and the launcher's guards.

    dW2 = dpre2^T Z,  db2 = column sums of dpre2,  dE[p] = sum over p's rows of dx h,  dbe[p] = sum over p's rows of dx,
    dpre2[r][j] = dx[r] E[p(r)][j] h (1 - h),  h = Sigmoid(pre2[r][j]).

Every call goes through _lib.call with a workspace the test sizes (dfol_pair_wgrad_fused_sums_workspace / dfol_pair_wgrad_fused_workspace) and FILLS WITH
NaN, every output pre-filled with NaN; pre2, Z, E and dE are column slices of wider NaN-filled matrices, dx has NaN behind its M values.  Whatever
the kernels read that they did not write, or read past an operand, shows as NaN.

References and bounds (the project's own):
  * fp32 storage against float64 on the device, test_pair_head_backward_without_dpre2's formulas: dW2 within 2^-20 (|dpre2|^T |Z|) + 2^-37 x (largest
    row bound |dx| max|E| / 4) x sum|Z|; dE, dbe, db2 per element within 4e-6 x the sum of the absolute terms + 1e-30.  The multi-reader form (case 1
    only) is held to the same dW2 formula with |dpre2| and the row bound summed over the readers.
  * bf16 storage against the materialised bf16 route on the same values (pair_logit_bwd, then linear_wgrad(bias=True) under dense_math("bf16")), the
    bounds of test_pair_wgrad_sums_bf16_storage_against_the_materialised_bf16_route: dW2 within 4e-6 |dpre2|^T |Z|, db2 within 4e-6 sum|dpre2|,
    dE and dbe within 2e-5 |ref| + 2e-5 max|ref|.
Beside every case the same sums and products are restated in float32 on the CPU and measured against float64: that error must stay below a quarter
of the bound; where it does not, that (case, quantity) is held to 8 x the restatement's largest error instead, wherever that is more than the project's
bound (test_pair_train_shapes_gpu.py's rule; printed as [8 x float32 bound]).
Every case asserts two bit-identical runs and prints its worst error / bound (pytest -s).

Measured on an MI355X (88 tests, 4.4 s for the whole file; the slowest, M = 65 537 at fp32, 1.5 s): every case passed, every pair of runs was
bit-identical.  Worst error over the PROJECT'S bound per group, and beside it the float32 restatement's error over the same bound:
     group (cases)                                  dW2            db2            dE             dbe
     empty slabs, fp32 sums 24 x 8 (2)              0.021 [0.541]  0.003 (0.002)  0.017 (0.082)  0.008 (0.050)
     empty slabs, bf16 sums 16 x 8 (2)              0.003 (0.125)  0.002 (0.001)  0.016 (0.113)  0.021 (0.030)
     empty slabs, no sums 24 x 8, 16 x 8 (4)        0.021 [0.541]
     empty slabs, two readers 24 x 8 (2)            0.013 [0.519]
     widths fp32 24x4 .. 312x256 (5)                0.326 [0.692]  0.017 (0.019)  0.041 (0.084)  0.036 (0.036)
     widths bf16 16x4 .. 320x256 (5)                0.031 (0.077)  0.011 (0.009)  0.021 (0.038)  0.012 (0.045)
     flush positions fp32 24 x 8 (18)               0.584 [0.609]  0.055 (0.042)  0.032 (0.082)  0.024 (0.024)
     flush positions bf16 16 x 8 (18)               0.036 (0.110)  0.018 (0.018)  0.024 (0.044)  0.014 (0.063)
     predicates of 32 .. 63 rows fp32 (12)          0.317 [0.719]  0.027 (0.027)  0.036 (0.081)  0.059 (0.059)
     predicates of 32 .. 63 rows bf16 (12)          0.044 (0.140)  0.020 (0.013)  0.010 (0.011)  0.000 (0.009)
[..]: the float32 restatement did not stay below a quarter of the project's bound, so the 8 x rule set the bound - for dW2 of 38 of the 41
fp32-storage cases and for nothing else (float32's 1 - h loses what the 2^-20 bound allows at a few dozen rows).  The rule was never what let a case
pass: the kernel stayed within 0.584 of the project's own dW2 bound everywhere (the worst: M64), and within 0.257 of the bound in force.  db2, dE,
dbe and everything in bf16 storage are held to the project's bounds as they are.

What the file found.  (1) The empty-slab read is real: the parent build on the rows of case 1 gives NaN in db2 of both sums forms at M = 80 640 and at
M = 65 537 (4 failed) and passes the forms without sums and the two-reader form (7 passed); with the workspace zero-filled the parent's and this
build's outputs are the same bits in all 48 tensors of a dump of 14 of these cases.  (2) Predicates of exactly 32, 33, 40 and 63 rows at octet
offsets 0, 1 and 7 meet the bounds of the 64-row cases: the kernel's own floor of 32 rows holds, the callers' 64 is margin.  (3) The Python guard
agrees with the entry points at every width tried.

Two mutants of csrc/dfol_pair_wgrad.hip, each built on a scratch copy and run once against this file (neither reads or writes out of bounds):
  * the flush condition of pair_a off by one row (`rr > end_cur` for `rr >= end_cur`): 68 of 88 fail - every sums case with a predicate boundary, or
    the end of the rows, anywhere but on the first row of a 32-row step (NaN left in a dE partial row, or dE beyond its bound).  What passes: the
    layouts whose boundaries all fall on a step's first row (first_64_then_64s, M64, predicates of 32 rows at offset 0), the forms without sums,
    the refusals and the guards.
  * the reduce's partial row index `s + p` replaced by `p`: 62 of 88 fail - every sums case with rows in more than one slab and a non-zero dx.  What
    passes: the one-slab layouts (M64, M65, M137, no_dbe, wide_dE), all_dx0 (every partial row is zero), the forms without sums, the refusals
    and the guards.
"""

import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64, BF, I32, I64 = torch.float32, torch.float64, torch.bfloat16, torch.int32, torch.int64
NAN = float("nan")
PAD = 4                                                   # spare NaN columns behind every operand

_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _free_cases():
    yield
    _CASES.clear()


# ---------------------------------------------------------------------------------------------------
# the launcher's slab arithmetic (pw_slabs, rows_per_slab), restated
# ---------------------------------------------------------------------------------------------------
def slabs_of(M):
    return max(1, min(256, (M + 255) // 256))


def rows_per_slab(M):
    return (-(-M // slabs_of(M)) + 31) & ~31


def used_slabs(M):
    return -(-M // rows_per_slab(M))


# ---------------------------------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------------------------------
class _Case(object):
    pass


def _wide(x, dtype, pad=PAD):
    """x [.., rows, cols] (CPU) -> the first `cols` columns of a NaN-filled [.., rows, cols + pad] on the device"""
    w = torch.full(tuple(x.shape[:-1]) + (x.shape[-1] + pad,), NAN, dtype=dtype)
    w[..., :x.shape[-1]] = x.to(dtype)
    return w.to(DEV)[..., :x.shape[-1]]


def _case(name, counts, h2, h1, bio, zero=None, nr=1):
    """Operands of one layout: predicates of `counts` rows, storage fp32 or (bio) bfloat16; zero: a predicate whose dx is 0, or "all"."""
    key = (name, h2, h1, bio, nr)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))
    c = _Case()
    c.id = "%s %s %dx%d" % (name, "bf16" if bio else "fp32", h2, h1) + (" readers %d" % nr if nr > 1 else "")
    c.name, c.counts, c.h2, c.h1, c.bio, c.nr = name, list(counts), h2, h1, bio, nr
    c.P, c.M = len(counts), int(sum(counts))
    M, P = c.M, c.P
    cnt = torch.tensor(c.counts, dtype=I64)
    rep = torch.repeat_interleave(torch.arange(P, dtype=I64), cnt)
    store = BF if bio else F32
    p2 = (2.5 * torch.randn(M, h2, generator=g)).to(store)
    z = torch.nn.functional.elu(2.0 * torch.randn(M, h1, generator=g)).to(store)
    E = 0.3 * torch.randn(nr, P, h2, generator=g)
    dx = torch.randn(nr, M, generator=g) * torch.pow(10.0, torch.randint(-2, 3, (nr, M), generator=g).float())
    if nr > 1:
        dx[1] *= 2.0 ** -3
    if zero == "all":
        dx.zero_()
    elif zero is not None:
        dx[:, rep == zero] = 0.0
    c.cpu = dict(p2=p2.float(), z=z.float(), E=E, dx=dx, rep=rep)
    c.p2, c.z, c.E, c.dx = _wide(p2, store), _wide(z, store), _wide(E, F32), _wide(dx, F32, 8)      # E [nr, P, .], dx [nr, M + 8]
    c.pred_off = torch.cat([torch.zeros(1, dtype=I64), cnt.cumsum(0)]).to(DEV)
    c.row_pred = rep.to(I32).to(DEV)
    c.rep = rep.to(DEV)
    # {S, 1 / S} as pair_head_products forms it for one reader; several readers: the library's own kernel
    if nr == 1:
        emax = c.E[0].abs().amax(1)
        bound = (c.dx[0, :M].abs() * emax.index_select(0, c.rep)).amax() * 0.25
        _, ex = torch.frexp(bound)
        ok = torch.isfinite(bound) & (bound > 0)
        sexp = torch.where(ok, (14 - ex).clamp(-100, 100), torch.zeros_like(ex)).to(F32)
        c.scale = torch.stack([torch.exp2(sexp), torch.exp2(-sexp)]).contiguous()
    else:
        emax = c.E.abs().amax(2).contiguous()
        c.scale = torch.empty(4, dtype=F32, device=DEV)
        L.call("dfol_pair_wgrad_multi_scale_f32", c.dx.data_ptr(), c.dx.stride(0), nr, c.row_pred.data_ptr(), emax.data_ptr(), P, M, c.scale.data_ptr(),
               L._stream())
    _CASES[key] = c
    return c


def _sums_of(dx, h, dp, absdp, z, rep, P):
    """The four results and the sums of their absolute terms, in the dtype and on the device of the arguments."""
    h2 = h.shape[1]
    zero = lambda *s: torch.zeros(*s, dtype=h.dtype, device=h.device)
    return dict(dw=dp.t() @ z, dw_mag=absdp.t() @ z.abs(), db2=dp.sum(0), db2_mag=absdp.sum(0),
                dE=zero(P, h2).index_add_(0, rep, dx[:, None] * h), dE_mag=zero(P, h2).index_add_(0, rep, (dx[:, None] * h).abs()),
                dbe=zero(P).index_add_(0, rep, dx), dbe_mag=zero(P).index_add_(0, rep, dx.abs()))


def _formulas(p2, z, E, dx, rep, P):
    """float64 or float32 restatement from the operands themselves: E [nr, P, H2], dx [nr, M]; the sums are reader 0's."""
    h = torch.sigmoid(p2)
    coef = sum(dx[k][:, None] * E[k].index_select(0, rep) for k in range(E.shape[0]))
    acoef = sum(dx[k].abs()[:, None] * E[k].abs().index_select(0, rep) for k in range(E.shape[0]))
    r = _sums_of(dx[0], h, coef * h * (1.0 - h), acoef * h * (1.0 - h), z, rep, P)
    r["row_bound"] = sum(dx[k].abs() * E[k].abs().amax(1).index_select(0, rep) for k in range(E.shape[0])).max() * 0.25
    return r


def _reference_fp32(c):
    """fp32 storage: float64 on the device, its bounds, and the float32 restatement on the CPU."""
    if hasattr(c, "ref"):
        return c.ref, c.tol, c.r32
    M, h2 = c.M, c.h2
    r = _formulas(c.p2.double(), c.z.double(), c.E.double(), c.dx[:, :M].double(), c.rep, c.P)
    tol = dict(dw=2.0 ** -20 * r["dw_mag"] + 2.0 ** -37 * r["row_bound"] * c.z.double().abs().sum(0)[None, :] + 1e-30,
               db2=4e-6 * r["db2_mag"] + 1e-30, dE=4e-6 * r["dE_mag"] + 1e-30, dbe=4e-6 * r["dbe_mag"] + 1e-30)
    u = c.cpu
    c.ref, c.tol, c.r32 = r, tol, _formulas(u["p2"], u["z"], u["E"], u["dx"], u["rep"], c.P)
    return c.ref, c.tol, c.r32


def _reference_bf16(c):
    """bf16 storage: the materialised bf16 route on the same values, its bounds; float64 and float32 of the same sums over the STORED dpre2."""
    if hasattr(c, "ref"):
        return c.ref, c.tol, c.r64, c.r32
    M = c.M
    dx = c.dx[0, :M].contiguous()
    with L.dense_math("bf16"):
        dp2, de, dbe = L.pair_logit_bwd(dx, c.p2.contiguous(), c.E[0].contiguous(), c.pred_off)
        dw, db2 = L.linear_wgrad(dp2, c.z.contiguous(), bias=True)
    ref = dict(dw=dw.double(), db2=db2.double(), dE=de.double(), dbe=dbe.double())
    mag = dp2.float().abs().t() @ c.z.float().abs()
    tol = dict(dw=4e-6 * mag.double() + 1e-30, db2=4e-6 * dp2.float().abs().sum(0).double() + 1e-30,
               dE=2e-5 * ref["dE"].abs() + 2e-5 * ref["dE"].abs().max() + 1e-30, dbe=2e-5 * ref["dbe"].abs() + 2e-5 * ref["dbe"].abs().max() + 1e-30)
    d64 = dp2.double()
    c.r64 = _sums_of(dx.double(), torch.sigmoid(c.p2.double()), d64, d64.abs(), c.z.double(), c.rep, c.P)
    u = c.cpu
    d32 = dp2.float().cpu()
    c.r32 = _sums_of(u["dx"][0], torch.sigmoid(u["p2"]), d32, d32.abs(), u["z"], u["rep"], c.P)
    c.ref, c.tol = ref, tol
    return c.ref, c.tol, c.r64, c.r32


# ---------------------------------------------------------------------------------------------------
# the entry points, NaN in everything they are handed
# ---------------------------------------------------------------------------------------------------
SUMS_ORDER = ["pre2", "ld_p2", "dx", "row_pred", "pred_off", "P", "E", "ld_e", "scale", "Z", "ld_z", "M", "H2", "H1", "ws", "dW", "dE", "ld_de", "dbe", "db2"]
PLAIN_ORDER = ["pre2", "ld_p2", "dx", "row_pred", "pred_off", "E", "ld_e", "scale", "Z", "ld_z", "M", "H2", "H1", "ws", "dW"]
MULTI_ORDER = ["pre2", "ld_p2", "dx", "dx_stride", "nr", "row_pred", "pred_off", "E", "ld_e", "P", "scale", "Z", "ld_z", "M", "H2", "H1", "ws", "dW"]


def _nan(*shape):
    return torch.full(shape, NAN, dtype=F32, device=DEV)


def _common(c):
    return dict(pre2=c.p2.data_ptr(), ld_p2=c.p2.stride(0), dx=c.dx.data_ptr(), dx_stride=c.dx.stride(0), nr=c.nr, row_pred=c.row_pred.data_ptr(),
                pred_off=c.pred_off.data_ptr(), P=c.P, E=c.E.data_ptr(), ld_e=c.E.stride(1), scale=c.scale.data_ptr(), Z=c.z.data_ptr(), ld_z=c.z.stride(0),
                M=c.M, H2=c.h2, H1=c.h1)


def _run_sums(c, dbe=True, de_pad=PAD, fill=NAN, out=None, **over):
    """dfol_pair_wgrad_fused_sums_f32 / _bf16 -> {dw, dE (with its spare columns), dbe, db2}; over: arguments replaced (the guards' tests);
    out: the outputs to write (a refused call returns nothing: its caller keeps them)"""
    out = out if out is not None else dict(dw=_nan(c.h2, c.h1), dE=_nan(c.P, c.h2 + de_pad), dbe=_nan(c.P), db2=_nan(c.h2))
    ws = torch.full((L.load().dfol_pair_wgrad_fused_sums_workspace(c.M, c.h2, c.h1, c.P),), fill, dtype=F32, device=DEV)
    a = _common(c)
    a.update(ws=ws.data_ptr(), dW=out["dw"].data_ptr(), dE=out["dE"].data_ptr(), ld_de=out["dE"].stride(0), dbe=out["dbe"].data_ptr() if dbe else None,
             db2=out["db2"].data_ptr())
    a.update(over)
    order = [k for k in SUMS_ORDER if not (c.bio and k == "scale")]
    L.call("dfol_pair_wgrad_fused_sums_bf16" if c.bio else "dfol_pair_wgrad_fused_sums_f32", *([a[k] for k in order] + [L._stream()]))
    return out


def _run_plain(c, fill=NAN, out=None, **over):
    out = out if out is not None else dict(dw=_nan(c.h2, c.h1))
    ws = torch.full((L.load().dfol_pair_wgrad_fused_workspace(c.M, c.h2, c.h1),), fill, dtype=F32, device=DEV)
    a = _common(c)
    a.update(ws=ws.data_ptr(), dW=out["dw"].data_ptr())
    a.update(over)
    L.call("dfol_pair_wgrad_fused_f32", *([a[k] for k in PLAIN_ORDER] + [L._stream()]))
    return out


def _run_multi(c, fill=NAN):
    out = dict(dw=_nan(c.h2, c.h1))
    ws = torch.full((L.load().dfol_pair_wgrad_fused_workspace(c.M, c.h2, c.h1),), fill, dtype=F32, device=DEV)
    a = _common(c)
    a.update(ws=ws.data_ptr(), dW=out["dw"].data_ptr())
    L.call("dfol_pair_wgrad_fused_multi_f32", *([a[k] for k in MULTI_ORDER] + [L._stream()]))
    return out


def _same_bits(a, b):
    return all(torch.equal(a[k].view(I32), b[k].view(I32)) for k in a)


def _all_nan(out):
    return all(bool(v.isnan().all()) for v in out.values())


# ---------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------
def _ratio(c, what, got, r64, tol, e32):
    """max |got - r64| / bound.  e32: the float32 restatement's error per element; where it does not stay below a quarter of the project's bound
    `tol`, the bound becomes 8 x the restatement's largest error wherever that is more (never less than the project's)."""
    assert bool(torch.isfinite(got).all()), (c.id, what, "not finite")
    err = (got.double() - r64).abs()
    ratio32, project = float((e32 / tol).max()), float((err / tol).max())
    fallback = ratio32 >= 0.25
    if fallback:
        tol = torch.maximum(tol, 8.0 * e32.max())
    ratio = float((err / tol).max())
    print("pair-wgrad-sums %-46s %-3s %.3f of its bound (%.3f of the project's; float32 on the CPU: %.3f of the project's)%s"
          % (c.id, what, ratio, project, ratio32, "  [8 x float32 bound]" if fallback else ""))
    return ratio


def _check(c, out, what=("dw", "db2", "dE", "dbe")):
    """Every quantity of `what` within its bound; dE's spare columns still NaN."""
    if c.bio:
        ref, tol, r64, r32 = _reference_bf16(c)
    else:
        ref, tol, r32 = _reference_fp32(c)
        r64 = ref
    worst = {}
    for k in what:
        got = out[k][:, :c.h2] if k == "dE" else out[k]
        worst[k] = _ratio(c, k, got, ref[k], tol[k], (r32[k].to(DEV).double() - r64[k]).abs())
    if "dE" in what:
        assert bool(out["dE"][:, c.h2:].isnan().all()), (c.id, "columns behind dE written")
    assert all(v <= 1.0 for v in worst.values()), (c.id, worst)
    return worst


def _sums_case(c, **kw):
    out = _run_sums(c, **kw)
    what = ("dw", "db2", "dE", "dbe") if kw.get("dbe", True) else ("dw", "db2", "dE")
    _check(c, out, what)
    assert _same_bits(out, _run_sums(c, **kw)), (c.id, "two runs differ")
    return out


# ---------------------------------------------------------------------------------------------------
# 1. row slabs without rows
# ---------------------------------------------------------------------------------------------------
BIG = {"M80640": [1260] * 64,                                                    # 64 images x 36 objects; the last slab with rows is exactly full
       "M65537": [8000, 9000, 7777, 0, 8192, 8192, 8192, 8192, 7992]}            # just over the cap of 256 slabs of 256 rows


def test_the_big_layouts_have_the_empty_slabs_they_were_written_for():
    assert (sum(BIG["M80640"]), rows_per_slab(80640), used_slabs(80640)) == (80640, 320, 252) and 252 * 320 == 80640         # m_begin == M in slab 252
    assert (sum(BIG["M65537"]), rows_per_slab(65537), used_slabs(65537)) == (65537, 288, 228) and 65537 - 227 * 288 == 161
    for M, empty in ((322560, 4), (80640, 4), (141312, 10), (65537, 28)):
        assert slabs_of(M) - used_slabs(M) == empty, M


@pytest.mark.parametrize("bio,h2,h1", [(False, 24, 8), (True, 16, 8)])
@pytest.mark.parametrize("name", sorted(BIG))
def test_empty_slabs_sums_forms(name, bio, h2, h1):
    _sums_case(_case(name, BIG[name], h2, h1, bio))


@pytest.mark.parametrize("h2,h1", [(24, 8), (16, 8)])
@pytest.mark.parametrize("name", sorted(BIG))
def test_empty_slabs_without_sums(name, h2, h1):
    c = _case(name, BIG[name], h2, h1, False)
    out = _run_plain(c)
    _check(c, out, ("dw",))
    assert _same_bits(out, _run_plain(c))


@pytest.mark.parametrize("name", sorted(BIG))
def test_empty_slabs_two_readers(name):
    c = _case(name, BIG[name], 24, 8, False, nr=2)
    out = _run_multi(c)
    _check(c, out, ("dw",))
    assert _same_bits(out, _run_multi(c))


# ---------------------------------------------------------------------------------------------------
# 2. widths
# ---------------------------------------------------------------------------------------------------
RAGGED = [70, 0, 64, 1207, 65, 0, 0, 97, 300]                                    # M = 1803: eight slabs of 256 rows, every predicate >= 64 rows or none


@pytest.mark.parametrize("h2,h1", [(24, 4), (36, 100), (192, 252), (300, 8), (312, 256)])
def test_widths_fp32_storage(h2, h1):
    _sums_case(_case("ragged", RAGGED, h2, h1, False))


@pytest.mark.parametrize("h2,h1", [(16, 4), (20, 12), (260, 128), (304, 256), (320, 256)])
def test_widths_bf16_storage(h2, h1):
    _sums_case(_case("ragged", RAGGED, h2, h1, True))


@pytest.mark.parametrize("h2", [16, 20, 320])
def test_fp32_sums_refuses_widths_that_are_no_multiple_of_three(h2):
    c = _case("ragged", RAGGED, h2, 8, False)
    assert _all_nan(_refused(c, _run_sums, "multiple of 3"))


def _refused(c, run, word, **over):
    """The call must raise a DfolError that says `word`, before any launch: -> the outputs it was handed, for the caller to find still NaN."""
    out = dict(dw=_nan(c.h2, c.h1), dE=_nan(c.P, c.h2 + PAD), dbe=_nan(c.P), db2=_nan(c.h2))
    with pytest.raises(L.DfolError) as e:
        run(c, out=out, **over)
    assert word in str(e.value), str(e.value)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------
# 3. where the running sums are flushed
# ---------------------------------------------------------------------------------------------------
RPS_1000 = rows_per_slab(1000)                                                   # 256: four slabs
LAYOUTS = {}
for _k in (0, 1, 7, 8, 9, 31):                                                   # a boundary at every position of an octet and of a 32-row step
    LAYOUTS["first_%d_then_64s" % (64 + _k)] = dict(counts=[64 + _k] + [64] * 5)
for _d, _n in ((0, "on_the_slabs_last_row"), (-1, "one_row_before_the_slabs_end"), (1, "one_row_into_the_next_slab")):
    LAYOUTS["boundary_" + _n] = dict(counts=[RPS_1000 + _d, 300, 1000 - 300 - RPS_1000 - _d])
LAYOUTS.update({
    "empty_predicates": dict(counts=[0, 100, 0, 0, 156, 0, 300, 444, 0]),          # first, last, two in a row, one on the slab edge at row 256
    "one_predicate_3000": dict(counts=[3000]),                                     # twelve slabs
    "M64": dict(counts=[64]),
    "M65": dict(counts=[65]),
    "M137": dict(counts=[70, 67]),                                                 # no multiple of 8
    "one_predicate_dx0": dict(counts=[100, 80, 120], zero=1),
    "all_dx0": dict(counts=[100, 80, 120], zero="all"),
    "no_dbe": dict(counts=[70, 0, 90, 64], dbe=False),
    "wide_dE": dict(counts=[70, 0, 90, 64], de_pad=36),
})


@pytest.mark.parametrize("bio,h2,h1", [(False, 24, 8), (True, 16, 8)])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_flush_positions(name, bio, h2, h1):
    lay = LAYOUTS[name]
    assert RPS_1000 == 256 and sum(LAYOUTS["empty_predicates"]["counts"][:5]) == RPS_1000
    c = _case(name, lay["counts"], h2, h1, bio, zero=lay.get("zero"))
    kw = {k: lay[k] for k in ("dbe", "de_pad") if k in lay}
    out = _sums_case(c, **kw)
    for p, n in enumerate(c.counts):
        if n == 0 or lay.get("zero") in (p, "all"):                               # no rows, or no gradient: exact zeros
            assert not bool(out["dE"][p, :h2].any()), (c.id, p)
            assert kw.get("dbe", True) is False or float(out["dbe"][p]) == 0.0, (c.id, p)
    if lay.get("zero") == "all":
        assert not bool(out["dw"].any()) and not bool(out["db2"].any()), c.id
    if kw.get("dbe", True) is False:
        assert bool(out["dbe"].isnan().all()), c.id


# ---------------------------------------------------------------------------------------------------
# 4. the kernel's own floor: 32 rows per predicate (callers check 64)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bio,h2,h1", [(False, 24, 8), (True, 16, 8)])
@pytest.mark.parametrize("off", [0, 1, 7])
@pytest.mark.parametrize("n", [32, 33, 40, 63])
def test_predicates_below_64_rows(n, off, bio, h2, h1):
    _sums_case(_case("floor_%d_at_%d" % (n, off), [64 + off] + [n] * 7 + [64], h2, h1, bio))


# ---------------------------------------------------------------------------------------------------
# 5. guards (nothing here launches a kernel)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sums_f32", "sums_bf16", "plain_f32"])
def test_bad_arguments_raise_and_launch_nothing(form):
    bio = form == "sums_bf16"
    h2, h1 = (16, 8) if bio else (24, 8)
    c = _case("guards", [70, 0, 90, 64], h2, h1, bio)
    run = _run_plain if form == "plain_f32" else _run_sums
    bad = [(dict(ld_p2=h2 - 4), "row strides"), (dict(ld_z=h1 - 4), "row strides"), (dict(ld_e=h2 - 4), "row strides"), (dict(pre2=None), "null pointer"),
           (dict(Z=None), "null pointer"), (dict(ws=None), "null pointer")]
    bad += [(dict(H2=v), "bad sizes") for v in (0, 2)] + [(dict(H1=v), "bad sizes") for v in (0, 2, 260)]
    bad += [(dict(H2=324), "bad sizes" if form == "plain_f32" else "bad arguments")]          # (the sums forms' own check of H2 <= 320 comes first)
    if form != "plain_f32":
        bad += [(dict(ld_de=h2 - 4), "bad arguments"), (dict(P=0), "bad arguments"), (dict(dE=None), "bad arguments"), (dict(db2=None), "bad arguments")]
    for over, word in bad:
        assert _all_nan(_refused(c, run, word, **over)), (form, over)


def _sizes_accepted(name, *args):
    """The entry point's verdict on the SIZES alone: every operand is a null pointer, so an accepted size ends in `null pointer` (or, with no
    rows / predicates, returns before the operands are looked at)."""
    try:
        L.call(name, *args)
    except L.DfolError as e:
        return "null pointer" in str(e)
    return True


def test_python_guard_agrees_with_the_entry_points():
    for hid1 in (0, 2, 4, 6, 8, 252, 256, 260):
        for hid2 in (0, 2, 4, 12, 14, 16, 20, 300, 318, 320, 324):
            l1, l2 = (hid1 + 3) // 4 * 4, (hid2 + 3) // 4 * 4                        # legal row strides whatever the width
            st = L._stream()
            accept = [_sizes_accepted("dfol_pair_wgrad_fused_f32", None, l2, None, None, None, None, l2, None, None, l1, 64, hid2, hid1, None, None, st),
                      _sizes_accepted("dfol_pair_dz_fused_f32", None, l2, None, None, None, l2, None, None, None, l1, 0, hid1, hid2, 0, st),
                      _sizes_accepted("dfol_pair_logit_bwd_sums_f32", None, None, l2, hid2, None, l2, None, 0, None, l2, None, None, l2, st)]
            assert L.pair_head_fused_supported(hid1, hid2) == all(accept), (hid1, hid2, accept)
