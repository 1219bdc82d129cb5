"""The answer-side kernels at the tail of csrc/dfol_logic.hip off their one shape: quantify (soft and hard), find_max_ind, segment_or (both
forms), the option normalisation and the two gathers in the forward, and the row-wise kernels (gate, gather_rows, select_rows, parametric_not,
implication, logic, compare, modulate) - every one called through dfol_vqa_amd._lib and compared with a plain numpy / torch restatement of the
reference's formula (oracle/dfol_oracle.py, golden_util.t_*) in float64, with the same formula in float32 beside it as the yardstick of
golden_util.check_logprob.  Copies and selects are compared bit for bit.

dfol_quantify_fwd_f32 dispatches on NS; a workgroup of quantify_fwd4_kernel<LPP> (4 wavefronts, QUANT_UNR = 4 groups in flight, 64 / LPP
predicates per group) holds G = 4 * QUANT_UNR * (64 / LPP) predicates, and every NS runs with P = G - 1, G, G + 1 and 2 G + 3:

      NS   NS / 4   LPP     G    dead lanes (col_ok == false)
       4        1     1  1024    -
       8        2     2   512    -
      12        3     4   256    1 of 4
      16        4     4   256    -
      20        5     8   128    3 of 8
      32        8     8   128    -
      36        9    16    64    7 of 16
      64       16    16    64    -
     100       25    32    32    7 of 32
     128       32    32    32    -
     132       33    64    16    31 of 64
     256       64    64    16    -
     260, 300  > 64  quantify_fwd_kernel (a wavefront per predicate, 4 per workgroup: G = 4)
      10   NS % 4 != 0: quantify_fwd_kernel (G = 4)

The group sizes rest on QUANT_UNR = 4 in csrc/dfol_logic.hip; the test reads the constant from the source and fails if it moves.

Inputs: attentions are non-positive log-probabilities of dfol_vqa_amd.synthetic.table_log_likelihood (beyond 100 objects in the rescaling
of test_logic_backward_gpu._likelihood), the family chosen by the object count so that an EXISTS aggregate is not saturated (asserted on
the float64 reference before the device is asked: at least half of the EXISTS outputs of a run lie in [-5, -1e-3]).  Padding holds NaN in
the even predicates and 7.0 in the odd ones.  Predicate 0 of a case carries 0.0, -30, -100, +0.5 and a second 0.0; with 30 predicates or
more, predicates 1..5 carry one of these each (a single 0.0, a pair of 0.0s, -30, -100, +0.5).
"""

import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
from oracle import dfol_oracle as orc  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from test_logic_backward_gpu import _likelihood  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LISTS = [[1, 4, 3], [36, 33], [100, 37, 2], [260, 17]]


@pytest.fixture(scope="module")
def L():
    from dfol_vqa_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return _lib


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def ns_of(n_max):
    return max(4, (int(n_max) + 3) // 4 * 4)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pad_fill(p):
    """What a predicate's padding holds: NaN in the even predicates, 7.0 in the odd ones."""
    return np.float32(np.nan) if p % 2 == 0 else np.float32(7.0)


def _attention(rng, n):
    """n attentions of one predicate whose EXISTS aggregate is neither 0 nor at the clamp: uniform probabilities for up to 4 objects, the 10 % /
    90 % mixture up to 30, weak ones (their sum about n / 100, beyond 100 objects about 1) above."""
    if n <= 4:
        return syn.table_log_likelihood(rng, (n,), "unif")
    if n <= 30:
        return syn.table_log_likelihood(rng, (n,), "mix10")
    return _likelihood(rng, (n,), "weak", n)


# ---------------------------------------------------------------------------------------------------
# 1. quantify forward
# ---------------------------------------------------------------------------------------------------
def _quant_unr():
    with open(os.path.join(ROOT, "dfol_vqa_amd", "csrc", "dfol_logic.hip")) as f:
        return int(re.search(r"constexpr int QUANT_UNR = (\d+);", f.read()).group(1))


def lpp_of(NS):
    """The instantiation dfol_quantify_fwd_f32 picks (None: the one-wavefront-per-predicate kernel)."""
    if NS % 4 != 0 or NS // 4 > 64:
        return None
    return next(l for l in (1, 2, 4, 8, 16, 32, 64) if NS // 4 <= l)


def group_of(NS):
    lpp = lpp_of(NS)
    return 4 if lpp is None else 4 * 4 * (64 // lpp)          # 4 wavefronts x QUANT_UNR (= 4, asserted below) x predicates per wavefront


EDGES = [0.0, -30.0, -100.0, 0.5, 0.0]                       # predicate 0: log 1, the absent value, e^x underflows, above log 1, a second log 1
SINGLE_EDGES = [[0.0], [0.0, 0.0], [-30.0], [-100.0], [0.5]]   # predicates 1..5 of a case of 30 predicates or more


def _plant(att, n_of_p):
    att[0, :min(n_of_p[0], len(EDGES))] = EDGES[:n_of_p[0]]
    if att.shape[0] >= 30:
        for k, e in enumerate(SINGLE_EDGES):
            if n_of_p[1 + k] > len(e):                         # (leave at least one ordinary value beside the edge)
                att[1 + k, 1:1 + len(e)] = e


def _quantify_inputs(rng, NS, P, n_max=None):
    """Questions of 1, 2, n_max - 1, n_max and random object counts, several predicates each; two attention tables [P, NS] over them: `exists`
    (_attention) and `forall` (p ~ U(1 - min(.1, 20 / n), 1): a FOR_ALL sum above the clamp), edges planted in both."""
    n_max = NS if n_max is None else n_max
    Q = max(1, min(P // 3, 24))
    n_list = ([n_max, 1, max(1, n_max - 1), min(2, n_max)] + list(rng.randint(1, n_max + 1, Q)))[:Q]
    pq = np.sort(rng.randint(0, Q, P)).astype(np.int32)
    pq[:min(P, 6)] = 0                                         # the planted predicates belong to the largest question
    n_of_p = np.asarray(n_list)[pq]
    tables = []
    for fam in ("exists", "forall"):
        att = np.empty((P, NS), np.float32)
        for p in range(P):
            att[p] = pad_fill(p)
            n = n_of_p[p]
            att[p, :n] = _attention(rng, n) if fam == "exists" else _likelihood(rng, (n,), "forall", n)
        _plant(att, n_of_p)
        tables.append(att)
    return pq, np.asarray(n_list, np.int32), n_of_p, tables[0], tables[1]


def _quantify_ref(att, quant, n_of_p, dt):
    """log_parametric_not(sum(log_parametric_not(a[:n], q)), q) per predicate."""
    valid = np.arange(att.shape[1])[None, :] < n_of_p[:, None]
    a, q = np.where(valid, att, 0).astype(dt), quant.astype(dt)
    t = np.where(valid, orc.log_parametric_not(a, q[:, None], 1), dt(0))
    return orc.log_parametric_not(t.sum(1), q, 1)


def _quantify_modes(rng, P, att_e, att_f):
    i = np.arange(P)
    mixed = ((i + i // 7) % 2).astype(np.float32)
    frac = np.asarray([0.25, 0.6, 0.25, 1.0, 0.6, 0.0], np.float32)[rng.randint(0, 6, P)]
    frac[:2] = 0.25, 0.6
    return [("exists", np.ones(P, np.float32), att_e), ("for_all", np.zeros(P, np.float32), att_f),
            ("mixed", mixed, np.where(mixed[:, None] == 1, att_e, att_f)), ("fractional", frac[:P], att_e)]


def _exists_spread(r64, quant, what):
    """The reference-only guard: at least half of the EXISTS outputs in [-5, -1e-3]; -> the share."""
    e = r64[quant == 1]
    if not e.size:
        return None
    share = float(((e >= -5) & (e <= -1e-3)).mean())
    assert share >= 0.5, "%s: only %.3g of the float64 EXISTS outputs lie in [-5, -1e-3]: the comparison would be vacuous" % (what, share)
    return share


def _quantify(L, att, quant, pq, n_obj):
    """dfol_quantify_fwd_f32 through the raw entry point (any NS), the output pre-filled with NaN so that a predicate nobody wrote shows."""
    P, NS = att.shape
    a, q, lp = dev(att), dev(quant), torch.full((P,), float("nan"), device="cuda")
    pq_d, n_d = dev(pq), dev(n_obj)
    L.call("dfol_quantify_fwd_f32", a.data_ptr(), q.data_ptr(), pq_d.data_ptr(), n_d.data_ptr(), P, NS, lp.data_ptr(), L._stream())
    return lp.cpu().numpy()


@pytest.mark.parametrize("NS", [4, 8, 12, 16, 20, 32, 36, 64, 100, 128, 132, 256, 260, 300, 10])
def test_quantify_forward_every_dispatch_arm(L, NS):
    assert _quant_unr() == 4, "QUANT_UNR moved: the predicates per workgroup of this test (group_of) and the docstring's table rest on 4"
    G = group_of(NS)
    spread = 1.0
    for P in (G - 1, G, G + 1, 2 * G + 3):
        rng = np.random.RandomState(1000 * NS + P)
        pq, n_obj, n_of_p, att_e, att_f = _quantify_inputs(rng, NS, P)
        for mode, quant, att in _quantify_modes(rng, P, att_e, att_f):
            what = "quantify NS %d (LPP %s) P %d %s" % (NS, lpp_of(NS), P, mode)
            r32, r64 = _quantify_ref(att, quant, n_of_p, np.float32), _quantify_ref(att, quant, n_of_p, np.float64)
            s = _exists_spread(r64, quant, what)
            spread = spread if s is None else min(spread, s)
            got = _quantify(L, att, quant, pq, n_obj)
            gu.check_logprob(got, r32, r64, what)
    print("  quantify NS %d: smallest EXISTS share in [-5, -1e-3] %.3f" % (NS, spread))


def test_quantify_fallback_agrees_with_the_float4_kernel(L):
    """The same attentions at NS = 256 (quantify_fwd4_kernel<64>) and re-laid into NS = 260 (quantify_fwd_kernel): both meet the reference, and
    they agree with each other under the same policy (the float4 kernel's values in the place of the float32 reference), not bit for bit -
    the two kernels combine the lanes' partial sums in different orders."""
    for P in (15, 16, 17, 35):
        rng = np.random.RandomState(77 + P)
        pq, n_obj, n_of_p, att_e, att_f = _quantify_inputs(rng, 256, P)
        for mode, quant, att in _quantify_modes(rng, P, att_e, att_f):
            wide = np.empty((P, 260), np.float32)
            for p in range(P):
                wide[p] = pad_fill(p + 1)
            wide[:, :256] = att
            r32, r64 = _quantify_ref(att, quant, n_of_p, np.float32), _quantify_ref(att, quant, n_of_p, np.float64)
            _exists_spread(r64, quant, mode)
            g4, gw = _quantify(L, att, quant, pq, n_obj), _quantify(L, wide, quant, pq, n_obj)
            gu.check_logprob(g4, r32, r64, "float4 kernel P %d %s" % (P, mode))
            gu.check_logprob(gw, r32, r64, "fallback kernel P %d %s" % (P, mode))
            gu.check_logprob(gw, g4, r64, "fallback against float4 kernel P %d %s" % (P, mode))


# ---------------------------------------------------------------------------------------------------
# 2. quantify, hard mode
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 130, 300])
def test_quantify_hard(L, n):
    """dfol_quantify_hard_f32 against oracle.VarSet.log_probability(hard=True): pnot(min over ALL batch objects of mask * pnot(att, q), q).  A batch
    of one image (total_obj == n: the minimum starts at +inf) and one with a second image of 3 objects (total_obj > n: a 0 takes part).  The
    last predicate of question 0 holds POSITIVE attentions only: under FOR_ALL its result is the smallest of them in the first batch and the
    joined 0 in the second - the one case the start value decides."""
    NS = ns_of(n)
    for extra in (0, 3):
        img = np.concatenate([np.zeros(n, np.int64), np.ones(extra, np.int64)])
        n_list = [n, extra] if extra else [n]
        worlds = {dt: orc.World(None, None, None, img, dt) for dt in (np.float32, np.float64)}
        for P in (1, 3, 4, 5, 9):
            rng = np.random.RandomState(31 * n + 7 * P + extra)
            pq = np.zeros(P, np.int32)
            if extra and P >= 4:
                pq[-1] = 1                                     # one predicate of the other image
            flat, att = np.zeros((P, len(img)), np.float32), np.empty((P, NS), np.float32)
            for p in range(P):
                k, first = n_list[pq[p]], 0 if pq[p] == 0 else n
                v = syn.table_log_likelihood(rng, (k,), "mix10")
                if p == 0:
                    v[:min(k, len(EDGES))] = [0.0, 0.0, -30.0, -100.0, 0.5][:k] if k > 1 else [0.5]
                positive = P >= 3 and p == (P - 2 if pq[-1] == 1 else P - 1)
                if positive:
                    v = rng.uniform(0.05, 0.5, k).astype(np.float32)
                flat[p, first:first + k] = v
                att[p] = pad_fill(p)
                att[p, :k] = v
            for qv in (1.0, 0.0):
                quant = np.full(P, qv, np.float32)
                refs = [orc.VarSet(None, flat.astype(dt), quant.astype(dt), pq, worlds[dt]).log_probability(hard=True) for dt in (np.float32, np.float64)]
                if qv == 0.0 and P >= 3:                       # the case itself, on the reference alone
                    pp = P - 2 if pq[-1] == 1 else P - 1
                    assert (refs[1][pp] == 0.0) if extra else (refs[1][pp] > 0.04), (n, extra, P, refs[1][pp])
                got = L.quantify_hard(dev(att), dev(quant), dev(pq), dev(np.asarray(n_list, np.int32)), len(img)).cpu().numpy()
                gu.check_logprob(got, refs[0], refs[1], "quantify_hard n %d total_obj %d P %d q %g" % (n, len(img), P, qv))


# ---------------------------------------------------------------------------------------------------
# 3. find_max_ind
# ---------------------------------------------------------------------------------------------------
THRESHOLDS = (0.0, 0.5, 0.95)


def _find_max_inputs():
    """Probabilities on a jittered grid (neighbours at least 3.1e-3 apart, none within 1.2e-3 of a threshold), one draw without replacement per
    question; exact ties are copies of one float32 value."""
    rng = np.random.RandomState(11)
    counts = [70, 1, 130, 0, 65, 64, 2, 200, 3]
    grid = 0.003 + 0.0047 * np.arange(206)
    grid = grid[np.all(np.abs(grid[:, None] - np.asarray(THRESHOLDS)[None, :]) >= 2e-3, 1)]
    grid = grid + rng.uniform(-8e-4, 8e-4, len(grid))
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    lp = np.empty(seg[-1], np.float32)
    for q, c in enumerate(counts):
        pool = grid[grid < 0.45] if q == 4 else grid           # question 4: every value below the thresholds 0.5 and 0.95
        lp[seg[q]:seg[q + 1]] = np.log(rng.choice(pool, c, replace=False))
    ties = {}                                                  # question -> positions that hold the same value

    def tie(q, pos, top):
        v = lp[seg[q]:seg[q + 1]]
        val, at = (v.max(), int(v.argmax())) if top else (np.sort(v)[len(v) // 2], pos[0])
        if at not in pos:
            v[at] = v[pos[0]]                                  # the maximum moves to `pos`: its old place takes the value it displaces
        v[pos] = val
        ties.setdefault(q, []).append(list(pos))
    tie(0, [3, 67], True)                                      # the maximum twice, 64 apart: one lane, two stride iterations
    tie(2, [10, 11], True)                                     # at neighbouring positions
    tie(2, [40, 104], False)                                   # a tie below the maximum flags nothing
    tie(7, [5, 69, 133, 134], True)                            # three iterations of one lane and its neighbour
    tie(6, [0, 1], True)
    return counts, seg, lp


def _separation(lp, seg):
    """Smallest distance between two different probabilities of one question, and between a probability and a threshold (float64 of the
    float32 inputs)."""
    sep, thr = np.inf, np.inf
    for q in range(len(seg) - 1):
        pr = np.unique(np.exp(lp[seg[q]:seg[q + 1]].astype(np.float64)))
        if len(pr) > 1:
            sep = min(sep, np.diff(pr).min())
        if len(pr):
            thr = min(thr, np.abs(pr[:, None] - np.asarray(THRESHOLDS)[None, :]).min())
    return sep, thr


def test_find_max_ind_many_options_ties_and_empty_questions(L):
    """Q = 9 (not a multiple of the 4 questions of a workgroup), questions of more than 64 options, an empty one, one whose values all lie below the
    threshold, exact ties within a lane and between neighbours: flags equal to oracle.find_max_ind.  Different probabilities are at least 1e-3
    apart and at least 1e-3 from every threshold (asserted on the inputs), so the last bit of expf against numpy's exp decides no flag."""
    counts, seg, lp = _find_max_inputs()
    sep, thr = _separation(lp, seg)
    print("  find_max_ind: smallest separation %.3g, smallest distance to a threshold %.3g" % (sep, thr))
    assert sep >= 1e-3 and thr >= 1e-3, (sep, thr)
    pq = np.repeat(np.arange(len(counts)), counts)
    lp_d, seg_d = dev(lp), dev(seg)
    for t in THRESHOLDS:
        ref = orc.find_max_ind(lp, pq, len(counts), t)
        flag = torch.full((len(lp),), 7, dtype=torch.uint8, device="cuda")
        L.call("dfol_find_max_ind_f32", lp_d.data_ptr(), seg_d.data_ptr(), len(counts), float(t), flag.data_ptr(), L._stream())
        got = flag.cpu().numpy()
        assert got.tolist() == ref.tolist(), t
        per_q = [int(ref[seg[q]:seg[q + 1]].sum()) for q in range(len(counts))]
        if t == 0.0:
            assert per_q == [2, 1, 2, 0, 1, 1, 2, 4, 1], per_q          # every tie for a maximum is flagged, the tie below it is not
        else:
            assert per_q[4] == 0 and per_q[3] == 0, per_q               # all below the threshold / empty
    assert ref.sum() > 0                                                # (0.95 still leaves answers)


# ---------------------------------------------------------------------------------------------------
# 4. segment_or
# ---------------------------------------------------------------------------------------------------
def _segment_inputs(Q):
    rng = np.random.RandomState(500 + Q)
    lens = rng.randint(1, 21, Q)
    lens[rng.choice(Q, min(Q, 3), replace=False)] = [300, 1, 150][:min(Q, 3)]
    if Q == 1:
        lens[0] = 300
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    lp = np.concatenate([_attention(rng, int(k)) for k in lens]).astype(np.float32)
    return seg, lp


@pytest.mark.parametrize("Q", [1, 64, 65, 200])
def test_segment_or_both_forms(L, Q):
    """One thread per question: a second workgroup (Q > 64), segments of 1 to 300 options.  The complement form against float64 (check_logprob);
    the as-written form against the reference's own float32 values in probability space, |e^got - e^ref32| <= 2e-7, the float32 sum taken in
    the kernel's order (first option to last)."""
    seg, lp = _segment_inputs(Q)
    refs = []
    for dt in (np.float32, np.float64):
        s = [np.cumsum(orc.log_not(lp[seg[q]:seg[q + 1]].astype(dt)), dtype=dt)[-1:] for q in range(Q)]
        refs.append(np.concatenate([orc.log_not(x) for x in s]))
    share = _exists_spread(refs[1], np.ones(Q), "segment_or Q %d" % Q)
    print("  segment_or Q %d: share of the float64 aggregates in [-5, -1e-3] %.3f" % (Q, share))
    got = L.segment_or(dev(lp), dev(seg)).cpu().numpy()
    gu.check_logprob(got, refs[0], refs[1], "segment_or Q %d" % Q)
    gw = L.segment_or(dev(lp), dev(seg), as_written=True).cpu().numpy()
    d = np.abs(np.exp(gw.astype(np.float64)) - np.exp(refs[0].astype(np.float64))).max()
    print("  segment_or as written Q %d: |dp| %.3g" % (Q, d))
    assert np.all(np.isfinite(gw)) and d <= 2e-7, d
    if Q > 64:                                                 # saturation beyond the first workgroup: an option at log(1 - 1e-9) makes the aggregate exactly 0
        lp2 = lp.copy()
        lp2[seg[Q - 1]] = -1e-9
        lp2[seg[64]] = -1e-9
        sw = L.segment_or(dev(lp2), dev(seg), as_written=True).cpu().numpy()
        assert sw[64] == 0.0 and sw[Q - 1] == 0.0 and not np.signbit(sw[[64, Q - 1]]).any()
        keep = np.ones(Q, bool)
        keep[[64, Q - 1]] = False
        assert np.array_equal(bits(sw[keep]), bits(gw[keep]))


# ---------------------------------------------------------------------------------------------------
# 5. option normalisation, forward
# ---------------------------------------------------------------------------------------------------
def _option_segments(n_list, rank):
    """(question, options) per segment: 1, 2 and 26 options on every question; rank 2 above 36 objects keeps the 26 options to the smallest
    question (a predicate is an NS x NS tile there)."""
    NS = ns_of(max(n_list))
    plan = []
    for q in range(len(n_list)):
        small = rank == 1 or NS <= 36 or q == int(np.argmin(n_list))
        plan += [(q, 2), (q, 1)] + ([(q, 26)] if small else [])
    return plan


def _valid_cells(n, NS, rank):
    if rank == 1:
        return np.arange(NS) < n
    r, c = np.meshgrid(np.arange(NS), np.arange(NS), indexing="ij")
    return (r < n) & (c < n) & (r != c)


@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("n_list", N_LISTS)
def test_option_normalize_forward(L, n_list, rank):
    """x - log(max(sum over the segment's options of e^x, 1e-20)) on the cells objects own (golden_util.t_option_normalize in float64, atol
    2e-5); padding and the diagonal - NaN and 7.0 here - keep their bit patterns; the in-place launch is repeatable bit for bit.  One cell of
    every two-option segment holds -100 in both options (the sum underflows to the clamp)."""
    rng = np.random.RandomState(sum(n_list) + rank)
    NS = ns_of(max(n_list))
    plan = _option_segments(n_list, rank)
    pq = np.concatenate([[q] * k for q, k in plan]).astype(np.int32)
    seg = np.concatenate([[0], np.cumsum([k for _, k in plan])]).astype(np.int32)
    P = len(pq)
    shape = (P, NS) if rank == 1 else (P, NS, NS)
    x = np.empty(shape, np.float32)
    valid = np.zeros(shape, bool)
    for p in range(P):
        n = n_list[pq[p]]
        valid[p] = _valid_cells(n, NS, rank)
        x[p] = pad_fill(p)
        x[p][valid[p]] = _likelihood(rng, (int(valid[p].sum()),), "mix10", n)
    for s, (q, k) in enumerate(plan):
        cells = np.argwhere(valid[seg[s]])
        if k == 2 and len(cells):
            x[(slice(seg[s], seg[s + 1]),) + tuple(cells[0])] = -100.0
    ref = x.astype(np.float64)
    for s in range(len(plan)):
        m = valid[seg[s]]
        if m.any():
            ref[seg[s]:seg[s + 1], m] = gu.t_option_normalize(torch.tensor(x[seg[s]:seg[s + 1]][:, m], dtype=torch.float64)).numpy()
    outs = []
    for _ in range(2):
        t = dev(x)
        L.option_normalize_(t, dev(seg), dev(pq), dev(np.asarray(n_list, np.int32)), NS)
        outs.append(t.cpu().numpy())
    got = outs[0]
    assert np.array_equal(bits(got), bits(outs[1])), "two runs differ"
    assert np.array_equal(bits(got)[~valid], bits(x)[~valid]), "a skipped cell (padding, diagonal) changed"
    assert np.all(np.isfinite(got[valid]))
    err = np.abs(got[valid] - ref[valid]).max() if valid.any() else 0.0
    print("  option_normalize %s rank %d: |d| %.3g over %d cells" % (n_list, rank, err, int(valid.sum())))
    assert np.allclose(got[valid], ref[valid], rtol=0, atol=2e-5), err


# ---------------------------------------------------------------------------------------------------
# 6. gathers, forward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_list", N_LISTS)
def test_attr_and_rel_gather_forward(L, n_list):
    """dfol_attr_gather_f32 / dfol_rel_gather_f32 on tables that are column windows of wider ones (ld != columns): blocks and tiles bit-equal to
    numpy indexing of the tables (the pair rows placed by oracle.pair_indices), the default value in padding, on the diagonal and in every
    cell of a predicate whose column is < 0; both tile orientations."""
    rng = np.random.RandomState(sum(n_list))
    C, CR, NS, Q = 11, 5, ns_of(max(n_list)), len(n_list)
    img = np.repeat(np.arange(Q), n_list)
    obj_off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int32)
    pair_off = np.concatenate([[0], np.cumsum([n * (n - 1) for n in n_list])]).astype(np.int64)
    A_wide = syn.table_log_likelihood(rng, (len(img), C + 3))
    R_wide = syn.table_log_likelihood(rng, (max(1, int(pair_off[-1])), CR + 2))
    A, R = A_wide[:, 2:2 + C], R_wide[:, 1:1 + CR]
    A_d, R_d = dev(A_wide)[:, 2:2 + C], dev(R_wide)[:, 1:1 + CR]
    pq = np.repeat(np.arange(Q), 3).astype(np.int32)
    P = len(pq)
    cols, rcols = rng.randint(0, C, P).astype(np.int32), rng.randint(0, CR, P).astype(np.int32)
    cols[1], rcols[1] = -1, -1
    n_obj = np.asarray(n_list, np.int32)
    _, ind1, ind2 = orc.pair_indices(img)
    for dflt in (-30.0, -7.5):
        ref = np.full((P, NS), dflt, np.float32)
        for p in range(P):
            if cols[p] >= 0:
                ref[p, :n_list[pq[p]]] = A[obj_off[pq[p]]:obj_off[pq[p] + 1], cols[p]]
        got = L.attr_gather(A_d, dev(obj_off), dev(pq), dev(cols), NS, dflt).cpu().numpy()
        assert np.array_equal(bits(got), bits(ref)), dflt
        assert np.all(got[1] == np.float32(dflt))
        reft = np.full((P, NS, NS), dflt, np.float32)
        for p in range(P):
            if rcols[p] >= 0:
                dense = np.full((len(img), len(img)), dflt, np.float32)
                dense[ind1, ind2] = R[:len(ind1), rcols[p]]
                o0, o1 = obj_off[pq[p]], obj_off[pq[p] + 1]
                reft[p, :o1 - o0, :o1 - o0] = dense[o0:o1, o0:o1]
        for orient in (0, 1):
            gott = L.rel_gather(R_d, dev(pair_off), dev(n_obj), dev(pq), dev(rcols), NS, orient, dflt).cpu().numpy()
            want = reft if orient == 0 else np.ascontiguousarray(reft.transpose(0, 2, 1))
            assert np.array_equal(bits(gott), bits(want)), (dflt, orient)
            assert np.all(gott[1] == np.float32(dflt))


# ---------------------------------------------------------------------------------------------------
# 7. row-wise kernels
# ---------------------------------------------------------------------------------------------------
WIDTHS = [4, 64, 68, 132, 260]
ROWS = [1, 3, 70]


def _flags(rng, rows):
    f = (rng.uniform(size=rows) < 0.5).astype(np.float32)
    if rows >= 2:
        f[0], f[1] = 1.0, 0.0
    return f


@pytest.mark.parametrize("W", WIDTHS)
def test_rowwise_copies_and_selects_are_bit_exact(L, W):
    """gate with 0 / 1 flags, gather_rows, select_rows and LOGIC_AND at widths beyond one 64-thread block: the selected operand's bits.  gate's
    unselected operand holds NaN and inf in every cell: a select cannot leak them (0 * inf of the blend would)."""
    for rows in ROWS:
        rng = np.random.RandomState(100 * W + rows)
        x, y = syn.table_log_likelihood(rng, (rows, W)), syn.table_log_likelihood(rng, (rows, W), "unif")
        g, xq, yq = _flags(rng, rows), _flags(rng, rows)[::-1].copy(), _flags(rng, rows)
        o, oq = L.gate(dev(x), dev(y), dev(xq), dev(yq), dev(g))
        want, wantq = np.where(g[:, None] == 1, x, y), np.where(g == 1, xq, yq)
        assert np.array_equal(bits(o.cpu().numpy()), bits(want)) and np.array_equal(bits(oq.cpu().numpy()), bits(wantq)), rows
        xn, yn, xqn, yqn = x.copy(), y.copy(), xq.copy(), yq.copy()
        xn[g == 0], yn[g == 1], xqn[g == 0], yqn[g == 1] = np.nan, np.inf, np.inf, np.nan
        o, oq = L.gate(dev(xn), dev(yn), dev(xqn), dev(yqn), dev(g))
        assert np.all(np.isfinite(o.cpu().numpy())) and np.all(np.isfinite(oq.cpu().numpy())), "gate leaked the unselected operand"
        assert np.array_equal(bits(o.cpu().numpy()), bits(want)) and np.array_equal(bits(oq.cpu().numpy()), bits(wantq)), rows
        idx = rng.randint(0, rows, 50).astype(np.int32)
        assert np.array_equal(bits(L.gather_rows(dev(x), dev(idx)).cpu().numpy()), bits(x[idx])), rows
        fl = (g * (1 + 254 * (np.arange(rows) % 2))).astype(np.uint8)             # non-zero flags of 1 and 255
        assert np.array_equal(bits(L.select_rows(dev(x), dev(y), dev(fl)).cpu().numpy()), bits(want)), rows
        assert np.array_equal(bits(L.logic(L.LOGIC_AND, dev(x), dev(y)).cpu().numpy()), bits(x + y)), rows


@pytest.mark.parametrize("W", WIDTHS)
def test_gate_blends_fractional_flags(L, W):
    """g = 0.3 (and 0.75) with fractional quantifiers: g x + (1 - g) y in float64 of the float32 inputs at rtol 1e-6; rows with g of 0 or 1
    among them stay selects."""
    for rows in ROWS:
        rng = np.random.RandomState(200 * W + rows)
        x, y = syn.table_log_likelihood(rng, (rows, W)), syn.table_log_likelihood(rng, (rows, W), "unif")
        g = np.asarray([0.3, 1.0, 0.75, 0.0], np.float32)[np.arange(rows) % 4]
        xq, yq = rng.uniform(0.05, 0.95, rows).astype(np.float32), rng.uniform(0.05, 0.95, rows).astype(np.float32)
        o, oq = L.gate(dev(x), dev(y), dev(xq), dev(yq), dev(g))
        g64 = g.astype(np.float64)
        want = x.astype(np.float64) * g64[:, None] + y.astype(np.float64) * (1 - g64[:, None])
        wantq = xq.astype(np.float64) * g64 + yq.astype(np.float64) * (1 - g64)
        assert np.allclose(o.cpu().numpy(), want, rtol=1e-6, atol=0), rows
        assert np.allclose(oq.cpu().numpy(), wantq, rtol=1e-6, atol=0), rows
        sel = (g == 0) | (g == 1)
        assert np.array_equal(bits(o.cpu().numpy()[sel]), bits(np.where(g[:, None] == 1, x, y)[sel]))


@pytest.mark.parametrize("W", WIDTHS)
def test_rowwise_log_probability_kernels(L, W):
    """parametric_not (alpha 0, 1 and fractional per row), LOGIC_OR and implication (ragged object counts, zeros beyond n, NaN / 7.0 in the
    inputs' padding) at NS = W: check_logprob against the oracle's formulas."""
    for rows in ROWS:
        rng = np.random.RandomState(300 * W + rows)
        x, y = syn.table_log_likelihood(rng, (rows, W)), syn.table_log_likelihood(rng, (rows, W), "unif")
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        alpha = np.asarray([1.0, 0.0, 0.25, 0.6], np.float32)[np.arange(rows) % 4]
        gu.check_logprob(L.parametric_not(dev(x), dev(alpha)).cpu().numpy(), orc.log_parametric_not(x, alpha[:, None], 1),
                         orc.log_parametric_not(x64, alpha[:, None].astype(np.float64), 1), "parametric_not %d x %d" % (rows, W))
        gu.check_logprob(L.logic(L.LOGIC_OR, dev(x), dev(y)).cpu().numpy(), orc.log_or(x, y), orc.log_or(x64, y64), "or %d x %d" % (rows, W))
        Q = max(1, rows // 3)
        n_obj = np.concatenate([[W, 1, max(1, W - 1)], rng.randint(1, W + 1, Q)])[:Q].astype(np.int32)
        pq = rng.randint(0, Q, rows).astype(np.int32)
        pq[0] = 0
        prior = np.minimum(syn.table_log_likelihood(rng, (Q, W), "unif") * 0.3, 0).astype(np.float32)
        valid_q, valid = np.arange(W)[None, :] < n_obj[:, None], np.arange(W)[None, :] < n_obj[pq][:, None]
        xp, pp = x.copy(), prior.copy()
        xp[~valid & (np.arange(rows)[:, None] % 2 == 0)], xp[~valid & (np.arange(rows)[:, None] % 2 == 1)] = np.nan, 7.0
        pp[~valid_q] = np.nan
        imp = L.implication(dev(pp), dev(xp), dev(pq), dev(n_obj)).cpu().numpy()
        r32 = orc.log_not(prior[pq] + orc.log_not(x))
        r64 = orc.log_not(prior[pq].astype(np.float64) + orc.log_not(x64))
        gu.check_logprob(imp[valid], r32[valid], r64[valid], "implication %d x %d" % (rows, W))
        assert not imp[~valid].any() and not np.signbit(imp[~valid]).any(), "implication: a cell beyond n is not +0"


@pytest.mark.parametrize("n", [1, 257, 70000])
def test_logic_not_lengths(L, n):
    rng = np.random.RandomState(n)
    a = syn.table_log_likelihood(rng, (n,))
    a[0] = 0.0 if n > 1 else a[0]
    gu.check_logprob(L.logic(L.LOGIC_NOT, dev(a)).cpu().numpy(), orc.log_not(a), orc.log_not(a.astype(np.float64)), "not n %d" % n)


@pytest.mark.parametrize("Q", [1, 65, 200])
def test_compare_lengths(L, Q):
    """pnot(log_softmax([lp1, lp2]), is_less) (golden_util.t_compare) on aggregate-sized log-probabilities, a second workgroup included."""
    rng = np.random.RandomState(40 + Q)
    a, b = np.log(rng.uniform(0.01, 0.99, Q)).astype(np.float32), np.log(rng.uniform(0.01, 0.99, Q)).astype(np.float32)
    if Q > 2:
        b[1] = a[1]                                            # an exact draw
    less = (np.arange(Q) % 2).astype(np.float32)
    got = L.compare(dev(a), dev(b), dev(less)).cpu().numpy()
    r32, r64 = (gu.t_compare(torch.tensor(a, dtype=dt), torch.tensor(b, dtype=dt), torch.tensor(less, dtype=dt)).numpy() for dt in (torch.float32, torch.float64))
    assert got.shape == (Q, 2)
    gu.check_logprob(got, r32, r64, "compare Q %d" % Q)


@pytest.mark.parametrize("NS,n_list", [(4, [4, 1, 3, 2]), (68, [68, 1, 37, 65]), (132, [132, 5, 64, 129])])
def test_modulate_forward(L, NS, n_list):
    """dfol_modulate_f32 against ops._modulate_reference in float64 at the tolerance test_modulate_backward_kernel_against_autograd applies to this
    formula's attention gradient (atol = rtol = 2e-5), with that test's corners: attention at log 1, d = 0, d = 1, c = 0.  Zeros beyond n."""
    from dfol_vqa_amd import ops
    rng = np.random.RandomState(12 + NS)
    k_list = [2, 1, 3, 1]
    pq = np.repeat(np.arange(len(n_list)), k_list).astype(np.int32)
    P = len(pq)
    valid = np.arange(NS)[None, :] < np.asarray(n_list)[pq][:, None]
    att = (-np.abs(rng.normal(size=(P, NS))) * 2).astype(np.float32)
    att[0, 0] = 0.0
    mods = rng.uniform(0.02, 0.98, size=(P, 4)).astype(np.float32)
    mods[1, 3], mods[2, 3], mods[3, 2] = 0.0, 1.0, 0.0
    padded = att.copy()
    padded[~valid & (np.arange(P)[:, None] % 2 == 0)], padded[~valid & (np.arange(P)[:, None] % 2 == 1)] = np.nan, 7.0
    got = L.modulate(dev(padded), dev(mods), dev(pq), dev(np.asarray(n_list, np.int32))).cpu().numpy()
    ref = ops._modulate_reference(torch.tensor(att, dtype=torch.float64), torch.tensor(mods, dtype=torch.float64), torch.tensor(valid)).numpy()
    assert np.all(np.isfinite(got))
    assert not got[~valid].any() and not np.signbit(got[~valid]).any()
    err = np.abs(got - ref)[valid].max()
    print("  modulate NS %d: |d| %.3g, largest |value| %.3g" % (NS, err, np.abs(ref).max()))
    assert np.allclose(got[valid], ref[valid], rtol=2e-5, atol=2e-5), err
