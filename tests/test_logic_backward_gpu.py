"""Gradients of the soft-logic operators at the forward's edges: csrc/dfol_logic_bwd.hip (relate, filter, quantify, the two gather
backwards, option normalisation), the hand-written backwards of ops.py and the autograd glue of torch_ops.py, each called through
`ops.*(...).backward()` and compared with torch autograd of a restatement of the block formulas (golden_util.t_*).

Policy (golden_util.check_gradient): the restatement is differentiated on the CPU in float32 (r32) and float64 (r64); the kernel is
compared with r64 element by element, |g - r64| <= 8 own s with s = |r64| + 1e-3 max|r64|
and own = max(2^-20, max |r32 - r64| / s), the rounding noise the formula itself carries.  Cells nobody owns (padding, the diagonal,
inactive predicates) must be exactly +0.  Every case asserts that its float64 tile gradient is worth checking (max >= 1e-3, at least 10 %
of the owned cells above 1e-6 of it).  `pytest -s` prints own and the largest observed ratio of every check.

The value families are those of the forward tests (mix10, mix05, weak) plus two of this file's own, because FOR_ALL over ~100 objects is
clamped to zero gradient in all of them: `forall` (tiles p ~ U(1 - min(.1, 20 / n), 1), priors about -0.02) and `weak_forall` (weak tiles,
the same priors; for negated FOR_ALL).  Predicate 0 carries the planted clamps of test_relate_negated_and_forall_fast_paths and two
likelihoods at and above 0; padding holds NaN and 7.0.
"""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from oracle import dfol_oracle as orc  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def dev(x):
    return torch.tensor(x, device=DEV)


def ns_of(n):
    return max(4, (n + 3) // 4 * 4)


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def _likelihood(rng, shape, family, n):
    """Beyond 100 objects the forward tests' families saturate every EXISTS (a row holds dozens of strong likelihoods, 1 - prod(1 - p P)
    is 1 and its gradient 0), so there the share of strong values and the size of the weak ones shrink with 100 / n."""
    if family == "forall":
        return np.log(1 - min(0.1, 20.0 / max(n, 1)) * rng.uniform(size=shape)).astype(np.float32)
    family = "weak" if family == "weak_forall" else family
    if n <= 100:
        return syn.table_log_likelihood(rng, shape, family)
    r, u, pick = 100.0 / n, rng.uniform(size=shape), rng.uniform(size=shape)
    p = {"mix10": np.where(pick < 0.10 * r, 0.5 + 0.5 * u, 0.05 * r * u), "mix05": np.where(pick < 0.05 * r, 0.9 + 0.1 * u, 0.01 * r * u),
         "weak": 0.02 * r * u}[family]
    return np.log(np.maximum(p, 1e-5)).astype(np.float32)


def _prior(rng, n, family):
    if family in ("forall", "weak_forall"):
        return (-0.02 * rng.uniform(0.5, 1.5, size=n)).astype(np.float32)
    return np.minimum(syn.table_log_likelihood(rng, (n,), "unif") * 0.3, 0).astype(np.float32)


def logic_inputs(rng, n_list, k_list, family, diag=-30.0, plant=True, zero_prior=True):
    """Priors [Q, NS], tiles [P, NS, NS] (subjects along rows) and arity-1 likelihoods [P, NS]: planted clamps in predicate 0, NaN and
    7.0 in every padding cell.  `zero_prior=False` (negated FOR_ALL): the priors beside the planted likelihood 0 are -3 instead of 0; the
    negation's clamped log 1e-20 plus a prior of 0 would sit exactly on the FOR_ALL clamp's floor, where float32 and float64 may differ."""
    Q = len(n_list)
    pq = np.repeat(np.arange(Q), k_list).astype(np.int32)
    P, NS = len(pq), ns_of(max(n_list))
    prior_s, prior_o = np.full((Q, NS), np.nan, np.float32), np.full((Q, NS), 7.0, np.float32)
    tile, ll1 = np.full((P, NS, NS), 7.0, np.float32), np.full((P, NS), np.nan, np.float32)
    for q, n in enumerate(n_list):
        prior_s[q, :n], prior_o[q, :n] = _prior(rng, n, family), _prior(rng, n, family)
    for p in range(P):
        n = n_list[pq[p]]
        t = _likelihood(rng, (n, n), family, n)
        t[np.arange(n), np.arange(n)] = diag
        tile[p, n:, :] = np.nan
        tile[p, :n, :n] = t
        ll1[p, :n] = _likelihood(rng, (n,), family, n)
        if p % 2:
            ll1[p, n:] = 7.0
    q0, n0 = pq[0], n_list[pq[0]]
    if plant and n0 >= 4:
        tile[0, 1, 2] = 0.0                                                 # negated: 1 - E = 0; un-negated EXISTS: E = P = 1
        prior_s[q0, 1] = prior_o[q0, 2] = 0.0 if zero_prior else -3.0
        prior_o[q0, 3], tile[0, 0, 3] = -40.0, -20.0                        # FOR_ALL: l' + prior below log 1e-20
        tile[0, 2, 0], tile[0, 3, 0] = 0.0, 0.5                             # at and above 0: gradient 0, as torch relu
        ll1[0, 1], ll1[0, 2], ll1[0, 3] = 0.0, 0.5, -20.0                   # (with prior_s 0 at object 1; prior_s -40 at object 3 below)
    return pq, NS, prior_s, prior_o, tile, ll1


def _incoming(rng, shape):
    """Incoming gradients of one sign: a prior's gradient is a sum over objects and predicates, and with mixed signs the sum cancels to a
    few percent of its terms - the per-element bound would then measure the summation order, which one float32 sample (r32) does not bound."""
    return rng.uniform(0.5, 1.5, size=shape).astype(np.float32)


def _neg_of(mode, P):
    return {None: None, "ones": np.ones(P, np.uint8), "mixed": (np.arange(P) % 2).astype(np.uint8)}[mode]


# ---------------------------------------------------------------------------------------------------
# 1. the restatement itself, pinned to the oracle in float64 (no GPU)
# ---------------------------------------------------------------------------------------------------
def test_restatement_equals_the_oracle_in_float64():
    rng = np.random.RandomState(5)
    worst = 0.0
    for family, n in (("mix10", 9), ("mix05", 40), ("weak", 7), ("forall", 100), ("weak_forall", 30), ("mix10", 1), ("mix10", 2)):
        pq, NS, prior_s, prior_o, tile, ll1 = logic_inputs(rng, [n], [1], family)
        a, b, l = (x.astype(np.float64) for x in (prior_s[0, :n], prior_o[0, :n], tile[0, :n, :n]))
        for any_neg, neg in ((False, 0), (True, 0), (True, 1)):
            for qs, qo in ((1, 1), (0, 0), (1, 0), (0, 1)):
                want = orc.relate_block(a, b, l, float(qs), float(qo), float(neg), any_neg)
                got = gu.t_relate(torch.tensor(a), torch.tensor(b), torch.tensor(l), qs, qo, neg, any_neg)
                for g, w in zip(got, want):
                    worst = max(worst, np.abs(g.numpy() - w).max())
            x = ll1[0, :n].astype(np.float64)
            v = np.minimum(x, 0)
            v = orc.log_parametric_not(v, np.float64(neg), 1) if any_neg else v
            worst = max(worst, np.abs(gu.t_filter(torch.tensor(a), torch.tensor(x), neg, any_neg).numpy() - (a + v)).max())
        x = np.concatenate([ll1[0, :n].astype(np.float64), [0.0, -47.5, -1e-9]])
        x = np.minimum(x, 0)
        y = x[::-1].copy()
        for alpha in (0.0, 1.0):
            worst = max(worst, np.abs(gu.t_pnot(torch.tensor(x), alpha).numpy() - orc.log_parametric_not(x, np.float64(alpha), 1)).max())
            inner = orc.log_parametric_not(x[:n], np.float64(alpha), 1).sum(keepdims=True)
            worst = max(worst, abs(float(gu.t_quantify(torch.tensor(x[:n]), alpha)) - orc.log_parametric_not(inner, np.float64(alpha), 1)[0]))
        worst = max(worst, np.abs(gu.t_lnot(torch.tensor(x)).numpy() - orc.log_not(x)).max())
        worst = max(worst, np.abs(gu.t_or(torch.tensor(x), torch.tensor(y)).numpy() - orc.log_or(x, y)).max())
        worst = max(worst, abs(float(gu.t_segment_or(torch.tensor(x))) - float(orc.log_or_tensor(x, 0))))
        worst = max(worst, np.abs(gu.t_implication(torch.tensor(x), torch.tensor(y)).numpy() - orc.log_not(x + orc.log_not(y))).max())
    assert worst <= 1e-12, worst


def test_check_gradient_rejects_what_it_should():
    """The tolerance helper on made-up numbers: an element off by 1e-2 of its own size fails although the tensor's largest element is 100
    times larger (with per-row scales, also one in a row 1e6 times smaller); a stray value, a NaN and a trivial reference are refused."""
    rng = np.random.RandomState(1)
    r64 = rng.normal(size=(3, 50)) * np.array([[1.0], [1e-4], [1e2]])
    r32 = r64 * (1 + 1e-7 * rng.normal(size=r64.shape))
    gu.check_gradient(r64 * (1 + 2e-6), r32, r64, "helper: fine")
    bad = r64.copy()
    bad[0, np.argmax(np.abs(r64[0]))] *= 1 + 1e-2            # 1e-2 of an element 1e-2 of the largest: above 8 own s = 8e-6 (|r64| + 1e-3 max)
    with pytest.raises(AssertionError, match="own"):
        gu.check_gradient(bad, r32, r64, "helper: one element off")
    bad = r64.copy()
    bad[1, np.argmax(np.abs(r64[1]))] *= 1 + 1e-3
    with pytest.raises(AssertionError, match="own"):
        gu.check_gradient(bad, r32, r64, "helper: one small row off", block_axis0=True)
    owned = np.ones(r64.shape, bool)
    owned[:, 40:] = False
    z64, z32 = np.where(owned, r64, 0), np.where(owned, r32, 0)
    gu.check_gradient(z64, z32, z64, "helper: masked", owned=owned, min_max=1e-3, min_share=0.1)
    stray = z64.copy()
    stray[0, 45] = 1e-30
    with pytest.raises(AssertionError, match="nobody owns"):
        gu.check_gradient(stray, z32, z64, "helper: stray", owned=owned)
    with pytest.raises(AssertionError, match="non-finite"):
        gu.check_gradient(np.where(owned, z64, np.nan), z32, z64, "helper: nan", owned=owned)
    with pytest.raises(AssertionError, match="nothing to check"):
        gu.check_gradient(z64 * 1e-9, z32 * 1e-9, z64 * 1e-9, "helper: trivial", owned=owned, min_max=1e-3, min_share=0.1)
    with pytest.raises(AssertionError, match="boundary"):
        gu.check_gradient(z64, z32, z64, "helper: near", owned=owned, near=owned)


# ---------------------------------------------------------------------------------------------------
# 2. relate
# ---------------------------------------------------------------------------------------------------
def relate_reference(n_list, pq, prior_s, prior_o, tile, quant, neg, active, want, gs, go, lone):
    """-> (r32, r64, near, owned): gradients [d prior_s, d prior_o, d tile] of sum(post_s gs) + sum(post_o go), the clamp-boundary masks
    and the owned cells."""
    P, Q, NS = len(pq), len(n_list), tile.shape[1]
    any_neg = neg is not None
    near = [np.zeros((Q, NS), bool), np.zeros((Q, NS), bool), np.zeros((P, NS, NS), bool)]
    owned = [np.zeros((Q, NS), bool), np.zeros((Q, NS), bool), np.zeros((P, NS, NS), bool)]

    def loss(a, b, t, record=False):
        total = a.new_zeros(())
        for p in range(P):
            q, n = pq[p], n_list[pq[p]]
            if active is not None and not active[p]:
                rs, ro = a[q, :n], b[q, :n]
            else:
                nr = {} if record else None
                rs, ro = gu.t_relate(a[q, :n], b[q, :n], t[p, :n, :n], quant[p, 0], quant[p, 1], neg[p] if any_neg else 0, any_neg, lone, nr)
                if record:
                    near[2][p, :n, :n] = nr["tile"].numpy()
                    near[0][q, :n] |= nr["s"].numpy()
                    near[1][q, :n] |= nr["o"].numpy()
                    owned[2][p, :n, :n] = ~np.eye(n, dtype=bool)
            ws, wo = (1.0, 1.0) if want is None else (float(want[p] & 1 > 0), float(want[p] & 2 > 0))
            total = total + ws * (rs * torch.tensor(gs[p, :n], dtype=a.dtype)).sum() + wo * (ro * torch.tensor(go[p, :n], dtype=a.dtype)).sum()
            owned[0][q, :n] = owned[1][q, :n] = True
        return total

    with torch.no_grad():
        loss(*(torch.tensor(x, dtype=F64) for x in (prior_s, prior_o, tile)), record=True)
    r32, r64 = gu.autograd_pair(loss, (prior_s, prior_o, tile))
    return r32, r64, near, owned


def run_relate(what, n_list, k_list, family, qs, qo, neg_mode=None, orient=0, diag_absent=True, use_active=False, use_want=False, lone=False,
               need=("prior", "tile"), seed=0, repeat=False):
    rng = np.random.RandomState(sum(n_list) + 7 * seed + 1)
    pq, NS, prior_s, prior_o, tile, _ = logic_inputs(rng, n_list, k_list, family, diag=-30.0 if diag_absent else -0.5,
                                                     zero_prior=neg_mode is None or (qs == 1 and qo == 1))
    P, Q = len(pq), len(n_list)
    quant = np.tile(np.asarray([[qs, qo]], np.float32), (P, 1))
    neg = _neg_of(neg_mode, P)
    active = None
    if use_active:
        active = np.ones(P, np.uint8)
        active[1::3] = 0
    want = np.asarray([(3, 1, 2)[p % 3] for p in range(P)], np.uint8) if use_want else None
    gs, go = _incoming(rng, (P, NS)), _incoming(rng, (P, NS))
    for p in range(P):
        gs[p, n_list[pq[p]]:] = go[p, n_list[pq[p]]:] = 7.0
    r32, r64, near, owned = relate_reference(n_list, pq, prior_s, prior_o, tile, quant, neg, active, want, gs, go, lone)

    from dfol_vqa_amd import ops
    t_in = tile if orient == 0 else np.ascontiguousarray(tile.transpose(0, 2, 1))
    n_obj = dev(np.asarray(n_list, np.int32))
    runs = []
    for _ in range(2 if repeat else 1):
        ps_t, po_t, tl_t = dev(prior_s), dev(prior_o), dev(t_in)
        if "prior" in need:
            ps_t.requires_grad_(True), po_t.requires_grad_(True)
        if "tile" in need:
            tl_t.requires_grad_(True)
        ps, po = ops.relate_fwd(ps_t, po_t, tl_t, dev(pq), n_obj, dev(quant[:, 0]), dev(quant[:, 1]), None if neg is None else dev(neg),
                                None if active is None else dev(active), None if want is None else dev(want), orientation=orient,
                                lone_forall_identity=lone, diag_absent=diag_absent)
        for p in range(P):                                   # the forward the gradient belongs to: finite where an object lives, 0 in the padding
            n = n_list[pq[p]]
            for o, bit in ((ps, 1), (po, 2)):
                if want is None or want[p] & bit:
                    assert bool(torch.isfinite(o[p, :n]).all()) and not bool(o[p, n:].any()), (what, p)
        (ps * dev(gs)).sum().add((po * dev(go)).sum()).backward()
        runs.append([None if t.grad is None else t.grad.cpu().numpy() for t in (ps_t, po_t, tl_t)])
    if repeat:
        for a, b in zip(*runs):
            assert (a is None and b is None) or np.array_equal(a, b), what + ": two runs differ"
    g_s, g_o, g_t = runs[0]
    if "prior" in need:
        gu.check_gradient(g_s, r32[0], r64[0], what + " d prior_s", owned[0], near[0])
        gu.check_gradient(g_o, r32[1], r64[1], what + " d prior_o", owned[1], near[1])
    else:
        assert g_s is None and g_o is None
    if "tile" in need:
        if orient == 1:
            g_t = g_t.transpose(0, 2, 1)
        gu.check_gradient(g_t, r32[2], r64[2], what + " d tile", owned[2], near[2], min_max=1e-3, min_share=0.1)
    else:
        assert g_t is None


RELATE_SIZES = [[5, 1, 8, 3], [36, 20, 33], [100, 37, 64, 2], [130, 256], [290, 17], [650, 9]]       # registers, 16 wavefronts, 4 wavefronts (LDS)
# (family, quant_s, quant_o, neg, orientation, diag_absent, active mask, want mask)
RELATE_CONFIGS = [("mix10", 1, 1, None, 0, True, False, False),
                  ("mix10", 1, 1, "mixed", 1, False, True, False),
                  ("weak", 1, 1, None, 0, True, False, True),
                  ("mix05", 1, 1, None, 1, True, False, False),
                  ("mix05", 1, 0, "mixed", 0, False, False, False),
                  ("weak", 0, 1, None, 1, True, True, True),
                  ("forall", 1, 1, "ones", 0, True, False, True),         # negated EXISTS needs p near 1 (negated weak values are certain: saturated)
                  ("forall", 1, 1, "mixed", 1, False, False, False),
                  ("forall", 0, 0, None, 0, True, False, False),
                  ("forall", 0, 0, None, 1, False, True, True),
                  ("forall", 1, 0, None, 1, True, False, False),
                  ("forall", 0, 1, "mixed", 0, True, False, True),
                  ("weak_forall", 0, 0, "ones", 1, True, False, False),
                  ("weak_forall", 0, 1, "mixed", 0, False, True, False),
                  ("weak_forall", 1, 0, "ones", 0, True, False, True)]


def _k_list(n_list):
    return [(2, 1, 3)[i % 3] for i in range(len(n_list))]


# Combinations whose float64 reference fails the non-triviality or clamp-boundary asserts (measured on the CPU: the EXISTS side saturates, or
# one prior cell lands on the floor); every size keeps all four quantifier pairs, negation, both orientations and both masks without them.
RELATE_TRIVIAL = {4: (2, 3), 7: (4, 5), 10: (4, 5), 12: (2,), 14: (3, 4, 5)}               # index into RELATE_CONFIGS: indices into RELATE_SIZES
RELATE_TRIVIAL = {(c, s) for c, sizes in RELATE_TRIVIAL.items() for s in sizes}
RELATE_CASES = [(n_list, cfg) for s, n_list in enumerate(RELATE_SIZES) for c, cfg in enumerate(RELATE_CONFIGS) if (c, s) not in RELATE_TRIVIAL]


@gpu
@pytest.mark.parametrize("n_list,cfg", RELATE_CASES, ids=lambda c: ("n" if isinstance(c, list) else "") + "_".join(str(x) for x in c))
def test_relate_backward(n_list, cfg):
    family, qs, qo, neg_mode, orient, da, use_active, use_want = cfg
    what = "relate %s %s q=(%d,%d) neg=%s or=%d da=%d act=%d want=%d" % (n_list, family, qs, qo, neg_mode, orient, da, use_active, use_want)
    run_relate(what, n_list, _k_list(n_list), family, qs, qo, neg_mode, orient, da, use_active, use_want, seed=RELATE_CONFIGS.index(cfg),
               repeat=cfg in (RELATE_CONFIGS[1], RELATE_CONFIGS[11]))


@gpu
@pytest.mark.parametrize("need", [("prior",), ("tile",)])
@pytest.mark.parametrize("n_list", [[5, 1, 8, 3], [100, 37, 64, 2], [290, 17]], ids=lambda n: "n" + "_".join(map(str, n)))
def test_relate_backward_one_gradient_alone(n_list, need):
    """Only the priors, or only the tile, require a gradient (need_prior / need_tile of dfol_relate_bwd_f32)."""
    for family, qs, qo, neg_mode, orient in (("mix10", 1, 1, "mixed", 1), ("forall", 0, 1, None, 0)):
        what = "relate alone %s %s %s q=(%d,%d) or=%d" % (need[0], n_list, family, qs, qo, orient)
        run_relate(what, n_list, _k_list(n_list), family, qs, qo, neg_mode, orient, need=need, seed=20)


@gpu
@pytest.mark.parametrize("n", [5, 100, 290])
def test_relate_backward_lone_forall_identity(n):
    """A single predicate (P = 1) with lone_forall_identity: a FOR_ALL variable takes the literal branch (batch_base_ops.py:104-108), no
    parametric not and so no clamp - also where the clamped form would have zero gradient (the mix10 case at n >= 100)."""
    for family, qs, qo, neg_mode, orient in (("forall", 0, 0, None, 0), ("mix10", 0, 1, "ones", 1), ("mix10", 1, 0, None, 0), ("mix10", 0, 0, None, 1)):
        if neg_mode is not None and n > 100:                 # (negated mix10 values are all but certain: EXISTS over 290 of them is saturated)
            continue
        what = "relate lone n=%d %s q=(%d,%d) neg=%s or=%d" % (n, family, qs, qo, neg_mode, orient)
        run_relate(what, [n], [1], family, qs, qo, neg_mode, orient, lone=True, seed=30)


# ---------------------------------------------------------------------------------------------------
# 3. filter and quantify
# ---------------------------------------------------------------------------------------------------
FQ_SIZES = [([5, 1, 8, 3, 6], [2, 1, 0, 3, 1]), ([100, 37, 64, 2], [1, 2, 0, 3])]
FQ_CONFIGS = [("mix10", 1, None), ("mix10", 1, "mixed"), ("weak", 1, None), ("mix05", 1, None), ("forall", 1, "ones"), ("forall", 0, None),
              ("weak_forall", 0, "ones"), ("forall", 1, "mixed")]


def run_filter_quantify(what, n_list, k_list, family, qf, neg_mode, mode, seed=0):
    """mode: "filter", "quantify" or "chain" (quantify(filter(prior, ll)))."""
    from dfol_vqa_amd import ops
    rng = np.random.RandomState(sum(n_list) + 11 * seed + 3)
    pq, NS, prior_s, _, _, ll1 = logic_inputs(rng, n_list, k_list, family, zero_prior=neg_mode is None or qf == 1)
    q0, n0 = pq[0], n_list[pq[0]]
    if n0 >= 4:
        prior_s[q0, 3] = -40.0                               # with ll1[0, 3] = -20: below log 1e-20
    P, Q = len(pq), len(n_list)
    neg = _neg_of(neg_mode, P)
    any_neg = neg is not None
    active = np.ones(P, np.uint8)
    if P > 2:
        active[2] = 0
    quant = np.full(P, qf, np.float32)
    g_out, g_lp = _incoming(rng, (P, NS)), _incoming(rng, P)
    for p in range(P):
        g_out[p, n_list[pq[p]]:] = 7.0
    has_pred = np.isin(np.arange(Q), pq)
    owned_prior = (np.arange(NS)[None, :] < np.asarray(n_list)[:, None]) & has_pred[:, None]
    owned_ll = np.arange(NS)[None, :] < np.asarray(n_list)[pq][:, None]
    near_ll, near_prior = np.zeros((P, NS), bool), np.zeros((Q, NS), bool)

    def loss(a, x, record=False):
        total = a.new_zeros(())
        for p in range(P):
            q, n = pq[p], n_list[pq[p]]
            if mode == "quantify":
                att = x[p, :n]
            else:
                att = gu.t_filter(a[q, :n], x[p, :n], neg[p] if any_neg else 0, any_neg) if active[p] else a[q, :n] + 0 * x[p, :n]
                if record and any_neg and active[p]:
                    near_ll[p, :n] |= gu.t_near(-torch.relu(-x[p, :n]), float(neg[p])).numpy()
            if mode == "filter":
                total = total + (att * torch.tensor(g_out[p, :n], dtype=a.dtype)).sum()
            else:
                if record:
                    m = gu.t_near(att, float(qf)) | gu.t_near(gu.t_pnot(att, float(qf)).sum(), float(qf))
                    near_ll[p, :n] |= m.numpy()
                    near_prior[q, :n] |= m.numpy()
                total = total + float(g_lp[p]) * gu.t_quantify(att, qf)
        return total

    with torch.no_grad():
        loss(torch.tensor(prior_s, dtype=F64), torch.tensor(ll1, dtype=F64), record=True)
    r32, r64 = gu.autograd_pair(loss, (prior_s, ll1))
    n_obj, pq_t = dev(np.asarray(n_list, np.int32)), dev(pq)
    outs = []
    for _ in range(2):
        a_t, x_t = dev(prior_s).requires_grad_(mode != "quantify"), dev(ll1).requires_grad_(True)
        if mode == "quantify":
            lp = ops.quantify_fwd(x_t, dev(quant), pq_t, n_obj)
        else:
            att = ops.filter_fwd(a_t, x_t, pq_t, n_obj, None if neg is None else dev(neg), dev(active))
            lp = ops.quantify_fwd(att, dev(quant), pq_t, n_obj) if mode == "chain" else None
        ((att * dev(g_out)).sum() if mode == "filter" else (lp * dev(g_lp)).sum()).backward()
        outs.append((None if a_t.grad is None else a_t.grad.cpu().numpy(), x_t.grad.cpu().numpy()))
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(*outs)), what + ": two runs differ"
    g_a, g_x = outs[0]
    if mode == "quantify":
        gu.check_gradient(g_x, r32[1], r64[1], what + " d att", owned_ll, near_ll, min_max=1e-3, min_share=0.1)
        return
    owned_ll = owned_ll & (active[:, None] > 0)             # an inactive predicate passes the prior through: its likelihood has no gradient
    gu.check_gradient(g_a, r32[0], r64[0], what + " d prior", owned_prior, near_prior)
    gu.check_gradient(g_x, r32[1], r64[1], what + " d ll", owned_ll, near_ll, min_max=1e-3, min_share=0.1)


# (quantify takes no negation; chained behind negated mix10 likelihoods - all but certain - EXISTS saturates and the reference is trivial)
FQ_CASES = [(mode, cfg) for mode in ("filter", "quantify", "chain") for cfg in FQ_CONFIGS
            if (mode != "quantify" or cfg[2] is None) and (mode != "chain" or cfg != FQ_CONFIGS[1])]


@gpu
@pytest.mark.parametrize("mode,cfg", FQ_CASES, ids=lambda c: c if isinstance(c, str) else "-".join(str(x) for x in c))
@pytest.mark.parametrize("sizes", FQ_SIZES, ids=lambda s: "n" + "_".join(map(str, s[0])))
def test_filter_quantify_backward(sizes, mode, cfg):
    """filter_bwd and quantify_bwd alone and chained; the prior's gradient is the sum over a question's predicates (reduce_by_question),
    a question without predicates gets a zero row."""
    (n_list, k_list), (family, qf, neg_mode) = sizes, cfg
    what = "%s %s %s q=%d neg=%s" % (mode, n_list, family, qf, neg_mode)
    run_filter_quantify(what, n_list, k_list, family, qf, neg_mode, mode, seed=FQ_CONFIGS.index(cfg))


# ---------------------------------------------------------------------------------------------------
# 4. the gather backwards and option normalisation
# ---------------------------------------------------------------------------------------------------
def _sum_check(got, terms_sum, terms_abs, count, what):
    """A plain fp32 sum of `count` terms in a fixed order against float64: |got - sum| <= count 2^-23 sum|terms|; exactly 0 where nothing was added."""
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), what
    assert not got[count == 0].any(), what + ": a row nobody requested is not 0"
    err = np.abs(got - terms_sum)
    bound = count * 2.0 ** -23 * terms_abs
    worst = float((err / np.maximum(bound, 1e-300))[count > 0].max()) if (count > 0).any() else 0.0
    print("  %-78s worst error / bound %.3g  n %d" % (what, worst, int((count > 0).sum())))
    assert (err <= bound).all(), (what, worst)
    assert (count > 0).sum() >= 0.05 * count.size and np.abs(terms_sum).max() >= 1e-3, what + ": nothing to check"


GATHER_SIZES = [([5, 1, 2, 30, 7], [3, 2, 0, 2, 4]), ([100, 2, 1], [5, 1, 2]), ([70, 9], [3, 2])]


def _gather_cols(rng, pq, C):
    cols = rng.randint(0, C, len(pq)).astype(np.int32)
    cols[1] = -1                                             # a no-op column
    cols[2] = cols[0]                                        # the same column twice in image 0
    cols[-1] = cols[-2]
    return cols


@gpu
@pytest.mark.parametrize("sizes", GATHER_SIZES, ids=lambda s: "n" + "_".join(map(str, s[0])))
def test_attr_gather_backward(sizes):
    from dfol_vqa_amd import ops
    n_list, k_list = sizes
    rng = np.random.RandomState(sum(n_list))
    Q, C = len(n_list), 11
    pq = np.repeat(np.arange(Q), k_list).astype(np.int32)
    P, NS, O = len(pq), ns_of(max(n_list)), sum(n_list)
    obj_off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int32)
    cols = _gather_cols(rng, pq, C)
    table = syn.table_log_likelihood(rng, (O, C), "mix10")
    g = (rng.normal(size=(P, NS)) * np.power(10.0, rng.randint(-3, 3, size=(P, 1)))).astype(np.float32)
    for p in range(P):
        g[p, n_list[pq[p]]:] = 7.0
    outs = []
    for _ in range(2):
        t = dev(table).requires_grad_(True)
        ll = ops.attr_gather(t, dev(obj_off), dev(pq), dev(cols), NS)
        ll.backward(dev(g))
        outs.append(t.grad.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    ref, mag, cnt = np.zeros((O, C)), np.zeros((O, C)), np.zeros((O, C), np.int64)
    for p in range(P):
        q, n = pq[p], n_list[pq[p]]
        if cols[p] >= 0:
            rows = slice(obj_off[q], obj_off[q] + n)
            ref[rows, cols[p]] += g[p, :n].astype(np.float64)
            mag[rows, cols[p]] += np.abs(g[p, :n].astype(np.float64))
            cnt[rows, cols[p]] += 1
    assert cnt.max() >= 2
    _sum_check(outs[0], ref, mag, cnt, "attr_gather_bwd %s" % n_list)


@gpu
@pytest.mark.parametrize("orient", [0, 1])
@pytest.mark.parametrize("sizes", GATHER_SIZES, ids=lambda s: "n" + "_".join(map(str, s[0])))
def test_rel_gather_backward(sizes, orient):
    from dfol_vqa_amd import ops
    n_list, k_list = sizes
    rng = np.random.RandomState(sum(n_list) + orient)
    Q, C = len(n_list), 7
    pq = np.repeat(np.arange(Q), k_list).astype(np.int32)
    n = np.asarray(n_list, np.int64)
    P, NS, pairs = len(pq), ns_of(max(n_list)), int((n * (n - 1)).sum())
    pair_off = np.concatenate([[0], np.cumsum(n * (n - 1))]).astype(np.int64)
    cols = _gather_cols(rng, pq, C)
    table = syn.table_log_likelihood(rng, (pairs, C), "mix10")
    g = (rng.normal(size=(P, NS, NS)) * np.power(10.0, rng.randint(-3, 3, size=(P, 1, 1)))).astype(np.float32)
    for p in range(P):
        k = n_list[pq[p]]
        g[p, k:, :] = 7.0
        g[p, :, k:] = 7.0
        g[p, np.arange(k), np.arange(k)] = 7.0               # the diagonal belongs to no pair
    outs = []
    for _ in range(2):
        t = dev(table).requires_grad_(True)
        tile = ops.rel_gather(t, dev(pair_off), dev(np.asarray(n_list, np.int32)), dev(pq), dev(cols), NS, orient)
        tile.backward(dev(g))
        outs.append(t.grad.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    ref, mag, cnt = np.zeros((pairs, C)), np.zeros((pairs, C)), np.zeros((pairs, C), np.int64)
    for p in range(P):
        q, k = pq[p], n_list[pq[p]]
        if cols[p] < 0 or k < 2:
            continue
        s, o = np.nonzero(~np.eye(k, dtype=bool))            # row-major in the subject: the table's pair order (util.py:87-103)
        rows = pair_off[q] + np.arange(k * (k - 1))
        v = (g[p, o, s] if orient else g[p, s, o]).astype(np.float64)
        ref[rows, cols[p]] += v
        mag[rows, cols[p]] += np.abs(v)
        cnt[rows, cols[p]] += 1
    assert cnt.max() >= 2
    _sum_check(outs[0], ref, mag, cnt, "rel_gather_bwd %s orientation %d" % (n_list, orient))


@gpu
@pytest.mark.parametrize("rank", [1, 2])
@pytest.mark.parametrize("sizes", [([5, 1, 8, 3, 6], [1, 3, 2, 5, 1], 2, 4), ([100, 37, 2], [26, 1, 4], 2, 1), ([70, 9], [2, 7], 1, None)],
                         ids=lambda s: "n" + "_".join(map(str, s[0])))
def test_option_normalize_backward(sizes, rank):
    """x - log(max(sum e^x, 1e-20)) over the options of a question: segments of one option (gradient exactly 0), of mixed sizes, one whose
    options all lie below log 1e-20 (segment `sc`; clamp active: dx = g), one of a single option e^x = 0.6e-20 (segment `sb`: clamped
    although its softmax weight against the floor is 0.6); padding and diagonal pass g through."""
    from dfol_vqa_amd import ops
    n_list, k_list, sc, sb = sizes
    rng = np.random.RandomState(sum(n_list) + rank)
    Q = len(n_list)
    pq = np.repeat(np.arange(Q), k_list).astype(np.int32)
    P, NS = len(pq), ns_of(max(n_list))
    seg_off = np.concatenate([[0], np.cumsum(k_list)]).astype(np.int32)
    shape = (P, NS) if rank == 1 else (P, NS, NS)
    x = syn.table_log_likelihood(rng, shape, "mix10")
    x[seg_off[sc]:seg_off[sc + 1]] = -50.0 - 5.0 * rng.uniform(size=(k_list[sc],) + shape[1:]).astype(np.float32)     # Z <= 2e-22 k: a factor >= 7 below the floor
    if sb is not None:
        assert k_list[sb] == 1
        x[seg_off[sb]] = np.float32(np.log(0.6e-20))
    g = rng.normal(size=shape).astype(np.float32)
    real = np.zeros(shape, bool)
    for p in range(P):
        k = n_list[pq[p]]
        if rank == 1:
            real[p, :k] = True
        else:
            real[p, :k, :k] = ~np.eye(k, dtype=bool)
    x = np.where(real, x, np.where(rng.uniform(size=shape) < 0.5, np.float32(np.nan), np.float32(7.0))).astype(np.float32)
    near = np.zeros(shape, bool)

    def loss(t, record=False):
        total = t.new_zeros(())
        for s in range(Q):
            seg = t[seg_off[s]:seg_off[s + 1]]
            m = torch.tensor(real[seg_off[s]])
            y = gu.t_option_normalize(torch.where(m, seg, torch.zeros_like(seg)))
            if record:
                Z = torch.exp(torch.where(m, seg, torch.zeros_like(seg))).sum(0)
                near[seg_off[s]:seg_off[s + 1]] = ((Z > gu.EPS * (1 - gu.NEAR_FLOOR)) & (Z < gu.EPS * (1 + gu.NEAR_FLOOR))).numpy()
            total = total + (torch.where(m, y, torch.zeros_like(y)) * torch.tensor(g[seg_off[s]:seg_off[s + 1]], dtype=t.dtype)).sum()
        return total

    with torch.no_grad():
        loss(torch.tensor(x, dtype=F64), record=True)
    (r32,), (r64,) = gu.autograd_pair(loss, (x,))
    outs = []
    for _ in range(2):
        t = dev(x).requires_grad_(True)
        y = ops.option_normalize_(t, dev(seg_off), dev(pq), dev(np.asarray(n_list, np.int32)), NS)
        y.backward(dev(g))
        outs.append(t.grad.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    got = outs[0]
    assert np.array_equal(got[~real], g[~real])              # padding and diagonal: g passes through bit for bit
    gu.check_gradient(np.where(real, got, 0), r32, r64, "option_normalize_bwd rank %d %s" % (rank, n_list), real, near, min_max=1e-3, min_share=0.1)
    for s in range(Q):
        rows = slice(seg_off[s], seg_off[s + 1])
        if s in (sc, sb):
            assert np.array_equal(got[rows][real[rows]], g[rows][real[rows]]), "segment %d: clamped, dx = g" % s
        elif k_list[s] == 1:
            assert not got[rows][real[rows]].any(), "segment %d: one option, dx = 0" % s


# ---------------------------------------------------------------------------------------------------
# 5. the hand-written glue backwards (ops.py)
# ---------------------------------------------------------------------------------------------------
def _lp_values(rng, size, family):
    """Log-probabilities of one family with the planted edges in front: 0, a pair of 0s, and values below -47 (1 - e^x = 1 in float64)."""
    return syn.table_log_likelihood(rng, size, family)


@gpu
@pytest.mark.parametrize("family", ["mix10", "weak"])
def test_logic_backward(family):
    from dfol_vqa_amd import ops, _lib
    rng = np.random.RandomState(17)
    N = 4000
    a, b = _lp_values(rng, N, family), _lp_values(rng, N, family)
    a[0], b[0] = 0.0, -1.3                                   # a = 0
    a[1], b[1] = 0.0, 0.0                                    # a = b = 0
    a[2], b[2] = -48.0, -55.0                                # both below -47: 1 - (1 - e^a)(1 - e^b) = 0 in float64
    a[3], b[3] = -2.0, 0.0
    g = rng.normal(size=N).astype(np.float32)
    for op, name, fn in ((_lib.LOGIC_AND, "and", lambda x, y: x + y), (_lib.LOGIC_OR, "or", gu.t_or), (_lib.LOGIC_NOT, "not", lambda x, y: gu.t_lnot(x))):
        r32, r64 = gu.autograd_pair(lambda x, y: (fn(x, y) * torch.tensor(g, dtype=x.dtype)).sum(), (a, b))
        at, bt = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
        ops.logic(op, at, None if op == _lib.LOGIC_NOT else bt).backward(dev(g))
        a64, b64 = torch.tensor(a, dtype=F64), torch.tensor(b, dtype=F64)
        near = gu.t_near(a64, 1.0).numpy() if name == "not" else (gu.t_near(torch.log1p(-torch.exp(a64)) + torch.log1p(-torch.exp(b64)), 1.0).numpy() if name == "or" else None)
        gu.check_gradient(at.grad.cpu().numpy(), r32[0], r64[0], "logic %s %s da" % (name, family), near=near, min_max=1e-3, min_share=0.1)
        if name == "not":
            assert bt.grad is None
        else:
            gu.check_gradient(bt.grad.cpu().numpy(), r32[1], r64[1], "logic %s %s db" % (name, family), near=near, min_max=1e-3, min_share=0.1)
        if name == "and":
            assert np.array_equal(at.grad.cpu().numpy(), g) and np.array_equal(bt.grad.cpu().numpy(), g)


@gpu
@pytest.mark.parametrize("as_written", [False, True])
@pytest.mark.parametrize("family", ["mix10", "weak"])
def test_segment_or_backward(family, as_written):
    from dfol_vqa_amd import ops
    rng = np.random.RandomState(19 + as_written)
    sizes = [1, 3, 1, 26, 2, 0, 7, 2, 2, 1, 40, 5]
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    lp = _lp_values(rng, seg_off[-1], family)
    lp[seg_off[1]] = 0.0                                     # a = 0 in a segment of three
    lp[seg_off[4]:seg_off[5]] = 0.0                          # a = b = 0
    lp[seg_off[7]:seg_off[8]] = (-48.0, -60.0)               # both below -47: the inner sum is exactly 0
    lp[seg_off[9]] = -47.5                                   # alone, below -47
    g = rng.normal(size=len(sizes)).astype(np.float32)
    near = np.zeros(len(lp), bool)

    def loss(x, record=False):
        total = x.new_zeros(())
        for s in range(len(sizes)):
            seg = x[seg_off[s]:seg_off[s + 1]]
            if len(seg):
                if record:
                    near[seg_off[s]:seg_off[s + 1]] = (gu.t_near(seg, 1.0) | gu.t_near(gu.t_lnot(seg).sum(), 1.0)).numpy()
                total = total + float(g[s]) * gu.t_segment_or(seg)
        return total

    with torch.no_grad():
        loss(torch.tensor(lp, dtype=F64), record=True)
    (r32,), (r64,) = gu.autograd_pair(loss, (lp,))
    t = dev(lp).requires_grad_(True)
    ops.segment_or(t, dev(seg_off), as_written).backward(dev(g))
    gu.check_gradient(t.grad.cpu().numpy(), r32, r64, "segment_or %s as_written=%d" % (family, as_written), near=near, min_max=1e-3, min_share=0.1)


@gpu
@pytest.mark.parametrize("family", ["mix10", "weak"])
def test_implication_backward(family):
    from dfol_vqa_amd import ops
    rng = np.random.RandomState(23)
    n_list, k_list = [5, 1, 40, 3, 100], [2, 1, 3, 0, 1]
    pq, NS, prior, _, _, x = logic_inputs(rng, n_list, k_list, family, plant=False)
    P, Q = len(pq), len(n_list)
    x[0, 0] = 0.0                                            # a = 0
    x[0, 1], prior[0, 1] = 0.0, 0.0                          # a = b = 0
    x[0, 2], prior[0, 2] = -48.0, -50.0                      # both below -47
    x[0, 3], prior[0, 3] = -50.0, 0.0                        # prior + not(x) = 0: the outer not is clamped
    g = _incoming(rng, (P, NS))
    for p in range(P):
        g[p, n_list[pq[p]]:] = 7.0
    near_x, near_p = np.zeros((P, NS), bool), np.zeros((Q, NS), bool)

    def loss(a, t, record=False):
        total = a.new_zeros(())
        for p in range(P):
            q, n = pq[p], n_list[pq[p]]
            if record:
                m = (gu.t_near(t[p, :n], 1.0) | gu.t_near(a[q, :n] + gu.t_lnot(t[p, :n]), 1.0)).numpy()
                near_x[p, :n] = m
                near_p[q, :n] |= m
            total = total + (gu.t_implication(a[q, :n], t[p, :n]) * torch.tensor(g[p, :n], dtype=a.dtype)).sum()
        return total

    with torch.no_grad():
        loss(torch.tensor(prior, dtype=F64), torch.tensor(x, dtype=F64), record=True)
    r32, r64 = gu.autograd_pair(loss, (prior, x))
    at, xt = dev(prior).requires_grad_(True), dev(x).requires_grad_(True)
    ops.implication(at, xt, dev(pq), dev(np.asarray(n_list, np.int32))).backward(dev(g))
    owned_x = np.arange(NS)[None, :] < np.asarray(n_list)[pq][:, None]
    owned_p = (np.arange(NS)[None, :] < np.asarray(n_list)[:, None]) & np.isin(np.arange(Q), pq)[:, None]
    gu.check_gradient(at.grad.cpu().numpy(), r32[0], r64[0], "implication %s d prior" % family, owned_p, near_p, min_max=1e-3, min_share=0.1)
    gu.check_gradient(xt.grad.cpu().numpy(), r32[1], r64[1], "implication %s dx" % family, owned_x, near_x, min_max=1e-3, min_share=0.1,
                      signed_zero_ok=True)


@gpu
@pytest.mark.parametrize("family", ["mix10", "weak"])
def test_compare_backward(family):
    from dfol_vqa_amd import ops
    rng = np.random.RandomState(29)
    N = 2000
    a, b = _lp_values(rng, N, family), _lp_values(rng, N, family)
    a[0], b[0] = -48.0, -55.0                                # both below -47: the softmax does not care
    a[1], b[1] = -60.0, -60.0
    a[2], b[2] = 0.0, -50.0                                  # log-softmax 0 against -50: 1 - softmax = 2e-22, clamped
    a[3], b[3] = -50.0, 0.0
    a[4], b[4] = 0.0, 0.0
    is_less = (np.arange(N) % 2).astype(np.float32)
    is_less[2:4] = (1.0, 1.0)
    g = rng.normal(size=(N, 2)).astype(np.float32)
    r32, r64 = gu.autograd_pair(lambda x, y: (gu.t_compare(x, y, torch.tensor(is_less, dtype=x.dtype)) * torch.tensor(g, dtype=x.dtype)).sum(), (a, b))
    ls = torch.log_softmax(torch.stack([torch.tensor(a, dtype=F64), torch.tensor(b, dtype=F64)], 1), 1)
    near = gu.t_near(ls, torch.tensor(is_less, dtype=F64)[:, None]).any(1).numpy()
    at, bt = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    ops.compare(at, bt, dev(is_less)).backward(dev(g))
    gu.check_gradient(at.grad.cpu().numpy(), r32[0], r64[0], "compare %s d lp1" % family, near=near, min_max=1e-3, min_share=0.1)
    gu.check_gradient(bt.grad.cpu().numpy(), r32[1], r64[1], "compare %s d lp2" % family, near=near, min_max=1e-3, min_share=0.1)


@gpu
def test_gate_and_segment_sum_rows_backward_are_exact():
    from dfol_vqa_amd import ops
    rng = np.random.RandomState(31)
    P, NS = 37, 44
    x, y = rng.normal(size=(P, NS)).astype(np.float32), rng.normal(size=(P, NS)).astype(np.float32)
    xq, yq = rng.uniform(size=P).astype(np.float32), rng.uniform(size=P).astype(np.float32)
    sel = (rng.uniform(size=P) < 0.5).astype(np.float32)
    g = rng.normal(size=(P, NS)).astype(np.float32)
    xt, yt = dev(x).requires_grad_(True), dev(y).requires_grad_(True)
    att, quant = ops.gate(xt, yt, dev(xq), dev(yq), dev(sel))
    assert not quant.requires_grad
    att.backward(dev(g))
    r32, r64 = gu.autograd_pair(lambda u, v: ((u * torch.tensor(sel, dtype=u.dtype)[:, None] + v * (1 - torch.tensor(sel, dtype=u.dtype))[:, None])
                                              * torch.tensor(g, dtype=u.dtype)).sum(), (x, y))
    assert np.array_equal(xt.grad.cpu().numpy().astype(np.float64), r64[0]) and np.array_equal(yt.grad.cpu().numpy().astype(np.float64), r64[1])
    assert np.array_equal(xt.grad.cpu().numpy(), np.where(sel[:, None] > 0, g, 0)) and np.array_equal(yt.grad.cpu().numpy(), np.where(sel[:, None] > 0, 0, g))
    # segment_sum_rows: every row of a segment receives the segment's gradient row
    sizes = [1, 3, 0, 5, 1, 26, 0, 1]
    seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    for width in (1, 7, 300):
        src = rng.normal(size=(seg_off[-1], width)).astype(np.float32)
        gq = rng.normal(size=(len(sizes), width)).astype(np.float32)
        st = dev(src).requires_grad_(True)
        ops.segment_sum_rows(st, dev(seg_off)).backward(dev(gq))
        (r32,), (r64,) = gu.autograd_pair(lambda s: sum((s[seg_off[i]:seg_off[i + 1]].sum(0) * torch.tensor(gq[i], dtype=s.dtype)).sum()
                                                         for i in range(len(sizes))), (src,))
        assert np.array_equal(st.grad.cpu().numpy().astype(np.float64), r64)
        assert np.array_equal(st.grad.cpu().numpy(), np.repeat(gq, sizes, axis=0))
