"""The one-posterior Relate of the ungated train step (DFOL_RELATE_TRAIN=1): dfol_relate_keep_fwd_f32 (csrc/dfol_logic.hip) and
dfol_relate_keep_bwd_f32 (csrc/dfol_logic_bwd.hip) against the float64 restatement golden_util.t_relate and its torch autograd, and against the
generic route (gate, gate, relate_fwd(want), gate and dfol_relate_bwd_f32 with the unkept cotangent zero) they replace.

The tile S holds SUBJECTS along rows for every predicate.  Flag set -> the kept posterior is post_s of t_relate(a = x, b = prev, l = S);
clear -> post_o of t_relate(a = prev, b = x, l = S); both quantifiers prev's.  The kernels see NaN in every padding cell of x, prev and S and
a live value on S's diagonal; the restatement only ever sees the n x n block.

Dispatch arms (NS / 4 column groups -> lanes per row; NS > 256 -> the plain workgroup kernel):
NS 4 -> LPR 1 | 8 -> 2 | 20 -> 8 | 40 -> 16 | 104 -> 32 | 256 -> 64 | 260 -> plain.  The backward is one kernel for every NS <= 2048
(16 wavefronts up to NS = 680, four beyond).

Bounds: golden_util.check_logprob's policy forward, test_trainable_gate_gpu.grad_close (8 times the restatement's own fp32-vs-fp64
distance plus 2e-3 of the tensor's largest magnitude) backward.  No tolerance of this file's own."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as U  # noqa: E402
import test_trainable_gate_gpu as TG  # noqa: E402
from dfol_vqa_amd import _lib, ops  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu
dev = TG.dev
_CACHE = {}
LEAVES = ("x", "prev", "S")

# name: (NS, objects per image, predicates per image, negation, inactive rows, quantifiers, subject flags)
SHAPES = {
    "ns4_lpr1_n1234": (4, [1, 2, 3, 4], [1, 1, 1, 1], False, False, "mixed", "mixed"),      # n = 1: no off-diagonal term; 2, 3: padding inside the float4
    "ns8_lone_forall_row": (8, [7], [1], False, False, "forall", "one"),                     # P = 1: the lone FOR_ALL's literal branch, row aggregate
    "ns8_lone_forall_col": (8, [6], [1], False, False, "forall", "zero"),                    # ... column aggregate
    "ns8_lone_exists": (8, [8], [1], False, False, "exists", "one"),
    "ns8_lpr2_neg": (8, [5, 8, 6, 1], [1, 1, 1, 1], True, False, "mixed", "mixed"),          # one negated predicate clamps all
    "ns20_lpr8_P5_manytoone": (20, [17, 20], [3, 2], True, True, "mixed", "mixed"),          # P = 5: not a multiple of the workgroup's 4 predicates
    "ns40_lpr16_exists_rows": (40, [40, 33], [2, 2], False, True, "exists", "one"),
    "ns40_lpr16_forall_cols": (40, [37, 40], [2, 2], False, False, "forall", "zero"),
    "ns40_lpr16_forall_neg": (40, [40, 21], [2, 2], True, False, "forall", "mixed"),
    "ns104_lpr32": (104, [101, 104, 1], [1, 2, 1], True, False, "mixed", "mixed"),
    "ns256_lpr64": (256, [256, 130], [2, 2], False, False, "mixed", "mixed"),
    "ns260_plain": (260, [257, 3], [2, 2], True, True, "mixed", "mixed"),
}


def keep_problem(name):
    """Inputs of one shape, the restatement's kept posterior and its gradients (the problem's own random cotangent, zero on padding) in float32
    and float64; computed once, shared, never modified."""
    if name not in _CACHE:
        _CACHE[name] = make_problem(name, SHAPES[name])
    return _CACHE[name]


def make_problem(name, spec, restate=True):
    """The generator behind keep_problem for a shape tuple of SHAPES' form (the name seeds it); a new dict each call, nothing cached.
    restate=False leaves the float32 / float64 restatement out, for a test that compares kernels with each other."""
    NS, n_list, k_list, with_neg, with_inactive, quants, flags = spec
    rng = np.random.RandomState(sum(map(ord, name)))
    Q, pq = len(n_list), np.repeat(np.arange(len(n_list)), k_list).astype(np.int32)
    P = len(pq)
    kp = dict(NS=NS, n=np.asarray(n_list, np.int32), pq=pq, P=P, Q=Q, lone=(P == 1))
    idx = np.arange(P)
    # one quantifier per question (its predicates share prev, whose scale below goes with the quantifier); the flags alternate against it
    kp["quant"] = {"exists": np.ones(P), "forall": np.zeros(P), "mixed": pq % 2}[quants].astype(np.float32)
    kp["flag"] = {"one": np.ones(P), "zero": np.zeros(P), "mixed": (idx // 2) % 2 if max(k_list) == 1 else idx % 2}[flags].astype(np.uint8)
    kp["neg"] = (idx % 3 == 1).astype(np.uint8) if with_neg else None                     # (negated somewhere: every predicate goes through the clamp)
    kp["active"] = (idx != 1).astype(np.uint8) if with_inactive else None
    kp["x"], kp["prev"], kp["S"] = np.zeros((P, NS), np.float32), np.zeros((Q, NS), np.float32), np.zeros((P, NS, NS), np.float32)
    # The aggregate over n objects must stay off its clamp, or forward and gradient are constants and check nothing: a FOR_ALL sum of n terms
    # gets terms of size 3 / n (a negated one l' = log(1 - e^l) with l <= -3), an EXISTS union of n terms gets prev lowered by log(n / 4).
    for p in range(P):
        q = pq[p]
        n = n_list[q]
        kp["x"][p, :n] = np.minimum(syn.table_log_likelihood(rng, (n,), "unif") * 0.3, 0)
        t = syn.table_log_likelihood(rng, (n, n), "mix10")                               # (the diagonal too: the kernels must drop it themselves)
        prev = np.minimum(syn.table_log_likelihood(rng, (n,), "unif") * 0.3, 0)
        if n > 4 and kp["quant"][p] == 0:
            prev = prev * (3.0 / n)
            t = -(3.0 + 0.3 * np.abs(t)) if (with_neg and kp["neg"][p]) else t * (3.0 / n)
        elif n > 8:
            prev = prev - np.log(n / 4.0)
        kp["S"][p, :n, :n] = t
        if p == 0 or pq[p - 1] != q:
            kp["prev"][q, :n] = prev
    kp["live"] = np.ones(P, bool) if kp["active"] is None else kp["active"].astype(bool)
    kp["cot"] = rng.normal(size=(P, NS)).astype(np.float32)
    for p in range(P):
        kp["cot"][p, n_list[pq[p]]:] = 0
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)) if restate else ():
        kp[tag] = restate_keep(kp, dt, kp["cot"])
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)) if restate else ():   # the cotangent of the live rows alone
        kp[tag + "_live"] = kp[tag]["g"] if kp["live"].all() else restate_keep(kp, dt, kp["cot"] * kp["live"][:, None])["g"]
    return kp


def restate_keep(kp, dt, cot):
    lv = {k: torch.tensor(kp[k], dtype=dt, requires_grad=True) for k in LEAVES}
    any_neg = kp["neg"] is not None
    rows = []
    for p in range(kp["P"]):
        q = kp["pq"][p]
        n = kp["n"][q]
        x, prev, S = lv["x"][p, :n], lv["prev"][q, :n], lv["S"][p, :n, :n]
        if not kp["live"][p]:
            post = prev
        else:
            ng, qp = (float(kp["neg"][p]) if any_neg else 0.0), kp["quant"][p]
            if kp["flag"][p]:
                post = U.t_relate(x, prev, S, qp, qp, ng, any_neg, lone_forall_identity=kp["lone"])[0]
            else:
                post = U.t_relate(prev, x, S, qp, qp, ng, any_neg, lone_forall_identity=kp["lone"])[1]
        rows.append(torch.cat([post, torch.zeros(kp["NS"] - n, dtype=dt)]))
    out = torch.stack(rows)
    g = torch.autograd.grad((out * torch.tensor(cot, dtype=dt)).sum(), [lv[k] for k in LEAVES], allow_unused=True)
    return {"out": out.detach().numpy(), "g": {k: (np.zeros(lv[k].shape) if v is None else v.numpy().astype(np.float64)) for k, v in zip(LEAVES, g)}}


def owned_masks(kp):
    col = np.arange(kp["NS"])
    prev = col[None, :] < kp["n"][:, None]                                   # [Q, NS]
    row = col[None, :] < kp["n"][kp["pq"]][:, None]                          # [P, NS]
    x = row & kp["live"][:, None]                                            # a no-op predicate's posterior does not see x
    tile = x[:, :, None] & x[:, None, :] & ~np.eye(kp["NS"], dtype=bool)[None]
    return x, prev, tile, row


def poisoned(kp):
    """x, prev and S with NaN in every padding cell: nothing of it may reach an output."""
    _, o_prev, _, row = owned_masks(kp)
    x = np.where(row, kp["x"], np.nan).astype(np.float32)
    prev = np.where(o_prev, kp["prev"], np.nan).astype(np.float32)
    S = np.where(row[:, :, None] & row[:, None, :], kp["S"], np.nan).astype(np.float32)
    return x, prev, S


def device_args(kp):
    pq = dev(kp["pq"])
    pq._dfol_sorted = True                                        # (np.repeat of arange: non-decreasing)
    return pq, dev(kp["n"]), dev(kp["quant"]), dev(kp["flag"]), dev(kp["neg"]), dev(kp["active"])


def run_fwd(kp):
    x, prev, S = (dev(a) for a in poisoned(kp))
    pq, n, quant, flag, neg, active = device_args(kp)
    return _lib.relate_keep_fwd(x, prev, S, pq, n, quant, flag, neg, active, lone_forall_identity=kp["lone"])


def run_autograd(kp, cot):
    """ops.relate_keep and its backward on the poisoned inputs -> (posterior, {leaf name: gradient})."""
    x, prev, S = (torch.tensor(a, device=TG.DEV, requires_grad=True) for a in poisoned(kp))
    pq, n, quant, flag, neg, active = device_args(kp)
    out = ops.relate_keep(x, prev, S, pq, n, quant, flag, neg, active, lone_forall_identity=kp["lone"])
    assert out.grad_fn is not None
    (out * dev(cot)).sum().backward()
    return out.detach(), {"x": x.grad.cpu().numpy(), "prev": prev.grad.cpu().numpy(), "S": S.grad.cpu().numpy()}


def run_generic(kp, cot):
    """gate, gate, ops.relate_fwd(want), gate under autograd, one question per predicate, on the clean inputs."""
    x, prev, S = (torch.tensor(kp[k], device=TG.DEV, requires_grad=True) for k in LEAVES)
    quant, g = dev(kp["quant"]), dev(kp["flag"].astype(np.float32))
    prev_p = prev[torch.tensor(kp["pq"].astype(np.int64), device=TG.DEV)]
    prior_s, _ = ops.gate(x, prev_p, quant, quant, g)
    prior_o, _ = ops.gate(prev_p, x, quant, quant, g)
    want = dev(np.where(kp["flag"] > 0, _lib.WANT_SUBJECT, _lib.WANT_OBJECT).astype(np.uint8))
    ident = dev(np.arange(kp["P"], dtype=np.int32))
    ident._dfol_sorted = True
    ps, po = ops.relate_fwd(prior_s, prior_o, S, ident, dev(kp["n"][kp["pq"]]), quant, quant, dev(kp["neg"]), dev(kp["active"]), want=want,
                            lone_forall_identity=kp["lone"])
    kept, _ = ops.gate(ps, po, quant, quant, g)
    (kept * dev(cot)).sum().backward()
    return kept.detach().cpu().numpy(), {"x": x.grad.cpu().numpy(), "prev": prev.grad.cpu().numpy(), "S": S.grad.cpu().numpy()}


def check_grads(got, r32, r64, what):
    for k in LEAVES:
        TG.grad_close(got[k], r32[k], r64[k], "%s d %s" % (what, k))


def check_unowned_are_plus_zero(got, kp, what):
    o_x, o_prev, o_tile, _ = owned_masks(kp)
    for k, owned in (("x", o_x), ("prev", o_prev), ("S", o_tile)):
        stray = got[k][~owned]
        assert not stray.view(np.uint32).any(), "%s d %s: %d cells nobody owns are not +0" % (what, k, int((stray.view(np.uint32) != 0).sum()))


def test_the_cases_cover_what_they_are_for():
    kps = [keep_problem(n) for n in SHAPES]
    assert sorted({k["NS"] for k in kps}) == [4, 8, 20, 40, 104, 256, 260]
    assert {k["P"] for k in kps} >= {1, 5}
    for k in kps:
        assert (k["n"] <= k["NS"]).all()
    assert any((k["n"] == 1).any() for k in kps) and any((k["n"] == k["NS"]).any() for k in kps) and any((k["n"] % 4 != 0).any() for k in kps)
    for want in ({0.0}, {1.0}, {0.0, 1.0}):                      # all FOR_ALL, all EXISTS, mixed within a launch; the same for the flags
        assert any({float(v) for v in k["quant"]} == want for k in kps), want
        assert any({float(v) for v in k["flag"]} == want for k in kps), want
    both = [k for k in kps if k["P"] >= 4 and len(set(k["quant"])) == 2]
    assert both and all({(q, f) for q, f in zip(k["quant"], k["flag"])} == {(0, 0), (0, 1), (1, 0), (1, 1)} for k in both)
    assert any(k["neg"] is not None and 0 < k["neg"].sum() < k["P"] for k in kps)                      # one negated among un-negated
    assert any(k["neg"] is not None and k["neg"].any() and (k["quant"] == 0).all() for k in kps)        # the negated FOR_ALL form
    assert any(not k["live"].all() and k["live"].any() for k in kps)
    assert all(any(k["lone"] and k["quant"][0] == 0 and k["flag"][0] == f for k in kps) for f in (0, 1))
    assert any(len(k["pq"]) > len(set(k["pq"])) for k in kps)                                          # many-to-one pred_q
    for k in kps:                                                 # the two axes are told apart: the tile is not symmetric
        if k["n"].max() > 1:
            assert not np.array_equal(k["S"], k["S"].transpose(0, 2, 1))


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_against_the_float64_restatement(name):
    kp = keep_problem(name)
    with torch.no_grad():
        got = run_fwd(kp).cpu().numpy()
        again = run_fwd(kp).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))                          # two launches, the same bits
    U.check_logprob(got, kp["f32"]["out"], kp["f64"]["out"], name)
    for p in range(kp["P"]):
        assert not got[p, kp["n"][kp["pq"][p]]:].view(np.uint32).any(), (name, p, "padding")  # exactly +0
    for p in np.nonzero(~kp["live"])[0]:                           # a no-op row is prev's row, bit for bit
        q, n = kp["pq"][p], kp["n"][kp["pq"][p]]
        assert np.array_equal(got[p, :n].view(np.uint32), kp["prev"][q, :n].view(np.uint32))
    # the other axis summed out lies outside the bound wherever there is more than one object: the bound tells the two apart
    if kp["n"].max() > 2 and kp["live"].any():
        wrong = dict(kp, flag=1 - kp["flag"])
        with pytest.raises(AssertionError):
            U.check_logprob(restate_keep(wrong, torch.float64, kp["cot"])["out"], kp["f32"]["out"], kp["f64"]["out"], name + " with the axes swapped")


@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_against_the_float64_restatement(name):
    kp = keep_problem(name)
    out, got = run_autograd(kp, kp["cot"])
    U.check_logprob(out.cpu().numpy(), kp["f32"]["out"], kp["f64"]["out"], name + " forward under autograd")
    check_grads(got, kp["f32"]["g"], kp["f64"]["g"], name)
    check_unowned_are_plus_zero(got, kp, name)
    _, again = run_autograd(kp, kp["cot"])                         # two runs, the same bits
    for k in LEAVES:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), (name, k)


@pytest.mark.parametrize("name", list(SHAPES))
def test_exact_outputs_of_the_backward_kernel(name):
    """The kernel's own outputs, before any reduction by question: g_x is the cotangent on a live row and +0 on a no-op one, a no-op row's g_prev is
    its cotangent bit for bit, and padding, the diagonal and a no-op predicate's tile are +0."""
    kp = keep_problem(name)
    x, prev, S = (dev(a) for a in poisoned(kp))
    pq, n, quant, flag, neg, active = device_args(kp)
    g_x, pp, g_tile = (t.cpu().numpy() for t in _lib.relate_keep_bwd(dev(kp["cot"]), x, prev, S, pq, n, quant, flag, neg, active, kp["lone"],
                                                                     identity=True))
    assert pp.shape == (kp["P"], kp["NS"])
    o_x, _, o_tile, row = owned_masks(kp)
    assert not g_tile[~o_tile].view(np.uint32).any() and not pp[~row].view(np.uint32).any() and not g_x[~o_x].view(np.uint32).any()
    assert np.array_equal(g_x[o_x].view(np.uint32), kp["cot"][o_x].view(np.uint32))
    dead = ~kp["live"]
    assert np.array_equal(pp[dead].view(np.uint32), kp["cot"][dead].view(np.uint32))
    assert np.isfinite(g_tile).all() and np.isfinite(pp).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_generic_route(name):
    """Both routes within the bounds of the same float64 values (no bit equality is promised).  A no-op row of the generic cell is the wanted side's
    own prior - x where x is the subject - and the interpreter's mask puts prev back; the one-launch kernel writes prev at once.  So the cotangent
    here is the problem's on the live rows and zero on the no-op rows, and the posteriors are compared on the live rows: what the two routes share."""
    kp = keep_problem(name)
    cot = kp["cot"] * kp["live"][:, None]
    out_one, one = run_autograd(kp, cot)
    out_gen, generic = run_generic(kp, cot)
    live = kp["live"]
    U.check_logprob(out_one.cpu().numpy()[live], kp["f32"]["out"][live], kp["f64"]["out"][live], name + " one launch")
    U.check_logprob(out_gen[live], kp["f32"]["out"][live], kp["f64"]["out"][live], name + " generic route")
    for what, got in (("one launch", one), ("generic route", generic)):
        check_grads(got, kp["f32_live"], kp["f64_live"], "%s %s" % (name, what))
    same = all(np.array_equal(one[k].view(np.uint32), generic[k].view(np.uint32)) for k in LEAVES)
    print("  %s: the two routes' gradients %s" % (name, "agree to the bit" if same else "differ in bits (within the bound)"))


def test_refusals_come_before_any_launch():
    """1 object slot beyond the backward's limit, a bf16 tile, a non-contiguous tensor, CPU tensors, a wrong flag count: every one refused, and the
    two entry points were not called once (the wrappers' per-entry-point launch record stays empty)."""
    kp = keep_problem("ns8_lpr2_neg")
    x, prev, S = (dev(kp[k]) for k in LEAVES)
    pq, n, quant, flag, neg, active = device_args(kp)
    cot = dev(kp["cot"])
    names = ("dfol_relate_keep_fwd_f32", "dfol_relate_keep_bwd_f32", "dfol_reduce_by_question_f32")
    _lib.enable_kernel_timing(names)
    try:
        with pytest.raises(_lib.DfolError, match="fp32 tiles"):
            _lib.relate_keep_fwd(x, prev, S.to(torch.bfloat16), pq, n, quant, flag, neg, active)
        with pytest.raises(_lib.DfolError, match="fp32 tiles"):
            _lib.relate_keep_bwd(cot, x, prev, S.to(torch.bfloat16), pq, n, quant, flag, neg, active, False)
        with pytest.raises(_lib.DfolError, match="contiguous"):
            _lib.relate_keep_fwd(x, prev, S.transpose(1, 2), pq, n, quant, flag, neg, active)
        with pytest.raises(_lib.DfolError, match="contiguous"):
            _lib.relate_keep_bwd(cot.t().contiguous().t(), x, prev, S, pq, n, quant, flag, neg, active, False)
        with pytest.raises(_lib.DfolError, match="no CPU fallback"):
            _lib.relate_keep_fwd(x.cpu(), prev, S, pq, n, quant, flag, neg, active)
        with pytest.raises(_lib.DfolError, match="no CPU fallback"):
            _lib.relate_keep_bwd(cot, x, prev.cpu(), S, pq, n, quant, flag, neg, active, False)
        with pytest.raises(_lib.DfolError, match="subject flags"):
            _lib.relate_keep_fwd(x, prev, S, pq, n, quant, flag[:2], neg, active)
        with pytest.raises(_lib.DfolError, match="do not match"):
            _lib.relate_keep_bwd(cot, x[:, :4].contiguous(), prev, S, pq, n, quant, flag, neg, active, False)
        NS = _lib.RELATE_KEEP_BWD_MAX_NS + 4
        z = lambda *s: torch.zeros(*s, device=TG.DEV)
        one = torch.ones(1, dtype=torch.uint8, device=TG.DEV)
        i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=TG.DEV)
        with pytest.raises(_lib.DfolError, match="at most 2048"):
            _lib.relate_keep_bwd(z(1, NS), z(1, NS), z(1, NS), z(1, NS, NS), i32(0), i32(NS), z(1), one, None, None, True)
        with pytest.raises(_lib.DfolError, match="at most 2048"):   # through the autograd front too
            out = ops.relate_keep(z(1, NS).requires_grad_(True), z(1, NS), z(1, NS, NS), i32(0), i32(3), z(1), one)
            out.sum().backward()
    finally:
        torch.cuda.synchronize()                                    # (the record's events must have completed before it is read)
        counts = _lib.disable_kernel_timing()
    assert counts["dfol_relate_keep_bwd_f32"][0] == 0 and counts["dfol_reduce_by_question_f32"][0] == 0, counts
    assert counts["dfol_relate_keep_fwd_f32"][0] == 1, counts      # only the forward of the last case, whose backward was refused
