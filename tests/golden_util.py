"""Helpers shared by the golden tests: loading fixtures, rebuilding questions, the tolerance policy."""

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    arrays = np.load(os.path.join(GOLDEN, name + ".npz"))
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    return arrays, meta


def questions_and_scenes(arrays, meta, feature_key=None):
    qs, scenes = [], []
    for i, q in enumerate(meta["questions"]):
        qs.append({"program": q["program"], "answer": q["answer"], "question_id": q["question_id"],
                   "image_id": "img%03d" % (q["question_id"] % 64), "tokens": [], "original_dict": None, "question": None})
        if feature_key is None:
            scenes.append({"n": q["n"], "A": arrays["A_%d" % i], "R": arrays["R_%d" % i]})
        else:
            scenes.append({"n": q["n"], "X": arrays["%s_%d" % (feature_key, i)]})
    return qs, scenes


G4_CASES = ["g4_exist", "g4_exist_split3", "g4_threehop_n36", "g4_verify_attrs", "g4_choose_attr", "g4_choose_attr_nonorm",
            "g4_query_attr", "g4_verify_rel", "g4_choose_rel", "g4_and", "g4_or", "g4_two_same", "g4_two_different",
            "g4_all_same", "g4_all_different", "g4_compare"]
G4_STRESS = ["g4_stress_mix05", "g4_stress_weak"]
G14_CASES = ["g14_threshold_query_attr", "g14_threshold_choose_attr", "g14_threshold_choose_rel"]      # likelihood_threshold > 0
G11_CASES = ["g11_hard_exist", "g11_hard_single", "g11_hard_verify_attrs", "g11_hard_query_attr", "g11_hard_choose_rel", "g11_hard_and",
             "g11_hard_two_same", "g11_hard_all_same", "g11_hard_all_different", "g11_hard_two_different", "g11_hard_compare"]       # hard_mode = True (batch_base_types.py:104-112)


def check_logprob(got, ref32, ref64, what="", lp_tol=1e-4, p_tol=1e-6, K=2.0, floor=-5.0):
    """Tolerance policy for fp32 log-probabilities (SURVEY.md §7 hard part 1).

    The reference evaluates log(1 - e^x) naively in fp32, so some outputs are ill-conditioned: the
    reference's own fp32 run then differs from its fp64 run by far more than 1e-4 (and `compare`
    renormalises two such values).  Every golden therefore carries both runs, and the reference's own
    fp32-vs-fp64 deviation is the yardstick for how much rounding noise an output carries:

    (i)   where the fp64 golden says lp >= floor AND the reference's own fp32 run is within lp_tol/4 of it
          (the output is demonstrably well-conditioned):   |got - ref32| <= lp_tol           (the 1e-4 bar)
    (ii)  everywhere, in probability space:  |e^got - e^ref64| <= K * max|e^ref32 - e^ref64| + p_tol
    (iii) where lp >= floor:                 |got - ref64|     <= K * max|ref32 - ref64|     + lp_tol
          (max over the case: one fp32 sample of the noise is not a bound for another)
    """
    got, ref32, ref64 = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref32, ref64))
    assert got.shape == ref32.shape == ref64.shape, (what, got.shape, ref32.shape)
    assert np.all(np.isfinite(got)), what
    err_ref = np.abs(ref32 - ref64)
    region = ref64 >= floor
    good = region & (err_ref <= lp_tol / 4)
    d = np.abs(got - ref32)
    if good.any():
        assert np.all(d[good] <= lp_tol), "%s: |dlp| %.3g > %g on well-conditioned outputs" % (what, d[good].max(), lp_tol)
    ep_ref = np.abs(np.exp(ref32) - np.exp(ref64)).max()
    ep_got = np.abs(np.exp(got) - np.exp(ref64))
    assert ep_got.max() <= K * ep_ref + p_tol, "%s: |dp| %.3g vs reference's own %.3g" % (what, ep_got.max(), ep_ref)
    if region.any():
        e_got = np.abs(got - ref64)[region]
        assert e_got.max() <= K * err_ref[region].max() + lp_tol, \
            "%s: |dlp vs fp64| %.3g vs reference's own %.3g" % (what, e_got.max(), err_ref[region].max())
    return int(good.sum()), int(len(got))


G17_CASES = ["c1_n36"] + [k + "_n60_100" for k in ("exist", "and", "or", "verify_attrs", "verify_rel", "choose_attr", "query_attr", "choose_rel",
                                                    "two_same", "two_different", "all_same", "all_different", "compare")]


def g17_case(name, arrays, meta):
    """Questions and scenes of one case of golden family g17 (the reference at full model size): everything but the reference's outputs
    is regenerated from seeds by dfol_vqa_amd.synthetic."""
    from dfol_vqa_amd import synthetic as syn
    cm = meta["cases"][name]
    qs = [syn.question(q["question_id"], q["program"]["branches"], q["program"]["last_op"], q["answer"]) for q in cm["questions"]]
    scenes = [syn.feature_scene(q["question_id"], q["n"], meta["feature_dim"]) for q in cm["questions"]]
    return qs, scenes, cm, arrays[name + ":lp_f32"], arrays[name + ":lp_f64"]


def decided_answers(cm, lp32, lp64):
    """Which questions' answers the reference's own fp32 and fp64 runs agree on with a margin (an arg-max over near-ties, or a yes / no
    at p ~ 0.5, is decided by rounding noise)."""
    lp32, lp64 = np.asarray(lp32, np.float64), np.asarray(lp64, np.float64)
    if cm["type"] == 1 and cm["options"] and isinstance(cm["options"][0], list):            # QUERY: per-question option lists
        sizes = [len(o) for o in cm["options"]]
        off = np.concatenate([[0], np.cumsum(sizes)])
        out = []
        for i in range(len(sizes)):
            a64, a32 = lp64[off[i]:off[i + 1]], lp32[off[i]:off[i + 1]]
            top = np.sort(a64)[::-1]
            out.append(len(top) < 2 or top[0] - top[1] > 4 * np.abs(a32 - a64).max() + 1e-4)
        return out
    return list(np.abs(np.exp(lp64) - 0.5) > 4 * np.abs(np.exp(lp32) - np.exp(lp64)) + 1e-5)


G19_CASES = ["binary_small", "query_rel_small", "binary_tall", "query_rel_tall"]
# round 6: the attribute-side and two-branch terminals (QUERY loss over a category's 26 options, choose_attr, verify_attrs, and / or,
# compare, two_same, all_different) - VERDICT r5 #1
G19_ATTR_CASES = ["query_attr_small", "choose_attr_small", "verify_attrs_small", "and_small", "and_tall", "or_small", "compare_small", "two_same_small",
                  "all_different_small"]


def g19_case(name, arrays, meta):
    """One case of golden family g19 (the reference's `_train_batch` gradients at full model size): questions with their scenes (regenerated
    from seeds), the reference's loss / log-probabilities and, per weight tensor, gradient norm + sampled values, fp32 and fp64."""
    from dfol_vqa_amd import synthetic as syn
    cm = meta["cases"][name]
    qs = [syn.question(q["question_id"], q["program"]["branches"], q["program"]["last_op"], q["answer"], syn.feature_scene(q["question_id"], q["n"], 2048))
          for q in cm["questions"]]
    grads = {}
    for k in arrays.files:
        if k.startswith(name + ":gs:") and k.endswith(":f64"):
            pname = k[len(name) + 4:-4]
            grads[pname] = {"sample64": arrays[k], "sample32": arrays[k[:-3] + "f32"],
                            "norm64": float(arrays["%s:gn:%s:f64" % (name, pname)]), "norm32": float(arrays["%s:gn:%s:f32" % (name, pname)])}
    return qs, cm, {t: (float(arrays["%s:loss_%s" % (name, t)]), arrays["%s:lp_%s" % (name, t)]) for t in ("f32", "f64")}, grads


def check_g19_gradients(got, grads, what, rtol=2e-3, K=8.0):
    """got: {parameter name: full gradient array}.  Sampled values and norm against the reference's fp64 run, with the reference's own
    fp32-vs-fp64 deviation as the yardstick (the policy of test_backward_gpu.grad_close)."""
    from dfol_vqa_amd import synthetic as syn
    assert len(grads) == 12, sorted(grads)
    for pname, g in grads.items():
        full = np.asarray(got[pname], np.float64).reshape(-1)
        smp = full[syn.gradient_sample_index(pname, full.size)]
        ref64, ref32 = g["sample64"].astype(np.float64), g["sample32"].astype(np.float64)
        scale = max(np.abs(ref64).max(), g["norm64"] / np.sqrt(full.size)) + 1e-30
        own = np.abs(ref32 - ref64).max()
        err = np.abs(smp - ref64).max()
        assert err <= K * own + rtol * scale, "%s d%s: |dgrad| %.3g vs the reference's own %.3g (scale %.3g)" % (what, pname, err, own, scale)
        norm = np.sqrt((full ** 2).sum())
        assert abs(norm - g["norm64"]) <= K * abs(g["norm32"] - g["norm64"]) + rtol * g["norm64"] + 1e-30, \
            "%s |d%s| %.6g vs %.6g (the reference's own fp32 run %.6g)" % (what, pname, norm, g["norm64"], g["norm32"])


G23_KINDS = ["exist", "verify_attrs", "verify_rel", "choose_rel", "query_attr", "and", "two_same", "compare"]


def g23_case(kind, arrays, meta):
    """One case of golden family g23 (the reference's CALIBRATED forward at full model size): questions with their scenes regenerated from seeds."""
    from dfol_vqa_amd import synthetic as syn
    cm = meta["cases"][kind]
    qs = [syn.question(q["question_id"], q["program"]["branches"], q["program"]["last_op"], q["answer"], syn.feature_scene(q["question_id"], q["n"], meta["feature_dim"]))
          for q in cm["questions"]]
    return qs, cm


# ---------------------------------------------------------------------------------------------------
# soft-logic gradients: a torch restatement of the block formulas, differentiated by torch autograd on the
# CPU in float32 and float64, and the per-element tolerance policy of tests/test_logic_backward_gpu.py
# ---------------------------------------------------------------------------------------------------
EPS = 1e-20
NEAR_FLOOR = 1e-4             # a float64 denominator within a factor 1 +- NEAR_FLOOR of EPS may be clamped in one precision and not the other
GRAD_FLOOR = 2.0 ** -20       # dfol_exp scales x by log2(e) in fp32: e^x carries up to |x| 2^-24 (2.7e-6 at the clamp's x = -46); a gradient is a product of three such factors
GRAD_TINY = 2.0 ** -106       # fp32's smallest normal number over GRAD_FLOOR: below it a kernel that flushes subnormals is off by more than the floor allows


def t_slog(x):
    import torch
    return torch.log(x.clamp_min(EPS))


def t_pnot(x, a):
    import torch
    return t_slog(a + (1 - 2 * a) * torch.exp(x))


def t_near(x, a):
    """Where the denominator of t_pnot(x, a) lies at the clamp's boundary (float64 inputs)."""
    import torch
    d = a + (1 - 2 * a) * torch.exp(x.detach())
    return (d > EPS * (1 - NEAR_FLOOR)) & (d < EPS * (1 + NEAR_FLOOR))


def t_prep(l, neg, any_neg):
    """-relu(-l) (subgradient 0 at and above 0, as the reference's torch relu) and the optional negation."""
    import torch
    v = -torch.relu(-l)
    return t_pnot(v, float(neg)) if any_neg else v


def t_relate(a, b, l, qs, qo, neg, any_neg, lone_forall_identity=False, near=None):
    """oracle.relate_block in torch: a, b [n]; l [n, n] the raw tile, subjects along rows.  `lone_forall_identity`: a FOR_ALL variable
    takes the literal branch of a single predicate (no parametric not, no clamp).  `near` (a dict) receives the clamp-boundary masks."""
    import torch
    n = a.shape[0]
    qs, qo = float(qs), float(qo)
    v = t_prep(l, neg, any_neg)
    off = 1 - torch.eye(n, dtype=l.dtype)
    id_s, id_o = lone_forall_identity and qs == 0, lone_forall_identity and qo == 0
    F_s = (lambda x: x) if id_s else (lambda x: t_pnot(x, qs))
    F_o = (lambda x: x) if id_o else (lambda x: t_pnot(x, qo))
    u1, u2 = v + b[None, :], v + a[:, None]
    S, T = (F_o(u1) * off).sum(1), (F_s(u2) * off).sum(0)
    if near is not None:
        m = torch.zeros(n, n, dtype=torch.bool)
        if any_neg:
            m |= t_near(-torch.relu(-l), float(neg))
        if not id_o:
            m |= t_near(u1, qo) | t_near(S, qo)[:, None]
        if not id_s:
            m |= t_near(u2, qs) | t_near(T, qs)[None, :]
        m &= off.bool()
        near["tile"], near["s"], near["o"] = m, m.any(1), m.any(0)
    return a + F_o(S), b + F_s(T)


def t_filter(prior, ll, neg, any_neg):
    return prior + t_prep(ll, neg, any_neg)


def t_quantify(att, qf):
    qf = float(qf)
    return t_pnot(t_pnot(att, qf).sum(), qf)


def t_lnot(x):
    return t_pnot(x, 1.0)


def t_or(a, b):
    import torch
    return t_slog(1 - (1 - torch.exp(a)) * (1 - torch.exp(b)))


def t_segment_or(lp):
    return t_lnot(t_lnot(lp).sum())


def t_implication(prior, x):
    return t_lnot(prior + t_lnot(x))


def t_compare(lp1, lp2, is_less):
    import torch
    ls = torch.log_softmax(torch.stack([lp1, lp2], 1), 1)
    return t_pnot(ls, is_less[:, None])


def t_option_normalize(x):
    """x [K, ...]: the K options of one segment."""
    import torch
    return x - t_slog(torch.exp(x).sum(0, keepdim=True))


def autograd_pair(fn, inputs):
    """fn(*tensors) -> scalar.  Gradients w.r.t. every input from torch autograd on the CPU, once in float32 and once in float64:
    ([r32...], [r64...]) as float64 numpy arrays (an input that does not reach the result has gradient 0)."""
    import torch
    out = []
    for dt in (torch.float32, torch.float64):
        leaves = [torch.tensor(np.asarray(x), dtype=dt, requires_grad=True) for x in inputs]
        fn(*leaves).backward()
        out.append([np.zeros(t.shape) if t.grad is None else t.grad.numpy().astype(np.float64) for t in leaves])
    return out[0], out[1]


GRAD_TABLE = []               # (what, own, largest ratio, elements, left out) of every check_gradient call, for the printed table


def check_gradient(got, r32, r64, what, owned=None, near=None, K=8.0, own=None, block_axis0=False, min_max=None, min_share=None,
                   signed_zero_ok=False):
    """A kernel's gradient against the float64 autograd of the restatement, element by element:

        s_i = |r64_i| + 1e-3 max|r64|        (the max over the tensor; with block_axis0 over the element's slice along axis 0)
        own = max(2^-20, max_i |r32_i - r64_i| / s_i)          (how much rounding noise the formula itself carries; may be given)
        |got_i - r64_i| <= K own s_i

    owned: the cells some object owns; every other cell must be exactly 0 (bit for bit: +0, unless signed_zero_ok).  near: cells at the clamp's boundary, left out
    (at most 0.1 % of the owned ones).  min_max / min_share: the float64 gradient itself must be worth checking (largest magnitude;
    share of the owned cells above 1e-6 of it).  Prints and records own and the largest observed ratio."""
    got, r32, r64 = (np.asarray(x, np.float64) for x in (got, r32, r64))
    assert got.shape == r32.shape == r64.shape, (what, got.shape, r32.shape, r64.shape)
    assert np.all(np.isfinite(got)), "%s: %d non-finite values" % (what, int((~np.isfinite(got)).sum()))
    assert np.all(np.isfinite(r64)) and np.all(np.isfinite(r32)), what
    owned = np.ones(got.shape, bool) if owned is None else np.asarray(owned, bool)
    if not owned.all():
        stray = got[~owned]
        assert not stray.any() and (signed_zero_ok or not np.signbit(stray).any()), "%s: %d cells nobody owns are not +0" % (what, int((stray != 0).sum()))
        assert not r64[~owned].any(), what + ": the reference has a gradient in a cell nobody owns"
    if min_max is not None:
        top = np.abs(r64).max() if r64.size else 0.0
        assert top >= min_max, "%s: the float64 gradient is at most %.3g: nothing to check" % (what, top)
        share = (np.abs(r64[owned]) > 1e-6 * top).mean()
        assert share >= min_share, "%s: only %.3g of the owned cells carry a gradient" % (what, share)
    keep = owned.copy()
    left_out = 0
    if near is not None:
        near = np.asarray(near, bool) & owned
        left_out = int(near.sum())
        assert left_out <= 1e-3 * owned.sum(), "%s: %d of %d cells at the clamp's boundary" % (what, left_out, int(owned.sum()))
        keep &= ~near
    if block_axis0 and r64.ndim > 1:
        top = np.abs(r64).reshape(r64.shape[0], -1).max(1).reshape((-1,) + (1,) * (r64.ndim - 1))
    else:
        top = np.abs(r64).max() if r64.size else 0.0
    s = np.abs(r64) + 1e-3 * top + GRAD_TINY
    measured = float((np.abs(r32 - r64) / s)[keep].max()) if keep.any() else 0.0
    own = max(GRAD_FLOOR, measured if own is None else own)
    ratio = float((np.abs(got - r64) / s)[keep].max()) if keep.any() else 0.0
    GRAD_TABLE.append((what, own, ratio, int(keep.sum()), left_out))
    print("  %-78s own %.3g  ratio %.3g (%.3g of the bound)  n %d  left out %d" % (what, own, ratio, ratio / (K * own), int(keep.sum()), left_out))
    if ratio > K * own:
        bad = np.unravel_index(np.argmax(np.where(keep, np.abs(got - r64) / s, 0)), got.shape)
        raise AssertionError("%s: |g - r64| / s = %.3g > %g * own (%.3g) at %s: got %.9g, r64 %.9g, r32 %.9g"
                             % (what, ratio, K, own, bad, got[bad], r64[bad], r32[bad]))
    return own, ratio
