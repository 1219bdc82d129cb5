"""The logic cell with the trainable gate, restated in torch from the block formulas, float32 / float64 parametric.

Pinned against the reference's own gated cell (golden family g25_gate_cell, tests/test_trainable_gate_cpu.py); after that it is the
per-element reference of the GPU tests, as golden_util.t_relate / t_filter are for the ungated cell."""

import numpy as np
import torch

from golden_util import EPS, NEAR_FLOOR, t_pnot, t_prep, t_slog


def t_gate_parts(a, b, W, c):
    """-> (va_raw, vb_raw, m_raw) of G(a, b) = log(max(m_raw, eps)); a, b broadcast against each other, W [6, 2], c [6]."""
    a, b = torch.broadcast_tensors(a, b)
    al = torch.sigmoid(a[..., None] * W[:, 0] + b[..., None] * W[:, 1] + c)
    va = al[..., 0] + al[..., 3] * (1 - 2 * al[..., 0]) * torch.exp(a)
    vb = al[..., 1] + al[..., 4] * (1 - 2 * al[..., 1]) * torch.exp(b)
    m = al[..., 2] + al[..., 5] * (1 - 2 * al[..., 2]) * va.clamp_min(EPS) * vb.clamp_min(EPS)
    return va, vb, m


def t_gate(a, b, W, c, near=None):
    """near (a list) receives the mask of elements with one of the three clamp arguments at the clamp's boundary."""
    va, vb, m = t_gate_parts(a, b, W, c)
    if near is not None:
        hit = torch.zeros(m.shape, dtype=torch.bool)
        for x in (va, vb, m):
            x = x.detach()
            hit |= (x > EPS * (1 - NEAR_FLOOR)) & (x < EPS * (1 + NEAR_FLOOR))
        near.append(hit)
    return t_slog(m)


def t_filter_gate(prior, ll, neg, any_neg, W, c, near=None):
    """prior, ll [n] -> [n]."""
    return t_gate(t_prep(ll, neg, any_neg), prior, W, c, near)


def t_relate_gate(a, b, l, qs, qo, neg, any_neg, Ws, cs, Wo, co, lone_forall_identity=False, near=None):
    """a, b [n] the subject / object priors, l [n, n] the raw tile (subjects along rows); (Ws, cs) the gate of axis 0, (Wo, co) of axis 1.
    near (a dict) receives 's' / 'o' masks: outputs that a clamp boundary of some gate reaches."""
    n = a.shape[0]
    qs, qo = float(qs), float(qo)
    v = t_prep(l, neg, any_neg)
    off = 1 - torch.eye(n, dtype=l.dtype)
    id_s, id_o = lone_forall_identity and qs == 0, lone_forall_identity and qo == 0
    F_s = (lambda x: x) if id_s else (lambda x: t_pnot(x, qs))
    F_o = (lambda x: x) if id_o else (lambda x: t_pnot(x, qo))
    ns, no, outs, outo = [], [], [], []
    S = (F_o(t_gate(v, b[None, :], Wo, co, ns)) * off).sum(1)
    T = (F_s(t_gate(v, a[:, None], Ws, cs, no)) * off).sum(0)
    post_s, post_o = t_gate(F_o(S), a, Ws, cs, outs), t_gate(F_s(T), b, Wo, co, outo)
    if near is not None:
        near["s"] = (ns[0] & off.bool()).any(1) | outs[0]
        near["o"] = (no[0] & off.bool()).any(0) | outo[0]
    return post_s, post_o


# ---- the flat layout of the g25_gate_cell goldens (the reference's: objects of all images concatenated) ------------------------------
def cell_case(arrays, name, arity):
    """One golden case as numpy: its inputs, and per dtype tag the reference's output and gradients."""
    keys = ["prior", "ll", "quant", "img", "pq", "W", "c", "cot"]
    case = {k: arrays["%s_%s" % (name, k)] for k in keys}
    case["neg"] = arrays[name + "_neg"] if (name + "_neg") in arrays.files else None
    for tag in ("f32", "f64"):
        case[tag] = {"out": arrays["%s_out_%s" % (name, tag)], "gprior": arrays["%s_gprior_%s" % (name, tag)],
                     "gll": arrays["%s_gll_%s" % (name, tag)],
                     "gW": np.stack([arrays["%s_gW%d_%s" % (name, k, tag)] for k in range(arity)]),
                     "gc": np.stack([arrays["%s_gc%d_%s" % (name, k, tag)] for k in range(arity)])}
    return case


def restate_cell(case, arity, dtype):
    """The restatement over a flat-layout case: -> (out [P, arity, O], leaves dict) with out's padding (objects of other images) 0."""
    prior = torch.tensor(case["prior"], dtype=dtype, requires_grad=True)
    ll = torch.tensor(case["ll"], dtype=dtype, requires_grad=True)
    W = torch.tensor(case["W"], dtype=dtype, requires_grad=True)
    c = torch.tensor(case["c"], dtype=dtype, requires_grad=True)
    img, pq, quant, neg = case["img"], case["pq"], case["quant"], case["neg"]
    P, O = len(pq), len(img)
    any_neg = neg is not None
    rows = []
    for p in range(P):
        idx = torch.tensor(np.nonzero(img == pq[p])[0])
        ng = float(neg[p]) if any_neg else 0.0
        full = torch.zeros(arity, O, dtype=dtype)
        if arity == 1:
            post = t_filter_gate(prior[pq[p], 0, idx], ll[p, idx, 0], ng, any_neg, W[0], c[0])
            full = full.index_put((torch.zeros_like(idx), idx), post)
        else:
            tile = ll[p][idx][:, idx][:, :, 0]
            ps, po = t_relate_gate(prior[pq[p], 0, idx], prior[pq[p], 1, idx], tile, quant[p, 0], quant[p, 1], ng, any_neg,
                                   W[0], c[0], W[1], c[1], lone_forall_identity=(P == 1))
            full = full.index_put((torch.zeros_like(idx), idx), ps).index_put((torch.ones_like(idx), idx), po)
        rows.append(full)
    return torch.stack(rows), {"prior": prior, "ll": ll, "W": W, "c": c}


def block_case(case, arity, NS=None):
    """The block layout the kernels read, from a flat case: prior [Q, arity, NS], ll [P, NS(, NS)], n_obj [Q], and `place`:
    place(flat [P, arity, O]) -> [P, arity, NS] (an image's objects to the front, padding 0)."""
    img, pq = case["img"], case["pq"]
    Q, P = int(img.max()) + 1, len(pq)
    n = np.bincount(img, minlength=Q)
    NS = NS or int(-(-n.max() // 4) * 4)
    first = np.concatenate([[0], np.cumsum(n)])
    prior = np.zeros((Q, arity, NS), np.float32)
    for q in range(Q):
        prior[q, :, :n[q]] = case["prior"][q][:, first[q]:first[q] + n[q]]
    ll = np.full((P,) + (NS,) * arity, -30.0, np.float32)
    for p in range(P):
        q = pq[p]
        sl = slice(first[q], first[q] + n[q])
        if arity == 1:
            ll[p, :n[q]] = case["ll"][p, sl, 0]
        else:
            ll[p, :n[q], :n[q]] = case["ll"][p, sl, sl, 0]

    def place(flat):
        out = np.zeros(flat.shape[:-1] + (NS,), flat.dtype)
        for p in range(P):
            q = pq[p]
            out[p, ..., :n[q]] = flat[p, ..., first[q]:first[q] + n[q]]
        return out

    def place_prior(flat):                                    # [Q, arity, O] -> [Q, arity, NS]
        out = np.zeros((Q, arity, NS), flat.dtype)
        for q in range(Q):
            out[q, :, :n[q]] = flat[q][:, first[q]:first[q] + n[q]]
        return out

    def place_ll(flat):                                       # [P, O(, O), 1] -> [P, NS(, NS)]
        out = np.zeros((P,) + (NS,) * arity, flat.dtype)
        for p in range(P):
            q = pq[p]
            sl = slice(first[q], first[q] + n[q])
            if arity == 1:
                out[p, :n[q]] = flat[p, sl, 0]
            else:
                out[p, :n[q], :n[q]] = flat[p, sl, sl, 0]
        return out

    return {"prior": prior, "ll": ll, "n_obj": n.astype(np.int32), "pq": pq.astype(np.int32), "NS": NS, "place": place,
            "place_prior": place_prior, "place_ll": place_ll}
