"""Autograd-aware front of the C-ABI wrappers.

Every function here has the signature of its namesake in `_lib`.  Under `torch.no_grad()` (inference) the call
goes straight to the kernel; when a floating-point input requires grad, the core entry points (filter, relate, quantify,
linear_act) go through the registered PyTorch operators `torch.ops.dfol.*` (torch_ops.py: custom_op + register_autograd +
register_fake), the small glue through a `torch.autograd.Function`; either way the backward launches the HIP backward
kernels (`csrc/dfol_logic_bwd.hip`).  The backward of the tiny per-question
vector glue (gate, segment reductions, and/or/not, compare) and of the dense layers is written with torch tensor ops /
library GEMMs on the GPU — plumbing, as the design notes say.
"""

import os

import torch

from . import _lib
from . import torch_ops  # noqa: F401  (registers torch.ops.dfol.*)
from ._lib import *  # noqa: F401,F403  (constants, DfolError, non-differentiable wrappers)
from ._lib import DfolError  # noqa: F401

_EPS = 1e-20


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _dpnot(x, alpha):
    """d/dx log(max(alpha + (1 - 2 alpha) e^x, eps)); zero where the clamp is active."""
    e = torch.exp(x)
    d = alpha + (1 - 2 * alpha) * e
    return torch.where(d > _EPS, (1 - 2 * alpha) * e / d.clamp_min(_EPS), torch.zeros_like(d))


# ---- filter ------------------------------------------------------------------------------------------
def filter_fwd(att_in, ll, pred_q, n_obj, neg=None, active=None):
    if _needs_grad(att_in, ll):
        return torch.ops.dfol.filter_fwd(att_in, ll, pred_q, n_obj, neg, active)
    return _lib.filter_fwd(att_in, ll, pred_q, n_obj, neg, active)


# ---- relate ------------------------------------------------------------------------------------------
def relate_fwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, neg=None, active=None, want=None,
               orientation=_lib.TILE_SUBJECT_ROWS, lone_forall_identity=False, need_s=True, need_o=True, diag_absent=False):
    if _needs_grad(prior_s, prior_o, tile):
        return torch.ops.dfol.relate_fwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, neg, active, want, int(orientation),
                                         bool(lone_forall_identity), bool(diag_absent))
    return _lib.relate_fwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, neg, active, want, orientation, lone_forall_identity,
                           need_s, need_o, diag_absent)


class _RelateKeep(torch.autograd.Function):
    """The one posterior an ungated relate hop keeps, forward and backward in one launch each (DFOL_RELATE_TRAIN=1): only the inputs are saved,
    the aggregate is recomputed by the backward."""

    @staticmethod
    def forward(ctx, x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, active, lone):
        ctx.save_for_backward(x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, active)
        ctx.lone, ctx.identity = lone, _lib.is_identity_map(pred_q, prev.shape[0])
        return _lib.relate_keep_fwd(x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, active, lone)

    @staticmethod
    def backward(ctx, g):
        x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, active = ctx.saved_tensors
        g_x, g_prev, g_tile = _lib.relate_keep_bwd(g.contiguous(), x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, active, ctx.lone,
                                                   identity=ctx.identity)
        return (g_x if ctx.needs_input_grad[0] else None), (g_prev if ctx.needs_input_grad[1] else None), \
            (g_tile if ctx.needs_input_grad[2] else None), None, None, None, None, None, None, None


def relate_keep(x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, neg=None, active=None, lone_forall_identity=False):
    """The posterior GQARelateBatch keeps, on the train step's subject-row tile: x [P, NS] the selected variable, prev [Q, NS] the incoming
    one, x_is_subject uint8 [P] (which axis x is on; the other is summed out)."""
    if _needs_grad(x, prev, tile):
        return _RelateKeep.apply(x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, active, bool(lone_forall_identity))
    return _lib.relate_keep_fwd(x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, active, lone_forall_identity)


# ---- the cell with the trainable gate (csrc/dfol_logic_gate.hip) -------------------------------------
def _gate_grads(g_gate, ctx, at):
    return (g_gate[:12].view(6, 2) if ctx.needs_input_grad[at] else None), (g_gate[12:] if ctx.needs_input_grad[at + 1] else None)


class _FilterGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, att_in, ll, weight, bias, pred_q, n_obj, neg, active):
        gate = _lib.gate_params(weight, bias)
        ctx.save_for_backward(att_in, ll, pred_q, n_obj, gate, neg, active)
        return _lib.filter_gate_fwd(att_in, ll, pred_q, n_obj, gate, neg, active)

    @staticmethod
    def backward(ctx, g):
        att_in, ll, pred_q, n_obj, gate, neg, active = ctx.saved_tensors
        g_prior, g_ll, g_gate = _lib.filter_gate_bwd(g.contiguous(), att_in, ll, pred_q, n_obj, gate, neg, active)
        return (g_prior if ctx.needs_input_grad[0] else None), (g_ll if ctx.needs_input_grad[1] else None), \
            *_gate_grads(g_gate, ctx, 2), None, None, None, None


def filter_gate_fwd(att_in, ll, pred_q, n_obj, weight, bias, neg=None, active=None):
    """filter_fwd of a cell with trainable_gate: weight [6, 2] / bias [6] of the gate of axis 0 (NeuralLogicGate._linear)."""
    if _needs_grad(att_in, ll, weight, bias):
        return _FilterGate.apply(att_in, ll, weight, bias, pred_q, n_obj, neg, active)
    return _lib.filter_gate_fwd(att_in, ll, pred_q, n_obj, _lib.gate_params(weight, bias), neg, active)


class _RelateGate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prior_s, prior_o, tile, w_s, b_s, w_o, b_o, pred_q, n_obj, quant_s, quant_o, neg, active, want, orientation, lone, diag_absent):
        gate_s, gate_o = _lib.gate_params(w_s, b_s), _lib.gate_params(w_o, b_o)
        ctx.save_for_backward(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, gate_s, gate_o, neg, active, want)
        ctx.orientation, ctx.lone = orientation, lone
        return _lib.relate_gate_fwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, gate_s, gate_o, neg, active, want, orientation, lone,
                                    diag_absent=diag_absent)

    @staticmethod
    def backward(ctx, gs, go):
        prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, gate_s, gate_o, neg, active, want = ctx.saved_tensors
        gs, go = gs.contiguous(), go.contiguous()
        if want is not None:                                     # a posterior the forward did not produce carries no gradient
            gs = gs * ((want & 1) > 0).to(gs.dtype).unsqueeze(1)
            go = go * ((want & 2) > 0).to(go.dtype).unsqueeze(1)
        g_ps, g_po, g_tile, gg_s, gg_o = _lib.relate_gate_bwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, gate_s, gate_o, neg, active,
                                                              gs, go, ctx.orientation, ctx.lone)
        return (g_ps if ctx.needs_input_grad[0] else None), (g_po if ctx.needs_input_grad[1] else None), \
            (g_tile if ctx.needs_input_grad[2] else None), *_gate_grads(gg_s, ctx, 3), *_gate_grads(gg_o, ctx, 5), \
            None, None, None, None, None, None, None, None, None, None


def relate_gate_fwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, w_s, b_s, w_o, b_o, neg=None, active=None, want=None,
                    orientation=_lib.TILE_SUBJECT_ROWS, lone_forall_identity=False, need_s=True, need_o=True, diag_absent=False):
    """relate_fwd of a cell with trainable_gate: (w_s, b_s) the gate of axis 0 (joins the subject prior), (w_o, b_o) of axis 1."""
    if _needs_grad(prior_s, prior_o, tile, w_s, b_s, w_o, b_o):
        return _RelateGate.apply(prior_s, prior_o, tile, w_s, b_s, w_o, b_o, pred_q, n_obj, quant_s, quant_o, neg, active, want, int(orientation),
                                 bool(lone_forall_identity), bool(diag_absent))
    return _lib.relate_gate_fwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, _lib.gate_params(w_s, b_s), _lib.gate_params(w_o, b_o),
                                neg, active, want, orientation, lone_forall_identity, need_s, need_o, diag_absent)


class _RelateKeepGate(torch.autograd.Function):
    """The one posterior a relate hop keeps, forward and backward in one launch each (DFOL_GATE_TRAIN=1): the inputs and the packed gates are
    saved, the aggregate is recomputed by the backward."""

    @staticmethod
    def forward(ctx, x, prev, tile, w_s, b_s, w_o, b_o, pred_q, n_obj, quant_prev, x_is_subject, neg, active, lone):
        gate_s, gate_o = _lib.gate_params(w_s, b_s), _lib.gate_params(w_o, b_o)
        ctx.save_for_backward(x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, gate_s, gate_o, neg, active)
        ctx.lone, ctx.identity = lone, _lib.is_identity_map(pred_q, prev.shape[0])
        return _lib.relate_keep_gate_fwd(x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, gate_s, gate_o, neg, active, lone)

    @staticmethod
    def backward(ctx, g):
        x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, gate_s, gate_o, neg, active = ctx.saved_tensors
        g_x, g_prev, g_tile, gg_s, gg_o = _lib.relate_keep_gate_bwd(g.contiguous(), x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, gate_s,
                                                                    gate_o, neg, active, ctx.lone, identity=ctx.identity)
        return (g_x if ctx.needs_input_grad[0] else None), (g_prev if ctx.needs_input_grad[1] else None), \
            (g_tile if ctx.needs_input_grad[2] else None), *_gate_grads(gg_s, ctx, 3), *_gate_grads(gg_o, ctx, 5), \
            None, None, None, None, None, None, None


def relate_keep_gate(x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, w_s, b_s, w_o, b_o, neg=None, active=None, lone_forall_identity=False):
    """The posterior GQARelateBatch keeps, from a cell with trainable_gate, on the train step's subject-row tile: x [P, NS] the selected
    variable, prev [Q, NS] the incoming one, x_is_subject uint8 [P]; (w_s, b_s) the gate of axis 0, (w_o, b_o) of axis 1."""
    if _needs_grad(x, prev, tile, w_s, b_s, w_o, b_o):
        return _RelateKeepGate.apply(x, prev, tile, w_s, b_s, w_o, b_o, pred_q, n_obj, quant_prev, x_is_subject, neg, active,
                                     bool(lone_forall_identity))
    return _lib.relate_keep_gate_fwd(x, prev, tile, pred_q, n_obj, quant_prev, x_is_subject, _lib.gate_params(w_s, b_s), _lib.gate_params(w_o, b_o),
                                     neg, active, lone_forall_identity)


# ---- quantify ----------------------------------------------------------------------------------------
def quantify_fwd(att, quant, pred_q, n_obj):
    if _needs_grad(att):
        return torch.ops.dfol.quantify_fwd(att, quant, pred_q, n_obj)
    return _lib.quantify_fwd(att, quant, pred_q, n_obj)


def quantify_hard(att, quant, pred_q, n_obj, total_obj):
    """hard_mode aggregation; the reference only uses it when answering (give_answer and hard_mode), so it carries no gradient."""
    return _lib.quantify_hard(att.detach(), quant, pred_q, n_obj, total_obj)


# ---- gathers and option normalisation ----------------------------------------------------------------
class _AttrGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, obj_off, pred_q, pred_col, NS, default_ll):
        ctx.save_for_backward(obj_off, pred_q, pred_col)
        ctx.shape = tuple(table.shape)
        return _lib.attr_gather(table, obj_off, pred_q, pred_col, NS, default_ll)

    @staticmethod
    def backward(ctx, g):
        obj_off, pred_q, pred_col = ctx.saved_tensors
        return _lib.attr_gather_bwd(g.contiguous(), obj_off, pred_q, pred_col, ctx.shape), None, None, None, None, None


def attr_gather(table, obj_off, pred_q, pred_col, NS, default_ll=-30.0):
    if _needs_grad(table):
        return _AttrGather.apply(table.contiguous(), obj_off, pred_q, pred_col, NS, default_ll)
    return _lib.attr_gather(table, obj_off, pred_q, pred_col, NS, default_ll)


class _RelGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, pair_off, n_obj, pred_q, pred_col, NS, orientation, default_ll):
        ctx.save_for_backward(pair_off, n_obj, pred_q, pred_col)
        ctx.meta = (tuple(table.shape), orientation)
        return _lib.rel_gather(table, pair_off, n_obj, pred_q, pred_col, NS, orientation, default_ll)

    @staticmethod
    def backward(ctx, g):
        pair_off, n_obj, pred_q, pred_col = ctx.saved_tensors
        shape, orientation = ctx.meta
        return _lib.rel_gather_bwd(g.contiguous(), pair_off, n_obj, pred_q, pred_col, orientation, shape), None, None, None, None, None, None, None


def rel_gather(table, pair_off, n_obj, pred_q, pred_col, NS, orientation=_lib.TILE_SUBJECT_ROWS, default_ll=-30.0):
    if _needs_grad(table):
        return _RelGather.apply(table.contiguous(), pair_off, n_obj, pred_q, pred_col, NS, orientation, default_ll)
    return _lib.rel_gather(table, pair_off, n_obj, pred_q, pred_col, NS, orientation, default_ll)


class _OptionNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ll, seg_off, pred_q, n_obj, NS):
        y = _lib.option_normalize_(ll.clone(), seg_off, pred_q, n_obj, NS)
        ctx.save_for_backward(y, seg_off, pred_q, n_obj)
        ctx.NS = NS
        return y

    @staticmethod
    def backward(ctx, g):
        y, seg_off, pred_q, n_obj = ctx.saved_tensors
        return _lib.option_normalize_bwd(g.contiguous(), y, seg_off, pred_q, n_obj, ctx.NS), None, None, None, None


def option_normalize_(ll, seg_off, pred_q, n_obj, NS):
    """In place for inference; under autograd the normalised copy is returned (callers use the return value)."""
    if _needs_grad(ll):
        return _OptionNormalize.apply(ll, seg_off, pred_q, n_obj, NS)
    return _lib.option_normalize_(ll, seg_off, pred_q, n_obj, NS)


# ---- small per-question glue: forward = HIP kernel, backward = a few tensor ops ----------------------
class _Gate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_att, y_att, x_quant, y_quant, g):
        ctx.save_for_backward(g)
        att, quant = _lib.gate(x_att, y_att, x_quant, y_quant, g)
        ctx.mark_non_differentiable(quant)
        return att, quant

    @staticmethod
    def backward(ctx, g_att, _g_quant):
        (g,) = ctx.saved_tensors
        sel = (g > 0).unsqueeze(1)
        zero = torch.zeros_like(g_att)
        return torch.where(sel, g_att, zero), torch.where(sel, zero, g_att), None, None, None


def gate(x_att, y_att, x_quant, y_quant, g):
    if _needs_grad(x_att, y_att):
        return _Gate.apply(x_att, y_att, x_quant, y_quant, g)
    return _lib.gate(x_att, y_att, x_quant, y_quant, g)


class _SegmentSumRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, seg_off):
        ctx.save_for_backward(seg_off)
        ctx.P = src.shape[0]
        return _lib.segment_sum_rows(src, seg_off)

    @staticmethod
    def backward(ctx, g):
        (seg_off,) = ctx.saved_tensors
        counts = (seg_off[1:] - seg_off[:-1]).to(torch.int64)
        idx = torch.repeat_interleave(torch.arange(counts.numel(), device=g.device), counts).to(torch.int32)
        return _lib.gather_rows(g.contiguous(), idx), None


def segment_sum_rows(src, seg_off):
    if _needs_grad(src):
        return _SegmentSumRows.apply(src, seg_off)
    return _lib.segment_sum_rows(src, seg_off)


class _SegmentOr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, seg_off, as_written=False):
        ctx.save_for_backward(lp, seg_off)
        return _lib.segment_or(lp, seg_off, as_written)

    @staticmethod
    def backward(ctx, g):
        lp, seg_off = ctx.saved_tensors
        counts = (seg_off[1:] - seg_off[:-1]).to(torch.int64)
        idx = torch.repeat_interleave(torch.arange(counts.numel(), device=g.device), counts)
        one = torch.ones((), device=lp.device)
        inner = torch.log((1 - torch.exp(lp)).clamp_min(_EPS))
        s = _lib.segment_sum_rows(inner.unsqueeze(1).contiguous(), seg_off).squeeze(1)     # (index_add_ would be atomic: not repeatable)
        return (g * _dpnot(s, one))[idx] * _dpnot(lp, one), None, None


def segment_or(lp, seg_off, as_written=False):
    if _needs_grad(lp):
        return _SegmentOr.apply(lp, seg_off, as_written)
    return _lib.segment_or(lp, seg_off, as_written)


class _Implication(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prior, x, pred_q, n_obj):
        ctx.save_for_backward(prior, x, pred_q, n_obj)
        return _lib.implication(prior, x, pred_q, n_obj)

    @staticmethod
    def backward(ctx, g):
        prior, x, pred_q, n_obj = ctx.saved_tensors
        one = torch.ones((), device=x.device)
        pq = pred_q.to(torch.int64)
        valid = torch.arange(x.shape[1], device=x.device).unsqueeze(0) < n_obj.to(torch.int64)[pq].unsqueeze(1)
        m = torch.log((1 - torch.exp(x)).clamp_min(_EPS))
        z = prior[pq] + m
        dz = torch.where(valid, g * _dpnot(z, one), torch.zeros_like(g))
        g_prior = _lib.reduce_by_question(dz.contiguous(), pred_q, None, prior.shape[0])    # deterministic (no atomics)
        return g_prior, dz * _dpnot(x, one), None, None


def implication(prior, x, pred_q, n_obj):
    if _needs_grad(prior, x):
        return _Implication.apply(prior, x, pred_q, n_obj)
    return _lib.implication(prior, x, pred_q, n_obj)


class _Logic(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op, a, b):
        ctx.op = op
        ctx.save_for_backward(a, b if b is not None else a.new_empty(0))
        return _lib.logic(op, a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        if ctx.op == _lib.LOGIC_AND:
            return None, g, g
        one = torch.ones((), device=a.device)
        if ctx.op == _lib.LOGIC_NOT:
            return None, g * _dpnot(a, one), None
        ea, eb = torch.exp(a), torch.exp(b)
        x = 1 - (1 - ea) * (1 - eb)
        live = x > _EPS
        xs = x.clamp_min(_EPS)
        zero = torch.zeros_like(g)
        return None, torch.where(live, g * ea * (1 - eb) / xs, zero), torch.where(live, g * eb * (1 - ea) / xs, zero)


def logic(op, a, b=None):
    if _needs_grad(a, b):
        return _Logic.apply(op, a, b)
    return _lib.logic(op, a, b)


class _Compare(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp1, lp2, is_less):
        ctx.save_for_backward(lp1, lp2, is_less)
        return _lib.compare(lp1, lp2, is_less)

    @staticmethod
    def backward(ctx, g):
        lp1, lp2, is_less = ctx.saved_tensors
        st = torch.stack([lp1, lp2], 1)
        ls = torch.log_softmax(st, 1)
        gl = g * _dpnot(ls, is_less.unsqueeze(1))
        gst = gl - torch.exp(ls) * gl.sum(1, keepdim=True)
        return gst[:, 0], gst[:, 1], None


def compare(lp1, lp2, is_less):
    if _needs_grad(lp1, lp2):
        return _Compare.apply(lp1, lp2, is_less)
    return _lib.compare(lp1, lp2, is_less)


# ---- dense layers: forward = fused MFMA kernel, backward = the same kernels + the TN weight-gradient kernel ------
def linear_act(x, weight, bias, act, out=None):
    if out is None and _needs_grad(x, weight, bias):
        return torch.ops.dfol.linear_act(x, weight, bias, int(act))
    return _lib.linear_act(x, weight, bias, act, out)


# ---- scene-graph supervision: weighted BCE of all concept columns (operator `scene`; trainer.py:235-256, :265-275) -----------------------
SCENE_BCE_ROUTE = os.environ.get("DFOL_SCENE_BCE", "hip")     # "torch": the tensor-op route on the GPU too (A/B runs, tools/bench_scene.py)
_SCENE_COLS_CHECKED = {}


def _scene_cols_checked(cols, n_rows):
    """cols names every embedding row at most once and none beyond the layer: the backward adds its compact rows into the layer's gradient with
    index_add_, which is ordered only without repeats, and the kernels clamp a row index instead of faulting.  Checked once per index tensor
    and content version (it is a registered buffer or a cached upload); the entry dies with the tensor, so a reused address is checked again.
    (A direct call of torch.ops.dfol.scene_bce is the caller's own: this front is where the check lives.)"""
    import weakref
    key = id(cols)
    hit = _SCENE_COLS_CHECKED.get(key)
    if hit is not None and hit[0]() is cols and hit[1] == (cols._version, n_rows):
        return
    if cols.numel():
        if torch.unique(cols).numel() != cols.numel():
            raise DfolError("scene_bce: cols repeats a row of the embedding layer")
        lo, hi = int(cols.min()), int(cols.max())
        if lo < 0 or hi >= n_rows:
            raise DfolError("scene_bce: cols names rows %d .. %d of an embedding layer of %d rows" % (lo, hi, n_rows))
    _SCENE_COLS_CHECKED[key] = (weakref.ref(cols, lambda _, k=key: _SCENE_COLS_CHECKED.pop(k, None)), (cols._version, n_rows))


def scene_bce_reference(h, emb_w, emb_b, cols, target, weight, thr):
    """The reference's expressions in tensor ops, in the dtype of h (classifier_oracle.py:139-143, trainer.py:235-256, :265-275): the route of CPU
    tensors and of sizes the kernels decline; tests run it in float64."""
    idx = cols.to(torch.int64)
    z = h @ emb_w[idx].t()
    if emb_b is not None:
        z = z + emb_b[idx]
    lp = torch.nn.functional.logsigmoid(z)
    loss = torch.nn.functional.binary_cross_entropy(lp.exp(), target, weight=weight, reduction="sum")
    with torch.no_grad():
        a = (lp > thr).to(target.dtype)
        either = ((target + a) > 0).to(target.dtype)
        num = (weight * either * (target != a).to(target.dtype)).sum()
        den = (weight * either).sum()
    return loss, num, den


def scene_bce(h, emb_w, emb_b, cols, target, weight, thr):
    """(loss, num, den) of the scene-graph supervision over the rows `cols` of the embedding layer: z = h emb_w[cols]^T + emb_b[cols],
    loss = binary_cross_entropy(exp(logsigmoid(z)), target, weight, 'sum'); num / den = the weighted mismatch count of the metric and its
    denominator at the threshold thr on the log-likelihood.  On the GPU one fused launch (+ an ordered sum) without any [M, C] array; the
    gradient goes to h, emb_w and emb_b through two more.  CPU tensors, and sizes dfol_scene_bce_supported declines, take the tensor-op route."""
    M, H = h.shape
    if not h.is_cuda or SCENE_BCE_ROUTE == "torch" or h.dtype != torch.float32 or not _lib.scene_bce_supported(M, H, cols.numel()):
        _lib.note("scene_bce_torch")
        return scene_bce_reference(h, emb_w, emb_b, cols, target, weight, thr)
    _scene_cols_checked(cols, emb_w.shape[0])
    _lib.note("scene_bce_hip")
    if h.stride(-1) != 1:
        h = h.contiguous()
    target, weight = target.contiguous(), weight.contiguous()
    if _needs_grad(h, emb_w, emb_b):
        s = torch.ops.dfol.scene_bce(h, emb_w, emb_b, cols, target, weight, float(thr))
    else:
        s = _lib.scene_bce_fwd(h, emb_w, emb_b, cols, target, weight, thr)
    return s[0], s[1].detach(), s[2].detach()


def scene_pair_rows_reference(obj, ind_s, ind_o):
    """[obj[s], obj[o], distance, angle, sides] of the listed pairs in tensor ops (batch_gqa_boxfeatures_pipeline.py:225-279, the distance and
    angle of :271-278): the route of CPU tensors and of a batch that was not prepared; its autograd sends the gradient back through index_add_.
    ind_s / ind_o: int64 rows of obj, at least one."""
    D = obj.shape[1]
    s, o = obj.index_select(0, ind_s), obj.index_select(0, ind_o)
    ps, po = s[:, D - 4:], o[:, D - 4:]
    dx = ps[:, 0] + ps[:, 2] / 2.0 - po[:, 0] - po[:, 2] / 2.0
    dy = ps[:, 1] + ps[:, 3] / 2.0 - po[:, 1] - po[:, 3] / 2.0
    dist = torch.sqrt(dx * dx + dy * dy)                                                       # :271-278
    geo = torch.stack([dist, torch.asin(dy / dist.clamp(min=1e-10)), (po[:, 0] - ps[:, 0]).sign(), (po[:, 1] - ps[:, 1]).sign()], 1)
    return torch.cat([s, o, geo], 1).contiguous()


def scene_pair_rows(obj, pair_s, pair_o, csr):
    """The rows [P, 2 D + 4] of the listed pairs of a scene batch: obj [O, D] fp32 (the box in its last four columns), pair_s / pair_o int32 [P]
    rows of obj, csr = (seg_off [O + 1], slot [2 P]) the by-object list of the pairs (data.scene_pair_csr).  On the GPU one launch forward and
    one backward (dfol_scene_pair_rows_f32 / _bwd_f32): the gradient reaches obj without atomics, in the list's order, so two runs give the same
    bits; the four geometry columns send none back (the box columns feed no parameter).  CPU tensors take the tensor-op expression."""
    if pair_s.numel() == 0:
        return obj.new_zeros(0, 2 * obj.shape[1] + 4)
    if not obj.is_cuda or obj.dtype != torch.float32:
        _lib.note("scene_pair_rows_torch")
        return scene_pair_rows_reference(obj, pair_s.to(torch.int64), pair_o.to(torch.int64))
    _lib.note("scene_pair_rows_hip")
    if obj.stride(-1) != 1:
        obj = obj.contiguous()
    if _needs_grad(obj):
        seg_off, slot = csr
        return torch.ops.dfol.scene_pair_rows(obj, pair_s, pair_o, seg_off, slot)
    return _lib.scene_pair_rows(obj, pair_s, pair_o)


class _PairFeatures(torch.autograd.Function):
    """[obj_s, obj_o, geometry]: the gradient flows back to the two object rows (the geometry comes from the raw boxes).  Only the
    full-table compatibility dataflow (`_needed_columns = False`) builds the [pairs, 1036] matrix; its backward is torch's atomic
    index_add_ - the one place the deterministic-backward guarantee does not cover."""

    @staticmethod
    def forward(ctx, obj, D, obj_off, pair_off, Q, max_n, pairs, ind_s, ind_o):
        ctx.save_for_backward(ind_s, ind_o)
        ctx.meta = (tuple(obj.shape), D)
        return _lib.pair_features(obj, D, obj_off, pair_off, Q, max_n, pairs)

    @staticmethod
    def backward(ctx, g):
        ind_s, ind_o = ctx.saved_tensors
        shape, D = ctx.meta
        g_obj = torch.zeros(shape, dtype=g.dtype, device=g.device)
        g_obj[:, :D].index_add_(0, ind_s, g[:, :D])
        g_obj[:, :D].index_add_(0, ind_o, g[:, D:2 * D])
        return g_obj, None, None, None, None, None, None, None, None


class _PairFeaturesOrdered(torch.autograd.Function):
    """The same forward with the backward of csrc/dfol_dropout.hip: no atomics, one fixed summation order.  The dropout route's: there the pair
    matrix is the training route's heaviest backward, and its steps must repeat bit for bit."""

    @staticmethod
    def forward(ctx, obj, D, obj_off, pair_off, Q, max_n, pairs):
        ctx.save_for_backward(obj_off, pair_off)
        ctx.meta = (tuple(obj.shape), D, Q, max_n)
        return _lib.pair_features(obj, D, obj_off, pair_off, Q, max_n, pairs)

    @staticmethod
    def backward(ctx, g):
        obj_off, pair_off = ctx.saved_tensors
        shape, D, Q, max_n = ctx.meta
        if g.stride(1) != 1:
            g = g.contiguous()
        g_obj = _lib.pair_features_bwd(g, D, obj_off, pair_off, Q, max_n, shape[0])
        if shape[1] != D:                                   # (an object matrix wider than the D columns the pairs read)
            wide = torch.zeros(shape, dtype=g.dtype, device=g.device)
            wide[:, :D] = g_obj
            g_obj = wide
        return g_obj, None, None, None, None, None, None


def pair_features(obj, D, obj_off, pair_off, Q, max_n, pairs, pair_index=None, ordered=False):
    """ordered=True: the backward without atomics (dfol_pair_features_bwd_f32) instead of index_add_ - the dropout route asks for it; the
    dropout-0 full-table route keeps index_add_ and its bits."""
    if _needs_grad(obj):
        if ordered:
            _lib.note("pair_features_bwd_ordered")
            return _PairFeaturesOrdered.apply(obj, D, obj_off, pair_off, Q, max_n, pairs)
        ind_s, ind_o = pair_index()
        return _PairFeatures.apply(obj, D, obj_off, pair_off, Q, max_n, pairs, ind_s, ind_o)
    return _lib.pair_features(obj, D, obj_off, pair_off, Q, max_n, pairs)


class _Dropout(torch.autograd.Function):
    """y = x * mask / (1 - p) by dfol_dropout_f32.  Nothing of the mask is saved but the 8 bytes of the key it was drawn under and the site
    number: the backward runs the same kernel over the incoming gradient, also after a later forward has advanced the step."""

    @staticmethod
    def forward(ctx, x, p, key, site):
        ctx.save_for_backward(key)
        ctx.meta = (p, site)
        return _lib.dropout(x, p, key, site)

    @staticmethod
    def backward(ctx, g):
        (key,) = ctx.saved_tensors
        p, site = ctx.meta
        if g.shape[1] > 1 and g.stride(1) != 1:
            g = g.contiguous()
        return _lib.dropout(g, p, key, site), None, None, None


def dropout(x, p):
    """nn.Dropout(p) in training mode on a matrix [rows, cols] (any row stride): the next site of this forward under the device's current key
    (csrc/dfol_dropout.hip; _lib.dropout_next_site).  p = 0 returns x without a launch."""
    if p <= 0:
        return x
    if not 0 < p < 1:
        raise DfolError("dropout: p = %r is not in [0, 1)" % (p,))
    if not x.is_cuda:
        raise DfolError("the HIP path needs tensors on the GPU (got a %s tensor); there is no CPU fallback" % x.device)
    site = _lib.dropout_next_site(x.device)
    key = _lib.dropout_key(x.device)
    if _needs_grad(x):
        return _Dropout.apply(x, float(p), key.clone(), site)      # (its own copy of the key: a backward after a later forward keeps its mask)
    return _lib.dropout(x, float(p), key, site)


def _modulate_reference(att, mods, valid):
    """apply_modulations (batch_base_types.py:170-179) in tensor ops; used for the backward of the HIP kernel."""
    alpha, beta, c, d = (mods[:, k].unsqueeze(1) * (10.0 if k < 3 else 1.0) for k in range(4))
    slog = lambda x: torch.log(x.clamp_min(_EPS))
    t = alpha * att + slog(c) + slog(d)
    u = beta * slog(1 - torch.exp(att)) + slog(1 - d)
    return torch.where(valid, t - slog(torch.exp(u) + torch.exp(t)), torch.zeros_like(att))


class _Modulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, att, mods, pred_q, n_obj):
        ctx.save_for_backward(att, mods, pred_q, n_obj)
        return _lib.modulate(att, mods.contiguous(), pred_q, n_obj)

    @staticmethod
    def backward(ctx, g):
        att, mods, pred_q, n_obj = ctx.saved_tensors
        if os.environ.get("DFOL_MODULATE_BWD", "hip") == "torch":      # A/B: autograd through the tensor-op restatement (~70 launches)
            valid = torch.arange(att.shape[1], device=att.device).unsqueeze(0) < n_obj.to(torch.int64)[pred_q.to(torch.int64)].unsqueeze(1)
            with torch.enable_grad():
                a = att.detach().requires_grad_(True)
                m = mods.detach().requires_grad_(True)
                out = _modulate_reference(a, m, valid)
                ga, gm = torch.autograd.grad(out, (a, m), g, allow_unused=True)
            return ga, gm, None, None
        ga, gm = _lib.modulate_bwd(g.contiguous(), att.contiguous(), mods.contiguous(), pred_q, n_obj)      # one launch, deterministic
        return ga, gm, None, None


def modulate(att, mods, pred_q, n_obj):
    if _needs_grad(att, mods):
        return _Modulate.apply(att, mods, pred_q, n_obj)
    return _lib.modulate(att, mods.contiguous(), pred_q, n_obj)
