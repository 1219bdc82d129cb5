"""ctypes binding of the C-ABI library (include/dfol_vqa.h, built from csrc/ by hipcc).

There is no CPU fallback: if `libdfolvqa.so` is missing, or a tensor is not a contiguous CUDA
(ROCm) tensor of the declared dtype, the call raises.
"""

import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DFOL_LIB") or os.path.join(_HERE, "libdfolvqa.so")     # DFOL_LIB: an A/B build (e.g. -DDFOL_PRECISE_MATH)
_lib = None

TILE_SUBJECT_ROWS, TILE_OBJECT_ROWS = 0, 1
WANT_SUBJECT, WANT_OBJECT = 1, 2
RELATE_LONE_FORALL_IDENTITY, RELATE_DIAG_ABSENT = 1, 2
TILE_F32, TILE_BF16 = 0, 1
ACT_NONE, ACT_SIGMOID, ACT_ELU, ACT_LOGSIGMOID = 0, 1, 2, 3
LOGIC_AND, LOGIC_OR, LOGIC_NOT = 0, 1, 2


class DfolError(RuntimeError):
    pass


class LRUCache(object):
    """Bounded content-keyed cache with least-recently-used eviction (round 2's caches dropped EVERYTHING when full: with the token
    diversity of real GQA batches that is a periodic full re-upload through pageable, stream-synchronising copies)."""

    def __init__(self, capacity):
        import collections
        self.capacity = int(capacity)
        self._d = collections.OrderedDict()

    def get(self, key, default=None):
        hit = self._d.get(key)
        if hit is None:
            return default
        self._d.move_to_end(key)
        if _KEEP is not None:                               # a graph capture is recording: whatever a cache hands out may end up in a launch
            _KEEP.append(hit)                               # (of this library or of torch), so the graph keeps it alive - see keep_alive()
        return hit

    def __setitem__(self, key, value):
        self._d[key] = value
        self._d.move_to_end(key)
        if _KEEP is not None:
            _KEEP.append(value)
        while len(self._d) > self.capacity:
            self._d.popitem(last=False)

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        return key in self._d

    def clear(self):
        self._d.clear()


# ---- which route did a step take?  Counters the tests read (and a once-per-route warning when the training dataflow leaves this library's
# kernels for torch / vendor-library operators: a relation network whose widths the fused kernels do not take trains correctly, but not on
# the code this library exists for - round 4's reference gradient golden went through such a route unnoticed) -------------------------------
import collections as _collections
import warnings as _warnings

PATH_COUNTS = _collections.Counter()
_WARNED = set()


def note(route):
    PATH_COUNTS[route] += 1


def fallback(route, why, what="runs on torch / vendor-library operators instead of this library's HIP kernels"):
    """Count a step that left the route it was meant to take and say so once per route.  what: the clause after the route's name, for a step that
    stays on this library's kernels but not on the ones asked for (range_rerun: the same forward again, on the wide-range arithmetic)."""
    PATH_COUNTS["fallback:" + route] += 1
    if route not in _WARNED:
        _WARNED.add(route)
        _warnings.warn("dfol_vqa_amd: %s %s (%s)" % (route, what, why), RuntimeWarning, stacklevel=3)


_p, _i32, _i64, _f = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float

# name -> argtypes, exactly as declared in include/dfol_vqa.h
SIGNATURES = {
    "dfol_attr_gather_f32": [_p, _i64, _p, _p, _p, _i32, _i32, _f, _p, _p],
    "dfol_rel_gather_f32": [_p, _i64, _p, _p, _p, _p, _i32, _i32, _i32, _f, _p, _p],
    "dfol_option_normalize_f32": [_p, _p, _i32, _p, _p, _i32, _i32, _p],
    "dfol_filter_fwd_f32": [_p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _p, _p],
    "dfol_relate_fwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p],
    "dfol_quantify_fwd_f32": [_p, _p, _p, _p, _i32, _i32, _p, _p],
    "dfol_find_max_ind_f32": [_p, _p, _i32, _f, _p, _p],
    "dfol_quantify_hard_f32": [_p, _p, _p, _p, _i32, _i32, _i32, _p, _p],
    "dfol_relate_one_fwd_f32": [_p, _p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p],
    "dfol_gate_f32": [_p, _p, _p, _p, _p, _i32, _i32, _p, _p, _p],
    "dfol_gather_rows_f32": [_p, _p, _i32, _i32, _p, _p],
    "dfol_gather_object_rows_f32": [_p, _p, _p, _p, _p, _i32, _i32, _i32, _p, _i64, _p],
    "dfol_store_round_bf16": [_p, _i64, _p, _p],
    "dfol_gather_object_rows_bf16_f32": [_p, _p, _p, _p, _p, _i32, _i32, _i32, _p, _i64, _p],
    "dfol_store_rows_f32": [_p, _p, _p, _p, _i32, _i32, _i32, _p, _p, _p],
    "dfol_store_objects_f32": [_p, _i64, _p, _p, _i32, _i32, _p, _i64, _p],
    "dfol_segment_sum_rows_f32": [_p, _p, _i32, _i32, _p, _p],
    "dfol_logic_f32": [_i32, _p, _p, _i64, _p, _p],
    "dfol_parametric_not_f32": [_p, _p, _i32, _i32, _p, _p],
    "dfol_segment_or_f32": [_p, _p, _i32, _p, _p],
    "dfol_segment_or_ref_f32": [_p, _p, _i32, _p, _p],
    "dfol_pair_train_fwd_h2_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _p, _i32, _p, _i64, _p, _p, _p, _i32, _i32, _p, _i32, _p, _p, _i64, _p, _p, _i64, _p],
    "dfol_select_rows_f32": [_p, _p, _p, _i32, _i32, _p, _p],
    "dfol_calib_features_f32": [_p, _i32, _p, _i32, _p, _i32, _p, _p],
    "dfol_attention_modulations_f32": [_p, _p, _p, _i64, _p, _i32, _i32, _i32, _p, _p],
    "dfol_implication_f32": [_p, _p, _p, _p, _i32, _i32, _p, _p],
    "dfol_compare_f32": [_p, _p, _p, _i32, _p, _p],
    "dfol_linear_act_f32": [_p, _i64, _p, _i64, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_box_positions_f32": [_p, _i64, _i32, _i32, _p, _i64, _i32, _p],
    "dfol_pair_features_f32": [_p, _i64, _i32, _p, _p, _i32, _i32, _p, _i64, _p],
    "dfol_reduce_by_question_f32": [_p, _p, _p, _i32, _i32, _i32, _p, _p],
    "dfol_filter_bwd_f32": [_p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p, _p],
    "dfol_relate_bwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p],
    "dfol_linear_wgrad_slabs": [_i64, _i32, _i32],          # returns a count, not a status: called directly, not through call()
    "dfol_linear_wgrad_f32": [_p, _i64, _p, _i64, _i64, _i32, _i32, _p, _p, _p],
    "dfol_linear_wgrad_workspace": [_i64, _i32, _i32],      # returns a float count (int64), called directly
    "dfol_linear_wgrad_bias_f32": [_p, _i64, _p, _i64, _i64, _i32, _i32, _p, _p, _p, _p],
    "dfol_attr_ll_bwd_f32": [_p, _p, _i64, _i32, _p, _i64, _p, _p, _p, _p, _i32, _i32, _i32, _p, _p, _i64, _p, _i64, _p, _p],
    "dfol_quantify_bwd_f32": [_p, _p, _p, _p, _p, _i32, _i32, _p, _p],
    "dfol_filter_gate_fwd_f32": [_p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _p, _p, _p],
    "dfol_relate_gate_fwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p],
    "dfol_relate_one_gate_fwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p, _p, _p],
    "dfol_relate_one_gate_fwd_bf16": [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p, _p, _p],
    "dfol_relate_keep_gate_fwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p, _p, _p],
    "dfol_relate_keep_gate_bwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "dfol_relate_keep_fwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p],
    "dfol_relate_keep_bwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p, _p, _p],
    "dfol_filter_gate_bwd_scratch": [_i32, _i32],         # returns a float count (int64), called directly
    "dfol_filter_gate_bwd_f32": [_p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _p, _p, _p, _p, _p, _p],
    "dfol_relate_gate_bwd_f32": [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "dfol_attr_gather_bwd_f32": [_p, _p, _p, _p, _i32, _i32, _i32, _p, _i64, _p],
    "dfol_rel_gather_bwd_f32": [_p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _i64, _p],
    "dfol_option_normalize_bwd_f32": [_p, _p, _p, _i32, _p, _p, _i32, _i32, _p, _p],
    "dfol_modulate_f32": [_p, _p, _p, _p, _i32, _i32, _p, _p],
    "dfol_lstm_cell_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _i64, _p, _i64, _p, _p, _i32, _i32, _p, _p, _p],
    "dfol_lstm_cell_tokens_f32": [_p, _i32, _p, _i32, _p, _p, _i64, _p, _p, _i64, _p, _i64, _p, _p, _i32, _i32, _p, _p, _p],
    "dfol_lstm_pointwise_f32": [_p, _p, _p, _i32, _i32, _p, _p, _p],
    "dfol_lstm_cell_train_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _i64, _p, _i64, _p, _p, _i32, _i32, _p, _p, _p, _p],
    "dfol_lstm_cell_bwd_f32": [_p, _p, _p, _p, _p, _i32, _i32, _p, _p, _p],
    "dfol_lstm_cell_supported": [_i32, _i32],               # returns 0 / 1, not a status: called directly
    "dfol_calib_walk_supported": [_i32, _i32],
    "dfol_modulate_bwd_f32": [_p, _p, _p, _p, _p, _i32, _i32, _p, _p, _p],
    "dfol_attr_ll_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _p, _p, _i32, _i32, _f, _p, _p],
    "dfol_attr_head_h2_f32": [_p, _i64, _i32, _p, _p, _i32, _p, _i64, _p, _p, _i32, _i32, _p, _p, _i32, _i32, _f, _p, _p],
    "dfol_pair_ll_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _i64, _i32, _p, _i32, _p, _i64, _p, _p, _p, _i32, _i32, _p, _p, _p, _i32,
                         _i32, _f, _p, _p],
    "dfol_pair_pack_w2_f32": [_p, _i64, _i32, _i32, _p, _p],
    "dfol_pair_ll_packed_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _p, _i32, _p, _i64, _p, _p, _p, _i32, _i32, _p, _p, _p, _i32, _i32, _f,
                                _i32, _p, _p],
    "dfol_pair_hidden1_fwd_f32": [_p, _i64, _p, _i64, _p, _i64, _p, _p, _p, _p, _i32, _i32, _i32, _p, _p, _p],
    "dfol_pair_hidden1_bwd_f32": [_p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p, _i64, _p, _i64, _p, _p],
    "dfol_pair_hidden1_bwd_recompute_supported": [_i32, _i32],
    "dfol_pair_hidden1_bwd_recompute_f32": [_p, _p, _i64, _p, _i64, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p, _i64, _p, _i64, _p, _p],
    "dfol_pair_logit_fwd_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _i32, _i64, _i64, _p, _p],
    "dfol_pair_logit_bwd_f32": [_p, _p, _i64, _i32, _p, _i64, _p, _i32, _p, _i64, _p, _i64, _p, _p],
    "dfol_pair_logit_bwd_sums_f32": [_p, _p, _i64, _i32, _p, _i64, _p, _i32, _p, _i64, _p, _p, _i64, _p],
    "dfol_linear_tall_supported": [_i64, _i32, _i32],
    "dfol_linear_tall_h2_f32": [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _p, _p, _i64, _p, _i64, _p],
    "dfol_pair_dz_tall_f32": [_p, _i64, _p, _p, _p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p, _p],
    "dfol_pair_dz_tall_multi_f32": [_p, _i64, _p, _i64, _i32, _p, _p, _i64, _i32, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p, _p],
    "dfol_linear_tall_bf16_bf16": [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _p, _p, _i64, _p, _i64, _p],
    "dfol_pair_dz_tall_bf16": [_p, _i64, _p, _p, _p, _i64, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_linear_logit_h2_f32": [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _p, _p, _i64, _p, _i64, _p],
    "dfol_pair_dz_fused_f32": [_p, _i64, _p, _p, _p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_pair_wgrad_fused_workspace": [_i64, _i32, _i32],
    "dfol_pair_wgrad_fused_sums_workspace": [_i64, _i32, _i32, _i32],
    "dfol_pair_wgrad_fused_sums_f32": [_p, _i64, _p, _p, _p, _i32, _p, _i64, _p, _p, _i64, _i64, _i32, _i32, _p, _p, _p, _i64, _p, _p, _p],
    "dfol_pair_wgrad_fused_sums_bf16": [_p, _i64, _p, _p, _p, _i32, _p, _i64, _p, _i64, _i64, _i32, _i32, _p, _p, _p, _i64, _p, _p, _p],
    "dfol_pair_wgrad_fused_f32": [_p, _i64, _p, _p, _p, _p, _i64, _p, _p, _i64, _i64, _i32, _i32, _p, _p, _p],
    "dfol_pair_wgrad_multi_scale_f32": [_p, _i64, _i32, _p, _p, _i32, _i64, _p, _p],
    "dfol_pair_wgrad_fused_multi_f32": [_p, _i64, _p, _i64, _i32, _p, _p, _p, _i64, _i32, _p, _p, _i64, _i64, _i32, _i32, _p, _p, _p],
    "dfol_linear_pack_w_bf16x3": [_p, _i64, _i32, _i32, _p, _p],
    "dfol_linear_act_split_f32": [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_linear_pack_w_bf16": [_p, _i64, _i32, _i32, _p, _p],
    "dfol_linear_act_bf16_f32": [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_linear_wgrad_bias_bf16": [_p, _i64, _p, _i64, _i64, _i32, _i32, _p, _p, _p, _p],
    "dfol_linear_wgrad_rows_supported": [_i32, _i32, _i64, _i64],      # returns 0 / 1, not a status: called directly
    "dfol_linear_wgrad_bias_rows_f32": [_p, _i64, _p, _i64, _p, _i64, _i32, _i32, _p, _p, _p, _p],
    "dfol_linear_wgrad_bias_rows_bf16": [_p, _i64, _p, _i64, _p, _i64, _i32, _i32, _p, _p, _p, _p],
    "dfol_linear_wgrad_rows_bf16t_supported": [_i32, _i32, _i64, _i64],
    "dfol_linear_wgrad_bias_rows_bf16t": [_p, _i64, _p, _i64, _p, _i64, _i32, _i32, _p, _p, _p, _p],
    "dfol_linear_wgrad_rows_bf16t_x3_supported": [_i32, _i32, _i64, _i64],
    "dfol_linear_wgrad_bias_rows_bf16t_x3": [_p, _i64, _p, _i64, _p, _i64, _i32, _i32, _p, _p, _p, _p],
    "dfol_linear_rows_bf16t_supported": [_i32, _i32, _i64],            # returns 0 / 1
    "dfol_linear_act_rows_bf16t_f32": [_p, _i64, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_act_bwd_f32": [_p, _p, _i64, _i32, _p, _p],
    "dfol_linear_act_bf16_bf16": [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_linear_wgrad_bias_bf16_bf16": [_p, _i64, _p, _i64, _i64, _i32, _i32, _p, _p, _p, _p],
    "dfol_pair_hidden1_fwd_bf16": [_p, _i64, _p, _i64, _p, _i64, _p, _p, _p, _p, _i32, _i32, _i32, _p, _p, _p],
    "dfol_pair_hidden1_bwd_bf16": [_p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p, _i64, _p, _i64, _p, _p],
    "dfol_pair_logit_fwd_bf16": [_p, _i64, _i32, _p, _i64, _p, _p, _i32, _i64, _i64, _p, _p],
    "dfol_pair_logit_bwd_bf16": [_p, _p, _i64, _i32, _p, _i64, _p, _i32, _p, _i64, _p, _i64, _p, _p],
    "dfol_pair_pack_w2_bf16x3": [_p, _i64, _i32, _i32, _p, _p],
    "dfol_pair_ll_split_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _p, _i32, _p, _i64, _p, _p, _p, _i32, _i32, _p, _p, _p, _i32, _i32, _f,
                               _i32, _p, _p],
    "dfol_relate_one_fwd_bf16": [_p, _p, _p, _p, _p, _p, _p, _i32, _p, _i32, _i32, _i32, _p, _p],
    "dfol_linear_w_f16x2_bytes": [_i32, _i32],
    "dfol_linear_pack_w_f16x2": [_p, _i64, _i32, _i32, _p, _p],
    "dfol_linear_act_h2_f32": [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_linear_wide_supported": [_i64, _i32, _i32],
    "dfol_concept_rows_f32": [_p, _i64, _p, _p, _p, _i32, _i32, _p, _i64, _i32, _p],
    "dfol_grad_sqnorm_parts": [],
    "dfol_clip_adam_chunk": [],
    "dfol_grad_sqnorm_f32": [_p, _i64, _p, _p],
    "dfol_clip_adam_f32": [_p, _p, _p, _p, _p, _p, _p, _i32, _p, _p, _i32, _p, _f, _f, _f, _f, _f, _f, _f, _p, _p],
    "dfol_linear_wide_h2_f32": [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_linear_wide_rows_h2_f32": [_p, _i64, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_linear_wide_rows_bf16t_supported": [_i64, _i32, _i32, _i64],  # returns 0 / 1
    "dfol_linear_wide_rows_bf16t_h2_f32": [_p, _i64, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _p],
    "dfol_linear_wide_rows_bf16t_f16_h2_f32": [_p, _i64, _p, _p, _p, _p, _i64, _i32, _i32, _i32, _i32, _i32, _p],
    "dfol_store_bf16_is_f16": [_p, _i64, _p, _p],
    "dfol_pair_w2_f16x2_bytes": [_i32],
    "dfol_pair_pack_w2_f16x2": [_p, _i64, _i32, _i32, _p, _p],
    "dfol_pair_ll_h2_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _p, _i32, _p, _i64, _p, _p, _p, _i32, _i32, _p, _p, _p, _i32, _i32, _f,
                            _i32, _p, _p],
    "dfol_pair_w2_f16_bytes": [_i32],
    "dfol_pair_pack_w2_f16": [_p, _i64, _i32, _i32, _p, _p],
    "dfol_pair_ll_h1_f32": [_p, _i64, _i32, _p, _i64, _p, _p, _p, _i32, _p, _i64, _p, _p, _p, _i32, _i32, _p, _p, _p, _i32, _i32, _f,
                            _i32, _p, _p],
    "dfol_run_program": [_p, _p, _p, _i32, _p, _p, _p],
    "dfol_set_range_status": [_p],
    "dfol_pair_features_bwd_f32": [_p, _i64, _i32, _p, _p, _i32, _i32, _p, _i64, _p],
    "dfol_dropout_advance": [_p, _p],
    "dfol_dropout_f32": [_p, _i64, _p, _i64, _i64, _i32, _f, _p, ctypes.c_uint32, _p],
    "dfol_scene_bce_supported": [_i32, _i32, _i32],         # 1 / 0, called directly
    "dfol_scene_bce_fwd_workspace": [_i32, _i32, _i32],     # float counts (int64), called directly
    "dfol_scene_bce_bwd_cols_workspace": [_i32, _i32, _i32],
    "dfol_scene_bce_fwd_f32": [_p, _i64, _i32, _i32, _p, _i64, _i32, _p, _p, _i32, _p, _p, _f, _p, _p, _p],
    "dfol_scene_bce_bwd_rows_f32": [_p, _p, _i64, _i32, _i32, _p, _i64, _i32, _p, _p, _i32, _p, _p, _p, _i64, _p],
    "dfol_scene_bce_bwd_cols_f32": [_p, _p, _i64, _i32, _i32, _p, _i64, _i32, _p, _p, _i32, _p, _p, _p, _p, _p, _p],
    "dfol_scene_pair_rows_f32": [_p, _i64, _i32, _i32, _p, _p, _i32, _p, _i64, _p],
    "dfol_scene_pair_rows_bwd_f32": [_p, _i64, _i32, _i32, _p, _p, _i32, _p, _i64, _p],
}


ABI_VERSION = 4      # include/dfol_vqa.h: DFOL_ABI_VERSION


def load():
    """Load the library once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DfolError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    lib.dfol_last_error.restype = ctypes.c_char_p
    lib.dfol_abi_version.restype = ctypes.c_int
    if lib.dfol_abi_version() != ABI_VERSION:        # a stale build answers wrongly without a message (UV units changed between 2 and 3, struct layouts between 3 and 4)
        raise DfolError("%s has ABI version %d, this host side needs %d: rebuild it (make -C dfol_vqa_amd/csrc)"
                        % (LIB_PATH, lib.dfol_abi_version(), ABI_VERSION))
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int
    lib.dfol_linear_wgrad_workspace.restype = ctypes.c_int64
    lib.dfol_filter_gate_bwd_scratch.restype = ctypes.c_int64
    lib.dfol_pair_w2_f16x2_bytes.restype = ctypes.c_int64
    lib.dfol_pair_w2_f16_bytes.restype = ctypes.c_int64
    lib.dfol_linear_w_f16x2_bytes.restype = ctypes.c_int64
    lib.dfol_pair_wgrad_fused_workspace.restype = ctypes.c_int64
    lib.dfol_pair_wgrad_fused_sums_workspace.restype = ctypes.c_int64
    lib.dfol_set_range_status.restype = ctypes.c_int
    lib.dfol_scene_bce_fwd_workspace.restype = ctypes.c_int64
    lib.dfol_scene_bce_bwd_cols_workspace.restype = ctypes.c_int64
    _lib = lib
    return lib


def _ptr(t, dtype=None, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise DfolError("missing tensor argument")
    if not t.is_cuda:
        raise DfolError("the HIP path needs tensors on the GPU (got a %s tensor); there is no CPU fallback" % t.device)
    if dtype is not None and t.dtype != dtype:
        raise DfolError("expected dtype %s, got %s" % (dtype, t.dtype))
    if not t.is_contiguous():
        raise DfolError("tensor must be contiguous")
    if _KEEP is not None:                                   # a graph capture is recording: the graph bakes this address in (see keep_alive)
        _KEEP.append(t)
    return t.data_ptr()


def _dp(t):
    """data_ptr() of a (possibly strided) tensor handed to a kernel; like _ptr, it pins the tensor to a capturing graph."""
    if _KEEP is not None:
        _KEEP.append(t)
    return t.data_ptr()


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_CUR_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """The current HIP stream's handle.  (torch.cuda.current_stream() builds a Stream object through four Python layers: 10 us a call,
    0.35 ms of an eager 256-question batch's 34 launches; the raw accessors behind it are two C calls.)"""
    if _RAW_STREAM is not None and _CUR_DEVICE is not None:
        return _RAW_STREAM(_CUR_DEVICE())
    return torch.cuda.current_stream().cuda_stream


# Optional per-entry-point timing with HIP events on the launch stream (bench.py's roofline leg).
_timed = None          # None, or {entry point name: [(start_event, end_event), ...]}


def enable_kernel_timing(names):
    global _timed
    _timed = {n: [] for n in names}


def disable_kernel_timing():
    """-> {name: (launches, total seconds)}; call after torch.cuda.synchronize()."""
    global _timed
    out = {}
    if _timed is not None:
        for n, evs in _timed.items():
            out[n] = (len(evs), sum(s.elapsed_time(e) for s, e in evs) * 1e-3)
    _timed = None
    return out


def call(name, *args):
    lib = load()
    if _timed is not None and name in _timed:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()                      # torch's current stream == the stream handed to the kernel (_stream())
        rc = getattr(lib, name)(*args)
        e.record()
        _timed[name].append((s, e))
    else:
        rc = getattr(lib, name)(*args)
    if rc != 0:
        raise DfolError("%s failed (%d): %s" % (name, rc, lib.dfol_last_error().decode()))


F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


# ---- fp16 range status (include/dfol_vqa.h: dfol_set_range_status) -----------------------------------------------------------------------------
RANGE_X_OVERFLOW = 1
RANGE_PAIR_SATURATED = 2
_RANGE_WORDS = {}
_RANGE_RING = 8
_RANGE_ACTIVE = threading.local()    # .word: the status word of this thread's open RangeWatch (a watch opened inside another hands it back)


def range_message(flags):
    """What a non-zero fp16-range status word says, and the remedy: the text of the error a forward raises, and of the warning of a forward that
    runs the batch again instead (`range_overflow: rerun`)."""
    what = []
    if flags & RANGE_X_OVERFLOW:
        what.append("an input of a dense layer (object features, or a hidden activation) is beyond fp16's largest finite value 65504 or NaN")
    if flags & RANGE_PAIR_SATURATED:
        what.append("a first-layer sum of the relation MLP reaches the fused pair kernel's saturation point (ELU outputs beyond 4.16e4) or is NaN")
    return ("fp16 range exceeded in the two-piece fp16 arithmetic (dense math 'f16x2', the default): %s. The results of this "
            "forward are not valid. Use `mlp_math: bf16x3` (config key; three bf16 pieces, fp32's exponent range) or "
            "DFOL_DENSE_MATH=bf16x3 / DFOL_PAIR_MATH=bf16x3, or normalise the features." % "; ".join(what))


class RangeWatch(object):
    """One forward's watch on the fp16-range status word of its device.  The default dense arithmetic ("f16x2") splits activations into two
    UNSCALED fp16 pieces: an object feature beyond 65504 would come back as NaN log-probabilities.  The dense kernels flag that in a device word; `finish()` queues its copy behind the forward's launches (pinned, asynchronous - no
    extra synchronisation) and returns the closure that, once the answers have been read back, raises DfolError naming the remedy."""

    def __init__(self, device):
        dev = torch.device(device)
        key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
        if CAPTURE_RANGE_WORD is not None and capturing():
            word = CAPTURE_RANGE_WORD
        else:
            # a small ring of words per device: forwards in flight at once on DIFFERENT streams (bench.py's fresh-programs loop alternates two)
            # must not share one - each clears its word on its own stream behind its copy
            ring = _RANGE_WORDS.get(key)
            if ring is None:
                ring = _RANGE_WORDS[key] = [torch.zeros(_RANGE_RING, dtype=torch.int32, device=dev), 0]
            word = ring[0][ring[1] % _RANGE_RING:ring[1] % _RANGE_RING + 1]
            ring[1] += 1
        self.word, self.device = word, dev
        self._outer, _RANGE_ACTIVE.word = getattr(_RANGE_ACTIVE, "word", None), word
        load().dfol_set_range_status(word.data_ptr())           # (thread-local in the library: the launches of THIS thread carry it)

    def finish(self):
        # (a graph capture must not allocate pinned memory: its owner - GraphedForward / GraphedTrainStep - hands one in before it starts)
        host = CAPTURE_RANGE_HOST if (capturing() and CAPTURE_RANGE_HOST is not None) else _range_host()
        if _KEEP is not None:
            _KEEP.append(host)
        host.copy_(self.word, non_blocking=True)
        if capturing() and CAPTURE_RANGE_DEV is not None:         # (a pipelined replay reads its OWN copy of the word: GraphedForward.submit)
            CAPTURE_RANGE_DEV.copy_(self.word)
        # cleared ON THE STREAM behind the copy: the next forward queued behind this one (test_epoch and the bench keep two or more in flight)
        # starts from a clean word instead of inheriting this one's flag until the host gets round to its check
        self.word.zero_()
        # the library's pointer is a thread-local of THIS thread: later direct calls - possibly on another device - must not OR into this word
        # (a watch opened inside another one - the feature store building its cache on a forward's first use - hands the outer word back)
        _RANGE_ACTIVE.word = self._outer
        load().dfol_set_range_status(None if self._outer is None else self._outer.data_ptr())
        word, dev = self.word, self.device
        # (an event behind the copy: waiting for the STREAM would also wait for whatever was queued after this forward - the next batch of a
        # pipelined loop; a captured forward has no event of its own: its replay's owner waits for the stream)
        done = None
        if not capturing():
            done = torch.cuda.Event()
            done.record()

        def check(sync=True, value=None, throw=True):
            """sync=False: look at what has arrived so far (a replayed train step checks the step BEFORE it: no host wait per step); value: the word
            as the caller read it back itself (a pipelined graph replay); throw=False: hand the flags back (0: in range) instead of raising - the
            caller re-runs the batch on the wide-range arithmetic (interpreter: `range_overflow: rerun`)."""
            if sync and value is None:
                if done is not None:
                    done.synchronize()
                else:
                    torch.cuda.current_stream(dev).synchronize()
            v = int(host[0]) if value is None else int(value)
            if v:
                word.zero_()
                if throw:
                    raise DfolError(range_message(v))
            if not throw:
                return v
        check.range_check = True
        return check


def range_status_off():
    """No status word on this thread: what a forward does on its way out, also when it raised before its watch finished."""
    _RANGE_ACTIVE.word = None
    load().dfol_set_range_status(None)


_RANGE_HOSTS = []
CAPTURE_RANGE_HOST = None
CAPTURE_RANGE_WORD = None            # the status word of ONE captured forward (graphs replayed side by side on two streams must not share the device's)
CAPTURE_RANGE_DEV = None             # a device int32 a captured forward also leaves its status word in (before clearing it), or None
CAPTURE_RANGE_CHECKS = []            # checks of forwards that ran INSIDE a capture without a deferred queue: the graph's owner runs them after replays


def new_range_host():
    return torch.zeros(1, dtype=torch.int32).pin_memory()        # (zero: a replayed step looks at it before its first copy has arrived)


def _range_host():
    """A pinned int32 for one forward's copy of the status word (a small ring: forwards in flight at once - forward_async - keep their own)."""
    if len(_RANGE_HOSTS) < 16:
        _RANGE_HOSTS.append(torch.zeros(1, dtype=torch.int32).pin_memory())
        return _RANGE_HOSTS[-1]
    _RANGE_HOSTS.append(_RANGE_HOSTS.pop(0))
    return _RANGE_HOSTS[-1]


# ---- keep-alive registry for captured graphs ---------------------------------------------------------------------------------
# A captured HIP graph bakes in the raw device addresses of every tensor its launches read.  Several of those tensors are owned only
# by evictable caches (host_util's upload cache, the geometry caches, the packed weight images, lowered token arrays); once an
# eviction frees one, the allocator recycles the memory and a replay would silently read unrelated data.  While a capture runs,
# every cache hands what it returns to keep_alive(), and the GraphedForward object holds those references for as long as it lives.
# Since round 3 that convention is belt and braces, the mechanism is structural: (a) _ptr() / _dp() - through which EVERY tensor address
# reaches a launch of this library - and (b) LRUCache.get / __setitem__ - through which every content-keyed cache hands out what torch's
# own launches may read (index arrays, geometry, masks) - append to the same list while a capture is recording.  A cache that forgets to
# call keep_alive() can no longer leave a dangling address in a graph: tests/test_interpreter_gpu.py::
# test_graphed_forward_survives_cache_eviction runs with the explicit calls switched off (EXPLICIT_KEEP_ALIVE) as well.
_KEEP = None
EXPLICIT_KEEP_ALIVE = True       # tests switch the caches' own keep_alive() calls off to show that the registration in _ptr / _dp suffices


def keep_alive(obj):
    if _KEEP is not None and EXPLICIT_KEEP_ALIVE:
        _KEEP.append(obj)
    return obj


class keeping(object):
    """Context manager: collect into `sink` everything the caches hand out while it is active."""

    def __init__(self, sink):
        self._sink = sink

    def __enter__(self):
        global _KEEP
        self._outer, _KEEP = _KEEP, self._sink
        return self._sink

    def __exit__(self, *exc):
        global _KEEP
        _KEEP = self._outer
        return False


# ---- thin typed wrappers (tensor in / tensor out), one per entry point -------------------------------
def attr_gather(table, obj_off, pred_q, pred_col, NS, default_ll=-30.0):
    P = pred_q.numel()
    ll = torch.empty(P, NS, dtype=F32, device=table.device)
    assert table.stride(1) == 1
    call("dfol_attr_gather_f32", _dp(table), table.stride(0), _ptr(obj_off, I32), _ptr(pred_q, I32), _ptr(pred_col, I32),
         P, NS, default_ll, _ptr(ll), _stream())
    return ll


def rel_gather(table, pair_off, n_obj, pred_q, pred_col, NS, orientation=TILE_SUBJECT_ROWS, default_ll=-30.0):
    P = pred_q.numel()
    tile = torch.empty(P, NS, NS, dtype=F32, device=table.device)
    assert table.stride(1) == 1
    call("dfol_rel_gather_f32", _dp(table), table.stride(0), _ptr(pair_off, I64), _ptr(n_obj, I32), _ptr(pred_q, I32),
         _ptr(pred_col, I32), P, NS, orientation, default_ll, _ptr(tile), _stream())
    return tile


def option_normalize_(ll, seg_off, pred_q, n_obj, NS):
    rank = ll.dim() - 1
    call("dfol_option_normalize_f32", _ptr(ll, F32), _ptr(seg_off, I32), seg_off.numel() - 1, _ptr(pred_q, I32), _ptr(n_obj, I32),
         NS, rank, _stream())
    return ll


def filter_fwd(att_in, ll, pred_q, n_obj, neg=None, active=None):
    P, NS = ll.shape
    out = torch.empty(P, NS, dtype=F32, device=ll.device)
    call("dfol_filter_fwd_f32", _ptr(att_in, F32), _ptr(ll, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), _ptr(neg, U8, True),
         0 if neg is None else 1, _ptr(active, U8, True), P, NS, _ptr(out), _stream())
    return out


def relate_fwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, neg=None, active=None, want=None,
               orientation=TILE_SUBJECT_ROWS, lone_forall_identity=False, need_s=True, need_o=True, diag_absent=False):
    """`diag_absent`: the caller guarantees every tile's diagonal holds the absent likelihood (tiles made by the oracle do)."""
    P, NS = tile.shape[0], tile.shape[1]
    flags = (RELATE_LONE_FORALL_IDENTITY if lone_forall_identity else 0) | (RELATE_DIAG_ABSENT if diag_absent else 0)
    post_s = torch.empty(P, NS, dtype=F32, device=tile.device) if need_s else None
    post_o = torch.empty(P, NS, dtype=F32, device=tile.device) if need_o else None
    call("dfol_relate_fwd_f32", _ptr(prior_s, F32), _ptr(prior_o, F32), _ptr(tile, F32), _ptr(pred_q, I32), _ptr(n_obj, I32),
         _ptr(quant_s, F32), _ptr(quant_o, F32), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True),
         _ptr(want, U8, True), P, NS, orientation, flags, _ptr(post_s, F32, True), _ptr(post_o, F32, True), _stream())
    return post_s, post_o


def gate_params(weight, bias):
    """The float[18] image of a NeuralLogicGate's nn.Linear(2, 6) the gated kernels read: W row-major, then c (no host read, no sync)."""
    if tuple(weight.shape) != (6, 2) or tuple(bias.shape) != (6,):
        raise DfolError("a logic gate holds nn.Linear(2, 6): weight [6, 2] and bias [6], got %s and %s" % (tuple(weight.shape), tuple(bias.shape)))
    return torch.cat([weight.detach().reshape(12), bias.detach().reshape(6)]).to(F32).contiguous()


def filter_gate_fwd(att_in, ll, pred_q, n_obj, gate, neg=None, active=None):
    """filter_fwd with the trainable gate: gate = gate_params(weight, bias) of axis 0."""
    P, NS = ll.shape
    out = torch.empty(P, NS, dtype=F32, device=ll.device)
    call("dfol_filter_gate_fwd_f32", _ptr(att_in, F32), _ptr(ll, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), _ptr(neg, U8, True),
         0 if neg is None else 1, _ptr(active, U8, True), P, NS, _ptr(gate, F32), _ptr(out), _stream())
    return out


def relate_gate_fwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, gate_s, gate_o, neg=None, active=None, want=None,
                    orientation=TILE_SUBJECT_ROWS, lone_forall_identity=False, need_s=True, need_o=True, diag_absent=False):
    """relate_fwd with the trainable gates: gate_s / gate_o = gate_params of axis 0 / axis 1."""
    if tile.dtype != F32:
        raise DfolError("the gated relate kernels read fp32 tiles (got %s): relation_tile_dtype: bf16 and trainable_gate: True do not combine" % tile.dtype)
    P, NS = tile.shape[0], tile.shape[1]
    flags = (RELATE_LONE_FORALL_IDENTITY if lone_forall_identity else 0) | (RELATE_DIAG_ABSENT if diag_absent else 0)
    post_s = torch.empty(P, NS, dtype=F32, device=tile.device) if need_s else None
    post_o = torch.empty(P, NS, dtype=F32, device=tile.device) if need_o else None
    call("dfol_relate_gate_fwd_f32", _ptr(prior_s, F32), _ptr(prior_o, F32), _ptr(tile, F32), _ptr(pred_q, I32), _ptr(n_obj, I32),
         _ptr(quant_s, F32), _ptr(quant_o, F32), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True),
         _ptr(want, U8, True), P, NS, orientation, flags, _ptr(gate_s, F32), _ptr(gate_o, F32), _ptr(post_s, F32, True),
         _ptr(post_o, F32, True), _stream())
    return post_s, post_o


def gate_native():
    """DFOL_GATE_NATIVE=1 (opt-in, read when a forward starts): a model with trainable gates takes the fast inference routes - the one-launch
    gated Relate in the Python loop and the gated opcodes of the native executor.  Unset: the generic gated route and the Python loop, as before."""
    return os.environ.get("DFOL_GATE_NATIVE", "0") == "1"


def relate_one_gate_fwd(x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, gate_s, gate_o, neg=None, active=None,
                        lone_forall_identity=False):
    """relate_one_fwd with the trainable gates: gate_s / gate_o = gate_params of axis 0 / axis 1, x_is_subject uint8 [P] (which axis x is on)."""
    if tile.dtype != F32:
        raise DfolError("the gated relate kernels read fp32 tiles (got %s): relation_tile_dtype: bf16 and trainable_gate: True do not combine" % tile.dtype)
    P, NS = tile.shape[0], tile.shape[1]
    if x_is_subject.numel() != P:
        raise DfolError("relate_one_gate_fwd: %d subject flags for %d predicates" % (x_is_subject.numel(), P))
    post = torch.empty(P, NS, dtype=F32, device=tile.device)
    call("dfol_relate_one_gate_fwd_f32", _ptr(x_att, F32), _ptr(prev_att, F32), _ptr(tile, F32), _ptr(pred_q, I32), _ptr(n_obj, I32),
         _ptr(quant_prev, F32), _ptr(x_is_subject, U8), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True), P, NS,
         1 if lone_forall_identity else 0, _ptr(gate_s, F32), _ptr(gate_o, F32), _ptr(post), _stream())
    return post


def gate_bf16():
    """DFOL_GATE_BF16=1 together with DFOL_GATE_NATIVE=1 (opt-in, read when a forward starts): a gated model with `relation_tile_dtype: bf16` keeps
    bf16 relation tiles where the one-launch gated Relate reads them (relate_one_gate_fwd_bf16: inference, no gradient recorded, NS % 8 == 0, no
    choose_rel in the batch); without DFOL_GATE_NATIVE it has no effect, only the one-launch route has a bf16 form.  Unset: the combination of the
    two config keys is refused, as before."""
    return gate_native() and os.environ.get("DFOL_GATE_BF16", "0") == "1"


def relate_one_gate_fwd_bf16(x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, gate_s, gate_o, neg=None, active=None,
                             lone_forall_identity=False):
    """relate_one_gate_fwd on bfloat16 tiles (NS % 8 == 0, NS <= 256)."""
    if tile.dtype != torch.bfloat16:
        raise DfolError("relate_one_gate_fwd_bf16 reads bfloat16 tiles (got %s): fp32 tiles go to relate_one_gate_fwd" % tile.dtype)
    P, NS = tile.shape[0], tile.shape[1]
    if NS % 8 != 0 or NS > 256:
        raise DfolError("relate_one_gate_fwd_bf16: NS=%d (a multiple of 8, at most 256)" % NS)
    if x_is_subject.numel() != P:
        raise DfolError("relate_one_gate_fwd_bf16: %d subject flags for %d predicates" % (x_is_subject.numel(), P))
    post = torch.empty(P, NS, dtype=F32, device=tile.device)
    call("dfol_relate_one_gate_fwd_bf16", _ptr(x_att, F32), _ptr(prev_att, F32), _ptr(tile, torch.bfloat16), _ptr(pred_q, I32), _ptr(n_obj, I32),
         _ptr(quant_prev, F32), _ptr(x_is_subject, U8), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True), P, NS,
         1 if lone_forall_identity else 0, _ptr(gate_s, F32), _ptr(gate_o, F32), _ptr(post), _stream())
    return post


def gate_train():
    """DFOL_GATE_TRAIN=1 (opt-in, read when a forward starts; independent of DFOL_GATE_NATIVE): a gated relate hop that a gradient reaches runs
    the one-posterior kernels (relate_keep_gate_fwd / relate_keep_gate_bwd) instead of gate, gate, relate_gate_fwd(want), gate and their autograd
    backward.  Unset: the generic gated route under autograd, as before."""
    return os.environ.get("DFOL_GATE_TRAIN", "0") == "1"


def _keep_gate_check(what, tile, x_is_subject):
    if tile.dtype != F32:
        raise DfolError("the gated relate kernels read fp32 tiles (got %s): relation_tile_dtype: bf16 and trainable_gate: True do not combine" % tile.dtype)
    P, NS = tile.shape[0], tile.shape[1]
    if x_is_subject.numel() != P:
        raise DfolError("%s: %d subject flags for %d predicates" % (what, x_is_subject.numel(), P))
    return P, NS


def relate_keep_gate_fwd(x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, gate_s, gate_o, neg=None, active=None,
                         lone_forall_identity=False):
    """relate_one_gate_fwd on the train step's tile: SUBJECTS along rows for every predicate, x_is_subject uint8 [P] picks the axis summed out."""
    P, NS = _keep_gate_check("relate_keep_gate_fwd", tile, x_is_subject)
    post = torch.empty(P, NS, dtype=F32, device=tile.device)
    call("dfol_relate_keep_gate_fwd_f32", _ptr(x_att, F32), _ptr(prev_att, F32), _ptr(tile, F32), _ptr(pred_q, I32), _ptr(n_obj, I32),
         _ptr(quant_prev, F32), _ptr(x_is_subject, U8), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True), P, NS,
         1 if lone_forall_identity else 0, _ptr(gate_s, F32), _ptr(gate_o, F32), _ptr(post), _stream())
    return post


def relate_train():
    """DFOL_RELATE_TRAIN=1 (opt-in, read when a forward starts): an ungated relate hop that a gradient reaches runs the one-posterior kernels
    (relate_keep_fwd / relate_keep_bwd) instead of gate, gate, relate_fwd(want), gate and their autograd backward over both directions.
    Unset: the generic route under autograd, as before."""
    return os.environ.get("DFOL_RELATE_TRAIN", "0") == "1"


RELATE_KEEP_BWD_MAX_NS = 2048      # the backward's (2 + 4) NS floats of LDS = 48 KB


def _keep_check(what, x_att, prev_att, tile, x_is_subject):
    if tile.dtype != F32:
        raise DfolError("%s reads fp32 tiles (got %s): the train step never stores bf16 relation tiles" % (what, tile.dtype))
    if tile.dim() != 3 or tile.shape[1] != tile.shape[2]:
        raise DfolError("%s: tile of shape %s (expected [P, NS, NS])" % (what, tuple(tile.shape)))
    P, NS = tile.shape[0], tile.shape[1]
    if tuple(x_att.shape) != (P, NS) or prev_att.dim() != 2 or prev_att.shape[1] != NS:
        raise DfolError("%s: x %s / prev %s do not match the tile's [%d, %d, %d]" % (what, tuple(x_att.shape), tuple(prev_att.shape), P, NS, NS))
    if x_is_subject.numel() != P:
        raise DfolError("%s: %d subject flags for %d predicates" % (what, x_is_subject.numel(), P))
    return P, NS


def relate_keep_fwd(x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, neg=None, active=None, lone_forall_identity=False):
    """relate_one_fwd on the train step's tile: fp32, SUBJECTS along rows for every predicate; x_is_subject uint8 [P] picks the axis summed out."""
    P, NS = _keep_check("relate_keep_fwd", x_att, prev_att, tile, x_is_subject)
    args = (_ptr(x_att, F32), _ptr(prev_att, F32), _ptr(tile, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), _ptr(quant_prev, F32),
            _ptr(x_is_subject, U8), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True), P, NS, 1 if lone_forall_identity else 0)
    post = torch.empty(P, NS, dtype=F32, device=tile.device)
    call("dfol_relate_keep_fwd_f32", *args, _ptr(post), _stream())
    return post


def relate_one_fwd(x_att, prev_att, tile, pred_q, n_obj, quant_prev, neg=None, active=None, lone_forall_identity=False):
    P, NS = tile.shape[0], tile.shape[1]
    post = torch.empty(P, NS, dtype=F32, device=tile.device)
    call("dfol_relate_one_fwd_f32", _ptr(x_att, F32), _ptr(prev_att, F32), _ptr(tile, F32), _ptr(pred_q, I32), _ptr(n_obj, I32),
         _ptr(quant_prev, F32), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True), P, NS,
         1 if lone_forall_identity else 0, _ptr(post), _stream())
    return post


def relate_one_fwd_bf16(x_att, prev_att, tile, pred_q, n_obj, quant_prev, neg=None, active=None, lone_forall_identity=False):
    """relate_one_fwd on bfloat16 tiles (NS % 8 == 0)."""
    P, NS = tile.shape[0], tile.shape[1]
    post = torch.empty(P, NS, dtype=F32, device=tile.device)
    call("dfol_relate_one_fwd_bf16", _ptr(x_att, F32), _ptr(prev_att, F32), _ptr(tile, torch.bfloat16), _ptr(pred_q, I32), _ptr(n_obj, I32),
         _ptr(quant_prev, F32), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True), P, NS,
         1 if lone_forall_identity else 0, _ptr(post), _stream())
    return post


def quantify_fwd(att, quant, pred_q, n_obj):
    P, NS = att.shape
    lp = torch.empty(P, dtype=F32, device=att.device)
    call("dfol_quantify_fwd_f32", _ptr(att, F32), _ptr(quant, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), P, NS, _ptr(lp), _stream())
    return lp


def quantify_hard(att, quant, pred_q, n_obj, total_obj):
    P, NS = att.shape
    lp = torch.empty(P, dtype=F32, device=att.device)
    call("dfol_quantify_hard_f32", _ptr(att, F32), _ptr(quant, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), P, NS, int(total_obj), _ptr(lp),
         _stream())
    return lp


def find_max_ind(lp, seg_off, likelihood_threshold=0.0):
    """uint8 [P]: 1 where a predicate attains its question's maximum probability above the threshold (util.py:64-66)."""
    flag = torch.empty(lp.numel(), dtype=U8, device=lp.device)
    call("dfol_find_max_ind_f32", _ptr(lp, F32), _ptr(seg_off, I32), seg_off.numel() - 1, float(likelihood_threshold), _ptr(flag, U8), _stream())
    return flag


def gate(x_att, y_att, x_quant, y_quant, g):
    P, NS = x_att.shape
    out = torch.empty_like(x_att)
    outq = torch.empty_like(x_quant)
    call("dfol_gate_f32", _ptr(x_att, F32), _ptr(y_att, F32), _ptr(x_quant, F32), _ptr(y_quant, F32), _ptr(g, F32), P, NS,
         _ptr(out), _ptr(outq), _stream())
    return out, outq


def gather_rows(src, idx):
    src2 = src.reshape(src.shape[0], -1)
    P, width = idx.numel(), src2.shape[1]
    out = torch.empty((P,) + tuple(src.shape[1:]), dtype=F32, device=src.device)
    call("dfol_gather_rows_f32", _ptr(src2, F32), _ptr(idx, I32), P, width, _ptr(out), _stream())
    return out


def gather_object_rows(features, boxes, sizes, slot, obj_off, out):
    """out[obj_off[i] + j] = [features[slot[i]][j], W, H, x1, y1, x2 - x1, y2 - y1] (csrc/dfol_store.hip); features [S, max_obj, F], boxes
    [S, max_obj, 4], sizes [S, 2]; slot [I] and obj_off [I + 1] int32 on the device; out [O, >= F + 6] rows of unit column stride."""
    S, max_obj, F = features.shape
    if tuple(boxes.shape) != (S, max_obj, 4) or tuple(sizes.shape) != (S, 2) or obj_off.numel() != slot.numel() + 1:
        raise DfolError("gather_object_rows: store tensors / index arrays of mismatched shapes")
    if out.dim() != 2 or out.dtype != F32 or not out.is_cuda or (out.shape[0] > 1 and out.stride(1) != 1) or out.shape[1] < F + 6:
        raise DfolError("gather_object_rows: out must be fp32 device rows of at least F + 6 = %d columns" % (F + 6))
    bf16t = features.dtype == torch.bfloat16                # (a bf16 store's table: the stored values widened exactly, the same matrix)
    call("dfol_gather_object_rows_bf16_f32" if bf16t else "dfol_gather_object_rows_f32", _ptr(features, torch.bfloat16 if bf16t else F32), _ptr(boxes, F32), _ptr(sizes, F32), _ptr(slot, I32), _ptr(obj_off, I32),
         slot.numel(), max_obj, F, _dp(out), out.stride(0), _stream())
    return out


def store_round_bf16(src, dst):
    """dst = bfloat16(src), round to nearest even by the dense kernels' own dfol_rne2 (csrc/dfol_store.hip): how a bf16 feature store's chunk
    goes from its fp32 upload buffer into the table.  src fp32, dst bfloat16, contiguous device tensors of the same element count."""
    if src.numel() != dst.numel():
        raise DfolError("store_round_bf16: %d source elements for %d destination elements" % (src.numel(), dst.numel()))
    call("dfol_store_round_bf16", _ptr(src, F32), src.numel(), _ptr(dst, torch.bfloat16), _stream())
    return dst


def store_rows(boxes, sizes, slot, obj_off, src_row, box6):
    """The index form of a store-backed batch (csrc/dfol_store.hip): src_row[obj_off[i] + j] = slot[i] * max_obj + j and box6 = the gather's last
    six columns, written into src_row [O] int32 and box6 [O, 6] fp32; boxes [S, max_obj, 4], sizes [S, 2]."""
    S, max_obj = boxes.shape[0], boxes.shape[1]
    if tuple(boxes.shape) != (S, max_obj, 4) or tuple(sizes.shape) != (S, 2) or obj_off.numel() != slot.numel() + 1:
        raise DfolError("store_rows: store tensors / index arrays of mismatched shapes")
    if src_row.dim() != 1 or box6.dim() != 2 or tuple(box6.shape) != (src_row.numel(), 6):
        raise DfolError("store_rows: src_row [O] int32 and box6 [O, 6] fp32")
    call("dfol_store_rows_f32", _ptr(boxes, F32), _ptr(sizes, F32), _ptr(slot, I32), _ptr(obj_off, I32), slot.numel(), S, max_obj,
         _ptr(src_row, I32), _ptr(box6, F32), _stream())
    return src_row, box6


def store_objects(cache, src_row, box6, out=None):
    """The object matrix of a store-backed batch from cached featurizer outputs (csrc/dfol_store.hip): out[r] = [cache[src_row[r]], box positions
    of box6[r]], [O, W + 4]; cache [rows, W] fp32 with unit column stride, src_row [O] int32 and box6 [O, 6] from store_rows.  out=: rows of
    unit column stride and at least W + 4 columns; columns beyond W + 4 are left alone."""
    O, W = src_row.numel(), cache.shape[1]
    if cache.dim() != 2 or cache.dtype != F32 or cache.stride(1) != 1 or src_row.dim() != 1 or tuple(box6.shape) != (O, 6):
        raise DfolError("store_objects: cache [rows, W] fp32 with unit column stride, src_row [O] int32 and box6 [O, 6] fp32")
    if out is None:
        out = torch.empty(O, W + 4, dtype=F32, device=cache.device)
    elif out.dim() != 2 or out.shape[0] != O or out.dtype != F32 or out.stride(1) != 1 or out.device != cache.device:
        raise DfolError("store_objects: out= must be [%d, >= %d] fp32 rows of unit column stride on %s" % (O, W + 4, cache.device))
    call("dfol_store_objects_f32", _dp(cache), cache.stride(0), _ptr(src_row, I32), _ptr(box6, F32), O, W, _dp(out), out.stride(0), _stream())
    return out


def segment_sum_rows(src, seg_off):
    Q, width = seg_off.numel() - 1, src.shape[1]
    out = torch.empty(Q, width, dtype=F32, device=src.device)
    call("dfol_segment_sum_rows_f32", _ptr(src, F32), _ptr(seg_off, I32), Q, width, _ptr(out), _stream())
    return out


def concept_rows(rows, order, seg_off, ucols, out, accumulate):
    """out[ucols[u]] (+)= sum of rows[order[k]] over segment u, in slot order (csrc/dfol_logic.hip: concept_rows_kernel); rows [P, width]."""
    rows2, out2 = rows.reshape(rows.shape[0], -1), out.reshape(out.shape[0], -1)
    call("dfol_concept_rows_f32", _dp(rows2), rows2.stride(0), _ptr(order, I32), _ptr(seg_off, I32), _ptr(ucols, I64), ucols.numel(), rows2.shape[1],
         _dp(out2), out2.stride(0), 1 if accumulate else 0, _stream())
    return out


def logic(op, a, b=None):
    out = torch.empty_like(a)
    call("dfol_logic_f32", op, _ptr(a, F32), _ptr(b, F32, True), a.numel(), _ptr(out), _stream())
    return out


def parametric_not(x, alpha):
    x2 = x.reshape(alpha.numel(), -1)
    out = torch.empty_like(x2)
    call("dfol_parametric_not_f32", _ptr(x2, F32), _ptr(alpha, F32), x2.shape[0], x2.shape[1], _ptr(out), _stream())
    return out.reshape(x.shape)


def segment_or(lp, seg_off, as_written=False):
    """as_written: the reference's fp32 formula instead of the complement form (callers that negate the aggregate: include/dfol_vqa.h)."""
    Q = seg_off.numel() - 1
    out = torch.empty(Q, dtype=F32, device=lp.device)
    call("dfol_segment_or_ref_f32" if as_written else "dfol_segment_or_f32", _ptr(lp, F32), _ptr(seg_off, I32), Q, _ptr(out), _stream())
    return out


def implication(prior, x, pred_q, n_obj):
    P, NS = x.shape
    out = torch.empty_like(x)
    call("dfol_implication_f32", _ptr(prior, F32), _ptr(x, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), P, NS, _ptr(out), _stream())
    return out


def compare(lp1, lp2, is_less):
    Q = lp1.numel()
    out = torch.empty(Q, 2, dtype=F32, device=lp1.device)
    call("dfol_compare_f32", _ptr(lp1, F32), _ptr(lp2, F32), _ptr(is_less, F32), Q, _ptr(out), _stream())
    return out


_SPLIT_W_CACHE = {}                    # (data_ptr, version, shape, stride) -> (weight kept alive, packed image)
SPLIT_MIN_WEIGHT = 65536              # weights of at least this many elements run on the bf16x3 split kernel, WHATEVER the row count:
#                                       the kernel choice must not depend on the batch size, or a question sharded across ranks would
#                                       see different roundings than in one process (tests/test_multirank_gpu.py asserts bit-equality)


def linear_pack_w_split(weight, transpose=False, pieces=3):
    """The bf16x3 image of a Linear weight [N, K] for dfol_linear_act_split_f32, cached per weight version (the cache holds the
    weight tensor, so its address cannot be recycled while the entry lives).  The version counter is what optimizers, load_state_dict
    and nn.init bump; writes through `.data` do not - call `_SPLIT_W_CACHE.clear()` after such a write.
    transpose=True packs weight^T (the operand of the backward product g @ W) under the ORIGINAL parameter's key, so a train step
    finds it by the parameter's version instead of inserting one dead entry per temporary transposed copy."""
    key = (_dp(weight), weight._version, tuple(weight.shape), weight.stride(0), bool(transpose), pieces)
    if weight.grad_fn is not None:
        # a TEMPORARY built from parameters inside a train step (the joined U | V weight: torch.cat of two column blocks): a new tensor every
        # step, so keyed by address it left one dead 4 - 6 MB entry per step and pushed live parameters out of the FIFO.  One slot per shape
        # instead, valid only for the very tensor it was packed from.
        key = ("temporary", 0, tuple(weight.shape), weight.stride(0), bool(transpose), pieces)
    hit = _SPLIT_W_CACHE.get(key)
    if hit is not None and hit[0] is not weight and weight.grad_fn is not None:
        hit = None
    if hit is None:
        src = weight.detach().t().contiguous() if transpose else weight
        N, K = src.shape
        # pieces = 3: the exact three-way bf16 split; 2: two fp16 pieces of the row-scaled weights (+ the per-row factors); 1: the bf16
        # mode's image (rounded to nearest)
        if pieces == 2:
            out = torch.empty(load().dfol_linear_w_f16x2_bytes(N, K) // 2, dtype=torch.bfloat16, device=weight.device)
        else:
            out = torch.empty(((N + 127) // 128) * ((K + 31) // 32) * 8192 * pieces // 2, dtype=torch.bfloat16, device=weight.device)
        call({3: "dfol_linear_pack_w_bf16x3", 2: "dfol_linear_pack_w_f16x2", 1: "dfol_linear_pack_w_bf16"}[pieces], _dp(src), src.stride(0), N, K,
             _ptr(out, torch.bfloat16), _stream())
        for stale in [k for k in _SPLIT_W_CACHE if k[0] == key[0] and k[4:] == key[4:]]:    # an older version of the same parameter
            del _SPLIT_W_CACHE[stale]
        if len(_SPLIT_W_CACHE) >= 64:
            _SPLIT_W_CACHE.pop(next(iter(_SPLIT_W_CACHE)))
        hit = _SPLIT_W_CACHE[key] = (weight, out)
    return keep_alive(hit)[1]


def linear_act_split(x, weight, bias, act, out=None, transpose_w=False):
    """y = act(x @ weight.T + bias) on the 16-bit matrix pipes with split operands: fp32 results.  Forward products (activations of order
    one) take two fp16 pieces and three products (dense_math "f16x2", the default); transpose_w=True: y = act(x @ weight + bias) (weight
    [K, N]) is the input-gradient product of a backward pass - operands of any magnitude - and keeps the three bf16 pieces, six
    products ("bf16x3"), whose exponent range is fp32's."""
    bf16 = _dense_math() == "bf16"                         # the bf16 mode: operands rounded to bf16, one product (configs[3])
    h2 = _dense_math() == "f16x2" and not transpose_w and x.dtype == F32
    M, K = x.shape
    N = weight.shape[1] if transpose_w else weight.shape[0]
    if x.dtype == torch.bfloat16:                          # bf16-STORED activations (the per-pair tensors of a bf16-mode train step): bf16 in, bf16 out
        if not bf16:
            raise DfolError("linear_act_split: a bfloat16 input needs the bf16 mode (dense_math('bf16'))")
        if out is None:
            out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        if act == ACT_NONE and N % 4 == 0 and out.stride(0) % 4 == 0 and linear_tall_supported(M, N, K):
            # the persistent form (csrc/dfol_dense_tall.hip): the same bits, 0.81 ms against 0.89 - 0.95 for the two tall products of a bf16 step
            call("dfol_linear_tall_bf16_bf16", _dp(x), x.stride(0), _ptr(linear_pack_w_split(weight, transpose_w, 1), torch.bfloat16), _ptr(bias, F32, True),
                 _dp(out), out.stride(0), M, N, K, None, None, 0, None, 0, _stream())
            return out
        call("dfol_linear_act_bf16_bf16", _dp(x), x.stride(0), _ptr(linear_pack_w_split(weight, transpose_w, 1), torch.bfloat16),
             _ptr(bias, F32, True), _dp(out), out.stride(0), M, N, K, act, _stream())
        return out
    if out is None:
        out = torch.empty(M, N, dtype=F32, device=x.device)
    call("dfol_linear_act_bf16_f32" if bf16 else ("dfol_linear_act_h2_f32" if h2 else "dfol_linear_act_split_f32"), _dp(x), x.stride(0),
         _ptr(linear_pack_w_split(weight, transpose_w, 1 if bf16 else (2 if h2 else 3)), torch.bfloat16), _ptr(bias, F32, True), _dp(out),
         out.stride(0), M, N, K, act, _stream())
    return out


def linear_wide(x, weight, bias, act, out=None):
    """linear_act_split's two-fp16-piece product through the persistent wide kernel (csrc/dfol_dense_wide.hip: 256 < N <= 512, X fetched and
    split once), whatever M: what dfol_linear_act_h2_f32 forwards to by itself for batches that fill the chip.  Same bits as the tiled kernel."""
    M, K = x.shape
    N = weight.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=F32, device=x.device)
    call("dfol_linear_wide_h2_f32", _dp(x), x.stride(0), _ptr(linear_pack_w_split(weight, False, 2), torch.bfloat16), _ptr(bias, F32, True), _dp(out),
         out.stride(0), M, N, K, act, _stream())
    return out


def linear_wide_supported(M, N, K):
    """dfol_linear_wide_supported: the persistent wide kernel takes the shape and it pays (DFOL_DENSE_WIDE: 0 never, 2 whenever taken)."""
    return bool(load().dfol_linear_wide_supported(int(M), int(N), int(K)))


def linear_wide_rows(table, src_row, weight, bias, act, out=None):
    """linear_wide over indexed rows: y[r] = act(table[src_row[r]] @ weight.T + bias), table [rows, K] fp32 (a feature store's features as a
    matrix), src_row [M] int32.  Bit for bit linear_wide(table[src_row]) without the gathered copy (csrc/dfol_dense_wide.hip, ROWS)."""
    M, K = src_row.numel(), table.shape[1]
    N = weight.shape[0]
    if weight.shape[1] != K or table.dtype != F32 or table.stride(1) != 1:
        raise DfolError("linear_wide_rows: table [rows, %d] fp32 with unit column stride, weight [N, %d]" % (K, K))
    if out is None:
        out = torch.empty(M, N, dtype=F32, device=table.device)
    call("dfol_linear_wide_rows_h2_f32", _dp(table), table.stride(0), _ptr(src_row, I32), _ptr(linear_pack_w_split(weight, False, 2), torch.bfloat16),
         _ptr(bias, F32, True), _dp(out), out.stride(0), M, N, K, act, _stream())
    return out


def store_bf16_direct():
    """DFOL_STORE_BF16_DIRECT=1 (opt-in, read when a forward starts): the default arithmetic ("f16x2") reads a bf16 feature store's rows in place
    on the inference route (linear_wide_rows_bf16t) instead of the gathered, widened matrix - the same bits.  Unset: every route as before."""
    return os.environ.get("DFOL_STORE_BF16_DIRECT", "0") == "1"


def linear_wide_rows_bf16t_supported(M, N, K, ld_table):
    """dfol_linear_wide_rows_bf16t_supported: the wide kernel takes the shape and it pays (linear_wide_supported), over a bf16 table of row
    stride ld_table (elements, a multiple of 4, at least K)."""
    return bool(load().dfol_linear_wide_rows_bf16t_supported(int(M), int(N), int(K), int(ld_table)))


def store_bf16_is_f16(table):
    """dfol_store_bf16_is_f16: True when every element of the bfloat16 tensor `table` (contiguous) is finite and an fp16 value,
    float(half(x)) == x - the certificate the two-product form of linear_wide_rows_bf16t stands on.  One pass over the table and a host wait."""
    if table.dtype != torch.bfloat16 or not table.is_contiguous():
        raise DfolError("store_bf16_is_f16: a contiguous bfloat16 tensor (got %s)" % table.dtype)
    flag = torch.ones(1, dtype=I32, device=table.device)
    call("dfol_store_bf16_is_f16", _dp(table), table.numel(), _ptr(flag, I32), _stream())
    return bool(flag.item())


def linear_wide_rows_bf16t(table, src_row, weight, bias, act, out=None, store=None):
    """linear_wide over the indexed rows of a bf16 table: y[r] = act(table[src_row[r]] @ weight.T + bias), table [rows, K] bfloat16 (a bf16 feature
    store's features as a matrix), src_row [M] int32, fp32 y, the packed weight image of linear_wide_rows.  Bit for bit
    linear_wide(table.float()[src_row]) - the stored values are widened exactly and split in the kernel (csrc/dfol_dense_wide.hip, BF16T) - without
    the widened copy, range report included.  Any M.  store: the DeviceFeatureStore whose table this is - a request for the two-product form,
    which runs only when the store's certificate `f16_exact` holds (every value an fp16 value: the same bits); otherwise three products."""
    M, K = src_row.numel(), table.shape[1]
    N = weight.shape[0]
    if weight.shape[1] != K or table.dtype != torch.bfloat16 or table.stride(1) != 1:
        raise DfolError("linear_wide_rows_bf16t: table [rows, %d] bfloat16 with unit column stride, weight [N, %d]" % (K, K))
    if out is None:
        out = torch.empty(M, N, dtype=F32, device=table.device)
    two = store is not None and bool(store.f16_exact)
    call("dfol_linear_wide_rows_bf16t_f16_h2_f32", _dp(table), table.stride(0), _ptr(src_row, I32), _ptr(linear_pack_w_split(weight, False, 2), torch.bfloat16),
         _ptr(bias, F32, True), _dp(out), out.stride(0), M, N, K, act, 1 if two else 0, _stream())
    return out


def linear_rows_bf16t_supported(N, K, ld_table):
    """dfol_linear_rows_bf16t_supported: linear_rows_bf16t takes a [N, K] weight over a bf16 table of row stride ld_table (elements)."""
    return bool(load().dfol_linear_rows_bf16t_supported(int(N), int(K), int(ld_table)))


def linear_rows_bf16t(table, src_row, weight, bias, act, out=None):
    """The bf16 mode's product over the indexed rows of a bf16 table: y[r] = act(table[src_row[r]] @ weight.T + bias), table [rows, K] bfloat16
    (a bf16 feature store's features as a matrix), src_row [M] int32, fp32 y.  Bit for bit linear_act_split(table.float()[src_row]) under
    dense_math("bf16"), which rounds an fp32 feature to the value the table holds (csrc/dfol_dense_split.hip, MODE 3).  Any M."""
    M, K = src_row.numel(), table.shape[1]
    N = weight.shape[0]
    if weight.shape[1] != K or table.dtype != torch.bfloat16 or table.stride(1) != 1:
        raise DfolError("linear_rows_bf16t: table [rows, %d] bfloat16 with unit column stride, weight [N, %d]" % (K, K))
    if out is None:
        out = torch.empty(M, N, dtype=F32, device=table.device)
    call("dfol_linear_act_rows_bf16t_f32", _dp(table), table.stride(0), _ptr(src_row, I32), _ptr(linear_pack_w_split(weight, False, 1), torch.bfloat16),
         _ptr(bias, F32, True), _dp(out), out.stride(0), M, N, K, act, _stream())
    return out


def linear_wgrad(dy, x, bias=False):
    """dW [N, K] = dy^T x for dy [M, N], x [M, K] (fp32, unit column stride); bias=True: (dW, db) with db [N] = dy.sum(0) from the
    same pass.  fp32 results on the matrix cores, deterministic (csrc/dfol_dense_wgrad.hip)."""
    M, N = dy.shape
    K = x.shape[1]
    stored_bf16 = dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16      # the bf16 mode's bf16-stored per-pair activations
    for t in (dy, x):
        if not t.is_cuda or (t.dtype != F32 and not stored_bf16) or t.stride(1) != 1:
            raise DfolError("linear_wgrad needs fp32 (or, both, bfloat16) GPU matrices with unit column stride")
    ws, dw, db, bf16 = _linear_wgrad_buffers(dy.device, M, N, K, bias)
    if ws is not None:
        name = "dfol_linear_wgrad_bias_bf16_bf16" if stored_bf16 else ("dfol_linear_wgrad_bias_bf16" if bf16 else "dfol_linear_wgrad_bias_f32")
        call(name, _dp(dy), dy.stride(0), _dp(x), x.stride(0), M, N, K, _ptr(ws), _ptr(dw), _ptr(db, F32, True), _stream())
    return (dw, db) if bias else dw


def _linear_wgrad_buffers(device, M, N, K, bias):
    """What linear_wgrad and linear_wgrad_rows share: (workspace, dW, db or None, bf16 mode).  Without rows (a shard without object pairs,
    a batch without rows) there is nothing to launch: the workspace is None and dW, db are the zero gradient, as dy.t() @ x gives."""
    new = torch.empty if M else torch.zeros
    dw = new(N, K, dtype=F32, device=device)
    db = new(N, dtype=F32, device=device) if bias else None
    ws = torch.empty(load().dfol_linear_wgrad_workspace(M, N, K), dtype=F32, device=device) if M else None
    # bf16 mode: the same layers whose forward product ran on bf16 operands (linear_act: weights of >= SPLIT_MIN_WEIGHT elements); the small
    # LSTM / attention layers stay fp32 forward AND backward
    return ws, dw, db, _dense_math() == "bf16" and N * K >= SPLIT_MIN_WEIGHT


def linear_wgrad_rows_supported(N, K, ld_dy, ld_table, bf16_table=False):
    """dfol_linear_wgrad_rows_supported: linear_wgrad_rows exists for the shape (where linear_wgrad runs its bf16-pipe kernel).  bf16_table: the
    question for a bf16 store's table (dfol_linear_wgrad_rows_bf16t_supported; ld_table in elements)."""
    fn = load().dfol_linear_wgrad_rows_bf16t_supported if bf16_table else load().dfol_linear_wgrad_rows_supported
    return bool(fn(int(N), int(K), int(ld_dy), int(ld_table)))


def linear_wgrad_rows(dy, table, src_row, bias=False):
    """linear_wgrad over indexed rows: dW [N, K] = dy^T table[src_row] for dy [M, N], table [rows, K] fp32 (a feature store's features as a
    matrix), src_row [M] int32; bias=True: (dW, db).  Bit for bit linear_wgrad(dy, table[src_row]) without the gathered copy
    (csrc/dfol_dense_wgrad.hip, ROWS); shapes linear_wgrad_rows_supported does not take are refused.  A bfloat16 table (a bf16 feature store's)
    is taken where the bf16 mode applies to the layer - linear_wgrad(dy, table.float()[src_row])'s bits there - and refused elsewhere."""
    M, N = dy.shape
    K = table.shape[1]
    bf16t = table.dtype == torch.bfloat16
    for t in (dy, table):
        if not t.is_cuda or (t.dtype != F32 and not (bf16t and t is table)) or t.stride(1) != 1:
            raise DfolError("linear_wgrad_rows needs fp32 GPU matrices (or a bfloat16 table) with unit column stride")
    if src_row.numel() != M:
        raise DfolError("linear_wgrad_rows: src_row has %d entries for %d rows of dy" % (src_row.numel(), M))
    ws, dw, db, bf16 = _linear_wgrad_buffers(dy.device, M, N, K, bias)
    if bf16t and not bf16:
        raise DfolError("linear_wgrad_rows: a bfloat16 table needs the bf16 mode on this layer (dense_math('bf16') and a weight of at least %d "
                        "elements; the arithmetic is %r, the weight [%d, %d]): use the gathered matrix" % (SPLIT_MIN_WEIGHT, _dense_math(), N, K))
    if ws is not None:
        call("dfol_linear_wgrad_bias_rows_bf16t" if bf16t else "dfol_linear_wgrad_bias_rows_bf16" if bf16 else "dfol_linear_wgrad_bias_rows_f32", _dp(dy), dy.stride(0), _dp(table), table.stride(0),
             _ptr(src_row, I32), M, N, K, _ptr(ws), _ptr(dw), _ptr(db, F32, True), _stream())
    return (dw, db) if bias else dw


def store_bf16_train():
    """DFOL_STORE_BF16_TRAIN=1 (opt-in, read when a forward starts): a featurizer that TRAINS in the default arithmetic ("f16x2") reads a bf16
    feature store's rows in place, forward (linear_wide_rows_bf16t) and first-layer weight gradient (linear_wgrad_rows_bf16t_x3), instead of
    the gathered, widened matrix - the same bits.  Unset: every route as before."""
    return os.environ.get("DFOL_STORE_BF16_TRAIN", "0") == "1"


def linear_wgrad_rows_bf16t_x3_supported(N, K, ld_dy, ld_table):
    """dfol_linear_wgrad_rows_bf16t_x3_supported: linear_wgrad_rows_bf16t_x3 exists for the shape over a bf16 table of row stride ld_table
    (elements) - never under DFOL_WGRAD_MATH=f32."""
    return bool(load().dfol_linear_wgrad_rows_bf16t_x3_supported(int(N), int(K), int(ld_dy), int(ld_table)))


def linear_wgrad_rows_bf16t_x3(dy, table, src_row, bias=False):
    """The default arithmetic's linear_wgrad over the indexed rows of a bf16 table: dW [N, K] = dy^T table[src_row] for dy [M, N] fp32, table
    [rows, K] bfloat16 (a bf16 feature store's features as a matrix), src_row [M] int32; bias=True: (dW, db).  Bit for bit what linear_wgrad(dy,
    table.float()[src_row]) gives in "f16x2" on its bf16-pipe kernel, without the gathered copy: dy in three bf16 pieces, a table value its own
    one piece, three products (csrc/dfol_dense_wgrad.hip).  Shapes linear_wgrad_rows_bf16t_x3_supported does not take are refused."""
    M, N = dy.shape
    K = table.shape[1]
    if not dy.is_cuda or not table.is_cuda or dy.dtype != F32 or table.dtype != torch.bfloat16 or dy.stride(1) != 1 or table.stride(1) != 1:
        raise DfolError("linear_wgrad_rows_bf16t_x3 needs an fp32 GPU matrix and a bfloat16 GPU table with unit column stride")
    if src_row.numel() != M:
        raise DfolError("linear_wgrad_rows_bf16t_x3: src_row has %d entries for %d rows of dy" % (src_row.numel(), M))
    ws, dw, db, bf16 = _linear_wgrad_buffers(dy.device, M, N, K, bias)
    if bf16:
        raise DfolError("linear_wgrad_rows_bf16t_x3: the bf16 mode applies to this layer (weight [%d, %d]): its form is linear_wgrad_rows" % (N, K))
    if ws is not None:
        call("dfol_linear_wgrad_bias_rows_bf16t_x3", _dp(dy), dy.stride(0), _dp(table), table.stride(0), _ptr(src_row, I32), M, N, K, _ptr(ws), _ptr(dw),
             _ptr(db, F32, True), _stream())
    return (dw, db) if bias else dw


def act_bwd(g, y, act):
    """dz = g * act'(.) from the activation's output y (same shape, fp32, contiguous): one launch."""
    g = g if g.is_contiguous() else g.contiguous()
    dz = torch.empty_like(y)
    call("dfol_act_bwd_f32", _ptr(g, F32), _ptr(y, F32), y.numel(), act, _ptr(dz), _stream())
    return dz


def linear_gradx(dz, weight):
    """dx = dz @ weight (dz [M, N], weight [N, K]): the input gradient of y = x W^T, on the same kernels as the forward."""
    M, N = dz.shape
    K = weight.shape[1]
    if N * K >= SPLIT_MIN_WEIGHT and N % 4 == 0 and dz.stride(0) % 2 == 0 and _dp(dz) % 8 == 0 and _dense_math() != "f32":
        return linear_act_split(dz, weight, None, ACT_NONE, transpose_w=True)
    return linear_act(dz, weight.detach().t().contiguous(), None, ACT_NONE)


_MATH_OVERRIDE = None


def _dense_math():
    """Arithmetic of the large dense products: "f16x2" (default: fp32 results from the fp16 pipe, two pieces per operand and three
    products for the forward products, the backward products as "bf16x3"), "bf16x3" (fp32 results from the bf16 pipe: three pieces, six
    products), "f32" (the fp32 pipe) or "bf16" (operands rounded to bf16, fp32 accumulation: BASELINE configs[3]'s "bf16 forward",
    config key `mlp_math: bf16`).  A dense_math() scope takes precedence over the DFOL_DENSE_MATH environment variable."""
    return _MATH_OVERRIDE or os.environ.get("DFOL_DENSE_MATH", "f16x2")


class dense_math:
    """with dense_math("bf16"): ...   - the arithmetic of linear_act / linear_gradx / linear_wgrad inside the block.  Autograd functions
    record the mode of their forward and re-enter it in backward."""

    def __init__(self, mode):
        if mode not in (None, "f16x2", "bf16x3", "f32", "bf16"):
            raise DfolError("unknown dense math mode %r" % (mode,))
        self.mode = mode

    def __enter__(self):
        global _MATH_OVERRIDE
        self.saved, _MATH_OVERRIDE = _MATH_OVERRIDE, (self.mode or _MATH_OVERRIDE)
        return self

    def __exit__(self, *exc):
        global _MATH_OVERRIDE
        _MATH_OVERRIDE = self.saved
        return False


def linear_act(x, weight, bias, act, out=None):
    """y = act(x @ weight.T + bias); x may be a column slice of a wider matrix (row stride = x.stride(0)).  Large products go through
    the bf16x3 split kernel (fp32 results, csrc/dfol_dense_split.hip) unless DFOL_DENSE_MATH=f32."""
    M, K = x.shape
    N = weight.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=F32, device=x.device)
    for t in (x, weight, out):
        if not t.is_cuda or t.dtype != F32 or t.stride(1) != 1:
            raise DfolError("linear_act needs fp32 GPU matrices with unit column stride")
    if N * K >= SPLIT_MIN_WEIGHT and K % 4 == 0 and x.stride(0) % 2 == 0 and _dp(x) % 8 == 0 and _dense_math() != "f32":
        return linear_act_split(x, weight, bias, act, out)
    call("dfol_linear_act_f32", _dp(x), x.stride(0), _dp(weight), weight.stride(0), _ptr(bias, F32, True),
         _dp(out), out.stride(0), M, N, K, act, _stream())
    return out


def lstm_cell_supported(KX, H):
    """The one-launch cell (lstm_cell / lstm_cell_tokens / lstm_cell_train) takes this input and state width: KX + H <= 496, the kernel's own rule."""
    return bool(load().dfol_lstm_cell_supported(int(KX), int(H)))


def calib_walk_supported(KX, H):
    """DFOL_OP_CALIB_WALK takes a calibrator of these widths: KX + 9 H + 2 <= 1024, the walk kernel's own rule."""
    return bool(load().dfol_calib_walk_supported(int(KX), int(H)))


def lstm_pointwise(igates, hgates, c):
    rows, H = c.shape
    hy, cy = torch.empty_like(c), torch.empty_like(c)
    call("dfol_lstm_pointwise_f32", _ptr(igates, F32), _ptr(hgates, F32), _ptr(c, F32), rows, H, _ptr(hy), _ptr(cy), _stream())
    return hy, cy


def lstm_cell(x, h, c, w_ih_t, w_hh_t, b_ih, b_hh):
    """nn.LSTMCell forward in one launch; w_ih_t = weight_ih.t().contiguous() [KX, 4H], w_hh_t likewise; fp32, unit column stride."""
    rows, H = c.shape
    hy, cy = torch.empty_like(c), torch.empty_like(c)
    call("dfol_lstm_cell_f32", _dp(x), x.stride(0), x.shape[1], _dp(h), h.stride(0), _ptr(c, F32), _ptr(w_ih_t, F32),
         w_ih_t.stride(0), _ptr(w_hh_t, F32), w_hh_t.stride(0), _ptr(b_ih, F32, True), _ptr(b_hh, F32, True), rows, H, _ptr(hy), _ptr(cy),
         _stream())
    return hy, cy


def lstm_cell_tokens(head, table, idx, h, c, w_ih_t, w_hh_t, b_ih, b_hh):
    """lstm_cell on rows built from tokens: x[p] = [head | table[idx[p]]] (zeros where idx[p] < 0) - calib_features + lstm_cell in one launch."""
    rows, H = c.shape
    hy, cy = torch.empty_like(c), torch.empty_like(c)
    call("dfol_lstm_cell_tokens_f32", _ptr(head, F32), head.numel(), _ptr(table, F32), table.shape[1], _ptr(idx, I32), _dp(h), h.stride(0), _ptr(c, F32),
         _ptr(w_ih_t, F32), w_ih_t.stride(0), _ptr(w_hh_t, F32), w_hh_t.stride(0), _ptr(b_ih, F32, True), _ptr(b_hh, F32, True), rows, H, _ptr(hy),
         _ptr(cy), _stream())
    return hy, cy


def lstm_cell_train(x, h, c, w_ih_t, w_hh_t, b_ih, b_hh):
    """lstm_cell that also returns the activated gates [rows, 4H] for lstm_cell_bwd."""
    rows, H = c.shape
    hy, cy = torch.empty_like(c), torch.empty_like(c)
    gates = torch.empty(rows, 4 * H, dtype=F32, device=c.device)
    call("dfol_lstm_cell_train_f32", _dp(x), x.stride(0), x.shape[1], _dp(h), h.stride(0), _ptr(c, F32), _ptr(w_ih_t, F32),
         w_ih_t.stride(0), _ptr(w_hh_t, F32), w_hh_t.stride(0), _ptr(b_ih, F32, True), _ptr(b_hh, F32, True), rows, H, _ptr(hy), _ptr(cy),
         _ptr(gates), _stream())
    return hy, cy, gates


def lstm_cell_bwd(gates, c_prev, c_new, d_hy, d_cy):
    """-> (d_gates [rows, 4H] w.r.t. the pre-activation gates, d_c_prev [rows, H]); d_hy or d_cy may be None."""
    rows, H = c_prev.shape
    dg = torch.empty(rows, 4 * H, dtype=F32, device=c_prev.device)
    dc = torch.empty(rows, H, dtype=F32, device=c_prev.device)
    call("dfol_lstm_cell_bwd_f32", _ptr(gates, F32), _ptr(c_prev, F32), _ptr(c_new, F32), _ptr(d_hy, F32, True), _ptr(d_cy, F32, True), rows, H,
         _ptr(dg), _ptr(dc), _stream())
    return dg, dc


def modulate_bwd(g_out, att, mods, pred_q, n_obj):
    P, NS = att.shape
    g_att = torch.empty_like(att)
    g_mods = torch.empty(P, 4, dtype=F32, device=att.device)
    call("dfol_modulate_bwd_f32", _ptr(g_out, F32), _ptr(att, F32), _ptr(mods, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), P, NS, _ptr(g_att),
         _ptr(g_mods), _stream())
    return g_att, g_mods


def box_positions(raw, obj, pos_col):
    call("dfol_box_positions_f32", _dp(raw), raw.stride(0), raw.shape[1], raw.shape[0], _dp(obj), obj.stride(0),
         pos_col, _stream())


def pair_features(obj, D, obj_off, pair_off, Q, max_n, pairs):
    out = torch.empty(pairs, 2 * D + 4, dtype=F32, device=obj.device)
    call("dfol_pair_features_f32", _dp(obj), obj.stride(0), D, _ptr(obj_off, I32), _ptr(pair_off, I64), Q, max_n,
         _dp(out), out.stride(0), _stream())
    return out


def pair_features_bwd(g, D, obj_off, pair_off, Q, max_n, objects):
    """The gradient of the object matrix [objects, D] from the pair matrix's g [pairs, >= 2 D], without atomics and in one fixed order
    (csrc/dfol_dropout.hip: pair_features_bwd_kernel)."""
    if g.dim() != 2 or g.dtype != F32 or g.shape[1] < 2 * D or (g.shape[0] > 1 and g.stride(1) != 1):
        raise DfolError("pair_features_bwd: g must be fp32 rows of unit column stride and at least 2 D = %d columns" % (2 * D))
    out = torch.empty(objects, D, dtype=F32, device=g.device)
    call("dfol_pair_features_bwd_f32", _dp(g), g.stride(0), D, _ptr(obj_off, I32), _ptr(pair_off, I64), Q, max_n, _dp(out), out.stride(0),
         _stream())
    return out


# ---- dropout: counter-based masks (csrc/dfol_dropout.hip) -----------------------------------------------------------------
# One 32-byte state per device: {seed u64, step u64, key u32[2], rank u32, pad} as four int64.  A forward that drops advances the step with one
# tiny launch - on the device, so a replayed graph draws new masks on every replay - and every Dropout of that forward takes the next SITE
# number: a host counter that starts at zero with the forward, hence the same at capture and at every replay.
_DROPOUT_STATES = {}                 # device index -> int64 [4] on that device
_DROPOUT_SEED = None                 # (seed, rank or None) of the last seed_dropout(), for states created after it
_DROPOUT_FORWARD = threading.local()  # .site: the next site number; .pending: this forward has not advanced the step yet
DROPOUT_TRACE = None                 # tests: a list that receives (site, shape, p) of every dropout launch of a forward


def philox4x32_10(counter, key):
    """Philox4x32-10 on the host (the kernels' generator, restated with Python integers): -> four 32-bit words."""
    c0, c1, c2, c3 = (int(v) & 0xFFFFFFFF for v in counter)
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _dropout_record(seed, rank):
    """The state at step 0 as four signed int64: its key is already the advance rule's for step 0."""
    seed, rank = int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank) & 0xFFFFFFFF
    k = philox4x32_10((0, 0, rank, 0), (seed & 0xFFFFFFFF, seed >> 32))
    signed = lambda v: v - (1 << 64) if v >= (1 << 63) else v
    return [signed(seed), 0, signed(k[0] | (k[1] << 32)), rank]


def _dropout_rank(rank=None):
    if rank is not None:
        return int(rank)
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def dropout_state(device=None):
    """The dropout stream state of `device` (default: the current one), created on first use from torch.initial_seed() and the process-group
    rank (0 without a group), or from the last seed_dropout()."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise DfolError("the HIP path needs tensors on the GPU (got device %s); there is no CPU fallback" % dev)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    state = _DROPOUT_STATES.get(index)
    if state is None:
        seed, rank = _DROPOUT_SEED if _DROPOUT_SEED is not None else (torch.initial_seed(), None)
        state = _DROPOUT_STATES[index] = torch.tensor(_dropout_record(seed, _dropout_rank(rank)), dtype=I64, device=torch.device("cuda", index))
    return state


def seed_dropout(seed, rank=None):
    """Restart the dropout streams of every device at step 0 of (seed, rank); rank=None: the process-group rank, 0 without a group.  States
    are rewritten in place: a captured graph keeps reading the same record."""
    global _DROPOUT_SEED
    _DROPOUT_SEED = (int(seed), rank)
    record = _dropout_record(seed, _dropout_rank(rank))
    for state in _DROPOUT_STATES.values():
        state.copy_(torch.tensor(record, dtype=I64))


def dropout_key(device=None):
    """The 8 bytes of the current key as a view of the state: what dfol_dropout_f32 reads at run time."""
    return dropout_state(device)[2:3]


def dropout_advance(device=None):
    """step += 1 and the step's key, one tiny launch on the current stream (a node of whatever capture is running)."""
    state = dropout_state(device)
    call("dfol_dropout_advance", _ptr(state, I64), _stream())


def dropout_forward_begins():
    """A forward starts (interpreter._forward): its Dropouts count their sites from zero, and the first of them advances the step - a forward
    without an active Dropout launches nothing."""
    _DROPOUT_FORWARD.site, _DROPOUT_FORWARD.pending = 0, True


def dropout_next_site(device):
    """-> the site number of the next Dropout of this forward; the forward's first one advances the device's step before it."""
    if getattr(_DROPOUT_FORWARD, "pending", False):
        _DROPOUT_FORWARD.pending = False
        dropout_advance(device)
    site = getattr(_DROPOUT_FORWARD, "site", 0)
    _DROPOUT_FORWARD.site = site + 1
    return site


def dropout(x, p, key, site, out=None, count=True):
    """y = x * mask(key, site) / (1 - p) over a matrix [rows, cols] of unit column stride and any row stride (dfol_dropout_f32); key: int64 [1]
    on the device - dropout_key() or a copy of it; out= may be x itself.  count=False: a read-out of the mask, not a use (no route counter)."""
    if x.dim() != 2 or x.dtype != F32 or not x.is_cuda or x.shape[1] < 1 or (x.shape[1] > 1 and x.stride(1) != 1):
        raise DfolError("dropout: x must be an fp32 device matrix [rows, cols >= 1] of unit column stride (got %s, strides %s, %s on %s)"
                        % (tuple(x.shape), tuple(x.stride()), x.dtype, x.device))
    if out is None:
        out = torch.empty(x.shape, dtype=F32, device=x.device)
    elif out.shape != x.shape or out.dtype != F32 or out.device != x.device or (x.shape[1] > 1 and out.stride(1) != 1):
        raise DfolError("dropout: out= must match x in shape, dtype and device, with unit column stride")
    rows, cols = x.shape
    if rows > 1 and x.stride(0) < cols:                      # (an expanded tensor - the gradient of a sum - has no rows of its own)
        x = x.contiguous()
    if rows > 1 and out.stride(0) < cols:
        raise DfolError("dropout: out= has overlapping rows (row stride %d < %d columns)" % (out.stride(0), cols))
    ldx = x.stride(0) if rows > 1 else cols
    ldy = out.stride(0) if rows > 1 else cols
    if count:
        note("dropout")
        if DROPOUT_TRACE is not None:
            DROPOUT_TRACE.append((int(site), (rows, cols), float(p)))
    call("dfol_dropout_f32", _dp(x), ldx, _dp(out), ldy, rows, cols, float(p), _ptr(key, I64), int(site), _stream())
    return out


def dropout_mask(shape, p, site, device=None, key=None):
    """The keep mask (bool) of (shape, p, site) under the device's current key - or under `key` -, by running the kernel on ones."""
    rows, cols = shape
    state = dropout_state(device)
    y = dropout(torch.ones(int(rows), int(cols), dtype=F32, device=state.device), p, state[2:3] if key is None else key, site, count=False)
    return y != 0


def attr_ll(hidden, emb_w, emb_b, obj_off, pred_q, pred_col, NS, default_ll=-30.0):
    P = pred_q.numel()
    ll = torch.empty(P, NS, dtype=F32, device=hidden.device)
    call("dfol_attr_ll_f32", _dp(hidden), hidden.stride(0), hidden.shape[1], _dp(emb_w), emb_w.stride(0),
         _ptr(emb_b, F32, True), _ptr(obj_off, I32), _ptr(pred_q, I32), _ptr(pred_col, I32), P, NS, default_ll, _ptr(ll), _stream())
    return ll


def attr_head_supported(hid1, hid2):
    """Shapes dfol_attr_head_h2_f32 takes (the full-size attribute network: 516 -> 256 -> 300): the pair kernel's second-layer shapes."""
    return pair_split_supported(hid1, hid2)


def attr_head_h2(pre1, w2_h2, b2, hid2, emb_w, emb_b, obj_off, pred_q, pred_col, NS, default_ll=-30.0):
    """attr_ll without the hidden table (csrc/dfol_pair_h2.hip: attr_head_h2_kernel): pre1 [O, hid1] = the attribute network's first-layer
    pre-activations, w2_h2 = pair_pack_w2_h2 of its second layer.  Same result layout as attr_ll; pred_q in any order."""
    P = pred_q.numel()
    ll = torch.empty(P, NS, dtype=F32, device=pre1.device)
    call("dfol_attr_head_h2_f32", _dp(pre1), pre1.stride(0), pre1.shape[1], _ptr(w2_h2, torch.float16), _ptr(b2, F32), hid2, _dp(emb_w), emb_w.stride(0),
         _ptr(emb_b, F32, True), _ptr(obj_off, I32), obj_off.numel() - 1, pre1.shape[0], _ptr(pred_q, I32), _ptr(pred_col, I32), P, NS, default_ll,
         _ptr(ll), _stream())
    return ll


# ---- scene-graph supervision: the fused all-concepts BCE (csrc/dfol_scene.hip) ---------------------------------------------------------
def scene_bce_supported(M, H, C):
    """Sizes the fused kernels take (dfol_scene_bce_supported); what they decline runs the tensor-op route of ops.scene_bce."""
    return bool(load().dfol_scene_bce_supported(int(M), int(H), int(C)))


def _scene_args(h, emb_w, emb_b, cols, target, weight):
    M, H = h.shape
    C = cols.numel()
    if emb_w.shape[1] != H or tuple(target.shape) != (M, C) or tuple(weight.shape) != (M, C):
        raise DfolError("scene_bce: h %s, emb_w %s, cols [%d], target %s, weight %s do not fit together"
                        % (tuple(h.shape), tuple(emb_w.shape), C, tuple(target.shape), tuple(weight.shape)))
    if h.dtype != F32 or emb_w.dtype != F32 or (M and h.stride(1) != 1) or emb_w.stride(1) != 1:
        raise DfolError("scene_bce: h and emb_w must be fp32 with unit column stride")
    return M, H, C, (_dp(h), h.stride(0) if M else H, M, H, _dp(emb_w), emb_w.stride(0), emb_w.shape[0], _ptr(emb_b, F32, True), _ptr(cols, I32), C,
                     _ptr(target, F32), _ptr(weight, F32))


def scene_bce_fwd(h, emb_w, emb_b, cols, target, weight, thr):
    """-> sums [3] = (loss, metric numerator, metric denominator) of the weighted BCE over emb_w's rows `cols` (dfol_scene_bce_fwd_f32)."""
    M, H, C, args = _scene_args(h, emb_w, emb_b, cols, target, weight)
    sums = torch.empty(3, dtype=F32, device=h.device)
    n = load().dfol_scene_bce_fwd_workspace(M, H, C)
    ws = torch.empty(n, dtype=F32, device=h.device) if n else None
    call("dfol_scene_bce_fwd_f32", *args, float(thr), _ptr(ws, F32, True), _ptr(sums), _stream())
    return sums


def scene_bce_bwd_rows(g, h, emb_w, emb_b, cols, target, weight):
    """-> dh [M, H] for the upstream gradient g of the loss (a device scalar): dfol_scene_bce_bwd_rows_f32."""
    M, H, C, args = _scene_args(h, emb_w, emb_b, cols, target, weight)
    dh = torch.empty(M, H, dtype=F32, device=h.device)
    call("dfol_scene_bce_bwd_rows_f32", _ptr(g, F32), *args, _ptr(dh), H, _stream())
    return dh


def scene_bce_bwd_cols(g, h, emb_w, emb_b, cols, target, weight):
    """-> (dE [C, H], db [C]) of emb_w's rows `cols` and their biases, compact: dfol_scene_bce_bwd_cols_f32."""
    M, H, C, args = _scene_args(h, emb_w, emb_b, cols, target, weight)
    dE, db = torch.empty(C, H, dtype=F32, device=h.device), torch.empty(C, dtype=F32, device=h.device)
    n = load().dfol_scene_bce_bwd_cols_workspace(M, H, C)
    ws = torch.empty(n, dtype=F32, device=h.device) if n else None
    call("dfol_scene_bce_bwd_cols_f32", _ptr(g, F32), *args, _ptr(ws, F32, True), _ptr(dE), _ptr(db), _stream())
    return dE, db


# ---- scene-graph supervision: the rows of the listed pairs (csrc/dfol_scene_pairs.hip) ----------------------------------------------------
def scene_pair_rows(obj, pair_s, pair_o):
    """-> [P, 2 D + 4] rows [obj[s], obj[o], dist, angle, sign(xo - xs), sign(yo - ys)] of the listed pairs (dfol_scene_pair_rows_f32); obj [O, D]
    fp32 with the box in its last four columns, pair_s / pair_o int32 [P] rows of obj (the kernel clamps an index, the caller has checked it)."""
    if obj.dim() != 2 or obj.dtype != F32 or obj.shape[1] < 4 or (obj.shape[0] > 1 and obj.stride(1) != 1):
        raise DfolError("scene_pair_rows: obj must be fp32 rows of unit column stride and at least the four box columns")
    O, D = obj.shape
    P = pair_s.numel()
    if pair_o.numel() != P or (P and O == 0):
        raise DfolError("scene_pair_rows: %d subjects, %d objects of the pairs, %d object rows" % (P, pair_o.numel(), O))
    out = torch.empty(P, 2 * D + 4, dtype=F32, device=obj.device)
    if P:
        call("dfol_scene_pair_rows_f32", _dp(obj), obj.stride(0), O, D, _ptr(pair_s, I32), _ptr(pair_o, I32), P, _ptr(out), out.stride(0), _stream())
    return out


def scene_pair_rows_bwd(g, D, seg_off, slot, objects):
    """-> d_obj [objects, D]: the sum of g's [P, >= 2 D] subject / object blocks per object in the order of the by-object list (seg_off
    [objects + 1], slot [2 P], int32: data.scene_pair_csr), without atomics (dfol_scene_pair_rows_bwd_f32).  The geometry columns of g are not
    propagated: they come from the box columns, which feed no parameter."""
    if g.dim() != 2 or g.dtype != F32 or g.shape[1] < 2 * D or (g.shape[0] > 1 and g.stride(1) != 1):
        raise DfolError("scene_pair_rows_bwd: g must be fp32 rows of unit column stride and at least 2 D = %d columns" % (2 * D))
    P = g.shape[0]
    if seg_off.numel() != objects + 1 or slot.numel() != 2 * P:
        raise DfolError("scene_pair_rows_bwd: seg_off [%d] and slot [%d] do not describe %d objects and %d pairs" % (seg_off.numel(), slot.numel(), objects, P))
    out = torch.empty(objects, D, dtype=F32, device=g.device)
    if objects:
        call("dfol_scene_pair_rows_bwd_f32", _dp(g), g.stride(0) if P else 2 * D, P, D, _ptr(seg_off, I32), _ptr(slot, I32), objects, _ptr(out),
             out.stride(0), _stream())
    return out


def pair_ll(uv, hid1, pos, wg, w2, b2, emb_w, emb_b, n_obj, obj_off, max_n, req_col, req_tile, req_orient, tiles, default_ll=-30.0,
            hid2=None):
    """req_col / req_tile: int32 [K, Q]; req_orient: uint8 [K, Q] or None; tiles: [T, NS, NS] written in place.
    w2 may be allocated with more (zero) rows than hid2 = the layer's true output width."""
    K, Q = req_col.shape
    NS = tiles.shape[1]
    hid2 = w2.shape[0] if hid2 is None else hid2
    call("dfol_pair_ll_f32", _dp(uv), uv.stride(0), hid1, _dp(pos), pos.stride(0), _ptr(wg, F32), _dp(w2),
         w2.stride(0), w2.shape[0], _ptr(b2, F32), hid2, _dp(emb_w), emb_w.stride(0), _ptr(emb_b, F32, True), _ptr(n_obj, I32),
         _ptr(obj_off, I32), Q, max_n, _ptr(req_col, I32), _ptr(req_tile, I32), _ptr(req_orient, U8, True), K, NS, default_ll,
         _ptr(tiles, F32), _stream())
    return tiles


PACKED_W2_ROWS, PACKED_W2_CHUNK = 320, 16
SPLIT_W2_CHUNK_BYTES = 3 * 320 * 32 * 2                        # three bf16 pieces of 20 column tiles x 32 k
LOG2E = 1.4426950408889634

# The forms in which the pair network's second layer W2 reaches the fused pair kernel, one row each: the executor's code (include/dfol_vqa.h:
# DFOL_PAIR_*), the names of this module's pack and launch wrappers, the image's dtype, whether the kernel takes U | V in units of ln 2
# (multiplied by log2 e), whether it can write bf16 tiles.  A new form is one row here, one pack kernel and one entry point.
PairKind = _collections.namedtuple("PairKind", "code pack launch dtype ln2_units bf16_tiles")
PAIR_KINDS = {
    "f16x2": PairKind(3, "pair_pack_w2_h2", "pair_ll_h2", torch.float16, True, True),
    "f16": PairKind(4, "pair_pack_w2_h1", "pair_ll_h1", torch.float16, True, True),
    "bf16x3": PairKind(2, "pair_pack_w2_split", "pair_ll_split", torch.bfloat16, False, True),
    "packed": PairKind(1, "pair_pack_w2", "pair_ll_packed", F32, False, True),
    "plain": PairKind(0, None, "pair_ll", F32, False, False),      # (no image: the zero-padded weight itself)
}


def pair_split_supported(hid1, hid2):
    """Shapes dfol_pair_ll_split_f32 takes (the full-size oracle: 256 -> 300)."""
    return hid1 % 32 == 0 and 0 < hid1 <= 256 and 256 < hid2 <= 320


def pair_kind_for(math, hid1, hid2):
    """The PAIR_KINDS row that evaluates a HID1 -> HID2 second layer under the pair arithmetic `math` (pair_math()): the packed layout of the
    occupancy-2 kernel (csrc/dfol_pair.hip) where the shape allows it and DFOL_PAIR_PACKED is not 0; on a full-size layer fp32 results from
    the fp16 matrix pipe ("f16x2": two pieces per operand, three products; "f16": opt-in reduced precision, the hi pieces alone, one
    product per MAC on the same kernel body: csrc/dfol_pair_h2.hip) or from the bf16 pipe ("bf16x3": three pieces, six products:
    csrc/dfol_pair_split.hip); "f32" keeps the fp32 matrix pipe."""
    if not (hid1 % PACKED_W2_CHUNK == 0 and hid1 <= 256 and hid2 <= PACKED_W2_ROWS) or os.environ.get("DFOL_PAIR_PACKED", "1") == "0":
        return "plain"
    return "packed" if math == "f32" or not pair_split_supported(hid1, hid2) else math


def pair_tiles_bf16_ok(hid1, hid2):
    """bf16 tile storage (config key relation_tile_dtype: bf16) is possible: the pair kernels that write bf16 tiles are the packed ones over a
    second layer of more than 256 rows.  The weight's shape decides, not its values or the arithmetic."""
    return hid2 > 256 and PAIR_KINDS[pair_kind_for("f32", hid1, hid2)].bf16_tiles


def _pair_pack(entry, dtype, nbytes, w2, hid2):
    out = torch.empty(nbytes // dtype.itemsize, dtype=dtype, device=w2.device)
    call(entry, _ptr(w2, F32), w2.stride(0), w2.shape[0] if hid2 is None else hid2, w2.shape[1], _ptr(out, dtype), _stream())
    return out


def _pair_ll_image(entry, dtype, scale_uv, uv, hid1, pos, wg, image, b2, hid2, emb_w, emb_b, n_obj, obj_off, max_n, req_col, req_tile, req_orient,
                   tiles, default_ll):
    """The four entry points that take a packed image of W2 (same argument list).  scale_uv: `uv` is still in natural units and the kernel
    takes it multiplied by log2(e)."""
    if scale_uv:
        uv = uv * LOG2E
    K, Q = req_col.shape
    NS = tiles.shape[1]
    bf16 = tiles.dtype == torch.bfloat16
    call(entry, _dp(uv), uv.stride(0), hid1, _dp(pos), pos.stride(0), _ptr(wg, F32), _ptr(image, dtype), _ptr(b2, F32), hid2, _dp(emb_w),
         emb_w.stride(0), _ptr(emb_b, F32, True), _ptr(n_obj, I32), _ptr(obj_off, I32), Q, max_n, _ptr(req_col, I32), _ptr(req_tile, I32),
         _ptr(req_orient, U8, True), K, NS, default_ll, TILE_BF16 if bf16 else TILE_F32, _ptr(tiles, torch.bfloat16 if bf16 else F32), _stream())
    return tiles


def pair_pack_w2(w2, hid2=None):
    """W2 [HID2(+padding), HID1] -> the packed image dfol_pair_ll_packed_f32 reads ([HID1/16][320][16], swizzled)."""
    return _pair_pack("dfol_pair_pack_w2_f32", F32, (w2.shape[1] // PACKED_W2_CHUNK) * PACKED_W2_ROWS * PACKED_W2_CHUNK * 4, w2, hid2)


def pair_ll_packed(uv, hid1, pos, wg, w2_packed, b2, hid2, emb_w, emb_b, n_obj, obj_off, max_n, req_col, req_tile, req_orient, tiles,
                   default_ll=-30.0):
    """As pair_ll, with the second layer packed by pair_pack_w2 (hid1 % 16 == 0, hid2 <= 320).  `tiles` may be bfloat16
    (TILE_BF16 storage for relate_one_fwd_bf16; needs hid2 > 256 and NS % 8 == 0)."""
    return _pair_ll_image("dfol_pair_ll_packed_f32", F32, False, uv, hid1, pos, wg, w2_packed, b2, hid2, emb_w, emb_b, n_obj, obj_off, max_n,
                          req_col, req_tile, req_orient, tiles, default_ll)


def pair_pack_w2_split(w2, hid2=None):
    """W2 [HID2(+padding), HID1] -> the bf16x3 image dfol_pair_ll_split_f32 reads (SPLIT_W2_CHUNK_BYTES per 32 k, swizzled)."""
    return _pair_pack("dfol_pair_pack_w2_bf16x3", torch.bfloat16, (w2.shape[1] // 32) * SPLIT_W2_CHUNK_BYTES, w2, hid2)


def pair_ll_split(uv, hid1, pos, wg, w2_split, b2, hid2, emb_w, emb_b, n_obj, obj_off, max_n, req_col, req_tile, req_orient, tiles,
                  default_ll=-30.0):
    """As pair_ll_packed, with the second layer split by pair_pack_w2_split: bf16 matrix pipes, fp32 results."""
    return _pair_ll_image("dfol_pair_ll_split_f32", torch.bfloat16, False, uv, hid1, pos, wg, w2_split, b2, hid2, emb_w, emb_b, n_obj, obj_off,
                          max_n, req_col, req_tile, req_orient, tiles, default_ll)


def pair_pack_w2_h2(w2, hid2=None):
    """W2 [HID2(+padding), HID1] -> the fp16x2 image dfol_pair_ll_h2_f32 reads (rows scaled by powers of two, two fp16 pieces, swizzled;
    the per-column multipliers of the epilogue behind the chunks)."""
    return _pair_pack("dfol_pair_pack_w2_f16x2", torch.float16, load().dfol_pair_w2_f16x2_bytes(w2.shape[1]), w2, hid2)


def pair_ll_h2(uv, hid1, pos, wg, w2_h2, b2, hid2, emb_w, emb_b, n_obj, obj_off, max_n, req_col, req_tile, req_orient, tiles,
               default_ll=-30.0, uv_prescaled=False):
    """As pair_ll_split, with the second layer split by pair_pack_w2_h2: fp16 matrix pipe, three products per fp32 product, fp32 results
    (csrc/dfol_pair_h2.hip).  Ordered pairs only: `tiles` must be pre-filled with default_ll (diagonal and padding keep the fill).
    The kernel takes U | V MULTIPLIED BY log2(e) (include/dfol_vqa.h): uv_prescaled=True says `uv` already is (the oracle scales the stacked
    first-layer weight once per weight version); otherwise it is scaled here, with one extra pass over it (tests, lab scripts)."""
    return _pair_ll_image("dfol_pair_ll_h2_f32", torch.float16, not uv_prescaled, uv, hid1, pos, wg, w2_h2, b2, hid2, emb_w, emb_b, n_obj, obj_off,
                          max_n, req_col, req_tile, req_orient, tiles, default_ll)


def pair_pack_w2_h1(w2, hid2=None):
    """W2 [HID2(+padding), HID1] -> the one-piece fp16 image dfol_pair_ll_h1_f32 reads: the hi pieces of pair_pack_w2_h2's image (same row
    scales, swizzle and tail), 20 KB per 32 k."""
    return _pair_pack("dfol_pair_pack_w2_f16", torch.float16, load().dfol_pair_w2_f16_bytes(w2.shape[1]), w2, hid2)


def pair_ll_h1(uv, hid1, pos, wg, w2_h1, b2, hid2, emb_w, emb_b, n_obj, obj_off, max_n, req_col, req_tile, req_orient, tiles,
               default_ll=-30.0, uv_prescaled=False):
    """As pair_ll_h2 in the opt-in reduced-precision mode (pair_math "f16"): operands rounded to fp16, ONE product per MAC, fp32
    accumulation, on the image of pair_pack_w2_h1.  Same arguments, same units of `uv`, same saturation report."""
    return _pair_ll_image("dfol_pair_ll_h1_f32", torch.float16, not uv_prescaled, uv, hid1, pos, wg, w2_h1, b2, hid2, emb_w, emb_b, n_obj, obj_off,
                          max_n, req_col, req_tile, req_orient, tiles, default_ll)


def pair_train_fwd_h2(uv_scaled, hid1, pos, wg, w2_h2, b2, hid2, n_obj, obj_off, pair_off, max_n, pairs, e_rows=None, req_row=None):
    """The forward of a train step's pair MLP in one launch (include/dfol_vqa.h: dfol_pair_train_fwd_h2_f32).  uv_scaled: U | V times log2(e).
    -> (Z [pairs, hid1], pre2 [pairs, hid2], geo [pairs, 4], x [K, pairs] or None).  req_row [K, Q] int32 (device): the row of e_rows
    every image's reader uses in slot k (-1: none)."""
    Q = n_obj.shape[0]
    dev = uv_scaled.device
    z = torch.empty(pairs, hid1, dtype=F32, device=dev)
    pre2 = torch.empty(pairs, hid2, dtype=F32, device=dev)
    geo = torch.empty(pairs, 4, dtype=F32, device=dev)
    K = 0 if req_row is None else req_row.shape[0]
    x = torch.zeros(K, pairs, dtype=F32, device=dev) if K else None
    call("dfol_pair_train_fwd_h2_f32", _dp(uv_scaled), uv_scaled.stride(0), hid1, _dp(pos), pos.stride(0), _ptr(wg, F32), _ptr(w2_h2, torch.float16), _ptr(b2, F32),
         hid2, None if e_rows is None else _dp(e_rows), 0 if e_rows is None else e_rows.stride(0), _ptr(n_obj, I32), _ptr(obj_off, I32), _ptr(pair_off, torch.int64),
         Q, max_n, _ptr(req_row, I32, True), K, _ptr(z), _ptr(pre2), pre2.stride(0), _ptr(geo), _ptr(x, F32, True), pairs, _stream())
    return z, pre2, geo, x


PAIR_MATH_MODES = ("f16x2", "bf16x3", "f32", "f16")
_PAIR_MATH_OVERRIDE = None


def pair_math():
    """Arithmetic of the fused pair kernel's second layer: "f16x2" (default: two fp16 pieces, three products), "bf16x3" (round 3's: three
    bf16 pieces, six products) or "f32" (the fp32 matrix pipe) - all with fp32 results - or "f16": REDUCED precision, operands rounded to
    fp16 and one product per MAC (a third of the matrix work; opt-in only, inference only: config key `pair_math: f16`).  A
    pair_math_scope() takes precedence over the DFOL_PAIR_MATH environment variable, which takes precedence over the rule: "bf16x3" when
    the dense math is, otherwise "f16x2" (`mlp_math: bf16` does not imply "f16")."""
    # (`mlp_math: bf16x3` / dense_math("bf16x3") - the remedy for activations beyond fp16's range - moves the pair kernel along with the dense layers)
    m = _PAIR_MATH_OVERRIDE or os.environ.get("DFOL_PAIR_MATH") or ("bf16x3" if _dense_math() == "bf16x3" else "f16x2")
    if m not in PAIR_MATH_MODES:
        raise DfolError("DFOL_PAIR_MATH=%r (f16x2, bf16x3, f32, or f16: reduced precision, one fp16 product per MAC)" % m)
    return m


class pair_math_scope:
    """with pair_math_scope("f16"): ...   - the pair kernel's arithmetic inside the block (None: no change), as dense_math for the dense layers."""

    def __init__(self, mode):
        if mode is not None and mode not in PAIR_MATH_MODES:
            raise DfolError("unknown pair math mode %r (%s)" % (mode, ", ".join(PAIR_MATH_MODES)))
        self.mode = mode

    def __enter__(self):
        global _PAIR_MATH_OVERRIDE
        self.saved, _PAIR_MATH_OVERRIDE = _PAIR_MATH_OVERRIDE, (self.mode or _PAIR_MATH_OVERRIDE)
        return self

    def __exit__(self, *exc):
        global _PAIR_MATH_OVERRIDE
        _PAIR_MATH_OVERRIDE = self.saved
        return False


# ---- training path of the pair MLP (csrc/dfol_pair_train.hip) ------------------------------------------------------
def pair_train_supported(hid1, hid2, max_n):
    lpr = hid1 // 4
    return hid1 % 4 == 0 and 16 <= hid1 <= 1024 and lpr & (lpr - 1) == 0 and lpr <= 256 and hid2 <= 512 and max_n <= 16 * (1024 // lpr)


def bf16_store(hid1, hid2):
    """True when a train step keeps its per-pair activations (Z, pre2 and their gradients) in bfloat16: the bf16 mode (dense_math('bf16'),
    config key mlp_math: bf16) unless DFOL_BF16_STORE=0, widths the 8-byte-row kernels take, and a second layer large enough for the
    matrix-pipe kernel (the same SPLIT_MIN_WEIGHT rule as the fp32-storage products)."""
    return _dense_math() == "bf16" and os.environ.get("DFOL_BF16_STORE", "1") != "0" and hid1 % 4 == 0 and hid2 % 4 == 0 and hid2 >= 16 and \
        hid1 * hid2 >= SPLIT_MIN_WEIGHT


def pair_hidden1_fwd(u, v, pos, wg, obj_off, pair_off, n_obj, max_n, pairs, store=F32):
    """z [pairs, HID1] = ELU(U[s] + V[o] + Wg geo) and geo [pairs, 4]; u, v [O, HID1] (row stride a multiple of 4), pos [O, >=4] view.
    store = torch.bfloat16: z is stored in bfloat16 (rounded to nearest even)."""
    Q, hid1 = n_obj.shape[0], u.shape[1]
    z = torch.empty(pairs, hid1, dtype=store, device=u.device)
    geo = torch.empty(pairs, 4, dtype=F32, device=u.device)
    call("dfol_pair_hidden1_fwd_bf16" if store == torch.bfloat16 else "dfol_pair_hidden1_fwd_f32", _dp(u), u.stride(0), _dp(v), v.stride(0), _dp(pos), pos.stride(0), _ptr(wg, F32),
         _ptr(obj_off, I32), _ptr(pair_off, torch.int64), _ptr(n_obj, I32), Q, max_n, hid1, _ptr(z), _ptr(geo), _stream())
    return z, geo


def pair_hidden1_bwd(dz, z, geo, obj_off, pair_off, n_obj, max_n, total_obj, joined=False, uvw=None):
    """(dU [O, HID1], dV [O, HID1], dWg [HID1, 4]) from dZ; deterministic (no atomics).  joined: dU and dV are the two column halves of one
    [O, 2 HID1] buffer (the gradient of a joined U|V product - visual_oracle._pair_pre2_autograd).  uvw = (U, V, Wg), fp32 storage: z is
    rebuilt from them inside the kernel instead of being read (`z` may be None; DFOL_H1B_RECOMPUTE=0 reads it)."""
    Q, hid1 = n_obj.shape[0], dz.shape[1]
    if joined:
        duv = torch.zeros(total_obj, 2 * hid1, dtype=F32, device=dz.device)
        du, dv = duv[:, :hid1], duv[:, hid1:]
    else:
        du = torch.zeros(total_obj, hid1, dtype=F32, device=dz.device)        # objects of images with < 2 objects get no row written
        dv = torch.zeros(total_obj, hid1, dtype=F32, device=dz.device)
    part = torch.zeros(Q, hid1, 4, dtype=F32, device=dz.device)
    if hidden1_recompute(uvw, dz, max_n, hid1) or z is None:
        u, v, wg = uvw
        call("dfol_pair_hidden1_bwd_recompute_f32", _ptr(dz, F32), _dp(u), u.stride(0), _dp(v), v.stride(0), _ptr(wg, F32), _ptr(geo, F32), _ptr(obj_off, I32),
             _ptr(pair_off, torch.int64), _ptr(n_obj, I32), Q, max_n, hid1, _dp(du), du.stride(0), _dp(dv), dv.stride(0), _ptr(part), _stream())
        return (duv, None, part.sum(0)) if joined else (du, dv, part.sum(0))
    if z.dtype == torch.bfloat16 and dz.dtype != torch.bfloat16:
        dz = dz.to(torch.bfloat16)
    call("dfol_pair_hidden1_bwd_bf16" if z.dtype == torch.bfloat16 else "dfol_pair_hidden1_bwd_f32", _ptr(dz, z.dtype), _ptr(z, z.dtype), _ptr(geo, F32), _ptr(obj_off, I32), _ptr(pair_off, torch.int64),
         _ptr(n_obj, I32), Q, max_n, hid1, _dp(du), du.stride(0), _dp(dv), dv.stride(0), _ptr(part), _stream())
    return (duv, None, part.sum(0)) if joined else (du, dv, part.sum(0))


def hidden1_recompute(uvw, dz, max_n, hid1):
    """True when the pair layer's first-stage backward rebuilds z instead of reading it (fp32 storage, the image fits the 512-thread form)."""
    return uvw is not None and dz.dtype == F32 and os.environ.get("DFOL_H1B_RECOMPUTE", "1") != "0" and \
        bool(load().dfol_pair_hidden1_bwd_recompute_supported(int(max_n), int(hid1)))


def pair_logit_fwd(p2, e_rows, be_rows, pred_off, max_rows):
    """max_rows: the largest number of rows a predicate owns (host value; the launch is one row tile grid per predicate)."""
    rows, P = p2.shape[0], e_rows.shape[0]
    x = torch.empty(rows, dtype=F32, device=p2.device)
    call("dfol_pair_logit_fwd_bf16" if p2.dtype == torch.bfloat16 else "dfol_pair_logit_fwd_f32", _dp(p2), p2.stride(0), p2.shape[1], _dp(e_rows), e_rows.stride(0), _ptr(be_rows, F32, True),
         _ptr(pred_off, torch.int64), P, rows, int(max_rows), _ptr(x), _stream())
    return x


def pair_logit_bwd(dx, p2, e_rows, pred_off, need_bias=True):
    P = e_rows.shape[0]
    dp2 = torch.empty_like(p2)
    de = torch.empty(P, p2.shape[1], dtype=F32, device=p2.device)
    dbe = torch.empty(P, dtype=F32, device=p2.device) if need_bias else None
    call("dfol_pair_logit_bwd_bf16" if p2.dtype == torch.bfloat16 else "dfol_pair_logit_bwd_f32", _ptr(dx, F32), _dp(p2), p2.stride(0), p2.shape[1], _dp(e_rows), e_rows.stride(0),
         _ptr(pred_off, torch.int64), P, _dp(dp2), dp2.stride(0), _dp(de), de.stride(0), _ptr(dbe, F32, True), _stream())
    return dp2, de, dbe


def pair_head_fused_supported(hid1, hid2):
    """Widths the fused head backward takes (csrc/dfol_pair_wgrad.hip, pair_wgrad_fused_kernel: all of dW2 in one workgroup's accumulators)."""
    return hid1 % 4 == 0 and hid2 % 4 == 0 and 16 <= hid2 <= 320 and 4 <= hid1 <= 256


def tall_enabled():
    """The persistent one-workgroup-per-CU form of the tall products (csrc/dfol_dense_tall.hip); DFOL_TALL=0 keeps the tiled kernels."""
    return os.environ.get("DFOL_TALL", "1") != "0"


def linear_tall_supported(M, N, K):
    return tall_enabled() and bool(load().dfol_linear_tall_supported(M, N, K))


def linear_tall_h2(x, weight, bias, row_pred=None, e_rows=None):
    """y [M, N] = x @ weight.T + bias on two fp16 pieces, persistent form (M >= 16384, N <= 320): bit for bit linear_act_split's result.
    With row_pred / e_rows also the logit layer's partial sums x_part [4, M] (see linear_logit_h2) -> (y, x_part), else (y, None).
    A bfloat16 x (the bf16 mode's stored activations): one bf16 piece per operand, bfloat16 y - bit for bit dfol_linear_act_bf16_bf16."""
    M, K = x.shape
    N = weight.shape[0]
    if x.dtype == torch.bfloat16:
        y = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        xp = torch.empty(4, M, dtype=F32, device=x.device) if row_pred is not None else None
        call("dfol_linear_tall_bf16_bf16", _dp(x), x.stride(0), _ptr(linear_pack_w_split(weight, False, 1), torch.bfloat16), _ptr(bias, F32, True), _dp(y),
             y.stride(0), M, N, K, _ptr(row_pred, I32, True), _ptr(e_rows, F32, True), 0 if e_rows is None else e_rows.stride(0), _ptr(xp, F32, True),
             0 if xp is None else xp.stride(0), _stream())
        return y, xp
    y = torch.empty(M, N, dtype=F32, device=x.device)
    xp = torch.empty(4, M, dtype=F32, device=x.device) if row_pred is not None else None
    call("dfol_linear_tall_h2_f32", _dp(x), x.stride(0), _ptr(linear_pack_w_split(weight, False, 2), torch.bfloat16), _ptr(bias, F32, True), _dp(y),
         y.stride(0), M, N, K, _ptr(row_pred, I32, True), _ptr(e_rows, F32, True), 0 if e_rows is None else e_rows.stride(0), _ptr(xp, F32, True),
         0 if xp is None else xp.stride(0), _stream())
    return y, xp


def linear_logit_h2(x, weight, bias, row_pred, e_rows):
    """(y [M, N] = x @ weight.T + bias, x_part [2 ceil(N / 128), M]) on two fp16 pieces: the second layer of the pair MLP and, from the same
    pass, the logit layer's partial sums x_part[s][r] = sum over the s-th 64-column half block of Sigmoid(y[r, j]) e_rows[row_pred[r], j]."""
    M, K = x.shape
    N = weight.shape[0]
    y = torch.empty(M, N, dtype=F32, device=x.device)
    xp = torch.empty(2 * ((N + 127) // 128), M, dtype=F32, device=x.device)
    call("dfol_linear_logit_h2_f32", _dp(x), x.stride(0), _ptr(linear_pack_w_split(weight, False, 2), torch.bfloat16), _ptr(bias, F32, True), _dp(y),
         y.stride(0), M, N, K, _ptr(row_pred, I32), _ptr(e_rows, F32), e_rows.stride(0), _ptr(xp), xp.stride(0), _stream())
    return y, xp


def pair_dz_tall_bf16(dx, p2, e_rows, row_pred, w2, dz_out=None):
    """dz [M, HID1] bfloat16 (+)= dpre2 W2 for bfloat16-stored p2 = pre2 [M, HID2] (the bf16 mode): dpre2 rebuilt in the kernel and rounded to
    bfloat16 as dfol_pair_logit_bwd_bf16 stores it, one bf16 piece per operand - bit for bit that kernel followed by the bf16 product."""
    M, H2 = p2.shape
    H1 = w2.shape[1]
    dz = dz_out if dz_out is not None else torch.empty(M, H1, dtype=torch.bfloat16, device=p2.device)
    call("dfol_pair_dz_tall_bf16", _dp(p2), p2.stride(0), _ptr(dx, F32), _ptr(row_pred, I32), _ptr(e_rows, F32), e_rows.stride(0),
         _ptr(linear_pack_w_split(w2, True, 1), torch.bfloat16), _dp(dz), dz.stride(0), M, H1, H2, 1 if dz_out is not None else 0, _stream())
    return dz


def pair_wgrad_sums_bf16(dx, p2, z, e_rows, pred_off, row_pred, need_bias=True):
    """(dW2 [HID2, HID1], dE [P, HID2], dbe [P] or None, db2 [HID2]), all fp32, from bfloat16-stored p2 = pre2 and z (the bf16 mode): the weight
    gradient with dpre2 rebuilt in the kernel (rounded to bfloat16 as dfol_pair_logit_bwd_bf16 stores it) and the logit layer's sums from the
    same pass.  Every predicate must own >= 64 pair rows or none."""
    M, H2 = p2.shape
    H1 = z.shape[1]
    P = e_rows.shape[0]
    dev = p2.device
    ws = torch.empty(load().dfol_pair_wgrad_fused_sums_workspace(M, H2, H1, P), dtype=F32, device=dev)
    dw = torch.empty(H2, H1, dtype=F32, device=dev)
    de = torch.empty(P, H2, dtype=F32, device=dev)
    dbe = torch.empty(P, dtype=F32, device=dev) if need_bias else None
    db2 = torch.empty(H2, dtype=F32, device=dev)
    call("dfol_pair_wgrad_fused_sums_bf16", _dp(p2), p2.stride(0), _ptr(dx, F32), _ptr(row_pred, I32), _ptr(pred_off, torch.int64), P, _ptr(e_rows, F32),
         e_rows.stride(0), _dp(z), z.stride(0), M, H2, H1, _ptr(ws), _ptr(dw), _ptr(de), de.stride(0), _ptr(dbe, F32, True), _ptr(db2), _stream())
    return dw, de, dbe, db2


def pair_head_sums(dx, p2, e_rows, pred_off, need_bias=True):
    """(dE [P, HID2], dbe [P] or None, dB2 [P, HID2]) of one use of the hidden layer: the sums of the logit layer's backward; dB2's rows add
    up to the second layer's bias gradient.  dpre2 itself is not written (pair_head_products rebuilds it where it is consumed)."""
    H2, P = p2.shape[1], e_rows.shape[0]
    de = torch.empty(P, H2, dtype=F32, device=p2.device)
    dbe = torch.empty(P, dtype=F32, device=p2.device) if need_bias else None
    db2p = torch.empty(P, H2, dtype=F32, device=p2.device)
    call("dfol_pair_logit_bwd_sums_f32", _ptr(dx, F32), _dp(p2), p2.stride(0), H2, _ptr(e_rows, F32), e_rows.stride(0), _ptr(pred_off, torch.int64), P,
         _ptr(de), de.stride(0), _ptr(dbe, F32, True), _ptr(db2p), db2p.stride(0), _stream())
    return de, dbe, db2p


def pair_head_products(dx, p2, z, w2, e_rows, pred_off, row_pred, need_dz=True, need_dw=True, dz_out=None, sums=False, need_bias=True):
    """(dz [M, HID1], dW2 [HID2, HID1]) of one use: dz (+)= dpre2 W2 and dW2 = dpre2^T z with dpre2[r, j] = dx[r] E[row_pred[r], j] h (1 - h),
    h = Sigmoid(p2[r, j]), produced inside the two kernels.  dz_out: a previous use's dz to add to (in place).  row_pred [M] int32,
    non-decreasing; pred_off [P + 1] int64.
    sums=True (needs need_dw; every predicate owns >= 64 rows or none): the weight-gradient pass also returns the logit layer's sums -
    (dz, dW2, dE [P, HID2], dbe [P] or None, db2 [HID2]) - and pair_head_sums' pass over p2 is not needed."""
    M, H2 = p2.shape
    H1 = z.shape[1]
    dev = p2.device
    emax = e_rows.abs().amax(1)
    dz = dw = scale = None
    if need_dz:
        dz = dz_out if dz_out is not None else torch.empty(M, H1, dtype=F32, device=dev)
        if linear_tall_supported(M, H1, H2):
            ws = torch.empty(2 * M + 4, dtype=F32, device=dev)
            scale = ws[2 * M + 1:2 * M + 3]                    # {S, 1 / S} of the launch's largest bound: the weight gradient's scale, from the same pass
            call("dfol_pair_dz_tall_f32", _dp(p2), p2.stride(0), _ptr(dx, F32), _ptr(row_pred, I32), _ptr(e_rows, F32), e_rows.stride(0), _ptr(emax, F32),
                 _ptr(linear_pack_w_split(w2, True, 2), torch.bfloat16), _dp(dz), dz.stride(0), M, H1, H2, 1 if dz_out is not None else 0, _ptr(ws),
                 _stream())
        else:
            call("dfol_pair_dz_fused_f32", _dp(p2), p2.stride(0), _ptr(dx, F32), _ptr(row_pred, I32), _ptr(e_rows, F32), e_rows.stride(0), _ptr(emax, F32),
             _ptr(linear_pack_w_split(w2, True, 2), torch.bfloat16), _dp(dz), dz.stride(0), M, H1, H2, 1 if dz_out is not None else 0, _stream())
    if need_dw and scale is None:
        # one power of two for the weight gradient's fp16 pieces: S max_r |dx[r]| emax[p(r)] / 4 in [2^13, 2^14) (device-side: no sync)
        bound = (dx.abs() * emax.index_select(0, row_pred)).amax() * 0.25
        _, ex = torch.frexp(bound)
        ok = torch.isfinite(bound) & (bound > 0)
        sexp = torch.where(ok, (14 - ex).clamp(-100, 100), torch.zeros_like(ex)).to(F32)
        scale = torch.stack([torch.exp2(sexp), torch.exp2(-sexp)]).contiguous()
    if need_dw and sums:
        P = e_rows.shape[0]
        ws = torch.empty(load().dfol_pair_wgrad_fused_sums_workspace(M, H2, H1, P), dtype=F32, device=dev)
        dw = torch.empty(H2, H1, dtype=F32, device=dev)
        de = torch.empty(P, H2, dtype=F32, device=dev)
        dbe = torch.empty(P, dtype=F32, device=dev) if need_bias else None
        db2 = torch.empty(H2, dtype=F32, device=dev)
        call("dfol_pair_wgrad_fused_sums_f32", _dp(p2), p2.stride(0), _ptr(dx, F32), _ptr(row_pred, I32), _ptr(pred_off, torch.int64), P, _ptr(e_rows, F32),
             e_rows.stride(0), _dp(scale), _dp(z), z.stride(0), M, H2, H1, _ptr(ws), _ptr(dw), _ptr(de), de.stride(0), _ptr(dbe, F32, True), _ptr(db2),
             _stream())
        return dz, dw, de, dbe, db2
    if need_dw:
        ws = torch.empty(load().dfol_pair_wgrad_fused_workspace(M, H2, H1), dtype=F32, device=dev)
        dw = torch.empty(H2, H1, dtype=F32, device=dev)
        call("dfol_pair_wgrad_fused_f32", _dp(p2), p2.stride(0), _ptr(dx, F32), _ptr(row_pred, I32), _ptr(pred_off, torch.int64), _ptr(e_rows, F32),
             e_rows.stride(0), _dp(scale), _dp(z), z.stride(0), M, H2, H1, _ptr(ws), _ptr(dw), _stream())
    return dz, dw


PAIR_DZ_MULTI_MAX = 4


def pair_dz_tall_multi(dx_list, p2, e_rows_list, row_pred, w2, dz_out=None):
    """dz (+)= dpre2 W2 for SEVERAL readers of one hidden layer in one pass (csrc/dfol_dense_tall.hip, dfol_pair_dz_tall_multi_f32):
    dpre2[r, j] = h (1 - h) sum_k dx_k[r] E_k[row_pred[r], j].  The readers share row_pred [M] (int32) and P; up to PAIR_DZ_MULTI_MAX per launch
    (more: further launches that add).  -> dz [M, HID1]."""
    M, H2 = p2.shape
    H1 = w2.shape[1]
    dev = p2.device
    dz = dz_out if dz_out is not None else torch.empty(M, H1, dtype=F32, device=dev)
    acc = dz_out is not None
    wp = linear_pack_w_split(w2, True, 2)
    for i in range(0, len(dx_list), PAIR_DZ_MULTI_MAX):
        dxs, es = dx_list[i:i + PAIR_DZ_MULTI_MAX], e_rows_list[i:i + PAIR_DZ_MULTI_MAX]
        nr, P = len(dxs), es[0].shape[0]
        dx = torch.stack([d.reshape(-1) for d in dxs]).contiguous()
        E = torch.stack([e if e.is_contiguous() else e.contiguous() for e in es]).contiguous()      # [nr, P, HID2]
        emax = E.abs().amax(2).contiguous()
        ws = torch.empty((nr + 1) * M, dtype=F32, device=dev)
        call("dfol_pair_dz_tall_multi_f32", _dp(p2), p2.stride(0), _ptr(dx, F32), dx.stride(0), nr, _ptr(row_pred, I32), _ptr(E, F32), E.stride(1), P,
             _ptr(emax, F32), _ptr(wp, torch.bfloat16), _dp(dz), dz.stride(0), M, H1, H2, 1 if acc else 0, _ptr(ws), _stream())
        acc = True
    return dz


def pair_wgrad_multi(dx_list, p2, z, e_rows_list, pred_off, row_pred):
    """dW2 [HID2, HID1] = sum_k dpre2_k^T z for SEVERAL readers of one hidden layer in one pass over p2 = pre2 and z (csrc/dfol_pair_wgrad.hip,
    dfol_pair_wgrad_fused_multi_f32): dpre2_k[r, j] = dx_k[r] E_k[row_pred[r], j] h (1 - h).  The readers share row_pred [M] (int32, non-decreasing),
    pred_off [P + 1] (int64) and P; up to PAIR_DZ_MULTI_MAX per launch (more: further launches, added in order).  The launch's scale comes from
    the device (dfol_pair_wgrad_multi_scale_f32: no sync); the readers' own sums are pair_head_sums'."""
    M, H2 = p2.shape
    H1 = z.shape[1]
    dev = p2.device
    ws = torch.empty(load().dfol_pair_wgrad_fused_workspace(M, H2, H1), dtype=F32, device=dev)
    dw = None
    for i in range(0, len(dx_list), PAIR_DZ_MULTI_MAX):
        dxs, es = dx_list[i:i + PAIR_DZ_MULTI_MAX], e_rows_list[i:i + PAIR_DZ_MULTI_MAX]
        nr, P = len(dxs), es[0].shape[0]
        dx = torch.stack([d.reshape(-1) for d in dxs]).contiguous()
        E = torch.stack([e if e.is_contiguous() else e.contiguous() for e in es]).contiguous()      # [nr, P, HID2]
        emax = E.abs().amax(2).contiguous()
        scale = torch.empty(4, dtype=F32, device=dev)
        call("dfol_pair_wgrad_multi_scale_f32", _ptr(dx, F32), dx.stride(0), nr, _ptr(row_pred, I32), _ptr(emax, F32), P, M, _ptr(scale), _stream())
        part = torch.empty(H2, H1, dtype=F32, device=dev)
        call("dfol_pair_wgrad_fused_multi_f32", _dp(p2), p2.stride(0), _ptr(dx, F32), dx.stride(0), nr, _ptr(row_pred, I32), _ptr(pred_off, torch.int64),
             _ptr(E, F32), E.stride(1), P, _ptr(scale), _dp(z), z.stride(0), M, H2, H1, _ptr(ws), _ptr(part), _stream())
        dw = part if dw is None else dw + part
    return dw


def pair_head_bwd(dx, p2, z, w2, e_rows, pred_off, row_pred, need_bias=True, dz_out=None, sums=False):
    """The backward of x = logit(Sigmoid(z W2^T + b2)) for ONE use of the hidden layer, without dpre2 in memory:
    -> (dz [M, HID1], dW2 [HID2, HID1], db2 [HID2], dE [P, HID2], dbe [P] or None).  sums=True: the sums from the weight-gradient pass
    (every predicate >= 64 rows or none), else from their own pass over p2."""
    e_rows = e_rows if e_rows.is_contiguous() else e_rows.contiguous()
    if sums:
        dz, dw, de, dbe, db2 = pair_head_products(dx, p2, z, w2, e_rows, pred_off, row_pred, dz_out=dz_out, sums=True, need_bias=need_bias)
        return dz, dw, db2, de, dbe
    de, dbe, db2p = pair_head_sums(dx, p2, e_rows, pred_off, need_bias)
    dz, dw = pair_head_products(dx, p2, z, w2, e_rows, pred_off, row_pred, dz_out=dz_out)
    return dz, dw, db2p.sum(0), de, dbe


def capturing():
    """True while a graph capture records through this module (keeping(): GraphedForward / GraphedTrainStep)."""
    return _KEEP is not None


# ---- backward wrappers (deterministic: no atomics; pred_q non-decreasing) --------------------------------------------
def require_sorted(pred_q, what):
    """The deterministic backward kernels find a question's predicates by binary search in pred_q (csrc/dfol_logic_bwd.hip,
    dfol_pred_range), so the map must be non-decreasing - every map the operators build is (flatten_list order).  An unsorted map would
    silently drop gradient contributions, so it is refused here.  Checked once per tensor object (one device->host read), remembered on
    the tensor; the maps come out of content-keyed caches, so a train loop pays once per distinct map."""
    flag = getattr(pred_q, "_dfol_sorted", None)
    if flag is None:
        if _KEEP is not None:
            raise DfolError("%s: the predicate -> question map has not been checked for order and a graph capture is recording (the check reads "
                            "the device): build the map through BatchWorld.pred_q / host_util.upload, or run one eager step first" % what)
        flag = bool(pred_q.numel() < 2 or bool((pred_q[1:] >= pred_q[:-1]).all().item()))
        try:
            pred_q._dfol_sorted = flag
        except Exception:
            pass
    if not flag:
        raise DfolError("%s: the predicate -> question map must be non-decreasing (the deterministic backward finds a question's predicates "
                        "by binary search); sort the predicates by question, as util.flatten_list does" % what)


def reduce_by_question(src, pred_q, n_obj, Q):
    """out[q] = sum of src[p] over the predicates p of question q (src [P, NS] -> [Q, NS])."""
    require_sorted(pred_q, "reduce_by_question")
    P, NS = src.shape
    out = torch.empty(Q, NS, dtype=F32, device=src.device)
    call("dfol_reduce_by_question_f32", _ptr(src, F32), _ptr(pred_q, I32), _ptr(n_obj, I32, True), P, Q, NS, _ptr(out), _stream())
    return out


def filter_bwd(g_out, ll, pred_q, n_obj, neg, active, Q, need_prior=True, need_ll=True):
    require_sorted(pred_q, "filter_bwd")
    P, NS = ll.shape
    g_prior = torch.empty(Q, NS, dtype=F32, device=ll.device) if need_prior else None
    g_ll = torch.empty(P, NS, dtype=F32, device=ll.device) if need_ll else None
    call("dfol_filter_bwd_f32", _ptr(g_out, F32), _ptr(ll, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), _ptr(neg, U8, True),
         0 if neg is None else 1, _ptr(active, U8, True), P, Q, NS, _ptr(g_prior, F32, True), _ptr(g_ll, F32, True), _stream())
    return g_prior, g_ll


def relate_bwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, neg, active, g_post_s, g_post_o, orientation,
               lone_forall_identity, need_prior=True, need_tile=True):
    if need_prior:
        require_sorted(pred_q, "relate_bwd")
    P, NS = tile.shape[0], tile.shape[1]
    Q = prior_s.shape[0]
    pp_s = torch.empty(P, NS, dtype=F32, device=tile.device) if need_prior else None      # per predicate
    pp_o = torch.empty(P, NS, dtype=F32, device=tile.device) if need_prior else None
    g_tile = torch.empty(P, NS, NS, dtype=F32, device=tile.device) if need_tile else None
    call("dfol_relate_bwd_f32", _ptr(prior_s, F32), _ptr(prior_o, F32), _ptr(tile, F32), _ptr(pred_q, I32), _ptr(n_obj, I32),
         _ptr(quant_s, F32), _ptr(quant_o, F32), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True),
         _ptr(g_post_s, F32, True), _ptr(g_post_o, F32, True), P, NS, orientation, 1 if lone_forall_identity else 0,
         _ptr(pp_s, F32, True), _ptr(pp_o, F32, True), _ptr(g_tile, F32, True), _stream())
    if need_prior:
        return reduce_by_question(pp_s, pred_q, None, Q), reduce_by_question(pp_o, pred_q, None, Q), g_tile
    return None, None, g_tile


def filter_gate_bwd(g_out, att_in, ll, pred_q, n_obj, gate, neg, active):
    """-> (g_prior [Q, NS], g_ll [P, NS], g_gate [18]); the parameter sums are taken in a fixed order (no atomics)."""
    require_sorted(pred_q, "filter_gate_bwd")
    P, NS = ll.shape
    pp = torch.empty(P, NS, dtype=F32, device=ll.device)                                  # per predicate
    g_ll = torch.empty(P, NS, dtype=F32, device=ll.device)
    g_gate = torch.empty(18, dtype=F32, device=ll.device)
    scratch = torch.empty(max(1, load().dfol_filter_gate_bwd_scratch(P, NS)), dtype=F32, device=ll.device)
    call("dfol_filter_gate_bwd_f32", _ptr(g_out, F32), _ptr(att_in, F32), _ptr(ll, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), _ptr(neg, U8, True),
         0 if neg is None else 1, _ptr(active, U8, True), P, NS, _ptr(gate, F32), _ptr(scratch), _ptr(pp), _ptr(g_ll), _ptr(g_gate), _stream())
    return reduce_by_question(pp, pred_q, None, att_in.shape[0]), g_ll, g_gate


def relate_gate_bwd(prior_s, prior_o, tile, pred_q, n_obj, quant_s, quant_o, gate_s, gate_o, neg, active, g_post_s, g_post_o, orientation,
                    lone_forall_identity):
    """-> (g_prior_s [Q, NS], g_prior_o [Q, NS], g_tile [P, NS, NS], g_gate_s [18], g_gate_o [18])."""
    require_sorted(pred_q, "relate_gate_bwd")
    P, NS = tile.shape[0], tile.shape[1]
    if NS > 1024:
        raise DfolError("relate_gate_bwd: images of %d object slots; the gated Relate backward keeps its row and column sums in LDS and takes at most 1024" % NS)
    Q = prior_s.shape[0]
    dev = tile.device
    pp_s = torch.empty(P, NS, dtype=F32, device=dev)
    pp_o = torch.empty(P, NS, dtype=F32, device=dev)
    g_tile = torch.empty(P, NS, NS, dtype=F32, device=dev)
    gg_s = torch.empty(18, dtype=F32, device=dev)
    gg_o = torch.empty(18, dtype=F32, device=dev)
    scratch = torch.empty(max(1, 36 * P), dtype=F32, device=dev)
    call("dfol_relate_gate_bwd_f32", _ptr(prior_s, F32), _ptr(prior_o, F32), _ptr(tile, F32), _ptr(pred_q, I32), _ptr(n_obj, I32),
         _ptr(quant_s, F32), _ptr(quant_o, F32), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True),
         _ptr(g_post_s, F32, True), _ptr(g_post_o, F32, True), P, NS, orientation, 1 if lone_forall_identity else 0, _ptr(gate_s, F32),
         _ptr(gate_o, F32), _ptr(scratch), _ptr(pp_s), _ptr(pp_o), _ptr(g_tile), _ptr(gg_s), _ptr(gg_o), _stream())
    return reduce_by_question(pp_s, pred_q, None, Q), reduce_by_question(pp_o, pred_q, None, Q), g_tile, gg_s, gg_o


def is_identity_map(pred_q, Q):
    """True when pred_q is known, without reading the device, to map predicate p to question p (BatchWorld._ident carries the mark)."""
    return bool(getattr(pred_q, "_dfol_identity", False)) and pred_q.numel() == Q


def relate_keep_gate_bwd(g_post, x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, gate_s, gate_o, neg, active,
                         lone_forall_identity, identity=None):
    """-> (g_x [P, NS], g_prev [Q, NS], g_tile [P, NS, NS] subjects along rows, g_gate_s [18], g_gate_o [18]).  identity: pred_q maps predicate p
    to question p, so g_prev needs no reduction (None: is_identity_map)."""
    P, NS = _keep_gate_check("relate_keep_gate_bwd", tile, x_is_subject)
    if NS > 1024:
        raise DfolError("relate_keep_gate_bwd: images of %d object slots; the gated Relate backward keeps its row and column sums in LDS and takes at most 1024" % NS)
    Q = prev_att.shape[0]
    if identity is None:
        identity = is_identity_map(pred_q, Q)
    if not identity:
        require_sorted(pred_q, "relate_keep_gate_bwd")
    dev = tile.device
    g_x = torch.empty(P, NS, dtype=F32, device=dev)
    pp = torch.empty(P, NS, dtype=F32, device=dev)                                          # per predicate
    g_tile = torch.empty(P, NS, NS, dtype=F32, device=dev)
    gg_s = torch.empty(18, dtype=F32, device=dev)
    gg_o = torch.empty(18, dtype=F32, device=dev)
    scratch = torch.empty(max(1, 36 * P), dtype=F32, device=dev)
    call("dfol_relate_keep_gate_bwd_f32", _ptr(g_post, F32), _ptr(x_att, F32), _ptr(prev_att, F32), _ptr(tile, F32), _ptr(pred_q, I32),
         _ptr(n_obj, I32), _ptr(quant_prev, F32), _ptr(x_is_subject, U8), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True),
         P, NS, 1 if lone_forall_identity else 0, _ptr(gate_s, F32), _ptr(gate_o, F32), _ptr(scratch), _ptr(g_x), _ptr(pp), _ptr(g_tile),
         _ptr(gg_s), _ptr(gg_o), _stream())
    return g_x, (pp if identity else reduce_by_question(pp, pred_q, None, Q)), g_tile, gg_s, gg_o


def relate_keep_bwd(g_post, x_att, prev_att, tile, pred_q, n_obj, quant_prev, x_is_subject, neg, active, lone_forall_identity, identity=None):
    """-> (g_x [P, NS], g_prev [Q, NS], g_tile [P, NS, NS] subjects along rows).  identity: pred_q maps predicate p to question p, so g_prev
    needs no reduction (None: is_identity_map)."""
    P, NS = _keep_check("relate_keep_bwd", x_att, prev_att, tile, x_is_subject)
    if NS > RELATE_KEEP_BWD_MAX_NS:
        raise DfolError("relate_keep_bwd: images of %d object slots; the one-posterior Relate backward keeps its row and column sums in LDS and "
                        "takes at most %d" % (NS, RELATE_KEEP_BWD_MAX_NS))
    if tuple(g_post.shape) != (P, NS):
        raise DfolError("relate_keep_bwd: cotangent of shape %s for a posterior of [%d, %d]" % (tuple(g_post.shape), P, NS))
    Q = prev_att.shape[0]
    if identity is None:
        identity = is_identity_map(pred_q, Q)
    if not identity:
        require_sorted(pred_q, "relate_keep_bwd")
    args = (_ptr(g_post, F32), _ptr(x_att, F32), _ptr(prev_att, F32), _ptr(tile, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), _ptr(quant_prev, F32),
            _ptr(x_is_subject, U8), _ptr(neg, U8, True), 0 if neg is None else 1, _ptr(active, U8, True), P, NS, 1 if lone_forall_identity else 0)
    dev = tile.device
    g_x = torch.empty(P, NS, dtype=F32, device=dev)
    pp = torch.empty(P, NS, dtype=F32, device=dev)                                          # per predicate
    g_tile = torch.empty(P, NS, NS, dtype=F32, device=dev)
    call("dfol_relate_keep_bwd_f32", *args, _ptr(g_x), _ptr(pp), _ptr(g_tile), _stream())
    return g_x, (pp if identity else reduce_by_question(pp, pred_q, None, Q)), g_tile


def quantify_bwd(g_lp, att, quant, pred_q, n_obj):
    P, NS = att.shape
    g_att = torch.empty(P, NS, dtype=F32, device=att.device)
    call("dfol_quantify_bwd_f32", _ptr(g_lp, F32), _ptr(att, F32), _ptr(quant, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), P, NS,
         _ptr(g_att), _stream())
    return g_att


def attr_gather_bwd(g_ll, obj_off, pred_q, pred_col, table_shape):
    require_sorted(pred_q, "attr_gather_bwd")
    P, NS = g_ll.shape
    Q = obj_off.numel() - 1
    g_table = torch.zeros(table_shape, dtype=F32, device=g_ll.device)
    call("dfol_attr_gather_bwd_f32", _ptr(g_ll, F32), _ptr(obj_off, I32), _ptr(pred_q, I32), _ptr(pred_col, I32), P, Q, NS, _ptr(g_table),
         g_table.stride(0), _stream())
    return g_table


def rel_gather_bwd(g_tile, pair_off, n_obj, pred_q, pred_col, orientation, table_shape):
    require_sorted(pred_q, "rel_gather_bwd")
    P, NS = g_tile.shape[0], g_tile.shape[1]
    Q = n_obj.numel()
    g_table = torch.zeros(table_shape, dtype=F32, device=g_tile.device)
    call("dfol_rel_gather_bwd_f32", _ptr(g_tile, F32), _ptr(pair_off, I64), _ptr(n_obj, I32), _ptr(pred_q, I32), _ptr(pred_col, I32),
         P, Q, NS, orientation, _ptr(g_table), g_table.stride(0), _stream())
    return g_table


def attr_ll_bwd(g, hidden, emb_w, emb_b, obj_off, pred_q, pred_col, need_hidden=True, need_emb=True, need_bias=True):
    """-> (d_hidden [O, H], dE [P, H] per predicate, db [P] per predicate); deterministic (no atomics)."""
    require_sorted(pred_q, "attr_ll_bwd")
    P, NS = g.shape
    O, H = hidden.shape
    Q = obj_off.numel() - 1
    gx = torch.empty(P, NS, dtype=F32, device=g.device)
    d_hidden = torch.empty(O, H, dtype=F32, device=g.device) if need_hidden else None
    dE = torch.empty(P, H, dtype=F32, device=g.device) if need_emb else None
    db = torch.empty(P, dtype=F32, device=g.device) if need_bias else None
    call("dfol_attr_ll_bwd_f32", _ptr(g, F32), _dp(hidden), hidden.stride(0), H, _dp(emb_w), emb_w.stride(0), _ptr(emb_b, F32, True),
         _ptr(obj_off, I32), _ptr(pred_q, I32), _ptr(pred_col, I32), P, Q, NS, _ptr(gx), _ptr(d_hidden, F32, True), H,
         _ptr(dE, F32, True), H, _ptr(db, F32, True), _stream())
    return d_hidden, dE, db


def option_normalize_bwd(g_y, y, seg_off, pred_q, n_obj, NS):
    g_x = torch.empty_like(g_y)
    call("dfol_option_normalize_bwd_f32", _ptr(g_y, F32), _ptr(y, F32), _ptr(seg_off, I32), seg_off.numel() - 1, _ptr(pred_q, I32),
         _ptr(n_obj, I32), NS, y.dim() - 1, _ptr(g_x), _stream())
    return g_x


def select_rows(x, y, flags_u8):
    """out[p] = flags[p] ? x[p] : y[p] (rows of floats; flags uint8 [P] on the device)."""
    x, y = x.contiguous(), y.contiguous()
    out = torch.empty_like(x)
    call("dfol_select_rows_f32", _ptr(x, F32), _ptr(y, F32), _ptr(flags_u8, U8), x.shape[0], x.shape[1], _ptr(out), _stream())
    return out


def attention_modulations(fs, bs, weight, bias):
    """Sigmoid(Linear([fs | bs])) of the attention-output network in one launch; fs / bs [P, S] (either may be None = zeros), weight [N, 2 S]."""
    ref = fs if fs is not None else bs
    P, S = ref.shape
    N = weight.shape[0]
    w = weight.detach()
    w = w if w.stride(1) == 1 else w.contiguous()
    out = torch.empty(P, N, dtype=F32, device=ref.device)
    call("dfol_attention_modulations_f32", _ptr(None if fs is None else fs.contiguous(), F32, True), _ptr(None if bs is None else bs.contiguous(), F32, True),
         _dp(w), w.stride(0), _ptr(None if bias is None else bias.detach(), F32, True), P, S, N, _ptr(out), _stream())
    return out


def modulate(att, mods, pred_q, n_obj):
    P, NS = att.shape
    out = torch.empty_like(att)
    call("dfol_modulate_f32", _ptr(att, F32), _ptr(mods, F32), _ptr(pred_q, I32), _ptr(n_obj, I32), P, NS, _ptr(out), _stream())
    return out
