"""The program interpreter (reference: src/nsvqa/nn/interpreter/batch_base_interpreter.py,
batch_gqa_interpreter.py, data_parallel.py:15-50 and the featurizer of
src/nsvqa/data/batch_gqa_boxfeatures_pipeline.py:193-281)."""

import inspect
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops as L
from . import gqa_ops as gqa
from .fol_types import BatchAttentionState, BatchVariableSet, BatchWorld, QuestionType
from .host_util import keeping, reverse_dependencies, upload


def gather_results(outputs, target_device=None, is_cuda=True):
    """Concatenate per-ProgramBatch results (data_parallel.py:15-50)."""
    if outputs[0]['type'] == QuestionType.SCENE_GRAPH:       # data_parallel.py:16-30: each table along dim 0, each answer array along axis 0
        from .visual_oracle import SceneLikelihood
        n_answers = len(outputs[0]['answer'])
        return {'answer': [np.concatenate([o['answer'][i] for o in outputs], axis=0) for i in range(n_answers)],
                'log_probability': SceneLikelihood.concat([o['log_probability'] for o in outputs]), 'options': outputs[0]['options'],
                'variable_set': None, 'type': outputs[0]['type'], 'cumulative_loss': sum(o['cumulative_loss'] for o in outputs),
                'variable_sets_num': sum(o['variable_sets_num'] for o in outputs), 'answer_log_probability': []}
    log_probability = torch.cat([o['log_probability'].reshape(-1) for o in outputs]) if len(outputs) > 1 else \
        outputs[0]['log_probability'].reshape(-1)
    answer = [a for o in outputs for a in o['answer']]
    answer_log_probability = [a for o in outputs for a in o['answer_log_probability']]
    if outputs[0]['type'] == QuestionType.QUERY:
        options = [x for o in outputs for x in o['options']]
    else:
        options = outputs[0]['options']
    return {'answer': answer, 'log_probability': log_probability, 'options': options, 'variable_set': None, 'type': outputs[0]['type'],
            'cumulative_loss': sum(o['cumulative_loss'] for o in outputs), 'variable_sets_num': sum(o['variable_sets_num'] for o in outputs),
            'answer_log_probability': answer_log_probability}


def featurizer_trains(net):
    """A gradient reaches the featurizer network's weights under the current grad mode: its output is then part of the graph, not a constant."""
    return torch.is_grad_enabled() and any(p.requires_grad for p in net.parameters())


def active_dropout(net):
    """The first nn.Dropout of a featurizer network (a RegularMLP) that drops under the current mode (training, p > 0), or None."""
    seq = getattr(net, "_network", None)
    for m in (() if seq is None else seq):
        if isinstance(m, nn.Dropout) and m.training and m.p > 0:
            return m
    return None


def store_layers_of(net, F, M, bf16_ld=None):
    """-> (the featurizer network's layers [(Linear, activation)], None) when its first product can read M rows of a feature store of width F in
    place - the two-piece fp16 arithmetic on a weight of the split kernels' size, the store's width, a shape the wide kernel takes and pays for
    (dfol_linear_wide_supported) - else (None, why not).  ONE predicate for the direct route (M = the batch's rows), the executor and the store's
    cache builder (M = its row block).  bf16_ld: the store's table is bfloat16 with this row stride (feature_dtype="bf16") - then the question is
    the bf16 arithmetic's: `mlp_math: bf16`, whose first product rounds a feature to the value the table holds, on a weight of the split
    kernels' size, any M (dfol_linear_rows_bf16t_supported).  With DFOL_STORE_BF16_DIRECT=1 a bf16 table also says yes to the two-piece fp16
    arithmetic of a featurizer that does not train, where the wide kernel splits the table's rows in place
    (dfol_linear_wide_rows_bf16t_supported: the fp32 table's question and rows the kernel can load); the dense arithmetic tells the two apart.
    With DFOL_STORE_BF16_TRAIN=1 the same holds for a featurizer that TRAINS in that arithmetic (the forward is the same product; the caller,
    BatchGQABoxFeaturizer._store_train_layers, asks for the weight gradient's form besides: dfol_linear_wgrad_rows_bf16t_x3_supported)."""
    from . import _lib, native_exec
    if net is None or getattr(net, "_network", None) is None or not hasattr(net, "output_width"):
        return None, "the featurizer has no network"
    layers = native_exec._layers(net._network)
    if not layers:
        return None, "the featurizer network is not a chain of Linear layers and activations (or a Dropout is active)"
    h2 = bf16_ld is not None and _lib._dense_math() == "f16x2" and (_lib.store_bf16_train() if featurizer_trains(net) else _lib.store_bf16_direct())
    want = "f16x2" if bf16_ld is None or h2 else "bf16"
    if _lib._dense_math() != want:
        return None, "the dense arithmetic is %r, not %r" % (_lib._dense_math(), want)
    w = layers[0][0].weight
    N, K = w.shape
    if K != F:
        return None, "the featurizer's first layer takes %d features, the store holds %d" % (K, F)
    if h2:
        if N * K < _lib.SPLIT_MIN_WEIGHT or w.stride(1) != 1 or not _lib.linear_wide_rows_bf16t_supported(M, N, K, bf16_ld):
            return None, "the wide kernel does not take a %d -> %d product over %d rows of a bf16 table of row stride %d" % (K, N, M, bf16_ld)
        return layers, None
    if bf16_ld is not None:
        if N * K < _lib.SPLIT_MIN_WEIGHT or w.stride(1) != 1 or not _lib.linear_rows_bf16t_supported(N, K, bf16_ld):
            return None, "the bf16 mode's tiled kernel does not take a %d -> %d product over a bf16 table of row stride %d" % (K, N, bf16_ld)
        return layers, None
    if N * K < _lib.SPLIT_MIN_WEIGHT or w.stride(1) != 1 or not _lib.linear_wide_supported(M, N, K):
        return None, "the wide kernel does not take a %d -> %d product over %d rows" % (K, N, M)
    return layers, None


class BatchGQABoxFeaturizer(nn.Module):
    """Object and pair features of a scene (batch_gqa_boxfeatures_pipeline.py:193-281).

    featurize_scene keeps the reference's return dict.  The pair matrix [pairs, 2(D+4)+4] is the reference's
    layout; it is materialised only because compute_all_log_likelihood_2 asks for it (full cached tables)."""

    def __init__(self, featurizer_network=None):
        super(BatchGQABoxFeaturizer, self).__init__()
        self._featurizer_network = featurizer_network

    def _store_layers(self, rows):
        """The featurizer's layers [(Linear, activation)] when its FIRST product can read a direct feature store's rows in place (a StoreRows):
        inference, the two-piece fp16 arithmetic on a weight of the split kernels' size, the store's feature width, and a shape the wide kernel
        takes and pays for (dfol_linear_wide_supported - the same question the tiled kernel asks before it forwards there, so either route runs
        the same kernel body on the same rows).  None: the caller materialises the matrix and goes on as ever."""
        net = self._featurizer_network
        if rows.O == 0 or (net is not None and featurizer_trains(net)):
            return None
        return store_layers_of(net, rows.store.F, rows.O, getattr(rows, "bf16_ld", None))[0]

    def _store_train_layers(self, rows):
        """The same layers when the featurizer TRAINS and its first layer can run as visual_oracle.StoreRowsLinear: forward as on the inference
        route (so store_layers_of decides - an active Dropout, another arithmetic, a narrow first layer or a small batch say no), and a weight
        gradient that reads the table through src_row too (dfol_linear_wgrad_rows_supported; dz is a contiguous [O, N]).  A bf16 table in the
        default arithmetic (DFOL_STORE_BF16_TRAIN=1, what store_layers_of admitted) asks dfol_linear_wgrad_rows_bf16t_x3_supported.  None: the matrix."""
        from . import _lib
        net = self._featurizer_network
        if rows.O == 0 or rows.table is None or net is None or not featurizer_trains(net) or active_dropout(net) is not None:
            return None
        layers = store_layers_of(net, rows.store.F, rows.O, getattr(rows, "bf16_ld", None))[0]
        if layers is None:
            return None
        N, K = layers[0][0].weight.shape
        bf16t = getattr(rows, "bf16_ld", None) is not None
        if bf16t and _lib._dense_math() == "f16x2":
            return layers if _lib.linear_wgrad_rows_bf16t_x3_supported(N, K, N, rows.table.stride(0)) else None
        return layers if _lib.linear_wgrad_rows_supported(N, K, N, rows.table.stride(0), bf16_table=bf16t) else None

    def _cached_objects(self, rows):
        """The object matrix of a `featurized` store's batch from the store's cached featurizer rows (feature_store.DeviceFeatureStore.featurize:
        built on first use, rebuilt once when a weight's version has changed), or None: a store without a cache, a featurizer that trains under
        the current grad mode (its output is no constant), one with an active Dropout (its output differs from step to step), or a network the
        cache cannot be built for - the caller goes on as for a direct store."""
        net = self._featurizer_network
        if not getattr(rows.store, "featurized", False) or net is None or featurizer_trains(net):
            return None
        if active_dropout(net) is not None:                   # (the cached rows were never dropped: a frozen featurizer in train() drops anew)
            return None
        cache = rows.store.cached_for(net, build=True)
        return None if cache is None else rows.objects(cache)

    def featurize_scene(self, device, objects_list, batch_index, meta_data, world_geometry=None):
        from . import _lib
        from .feature_store import StoreRows
        if isinstance(objects_list, StoreRows):
            obj = self._cached_objects(objects_list)
            if obj is not None:
                # a frozen featurizer over a featurized store: its rows were computed once, the batch's are gathered beside their box positions
                _lib.note("feature_store_featurized")
                return self._with_pairs(obj, obj.shape[1], objects_list.O, world_geometry)
            layers = self._store_layers(objects_list)
            if layers is not None:
                # the index form of a store-backed batch: the first product gathers the store's rows through src_row, the rest is as below
                rows, net = objects_list, self._featurizer_network
                D = net.output_width() + 4
                obj = torch.empty(rows.O, D, dtype=torch.float32, device=device)
                x = None
                # (a bf16 table: the bf16 mode's product, or - DFOL_STORE_BF16_DIRECT=1 - the default arithmetic's over the table's own rows)
                bf16_h2 = getattr(rows, "bf16_ld", None) is not None and _lib._dense_math() == "f16x2"      # (what store_layers_of admitted)
                certified = bf16_h2 and rows.store._f16_exact is True                                       # (two products: the same bits)
                first = _lib.linear_wide_rows if getattr(rows, "bf16_ld", None) is None else \
                    (_lib.linear_wide_rows_bf16t if bf16_h2 else _lib.linear_rows_bf16t)
                for k, (lin, act) in enumerate(layers):
                    out = obj[:, :D - 4] if k == len(layers) - 1 else None
                    x = first(rows.table, rows.src_row, lin.weight, lin.bias, act, out, **({"store": rows.store} if certified else {})) if k == 0 else \
                        L.linear_act(x, lin.weight, lin.bias, act, out)
                L.box_positions(rows.box6, obj, D - 4)
                _lib.note("feature_store_direct")
                if bf16_h2:
                    _lib.note("feature_store_direct_bf16_h2")
                return self._with_pairs(obj, D, rows.O, world_geometry)
            layers = self._store_train_layers(objects_list)
            if layers is not None:
                # a featurizer that trains: the first layer's forward AND weight gradient read the store's rows through src_row (the features
                # are data: no gradient goes to the table), later layers are ordinary trained dense layers; the bits of the matrix route
                from .visual_oracle import StoreRowsLinear
                rows = objects_list
                lin, act = layers[0]
                bf16_x3 = getattr(rows, "bf16_ld", None) is not None and _lib._dense_math() == "f16x2"     # (DFOL_STORE_BF16_TRAIN=1: what was admitted)
                f = StoreRowsLinear.apply(lin.weight, lin.bias, rows.table, rows.src_row, act, bf16_x3 and rows.store._f16_exact is True)
                for lin, act in layers[1:]:
                    f = L.linear_act(f, lin.weight, lin.bias, act)
                D = f.size(1) + 4
                obj = torch.empty(rows.O, D, dtype=torch.float32, device=device)
                obj[:, :D - 4] = f
                L.box_positions(rows.box6, obj, D - 4)
                _lib.note("feature_store_direct")                 # (a batch whose featurizer read the store in place ...
                _lib.note("feature_store_direct_train")           # ... and, of those, one whose weight gradient will too)
                if bf16_x3:
                    _lib.note("feature_store_direct_train_bf16_x3")
                return self._with_pairs(obj, D, rows.O, world_geometry)
            objects_list = objects_list.materialize()             # a Dropout that drops, another arithmetic, a narrow first layer, a small batch: the matrix
            _lib.note("feature_store_direct_materialized")
        object_num = objects_list.size()[0]
        raw_cols = objects_list.size()[1]
        feat = objects_list[:, :raw_cols - 6]                    # a strided view: the GEMM reads it in place
        net = self._featurizer_network
        direct = net is not None and getattr(net, "_network", None) is not None and hasattr(net, "output_width") and feat.is_cuda and \
            not (torch.is_grad_enabled() and (feat.requires_grad or any(p.requires_grad for p in net.parameters())))
        if direct:
            # inference: the featurizer's last layer writes straight into the object matrix (row stride D), no [O, D - 4] copy
            D = net.output_width() + 4
            obj = torch.empty(object_num, D, dtype=torch.float32, device=device)
            net(feat, out=obj[:, :D - 4])
        else:
            f = net(feat) if net is not None and getattr(net, "_network", None) is not None else feat
            D = f.size(1) + 4
            obj = torch.empty(object_num, D, dtype=torch.float32, device=device)
            obj[:, :D - 4] = f
        L.box_positions(objects_list, obj, D - 4)                # :208-211
        return self._with_pairs(obj, D, object_num, world_geometry)

    def _with_pairs(self, obj, D, object_num, world_geometry):
        geo = world_geometry
        pair = None
        if geo is not None and geo._pair_num > 0:
            pair = L.pair_features(obj, D, geo._obj_off, geo._pair_off, geo._batch_size, max(geo._n_list), geo._pair_num,
                                   pair_index=geo.pair_index, ordered=getattr(geo, "_dropout_route", False))                 # :252-279
        return {'attribute_features': obj, 'relation_features': {'features': pair, 'index': None}, 'object_num': object_num}


class _LazyGather(object):
    """Per-ProgramBatch results whose answers are still queued (inside a graph capture); gather() after the queue has run."""

    def __init__(self, results, device):
        self.results, self.device = results, device

    def gather(self):
        return gather_results(self.results, self.device, True)


def _range_flags(queue, value=None):
    """`range_overflow: rerun`: run a finished forward's deferred closures (the answers' read-backs, then its fp16-range check) with the check
    handing its flags back instead of raising -> the forward's status word (0: in range).  value: the word as the caller read it back itself (a
    pipelined replay).  (Under `raise` the owners run their queues as they always have.)"""
    flags = 0
    for fill in queue:
        if getattr(fill, "range_check", False):
            flags |= fill(value is None, value, False)
        else:
            fill()
    return flags


def range_rerun(model, program_batch_list, flags, return_trace=False, modulator_switch=True):
    """`range_overflow: rerun`: the inference forward of `program_batch_list` again, on the wide-range arithmetic - what this model returns for the
    batch with `mlp_math: bf16x3` - after its first run left fp16's range (`flags`: its status word).  Eager, on the current stream, under
    no_grad; the caller has waited for the first run and discards its results.  The model's own modes are set for the duration (restored on
    the way out), so that everything that asks the model - the forward's scopes, the executor's model cache and spec, the attribute head's
    predicate - agrees: dense AND pair arithmetic "bf16x3" (a `pair_math: f16` or DFOL_PAIR_MATH left in place would saturate again).  The re-run
    has a watch of its own and raises like any forward.  Its log-probabilities, and the object features it read, must be finite (a NaN or inf
    feature is beyond any arithmetic): DfolError otherwise; an error of the re-run itself propagates with the range error as its cause."""
    from . import _lib
    why = _lib.range_message(flags)
    _lib.note("range_rerun")
    _lib.fallback("range_rerun", why, "ran a batch again on the 'bf16x3' arithmetic, dense layers and pair kernel (every such batch costs one extra forward)")
    saved = [(k, k in model.__dict__, model.__dict__.get(k)) for k in ("_mlp_math", "_pair_math")]
    try:
        model._mlp_math = model._pair_math = "bf16x3"
        with torch.no_grad():
            out = model._forward(program_batch_list, False, return_trace, modulator_switch, rerun=False)
    except Exception as err:
        raise err from _lib.DfolError(why)
    finally:
        for k, had, v in saved:
            if had:
                model.__dict__[k] = v
            else:
                model.__dict__.pop(k, None)
    # (the features are looked at too: the logic kernels clamp log-likelihoods at 0 with fminf, which drops a NaN - an object whose features hold
    # one would come back as a certain match, finite and wrong.  A re-run is rare: two small reductions and a host wait do not matter here)
    res = out[0] if return_trace else out
    feats = [pb._object_features for pb in program_batch_list if isinstance(pb._object_features, torch.Tensor)]
    if not all(bool(torch.isfinite(t).all()) for t in [res['log_probability']] + feats):
        raise _lib.DfolError(why + " The re-run on 'bf16x3' (`range_overflow: rerun`) did not help: the object features or the re-run's "
                             "log-probabilities are not all finite (a NaN or infinite feature is beyond every arithmetic).")
    return out


class PendingForward(object):
    """A forward whose launches are enqueued but whose answers have not been read back (`BatchInterpreterBase.forward_async`): the host
    is free - to collate the next ProgramBatch, say - while the device runs this one; `result()` waits for the device, reads the terminal
    operators' log-probabilities back and returns what `forward` would have.  rerun = (model, program_batch_list, modulator_switch) of a forward
    under `range_overflow: rerun`: a flagged forward is run again inside `result()` (range_rerun), on the stream current THERE, behind this
    forward - a forward queued after this one keeps its own tensors and status word."""

    def __init__(self, lazy, queue, rerun=None):
        self._lazy, self._queue, self._result, self._rerun = lazy, queue, None, rerun

    def result(self):
        if self._result is None:
            flags = 0
            if self._rerun is None:
                for fill in self._queue:
                    fill()
            else:
                flags = _range_flags(self._queue)
            if flags:
                model, pbs, modulator_switch = self._rerun
                self._result = range_rerun(model, pbs, flags, modulator_switch=modulator_switch)
            else:
                self._result = self._lazy.gather()
            self._lazy = self._queue = self._rerun = None
        return self._result


class GraphedForward(object):
    """The inference forward of one fixed list of ProgramBatches as a captured HIP graph (the launch sequence of a program batch is
    static: 16 launches for a 3-hop program).  Replaying it removes the per-launch host work, which is 7-10 % of a step at 36
    objects per scene.  The object features are read from the ProgramBatches' own tensors, so new scenes of the same shapes are
    served by copying into `program_batch._object_features` before `__call__`.  Answers are decoded after the replay.

    Lifetime: the graph holds raw device addresses.  Tensors created during the capture live in the graph's own memory pool; tensors
    that came out of a cache (uploaded index arrays, batch geometry, packed / split weight images, transposed LSTM weights) are
    referenced from `self._keep`, so cache evictions cannot free them under the graph.  The graph reads the weight images of the
    weight VERSION it was captured with: rebuild it after an optimizer step or load_state_dict."""

    def __init__(self, model, program_batch_list, warmup=2):
        from . import gqa_ops, native_exec
        self._model, self._pbs = model, program_batch_list
        with torch.no_grad():
            with native_exec.suspended():                        # (the capture records the Python operator loop: warm ITS caches)
                for _ in range(warmup):                          # fills the host-side caches (geometry, lowered tokens, packed weights)
                    model(program_batch_list, False)
            torch.cuda.synchronize()
            self._queue = []
            self._keep = []                                      # everything the caches handed to the captured launches (host_util.keeping)
            self._graph = torch.cuda.CUDAGraph()
            gqa_ops.DEFERRED.queue = self._queue
            gqa_ops.DEFERRED.outputs = self._outputs = []        # the device tensors the answers are decoded from
            from . import _lib
            _lib.CAPTURE_RANGE_HOST = self._range_host = _lib.new_range_host()     # (the replay copies the fp16-range status word into it)
            dev = program_batch_list[0].device
            _lib.CAPTURE_RANGE_DEV = self._range_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.CAPTURE_RANGE_WORD = self._range_word = torch.zeros(1, dtype=torch.int32, device=dev)   # (this graph's own: see ReplayLanes)
            try:
                with keeping(self._keep), torch.cuda.graph(self._graph):
                    self._lazy = model(program_batch_list, False)
            finally:
                gqa_ops.DEFERRED.queue = None
                gqa_ops.DEFERRED.outputs = None
                _lib.CAPTURE_RANGE_HOST = None
                _lib.CAPTURE_RANGE_DEV = None
                _lib.CAPTURE_RANGE_WORD = None
        self._outputs.extend(r['log_probability'] for r in self._lazy.results)
        seen, uniq = set(), []
        for t in self._outputs + [self._range_dev]:
            if id(t) not in seen:
                seen.add(id(t))
                uniq.append(t)
        self._outputs, self._slots, self._next = uniq, [], 0

    def __call__(self):
        self._graph.replay()
        if getattr(self._model, "_range_overflow", "raise") == "rerun":      # (a captured forward is an inference forward under no_grad)
            flags = _range_flags(self._queue)                    # (the range check waits for the replay's stream)
            if flags:
                # the replay is discarded; the batch runs again eagerly - outside any capture, behind the replay
                return range_rerun(self._model, self._pbs, flags)
            return self._lazy.gather()
        for fill in self._queue:
            fill()
        return self._lazy.gather()

    # ---- pipelined replays: the host decodes replay i's answers while the device runs replay i + 1 ------------------------------------------------
    def submit(self, depth=2):
        """Replay, and queue behind it the copies of everything the answers are decoded from (log-probabilities, arg-max flags, the fp16-range
        status word) into one of `depth` pinned slots - no host wait.  Returns the ticket `collect` takes.  At most `depth` tickets may be
        outstanding; new features for the next replay may be copied into the ProgramBatches' tensors right after this call (stream order)."""
        while len(self._slots) < max(1, depth):
            self._slots.append({"host": [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in self._outputs], "event": torch.cuda.Event(), "busy": False})
        slot = self._slots[self._next % len(self._slots)]
        if slot["busy"]:
            raise RuntimeError("GraphedForward.submit: %d replays outstanding; collect() the oldest first" % len(self._slots))
        self._next += 1
        self._graph.replay()
        for t, h in zip(self._outputs, slot["host"]):
            h.copy_(t, non_blocking=True)
        slot["event"].record()
        slot["busy"] = True
        slot["serial"] = self._next                              # (collect: no submit since - the ProgramBatches still hold this replay's features)
        return slot

    def collect(self, ticket):
        """Wait for that replay (only), decode its answers from its own copies and return what `forward` would have - with the log-probabilities
        as a host tensor (the device buffers belong to the replays behind it).  `range_overflow: rerun`: a flagged replay is run again eagerly
        over the ProgramBatches (range_rerun, on the current stream, after the wait for the ticket's event) - while they still hold that replay's
        features, that is with no `submit` on this graph since the ticket's; otherwise the range error is raised as under `raise`."""
        from . import gqa_ops
        ticket["event"].synchronize()
        snap = {id(t): h.numpy() for t, h in zip(self._outputs, ticket["host"])}
        gqa_ops.DEFERRED.snapshot = snap
        flags = 0
        try:
            if getattr(self._model, "_range_overflow", "raise") == "rerun":
                flags = _range_flags(self._queue, int(snap[id(self._range_dev)][0]))
            else:
                for fill in self._queue:
                    if getattr(fill, "range_check", False):
                        fill(False, int(snap[id(self._range_dev)][0]))
                    else:
                        fill()
            res = None if flags else self._lazy.gather()
        finally:
            gqa_ops.DEFERRED.snapshot = None
            ticket["busy"] = False
        if flags:
            from . import _lib
            if ticket["serial"] != self._next:
                raise _lib.DfolError(_lib.range_message(flags) + " `range_overflow: rerun` could not run this batch again: a later submit() on the "
                                     "same graph may have replaced its features in the ProgramBatches.")
            res = dict(range_rerun(self._model, self._pbs, flags))
            res['log_probability'] = res['log_probability'].cpu()
            return res
        res = dict(res)
        res['answer'] = [list(a) for a in res['answer']]         # (the queued closures refill the same lists at every replay)
        res['answer_log_probability'] = [list(a) for a in res['answer_log_probability']]
        res['log_probability'] = torch.cat([torch.from_numpy(snap[id(r['log_probability'])].reshape(-1).copy()) for r in self._lazy.results])
        return res


class ReplayLanes(object):
    """Several captured forwards of one batch shape - each over its OWN ProgramBatch tensors, intermediates and fp16-range status word - replayed
    round-robin on as many HIP streams, so that consecutive batches OVERLAP on the device: a forward ends in a dozen small logic launches (a few
    workgroups each, the rest of the 256 CUs idle, ~10 us apart) and begins with the featurizer and the pair kernel, which fill the chip - side by
    side the next batch's head runs in the previous one's tail.  256 questions x 100 objects: 1.52 ms per batch one replay at a time, 1.45 with
    two replays of one graph in flight on one stream (the host's read-back hidden), 1.35 on two lanes (tools/lab/time_step_forms.py).
    submit(fill) -> ticket: `fill(program_batch_list)` (optional) runs on the lane's stream before its replay - copy the batch's new features into
    the lane's tensors there; collect(ticket) -> the result dict of that batch (GraphedForward.collect).  At most one outstanding ticket per lane."""

    def __init__(self, model, program_batch_lists):
        assert len(program_batch_lists) >= 1
        self._graphs = [GraphedForward(model, pbs) for pbs in program_batch_lists]
        dev = program_batch_lists[0][0].device
        self._streams = [torch.cuda.Stream(device=dev) for _ in self._graphs]
        self._next = 0
        cur = torch.cuda.current_stream(dev)
        for s in self._streams:
            s.wait_stream(cur)                                   # (whatever uploaded the batches comes first)

    def __len__(self):
        return len(self._graphs)

    def batches(self, lane):
        return self._graphs[lane]._pbs

    def submit(self, fill=None):
        lane = self._next % len(self._graphs)
        self._next += 1
        g = self._graphs[lane]
        with torch.cuda.stream(self._streams[lane]):
            if fill is not None:
                fill(g._pbs)
            ticket = g.submit(depth=1)
        return (g, ticket)

    def collect(self, ticket):
        return ticket[0].collect(ticket[1])


class BatchInterpreterBase(nn.Module):
    """batch_base_interpreter.py:14-183."""

    def __init__(self, name, oracle, featurizer=None, attention_transfer_state_dim=0, apply_modulation_everywhere=True, cached=False,
                 visual_rule_learner=None, calibrator=None):
        super(BatchInterpreterBase, self).__init__()
        self._featurizer = featurizer
        self._oracle = oracle
        self._name = name
        self._global_step = nn.Parameter(torch.tensor([0], dtype=torch.float), requires_grad=False)
        self._has_modulator = False
        self._attention_transfer_state_dim = attention_transfer_state_dim
        self._apply_modulation_everywhere = apply_modulation_everywhere
        self._cached = cached
        if visual_rule_learner is not None or calibrator is not None:
            raise NotImplementedError("visual_rule_learner / calibrator are None in every reference configuration")

    def _execute(self, op_id, world, operator_batch, input_tuple, is_terminal, is_training):
        raise NotImplementedError

    def parameter_count(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def save(self, export_path_base):                          # :39-40
        torch.save(self.state_dict(), os.path.join(export_path_base, self._name))

    def load(self, import_path_base):                          # :42-43
        self.load_state_dict(torch.load(os.path.join(import_path_base, self._name)), strict=False)

    def build_scene(self, device, object_features, batch_index, meta_data, object_nums=None, question_image=None):
        """batch_base_interpreter.py:45-70: featurizer + oracle MLPs -> cached likelihood tables -> BatchWorld.
        `question_image` (ProgramBatch._question_image; None = one scene per question, the reference's layout): the object rows hold
        every distinct scene once and question k looks at scene question_image[k]."""
        if self._featurizer is None:
            raise NotImplementedError("a featurizer is required (the reference's featurizer-less branch :62-67 is dead code)")
        # needed-columns mode: no pair matrix, no full tables; the oracle keeps hidden activations and evaluates the concept
        # columns a program names.  The fused kernels are forward-only: they run whenever no gradient has to reach the oracle's
        # or the featurizer's weights (inference, and the calibrator-only phases cur6-7 where both are frozen); when those
        # weights train, the same columns come from differentiable tensor ops (visual_oracle._*_autograd).
        oracle_trains = torch.is_grad_enabled() and any(p.requires_grad for m in (self._oracle, self._featurizer)
                                                        if isinstance(m, nn.Module) for p in m.parameters())
        needed = self._cached and isinstance(self._featurizer, BatchGQABoxFeaturizer) and \
            getattr(self._oracle, "supports_needed_columns", lambda: False)()
        if question_image is not None and (not needed or oracle_trains or (self._has_modulator and torch.is_grad_enabled())):
            # shared scenes are served by the needed-columns inference dataflow; the other dataflows (full cached tables, training)
            # take the reference's layout: one copy of its scene per question
            if object_nums is None:
                bi = batch_index if isinstance(batch_index, torch.Tensor) else torch.as_tensor(batch_index)
                object_nums = torch.bincount(bi.to(torch.int64).cpu()).tolist()
            off = np.concatenate([[0], np.cumsum(object_nums)])
            rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in question_image]) if len(question_image) else np.zeros(0, np.int64)
            rows = torch.as_tensor(rows, dtype=torch.int64).to(object_features.device)
            object_features = object_features.select_rows(rows) if hasattr(object_features, "select_rows") else object_features.index_select(0, rows)
            object_nums = [int(object_nums[i]) for i in question_image]
            batch_index = torch.as_tensor(np.repeat(np.arange(len(object_nums)), object_nums).astype(np.int64)).to(object_features.device)
            question_image = None
        geometry = BatchWorld(device, object_features.size(0), None, None, batch_index, meta_data,
                              attention_transfer_state_dim=self._attention_transfer_state_dim, object_nums=object_nums,
                              question_image=question_image)
        dropping = None if needed or not self._cached else getattr(self._oracle, "active_dropout", lambda: None)()
        if dropping is not None:
            # the full-table dataflow because a Dropout drops: every Dropout of the reference is an element-wise kernel on a tensor that exists
            # there (csrc/dfol_dropout.hip), and the pair matrix's backward takes the ordered kernel instead of atomic index_add_
            from . import _lib
            geometry._dropout_route = True
            _lib.fallback("dropout_full_tables", "nn.%r is in training mode" % (dropping,),
                          what="takes the full-table dataflow: it stays on this library's dense kernels, with counter-based dropout masks, but "
                               "not on the fused pair and attribute kernels")
        if needed:
            features = self._featurizer.featurize_scene(device, object_features, batch_index, meta_data, world_geometry=None)
            self._oracle.prepare_scene(geometry, features['attribute_features'], train=oracle_trains)
            return geometry
        if 'world_geometry' in inspect.signature(self._featurizer.featurize_scene).parameters:
            features = self._featurizer.featurize_scene(device, object_features, batch_index, meta_data, world_geometry=geometry)
        else:                   # a featurizer written against the reference's 4-argument signature
            features = self._featurizer.featurize_scene(device, object_features, batch_index, meta_data)
        attribute_features = features['attribute_features']
        relation_features = features['relation_features']
        if self._cached:
            attribute_features, relation_features['features'] = self._oracle.compute_all_log_likelihood_2(
                attribute_features, relation_features['features'])
        geometry._attribute_features = attribute_features
        geometry._relation_features = relation_features
        return geometry

    def build_scene_graph(self, device, program_batch):
        """The world of a batch whose program is `scene` alone (operator scene, batch_gqa_ops.py:883-902): the featurizer, the attribute
        network over every object row, and the relation network over the pairs `meta_data['object_pairs']` lists - the rows
        [subject, object, distance, angle, sides] of batch_gqa_boxfeatures_pipeline.py:225-279 for the listed (subject, object) indices,
        offset per image (:238-249), in torch index ops (P is small) - never over all pairs of an image: no pair trunk runs.  The world
        carries a SceneLikelihood (the hidden rows of both sides) instead of likelihood tables."""
        from .visual_oracle import SceneLikelihood
        if self._featurizer is None:
            raise NotImplementedError("a featurizer is required (the reference's featurizer-less branch :62-67 is dead code)")
        if getattr(program_batch, "_question_image", None) is not None:
            raise NotImplementedError("a `scene` batch names one image per question: share_scenes is not built for it")
        meta = program_batch._meta_data or {}
        prepared = getattr(program_batch, "_scene_prepared", None)
        feats, batch_index = program_batch._object_features, program_batch._object_batch_index
        if prepared is not None:
            # data.prepare_scene_batch: the object rows (padded to the batch's capacity), the pairs and their by-object list sit in persistent
            # device tensors - nothing is built from host lists here, so a graph capture can bake the addresses in and be fed another batch
            feats = prepared.features
        world = BatchWorld(device, sum(program_batch._object_nums) if prepared is not None else feats.size(0), None, None, batch_index, meta,
                           attention_transfer_state_dim=self._attention_transfer_state_dim, object_nums=getattr(program_batch, "_object_nums", None))
        if 'world_geometry' in inspect.signature(self._featurizer.featurize_scene).parameters:
            obj = self._featurizer.featurize_scene(device, feats, batch_index, meta, world_geometry=None)['attribute_features']
        else:
            raise NotImplementedError("operator `scene` needs this package's featurizer (it builds the listed pairs' rows itself)")
        if prepared is not None:
            from . import _lib
            _lib.note("scene_pair_rows")
            pair_rows = L.scene_pair_rows(obj, prepared.pair_s, prepared.pair_o, (prepared.seg_off, prepared.slot))
        else:
            first = np.concatenate([[0], np.cumsum(world._img_n_list)])[:-1]
            pairs = meta.get('object_pairs') or {'subject_id': [], 'object_id': []}
            ind_s = [int(i) + int(o) for o, ids in zip(first, pairs['subject_id']) for i in ids]          # :242-246
            ind_o = [int(i) + int(o) for o, ids in zip(first, pairs['object_id']) for i in ids]
            if len(ind_s) != len(ind_o) or any(not 0 <= i < world._object_num for i in ind_s + ind_o):
                raise L.DfolError("object_pairs: subject and object lists differ in length or name an object the batch does not have")
            if ind_s:
                pair_rows = L.scene_pair_rows_reference(obj, upload(np.asarray(ind_s, np.int64), device), upload(np.asarray(ind_o, np.int64), device))
            else:
                pair_rows = obj.new_zeros(0, 2 * obj.shape[1] + 4)
        world._attribute_features, world._relation_features = obj, {'features': pair_rows, 'index': None}      # (the rows, as in the uncached reference)
        world._scene_likelihood = SceneLikelihood(*self._oracle.scene_hidden(obj, pair_rows), self._oracle)
        return world

    # `range_overflow` (config key, experiment.build_interpreter): what an INFERENCE forward does when a kernel of the default two-piece fp16
    # arithmetic left fp16's range - "raise" (DfolError naming the remedy) or "rerun" (that batch again on "bf16x3": range_rerun).  A forward a
    # gradient reaches - training.train_batch, GraphedTrainStep - raises under either: by the time the flag is read its backward has run, and
    # the optimizer step may have; DeviceFeatureStore.featurize() raises too: it speaks for a whole corpus, not for one batch.
    _range_overflow = "raise"

    def _may_rerun(self, program_batch_list, is_training):
        """This forward may be run again when it leaves fp16's range: the switch is on, and no gradient reaches the forward."""
        if self._range_overflow != "rerun":
            return False
        return not is_training and not (torch.is_grad_enabled() and (
            any(p.requires_grad for p in self.parameters()) or
            any(getattr(pb._object_features, "requires_grad", False) for pb in program_batch_list)))

    def forward(self, program_batch_list, is_training, return_trace=False, modulator_switch=True):
        """batch_base_interpreter.py:72-183.  Terminal operators defer reading their log-probabilities back until every
        ProgramBatch has been enqueued: one device->host synchronisation per forward.  Under `range_overflow: rerun` an inference forward
        that no gradient reaches and that left fp16's range is run again on the wide-range arithmetic (range_rerun) instead of raising."""
        return self._forward(program_batch_list, is_training, return_trace, modulator_switch, rerun=self._may_rerun(program_batch_list, is_training))

    def _forward(self, program_batch_list, is_training, return_trace, modulator_switch, rerun):
        """rerun: this forward reads its own answers back (no outer queue) and may run the batch again when its range check flags it; a forward
        whose read-backs an owner runs - forward_async, a graph capture - leaves that to the owner."""
        from . import gqa_ops, _lib
        _lib.dropout_forward_begins()                          # Dropout sites count from zero; the first one that drops advances the step
        outer = gqa_ops.DEFERRED.queue
        queue = [] if outer is None else outer                 # (a graph capture installs its own queue, see GraphedForward)
        gqa_ops.DEFERRED.queue = queue
        watch = None
        try:
            # `_mlp_math` (config key `mlp_math`, experiment.build_interpreter): "bf16" runs the large dense products of the featurizer and
            # the oracle MLPs - forward, and through the autograd functions' recorded mode their backward - on bf16-rounded operands with
            # fp32 accumulation (BASELINE configs[3]: "bf16 fwd / fp32 logic"); the logic kernels and everything small stay fp32
            from . import _lib
            dev0 = program_batch_list[0].device if program_batch_list else None
            watch = _lib.RangeWatch(dev0) if dev0 is not None and torch.device(dev0).type == "cuda" else None
            # `_pair_math` (config key `pair_math`): "f16" runs the fused pair kernel of an INFERENCE forward with one fp16 product per MAC
            # (reduced precision, opt-in); a train step's pair branch stays on the default (visual_oracle._train_pair_math)
            with _lib.dense_math(getattr(self, "_mlp_math", None)), _lib.pair_math_scope(getattr(self, "_pair_math", None)):
                all_results, all_traces, device = self._run_batches(program_batch_list, is_training, modulator_switch, return_trace)
            if watch is not None:
                check = watch.finish()                           # (runs after the answers' read-backs: raises if a kernel left fp16's range)
                if outer is None and _lib.capturing():
                    _lib.CAPTURE_RANGE_CHECKS.append(check)      # a captured train step: its owner checks after replays
                else:
                    queue.append(check)
        finally:
            gqa_ops.DEFERRED.queue = outer
            if watch is not None:
                _lib.range_status_off()                          # (also when the forward raised before watch.finish())
        if outer is None:
            if rerun:
                flags = _range_flags(queue)
                if flags:
                    return range_rerun(self, program_batch_list, flags, return_trace, modulator_switch)
            else:
                for fill in queue:
                    fill()
        result = gather_results(all_results, device, True) if outer is None else _LazyGather(all_results, device)
        return (result, all_traces) if return_trace else result

    def forward_async(self, program_batch_list, is_training=False, modulator_switch=True):
        """`forward` without its device->host synchronisation: enqueues every launch and returns a PendingForward.  The reference's test()
        loop (trainer.py:685-720) reads the answers of a batch before it collates the next; with this the two overlap on one thread."""
        from . import gqa_ops
        if gqa_ops.DEFERRED.queue is not None:
            raise RuntimeError("forward_async inside a graph capture or another pending forward's launch")
        queue = []
        gqa_ops.DEFERRED.queue = queue
        try:
            lazy = self._forward(program_batch_list, is_training, False, modulator_switch, rerun=False)
        finally:
            gqa_ops.DEFERRED.queue = None
        return PendingForward(lazy, queue, (self, program_batch_list, modulator_switch) if self._may_rerun(program_batch_list, is_training) else None)

    def _native_spec(self, is_training, modulator_switch, return_trace):
        """The lowering spec when this forward may run on the native executor (native_exec / native_plan: one C call per ProgramBatch instead
        of one Python dispatch per operator), else None: inference without gradients reaching the oracle or the calibrator, soft quantifiers, no
        trace, and not inside a graph capture (a capture records the Python loop's launches, as before).  Since round 6 the calibrated forward
        (activate_attention_transfer, the reference's default), shared scenes and bf16 relation tiles stay on the executor."""
        from . import _lib, native_exec
        if not native_exec.enabled() or is_training or return_trace or _lib.capturing() or getattr(self, "_hard_mode", False):
            return None
        calibrate = bool(self._has_modulator and modulator_switch)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return None                                      # gradients reach the oracle or the calibrator: the differentiable Python operators
        if not hasattr(self, "_ontology"):
            return None
        if self._gated() and not _lib.gate_native():         # trainable_gate: True - the gated opcodes are opt-in (DFOL_GATE_NATIVE=1)
            _lib.fallback("trainable_gate", "the native executor has no gated Filter / Relate instruction",
                          "runs the Python operator loop on the gated HIP kernels instead of the native executor")
            return None
        return native_exec.model_spec(self, calibrate)

    def _gated(self):
        """Do the logic cells hold trainable gates (`trainable_gate: True`)?  (The modules do not change after construction: looked up once.)"""
        gated = self.__dict__.get("_gated_cells")
        if gated is None:
            gated = self.__dict__["_gated_cells"] = any(getattr(m, "_trainable_gate", False) for m in self.modules())
        return gated

    def _run_batches(self, program_batch_list, is_training, modulator_switch, return_trace=False):
        from . import _lib
        all_traces, all_results = [], []
        device = program_batch_list[0].device
        spec = self._native_spec(is_training, modulator_switch, return_trace)
        for program_batch in program_batch_list:
            feats = program_batch._object_features
            if (program_batch.terminal_op_name() if hasattr(program_batch, "terminal_op_name") else None) == 'scene':
                ops = list(program_batch._op_batch_list)
                if any(ob._op_name != 'scene' for ob in ops):
                    raise NotImplementedError("operator `scene` is served for a batch whose program is `scene` alone")
                # scene-graph supervision: the Python operator on a world without likelihood tables; the native executor has no opcode for
                # it, and a graph capture takes it only as a prepared batch (data.prepare_scene_batch: DESIGN.md 3.8)
                if _lib.capturing() and getattr(program_batch, "_scene_prepared", None) is None:
                    raise NotImplementedError("a `scene` batch inside a graph capture (GraphedForward / GraphedTrainStep) must be prepared first: "
                                              "data.prepare_scene_batch holds what the step reads in persistent device tensors")
                _lib.note("scene_python")
                world = self.build_scene_graph(program_batch.device, program_batch)
                x, _ = self._execute(ops[-1]._op_id, world, ops[-1], (), True, is_training)
                all_results.append(x)
                all_traces.append([x])
                continue
            if spec is not None and (isinstance(feats, torch.Tensor) or hasattr(feats, "materialize")) and feats.is_cuda:
                from . import gqa_ops, native_exec
                plan = native_exec.plan_for(self, program_batch, spec)
                if plan is not None:
                    all_results.append(native_exec.run(self, program_batch, plan, gqa_ops.DEFERRED.queue, give_answer=not is_training))
                    all_traces.append([])
                    continue
            _lib.note("python_program")                         # (route counter: a ProgramBatch that ran the Python operator loop)
            world = self.build_scene(program_batch.device, program_batch._object_features, program_batch._object_batch_index,
                                     program_batch._meta_data, object_nums=getattr(program_batch, "_object_nums", None),
                                     question_image=getattr(program_batch, "_question_image", None))
            if self._has_modulator and modulator_switch:
                self._calibration_passes(world, program_batch, device, is_training)
            if world._lazy is not None:
                # with a training calibrator the attentions carry gradients and the relates run on the generic cell; a gated model's do too,
                # unless its one-launch Relate is switched on (DFOL_GATE_NATIVE=1) and no gradient is recorded
                self._oracle.prefetch_relations(world, program_batch, fused=not (self._has_modulator and modulator_switch and torch.is_grad_enabled())
                                                and (not self._gated() or (_lib.gate_native() and not torch.is_grad_enabled())), gated=self._gated())
                if hasattr(self._oracle, "prefetch_attributes"):
                    self._oracle.prefetch_attributes(world, program_batch)
            ops = program_batch._op_batch_list
            trace = []
            for i, op_batch in enumerate(ops):                   # execution loop :145-172
                deps = program_batch._dependencies[i]
                input_tuple = tuple(trace[d] for d in deps)
                x, terminate = self._execute(op_batch._op_id, world, op_batch, input_tuple, i == len(ops) - 1, is_training)
                if isinstance(x, BatchVariableSet) and len(input_tuple) > 0 and op_batch._mask is not None:
                    x = x.gate(input_tuple[0], op_batch._mask)   # questions lacking this op keep their attention (:166-167)
                trace.append(x)
                if terminate:
                    break
            all_results.append(trace[-1] if trace else None)
            all_traces.append(trace)
        return all_results, all_traces, device


def _calibration_passes(self, world, program_batch, device, is_training):
    """The LSTM walks the aligned program forward (batch_base_interpreter.py:92-111) and backward (:113-140); each operator
    leaves its [P, 4] modulations in its own dictionary, keyed by op id, for the execution loop to apply."""
    ops, deps_all = program_batch._op_batch_list, program_batch._dependencies
    last = len(ops) - 1
    trace = []
    for i, op_batch in enumerate(ops):
        deps = deps_all[i]
        input_tuple = tuple(trace[d] for d in deps) if deps else (None,)
        x, _ = self._transform_attention(op_batch._op_id, True, world, op_batch, input_tuple, i == last, is_training)
        if i < last and input_tuple[0] is not None and op_batch._mask is not None:
            x = x.gate(input_tuple[0], op_batch._mask)
        trace.append(x)
    reversed_dependencies = reverse_dependencies(deps_all)
    final = trace[-1]
    if isinstance(final, (tuple, list)):
        first_state = tuple(BatchAttentionState(a._name, device, a._state, set_zeros=True) for a in final)
    else:
        first_state = (BatchAttentionState(final._name, device, final._state, set_zeros=True),)
    trace = [None] * len(ops)
    for i in reversed(range(len(ops))):
        op_batch = ops[i]
        if len(reversed_dependencies[i]) == 1:
            temp = trace[reversed_dependencies[i][0]]
            if isinstance(temp, (tuple, list)):
                input_tuple = (temp[1],) if i == len(ops) - 2 else (temp[0],)
            else:
                input_tuple = (temp,)
        else:
            input_tuple = first_state
        x, _ = self._transform_attention(op_batch._op_id, False, world, op_batch, input_tuple, i == 0, is_training)
        if len(deps_all[i]) > 0 and op_batch._mask is not None and isinstance(x, BatchAttentionState) and i != last:
            x = x.gate(input_tuple[0], op_batch._mask)
        trace[i] = x


BatchInterpreterBase._calibration_passes = _calibration_passes


class BatchGQAInterpreter(BatchInterpreterBase):
    """batch_gqa_interpreter.py:13-86: the operator registry and its dispatch."""

    def __init__(self, name, oracle, ontology, featurizer=None, trainable_module_type=None, feature_dim=1, trainable_gate=False,
                 likelihood_threshold=0, hard_mode=False, attention_transfer_state_dim=0, forward_attention_network=None,
                 backward_attention_network=None, attention_output_network=None, apply_modulation_everywhere=True, cached=False,
                 visual_rule_learner=None, calibrator=None):
        super(BatchGQAInterpreter, self).__init__(name, oracle, featurizer, attention_transfer_state_dim=attention_transfer_state_dim,
                                                  apply_modulation_everywhere=apply_modulation_everywhere, cached=cached,
                                                  visual_rule_learner=visual_rule_learner, calibrator=calibrator)
        self._ontology = ontology
        self._likelihood_threshold = likelihood_threshold
        self._hard_mode = hard_mode
        self._has_modulator = forward_attention_network is not None and backward_attention_network is not None and \
            attention_output_network is not None
        kw = dict(trainable_module_type=trainable_module_type, feature_dim=feature_dim, trainable_gate=trainable_gate,
                  forward_attention_network=forward_attention_network, backward_attention_network=backward_attention_network,
                  attention_output_network=attention_output_network)
        o, t = self._oracle, self._ontology
        self._ops = nn.ModuleDict({
            'select': gqa.GQASelectBatch(o, t, **kw), 'filter': gqa.GQAFilterBatch(o, t, **kw), 'relate': gqa.GQARelateBatch(o, t, **kw),
            'query_attr': gqa.GQAQueryAttrBatch(o, t, **kw), 'choose_attr': gqa.GQAChooseAttrBatch(o, t, **kw),
            'verify_attrs': gqa.GQAVerifyAttrsBatch(o, t, **kw), 'choose_rel': gqa.GQAChooseRelBatch(o, t, **kw),
            'verify_rel': gqa.GQAVerifyRelBatch(o, t, **kw), 'exist': gqa.GQAExistBatch(o, t), 'and': gqa.GQAAndBatch(o, t),
            'or': gqa.GQAOrBatch(o, t), 'all_same': gqa.GQAAllSameBatch(o, t, **kw), 'all_different': gqa.GQAAllDifferentBatch(o, t, **kw),
            'two_same': gqa.GQATwoSameBatch(o, t, **kw), 'two_different': gqa.GQATwoDifferentBatch(o, t, **kw),
            'compare': gqa.GQACompareBatch(o, t, **kw), 'end': gqa.GQAEndBatch(o, t), 'scene': gqa.GQASceneOpBatch(o, t),
        })

    # one-hot position of every operator in the LSTM input (batch_gqa_interpreter.py:67-70)
    _OPS_INDEX = {'all_different': 0, 'all_same': 1, 'and': 2, 'choose_attr': 3, 'choose_rel': 4, 'compare': 5, 'end': 6, 'exist': 7,
                  'filter': 8, 'or': 9, 'query_attr': 10, 'relate': 11, 'select': 12, 'two_different': 13, 'two_same': 14,
                  'verify_attrs': 15, 'verify_rel': 16}

    def _transform_attention(self, op_id, is_forward, world, operator_batch, input_tuple, is_terminal, is_training):   # :80-86
        onehot = np.zeros(len(self._OPS_INDEX), np.float32)
        onehot[self._OPS_INDEX[operator_batch._op_name]] = 1.0
        temp = upload(onehot, world._device)                   # (memoised; an indexed assignment on the device is not graph-capturable)
        temp._host = onehot                                    # lets the operators build their constant feature columns on the host
        x = self._ops[operator_batch._op_name].transform_attention(*((op_id, is_forward, world) + input_tuple + tuple(operator_batch._arguments) +
                                                                     (temp, operator_batch._predicate_question_map)))
        return x, is_terminal

    def _execute(self, op_id, world, operator_batch, input_tuple, is_terminal, is_training):
        gqa.refuse_direct_supervision(operator_batch._op_name)
        op = self._ops[operator_batch._op_name]
        x = op(*((op_id, world) + input_tuple + tuple(operator_batch._arguments) +
                 (not is_training, operator_batch._predicate_question_map, self._likelihood_threshold, self._hard_mode)))
        if is_terminal and not operator_batch._is_terminal:      # append `end` to read out a log-likelihood (:75-76)
            return self._ops['end'](op_id, world, x, not is_training, operator_batch._predicate_question_map), is_terminal
        return x, is_terminal
