#!/usr/bin/env python3
"""What the device-resident feature store (dfol_vqa_amd/feature_store.py, csrc/dfol_store.hip) buys a stream of unseen batches.

Synthetic chunk files in the collator's layout (default 2048 images x 100 objects x 2048 features, .npz, in a temporary directory), then a
stream of unseen 256-question batches - DataLoader workers collate and lower them to plans, this process uploads, launches the native
executor and decodes the answers - with the object features arriving five ways:

  pool          already on the device (a pool of two feature sets, `value_fresh_programs`'s form): the upper bound
  store         an ObjectFeatureRef per batch, gathered from the store by ProgramBatch.to_cuda
  store_direct  the same refs and workers with the store in its index form (`direct=True`): to_cuda writes row numbers and box columns, the
                featurizer's first product reads the store's rows in place (csrc/dfol_dense_wide.hip, ROWS) - no [O, F + 6] matrix
  store_featurized  the same refs and workers with the store's cache of featurizer rows (`featurized=True`, built once before the runs): to_cuda
                writes row numbers and box columns, one launch gathers the batch's cached [O, 512] rows beside their box positions
                (csrc/dfol_store.hip, dfol_store_objects_f32) - no featurizer product per batch
  host          today's route: the worker builds [O, F + 6] from the chunk files, the matrix travels to this process, is pinned and uploaded

The legs alternate in one process, `--runs` runs each (a difference counts only when the ranges are apart).  The gather kernel
alone is timed by HIP events beside a device-to-device copy_ of the same byte count, and the featurizer's first product both ways: gather +
dfol_linear_wide_h2_f32 against dfol_store_rows_f32 + dfol_linear_wide_rows_h2_f32, alternating; the cached-row kernel likewise beside a copy_
of its bytes, with the one-off featurize() time and the cache's size.  Prints one JSON line.

`--leg train` is the train step instead (a featurizer that trains, nothing frozen): replayed GraphedTrainStep steps over one batch of `--batch`
questions x `--objects` objects at the full model widths, with the store plain (the matrix route: gather, then forward product and weight
gradient over the [O, F + 6] matrix) against `direct=True` (interpreter.featurize_scene's train route: both read the store's rows through
src_row), alternating, `--runs` runs each; the peak device memory of each route's batch upload, warm-up and capture above what was allocated before them (model copy and optimizer state included, alike); and
the weight-gradient kernel alone both ways (dfol_linear_wgrad_bias_f32 over the gathered matrix, dfol_linear_wgrad_bias_rows_f32 over the
table).  One JSON line.

`--leg bf16` is the same train leg in `mlp_math: bf16` with the store in its bf16 form (`feature_dtype="bf16"`: half the bytes, the first
layer reads the table in place - dfol_linear_act_rows_bf16t_f32, dfol_linear_wgrad_bias_rows_bf16t) against the fp32 store's matrix route
(`direct=False`), alternating in one session; beside the replayed step and the weight gradient it times the first product with what runs in
front of it (dfol_store_rows_f32 + the row kernel against the gather + dfol_linear_act_bf16_f32) and reports both stores' bytes.

`--leg bf16-direct` is inference in the DEFAULT arithmetic over the bf16 store, DFOL_STORE_BF16_DIRECT unset against set, alternating in one
process: the featurizer's first product with what runs in front of it (dfol_gather_object_rows_bf16_f32 + dfol_linear_wide_h2_f32 over the
widened matrix against dfol_store_rows_f32 + dfol_linear_wide_rows_bf16t_h2_f32 over the table), the rate of `--batches` unseen batches
(collated on the host beforehand; upload, forward and read-back are timed), the peak device memory of a pass, and "same bits" for each pair.

`--leg bf16-train` is the train step in the DEFAULT arithmetic over the bf16 store, DFOL_STORE_BF16_TRAIN unset against set, alternating in one
process: the first-layer forward with what runs in front of it (gather + product over the widened matrix against dfol_store_rows_f32 + the
in-place product), the weight gradient alone (dfol_linear_wgrad_bias_f32 over the matrix against dfol_linear_wgrad_bias_rows_bf16t_x3 over the
table), replayed GraphedTrainStep steps of `--batch` questions x `--objects` objects (each route trains a copy of the model from the same state:
"same bits" compares the copies after the same number of steps), and the peak device memory of each route's upload, warm-up and capture.

usage: python tools/bench_feature_store.py [--leg stream|train|bf16|bf16-direct|bf16-train][--images 2048] [--objects 100] [--features 2048] [--batch 256] [--batches 24] [--runs 4]
                                           [--workers 5] [--steps 20]
"""
import argparse
import collections
import copy
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dfol_vqa_amd as D  # noqa: E402
from dfol_vqa_amd import data, experiment  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402

KINDS = ["exist", "verify_rel", "choose_attr", "and", "query_attr", "verify_attrs", "or", "choose_rel"]


class HostCollator(data.BatchGQABoxFeaturesCollator):
    """The host route over .npz chunks: every chunk is read ONCE per process (numpy re-reads a whole .npz member on every access; the
    reference's .h5 chunks are read row by row)."""

    def _chunk(self, i):
        arrays = data._open_arrays(self._chunk_path(i))
        return {k: np.asarray(arrays[k]) for k in ("features", "bboxes")}


class PoolCollator(D.ProgramCollaterBase):
    """No features at all: the launching process points every batch at a device-resident feature set."""

    def __init__(self, ontology, counts):
        super(PoolCollator, self).__init__("select", "relate", "filter", 1, ontology=ontology)
        self._counts = counts

    def collate_object_features(self, questions):
        return None, torch.from_numpy(np.repeat(np.arange(len(questions)), [self._counts[q["image_id"]] for q in questions]).astype(np.int64))

    def collate_meta_data(self, questions):
        return {"index": {}, "embedding": torch.zeros(1, 1)}


class Collate(object):
    """A DataLoader worker's collate function: collate -> lower -> plan -> sparse maps (the worker never opens the GPU)."""

    def __init__(self, collator):
        self.collator = collator

    def __call__(self, questions):
        pbs = self.collator.collate(questions)
        for pb in pbs:
            pb.create_sparse_tensors()
        return pbs


def one_thread(_):
    torch.set_num_threads(1)


def write_corpus(directory, images, objects, features, per_chunk, seed=3):
    rng = np.random.default_rng(seed)
    info, chunks = {}, (images + per_chunk - 1) // per_chunk
    for c in range(chunks):
        n = min(per_chunk, images - c * per_chunk)
        feats = rng.random((n, objects, features), dtype=np.float32)
        boxes = np.empty((n, objects, 4), np.float32)
        boxes[..., 0] = rng.random((n, objects), dtype=np.float32) * 500
        boxes[..., 1] = rng.random((n, objects), dtype=np.float32) * 400
        boxes[..., 2:] = boxes[..., :2] + 5 + rng.random((n, objects, 2), dtype=np.float32) * 100
        np.savez(os.path.join(directory, "objs_%d.npz" % c), features=feats, bboxes=boxes)
        for i in range(n):
            info["img%05d" % (c * per_chunk + i)] = {"objectsNum": objects, "width": 640, "height": 480, "idx": i, "file": c}
    path = os.path.join(directory, "objs_info.json")
    with open(path, "w") as f:
        json.dump(info, f)
    return chunks, path, info


def load_wide(_lib, O, N, K):
    """The wide kernel takes the featurizer's first product at this shape (what both routes of the product comparison run)."""
    return 256 < N <= 512 and K >= 128 and K % 4 == 0 and _lib.linear_wide_supported(O, N, K)


def span(xs):
    return {"min": min(xs), "median": float(np.median(xs)), "max": max(xs)}


def apart(a, b):
    """a against b in ms, by the rule that a difference counts only when the ranges of the runs are apart."""
    return "faster, ranges apart" if a["max"] < b["min"] else "slower, ranges apart" if a["min"] > b["max"] else "ranges overlap: no difference shown"


def train_leg(args, bf16=False):
    """Replayed train steps over a plain store against a direct store (see the module's docstring) -> the result dictionary.  bf16: the
    `mlp_math: bf16` arithmetic, and the direct store is the bf16 one."""
    from dfol_vqa_amd import _lib, training
    import bench
    device = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp(prefix="dfol_store_train_bench_")
    try:
        paths, names = syn.write_synthetic_ontology(os.path.join(tmp, "ontology"))
        cfg = syn.reference_config(paths, box_features_dim=args.features, freeze_featurizer=False, freeze_attribute_network=False,
                                   freeze_relation_network=False, freeze_embedding_network=False, dropout=0.0, **({"mlp_math": "bf16"} if bf16 else {}))
        ontology = experiment.build_ontology(cfg)
        torch.manual_seed(0)
        model = experiment.build_model(cfg, ontology)
        bench.init_weights(model)
        model = model.to(device).train()
        chunks, info_path, _ = write_corpus(tmp, args.images, args.objects, args.features, args.per_chunk)
        stores = {"matrix": data.DeviceFeatureStore(tmp, "objs", chunks, info_path, device),
                  "direct": data.DeviceFeatureStore(tmp, "objs", chunks, info_path, device, **({"feature_dtype": "bf16"} if bf16 else {"direct": True}))}
        with open(paths["attribute_file"]) as f:
            cats = json.load(f)
        rng = np.random.RandomState(9)
        qs = syn.full_size_questions("verify_rel", args.batch, args.objects, args.objects, names, cats, 7100, with_scene=False)
        for q in qs:
            q["image_id"] = "img%05d" % rng.randint(args.images)
        steps, peak, counts = {}, {}, {}
        for route, store in stores.items():
            pbs = data.BatchGQABoxFeaturesCollator(tmp, "objs", chunks, info_path, ontology, 1, device_store=store.index).collate([dict(q) for q in qs])
            for pb in pbs:
                pb.create_sparse_tensors()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()             # (before to_cuda: a plain store's batch IS the gathered [O, F + 6] matrix)
            torch.cuda.reset_peak_memory_stats()
            dev = [pb.to_cuda(device) for pb in pbs]
            net = copy.deepcopy(model)                       # (a graph bakes its parameters' addresses in: each route trains a copy of its own)
            opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4, capturable=True)
            before = dict(_lib.PATH_COUNTS)
            steps[route] = training.GraphedTrainStep(net, opt, dev, 0.65)
            torch.cuda.synchronize()
            peak[route] = torch.cuda.max_memory_allocated() - base
            counts[route] = {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0)
                             for k in ("feature_store_direct_train", "feature_store_direct_materialized", "python_program")}

        def replay_ms(step):
            step()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                step()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / args.steps
        ms = {route: [] for route in steps}
        for _ in range(args.runs):
            for route in steps:
                ms[route].append(replay_ms(steps[route]))

        # the weight-gradient kernel alone, both ways, on the batch's own rows (workspace and results allocated by the wrappers, alike)
        first = [m for m in model._featurizer._featurizer_network._network if isinstance(m, torch.nn.Linear)][0]
        ids = [q["image_id"] for q in qs]
        rows, mat = stores["direct"].rows(stores["direct"].index.ref(ids)), stores["matrix"].gather(stores["matrix"].index.ref(ids))
        dy = torch.randn(rows.O, first.out_features, device=device) * 0.01

        def kernel_ms(fn, n=20):
            for _ in range(3):
                fn()
            evs = []
            for _ in range(n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
            return float(np.median([a.elapsed_time(b) for a, b in evs]))
        kernel, product = {"matrix": [], "rows": []}, {"matrix": [], "rows": []}
        with _lib.dense_math("bf16" if bf16 else None):
            same = bool(torch.equal(_lib.linear_wgrad(dy, mat[:, :args.features]), _lib.linear_wgrad_rows(dy, rows.table, rows.src_row)))
            for _ in range(args.runs):
                kernel["matrix"].append(kernel_ms(lambda: _lib.linear_wgrad(dy, mat[:, :args.features], bias=True)))
                kernel["rows"].append(kernel_ms(lambda: _lib.linear_wgrad_rows(dy, rows.table, rows.src_row, bias=True)))
            if bf16:                                         # the first product with what runs in front of it: gather + matrix kernel, row kernel + rows
                refs = {k: st.index.ref(ids) for k, st in stores.items()}
                idx = {k: st.upload_index(refs[k]) for k, st in stores.items()}
                y, act = torch.empty(rows.O, first.out_features, device=device), _lib.ACT_SIGMOID

                def by_matrix():
                    stores["matrix"].gather(refs["matrix"], out=mat, index=idx["matrix"])
                    _lib.linear_act_split(mat[:, :args.features], first.weight, first.bias, act, out=y)

                def by_rows():
                    stores["direct"].rows(refs["direct"], out=rows, index=idx["direct"])
                    _lib.linear_rows_bf16t(rows.table, rows.src_row, first.weight, first.bias, act, out=y)
                by_matrix()
                y0 = y.clone()
                by_rows()
                same = same and bool(torch.equal(y0, y))
                for _ in range(args.runs):
                    product["matrix"].append(kernel_ms(by_matrix))
                    product["rows"].append(kernel_ms(by_rows))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    m, d = span(ms["matrix"]), span(ms["direct"])
    more = {}
    if bf16:
        more = {"first_product_ms": {"gather_and_matrix": span(product["matrix"]), "rows": span(product["rows"]),
                                     "rows_vs_matrix": apart(span(product["rows"]), span(product["matrix"]))},
                "store_bytes": {k: st.nbytes for k, st in stores.items()}}
    return {"tool": "bench_feature_store", "leg": "bf16" if bf16 else "train", **more,
            "shape": {"images": args.images, "objects": args.objects, "features": args.features, "batch": args.batch, "rows": rows.O,
                      "runs": args.runs, "replays_per_run": args.steps},
            "train_step_ms": {"matrix": m, "direct": d, "direct_vs_matrix": apart(d, m)},
            "peak_bytes_of_upload_warm_up_and_capture": peak, "peak_direct_minus_matrix_bytes": peak["direct"] - peak["matrix"],
            "matrix_bytes": rows.O * (args.features + 6) * 4,
            "wgrad_kernel_ms": {"matrix": span(kernel["matrix"]), "rows": span(kernel["rows"]),
                                "rows_vs_matrix": apart(span(kernel["rows"]), span(kernel["matrix"])), "same_bits": same},
            "routes": counts}


def bf16_direct_leg(args):
    """The default arithmetic over a bf16 store, DFOL_STORE_BF16_DIRECT unset against set (see the module's docstring) -> the result dictionary."""
    from dfol_vqa_amd import _lib
    import bench
    device = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp(prefix="dfol_store_bf16_direct_bench_")
    os.environ.pop("DFOL_STORE_BF16_DIRECT", None)
    try:
        paths, names = syn.write_synthetic_ontology(os.path.join(tmp, "ontology"))
        cfg = syn.reference_config(paths, box_features_dim=args.features)
        ontology = experiment.build_ontology(cfg)
        torch.manual_seed(0)
        model = experiment.build_model(cfg, ontology)
        bench.init_weights(model)
        model = model.to(device).eval()
        chunks, info_path, _ = write_corpus(tmp, args.images, args.objects, args.features, args.per_chunk)
        store = data.DeviceFeatureStore(tmp, "objs", chunks, info_path, device, feature_dtype="bf16")
        with open(paths["attribute_file"]) as f:
            cats = json.load(f)
        rng = np.random.RandomState(9)
        host = []
        for b in range(args.batches):                        # every batch other programs on other images
            qs = syn.full_size_questions(KINDS[b % len(KINDS)], args.batch, args.objects, args.objects, names, cats, 7000 + b, with_scene=False)
            for q in qs:
                q["image_id"] = "img%05d" % rng.randint(args.images)
            pbs = data.BatchGQABoxFeaturesCollator(tmp, "objs", chunks, info_path, ontology, 1, device_store=store.index).collate(qs)
            for pb in pbs:
                pb.create_sparse_tensors()
            host.append((pbs, [q["image_id"] for q in qs]))

        def kernel_ms(fn, n=20):
            for _ in range(3):
                fn()
            evs = []
            for _ in range(n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
            return float(np.median([a.elapsed_time(b) for a, b in evs]))

        # the first product with what runs in front of it, on the first batch's rows
        first = [m for m in model._featurizer._featurizer_network._network if isinstance(m, torch.nn.Linear)][0]
        ref = store.index.ref(host[0][1])
        idx = store.upload_index(ref)
        rows = store.rows(ref)
        mat = torch.empty(rows.O, args.features + 6, device=device)
        y, act = torch.empty(rows.O, first.out_features, device=device), _lib.ACT_SIGMOID
        wide = load_wide(_lib, rows.O, first.out_features, args.features)

        def by_matrix():                                     # dfol_gather_object_rows_bf16_f32 + dfol_linear_wide_h2_f32 over the matrix
            store.gather(ref, out=mat, index=idx)
            _lib.linear_wide(mat[:, :args.features], first.weight, first.bias, act, out=y)

        def by_rows():                                       # dfol_store_rows_f32 + dfol_linear_wide_rows_bf16t_h2_f32
            store.rows(ref, out=rows, index=idx)
            _lib.linear_wide_rows_bf16t(rows.table, rows.src_row, first.weight, first.bias, act, out=y)
        by_matrix()
        y0 = y.clone()
        y.fill_(-1.0)
        by_rows()
        product_same = bool(torch.equal(y0.view(torch.int32), y.view(torch.int32)))
        # (c) the two-product form on a CERTIFIED table: a copy of the store's table with every magnitude below 2^-10 set to zero (random
        # features hold a few values below 2^-17 whose low bits fp16 cannot keep); against the three-product kernel on the same copy
        class Certified(object):
            f16_exact = True
        store_certifies = bool(store.f16_exact)
        tab_c = rows.table.clone()
        tab_c[tab_c.float().abs() < 2.0 ** -10] = 0
        assert _lib.store_bf16_is_f16(tab_c)

        def by_rows_c3():
            store.rows(ref, out=rows, index=idx)
            _lib.linear_wide_rows_bf16t(tab_c, rows.src_row, first.weight, first.bias, act, out=y)

        def by_rows_c2():
            store.rows(ref, out=rows, index=idx)
            _lib.linear_wide_rows_bf16t(tab_c, rows.src_row, first.weight, first.bias, act, out=y, store=Certified)
        by_rows_c3()
        y0 = y.clone()
        y.fill_(-1.0)
        by_rows_c2()
        two_same = bool(torch.equal(y0.view(torch.int32), y.view(torch.int32)))
        product = {"matrix": [], "rows": [], "rows_c3": [], "rows_c2": []}
        for _ in range(args.runs):
            product["matrix"].append(kernel_ms(by_matrix))
            product["rows"].append(kernel_ms(by_rows))
            product["rows_c3"].append(kernel_ms(by_rows_c3))
            product["rows_c2"].append(kernel_ms(by_rows_c2))
        del mat, y, y0, tab_c

        # unseen batches: upload (to_cuda resolves the batch's ref from the store), forward, answers read back; the host collation is outside
        def run(on):
            if on:
                os.environ["DFOL_STORE_BF16_DIRECT"] = "1"
            else:
                os.environ.pop("DFOL_STORE_BF16_DIRECT", None)
            before = dict(_lib.PATH_COUNTS)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            lps = []
            t0 = time.perf_counter()
            with torch.no_grad():
                for pbs, _ in host:
                    res = model([pb.to_cuda(device) for pb in pbs], False)
                    lps.append(res["log_probability"])
            torch.cuda.synchronize()
            s = time.perf_counter() - t0
            peak = torch.cuda.max_memory_allocated() - base
            counts = {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0)
                      for k in ("feature_store_direct", "feature_store_direct_bf16_h2", "feature_store_direct_materialized", "native_program")}
            return args.batches * args.batch / s, peak, counts, torch.cat([lp.flatten() for lp in lps])
        rate, peak, counts, lp = {}, {}, {}, {}
        for on in (False, True):                             # (warm-up: plans, packed weights, allocator)
            run(on)
        rate = {False: [], True: []}
        for _ in range(args.runs):
            for on in (False, True):
                r, peak[on], counts[on], lp[on] = run(on)
                rate[on].append(r)
        os.environ.pop("DFOL_STORE_BF16_DIRECT", None)
        forward_same = bool(torch.equal(lp[False].view(torch.int32), lp[True].view(torch.int32)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    a, b = span(product["matrix"]), span(product["rows"])
    off, on = span(rate[False]), span(rate[True])
    return {"tool": "bench_feature_store", "leg": "bf16-direct",
            "shape": {"images": args.images, "objects": args.objects, "features": args.features, "batch": args.batch, "rows": rows.O,
                      "batches": args.batches, "runs": args.runs, "wide_kernel_takes_the_shape": bool(wide)},
            "first_product_ms": {"a_gather_bf16_and_wide_over_the_matrix": a, "b_store_rows_and_in_place_three_products": b,
                                 "b_vs_a": apart(b, a), "same_bits": product_same,
                                 "b_on_the_certified_copy": span(product["rows_c3"]), "c_in_place_two_products_on_the_certified_copy": span(product["rows_c2"]),
                                 "c_vs_b_on_the_same_copy": apart(span(product["rows_c2"]), span(product["rows_c3"])), "c_same_bits_as_b": two_same,
                                 "the_random_store_itself_certifies": store_certifies,
                                 "caveat": "every sample launches on the same rows back to back: the bf16 routes' 105 MB fit the 256 MB last-level "
                                           "cache between launches, route (a)'s matrix traffic does not - a stream of unseen batches has no such help"},
            "unseen_batches_questions_per_s": {"switch_off": off, "switch_on": on,
                                               "on_vs_off": "faster, ranges apart" if on["min"] > off["max"] else
                                               "slower, ranges apart" if on["max"] < off["min"] else "ranges overlap: no difference shown",
                                               "same_bits": forward_same},
            "peak_bytes_of_a_pass": {"switch_off": peak[False], "switch_on": peak[True], "on_minus_off": peak[True] - peak[False]},
            "matrix_bytes": rows.O * (args.features + 6) * 4, "store_bytes": store.nbytes,
            "routes": {"switch_off": counts[False], "switch_on": counts[True]}}


def bf16_train_leg(args):
    """The default arithmetic's train step over a bf16 store, DFOL_STORE_BF16_TRAIN unset against set (see the module's docstring) -> the result
    dictionary."""
    from dfol_vqa_amd import _lib, training
    import bench
    device = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp(prefix="dfol_store_bf16_train_bench_")
    for k in ("DFOL_STORE_BF16_TRAIN", "DFOL_STORE_BF16_DIRECT"):
        os.environ.pop(k, None)

    def switch(on):
        if on:
            os.environ["DFOL_STORE_BF16_TRAIN"] = "1"
        else:
            os.environ.pop("DFOL_STORE_BF16_TRAIN", None)
    try:
        paths, names = syn.write_synthetic_ontology(os.path.join(tmp, "ontology"))
        cfg = syn.reference_config(paths, box_features_dim=args.features, freeze_featurizer=False, freeze_attribute_network=False,
                                   freeze_relation_network=False, freeze_embedding_network=False, dropout=0.0)
        ontology = experiment.build_ontology(cfg)
        torch.manual_seed(0)
        model = experiment.build_model(cfg, ontology)
        bench.init_weights(model)
        model = model.to(device).train()
        chunks, info_path, _ = write_corpus(tmp, args.images, args.objects, args.features, args.per_chunk)
        store = data.DeviceFeatureStore(tmp, "objs", chunks, info_path, device, feature_dtype="bf16")
        with open(paths["attribute_file"]) as f:
            cats = json.load(f)
        rng = np.random.RandomState(9)
        qs = syn.full_size_questions("verify_rel", args.batch, args.objects, args.objects, names, cats, 7100, with_scene=False)
        for q in qs:
            q["image_id"] = "img%05d" % rng.randint(args.images)
        ids = [q["image_id"] for q in qs]
        steps, nets, peak, counts = {}, {}, {}, {}
        for on in (False, True):                             # (the route is baked into the capture: the switch matters here only)
            switch(on)
            pbs = data.BatchGQABoxFeaturesCollator(tmp, "objs", chunks, info_path, ontology, 1, device_store=store.index).collate([dict(q) for q in qs])
            for pb in pbs:
                pb.create_sparse_tensors()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            dev = [pb.to_cuda(device) for pb in pbs]
            nets[on] = copy.deepcopy(model)                  # (a graph bakes its parameters' addresses in: each route trains a copy of its own)
            opt = torch.optim.Adam([p for p in nets[on].parameters() if p.requires_grad], lr=1e-4, capturable=True)
            before = dict(_lib.PATH_COUNTS)
            steps[on] = training.GraphedTrainStep(nets[on], opt, dev, 0.65)
            torch.cuda.synchronize()
            peak[on] = torch.cuda.max_memory_allocated() - base
            counts[on] = {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0)
                          for k in ("feature_store_direct_train", "feature_store_direct_train_bf16_x3", "feature_store_direct_materialized", "python_program")}
        switch(False)

        def replay_ms(step):
            step()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                step()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / args.steps
        ms = {False: [], True: []}
        for _ in range(args.runs):
            for on in (False, True):
                ms[on].append(replay_ms(steps[on]))
        # both copies have taken the same number of steps from the same state on the same batch
        losses = {on: float(steps[on]()[0]) for on in (False, True)}
        torch.cuda.synchronize()
        step_same = losses[False] == losses[True] and all(
            torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(nets[False].parameters(), nets[True].parameters()))

        def kernel_ms(fn, n=20):
            for _ in range(3):
                fn()
            evs = []
            for _ in range(n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
            return float(np.median([a.elapsed_time(b) for a, b in evs]))

        # the first-layer forward with what runs in front of it, and the weight gradient alone, on the batch's own rows
        first = [m for m in model._featurizer._featurizer_network._network if isinstance(m, torch.nn.Linear)][0]
        ref = store.index.ref(ids)
        idx = store.upload_index(ref)
        rows = store.rows(ref)
        mat = torch.empty(rows.O, args.features + 6, device=device)
        y, act = torch.empty(rows.O, first.out_features, device=device), _lib.ACT_SIGMOID
        dy = torch.randn(rows.O, first.out_features, device=device) * 0.01
        wide = load_wide(_lib, rows.O, first.out_features, args.features)

        if not wide:
            raise SystemExit("bench_feature_store: --leg bf16-train needs a shape the wide kernel takes (the route's own condition)")

        def by_matrix():                                     # dfol_gather_object_rows_bf16_f32 + dfol_linear_wide_h2_f32 over the widened matrix
            store.gather(ref, out=mat, index=idx)
            _lib.linear_wide(mat[:, :args.features], first.weight, first.bias, act, out=y)

        def by_rows():                                       # dfol_store_rows_f32 + dfol_linear_wide_rows_bf16t_h2_f32 over the table
            store.rows(ref, out=rows, index=idx)
            _lib.linear_wide_rows_bf16t(rows.table, rows.src_row, first.weight, first.bias, act, out=y)
        with torch.no_grad():
            by_matrix()
            y0 = y.clone()
            y.fill_(-1.0)
            by_rows()
            product_same = bool(torch.equal(y0.view(torch.int32), y.view(torch.int32)))
            w0, b0 = _lib.linear_wgrad(dy, mat[:, :args.features], bias=True)
            w1, b1 = _lib.linear_wgrad_rows_bf16t_x3(dy, rows.table, rows.src_row, bias=True)
            wgrad_same = bool(torch.equal(w0.view(torch.int32), w1.view(torch.int32)) and torch.equal(b0.view(torch.int32), b1.view(torch.int32)))
            product, kernel = {"matrix": [], "rows": []}, {"matrix": [], "rows": []}
            for _ in range(args.runs):
                product["matrix"].append(kernel_ms(by_matrix))
                product["rows"].append(kernel_ms(by_rows))
                kernel["matrix"].append(kernel_ms(lambda: _lib.linear_wgrad(dy, mat[:, :args.features], bias=True)))
                kernel["rows"].append(kernel_ms(lambda: _lib.linear_wgrad_rows_bf16t_x3(dy, rows.table, rows.src_row, bias=True)))
    finally:
        switch(False)
        shutil.rmtree(tmp, ignore_errors=True)
    off, on = span(ms[False]), span(ms[True])
    pa, pb_ = span(product["matrix"]), span(product["rows"])
    ka, kb = span(kernel["matrix"]), span(kernel["rows"])
    return {"tool": "bench_feature_store", "leg": "bf16-train",
            "shape": {"images": args.images, "objects": args.objects, "features": args.features, "batch": args.batch, "rows": rows.O,
                      "runs": args.runs, "replays_per_run": args.steps, "wide_kernel_takes_the_shape": bool(wide)},
            "first_layer_forward_ms": {"gather_bf16_and_product_over_the_matrix": pa, "store_rows_and_in_place_product": pb_, "in_place_vs_matrix": apart(pb_, pa),
                                       "same_bits": product_same,
                                       "caveat": "every sample launches on the same rows back to back: the in-place route's 105 MB fit the 256 MB last-level "
                                                 "cache between launches, the matrix route's traffic does not - a stream of unseen batches has no such help"},
            "wgrad_kernel_ms": {"six_products_over_the_matrix": ka, "three_products_over_the_table": kb, "table_vs_matrix": apart(kb, ka), "same_bits": wgrad_same},
            "train_step_ms": {"switch_off": off, "switch_on": on, "on_vs_off": apart(on, off), "same_bits": bool(step_same),
                              "loss_after_the_same_steps": {"switch_off": losses[False], "switch_on": losses[True]}},
            "peak_bytes_of_upload_warm_up_and_capture": {"switch_off": peak[False], "switch_on": peak[True], "on_minus_off": peak[True] - peak[False]},
            "matrix_bytes": rows.O * (args.features + 6) * 4, "store_bytes": store.nbytes,
            "routes": {"switch_off": counts[False], "switch_on": counts[True]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("stream", "train", "bf16", "bf16-direct", "bf16-train"), default="stream",
                    help="the stream of unseen inference batches, replayed train steps, the train leg in mlp_math: bf16 over the bf16 store, the "
                         "default arithmetic's inference over the bf16 store with DFOL_STORE_BF16_DIRECT unset and set, or its train step over the "
                         "bf16 store with DFOL_STORE_BF16_TRAIN unset and set")
    ap.add_argument("--steps", type=int, default=20, help="--leg train: replays per timed run")
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--objects", type=int, default=100)
    ap.add_argument("--features", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=24, help="unseen batches per run of a leg (at least 4)")
    ap.add_argument("--runs", type=int, default=4, help="runs of every leg, alternating (at least four for a comparison)")
    ap.add_argument("--workers", type=int, default=5)
    ap.add_argument("--per-chunk", type=int, default=256, help="images per chunk file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feature_store: needs a GPU (there is no CPU form of this measurement)")
    if args.leg == "bf16-direct":
        print(json.dumps(bf16_direct_leg(args)))
        return
    if args.leg == "bf16-train":
        print(json.dumps(bf16_train_leg(args)))
        return
    if args.leg in ("train", "bf16"):
        print(json.dumps(train_leg(args, bf16=args.leg == "bf16")))
        return
    import bench
    from dfol_vqa_amd import _lib, native_exec, training
    device = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp(prefix="dfol_store_bench_")
    loaders = {}
    try:
        paths, names = syn.write_synthetic_ontology(os.path.join(tmp, "ontology"))
        cfg = syn.reference_config(paths)
        ontology = experiment.build_ontology(cfg)
        torch.manual_seed(0)
        model = experiment.build_model(cfg, ontology)
        bench.init_weights(model)
        model = model.to(device).eval()
        spec = native_exec.model_spec(model) if native_exec.enabled() else None
        t0 = time.perf_counter()
        chunks, info_path, info = write_corpus(tmp, args.images, args.objects, args.features, args.per_chunk)
        write_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        store = data.DeviceFeatureStore(tmp, "objs", chunks, info_path, device)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0

        with open(paths["attribute_file"]) as f:
            cats = json.load(f)
        rng = np.random.RandomState(9)
        questions = []
        for b in range(args.batches):                        # every batch other programs on other images
            qs = syn.full_size_questions(KINDS[b % len(KINDS)], args.batch, args.objects, args.objects, names, cats, 7000 + b, with_scene=False)
            for q in qs:
                q["image_id"] = "img%05d" % rng.randint(args.images)
            questions += qs
        sampler = [list(range(b * args.batch, (b + 1) * args.batch)) for b in range(args.batches)]

        collators = {"pool": PoolCollator(ontology, {k: v["objectsNum"] for k, v in info.items()}),
                     "store": HostCollator(tmp, "objs", chunks, info_path, ontology, 1, device_store=store.index),
                     "host": HostCollator(tmp, "objs", chunks, info_path, ontology, 1)}
        for c in collators.values():
            c._native_spec = spec
        batch_bytes = args.batch * args.objects * (args.features + 6) * 4
        # the host leg's matrices cross from the workers through shared memory: as many workers as it has room for, else this process collates
        shm_free = shutil.disk_usage("/dev/shm").free if os.path.isdir("/dev/shm") else 0
        host_workers = int(max(0, min(args.workers, shm_free // (3 * batch_bytes))))
        for leg, c in collators.items():
            w = host_workers if leg == "host" else args.workers
            kw = dict(multiprocessing_context="spawn", persistent_workers=True, worker_init_fn=one_thread, prefetch_factor=1 if leg == "host" else 2) if w else {}
            # (pinning is the host leg's: the reference's pin_memory DataLoader for the feature matrix; a store batch's few hundred bytes of
            # index arrays go through the pinned staging ring)
            loaders[leg] = torch.utils.data.DataLoader(questions, batch_sampler=sampler, num_workers=w, collate_fn=Collate(c), pin_memory=leg == "host", **kw)

        refs = [store.index.ref([q["image_id"] for q in questions[i * args.batch:(i + 1) * args.batch]]) for i in range(min(8, args.batches))]
        pool = [store.gather(r) for r in refs[:2]]
        first_lp = {}
        # the cache of featurizer rows, built once (the model's featurizer is frozen: reference_config); the store's flags are set per leg
        fnet = model._featurizer._featurizer_network
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cache = store.featurize(fnet)
        torch.cuda.synchronize()
        featurize_s = time.perf_counter() - t0

        def run(leg):
            """One pass over the stream: -> (seconds, host seconds spent in to_cuda)."""
            inflight, k, to_cuda_s = collections.deque(), 0, 0.0

            def finish():
                pbs, pending = inflight.popleft()
                res = pending.result()
                training.compute_evaluation_metrics(pbs, res)
                return res
            store.featurized = leg == "store_featurized"     # (recorded on the store only: the same index, refs, collator and workers)
            store.direct = leg in ("store_direct", "store_featurized")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for pbs in loaders["store" if leg.startswith("store_") else leg]:
                h0 = time.perf_counter()
                if leg == "pool":
                    for pb in pbs:
                        pb._object_features = pool[k % len(pool)]
                dev = [pb.to_cuda(device) for pb in pbs]
                to_cuda_s += time.perf_counter() - h0
                inflight.append((dev, model.forward_async(dev, False)))
                if len(inflight) > 2:                        # two batches in flight, as value_fresh_programs
                    res = finish()
                    if k == 2 and leg not in first_lp:
                        first_lp[leg] = res["log_probability"].cpu().numpy().copy()
                k += 1
            while inflight:
                finish()
            torch.cuda.synchronize()
            store.direct = store.featurized = False
            return time.perf_counter() - t0, to_cuda_s

        legs = ("pool", "store", "store_direct", "store_featurized", "host")
        with torch.no_grad():
            for leg in legs:                                 # warm-up: workers up, allocator, weight images
                run(leg)
            _lib.PATH_COUNTS.clear()
            times = {leg: [] for leg in legs}
            to_cuda = {leg: [] for leg in legs}
            for _ in range(args.runs):
                for leg in legs:
                    dt, h = run(leg)
                    times[leg].append(dt / args.batches * 1e3)
                    to_cuda[leg].append(h / args.batches * 1e3)
        counts = {k: v for k, v in _lib.PATH_COUNTS.items() if k in ("native_program", "python_program", "feature_store_batch", "feature_store_miss",
                                                                     "feature_store_direct", "feature_store_direct_materialized",
                                                                     "feature_store_featurized", "feature_store_featurize")}

        # the gather alone, and a device-to-device copy of the same bytes, by HIP events in the same session
        out = torch.empty_like(pool[0])
        src = pool[1]

        def event_ms(fn, n=20):
            for i in range(3):
                fn(i)
            evs = []
            for i in range(n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn(i)
                b.record()
                evs.append((a, b))
            torch.cuda.synchronize()
            return sorted(a.elapsed_time(b) for a, b in evs)
        # (the kernel alone: every ref's index arrays are on the device before the first event, nothing is allocated between the events)
        on_dev = [store.upload_index(r) for r in refs]
        torch.cuda.synchronize()
        gather_ms = event_ms(lambda i: store.gather(refs[i % len(refs)], out=out, index=on_dev[i % len(refs)]))
        copy_ms = event_ms(lambda i: out.copy_(src))
        same = bool(np.array_equal(first_lp["store"].view(np.uint32), first_lp["host"].view(np.uint32)))
        same_direct = bool(np.array_equal(first_lp["store_direct"].view(np.uint32), first_lp["store"].view(np.uint32)))
        same_featurized = bool(np.array_equal(first_lp["store_featurized"].view(np.uint32), first_lp["store"].view(np.uint32)))

        # the cached-row kernel alone (row numbers and box columns on the device before the first event), and a device-to-device copy of the bytes it
        # writes - it reads four columns per row fewer, from rows scattered over the cache
        batch_rows = [store.rows(r, index=i) for r, i in zip(refs, on_dev)]
        obj = torch.empty(batch_rows[0].O, cache.shape[1] + 4, device=device)
        obj_src = torch.rand_like(obj)
        objects_ms = event_ms(lambda i: batch_rows[i % len(refs)].objects(cache, out=obj))
        objects_copy_ms = event_ms(lambda i: obj.copy_(obj_src))
        objects_bytes = obj.numel() * 4 + batch_rows[0].O * cache.shape[1] * 4

        # the featurizer's first product both ways, alternating in `runs` rounds: the matrix route (gather + the wide product over the matrix) against
        # the index route (row numbers and box columns + the wide product over the store's rows); index arrays uploaded and buffers allocated before
        first = [m for m in model._featurizer._featurizer_network._network if isinstance(m, torch.nn.Linear)][0]
        O, N = out.shape[0], first.out_features
        product = None
        if first.in_features == args.features and _lib._dense_math() == "f16x2" and load_wide(_lib, O, N, args.features):
            rows = [store.rows(r, index=i) for r, i in zip(refs, on_dev)]
            y = torch.empty(O, N, device=device)
            act = _lib.ACT_SIGMOID

            def matrix_route(i):
                store.gather(refs[i % len(refs)], out=out, index=on_dev[i % len(refs)])
                _lib.linear_wide(out[:, :args.features], first.weight, first.bias, act, out=y)

            def index_route(i):
                r = rows[i % len(refs)]
                store.rows(refs[i % len(refs)], out=r, index=on_dev[i % len(refs)])
                _lib.linear_wide_rows(r.table, r.src_row, first.weight, first.bias, act, out=y)
            matrix_route(0)
            y_matrix = y.clone()
            index_route(0)
            product = {"same_bits": bool(torch.equal(y, y_matrix)), "matrix_route_ms": [], "index_route_ms": [], "wide_over_matrix_ms": [], "wide_over_rows_ms": []}
            for _ in range(args.runs):
                product["matrix_route_ms"].append(float(np.median(event_ms(matrix_route))))
                product["index_route_ms"].append(float(np.median(event_ms(index_route))))
                product["wide_over_matrix_ms"].append(float(np.median(event_ms(
                    lambda i: _lib.linear_wide(out[:, :args.features], first.weight, first.bias, act, out=y)))))
                product["wide_over_rows_ms"].append(float(np.median(event_ms(
                    lambda i: _lib.linear_wide_rows(rows[i % len(refs)].table, rows[i % len(refs)].src_row, first.weight, first.bias, act, out=y)))))
    finally:
        for ld in loaders.values():                          # (persistent workers: stop them before the files go)
            it = getattr(ld, "_iterator", None)
            if it is not None:
                it._shutdown_workers()
        shutil.rmtree(tmp, ignore_errors=True)

    ms = {leg: span(times[leg]) for leg in legs}
    qps = {leg: {"min": args.batch / ms[leg]["max"] * 1e3, "median": args.batch / ms[leg]["median"] * 1e3, "max": args.batch / ms[leg]["min"] * 1e3} for leg in legs}
    g, c = float(np.median(gather_ms)), float(np.median(copy_ms))
    extra = ms["store"]["median"] - ms["pool"]["median"]
    moved = 2.0 * batch_bytes
    result = {
        "tool": "bench_feature_store", "shape": {"images": args.images, "objects": args.objects, "features": args.features, "batch": args.batch,
                                                 "batches_per_run": args.batches, "runs": args.runs, "workers": args.workers, "host_leg_workers": host_workers},
        "store": {"bytes": store.nbytes, "slots": store.S, "chunks": chunks, "write_files_s": write_s, "build_s": build_s},
        "ms_per_batch": ms, "questions_per_s": qps, "to_cuda_host_ms_per_batch": {leg: span(to_cuda[leg]) for leg in legs},
        "store_vs_host": apart(ms["store"], ms["host"]), "store_vs_pool": apart(ms["store"], ms["pool"]),
        "store_over_pool_questions_per_s": qps["store"]["median"] / qps["pool"]["median"],
        "store_over_host_questions_per_s": qps["store"]["median"] / qps["host"]["median"],
        "gather_kernel": {"ms": span(gather_ms), "GBps_read_plus_written": moved / g / 1e6, "bytes_read_plus_written": moved},
        "copy_d2d": {"ms": span(copy_ms), "GBps_read_plus_written": moved / c / 1e6},
        "gather_over_copy": g / c,
        "store_step_beyond_pool": {"ms_per_batch": extra, "gather_kernel_ms": g, "not_explained_by_the_gather_ms": extra - g,
                                   "to_cuda_host_ms_store_minus_pool": float(np.median(to_cuda["store"]) - np.median(to_cuda["pool"])),
                                   "named": "the gather runs on the launch stream ahead of the batch's featurizer (nothing overlaps it), and to_cuda of a "
                                            "store batch allocates the [O, F + 6] matrix, uploads the index arrays and launches on the launching thread: "
                                            "to_cuda_host_ms_store_minus_pool is that host share"},
        "store_direct_vs_store": apart(ms["store_direct"], ms["store"]), "store_direct_vs_pool": apart(ms["store_direct"], ms["pool"]),
        "store_direct_over_store_questions_per_s": qps["store_direct"]["median"] / qps["store"]["median"],
        "featurizer_first_product": None if product is None else dict(
            product, matrix_route=span(product["matrix_route_ms"]), index_route=span(product["index_route_ms"]),
            index_vs_matrix=apart(span(product["index_route_ms"]), span(product["matrix_route_ms"])),
            wide_rows_vs_wide=apart(span(product["wide_over_rows_ms"]), span(product["wide_over_matrix_ms"]))),
        "store_featurized_vs_store_direct": apart(ms["store_featurized"], ms["store_direct"]),
        "store_featurized_vs_store": apart(ms["store_featurized"], ms["store"]), "store_featurized_vs_pool": apart(ms["store_featurized"], ms["pool"]),
        "store_featurized_over_store_direct_questions_per_s": qps["store_featurized"]["median"] / qps["store_direct"]["median"],
        "featurized_cache": {"featurize_s": featurize_s, "bytes": store.cache_nbytes, "rows": int(cache.shape[0]), "width": int(cache.shape[1]),
                             "raw_feature_bytes": store.S * store.max_obj * store.F * 4},
        "objects_kernel": {"ms": span(objects_ms), "bytes_read_plus_written": objects_bytes,
                           "GBps_read_plus_written": objects_bytes / float(np.median(objects_ms)) / 1e6},
        "objects_copy_d2d": {"ms": span(objects_copy_ms), "GBps_read_plus_written": 2.0 * obj.numel() * 4 / float(np.median(objects_copy_ms)) / 1e6},
        "objects_over_copy": float(np.median(objects_ms)) / float(np.median(objects_copy_ms)),
        "routes": counts, "store_equals_host_bitwise_first_batch": same, "store_direct_equals_store_bitwise_first_batch": same_direct,
        "store_featurized_equals_store_bitwise_first_batch": same_featurized,
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
