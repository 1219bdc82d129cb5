"""Child process of tests/test_store_direct_gpu.py: a `direct=True` feature store against a `direct=False` one over the same chunk files, on
the full-size synthetic model.  The library reads DFOL_DENSE_WIDE once per process, so each setting needs a process of its own:

  wide     DFOL_DENSE_WIDE=2 (the parent sets it): small batches take the wide kernel, the direct route reads the store's rows in place
  default  the switch unset: small batches are not the wide kernel's, the direct store materialises the matrix

usage: python tests/_store_direct_worker.py wide|default <directory>      prints one JSON line; any mismatch is an AssertionError.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from dfol_vqa_amd import _lib, data, experiment  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from dfol_vqa_amd.interpreter import GraphedForward  # noqa: E402
from test_feature_store import write_chunks  # noqa: E402

DEV = torch.device("cuda:0")
MAX_OBJ = 40
COUNTS = [40, 10, 25, 40, 10, 25, 13, 37]          # images 0-2 and 3-5 have the same object counts: a second scene for a captured batch
KEYS = ("feature_store_direct", "feature_store_direct_materialized", "native_program", "python_program")


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def counts_of(fn):
    before = dict(_lib.PATH_COUNTS)
    out = fn()
    return out, {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in KEYS}


def forward(model, collator, questions):
    pbs = collator.collate([dict(q) for q in questions])
    for pb in pbs:
        pb.create_sparse_tensors()
    with torch.no_grad():
        res = model([pb.to_cuda(DEV) for pb in pbs], False)
    return len(pbs), res["log_probability"].cpu().numpy().copy(), res["answer"]


def main(mode, directory):
    assert (os.environ.get("DFOL_DENSE_WIDE") == "2") == (mode == "wide")
    chunks, info = write_chunks(directory, feature_dim=2048, max_obj=MAX_OBJ, counts=COUNTS, per_chunk=4, seed=17)
    paths, names = syn.write_synthetic_ontology(os.path.join(directory, "ontology"))
    cfg = syn.reference_config(paths)
    ont = experiment.build_ontology(cfg)
    torch.manual_seed(0)
    model = experiment.build_model(cfg, ont)
    with torch.no_grad():
        model._oracle._embedding_network.linear.weight.normal_(0.0, 0.1)
        model._oracle._embedding_network.linear.bias.fill_(-2.0)
    model = model.to(DEV).eval()
    with open(paths["attribute_file"]) as f:
        cats = json.load(f)
    stores = {d: data.DeviceFeatureStore(directory, "objs", chunks, info, DEV, direct=d) for d in (False, True)}
    assert stores[True].direct and not stores[False].direct
    report = {"mode": mode, "cases": 0}

    def collator(direct, share):
        return data.BatchGQABoxFeaturesCollator(directory, "objs", chunks, info, ont, 2, device_store=stores[direct].index, share_scenes=share)
    images = [6, 1, 6, 3, 0]                       # 13 .. 40 objects, one image asked twice
    for kind in ("exist", "choose_attr", "verify_rel"):
        qs = syn.full_size_questions(kind, len(images), 10, MAX_OBJ, names, cats, 900 + len(kind), with_scene=False)
        for q, im in zip(qs, images):
            q["image_id"] = "img%03d" % im
        for share in (False, True):
            for native in ("1", "0"):
                os.environ["DFOL_NATIVE"] = native
                (n0, lp0, ans0), c0 = counts_of(lambda: forward(model, collator(False, share), qs))
                (n1, lp1, ans1), c1 = counts_of(lambda: forward(model, collator(True, share), qs))
                where = (kind, share, native, c0, c1)
                assert n0 == n1 and np.array_equal(lp0.view(np.uint32), lp1.view(np.uint32)) and ans0 == ans1, where
                assert c0["feature_store_direct"] == c0["feature_store_direct_materialized"] == 0, where
                assert c1["native_program" if native == "1" else "python_program"] == n1 and c0["native_program"] == c1["native_program"], where
                if mode == "wide":
                    assert c1["feature_store_direct"] == n1 and c1["feature_store_direct_materialized"] == 0, where
                else:
                    assert c1["feature_store_direct"] == 0 and c1["feature_store_direct_materialized"] == n1, where
                report["cases"] += 1
    os.environ["DFOL_NATIVE"] = "1"

    # a captured forward over StoreRows batches; a second scene (other images, the same object counts) served between replays
    store = stores[True]
    qs = syn.full_size_questions("exist", 4, 10, MAX_OBJ, names, cats, 77, with_scene=False)
    scenes = ([0, 1, 2, 1], [3, 4, 5, 4])
    host = []
    for ims in scenes:
        for q, im in zip(qs, ims):
            q["image_id"] = "img%03d" % im
        pbs = collator(True, False).collate([dict(q) for q in qs])
        for pb in pbs:
            pb.create_sparse_tensors()
        host.append(pbs)
    dev = [pb.to_cuda(DEV) for pb in host[0]]
    assert all(hasattr(pb._object_features, "materialize") for pb in dev)
    with torch.no_grad():
        eager = [model([pb.to_cuda(DEV) for pb in pbs], False) for pbs in host]
    assert not np.array_equal(bits(eager[0]["log_probability"]), bits(eager[1]["log_probability"]))
    g, c = counts_of(lambda: GraphedForward(model, dev))
    assert (c["feature_store_direct"] > 0) == (mode == "wide") and (c["feature_store_direct_materialized"] > 0) == (mode != "wide"), c
    r = g()
    assert np.array_equal(bits(r["log_probability"]), bits(eager[0]["log_probability"])) and r["answer"] == eager[0]["answer"]
    for pb, pb2 in zip(dev, host[1]):
        assert store.rows(pb2._object_features, out=pb._object_features) is pb._object_features
    r2 = g()
    assert np.array_equal(bits(r2["log_probability"]), bits(eager[1]["log_probability"])) and r2["answer"] == eager[1]["answer"]
    # inside a capture the rows cannot be rewritten (the index arrays would be baked into the graph)
    one, raised = torch.zeros(1, device=DEV), []
    ref2, rows = host[1][0]._object_features, dev[0]._object_features
    on_dev = store.upload_index(ref2)
    torch.cuda.synchronize()
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        one.add_(1)
        for kw in ({}, {"index": on_dev}):
            try:
                store.rows(ref2, out=rows, **kw)
            except _lib.DfolError:
                raised.append(True)
    assert raised == [True, True]
    report["graph"] = True
    print(json.dumps(report))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
