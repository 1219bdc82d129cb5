"""Child process of tests/test_store_featurized_gpu.py: a `featurized=True` feature store against a `direct=True` and a plain one over the same
chunk files.  The library reads DFOL_DENSE_WIDE once per process, so each setting needs a process of its own:

  wide     DFOL_DENSE_WIDE=2 (the parent sets it): the direct store's small batches read the store's rows in place (the wide kernel)
  default  the switch unset: the direct store's small batches materialise the matrix (the tiled kernel)

The cached route must give the bits of either.  usage: python tests/_store_featurized_worker.py wide|default <directory>; prints one JSON
line; any mismatch is an AssertionError.
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
from dfol_vqa_amd.data import ObjectFeatureRef  # noqa: E402
from dfol_vqa_amd.feature_store import FEATURIZE_BLOCK_ROWS, StoreRows  # noqa: E402
from dfol_vqa_amd.interpreter import BatchGQABoxFeaturizer, GraphedForward  # noqa: E402
from dfol_vqa_amd.visual_oracle import RegularMLP  # noqa: E402
from test_feature_store import write_chunks  # noqa: E402

DEV = torch.device("cuda:0")
MAX_OBJ, S, F = 40, 6, 2048
COUNTS = [MAX_OBJ, 1, 13, 37, 40, 40]              # six images in two chunks (tests/test_store_direct_gpu.py's corpus)
KEYS = ("feature_store_featurized", "feature_store_featurize", "feature_store_direct", "feature_store_direct_materialized", "native_program",
        "python_program")


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def counts_of(fn):
    before = dict(_lib.PATH_COUNTS)
    out = fn()
    return out, {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in KEYS}


def forward(model, collator, questions, grad=False):
    pbs = collator.collate([dict(q) for q in questions])
    for pb in pbs:
        pb.create_sparse_tensors()
    with torch.set_grad_enabled(grad):
        res = model([pb.to_cuda(DEV) for pb in pbs], False)
    return len(pbs), res["log_probability"].detach().cpu().numpy().copy(), res["answer"]


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2] == b[2]


def raises_naming(word, fn):
    try:
        fn()
    except _lib.DfolError as e:
        assert word in str(e), str(e)
        return True
    return False


def main(mode, directory):
    assert (os.environ.get("DFOL_DENSE_WIDE") == "2") == (mode == "wide")
    chunks, info = write_chunks(directory, feature_dim=F, max_obj=MAX_OBJ, counts=COUNTS, per_chunk=3, seed=17)

    def store_of(**kw):
        return data.DeviceFeatureStore(directory, "objs", chunks, info, DEV, **kw)
    stores = {"plain": store_of(), "direct": store_of(direct=True), "featurized": store_of(featurized=True)}
    sf = stores["featurized"]
    assert sf.featurized and sf.direct and not stores["direct"].featurized and (sf.S, sf.max_obj, sf.F) == (S, MAX_OBJ, F)
    assert S * MAX_OBJ < FEATURIZE_BLOCK_ROWS
    report = {"mode": mode}

    # ---- 2. the cache equals the per-batch featurizer: a single-layer and a two-layer network, bit for bit the direct route's object matrix -----
    refs = {"ragged": ObjectFeatureRef(sf.id, [3, 0, 5, 5, 2, 1, 3, 4], [40, 0, 37, 1, 40, 13, 7, 40]),
            "last": ObjectFeatureRef(sf.id, [S - 1], [MAX_OBJ]),
            "one": ObjectFeatureRef(sf.id, [1], [1])}
    torch.manual_seed(5)
    for name, hidden in (("single", []), ("two", [448])):
        net = RegularMLP(F, 512, hidden, 0.0).to(DEV).eval()
        feat = BatchGQABoxFeaturizer(net)
        assert sf.cached_for(net) is None
        cache, c = counts_of(lambda: sf.featurize(net))
        assert c["feature_store_featurize"] == 1 and tuple(cache.shape) == (S * MAX_OBJ, 512) and cache.dtype == torch.float32
        assert sf.cached_for(net) is cache and sf.cache_nbytes == S * MAX_OBJ * 512 * 4
        for rname, ref in refs.items():
            sd = stores["direct"]
            with torch.no_grad():
                want, c = counts_of(lambda: feat.featurize_scene(DEV, sd.rows(ObjectFeatureRef(sd.id, ref.slots, ref.counts)), None, None)["attribute_features"])
            assert c["feature_store_direct"] + c["feature_store_direct_materialized"] == 1 and c["feature_store_featurized"] == 0
            rows = sf.rows(ref)
            got = rows.objects(cache)
            assert got.shape == want.shape == (int(ref.counts.sum()), 516), (name, rname)
            diff = int((bits(got) != bits(want)).sum())
            print("cache against the direct route: %s %s %s: %d of %d words differ" % (mode, name, rname, diff, got.numel()))
            assert diff == 0, (mode, name, rname, diff)
            with torch.no_grad():                                              # and through the featurizer: the cached route, no rebuild
                again, c = counts_of(lambda: feat.featurize_scene(DEV, rows, None, None)["attribute_features"])
            assert c["feature_store_featurized"] == 1 and c["feature_store_featurize"] == 0 and np.array_equal(bits(again), bits(want))
    report["cache"] = True

    # ---- 3. through the interpreter: plain, direct and featurized stores, the Python loop and the executor ------------------------------------
    paths, names = syn.write_synthetic_ontology(os.path.join(directory, "ontology"))
    cfg = syn.reference_config(paths)
    ont = experiment.build_ontology(cfg)
    torch.manual_seed(0)
    model = experiment.build_model(cfg, ont)
    with torch.no_grad():
        model._oracle._embedding_network.linear.weight.normal_(0.0, 0.1)
        model._oracle._embedding_network.linear.bias.fill_(-2.0)
    model = model.to(DEV).eval()
    fnet = model._featurizer._featurizer_network
    with open(paths["attribute_file"]) as f:
        cats = json.load(f)

    def collator(store, share=False):
        return data.BatchGQABoxFeaturesCollator(directory, "objs", chunks, info, ont, 2, device_store=store.index, share_scenes=share)
    images = [2, 3, 2, 5, 0]                       # 13 .. 40 objects, one image asked twice
    cases, built = 0, 0
    for kind in ("exist", "choose_attr", "verify_rel"):
        qs = syn.full_size_questions(kind, len(images), 10, MAX_OBJ, names, cats, 900 + len(kind), with_scene=False)
        for q, im in zip(qs, images):
            q["image_id"] = "img%03d" % im
        for share in (False, True):
            for native in ("1", "0"):
                os.environ["DFOL_NATIVE"] = native
                r0, c0 = counts_of(lambda: forward(model, collator(stores["plain"], share), qs))
                r1, c1 = counts_of(lambda: forward(model, collator(stores["direct"], share), qs))
                r2, c2 = counts_of(lambda: forward(model, collator(sf, share), qs))
                where = (kind, share, native, c0, c1, c2)
                assert same(r0, r1) and same(r0, r2), where
                n = r2[0]
                assert c2["feature_store_featurized"] == n and c2["feature_store_direct"] == c2["feature_store_direct_materialized"] == 0, where
                assert c2["native_program" if native == "1" else "python_program"] == n and c2["native_program"] == c0["native_program"], where
                assert c0["feature_store_featurized"] == c1["feature_store_featurized"] == 0, where
                assert c0["feature_store_featurize"] == c1["feature_store_featurize"] == 0, where
                built += c2["feature_store_featurize"]
                assert built == 1, where                                       # built by the first forward, never again
                cases += 1
    os.environ["DFOL_NATIVE"] = "1"
    report["cases"] = cases

    # a captured forward over a featurized store's batches; a second scene (other images, the same object counts) served between replays
    qs = syn.full_size_questions("exist", 4, 10, MAX_OBJ, names, cats, 77, with_scene=False)
    scenes = ([0, 4, 2, 4], [5, 0, 2, 0])          # images 0, 4 and 5 have 40 objects each
    host = []
    for ims in scenes:
        for q, im in zip(qs, ims):
            q["image_id"] = "img%03d" % im
        pbs = collator(sf).collate([dict(q) for q in qs])
        for pb in pbs:
            pb.create_sparse_tensors()
        host.append(pbs)
    dev = [pb.to_cuda(DEV) for pb in host[0]]
    assert all(isinstance(pb._object_features, StoreRows) for pb in dev)
    with torch.no_grad():
        eager = [model([pb.to_cuda(DEV) for pb in pbs], False) for pbs in host]
    assert not np.array_equal(bits(eager[0]["log_probability"]), bits(eager[1]["log_probability"]))
    g, c = counts_of(lambda: GraphedForward(model, dev))
    assert c["feature_store_featurized"] > 0 and c["feature_store_featurize"] == 0 and c["feature_store_direct"] == c["feature_store_direct_materialized"] == 0, c
    r = g()
    assert np.array_equal(bits(r["log_probability"]), bits(eager[0]["log_probability"])) and r["answer"] == eager[0]["answer"]
    for pb, pb2 in zip(dev, host[1]):
        assert sf.rows(pb2._object_features, out=pb._object_features) is pb._object_features
    r2 = g()
    assert np.array_equal(bits(r2["log_probability"]), bits(eager[1]["log_probability"])) and r2["answer"] == eager[1]["answer"]
    report["graph"] = True

    # ---- 4. invalidation: an in-place weight update rebuilds once; a featurizer that trains steps aside -------------------------------------
    qs = syn.full_size_questions("exist", len(images), 10, MAX_OBJ, names, cats, 41, with_scene=False)
    for q, im in zip(qs, images):
        q["image_id"] = "img%03d" % im
    old = forward(model, collator(sf), qs)
    with torch.no_grad():
        fnet._network[1].weight.mul_(-0.5)
    assert sf.cached_for(fnet) is None
    new, c = counts_of(lambda: forward(model, collator(sf), qs))
    assert c["feature_store_featurize"] == 1 and c["feature_store_featurized"] == new[0], c
    assert same(new, forward(model, collator(stores["direct"]), qs)) and not same(new, old)
    again, c = counts_of(lambda: forward(model, collator(sf), qs))
    assert c["feature_store_featurize"] == 0 and c["feature_store_featurized"] == new[0] and same(again, new), c
    assert _lib.PATH_COUNTS["feature_store_featurize"] == 4                    # two networks of part 2, the model, the model's new weights
    assert not any(p.requires_grad for p in model.parameters())               # (the reference's frozen stages: the cached route's own ground)
    for p in fnet.parameters():
        p.requires_grad_(True)
    for native in ("1", "0"):                      # (with gradients wanted the executor steps aside too: the Python loop either way)
        os.environ["DFOL_NATIVE"] = native
        tr, c = counts_of(lambda: forward(model, collator(sf), qs, grad=True))
        assert c["feature_store_featurized"] == c["feature_store_featurize"] == 0, c
        assert c["feature_store_direct"] + c["feature_store_direct_materialized"] == tr[0] == c["python_program"], c
        assert same(tr, forward(model, collator(stores["direct"]), qs, grad=True))
    os.environ["DFOL_NATIVE"] = "1"
    for p in fnet.parameters():
        p.requires_grad_(False)
    assert sf.cached_for(fnet) is not None                                     # (stepping aside left the cache alone)
    report["invalidation"] = True

    # ---- 6. release_raw ------------------------------------------------------------------------------------------------------------------------
    # a rebuild inside a stream capture: refused (the raw features are still there: it is the capture that forbids it)
    with torch.no_grad():
        fnet._network[1].bias.add_(0.25)
    one, raised = torch.zeros(1, device=DEV), []
    torch.cuda.synchronize()
    with torch.cuda.graph(torch.cuda.CUDAGraph()):
        one.add_(1)
        raised.append(raises_naming("capture", lambda: sf.cached_for(fnet, build=True)))
        raised.append(raises_naming("capture", lambda: sf.featurize(fnet)))
    assert raised == [True, True] and sf.cached_for(fnet) is None
    try:
        sf.release_raw()                           # the cache is stale, but it exists: allowed - and then every batch raises until ...
    except _lib.DfolError:
        raise AssertionError("release_raw() with a cache")
    assert raises_naming("release_raw", lambda: forward(model, collator(sf), qs))                      # ... a stale cache cannot be rebuilt
    report["stale"] = True

    sr = store_of(featurized=True)
    assert raises_naming("featurize", sr.release_raw)                          # nothing cached yet
    want = forward(model, collator(stores["direct"]), qs)
    got, c = counts_of(lambda: forward(model, collator(sr), qs))
    assert same(got, want) and c["feature_store_featurize"] == 1
    before = sr.nbytes
    assert before == stores["plain"].nbytes
    assert sr.release_raw() is sr and sr.features is None
    assert before - sr.nbytes == S * MAX_OBJ * F * 4
    for native in ("1", "0"):
        os.environ["DFOL_NATIVE"] = native
        for share in (False, True):
            got, c = counts_of(lambda: forward(model, collator(sr, share), qs))
            assert same(got, want) and c["feature_store_featurize"] == 0 and c["feature_store_featurized"] == got[0], (native, share, c)
    os.environ["DFOL_NATIVE"] = "1"
    ref = ObjectFeatureRef(sr.id, [2, 0], [13, 40])
    rows = sr.rows(ref)                                                        # the index form needs no raw feature
    assert rows.table is None and tuple(rows.objects(sr.cached_for(fnet)).shape) == (53, 516)
    assert raises_naming("release_raw", lambda: sr.gather(ref))
    assert raises_naming("release_raw", rows.materialize)
    assert raises_naming("release_raw", lambda: rows.select_rows(torch.tensor([1, 0], device=DEV)).materialize())
    for p in fnet.parameters():
        p.requires_grad_(True)
    assert raises_naming("release_raw", lambda: forward(model, collator(sr), qs, grad=True))          # a featurizer that trains
    for p in fnet.parameters():
        p.requires_grad_(False)
    assert same(forward(model, collator(sr), qs), want)                        # (and the cache still serves the frozen one)
    with torch.no_grad():
        fnet._network[1].bias.add_(0.25)
    assert raises_naming("release_raw", lambda: sr.featurize(fnet))
    assert raises_naming("release_raw", lambda: forward(model, collator(sr), qs))                      # a stale cache
    report["release_raw"] = True
    print(json.dumps(report))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
