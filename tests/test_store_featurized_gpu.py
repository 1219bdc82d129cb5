"""GPU tests of the feature store's cached form (`DeviceFeatureStore(..., featurized=True)`): the cached-row kernel (csrc/dfol_store.hip,
dfol_store_objects_f32) against index_select and box_positions, the cache against the direct route's per-batch featurizer, the routes -
featurizer, native executor, shared scenes, captured forward, invalidation, release_raw - against plain and direct stores, and a train step with
a frozen featurizer.  Every comparison is bit equality."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfol_vqa_amd as D  # noqa: E402,F401
from dfol_vqa_amd import _lib, data  # noqa: E402
from dfol_vqa_amd import ops as L  # noqa: E402
from dfol_vqa_amd.data import DeviceFeatureStore, ObjectFeatureRef  # noqa: E402
from dfol_vqa_amd.feature_store import StoreRows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAX_OBJ, S = 40, 6
HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -12345.5


def bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """src_row / box6 of one batch of a small store, from dfol_store_rows_f32: rows repeated (slots 3 and 5 named twice), an empty image, and the
    table's last row (slot S - 1 with every row); and the positions box_positions writes for box6 - the reference, computed once."""
    from test_feature_store import write_chunks
    d = tmp_path_factory.mktemp("featurized_kernel")
    chunks, info = write_chunks(d, feature_dim=128, max_obj=MAX_OBJ, counts=[MAX_OBJ, 1, 13, 37, 40, 40], per_chunk=3, seed=11)
    store = DeviceFeatureStore(str(d), "objs", chunks, info, DEV, featurized=True)
    assert store.featurized and store.direct and (store.S, store.max_obj) == (S, MAX_OBJ)
    rows = store.rows(ObjectFeatureRef(store.id, [3, 0, 5, 5, 2, 1, 3, 5], [40, 0, 37, 1, 40, 13, 7, 40]))
    src = rows.src_row.cpu().numpy()
    assert rows.O == 178 and int(src.max()) == S * MAX_OBJ - 1 and len(np.unique(src)) < len(src)
    pos = torch.full((rows.O, 4), SENTINEL, device=DEV)
    L.box_positions(rows.box6, pos, 0)
    return store, rows, pos


# ---- 1. dfol_store_objects_f32 alone ------------------------------------------------------------------------------------------------------------
# W: 1 and 6 scalar loads, 8 rows per wavefront; 8 and 128 the 16-byte loads with 8 and 2 rows per wavefront (128: the last width below a whole
# wavefront per row); 130 a wavefront per row, scalar; 512 the featurizer's width.  pad: 0 the matrix itself; 3 a wider buffer whose rows start at
# every alignment (4, 8, 12, 16 bytes) and whose further columns must stay.  132:130 = a table of row stride 132 read 130 wide (16-byte loads and a
# two-column tail).
@pytest.mark.parametrize("pad", [0, 3], ids=["ld=W+4", "ld=W+7"])
@pytest.mark.parametrize("W", [1, 6, 8, 128, 130, 512, (132, 130)], ids=str)
def test_store_objects_kernel(batch, W, pad):
    store, rows, pos = batch
    ld_cache, W = W if isinstance(W, tuple) else (W, W)
    g = torch.Generator(device="cpu").manual_seed(100 * W + pad)
    table = torch.randn(S * MAX_OBJ, ld_cache, generator=g).to(DEV)
    cache = table[:, :W]
    want = cache.index_select(0, rows.src_row.long())
    out = torch.full((rows.O, W + 4 + pad), SENTINEL, device=DEV)
    assert _lib.store_objects(cache, rows.src_row, rows.box6, out=out) is out
    assert np.array_equal(bits(out[:, :W]), bits(want)), "cached columns"
    assert np.array_equal(bits(out[:, W:W + 4]), bits(pos)), "position columns"
    assert bool((out[:, W + 4:] == SENTINEL).all()), "columns beyond W + 4"
    if pad == 0:
        fresh = _lib.store_objects(cache, rows.src_row, rows.box6)
        assert tuple(fresh.shape) == (rows.O, W + 4) and np.array_equal(bits(fresh), bits(out))
        if ld_cache == W:
            assert np.array_equal(bits(rows.objects(cache)), bits(out))                          # StoreRows.objects is the same call
            pick = torch.tensor([177, 0, 0, 40, 77, 39, 76], dtype=torch.int64, device=DEV)     # ... and a selection of rows has it too
            assert np.array_equal(bits(rows.select_rows(pick).objects(cache)), bits(out.index_select(0, pick)))


def test_store_objects_guards(batch):
    store, rows, _ = batch
    W = 130
    cache = torch.zeros(S * MAX_OBJ, W, device=DEV)
    h = _lib.load()
    assert h.dfol_store_objects_f32(None, W, None, None, 0, W, None, W + 4, None) == 0          # O == 0: no launch, no error
    none = store.rows(ObjectFeatureRef(store.id, [2, 0], [0, 0]))
    assert tuple(none.objects(cache).shape) == (0, W + 4)
    with pytest.raises(_lib.DfolError, match="ld_out"):
        _lib.store_objects(cache, rows.src_row, rows.box6, out=torch.empty(rows.O, W + 3, device=DEV))
    with pytest.raises(_lib.DfolError):
        _lib.store_objects(cache, rows.src_row, rows.box6, out=torch.empty(rows.O - 1, W + 4, device=DEV))
    with pytest.raises(_lib.DfolError):
        _lib.store_objects(cache, rows.src_row, rows.box6[:, :5].contiguous())
    with pytest.raises(_lib.DfolError):
        rows.objects(torch.zeros(S * MAX_OBJ - 1, W, device=DEV))                                  # not this store's cache
    for O, Wb, ld_cache, ld_out in ((-1, W, W, W + 4), (1, 0, W, W + 4), (1, W, W - 1, W + 4), (1, W, W, W + 3)):
        assert h.dfol_store_objects_f32(cache.data_ptr(), ld_cache, rows.src_row.data_ptr(), rows.box6.data_ptr(), O, Wb, cache.data_ptr(), ld_out, None) != 0
        assert b"store_objects" in h.dfol_last_error()


# ---- 2 - 4, 6. the cache and the routes, one child process per setting of DFOL_DENSE_WIDE (the library reads it once) -----------------------------
@pytest.mark.parametrize("mode", ["wide", "default"])
def test_featurized_store_equals_direct_and_plain_stores(mode, tmp_path):
    """Six images of 1 - 40 objects in two chunks, 2048 features.  `featurize(net)` for a single-layer and a two-layer featurizer: a batch's
    `rows.objects(cache)` is bit for bit the object matrix the `direct=True` route computes for the same batch - the claim being that a row's
    product does not depend on which rows share its block (`wide`: the direct route reads the store's rows in place; `default`: it
    materialises and the tiled kernel runs).  Then the full-size synthetic model over a plain, a direct and a featurized store, on the native
    executor and the Python loop, with and without shared scenes: identical log-probabilities and answers, the cached route counted once per
    batch and the cache built once; a captured forward served a second scene through `rows(ref2, out=rows)`; an in-place weight update
    rebuilds once, a featurizer that trains steps aside; release_raw drops `nbytes` by the features' size, forwards still match and every
    route that needs raw rows raises naming it; a rebuild inside a stream capture raises.  (tests/_store_featurized_worker.py)"""
    env = dict(os.environ)
    env.pop("DFOL_DENSE_WIDE", None)
    env.pop("DFOL_NATIVE", None)
    if mode == "wide":
        env["DFOL_DENSE_WIDE"] = "2"
    out = subprocess.run([sys.executable, os.path.join(HERE, "_store_featurized_worker.py"), mode, str(tmp_path)], env=env, capture_output=True,
                         text=True, timeout=300)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report == {"mode": mode, "cache": True, "cases": 12, "graph": True, "invalidation": True, "stale": True, "release_raw": True}


# ---- 5. a train step whose featurizer is frozen -----------------------------------------------------------------------------------------------
def test_frozen_featurizer_train_step_takes_the_cached_route(tmp_path):
    from dfol_vqa_amd import experiment, training
    from dfol_vqa_amd import synthetic as syn
    from test_feature_store import write_chunks
    counts = [40, 10, 25, 33]
    chunks, info = write_chunks(tmp_path, feature_dim=2048, max_obj=MAX_OBJ, counts=counts, per_chunk=2, seed=23)
    paths, names = syn.write_synthetic_ontology(str(tmp_path / "ontology"))
    cfg = syn.reference_config(paths, freeze_featurizer=True, freeze_attribute_network=False, freeze_relation_network=False,
                               freeze_embedding_network=False, dropout=0.0)
    ont = experiment.build_ontology(cfg)
    torch.manual_seed(3)
    model = experiment.build_model(cfg, ont).to(DEV).train()
    assert not any(p.requires_grad for p in model._featurizer.parameters()) and any(p.requires_grad for p in model._oracle.parameters())
    with open(paths["attribute_file"]) as f:
        cats = json.load(f)
    qs = syn.full_size_questions("exist", 4, 10, MAX_OBJ, names, cats, 31, with_scene=False)
    for q, im in zip(qs, [2, 0, 3, 1]):
        q["image_id"] = "img%03d" % im
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    keys = ("feature_store_featurized", "feature_store_featurize", "feature_store_direct", "feature_store_direct_materialized")
    runs = {}
    for form in ("direct", "featurized"):
        store = DeviceFeatureStore(str(tmp_path), "objs", chunks, info, DEV, **{form: True})
        pbs = data.BatchGQABoxFeaturesCollator(str(tmp_path), "objs", chunks, info, ont, 1, device_store=store.index).collate([dict(q) for q in qs])
        for pb in pbs:
            pb.create_sparse_tensors()
        before = dict(_lib.PATH_COUNTS)
        dev = [pb.to_cuda(DEV) for pb in pbs]
        assert isinstance(dev[0]._object_features, StoreRows)
        loss, _ = training.train_batch(model, opt, dev, clip_norm=0.65)
        grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}
        runs[form] = (loss, grads, {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in keys})
    (l0, g0, c0), (l1, g1, c1) = runs["direct"], runs["featurized"]
    print("loss", l0, l1, "counters", c0, c1)
    assert np.float64(l0).tobytes() == np.float64(l1).tobytes() and np.isfinite(l0)
    assert sorted(g0) == sorted(g1) and g0 and all(k.startswith("_oracle") for k in g0)
    assert any(np.abs(g).max() > 0 for g in g0.values())
    for k in g0:
        assert np.array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32)), k
    assert c0["feature_store_featurized"] == c0["feature_store_featurize"] == 0
    assert c0["feature_store_direct"] + c0["feature_store_direct_materialized"] == 1
    if os.environ.get("DFOL_DENSE_WIDE") != "2":
        assert c0["feature_store_direct_materialized"] == 1                     # (138 rows are not the wide kernel's by default)
    assert c1 == {"feature_store_featurized": 1, "feature_store_featurize": 1, "feature_store_direct": 0, "feature_store_direct_materialized": 0}
