"""GPU tests of the feature store's index form (`DeviceFeatureStore(..., direct=True)`): the row / box kernel (csrc/dfol_store.hip), the wide
product over indexed rows (csrc/dfol_dense_wide.hip, ROWS) against the wide product over the gathered matrix, and the routes - featurizer,
native executor, shared scenes, train step, captured forward - against a `direct=False` store.  Every comparison is bit equality."""

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
from dfol_vqa_amd.data import DeviceFeatureStore, ObjectFeatureRef  # noqa: E402
from dfol_vqa_amd.feature_store import StoreRows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAX_OBJ, S = 40, 6
HERE = os.path.dirname(os.path.abspath(__file__))


def bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def refs_of(store):
    """Ragged counts with an empty image, slots out of order and repeated; the last slot alone with every row; all counts zero; no image."""
    return {"ragged": ObjectFeatureRef(store.id, [3, 0, 5, 5, 2, 1, 3], [40, 0, 37, 1, 40, 13, 7]),
            "last": ObjectFeatureRef(store.id, [S - 1], [MAX_OBJ]),
            "zeros": ObjectFeatureRef(store.id, [2, 0, 2], [0, 0, 0]),
            "none": ObjectFeatureRef(store.id, [], [])}


def ref_of_rows(store, O):
    """A ref of exactly O object rows: slots out of order and repeated, full images and one ragged image at the end."""
    order = [5, 2, 5, 0, 3, 1, 4, 5]
    n = (O + MAX_OBJ - 1) // MAX_OBJ
    counts = [MAX_OBJ] * (n - 1) + [O - MAX_OBJ * (n - 1)]
    return ObjectFeatureRef(store.id, [order[i % len(order)] for i in range(n)], counts)


@pytest.fixture(scope="module", params=[128, 132, 516], ids=lambda f: "F%d" % f)
def corpus(request, tmp_path_factory):
    """A synthetic store of S = 6 images x 40 rows per feature width, with the weights of the products over it; built once per width."""
    from test_feature_store import write_chunks
    F = request.param
    d = tmp_path_factory.mktemp("direct_F%d" % F)
    chunks, info = write_chunks(d, feature_dim=F, max_obj=MAX_OBJ, counts=[MAX_OBJ, 1, 13, 37, 40, 40], per_chunk=3, seed=F)
    store = DeviceFeatureStore(str(d), "objs", chunks, info, DEV, direct=True)
    assert (store.S, store.max_obj, store.F, store.direct) == (S, MAX_OBJ, F, True)
    g = torch.Generator(device="cpu").manual_seed(F)
    weights = {N: ((torch.randn(N, F, generator=g) / np.sqrt(F)).to(DEV), torch.randn(N, generator=g).to(DEV)) for N in (260, 512)}
    return store, weights


# ---- 1. dfol_store_rows_f32 ------------------------------------------------------------------------------------------------------------
def test_store_rows_kernel(corpus):
    store, _ = corpus
    F = store.F
    for name, ref in refs_of(store).items():
        rows = store.rows(ref)
        O = int(ref.counts.sum())
        assert isinstance(rows, StoreRows) and rows.O == O and rows.shape == (O, F + 6) and rows.device == DEV and rows.is_cuda
        assert rows.src_row.dtype == torch.int32 and tuple(rows.src_row.shape) == (O,) and tuple(rows.box6.shape) == (O, 6)
        assert rows.table.data_ptr() == store.features.data_ptr() and tuple(rows.table.shape) == (S * MAX_OBJ, F)
        assert np.array_equal(rows.src_row.cpu().numpy(), ref.source_rows(MAX_OBJ)), name
        assert np.array_equal(bits(rows.box6), bits(store.gather(ref)[:, F:F + 6])), name
    assert int(store.rows(refs_of(store)["last"]).src_row[-1]) == S * MAX_OBJ - 1           # the table's last row
    h = _lib.load()
    assert h.dfol_store_rows_f32(None, None, None, None, 0, S, MAX_OBJ, None, None, None) == 0           # I == 0: no launch, no error
    # rows into an existing StoreRows, sentinel-filled: only the ref's rows are written
    ref = refs_of(store)["ragged"]
    rows = store.rows(ref)
    rows.src_row.fill_(-7)
    rows.box6.fill_(-12345.5)
    assert store.rows(ref, out=rows) is rows
    assert np.array_equal(rows.src_row.cpu().numpy(), ref.source_rows(MAX_OBJ)) and np.array_equal(bits(rows.box6), bits(store.gather(ref)[:, F:]))
    with pytest.raises(_lib.DfolError):
        store.rows(refs_of(store)["last"], out=rows)                                    # another batch shape
    for bad in (ObjectFeatureRef(store.id, [S], [1]), ObjectFeatureRef(store.id, [0], [MAX_OBJ + 1]), ObjectFeatureRef("another store", [0], [1])):
        with pytest.raises(_lib.DfolError):
            store.rows(bad)


# ---- 2. the wide product over indexed rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O", [1, 127, 128, 131, 300])
def test_wide_rows_equals_wide_over_the_gathered_matrix(corpus, O):
    store, weights = corpus
    F = store.F
    ref = ref_of_rows(store, O)
    rows, matrix = store.rows(ref), store.gather(ref)
    for N, (W, b) in weights.items():
        for act in (_lib.ACT_NONE, _lib.ACT_SIGMOID):
            want = _lib.linear_wide(matrix[:, :F], W, b, act)
            got = _lib.linear_wide_rows(rows.table, rows.src_row, W, b, act)
            assert got.shape == want.shape == (O, N) and np.array_equal(bits(got), bits(want)), (F, N, act, O)
    # into a strided destination (the object matrix's first columns), the padding untouched
    W, b = weights[512]
    wide = torch.full((O, 512 + 4), -12345.5, device=DEV)
    _lib.linear_wide_rows(rows.table, rows.src_row, W, b, _lib.ACT_SIGMOID, out=wide[:, :512])
    assert np.array_equal(bits(wide[:, :512]), bits(_lib.linear_wide(matrix[:, :F], W, b, _lib.ACT_SIGMOID))) and bool((wide[:, 512:] == -12345.5).all())


def test_wide_rows_on_the_tables_last_row(corpus):
    """The last row of the table with every row of its image, and alone (M = 1): the clamped rows and the clamped K tail stay inside the table -
    the store's features end where the table ends."""
    store, weights = corpus
    F = store.F
    W, b = weights[260]
    last = refs_of(store)["last"]
    rows, matrix = store.rows(last), store.gather(last)
    assert np.array_equal(bits(_lib.linear_wide_rows(rows.table, rows.src_row, W, b, _lib.ACT_NONE)), bits(_lib.linear_wide(matrix[:, :F], W, b, _lib.ACT_NONE)))
    alone = torch.tensor([S * MAX_OBJ - 1], dtype=torch.int32, device=DEV)
    got = _lib.linear_wide_rows(rows.table, alone, W, b, _lib.ACT_SIGMOID)
    assert np.array_equal(bits(got), bits(_lib.linear_wide(matrix[MAX_OBJ - 1:, :F], W, b, _lib.ACT_SIGMOID)))
    # table rows that are 8-byte, not 16-byte aligned (a 128-column product over a table of row stride F = 132 + 2 floats: the two-float loads)
    if F == 132:
        padded = torch.zeros(S * MAX_OBJ, F + 2, device=DEV)
        padded[:, :F] = rows.table
        W128, b128 = W[:, :128].contiguous(), b
        want = _lib.linear_wide(padded[rows.src_row.long()][:, :128], W128, b128, _lib.ACT_NONE)
        assert np.array_equal(bits(_lib.linear_wide_rows(padded[:, :128], rows.src_row, W128, b128, _lib.ACT_NONE)), bits(want))


def test_wide_rows_across_block_boundaries():
    """More 128-row blocks than CUs: workgroups go on to a second block with that block's rows in flight (the index is read at the transition)."""
    from test_feature_store import write_chunks
    import tempfile
    F, N = 128, 260
    with tempfile.TemporaryDirectory() as d:
        chunks, info = write_chunks(d, feature_dim=F, max_obj=MAX_OBJ, counts=[MAX_OBJ] * S, per_chunk=3, seed=5)
        store = DeviceFeatureStore(d, "objs", chunks, info, DEV, direct=True)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    O = 128 * (cus + 3) + 5
    ref = ref_of_rows(store, O)
    rows, matrix = store.rows(ref), store.gather(ref)
    g = torch.Generator(device="cpu").manual_seed(1)
    W, b = (torch.randn(N, F, generator=g) / np.sqrt(F)).to(DEV), torch.randn(N, generator=g).to(DEV)
    got = _lib.linear_wide_rows(rows.table, rows.src_row, W, b, _lib.ACT_SIGMOID)
    want = _lib.linear_wide(matrix[:, :F], W, b, _lib.ACT_SIGMOID)
    assert got.shape == (O, N) and torch.equal(got, want)


# ---- 3. the range word -----------------------------------------------------------------------------------------------------------------
def test_range_word_covers_the_indexed_rows_only(corpus):
    store, weights = corpus
    F = store.F
    W, b = weights[512]
    ref = ObjectFeatureRef(store.id, [3, 0, 3], [37, 40, 5])                  # slots 1, 2, 4, 5 and rows 37 .. 39 of slot 3 are not named
    rows = store.rows(ref)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib = _lib.load()

    def flagged(route):
        word.zero_()
        lib.dfol_set_range_status(word.data_ptr())
        try:
            if route == "rows":
                _lib.linear_wide_rows(rows.table, rows.src_row, W, b, _lib.ACT_NONE)
            else:
                _lib.linear_wide(store.gather(ref)[:, :F], W, b, _lib.ACT_NONE)
        finally:
            lib.dfol_set_range_status(None)
        return int(word.item()) & _lib.RANGE_X_OVERFLOW
    assert flagged("rows") == 0 and flagged("matrix") == 0
    for slot, row, col, hot in ((3, 36, F - 1, True), (0, 0, 0, True), (3, 38, 5, False), (5, MAX_OBJ - 1, F - 1, False), (1, 0, 0, False)):
        keep = float(store.features[slot, row, col])
        store.features[slot, row, col] = 7.0e4
        try:
            assert bool(flagged("rows")) == hot and bool(flagged("matrix")) == hot, (slot, row, col)
        finally:
            store.features[slot, row, col] = keep
    assert flagged("rows") == 0


# ---- 9. StoreRows.materialize / select_rows --------------------------------------------------------------------------------------------
def test_materialize_and_select_rows(corpus):
    store, _ = corpus
    for name, ref in refs_of(store).items():
        rows, want = store.rows(ref), store.gather(ref)
        got = rows.materialize()
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), name
        buf = torch.full((want.shape[0], want.shape[1] + 3), -12345.5, device=DEV)
        assert rows.materialize(out=buf) is buf
        assert np.array_equal(bits(buf[:, :want.shape[1]]), bits(want)) and bool((buf[:, want.shape[1]:] == -12345.5).all())
    ref = refs_of(store)["ragged"]
    rows, want = store.rows(ref), store.gather(ref)
    pick = torch.tensor([137, 0, 0, 40, 77, 39, 76], dtype=torch.int64, device=DEV)
    sel = rows.select_rows(pick)
    assert sel.O == 7 and sel.shape == (7, store.F + 6)
    assert np.array_equal(sel.src_row.cpu().numpy(), ref.source_rows(MAX_OBJ)[pick.cpu().numpy()])
    assert np.array_equal(bits(sel.materialize()), bits(want.index_select(0, pick)))
    assert np.array_equal(bits(sel.select_rows(torch.tensor([6, 1], device=DEV)).materialize()), bits(want.index_select(0, pick[[6, 1]])))
    # resolve: a direct store hands ProgramBatch.to_cuda a StoreRows, a plain one the matrix
    from dfol_vqa_amd import feature_store
    assert isinstance(feature_store.resolve(ref, DEV), StoreRows)
    store.direct = False
    try:
        assert isinstance(feature_store.resolve(ref, DEV), torch.Tensor)
    finally:
        store.direct = True


# ---- 4 - 6, 8. the routes, one child process per setting of DFOL_DENSE_WIDE (the library reads it once) ----------------------------------
@pytest.mark.parametrize("mode", ["wide", "default"])
def test_direct_store_equals_plain_store_through_the_interpreter(mode, tmp_path):
    """Full-size synthetic model, 3 - 5 images of 10 - 40 objects: `direct=True` against `direct=False` with the same collator and questions on
    the native executor and the Python loop, with and without shared scenes, and a captured forward served a second scene through
    `rows(ref2, out=rows)` - identical log-probabilities and answers; `wide` (DFOL_DENSE_WIDE=2) counts the direct route once per batch,
    `default` counts the materialised one and no direct one.  (tests/_store_direct_worker.py; one child at a time.)"""
    env = dict(os.environ)
    env.pop("DFOL_DENSE_WIDE", None)
    env.pop("DFOL_NATIVE", None)
    if mode == "wide":
        env["DFOL_DENSE_WIDE"] = "2"
    out = subprocess.run([sys.executable, os.path.join(HERE, "_store_direct_worker.py"), mode, str(tmp_path)], env=env, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report == {"mode": mode, "cases": 12, "graph": True}


# ---- 7. a train step on a direct store ---------------------------------------------------------------------------------------------------
def test_train_batch_on_a_direct_store_materialises(tmp_path):
    from dfol_vqa_amd import experiment, training
    from dfol_vqa_amd import synthetic as syn
    from test_feature_store import write_chunks
    counts = [40, 10, 25, 33]
    chunks, info = write_chunks(tmp_path, feature_dim=2048, max_obj=MAX_OBJ, counts=counts, per_chunk=2, seed=23)
    paths, names = syn.write_synthetic_ontology(str(tmp_path / "ontology"))
    cfg = syn.reference_config(paths, freeze_featurizer=False, freeze_attribute_network=False, freeze_relation_network=False,
                               freeze_embedding_network=False, dropout=0.0)
    ont = experiment.build_ontology(cfg)
    torch.manual_seed(3)
    model = experiment.build_model(cfg, ont).to(DEV).train()
    with open(paths["attribute_file"]) as f:
        cats = json.load(f)
    qs = syn.full_size_questions("exist", 4, 10, MAX_OBJ, names, cats, 31, with_scene=False)
    for q, im in zip(qs, [2, 0, 3, 1]):
        q["image_id"] = "img%03d" % im
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    runs = {}
    for direct in (False, True):
        store = DeviceFeatureStore(str(tmp_path), "objs", chunks, info, DEV, direct=direct)
        pbs = data.BatchGQABoxFeaturesCollator(str(tmp_path), "objs", chunks, info, ont, 1, device_store=store.index).collate([dict(q) for q in qs])
        for pb in pbs:
            pb.create_sparse_tensors()
        before = dict(_lib.PATH_COUNTS)
        dev = [pb.to_cuda(DEV) for pb in pbs]
        assert isinstance(dev[0]._object_features, StoreRows if direct else torch.Tensor)
        loss, _ = training.train_batch(model, opt, dev, clip_norm=0.65)
        grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}
        runs[direct] = (loss, grads, {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in ("feature_store_direct", "feature_store_direct_materialized")})
    (l0, g0, c0), (l1, g1, c1) = runs[False], runs[True]
    assert np.float64(l0).tobytes() == np.float64(l1).tobytes() and np.isfinite(l0)
    assert sorted(g0) == sorted(g1) and any(k.startswith("_featurizer") for k in g0)
    for k in g0:
        assert np.array_equal(g0[k].view(np.uint32), g1[k].view(np.uint32)), k
    assert c0 == {"feature_store_direct": 0, "feature_store_direct_materialized": 0}
    assert c1 == {"feature_store_direct": 0, "feature_store_direct_materialized": len(qs) and 1}
