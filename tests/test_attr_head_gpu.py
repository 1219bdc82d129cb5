"""The fused attribute head (csrc/dfol_pair_h2.hip: attr_head_h2_kernel, dfol_attr_head_h2_f32) against the route it replaces - the
attribute network's two dense layers into a hidden table [O, 300] and dfol_attr_ll_f32 over it.

Both routes round differently (the head keeps the hidden layer in registers and sums its K = 256 products in another order), so each is
compared with the float64 value of the same fp32 inputs (oracle/dfol_oracle.py's formulas): where that value is >= -5, the head's largest
error may be at most twice the present route's plus 1e-6 in log-likelihood.  Cells that no object owns (no-op tokens, columns >= n) must
be bit-equal.  Every case prints both maxima (pytest -s)."""

import os

import numpy as np
import pytest
import torch

from oracle import dfol_oracle as orc

pytestmark = pytest.mark.gpu

D, HID1, HID2, C = 516, 256, 300, 2335


@pytest.fixture(scope="module")
def L():
    from dfol_vqa_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return _lib


@pytest.fixture(scope="module")
def weights(L):
    g = torch.Generator().manual_seed(11)
    dev = torch.device("cuda")
    w1 = (torch.randn(HID1, D, generator=g) / np.sqrt(D)).to(dev)
    b1 = (torch.randn(HID1, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(HID2, HID1, generator=g) / 16).to(dev)
    b2 = (torch.randn(HID2, generator=g) * 0.5).to(dev)
    emb = (torch.randn(C, HID2, generator=g) / 17).to(dev)
    be = (torch.randn(C, generator=g) - 1.0).to(dev)
    return w1, b1, w2, b2, emb, be, L.pair_pack_w2_h2(w2, HID2)


def _requests(n_list, per_image, seed, drop_q=(), noop=0.0, repeat=False, sort=False):
    """per_image predicates for every image (none for those in drop_q), in the order visual_oracle.prefetch_attributes builds them - the
    images once per token list, i.e. NOT sorted by image - unless sort."""
    rng = np.random.RandomState(seed)
    Q = len(n_list)
    pq, col = [], []
    for k in range(per_image):
        for q in range(Q):
            if q in drop_q:
                continue
            pq.append(q)
            col.append(-1 if rng.rand() < noop else (7 if repeat and k % 2 == 0 else int(rng.randint(0, C))))
    pq, col = np.asarray(pq, np.int32), np.asarray(col, np.int32)
    if sort:
        order = np.argsort(pq, kind="stable")
        pq, col = pq[order], col[order]
    return pq, col


def _both(L, weights, n_list, pq, col, seed, scale=1.0):
    """-> (present route's blocks, the head's blocks, float64 blocks with NaN in the cells no object owns) as numpy [P, NS]."""
    w1, b1, w2, b2, emb, be, w2h = weights
    dev = torch.device("cuda")
    rng = np.random.RandomState(seed)
    O = int(sum(n_list))
    NS = max(4, (max(n_list) + 3) // 4 * 4)
    x = torch.from_numpy((rng.randn(O, D) * scale).astype(np.float32)).to(dev)
    off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int32)
    off_d, pq_d, col_d = (torch.from_numpy(a).to(dev) for a in (off, pq, col))
    hidden = L.linear_act(L.linear_act(x, w1, b1, L.ACT_ELU), w2, b2, L.ACT_SIGMOID)
    old = L.attr_ll(hidden, emb, be, off_d, pq_d, col_d, NS, -30.0)
    new = L.attr_head_h2(L.linear_act(x, w1, b1, L.ACT_NONE), w2h, b2, HID2, emb, be, off_d, pq_d, col_d, NS, -30.0)
    torch.cuda.synchronize()
    f64 = lambda t: t.detach().cpu().numpy().astype(np.float64)
    h = orc._sigmoid(orc._linear(orc._elu(orc._linear(f64(x), f64(w1), f64(b1))), f64(w2), f64(b2)))
    ref = np.full((len(pq), NS), np.nan)
    E, B = f64(emb), f64(be)
    for p in range(len(pq)):
        if col[p] >= 0:
            n = n_list[pq[p]]
            ref[p, :n] = orc._log_sigmoid(h[off[pq[p]]:off[pq[p]] + n] @ E[col[p]] + B[col[p]])
    return old.cpu().numpy(), new.cpu().numpy(), ref


def _check(name, old, new, ref):
    owned = ~np.isnan(ref)
    assert owned.any(), "no requested cell"
    # cells no object owns: the default, bit for bit
    assert np.array_equal(old[~owned].view(np.int32), new[~owned].view(np.int32)) and (new[~owned] == -30.0).all()
    assert np.isfinite(new[owned]).all()
    m = owned & (np.nan_to_num(ref, nan=-np.inf) >= -5.0)
    assert m.any(), "no cell with a float64 value >= -5"
    e_old, e_new = np.abs(old[m] - ref[m]).max(), np.abs(new[m] - ref[m]).max()
    e_all = np.abs(new[owned] - ref[owned]).max()
    print("attr_head %-28s cells %8d  max |err| vs float64 (value >= -5): present %.3e  fused %.3e   fused, all cells: %.3e"
          % (name, int(m.sum()), e_old, e_new, e_all))
    assert e_new <= 2.0 * e_old + 1e-6, (name, e_old, e_new)
    return e_old, e_new


def test_head_bench_shape(L, weights):
    n_list = [100] * 256
    pq, col = _requests(n_list, 3, seed=1)                    # 768 predicates: two request windows, tiles over two and three images
    _check("bench 256 x 100, 3 / image", *_both(L, weights, n_list, pq, col, seed=2))


def test_head_ragged_images(L, weights):
    # images of 1, 2, 37 and 100 objects in one batch: tiles over many images, images that start mid-tile, a last partial tile
    n_list = [1, 2, 37, 100, 1, 1, 2, 100, 37, 1, 2, 2, 100, 37, 37, 1, 100, 2, 1, 37] * 3
    pq, col = _requests(n_list, 2, seed=3)
    _check("ragged 1/2/37/100", *_both(L, weights, n_list, pq, col, seed=4))
    pq, col = _requests(n_list, 2, seed=5, sort=True)         # the same sorted by image (the executor's option lists)
    _check("ragged, sorted requests", *_both(L, weights, n_list, pq, col, seed=4))


def test_head_images_without_requests_and_noop_tokens(L, weights):
    n_list = [37, 100, 2, 64, 1, 100, 99, 3] * 4
    pq, col = _requests(n_list, 3, seed=6, drop_q=(0, 5, 6, 7, 13, 31), noop=0.25)
    old, new, ref = _both(L, weights, n_list, pq, col, seed=7)
    assert (col < 0).any()
    _check("no requests / no-op tokens", old, new, ref)


def test_head_more_rows_than_the_staging_area(L, weights):
    # 30 predicates on every image of a tile (the staging area holds 24 rows at 300 hidden columns) and small images, 3 predicates each:
    # ~100 entries per 128-object tile; the rows past the staging area come from global memory
    n_list = [100, 28, 100]
    pq, col = _requests(n_list, 30, seed=8)
    _check("30 predicates per image", *_both(L, weights, n_list, pq, col, seed=9))
    n_list = [3, 4, 5, 2, 1, 6] * 40
    pq, col = _requests(n_list, 3, seed=10)
    _check("small images, 3 / image", *_both(L, weights, n_list, pq, col, seed=11))


def test_head_repeated_columns(L, weights):
    n_list = [100, 37, 2, 100, 64]
    pq, col = _requests(n_list, 6, seed=12, repeat=True)
    old, new, ref = _both(L, weights, n_list, pq, col, seed=13)
    _check("repeated columns", old, new, ref)
    rows = [p for p in range(len(pq)) if col[p] == 7 and pq[p] == 0]
    assert len(rows) >= 2 and all(np.array_equal(new[rows[0]], new[r]) for r in rows[1:])      # the same request twice: the same bits


def test_head_activation_beyond_fp16_range_is_flagged(L, weights):
    """First-layer sums of ~1e6: the ELU outputs saturate in the head, so the launch must leave DFOL_RANGE_X_OVERFLOW in the status word (the bit
    the dense second layer raises for the same input); inputs in range leave the word clean."""
    w1, b1, w2, b2, emb, be, w2h = weights
    dev = torch.device("cuda")
    n_list = [5, 9]
    off = torch.tensor([0, 5, 14], dtype=torch.int32, device=dev)
    pq, col = torch.tensor([0, 1], dtype=torch.int32, device=dev), torch.tensor([3, 4], dtype=torch.int32, device=dev)
    pre1 = torch.randn(14, HID1, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = L.load()
    try:
        lib.dfol_set_range_status(word.data_ptr())
        L.attr_head_h2(pre1, w2h, b2, HID2, emb, be, off, pq, col, 12, -30.0)
        assert int(word.item()) == 0
        pre1[7, 100] = 1.0e6
        L.attr_head_h2(pre1, w2h, b2, HID2, emb, be, off, pq, col, 12, -30.0)
        assert int(word.item()) & L.RANGE_X_OVERFLOW
    finally:
        lib.dfol_set_range_status(None)


def _smoke_model():
    import tempfile
    import dfol_vqa_amd as Dm
    from dfol_vqa_amd import experiment
    from dfol_vqa_amd import synthetic as syn
    dev = torch.device("cuda:0")
    paths, names = syn.write_synthetic_ontology(tempfile.mkdtemp(prefix="dfol_attr_head_"))
    cfg = syn.reference_config(paths)
    ont = experiment.build_ontology(cfg)
    torch.manual_seed(0)
    model = experiment.build_model(cfg, ont)
    with torch.no_grad():
        model._oracle._embedding_network.linear.weight.normal_(0.0, 0.1)
        model._oracle._embedding_network.linear.bias.fill_(-2.0)
    model = model.to(dev).eval()

    class Collater(Dm.ProgramCollaterBase):
        def __init__(self):
            super(Collater, self).__init__("select", "relate", "filter", 1, ontology=ont)

        def collate_object_features(self, questions):
            feats = torch.cat([torch.from_numpy(q["scene"]["X"]) for q in questions], 0)
            bi = torch.cat([torch.full((q["scene"]["n"],), i, dtype=torch.int64) for i, q in enumerate(questions)])
            return feats, bi

        def collate_meta_data(self, questions):
            return {"index": {}, "embedding": torch.zeros(1, 1)}

    qs = []
    for i, n in enumerate((9, 100, 5, 37, 1, 64, 2, 100)):
        br, last = syn.three_hop_program(i, names["nouns"][:8], names["attributes"][:6], names["relations"][:5])
        qs.append(syn.question(i, br, last, "yes", syn.feature_scene(i, n, 2048)))
    oont = orc.Ontology(paths["attribute_file"], paths["class_file"], paths["vocabulary_file"], paths["relation_file"])
    return model, Collater(), qs, oont, dev


def test_interpreter_routes_with_and_without_the_head(L, monkeypatch):
    """The full-size interpreter on a ragged batch: with the head (the default) the executor and the Python operator loop agree bit for bit and
    the hidden table is never built; DFOL_ATTR_HEAD=0 takes the table route again (also bit-equal between the two); both match the float64
    oracle to 1e-5 in probability and give the same answers."""
    model, collater, qs, oont, dev = _smoke_model()
    weights = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if k.startswith("_featurizer.") or k.startswith("_oracle.")}
    ref = orc.run_questions(oont, qs, [q["scene"] for q in qs], np.float64, weights=weights)
    got = {}
    for head in ("1", "0"):
        for native in ("1", "0"):
            monkeypatch.setenv("DFOL_ATTR_HEAD", head)
            monkeypatch.setenv("DFOL_NATIVE", native)
            pbs = collater.collate([dict(q) for q in qs])
            for pb in pbs:
                pb.create_sparse_tensors()
            L.PATH_COUNTS.clear()
            on_dev = [pb.to_cuda(dev) for pb in pbs]
            calls = []                                         # forwards of the attribute network = builds of the hidden table
            hook = model._oracle._attribute_network.register_forward_hook(lambda *a: calls.append(1))
            try:
                with torch.no_grad():
                    res = model(on_dev, False)
            finally:
                hook.remove()
            # with the head nothing on the way builds the table; the table route's Python loop builds it once per batch (the executor runs
            # the layers from its own instruction table, not through the module)
            assert len(calls) == (len(on_dev) if (head, native) == ("0", "0") else 0), (head, native, len(calls))
            routes = dict(L.PATH_COUNTS)
            if native == "1":                                  # the executor's plan takes the head's instruction, or the table route's
                from dfol_vqa_amd import native_plan as NP
                ops = np.concatenate([pb._native_plan.instrs[:, 0] for pb in on_dev])
                assert bool((ops == NP.OP_ATTR_HEAD).any()) == (head == "1") and bool((ops == NP.OP_ATTR_LL).any()) == (head == "0")
            assert routes.get("native_program" if native == "1" else "python_program", 0) >= 1, routes
            if native == "0":
                assert (routes.get("attr_head", 0) >= 1) == (head == "1"), routes
            lp = res["log_probability"].cpu().numpy()
            assert np.abs(np.exp(lp) - np.exp(ref["log_probability"])).max() < 1e-5, (head, native)
            assert res["answer"] == ref["answer"]
            got[head, native] = lp
    assert np.array_equal(got["1", "1"].view(np.int32), got["1", "0"].view(np.int32))
    assert np.array_equal(got["0", "1"].view(np.int32), got["0", "0"].view(np.int32))
    print("attr_head interpreter: max |d log_probability| head vs table route %.3e" % np.abs(got["1", "1"] - got["0", "1"]).max())


def test_scene_keeps_the_head_it_was_prepared_with(L, monkeypatch):
    """A scene prepared with the head answers with it after the switch (or the arithmetic scope) changed: it carries its own packed image."""
    model, collater, qs, oont, dev = _smoke_model()
    monkeypatch.setenv("DFOL_ATTR_HEAD", "1")
    pb = collater.collate([dict(q) for q in qs[:3]])[0].to_cuda(dev)
    with torch.no_grad():
        world = model.build_scene(pb.device, pb._object_features, pb._object_batch_index, pb._meta_data, object_nums=getattr(pb, "_object_nums", None))
        assert world._attr_pre1 is not None
        cols = torch.arange(3, 3 + world._batch_size, dtype=torch.int32, device=dev)
        a = model._oracle._attr_columns(world, world._ident, cols)
        monkeypatch.setenv("DFOL_ATTR_HEAD", "0")
        with L.dense_math("bf16x3"):
            b = model._oracle._attr_columns(world, world._ident, cols)
    assert torch.equal(a, b) and world._hidden_attr_table is None


def test_hidden_table_is_built_for_whoever_reads_it(L, monkeypatch):
    """An inference scene holds the first layer's pre-activations only; world._hidden_attr still answers, with the table route's values."""
    model, collater, qs, oont, dev = _smoke_model()
    monkeypatch.setenv("DFOL_ATTR_HEAD", "1")
    pbs = collater.collate([dict(q) for q in qs[:3]])
    pb = pbs[0].to_cuda(dev)
    with torch.no_grad():
        world = model.build_scene(pb.device, pb._object_features, pb._object_batch_index, pb._meta_data, object_nums=getattr(pb, "_object_nums", None))
        assert world._attr_pre1 is not None and world._hidden_attr_table is None
        hidden = world._hidden_attr
        assert hidden.shape == (world._attr_pre1.shape[0], HID2)
        assert torch.equal(hidden, model._oracle._attribute_network(world._obj))
