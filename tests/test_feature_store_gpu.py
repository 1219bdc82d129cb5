"""GPU tests of the device-resident feature store: the gather kernel (csrc/dfol_store.hip) against the host collator bit for bit, and
store-backed batches through ProgramBatch.to_cuda, the interpreter and DataLoader workers against the host route."""

import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
import dfol_vqa_amd as D  # noqa: E402
from dfol_vqa_amd import _lib, data  # noqa: E402
from dfol_vqa_amd.data import DeviceFeatureStore, ObjectFeatureRef  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def ontology(mini_ontology_paths):
    p = mini_ontology_paths
    return D.GQAOntology(p["attribute_file"], p["class_file"], p["vocabulary_file"], p["word_embedding_file"],
                         relation_json_path=p["relation_file"])


def bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


# ---- the kernel against the host collator ---------------------------------------------------------------------------------------------
MAX_OBJ = 9                                             # odd, and more rows than a workgroup has wavefronts
COUNTS = [1, MAX_OBJ, 4, 2, MAX_OBJ, 3, 7]              # images of 1 object and of max_obj objects; 3 + 3 + 1 images in three chunks
ORDER = [6, 4, 3, 3, 1, 0, 5, 2, 1]                     # slots in descending order, repeats, then unordered


@pytest.fixture(scope="module", params=[2048, 7, 10], ids=lambda f: "F%d" % f)
def corpus(request, tmp_path_factory, ontology):
    """(store, plain collator, questions, the host collator's matrix) over tiny synthetic .npz chunks; computed once per width."""
    from test_feature_store import write_chunks
    F = request.param
    d = tmp_path_factory.mktemp("store_F%d" % F)
    chunks, info = write_chunks(d, feature_dim=F, max_obj=MAX_OBJ, counts=COUNTS, per_chunk=3, seed=F)
    store = DeviceFeatureStore(str(d), "objs", chunks, info, DEV)
    plain = data.BatchGQABoxFeaturesCollator(str(d), "objs", chunks, info, ontology, 1)
    backed = data.BatchGQABoxFeaturesCollator(str(d), "objs", chunks, info, ontology, 1, device_store=store.index)
    questions = [{"image_id": "img%03d" % k} for k in ORDER]
    want, want_bi = plain.collate_object_features(questions)
    want.numpy().setflags(write=False)
    return store, plain, backed, questions, want, want_bi


def test_store_layout(corpus):
    store, plain, backed, questions, want, _ = corpus
    F = want.shape[1] - 6
    assert (store.S, store.max_obj, store.F, store.resident_chunks) == (9, MAX_OBJ, F, 3)
    assert store.features.shape == (9, MAX_OBJ, F) and store.boxes.shape == (9, MAX_OBJ, 4) and store.sizes.shape == (9, 2)
    assert store.features.device == store.boxes.device == store.sizes.device == DEV
    assert store.nbytes == sum(t.numel() * 4 for t in (store.features, store.boxes, store.sizes))
    assert store.index.get("img006") == (6, 7) and store.sizes[6].tolist() == [634.0, 486.0]


def test_gather_equals_the_host_collator(corpus):
    store, plain, backed, questions, want, want_bi = corpus
    ref, bi = backed.collate_object_features(questions)
    assert isinstance(ref, ObjectFeatureRef) and ref.slots.tolist() == ORDER and torch.equal(bi, want_bi)
    got = store.gather(ref)
    assert got.shape == want.shape and got.dtype == torch.float32 and got.device == DEV and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want.numpy()) and np.array_equal(bits(got), bits(want))
    pinned = store.gather(backed.collate_object_features(questions)[0].pin_memory())          # (the index arrays from the ref's own pinned copy)
    assert np.array_equal(bits(pinned), bits(want))


@pytest.mark.parametrize("pad", [1, 2, 3, 10])
def test_gather_into_wider_rows_leaves_the_padding(corpus, pad):
    """ld_out > F + 6: with F = 2048 the rows are 4-byte (pad 1, 3), 16-byte (pad 2) and alternately 16- / 8-byte (pad 10, as pad 0) aligned."""
    store, plain, backed, questions, want, _ = corpus
    ref, _ = backed.collate_object_features(questions)
    O, W = want.shape
    wide = torch.full((O + 2, W + pad), SENTINEL, device=DEV)
    out = store.gather(ref, out=wide[1:O + 1])                                # all columns handed over: the kernel writes F + 6 of them
    assert out.data_ptr() == wide[1:].data_ptr()
    host = wide.cpu().numpy()
    assert np.array_equal(host[1:O + 1, :W].view(np.uint32), bits(want))
    assert np.all(host[1:O + 1, W:] == SENTINEL) and np.all(host[0] == SENTINEL) and np.all(host[O + 1] == SENTINEL)
    wide.fill_(SENTINEL)
    store.gather(ref, out=wide[1:O + 1, :W])                                  # a strided [O, F + 6] view
    host = wide.cpu().numpy()
    assert np.array_equal(host[1:O + 1, :W].view(np.uint32), bits(want)) and np.all(host[1:O + 1, W:] == SENTINEL)


def test_gather_into_an_existing_buffer_and_empty_batches(corpus):
    store, plain, backed, questions, want, _ = corpus
    ref, _ = backed.collate_object_features(questions)
    buf = torch.full(tuple(want.shape), SENTINEL, device=DEV)
    assert store.gather(ref, out=buf) is buf
    assert np.array_equal(bits(buf), bits(want))
    # unaligned output rows (a buffer that starts 4 bytes into an allocation)
    flat = torch.full((want.numel() + 1,), SENTINEL, device=DEV)
    store.gather(ref, out=flat[1:].view(want.shape))
    assert np.array_equal(bits(flat[1:].view(want.shape)), bits(want)) and float(flat[0]) == SENTINEL
    F = want.shape[1] - 6
    empty = store.gather(ObjectFeatureRef(store.id, [], []))                  # O == 0: no launch
    assert empty.shape == (0, F + 6) and empty.device == DEV
    none = store.gather(ObjectFeatureRef(store.id, [2, 0], [0, 0]))
    assert none.shape == (0, F + 6)
    for bad in (ObjectFeatureRef(store.id, [9], [1]), ObjectFeatureRef(store.id, [-1], [1]), ObjectFeatureRef(store.id, [0], [MAX_OBJ + 1]),
                ObjectFeatureRef("another store", [0], [1])):
        with pytest.raises(_lib.DfolError):                                   # bounds are checked on the host, before the launch
            store.gather(bad)
    with pytest.raises(_lib.DfolError):
        store.gather(ref, out=torch.empty(want.shape[0] + 1, want.shape[1], device=DEV))
    idx = store.upload_index(ref)                                             # uploaded once, gathered twice
    again = store.gather(ref, index=idx)
    assert np.array_equal(bits(again), bits(want)) and np.array_equal(bits(store.gather(ref, out=buf.fill_(SENTINEL), index=idx)), bits(want))
    h = _lib.load()
    assert h.dfol_gather_object_rows_f32(None, None, None, None, None, 0, 4, 8, None, 14, None) == 0       # I == 0
    for I, max_obj, F, ld in ((1, 4, 0, 14), (1, 0, 8, 14), (1, 4, 8, 13)):
        assert h.dfol_gather_object_rows_f32(None, None, None, None, None, I, max_obj, F, None, ld, None) != 0
        assert b"gather_object_rows" in h.dfol_last_error()


def test_gather_beyond_two_to_the_31_elements():
    """A store of more than 2^31 feature elements (the corpus is ~3e10): the last slot's rows lie past what 32-bit element offsets reach.
    The store tensors are allocated, not filled - only the gathered slots hold data.  Footprint: 8.6 GB of device memory for the length of
    the test; an offset past 2^31 elements needs that many elements behind the pointer, whatever max_obj and F are."""
    max_obj, F = 100, 2048
    S = (1 << 31) // (max_obj * F) + 2
    feats = torch.empty((S, max_obj, F), dtype=torch.float32, device=DEV)
    boxes = torch.empty((S, max_obj, 4), dtype=torch.float32, device=DEV)
    sizes = torch.empty((S, 2), dtype=torch.float32, device=DEV)
    assert (S - 1) * max_obj * F > (1 << 31)
    g = torch.Generator(device="cpu").manual_seed(5)
    slots, counts = [S - 1, 0, S - 1], [max_obj, 3, 1]
    for s in set(slots):
        feats[s] = torch.randn(max_obj, F, generator=g).to(DEV)
        boxes[s] = (torch.rand(max_obj, 4, generator=g) * 300).to(DEV)
        sizes[s] = torch.tensor([640.0 + s % 7, 480.0])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out = torch.full((int(off[-1]), F + 6), SENTINEL, device=DEV)
    _lib.gather_object_rows(feats, boxes, sizes, torch.tensor(slots, dtype=torch.int32, device=DEV), torch.tensor(off, device=DEV), out)
    want = []
    for s, n in zip(slots, counts):
        b = boxes[s, :n].cpu().numpy().copy()
        b[:, 2] -= b[:, 0]
        b[:, 3] -= b[:, 1]
        want.append(np.concatenate([feats[s, :n].cpu().numpy(), np.tile(sizes[s].cpu().numpy()[None], (n, 1)), b], 1))
    assert np.array_equal(bits(out), np.concatenate(want, 0).view(np.uint32))


def test_memory_refusal(tmp_path, monkeypatch):
    """max_bytes=None takes the whole corpus or nothing: when it does not fit 80 % of the free device memory, DfolError names both sizes."""
    from test_feature_store import write_chunks
    chunks, info = write_chunks(tmp_path, feature_dim=10, max_obj=MAX_OBJ, counts=COUNTS, per_chunk=3)
    need = 9 * 4 * (MAX_OBJ * 10 + MAX_OBJ * 4 + 2)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (need + need // 8, 1 << 38))       # need > 0.8 x free
    with pytest.raises(_lib.DfolError) as err:
        DeviceFeatureStore(str(tmp_path), "objs", chunks, info, DEV)
    assert str(need) in str(err.value) and str(int(0.8 * (need + need // 8))) in str(err.value)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (2 * need, 1 << 38))
    assert DeviceFeatureStore(str(tmp_path), "objs", chunks, info, DEV).S == 9
    part = DeviceFeatureStore(str(tmp_path), "objs", chunks, info, DEV, max_bytes=need - 1)                # an explicit budget: whole chunks
    assert (part.S, part.resident_chunks) == (6, 2) and part.index.get("img006") == (-1, 7)
    with pytest.raises(_lib.DfolError):
        DeviceFeatureStore(str(tmp_path), "objs", chunks, info, "cpu")


# ---- through ProgramBatch.to_cuda and the interpreter ------------------------------------------------------------------------------------
def test_g16_through_the_store(ontology, golden_dir):
    """The reference-written .h5 feature chunks (golden g16): a store-backed batch's device matrix is the host route's uploaded tensor."""
    from test_data_path import _h5_or_skip
    from test_feature_store import items_of
    _h5_or_skip()
    a, meta = gu.load("g16_hdf5_containers")
    h5 = os.path.join(golden_dir, "h5")
    info = os.path.join(h5, "gqa_objects_info.json")
    store = DeviceFeatureStore(h5, "gqa_objects", 2, info, DEV)
    plain = data.BatchGQABoxFeaturesCollator(h5, "gqa_objects", 2, info, ontology, 1)
    backed = data.BatchGQABoxFeaturesCollator(h5, "gqa_objects", 2, info, ontology, 1, device_store=store.index)
    items = items_of(ontology, meta["chunks"]["order"])
    host = plain.collate(copy.deepcopy(items))[0].to_cuda(DEV)
    before = _lib.PATH_COUNTS["feature_store_batch"], _lib.PATH_COUNTS["feature_store_miss"]
    pb = backed.collate(copy.deepcopy(items))[0]
    assert isinstance(pb._object_features, ObjectFeatureRef)
    dev = pb.to_cuda(DEV)
    assert (_lib.PATH_COUNTS["feature_store_batch"], _lib.PATH_COUNTS["feature_store_miss"]) == (before[0] + 1, before[1])
    assert isinstance(dev._object_features, torch.Tensor) and dev._object_features.device == DEV
    assert dev._object_features.shape == host._object_features.shape and np.array_equal(bits(dev._object_features), bits(host._object_features))
    assert np.array_equal(dev._object_features.cpu().numpy(), a["features"])               # bit-equal here; the host collator's own test allows 1e-6
    assert torch.equal(dev._object_batch_index, host._object_batch_index) and dev._object_nums == host._object_nums
    pinned = backed.collate(copy.deepcopy(items))[0].pin_memory()
    assert pinned._object_features._pinned.is_pinned()
    assert np.array_equal(bits(pinned.to_cuda(DEV)._object_features), bits(host._object_features))


def g18_items(ontology, golden_dir):
    a, meta = gu.load("g18_h5_end_to_end")
    h5 = os.path.join(golden_dir, "h5")
    for name in sorted(meta["files"]):
        ds = data.ProgramDataset(os.path.join(h5, name + ".h5"), ontology, in_memory=False, shuffle_options=False)
        yield name, meta["files"][name], [ds[i] for i in range(len(ds))]


def run_model(model, pbs):
    for pb in pbs:
        pb.create_sparse_tensors()
    with torch.no_grad():
        res = model([pb.to_cuda(DEV) for pb in pbs], False)
    return res["log_probability"].cpu().numpy(), res["answer"], res


def test_g18_end_to_end_with_a_store_backed_collator(ontology, golden_dir):
    """Golden g18 (the reference's files -> answers) with the features served from the store: bit-identical to the host route run beside it."""
    from test_data_path import _h5_or_skip
    from test_interpreter_gpu import neural_model
    _h5_or_skip()
    a, meta = gu.load("g18_h5_end_to_end")
    h5 = os.path.join(golden_dir, "h5")
    info = os.path.join(h5, meta["info"])
    store = DeviceFeatureStore(h5, meta["feature_prefix"], meta["chunk_num"], info, DEV)
    plain = data.BatchGQABoxFeaturesCollator(h5, meta["feature_prefix"], meta["chunk_num"], info, ontology, 1)
    backed = data.BatchGQABoxFeaturesCollator(h5, meta["feature_prefix"], meta["chunk_num"], info, ontology, 1, device_store=store.index)
    model = neural_model(ontology, meta["config"], {k[2:]: a[k] for k in a.files if k.startswith("w:")})
    seen = 0
    for name, fm, items in g18_items(ontology, golden_dir):
        c0 = dict(_lib.PATH_COUNTS)
        lp_host, ans_host, _ = run_model(model, plain.collate(copy.deepcopy(items)))
        c1 = dict(_lib.PATH_COUNTS)
        pbs = backed.collate(copy.deepcopy(items))
        lp, ans, res = run_model(model, pbs)
        c2 = dict(_lib.PATH_COUNTS)
        assert np.array_equal(lp.view(np.uint32), lp_host.view(np.uint32)) and ans == ans_host, name
        gu.check_logprob(lp, a[name + ":lp_f32"], a[name + ":lp_f64"], name)
        assert int(res["type"]) == fm["type"], name
        assert c2.get("feature_store_batch", 0) - c1.get("feature_store_batch", 0) == len(pbs) == 1
        assert c1.get("feature_store_batch", 0) == c0.get("feature_store_batch", 0)
        assert c2.get("feature_store_miss", 0) == c0.get("feature_store_miss", 0)
        assert c2.get("native_program", 0) - c1.get("native_program", 0) == c1.get("native_program", 0) - c0.get("native_program", 0), name
        seen += 1
    assert seen == 8


def rechunk_g18(golden_dir, directory, per_chunk=12):
    """The g18 feature chunks (three .h5 files of eight images) rewritten as two .npz chunks of twelve, with their info JSON."""
    a, meta = gu.load("g18_h5_end_to_end")
    h5 = os.path.join(golden_dir, "h5")
    with open(os.path.join(h5, meta["info"])) as f:
        info = json.load(f)
    chunks = [data._open_arrays(os.path.join(h5, "%s_%d.h5" % (meta["feature_prefix"], c))) for c in range(meta["chunk_num"])]
    feats = np.concatenate([np.asarray(c["features"][...], np.float32) for c in chunks], 0)
    boxes = np.concatenate([np.asarray(c["bboxes"][...], np.float32) for c in chunks], 0)
    rows = chunks[0]["features"].shape[0]
    new_info = {}
    for im, inf in info.items():
        k = inf["file"] * rows + inf["idx"]
        new_info[im] = dict(inf, file=k // per_chunk, idx=k % per_chunk)
    n = (len(feats) + per_chunk - 1) // per_chunk
    for c in range(n):
        np.savez(os.path.join(str(directory), "re_%d.npz" % c), features=feats[c * per_chunk:(c + 1) * per_chunk],
                 bboxes=boxes[c * per_chunk:(c + 1) * per_chunk])
    path = os.path.join(str(directory), "re_info.json")
    with open(path, "w") as f:
        json.dump(new_info, f)
    return n, path, feats.shape


def test_partial_residency(ontology, golden_dir, tmp_path):
    """max_bytes with room for one of two chunks: resident batches come from the store, the others over the host route, same results."""
    from test_data_path import _h5_or_skip
    from test_interpreter_gpu import neural_model
    _h5_or_skip()
    a, meta = gu.load("g18_h5_end_to_end")
    n, info, shape = rechunk_g18(golden_dir, tmp_path)
    assert n == 2
    one_chunk = 12 * 4 * (shape[1] * shape[2] + shape[1] * 4 + 2)
    store = DeviceFeatureStore(str(tmp_path), "re", n, info, DEV, max_bytes=2 * one_chunk - 1)
    assert (store.resident_chunks, store.S, store.nbytes) == (1, 12, one_chunk)
    plain = data.BatchGQABoxFeaturesCollator(str(tmp_path), "re", n, info, ontology, 2)                 # two ProgramBatches of three questions
    backed = data.BatchGQABoxFeaturesCollator(str(tmp_path), "re", n, info, ontology, 2, device_store=store.index)
    model = neural_model(ontology, meta["config"], {k[2:]: a[k] for k in a.files if k.startswith("w:")})
    c0 = dict(_lib.PATH_COUNTS)
    kinds = []
    for name, fm, items in g18_items(ontology, golden_dir):
        lp_host, ans_host, _ = run_model(model, plain.collate(copy.deepcopy(items)))
        pbs = backed.collate(copy.deepcopy(items))
        kinds += [getattr(pb, "_feature_source", "store") for pb in pbs]
        lp, ans, _ = run_model(model, pbs)
        assert np.array_equal(lp.view(np.uint32), lp_host.view(np.uint32)) and ans == ans_host, name
    hits, misses = kinds.count("store"), kinds.count("host")
    assert hits > 0 and misses > 0 and hits + misses == 16
    assert _lib.PATH_COUNTS["feature_store_batch"] - c0.get("feature_store_batch", 0) == hits
    assert _lib.PATH_COUNTS["feature_store_miss"] - c0.get("feature_store_miss", 0) == misses


class WorkerCollate(object):
    """The collate function of a DataLoader worker: collates, and checks that the worker process never opens the GPU."""

    def __init__(self, collator):
        self.collator = collator

    def __call__(self, items):
        assert torch.utils.data.get_worker_info() is not None
        assert not torch.cuda.is_initialized()
        pbs = self.collator.collate(items)
        assert not torch.cuda.is_initialized()
        return pbs


def test_dataloader_workers_carry_the_index_only(ontology, golden_dir):
    """Two spawned DataLoader workers collate g18 with the store-backed collator (pickled to them: the index, not the store); the batches
    they hand back resolve in this process to the host route's features."""
    from test_data_path import _h5_or_skip
    _h5_or_skip()
    a, meta = gu.load("g18_h5_end_to_end")
    h5 = os.path.join(golden_dir, "h5")
    info = os.path.join(h5, meta["info"])
    store = DeviceFeatureStore(h5, meta["feature_prefix"], meta["chunk_num"], info, DEV)
    plain = data.BatchGQABoxFeaturesCollator(h5, meta["feature_prefix"], meta["chunk_num"], info, ontology, 1)
    backed = data.BatchGQABoxFeaturesCollator(h5, meta["feature_prefix"], meta["chunk_num"], info, ontology, 1, device_store=store.index)
    files = list(g18_items(ontology, golden_dir))
    items, batches = [], []
    for name, fm, its in files:
        batches.append(list(range(len(items), len(items) + len(its))))
        items += its
    loader = torch.utils.data.DataLoader(items, batch_sampler=batches, num_workers=2, collate_fn=WorkerCollate(backed), pin_memory=True,
                                         multiprocessing_context="spawn")
    seen = 0
    for (name, fm, its), pbs in zip(files, loader):
        assert len(pbs) == 1
        pb, mine, host = pbs[0], backed.collate(copy.deepcopy(its))[0], plain.collate(copy.deepcopy(its))[0]
        ref = pb._object_features
        assert isinstance(ref, ObjectFeatureRef) and ref.store_id == store.id and ref._pinned is not None and ref._pinned.is_pinned()
        assert ref.slots.tolist() == mine._object_features.slots.tolist() and ref.counts.tolist() == mine._object_features.counts.tolist()
        assert torch.equal(pb._object_batch_index, host._object_batch_index) and pb._answers == host._answers == fm["gold"]
        assert [int(x) for x in pb._object_nums] == fm["objects"], name
        assert np.array_equal(bits(pb.to_cuda(DEV)._object_features), bits(host._object_features)), name
        seen += 1
    assert seen == 8


def test_an_unresolvable_ref_raises_uncounted(ontology, tmp_path):
    """A ref whose store is gone raises in to_cuda and is not counted as a store batch."""
    from test_feature_store import items_of, write_chunks
    chunks, info = write_chunks(tmp_path)
    store = DeviceFeatureStore(str(tmp_path), "objs", chunks, info, DEV)
    backed = data.BatchGQABoxFeaturesCollator(str(tmp_path), "objs", chunks, info, ontology, 1, device_store=store.index)
    pb = backed.collate(items_of(ontology, ["img001", "img004"]))[0]
    before = dict(_lib.PATH_COUNTS)
    assert pb.to_cuda(DEV)._object_features.shape == (12, 13)
    assert _lib.PATH_COUNTS["feature_store_batch"] == before.get("feature_store_batch", 0) + 1
    del store, backed
    import gc
    gc.collect()
    with pytest.raises(_lib.DfolError):
        pb.to_cuda(DEV)
    assert _lib.PATH_COUNTS["feature_store_batch"] == before.get("feature_store_batch", 0) + 1
