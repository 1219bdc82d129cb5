"""CPU tests of the device-resident feature store's host half: the picklable index a collator carries, the ObjectFeatureRef a store-backed
BatchGQABoxFeaturesCollator returns instead of the feature matrix, and the host route it keeps for batches the store does not hold."""

import copy
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfol_vqa_amd as D  # noqa: E402
from dfol_vqa_amd import data  # noqa: E402
from dfol_vqa_amd.data import DeviceFeatureStore, ObjectFeatureRef  # noqa: E402,F401
from dfol_vqa_amd.feature_store import FeatureStoreIndex, StoreLayout  # noqa: E402

F, MAX_OBJ, PER_CHUNK = 7, 6, 3
COUNTS = [1, MAX_OBJ, 4, 2, MAX_OBJ, 3]            # images of 1 object and of max_obj objects both occur


@pytest.fixture(scope="module")
def ontology(mini_ontology_paths):
    p = mini_ontology_paths
    return D.GQAOntology(p["attribute_file"], p["class_file"], p["vocabulary_file"], p["word_embedding_file"],
                         relation_json_path=p["relation_file"])


def write_chunks(directory, feature_dim=F, max_obj=MAX_OBJ, counts=COUNTS, per_chunk=PER_CHUNK, seed=0):
    """Two (or more) tiny .npz feature chunks and their info JSON, in the layout BatchGQABoxFeaturesCollator reads."""
    rng = np.random.RandomState(seed)
    info = {}
    chunks = (len(counts) + per_chunk - 1) // per_chunk
    for c in range(chunks):
        feats = rng.standard_normal((per_chunk, max_obj, feature_dim)).astype(np.float32)
        boxes = np.zeros((per_chunk, max_obj, 4), np.float32)
        boxes[..., :2] = rng.uniform(0, 300, (per_chunk, max_obj, 2))
        boxes[..., 2:] = boxes[..., :2] + rng.uniform(0.1, 333.3, (per_chunk, max_obj, 2))
        np.savez(os.path.join(str(directory), "objs_%d.npz" % c), features=feats, bboxes=boxes)
        for i in range(per_chunk):
            k = c * per_chunk + i
            if k < len(counts):
                info["img%03d" % k] = {"objectsNum": int(counts[k]), "width": 640 - k, "height": 480 + k, "idx": i, "file": c}
    path = os.path.join(str(directory), "info.json")
    with open(path, "w") as f:
        json.dump(info, f)
    return chunks, path


def question(image_id, k=0):
    return {"imageId": image_id, "answer": "yes", "question": "q", "question_id": str(k),
            "program": {"branches": [[{"operator": "select", "arguments": ["dog"]}, {"operator": "filter", "arguments": ["red"]}]],
                        "last_op": {"operator": "exist", "arguments": []}}}


def items_of(ontology, image_ids):
    ds = data.ProgramDataset([question(im, k) for k, im in enumerate(image_ids)], ontology, in_memory=True)
    return [ds[i] for i in range(len(ds))]


def collators(tmp_path, ontology, max_bytes=None, **kw):
    chunks, info = write_chunks(tmp_path)
    lay = StoreLayout(str(tmp_path), "objs", chunks, info)
    index, sizes, base = lay.index("store-under-test", max_bytes)
    plain = data.BatchGQABoxFeaturesCollator(str(tmp_path), "objs", chunks, info, ontology, 1, **kw)
    backed = data.BatchGQABoxFeaturesCollator(str(tmp_path), "objs", chunks, info, ontology, 1, device_store=index, **kw)
    return plain, backed, index, lay


def reachable(obj, seen=None):
    """Every object reachable from `obj` through attributes, slots and containers."""
    seen = {} if seen is None else seen
    if id(obj) in seen:
        return seen
    seen[id(obj)] = obj
    if isinstance(obj, dict):
        children = list(obj.keys()) + list(obj.values())
    elif isinstance(obj, (list, tuple, set, frozenset)):
        children = list(obj)
    else:
        children = list(getattr(obj, "__dict__", {}).values()) + [getattr(obj, s) for s in getattr(type(obj), "__slots__", ()) if hasattr(obj, s)]
    for c in children:
        reachable(c, seen)
    return seen


def test_index_pickles_and_holds_no_tensor(tmp_path, ontology):
    _, _, index, lay = collators(tmp_path, ontology)
    assert lay.shapes == [(PER_CHUNK, MAX_OBJ, F)] * 2 and lay.chunk_bytes == [PER_CHUNK * 4 * (MAX_OBJ * F + MAX_OBJ * 4 + 2)] * 2
    assert isinstance(index, FeatureStoreIndex) and (index.F, index.max_obj, index.store_id) == (F, MAX_OBJ, "store-under-test")
    assert [index.get("img%03d" % k) for k in range(6)] == [(k, COUNTS[k]) for k in range(6)]          # slot = rows of earlier chunks + idx
    assert "img004" in index and "img999" not in index and index.get("img999") == (-1, 0)
    assert not any(isinstance(o, torch.Tensor) for o in reachable(index).values())
    blob = pickle.dumps(index)
    assert b"torch" not in blob
    back = pickle.loads(blob)
    assert (back.store_id, back.F, back.max_obj) == (index.store_id, F, MAX_OBJ) and back._table == index._table
    ref = back.ref(["img005", "img000"])
    ref2 = pickle.loads(pickle.dumps(ref))
    assert ref2.store_id == "store-under-test" and ref2.slots.tolist() == [5, 0] and ref2.counts.tolist() == [3, 1]
    assert ref2.slots.dtype == ref2.counts.dtype == np.int32
    assert ref2.index_array().tolist() == [5, 0, 0, 3, 4]


def test_the_collator_takes_an_index_not_a_store(tmp_path, ontology):
    chunks, info = write_chunks(tmp_path)
    with pytest.raises(TypeError):
        data.BatchGQABoxFeaturesCollator(str(tmp_path), "objs", chunks, info, ontology, 1, device_store=object())
    with pytest.raises(TypeError):                       # keyword-only
        data.BatchGQABoxFeaturesCollator(str(tmp_path), "objs", chunks, info, ontology, 1, True, False, None)
    other = FeatureStoreIndex("x", F + 1, MAX_OBJ, {})
    with pytest.raises(ValueError):
        data.BatchGQABoxFeaturesCollator(str(tmp_path), "objs", chunks, info, ontology, 1, device_store=other)


@pytest.mark.parametrize("share_scenes", [False, True])
def test_resident_batch_returns_a_ref(tmp_path, ontology, share_scenes):
    plain, backed, index, _ = collators(tmp_path, ontology, share_scenes=share_scenes)
    images = ["img004", "img000", "img005", "img004", "img001", "img000"]          # descending slots, repeats
    items = items_of(ontology, images)
    host = plain.collate(copy.deepcopy(items))[0]
    pb = backed.collate(copy.deepcopy(items))[0]
    ref = pb._object_features
    assert isinstance(ref, ObjectFeatureRef) and ref.store_id == index.store_id
    distinct = ["img004", "img000", "img005", "img001"] if share_scenes else images          # (one representative question per image)
    assert ref.slots.tolist() == [int(im[3:]) for im in distinct]
    assert ref.counts.tolist() == [COUNTS[int(im[3:])] for im in distinct]
    assert pb._object_batch_index.dtype == host._object_batch_index.dtype == torch.int64
    assert torch.equal(pb._object_batch_index, host._object_batch_index)
    assert pb._object_nums == host._object_nums == ref.counts.tolist()
    assert pb._question_image == host._question_image
    assert not hasattr(pb, "_feature_source") and not hasattr(host, "_feature_source")
    assert host._object_features.shape == (int(ref.counts.sum()), F + 6)
    back = pickle.loads(pickle.dumps(pb))                        # the way a DataLoader worker hands it over
    assert back._object_features.slots.tolist() == ref.slots.tolist() and back._object_features.counts.tolist() == ref.counts.tolist()


def test_partly_resident_batch_takes_the_host_route(tmp_path, ontology):
    lay_bytes = PER_CHUNK * 4 * (MAX_OBJ * F + MAX_OBJ * 4 + 2)
    plain, backed, index, _ = collators(tmp_path, ontology, max_bytes=lay_bytes + lay_bytes // 2)       # room for one of the two chunks
    assert [index.get("img%03d" % k)[0] for k in range(6)] == [0, 1, 2, -1, -1, -1]
    assert [index.get("img%03d" % k)[1] for k in range(6)] == COUNTS
    items = items_of(ontology, ["img002", "img004", "img000"])            # img004 lives in the chunk that did not fit
    host = plain.collate(copy.deepcopy(items))[0]
    pb = backed.collate(copy.deepcopy(items))[0]
    assert isinstance(pb._object_features, torch.Tensor) and pb._feature_source == "host"
    assert pb._object_features.dtype == torch.float32
    assert np.array_equal(pb._object_features.numpy().view(np.uint32), host._object_features.numpy().view(np.uint32))
    assert torch.equal(pb._object_batch_index, host._object_batch_index)
    resident = backed.collate(copy.deepcopy(items_of(ontology, ["img002", "img000"])))[0]
    assert isinstance(resident._object_features, ObjectFeatureRef) and not hasattr(resident, "_feature_source")
    none_fit, _, _ = StoreLayout(str(tmp_path), "objs", 2, os.path.join(str(tmp_path), "info.json")).index("s", max_bytes=lay_bytes - 1)
    assert all(none_fit.get("img%03d" % k) == (-1, COUNTS[k]) for k in range(6))


def test_store_backed_collate_opens_no_chunk_file(tmp_path, ontology, monkeypatch):
    _, backed, index, _ = collators(tmp_path, ontology)

    def refuse(i):
        raise AssertionError("chunk file %d opened" % i)
    monkeypatch.setattr(backed, "_chunk", refuse)
    feats, bi = backed.collate_object_features([{"image_id": im} for im in ("img003", "img001", "img003")])
    assert isinstance(feats, ObjectFeatureRef) and feats.slots.tolist() == [3, 1, 3]
    assert bi.tolist() == [0] * COUNTS[3] + [1] * COUNTS[1] + [2] * COUNTS[3]
    assert backed._file_handles is None
    pb = backed.collate(items_of(ontology, ["img005", "img002"]))[0]
    assert isinstance(pb._object_features, ObjectFeatureRef) and backed._file_handles is None
    with pytest.raises(AssertionError):                  # (the guard is live: an unknown image goes to the files)
        backed.collate_object_features([{"image_id": "img001"}, {"image_id": "img999"}])


def test_g16_h5_chunks_through_the_index(ontology, golden_dir):
    """The same on the reference-written .h5 feature chunks (golden g16): shapes come from the datasets, no array is read."""
    from test_data_path import _h5_or_skip
    _h5_or_skip()
    h5 = os.path.join(golden_dir, "h5")
    info_path = os.path.join(h5, "gqa_objects_info.json")
    lay = StoreLayout(h5, "gqa_objects", 2, info_path)
    index, sizes, base = lay.index("g16")
    with open(info_path) as f:
        info = json.load(f)
    assert base.tolist() == [0, lay.shapes[0][0], lay.shapes[0][0] + lay.shapes[1][0]] and sizes.shape == (base[-1], 2)
    for im, inf in info.items():
        slot, n = index.get(im)
        assert (slot, n) == (int(base[inf["file"]]) + inf["idx"], inf["objectsNum"])
        assert sizes[slot].tolist() == [inf["width"], inf["height"]]
    plain = data.BatchGQABoxFeaturesCollator(h5, "gqa_objects", 2, info_path, ontology, 1)
    backed = data.BatchGQABoxFeaturesCollator(h5, "gqa_objects", 2, info_path, ontology, 1, device_store=index)
    order = [{"image_id": im} for im in sorted(info, reverse=True)]
    ref, bi = backed.collate_object_features(order)
    assert torch.equal(bi, plain.collate_object_features(order)[1]) and ref.counts.tolist() == [info[q["image_id"]]["objectsNum"] for q in order]


def test_entry_point_validates_its_sizes_without_a_device():
    import __graft_entry__ as g
    g.build()
    from dfol_vqa_amd import _lib
    h = _lib.load()
    assert h.dfol_gather_object_rows_f32(None, None, None, None, None, 0, 4, 8, None, 14, None) == 0       # I == 0: nothing to do, no launch
    for I, max_obj, feature_dim, ld in ((1, 4, 0, 14), (1, 0, 8, 14), (1, 4, 8, 13), (0, 4, 8, 13)):
        assert h.dfol_gather_object_rows_f32(None, None, None, None, None, I, max_obj, feature_dim, None, ld, None) != 0
        assert b"gather_object_rows" in h.dfol_last_error()


def test_lowered_tokens_pickle_without_their_device_copies(ontology):
    """A collator pickled to a spawned DataLoader worker takes its ontology along, and the ontology caches lowered token lists whose device
    copies a forward in this process has filled in: they stay behind, or the worker would open the GPU to receive them."""
    from dfol_vqa_amd.fol_types import TokenType
    from dfol_vqa_amd.host_util import lower_tokens
    low = lower_tokens(["dog", "not(red)", None], ontology, TokenType.ATTRIBUTE)
    low._dev["cuda:0"] = ("stands for three device tensors",)
    try:
        back = pickle.loads(pickle.dumps(low))
        assert back._dev == {} and low._dev
        assert back.cols.tolist() == low.cols.tolist() and back.neg.tolist() == [0, 1, 0] and back.valid.tolist() == [1, 1, 0]
        assert (back.any_neg, back.any_valid, back.all_valid) == (True, True, False)
        cache = pickle.loads(pickle.dumps(ontology)).__dict__["_lower_cache"]
        assert all(v._dev == {} for v in cache._d.values())
    finally:
        low._dev.clear()
