"""data.prepare_scene_batch without a GPU: the 3-image scene batch of golden g25_scene (hand-written scene questions over the g18 fixture files,
through the dataset's line transform and the collater) prepared on the CPU - the by-object list of the listed pairs, the padding, the capacity
checks, `load`, and the prepared arrays against data.scene_meta_data's."""

import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402

TARGETS = ("attribute_answer", "attribute_weight", "relation_answer", "relation_weight")


@pytest.fixture(scope="module")
def g25(mini_ontology_paths, golden_dir):
    import __graft_entry__ as g
    g.build()
    import dfol_vqa_amd as D
    from dfol_vqa_amd import data
    p = mini_ontology_paths
    ontology = D.GQAOntology(p["attribute_file"], p["class_file"], p["vocabulary_file"], p["word_embedding_file"], relation_json_path=p["relation_file"])
    a, meta = gu.load("g25_scene")
    h5 = os.path.join(golden_dir, "h5")
    coll = data.BatchGQABoxFeaturesCollator(h5, meta["feature_prefix"], meta["chunk_num"], os.path.join(h5, meta["info"]), ontology, 1)
    ds = object.__new__(data.ProgramDataset)
    ds._ontology, ds._shuffle_options, ds._is_bytecode, ds._keep_original_dict = ontology, False, False, False
    collate = lambda qs: coll.collate([ds._transform_line(copy.deepcopy(q)) for q in qs])[0]
    return ontology, meta, coll, collate


def listed(pb):
    first = np.concatenate([[0], np.cumsum(pb._object_nums)])[:-1]
    pairs = pb._meta_data["object_pairs"]
    s = [int(i) + int(f) for f, ids in zip(first, pairs["subject_id"]) for i in ids]
    o = [int(i) + int(f) for f, ids in zip(first, pairs["object_id"]) for i in ids]
    return s, o


def check_csr(seg_off, slot, pair_s, pair_o, objects):
    """Every (pair, half) once; the entries of an object are its own, by pair number, the subject half before the object half."""
    P = len(pair_s)
    assert seg_off.shape == (objects + 1,) and slot.shape == (2 * P,) and seg_off.dtype == slot.dtype == np.int32
    assert sorted(slot.tolist()) == list(range(2 * P))
    assert seg_off[0] == 0 and seg_off[-1] == 2 * P and (np.diff(seg_off) >= 0).all()
    for t in range(objects):
        mine = slot[seg_off[t]:seg_off[t + 1]].tolist()
        assert mine == sorted(mine)                                  # 2 pair + half ascending: by pair number, subject (0) before object (1)
        assert all((pair_s if e % 2 == 0 else pair_o)[e // 2] == t for e in mine)


def test_unpadded_arrays_are_the_collaters(g25):
    from dfol_vqa_amd import data
    ontology, meta, coll, collate = g25
    pb = collate(meta["questions"])
    assert pb.batch_size() == 3
    prep = data.prepare_scene_batch(pb, "cpu")
    ps = prep._scene_prepared
    s, o = listed(pb)
    assert len(s) >= 3 and (ps.O, ps.P, ps.objects, ps.pairs, ps.images) == (sum(pb._object_nums), len(s), sum(pb._object_nums), len(s), 3)
    assert ps.pair_s.tolist() == s and ps.pair_o.tolist() == o and ps.pair_s.dtype == torch.int32
    md = data.scene_meta_data([ds for ds in map(copy.deepcopy, meta["questions"])], pb._object_nums, ontology)
    for key in TARGETS:
        assert np.array_equal(getattr(ps, key).numpy(), md[key]) and np.array_equal(md[key], pb._meta_data[key]), key
    assert torch.equal(ps.features, pb._object_features) and prep._object_features is ps.features
    assert prep is not pb and getattr(pb, "_scene_prepared", None) is None       # the batch handed in stays an unprepared one
    check_csr(ps.seg_off.numpy(), ps.slot.numpy(), s, o, ps.O)
    counts = np.bincount(np.asarray(s + o), minlength=ps.O)
    assert np.array_equal(np.diff(ps.seg_off.numpy()), counts) and (counts == 0).any()       # an object no pair names: an empty segment


def test_padding_rows_carry_zero_weights_and_index_zero(g25):
    from dfol_vqa_amd import data
    ontology, meta, coll, collate = g25
    pb = collate(meta["questions"])
    O, (s, o) = sum(pb._object_nums), listed(pb)
    P = len(s)
    ps = data.prepare_scene_batch(pb, "cpu", objects=O + 37, pairs=P + 19)._scene_prepared
    assert (ps.objects, ps.pairs, ps.O, ps.P) == (O + 37, P + 19, O, P)
    assert tuple(ps.features.shape) == (O + 37, pb._object_features.shape[1]) and not ps.features[O:].any()
    assert torch.equal(ps.features[:O], pb._object_features)
    assert ps.pair_s[:P].tolist() == s and ps.pair_o[:P].tolist() == o
    assert not ps.pair_s[P:].any() and not ps.pair_o[P:].any()                     # a padded pair names row 0 twice
    for key, real in zip(TARGETS, (O, O, P, P)):
        a = getattr(ps, key).numpy()
        assert np.array_equal(a[:real], pb._meta_data[key]) and not a[real:].any(), key
    assert pb._meta_data["relation_weight"].min() > 0                              # (the collater's relation weights start at 1: the padding's do not)
    check_csr(ps.seg_off.numpy(), ps.slot.numpy(), ps.pair_s.tolist(), ps.pair_o.tolist(), O + 37)
    # the real entries of object 0 keep their places in front: the padded pairs' entries follow them
    seg0 = ps.slot[:int(ps.seg_off[1])].tolist()
    real0 = [e for e in seg0 if e < 2 * P]
    assert seg0 == real0 + list(range(2 * P, 2 * (P + 19))) and not np.diff(ps.seg_off.numpy())[O:].any()


def test_capacities_below_the_batch_raise(g25):
    from dfol_vqa_amd import _lib, data
    ontology, meta, coll, collate = g25
    pb = collate(meta["questions"])
    O, P = sum(pb._object_nums), len(listed(pb)[0])
    with pytest.raises(_lib.DfolError, match="O = %d objects" % O):
        data.prepare_scene_batch(pb, "cpu", objects=O - 1)
    with pytest.raises(_lib.DfolError, match="P = %d pairs" % P):
        data.prepare_scene_batch(pb, "cpu", pairs=P - 1)
    bad = copy.copy(pb)
    pairs = copy.deepcopy(pb._meta_data["object_pairs"])
    pairs["subject_id"][0][0] = O                                              # (image 0's offset is 0: row O does not exist)
    bad._meta_data = dict(pb._meta_data, object_pairs=pairs)
    with pytest.raises(_lib.DfolError, match="name an object the batch does not have"):
        data.prepare_scene_batch(bad, "cpu")


def test_load_rewrites_the_arrays_and_the_padding(g25):
    from dfol_vqa_amd import _lib, data
    ontology, meta, coll, collate = g25
    qs = meta["questions"]
    pb = collate(qs)
    O, P = sum(pb._object_nums), len(listed(pb)[0])
    prep = data.prepare_scene_batch(pb, "cpu", objects=O + 5, pairs=P + 4)
    ps = prep._scene_prepared
    kept = {k: t.data_ptr() for k, t in ps.tensors().items()}
    other = collate([qs[2], qs[0], qs[1]])                                       # the same images in another order: other offsets
    data.load_scene_batch(prep, other)
    assert {k: t.data_ptr() for k, t in ps.tensors().items()} == kept              # the same tensors, other contents
    fresh = data.prepare_scene_batch(other, "cpu", objects=O + 5, pairs=P + 4)._scene_prepared
    for k, t in ps.tensors().items():
        assert torch.equal(t, getattr(fresh, k)), k
    assert prep._object_nums == other._object_nums and prep._meta_data is other._meta_data
    with pytest.raises(_lib.DfolError, match="2 images"):
        data.load_scene_batch(prep, collate(qs[:2]))
    small = data.prepare_scene_batch(collate([qs[1], qs[1], qs[1]]), "cpu", pairs=P)      # three times the image of 4 objects and no pair
    assert sum(small._object_nums) == 12 < O
    with pytest.raises(_lib.DfolError, match="above the capacity of 12 object rows"):
        data.load_scene_batch(small, pb)
    few = data.prepare_scene_batch(collate([qs[1], qs[1], qs[1]]), "cpu", objects=O)
    with pytest.raises(_lib.DfolError, match="above the capacity of 0 pair rows"):
        data.load_scene_batch(few, pb)
