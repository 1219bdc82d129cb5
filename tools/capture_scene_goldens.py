#!/usr/bin/env python3
"""Capture golden family g25 - scene-graph supervision - from the imported reference (runs only in the build container, like
tools/capture_goldens.py; the reference is imported at run time through tools/ref_harness.py, none of its text is copied).

    python tools/capture_scene_goldens.py          # rewrites tests/golden/g25_scene.npz|json

Hand-written questions with `attribute_dict`, `relation_list` and `object_pairs` over the g18 fixture files (tests/golden/h5/g18_objects_*)
go through the reference's own BatchGQABoxFeaturesCollator (batch_gqa_boxfeatures_pipeline.py:37-155) and its featurizer's listed-pairs
branch (:225-279).  With the reference's model at g18's reduced dims and seeded weights the tool records
  * the collater's object_pairs, attribute_answer / attribute_weight, relation_answer / relation_weight;
  * the hidden rows entering the embedding layer (attribute network over the objects, relation network over the listed pairs) and
    ClassifierOracle(cached=False).compute_all_log_likelihood (classifier_oracle.py:139-143), at fp32 and fp64;
  * VQATrainer._compute_loss and _compute_evaluation_metrics (trainer.py:235-256, :265-275) for the SCENE_GRAPH prediction GQASceneOpBatch
    forms from those tables (batch_gqa_ops.py:883-902), at fp32 and fp64.
The trainer cannot be constructed without its whole experiment, so its two methods are called UNBOUND on a stub that carries `_device`
and `_config` (the way tools/capture_goldens.py calls _compute_loss).  _compute_loss builds fp32 targets; for the fp64 run - and only
for it - binary_cross_entropy is wrapped so that target and weight are cast to the input's dtype before the reference's own call goes on."""

import copy
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ref_harness  # noqa: E402
from dfol_vqa_amd import h5lite  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402

import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
H5 = os.path.join(OUT, "h5")


def scene_questions():
    """Three images of the g18 fixture (5, 4 and 8 objects).  Attribute lists name adjectives, nouns (their class family and every noun column
    get weight 1), a relation name and a word outside the vocabulary (both skipped); relation lists name a relation outside the vocabulary
    ('riding') and an attribute (skipped, their rows keep weight 1 everywhere); one image lists no pairs."""
    Q = lambda i, im, pairs, attrs, rels: {
        "image_id": im, "imageId": im, "answer": "", "question": "scene %d" % i, "question_id": str(900 + i), "tokens": [],
        "program": {"branches": [], "last_op": syn.op("scene")}, "object_pairs": pairs, "attribute_dict": attrs, "relation_list": rels}
    return [
        Q(0, "img012", {"subject_id": [0, 3, 4], "object_id": [1, 0, 2]},
          {"0": [["red", 1.0], ["dog", 0.5]], "2": [["wood", 2.0], ["on", 1.0]], "4": [["zebra", 1.0], ["chair", 1.5], ["large", 0.25]]},
          [["on", 1.0], ["riding", 2.0], ["to the left of", 0.5]]),
        Q(1, "img013", {"subject_id": [], "object_id": []}, {"1": [["cup", 1.0]], "3": []}, []),
        Q(2, "img014", {"subject_id": [7, 7, 1, 2, 5, 0, 6], "object_id": [0, 3, 2, 1, 6, 7, 5]},
          {str(j): [[a, w]] for j, (a, w) in enumerate([("blue", 1.0), ("man", 0.75), ("glass", 1.25), ("sitting", 1.0), ("bus", 2.0),
                                                        ("small", 0.5), ("tree", 1.0), ("black", 1.5)])},
          [["near", 1.0], ["holding", 0.5], ["red", 1.0], ["behind", 2.0], ["under", 1.0], ["on", 0.25], ["to the right of", 1.0]]),
    ]


def main():
    ref = ref_harness.import_reference()
    saved = sys.modules.get("h5py")
    sys.modules["h5py"] = h5lite
    for name in ("pattern", "pattern.text", "pattern.text.en"):
        m = types.ModuleType(name)
        m.__path__ = []
        m.singularize = lambda w: w
        sys.modules.setdefault(name, m)
    from nsvqa.data import batch_gqa_boxfeatures_pipeline as bfp
    from nsvqa.train.trainer import VQATrainer
    bfp.h5py = h5lite
    import gqa_interpreter_experiments as gie
    d = os.path.join(OUT, "mini_ontology")
    paths = {"attribute_file": os.path.join(d, "attribute.json"), "class_file": os.path.join(d, "class.json"),
             "relation_file": os.path.join(d, "relation.json"), "vocabulary_file": os.path.join(d, "vocab.json"),
             "word_embedding_file": os.path.join(d, "glove.txt")}
    ontology = ref_harness.build_ontology(ref, paths)
    g18 = json.load(open(os.path.join(OUT, "g18_h5_end_to_end.json")))
    cfg = dict(g18["config"], model_name="g25")
    exp = gie.GQAObjectBoxExperiment()
    exp._local_rank = 0
    torch.manual_seed(25)
    model = exp.build_model(cfg, ontology, None)
    with torch.no_grad():                                     # informative likelihoods: a fresh embedding layer saturates every concept
        lin = model._oracle._embedding_network._network[1]
        lin.weight.normal_(0.0, 0.6)
        lin.bias.fill_(-1.0)
    model.eval()
    questions = scene_questions()
    coll = bfp.BatchGQABoxFeaturesCollator(H5, g18["feature_prefix"], g18["chunk_num"], os.path.join(H5, g18["info"]), ontology, 1)
    md = coll.collate_meta_data(copy.deepcopy(questions))
    feats, batch_index = coll.collate_object_features(copy.deepcopy(questions))
    arrays = {"w:" + k: v.numpy().copy() for k, v in model.state_dict().items() if k.startswith("_featurizer.") or k.startswith("_oracle.")}
    for key in ("attribute_answer", "attribute_weight", "relation_answer", "relation_weight"):
        arrays[key] = np.asarray(md[key])
    arrays["object_features"] = feats.numpy()
    meta = {"source": "batch_gqa_boxfeatures_pipeline.py:37-155,225-279; classifier_oracle.py:139-143; batch_gqa_ops.py:883-902; "
                      "trainer.py:235-256,265-275", "config": cfg, "h5_dir": "tests/golden/h5", "feature_prefix": g18["feature_prefix"],
            "chunk_num": g18["chunk_num"], "info": g18["info"], "questions": questions, "object_pairs": md["object_pairs"],
            "objects": [int(x) for x in torch.bincount(batch_index).tolist()], "torch": torch.__version__}
    fake = types.SimpleNamespace(_device=torch.device("cpu"), _config={})
    pbs = [types.SimpleNamespace(_meta_data=md)]
    QT = ref.base_types.QuestionType
    bce = torch.nn.functional.binary_cross_entropy
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        net = model if dt == torch.float32 else copy.deepcopy(model).double()
        oracle = ref.ClassifierOracle(ontology, net._oracle._attribute_network, net._oracle._relation_network, net._oracle._embedding_network,
                                      cached=False)
        with torch.no_grad():
            scene = net._featurizer.featurize_scene(torch.device("cpu"), feats.to(dt), batch_index, dict(md))
            obj, pair = scene["attribute_features"], scene["relation_features"]
            arrays["h_attr_" + tag] = net._oracle._attribute_network(obj).numpy()
            arrays["h_rel_" + tag] = net._oracle._relation_network(pair["features"]).numpy()
            attr, rel = oracle.compute_all_log_likelihood(obj, pair)
            arrays["attr_table_" + tag], arrays["rel_table_" + tag] = attr.numpy(), rel.numpy()
            res = {"type": QT.SCENE_GRAPH, "log_probability": [attr, rel],
                   "answer": [(attr > 0.5).float().cpu().numpy(), (rel > 0.5).float().cpu().numpy()]}        # batch_gqa_ops.py:883-902
            if dt == torch.float64:
                torch.nn.functional.binary_cross_entropy = lambda x, t, weight=None, **kw: bce(x, t.to(x.dtype), weight=weight.to(x.dtype), **kw)
            try:
                arrays["loss_" + tag] = VQATrainer._compute_loss(fake, pbs, res).numpy()
            finally:
                torch.nn.functional.binary_cross_entropy = bce
            with np.errstate(divide="ignore", invalid="ignore"):
                arrays["metric_" + tag] = np.asarray(VQATrainer._compute_evaluation_metrics(fake, pbs, res))
        print(tag, "loss", arrays["loss_" + tag], "metric", arrays["metric_" + tag], "tables", attr.shape, rel.shape)
    np.savez_compressed(os.path.join(OUT, "g25_scene.npz"), **arrays)
    with open(os.path.join(OUT, "g25_scene.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("wrote g25_scene, bytes:", os.path.getsize(os.path.join(OUT, "g25_scene.npz")))
    if saved is not None:
        sys.modules["h5py"] = saved


if __name__ == "__main__":
    main()
