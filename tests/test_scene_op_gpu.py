"""Operator `scene` end to end on the GPU: a scene-only batch of 3 images (1, 5 and 12 objects; 0, 3 and 7 listed pairs) through the collater's
dense targets, interpreter.build_scene_graph, GQASceneOpBatch, gather_results, training.compute_loss / compute_evaluation_metrics and
training.train_batch, against a float64 restatement of featurizer -> networks -> compute_all_log_likelihood (classifier_oracle.py:139-143) ->
the loss of trainer.py:235-256 (rule: DESIGN.md 5, golden_util.check_gradient; the same restatement in float32 is the yardstick).  The model
is the narrow synthetic-ontology model of tests/test_train_dropout_gpu.py; with `dropout: 0.2` the restatement runs with the masks the kernel
drew (that file's method)."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
import scene_util as su  # noqa: E402
from dfol_vqa_amd import _lib, data, parallel, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from dfol_vqa_amd.fol_types import QuestionType  # noqa: E402
from test_interpreter_gpu import DEV, TableCollater  # noqa: E402
from test_train_dropout_gpu import _elu, build, world  # noqa: E402,F401

pytestmark = pytest.mark.gpu
P = 0.2
N_OBJECTS, N_PAIRS = (1, 5, 12), (0, 3, 7)


class SceneCollater(TableCollater):
    def collate_meta_data(self, questions):
        md = super(SceneCollater, self).collate_meta_data(questions)
        md.update(data.scene_meta_data(questions, [q["scene"]["n"] for q in questions], self._ontology))
        return md


def questions(world, pairs=N_PAIRS, first=9100):
    paths, names, ont = world
    rng = np.random.RandomState(4)
    attrs, rels = names["attributes"][:6] + names["nouns"][:6], names["relations"][:5]
    qs = []
    for i, (n, k) in enumerate(zip(N_OBJECTS, pairs)):
        q = syn.question(first + i, [], syn.op("scene"), "", syn.feature_scene(first + i, n, 32))
        s = [int(x) for x in rng.randint(0, n, size=k)]
        o = [int((a + 1 + rng.randint(0, n - 1)) % n) for a in s] if n > 1 else []
        q["object_pairs"] = {"subject_id": s, "object_id": o}
        q["attribute_dict"] = {str(j): [(attrs[rng.randint(len(attrs))], float(rng.randint(1, 9)) / 4.0) for _ in range(1 + j % 2)]
                               for j in range(0, n, 2)}
        q["relation_list"] = [(rels[rng.randint(len(rels))], float(rng.randint(1, 9)) / 4.0) for _ in range(k)]
        qs.append(q)
    return qs


def batches(world, qs, split=1):
    pbs = SceneCollater(split, world[2], "X").collate([dict(q) for q in qs])
    return [pb.to_cuda(DEV) for pb in pbs]


def restated(weights, raw, pbs, ont, dtype, masks=None, scale=1.0):
    """featurizer, the two networks over the objects and the LISTED pairs (batch_gqa_boxfeatures_pipeline.py:225-279), the two tables
    (classifier_oracle.py:139-143) and the loss of trainer.py:235-256, in `dtype` on the CPU; masks: the 7 keep masks in site order."""
    w = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in weights.items()}
    m = [1.0] * 7 if masks is None else [mk.to(dtype) * scale for mk in masks]
    lin = lambda name, x: x @ w[name + ".weight"].t() + w[name + ".bias"]
    raw = raw.detach().cpu().to(dtype)
    F = raw.shape[1] - 6
    f = torch.sigmoid(lin("_featurizer._featurizer_network._network.1", raw[:, :F] * m[0]))
    tail = raw[:, F:]
    pos = tail[:, 2:6] / torch.clamp(torch.stack([tail[:, 0], tail[:, 1], tail[:, 0], tail[:, 1]], 1), min=1.0)
    obj = torch.cat([f, pos], 1)
    h = _elu(lin("_oracle._attribute_network._network.1", obj * m[1]))
    h = torch.sigmoid(lin("_oracle._attribute_network._network.4", h * m[2]))
    ai, ri = torch.as_tensor(np.asarray(ont._attribute_index, np.int64)), torch.as_tensor(np.asarray(ont._relation_index, np.int64))
    attr = torch.nn.functional.logsigmoid(lin("_oracle._embedding_network._network.1", h * m[3]))[:, ai]
    s_all, o_all, first = [], [], 0
    for pb in pbs:
        for n, s, o in zip(pb._object_nums, pb._meta_data["object_pairs"]["subject_id"], pb._meta_data["object_pairs"]["object_id"]):
            s_all += [first + i for i in s]
            o_all += [first + i for i in o]
            first += n
    s, o = torch.as_tensor(s_all, dtype=torch.int64), torch.as_tensor(o_all, dtype=torch.int64)
    ps, po = pos[s], pos[o]
    dx = ps[:, 0] + ps[:, 2] / 2 - po[:, 0] - po[:, 2] / 2
    dy = ps[:, 1] + ps[:, 3] / 2 - po[:, 1] - po[:, 3] / 2
    dist = torch.sqrt(dx * dx + dy * dy)
    geo = torch.stack([dist, torch.asin(dy / torch.clamp(dist, min=1e-10)), torch.sign(po[:, 0] - ps[:, 0]), torch.sign(po[:, 1] - ps[:, 1])], 1)
    pair = torch.cat([obj[s], obj[o], geo], 1)
    h = _elu(lin("_oracle._relation_network._network.1", pair * m[4]))
    h = torch.sigmoid(lin("_oracle._relation_network._network.4", h * m[5]))
    rel = torch.nn.functional.logsigmoid(lin("_oracle._embedding_network._network.1", h * m[6]))[:, ri]
    cat = lambda key: torch.as_tensor(np.concatenate([pb._meta_data[key] for pb in pbs], 0)).to(dtype)
    bce = torch.nn.functional.binary_cross_entropy
    terms = [bce(attr.exp(), cat("attribute_answer"), weight=cat("attribute_weight"), reduction="none"),
             bce(rel.exp(), cat("relation_answer"), weight=cat("relation_weight"), reduction="none")]
    loss = terms[0].sum() + terms[1].sum()
    B = sum(pb.batch_size() for pb in pbs)
    (loss / B).backward()
    return {"loss": loss.item(), "abs_terms": float((terms[0].abs().sum() + terms[1].abs().sum()).detach()), "attr": attr.detach().double().numpy(),
            "rel": rel.detach().double().numpy(), "grads": {k: v.grad.double().numpy() for k, v in w.items() if v.grad is not None}}


def train_once(model, pbs, clip=1e9):
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.0)       # gradients stay in .grad, unscaled; weights stay
    loss, result = training.train_batch(model, opt, pbs, clip_norm=clip)
    return loss, result, {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}


def check_step(model, pbs, ont, loss, grads, what, masks=None, scale=1.0):
    weights = dict(model.named_parameters())
    raw = torch.cat([pb._object_features for pb in pbs], 0)
    r64, r32 = (restated(weights, raw, pbs, ont, dt, masks, scale) for dt in (torch.float64, torch.float32))
    B = sum(pb.batch_size() for pb in pbs)
    su.check_loss(loss, r32, r64, what)                           # (train_batch returns the summed loss)
    assert sorted(grads) == sorted(r64["grads"]) and len(grads) == 12, sorted(grads)
    for k in sorted(grads):
        gu.check_gradient(grads[k], r32["grads"][k], r64["grads"][k], what + " d " + k)
    return r64, r32


def test_train_batch_against_the_restatement(world):
    model, _ = build(world, "narrow", 0.0)
    model.train()
    pbs = batches(world, questions(world))
    assert [pb._meta_data["attribute_answer"].shape for pb in pbs] == [(18, len(world[2]._attribute_index))]
    assert [pb._meta_data["relation_answer"].shape for pb in pbs] == [(10, len(world[2]._relation_index))]
    _lib.PATH_COUNTS.clear()
    loss, result, grads = train_once(model, pbs)
    routes = dict(_lib.PATH_COUNTS)
    assert routes.get("scene_python") == 1 and routes.get("scene_bce_hip") == 2, routes
    assert not [r for r in routes if r in ("python_program", "native_program", "pair_trunk", "fused_hidden1", "attr_head") or r.startswith("fallback:")], routes
    assert result["type"] == QuestionType.SCENE_GRAPH and result["answer"] == []
    check_step(model, pbs, world[2], loss, grads, "scene step")
    metric = training.compute_evaluation_metrics(pbs, result)
    assert metric == 1.0                                          # every answer is 0 at the 0.5 threshold: each counted cell is a set target


def test_train_batch_with_dropout_and_the_kernels_masks(world):
    model, _ = build(world, "narrow", P)
    model.train()
    pbs = batches(world, questions(world))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(P)))
    drawn = []
    try:
        _lib.seed_dropout(13)
        for step in range(2):
            trace = _lib.DROPOUT_TRACE = []
            loss, _, grads = train_once(model, pbs)
            _lib.DROPOUT_TRACE = None
            fwd = trace[:7]
            assert [(s, p) for s, _, p in fwd] == [(i, P) for i in range(7)], trace
            assert [sh[0] for _, sh, _ in fwd] == [18, 18, 18, 18, 10, 10, 10], trace
            masks = [_lib.dropout_mask(shape, p, site, DEV).cpu() for site, shape, p in fwd]
            drawn.append(masks)
            check_step(model, pbs, world[2], loss, grads, "dropout step %d" % step, masks, scale)
    finally:
        _lib.DROPOUT_TRACE = None
        _lib.seed_dropout(torch.initial_seed())
    assert all(not torch.equal(a, b) for a, b in zip(*drawn))      # two steps, other masks


def test_fused_clip_adam_and_no_listed_pairs(world):
    """train_batch with the flat bucket and FusedClipAdam, on a batch with P = 0 listed pairs: finite loss, the weights of the object side move."""
    model, _ = build(world, "narrow", 0.0)
    model.train()
    pbs = batches(world, questions(world, pairs=(0, 0, 0)))
    assert pbs[0]._meta_data["relation_answer"].shape[0] == 0
    params = [p for p in model.parameters() if p.requires_grad]
    opt, bucket = torch.optim.Adam(params, lr=1e-2), parallel.GradBucket(params)
    assert training.FusedClipAdam.make(opt, bucket) is not None
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    losses = [training.train_batch(model, opt, pbs, 0.65, bucket=bucket)[0] for _ in range(2)]
    assert all(np.isfinite(l) for l in losses)
    moved = [k for k, v in model.named_parameters() if not torch.equal(v, before[k])]
    assert any("_attribute_network" in k for k in moved) and any("_embedding_network" in k for k in moved), moved
    assert not [k for k in moved if "_relation_network" in k], moved


def test_tables_answers_and_gather(world):
    model, _ = build(world, "narrow", 0.0)
    model.eval()
    qs = questions(world)
    ont = world[2]
    (pb,) = batches(world, qs)
    with torch.no_grad():
        scene = model.build_scene_graph(DEV, pb)
        like = scene._scene_likelihood
        tables = like.tables()
        again = model._oracle.compute_all_log_likelihood(scene._attribute_features, scene._relation_features)
    assert all(torch.equal(a, b) for a, b in zip(tables, again))
    raw = pb._object_features
    r64, r32 = (restated(dict(model.named_parameters()), raw, [pb], ont, dt) for dt in (torch.float64, torch.float32))
    for got, key in zip(tables, ("attr", "rel")):
        got = got.cpu().double().numpy()
        assert got.shape == r64[key].shape
        scale = np.abs(r64[key]).max()
        own = max(2.0 ** -20 * scale, np.abs(r32[key] - r64[key]).max())
        assert np.abs(got - r64[key]).max() <= 8 * own, (key, np.abs(got - r64[key]).max(), own)
    # two batches through the interpreter: answers and likelihood rows concatenate in batch order (data_parallel.py:16-30)
    two = batches(world, qs, split=2)
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        res = model(two, False)
    assert _lib.PATH_COUNTS["scene_python"] == 2
    assert res["type"] == QuestionType.SCENE_GRAPH and len(res["answer"]) == 2
    assert res["answer"][0].shape == (18, len(ont._attribute_index)) and res["answer"][1].shape == (10, len(ont._relation_index))
    assert not res["answer"][0].any() and not res["answer"][1].any()              # (table > 0.5) on a log-likelihood: the reproduced quirk
    both = res["log_probability"].tables()
    assert torch.equal(both[0], tables[0]) and torch.equal(both[1], tables[1])
    assert training.compute_evaluation_metrics(two, res) == 1.0


def test_object_attr_and_object_rel_are_not_registered(world):
    model, _ = build(world, "narrow", 0.0)
    assert "scene" in model._ops and "object_attr" not in model._ops and "object_rel" not in model._ops
    with pytest.raises(NotImplementedError):
        training.compute_loss([], {"type": QuestionType.OBJECT_STATEMENT, "log_probability": torch.zeros(1)})


def test_reference_golden_tables_loss_and_metric(mini_ontology_paths, golden_dir):
    """Golden g25_scene end to end on the GPU: the reference's hand-written scene questions over the g18 fixture files through this package's
    dataset transform, collater and interpreter, with the reference's weights; `.tables()`, the loss and the metric against what the
    reference's ClassifierOracle(cached=False).compute_all_log_likelihood, _compute_loss and _compute_evaluation_metrics recorded (fp32 and
    fp64; tools/capture_scene_goldens.py).  Tables: |t - f64| <= 8 max(2^-20 max|f64|, max|f32 - f64|); the loss by the rule of DESIGN.md 5."""
    import copy
    import dfol_vqa_amd as D
    from test_interpreter_gpu import neural_model
    p = mini_ontology_paths
    ontology = D.GQAOntology(p["attribute_file"], p["class_file"], p["vocabulary_file"], p["word_embedding_file"], relation_json_path=p["relation_file"])
    a, meta = gu.load("g25_scene")
    h5 = os.path.join(golden_dir, "h5")
    coll = data.BatchGQABoxFeaturesCollator(h5, meta["feature_prefix"], meta["chunk_num"], os.path.join(h5, meta["info"]), ontology, 1)
    ds = object.__new__(data.ProgramDataset)
    ds._ontology, ds._shuffle_options, ds._is_bytecode, ds._keep_original_dict = ontology, False, False, False
    pbs = [pb.to_cuda(DEV) for pb in coll.collate([ds._transform_line(copy.deepcopy(q)) for q in meta["questions"]])]
    model = neural_model(ontology, meta["config"], {k[2:]: a[k] for k in a.files if k.startswith("w:")})
    model.eval()
    with torch.no_grad():
        res = model(pbs, False)
        tables = res["log_probability"].tables()
    for got, key in zip(tables, ("attr", "rel")):
        r32, r64 = a[key + "_table_f32"], a[key + "_table_f64"]
        got = got.cpu().double().numpy()
        assert got.shape == r64.shape
        own = max(2.0 ** -20 * np.abs(r64).max(), np.abs(r32 - r64).max())
        print(key, "table: max error %.3g, the reference's fp32 %.3g" % (np.abs(got - r64).max(), np.abs(r32 - r64).max()))
        assert np.abs(got - r64).max() <= 8 * own, key
    assert not res["answer"][0].any() and not res["answer"][1].any()
    loss = training.compute_loss(pbs, res).item()
    s = 0.0
    for key, which in (("attr", "attribute"), ("rel", "relation")):
        pr, t, w = np.exp(a[key + "_table_f64"]), a[which + "_answer"], a[which + "_weight"]
        with np.errstate(divide="ignore"):
            s += np.abs(w * (t * np.maximum(np.log(pr), -100) + (1 - t) * np.maximum(np.log1p(-pr), -100))).sum()
    own = max(2.0 ** -20, abs(float(a["loss_f32"]) - float(a["loss_f64"])) / s)
    print("loss %.9g  reference fp32 %.9g fp64 %.9g  own %.3g" % (loss, float(a["loss_f32"]), float(a["loss_f64"]), own))
    assert abs(loss - float(a["loss_f64"])) <= 8 * own * s
    assert training.compute_evaluation_metrics(pbs, res) == float(a["metric_f32"])
