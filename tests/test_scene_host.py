"""Scene-graph supervision without a GPU: the tensor-op route of ops.scene_bce (the one CPU tensors and declined sizes take), SceneLikelihood,
and the SCENE_GRAPH branches of training.compute_loss / compute_evaluation_metrics, against the float64 restatement of the reference's
expressions (tests/scene_util.py; classifier_oracle.py:139-143, trainer.py:235-256, :265-275) by the rule of DESIGN.md 5."""

import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
import scene_util as su  # noqa: E402


@pytest.fixture(scope="module")
def D():
    import __graft_entry__ as g
    g.build()
    import dfol_vqa_amd
    return dfol_vqa_amd


@pytest.mark.parametrize("M,H,C,bias,thr", [(37, 20, 33, True, 0.5), (5, 300, 333, False, -0.7), (130, 20, 1, True, -0.7), (0, 20, 33, True, 0.5),
                                            (37, 324, 33, True, -0.7)])
def test_cpu_route_of_scene_bce(D, M, H, C, bias, thr):
    from dfol_vqa_amd import ops
    case, r64 = su.make_case(M, H, C, bias=bias, thr=thr, seed=M + H + C)
    r32 = su.restate(case["h"], case["emb_w"], case["emb_b"], case["cols"], case["target"], case["weight"], thr, torch.float32)
    t = lambda x: None if x is None else torch.as_tensor(x)
    h, w, b = t(case["h"]).requires_grad_(True), t(case["emb_w"]).requires_grad_(True), t(case["emb_b"])
    if b is not None:
        b.requires_grad_(True)
    before = ops.PATH_COUNTS["scene_bce_torch"]
    loss, num, den = ops.scene_bce(h, w, b, t(case["cols"]), t(case["target"]), t(case["weight"]), thr)
    assert ops.PATH_COUNTS["scene_bce_torch"] == before + 1
    assert not num.requires_grad and not den.requires_grad
    assert num.item() == float(r64["num"]) and den.item() == float(r64["den"])
    su.check_loss(loss.item(), r32, r64, "cpu route")
    if M:
        loss.backward()
        idx = case["cols"].astype(np.int64)
        gu.check_gradient(h.grad.numpy(), r32["dh"], r64["dh"], "cpu dh")
        gu.check_gradient(w.grad.numpy()[idx], r32["dE"], r64["dE"], "cpu dE")
        rest = np.ones(w.shape[0], bool)
        rest[idx] = False
        assert not w.grad.numpy()[rest].any()
        if b is not None:
            gu.check_gradient(b.grad.numpy()[idx], r32["db"], r64["db"], "cpu db")


def _oracle_and_batches(seed=0, O=18, P=9, H=12, C_all=40):
    from dfol_vqa_amd.visual_oracle import ClassifierOracle, EmbeddingLayer, SceneLikelihood
    rng = np.random.RandomState(seed)
    perm = rng.permutation(C_all)
    ontology = types.SimpleNamespace(_attribute_index=[int(i) for i in perm[:23]], _relation_index=[int(i) for i in perm[25:36]])
    torch.manual_seed(seed)
    oracle = ClassifierOracle(ontology, None, None, EmbeddingLayer(H, C_all, 0.0))
    h_attr = torch.rand(O, H).requires_grad_(True)
    h_rel = torch.rand(P, H).requires_grad_(True)
    like = SceneLikelihood(h_attr, h_rel, oracle)
    dy = lambda *s: (rng.randint(0, 17, size=s) / 8.0).astype(np.float32)
    bits = lambda *s: (rng.uniform(size=s) < 0.3).astype(np.float32)
    cut_o, cut_p = O // 3, P // 2                                   # two batches: meta data is concatenated along the rows
    meta = [{"attribute_answer": bits(cut_o, 23), "attribute_weight": dy(cut_o, 23), "relation_answer": bits(cut_p, 11), "relation_weight": dy(cut_p, 11)},
            {"attribute_answer": bits(O - cut_o, 23), "attribute_weight": dy(O - cut_o, 23), "relation_answer": bits(P - cut_p, 11),
             "relation_weight": dy(P - cut_p, 11)}]
    return oracle, like, [types.SimpleNamespace(_meta_data=m) for m in meta]


def _restate_sides(oracle, like, batches, thr, dtype):
    lin = oracle._embedding_network.linear
    out = []
    for which, h, index in (("attribute", like.h_attr, oracle._ontology._attribute_index), ("relation", like.h_rel, oracle._ontology._relation_index)):
        cat = lambda key: np.concatenate([pb._meta_data[key] for pb in batches], 0)
        out.append(su.restate(h.detach().numpy(), lin.weight.detach().numpy(), lin.bias.detach().numpy(), np.asarray(index), cat(which + "_answer"),
                              cat(which + "_weight"), thr, dtype))
    return out


def test_scene_loss_and_metric_on_the_cpu(D):
    from dfol_vqa_amd import training
    from dfol_vqa_amd.fol_types import QuestionType
    from dfol_vqa_amd.visual_oracle import SCENE_THRESHOLD
    assert SCENE_THRESHOLD == 0.5                                   # the reference's (table > 0.5) on a log-likelihood
    oracle, like, batches = _oracle_and_batches()
    prediction = {"type": QuestionType.SCENE_GRAPH, "log_probability": like}
    loss = training.compute_loss(batches, prediction)
    r64, r32 = _restate_sides(oracle, like, batches, 0.5, torch.float64), _restate_sides(oracle, like, batches, 0.5, torch.float32)
    both = lambda rs, k: sum(float(r[k]) for r in rs)
    su.check_loss(loss.item(), {"loss": both(r32, "loss")}, {"loss": both(r64, "loss"), "abs_terms": both(r64, "abs_terms")}, "compute_loss")
    loss.backward()
    gu.check_gradient(like.h_attr.grad.numpy(), r32[0]["dh"], r64[0]["dh"], "h_attr")
    gu.check_gradient(like.h_rel.grad.numpy(), r32[1]["dh"], r64[1]["dh"], "h_rel")
    # the metric: every answer is 0 (no log-likelihood exceeds 0.5), so the cells that count are the set targets and all of them are mismatches
    metric = training.compute_evaluation_metrics(batches, prediction)
    assert both(r64, "den") > 0 and metric == np.float32(both(r64, "num")) / np.float32(both(r64, "den")) == 1.0
    # a zero denominator: numpy's 0 / 0
    for pb in batches:
        for k in pb._meta_data:
            pb._meta_data[k] = np.zeros_like(pb._meta_data[k])
    fresh = {"type": QuestionType.SCENE_GRAPH, "log_probability": like}      # (a prediction keeps the sums of its batches)
    assert np.isnan(training.compute_evaluation_metrics(batches, fresh))


def test_l1_term_follows_the_scene_loss(D):
    from dfol_vqa_amd import training
    from dfol_vqa_amd.fol_types import QuestionType
    oracle, like, batches = _oracle_and_batches(seed=3)
    prediction = {"type": QuestionType.SCENE_GRAPH, "log_probability": like}
    params = list(oracle.parameters())
    plain = training.compute_loss(batches, prediction).item()
    allp = torch.cat([p.view(-1) for p in params])
    with_l1 = training.compute_loss(batches, prediction, l1_lambda=0.25, parameters=params).item()
    assert abs(with_l1 - (plain + 0.25 * allp.abs().sum().item() / allp.numel())) <= 1e-5 * abs(plain)


# ---- golden g25_scene: the reference's own collater, oracle tables, loss and metric (tools/capture_scene_goldens.py) --------------------------
@pytest.fixture(scope="module")
def g25(D, mini_ontology_paths, golden_dir):
    from dfol_vqa_amd import data
    p = mini_ontology_paths
    ontology = D.GQAOntology(p["attribute_file"], p["class_file"], p["vocabulary_file"], p["word_embedding_file"], relation_json_path=p["relation_file"])
    a, meta = gu.load("g25_scene")
    h5 = os.path.join(golden_dir, "h5")
    coll = data.BatchGQABoxFeaturesCollator(h5, meta["feature_prefix"], meta["chunk_num"], os.path.join(h5, meta["info"]), ontology, 1)
    return ontology, a, meta, coll


def test_collater_targets_are_the_references(D, g25):
    """attribute_answer / weight, relation_answer / weight and object_pairs of hand-written questions over the g18 fixture files, against what
    the reference's collater built (batch_gqa_boxfeatures_pipeline.py:94-155): named adjectives and nouns, the noun and family columns, a
    relation and an unknown word among the attributes, an attribute and an out-of-vocabulary relation among the relations, an image
    without pairs; through collate_meta_data (the objectsNum lookup) and through the dataset's line transform and collate()."""
    from dfol_vqa_amd import data
    ontology, a, meta, coll = g25
    import copy
    md = coll.collate_meta_data(copy.deepcopy(meta["questions"]))
    assert md["object_pairs"] == meta["object_pairs"]
    for key in ("attribute_answer", "attribute_weight", "relation_answer", "relation_weight"):
        assert md[key].shape == a[key].shape and md[key].dtype == np.float32 and np.array_equal(md[key], a[key]), key
    assert a["attribute_answer"].sum() >= 10 and a["relation_answer"].sum() >= 6 and (a["relation_weight"] != 1).any()          # the golden has content
    assert (a["attribute_weight"].sum(1) == 0).any() and (a["attribute_weight"].sum(1) > 0).any()      # objects nobody names weigh nothing
    # the dataset's pass-through (data_pipeline.py:607-620) and a whole collate(): a scene-only ProgramBatch with the reference's object rows
    ds = object.__new__(data.ProgramDataset)
    ds._ontology, ds._shuffle_options, ds._is_bytecode, ds._keep_original_dict = ontology, False, False, False
    items = [ds._transform_line(copy.deepcopy(q)) for q in meta["questions"]]
    assert all(it["tokens"] == [] and "attribute_dict" in it and "relation_list" in it and "object_pairs" in it for it in items)
    (pb,) = coll.collate(items)
    assert [ob._op_name for ob in pb._op_batch_list] == ["scene"] and pb._dependencies == [[]] and pb.terminal_op_name() == "scene"
    assert pb._object_nums == meta["objects"] and np.array_equal(pb._object_features.numpy(), a["object_features"])
    assert np.array_equal(pb._meta_data["attribute_weight"], a["attribute_weight"]) and pb._meta_data["object_pairs"] == meta["object_pairs"]


def test_cpu_route_loss_and_metric_against_the_reference(D, g25):
    """ops.scene_bce's tensor-op route, compute_loss and compute_evaluation_metrics over the reference's hidden rows and this package's
    collated targets, against the reference's recorded compute_all_log_likelihood tables, _compute_loss and _compute_evaluation_metrics
    (fp32 and fp64): the loss by the rule of DESIGN.md 5 with s = sum |terms| of the fp64 tables, the metric exactly."""
    import copy
    from dfol_vqa_amd import ops, training
    from dfol_vqa_amd.fol_types import QuestionType
    from dfol_vqa_amd.visual_oracle import ClassifierOracle, EmbeddingLayer, SceneLikelihood
    ontology, a, meta, coll = g25
    w, b = torch.from_numpy(a["w:_oracle._embedding_network._network.1.weight"]), torch.from_numpy(a["w:_oracle._embedding_network._network.1.bias"])
    oracle = ClassifierOracle(ontology, None, None, EmbeddingLayer(w.shape[1], w.shape[0], 0.0, weights=w.clone(), biases=b.clone()))
    md = coll.collate_meta_data(copy.deepcopy(meta["questions"]))
    sides = (("attribute", "attr", ontology._attribute_index), ("relation", "rel", ontology._relation_index))

    def terms64(key, which):
        lp = a[key + "_table_f64"]
        p, t, wt = np.exp(lp), a[which + "_answer"], a[which + "_weight"]
        with np.errstate(divide="ignore"):
            return -wt * (t * np.maximum(np.log(p), -100) + (1 - t) * np.maximum(np.log1p(-p), -100))
    per_side = {which: terms64(key, which) for which, key, _ in sides}
    s = sum(np.abs(v).sum() for v in per_side.values())
    assert abs(sum(v.sum() for v in per_side.values()) - float(a["loss_f64"])) <= 1e-9 * s      # the recorded tables and the recorded loss belong together
    own = max(2.0 ** -20, abs(float(a["loss_f32"]) - float(a["loss_f64"])) / s)
    # each side through the public op, on the reference's fp32 hidden rows
    for which, key, index in sides:
        h = torch.from_numpy(a["h_%s_f32" % key])
        loss, num, den = ops.scene_bce(h, w, b, torch.as_tensor(np.asarray(index, np.int32)), torch.from_numpy(md[which + "_answer"]),
                                       torch.from_numpy(md[which + "_weight"]), 0.5)
        assert abs(loss.item() - per_side[which].sum()) <= 8 * own * s, (which, loss.item(), per_side[which].sum())
        t, wt = a[which + "_answer"], a[which + "_weight"]
        assert num.item() == den.item() == float((wt * (t > 0)).sum())            # every answer is 0: the set targets count, all as mismatches
    like = SceneLikelihood(torch.from_numpy(a["h_attr_f32"]), torch.from_numpy(a["h_rel_f32"]), oracle)
    prediction = {"type": QuestionType.SCENE_GRAPH, "log_probability": like}
    batches = [types.SimpleNamespace(_meta_data=md)]
    loss = training.compute_loss(batches, prediction).item()
    print("compute_loss %.9g  reference fp32 %.9g fp64 %.9g  own %.3g  ratio %.3g" % (loss, float(a["loss_f32"]), float(a["loss_f64"]), own,
                                                                                   abs(loss - float(a["loss_f64"])) / (own * s)))
    assert abs(loss - float(a["loss_f64"])) <= 8 * own * s
    metric = training.compute_evaluation_metrics(batches, prediction)
    assert metric == float(a["metric_f32"]) == float(a["metric_f64"])


def test_object_attr_and_object_rel_are_refused(D, g25):
    """A program that names object_attr or object_rel is refused with the reason, by the dataset's token extraction and by the interpreter's
    dispatch; `scene` is not."""
    from dfol_vqa_amd import data, gqa_ops
    from dfol_vqa_amd.interpreter import BatchGQAInterpreter
    ontology = g25[0]
    ds = object.__new__(data.ProgramDataset)
    ds._ontology = ontology
    assert ds._collect_tokens({"branches": [], "last_op": {"operator": "scene", "arguments": []}}) == []
    for name, word in (("object_attr", "follow-up"), ("object_rel", "cannot run in the reference")):
        with pytest.raises(NotImplementedError, match=word):
            ds._collect_tokens({"branches": [], "last_op": {"operator": name, "arguments": []}})
        with pytest.raises(NotImplementedError, match=word):
            BatchGQAInterpreter._execute(None, "0:0", None, types.SimpleNamespace(_op_name=name), (), True, False)
    gqa_ops.refuse_direct_supervision("scene")


def test_object_statement_loss_still_raises(D):
    from dfol_vqa_amd import training
    from dfol_vqa_amd.fol_types import QuestionType
    with pytest.raises(NotImplementedError):
        training.compute_loss([], {"type": QuestionType.OBJECT_STATEMENT, "log_probability": torch.zeros(1)})
