"""CPU tests of the host-side mirror of the reference API: program collation, lowering, ontology, gather."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
import dfol_vqa_amd as D  # noqa: E402
from dfol_vqa_amd import host_util as hu  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from dfol_vqa_amd.fol_types import TokenType  # noqa: E402
from oracle import dfol_oracle as orc  # noqa: E402


@pytest.fixture(scope="module")
def ontology(mini_ontology_paths):
    p = mini_ontology_paths
    return D.GQAOntology(p["attribute_file"], p["class_file"], p["vocabulary_file"], p["word_embedding_file"],
                         relation_json_path=p["relation_file"])


def test_g7_collate_matches_reference():
    _, meta = gu.load("g7_collate")
    coll = D.ProgramCollaterBase("select", "relate", "filter", 1)
    for case in meta["cases"]:
        ops, deps = coll.collate_programs(case["questions"])
        assert deps == case["dependencies"], case["name"]
        assert len(ops) == len(case["ops"])
        for mine, ref in zip(ops, case["ops"]):
            assert mine._op_name == ref["op_name"] and mine._is_terminal == ref["is_terminal"]
            assert [list(a) for a in mine._arguments] == ref["arguments"], (case["name"], ref["op_name"])
            assert mine._mask.tolist() == ref["mask"]
            assert mine._predicate_num == ref["predicate_num"]
            qi = None if mine._question_index is None else mine._question_index.tolist()
            assert qi == ref["question_index"]
    coll3 = D.ProgramCollaterBase("select", "relate", "filter", 3)
    qs = [dict(q, answer="yes") for q in meta["cases"][0]["questions"]]
    pbs = coll3.collate(qs)
    assert [pb.batch_size() for pb in pbs] == meta["split3_sizes"]
    assert [[ob._op_name for ob in pb._op_batch_list] for pb in pbs] == meta["split3_ops"]
    assert all(ob._op_id.startswith("%d:" % i) for i, pb in enumerate(pbs) for ob in pb._op_batch_list)


def test_collate_agrees_with_oracle_collate():
    _, meta = gu.load("g4_exist")
    qs = [{"program": q["program"]} for q in meta["questions"]]
    ops, deps = D.ProgramCollaterBase("select", "relate", "filter").collate_programs(qs)
    o_ops, o_deps = orc.collate_programs(qs)
    assert deps == o_deps
    for a, b in zip(ops, o_ops):
        assert a._op_name == b["op_name"] and [list(x) for x in a._arguments] == b["arguments"] and a._mask.tolist() == b["mask"]


def test_g8_gather_results():
    _, meta = gu.load("g8_gather")
    QT = D.QuestionType
    outs = [{"answer": [["yes"], ["no"]], "log_probability": torch.tensor([-0.1, -2.0]), "options": ["no", "yes"], "variable_set": None,
             "type": QT.BINARY, "cumulative_loss": 0, "variable_sets_num": 3, "answer_log_probability": [[-0.1], [-0.14]]},
            {"answer": [["no"], ["yes"]], "log_probability": torch.tensor([-3.0, -0.2]), "options": ["no", "yes"], "variable_set": None,
             "type": QT.BINARY, "cumulative_loss": 0, "variable_sets_num": 4, "answer_log_probability": [[-0.05], [-0.2]]}]
    res = D.gather_results(outs)
    ref = meta["binary"]
    for k in ("answer", "options", "answer_log_probability", "variable_sets_num", "cumulative_loss"):
        assert res[k] == ref[k], k
    assert int(res["type"]) == ref["type"]
    assert np.allclose(res["log_probability"].numpy(), ref["log_probability"])
    outs_q = [{"answer": [["red"]], "log_probability": torch.tensor([-0.1, -2.0]), "options": [["red", "blue"]], "variable_set": None,
               "type": QT.QUERY, "cumulative_loss": 0, "variable_sets_num": 1, "answer_log_probability": [[-0.1]]},
              {"answer": [["on"]], "log_probability": torch.tensor([-0.3, -1.0]), "options": [["on", "under"]], "variable_set": None,
               "type": QT.QUERY, "cumulative_loss": 0, "variable_sets_num": 2, "answer_log_probability": [[-0.3]]}]
    res = D.gather_results(outs_q)
    assert res["options"] == meta["query"]["options"] and res["answer"] == meta["query"]["answer"]


def test_ontology_matches_oracle_ontology(ontology, mini_ontology_paths):
    p = mini_ontology_paths
    o = orc.Ontology(p["attribute_file"], p["class_file"], p["vocabulary_file"], p["relation_file"])
    assert ontology._relation_index == o.relation_index
    assert ontology._relation_reveresed_index == o.relation_reversed
    assert "riding" in ontology._relations and "riding" not in ontology._vocabulary["arg_to_idx"]
    for name in ("color", "animal", "entity", "cup", None):
        assert sorted(map(str, ontology.query(name))) == sorted(map(str, o.query(name)))
    assert ontology.decode_token(ontology.encode_token("not(red)")) == "not(red)"
    assert ontology.decode_token(ontology.encode_token("true")) is True
    emb = ontology.get_embeddings(["to the left of", "red", "unknownword"])
    assert emb.shape == (3, 12) and np.all(emb[2] == 0) and np.abs(emb[0]).sum() > 0


def test_real_metadata_parses_like_the_reference(golden_dir):
    """The GQA metadata the reference ships (golden g25: its image-id tables stored empty) gives 2335 / 333 columns."""
    base = os.path.join(golden_dir, "g25_gqa_metadata")
    o = D.GQAOntology(os.path.join(base, "gqa_all_attribute.json"), os.path.join(base, "gqa_all_class.json"),
                      os.path.join(base, "gqa_vocab.json"), None, relation_json_path=os.path.join(base, "gqa_relation.json"))
    assert len(o._vocabulary["idx_to_arg"]) == 2335 and len(o._relation_index) == 333
    assert len(o._attribute_index) == 2335 - 333


def test_token_lowering(ontology):
    toks = ["red", None, "_", " not(blue) ", "small"]
    low = hu.lower_tokens(toks, ontology, TokenType.ATTRIBUTE)
    a2i = ontology._vocabulary["arg_to_idx"]
    assert low.cols.tolist() == [a2i["red"] - 1, -1, -1, a2i["blue"] - 1, a2i["small"] - 1]
    assert low.neg.tolist() == [0, 0, 0, 1, 0] and low.valid.tolist() == [1, 0, 0, 1, 1]
    assert low.any_neg and low.any_valid and not low.all_valid
    rel = hu.lower_tokens(["on", "not(to the left of)"], ontology, TokenType.RELATION)
    assert rel.cols.tolist() == [ontology._relation_reveresed_index[a2i["on"] - 1], ontology._relation_reveresed_index[a2i["to the left of"] - 1]]
    with pytest.raises(KeyError):
        hu.lower_tokens(["no such concept"], ontology, TokenType.ATTRIBUTE)
    # the memoised pass (every token met before: one dict.get per token inside numpy.fromiter) gives the same arrays as the first
    # resolution, also for a list that mixes met and unmet tokens, and an unknown token still raises the second time (it is never memoised)
    again = hu.lower_tokens(["small", " not(blue) ", None, "red", "red"], ontology, TokenType.ATTRIBUTE)
    assert again.cols.tolist() == [a2i["small"] - 1, a2i["blue"] - 1, -1, a2i["red"] - 1, a2i["red"] - 1] and again.neg.tolist() == [0, 1, 0, 0, 0]
    assert again.valid.tolist() == [1, 1, 0, 1, 1] and again.cols.dtype == np.int32 and again.neg.dtype == np.uint8
    mixed = hu.lower_tokens(["red", "large", "not(large)", ""], ontology, TokenType.ATTRIBUTE)
    assert mixed.cols.tolist() == [a2i["red"] - 1, a2i["large"] - 1, a2i["large"] - 1, -1] and mixed.neg.tolist() == [0, 0, 1, 0]
    with pytest.raises(KeyError):
        hu.lower_tokens(["red", "no such concept"], ontology, TokenType.ATTRIBUTE)
    same_word = hu.lower_tokens(["on"], ontology, TokenType.ATTRIBUTE) if "on" in ontology._vocabulary["arg_to_idx"] else None
    if same_word is not None:                                # (the memo is per token TYPE: a relation's column is not an attribute's)
        assert same_word.cols.tolist() == [a2i["on"] - 1]
    assert hu.detect_negations(["not(red)", "blue"]) == (True, [True, False], ["red", "blue"])
    assert hu.segments_of([0, 0, 1, 2, 2, 2]).tolist() == [0, 2, 3, 6]


def test_collater_lowers_when_given_an_ontology(ontology):
    _, meta = gu.load("g4_exist")
    qs = [{"program": q["program"], "answer": q["answer"]} for q in meta["questions"]]
    pb = D.ProgramCollaterBase("select", "relate", "filter", 1, ontology=ontology).collate(qs)[0]
    sel = pb._op_batch_list[0]
    assert sel._arguments[0].lowered is not None and sel._arguments[0].lowered.valid.tolist() == [1, 1, 0, 1, 1, 0]
    rel = [ob for ob in pb._op_batch_list if ob._op_name == "relate"][0]
    assert rel._arguments[0].lowered_type == TokenType.RELATION and rel._arguments[2].lowered_type == TokenType.ATTRIBUTE
    assert pb._question_type == D.QuestionType.BINARY
    # a collate worker process hands the batch over pickled: the operators' small host tensors travel as numpy arrays and come back as
    # tensors with their host shadows, the token lists keep their lowered forms
    import pickle
    pb.create_sparse_tensors()
    state = pb._op_batch_list[1].__getstate__()
    assert not any(isinstance(v, torch.Tensor) for v in state.values())
    back = pickle.loads(pickle.dumps([pb], protocol=pickle.HIGHEST_PROTOCOL))[0]
    assert [ob._op_name for ob in back._op_batch_list] == [ob._op_name for ob in pb._op_batch_list] and back._dependencies == pb._dependencies
    for a, b in zip(pb._op_batch_list, back._op_batch_list):
        assert (a._mask is None) == (b._mask is None) and a._predicate_num == b._predicate_num and a._op_id == b._op_id
        if a._mask is not None:
            assert isinstance(b._mask, torch.Tensor) and torch.equal(a._mask, b._mask) and b._mask._host == a._mask._host
        if a._predicate_question_map is not None:
            assert torch.equal(a._predicate_question_map, b._predicate_question_map) and b._predicate_question_map._host == a._predicate_question_map._host
        for ta, tb in zip(a._arguments, b._arguments):
            assert list(ta) == list(tb) and (ta.lowered is None) == (tb.lowered is None)
            if ta.lowered is not None:
                assert tb.lowered_type == ta.lowered_type and np.array_equal(ta.lowered.cols, tb.lowered.cols) and tb.lowered.any_valid == ta.lowered.any_valid


def test_find_max_ind_matches_oracle():
    rng = np.random.RandomState(0)
    lp = np.log(rng.uniform(size=9)).astype(np.float32)
    lp[4] = lp[3]
    pq = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2])
    assert hu.find_max_ind(lp, pq, 3).tolist() == orc.find_max_ind(lp, pq, 3).tolist()


def test_evaluation_metrics():
    from dfol_vqa_amd import training
    pb = type("PB", (), {})()
    pb._answers = ["yes", "no", "yes", "no"]
    pb.batch_size = lambda: 4
    pb._op_batch_list = [type("OB", (), {"_op_name": "exist"})()]
    pred = {"type": D.QuestionType.BINARY, "answer": [["yes"], ["yes"], ["no"], ["no"]]}
    assert training.compute_evaluation_metrics([pb], pred) == 0.5
    pq = type("PB", (), {})()
    pq._answers = ["red", "blue", "small"]
    pq.batch_size = lambda: 3
    pq._op_batch_list = [type("OB", (), {"_op_name": "query_attr"})()]
    predq = {"type": D.QuestionType.QUERY, "answer": [["red"], ["red", "blue"], []]}
    assert abs(training.compute_evaluation_metrics([pq], predq) - (1 - (1 + 0.5 + 0) / 3)) < 1e-6
    assert abs(training.compute_evaluation_metrics([pq], predq, first_answer=True) - (1 - 1 / 3)) < 1e-6
    err, tot = np.zeros(training.ERROR_DIM, np.float32), np.zeros(training.ERROR_DIM, np.float32)
    training.accumulate_test_batch(err, tot, [pb], pred)
    training.accumulate_test_batch(err, tot, [pq], predq)
    d = training.metric_dict(err / np.maximum(tot, 1))
    assert abs(d["exist"] - 0.5) < 1e-6 and abs(d["query_attr"] - 0.5) < 1e-6 and abs(d["over_all"] - (2 + 1.5) / 7) < 1e-6
    # the prediction records of VQATrainer._print_predictions (trainer.py:320-337)
    pb._meta_data = {"question_ids": ["q0", "q1", "q2", "q3"]}
    pq._meta_data = {"question_ids": ["q4", "q5", "q6"]}
    predq["options"] = [["red", "blue"], ["red", "blue"], ["small", "large"]]
    assert training.collect_predictions([pb], pred) == [{"questionId": "q%d" % i, "prediction": a, "type": "binary"}
                                                        for i, a in enumerate(["yes", "yes", "no", "no"])]
    recs = training.collect_predictions([pq], predq)
    assert recs[1] == {"questionId": "q5", "prediction": ["red", "blue"], "type": "open", "options": ["red", "blue"]}
    assert training.collect_predictions([pb], pred, is_submission=True)[2] == {"questionId": "q2", "prediction": "no"}


def test_reference_config_yamls_build(tmp_path, golden_dir):
    """Every config YAML shipped with the reference (config/*.yaml: the sample and the curriculum stages cur0..cur7, stored parsed as golden
    g26 and written back out as YAML here) loads through experiment.load_config / build_model (base_experiment.py:43-47,
    gqa_interpreter_experiments.py:107-240) with the reference's parameter counts."""
    import json
    import yaml
    from dfol_vqa_amd import experiment
    paths, _ = syn.write_synthetic_ontology(str(tmp_path))
    with open(os.path.join(golden_dir, "g26_reference_configs.json")) as f:
        stored = json.load(f)["configs"]
    cfgs = []
    for rel in sorted(stored):
        f = tmp_path / os.path.basename(rel)
        f.write_text(yaml.dump(stored[rel]))
        cfg = experiment.load_config(str(f))
        cfg.update(paths)
        cfgs.append((os.path.basename(rel), cfg))
    assert len(cfgs) == 9
    trainable = set()
    for name, cfg in cfgs:
        ont = experiment.build_ontology(cfg)
        model = experiment.build_model(cfg, ont)
        total = sum(p.numel() for p in model.parameters())
        assert total in (2303948, 2452352), (name, total)                       # without / with the attention-transfer networks
        assert total == (2452352 if cfg.get("activate_attention_transfer") else 2303948), (name, total)
        trainable.add(sum(p.numel() for p in model.parameters() if p.requires_grad))
        names = set(model.state_dict())
        assert "_oracle._embedding_network._network.1.weight" in names and "_featurizer._featurizer_network._network.1.weight" in names
    if len(cfgs) == 9:                                       # oracle phases, embedding-frozen phase, calibrator phases
        assert trainable == {2303947, 1254859, 148404}, trainable


def test_mlp_math_config_key(tmp_path):
    """`mlp_math` (an extra key of this build, BASELINE configs[3]): fp32 is the default, bf16 is recorded on the interpreter, anything
    else is rejected."""
    from dfol_vqa_amd import experiment
    from dfol_vqa_amd import synthetic as syn
    paths, _ = syn.write_synthetic_ontology(str(tmp_path))
    cfg = syn.reference_config(paths)
    ont = experiment.build_ontology(cfg)
    assert getattr(experiment.build_model(dict(cfg), ont), "_mlp_math", None) is None
    assert experiment.build_model(dict(cfg, mlp_math="bf16"), ont)._mlp_math == "bf16"
    assert experiment.build_model(dict(cfg, mlp_math="bf16x3"), ont)._mlp_math == "bf16x3"      # exact-range forward products
    with pytest.raises(ValueError):
        experiment.build_model(dict(cfg, mlp_math="fp8"), ont)


def test_pattern_singularize_restatement():
    """preprocess.pattern_singularize restates pattern.text.en.singularize (parse_utils.py:6, 20; the library is not in this image, so
    this is a self-consistency table, not a pinned one): exception tables before suffix rules, first matching rule wins.  One check IS anchored
    in the reference: its own `irregulars` table (parse_utils.py:14) exists to override what the library returns for 'shelves' - and the
    restated rules do return 'shelve' for it - while `normalize` applies the reference's table first."""
    from dfol_vqa_amd.preprocess import normalize, pattern_singularize as sg
    expect = {"dogs": "dog", "men": "man", "women": "woman", "people": "person", "children": "child", "leaves": "leaf", "knives": "knife",
              "wolves": "wolf", "boxes": "box", "buses": "bus", "dishes": "dish", "benches": "bench", "tomatoes": "tomato", "shoes": "shoe",
              "mice": "mouse", "feet": "foot", "teeth": "tooth", "geese": "goose", "cherries": "cherry", "keys": "key", "cookies": "cookies", "Ties": "ties",
              "movies": "movie", "halves": "half", "wives": "wife", "scarves": "scarf", "sandwiches": "sandwich", "cacti": "cactus",
              "media": "medium", "analyses": "analysis", "oxen": "ox", "matrices": "matrix", "vertices": "vertex", "news": "news",
              "series": "series", "fish": "fish", "sheep": "sheep", "deer": "deer", "scissors": "scissors", "mothers-in-law": "mother-in-law",
              "dogs'": "dog's", "shelves": "shelve"}
    got = {w: sg(w) for w in expect}
    assert got == expect, {w: (got[w], expect[w]) for w in expect if got[w] != expect[w]}
    assert normalize("Shelves") == "shelf" and normalize(" Men ") == "man" and normalize("glasses") == "glasses" and normalize("dress") == "dress"
    assert normalize("tennis shorts") == "tennis shorts" and normalize("Buses") == "bus" and normalize("grass") == "grass"
    # the -ie plurals: pattern 3.x hands them back unchanged (see pattern_singularize), which is WHY the reference lists these two as irregulars
    assert normalize("cookies") == "cookie" and normalize("Brownies") == "brownie" and sg("zombies") == "zombies"


def test_operator_batch_from_pretransposed_arguments_keeps_the_reference_analysis():
    """data_pipeline.py:33-62: OperatorBatch(..., process_args=False) takes the argument slots as given but STILL derives the predicate count
    and the predicate -> question index from the first slot; only to_cuda's internal field-by-field copy skips the analysis."""
    import dfol_vqa_amd as D
    slots = [[["red", "small"], ["blue"], ["tall", "thin", "old"]], [None, None, None]]
    ob = D.OperatorBatch("filter", slots, 3, False, process_args=False)
    assert ob._predicate_num == 6 and ob._question_index.tolist() == [0, 0, 1, 2, 2, 2]
    same = D.OperatorBatch("filter", [["red", None], ["blue", None], ["tall", None]], 3, False)
    flat = D.OperatorBatch("filter", same._arguments, 3, False, process_args=False)
    assert flat._predicate_num == 3 and flat._question_index is None
