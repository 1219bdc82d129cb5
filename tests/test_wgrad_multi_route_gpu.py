"""The train step's route to the one-pass weight gradient of several readers (DFOL_WGRAD_MULTI=1; visual_oracle._HeadUse.backward defers the
reader's dW2 share, _PairTrunk.backward runs ONE dfol_pair_wgrad_fused_multi_f32 before it hands out dW2): a full-size train step (dropout 0) on
8 questions x 20..40 objects with select -> 1..3 relate hops -> exist, and on golden g19's choose_rel batch (two option slots = two readers).

With the switch on the route is taken (asserted from `_lib.PATH_COUNTS`), the loss is the bits of the DFOL_WGRAD_MULTI=0 run, every gradient meets
test_backward_gpu.grad_close's rule (8 x the fp32 restatement's own deviation from fp64 + 2e-3 of the scale) against that run and against the fp64
CPU autograd of oracle/dfol_oracle_torch.train_loss; a replayed GraphedTrainStep equals eager steps bit for bit; a one-reader batch and a
DFOL_HEAD_SUMS=1 run never take the route."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
from dfol_vqa_amd import _lib, parallel, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from test_interpreter_gpu import DEV, TableCollater  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from dfol_vqa_amd import experiment
    from oracle import dfol_oracle as orc
    paths, names = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("wgrad_multi")))
    cfg = syn.reference_config(paths, freeze_featurizer=False, freeze_attribute_network=False, freeze_relation_network=False, freeze_embedding_network=False)
    ont = experiment.build_ontology(cfg)
    model = experiment.build_model(cfg, ont)
    a, meta = gu.load("g19_full_size_train_step")
    weights = syn.load_seeded_weights(model, meta["weight_seed"])
    oont = orc.Ontology(paths["attribute_file"], paths["class_file"], paths["vocabulary_file"], paths["relation_file"])
    return model.to(DEV).train(), ont, oont, weights, a, meta, names


def _hop_questions(names, hops_of, base):
    """select -> hops_of[i] relate hops -> exist on scenes of 20..40 objects"""
    rels, nouns = names["relations"][:5], names["nouns"][:8]
    qs = []
    for i, hops in enumerate(hops_of):
        qid = base + i
        branch = [syn.op("select", nouns[i % 8])]
        for h in range(hops):
            branch.append(syn.op("relate", rels[(i + h) % 5], bool((i + h) % 2), nouns[(i + h + 1) % 8] if h + 1 < hops else "_"))
        qs.append(syn.question(qid, [branch], syn.op("exist"), "yes" if i % 2 else "no", syn.feature_scene(qid, 20 + (7 * i) % 21, 2048)))
    return qs


def _step(model, ont, qs):
    pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ont, "X").collate([dict(q) for q in qs])]
    model.zero_grad(set_to_none=True)
    _lib.PATH_COUNTS.clear()
    res = model(pbs, True)
    loss = training.compute_loss(pbs, res) / len(qs)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().numpy() for k, p in model.named_parameters()}
    return float(loss.detach()), grads, dict(_lib.PATH_COUNTS)


def _close(got, other, ref32, ref64, what):
    """grad_close's rule (test_backward_gpu.py) with `other` in the place of the fp64 reference"""
    got, other, ref32, ref64 = (np.asarray(x, np.float64) for x in (got, other, ref32, ref64))
    scale, own = np.abs(ref64).max() + 1e-30, np.abs(ref32 - ref64).max()
    err = np.abs(got - other).max()
    assert err <= 8 * own + 2e-3 * scale, "%s: |dgrad| %.3g vs the restatement's own %.3g (scale %.3g)" % (what, err, own, scale)


def _batch(setup, which):
    model, ont, oont, weights, a, meta, names = setup
    if which == "hops":
        return _hop_questions(names, [1, 2, 3, 2, 1, 3, 3, 2], 881000)
    return gu.g19_case("query_rel_small", a, meta)[0]


@pytest.mark.parametrize("which", ["hops", "choose_rel"])
def test_train_step_takes_the_one_pass_and_computes_what_the_readers_one_by_one_do(setup, which, monkeypatch):
    from oracle import dfol_oracle_torch as orct
    model, ont, oont, weights, a, meta, names = setup
    qs = _batch(setup, which)
    monkeypatch.setenv("DFOL_HEAD_SUMS", "auto")
    monkeypatch.setenv("DFOL_WGRAD_MULTI", "0")
    loss0, g0, r0 = _step(model, ont, qs)
    assert r0.get("pair_wgrad_multi", 0) == 0 and r0.get("head_use_dw_deferred", 0) == 0, r0
    monkeypatch.setenv("DFOL_WGRAD_MULTI", "1")
    loss1, g1, r1 = _step(model, ont, qs)
    assert not [r for r in r1 if r.startswith("fallback:")], r1
    assert r1.get("pair_wgrad_multi", 0) == 1 and r1.get("head_use_dw_deferred", 0) >= 2, r1
    assert r1.get("head_use_backward", 0) >= 2, r1
    assert loss1 == loss0
    scenes = [q["scene"] for q in qs]
    _, _, o64 = orct.train_loss(oont, qs, scenes, weights, torch.float64)
    _, _, o32 = orct.train_loss(oont, qs, scenes, weights, torch.float32)
    for pname, ref64 in o64.items():
        _close(g1[pname], g0[pname], o32[pname], ref64, "%s d%s against the readers one by one" % (which, pname))
        _close(g1[pname], ref64, o32[pname], ref64, "%s d%s against fp64" % (which, pname))
    # the same step again: the same bits (no atomics in the new pass; ragged hop counts bring torch's atomic index_select backward in elsewhere)
    if which == "choose_rel":
        loss2, g2, _ = _step(model, ont, qs)
        assert loss2 == loss1


def test_one_reader_and_the_sums_route_never_defer(setup, monkeypatch):
    model, ont, oont, weights, a, meta, names = setup
    monkeypatch.setenv("DFOL_WGRAD_MULTI", "1")
    monkeypatch.setenv("DFOL_HEAD_SUMS", "auto")
    _, _, r = _step(model, ont, _hop_questions(names, [1] * 8, 882000))
    assert r.get("head_use", 0) == 1 and r.get("pair_wgrad_multi", 0) == 0 and r.get("head_use_dw_deferred", 0) == 0, r
    monkeypatch.setenv("DFOL_HEAD_SUMS", "1")
    _, _, r = _step(model, ont, _hop_questions(names, [2] * 8, 883000))
    assert r.get("head_use", 0) >= 2 and r.get("pair_wgrad_multi", 0) == 0 and r.get("head_use_dw_deferred", 0) == 0, r


def test_graphed_replay_equals_eager_with_the_one_pass(setup, monkeypatch):
    """select -> relate -> relate -> exist for every question (aligned hop counts: every route deterministic)"""
    model, ont, oont, weights, a, meta, names = setup
    monkeypatch.setenv("DFOL_WGRAD_MULTI", "1")
    monkeypatch.setenv("DFOL_HEAD_SUMS", "auto")
    qs = _hop_questions(names, [2] * 8, 884000)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    finals = []
    try:
        for graphed in (False, True):
            model.load_state_dict(start)
            model.zero_grad(set_to_none=True)
            pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ont, "X").collate([dict(q) for q in qs])]
            params = [p for p in model.parameters() if p.requires_grad]
            opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
            bucket = parallel.GradBucket(params)
            _lib.PATH_COUNTS.clear()
            if graphed:
                step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=1)
                losses = [float(step()[0]) for _ in range(3)]
            else:
                losses = [float(training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)[0]) for _ in range(4)][1:]
            torch.cuda.synchronize()
            assert _lib.PATH_COUNTS.get("pair_wgrad_multi", 0) >= 1, dict(_lib.PATH_COUNTS)
            finals.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    finally:
        model.load_state_dict(start)
        model.zero_grad(set_to_none=True)
    (l0, s0), (l1, s1) = finals
    assert l0 == l1, (l0, l1)
    bad = [k for k in s0 if not torch.equal(s0[k], s1[k])]
    assert not bad, bad
