"""The two one-posterior train routes of gqa_ops.GQARelateBatch._forward_train_one under a CALIBRATED operator, where no golden
exists: DFOL_RELATE_TRAIN=1 on the ungated model and DFOL_GATE_TRAIN=1 on the gated one, both built with activate_attention_transfer as
test_gate_native_gpu.test_calibrated_gated_model_stays_on_the_executor builds its model (seeded weights, a seeded calibrator whose output layer is
not zero, distinct gates).  Every floating-point parameter trains (the fresh() convention), so the calibrated branch's backward carries gradient
into the LSTM calibrator, through relate_keep*_bwd into x, prev and the tile - the relation network - and, gated, into the gates.  (Golden g24
pins the ungated route against the reference with the oracle frozen and no gates: tests/test_backward_gpu.py.)

No float64 run of these models exists, so the routes are held to each other under the cross-route policy of
test_relate_train_route_gpu.test_the_two_routes_agree: |d exp(log p)| <= 1e-5, the loss within 1e-5 max(1, |loss|), every gradient under
test_trainable_gate_gpu.grad_close with the generic route in both reference slots (2e-3 of the tensor's largest magnitude).  The generic route
calibrates both posteriors of a hop and discards one; the one-launch route never computes it, so the calibrator's gradients agreeing is the
check that the discarded side contributes nothing.

Batches: syn.full_size_questions for exist and verify_rel (6 questions, 3..12 objects) and one exist batch whose largest scene has 70 objects
(NS > 64: dfol_modulate_bwd_f32's second pass of the column loop, through the route), collated with test_native_gpu's full calibration
collater."""

import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_trainable_gate_gpu as TG  # noqa: E402
import test_relate_train_route_gpu as RT  # noqa: E402
from test_gate_native_gpu import _FullCalibrationCollater, distinct_gates  # noqa: E402
from dfol_vqa_amd import _lib, parallel, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu
SWITCH = {False: "DFOL_RELATE_TRAIN", True: "DFOL_GATE_TRAIN"}
COUNTER = {False: "relate_train_one", True: "relate_gate_train_one"}
KINDS = {"exist": ("exist", 3100), "verify_rel": ("verify_rel", 3101), "exist70": ("exist", 3102)}     # name -> (terminal operator, seed)
STATE = ("_modulations", "_subject_modulations", "_object_modulations", "_forward_state", "_forward_subject_state", "_forward_object_state")
GATED = pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
_RUNS = {}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The ungated and the gated calibrated model, once, and the three batches."""
    from dfol_vqa_amd import experiment
    paths, names = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("relate_train_calibrated")))
    with open(paths["attribute_file"]) as f:
        categories = json.load(f)
    by = {}
    for gated in (False, True):
        cfg = syn.reference_config(paths, activate_attention_transfer=True, trainable_gate=gated)
        ont = experiment.build_ontology(cfg)
        torch.manual_seed(5)
        model = experiment.build_model(cfg, ont)
        syn.load_seeded_weights(model, 23)
        syn.load_seeded_calibrator(model, 29)                      # (the reference initialises the output layer's weight to zero)
        if gated:
            distinct_gates(model)
        assert model._has_modulator
        by[gated] = (model.to(TG.DEV).eval(), ont)
    questions = {}
    for name, (kind, seed) in KINDS.items():
        qs = syn.full_size_questions(kind, 6, 3, 12, names, categories, seed)
        if name == "exist70":                                      # the question with two relate hops looks at 70 objects
            assert sum(o["operator"] == "relate" for o in qs[3]["program"]["branches"][0]) == 2
            qs[3]["scene"] = syn.feature_scene(qs[3]["question_id"], 70, 2048)
        questions[name] = qs
    assert max(q["scene"]["n"] for q in questions["exist70"]) == 70 and max(q["scene"]["n"] for q in questions["exist"]) <= 12
    return by, questions


def batches(setup, gated, name):
    by, questions = setup
    pbs = _FullCalibrationCollater(1, by[gated][1]).collate([dict(q) for q in questions[name]])
    for pb in pbs:
        pb.create_sparse_tensors()
    return [pb.to_cuda(TG.DEV) for pb in pbs]


def fresh(setup, gated):
    """A copy in train mode whose every floating-point parameter trains: the oracle, the calibrator and the gates all receive gradient."""
    model = copy.deepcopy(setup[0][gated][0]).train()
    for k, p in model.named_parameters():
        p.requires_grad_(k != "_global_step")
    return model


class Calls(RT.Calls):
    """test_relate_train_route_gpu.Calls, and how many of the valid calls found their op_id in BOTH modulation dictionaries."""

    def __init__(self, model):
        self.calibrated = 0
        super(Calls, self).__init__(model)

    def _hop(self, module, args, kwargs):
        before = self.valid
        super(Calls, self)._hop(module, args, kwargs)
        op_id, r = (args[0] if args else kwargs["op_id"]), module._relate
        if self.valid > before:
            self.calibrated += (r._subject_modulations.get(op_id) is not None and r._object_modulations.get(op_id) is not None)


def no_state_left(model, when):
    for mod in model.modules():
        for attr in STATE:
            assert not getattr(mod, attr, None), (when, type(mod).__name__, attr)


def grad_step(setup, gated, name, monkeypatch, value):
    """One training.train_batch whose step moves nothing (lr 0, a clip no gradient reaches) with the model's switch at `value` (None: undefined)
    -> (log-probabilities, loss, {name: gradient}, calls, route counters); once per (model, batch, value)."""
    key = (gated, name, value)
    if key in _RUNS:
        return _RUNS[key]
    for k in SWITCH.values():
        monkeypatch.delenv(k, raising=False)
    if value is not None:
        monkeypatch.setenv(SWITCH[gated], value)
    model, pbs = fresh(setup, gated), batches(setup, gated, name)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.0)
    calls = Calls(model)
    _lib.PATH_COUNTS.clear()
    try:
        loss, res = training.train_batch(model, opt, pbs, clip_norm=1e9)
    finally:
        calls.close()
    torch.cuda.synchronize()
    no_state_left(model, key)
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    _RUNS[key] = (res["log_probability"].detach().clone(), loss, grads, calls, dict(_lib.PATH_COUNTS))
    return _RUNS[key]


def calibrator_names(grads):
    names = sorted(k for k in grads if "attention" in k)
    assert len(names) == 10, names                                  # LSTMCell x 2 (4 tensors each) + the output layer's weight and bias, shared
    return names


@GATED
@pytest.mark.parametrize("name", list(KINDS))
def test_switch_set_every_calibrated_hop_takes_the_one_launch_route(setup, gated, name, monkeypatch):
    _, loss, grads, calls, counts = grad_step(setup, gated, name, monkeypatch, "1")
    assert calls.valid >= (3 if name == "verify_rel" else 1) and calls.calibrated == calls.valid, (calls.valid, calls.calibrated)
    assert counts.get(COUNTER[gated], 0) == calls.valid and COUNTER[not gated] not in counts, (counts, calls.hops, calls.valid)
    assert calls.generic == calls.hops - calls.valid               # only a hop with nothing to relate goes through RelateBatch.forward
    assert not [k for k in counts if k.startswith("fallback:")], counts
    assert np.isfinite(loss) and all(torch.isfinite(g).all() for g in grads.values())
    lstm = [k for k in calibrator_names(grads) if "_forward_attention_network" in k or "_backward_attention_network" in k]
    assert len(lstm) == 8 and any(grads[k].abs().max() > 0 for k in lstm)
    assert any(grads[k].abs().max() > 0 for k in grads if "_relation_network" in k)
    if gated:
        used = [k for k in grads if "_ops.relate._relate._blc._nlg" in k]
        assert len(used) == 4 and all(grads[k].abs().max() > 0 for k in used), used


@GATED
@pytest.mark.parametrize("name", list(KINDS))
def test_the_two_routes_agree(setup, gated, name, monkeypatch):
    lp0, loss0, g0, calls0, counts0 = grad_step(setup, gated, name, monkeypatch, None)
    lp1, loss1, g1, _, counts1 = grad_step(setup, gated, name, monkeypatch, "1")
    assert COUNTER[gated] not in counts0 and calls0.generic == calls0.hops and counts1.get(COUNTER[gated], 0) >= 1
    # the generic route calibrates the posterior it then discards: its zero cotangent must leave no NaN or Inf in a calibrator gradient
    for k in calibrator_names(g0):
        assert torch.isfinite(g0[k]).all() and g0[k].abs().max() > 0, k
    assert (torch.exp(lp0) - torch.exp(lp1)).abs().max().item() <= 1e-5
    assert abs(loss0 - loss1) <= 1e-5 * max(1.0, abs(loss0)), (loss0, loss1)
    assert g0.keys() == g1.keys() and calibrator_names(g1) == calibrator_names(g0)
    assert any("_relation_network" in k for k in g0) and (not gated or sum("_nlg" in k for k in g0) >= 4)
    worst = {}
    for k in sorted(g0):
        a, b = g1[k].cpu().numpy(), g0[k].cpu().numpy()
        TG.grad_close(a, b, b, k)
        group = "calibrator" if "attention" in k else "gates" if "_nlg" in k else "oracle"
        worst[group] = max(worst.get(group, 0.0), float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)))
    print("  %s %s: |d exp(lp)| %.3g  |d loss| %.3g  largest |d grad| / scale (bound 2e-3): %s" % (
        "gated" if gated else "ungated", name, (torch.exp(lp0) - torch.exp(lp1)).abs().max().item(), abs(loss0 - loss1),
        ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


@GATED
def test_switch_unset_nothing_moves(setup, gated, monkeypatch):
    """The variable set to "0" is the variable never defined, bit for bit, and the counter is absent."""
    runs = [grad_step(setup, gated, "exist", monkeypatch, value) for value in (None, "0")]
    for run in runs:
        assert COUNTER[gated] not in run[4] and run[3].generic == run[3].hops >= 1
    RT.same_bits(runs[0], runs[1])


@GATED
def test_graph_capture_under_the_switch(setup, gated, monkeypatch):
    """GraphedTrainStep(warmup=1) and two replays against three eager steps at the tolerances of
    test_backward_gpu.test_graphed_train_step_equals_eager (which says why a calibrator phase is not bit-exact): the warm-up and the capture
    both take the route, and no modulation is left behind by the capture or by a replay."""
    for k in SWITCH.values():
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(SWITCH[gated], "1")
    states, per_step = {}, None
    for graphed in (False, True):
        model, pbs = fresh(setup, gated), batches(setup, gated, "exist")
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        bucket = parallel.GradBucket(params)
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        _lib.PATH_COUNTS.clear()
        if graphed:
            step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=1)
            assert _lib.PATH_COUNTS.get(COUNTER[gated], 0) == 2 * per_step, dict(_lib.PATH_COUNTS)     # the warm-up step and the capture
            no_state_left(model, "after capture")
            for i in range(2):
                step()
                no_state_left(model, "after replay %d" % i)
            assert _lib.PATH_COUNTS.get(COUNTER[gated], 0) == 2 * per_step                             # (a replay runs no Python)
        else:
            for _ in range(3):
                training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)
            assert _lib.PATH_COUNTS.get(COUNTER[gated], 0) % 3 == 0
            per_step = _lib.PATH_COUNTS.get(COUNTER[gated], 0) // 3
            assert per_step >= 1
            no_state_left(model, "after the eager steps")
        torch.cuda.synchronize()
        states[graphed] = {k: v.detach().clone() for k, v in model.state_dict().items()}
        moved = [k for k in before if before[k].is_floating_point() and not torch.equal(before[k], states[graphed][k])]
        assert any("attention" in k for k in moved) and any("_relation_network" in k for k in moved), moved
        assert not gated or sum("_ops.relate._relate._blc._nlg" in k for k in moved) == 4, moved
    for k in states[False]:
        a, b = states[False][k].float(), states[True][k].float()
        assert torch.allclose(a, b, rtol=1e-5, atol=2e-6), (k, (a - b).abs().max().item())
