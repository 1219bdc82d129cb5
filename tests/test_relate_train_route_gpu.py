"""The route of the one-posterior Relate under autograd for the UNGATED model (DFOL_RELATE_TRAIN=1; gqa_ops.GQARelateBatch._forward_train_one,
DESIGN.md 3.7) on the synthetic ungated model of test_trainable_gate_gpu, scenes of 3..12 objects (5..20 for the one-hop program): which hops
take it, that nothing moves while the switch is unset, the two routes against each other, graph capture, and the hops that step aside."""

import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_trainable_gate_gpu as TG  # noqa: E402
from test_interpreter_gpu import TableCollater  # noqa: E402
from dfol_vqa_amd import _lib, gqa_ops, parallel, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from dfol_vqa_amd.host_util import is_valid_token  # noqa: E402

pytestmark = pytest.mark.gpu
models = TG.models                      # the seeded synthetic model, gated and ungated (module fixture, one instance for this file)
COUNTER = "relate_train_one"
SWITCH = "DFOL_RELATE_TRAIN"


@pytest.fixture(scope="module")
def ungated(models, tmp_path_factory):
    by, names = models
    model, ont = by[False]
    paths, _ = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("relate_train")))
    with open(paths["attribute_file"]) as f:
        categories = json.load(f)
    return model, ont, names, categories


def fresh(base):
    """A copy in train mode whose every floating-point parameter trains: the tile's gradient reaches the relation network and the featurizer."""
    model = copy.deepcopy(base).train()
    for k, p in model.named_parameters():
        p.requires_grad_(k != "_global_step")
    return model


def collate(ont, qs):
    pbs = TableCollater(1, ont, "X").collate([dict(q) for q in qs])
    for pb in pbs:
        pb.create_sparse_tensors()
    return [pb.to_cuda(TG.DEV) for pb in pbs]


def program_batches(ont, names, categories, kind):
    """one_hop: select -> filter -> relate -> exist; otherwise select -> 1..3 filter / relate hops -> <kind> (exist, verify_rel, choose_rel)."""
    if kind == "one_hop":
        return TG.batches(ont, names, first=80)                    # 5..20 objects
    qs = syn.full_size_questions(kind, 6, 3, 12, names, categories, 2100 + len(kind))
    return collate(ont, qs)


class Calls(object):
    """Every GQARelateBatch of the model (the relate operator's and the one verify_rel owns): how often it ran, how often with a valid token,
    and how often it went through RelateBatch.forward (the generic route; the one-launch routes do not).  inject: leave a one-sided calibration
    for the hop (subject modulations only) before it runs."""

    def __init__(self, model, inject=False):
        self.hops = self.valid = self.generic = 0
        self.inject = inject
        self._handles = []
        for m in model.modules():
            if isinstance(m, gqa_ops.GQARelateBatch):
                self._handles += [m.register_forward_pre_hook(self._hop, with_kwargs=True), m._relate.register_forward_pre_hook(self._generic)]
        assert self._handles

    def _hop(self, module, args, kwargs):
        self.hops += 1
        rel = args[3] if len(args) > 3 else kwargs["relation_list"]
        rel = rel if isinstance(rel, list) else [rel]
        self.valid += any(is_valid_token(v) for v in rel)
        if self.inject:                                               # alpha = beta = c = 1, d = 0.5: a calibration close to the identity
            mods = torch.tensor([0.1, 0.1, 0.1, 0.5], device=TG.DEV).repeat(len(rel), 1)
            module._relate._subject_modulations[args[0] if args else kwargs["op_id"]] = mods

    def _generic(self, *a):
        self.generic += 1

    def close(self):
        for h in self._handles:
            h.remove()


def grad_step(model, pbs, inject=False):
    """One training.train_batch whose step moves nothing (lr 0, a clip no gradient reaches) -> (log-probabilities, loss, {name: gradient}, calls)."""
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.0)
    calls = Calls(model, inject)
    _lib.PATH_COUNTS.clear()
    try:
        loss, res = training.train_batch(model, opt, pbs, clip_norm=1e9)
    finally:
        calls.close()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return res["log_probability"].detach().clone(), loss, grads, calls


def same_bits(a, b):
    assert np.array_equal(TG.bits(a[0]), TG.bits(b[0])) and a[1] == b[1]
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        assert np.array_equal(TG.bits(a[2][k]), TG.bits(b[2][k])), k


def no_fallbacks():
    assert not [k for k in _lib.PATH_COUNTS if k.startswith("fallback:")], dict(_lib.PATH_COUNTS)


@pytest.mark.parametrize("kind", ["one_hop", "exist", "verify_rel"])
def test_switch_set_every_relate_hop_takes_the_one_launch_route(ungated, kind, monkeypatch):
    base, ont, names, categories = ungated
    monkeypatch.setenv(SWITCH, "1")
    pbs = program_batches(ont, names, categories, kind)
    model = fresh(base)
    _, loss, grads, calls = grad_step(model, pbs)
    assert calls.valid >= 1 and _lib.PATH_COUNTS.get(COUNTER, 0) == calls.valid, (dict(_lib.PATH_COUNTS), calls.hops, calls.valid)
    assert calls.generic == calls.hops - calls.valid               # only a hop with nothing to relate goes through RelateBatch.forward
    no_fallbacks()
    assert np.isfinite(loss) and grads and all(torch.isfinite(g).all() for g in grads.values())
    # without a gradient the train route is not taken, whatever the switch says
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        model.eval()(pbs, False)
    assert not _lib.PATH_COUNTS.get(COUNTER)


@pytest.mark.parametrize("kind", ["one_hop", "exist"])
def test_switch_unset_nothing_moves(ungated, kind, monkeypatch):
    """The default's guarantee: the variable set to anything but 1 is the variable never defined, bit for bit, and the counter is absent."""
    base, ont, names, categories = ungated
    pbs = program_batches(ont, names, categories, kind)
    runs = []
    for value in (None, "0"):
        if value is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, value)
        run = grad_step(fresh(base), pbs)
        assert COUNTER not in _lib.PATH_COUNTS and run[3].generic == run[3].hops >= 1
        runs.append(run)
    same_bits(runs[0], runs[1])


@pytest.mark.parametrize("kind", ["one_hop", "exist", "verify_rel"])
def test_the_two_routes_agree(ungated, kind, monkeypatch):
    """The loss's log-probabilities under the policy of the cross-route tests (|d exp(log p)| <= 1e-5); every gradient - the oracle's weights and,
    through them, the attention inputs' - under test_trainable_gate_gpu.grad_close.  No float64 run of this model exists (the kernels compute in
    float32), so the generic route's gradient stands in both reference slots: the bound is 2e-3 of the tensor's largest magnitude."""
    base, ont, names, categories = ungated
    pbs = program_batches(ont, names, categories, kind)
    monkeypatch.delenv(SWITCH, raising=False)
    lp0, loss0, g0, _ = grad_step(fresh(base), pbs)
    monkeypatch.setenv(SWITCH, "1")
    lp1, loss1, g1, _ = grad_step(fresh(base), pbs)
    assert _lib.PATH_COUNTS.get(COUNTER, 0) >= 1
    assert (torch.exp(lp0) - torch.exp(lp1)).abs().max().item() <= 1e-5
    assert abs(loss0 - loss1) <= 1e-5 * max(1.0, abs(loss0)), (loss0, loss1)
    assert g0.keys() == g1.keys() and len(g0) >= 4
    for k in sorted(g0):
        TG.grad_close(g1[k].cpu().numpy(), g0[k].cpu().numpy(), g0[k].cpu().numpy(), k)


def test_graph_capture_under_the_switch(ungated, monkeypatch):
    """GraphedTrainStep(warmup=1) and two replays against three eager steps: the same weights, bit for bit, and the weights move."""
    base, ont, names, categories = ungated
    monkeypatch.setenv(SWITCH, "1")
    pbs = program_batches(ont, names, categories, "one_hop")
    states = {}
    for graphed in (False, True):
        model = fresh(base)
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        bucket = parallel.GradBucket(params)
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        _lib.PATH_COUNTS.clear()
        if graphed:
            step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=1)
            assert _lib.PATH_COUNTS.get(COUNTER, 0) >= 2              # the warm-up step and the capture both took the route
            step()
            step()
        else:
            for _ in range(3):
                training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)
            assert _lib.PATH_COUNTS.get(COUNTER, 0) >= 3
        torch.cuda.synchronize()
        states[graphed] = {k: v.detach().clone() for k, v in model.state_dict().items()}
        assert any(not torch.equal(before[k], states[graphed][k]) for k in before if before[k].is_floating_point())
    for k in states[False]:
        assert np.array_equal(TG.bits(states[False][k].float()), TG.bits(states[True][k].float())), k


def test_hops_that_step_aside(ungated, monkeypatch):
    """A one-sided calibration, a hop whose tokens are all invalid and choose_rel's two-posterior cell keep the generic route under the switch and
    give the bits they give without it."""
    base, ont, names, categories = ungated
    nouns, attrs = names["nouns"][:4], names["attributes"][:4]
    invalid = [syn.question(2300 + i, [[syn.op("select", nouns[i % 4]), syn.op("filter", attrs[i % 4]), syn.op("relate", "_", bool(i % 2), nouns[(i + 1) % 4])]],
                            syn.op("exist"), "yes", syn.feature_scene(2300 + i, 3 + 2 * i, 2048)) for i in range(4)]
    choose = [syn.question(2400 + i, [[syn.op("select", nouns[i % 4]), syn.op("filter", attrs[i % 4])]],
                           syn.op("choose_rel", [names["relations"][0], names["relations"][1]], bool(i % 2), nouns[(i + 1) % 4]), "yes",
                           syn.feature_scene(2400 + i, 3 + 2 * i, 2048)) for i in range(4)]
    cases = (("one-sided calibration", TG.batches(ont, names, first=80), True), ("all tokens invalid", collate(ont, invalid), False),
             ("choose_rel", collate(ont, choose), False))
    for what, pbs, inject in cases:
        runs = []
        for value in (None, "1"):
            if value is None:
                monkeypatch.delenv(SWITCH, raising=False)
            else:
                monkeypatch.setenv(SWITCH, value)
            run = grad_step(fresh(base), pbs, inject)
            assert COUNTER not in _lib.PATH_COUNTS, (what, dict(_lib.PATH_COUNTS))
            assert run[3].generic == run[3].hops, (what, run[3].generic, run[3].hops)
            runs.append(run)
        assert (runs[0][3].hops >= 1) == (what != "choose_rel"), what
        same_bits(runs[0], runs[1])
