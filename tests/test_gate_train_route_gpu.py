"""The route of the one-posterior gated Relate under autograd (DFOL_GATE_TRAIN=1; gqa_ops.GQARelateBatch._forward_train_one) on the
gated synthetic model of test_trainable_gate_gpu: which hops take it, that nothing moves while the switch is unset, the two routes against each
other, graph capture, and the ungated model."""

import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_trainable_gate_gpu as TG  # noqa: E402
from dfol_vqa_amd import _lib, parallel, training  # noqa: E402

pytestmark = pytest.mark.gpu
models = TG.models                      # the seeded synthetic model, gated and ungated (module fixture, one instance for this file)
COUNTER = "relate_gate_train_one"


def distinct_gates(model, seed=7):
    """Every gate tensor its own values (torch's initialisation leaves them small)."""
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "_nlg" in k:
                p.copy_(torch.from_numpy(rng.uniform(-0.7, 0.7, tuple(p.shape)).astype(np.float32)))


def fresh(base, gates_only=False):
    """A copy in train mode.  The fixture's config freezes the oracle: gates_only keeps that (the relation tile then needs no gradient), otherwise
    every floating-point parameter trains, so the tile's gradient reaches the relation network and the featurizer."""
    model = copy.deepcopy(base).train()
    distinct_gates(model)
    for k, p in model.named_parameters():
        p.requires_grad_("_nlg" in k or (not gates_only and k != "_global_step"))
    return model


class Calls(object):
    """How often the relate operator ran, and how often it went through RelateBatch.forward (the generic route; the one-launch routes do not)."""

    def __init__(self, model):
        self.hops = self.generic = 0
        op = model._ops["relate"]
        self._handles = [op.register_forward_pre_hook(self._hop), op._relate.register_forward_pre_hook(self._generic)]

    def _hop(self, *a):
        self.hops += 1

    def _generic(self, *a):
        self.generic += 1

    def close(self):
        for h in self._handles:
            h.remove()


def grad_step(model, pbs):
    """One training.train_batch whose step moves nothing (lr 0, a clip no gradient reaches) -> (log-probabilities, loss, {name: gradient}, calls)."""
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=0.0)
    calls = Calls(model)
    _lib.PATH_COUNTS.clear()
    try:
        loss, res = training.train_batch(model, opt, pbs, clip_norm=1e9)
    finally:
        calls.close()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return res["log_probability"].detach().clone(), loss, grads, calls


def test_switch_set_every_relate_hop_takes_the_one_launch_route(models, monkeypatch):
    by, names = models
    base, ont = by[True]
    monkeypatch.setenv("DFOL_GATE_TRAIN", "1")
    for gates_only in (False, True):                              # the oracle trains too / the gates alone require a gradient
        model = fresh(base, gates_only)
        pbs = TG.batches(ont, names, first=80)
        _, loss, grads, calls = grad_step(model, pbs)
        assert calls.hops >= 1 and _lib.PATH_COUNTS.get(COUNTER, 0) == calls.hops, (dict(_lib.PATH_COUNTS), calls.hops)
        assert calls.generic == 0
        assert np.isfinite(loss)
        used = [k for k in grads if "_ops.relate._relate._blc._nlg" in k]
        assert len(used) == 4 and all(grads[k].abs().max() > 0 and torch.isfinite(grads[k]).all() for k in used), used
    # without a gradient the train route is not taken, whatever the switch says
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        model.eval()(pbs, False)
    assert not _lib.PATH_COUNTS.get(COUNTER)


def test_switch_unset_nothing_moves(models, monkeypatch):
    by, names = models
    base, ont = by[True]
    monkeypatch.delenv("DFOL_GATE_TRAIN", raising=False)
    pbs = TG.batches(ont, names, first=80)
    runs = []
    for _ in range(2):
        lp, loss, grads, calls = grad_step(fresh(base), pbs)
        assert not _lib.PATH_COUNTS.get(COUNTER) and calls.generic == calls.hops >= 1
        runs.append((lp, loss, grads))
    assert np.array_equal(TG.bits(runs[0][0]), TG.bits(runs[1][0])) and runs[0][1] == runs[1][1]
    assert runs[0][2].keys() == runs[1][2].keys()
    for k in runs[0][2]:
        assert np.array_equal(TG.bits(runs[0][2][k]), TG.bits(runs[1][2][k])), k


def test_the_two_routes_agree(models, monkeypatch):
    """The loss's log-probabilities under the policy of the cross-route test of test_gate_native_gpu (|d exp(log p)| <= 1e-5); every gradient
    under test_trainable_gate_gpu.grad_close.  No float64 run of this model exists (the kernels compute in float32), so the generic route's
    gradient stands in both reference slots: the bound is 2e-3 of the tensor's largest magnitude."""
    by, names = models
    base, ont = by[True]
    pbs = TG.batches(ont, names, first=80)
    monkeypatch.delenv("DFOL_GATE_TRAIN", raising=False)
    lp0, loss0, g0, _ = grad_step(fresh(base), pbs)
    monkeypatch.setenv("DFOL_GATE_TRAIN", "1")
    lp1, loss1, g1, _ = grad_step(fresh(base), pbs)
    assert _lib.PATH_COUNTS.get(COUNTER, 0) >= 1
    assert (torch.exp(lp0) - torch.exp(lp1)).abs().max().item() <= 1e-5
    assert abs(loss0 - loss1) <= 1e-5 * max(1.0, abs(loss0)), (loss0, loss1)
    assert g0.keys() == g1.keys() and any("_nlg" in k for k in g0)
    for k in sorted(g0):
        TG.grad_close(g1[k].cpu().numpy(), g0[k].cpu().numpy(), g0[k].cpu().numpy(), k)


def test_graph_capture_under_the_switch(models, monkeypatch):
    """GraphedTrainStep(warmup=1) and two replays against three eager steps: the same weights, bit for bit, and the gates move."""
    by, names = models
    base, ont = by[True]
    monkeypatch.setenv("DFOL_GATE_TRAIN", "1")
    pbs = TG.batches(ont, names, first=80)
    states = {}
    for graphed in (False, True):
        model = fresh(base, gates_only=True)
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-2, capturable=True)
        bucket = parallel.GradBucket(params)
        before = {k: v.detach().clone() for k, v in model.state_dict().items() if "_nlg" in k}
        _lib.PATH_COUNTS.clear()
        if graphed:
            step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=1)
            assert _lib.PATH_COUNTS.get(COUNTER, 0) >= 2              # the warm-up step and the capture both took the route
            step()
            step()
        else:
            for _ in range(3):
                training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)
        torch.cuda.synchronize()
        states[graphed] = {k: v.detach().clone() for k, v in model.state_dict().items()}
        moved = [k for k in before if not torch.equal(before[k], states[graphed][k])]
        assert sum("_ops.relate._relate." in k for k in moved) == 4, moved
    for k in states[False]:
        assert np.array_equal(TG.bits(states[False][k].float()), TG.bits(states[True][k].float())), k


def test_ungated_model_ignores_the_switch(models, monkeypatch):
    by, names = models
    base, ont = by[False]
    pbs = TG.batches(ont, names, first=80)
    out = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("DFOL_GATE_TRAIN", switch)
        lp, loss, grads, _ = grad_step(fresh(base), pbs)            # (no gates to set; the oracle trains)
        assert grads
        assert not _lib.PATH_COUNTS.get(COUNTER)
        out[switch] = (lp, loss, grads)
    assert np.array_equal(TG.bits(out["0"][0]), TG.bits(out["1"][0])) and out["0"][1] == out["1"][1]
    for k in out["0"][2]:
        assert np.array_equal(TG.bits(out["0"][2][k]), TG.bits(out["1"][2][k])), k
