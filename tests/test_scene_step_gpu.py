"""The scene-graph train step over a PREPARED batch (data.prepare_scene_batch) on the GPU: eager against the float64 restatement of
tests/test_scene_op_gpu.py (the same 3-image batch, model and tolerances), exact padding, the captured step (training.GraphedTrainStep) against
eager steps bit for bit, `load`, Dropout 0.2 under capture, repeatability and a batch without listed pairs.

GraphedTrainStep's warm-up steps are train steps (warmup >= 1 is required): a captured step with warmup=1 followed by three replays is compared
with FOUR eager train_batch steps from the same initial weights and optimizer state - replay k against eager step k + 1."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
from dfol_vqa_amd import _lib, data, parallel, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from test_interpreter_gpu import DEV  # noqa: E402
from test_scene_op_gpu import SceneCollater, check_step, train_once  # noqa: E402
from test_scene_op_gpu import questions as base_questions  # noqa: E402
from test_train_dropout_gpu import build, same_bits, state_bits, world  # noqa: E402,F401

pytestmark = pytest.mark.gpu
P_DROP = 0.2
PAD_O, PAD_P = 37, 19


def scene_questions(world, objects, pairs, first, seed):
    """test_scene_op_gpu.questions with the object counts as a parameter (the second batch of `load`)."""
    paths, names, ont = world
    rng = np.random.RandomState(seed)
    attrs, rels = names["attributes"][:6] + names["nouns"][:6], names["relations"][:5]
    qs = []
    for i, (n, k) in enumerate(zip(objects, pairs)):
        q = syn.question(first + i, [], syn.op("scene"), "", syn.feature_scene(first + i, n, 32))
        s = [int(x) for x in rng.randint(0, n, size=k)]
        o = [int((a + 1 + rng.randint(0, n - 1)) % n) for a in s] if n > 1 else []
        q["object_pairs"] = {"subject_id": s, "object_id": o}
        q["attribute_dict"] = {str(j): [(attrs[rng.randint(len(attrs))], float(rng.randint(1, 9)) / 4.0) for _ in range(1 + j % 2)] for j in range(0, n, 2)}
        q["relation_list"] = [(rels[rng.randint(len(rels))], float(rng.randint(1, 9)) / 4.0) for _ in range(k)]
        qs.append(q)
    return qs


def host_batch(world, qs):
    (pb,) = SceneCollater(1, world[2], "X").collate([dict(q) for q in qs])
    return pb


def prepared(world, qs, objects=None, pairs=None):
    return data.prepare_scene_batch(host_batch(world, qs), DEV, objects=objects, pairs=pairs)


def sums_of(pbs, result):
    return [[float(x.detach()) for x in side] for side in training._scene_sums(pbs, result)]


def grads_bits_equal(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_prepared_batch_against_the_restatement(world):
    model, _ = build(world, "narrow", 0.0)
    model.train()
    pbs = [prepared(world, base_questions(world))]
    ps = pbs[0]._scene_prepared
    assert (ps.O, ps.P, ps.objects, ps.pairs, ps.images) == (18, 10, 18, 10, 3) and ps.features.is_cuda
    _lib.PATH_COUNTS.clear()
    loss, result, grads = train_once(model, pbs)
    routes = dict(_lib.PATH_COUNTS)
    assert routes.get("scene_python") == 1 and routes.get("scene_pair_rows") == 1 and routes.get("scene_pair_rows_hip") == 1, routes
    assert routes.get("scene_bce_hip") == 2 and not [r for r in routes if r.startswith("fallback:")], routes
    check_step(model, pbs, world[2], loss, grads, "prepared scene step")
    assert training.compute_evaluation_metrics(pbs, result) == 1.0
    # the unprepared route still takes the tensor-op rows
    plain = [host_batch(world, base_questions(world)).to_cuda(DEV)]
    _lib.PATH_COUNTS.clear()
    train_once(model, plain)
    assert _lib.PATH_COUNTS.get("scene_python") == 1 and "scene_pair_rows" not in _lib.PATH_COUNTS


def test_padding_is_exact(world):
    model, _ = build(world, "narrow", 0.0)
    model.train()
    qs = base_questions(world)
    plain = [prepared(world, qs)]
    loss0, result0, grads0 = train_once(model, plain)
    sums0 = sums_of(plain, result0)
    r64, r32 = check_step(model, plain, world[2], loss0, grads0, "unpadded")
    outs = []
    for seed in (1, 2):
        pbs = [prepared(world, qs, objects=18 + PAD_O, pairs=10 + PAD_P)]
        ps = pbs[0]._scene_prepared
        assert tuple(ps.features.shape)[0] == 18 + PAD_O and tuple(ps.relation_weight.shape)[0] == 10 + PAD_P
        noise = torch.as_tensor(np.random.RandomState(seed).normal(size=(PAD_O, ps.features.shape[1])).astype(np.float32)).to(DEV)
        noise[:, -6:] = noise[:, -6:].abs() + 1.0                   # (image size and box columns: positive, as a collater's)
        ps.features[18:].copy_(noise)                               # finite, arbitrary rows where the padding's zero rows were
        loss, result, grads = train_once(model, pbs)
        outs.append((loss, sums_of(pbs, result), grads))
    assert not torch.equal(noise, torch.zeros_like(noise))
    (la, sa, ga), (lb, sb, gb) = outs
    assert la == lb and sa == sb and grads_bits_equal(ga, gb), "two paddings, other bits"
    # against the unpadded batch: the restatement's tolerances (test_scene_op_gpu.check_step: check_loss and check_gradient)
    import scene_util as su
    su.check_loss(la, r32, r64, "padded")
    for k in sorted(ga):
        gu.check_gradient(ga[k], r32["grads"][k], r64["grads"][k], "padded d " + k)
    assert sa[0][1:] == sums0[0][1:] and sa[1][1:] == sums0[1][1:]  # the metric's sums are sums of eighths and quarters: exact


def start(world, dropout, seed=9):
    model, _ = build(world, "narrow", dropout, seed=seed)
    model.train()
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-2, capturable=True)
    bucket = parallel.GradBucket(params)
    assert training.FusedClipAdam.make(opt, bucket) is not None
    return model, opt, bucket


def eager_steps(world, pbs, n, dropout=0.0, seed_dropout=None):
    model, opt, bucket = start(world, dropout)
    if seed_dropout is not None:
        _lib.seed_dropout(seed_dropout)
    out = []
    for _ in range(n):
        loss, _ = training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)
        out.append((float(loss), state_bits(model)))
    return out


def graphed_steps(world, pbs, replays, dropout=0.0, seed_dropout=None, between=None):
    model, opt, bucket = start(world, dropout)
    if seed_dropout is not None:
        _lib.seed_dropout(seed_dropout)
    step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=1)
    out = []
    for k in range(replays):
        if between is not None:
            between(k, step)
        loss, result = step()
        out.append((float(loss), state_bits(model)))
    return out, step, model


def same_steps(got, want, what):
    for k, ((lg, sg), (lw, sw)) in enumerate(zip(got, want)):
        assert lg == lw, "%s: replay %d loss %.9g, eager %.9g" % (what, k, lg, lw)
        assert same_bits(sg, sw), "%s: replay %d left other weights than the eager step" % (what, k)


def test_capture_replays_are_the_eager_steps(world):
    qs = base_questions(world)
    pad = dict(objects=18 + PAD_O, pairs=10 + PAD_P)
    want = eager_steps(world, [prepared(world, qs, **pad)], 4)
    pbs = [prepared(world, qs, **pad)]
    got, step, model = graphed_steps(world, pbs, 3)
    same_steps(got, want[1:], "capture")
    assert want[1][0] != want[2][0] and not same_bits(want[1][1], want[2][1])          # the steps move
    assert training.compute_evaluation_metrics(pbs, step.result) == 1.0                  # the replay's own sums, no launch
    assert step.result["_scene_sums"][0] is pbs


def test_unprepared_batch_is_refused_under_capture(world, monkeypatch):
    """The guard of the interpreter, asked as a capture asks it (_lib.capturing()), without starting one: the message names the remedy."""
    model, _ = build(world, "narrow", 0.0)
    model.train()
    plain = [host_batch(world, base_questions(world)).to_cuda(DEV)]
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    with pytest.raises(NotImplementedError, match="prepare_scene_batch"):
        model(plain, True)


def test_load_serves_another_batch(world):
    qs = base_questions(world)
    other = scene_questions(world, (4, 9, 7), (2, 0, 11), first=9300, seed=6)       # 20 objects, 13 pairs: other counts, within the capacities
    caps = dict(objects=18 + PAD_O, pairs=10 + PAD_P)
    # eager: one step on the first batch (the capture's warm-up), then steps on the second, prepared to the same capacities
    model, opt, bucket = start(world, 0.0)
    training.train_batch(model, opt, [prepared(world, qs, **caps)], 0.65, bucket=bucket, sync_loss=False)
    second = [prepared(world, other, **caps)]
    want = []
    for _ in range(2):
        loss, _ = training.train_batch(model, opt, second, 0.65, bucket=bucket, sync_loss=False)
        want.append((float(loss), state_bits(model)))
    pbs = [prepared(world, qs, **caps)]
    got, step, _ = graphed_steps(world, pbs, 2, between=lambda k, step: step.load(host_batch(world, other)) if k == 0 else None)
    same_steps(got, want, "load")
    ps = pbs[0]._scene_prepared
    assert (ps.O, ps.P) == (20, 13) and pbs[0]._object_nums == [4, 9, 7]
    assert not ps.features[20:].any() and not ps.attribute_weight[20:].any() and not ps.relation_weight[13:].any() and not ps.pair_s[13:].any()
    metric = training.compute_evaluation_metrics(pbs, step.result)
    assert metric == 1.0
    four = scene_questions(world, (4, 9, 7, 2), (2, 0, 11, 1), first=9300, seed=6)
    with pytest.raises(_lib.DfolError, match="4 images"):
        step.load(host_batch(world, four))
    with pytest.raises(_lib.DfolError, match="above the capacity of %d object rows" % (18 + PAD_O)):
        step.load(host_batch(world, scene_questions(world, (30, 20, 6), (2, 0, 1), first=9400, seed=7)))
    with pytest.raises(_lib.DfolError, match="above the capacity of %d pair rows" % (10 + PAD_P)):
        step.load(host_batch(world, scene_questions(world, (4, 9, 7), (12, 9, 9), first=9500, seed=8)))
    assert (ps.O, ps.P) == (20, 13)                                  # a refused batch leaves the loaded one in place


def test_dropout_under_capture(world):
    qs = base_questions(world)
    caps = dict(objects=18 + PAD_O, pairs=10 + PAD_P)
    try:
        want = eager_steps(world, [prepared(world, qs, **caps)], 3, dropout=P_DROP, seed_dropout=13)
        got, _, _ = graphed_steps(world, [prepared(world, qs, **caps)], 2, dropout=P_DROP, seed_dropout=13)
        same_steps(got, want[1:], "dropout")
        assert got[0][0] != got[1][0]                                # two consecutive replays: other masks, another loss
        # and the masks do matter: the same replays at another seed give another loss
        again, _, _ = graphed_steps(world, [prepared(world, qs, **caps)], 1, dropout=P_DROP, seed_dropout=14)
        assert again[0][0] != got[0][0]
    finally:
        _lib.seed_dropout(torch.initial_seed())


def test_two_constructions_give_the_same_bits(world):
    qs = base_questions(world)
    caps = dict(objects=18 + PAD_O, pairs=10 + PAD_P)
    try:
        a, _, _ = graphed_steps(world, [prepared(world, qs, **caps)], 3, dropout=P_DROP, seed_dropout=21)
        b, _, _ = graphed_steps(world, [prepared(world, qs, **caps)], 3, dropout=P_DROP, seed_dropout=21)
    finally:
        _lib.seed_dropout(torch.initial_seed())
    same_steps(a, b, "repeat")


def test_no_listed_pairs_captures_and_replays(world):
    qs = base_questions(world, pairs=(0, 0, 0))
    want = eager_steps(world, [prepared(world, qs)], 3)
    pbs = [prepared(world, qs)]
    assert pbs[0]._scene_prepared.pairs == 0
    got, step, _ = graphed_steps(world, pbs, 2)
    same_steps(got, want[1:], "no pairs")
    assert all(np.isfinite(l) for l, _ in got)
