"""GPU tests of training with dropout: a model in train() with `dropout: 0.2` takes the full-table dataflow, where every
nn.Dropout of the reference is the counter-based mask kernel of csrc/dfol_dropout.hip - exact, deterministic, replayable in a graph."""

import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import _lib, data, experiment, parallel, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from dfol_vqa_amd.data import DeviceFeatureStore  # noqa: E402
from dfol_vqa_amd.feature_store import StoreRows  # noqa: E402
from test_interpreter_gpu import DEV, TableCollater  # noqa: E402

pytestmark = pytest.mark.gpu
P = 0.2
UNFROZEN = dict(freeze_featurizer=False, freeze_attribute_network=False, freeze_relation_network=False, freeze_embedding_network=False)
# narrow networks as in golden g12's config; "full": the reference's widths (2048 -> 512, 516 / 1036 -> 256 -> 300 -> 2335)
NARROW = dict(box_features_dim=32, oracle_input_dim=16, attribute_network_layers_config=[8], relation_network_layers_config=[8], word_embedding_dim=12)
WIDTHS = {"narrow": NARROW, "full": {}}
N_OBJECTS = (3, 9, 5, 7)                                # 4 questions of 3 - 9 objects


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    paths, names = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("dropout_ontology")))
    ont = experiment.build_ontology(syn.reference_config(paths))
    return paths, names, ont


def build(world, width, dropout, seed=5, **over):
    paths, names, ont = world
    cfg = syn.reference_config(paths, dropout=dropout, **dict(UNFROZEN, **dict(WIDTHS[width], **over)))
    torch.manual_seed(seed)
    model = experiment.build_model(cfg, ont)
    with torch.no_grad():                                # GloVe-like magnitudes: sparse concept probabilities instead of saturated ones
        model._oracle._embedding_network.linear.weight.normal_(0.0, 0.1)
        model._oracle._embedding_network.linear.bias.fill_(-2.0)
    return model.to(DEV), cfg


def questions(world, width, first=8800):
    paths, names, ont = world
    F = WIDTHS[width].get("box_features_dim", 2048)
    qs = []
    for i, n in enumerate(N_OBJECTS):
        br, last = syn.three_hop_program(first + i, names["nouns"][:8], names["attributes"][:6], names["relations"][:5])
        qs.append(syn.question(first + i, br, last, "yes" if i % 2 else "no", syn.feature_scene(first + i, n, F)))
    return qs


def batches(world, qs):
    pbs = TableCollater(1, world[2], "X").collate([dict(q) for q in qs])
    return [pb.to_cuda(DEV) for pb in pbs]


def state_bits(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.named_parameters()}      # (each shared tensor once)


def same_bits(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


# ---- 1. it trains ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["narrow", "full"])
def test_train_batch_runs_with_dropout(world, width):
    """model.train() + training.train_batch at dropout 0.2: before this route existed, visual_oracle._run_layers raised DfolError here."""
    model, _ = build(world, width, P)
    model.train()
    pbs = batches(world, questions(world, width))
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    before = state_bits(model)
    _lib.PATH_COUNTS.clear()
    _lib._WARNED.discard("dropout_full_tables")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        losses = [training.train_batch(model, opt, pbs, clip_norm=0.65)[0] for _ in range(2)]
    said = [str(w.message) for w in caught if "dropout_full_tables" in str(w.message)]
    assert len(said) == 1 and "dense kernels" in said[0] and "fused pair and attribute kernels" in said[0], said     # once, not per step
    routes = dict(_lib.PATH_COUNTS)
    print(width, "losses", losses, "routes", routes)
    assert all(np.isfinite(l) for l in losses)
    assert routes.get("fallback:dropout_full_tables") == 2 and routes.get("python_program") == 2, routes
    # per forward: the featurizer's Dropout, two of each oracle MLP, the embedding layer's over the attribute and over the pair rows = 7 sites;
    # per backward one launch less: the featurizer's input takes no gradient
    assert routes.get("dropout") == 2 * (7 + 6) and routes.get("pair_features_bwd_ordered") == 2, routes
    assert not [r for r in routes if r in ("fused_hidden1", "pair_trunk", "attr_head", "native_program", "attr_ll_fused")], routes
    after = state_bits(model)
    moved = [k for k in after if not np.array_equal(after[k], before[k])]
    assert len(moved) >= 12, moved                                            # every weight and bias of the four networks trains


# ---- 2. exactness: the three MLPs restated with the kernel's own masks in float64 ----------------------------------------------------------
def _elu(x):
    return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0)))


def restated_tables(weights, raw, n_list, masks, scale, relation_index):
    """The featurizer and the oracle's tables (classifier_oracle.py:145-156; batch_gqa_boxfeatures_pipeline.py:193-281) in float64 torch on the
    CPU with the given keep masks, in site order: featurizer, attribute MLP (2), embedding over objects, relation MLP (2), embedding over pairs."""
    m = [mk.to(torch.float64) * scale for mk in masks]
    lin = lambda name, x: x @ weights[name + ".weight"].t() + weights[name + ".bias"]
    F = raw.shape[1] - 6
    f = torch.sigmoid(lin("_featurizer._featurizer_network._network.1", raw[:, :F] * m[0]))
    tail = raw[:, F:].detach()
    size = torch.clamp(torch.stack([tail[:, 0], tail[:, 1], tail[:, 0], tail[:, 1]], 1), min=1.0)
    pos = tail[:, 2:6] / size                                                        # :208-211
    obj = torch.cat([f, pos], 1)
    h = _elu(lin("_oracle._attribute_network._network.1", obj * m[1]))
    h = torch.sigmoid(lin("_oracle._attribute_network._network.4", h * m[2]))
    attr = torch.nn.functional.logsigmoid(lin("_oracle._embedding_network._network.1", h * m[3]))
    s_all, o_all, first = [], [], 0
    for n in n_list:
        s, o = np.nonzero(~np.eye(n, dtype=bool))
        s_all.append(s + first)
        o_all.append(o + first)
        first += n
    s, o = torch.from_numpy(np.concatenate(s_all)), torch.from_numpy(np.concatenate(o_all))
    ps, po = pos[s], pos[o]
    dx = ps[:, 0] + ps[:, 2] / 2 - po[:, 0] - po[:, 2] / 2
    dy = ps[:, 1] + ps[:, 3] / 2 - po[:, 1] - po[:, 3] / 2
    dist = torch.sqrt(dx * dx + dy * dy)
    geo = torch.stack([dist, torch.asin(dy / torch.clamp(dist, min=1e-10)), torch.sign(po[:, 0] - ps[:, 0]), torch.sign(po[:, 1] - ps[:, 1])], 1)
    pair = torch.cat([obj[s], obj[o], geo], 1)                                       # :252-279
    h = _elu(lin("_oracle._relation_network._network.1", pair * m[4]))
    h = torch.sigmoid(lin("_oracle._relation_network._network.4", h * m[5]))
    rel = torch.nn.functional.logsigmoid(lin("_oracle._embedding_network._network.1", h * m[6]))[:, relation_index]
    return attr, rel


def _tables_and_gradients(model, pb, fa, fr):
    """The scene's likelihood tables on the device, and the gradient of the fixed functional sum(A fa) + sum(R fr) w.r.t. every weight and
    the featurizer's input; the (site, shape, p) trace of the forward and its masks, read back before anything advances the step."""
    raw = pb._object_features.detach().clone().requires_grad_(True)
    model.zero_grad(set_to_none=True)
    trace = _lib.DROPOUT_TRACE = []
    try:
        _lib.dropout_forward_begins()
        scene = model.build_scene(DEV, raw, pb._object_batch_index, pb._meta_data, object_nums=getattr(pb, "_object_nums", None))
    finally:
        _lib.DROPOUT_TRACE = None
    A, R = scene._attribute_features, scene._relation_features["features"]
    masks = [_lib.dropout_mask(shape, p, site, DEV).cpu() for site, shape, p in trace]
    ((A * fa.to(DEV)).sum() + (R * fr.to(DEV)).sum()).backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    grads["input"] = raw.grad.detach().cpu()[:, :raw.shape[1] - 6]
    return A.detach().cpu(), R.detach().cpu(), grads, trace, masks


def _errors(model, pb, n_list, fa, fr, masks_of):
    A, R, grads, trace, masks = _tables_and_gradients(model, pb, fa, fr)
    w64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.named_parameters()}
    raw64 = pb._object_features.detach().cpu().double().requires_grad_(True)
    shapes = [tuple(raw64[:, :-6].shape)]
    rel_index = torch.as_tensor(np.asarray(model._oracle._ontology._relation_index, np.int64))
    use, scale = masks_of(trace, masks)
    A64, R64 = restated_tables(w64, raw64, n_list, use, scale, rel_index)
    ((A64 * fa.double()).sum() + (R64 * fr.double()).sum()).backward()
    g64 = {k: v.grad for k, v in w64.items() if v.grad is not None}
    g64["input"] = raw64.grad[:, :-6]
    assert sorted(g64) == sorted(grads) and len(grads) == 13, (sorted(g64), sorted(grads))
    rel = lambda got, ref: float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-300))
    err = {"attribute table": rel(A, A64.detach()), "relation table": rel(R, R64.detach())}
    err.update({"d " + k: rel(grads[k], g64[k]) for k in grads})
    return err, trace, shapes


@pytest.mark.parametrize("width", ["narrow", "full"])
def test_tables_and_gradients_are_the_restated_networks_with_the_same_masks(world, width):
    """The tolerance is not tuned against the route under test: it is the error of the SAME comparison on the same inputs and weights at p = 0 -
    the full-table dataflow as it was before this route (no mask kernel, index_add_ backward) - times two, times 1 / (1 - p) for the scale the
    kept activations and gradients carry.  Both are relative to each tensor's largest reference entry; the test prints the two figures of each
    of the fifteen tensors before it asserts.  On an MI355X, full widths: the largest error at p = 0 is 1.19e-6 (allowed with masks: 2.97e-6), the
    largest with masks 1.06e-6 (allowed for that tensor: 2.02e-6); narrow: 9.6e-7 and 8.7e-7."""
    model, cfg = build(world, width, P)
    qs = questions(world, width)
    (pb,) = batches(world, qs)
    n_list = [q["scene"]["n"] for q in qs]
    O, pairs = sum(n_list), sum(n * (n - 1) for n in n_list)
    gen = torch.Generator().manual_seed(77)
    fa, fr = torch.randn(O, 2335, generator=gen), torch.randn(pairs, 333, generator=gen)
    # p = 0 on the same weights: eval() switches every Dropout off; the oracle is told to build the full tables as the dropout route does
    model.eval()
    model._oracle._needed_columns = False
    ones = lambda trace, masks: ([torch.ones(())] * 7, 1.0)
    base, trace0, _ = _errors(model, pb, n_list, fa, fr, ones)
    assert trace0 == []
    model._oracle._needed_columns = True
    model.train()
    _lib.seed_dropout(11)
    got, trace, _ = _errors(model, pb, n_list, fa, fr, lambda trace, masks: (masks, float(np.float32(1.0) / (np.float32(1.0) - np.float32(P)))))
    F, W, Da = cfg["box_features_dim"], cfg["oracle_input_dim"], cfg["oracle_input_dim"] + 4
    Ha, Hr, E = cfg["attribute_network_layers_config"][0], cfg["relation_network_layers_config"][0], cfg["word_embedding_dim"]
    assert trace == [(0, (O, F), P), (1, (O, Da), P), (2, (O, Ha), P), (3, (O, E), P), (4, (pairs, 2 * Da + 4), P), (5, (pairs, Hr), P),
                     (6, (pairs, E), P)], trace
    for k in sorted(got):
        tol = 2.0 * base[k] / (1.0 - P)
        print("%-7s %-52s error %.3g   at p = 0 %.3g   allowed %.3g" % (width, k, got[k], base[k], tol))
    for k in sorted(got):
        assert got[k] <= 2.0 * base[k] / (1.0 - P), (width, k, got[k], base[k])


# ---- 3. determinism and graphs -----------------------------------------------------------------------------------------------------------------
def _three_steps(world, graphed, rank=None):
    model, _ = build(world, "narrow", P, seed=9)
    model.train()
    pbs = batches(world, questions(world, "narrow"))
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-2, capturable=True)
    bucket = parallel.GradBucket(params)
    _lib.seed_dropout(7, rank=rank)
    masks = []
    look = lambda: masks.append(_lib.dropout_mask((16, 64), P, 0, DEV).cpu().numpy())
    if graphed:
        step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=2)
        torch.cuda.synchronize()
        look()                                                # after the two warm-up steps: the capture itself ran nothing
        step()
        torch.cuda.synchronize()
        look()
        third = state_bits(model)
        step()
        torch.cuda.synchronize()
        look()
        return third, masks
    for _ in range(3):
        training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)
        torch.cuda.synchronize()
        look()
    return state_bits(model), masks


def test_steps_repeat_bit_for_bit_and_graph_replays_draw_new_masks(world):
    try:
        a, masks_a = _three_steps(world, graphed=False)
        b, masks_b = _three_steps(world, graphed=False)
        assert same_bits(a, b), "two models with equal weights and seed_dropout(7): other weights after three eager steps"
        assert all(np.array_equal(x, y) for x, y in zip(masks_a, masks_b))
        assert not np.array_equal(masks_a[0], masks_a[1]) and not np.array_equal(masks_a[1], masks_a[2])      # a new step, new masks
        g, masks_g = _three_steps(world, graphed=True)
        # two warm-up steps and one replay are the three eager steps; the masks read before and after each replay follow the eager steps'
        assert np.array_equal(masks_g[0], masks_a[1]) and np.array_equal(masks_g[1], masks_a[2])
        assert not np.array_equal(masks_g[1], masks_g[2]), "a second replay drew the first replay's masks"
        assert same_bits(a, g), "GraphedTrainStep(warmup=2) + one replay: other weights than three eager steps"
        c, masks_c = _three_steps(world, graphed=False, rank=1)
        assert not np.array_equal(masks_c[0], masks_a[0]) and not same_bits(a, c)                             # another rank, other masks
    finally:
        _lib.seed_dropout(torch.initial_seed())


# ---- 4. eval() is untouched -------------------------------------------------------------------------------------------------------------------
def test_eval_with_dropout_configured_is_the_dropout_zero_model(world):
    m2, _ = build(world, "full", P)
    m0, _ = build(world, "full", 0.0)
    m0.load_state_dict(m2.state_dict())
    qs = questions(world, "full")
    out = {}
    for name, model in (("p=0.2", m2.eval()), ("p=0", m0.eval())):
        pbs = batches(world, qs)
        for pb in pbs:
            pb.create_sparse_tensors()
        _lib.PATH_COUNTS.clear()
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)       # no route announces itself
            with torch.no_grad():
                res = model(pbs, False)
        out[name] = (res["log_probability"].cpu().numpy(), res["answer"], dict(_lib.PATH_COUNTS))
    (lp2, ans2, routes2), (lp0, ans0, routes0) = out["p=0.2"], out["p=0"]
    print(routes2)
    assert np.array_equal(lp2.view(np.uint32), lp0.view(np.uint32)) and ans2 == ans0
    assert routes2 == routes0 and routes2.get("native_program") == 1, (routes2, routes0)       # the executor: the fused needed-columns kernels
    assert routes2.get("dropout", 0) == 0 and not [r for r in routes2 if r.startswith("fallback:")], routes2


# ---- 5. a frozen featurizer's cached rows are not served while its Dropout drops -----------------------------------------------------------------
def test_featurized_store_steps_aside_while_the_featurizer_drops(world, tmp_path):
    from test_feature_store import write_chunks
    paths, names, ont = world
    counts = [12, 5, 9, 7]
    chunks, info = write_chunks(tmp_path, feature_dim=2048, max_obj=12, counts=counts, per_chunk=2, seed=23)
    model, _ = build(world, "full", P, freeze_featurizer=True)
    net = model._featurizer._featurizer_network
    assert not any(p.requires_grad for p in net.parameters())
    with open(paths["attribute_file"]) as f:
        cats = json.load(f)
    qs = syn.full_size_questions("exist", 4, 5, 12, names, cats, 31, with_scene=False)
    for q, im in zip(qs, [2, 0, 3, 1]):
        q["image_id"] = "img%03d" % im
    store = DeviceFeatureStore(str(tmp_path), "objs", chunks, info, DEV, featurized=True)
    pbs = data.BatchGQABoxFeaturesCollator(str(tmp_path), "objs", chunks, info, ont, 1, device_store=store.index).collate([dict(q) for q in qs])
    for pb in pbs:
        pb.create_sparse_tensors()
    dev = [pb.to_cuda(DEV) for pb in pbs]
    assert isinstance(dev[0]._object_features, StoreRows)
    keys = ("feature_store_featurized", "feature_store_featurize", "feature_store_direct_materialized", "dropout")
    model.eval()
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        model(dev, False)
    assert _lib.PATH_COUNTS["feature_store_featurized"] == 1 and _lib.PATH_COUNTS["feature_store_featurize"] == 1      # eval(): the cache serves
    model.train()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.0)
    _lib.PATH_COUNTS.clear()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        loss, _ = training.train_batch(model, opt, dev, clip_norm=0.65)
    got = {k: _lib.PATH_COUNTS.get(k, 0) for k in keys}
    print("loss", loss, got)
    assert np.isfinite(loss)
    assert got["feature_store_featurized"] == 0 and got["feature_store_featurize"] == 0 and got["feature_store_direct_materialized"] == 1, got
    assert got["dropout"] >= 7, got                           # the seven sites of the forward (and the backward's of those a gradient reaches)
    with pytest.raises(_lib.DfolError, match="Dropout"):
        store.featurize(net)
    model.eval()
    assert store.cached_for(net) is not None                  # still valid for eval()
