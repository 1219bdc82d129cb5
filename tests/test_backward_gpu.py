"""GPU parity of the training path: loss values and gradients w.r.t. the cached tables against the goldens g6
(the reference's own autograd), kernel-level gradient checks against a torch fp64 restatement, and one train step."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
import dfol_vqa_amd as D  # noqa: E402
from dfol_vqa_amd import ops, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from test_interpreter_gpu import DEV, TableCollater, neural_model, table_model  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 1e-20


@pytest.fixture(scope="module")
def ontology(mini_ontology_paths):
    p = mini_ontology_paths
    return D.GQAOntology(p["attribute_file"], p["class_file"], p["vocabulary_file"], p["word_embedding_file"],
                         relation_json_path=p["relation_file"])


def grad_close(got, ref32, ref64, what, rtol=2e-3):
    """Gradients inherit the conditioning of the forward: yardstick = the reference's own fp32-vs-fp64 deviation."""
    got, ref32, ref64 = (np.asarray(x, np.float64) for x in (got, ref32, ref64))
    scale = np.abs(ref64).max() + 1e-30
    own = np.abs(ref32 - ref64).max()
    err = np.abs(got - ref64).max()
    assert err <= 8 * own + rtol * scale, "%s: |dgrad| %.3g vs reference's own %.3g (scale %.3g)" % (what, err, own, scale)


@pytest.mark.parametrize("name", ["g6_loss_binary", "g6_loss_query", "g6_loss_query_rel"])
def test_g6_loss_and_table_gradients(ontology, name):
    a, meta = gu.load(name)
    qs, scenes = gu.questions_and_scenes(a, meta)
    qq = [dict(q, scene=s) for q, s in zip(qs, scenes)]
    pbs = TableCollater(1, ontology).collate(qq)
    for pb in pbs:
        pb.create_sparse_tensors()
    pbs = [pb.to_cuda(DEV) for pb in pbs]
    pb = pbs[0]
    A = pb._object_features.clone().requires_grad_(True)
    R = pb._meta_data["R"].clone().requires_grad_(True)
    pb._object_features, pb._meta_data["R"] = A, R
    model = table_model(ontology).train()
    res = model(pbs, True)
    loss = training.compute_loss(pbs, res) / len(qs)
    loss.backward()
    l32, l64 = float(a["loss_f32"]), float(a["loss_f64"])
    assert abs(float(loss.detach()) - l64) <= 8 * abs(l32 - l64) + 2e-5 * max(1.0, abs(l64)), (float(loss.detach()), l32, l64)
    gu.check_logprob(res["log_probability"].detach().cpu().numpy(), a["lp_f32"], a["lp_f64"], name)
    grad_close(A.grad.cpu().numpy(), a["gA_f32"], a["gA_f64"], name + " dA")
    gR = np.zeros_like(a["gR_f64"]) if R.grad is None else R.grad.cpu().numpy()
    grad_close(gR, a["gR_f32"], a["gR_f64"], name + " dR")


# ---------------------------------------------------------------------------------------------------
# kernel-level gradient checks against torch autograd on an fp64 restatement of the block formulas
# ---------------------------------------------------------------------------------------------------
def t_slog(x):
    return torch.log(x.clamp_min(EPS))


def t_pnot(x, a):
    return t_slog(a + (1 - 2 * a) * torch.exp(x))


def ref_relate(a, b, l, qs, qo, neg, any_neg):
    n = a.shape[0]
    l = torch.minimum(l, torch.zeros_like(l))
    if any_neg:
        l = t_pnot(l, torch.tensor(float(neg), dtype=l.dtype))
    off = 1 - torch.eye(n, dtype=l.dtype)
    t = t_pnot(l + b[None, :], qo) * off
    ps = a + t_pnot(t.sum(1), qo)
    w = t_pnot(l + a[:, None], qs) * off
    po = b + t_pnot(w.sum(0), qs)
    return ps, po


@pytest.mark.parametrize("n_list,k_list,any_neg", [([5, 3, 8], [1, 1, 1], False), ([12, 7], [2, 1], True), ([70, 100], [1, 1], False),
                                                   ([290, 17], [1, 2], True),      # NS = 292: beyond the registers-per-row kernels
                                                   ([650, 9], [1, 1], False)])     # NS = 652: relate_bwd on four wavefronts per predicate (LDS), sixteen below
def test_relate_filter_quantify_backward(n_list, k_list, any_neg):
    rng = np.random.RandomState(sum(n_list) + int(any_neg))
    Q = len(n_list)
    pq = np.repeat(np.arange(Q), k_list).astype(np.int32)
    P, NS = len(pq), max(4, (max(n_list) + 3) // 4 * 4)
    prior_s = np.zeros((Q, NS), np.float32)
    prior_o = np.zeros((Q, NS), np.float32)
    tile = np.full((P, NS, NS), -30, np.float32)
    for q, n in enumerate(n_list):
        prior_s[q, :n] = np.minimum(syn.table_log_likelihood(rng, (n,), "unif") * 0.3, 0)
        prior_o[q, :n] = np.minimum(syn.table_log_likelihood(rng, (n,), "unif") * 0.3, 0)
    # With `unif` tiles every quantifier is saturated from about 60 objects on and the true tile gradient is below 1e-19: the large cases
    # (the 16-wavefront, 4-wavefront and LDS paths) take EXISTS over the thinned mix10 family of test_logic_backward_gpu.py (`forall`
    # where negated), whose float64 gradient passes the non-triviality assert below; FOR_ALL at these sizes is covered there.
    big = max(n_list) >= 64
    if big:
        from test_logic_backward_gpu import _likelihood
        quant = np.ones((P, 2), np.float32)
        neg = (rng.uniform(size=P) < 0.5).astype(np.uint8) if any_neg else None
    for p in range(P):
        n = n_list[pq[p]]
        t = _likelihood(rng, (n, n), "forall" if any_neg and neg[p] else "mix10", n) if big else syn.table_log_likelihood(rng, (n, n), "unif")
        t[np.arange(n), np.arange(n)] = -30
        tile[p, :n, :n] = t
    if not big:
        quant = (rng.uniform(size=(Q, 2)) < 0.6).astype(np.float32)[pq]
        neg = (rng.uniform(size=P) < 0.5).astype(np.uint8) if any_neg else None
    gs = rng.normal(size=(P, NS)).astype(np.float32)
    go = rng.normal(size=(P, NS)).astype(np.float32)
    dev = lambda x: torch.tensor(x, device=DEV)
    ps_t, po_t, tl_t = dev(prior_s).requires_grad_(True), dev(prior_o).requires_grad_(True), dev(tile).requires_grad_(True)
    n_obj = dev(np.array(n_list, np.int32))
    ps, po = ops.relate_fwd(ps_t, po_t, tl_t, dev(pq), n_obj, dev(quant[:, 0]), dev(quant[:, 1]), None if neg is None else dev(neg))
    (ps * dev(gs)).sum().add((po * dev(go)).sum()).backward()
    # fp64 torch restatement
    a64 = torch.tensor(prior_s, dtype=torch.float64, requires_grad=True)
    b64 = torch.tensor(prior_o, dtype=torch.float64, requires_grad=True)
    t64 = torch.tensor(tile, dtype=torch.float64, requires_grad=True)
    total = 0
    for p in range(P):
        q, n = pq[p], n_list[pq[p]]
        if n < 2:
            continue
        rs, ro = ref_relate(a64[q, :n], b64[q, :n], t64[p, :n, :n], float(quant[p, 0]), float(quant[p, 1]), 0 if neg is None else int(neg[p]), any_neg)
        total = total + (rs * torch.tensor(gs[p, :n], dtype=torch.float64)).sum() + (ro * torch.tensor(go[p, :n], dtype=torch.float64)).sum()
    total.backward()
    for got, ref, what in ((ps_t.grad, a64.grad, "d prior_s"), (po_t.grad, b64.grad, "d prior_o"), (tl_t.grad, t64.grad, "d tile")):
        g, r = got.cpu().numpy().astype(np.float64), ref.numpy()
        assert np.abs(g - r).max() <= 2e-4 * (np.abs(r).max() + 1), (what, np.abs(g - r).max(), np.abs(r).max())
    r = t64.grad.numpy()                                     # the tile gradient compared above is worth comparing
    owned = np.concatenate([np.abs(r[p, :n_list[pq[p]], :n_list[pq[p]]])[~np.eye(n_list[pq[p]], dtype=bool)] for p in range(P)])
    assert np.abs(r).max() >= 1e-3 and (owned > 1e-6 * np.abs(r).max()).mean() >= 0.1, (np.abs(r).max(), (owned > 1e-6 * np.abs(r).max()).mean())
    # filter + quantify chained
    ll = dev(tile[:, 0, :].copy()).requires_grad_(True)
    att0 = dev(prior_s).requires_grad_(True)
    out = ops.filter_fwd(att0, ll, dev(pq), n_obj, None if neg is None else dev(neg))
    lp = ops.quantify_fwd(out, dev(quant[:, 0]), dev(pq), n_obj)
    glp = rng.normal(size=P).astype(np.float32)
    (lp * dev(glp)).sum().backward()
    l64 = torch.tensor(tile[:, 0, :], dtype=torch.float64, requires_grad=True)
    p64 = torch.tensor(prior_s, dtype=torch.float64, requires_grad=True)
    tot = 0
    for p in range(P):
        q, n = pq[p], n_list[pq[p]]
        v = torch.minimum(l64[p, :n], torch.zeros(n, dtype=torch.float64))
        if any_neg:
            v = t_pnot(v, torch.tensor(float(neg[p]), dtype=torch.float64))
        o = p64[q, :n] + v
        qf = float(quant[p, 0])
        tot = tot + glp[p] * t_pnot(t_pnot(o, qf).sum(), qf)
    tot.backward()
    for got, ref, what in ((ll.grad, l64.grad, "d ll"), (att0.grad, p64.grad, "d att")):
        g, r = got.cpu().numpy().astype(np.float64), ref.numpy()
        assert np.abs(g - r).max() <= 2e-4 * (np.abs(r).max() + 1), (what, np.abs(g - r).max())


def test_train_step_changes_parameters_and_lowers_loss(ontology):
    """One reference-style train step (fwd + BCE + bwd + clip + Adam) on the reduced-dims neural oracle."""
    a, meta = gu.load("g5_neural_oracle")
    weights = {k[2:]: a[k] for k in a.files if k.startswith("w:")}
    model = neural_model(ontology, meta["config"], weights).train()
    qs, scenes = gu.questions_and_scenes(a, meta, "X")
    qq = [dict(q, scene=s, answer="yes" if i % 2 == 0 else "no") for i, (q, s) in enumerate(zip(qs, scenes))]
    pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ontology, "X").collate(qq)]
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    losses = [training.train_batch(model, opt, pbs, clip_norm=0.65)[0] for _ in range(5)]
    changed = [k for k, v in model.state_dict().items() if k.startswith("_oracle._") and not torch.equal(v, before[k])]
    assert len(changed) >= 6, changed
    assert losses[-1] < losses[0], losses
    assert all(np.isfinite(l) for l in losses)


@pytest.mark.parametrize("name", ["binary", "query_rel"])
@pytest.mark.parametrize("needed", [True, False])
def test_g12_weight_gradients(ontology, name, needed):
    """Gradients of the train-step loss w.r.t. every weight (featurizer, attribute / relation MLPs, embedding layer) equal the
    reference's own autograd (golden g12), on both training dataflows: the needed-columns one and the full cached tables."""
    a, meta = gu.load("g12_weight_gradients")
    weights = {k[2:]: a[k] for k in a.files if k.startswith("w:")}
    model = neural_model(ontology, meta["config"], weights).train()
    model._oracle._needed_columns = needed
    qs = [{"program": q["program"], "answer": q["answer"], "question_id": q["question_id"], "image_id": "img000", "tokens": [],
           "original_dict": None, "question": None, "scene": {"n": q["n"], "X": a["%s:X_%d" % (name, i)]}}
          for i, q in enumerate(meta["sets"][name]["questions"])]
    pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ontology, "X").collate(qs)]
    res = model(pbs, True)
    loss = training.compute_loss(pbs, res) / len(qs)
    loss.backward()
    l32, l64 = float(a[name + ":loss_f32"]), float(a[name + ":loss_f64"])
    assert abs(float(loss.detach()) - l64) <= 8 * abs(l32 - l64) + 2e-5 * max(1.0, abs(l64)), (float(loss.detach()), l32, l64)
    checked = 0
    for pname, prm in model.named_parameters():
        key = "%s:g:%s:f64" % (name, pname)
        if key not in a.files:
            continue
        g = np.zeros_like(a[key]) if prm.grad is None else prm.grad.detach().cpu().numpy()
        grad_close(g, a[key[:-3] + "f32"], a[key], "%s d%s (needed=%s)" % (name, pname, needed))
        checked += 1
    assert checked == 12


@pytest.mark.parametrize("n", [6, 9])
def test_uniform_batch_training_dataflow(ontology, n):
    """Batches whose images all have the same object count train on the broadcast form of the pair MLP ([Q, n, n, H], no gathers):
    its loss and weight gradients equal those of the full-table dataflow, which golden g12 pins to the reference."""
    a, meta = gu.load("g12_weight_gradients")
    weights = {k[2:]: a[k] for k in a.files if k.startswith("w:")}
    base = meta["sets"]["query_rel" if n == 9 else "binary"]["questions"]
    qs = [{"program": q["program"], "answer": q["answer"], "question_id": q["question_id"], "image_id": "img000", "tokens": [],
           "original_dict": None, "question": None, "scene": syn.feature_scene(7000 + i, n, meta["config"]["box_features_dim"])}
          for i, q in enumerate(base)]
    out = {}
    for needed in (True, False):
        model = neural_model(ontology, meta["config"], weights).train()
        model._oracle._needed_columns = needed
        pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ontology, "X").collate([dict(q) for q in qs])]
        res = model(pbs, True)
        loss = training.compute_loss(pbs, res) / len(qs)
        loss.backward()
        out[needed] = (float(loss.detach()), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None})
    assert abs(out[True][0] - out[False][0]) <= 1e-5 * max(1.0, abs(out[False][0]))
    assert set(out[True][1]) == set(out[False][1]) and len(out[True][1]) >= 12
    for k, g in out[False][1].items():
        scale = g.abs().max().item() + 1e-30
        assert (out[True][1][k] - g).abs().max().item() <= 2e-4 * scale + 1e-9, k


def test_calibrator_phase_train_step(ontology):
    """cur6-7 style: oracle frozen, only the attention-calibration networks train; the forward runs on the fused
    needed-columns kernels and the gradient reaches the LSTMs through the modulate op."""
    from test_interpreter_gpu import CalibrationCollater
    a, meta = gu.load("g10_calibration")
    weights = {k[2:]: a[k] for k in a.files if k.startswith("w:")}
    model = neural_model(ontology, meta["config"], weights).train()
    trainable = [n for n, p in model.named_parameters() if p.requires_grad]
    assert trainable and all("attention" in n for n in trainable), trainable
    run_meta = meta["runs"]["exist"]
    qs = [{"program": q["program"], "answer": "yes" if i % 2 else "no", "question_id": q["question_id"], "image_id": "img000", "tokens": [],
           "original_dict": None, "question": None, "scene": {"n": q["n"], "X": a["exist:X_%d" % i]}} for i, q in enumerate(run_meta["questions"])]
    pbs = [pb.to_cuda(DEV) for pb in CalibrationCollater(ontology).collate(qs)]
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=5e-2)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    losses = []
    for _ in range(6):
        loss, _ = training.train_batch(model, opt, pbs, clip_norm=0.65)
        losses.append(loss)
    after = model.state_dict()
    moved = {k for k in after if not torch.equal(after[k], before[k])}
    assert moved and all("attention" in k for k in moved), sorted(moved)[:5]
    assert losses[-1] < losses[0] and all(np.isfinite(l) for l in losses), losses


@pytest.mark.parametrize("phase", ["oracle", "calibrator"])
def test_graphed_train_step_equals_eager(ontology, phase):
    """training.GraphedTrainStep (zero grads -> forward -> loss -> backward -> clip -> Adam as ONE captured HIP graph) against the same
    steps launched eagerly: the same losses and parameters after three steps (the graph replays the same launches), for an oracle phase (g12's model: every weight trains) and a calibrator phase (g10's: attention networks only)."""
    from dfol_vqa_amd import parallel
    if phase == "oracle":
        from test_interpreter_gpu import TableCollater as Coll
        a, meta = gu.load("g12_weight_gradients")
        name = sorted(meta["sets"])[0]
        quest = meta["sets"][name]["questions"]
        make = lambda: Coll(1, ontology, "X")
        xkey = lambda i: "%s:X_%d" % (name, i)
    else:
        from test_interpreter_gpu import CalibrationCollater
        a, meta = gu.load("g10_calibration")
        quest = meta["runs"]["exist"]["questions"]
        make = lambda: CalibrationCollater(ontology)
        xkey = lambda i: "exist:X_%d" % i
    weights = {k[2:]: a[k] for k in a.files if k.startswith("w:")}
    qs = [{"program": q["program"], "answer": "yes" if i % 2 else "no", "question_id": q["question_id"], "image_id": "img000", "tokens": [],
           "original_dict": None, "question": None, "scene": {"n": q["n"], "X": a[xkey(i)]}} for i, q in enumerate(quest)]
    finals = []
    for graphed in (False, True):
        model = neural_model(ontology, meta["config"], weights).train()
        pbs = [pb.to_cuda(DEV) for pb in make().collate(qs)]
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-2, capturable=True)
        bucket = parallel.GradBucket(params)
        if graphed:                                          # one eager warm-up step (it fills the host-side caches), then three replays
            step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=1)
            losses = [float(step()[0]) for _ in range(3)]
        else:
            losses = [float(training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)[0]) for _ in range(4)][1:]
        finals.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    (l0, s0), (l1, s1) = finals
    # (not asserted bit for bit: at these reduced dims a few products fall below the size thresholds of this library's GEMM kernels and go
    # through the vendor BLAS, which picks another algorithm - other roundings, 1 ulp - when it cannot allocate workspace under capture)
    assert np.allclose(l0, l1, rtol=1e-5, atol=1e-6), (l0, l1)
    for k in s0:
        assert torch.allclose(s0[k], s1[k], rtol=1e-5, atol=2e-6), (k, (s0[k] - s1[k]).abs().max().item())
    assert l0[-1] != l0[0]


def test_calibrator_gradients_native_backward_equals_torch_autograd(ontology, monkeypatch):
    """The calibrator phases' backward on this library's kernels (dfol_lstm_cell_bwd_f32 + dense / TN products, dfol_modulate_bwd_f32)
    against the same step with torch's own LSTM cell and autograd through the tensor-op restatement of apply_modulations
    (DFOL_LSTM_BWD=torch, DFOL_MODULATE_BWD=torch): every trainable gradient agrees (batch_base_ops.py:407-467, 598-684;
    batch_base_interpreter.py:87-140)."""
    from test_interpreter_gpu import CalibrationCollater
    a, meta = gu.load("g10_calibration")
    weights = {k[2:]: a[k] for k in a.files if k.startswith("w:")}
    run_meta = meta["runs"]["verify_rel"] if "verify_rel" in meta["runs"] else meta["runs"]["exist"]
    name = "verify_rel" if "verify_rel" in meta["runs"] else "exist"
    qs = [{"program": q["program"], "answer": "yes" if i % 2 else "no", "question_id": q["question_id"], "image_id": "img000", "tokens": [],
           "original_dict": None, "question": None, "scene": {"n": q["n"], "X": a["%s:X_%d" % (name, i)]}} for i, q in enumerate(run_meta["questions"])]
    grads = {}
    for mode in ("hip", "torch"):
        monkeypatch.setenv("DFOL_LSTM_BWD", mode)
        monkeypatch.setenv("DFOL_MODULATE_BWD", mode)
        model = neural_model(ontology, meta["config"], weights).train()
        with torch.no_grad():                                # a non-degenerate attention output layer (the reference initialises it to zero)
            g = torch.Generator().manual_seed(3)
            for n_, p_ in model.named_parameters():
                if p_.requires_grad and p_.dim() == 2 and float(p_.abs().max()) == 0.0:
                    p_.copy_((torch.randn(p_.shape, generator=g) * 0.05).to(p_.device))
        pbs = [pb.to_cuda(DEV) for pb in CalibrationCollater(ontology).collate(qs)]
        res = model(pbs, True)
        loss = training.compute_loss(pbs, res) / len(qs)
        loss.backward()
        grads[mode] = {n_: p_.grad.detach().clone() for n_, p_ in model.named_parameters() if p_.requires_grad and p_.grad is not None}
    assert grads["hip"].keys() == grads["torch"].keys() and len(grads["hip"]) >= 6
    for n_ in grads["hip"]:
        gh, gt = grads["hip"][n_].double(), grads["torch"][n_].double()
        scale = gt.abs().max().item()
        assert scale > 0, n_
        assert (gh - gt).abs().max().item() <= 2e-4 * scale + 1e-7, (n_, (gh - gt).abs().max().item(), scale)


@pytest.mark.parametrize("n_list,hid1,hid2", [([7, 1, 13, 2, 30, 5], 64, 50), ([40, 33], 256, 300), ([3, 3, 3], 16, 7), ([100, 12], 256, 300),
                                              ([70, 1, 9, 71], 256, 20), ([100, 150, 1, 37], 128, 32)])       # (three slot batches per subject)
def test_fused_pair_training_kernels_against_autograd(n_list, hid1, hid2):
    """csrc/dfol_pair_train.hip against the tensor-op formulation it replaces (gathers, adds, ELU, Sigmoid, embedding product, row sums
    and their autograd): forward values and all five gradients, ragged scenes incl. images with one object, fp64 reference."""
    from dfol_vqa_amd import _lib
    rng = np.random.RandomState(sum(n_list) + hid1)
    n = np.asarray(n_list, np.int64)
    O, Q, pairs = int(n.sum()), len(n_list), int((n * (n - 1)).sum())
    obj_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    pair_off = np.concatenate([[0], np.cumsum(n * (n - 1))]).astype(np.int64)
    s_idx, o_idx = [], []
    for q, k in enumerate(n_list):
        s, o = np.nonzero(~np.eye(k, dtype=bool))
        s_idx.append(s + obj_off[q]), o_idx.append(o + obj_off[q])
    s_idx, o_idx = np.concatenate(s_idx), np.concatenate(o_idx)
    dev = lambda a, dt=None: torch.as_tensor(a if dt is None else np.asarray(a, dt)).to(DEV)
    U, V = rng.normal(size=(O, hid1)).astype(np.float32), rng.normal(size=(O, hid1)).astype(np.float32)
    pos = rng.uniform(0.05, 0.9, (O, 6)).astype(np.float32)[:, 1:5]              # a strided view, like obj[:, D-4:]
    Wg = rng.normal(size=(hid1, 4)).astype(np.float32) * 0.5
    gz = rng.normal(size=(pairs, hid1)).astype(np.float32)

    geom = (dev(obj_off), dev(pair_off), dev(n, np.int32), int(n.max()))
    z, geo = _lib.pair_hidden1_fwd(dev(U), dev(V), dev(pos), dev(Wg), geom[0], geom[1], geom[2], geom[3], pairs)
    # the geometry features against float64 (the angle through its sine: asin is ill-conditioned at +-1) ...
    p64 = np.ascontiguousarray(pos).astype(np.float64)
    ps, po = p64[s_idx], p64[o_idx]
    dx = ps[:, 0] + ps[:, 2] / 2.0 - po[:, 0] - po[:, 2] / 2.0
    dy = ps[:, 1] + ps[:, 3] / 2.0 - po[:, 1] - po[:, 3] / 2.0
    dist = np.sqrt(dx * dx + dy * dy)
    g = geo.cpu().numpy().astype(np.float64)
    assert np.allclose(g[:, 0], dist, rtol=1e-5, atol=1e-6)
    # (dy is a float32 difference of coordinates of order 1: its rounding, 2e-7 at most, is divided by the distance)
    assert (np.abs(np.sin(g[:, 1]) - dy / np.maximum(dist, 1e-10)) <= 2e-6 + 2e-7 / np.maximum(dist, 1e-10)).all()
    assert np.array_equal(g[:, 2], np.sign(po[:, 0] - ps[:, 0])) and np.array_equal(g[:, 3], np.sign(po[:, 1] - ps[:, 1]))
    # ... and everything downstream of them against float64 autograd on the same geometry
    Ut, Vt, Wt = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (U, V, Wg))
    z_ref = torch.nn.functional.elu(Ut[s_idx] + Vt[o_idx] + torch.tensor(g) @ Wt.t())
    z_ref.backward(torch.tensor(gz.astype(np.float64)))
    z64, du64, dv64, dw64 = [t.detach().numpy() for t in (z_ref, Ut.grad, Vt.grad, Wt.grad)]
    assert np.allclose(z.cpu().numpy(), z64, rtol=2e-5, atol=2e-5)
    du, dv, dw = _lib.pair_hidden1_bwd(dev(gz), z, geo, geom[0], geom[1], geom[2], geom[3], O)
    for got, want, tag in ((du, du64, "dU"), (dv, dv64, "dV"), (dw, dw64, "dWg")):
        scale = max(1.0, np.abs(want).max())
        assert np.abs(got.cpu().numpy() - want).max() <= 5e-5 * scale, tag
    du2, dv2, dw2 = _lib.pair_hidden1_bwd(dev(gz), z, geo, geom[0], geom[1], geom[2], geom[3], O)
    assert torch.equal(du, du2) and torch.equal(dv, dv2) and torch.equal(dw, dw2)          # no atomics: bitwise repeatable
    # the form that rebuilds z from U, V, Wg instead of reading it, into the two halves of a joined [O, 2 HID1] buffer: the same bits
    # (same expression as the forward kernel, same order of the sums)
    UV = dev(np.concatenate([U, V], 1))
    uvw = (UV[:, :hid1], UV[:, hid1:], dev(Wg))
    assert _lib.hidden1_recompute(uvw, dev(gz), geom[3], hid1)
    duv, none, dw3 = _lib.pair_hidden1_bwd(dev(gz), None, geo, geom[0], geom[1], geom[2], geom[3], O, joined=True, uvw=uvw)
    assert none is None and torch.equal(duv[:, :hid1], du) and torch.equal(duv[:, hid1:], dv) and torch.equal(dw3, dw)

    # logit stage: two predicates on image 0 are not expressible (one contiguous row range per predicate), so one predicate per image
    P2 = rng.normal(size=(pairs, hid2)).astype(np.float32) * 2
    keep = [q for q in range(Q) if n_list[q] > 1]
    pred_off = np.concatenate([[pair_off[q] for q in keep], [pairs]]).astype(np.int64)
    E, be = rng.normal(size=(len(keep), hid2)).astype(np.float32) * 0.3, rng.normal(size=len(keep)).astype(np.float32)
    gx = rng.normal(size=pairs).astype(np.float32)
    rep = np.repeat(np.arange(len(keep)), np.diff(pred_off))
    Pt, Et, bt = (torch.tensor(a.astype(np.float64), requires_grad=True) for a in (P2, E, be))
    x64 = (torch.sigmoid(Pt) * Et[rep]).sum(1) + bt[rep]
    x64.backward(torch.tensor(gx.astype(np.float64)))
    x = _lib.pair_logit_fwd(dev(P2), dev(E), dev(be), dev(pred_off), int(np.diff(pred_off).max()))
    assert np.allclose(x.cpu().numpy(), x64.detach().numpy(), rtol=2e-5, atol=2e-5)
    dp2, de, dbe = _lib.pair_logit_bwd(dev(gx), dev(P2), dev(E), dev(pred_off))
    assert np.allclose(dp2.cpu().numpy(), Pt.grad.numpy(), rtol=2e-5, atol=2e-6)
    assert np.abs(de.cpu().numpy() - Et.grad.numpy()).max() <= 5e-5 * max(1.0, np.abs(Et.grad.numpy()).max())
    assert np.abs(dbe.cpu().numpy() - bt.grad.numpy()).max() <= 5e-5 * max(1.0, np.abs(bt.grad.numpy()).max())


# ---------------------------------------------------------------------------------------------------
# round 2: deterministic backward (no atomics), the TN weight-gradient kernel, the attribute-column backward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,ldx", [(1000, 300, 256, 256), (4097, 512, 2048, 2054), (333, 256, 516, 516), (70, 7, 5, 5), (25600, 300, 256, 256),
                                       (129, 320, 100, 100), (5000, 72, 260, 260), (17, 300, 256, 256),
                                       (3000, 128, 640, 640), (2000, 64, 128, 128), (40000, 44, 256, 256)])     # 5 blocks (a last group of one), one narrow block
@pytest.mark.parametrize("math", ["bf16x3", "f32"])
def test_linear_wgrad_against_fp64(M, N, K, ldx, math, monkeypatch):
    """dW = dY^T X (csrc/dfol_dense_wgrad.hip) against float64, strided X, odd sizes; two runs are bit-identical.  Both arithmetic
    routes: three-way bf16 operand split on the bf16 matrix pipe (the default where the rows are 16-byte aligned) and the fp32 matrix
    pipe (DFOL_WGRAD_MATH=f32, and every shape the first does not take).  Operands span six decades so the split's low pieces matter."""
    from dfol_vqa_amd import _lib
    monkeypatch.setenv("DFOL_WGRAD_MATH", math)
    g = torch.Generator(device=DEV).manual_seed(M + N)
    dy = torch.randn(M, N, device=DEV, generator=g) * torch.pow(10.0, torch.randint(-3, 4, (M, 1), device=DEV, generator=g).float())
    xw = torch.randn(M, ldx, device=DEV, generator=g) * torch.pow(10.0, torch.randint(-3, 4, (1, ldx), device=DEV, generator=g).float())
    x = xw[:, :K]
    a, db = _lib.linear_wgrad(dy, x, bias=True)
    b, db2 = _lib.linear_wgrad(dy, x, bias=True)
    assert torch.equal(a, b) and torch.equal(db, db2)
    assert torch.equal(a, _lib.linear_wgrad(dy, x))
    # bias gradient: column sums of dy (fp32 sums in a fixed order)
    err = ((db.double() - dy.double().sum(0)).abs() / dy.double().abs().sum(0)).max().item()
    assert err <= 2e-6, err
    ref = dy.double().t() @ x.double()
    scale = dy.double().abs().t() @ x.double().abs()                    # per element: X's column scales must not hide small columns
    rel = ((a.double() - ref).abs() / scale).max().item()
    assert rel <= 2e-6, rel
    # the library's fp32 product is no closer
    lib = (((dy.t() @ x).double() - ref).abs() / scale).max().item()
    assert rel <= 4 * lib + 1e-7, (rel, lib)


def test_reduce_by_question_and_prior_gradients_are_repeatable():
    """Several predicates per question: the prior gradients of filter / relate are sums over a question's predicates, taken in a fixed
    order (no atomics): equal to an fp64 sum and bit-identical across runs."""
    from dfol_vqa_amd import _lib
    rng = np.random.RandomState(3)
    n_list, k_list = [9, 30, 4, 17], [3, 1, 5, 2]
    Q = len(n_list)
    pq = np.repeat(np.arange(Q), k_list).astype(np.int32)
    P, NS = len(pq), 32
    src = rng.normal(size=(P, NS)).astype(np.float32)
    dev = lambda x: torch.tensor(x, device=DEV)
    out = _lib.reduce_by_question(dev(src), dev(pq), dev(np.array(n_list, np.int32)), Q).cpu().numpy()
    for q in range(Q):
        ref = src[pq == q].astype(np.float64).sum(0)
        ref[n_list[q]:] = 0
        assert np.allclose(out[q], ref, atol=1e-5)
    # relate backward twice: bit-identical prior and tile gradients
    prior_s = np.minimum(rng.normal(size=(Q, NS)).astype(np.float32) - 1, 0)
    prior_o = np.minimum(rng.normal(size=(Q, NS)).astype(np.float32) - 1, 0)
    tile = (-np.abs(rng.normal(size=(P, NS, NS))) * 2).astype(np.float32)
    quant = np.ones(P, np.float32)
    gs, go = rng.normal(size=(P, NS)).astype(np.float32), rng.normal(size=(P, NS)).astype(np.float32)
    runs = []
    for _ in range(3):
        r = _lib.relate_bwd(dev(prior_s), dev(prior_o), dev(tile), dev(pq), dev(np.array(n_list, np.int32)), dev(quant), dev(quant), None, None,
                            dev(gs), dev(go), 0, False)
        runs.append([t.cpu().numpy() for t in r])
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], r))


def test_backward_refuses_an_unsorted_predicate_map():
    """The deterministic backward finds a question's predicates by binary search in the predicate -> question map; an unsorted map would
    silently drop gradient contributions, so every backward entry refuses it (the atomic-add kernels it replaced accepted any order)."""
    from dfol_vqa_amd import _lib
    rng = np.random.RandomState(4)
    n_list = np.array([5, 7, 3], np.int32)
    Q, NS = 3, 8
    dev = lambda x: torch.tensor(x, device=DEV)
    for pq in (np.array([0, 2, 1, 1], np.int32), np.array([1, 0], np.int32)):
        P = len(pq)
        src, ll = rng.normal(size=(P, NS)).astype(np.float32), (-np.abs(rng.normal(size=(P, NS)))).astype(np.float32)
        with pytest.raises(_lib.DfolError, match="non-decreasing"):
            _lib.reduce_by_question(dev(src), dev(pq), dev(n_list), Q)
        with pytest.raises(_lib.DfolError, match="non-decreasing"):
            _lib.filter_bwd(dev(src), dev(ll), dev(pq), dev(n_list), None, None, Q)
        tile = (-np.abs(rng.normal(size=(P, NS, NS)))).astype(np.float32)
        pr = (-np.abs(rng.normal(size=(Q, NS)))).astype(np.float32)
        with pytest.raises(_lib.DfolError, match="non-decreasing"):
            _lib.relate_bwd(dev(pr), dev(pr), dev(tile), dev(pq), dev(n_list), dev(np.ones(P, np.float32)), dev(np.ones(P, np.float32)), None, None,
                            dev(src), dev(src), 0, False)
    # a sorted map with gaps and repeats is fine
    pq = np.array([0, 0, 2], np.int32)
    out = _lib.reduce_by_question(dev(rng.normal(size=(3, NS)).astype(np.float32)), dev(pq), dev(n_list), Q)
    assert out.shape == (Q, NS) and bool((out[1] == 0).all())


@pytest.mark.parametrize("n_list,k_list,H", [([5, 12, 1, 30], [2, 1, 3, 1], 300), ([100, 64], [1, 26], 300), ([7, 9], [1, 1], 44)])
def test_attr_ll_backward_against_autograd(n_list, k_list, H):
    """csrc/dfol_logic_bwd.hip attr_ll_bwd (needed-columns attribute likelihood) against float64 autograd of the formulation it
    replaces (row gathers, products, row sums, LogSigmoid): gradients w.r.t. the hidden activations, the embedding rows (repeated
    concepts included: rows of equal concept are combined in a fixed order) and the biases; a no-op (-1) column in the batch."""
    from dfol_vqa_amd.visual_oracle import _AttrLL, _concept_plan
    rng = np.random.RandomState(sum(n_list) + H)
    Q, C = len(n_list), 23
    pq = np.repeat(np.arange(Q), k_list).astype(np.int32)
    P = len(pq)
    NS = max(4, (max(n_list) + 3) // 4 * 4)
    O = sum(n_list)
    obj_off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int32)
    cols = rng.randint(0, C, P).astype(np.int32)
    if P > 2:
        cols[1] = -1
        cols[-1] = cols[0]                                   # a concept named by two predicates
    hidden = torch.tensor(rng.uniform(0, 1, (O, H)).astype(np.float32), device=DEV, requires_grad=True)
    E = torch.tensor((rng.normal(size=(C, H)) * 0.1).astype(np.float32), device=DEV, requires_grad=True)
    b = torch.tensor(rng.normal(size=C).astype(np.float32), device=DEV, requires_grad=True)
    g = torch.tensor(rng.normal(size=(P, NS)).astype(np.float32), device=DEV)
    plan = _concept_plan(cols, DEV, {})
    dev = lambda x: torch.tensor(x, device=DEV)
    outs = []
    for _ in range(2):
        for t in (hidden, E, b):
            t.grad = None
        ll = _AttrLL.apply(hidden, E, b, dev(obj_off), dev(pq), dev(cols), NS, plan)
        ll.backward(g)
        outs.append((ll.detach().clone(), hidden.grad.clone(), E.grad.clone(), b.grad.clone()))
    assert all(torch.equal(a, c) for a, c in zip(outs[0], outs[1]))            # repeatable bit for bit
    h64, E64, b64 = (t.detach().double().requires_grad_(True) for t in (hidden, E, b))
    ref = torch.full((P, NS), -30.0, dtype=torch.float64, device=DEV)
    rows = []
    for p in range(P):
        q, n = pq[p], n_list[pq[p]]
        if cols[p] < 0:
            continue
        x = h64[obj_off[q]:obj_off[q] + n] @ E64[cols[p]] + b64[cols[p]]
        rows.append((p, n, torch.nn.functional.logsigmoid(x)))
    loss = sum((r * g[p, :n].double()).sum() for p, n, r in rows)
    loss.backward()
    for p, n, r in rows:
        assert torch.allclose(outs[0][0][p, :n].double(), r.detach(), atol=2e-6)
    for got, want, name in ((outs[0][1], h64.grad, "d hidden"), (outs[0][2], E64.grad, "dE"), (outs[0][3], b64.grad, "db")):
        scale = want.abs().max().item() + 1e-30
        assert (got.double() - want).abs().max().item() <= 2e-5 * scale, name


def test_concept_rows_one_launch_equals_the_three_kernel_form():
    """dfol_concept_rows_f32 (per-predicate gradient rows of the embedding layer combined per concept, one launch) against gather_rows +
    segment_sum_rows + index_copy into a zeroed matrix, bit for bit; and the direct form - rows added straight into a persistent gradient -
    against the dense intermediate followed by autograd's add."""
    from dfol_vqa_amd import _lib, visual_oracle as VO
    rng = np.random.RandomState(8)
    for width, P, C in ((300, 768, 2335), (1, 768, 2335), (12, 5, 9)):
        cols = rng.randint(0, C, size=P)
        cols[rng.rand(P) < 0.1] = -1
        plan = VO._concept_plan(cols, torch.device(DEV), _lib.LRUCache(4))
        order, seg_off, ucols = plan
        rows = torch.tensor(rng.normal(size=(P, width)).astype(np.float32), device=DEV)
        shape = (C, width) if width > 1 else (C,)
        rr = rows if width > 1 else rows[:, 0].contiguous()
        old = torch.zeros(C, width, device=DEV)
        old.index_copy_(0, ucols, _lib.segment_sum_rows(_lib.gather_rows(rows, order), seg_off))
        new = VO._combine_concept_rows(rr, plan, shape)
        assert torch.equal(new.reshape(C, width), old)
        leaf = torch.nn.Parameter(torch.zeros(shape, device=DEV))
        leaf.grad = torch.tensor(rng.normal(size=shape).astype(np.float32), device=DEV)
        want = leaf.grad + old.reshape(shape)
        with VO.direct_grad():
            assert VO._combine_concept_rows(rr, plan, shape, leaf) is None
        assert torch.equal(leaf.grad, want)
        assert VO._combine_concept_rows(rr, plan, shape, leaf) is not None          # outside the context: a returned value


@pytest.mark.parametrize("capturable", [False, True])
def test_fused_clip_adam_equals_torch(capturable):
    """training.FusedClipAdam (csrc/dfol_optim.hip: the norm of the flat gradient bucket + one update pass, 2 - 3 launches) against
    nn.utils.clip_grad_norm_ + torch.optim.Adam.step() (trainer.py:439-441): parameters, both moments, the clipped gradients left behind, the
    step counters and the total norm over three steps - with gradients above and below the clip threshold, weight decay, a tensor shorter
    than a chunk and a bucket whose length is not a multiple of four.  The state lives in the torch optimizer object: a plain
    optimizer.step() afterwards continues from it."""
    from dfol_vqa_amd import parallel, training
    g = torch.Generator(device=DEV).manual_seed(5)
    shapes = [(300, 256), (300,), (512, 2048), (7,), (333, 300), (3,)]
    for wd, scale in ((0.0, 3.0), (1e-2, 1e-3)):
        ref = [torch.nn.Parameter(torch.randn(*s, device=DEV, generator=g)) for s in shapes]
        mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
        o_ref = torch.optim.Adam(ref, lr=1e-2, weight_decay=wd, capturable=capturable)
        o_mine = torch.optim.Adam(mine, lr=1e-2, weight_decay=wd, capturable=capturable)
        bucket = parallel.GradBucket(mine)
        fused = training.FusedClipAdam.make(o_mine, bucket)
        assert fused is not None and training.FusedClipAdam.make(torch.optim.AdamW(mine), bucket) is None
        for step in range(3):
            grads = [torch.randn(*s, device=DEV, generator=g) * scale * (step + 1) for s in shapes]
            bucket.zero_()
            for p, q, gr in zip(ref, mine, grads):
                p.grad = gr.clone()
                q.grad.copy_(gr)
            norm_ref = torch.nn.utils.clip_grad_norm_(ref, 0.65)
            o_ref.step()
            norm = fused.step(0.65)
            assert abs(float(norm) - float(norm_ref)) <= 1e-5 * float(norm_ref)
            for p, q in zip(ref, mine):
                close = lambda a, b, what: (a - b).abs().max().item() <= 2e-6 * max(1e-3, b.abs().max().item()) or pytest.fail("%s step %d" % (what, step))
                close(q.detach(), p.detach(), "parameter")
                close(q.grad, p.grad, "clipped gradient")
                close(o_mine.state[q]["exp_avg"], o_ref.state[p]["exp_avg"], "exp_avg")
                close(o_mine.state[q]["exp_avg_sq"], o_ref.state[p]["exp_avg_sq"], "exp_avg_sq")
                assert float(o_mine.state[q]["step"]) == float(o_ref.state[p]["step"]) == step + 1
                assert o_mine.state[q]["step"].device == o_ref.state[p]["step"].device
        for p, q in zip(ref, mine):                                  # torch's own step continues from the fused steps' state
            p.grad = torch.ones_like(p)
            q.grad.fill_(1.0)
        o_ref.step()
        o_mine.step()
        for p, q in zip(ref, mine):
            assert (q.detach() - p.detach()).abs().max().item() <= 5e-6 * max(1e-3, p.detach().abs().max().item())


def test_fused_clip_adam_edge_cases_follow_torch():
    """a NaN gradient norm poisons gradients and parameters as clip_grad_norm_'s NaN coefficient does (fminf would have dropped
    it and stepped on); clip_norm = 0 zeroes the gradients as the reference's call would (trainer.py:438), None means no clipping; and with
    per-parameter step counts that differ (a partial load_state_dict) the step goes to torch's own, whose bias corrections are per tensor."""
    from dfol_vqa_amd import parallel, training
    g = torch.Generator(device=DEV).manual_seed(9)
    shapes = [(64, 32), (32,), (5,)]

    def pair():
        ref = [torch.nn.Parameter(torch.randn(*s, device=DEV, generator=g)) for s in shapes]
        mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
        o_ref, o_mine = torch.optim.Adam(ref, lr=1e-2), torch.optim.Adam(mine, lr=1e-2)
        bucket = parallel.GradBucket(mine)
        return ref, mine, o_ref, o_mine, bucket, training.FusedClipAdam.make(o_mine, bucket)

    # NaN norm
    ref, mine, o_ref, o_mine, bucket, fused = pair()
    for p, q in zip(ref, mine):
        p.grad = torch.ones_like(p)
        q.grad.fill_(1.0)
    ref[1].grad[3] = float("nan")
    mine[1].grad[3] = float("nan")
    torch.nn.utils.clip_grad_norm_(ref, 0.65)
    o_ref.step()
    fused.step(0.65)
    for p, q in zip(ref, mine):
        assert bool(torch.isnan(p.detach()).all()) and bool(torch.isnan(q.detach()).all())
    # clip_norm = 0 and None
    for clip in (0.0, None):
        ref, mine, o_ref, o_mine, bucket, fused = pair()
        for p, q in zip(ref, mine):
            gr = torch.randn(*p.shape, device=DEV, generator=g)
            p.grad = gr.clone()
            q.grad.copy_(gr)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(ref, clip)
        o_ref.step()
        fused.step(clip)
        for p, q in zip(ref, mine):
            assert (q.detach() - p.detach()).abs().max().item() <= 2e-6 * max(1e-3, p.detach().abs().max().item()), clip
            assert (q.grad - p.grad).abs().max().item() <= 1e-6, clip
    # differing step counts
    ref, mine, o_ref, o_mine, bucket, fused = pair()
    for o, params in ((o_ref, ref), (o_mine, mine)):
        for i, p in enumerate(params):
            o.state[p]["step"] = torch.tensor(float(3 * i + 1))
            o.state[p]["exp_avg"] = torch.full_like(p, 0.1)
            o.state[p]["exp_avg_sq"] = torch.full_like(p, 0.2)
    for p, q in zip(ref, mine):
        gr = torch.randn(*p.shape, device=DEV, generator=g)
        p.grad = gr.clone()
        q.grad.copy_(gr)
    torch.nn.utils.clip_grad_norm_(ref, 0.65)
    o_ref.step()
    fused.step(0.65)
    for i, (p, q) in enumerate(zip(ref, mine)):
        assert torch.equal(q.detach(), p.detach()) and float(o_mine.state[q]["step"]) == 3 * i + 2


def test_train_step_is_bitwise_repeatable(ontology):
    """One train step (forward, loss, backward, clip, Adam) on the needed-columns dataflow, twice from the same state: identical
    loss, gradients and updated weights, bit for bit - the backward kernels sum in a fixed order instead of using atomics.
    (Hidden width 32: the widths the fused training kernels take, like the reference's 256; narrower relation networks fall back to
    tensor ops whose index_select backward is an atomic scatter-add.)"""
    from dfol_vqa_amd import experiment
    a, meta = gu.load("g12_weight_gradients")
    cfg = dict(meta["config"], attribute_network_layers_config=[32], relation_network_layers_config=[32])
    for name in sorted(meta["sets"]):
        qs = [{"program": q["program"], "answer": q["answer"], "question_id": q["question_id"], "image_id": "img000", "tokens": [],
               "original_dict": None, "question": None, "scene": {"n": q["n"], "X": a["%s:X_%d" % (name, i)]}}
              for i, q in enumerate(meta["sets"][name]["questions"])]
        runs = []
        for _ in range(2):
            torch.manual_seed(11)
            model = experiment.build_model(dict(cfg), ontology).to(DEV).train()
            assert model._oracle._fused_training is not None
            pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ontology, "X").collate([dict(q) for q in qs])]
            opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
            loss, _ = training.train_batch(model, opt, pbs, clip_norm=0.65)
            grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
            runs.append((loss, grads, {k: v.detach().clone() for k, v in model.state_dict().items()}))
        assert len(runs[0][1]) >= 12 and all(float(g.abs().sum()) > 0 for k, g in runs[0][1].items() if "embedding" in k)
        assert runs[0][0] == runs[1][0], name
        for k in runs[0][1]:
            assert torch.equal(runs[0][1][k], runs[1][1][k]), (name, k)
        for k in runs[0][2]:
            assert torch.equal(runs[0][2][k], runs[1][2][k]), (name, k)


# ---------------------------------------------------------------------------------------------------
# the bf16 mode (BASELINE configs[3] "bf16 fwd / fp32 logic", config key mlp_math): opt-in, never the default
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,act", [(700, 512, 2048, 2), (513, 300, 256, 1), (4000, 256, 300, 0), (130, 768, 516, 3)])
def test_bf16_mode_dense_kernels_are_bf16_operands_fp32_accumulation(M, N, K, act):
    """dense_math("bf16"): y = act(x W^T + b), dx = dz W and dW = dz^T x equal the fp64 products of the bf16-ROUNDED operands to fp32
    accumulation error - the definition of the mode - and differ from the fp32 results by bf16-sized errors (so the mode is really on)."""
    from dfol_vqa_amd import _lib
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    rb = lambda t: t.bfloat16().double()                                   # round to nearest even
    act_f = [lambda z: z, torch.sigmoid, torch.nn.functional.elu, torch.nn.functional.logsigmoid][act]
    with _lib.dense_math("bf16"):
        y = _lib.linear_act(x, w, b, act)
        dz = torch.randn(M, N, device=DEV, generator=g)
        dx = _lib.linear_gradx(dz, w)
        dw, db = _lib.linear_wgrad(dz, x, bias=True)
    y32 = _lib.linear_act(x, w, b, act)
    ref = act_f(rb(x) @ rb(w).t() + b.double())
    assert (y.double() - ref).abs().max().item() <= 2e-5
    assert (y - y32).abs().max().item() > 1e-4                             # not the fp32 path
    ref_dx = rb(dz) @ rb(w)
    assert (dx.double() - ref_dx).abs().max().item() <= 2e-6 * (rb(dz).abs() @ rb(w).abs()).max().item()
    ref_dw = rb(dz).t() @ rb(x)
    assert (dw.double() - ref_dw).abs().max().item() <= 2e-6 * (rb(dz).abs().t() @ rb(x).abs()).max().item()
    assert ((db.double() - dz.double().sum(0)).abs() / dz.double().abs().sum(0)).max().item() <= 2e-6      # the bias gradient stays fp32


@pytest.mark.parametrize("store,objects,batch", [("1", 24, 16), ("0", 24, 16), ("1", 6, 4)])
def test_bf16_mode_train_step_close_to_fp32_and_repeatable(store, objects, batch, monkeypatch):
    """A full-size model trains with `mlp_math: bf16` (experiment config key): the step's loss is within 1 % of the fp32 step's, every
    weight gradient points the same way (cosine > 0.99), two bf16 steps from the same state are bit-identical, and the default stays fp32.
    store = 1 (default): the per-pair activations and their gradients are STORED in bfloat16 too; 0: fp32 storage (DFOL_BF16_STORE=0)."""
    import importlib.util
    monkeypatch.setenv("DFOL_BF16_STORE", store)
    from dfol_vqa_amd import ops as dops                  # (visual_oracle calls the wrappers through this namespace)
    stores, real = [], dops.pair_hidden1_fwd
    monkeypatch.setattr(dops, "pair_hidden1_fwd", lambda *a, **k: (stores.append(a[9] if len(a) > 9 else k.get("store", torch.float32)), real(*a, **k))[1])
    real_fused = dops.pair_train_fwd_h2                   # (round 6: the fp32-storage forward is the fused pair kernel, which stores fp32)
    monkeypatch.setattr(dops, "pair_train_fwd_h2", lambda *a, **k: (stores.append(torch.float32), real_fused(*a, **k))[1])
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    runs = {}
    for math in ("fp32", "bf16", "bf16"):
        args = bench.parse(["--mode", "train", "--objects", str(objects), "--batch", str(batch), "--mlp-math", math])      # (6 objects x 4: 120 pair rows)
        torch.manual_seed(3)
        model, ontology, paths, names = bench.build_model(args, DEV, train=True)
        assert getattr(model, "_mlp_math", None) == ("bf16" if math == "bf16" else None)
        _, pbs = bench.build_batch(args, 0, ontology, names, DEV)
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
        loss, _ = training.train_batch(model, opt, pbs, clip_norm=0.65)
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        runs.setdefault(math, []).append((loss, grads))
    assert stores == [torch.float32] + [torch.bfloat16 if store == "1" else torch.float32] * 2, stores
    (l32, g32), (lb, gb), (lb2, gb2) = runs["fp32"][0], runs["bf16"][0], runs["bf16"][1]
    assert abs(lb - l32) <= 1e-2 * abs(l32), (lb, l32)
    assert lb != l32                                                        # the mode changes the arithmetic
    assert lb == lb2 and all(torch.equal(gb[k], gb2[k]) for k in gb)
    for k in g32:
        if float(g32[k].abs().max()) == 0:
            continue
        cos = torch.nn.functional.cosine_similarity(g32[k].flatten().double(), gb[k].flatten().double(), dim=0).item()
        assert cos > 0.99, (k, cos)


# bf16 STORAGE of the per-pair activations in the bf16 mode (Z, pre2 and their gradients): every kernel against its fp32-storage form
def _pair_geometry(Q, n_lo, n_hi, seed):
    rng = np.random.RandomState(seed)
    n = rng.randint(n_lo, n_hi + 1, Q).astype(np.int32)
    obj_off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32)
    cnt = n.astype(np.int64) * (n - 1)
    pair_off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    t = lambda a: torch.as_tensor(a).to(DEV)
    return n, t(n), t(obj_off), t(pair_off), int(n.sum()), int(cnt.sum()), cnt


@pytest.mark.parametrize("H1,H2", [(256, 300), (64, 32)])
def test_bf16_storage_stream_kernels_equal_fp32_storage_kernels_on_the_same_values(H1, H2):
    from dfol_vqa_amd import _lib
    BF = torch.bfloat16
    n, n_obj, obj_off, pair_off, O, pairs, cnt = _pair_geometry(9, 2, 23, 5)
    g = torch.Generator(device=DEV).manual_seed(11)
    U = torch.randn(O, H1, device=DEV, generator=g)
    V = torch.randn(O, H1, device=DEV, generator=g)
    pos = torch.rand(O, 4, device=DEV, generator=g)
    Wg = torch.randn(H1, 4, device=DEV, generator=g) * 0.3
    max_n = int(n.max())
    z32, geo32 = _lib.pair_hidden1_fwd(U, V, pos, Wg, obj_off, pair_off, n_obj, max_n, pairs)
    zb, geob = _lib.pair_hidden1_fwd(U, V, pos, Wg, obj_off, pair_off, n_obj, max_n, pairs, store=BF)
    assert zb.dtype == BF and torch.equal(zb, z32.to(BF)) and torch.equal(geob, geo32)          # the fp32 value, rounded to nearest even
    dzb = torch.randn(pairs, H1, device=DEV, generator=g).to(BF)
    got = _lib.pair_hidden1_bwd(dzb, zb, geob, obj_off, pair_off, n_obj, max_n, O)
    want = _lib.pair_hidden1_bwd(dzb.float(), zb.float(), geob, obj_off, pair_off, n_obj, max_n, O)
    for a, b in zip(got, want):
        assert torch.equal(a, b)                                                                # same fp32 arithmetic on the same values
    # one predicate per image, in order
    P = len(n)
    pred_off = torch.as_tensor(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)).to(DEV)
    p2b = (torch.randn(pairs, H2, device=DEV, generator=g) * 3).to(BF)
    E = torch.randn(P, H2, device=DEV, generator=g)
    be = torch.randn(P, device=DEV, generator=g)
    xb = _lib.pair_logit_fwd(p2b, E, be, pred_off, int(cnt.max()))
    x32 = _lib.pair_logit_fwd(p2b.float(), E, be, pred_off, int(cnt.max()))
    ref = (torch.sigmoid(p2b.double()) * E.double().repeat_interleave(torch.as_tensor(cnt).to(DEV), 0)).sum(1) + be.double().repeat_interleave(torch.as_tensor(cnt).to(DEV), 0)
    assert (xb.double() - ref).abs().max().item() <= 2 * (x32.double() - ref).abs().max().item() + 1e-6      # (another summation order)
    dx = torch.randn(pairs, device=DEV, generator=g)
    dpb, deb, dbb = _lib.pair_logit_bwd(dx, p2b, E, pred_off)
    dp32, de32, db32 = _lib.pair_logit_bwd(dx, p2b.float(), E, pred_off)
    assert dpb.dtype == BF and torch.equal(dpb, dp32.to(BF)) and torch.equal(deb, de32) and torch.equal(dbb, db32)


@pytest.mark.parametrize("M,N,K", [(9000, 300, 256), (5000, 256, 300), (4100, 128, 64), (130, 512, 516)])
def test_bf16_storage_dense_kernels_equal_the_bf16_mode_on_widened_operands(M, N, K):
    """bf16 in / bf16 out product == the bf16 mode's fp32-storage kernel on the same (exactly representable) operands, rounded to nearest
    even; the weight gradient from bf16-stored dY and X == the bf16 mode's on the widened operands, bit for bit (no rounding happens)."""
    from dfol_vqa_amd import _lib
    BF = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(M + N)
    xb = torch.randn(M, K, device=DEV, generator=g).to(BF)
    w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
    b = torch.randn(N, device=DEV, generator=g)
    for act in (0, 2):
        with _lib.dense_math("bf16"):
            yb = _lib.linear_act_split(xb, w, b, act)
            y32 = _lib.linear_act_split(xb.float(), w, b, act)
        assert yb.dtype == BF and torch.equal(yb, y32.to(BF))
    dyb = torch.randn(M, N, device=DEV, generator=g).to(BF)
    with _lib.dense_math("bf16"):
        gxb = _lib.linear_act_split(dyb, w, None, 0, transpose_w=True)
        gx32 = _lib.linear_act_split(dyb.float(), w, None, 0, transpose_w=True)
        dwb, dbb = _lib.linear_wgrad(dyb, xb, bias=True)
        dw32, db32 = _lib.linear_wgrad(dyb.float(), xb.float(), bias=True)
    assert torch.equal(gxb, gx32.to(BF))
    if N * K >= _lib.SPLIT_MIN_WEIGHT:                                      # (smaller layers: the fp32-storage weight gradient stays fp32 arithmetic)
        assert torch.equal(dwb, dw32) and torch.equal(dbb, db32)
    ref = dyb.double().t() @ xb.double()
    assert (dwb.double() - ref).abs().max().item() <= 2e-6 * (dyb.double().abs().t() @ xb.double().abs()).max().item()
    assert (dbb.double() - dyb.double().sum(0)).abs().max().item() <= 2e-6 * dyb.double().abs().sum(0).max().item()
    with pytest.raises(Exception):
        _lib.linear_act_split(xb, w, b, 0)                                 # bf16-stored input outside the bf16 mode: refused


@pytest.mark.parametrize("store", [torch.float32, torch.bfloat16])
def test_pair_hidden1_kernels_with_one_object_images(store):
    """Images of ONE object have no pair rows (also as the last image of the batch, where their pair offset is the end of the arrays):
    hidden1_fwd / _bwd against torch autograd through the same formula."""
    from dfol_vqa_amd import _lib
    H1 = 256
    n = np.array([3, 1, 7, 2, 1], np.int32)
    t = lambda a: torch.as_tensor(a).to(DEV)
    obj_off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32)
    cnt = n.astype(np.int64) * (n - 1)
    pair_off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    O, pairs = int(n.sum()), int(cnt.sum())
    g = torch.Generator(device=DEV).manual_seed(2)
    U = torch.randn(O, H1, device=DEV, generator=g, requires_grad=True)
    V = torch.randn(O, H1, device=DEV, generator=g, requires_grad=True)
    pos = torch.rand(O, 4, device=DEV, generator=g)
    Wg = (torch.randn(H1, 4, device=DEV, generator=g) * 0.3).requires_grad_(True)
    z, geo = _lib.pair_hidden1_fwd(U.detach(), V.detach(), pos, Wg.detach(), t(obj_off), t(pair_off), t(n), int(n.max()), pairs, store=store)
    s_idx = np.concatenate([obj_off[q] + np.repeat(np.arange(n[q]), n[q] - 1) for q in range(len(n))]).astype(np.int64)
    o_idx = np.concatenate([obj_off[q] + np.array([o for s in range(n[q]) for o in range(n[q]) if o != s], np.int64) for q in range(len(n))]).astype(np.int64)
    ref = torch.nn.functional.elu(U[t(s_idx)] + V[t(o_idx)] + geo @ Wg.t())
    tol = 1e-5 if store == torch.float32 else 2e-2
    assert z.shape == (pairs, H1) and (z.float() - ref).abs().max().item() <= tol
    dz = torch.randn(pairs, H1, device=DEV, generator=g).to(store)
    du, dv, dwg = _lib.pair_hidden1_bwd(dz, z, geo, t(obj_off), t(pair_off), t(n), int(n.max()), O)
    # the kernel differentiates through the STORED z (ELU' from z): build the same reference
    zf = z.float()
    dpre = dz.float() * torch.where(zf > 0, torch.ones_like(zf), zf + 1)
    du_ref = torch.zeros(O, H1, device=DEV).index_add_(0, t(s_idx), dpre)
    dv_ref = torch.zeros(O, H1, device=DEV).index_add_(0, t(o_idx), dpre)
    assert (du - du_ref).abs().max().item() <= 1e-4 and (dv - dv_ref).abs().max().item() <= 1e-4
    assert (dwg - dpre.t() @ geo).abs().max().item() <= 1e-3
    assert du[obj_off[1]].abs().max().item() == 0 and dv[obj_off[4]].abs().max().item() == 0        # the one-object images get zero rows


@pytest.mark.parametrize("math", ["fp32", "bf16"])
def test_graphed_train_step_full_size_model_equals_eager_bit_for_bit(math):
    """The full-size model (every large product on this library's kernels, nothing through the vendor BLAS): three graphed steps ==
    three eager steps, losses and every parameter BIT FOR BIT - in fp32 mode and in the bf16 mode with bf16-stored activations."""
    import importlib.util
    from dfol_vqa_amd import parallel
    spec = importlib.util.spec_from_file_location("bench_for_test2", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    finals = []
    for graphed in (False, True):
        args = bench.parse(["--mode", "train", "--objects", "20", "--batch", "12", "--mlp-math", math])
        torch.manual_seed(5)
        model, ontology, paths, names = bench.build_model(args, DEV, train=True)
        _, pbs = bench.build_batch(args, 0, ontology, names, DEV)
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        bucket = parallel.GradBucket(params)
        if graphed:
            step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=1)
            losses = [float(step()[0]) for _ in range(3)]
        else:
            losses = [float(training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)[0]) for _ in range(4)][1:]
        finals.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    (l0, s0), (l1, s1) = finals
    assert l0 == l1, (l0, l1)
    bad = [k for k in s0 if not torch.equal(s0[k], s1[k])]
    assert not bad, bad
    assert l0[-1] != l0[0]


def test_evaluation_between_graph_replays_sees_current_weights():
    """The trainer's train-then-validate loop (trainer.py:429-442 then :685-720) with a replayed step graph: a replay rewrites the
    parameters on the device, so every version-keyed packed-weight cache (split images of the dense layers, the pair kernel's W2 image,
    the calibrator's transposed weights) must miss afterwards.  replay, eval, replay x2, eval == the same sequence with eager steps, bit
    for bit - the second evaluation would run on the first one's stale images if a replay did not bump the versions."""
    import importlib.util
    from dfol_vqa_amd import parallel
    spec = importlib.util.spec_from_file_location("bench_for_test4", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    with pytest.raises(ValueError):
        training.GraphedTrainStep(None, torch.optim.Adam([torch.zeros(1, device=DEV, requires_grad=True)], capturable=True), [], 0.65, warmup=0)
    runs = []
    for graphed in (False, True):
        args = bench.parse(["--mode", "train", "--objects", "20", "--batch", "12"])
        torch.manual_seed(9)
        model, ontology, paths, names = bench.build_model(args, DEV, train=True)
        _, pbs = bench.build_batch(args, 0, ontology, names, DEV)
        eargs = bench.parse(["--objects", "20", "--batch", "12"])
        _, ev = bench.build_batch(eargs, 3, ontology, names, DEV)              # other questions for the evaluation
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-2, capturable=True)
        bucket = parallel.GradBucket(params)
        if graphed:
            step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=1)
        else:
            training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)
            step = lambda: training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)

        def evaluate():
            model.eval()
            with torch.no_grad():
                lp = model(ev, False)["log_probability"].detach().clone()
            model.train()
            return lp
        seq = []
        step()
        seq.append(evaluate())
        step()
        step()
        seq.append(evaluate())
        runs.append(seq)
    (e0, e1), (g0, g1) = runs
    assert not torch.equal(e0, e1)                               # lr 1e-2: the weights moved between the two evaluations
    assert torch.equal(e0, g0), (e0 - g0).abs().max().item()
    assert torch.equal(e1, g1), (e1 - g1).abs().max().item()


def test_train_step_on_shared_scenes_equals_per_question_scenes():
    """A batch collated with share_scenes=True (every image once, eight questions per image) TRAINS through the reference's layout - the
    interpreter expands the scenes to one copy per question when gradients have to reach the oracle (build_scene) - so its loss and every
    gradient equal, bit for bit, those of the same questions collated with a scene copy each."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_test3", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    runs = []
    for share in ("1", "0"):
        args = bench.parse(["--mode", "train", "--objects", "20", "--ragged", "6", "--batch", "16", "--questions-per-image", "4", "--share-scenes", share])
        torch.manual_seed(7)
        model, ontology, paths, names = bench.build_model(args, DEV, train=True)
        _, pbs = bench.build_batch(args, 0, ontology, names, DEV)
        assert (pbs[0]._question_image is not None) == (share == "1")
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
        loss, _ = training.train_batch(model, opt, pbs, clip_norm=0.65)
        runs.append((loss, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}))
    (l1, g1), (l0, g0) = runs
    assert l1 == l0, (l1, l0)
    assert sorted(g1) == sorted(g0) and all(torch.equal(g1[k], g0[k]) for k in g1)


# ---------------------------------------------------------------------------------------------------
# round 4: the pair MLP head's backward without dpre2 in memory (dfol_pair_logit_bwd_sums_f32, dfol_pair_dz_fused_f32,
# dfol_pair_wgrad_fused_f32)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts,hid1,hid2,decades", [([90, 2, 6, 0, 132, 380, 30, 1], 256, 300, 0),        # tiny and empty predicates, M % 32 != 0
                                                      ([9900, 5112, 3540], 256, 300, 4),                    # several slabs, dx over eight decades
                                                      ([700, 650], 64, 128, 2),                             # four columns per building thread (HID2 % 3 != 0)
                                                      ([2450] * 9, 256, 300, 1),
                                                      ([64, 0, 71, 9900, 65, 0, 0, 1560, 97, 64 * 3 + 5], 256, 300, 2),     # boundaries in every position, empty predicates between
                                                      ([1260] * 37 + [380, 0, 3906], 256, 300, 1)])
def test_pair_head_backward_without_dpre2(counts, hid1, hid2, decades):
    """(dZ, dW2, db2, dE, dbe) of x = sum_j Sigmoid(Z W2^T + b2)[r, j] E[p(r), j] + be[p(r)] from the three kernels that rebuild dpre2 on
    the fly, against float64 from the materialised dpre2, with the tolerance of the operand model the kernels document: dpre2 and Z as
    two fp16 pieces (2^-22 relative per operand), the underflow floor of the row resp. launch scale, fp32 accumulation.  Two runs are
    bit-identical; a second use accumulates into dZ."""
    from dfol_vqa_amd import _lib
    rng = np.random.RandomState(len(counts) * 1000 + hid2)
    counts = np.asarray(counts, np.int64)
    M, P = int(counts.sum()), len(counts)
    pred_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rep = np.repeat(np.arange(P), counts).astype(np.int32)
    p2 = (rng.normal(size=(M, hid2)) * 2.5).astype(np.float32)
    z = np.where(rng.uniform(size=(M, hid1)) < 0.5, rng.uniform(-1, 0, (M, hid1)), rng.uniform(0, 6, (M, hid1))).astype(np.float32)      # ELU outputs
    w2 = (rng.normal(size=(hid2, hid1)) / 16).astype(np.float32)
    E = (rng.normal(size=(P, hid2)) * 0.1).astype(np.float32)
    dx = (rng.normal(size=M) * 10.0 ** rng.randint(-decades, decades + 1, M)).astype(np.float32)
    dx[rng.uniform(size=M) < 0.1] = 0.0
    dev = lambda a: torch.as_tensor(a).to(DEV)
    w2_t = dev(w2)
    args = (dev(dx), dev(p2), dev(z), w2_t, dev(E), dev(pred_off), dev(rep))
    dz, dw, db2, de, dbe = _lib.pair_head_bwd(*args)
    again = _lib.pair_head_bwd(*args)
    for a, b in zip((dz, dw, db2, de, dbe), again):
        assert torch.equal(a, b)
    # float64 from the same formulas
    p64, z64, w64, E64, g64 = (a.astype(np.float64) for a in (p2, z, w2, E, dx))
    h = 1.0 / (1.0 + np.exp(-p64))
    dp = g64[:, None] * E64[rep] * h * (1.0 - h)
    emax = np.abs(E64).max(1)
    bound = np.abs(g64) * emax[rep] * 0.25
    # dZ: rows scaled by their own bound
    want = dp @ w64
    tol = 2.0 ** -20 * (np.abs(dp) @ np.abs(w64)) + hid2 * 2.0 ** -37 * bound[:, None] * np.abs(w64).max() + 1e-30
    err = np.abs(dz.cpu().numpy() - want)
    assert (err <= tol).all(), ("dZ", float((err / tol).max()))
    # dW2: one scale for the launch
    want = dp.T @ z64
    tol = 2.0 ** -20 * (np.abs(dp).T @ np.abs(z64)) + 2.0 ** -37 * bound.max() * np.abs(z64).sum(0)[None, :] + 1e-30
    err = np.abs(dw.cpu().numpy() - want)
    assert (err <= tol).all(), ("dW2", float((err / tol).max()))
    for got, want, mag, tag in ((db2, dp.sum(0), np.abs(dp).sum(0), "db2"),
                                (de, np.add.reduceat(np.concatenate([g64[:, None] * h, np.zeros((1, hid2))]), np.minimum(pred_off[:-1], M), 0) * (counts > 0)[:, None],
                                 np.add.reduceat(np.concatenate([np.abs(g64[:, None] * h), np.zeros((1, hid2))]), np.minimum(pred_off[:-1], M), 0), "dE"),
                                (dbe, np.add.reduceat(np.concatenate([g64, [0.0]]), np.minimum(pred_off[:-1], M)) * (counts > 0),
                                 np.add.reduceat(np.concatenate([np.abs(g64), [0.0]]), np.minimum(pred_off[:-1], M)), "dbe")):
        err = np.abs(got.cpu().numpy() - want)
        assert (err <= 2e-6 * mag + 1e-30).all(), (tag, float(err.max()))
    # the sums from the weight-gradient pass (no pass of their own over pre2) where every predicate owns >= 64 rows or none
    if (counts[counts > 0] >= 64).all() and hid2 % 3 == 0:
        fz, fw, fb2, fe, fbe = _lib.pair_head_bwd(*args, sums=True)
        assert torch.equal(fz, dz)
        assert torch.equal(_lib.pair_head_bwd(*args, sums=True)[1], fw)
        for got, ref, mag, tag in ((fb2, dp.sum(0), np.abs(dp).sum(0), "db2"), (fe, de.cpu().numpy().astype(np.float64), None, "dE"), (fbe, dbe.cpu().numpy().astype(np.float64), None, "dbe")):
            m = np.abs(ref).max() if mag is None else mag
            err = np.abs(got.cpu().numpy() - ref)
            assert (err <= 4e-6 * m + 1e-30).all(), (tag + " (fused sums)", float(err.max()), float(np.max(m)))
        errw = np.abs(fw.cpu().numpy() - dw.cpu().numpy())
        assert float(errw.max()) <= 1e-6 * float(dw.abs().max()), "dW2 (fused sums)"
    # a second use of the hidden layer adds its input gradient
    dz2 = _lib.pair_head_bwd(*args, dz_out=dz.clone())[0]
    assert np.allclose(dz2.cpu().numpy(), 2.0 * dz.cpu().numpy(), rtol=1e-6, atol=0.0)
    # the materialised route (dfol_pair_logit_bwd_f32 -> bf16x3 products) agrees to the same tolerance class
    dp_dev, de_m, dbe_m = _lib.pair_logit_bwd(args[0], args[1], args[4], args[5])
    assert torch.equal(de_m, de) and torch.equal(dbe_m, dbe)
    assert np.allclose(dp_dev.cpu().numpy(), dp, rtol=2e-5, atol=1e-30 + 2e-6 * np.abs(dp).max())


@pytest.mark.parametrize("counts,nr,decades", [([9900, 5112, 3540], 2, 2), ([2450] * 9, 3, 1), ([1260] * 37 + [380, 0, 3906], 4, 3), ([870] * 30, 6, 1)])
def test_pair_dz_of_several_readers_in_one_pass(counts, nr, decades):
    """dfol_pair_dz_tall_multi_f32: dZ = (h (1 - h) sum_k dx_k E_k[p(r)]) W2 for nr readers of one hidden layer in ONE pass over pre2, against float64
    with the single-reader kernel's operand-model tolerance (the row's scale is that of the bound sum_k |dx_k| max|E_k|), against the sum of the
    readers' single passes, bit-repeatable, adding into a previous dZ; more than four readers go in two launches."""
    from dfol_vqa_amd import _lib
    hid1, hid2 = 256, 300
    rng = np.random.RandomState(len(counts) * 100 + nr)
    counts = np.asarray(counts, np.int64)
    M, P = int(counts.sum()), len(counts)
    assert _lib.linear_tall_supported(M, hid1, hid2)
    rep = np.repeat(np.arange(P), counts).astype(np.int32)
    p2 = (rng.normal(size=(M, hid2)) * 2.5).astype(np.float32)
    w2 = (rng.normal(size=(hid2, hid1)) / 16).astype(np.float32)
    Es = [(rng.normal(size=(P, hid2)) * 0.1 * 3.0 ** k).astype(np.float32) for k in range(nr)]
    dxs = []
    for k in range(nr):
        dx = (rng.normal(size=M) * 10.0 ** rng.randint(-decades, decades + 1, M)).astype(np.float32)
        dx[rng.uniform(size=M) < 0.3] = 0.0                       # (a reader's idle rows carry no gradient)
        dxs.append(dx)
    dev = lambda a: torch.as_tensor(a).to(DEV)
    p2_t, w2_t, rep_t = dev(p2), dev(w2), dev(rep)
    dz = _lib.pair_dz_tall_multi([dev(d) for d in dxs], p2_t, [dev(e) for e in Es], rep_t, w2_t)
    assert torch.equal(dz, _lib.pair_dz_tall_multi([dev(d) for d in dxs], p2_t, [dev(e) for e in Es], rep_t, w2_t))
    p64, w64 = p2.astype(np.float64), w2.astype(np.float64)
    h = 1.0 / (1.0 + np.exp(-p64))
    coef = sum(d.astype(np.float64)[:, None] * e.astype(np.float64)[rep] for d, e in zip(dxs, Es))
    dp = coef * h * (1.0 - h)
    groups = [range(i, min(i + _lib.PAIR_DZ_MULTI_MAX, nr)) for i in range(0, nr, _lib.PAIR_DZ_MULTI_MAX)]     # (one row scale per launch)
    tol = np.zeros((M, hid1))
    for grp in groups:
        dpg = sum(dxs[k].astype(np.float64)[:, None] * Es[k].astype(np.float64)[rep] for k in grp) * h * (1.0 - h)
        bound = sum(np.abs(dxs[k].astype(np.float64)) * np.abs(Es[k].astype(np.float64)).max(1)[rep] for k in grp) * 0.25
        absdp = sum(np.abs(dxs[k].astype(np.float64))[:, None] * np.abs(Es[k].astype(np.float64))[rep] for k in grp) * h * (1.0 - h)
        tol += 2.0 ** -20 * (absdp @ np.abs(w64)) + hid2 * 2.0 ** -37 * bound[:, None] * np.abs(w64).max() + 1e-30
    err = np.abs(dz.cpu().numpy() - dp @ w64)
    assert (err <= tol).all(), float((err / tol).max())
    # the readers one by one (each a pass of its own, adding into dZ): the same numbers to the kernels' tolerance
    z0 = torch.zeros(M, hid1, device=DEV)
    one = None
    for d, e in zip(dxs, Es):
        one, _ = _lib.pair_head_products(dev(d), p2_t, z0, w2_t, dev(e), None, rep_t, True, False, dz_out=one)
    assert (np.abs(one.cpu().numpy() - dz.cpu().numpy()) <= 2 * tol).all()
    # adding into an earlier dZ
    twice = _lib.pair_dz_tall_multi([dev(d) for d in dxs], p2_t, [dev(e) for e in Es], rep_t, w2_t, dz_out=dz.clone())
    assert np.allclose(twice.cpu().numpy(), 2.0 * dz.cpu().numpy(), rtol=1e-6, atol=2e-6 * float(dz.abs().max()))


@pytest.mark.parametrize("M,N,K", [(9900 * 3 + 77, 300, 256), (1000, 300, 256), (70000, 256, 64), (129, 44, 32)])
def test_linear_logit_h2_partial_sums(M, N, K):
    """dfol_linear_logit_h2_f32: the product is bit for bit dfol_linear_act_h2_f32's, and the partial sums its epilogue leaves add up to the
    logit layer's forward (dfol_pair_logit_fwd_f32 on the stored product) - interior tiles (staged stores), edge rows, the narrow last
    column block, 64-row blocks, rows without a predicate."""
    from dfol_vqa_amd import _lib
    g = torch.Generator(device=DEV).manual_seed(M + N)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / 8
    b = torch.randn(N, device=DEV, generator=g)
    P = 7
    E = torch.randn(P, N, device=DEV, generator=g) * 0.3
    cnt = np.full(P, M // P, np.int64)
    cnt[-1] += M - cnt.sum()
    rep = torch.as_tensor(np.repeat(np.arange(P), cnt).astype(np.int32)).to(DEV)
    pred_off = torch.as_tensor(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)).to(DEV)
    with _lib.dense_math("f16x2"):
        y_ref = _lib.linear_act_split(x, w, b, _lib.ACT_NONE)
        y, xp = _lib.linear_logit_h2(x, w, b, rep, E)
    assert torch.equal(y, y_ref)
    want = _lib.pair_logit_fwd(y_ref, E, None, pred_off, int(cnt.max()))
    got = xp.sum(0)
    h = torch.sigmoid(y_ref.double())
    exact = (h * E.double()[rep.long()]).sum(1)
    mag = (h * E.double()[rep.long()].abs()).sum(1)
    assert ((got.double() - exact).abs() <= 4e-6 * mag + 1e-7).all() and ((want.double() - exact).abs() <= 4e-6 * mag + 1e-7).all()
    # rows without a predicate (a leading run: the map is non-decreasing) add nothing
    rep2 = rep.clone()
    lead = min(200, M // 2)
    rep2[:lead] = -1
    with _lib.dense_math("f16x2"):
        _, xp2 = _lib.linear_logit_h2(x, w, b, rep2, E)
    got2 = xp2.sum(0)
    assert torch.equal(got2[lead:], got[lead:]) and float(got2[:lead].abs().max()) == 0.0


@pytest.mark.parametrize("kinds,n_lo,n_hi,count", [(("exist", "verify_rel"), 18, 30, 8), (("choose_rel", "query_attr"), 18, 30, 8),
                                                    (("exist", "verify_rel"), 2, 34, 12),       # images of 2 .. 8 objects: predicates of 2 .. 56 rows
                                                    (("exist", "verify_rel"), 34, 44, 8)])      # > 16384 pair rows: the persistent products
def test_deferred_head_backward_equals_the_materialised_one(kinds, n_lo, n_hi, count, monkeypatch):
    """The full-size model on ragged scenes with programs of one to three relation hops (several readers of one hidden layer: the deferred
    trunk adds their input and weight gradients), relation option lists and no-op tokens (readers that cannot register with the trunk and
    fall back to a second, ordinary evaluation): loss and every parameter gradient with the head's backward rebuilt on the fly
    (`_PairTrunk` / `_HeadUse`) against the materialised route (DFOL_TRAIN_HEAD_FUSED=0: dpre2 in memory, bf16x3 products)."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("bench_for_test5", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    args = bench.parse(["--mode", "train", "--objects", "24", "--batch", "16"])
    runs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("DFOL_TRAIN_HEAD_FUSED", fused)
        monkeypatch.setenv("DFOL_HEAD_SUMS", "1")             # the sums from the weight-gradient pass wherever every predicate is large enough
        torch.manual_seed(3)
        model, ontology, paths, names = bench.build_model(args, DEV, train=True)
        with open(paths["attribute_file"]) as f:
            categories = json.load(f)
        qs = []
        for j, kind in enumerate(kinds):
            qs += syn.full_size_questions(kind, count, n_lo, n_hi, names, categories, 40 + j)
        if "choose_rel" in kinds:
            qs[0]["program"]["last_op"]["arguments"][0][1] = "_"       # a no-op token inside an option list
        pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ontology, "X").collate([dict(q) for q in qs])]
        res = model(pbs, True)
        loss = training.compute_loss(pbs, res) / len(qs)
        loss.backward()
        runs.append((float(loss.detach()), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}))
    (l1, g1), (l0, g0) = runs
    assert abs(l1 - l0) <= 1e-6 * max(1.0, abs(l0)), (l1, l0)
    seen = 0
    for k in g0:
        if g0[k] is None:
            assert g1[k] is None, k
            continue
        scale = float(g0[k].abs().max())
        assert float((g1[k] - g0[k]).abs().max()) <= 3e-5 * scale + 1e-12, (k, float((g1[k] - g0[k]).abs().max()), scale)
        seen += scale > 0
    assert seen >= 8


@pytest.mark.parametrize("M,N,K", [(16384 + 77, 300, 256), (9900 * 4, 256, 300), (40000, 200, 100), (128 * 300 + 5, 320, 128)])
def test_tall_products_equal_the_tiled_kernels_bit_for_bit(M, N, K, monkeypatch):
    """csrc/dfol_dense_tall.hip (one persistent workgroup per CU over 128-row blocks and all columns) against csrc/dfol_dense_split.hip
    (128 x 128 tiles) on the same operands: the forward product with and without the logit partial sums, and the input-gradient product
    with dpre2 produced in the kernel, plain and accumulating - bit for bit (same pieces, same order of the products)."""
    from dfol_vqa_amd import _lib
    g = torch.Generator(device=DEV).manual_seed(M + N)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / 8
    b = torch.randn(N, device=DEV, generator=g)
    P = 5
    E = torch.randn(P, N, device=DEV, generator=g) * 0.3
    cnt = np.full(P, M // P, np.int64)
    cnt[-1] += M - cnt.sum()
    rep = torch.as_tensor(np.repeat(np.arange(P), cnt).astype(np.int32)).to(DEV)
    pred_off = torch.as_tensor(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)).to(DEV)
    assert _lib.linear_tall_supported(M, N, K)
    with _lib.dense_math("f16x2"):
        y_ref = _lib.linear_act_split(x, w, b, _lib.ACT_NONE)
        y, none = _lib.linear_tall_h2(x, w, b)
        y2, xp = _lib.linear_tall_h2(x, w, b, rep, E)
    assert none is None and torch.equal(y, y_ref) and torch.equal(y2, y_ref)
    want = _lib.pair_logit_fwd(y_ref, E, None, pred_off, int(cnt.max()))
    h = torch.sigmoid(y_ref.double())
    exact = (h * E.double()[rep.long()]).sum(1)
    mag = (h * E.double()[rep.long()].abs()).sum(1)
    assert ((xp.sum(0).double() - exact).abs() <= 4e-6 * mag + 1e-7).all() and ((want.double() - exact).abs() <= 4e-6 * mag + 1e-7).all()
    # the input-gradient product: here x plays pre2 [M, K = HID2], the result is [M, N = HID1].  The cases of 300 and 320 columns are left out:
    # the head's backward is only built for HID1 <= 256 (_lib.pair_head_fused_supported, the weight-gradient kernel's limit), so no caller
    # reaches a dZ product that wide; the two cases of 256 and 200 columns run it.
    if N <= 256:
        Ek = torch.randn(P, K, device=DEV, generator=g) * 0.3
        dx = torch.randn(M, device=DEV, generator=g) * torch.pow(10.0, torch.randint(-3, 4, (M,), device=DEV, generator=g).float())
        wt = torch.randn(K, N, device=DEV, generator=g) / 8                                # W2 [HID2, HID1]
        zz = torch.randn(M, N, device=DEV, generator=g)
        outs = []
        for tall in ("1", "0"):
            monkeypatch.setenv("DFOL_TALL", tall)
            dz, _ = _lib.pair_head_products(dx, x, zz, wt, Ek, pred_off, rep, need_dw=False)
            dz2, _ = _lib.pair_head_products(dx, x, zz, wt, Ek, pred_off, rep, need_dw=False, dz_out=dz.clone())
            outs.append((dz, dz2))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("N", [300, 256])
def test_tall_logit_partial_sums_across_predicate_boundaries(N):
    """The forward product's logit epilogue on 128-row blocks that lie inside one predicate, across ONE boundary (two embedding rows staged
    in LDS), across several (predicates of fewer than 128 rows: read element by element), with predicates that own no row and rows that
    have no predicate (-1): the partial sums against float64, the product itself bit for bit the tiled kernel's."""
    from dfol_vqa_amd import _lib
    K = 256
    g = torch.Generator(device=DEV).manual_seed(N)
    counts = [1260] * 6 + [0, 50, 3, 200, 0, 0, 130, 127, 129, 1, 1, 1, 2450] + [1260] * 5 + [90]
    lead = 70                                                # rows without a predicate first (row_pred is non-decreasing)
    M = lead + sum(counts)
    assert _lib.linear_tall_supported(M, N, K)
    rep_h = np.concatenate([np.full(lead, -1), np.repeat(np.arange(len(counts)), counts)]).astype(np.int32)
    rep = torch.as_tensor(rep_h).to(DEV)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / 8
    b = torch.randn(N, device=DEV, generator=g)
    E = torch.randn(len(counts), N, device=DEV, generator=g) * 0.3
    with _lib.dense_math("f16x2"):
        y_ref = _lib.linear_act_split(x, w, b, _lib.ACT_NONE)
        y, xp = _lib.linear_tall_h2(x, w, b, rep, E)
    assert torch.equal(y, y_ref)
    h = torch.sigmoid(y_ref.double())
    rows = E.double()[rep.clamp(min=0).long()] * (rep >= 0).double()[:, None]
    exact, mag = (h * rows).sum(1), (h * rows.abs()).sum(1)
    got = xp.sum(0).double()
    assert ((got - exact).abs() <= 4e-6 * mag + 1e-7).all()
    assert (got[:lead] == 0).all()
    y2, xp2 = _lib.linear_tall_h2(x, w, b, rep, E)
    assert torch.equal(xp, xp2)                              # repeatable bit for bit


@pytest.mark.parametrize("M,N,K", [(16384 + 77, 300, 256), (9900 * 4, 256, 300)])
def test_tall_products_bf16_storage_equal_the_tiled_bf16_kernels_bit_for_bit(M, N, K, monkeypatch):
    """The bf16 mode's persistent products (bf16-stored activations, one bf16 piece per operand) against the tiled bf16-storage kernel:
    the forward product bit for bit, its logit partial sums against dfol_pair_logit_fwd_bf16 on the stored product, and the input gradient
    with dpre2 produced in the kernel bit for bit dfol_pair_logit_bwd_bf16 -> dfol_linear_act_bf16_bf16 (plain and accumulating).
    The references are taken under DFOL_TALL=0: with the persistent form enabled _lib.linear_act_split forwards these very shapes to
    dfol_linear_tall_bf16_bf16, and the test compared the kernel with itself.  Which entry points ran is asserted on both sides."""
    from dfol_vqa_amd import _lib
    from test_tall_shapes_gpu import _kernels
    g = torch.Generator(device=DEV).manual_seed(M + N)
    x = (torch.randn(M, K, device=DEV, generator=g)).to(torch.bfloat16)
    w = torch.randn(N, K, device=DEV, generator=g) / 8
    b = torch.randn(N, device=DEV, generator=g)
    P = 5
    E = torch.randn(P, N, device=DEV, generator=g) * 0.3
    cnt = np.full(P, M // P, np.int64)
    cnt[-1] += M - cnt.sum()
    rep = torch.as_tensor(np.repeat(np.arange(P), cnt).astype(np.int32)).to(DEV)
    pred_off = torch.as_tensor(np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)).to(DEV)
    with _lib.dense_math("bf16"):
        with _kernels(monkeypatch, "0", ["dfol_linear_act_bf16_bf16"]):
            y_ref = _lib.linear_act_split(x, w, b, _lib.ACT_NONE)
        with _kernels(monkeypatch, "1", ["dfol_linear_tall_bf16_bf16"]):
            y, none = _lib.linear_tall_h2(x, w, b)
            y2, xp = _lib.linear_tall_h2(x, w, b, rep, E)
        assert y_ref.dtype == torch.bfloat16 and none is None and torch.equal(y, y_ref) and torch.equal(y2, y_ref)
        want = _lib.pair_logit_fwd(y_ref, E, None, pred_off, int(cnt.max()))
        assert torch.allclose(xp.sum(0), want, rtol=2e-5, atol=2e-5)
        if N <= 256:
            Ek = torch.randn(P, K, device=DEV, generator=g) * 0.3
            dx = torch.randn(M, device=DEV, generator=g) * torch.pow(10.0, torch.randint(-3, 4, (M,), device=DEV, generator=g).float())
            wt = torch.randn(K, N, device=DEV, generator=g) / 8                            # W2 [HID2, HID1]
            with _kernels(monkeypatch, "0", ["dfol_pair_logit_bwd_bf16", "dfol_linear_act_bf16_bf16"]):
                dp2, _, _ = _lib.pair_logit_bwd(dx, x, Ek, pred_off)
                dz_ref = _lib.linear_act_split(dp2, wt, None, _lib.ACT_NONE, transpose_w=True)
            with _kernels(monkeypatch, "1", ["dfol_pair_dz_tall_bf16"]):
                dz = _lib.pair_dz_tall_bf16(dx, x, Ek, rep, wt)
                dz2 = _lib.pair_dz_tall_bf16(dx, x, Ek, rep, wt, dz_out=dz.clone())
            assert dz.dtype == torch.bfloat16 and torch.equal(dz, dz_ref)
            assert torch.allclose(dz2.float(), 2 * dz.float(), rtol=1e-2, atol=0)


@pytest.mark.parametrize("counts,hid1,hid2", [([9900, 5112, 3540], 256, 300), ([64, 0, 71, 4000, 65, 0, 0, 1560, 97, 64 * 3 + 5], 256, 300), ([2450] * 9, 128, 64)])
def test_pair_wgrad_sums_bf16_storage_against_the_materialised_bf16_route(counts, hid1, hid2):
    """dfol_pair_wgrad_fused_sums_bf16 (pre2 and Z stored in bfloat16, dpre2 rebuilt and rounded in the kernel) against the bf16 mode's
    materialised route on the same tensors: dfol_pair_logit_bwd_bf16 (dpre2 stored in bfloat16, dE, dbe) and the bf16-storage weight gradient
    with its bias sums - equal up to the order of the fp32 accumulation; two runs are bit-identical."""
    from dfol_vqa_amd import _lib
    rng = np.random.RandomState(len(counts) + hid2)
    counts = np.asarray(counts, np.int64)
    M, P = int(counts.sum()), len(counts)
    dev = lambda a: torch.as_tensor(a).to(DEV)
    pred_off = dev(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64))
    rep = dev(np.repeat(np.arange(P), counts).astype(np.int32))
    p2 = dev((rng.normal(size=(M, hid2)) * 2.5).astype(np.float32)).to(torch.bfloat16)
    z = dev(np.where(rng.uniform(size=(M, hid1)) < 0.5, rng.uniform(-1, 0, (M, hid1)), rng.uniform(0, 6, (M, hid1))).astype(np.float32)).to(torch.bfloat16)
    E = dev((rng.normal(size=(P, hid2)) * 0.1).astype(np.float32))
    dx = dev((rng.normal(size=M) * 10.0 ** rng.randint(-2, 3, M)).astype(np.float32))
    with _lib.dense_math("bf16"):
        dp2, de_ref, dbe_ref = _lib.pair_logit_bwd(dx, p2, E, pred_off)
        dw_ref, db_ref = _lib.linear_wgrad(dp2, z, bias=True)
        dw, de, dbe, db2 = _lib.pair_wgrad_sums_bf16(dx, p2, z, E, pred_off, rep)
        again = _lib.pair_wgrad_sums_bf16(dx, p2, z, E, pred_off, rep)
    for a, b in zip((dw, de, dbe, db2), again):
        assert torch.equal(a, b)
    mag = (dp2.float().abs().t() @ z.float().abs())
    assert ((dw - dw_ref).abs() <= 4e-6 * mag + 1e-30).all()
    assert ((db2 - db_ref).abs() <= 4e-6 * dp2.float().abs().sum(0) + 1e-30).all()
    assert torch.allclose(de, de_ref, rtol=2e-5, atol=2e-5 * float(de_ref.abs().max()))
    assert torch.allclose(dbe, dbe_ref, rtol=2e-5, atol=2e-5 * float(dbe_ref.abs().max()))


# ---------------------------------------------------------------------------------------------------
# round 5: the FULL-SIZE train step end to end against the reference (golden g19) and against the reference's arithmetic restated under
# autograd in fp64 (oracle/dfol_oracle_torch.train_loss, itself pinned on g19 by tests/test_oracle_golden.py)
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g19_setup(tmp_path_factory):
    import json
    from dfol_vqa_amd import experiment
    from oracle import dfol_oracle as orc
    paths, names = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("g19")))
    cfg = syn.reference_config(paths, freeze_featurizer=False, freeze_attribute_network=False, freeze_relation_network=False, freeze_embedding_network=False)
    ont = experiment.build_ontology(cfg)
    model = experiment.build_model(cfg, ont)
    a, meta = gu.load("g19_full_size_train_step")
    weights = syn.load_seeded_weights(model, meta["weight_seed"])
    oont = orc.Ontology(paths["attribute_file"], paths["class_file"], paths["vocabulary_file"], paths["relation_file"])
    return model.to(DEV).train(), ont, oont, weights, a, meta


def _g19_step(model, ont, qs):
    from dfol_vqa_amd import _lib
    pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ont, "X").collate([dict(q) for q in qs])]
    model.zero_grad(set_to_none=True)
    _lib.PATH_COUNTS.clear()
    res = model(pbs, True)
    loss = training.compute_loss(pbs, res) / len(qs)
    loss.backward()
    grads = {k: (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().numpy() for k, p in model.named_parameters()}
    return float(loss.detach()), res["log_probability"].detach().cpu().numpy(), grads, dict(_lib.PATH_COUNTS)


@pytest.mark.parametrize("name,sums", [("binary_small", "auto"), ("query_rel_small", "auto"), ("binary_tall", "auto"), ("query_rel_tall", "auto"),
                                       ("binary_tall", "1"), ("query_rel_small", "1")] + [(n, "auto") for n in gu.G19_ATTR_CASES] + [("and_tall", "1")])
def test_g19_full_size_train_step_against_the_reference(g19_setup, name, sums, monkeypatch):
    """ONE `train_batch` forward + backward of the full-size model (2048 -> 512, 516 / 1036 -> 256 -> 300 -> 2335, dropout 0) on ragged 20..40
    object scenes with 0..3 relate hops, no-op tokens in the aligned relate batches and choose_rel option lists - and, round 6, the attribute-side
    and two-branch terminals (query_attr over 26-option categories, choose_attr, verify_attrs, and / or, compare, two_same, all_different;
    trainer.py:207-230's QUERY loss over <= 208 predicates) - through the FUSED training
    kernels (asserted: `_FusedHidden1`, `_PairTrunk`, `_HeadUse`, `_EmbRows`, the second-evaluation route for readers that cannot register
    with the trunk; no fallback to torch / vendor operators) - against (1) golden g19 = the reference's own `_train_batch` (loss,
    log-probabilities, norm and 4096 sampled entries of all twelve weight gradients; trainer.py:181-262, 429-442) and (2) the reference's
    arithmetic under autograd in fp64 on the CPU (oracle/dfol_oracle_torch.train_loss), full tensors.  `_tall`: >= 16384 pair rows, the
    persistent tall kernels; sums = "1": the logit layer's sums from the weight-gradient pass."""
    import warnings
    from oracle import dfol_oracle_torch as orct
    model, ont, oont, weights, a, meta = g19_setup
    monkeypatch.setenv("DFOL_HEAD_SUMS", sums)
    qs, cm, ref, grads = gu.g19_case(name, a, meta)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)           # a route that leaves the HIP kernels announces itself: here it must not happen
        loss, lp, got, routes = _g19_step(model, ont, qs)
    assert not [r for r in routes if r.startswith("fallback:")], routes
    assert routes.get("fused_hidden1", 0) == 1 and routes.get("pair_trunk", 0) == 1, routes
    assert routes.get("head_use", 0) >= 1 and routes.get("emb_rows", 0) >= 1, routes
    assert routes.get("head_use_backward_sums" if sums == "1" else "head_use_backward", 0) >= 1, routes
    if name in ("binary_tall", "query_rel_tall"):                # several readers of the trunk (>= 16384 pair rows: the persistent kernels): their dZ shares in one pass
        assert routes.get("pair_dz_multi", 0) == 1 and routes.get("head_use_dz_deferred", 0) >= 2, routes
    if name.startswith("binary"):                                # ragged hop counts: the aligned relate batches hold no-op tokens - their idle
        # questions ride along under a borrowed concept on the fused kernels (late round 6; before: tensor ops + a second evaluation of the trunk)
        assert routes.get("idle_questions_ride_along", 0) >= 1 and routes.get("head_use", 0) >= 2, routes
        assert routes.get("pair_second_evaluation", 0) == 0 and routes.get("logit_rows_gathered", 0) == 0, routes
    if name in gu.G19_ATTR_CASES:                                # round 6: the attribute-side terminals read their columns through the fused
        assert routes.get("attr_ll_fused", 0) >= 1, routes       # attribute-column function (visual_oracle._AttrLL), not gathers + tensor ops
    pairs = sum(q["scene"]["n"] * (q["scene"]["n"] - 1) for q in qs)
    assert (pairs >= 16384) == name.endswith("_tall")
    l32, l64 = ref["f32"][0], ref["f64"][0]
    assert abs(loss - l64) <= 8 * abs(l32 - l64) + 2e-5 * max(1.0, abs(l64)), (loss, l32, l64)
    gu.check_logprob(lp, ref["f32"][1], ref["f64"][1], "g19 " + name)
    gu.check_g19_gradients(got, grads, "g19 %s (sums=%s)" % (name, sums))
    # (2) every entry of every gradient against the fp64 autograd of the restated reference
    o_loss, o_lp, o_g = orct.train_loss(oont, qs, [q["scene"] for q in qs], weights, torch.float64)
    assert abs(o_loss - l64) <= 1e-9 * max(1.0, abs(l64))       # (the checker itself still agrees with the golden on this machine)
    for pname, g in grads.items():
        ref64 = o_g[pname]
        own = np.abs(g["sample32"].astype(np.float64) - g["sample64"]).max()     # the reference's own fp32 noise on this tensor (sampled)
        scale = np.abs(ref64).max() + 1e-30
        err = np.abs(got[pname].astype(np.float64) - ref64).max()
        assert err <= 16 * own + 2e-3 * scale, "%s d%s: |dgrad| %.3g vs the reference's own %.3g (scale %.3g)" % (name, pname, err, own, scale)


def test_pair_branch_on_its_side_stream_changes_no_bit(g19_setup, monkeypatch):
    """The pair branch of a train step is issued on a side stream (visual_oracle._pair_side_stream: its backward's large kernels then run beside the
    attribute branch's small launches).  Same kernels, same arithmetic, no shared accumulators: `training.train_batch` at FULL model size on the
    bench's program (select -> filter -> relate -> exist for every question: every route deterministic - ragged hop counts would bring torch's
    atomic index_select backward in, side stream or not) from the same state gives the same loss, gradients and updated weights bit for bit
    with the side stream (twice) and without it (DFOL_TRAIN_PAIR_STREAM=0); the route is taken by default."""
    from dfol_vqa_amd import _lib
    model, ont, oont, weights, a, meta = g19_setup
    voc = ont._vocabulary["idx_to_arg"]
    nouns = [t for t in voc if t.startswith("noun")][:8]
    attrs = [t for t in voc if t.startswith("attr")][:6]
    rels = [t for t in voc if t.startswith("rel ")][:5]
    assert nouns and attrs and rels
    qs = []
    for i in range(24):
        br, last = syn.three_hop_program(7100 + i, nouns, attrs, rels)
        qs.append(syn.question(7100 + i, br, last, "yes" if i % 2 else "no", syn.feature_scene(7100 + i, 14 + i % 9, 2048)))
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    runs = []
    try:
        for flag in ("1", "0", "1", "0"):
            monkeypatch.setenv("DFOL_TRAIN_PAIR_STREAM", flag)
            model.load_state_dict(start)
            model.zero_grad(set_to_none=True)
            pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ont, "X").collate([dict(q) for q in qs])]
            opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
            _lib.PATH_COUNTS.clear()
            loss, _ = training.train_batch(model, opt, pbs, clip_norm=0.65)
            torch.cuda.synchronize()
            routes = dict(_lib.PATH_COUNTS)
            assert (routes.get("pair_branch_side_stream", 0) >= 1) == (flag == "1") and not [r for r in routes if r.startswith("fallback:")], routes
            runs.append((float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None},
                         {k: v.detach().clone() for k, v in model.state_dict().items()}))
    finally:
        model.load_state_dict(start)
        model.zero_grad(set_to_none=True)
    assert len(runs[0][1]) >= 12 and all(float(g.abs().sum()) > 0 for g in runs[0][1].values())
    for other in runs[1:]:
        assert runs[0][0] == other[0]
        for k in runs[0][1]:
            assert torch.equal(runs[0][1][k], other[1][k]), ("gradient", k)
        for k in runs[0][2]:
            assert torch.equal(runs[0][2][k], other[2][k]), ("weights", k)


@pytest.mark.parametrize("n_list", [[5, 7], [2, 1, 9], [30]])
def test_small_batches_train_inside_the_library(g19_setup, n_list):
    """below 4096 pair rows the full-size model's tall products used to leave for nn.functional.linear / `@` (vendor GEMM,
    announced).  The split-operand and the TN weight-gradient kernels take any row count: 2 - 3 questions on 1 - 30 objects (34 - 870
    pair rows; an image of ONE object among them) train through the same fused routes - no fallback announced - and agree with the fp64
    autograd of the restated reference on every gradient entry."""
    import warnings
    from oracle import dfol_oracle_torch as orct
    model, ont, oont, weights, a, meta = g19_setup
    import tempfile
    names_ = syn.write_synthetic_ontology(tempfile.mkdtemp())[1]
    rels, nouns = names_["relations"][:5], names_["nouns"][:8]
    qs = []
    for i, n in enumerate(n_list):
        qid = 777000 + 10 * len(n_list) + i
        branch = [syn.op("select", nouns[i]), syn.op("relate", rels[i], bool(i % 2), nouns[i + 1]), syn.op("relate", "not(%s)" % rels[i + 1], not bool(i % 2), "_")]
        qs.append(syn.question(qid, [branch], syn.op("exist"), "yes" if i % 2 else "no", syn.feature_scene(qid, n, 2048)))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        loss, lp, got, routes = _g19_step(model, ont, qs)
    assert not [r for r in routes if r.startswith("fallback:")], routes
    assert routes.get("fused_hidden1", 0) == 1 and routes.get("pair_trunk", 0) == 1 and routes.get("head_use", 0) >= 1, routes
    o_loss, o_lp, o_g = orct.train_loss(oont, qs, [q["scene"] for q in qs], weights, torch.float64)
    l32 = orct.train_loss(oont, qs, [q["scene"] for q in qs], weights, torch.float32)
    assert abs(loss - o_loss) <= 8 * abs(l32[0] - o_loss) + 2e-5 * max(1.0, abs(o_loss)), (loss, l32[0], o_loss)
    for pname, ref64 in o_g.items():
        own = np.abs(l32[2][pname] - ref64).max()
        scale = np.abs(ref64).max() + 1e-30
        err = np.abs(got[pname].astype(np.float64) - ref64).max()
        assert err <= 16 * own + 2e-3 * scale, "%s d%s: |dgrad| %.3g vs the fp32 restatement's own %.3g (scale %.3g)" % (n_list, pname, err, own, scale)


def test_g19_detects_a_broken_trunk_accumulation(g19_setup, monkeypatch):
    """The check above has teeth: with the deferred trunk's accumulation across readers deliberately broken (every reader after the first
    overwrites the second layer's weight gradient instead of adding to it) the g19 comparison fails."""
    from dfol_vqa_amd import visual_oracle as vo
    model, ont, oont, weights, a, meta = g19_setup
    qs, cm, ref, grads = gu.g19_case("query_rel_small", a, meta)      # choose_rel's two option slots: two readers of one trunk
    orig = vo._HeadUse.backward

    def broken(ctx, dx):
        st = ctx.state
        if dx is not None and st.get("dw") is not None:
            st["dw"] = torch.zeros_like(st["dw"])               # drop what the earlier readers accumulated
        return orig(ctx, dx)
    monkeypatch.setattr(vo._HeadUse, "backward", staticmethod(broken))
    _, _, got, routes = _g19_step(model, ont, qs)
    assert routes.get("head_use", 0) >= 2, routes                # several readers: the accumulation matters
    with pytest.raises(AssertionError):
        gu.check_g19_gradients(got, grads, "broken")


def test_fallback_routes_announce_themselves(ontology):
    """A relation network the fused training kernels do not take (g12's 8-wide one) trains through torch operators - correctly (golden g12),
    and no longer silently: a RuntimeWarning names the widths, and `_lib.PATH_COUNTS` records the route."""
    from dfol_vqa_amd import _lib
    a, meta = gu.load("g12_weight_gradients")
    weights = {k[2:]: a[k] for k in a.files if k.startswith("w:")}
    model = neural_model(ontology, meta["config"], weights).train()
    qs = [{"program": q["program"], "answer": q["answer"], "question_id": q["question_id"], "image_id": "img000", "tokens": [],
           "original_dict": None, "question": None, "scene": {"n": q["n"], "X": a["binary:X_%d" % i]}}
          for i, q in enumerate(meta["sets"]["binary"]["questions"])]
    pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ontology, "X").collate(qs)]
    _lib.PATH_COUNTS.clear()
    _lib._WARNED.clear()
    with pytest.warns(RuntimeWarning, match="relation network training"):
        res = model(pbs, True)
        (training.compute_loss(pbs, res) / len(qs)).backward()
    assert any(r.startswith("fallback:relation network training") for r in _lib.PATH_COUNTS), dict(_lib.PATH_COUNTS)
    assert "pair_trunk" not in _lib.PATH_COUNTS


@pytest.mark.parametrize("mlp_math", ["fp32", "bf16"])
def test_train_from_h5_program_files(ontology, golden_dir, mini_ontology_paths, mlp_math):
    """BASELINE configs[3]'s input path on the GPU: the g18 program-bytecode .h5 files (written by the reference's GQAH5Encoder) and feature
    chunk files, read by data.ProgramDataset / BatchGQABoxFeaturesCollator (data_pipeline.py:328-367, 391-453), TRAINED for two
    `train_batch` steps per file (trainer.py:429-442) in the configured `mlp_math`.  The first step's loss equals the oracle's
    `compute_loss` (trainer.py:181-262) of its own fp64 forward on the same files; the second step runs on updated weights (its loss
    moves) and stays finite.  Eight terminal operators, BINARY and QUERY."""
    from oracle import dfol_oracle as orc
    from test_data_path import g18_batches
    p = mini_ontology_paths
    oont = orc.Ontology(p["attribute_file"], p["class_file"], p["vocabulary_file"], p["relation_file"])
    seen = 0
    for name, fm, items, pbs, lp32, lp64, a, meta in g18_batches(ontology, golden_dir):
        weights = {k[2:]: a[k] for k in a.files if k.startswith("w:")}
        model = neural_model(ontology, dict(meta["config"], mlp_math=mlp_math), weights).train()
        for prm in model.parameters():
            prm.requires_grad_(prm.dtype.is_floating_point and prm is not model._global_step)
        if mlp_math == "bf16":
            model._mlp_math = "bf16"
        dev_pbs = [pb.to_cuda(DEV) for pb in pbs]
        opt = torch.optim.Adam([q for q in model.parameters() if q.requires_grad], lr=1e-3)
        l0, res = training.train_batch(model, opt, dev_pbs, clip_norm=0.65)
        l1, _ = training.train_batch(model, opt, dev_pbs, clip_norm=0.65)
        feats = pbs[0]._object_features.numpy()
        off = np.concatenate([[0], np.cumsum(fm["objects"])])
        scenes = [{"n": int(n), "X": feats[off[i]:off[i + 1]]} for i, n in enumerate(fm["objects"])]
        qs = [{"program": it["program"], "answer": it["answer"], "question_id": i, "image_id": it["image_id"]} for i, it in enumerate(items)]
        r64 = orc.run_questions(oont, qs, scenes, np.float64, weights=weights, give_answer=False)
        r32 = orc.run_questions(oont, qs, scenes, np.float32, weights=weights, give_answer=False)
        ref64 = float(orc.compute_loss(r64, [q["answer"] for q in qs]))
        ref32 = float(orc.compute_loss(r32, [q["answer"] for q in qs]))
        tol = 8 * abs(ref32 - ref64) + (2e-2 if mlp_math == "bf16" else 2e-5) * max(1.0, abs(ref64))
        assert abs(l0 - ref64) <= tol, (name, mlp_math, l0, ref32, ref64)
        assert np.isfinite(l1) and l1 != l0, (name, l0, l1)
        seen += 1
    assert seen == 8


# ---------------------------------------------------------------------------------------------------
# round 6: the CALIBRATOR phases of the curriculum at FULL model size against the reference (golden g24)
# ---------------------------------------------------------------------------------------------------
G24_KINDS = ["exist", "verify_rel", "choose_rel", "query_attr", "and"]


@pytest.fixture(scope="module")
def g24_setup(tmp_path_factory):
    import json
    from dfol_vqa_amd import experiment
    d = str(tmp_path_factory.mktemp("g24"))
    paths, names = syn.write_synthetic_ontology(d)
    with open(paths["vocabulary_file"]) as f:
        vocab = json.load(f)
    paths["word_embedding_file"] = syn.write_synthetic_glove(os.path.join(d, "glove.txt"), vocab["idx_to_arg"])
    cfg = syn.reference_config(paths, activate_attention_transfer=True, dropout=0.0)
    ont = experiment.build_ontology(cfg)
    model = experiment.build_model(cfg, ont)
    a, meta = gu.load("g24_calibrator_train_step")
    syn.load_seeded_weights(model, meta["weight_seed"])
    syn.load_seeded_calibrator(model, meta["calibrator_seed"])
    return model.to(DEV).train(), ont, a, meta


def _g24_relate_hops(questions):
    """The relate calls of the collated batch, from the programs' structure: a branch is aligned on its relate operators, so it runs as many
    GQARelateBatch calls as its longest chain of relates (each holds at least one valid token), and verify_rel owns one more."""
    hops = sum(max(sum(o["operator"] == "relate" for o in q["program"]["branches"][b]) if b < len(q["program"]["branches"]) else 0 for q in questions)
               for b in range(max(len(q["program"]["branches"]) for q in questions)))
    return hops + any(q["program"]["last_op"]["operator"] == "verify_rel" for q in questions)


class _G24RelateCalls(object):
    """Forward pre-hooks on every GQARelateBatch (the relate operator's and the one verify_rel owns): the calls whose relation tokens include a
    valid one, and how many of those found their op_id in BOTH modulation dictionaries of their RelateBatch (the calibrated branch)."""

    def __init__(self, model):
        from dfol_vqa_amd import gqa_ops
        from dfol_vqa_amd.host_util import is_valid_token
        self.valid = self.calibrated = 0
        self._is_valid = is_valid_token
        self._handles = [m.register_forward_pre_hook(self._hop, with_kwargs=True) for m in model.modules() if isinstance(m, gqa_ops.GQARelateBatch)]
        assert len(self._handles) >= 2

    def _hop(self, module, args, kwargs):
        op_id = args[0] if args else kwargs["op_id"]
        rel = args[3] if len(args) > 3 else kwargs["relation_list"]
        if any(self._is_valid(v) for v in (rel if isinstance(rel, list) else [rel])):
            self.valid += 1
            r = module._relate
            self.calibrated += (r._subject_modulations.get(op_id) is not None and r._object_modulations.get(op_id) is not None)

    def close(self):
        for h in self._handles:
            h.remove()


# route: generic = every kind under both backwards, under the ids these cases have always had; relate_train = every kind with the HIP backward,
# and verify_rel under autograd (ops._RelateKeep.backward feeding torch's autograd through the modulate restatement)
@pytest.mark.parametrize("kind,backward,route", [pytest.param(k, b, "generic", id="%s-%s" % (k, b)) for b in ("hip", "autograd") for k in G24_KINDS] +
                         [pytest.param(k, b, "relate_train", id="%s-%s-relate_train" % (k, b))
                          for k, b in [(k, "hip") for k in G24_KINDS] + [("verify_rel", "autograd")]])
def test_g24_calibrator_phase_train_step_against_the_reference(g24_setup, kind, backward, route, monkeypatch):
    """ONE train-mode forward + loss + backward of the full-size model in the curriculum's CALIBRATOR phases (cur6-7: oracle frozen,
    LSTMCell(318 -> 50) x 2 + Linear(100 -> 4) train) against the REFERENCE's own `_train_batch` (golden g24: loss, log-probabilities, norm +
    sampled entries of all ten calibrator gradients, fp32 and fp64; trainer.py:181-262, 429-442 over batch_base_ops.py:407-467, 598-684) on
    ragged 10..40-object scenes, BINARY and QUERY losses.  `hip`: the hand-written LSTM-cell and modulate backward kernels (the defaults);
    `autograd`: the same forward with torch's autograd through those two ops.

    route `relate_train`: the same step under DFOL_RELATE_TRAIN=1, every assertion unchanged - the one-posterior ungated route
    (gqa_ops.GQARelateBatch._forward_train_one: dfol_relate_keep_fwd_f32 / dfol_relate_keep_bwd_f32, then the kept side's modulations through
    ops.modulate) against the reference.  Every relate call with a valid token takes the route, and takes its calibrated branch: the oracle is
    frozen, but each branch starts at select(<noun>) in some question, a calibrated filter, so the incoming variable carries the calibrator's
    gradient; the interpreter's op ids end in a digit (never 'n'), so both modulation dictionaries hold the hop; and the incoming set of a
    relate operator never carries a predicate-question map.  No hop steps aside, and the count is the one the programs' structure gives
    (_g24_relate_hops: exist 3, verify_rel 2 + 1, choose_rel 1, query_attr 1, and 3).  choose_rel's own two-posterior cell is a RelateBatch
    without a GQARelateBatch around it and stays on the generic route, as it does for an uncalibrated model."""
    from test_interpreter_gpu import CalibrationCollater
    from dfol_vqa_amd import _lib, logic_ops
    model, ont, a, meta = g24_setup
    if route == "relate_train":
        monkeypatch.setenv("DFOL_RELATE_TRAIN", "1")
    else:
        monkeypatch.delenv("DFOL_RELATE_TRAIN", raising=False)
    for k in ("DFOL_LSTM_BWD", "DFOL_MODULATE_BWD"):
        monkeypatch.setenv(k, "hip" if backward == "hip" else "torch")
    trainable = sorted(k for k, p in model.named_parameters() if p.requires_grad)
    assert len(trainable) == 10 and all("attention" in k for k in trainable), trainable
    cm = meta["cases"][kind]
    qs = [syn.question(q["question_id"], q["program"]["branches"], q["program"]["last_op"], q["answer"],
                       syn.feature_scene(q["question_id"], q["n"], meta["feature_dim"])) for q in cm["questions"]]
    pbs = [pb.to_cuda(DEV) for pb in CalibrationCollater(ont).collate([dict(q) for q in qs])]
    model.zero_grad(set_to_none=True)
    calls = _G24RelateCalls(model)
    _lib.PATH_COUNTS.clear()
    try:
        res = model(pbs, True)
    finally:
        calls.close()
    assert int(res["type"]) == cm["type"]
    loss = training.compute_loss(pbs, res) / len(qs)
    loss.backward()
    counts = dict(_lib.PATH_COUNTS)
    if route == "relate_train":
        expected = {"exist": 3, "verify_rel": 3, "choose_rel": 1, "query_attr": 1, "and": 3}[kind]
        assert _g24_relate_hops(cm["questions"]) == expected == calls.valid, (kind, _g24_relate_hops(cm["questions"]), calls.valid)
        assert counts.get("relate_train_one", 0) == calls.valid, (kind, counts, calls.valid)
        assert calls.calibrated == calls.valid, (kind, calls.calibrated, calls.valid)              # the calibrated branch ran in every one of them
        assert not [k for k in counts if k.startswith("fallback:")], counts
        for mod in model.modules():                                 # a leak would hand a stale modulation to the next batch's hop of the same op_id
            if isinstance(mod, logic_ops.RelateBatch):
                for attr in ("_subject_modulations", "_object_modulations", "_forward_subject_state", "_forward_object_state"):
                    assert not getattr(mod, attr), (kind, attr, list(getattr(mod, attr)))
    else:
        assert "relate_train_one" not in counts, counts
    l32, l64, got_loss = float(a[kind + ":loss_f32"]), float(a[kind + ":loss_f64"]), float(loss.detach())
    assert abs(got_loss - l64) <= 8 * abs(l32 - l64) + 2e-5 * max(1.0, abs(l64)), (got_loss, l32, l64)
    gu.check_logprob(res["log_probability"].detach().cpu().numpy(), a[kind + ":lp_f32"], a[kind + ":lp_f64"], "g24 " + kind)
    got = {}
    for k, p in model.named_parameters():
        if p.requires_grad:
            short = k[k.index("_filter.") + len("_filter."):]
            got.setdefault(short, (torch.zeros_like(p) if p.grad is None else p.grad).detach().cpu().numpy())
    grads = {}
    for key in a.files:
        if key.startswith(kind + ":gs:") and key.endswith(":f64"):
            pname = key[len(kind) + 4:-4]
            grads[pname] = {"sample64": a[key], "sample32": a[key[:-3] + "f32"], "norm64": float(a["%s:gn:%s:f64" % (kind, pname)]),
                            "norm32": float(a["%s:gn:%s:f32" % (kind, pname)])}
    assert sorted(grads) == sorted(got), (sorted(grads), sorted(got))
    for pname, g in grads.items():
        full = got[pname].astype(np.float64).reshape(-1)
        smp = full[syn.gradient_sample_index(pname, full.size)]
        ref64, ref32 = g["sample64"].astype(np.float64), g["sample32"].astype(np.float64)
        scale = max(np.abs(ref64).max(), g["norm64"] / np.sqrt(full.size)) + 1e-30
        own, err = np.abs(ref32 - ref64).max(), np.abs(smp - ref64).max()
        print("  g24 %s %s %s d%s: |dgrad| %.3g  bound %.3g" % (kind, backward, route, pname, err, 8 * own + 2e-3 * scale))
        assert err <= 8 * own + 2e-3 * scale, "g24 %s d%s: |dgrad| %.3g vs the reference's own %.3g (scale %.3g)" % (kind, pname, err, own, scale)
        norm = np.sqrt((full ** 2).sum())
        assert abs(norm - g["norm64"]) <= 8 * abs(g["norm32"] - g["norm64"]) + 2e-3 * g["norm64"] + 1e-30, (kind, pname, norm, g["norm64"], g["norm32"])


def test_train_step_over_programs_of_differing_lengths_graph_equals_eager():
    """bench.py --mode train --hops ragged (select -> 1..3 filter / relate hops -> exist: a program length per question, no-op tokens after collate) at
    full model size and >= 16384 pair rows: every relate reader stays on the fused kernels - the idle questions ride along, ONE dZ pass for all readers
    (dfol_pair_dz_tall_multi_f32), the later readers' logits out of the fused forward - with no fallback; the step replayed as a HIP graph leaves the
    same weights as the eager step, bit for bit, and the loss falls."""
    import importlib.util
    from dfol_vqa_amd import parallel, _lib
    spec = importlib.util.spec_from_file_location("bench_for_test_ragged", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    finals = []
    for graphed in (False, True):
        args = bench.parse(["--mode", "train", "--objects", "30", "--batch", "48", "--hops", "ragged"])
        torch.manual_seed(9)
        model, ontology, paths, names = bench.build_model(args, DEV, train=True)
        qs, pbs = bench.build_batch(args, 0, ontology, names, DEV)
        hops = [sum(1 for o in q["program"]["branches"][0] if o["operator"] == "relate") for q in qs]
        assert max(hops) >= 2 and len(set(len(q["program"]["branches"][0]) for q in qs)) >= 3      # differing lengths, several relate steps
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        bucket = parallel.GradBucket(params)
        _lib.PATH_COUNTS.clear()
        if graphed:
            step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=1)
            losses = [float(step()[0]) for _ in range(3)]
        else:
            losses = [float(training.train_batch(model, opt, pbs, 0.65, bucket=bucket, sync_loss=False)[0]) for _ in range(4)][1:]
            routes = dict(_lib.PATH_COUNTS)
            assert not [r for r in routes if r.startswith("fallback:")], routes
            assert routes.get("idle_questions_ride_along", 0) >= 4 and routes.get("pair_dz_multi", 0) == 4 and routes.get("head_use_logits_from_trunk", 0) >= 4, routes
            assert routes.get("pair_second_evaluation", 0) == 0 and routes.get("logit_rows_gathered", 0) == 0, routes
        torch.cuda.synchronize()
        assert all(np.isfinite(l) for l in losses) and losses[-1] < losses[0], losses
        finals.append((losses, {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert finals[0][0] == finals[1][0]
    for k in finals[0][1]:
        assert torch.equal(finals[0][1][k], finals[1][1][k]), k
