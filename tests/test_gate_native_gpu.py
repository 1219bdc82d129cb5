"""The gated model on the fast inference path (DFOL_GATE_NATIVE=1): the one-launch gated Relate (dfol_relate_one_gate_fwd_f32,
csrc/dfol_logic_gate.hip) against the float64 restatement of tests/gate_util.py and against the generic gated route, and the gated opcodes of
the native executor against the Python operator loop, bit for bit, and against the reference's own gated interpreter (g25_gate_interpreter).

The kernel's output is one half of the restatement's cell.  With x the selected variable, prev the incoming one and T the tile with prev's
objects along rows:  x_is_subject set -> post_s of t_relate_gate(a = x, b = prev, l = T^T);  clear -> post_o of t_relate_gate(a = prev, b = x, l = T).

Dispatch arms (NS / 4 column groups -> lanes per row; NS > 256 -> the plain workgroup kernel): the shapes of test_trainable_gate_gpu.SHAPES,
NS 4 -> LPR 1 | 8 -> 2 | 12, 16 -> 4 | 20, 32 -> 8 | 36, 64 -> 16 | 68, 128 -> 32 | 132, 256 -> 64 | 260 -> plain."""

import copy
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gate_util as GU  # noqa: E402
import golden_util as U  # noqa: E402
import test_trainable_gate_gpu as TG  # noqa: E402
from dfol_vqa_amd import _lib, native_exec, ops  # noqa: E402
from dfol_vqa_amd import native_plan as NP  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from test_native_gpu import ALL_KINDS, TableCollater, _FullCalibrationCollater, same_results  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = TG.DEV
dev = TG.dev
models = TG.models                      # the seeded synthetic model, gated and ungated (module fixture, one instance for this file)
mini_ontology = TG.mini_ontology
_CACHE = {}


# ---- the kernel -------------------------------------------------------------------------------------------------------------------------------
def one_problem(name):
    """test_trainable_gate_gpu.problem(name) turned into the one-posterior launch: x [P, NS] a row per predicate (its own values), prev = the
    problem's object priors [Q, NS], T = the problem's tile read as (prev rows, x columns), quant_prev = the problem's quant_s (EXISTS / FOR_ALL
    alternating; FOR_ALL for the lone predicate), subject flags mixed within the launch; the restatement in float32 and float64, once."""
    if name in _CACHE:
        return _CACHE[name]
    pr = TG.problem(name)
    rng = np.random.RandomState(sum(map(ord, name)) + 1)
    P, NS = pr["P"], pr["NS"]
    op = dict(pr=pr, x=np.zeros((P, NS), np.float32), prev=pr["prior_o"], T=pr["tile"], quant=pr["quant_s"],
              flag=((np.arange(P) + NS // 4) % 2).astype(np.uint8) if P > 1 else np.ones(1, np.uint8))
    for p in range(P):
        n = pr["n"][pr["pq"][p]]
        op["x"][p, :n] = np.minimum(syn.table_log_likelihood(rng, (n,), "unif") * 0.3, 0)
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        op[tag] = restate_one(op, dt)
    op["swapped"] = restate_one(op, torch.float64, swap=True)
    _CACHE[name] = op
    return op


def restate_one(op, dt, swap=False, W=None, c=None, near=None):
    """-> [P, NS].  swap: inner and outer gate exchanged (what the kernel must NOT compute).  near: a list that receives, per predicate, the
    mask of outputs a clamp boundary reaches (gate_util.t_relate_gate)."""
    pr = op["pr"]
    t = lambda a: torch.tensor(a, dtype=dt)
    W, c = (pr["W"], pr["c"]) if W is None else (W, c)
    (Ws, cs), (Wo, co) = ((t(W[0]), t(c[0])), (t(W[1]), t(c[1])))
    if swap:
        (Ws, cs), (Wo, co) = (Wo, co), (Ws, cs)
    any_neg = pr["neg"] is not None
    rows = []
    for p in range(pr["P"]):
        q = pr["pq"][p]
        n = pr["n"][q]
        x, prev, T = t(op["x"][p, :n]), t(op["prev"][q, :n]), t(op["T"][p, :n, :n])
        out = np.zeros(pr["NS"], np.float64)
        if pr["active"] is not None and not pr["active"][p]:
            out[:n] = prev.numpy()
        else:
            ng, qp, nr = (float(pr["neg"][p]) if any_neg else 0.0), op["quant"][p], {}
            if op["flag"][p]:
                post = GU.t_relate_gate(x, prev, T.t(), qp, qp, ng, any_neg, Ws, cs, Wo, co, lone_forall_identity=pr["lone"], near=nr)[0]
            else:
                post = GU.t_relate_gate(prev, x, T, qp, qp, ng, any_neg, Ws, cs, Wo, co, lone_forall_identity=pr["lone"], near=nr)[1]
            out[:n] = post.numpy()
            if near is not None:
                near.append(nr["s" if op["flag"][p] else "o"].numpy())
        rows.append(out)
    return np.stack(rows)


def run_one(op, tile=None, W=None, c=None):
    pr = op["pr"]
    W, c = (pr["W"], pr["c"]) if W is None else (W, c)
    gs, go = (_lib.gate_params(dev(W[k]), dev(c[k])) for k in (0, 1))
    return _lib.relate_one_gate_fwd(dev(op["x"]), dev(op["prev"]), dev(op["T"]) if tile is None else tile, dev(pr["pq"]), dev(pr["n"]), dev(op["quant"]),
                                    dev(op["flag"]), gs, go, dev(pr["neg"]), dev(pr["active"]), lone_forall_identity=pr["lone"])


def test_the_cases_cover_what_they_are_for():
    ops_ = [one_problem(n) for n in TG.SHAPES]
    assert sorted({o["pr"]["NS"] for o in ops_}) == [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260]
    assert any(len(set(o["flag"])) == 2 for o in ops_) and any(len(set(o["quant"])) == 2 for o in ops_)          # mixed within a launch
    assert any(o["pr"]["neg"] is not None and o["pr"]["neg"].any() for o in ops_) and any(o["pr"]["active"] is not None for o in ops_)
    assert any(o["pr"]["P"] == 1 and o["quant"][0] == 0 for o in ops_) and any(o["pr"]["P"] == 5 for o in ops_)   # the literal branch; P % 4 != 0
    assert any((o["pr"]["n"] == 1).any() for o in ops_) and any((o["pr"]["n"] % 4 != 0).any() for o in ops_)
    assert any(len(o["pr"]["pq"]) > len(set(o["pr"]["pq"])) for o in ops_)                                          # many-to-one pred_q
    for o in ops_:                                                # the two gates hold distinct values
        assert not np.array_equal(o["pr"]["W"][0], o["pr"]["W"][1]) and not np.array_equal(o["pr"]["c"][0], o["pr"]["c"][1])


@pytest.mark.parametrize("name", list(TG.SHAPES))
def test_kernel_against_the_float64_restatement(name):
    op = one_problem(name)
    pr = op["pr"]
    with torch.no_grad():
        out = run_one(op)
        again = run_one(op)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.cpu().numpy().view(np.uint32))           # two launches, the same bits
    U.check_logprob(got, op["f32"], op["f64"], name)
    for p in range(pr["P"]):
        assert not got[p, pr["n"][pr["pq"][p]]:].view(np.uint32).any(), (name, p, "padding")  # exactly +0
    if pr["active"] is not None:                                   # a no-op row is prev's row, bit for bit
        p = int(np.nonzero(pr["active"] == 0)[0][0])
        q, n = pr["pq"][p], pr["n"][pr["pq"][p]]
        assert np.array_equal(got[p, :n].view(np.uint32), op["prev"][q, :n].view(np.uint32))
    # inner and outer gate exchanged lies outside the bound: the bound tells the two apart (CPU, the restatement alone)
    with pytest.raises(AssertionError):
        U.check_logprob(op["swapped"], op["f32"], op["f64"], name + " with the gates swapped")


@pytest.mark.parametrize("name", list(TG.SHAPES))
def test_kernel_against_the_generic_route(name):
    """The same inputs through ops.relate_gate_fwd(..., want=...) on the un-oriented (subject-row) tile, one question per predicate: the kept
    rows agree under the policy (another summation order: not bits)."""
    op = one_problem(name)
    pr = op["pr"]
    P, f = pr["P"], op["flag"].astype(bool)
    prev_p = op["prev"][pr["pq"]]                                  # [P, NS]
    prior_s, prior_o = np.where(f[:, None], op["x"], prev_p), np.where(f[:, None], prev_p, op["x"])
    tile = np.where(f[:, None, None], op["T"].transpose(0, 2, 1), op["T"])
    want = np.where(f, _lib.WANT_SUBJECT, _lib.WANT_OBJECT).astype(np.uint8)
    Ws, cs, Wo, co = TG.gate_tensors(pr)
    with torch.no_grad():
        ps, po = ops.relate_gate_fwd(dev(prior_s), dev(prior_o), dev(np.ascontiguousarray(tile)), dev(np.arange(P, dtype=np.int32)), dev(pr["n"][pr["pq"]]),
                                     dev(op["quant"]), dev(op["quant"]), Ws, cs, Wo, co, dev(pr["neg"]), dev(pr["active"]), want=dev(want),
                                     lone_forall_identity=pr["lone"])
        one = run_one(op).cpu().numpy()
    kept = np.where(f[:, None], ps.cpu().numpy(), po.cpu().numpy())
    # (a no-op row of the generic cell is the wanted side's own prior - x where x is the subject - and the interpreter's mask gate puts prev back;
    # the one-launch kernel writes prev at once, as relate_one_fwd_kernel does: the live rows are what the two routes share)
    live = np.ones(P, bool) if pr["active"] is None else pr["active"].astype(bool)
    U.check_logprob(kept[live], op["f32"][live], op["f64"][live], name + " generic route")
    # the two routes against each other: each within the policy of the float64 value, so within twice the policy's slack of each other
    err = np.abs(np.exp(one[live]) - np.exp(kept[live])).max()
    own = np.abs(np.exp(op["f32"][live]) - np.exp(op["f64"][live])).max()
    assert err <= 2 * (2.0 * own + 1e-6), (name, err, own)


def test_saturated_sigmoids():
    """Gate weights of magnitude ~100 (pre-activations beyond +-90): sigmoids saturate to 0 / 1 in float32 and a clamp binds.  Finite, and within
    the policy of the float64 restatement, leaving out the outputs a clamp argument within 1 +- 1e-4 of 1e-20 reaches (at most 0.1 %) - the
    rule of test_trainable_gate_gpu.test_saturated_sigmoids_forward.  (Scale 4.0 is in the shapes above: ns16_lpr4, ns64_lpr16.)"""
    assert {TG.SHAPES[n][5] for n in ("ns16_lpr4", "ns64_lpr16")} == {4.0}
    rng = np.random.RandomState(100)                               # (that test's seed, so its gates: in the restatement 44 of the 118 outputs sit
    NS, n_list = 32, [32, 27, 30, 29]                              # on a clamp and none within 1e-4 of its boundary)
    P = len(n_list)
    W = (rng.choice([-1.0, 1.0], (2, 6, 2)) * rng.uniform(80, 120, (2, 6, 2))).astype(np.float32)
    c = (rng.choice([-1.0, 1.0], (2, 6)) * rng.uniform(80, 120, (2, 6))).astype(np.float32)
    pr = dict(P=P, NS=NS, n=np.asarray(n_list, np.int32), pq=np.arange(P, dtype=np.int32), neg=None, active=None, lone=False, W=W, c=c)
    op = dict(pr=pr, x=np.zeros((P, NS), np.float32), prev=np.zeros((P, NS), np.float32), T=np.full((P, NS, NS), -30, np.float32),
              quant=np.asarray([1, 0, 1, 0], np.float32), flag=np.asarray([1, 1, 0, 0], np.uint8))
    for p, n in enumerate(n_list):
        op["x"][p, :n], op["prev"][p, :n], op["T"][p, :n, :n] = -rng.uniform(0.01, 3, n), -rng.uniform(0.01, 3, n), -rng.uniform(0.01, 6, (n, n))
    near = []
    r32, r64 = restate_one(op, torch.float32), restate_one(op, torch.float64, near=near)
    live = np.concatenate([r64[p, :n] for p, n in enumerate(n_list)])
    assert (live < -46).sum() > 0, "no clamp binds: the case does not test what it is for"
    with torch.no_grad():
        got = run_one(op).cpu().numpy()
    assert np.isfinite(got).all()
    keep = ~np.concatenate(near)
    assert (~keep).sum() <= 1e-3 * keep.size, int((~keep).sum())
    flat = lambda a: np.concatenate([a[p, :n] for p, n in enumerate(n_list)])[keep]
    U.check_logprob(flat(got), flat(r32), flat(r64), "saturated one-posterior relate")


# ---- the interpreter ------------------------------------------------------------------------------------------------------------------------
def distinct_gates(model, seed=7):
    """Every gate tensor its own values (a fresh model's gates are torch's seeded initialisation: distinct already, but small)."""
    rng = np.random.RandomState(seed)
    named = [(k, p) for k, p in model.named_parameters() if "_nlg" in k]
    assert len(named) >= 32
    with torch.no_grad():
        for _, p in named:
            p.copy_(torch.from_numpy(rng.uniform(-0.7, 0.7, tuple(p.shape)).astype(np.float32)))
    flat = [p.detach().cpu().numpy().tobytes() for _, p in named]
    for i in range(len(flat)):
        for j in range(i):
            assert len(flat[i]) != len(flat[j]) or flat[i] != flat[j], (named[i][0], named[j][0])


@pytest.fixture(scope="module")
def gated(models, tmp_path_factory):
    by, names = models
    model, ont = by[True]
    distinct_gates(model)
    paths, _ = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("gate_native")))
    with open(paths["attribute_file"]) as f:
        categories = json.load(f)
    return model, ont, names, categories


def routes(model, qs, monkeypatch, split=1, collater=None, ont=None, **kw):
    """The same questions, switch on, through the executor (every batch a `native_program`, none a `python_program`, no fallback) and through the
    Python loop -> (native, python)."""
    monkeypatch.setenv("DFOL_GATE_NATIVE", "1")
    out = []
    for native in ("1", "0"):
        monkeypatch.setenv("DFOL_NATIVE", native)
        pbs = (collater or TableCollater(split, ont, "X")).collate([dict(q) for q in qs])
        for pb in pbs:
            pb.create_sparse_tensors()
        pbs = [pb.to_cuda(DEV) for pb in pbs]
        _lib.PATH_COUNTS.clear()
        with torch.no_grad():
            out.append(model(pbs, False, **kw))
        counts = dict(_lib.PATH_COUNTS)
        if native == "1":
            assert counts.get("native_program", 0) == len(pbs) and not counts.get("python_program") and not counts.get("fallback:trainable_gate"), counts
        else:
            assert counts.get("python_program", 0) == len(pbs) and not counts.get("native_program") and not counts.get("fallback:trainable_gate"), counts
    return out


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_executor_equals_python_loop(gated, kind, monkeypatch):
    """Every terminal operator family of tests/test_native_gpu.py on a ragged batch of 1..24-object scenes, two ProgramBatches."""
    model, ont, names, categories = gated
    qs = syn.full_size_questions(kind, 8, 1, 24, names, categories, 1200 + ALL_KINDS.index(kind))
    qs[0]["scene"] = syn.feature_scene(qs[0]["question_id"], 1, 2048)            # one image of ONE object for sure
    qs[1]["scene"] = syn.feature_scene(qs[1]["question_id"], 24, 2048)
    nat, py = routes(model, qs, monkeypatch, split=2, ont=ont)
    same_results(nat, py, "gated " + kind)
    assert bool(torch.isfinite(nat["log_probability"]).all())


def test_relate_with_mixed_subject_flags_and_the_gates_in_the_arithmetic(gated, models, monkeypatch):
    model, ont, names, categories = gated
    nouns, attrs, rels = names["nouns"][:4], names["attributes"][:4], names["relations"][:3]
    flags = [True, False, False, True, True, False]
    qs = [syn.question(1300 + i, [[syn.op("select", nouns[i % 4]), syn.op("filter", attrs[i % 4]), syn.op("relate", rels[i % 3], flags[i], nouns[(i + 1) % 4]),
                                   syn.op("relate", rels[i % 3], not flags[i], nouns[(i + 2) % 4])]], syn.op("exist"), "yes",
                       syn.feature_scene(1300 + i, 3 + 4 * i, 2048)) for i in range(6)]
    nat, py = routes(model, qs, monkeypatch, ont=ont)
    same_results(nat, py, "mixed subject flags")
    # the one-launch route against the generic gated route (switch unset: today's route): the policy's slack, not bits
    monkeypatch.delenv("DFOL_GATE_NATIVE")
    monkeypatch.setenv("DFOL_NATIVE", "0")
    pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ont, "X").collate([dict(q) for q in qs])]
    with torch.no_grad():
        generic = model(pbs, False)
        plain = models[0][False][0](pbs, False)
    assert generic["answer"] == nat["answer"]
    assert (torch.exp(generic["log_probability"]) - torch.exp(nat["log_probability"])).abs().max().item() <= 1e-5
    assert not torch.equal(plain["log_probability"], nat["log_probability"])


@pytest.mark.parametrize("name", sorted(TG.IM["forward"]))
def test_g25_interpreter_forward_on_the_executor(mini_ontology, name, monkeypatch):
    """The reference's own gated interpreter runs (exist / verify_rel / query_attr / choose_rel) with the switch on: its answers exactly, its
    log-probabilities under the policy, on the executor."""
    fm = TG.IM["forward"][name]
    model = TG.golden_model(mini_ontology).eval()
    pbs, _ = TG.golden_batches(mini_ontology, "fwd", name, fm["questions"])
    monkeypatch.setenv("DFOL_GATE_NATIVE", "1")
    monkeypatch.setenv("DFOL_NATIVE", "1")
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        res = model(pbs, False)
    assert _lib.PATH_COUNTS.get("native_program", 0) == 1 and not _lib.PATH_COUNTS.get("python_program"), dict(_lib.PATH_COUNTS)
    lp = res["log_probability"].cpu().numpy()
    print(name, "lp", lp, "reference fp64", TG.IA["fwd:%s:lp_f64" % name])
    U.check_logprob(lp, TG.IA["fwd:%s:lp_f32" % name], TG.IA["fwd:%s:lp_f64" % name], "g25 on the executor " + name)
    assert [list(a) if isinstance(a, (list, tuple)) else a for a in res["answer"]] == fm["answer_f64"], (res["answer"], fm["answer_f64"])
    assert int(res["type"]) == fm["type"]


def forward(model, pbs, native, monkeypatch):
    monkeypatch.setenv("DFOL_NATIVE", native)
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        lp = model(pbs, False)["log_probability"].clone()
    assert _lib.PATH_COUNTS.get("native_program", 0) == (len(pbs) if native == "1" else 0)
    return lp


def test_fresh_gates_after_an_in_place_change_and_after_a_train_step(gated, monkeypatch):
    from dfol_vqa_amd import parallel, training
    base, ont, names, categories = gated
    monkeypatch.setenv("DFOL_GATE_NATIVE", "1")
    base.__dict__.pop("_native_model", None)                      # (the C view of the weights is per model: the copy builds its own)
    model = copy.deepcopy(base).eval()
    pbs = TG.batches(ont, names, first=60)
    before = forward(model, pbs, "1", monkeypatch)
    p = dict(model.named_parameters())["_ops.relate._relate._blc._nlg.1._linear.weight"]
    p.data.add_(0.25)                                             # (through .data: the parameter's version does not move)
    after = forward(model, pbs, "1", monkeypatch)
    ref = forward(model, pbs, "0", monkeypatch)
    assert not torch.equal(before, after) and torch.equal(after, ref)
    # one optimiser step on the gates alone
    model.train()
    for k, q in model.named_parameters():
        q.requires_grad_("_nlg" in k)
    params = [q for q in model.parameters() if q.requires_grad]
    opt = torch.optim.Adam(params, lr=1e-2, capturable=True)
    training.train_batch(model, opt, pbs, 0.65, bucket=parallel.GradBucket(params), sync_loss=False)
    torch.cuda.synchronize()
    model.eval()
    stepped = forward(model, pbs, "1", monkeypatch)
    ref = forward(model, pbs, "0", monkeypatch)
    assert not torch.equal(stepped, after) and torch.equal(stepped, ref)


@pytest.mark.parametrize("kind", ["exist", "verify_rel", "choose_rel", "query_attr"])
def test_calibrated_gated_model_stays_on_the_executor(tmp_path_factory, kind, monkeypatch):
    """activate_attention_transfer with trainable gates, per question and on shared scenes: the modulation follows the cell, whatever its gate."""
    key = "calibrated"
    if key not in _CACHE:
        from dfol_vqa_amd import experiment
        paths, names = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("gate_calib")))
        cfg = syn.reference_config(paths, activate_attention_transfer=True, trainable_gate=True)
        ont = experiment.build_ontology(cfg)
        torch.manual_seed(5)
        model = experiment.build_model(cfg, ont)
        syn.load_seeded_weights(model, 23)
        with torch.no_grad():                                      # (the reference initialises the output layer's weight to zero)
            out = model._ops['filter']._filter._attention_output_network[0]
            out.weight.normal_(0.0, 0.5)
            out.bias.normal_(0.0, 0.5)
        distinct_gates(model)
        with open(paths["attribute_file"]) as f:
            categories = json.load(f)
        _CACHE[key] = (model.to(DEV).eval(), ont, names, categories)
    model, ont, names, categories = _CACHE[key]
    assert model._has_modulator and native_exec.calibrator(model) is not None and native_exec.gate_slots(model)
    qs = syn.full_size_questions(kind, 8, 1, 24, names, categories, 1400 + ALL_KINDS.index(kind))
    nat, py = routes(model, qs, monkeypatch, collater=_FullCalibrationCollater(1, ont))
    same_results(nat, py, "calibrated gated " + kind)
    for i, q in enumerate(qs):
        q["image_id"], q["scene"] = "img%d" % (i % 3), qs[i % 3]["scene"]
    nat2, py2 = routes(model, qs, monkeypatch, collater=_FullCalibrationCollater(1, ont, share=True))
    same_results(nat2, py2, "calibrated gated shared " + kind)
    off, _ = routes(model, qs, monkeypatch, collater=_FullCalibrationCollater(1, ont, share=True), modulator_switch=False)
    assert not torch.equal(off["log_probability"], nat2["log_probability"])        # the calibrator is not the identity


def test_graphed_forward_of_a_gated_model_with_the_switch_on(gated, monkeypatch):
    from dfol_vqa_amd.interpreter import GraphedForward
    model, ont, names, categories = gated
    monkeypatch.setenv("DFOL_GATE_NATIVE", "1")
    monkeypatch.setenv("DFOL_NATIVE", "1")
    pbs = TG.batches(ont, names)
    with torch.no_grad():
        eager = model(pbs, False)
    r = GraphedForward(model, pbs)()
    assert np.array_equal(TG.bits(r["log_probability"]), TG.bits(eager["log_probability"])) and r["answer"] == eager["answer"]


def test_refusals(monkeypatch):
    """Neither reaches a launch: the wrapper refuses a bf16 tile, dfol_run_program a gated opcode without (or beyond) its gate table."""
    op = one_problem("ns8_lone")
    with pytest.raises(_lib.DfolError):
        run_one(op, tile=dev(op["T"]).to(torch.bfloat16))
    NS, P = 4, 1
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    blob = torch.zeros(256, dtype=torch.uint8, device=DEV)                      # pred_q = [0] at 0, n_obj = [0] at 16: nothing would be computed
    model, scene = native_exec.ProgramModel(), native_exec.ProgramScene()
    scene.NS, scene.O, scene.max_n, scene.n_obj, scene.img_n_obj, scene.obj_off = NS, 0, 0, 16, 16, 32
    table = torch.zeros(2, 18, device=DEV)
    rows = {NP.OP_FILTER_GATE: [NP.OP_FILTER_GATE, 0, 256, 0, -1, -1, P, 512, 0],
            NP.OP_RELATE_ONE_GATE: [NP.OP_RELATE_ONE_GATE, 0, 256, 1024, 0, 48, -1, -1, P, 0, 512, NP.TILE_F32, 64, 0],
            NP.OP_RELATE_GATE: [NP.OP_RELATE_GATE, 0, 256, 1024, 0, 48, 48, -1, -1, -1, P, NP.TILE_SUBJECT_ROWS, 0, 512, 768, 0]}

    def run(row, gates=None, slot=0):
        row = list(row)
        row[{NP.OP_FILTER_GATE: 8, NP.OP_RELATE_ONE_GATE: 13, NP.OP_RELATE_GATE: 15}[row[0]]] = slot
        instr = np.zeros((1, NP.INSTR_WIDTH), np.int64)
        instr[0, :len(row)] = row
        model.gates, model.n_gates = (None, 0) if gates is None else (gates.data_ptr(), gates.shape[0])
        _lib.call("dfol_run_program", ctypes.byref(model), ctypes.byref(scene), instr.ctypes.data, 1, blob.data_ptr(), ws.data_ptr(), _lib._stream())

    for opcode, row in rows.items():
        with pytest.raises(_lib.DfolError, match="gate slot"):
            run(row)                                              # no table
        with pytest.raises(_lib.DfolError, match="gate slot"):
            run(row, table, slot=2 if opcode == NP.OP_FILTER_GATE else 1)       # beyond the table (an arity-2 cell needs slot + 1 as well)
        with pytest.raises(_lib.DfolError, match="gate slot"):
            run(row)                                              # after a refused run WITH a table, a model struct that carries none: nothing lingers
    torch.cuda.synchronize()                                      # nothing was launched, nothing faulted
    assert not ws.any().item()
