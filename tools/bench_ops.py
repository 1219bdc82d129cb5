#!/usr/bin/env python3
"""Forward throughput per terminal operator (BASELINE configs[2] shape: ragged N <= 100, the full operator set), one GPU.

usage: python tools/bench_ops.py [--batch 256] [--nmin 10] [--nmax 100] [--steps 5]
One JSON line per operator kind: questions/s of a batch of `--batch` programs  select -> filter -> relate -> <terminal op>.

       python tools/bench_ops.py --trainable-gate [--batch 256] [--nmax 100] [--rounds 15] [--reps 20] [--out FILE]
The logic cell's launches with and without the trainable gate (`trainable_gate: True`, csrc/dfol_logic_gate.hip): filter and relate, forward and
backward, at `--batch` predicates x `--nmax` objects, gated and ungated alternating in one process (every round times each of the eight
launches over `--reps` back-to-back launches between two events); one JSON line per launch with the median, minimum and maximum over the rounds.
Then two legs for the gated model's fast inference path (DFOL_GATE_NATIVE=1): the one-launch gated Relate against the sequence it replaces
(gate, gate, relate_gate_fwd under `want`, gate), and a stream of unseen gated batches on the native executor against the same stream on the
Python operator loop (switch unset), each alternating in one process.
Then two legs for the gated train step (DFOL_GATE_TRAIN=1; `--gate-train-only` runs these alone): the one-posterior forward and backward
launches against the sequence and the autograd backward they replace, and a whole gated train step, eager and replayed, with the switch unset
and set, on the one-hop program and on ragged 1..3-hop programs.
Then one leg for the gated model over bf16 relation tiles (DFOL_GATE_BF16=1; `--gate-bf16-only` runs it alone): the one-launch gated Relate on
bf16 tiles against the same launch on fp32 tiles, at `--batch` predicates x `--nmax` objects and x 256 objects (BASELINE configs[4]'s size), with
the tile bytes of both.

       python tools/bench_ops.py --relate-train-only [--relate-train-unset] [--batch 256] [--nmax 100] [--rounds 15] [--reps 20] [--out FILE]
The ungated train step's one-posterior Relate (DFOL_RELATE_TRAIN=1): the forward and the backward launch against the generic sequence and its
autograd backward, then a whole train step, eager and replayed, with the switch unset and set, on the one-hop program and on ragged 1..3-hop
programs, all alternating in one process.  `--relate-train-unset` times the unset step alone (a tree from before the switch runs it too).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

KINDS = ["exist", "verify_attrs", "verify_rel", "choose_attr", "choose_rel", "query_attr", "and", "or", "two_same", "two_different",
         "all_same", "all_different", "compare"]


def questions(kind, count, nmin, nmax, names, seed):
    from dfol_vqa_amd import synthetic as syn
    rng = np.random.RandomState(seed)
    nouns, attrs, rels = names["nouns"][:8], names["attributes"][:6], names["relations"][:5]
    op = syn.op
    pick = lambda xs: xs[rng.randint(len(xs))]
    qs = []
    for i in range(count):
        qid = seed * 100000 + i
        b1 = [op("select", pick(nouns)), op("filter", pick(attrs)), op("relate", pick(rels), bool(rng.uniform() < 0.5), pick(nouns))]
        branches = [b1]
        if kind in ("and", "or", "two_same", "two_different", "compare"):
            branches.append([op("select", pick(nouns)), op("filter", pick(attrs))])
        last = {"exist": op("exist"), "and": op("and"), "or": op("or"), "verify_attrs": op("verify_attrs", [pick(attrs), pick(attrs)]),
                "verify_rel": op("verify_rel", pick(rels), bool(rng.uniform() < 0.5), pick(nouns)),
                "choose_attr": op("choose_attr", [attrs[0], attrs[1]]), "query_attr": op("query_attr", "category%02d" % rng.randint(3)),
                "choose_rel": op("choose_rel", [rels[0], rels[1]], bool(rng.uniform() < 0.5), pick(nouns)),
                "two_same": op("two_same", "category00"), "two_different": op("two_different", "category01"),
                "all_same": op("all_same", "category02"), "all_different": op("all_different", "category00"),
                "compare": op("compare", pick(attrs), bool(rng.uniform() < 0.5))}[kind]
        n = int(rng.randint(nmin, nmax + 1))
        qs.append(syn.question(qid, branches, last, "yes", syn.feature_scene(qid, n, 2048)))
    return qs


def trainable_gate_launches(args):
    """The eight launches of the logic cell, gated and ungated, alternating."""
    from dfol_vqa_amd import _lib as L
    from dfol_vqa_amd import synthetic as syn
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(17)
    P, n = args.batch, args.nmax
    NS = (n + 3) // 4 * 4
    t = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    ll, tile = np.full((P, NS), -30, np.float32), np.full((P, NS, NS), -30, np.float32)
    ll[:, :n] = syn.table_log_likelihood(rng, (P, n), "mix10")
    tile[:, :n, :n] = syn.table_log_likelihood(rng, (P, n, n), "mix10")
    tile[:, np.arange(n), np.arange(n)] = -30
    prior = np.zeros((P, NS), np.float32)
    prior[:, :n] = -rng.uniform(0.01, 2.0, (P, n))
    pa, pb, ll, tile = t(prior), t(prior[::-1]), t(ll), t(tile)
    pq, n_obj = t(np.arange(P), torch.int32), t(np.full(P, n), torch.int32)
    pq._dfol_sorted = True
    ones = t(np.ones(P))
    gs, go = (L.gate_params(t(rng.uniform(-0.7, 0.7, (6, 2))), t(rng.uniform(-0.7, 0.7, 6))) for _ in range(2))
    g1, g2 = t(rng.normal(size=(P, NS))), t(rng.normal(size=(P, NS)))
    launches = [
        ("filter_fwd", lambda: L.filter_fwd(pa, ll, pq, n_obj)),
        ("filter_gate_fwd", lambda: L.filter_gate_fwd(pa, ll, pq, n_obj, gs)),
        ("relate_fwd", lambda: L.relate_fwd(pa, pb, tile, pq, n_obj, ones, ones)),
        ("relate_gate_fwd", lambda: L.relate_gate_fwd(pa, pb, tile, pq, n_obj, ones, ones, gs, go)),
        ("filter_bwd", lambda: L.filter_bwd(g1, ll, pq, n_obj, None, None, P)),
        ("filter_gate_bwd", lambda: L.filter_gate_bwd(g1, pa, ll, pq, n_obj, gs, None, None)),
        ("relate_bwd", lambda: L.relate_bwd(pa, pb, tile, pq, n_obj, ones, ones, None, None, g1, g2, L.TILE_SUBJECT_ROWS, False)),
        ("relate_gate_bwd", lambda: L.relate_gate_bwd(pa, pb, tile, pq, n_obj, ones, ones, gs, go, None, None, g1, g2, L.TILE_SUBJECT_ROWS, False)),
    ]
    if args.gate_bf16_only:                                    # the bf16-tile leg alone
        lines = gated_relate_one_bf16(args)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if args.gate_train_only:                                   # the two legs of the gated train step alone
        lines = gated_train_launches(args, L, t, rng, pa, pb, tile, pq, n_obj, ones, gs, go)
        lines += gated_train_step(args) + gated_train_step(args, hops="ragged")
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    for _, fn in launches:                                     # (the first launches of a kernel load its code object)
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in launches}
    for _ in range(args.rounds):
        for name, fn in launches:                              # gated and ungated side by side in every round
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.reps)
    lines = []
    for name, _ in launches:
        v = np.sort(np.asarray(times[name]))
        lines.append(json.dumps({"launch": name, "predicates": P, "objects": n, "us_median": float(np.median(v)), "us_min": float(v[0]),
                                 "us_max": float(v[-1]), "rounds": args.rounds, "reps": args.reps,
                                 "note": "backward entries include their reduce-by-question launches; host-side allocation of the outputs is inside the timed region"}))
        print(lines[-1], flush=True)
    lines += gated_relate_one(args, L, t, rng, pa, pb, tile, pq, n_obj, ones, gs, go)
    lines += gated_stream(args)
    lines += gated_train_launches(args, L, t, rng, pa, pb, tile, pq, n_obj, ones, gs, go)
    lines += gated_train_step(args) + gated_train_step(args, hops="ragged")
    lines += gated_relate_one_bf16(args)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def _summary(what, times, **more):
    v = np.sort(np.asarray(times))
    line = json.dumps(dict({"launch": what, "us_median": float(np.median(v)), "us_min": float(v[0]), "us_max": float(v[-1])}, **more))
    print(line, flush=True)
    return line


def gated_relate_one(args, L, t, rng, x, prev, tile, pq, n_obj, ones, gs, go):
    """The one-launch gated Relate (dfol_relate_one_gate_fwd_f32, DFOL_GATE_NATIVE=1) against the sequence a gated relate hop runs without it:
    gate, gate, relate_gate_fwd under `want`, gate - alternating in one process, medians over the rounds.  (The upload of `want` is memoised
    by content in the interpreter and is left out.)"""
    P = tile.shape[0]
    flag = (np.arange(P) % 2).astype(np.float32)                 # subject flags mixed over the batch
    flag_f, flag_u8 = t(flag), t(flag, torch.uint8)
    want = t(np.where(flag > 0, L.WANT_SUBJECT, L.WANT_OBJECT), torch.uint8)
    oriented = torch.where(flag_f.view(-1, 1, 1) > 0, tile.transpose(1, 2), tile).contiguous()      # the summed-out variable (prev) along rows

    def sequence():
        s, q_s = L.gate(x, prev, ones, ones, flag_f)
        o, q_o = L.gate(prev, x, ones, ones, flag_f)
        ps, po = L.relate_gate_fwd(s, o, tile, pq, n_obj, q_s, q_o, gs, go, None, None, want, diag_absent=True)
        return L.gate(ps, po, q_s, q_s, flag_f)[0]

    def one():
        return L.relate_one_gate_fwd(x, prev, oriented, pq, n_obj, ones, flag_u8, gs, go)

    a, b = sequence(), one()
    gap = float((torch.exp(a) - torch.exp(b)).abs().max())
    assert gap <= 1e-5, gap                                      # the same posterior (another summation order)
    launches = [("relate_gate_sequence(gate,gate,relate_gate_fwd,gate)", sequence), ("relate_one_gate_fwd", one)]
    times = {name: [] for name, _ in launches}
    for _ in range(args.rounds):
        for name, fn in launches:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.reps)
    more = dict(predicates=P, objects=args.nmax, rounds=args.rounds, reps=args.reps, max_abs_probability_gap=gap)
    lines = [_summary(name, times[name], **more) for name, _ in launches]
    ratio = float(np.median(times[launches[0][0]]) / np.median(times[launches[1][0]]))
    lines.append(json.dumps({"ratio": "sequence / one launch (medians)", "value": ratio}))
    print(lines[-1], flush=True)
    return lines


def gated_relate_one_bf16(args):
    """The one-launch gated Relate on bf16 tiles (dfol_relate_one_gate_fwd_bf16, DFOL_GATE_BF16=1) against the same launch on fp32 tiles
    (dfol_relate_one_gate_fwd_f32 over the widened values, so both compute the same posterior), alternating in one process: `--batch` predicates
    at `--nmax` objects and at 256 objects.  The gated cell is bound by its sigmoids, not by the tile stream: what bf16 storage buys is the tile
    bytes, reported beside the times.  `ranges_apart` false: no separated difference between the two launches."""
    from dfol_vqa_amd import _lib as L
    from dfol_vqa_amd import synthetic as syn
    dev = torch.device("cuda", 0)
    t = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    lines = []
    for n in (args.nmax, 256):
        rng = np.random.RandomState(1000 + n)
        P, NS = args.batch, (n + 7) // 8 * 8
        tile = np.full((P, NS, NS), -30, np.float32)
        tile[:, :n, :n] = syn.table_log_likelihood(rng, (P, n, n), "mix10")
        tile[:, np.arange(n), np.arange(n)] = -30
        prior = np.zeros((P, NS), np.float32)
        prior[:, :n] = -rng.uniform(0.01, 2.0, (P, n))
        x, prev = t(prior), t(prior[::-1])
        t16 = t(tile).to(torch.bfloat16)
        t32 = t16.to(torch.float32)                              # the widened values: the fp32 launch reads what the bf16 launch reads
        pq, n_obj, ones = t(np.arange(P), torch.int32), t(np.full(P, n), torch.int32), t(np.ones(P))
        flag = t(np.arange(P) % 2, torch.uint8)                  # subject flags mixed over the batch
        gs, go = (L.gate_params(t(rng.uniform(-0.7, 0.7, (6, 2))), t(rng.uniform(-0.7, 0.7, 6))) for _ in range(2))
        launches = [("relate_one_gate_fwd (fp32 tiles)", lambda: L.relate_one_gate_fwd(x, prev, t32, pq, n_obj, ones, flag, gs, go)),
                    ("relate_one_gate_fwd_bf16 (bf16 tiles)", lambda: L.relate_one_gate_fwd_bf16(x, prev, t16, pq, n_obj, ones, flag, gs, go))]
        gap = float((torch.exp(launches[0][1]()) - torch.exp(launches[1][1]())).abs().max())
        assert gap <= 1e-5, gap                                  # the same posterior (another summation order)
        for _, fn in launches:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in launches}
        for r in range(args.rounds):
            for name, fn in (launches if r % 2 == 0 else launches[::-1]):      # (who goes first alternates)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(args.reps):
                    fn()
                e.record()
                e.synchronize()
                times[name].append(s.elapsed_time(e) * 1e3 / args.reps)
        for (name, _), tl in zip(launches, (t32, t16)):
            lines.append(_summary(name, times[name], predicates=P, objects=n, NS=NS, tile_bytes=int(tl.numel() * tl.element_size()), rounds=args.rounds,
                                  reps=args.reps, max_abs_probability_gap=gap,
                                  note="event time over back-to-back calls of the Python wrappers: host-side allocation of the output is inside"))
        a, b = np.asarray(times[launches[0][0]]), np.asarray(times[launches[1][0]])
        lines.append(json.dumps({"ratio": "fp32 tiles / bf16 tiles (medians), %d x %d" % (P, n), "value": float(np.median(a) / np.median(b)),
                                 "ranges_apart": bool(a.min() > b.max() or b.min() > a.max())}))
        print(lines[-1], flush=True)
    return lines


def gated_train_launches(args, L, t, rng, x, prev, tile, pq, n_obj, ones, gs, go):
    """The one-posterior gated Relate under autograd (dfol_relate_keep_gate_fwd_f32 / _bwd_f32, DFOL_GATE_TRAIN=1) against the sequence a gated
    relate hop runs without it - forward: gate, gate, relate_gate_fwd under `want`, gate; backward: that sequence's autograd backward - on the
    subject-row tile with mixed subject flags, through the Python wrappers, alternating in one process.  A backward is timed as
    torch.autograd.grad over a retained graph, so the forward is not inside it."""
    from dfol_vqa_amd import ops
    P = tile.shape[0]
    flag = (np.arange(P) % 2).astype(np.float32)
    flag_f, flag_u8 = t(flag), t(flag, torch.uint8)
    want = t(np.where(flag > 0, L.WANT_SUBJECT, L.WANT_OBJECT), torch.uint8)
    pq._dfol_identity = True                                     # (what BatchWorld marks its identity map with: no reduction by question)
    leaf = lambda a: a.detach().clone().requires_grad_(True)
    xg, pg, tg = leaf(x), leaf(prev), leaf(tile)
    w = [leaf(gs[:12].view(6, 2)), leaf(gs[12:]), leaf(go[:12].view(6, 2)), leaf(go[12:])]
    leaves = [xg, pg, tg] + w
    cot = t(rng.normal(size=tuple(x.shape)))

    def sequence(a=x, b=prev, c=tile, gates=(gs[:12].view(6, 2), gs[12:], go[:12].view(6, 2), go[12:])):
        s, q_s = ops.gate(a, b, ones, ones, flag_f)
        o, q_o = ops.gate(b, a, ones, ones, flag_f)
        ps, po = ops.relate_gate_fwd(s, o, c, pq, n_obj, q_s, q_o, *gates, None, None, want, diag_absent=True)
        return ops.gate(ps, po, q_s, q_s, flag_f)[0]

    def one(a=x, b=prev, c=tile, gates=(gs[:12].view(6, 2), gs[12:], go[:12].view(6, 2), go[12:])):
        return ops.relate_keep_gate(a, b, c, pq, n_obj, ones, flag_u8, *gates)

    with torch.no_grad():
        gap = float((torch.exp(sequence()) - torch.exp(one())).abs().max())
    assert gap <= 1e-5, gap
    out_seq, out_one = sequence(xg, pg, tg, w), one(xg, pg, tg, w)
    g_seq = torch.autograd.grad(out_seq, leaves, cot, retain_graph=True)
    g_one = torch.autograd.grad(out_one, leaves, cot, retain_graph=True)
    grad_gap = max(float((a - b).abs().max() / max(1e-30, float(a.abs().max()))) for a, b in zip(g_seq, g_one))
    assert grad_gap <= 2e-3, grad_gap                            # the same gradients (another summation order), relative to each tensor's scale

    def fwd_seq():
        with torch.no_grad():
            sequence()

    def fwd_one():
        with torch.no_grad():
            one()

    launches = [("train forward, sequence(gate,gate,relate_gate_fwd,gate)", fwd_seq),
                ("train forward, relate_keep_gate_fwd", fwd_one),
                ("train backward, autograd of the sequence", lambda: torch.autograd.grad(out_seq, leaves, cot, retain_graph=True)),
                ("train backward, relate_keep_gate_bwd", lambda: torch.autograd.grad(out_one, leaves, cot, retain_graph=True))]
    for _, fn in launches:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in launches}
    for _ in range(args.rounds):
        for name, fn in launches:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.reps)
    more = dict(predicates=P, objects=args.nmax, rounds=args.rounds, reps=args.reps, max_abs_probability_gap=gap, max_rel_gradient_gap=grad_gap,
                note="event time over back-to-back calls of the Python wrappers: host-side allocation and autograd bookkeeping are inside")
    lines = [_summary(name, times[name], **more) for name, _ in launches]
    for a, b, what in ((0, 1, "forward"), (2, 3, "backward")):
        ta, tb = np.asarray(times[launches[a][0]]), np.asarray(times[launches[b][0]])
        lines.append(json.dumps({"ratio": "train %s: sequence / one launch (medians)" % what, "value": float(np.median(ta) / np.median(tb)),
                                 "ranges_apart": bool(ta.min() > tb.max() or tb.min() > ta.max())}))
        print(lines[-1], flush=True)
    return lines


def gated_train_step(args, hops="aligned"):
    """A gated train step (zero grads -> forward -> loss -> backward -> clip -> Adam; every parameter trains) on bench.py's one-hop program
    (select -> filter -> relate -> exist) or its ragged 1..3-hop programs, eager and replayed (GraphedTrainStep), with DFOL_GATE_TRAIN unset and
    set: four variants alternating in one process, each on its own copy of the model, wall time per step with a device synchronisation."""
    import copy
    from dfol_vqa_amd import _lib, experiment, parallel, training
    from dfol_vqa_amd import synthetic as syn
    device = torch.device("cuda", 0)
    paths, names = syn.write_synthetic_ontology(tempfile.mkdtemp(prefix="dfol_gate_train_"))
    cfg = syn.reference_config(paths, trainable_gate=True, dropout=0.0, freeze_featurizer=False, freeze_attribute_network=False,
                               freeze_relation_network=False, freeze_embedding_network=False)      # bench.py --mode train's oracle-training phases
    ontology = experiment.build_ontology(cfg)
    torch.manual_seed(0)
    base = experiment.build_model(cfg, ontology)
    bench.init_weights(base)
    base = base.to(device).train()
    shape = argparse.Namespace(batch=args.batch, objects=args.nmax, ragged=0, hops=hops, workload="north_star", questions_per_image=1, share_scenes=1)
    _, pbs = bench.build_batch(shape, 0, ontology, names, device)
    variants, counts = {}, {}
    for switch in ("0", "1"):
        os.environ["DFOL_GATE_TRAIN"] = switch
        for graphed in (False, True):
            model = copy.deepcopy(base)
            params = [p for p in model.parameters() if p.requires_grad]
            opt = torch.optim.Adam(params, lr=1e-4, capturable=True)
            bucket = parallel.GradBucket(params)
            _lib.PATH_COUNTS.clear()
            if graphed:
                step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=2)
            else:
                step = (lambda m, o, b: (lambda: training.train_batch(m, o, pbs, 0.65, bucket=b, sync_loss=False)))(model, opt, bucket)
                step()
                step()
            torch.cuda.synchronize()
            took = _lib.PATH_COUNTS.get("relate_gate_train_one", 0)
            assert (took > 0) == (switch == "1"), (switch, graphed, took)
            variants[switch, graphed] = step
            counts[switch, graphed] = took
    order = [("0", False), ("1", False), ("0", True), ("1", True)]
    times = {k: [] for k in order}
    rounds, n = max(4, args.rounds // 2), 4
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):           # (who goes first alternates)
            os.environ["DFOL_GATE_TRAIN"] = k[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                variants[k]()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / n * 1e6)
    os.environ.pop("DFOL_GATE_TRAIN", None)
    lines = []
    for k in order:
        lines.append(_summary("gated train step, %s hops, %s, DFOL_GATE_TRAIN %s" % (hops, "replayed" if k[1] else "eager", "set" if k[0] == "1" else "unset"),
                              times[k], questions=args.batch, objects=args.nmax, rounds=rounds, steps_per_round=n,
                              relate_gate_train_one_hops_in_setup=counts[k]))
    for graphed in (False, True):
        a, b = np.asarray(times["0", graphed]), np.asarray(times["1", graphed])
        lines.append(json.dumps({"ratio": "gated train step, %s hops, %s: unset / set (medians)" % (hops, "replayed" if graphed else "eager"),
                                 "value": float(np.median(a) / np.median(b)), "ranges_apart": bool(a.min() > b.max() or b.min() > a.max())}))
        print(lines[-1], flush=True)
    return lines


def relate_train_launches(args):
    """The one-posterior Relate under autograd for the ungated model (dfol_relate_keep_fwd_f32 / dfol_relate_keep_bwd_f32, DFOL_RELATE_TRAIN=1)
    against the generic sequence an ungated relate hop runs without it - forward: gate, gate, relate_fwd under `want`, gate; backward: that
    sequence's autograd backward (dfol_relate_bwd_f32 over both directions, two _Gate.backward, the want masks, the reductions by question) - on
    the subject-row tile with mixed subject flags, through the Python wrappers, alternating in one process.  A backward is timed as
    torch.autograd.grad over a retained graph, so the forward is not inside it."""
    from dfol_vqa_amd import _lib as L
    from dfol_vqa_amd import ops
    from dfol_vqa_amd import synthetic as syn
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(17)
    P, n = args.batch, args.nmax
    NS = (n + 3) // 4 * 4
    t = lambda a, dt=torch.float32: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    tile = np.full((P, NS, NS), -30, np.float32)
    tile[:, :n, :n] = syn.table_log_likelihood(rng, (P, n, n), "mix10")
    tile[:, np.arange(n), np.arange(n)] = -30
    prior = np.zeros((P, NS), np.float32)
    prior[:, :n] = -rng.uniform(0.01, 2.0, (P, n))
    x, prev, tile = t(prior), t(prior[::-1]), t(tile)
    pq, n_obj, ones = t(np.arange(P), torch.int32), t(np.full(P, n), torch.int32), t(np.ones(P))
    pq._dfol_sorted = pq._dfol_identity = True                    # (what BatchWorld marks its identity map with: no reduction by question)
    flag = (np.arange(P) % 2).astype(np.float32)
    flag_f, flag_u8 = t(flag), t(flag, torch.uint8)
    want = t(np.where(flag > 0, L.WANT_SUBJECT, L.WANT_OBJECT), torch.uint8)
    leaf = lambda a: a.detach().clone().requires_grad_(True)
    leaves = [leaf(x), leaf(prev), leaf(tile)]
    cot = t(rng.normal(size=tuple(x.shape)))

    def sequence(a=x, b=prev, c=tile):
        s, q_s = ops.gate(a, b, ones, ones, flag_f)
        o, q_o = ops.gate(b, a, ones, ones, flag_f)
        ps, po = ops.relate_fwd(s, o, c, pq, n_obj, q_s, q_o, None, None, want, diag_absent=True)
        return ops.gate(ps, po, q_s, q_s, flag_f)[0]

    def one(a=x, b=prev, c=tile):
        return ops.relate_keep(a, b, c, pq, n_obj, ones, flag_u8)

    with torch.no_grad():
        gap = float((torch.exp(sequence()) - torch.exp(one())).abs().max())
    assert gap <= 1e-5, gap
    out_seq, out_one = sequence(*leaves), one(*leaves)
    g_seq = torch.autograd.grad(out_seq, leaves, cot, retain_graph=True)
    g_one = torch.autograd.grad(out_one, leaves, cot, retain_graph=True)
    grad_gap = max(float((a - b).abs().max() / max(1e-30, float(a.abs().max()))) for a, b in zip(g_seq, g_one))
    assert grad_gap <= 2e-3, grad_gap                            # the same gradients, relative to each tensor's scale

    def fwd_seq():
        with torch.no_grad():
            sequence()

    def fwd_one():
        with torch.no_grad():
            one()

    launches = [("train forward, sequence(gate,gate,relate_fwd,gate)", fwd_seq),
                ("train forward, relate_keep_fwd", fwd_one),
                ("train backward, autograd of the sequence", lambda: torch.autograd.grad(out_seq, leaves, cot, retain_graph=True)),
                ("train backward, relate_keep_bwd", lambda: torch.autograd.grad(out_one, leaves, cot, retain_graph=True))]
    for _, fn in launches:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in launches}
    for _ in range(args.rounds):
        for name, fn in launches:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.reps)
    more = dict(predicates=P, objects=n, rounds=args.rounds, reps=args.reps, max_abs_probability_gap=gap, max_rel_gradient_gap=grad_gap,
                note="event time over back-to-back calls of the Python wrappers: host-side allocation and autograd bookkeeping are inside")
    lines = [_summary(name, times[name], **more) for name, _ in launches]
    for a, b, what in ((0, 1, "forward"), (2, 3, "backward")):
        ta, tb = np.asarray(times[launches[a][0]]), np.asarray(times[launches[b][0]])
        lines.append(json.dumps({"ratio": "train %s: sequence / one launch (medians)" % what, "value": float(np.median(ta) / np.median(tb)),
                                 "ranges_apart": bool(ta.min() > tb.max() or tb.min() > ta.max())}))
        print(lines[-1], flush=True)
    return lines


def relate_train_step(args, hops="aligned", switches=("0", "1")):
    """An ungated train step (zero grads -> forward -> loss -> backward -> clip -> Adam; the oracle and the featurizer train, as bench.py --mode
    train) on bench.py's one-hop program (select -> filter -> relate -> exist) or its ragged 1..3-hop programs, eager and replayed
    (GraphedTrainStep), with DFOL_RELATE_TRAIN unset and set: the variants alternate in one process, each on its own copy of the model, wall time
    per step with a device synchronisation per round.  switches=("0",): the unset variants alone - what a tree without the switch can run, for
    the parent commit's step in the same session."""
    import copy
    from dfol_vqa_amd import _lib, experiment, parallel, training
    from dfol_vqa_amd import synthetic as syn
    device = torch.device("cuda", 0)
    paths, names = syn.write_synthetic_ontology(tempfile.mkdtemp(prefix="dfol_relate_train_"))
    cfg = syn.reference_config(paths, dropout=0.0, freeze_featurizer=False, freeze_attribute_network=False, freeze_relation_network=False,
                               freeze_embedding_network=False)      # bench.py --mode train's oracle-training phases
    ontology = experiment.build_ontology(cfg)
    torch.manual_seed(0)
    base = experiment.build_model(cfg, ontology)
    bench.init_weights(base)
    base = base.to(device).train()
    shape = argparse.Namespace(batch=args.batch, objects=args.nmax, ragged=0, hops=hops, workload="north_star", questions_per_image=1, share_scenes=1)
    _, pbs = bench.build_batch(shape, 0, ontology, names, device)
    variants, counts = {}, {}
    for switch in switches:
        os.environ["DFOL_RELATE_TRAIN"] = switch
        for graphed in (False, True):
            model = copy.deepcopy(base)
            params = [p for p in model.parameters() if p.requires_grad]
            opt = torch.optim.Adam(params, lr=1e-4, capturable=True)
            bucket = parallel.GradBucket(params)
            _lib.PATH_COUNTS.clear()
            if graphed:
                step = training.GraphedTrainStep(model, opt, pbs, 0.65, bucket=bucket, warmup=2)
            else:
                step = (lambda m, o, b: (lambda: training.train_batch(m, o, pbs, 0.65, bucket=b, sync_loss=False)))(model, opt, bucket)
                step()
                step()
            torch.cuda.synchronize()
            took = _lib.PATH_COUNTS.get("relate_train_one", 0)
            assert (took > 0) == (switch == "1"), (switch, graphed, took)
            variants[switch, graphed] = step
            counts[switch, graphed] = took
    order = [(s, g) for g in (False, True) for s in switches]
    times = {k: [] for k in order}
    rounds, n = max(4, args.rounds // 2), 4
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):           # (who goes first alternates)
            os.environ["DFOL_RELATE_TRAIN"] = k[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                variants[k]()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / n * 1e6)
    os.environ.pop("DFOL_RELATE_TRAIN", None)
    lines = []
    for k in order:
        lines.append(_summary("train step, %s hops, %s, DFOL_RELATE_TRAIN %s" % (hops, "replayed" if k[1] else "eager", "set" if k[0] == "1" else "unset"),
                              times[k], questions=args.batch, objects=args.nmax, rounds=rounds, steps_per_round=n,
                              relate_train_one_hops_in_setup=counts[k]))
    for graphed in (False, True) if len(switches) == 2 else ():
        a, b = np.asarray(times["0", graphed]), np.asarray(times["1", graphed])
        lines.append(json.dumps({"ratio": "train step, %s hops, %s: unset / set (medians)" % (hops, "replayed" if graphed else "eager"),
                                 "value": float(np.median(a) / np.median(b)), "ranges_apart": bool(a.min() > b.max() or b.min() > a.max())}))
        print(lines[-1], flush=True)
    return lines


def relate_train_legs(args):
    """--relate-train-only: the launches, then the train step on the one-hop and on the ragged programs (--relate-train-unset: the step with the
    switch unset alone, no launches - the form a tree from before the switch can run)."""
    switches = ("0",) if args.relate_train_unset else ("0", "1")
    lines = [] if args.relate_train_unset else relate_train_launches(args)
    lines += relate_train_step(args, switches=switches) + relate_train_step(args, hops="ragged", switches=switches)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def gated_stream(args):
    """A stream of unseen gated batches (every batch collated afresh: no plan, no uploaded side array is reused) with DFOL_GATE_NATIVE=1 (the
    native executor; the plan is lowered at collate time, where a collate worker does it) against the same stream with the switch unset (the
    Python operator loop), alternating batch by batch in one process; per-batch wall time from enqueue to the answers on the host."""
    import dfol_vqa_amd as D
    from dfol_vqa_amd import _lib, experiment, native_exec
    from dfol_vqa_amd import synthetic as syn
    device = torch.device("cuda", 0)
    paths, names = syn.write_synthetic_ontology(tempfile.mkdtemp(prefix="dfol_gate_"))
    cfg = syn.reference_config(paths, trainable_gate=True)
    ontology = experiment.build_ontology(cfg)
    model = experiment.build_model(cfg, ontology)
    bench.init_weights(model)
    model = model.to(device).eval()
    os.environ["DFOL_GATE_NATIVE"] = "1"
    spec = native_exec.model_spec(model)
    assert spec is not None and spec.gates

    class Collater(D.ProgramCollaterBase):
        def __init__(self, spec):
            super(Collater, self).__init__("select", "relate", "filter", 1, ontology=ontology, native_spec=spec)

        def collate_object_features(self, qs):
            feats = torch.cat([torch.from_numpy(q["scene"]["X"]) for q in qs], 0)
            bi = torch.cat([torch.full((q["scene"]["n"],), i, dtype=torch.int64) for i, q in enumerate(qs)])
            return feats, bi

        def collate_meta_data(self, qs):
            return {"index": {}, "embedding": torch.zeros(1, 1)}

    kinds = ["exist", "verify_rel", "choose_rel", "query_attr"]
    times = {"1": [], "0": []}
    warm = 2
    for r in range(warm + args.rounds):
        kind = kinds[r % len(kinds)]
        for k, mode in enumerate(("1", "0") if r % 2 == 0 else ("0", "1")):          # (who goes first alternates)
            qs = questions(kind, args.batch, args.nmin, args.nmax, names, seed=5000 + 2 * r + k)
            pbs = Collater(spec if mode == "1" else None).collate(qs)
            for pb in pbs:
                pb.create_sparse_tensors()
            pbs = [pb.to_cuda(device) for pb in pbs]
            del qs
            if mode == "1":
                os.environ["DFOL_GATE_NATIVE"] = "1"
            else:
                os.environ.pop("DFOL_GATE_NATIVE", None)
            _lib.PATH_COUNTS.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                model(pbs, False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert _lib.PATH_COUNTS.get("native_program" if mode == "1" else "python_program", 0) == len(pbs), dict(_lib.PATH_COUNTS)
            if r >= warm:                                          # (the first batches of a route load its kernels' code objects)
                times[mode].append(dt * 1e6)
    os.environ.pop("DFOL_GATE_NATIVE", None)
    more = dict(batch=args.batch, objects=[args.nmin, args.nmax], batches=args.rounds, kinds=kinds)
    lines = [_summary("unseen gated batch, DFOL_GATE_NATIVE=1 (native executor)", times["1"], **more),
             _summary("unseen gated batch, switch unset (Python operator loop)", times["0"], **more)]
    lines.append(json.dumps({"ratio": "Python loop / executor (median per-batch time)", "value": float(np.median(times["0"]) / np.median(times["1"]))}))
    print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trainable-gate", action="store_true", help="time the gated and ungated logic-cell launches instead of the operator programs")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="--trainable-gate: also write the JSON lines to this file")
    ap.add_argument("--gate-train-only", action="store_true", help="--trainable-gate: only the two legs of the gated train step (DFOL_GATE_TRAIN)")
    ap.add_argument("--gate-bf16-only", action="store_true", help="--trainable-gate: only the leg of the one-launch gated Relate on bf16 tiles (DFOL_GATE_BF16)")
    ap.add_argument("--relate-train-only", action="store_true", help="only the legs of the ungated train step's one-posterior Relate (DFOL_RELATE_TRAIN)")
    ap.add_argument("--relate-train-unset", action="store_true", help="--relate-train-only: the train step with the switch unset alone")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nmin", type=int, default=10)
    ap.add_argument("--nmax", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kinds", default=",".join(KINDS))
    ap.add_argument("--graph", type=int, default=1, help="1: also time the forward replayed as a captured HIP graph")
    args = ap.parse_args()
    if args.relate_train_only:
        return relate_train_legs(args)
    if args.trainable_gate:
        return trainable_gate_launches(args)
    device = torch.device("cuda", 0)
    import dfol_vqa_amd as D
    from dfol_vqa_amd import experiment
    from dfol_vqa_amd import synthetic as syn
    tmp = tempfile.mkdtemp(prefix="dfol_ops_")
    paths, names = syn.write_synthetic_ontology(tmp)
    cfg = syn.reference_config(paths)
    ontology = experiment.build_ontology(cfg)
    model = experiment.build_model(cfg, ontology)
    bench.init_weights(model)
    model = model.to(device).eval()

    class Collater(D.ProgramCollaterBase):
        def __init__(self):
            super(Collater, self).__init__("select", "relate", "filter", 1, ontology=ontology)

        def collate_object_features(self, qs):
            feats = torch.cat([torch.from_numpy(q["scene"]["X"]) for q in qs], 0)
            bi = torch.cat([torch.full((q["scene"]["n"],), i, dtype=torch.int64) for i, q in enumerate(qs)])
            return feats, bi

        def collate_meta_data(self, qs):
            return {"index": {}, "embedding": torch.zeros(1, 1)}

    for kind in args.kinds.split(","):
        qs = questions(kind, args.batch, args.nmin, args.nmax, names, seed=1 + KINDS.index(kind))
        pbs = Collater().collate(qs)
        for pb in pbs:
            pb.create_sparse_tensors()
        pbs = [pb.to_cuda(device) for pb in pbs]
        # (a forward over 6656 predicates - query_attr - creates tens of thousands of small host objects; with the question dicts of every kind
        # alive, the collector's full passes turned that into 8.5 ms per eager step against 1.45 replayed: what a process keeps is frozen, as in bench.py)
        import gc
        gc.collect()
        gc.freeze()
        with torch.no_grad():
            for _ in range(4):                                 # (the first launches of a kernel variant load its code object)
                res = model(pbs, False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                res = model(pbs, False)
            torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        out = {"operator": kind, "questions_per_s": args.batch / dt, "ms_per_step": dt * 1e3, "batch": args.batch,
               "objects": [args.nmin, args.nmax], "predicates": int(res["log_probability"].numel())}
        if args.graph:
            from dfol_vqa_amd.interpreter import GraphedForward
            g = GraphedForward(model, pbs)
            r = g()
            assert torch.equal(r["log_probability"], res["log_probability"]) and r["answer"] == res["answer"], kind
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                g()
            torch.cuda.synchronize()
            dtg = (time.perf_counter() - t0) / args.steps
            out.update({"graph_ms_per_step": dtg * 1e3, "graph_questions_per_s": args.batch / dtg})
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
