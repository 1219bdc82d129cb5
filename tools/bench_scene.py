"""Scene-graph supervision: the fused weighted BCE (ops.scene_bce, csrc/dfol_scene.hip) against the tensor-op route of the same function
(embedding rows gathered, linear_act with LogSigmoid, exp, binary_cross_entropy, autograd), forward and forward + backward.

    python tools/bench_scene.py --M 25600 --H 300 --C 2002
    python tools/bench_scene.py --M 2560 --H 300 --C 333

The two routes alternate inside one process, --runs times (default 5); each run times --iters steps between two events after --warmup
steps and reports the mean per step.  Printed: one JSON line with the range (min, max) over the runs per route and leg, and the peak device
memory of each route above what the inputs hold.  Ranges that overlap show no difference.

    python tools/bench_scene.py --leg pair-rows --M 25600            # the listed pairs' rows: the two kernels of csrc/dfol_scene_pairs.hip against
                                                                     # the tensor-op expression and its autograd backward, P = M pairs, D = --D
    python tools/bench_scene.py --leg step --M 25600 --images 1000   # a whole scene train step (full-size model, synthetic ontology, dropout
                                                                     # --dropout) over about M objects and M listed pairs in --images images:
                                                                     # eager on the unprepared batch, eager on the prepared batch
                                                                     # (data.prepare_scene_batch), and the captured replay (GraphedTrainStep)"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def tensor_route(L, h, emb_w, emb_b, cols, target, weight, thr):
    idx = cols.to(torch.int64)
    lp = L.linear_act(h, emb_w.index_select(0, idx).contiguous(), emb_b.index_select(0, idx).contiguous(), L.ACT_LOGSIGMOID)
    loss = torch.nn.functional.binary_cross_entropy(lp.exp(), target, weight=weight, reduction="sum")
    with torch.no_grad():
        a = (lp > thr).to(target.dtype)
        either = ((target + a) > 0).to(target.dtype)
        num, den = (weight * either * (target != a).to(target.dtype)).sum(), (weight * either).sum()
    return loss, num, den


def timed_runs(routes, runs, iters, warmup, before=None):
    """{route: [ms per step, one per run]}: the routes alternate, `runs` times; each run is `warmup` calls, then `iters` between two events."""
    times = {r: [] for r in routes}
    for _ in range(runs):
        for r, fn in routes.items():
            for _ in range(warmup):
                fn()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            e.synchronize()
            times[r].append(s.elapsed_time(e) / iters)
    return times


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2.0 ** 20, 1)


def pair_rows_leg(args):
    from dfol_vqa_amd import data, ops as L
    rng = np.random.RandomState(0)
    O = P = args.M
    D = args.D
    obj = torch.as_tensor(rng.normal(size=(O, D)).astype(np.float32)).cuda()
    obj[:, D - 4:] = torch.rand(O, 4, device="cuda")
    obj.requires_grad_(True)
    s, o = rng.randint(0, O, size=P).astype(np.int32), rng.randint(0, O, size=P).astype(np.int32)
    dev = lambda a: torch.as_tensor(a).cuda()
    ps, po, s64, o64 = dev(s), dev(o), dev(s.astype(np.int64)), dev(o.astype(np.int64))
    csr = tuple(dev(a) for a in data.scene_pair_csr(s, o, O))
    g = torch.randn(P, 2 * D + 4, device="cuda")
    fwd = {"hip": lambda: L.scene_pair_rows(obj, ps, po, csr), "tensor": lambda: L.scene_pair_rows_reference(obj, s64, o64)}

    def both(fn):
        def run():
            obj.grad = None
            fn().backward(g)
        return run

    def only(fn):
        def run():
            with torch.no_grad():
                fn()
        return run
    out = {"leg": "pair-rows", "O": O, "P": P, "D": D, "runs": args.runs, "iters": args.iters}
    for leg, wrap in (("fwd", only), ("fwd_bwd", both)):
        for r, v in timed_runs({r: wrap(fn) for r, fn in fwd.items()}, args.runs, args.iters, args.warmup).items():
            out["%s_%s_ms" % (r, leg)] = [round(min(v), 4), round(max(v), 4)]
    for r, fn in fwd.items():
        out["%s_peak_MiB" % r] = peak_of(both(fn))
    print(json.dumps(out))


def step_leg(args):
    import tempfile
    import dfol_vqa_amd as D
    from dfol_vqa_amd import data, experiment, parallel, training
    from dfol_vqa_amd import synthetic as syn
    dev = torch.device("cuda:0")
    paths, names = syn.write_synthetic_ontology(tempfile.mkdtemp(prefix="dfol_scene_step_"))
    unfrozen = dict(freeze_featurizer=False, freeze_attribute_network=False, freeze_relation_network=False, freeze_embedding_network=False)
    cfg = syn.reference_config(paths, dropout=args.dropout, **unfrozen)
    ont = experiment.build_ontology(cfg)

    class Collater(D.ProgramCollaterBase):
        def __init__(self):
            super(Collater, self).__init__("select", "relate", "filter", 1, ontology=ont)

        def collate_object_features(self, questions):
            feats = torch.cat([torch.from_numpy(q["scene"]["X"]) for q in questions], 0)
            bi = torch.cat([torch.full((q["scene"]["n"],), i, dtype=torch.int64) for i, q in enumerate(questions)])
            return feats, bi

        def collate_meta_data(self, questions):
            md = {"index": {}, "embedding": torch.zeros(1, 1)}
            md.update(data.scene_meta_data(questions, [q["scene"]["n"] for q in questions], ont))
            return md

    def batch(first, seed):
        """--images images of M / images objects (+- 4) and as many listed pairs, every other object named with one or two attributes."""
        rng = np.random.RandomState(seed)
        attrs, rels = names["attributes"] + names["nouns"], names["relations"]
        mean = max(2, args.M // args.images)
        qs = []
        for i in range(args.images):
            n = int(max(2, mean + rng.randint(-4, 5)))
            q = syn.question(first + i, [], syn.op("scene"), "", syn.feature_scene(first + i, n, 2048))
            s = [int(x) for x in rng.randint(0, n, size=n)]
            q["object_pairs"] = {"subject_id": s, "object_id": [int((a + 1 + rng.randint(0, n - 1)) % n) for a in s]}
            q["attribute_dict"] = {str(j): [(attrs[rng.randint(len(attrs))], 1.0) for _ in range(1 + j % 2)] for j in range(0, n, 2)}
            q["relation_list"] = [(rels[rng.randint(len(rels))], 1.0) for _ in range(n)]
            qs.append(q)
        (pb,) = Collater().collate(qs)
        return pb

    host = [batch(0, 1), batch(100000, 2)]
    O = [sum(pb._object_nums) for pb in host]
    cap = (max(O) + 63) // 64 * 64                                   # one capacity for both batches: objects and pairs (P = O here)

    def fresh():
        torch.manual_seed(0)
        model = experiment.build_model(cfg, ont)
        with torch.no_grad():
            model._oracle._embedding_network.linear.weight.normal_(0.0, 0.1)
            model._oracle._embedding_network.linear.bias.fill_(-2.0)
        model = model.to(dev).train()
        params = [p for p in model.parameters() if p.requires_grad]
        return model, torch.optim.Adam(params, lr=1e-4, capturable=True), parallel.GradBucket(params)

    # one model per route (the same initial weights): the routes alternate, none trains on another's steps
    plain = [host[0].to_cuda(dev)]
    prep = [data.prepare_scene_batch(host[0], dev, objects=cap, pairs=cap)]
    cap_pbs = [data.prepare_scene_batch(host[0], dev, objects=cap, pairs=cap)]
    m_a, o_a, b_a = fresh()
    m_b, o_b, b_b = fresh()
    m_c, o_c, b_c = fresh()
    routes = {"eager_unprepared": lambda: training.train_batch(m_a, o_a, plain, 0.65, bucket=b_a, sync_loss=False),
              "eager_prepared": lambda: training.train_batch(m_b, o_b, prep, 0.65, bucket=b_b, sync_loss=False)}
    out = {"leg": "step", "images": args.images, "O": O[0], "P": O[0], "capacity": cap, "dropout": args.dropout, "runs": args.runs, "iters": args.iters,
           "A": len(ont._attribute_index), "R": len(ont._relation_index)}
    for r in list(routes):
        out["%s_peak_MiB" % r] = peak_of(routes[r])
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    graphed = training.GraphedTrainStep(m_c, o_c, cap_pbs, 0.65, bucket=b_c, warmup=2)
    torch.cuda.synchronize()
    out["captured_replay_peak_MiB"] = round((torch.cuda.max_memory_allocated() - base) / 2.0 ** 20, 1)      # (warm-up, capture and the graph's pool)
    routes["captured_replay"] = graphed
    for r, v in timed_runs(routes, args.runs, args.iters, args.warmup).items():
        out["%s_ms" % r] = [round(min(v), 4), round(max(v), 4)]
    # load: the host side (padding, by-object list, pinned copies) of feeding the captured step another batch, and a replay after it
    import time
    loads = []
    for k in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        graphed.load(host[(k + 1) % 2])
        loads.append((time.perf_counter() - t0) * 1e3)
        graphed()
    torch.cuda.synchronize()
    out["load_host_ms"] = [round(min(loads), 3), round(max(loads), 3)]
    out["loss_after"] = float(graphed.loss)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("bce", "step", "pair-rows"), default="bce")
    ap.add_argument("--D", type=int, default=516)
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--dropout", type=float, default=0.2)
    ap.add_argument("--M", type=int, default=25600)
    ap.add_argument("--H", type=int, default=300)
    ap.add_argument("--C", type=int, default=2002)
    ap.add_argument("--C_all", type=int, default=2335)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from dfol_vqa_amd import _lib
    from dfol_vqa_amd import ops as L
    _lib.load()                                                      # (raises with the build command when the library has not been built)
    if args.leg == "pair-rows":
        return pair_rows_leg(args)
    if args.leg == "step":
        return step_leg(args)

    rng = np.random.RandomState(0)
    dev = lambda x: torch.as_tensor(x).cuda()
    h = dev(rng.uniform(0.02, 0.98, size=(args.M, args.H)).astype(np.float32)).requires_grad_(True)
    emb_w = dev((rng.normal(size=(args.C_all, args.H)) * 3.0 / np.sqrt(0.33 * args.H)).astype(np.float32)).requires_grad_(True)
    emb_b = dev(rng.normal(size=args.C_all).astype(np.float32)).requires_grad_(True)
    cols = dev(rng.permutation(args.C_all)[:args.C].astype(np.int32))
    target = (torch.rand(args.M, args.C, device="cuda") < 0.02).float()
    weight = torch.rand(args.M, args.C, device="cuda")
    routes = {"fused": lambda: L.scene_bce(h, emb_w, emb_b, cols, target, weight, 0.5),
              "tensor": lambda: tensor_route(L, h, emb_w, emb_b, cols, target, weight, 0.5)}

    def step(fn, backward):
        if backward:
            h.grad = emb_w.grad = emb_b.grad = None
            fn()[0].backward()
        else:
            with torch.no_grad():
                fn()

    def timed(fn, backward):
        for _ in range(args.warmup):
            step(fn, backward)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(args.iters):
            step(fn, backward)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / args.iters

    times = {(r, leg): [] for r in routes for leg in ("fwd", "fwd_bwd")}
    peak = {}
    for _ in range(args.runs):
        for r, fn in routes.items():                                # the routes alternate
            for leg in ("fwd", "fwd_bwd"):
                times[(r, leg)].append(timed(fn, leg == "fwd_bwd"))
    for r, fn in routes.items():
        h.grad = emb_w.grad = emb_b.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(fn, True)
        torch.cuda.synchronize()
        peak[r] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
    out = {"M": args.M, "H": args.H, "C": args.C, "runs": args.runs, "iters": args.iters}
    for (r, leg), v in times.items():
        out["%s_%s_ms" % (r, leg)] = [round(min(v), 4), round(max(v), 4)]
    for r in routes:
        out["%s_peak_MiB" % r] = round(peak[r], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
