"""Scene-graph supervision: the fused weighted BCE (ops.scene_bce, csrc/dfol_scene.hip) against the tensor-op route of the same function
(embedding rows gathered, linear_act with LogSigmoid, exp, binary_cross_entropy, autograd), forward and forward + backward.

    python tools/bench_scene.py --M 25600 --H 300 --C 2002
    python tools/bench_scene.py --M 2560 --H 300 --C 333

The two routes alternate inside one process, --runs times (default 5); each run times --iters steps between two events after --warmup
steps and reports the mean per step.  Printed: one JSON line with the range (min, max) over the runs per route and leg, and the peak device
memory of each route above what the inputs hold.  Ranges that overlap show no difference."""

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=25600)
    ap.add_argument("--H", type=int, default=300)
    ap.add_argument("--C", type=int, default=2002)
    ap.add_argument("--C_all", type=int, default=2335)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from dfol_vqa_amd import ops as L

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
