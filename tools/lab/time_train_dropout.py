"""What training with dropout costs (results: profiles/r13_dropout.txt).

1. The mask kernel (dfol_dropout_f32) beside a `copy_` of the same tensor, alternating in one session: the featurizer's [25600, 2048] view of a
   [25600, 2054] matrix, and the [pairs, 1036] pair matrix of 64 images x 36 objects.  A copy moves the same 8 bytes per element; the ratio
   says how much of the kernel is its ten Philox rounds per four elements.
2. The pair matrix's ordered backward (dfol_pair_features_bwd_f32) beside the two index_add_ calls it replaces on the dropout route.
3. A train step at p = 0.1 on the full-table route beside the fused step at p = 0, at 256 x 36 objects and, if it fits, 256 x 100.

usage: python tools/lab/time_train_dropout.py [--skip-step] [--objects 36,100]"""
import argparse
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import dfol_vqa_amd as D  # noqa: E402
from dfol_vqa_amd import _lib, experiment, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, reps=10, rounds=5):
    """Best of `rounds` averages over `reps` back-to-back calls, in ms (HIP events on the launch stream)."""
    best = 1e9
    for _ in range(rounds):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(e) / reps)
    return best


def alternate(forms, sessions=3):
    """{name: best ms} with the forms taking turns, so that clock and cache state are shared."""
    best = {k: 1e9 for k in forms}
    for fn in forms.values():
        fn()
    for _ in range(sessions):
        for k, fn in forms.items():
            best[k] = min(best[k], timed(fn))
    return best


def kernel_beside_copy():
    g = torch.Generator(device=dev).manual_seed(0)
    key = _lib.dropout_key(dev)
    pairs = 64 * 36 * 35
    for name, x in (("featurizer view [25600, 2048] of [25600, 2054]", torch.rand(25600, 2054, device=dev, generator=g)[:, :2048]),
                    ("pair matrix [%d, 1036]" % pairs, torch.rand(pairs, 1036, device=dev, generator=g))):
        y = torch.empty(x.shape, device=dev)
        t = alternate({"dropout": lambda: _lib.dropout(x, 0.1, key, 3, out=y, count=False), "copy_": lambda: y.copy_(x),
                       "dropout in place": lambda: _lib.dropout(y, 0.1, key, 3, out=y, count=False)})
        gb = 8.0 * x.numel() / 1e9
        print("%-48s dropout %7.1f us (%5.2f TB/s)   copy_ %7.1f us (%5.2f TB/s)   ratio %.2f   in place %7.1f us" %
              (name, t["dropout"] * 1e3, gb / t["dropout"], t["copy_"] * 1e3, gb / t["copy_"], t["dropout"] / t["copy_"], t["dropout in place"] * 1e3))


def pair_backward():
    g = torch.Generator(device=dev).manual_seed(1)
    for Q, n, Dw in ((64, 36, 516), (256, 36, 516)):
        n_list = [n] * Q
        obj_off = torch.arange(Q + 1, dtype=torch.int32, device=dev) * n
        pair_off = torch.arange(Q + 1, dtype=torch.int64, device=dev) * (n * (n - 1))
        s, o = np.nonzero(~np.eye(n, dtype=bool))
        first = np.repeat(np.arange(Q) * n, n * (n - 1))
        ind_s = torch.as_tensor(np.tile(s, Q) + first, device=dev)
        ind_o = torch.as_tensor(np.tile(o, Q) + first, device=dev)
        grad = torch.randn(Q * n * (n - 1), 2 * Dw + 4, device=dev, generator=g)

        def atomic():
            out = torch.zeros(Q * n, Dw, device=dev)
            out.index_add_(0, ind_s, grad[:, :Dw])
            out.index_add_(0, ind_o, grad[:, Dw:2 * Dw])
            return out

        ordered = lambda: _lib.pair_features_bwd(grad, Dw, obj_off, pair_off, Q, n, Q * n)
        assert torch.allclose(atomic(), ordered(), rtol=1e-4, atol=1e-4)
        t = alternate({"ordered": ordered, "index_add_": atomic})
        print("pair backward %3d x %3d objects, D = %d: ordered %7.1f us (%5.2f TB/s read)   index_add_ x 2 %7.1f us   ratio %.2f" %
              (Q, n, Dw, t["ordered"] * 1e3, 8.0 * grad.shape[0] * Dw / 1e9 / t["ordered"], t["index_add_"] * 1e3, t["ordered"] / t["index_add_"]))
        del n_list


class Collater(D.ProgramCollaterBase):
    def __init__(self, ont):
        super(Collater, self).__init__("select", "relate", "filter", 1, ontology=ont)

    def collate_object_features(self, questions):
        feats = torch.cat([torch.from_numpy(q["scene"]["X"]) for q in questions], 0)
        bi = torch.cat([torch.full((q["scene"]["n"],), i, dtype=torch.int64) for i, q in enumerate(questions)])
        return feats, bi

    def collate_meta_data(self, questions):
        return {"index": {}, "embedding": torch.zeros(1, 1)}


def train_step(objects, Q=256):
    paths, names = syn.write_synthetic_ontology(tempfile.mkdtemp(prefix="dfol_dropout_"))
    for p in (0.0, 0.1):
        cfg = syn.reference_config(paths, dropout=p, freeze_featurizer=False, freeze_attribute_network=False, freeze_relation_network=False,
                                   freeze_embedding_network=False)
        ont = experiment.build_ontology(cfg)
        torch.manual_seed(0)
        model = experiment.build_model(cfg, ont)
        with torch.no_grad():
            model._oracle._embedding_network.linear.weight.normal_(0.0, 0.1)
            model._oracle._embedding_network.linear.bias.fill_(-2.0)
        model = model.to(dev).train()
        qs = []
        for i in range(Q):
            br, last = syn.three_hop_program(i, names["nouns"][:8], names["attributes"][:6], names["relations"][:5])
            qs.append(syn.question(i, br, last, "yes" if i % 2 else "no", syn.feature_scene(i, objects, 2048)))
        pbs = [pb.to_cuda(dev) for pb in Collater(ont).collate(qs)]
        opt = torch.optim.Adam([q for q in model.parameters() if q.requires_grad], lr=1e-4)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                for _ in range(2):
                    training.train_batch(model, opt, pbs, 0.65, sync_loss=False)
                torch.cuda.synchronize()
                _lib.PATH_COUNTS.clear()
                ms = timed(lambda: training.train_batch(model, opt, pbs, 0.65, sync_loss=False), reps=3, rounds=3)
        except torch.OutOfMemoryError as err:
            print("train step %d x %d objects, p = %.1f: does not fit (%s)" % (Q, objects, p, str(err).splitlines()[0]))
            continue
        route = "full tables + masks" if _lib.PATH_COUNTS.get("fallback:dropout_full_tables") else "fused needed-columns"
        print("train step %d x %3d objects, p = %.1f (%s): %8.2f ms eager   peak memory %6.2f GB   dropout launches per step %d" %
              (Q, objects, p, route, ms, torch.cuda.max_memory_allocated() / 2 ** 30, _lib.PATH_COUNTS.get("dropout", 0) // 9))
        del model, opt, pbs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--objects", default="36,100")
    args = ap.parse_args()
    kernel_beside_copy()
    pair_backward()
    if not args.skip_step:
        for n in (int(v) for v in args.objects.split(",")):
            train_step(n)
