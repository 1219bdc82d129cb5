"""Child process of tests/test_train_store_direct_gpu.py: train steps over a `direct=True` feature store against the same steps over a plain
store (the matrix route), on a narrow model whose featurizer the wide kernel still takes (260 features -> 260, a weight of the split kernels'
size).  The parent sets DFOL_DENSE_WIDE=2 - the library reads it once per process - so that batches of a few dozen rows take the wide kernel.

usage: python tests/_train_store_direct_worker.py <directory>      prints one JSON line: per case, what was equal and which routes were counted.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from dfol_vqa_amd import _lib, data, experiment, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from dfol_vqa_amd.feature_store import StoreRows  # noqa: E402
from test_feature_store import write_chunks  # noqa: E402

DEV = torch.device("cuda:0")
F, WIDTH, MAX_OBJ = 260, 260, 12
COUNTS = [5, 3, 12, 7, 5, 3, 12, 7]                 # images 4-7 have the object counts of 0-3: a second batch of the same shapes
BATCHES = ([0, 1, 2, 1, 3], [4, 5, 6, 5, 7])        # one image asked twice
KEYS = ("feature_store_direct_train", "feature_store_direct_materialized", "feature_store_direct")
CLIP = 0.65


def bits_equal(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def snapshot(model, grads):
    return {k: (p.grad if grads else p).detach().cpu().numpy().copy() for k, p in model.named_parameters() if not grads or p.grad is not None}


class Bench(object):
    def __init__(self, directory, **cfg_over):
        self.dir = directory
        self.chunks, self.info = write_chunks(directory, feature_dim=F, max_obj=MAX_OBJ, counts=COUNTS, per_chunk=4, seed=41)
        paths, self.names = syn.write_synthetic_ontology(os.path.join(directory, "ontology"))
        over = dict(box_features_dim=F, oracle_input_dim=WIDTH, freeze_featurizer=False, freeze_attribute_network=False,
                    freeze_relation_network=False, freeze_embedding_network=False, dropout=0.0)
        over.update(cfg_over)
        self.ont = experiment.build_ontology(syn.reference_config(paths, **over))
        torch.manual_seed(5)
        self.model = experiment.build_model(syn.reference_config(paths, **over), self.ont).to(DEV).train()
        self.state0 = copy.deepcopy(self.model.state_dict())
        with open(paths["attribute_file"]) as f:
            self.cats = json.load(f)
        self.stores = {d: data.DeviceFeatureStore(directory, "objs", self.chunks, self.info, DEV, direct=d) for d in (False, True)}

    def host_batches(self, direct, images, kind="verify_rel"):
        qs = syn.full_size_questions(kind, len(images), 3, MAX_OBJ, self.names, self.cats, 61, with_scene=False)
        for q, im in zip(qs, images):
            q["image_id"] = "img%03d" % im
        pbs = data.BatchGQABoxFeaturesCollator(self.dir, "objs", self.chunks, self.info, self.ont, 1,
                                               device_store=self.stores[direct].index).collate([dict(q) for q in qs])
        for pb in pbs:
            pb.create_sparse_tensors()
        return pbs

    def reset(self, opt=None):
        """The model's first weights; an optimizer handed in goes back to its first step (its state tensors stay where a graph baked them in)."""
        with torch.no_grad():
            self.model.load_state_dict(self.state0)
            for st in ([] if opt is None else opt.state.values()):
                for v in st.values():
                    if isinstance(v, torch.Tensor):
                        v.zero_()
        if opt is None:
            for p in self.model.parameters():
                p.grad = None

    def adam(self):
        return torch.optim.Adam([p for p in self.model.parameters() if p.requires_grad], lr=1e-3, capturable=True)

    def eager_step(self, direct, images):
        """One train_batch from the first weights -> (loss, gradients, weights after the Adam step, route counts)."""
        self.reset()
        dev = [pb.to_cuda(DEV) for pb in self.host_batches(direct, images)]
        assert isinstance(dev[0]._object_features, StoreRows if direct else torch.Tensor)
        before = dict(_lib.PATH_COUNTS)
        loss, _ = training.train_batch(self.model, self.adam(), dev, clip_norm=CLIP, sync_loss=False)      # (the loss as a captured step returns it)
        counts = {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in KEYS}
        return np.float64(float(loss)), snapshot(self.model, True), snapshot(self.model, False), counts, len(dev)


def compare(bench, images=BATCHES[0]):
    l0, g0, w0, c0, n = bench.eager_step(False, images)
    l1, g1, w1, c1, _ = bench.eager_step(True, images)
    moved = not bits_equal(w1, {k: v.cpu().numpy() for k, v in bench.state0.items() if k in w1})
    return {"loss_equal": l0.tobytes() == l1.tobytes() and bool(np.isfinite(l0)), "grads_equal": bits_equal(g0, g1), "weights_equal": bits_equal(w0, w1),
            "featurizer_grads": sorted(k for k in g1 if k.startswith("_featurizer")), "weights_moved": moved,
            "plain_counts": c0, "direct_counts": c1, "batches": n}


def graphed(bench):
    """A captured step over the direct store: its replay on the batch it was captured with, then on a second batch of the same shapes served
    through rows(ref, out=...), each against the eager step on that batch from the same weights and optimizer state."""
    eager = [bench.eager_step(True, images) for images in BATCHES]
    host = [bench.host_batches(True, images) for images in BATCHES]
    bench.reset()
    opt = bench.adam()
    dev = [pb.to_cuda(DEV) for pb in host[0]]
    before = dict(_lib.PATH_COUNTS)
    step = training.GraphedTrainStep(bench.model, opt, dev, CLIP, warmup=1)
    counts = {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in KEYS}
    out = {"capture_counts": counts, "replays": [], "batches_differ": eager[0][0].tobytes() != eager[1][0].tobytes()}
    store = bench.stores[True]
    for k in (0, 1, 0):
        for pb, pb2 in zip(dev, host[k]):
            assert store.rows(pb2._object_features, out=pb._object_features) is pb._object_features
        bench.reset(opt)
        loss, _ = step()
        torch.cuda.synchronize()
        l, g, w = np.float64(float(loss)), snapshot(bench.model, True), snapshot(bench.model, False)
        out["replays"].append({"batch": k, "loss_equal": l.tobytes() == eager[k][0].tobytes(), "grads_equal": bits_equal(g, eager[k][1]),
                               "weights_equal": bits_equal(w, eager[k][2])})
    return out


def main(directory):
    assert os.environ.get("DFOL_DENSE_WIDE") == "2"
    report = {}
    sub = lambda name: (os.makedirs(os.path.join(directory, name)), os.path.join(directory, name))[1]
    bench = Bench(sub("f16x2"))
    report["default"] = compare(bench)
    report["graphed"] = graphed(bench)
    report["bf16"] = compare(Bench(sub("bf16"), mlp_math="bf16"))
    report["dropout"] = compare(Bench(sub("dropout"), dropout=0.1))
    report["frozen"] = compare(Bench(sub("frozen"), freeze_featurizer=True))
    report["two_layer"] = compare(Bench(sub("two_layer"), featurizer_layers_config=[WIDTH]))
    print(json.dumps(report))


if __name__ == "__main__":
    main(sys.argv[1])
