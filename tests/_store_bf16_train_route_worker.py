"""Child process of tests/test_store_bf16_train_route_gpu.py: a train step in the default arithmetic over a bf16 feature store with
DFOL_STORE_BF16_TRAIN set and unset, on the full-size synthetic model of tests/test_store_bf16_gpu.py (its World: chunk files whose features are
bf16 values already, behind an fp32 store and a bf16 store - the two then hold the same numbers, so every route must give the fp32 store's bits:
the loss, every gradient and every parameter after Adam).  DFOL_DENSE_WIDE=2 (the parent sets it; the library reads it once per process): batches
of a few dozen rows are the wide kernel's.

usage: python tests/_store_bf16_train_route_worker.py <directory>      prints one JSON line {section: "ok" | what failed}."""
import json
import os
import sys
import traceback

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from dfol_vqa_amd import _lib, data, training  # noqa: E402
from dfol_vqa_amd.feature_store import StoreRows  # noqa: E402
from test_feature_store import write_chunks  # noqa: E402
from test_store_bf16 import rne_bf16, widen_bf16  # noqa: E402
from test_store_bf16_gpu import CLIP, DEV, E_COUNTS, KEYS, MAX_OBJ, World, same, steps_equal  # noqa: E402

X3 = "feature_store_direct_train_bf16_x3"
H2 = "feature_store_direct_bf16_h2"
ALL = KEYS + (X3, H2)
IMAGES = [6, 2, 6, 3, 0]                                                  # (not image 1: its 2^17 belongs to the range test)


def switch(on):
    if on:
        os.environ["DFOL_STORE_BF16_TRAIN"] = "1"
    else:
        os.environ.pop("DFOL_STORE_BF16_TRAIN", None)


def step(world, name, dtype, images=IMAGES):
    """World.eager_step with this worker's counters -> (loss, gradients, parameters, counts, batches)."""
    before = dict(_lib.PATH_COUNTS)
    s = world.eager_step(name, dtype, images)
    return s[:3] + ({k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in ALL}, s[4])


def counts(s):
    return {k: v for k, v in s[3].items() if k != H2}


def in_place(n):
    return {"feature_store_direct": n, "feature_store_direct_train": n, X3: n, "feature_store_direct_materialized": 0}


def matrix(n):
    return {"feature_store_direct": 0, "feature_store_direct_train": 0, X3: 0, "feature_store_direct_materialized": n}


def switch_set(world):
    world.mode(None, train=True)
    switch(False)
    s0 = step(world, "rounded", "f32")
    switch(True)
    s1 = step(world, "rounded", "bf16")
    n = s1[4]
    assert n == s0[4] and n > 0
    assert steps_equal(s0, s1)
    assert counts(s1) == in_place(n) and s1[3][H2] == 0, s1[3]
    assert counts(s0) == matrix(0), s0[3]                                                       # (an fp32 store with direct=False: the matrix from the collator)
    assert not same(s1[2], {k: v.cpu().numpy() for k, v in world.state0.items() if k in s1[2]})  # a non-zero Adam step
    assert any(k.startswith("_featurizer") for k in s1[1])


def switch_unset(world):
    world.mode(None, train=True)
    switch(False)
    s0, s1 = step(world, "rounded", "f32"), step(world, "rounded", "bf16")
    assert steps_equal(s0, s1)
    assert counts(s1) == matrix(s1[4]) and s1[4] > 0, s1[3]


def graphed(world, name, batches):
    """A captured train step over batches[0], refilled through store.rows(..., out=) and replayed in the order 0, 1, 0.  Over the `rounded` files
    the scenes are [0, 2, 2, 0] / [3, 5, 5, 3], as in tests/_store_bf16_direct_route_worker.py: image 1 holds 2^17 there, which no step in this
    arithmetic accepts, from either store.  The scenes [0, 1, 2, 1] / [3, 4, 5, 4] run over the `f16` files, which have no such value."""
    world.mode(None, train=True)
    switch(False)
    eager = [step(world, name, "f32", ims) for ims in batches]
    assert eager[0][0].tobytes() != eager[1][0].tobytes()
    switch(True)
    host = [world.host_batches(name, "bf16", ims) for ims in batches]
    store = world.stores[name, "bf16"]
    world.reset()
    opt = world.adam()
    dev = [pb.to_cuda(DEV) for pb in host[0]]
    assert all(isinstance(pb._object_features, StoreRows) for pb in dev)
    before = dict(_lib.PATH_COUNTS)
    graph = training.GraphedTrainStep(world.model, opt, dev, CLIP, warmup=1)
    c = {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in ALL}
    assert c[X3] >= 2 and c[X3] == c["feature_store_direct_train"] == c["feature_store_direct"] and c["feature_store_direct_materialized"] == 0, c
    for k in (0, 1, 0):
        for pb, pb2 in zip(dev, host[k]):
            assert store.rows(pb2._object_features, out=pb._object_features) is pb._object_features
        world.reset(opt)
        loss, _ = graph()
        torch.cuda.synchronize()
        assert steps_equal((np.float64(float(loss)), world.snapshot(True), world.snapshot(False)), eager[k]), k


def keeps_dropout(world):
    switch(True)
    world.mode(None, train=True, dropout=0.1)
    try:
        s = step(world, "rounded", "bf16")
    finally:
        world.mode(None, train=True)
    assert bool(np.isfinite(s[0])) and counts(s) == matrix(s[4]) and s[4] > 0, s[3]


def keeps_wgrad_f32(world):
    world.mode(None, train=True)
    os.environ["DFOL_WGRAD_MATH"] = "f32"
    try:
        switch(False)
        s0 = step(world, "rounded", "f32")
        switch(True)
        s1 = step(world, "rounded", "bf16")
    finally:
        os.environ.pop("DFOL_WGRAD_MATH", None)
    assert steps_equal(s0, s1)
    assert counts(s1) == matrix(s1[4]) and s1[4] > 0, s1[3]


def keeps_bf16_mode(world):
    world.mode("bf16", train=True)
    try:
        switch(False)
        s0 = step(world, "rounded", "f32")
        switch(True)
        s1 = step(world, "rounded", "bf16")
    finally:
        world.mode(None, train=True)
    n = s1[4]
    assert steps_equal(s0, s1)
    want = dict(in_place(n))
    want[X3] = 0                                                          # the bf16 mode's own in-place route
    assert counts(s1) == want and s1[3][H2] == 0, s1[3]


def keeps_inference(world):
    """A frozen featurizer in eval(), with and without grad mode: the inference routing, which this switch does not touch."""
    switch(True)
    os.environ["DFOL_NATIVE"] = "1"
    world.mode(None, train=False)
    feat = [p for k, p in world.model.named_parameters() if k.startswith("_featurizer")]
    assert feat
    try:
        for p in feat:
            p.requires_grad_(False)
        out = {}
        for dtype in ("f32", "bf16"):
            before = dict(_lib.PATH_COUNTS)
            n, lp, ans = world.infer("rounded", dtype, IMAGES)
            out[dtype] = (n, lp, ans, {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in ALL})
        dev = [pb.to_cuda(DEV) for pb in world.host_batches("rounded", "bf16", IMAGES)]
        before = dict(_lib.PATH_COUNTS)
        res = world.model(dev, False)                                     # grad mode on: the other networks still train, the featurizer does not
        c = {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in ALL}
    finally:
        for p in feat:
            p.requires_grad_(True)
        os.environ.pop("DFOL_NATIVE", None)
        world.mode(None, train=True)
    (n0, lp0, a0, c0), (n1, lp1, a1, c1) = out["f32"], out["bf16"]
    assert n0 == n1 and bool(np.isfinite(lp0).all()) and np.array_equal(lp0.view(np.uint32), lp1.view(np.uint32)) and a0 == a1
    assert {k: c1[k] for k in c1 if k != H2} == matrix(n1) and c1[H2] == 0, c1
    assert {k: c[k] for k in c if k != H2} == matrix(len(dev)) and c[H2] == 0, c
    assert bool(torch.isfinite(res["log_probability"]).all())


def f16_files(world, directory):
    """One more chunk directory, `f16`: features that are bf16 AND fp16 values, behind an fp32 store and a bf16 store as World's are."""
    d = os.path.join(directory, "f16")
    os.makedirs(d)
    chunks, info = write_chunks(d, feature_dim=2048, max_obj=MAX_OBJ, counts=E_COUNTS, per_chunk=4, seed=17)
    for c in range(chunks):
        z = dict(np.load(os.path.join(d, "objs_%d.npz" % c)))
        x = widen_bf16(rne_bf16(z["features"])).reshape(z["features"].shape)
        x[np.abs(x) < 2.0 ** -14] = 0.0                                   # below fp16's normal range: eight significant bits are not enough there
        assert np.array_equal(x.astype(np.float16).astype(np.float32), x) and np.abs(x).max() < 65504
        z["features"] = x
        np.savez(os.path.join(d, "objs_%d.npz" % c), **z)
    world.dirs["f16"] = (d, chunks, info)
    world.stores["f16", "f32"] = data.DeviceFeatureStore(d, "objs", chunks, info, DEV)
    world.stores["f16", "bf16"] = data.DeviceFeatureStore(d, "objs", chunks, info, DEV, feature_dtype="bf16")


def certificate(world):
    """Over the `f16` files the forward's two-product form (the store's certificate forced True) and its three-product form (False) both give
    the fp32 store's step."""
    store = world.stores["f16", "bf16"]
    store._f16_exact = None
    assert store.f16_exact is True                                        # (what the library's own pass says of these files)
    world.mode(None, train=True)
    switch(False)
    s0 = step(world, "f16", "f32")
    switch(True)
    for forced in (True, False):
        store._f16_exact = forced
        s1 = step(world, "f16", "bf16")
        assert store._f16_exact is forced
        assert steps_equal(s0, s1), forced
        assert counts(s1) == in_place(s1[4]), (forced, s1[3])


def main(directory):
    assert os.environ.get("DFOL_DENSE_WIDE") == "2"
    for k in ("DFOL_NATIVE", "DFOL_DENSE_MATH", "DFOL_WGRAD_MATH", "DFOL_STORE_BF16_DIRECT", "DFOL_STORE_BF16_TRAIN"):
        os.environ.pop(k, None)
    world = World(directory)
    f16_files(world, directory)
    report = {}
    for name, fn in (("switch_set", lambda: switch_set(world)), ("switch_unset", lambda: switch_unset(world)),
                     ("graphed", lambda: graphed(world, "rounded", ([0, 2, 2, 0], [3, 5, 5, 3]))),
                     ("graphed_f16", lambda: graphed(world, "f16", ([0, 1, 2, 1], [3, 4, 5, 4]))),
                     ("keeps_dropout", lambda: keeps_dropout(world)), ("keeps_wgrad_f32", lambda: keeps_wgrad_f32(world)),
                     ("keeps_bf16_mode", lambda: keeps_bf16_mode(world)), ("keeps_inference", lambda: keeps_inference(world)),
                     ("certificate", lambda: certificate(world))):
        try:
            fn()
            report[name] = "ok"
        except _lib.DfolError:
            report[name] = traceback.format_exc()[-1500:]
        except AssertionError:
            report[name] = traceback.format_exc()[-1500:]
        finally:
            switch(False)
    print(json.dumps(report))


if __name__ == "__main__":
    main(sys.argv[1])
