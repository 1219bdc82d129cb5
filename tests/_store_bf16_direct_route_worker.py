"""Child process of tests/test_store_bf16_direct_route_gpu.py: the default arithmetic over a bf16 feature store with DFOL_STORE_BF16_DIRECT set and
unset, on the full-size synthetic model of tests/test_store_bf16_gpu.py (its World: chunk files whose features are bf16 values already, behind an
fp32 store and a bf16 store - the two then hold the same numbers, so every route must give the fp32 store's bits).  DFOL_DENSE_WIDE=2 (the parent
sets it; the library reads it once per process): batches of a few dozen rows are the wide kernel's.

usage: python tests/_store_bf16_direct_route_worker.py <directory>      prints one JSON line {section: "ok" | what failed}."""
import json
import os
import sys
import traceback
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from dfol_vqa_amd import _lib, native_exec  # noqa: E402
from dfol_vqa_amd.feature_store import StoreRows  # noqa: E402
from dfol_vqa_amd.interpreter import GraphedForward  # noqa: E402
from test_store_bf16_gpu import DEV, KEYS, World, bits, steps_equal  # noqa: E402

H2 = "feature_store_direct_bf16_h2"
ALL = KEYS + (H2, "native_program", "python_program")
IMAGES = [6, 2, 6, 3, 0]                                                  # (not image 1: its 2^17 is the range re-run's)


def counts_of(fn):
    before = dict(_lib.PATH_COUNTS)
    out = fn()
    return out, {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in ALL}


def switch(on):
    if on:
        os.environ["DFOL_STORE_BF16_DIRECT"] = "1"
    else:
        os.environ.pop("DFOL_STORE_BF16_DIRECT", None)


def inference(world, on):
    """Every executor x shared scenes x question kind: the bf16 store's log-probabilities and answers against the fp32 store's."""
    world.mode(None, train=False)
    n_cases = 0
    for native in ("1", "0"):
        os.environ["DFOL_NATIVE"] = native
        for share in (False, True):
            for kind in ("exist", "verify_rel"):
                switch(False)
                (n0, lp0, a0), c0 = counts_of(lambda: world.infer("rounded", "f32", IMAGES, kind=kind, share=share))
                switch(on)
                (n1, lp1, a1), c1 = counts_of(lambda: world.infer("rounded", "bf16", IMAGES, kind=kind, share=share))
                where = (kind, share, native, c0, c1)
                assert n0 == n1 and bool(np.isfinite(lp0).all()) and np.array_equal(lp0.view(np.uint32), lp1.view(np.uint32)) and a0 == a1, where
                assert c0["feature_store_direct"] == c0["feature_store_direct_materialized"] == c0[H2] == 0, where
                assert c1["native_program" if native == "1" else "python_program"] == n1 and c0["native_program"] == c1["native_program"], where
                if on:
                    assert c1["feature_store_direct"] == c1[H2] == n1 and c1["feature_store_direct_materialized"] == 0, where
                else:
                    assert c1["feature_store_direct_materialized"] == n1 and c1["feature_store_direct"] == c1[H2] == 0, where
                assert c1["feature_store_direct_train"] == 0, where
                n_cases += 1
    assert n_cases == 8


def graphed(world):
    os.environ["DFOL_NATIVE"] = "1"
    world.mode(None, train=False)
    store = world.stores["rounded", "bf16"]
    scenes = ([0, 2, 2, 0], [3, 5, 5, 3])                                 # (the same object counts; neither names image 1)
    switch(True)
    host = [world.host_batches("rounded", "bf16", ims, kind="exist", seed=77) for ims in scenes]
    switch(False)
    want = [world.infer("rounded", "f32", ims, kind="exist", seed=77) for ims in scenes]
    assert not np.array_equal(want[0][1].view(np.uint32), want[1][1].view(np.uint32))
    switch(True)
    dev = [pb.to_cuda(DEV) for pb in host[0]]
    assert all(isinstance(pb._object_features, StoreRows) for pb in dev)
    g, c = counts_of(lambda: GraphedForward(world.model, dev))
    assert c["feature_store_direct"] > 0 and c[H2] == c["feature_store_direct"] and c["feature_store_direct_materialized"] == 0, c
    for k in (0, 1, 0):
        for pb, pb2 in zip(dev, host[k]):
            assert store.rows(pb2._object_features, out=pb._object_features) is pb._object_features
        r = g()
        assert np.array_equal(bits(r["log_probability"]), want[k][1].view(np.uint32)) and r["answer"] == want[k][2], k


def range_rerun(world):
    os.environ["DFOL_NATIVE"] = "1"
    images = [1, 2, 1, 0]                                                 # image 1 holds 2^17
    world.mode(None, train=False, overflow="rerun")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            switch(False)
            (n0, lp0, a0), c0 = counts_of(lambda: world.infer("rounded", "f32", images))
            before = _lib.PATH_COUNTS["fallback:range_rerun"]
            switch(True)
            (n1, lp1, a1), c1 = counts_of(lambda: world.infer("rounded", "bf16", images))
    finally:
        world.mode(None, train=False)
    assert _lib.PATH_COUNTS["fallback:range_rerun"] >= before + 1, "the in-place kernel did not raise the range flag"
    assert n0 == n1 and bool(np.isfinite(lp0).all()) and np.array_equal(lp0.view(np.uint32), lp1.view(np.uint32)) and a0 == a1
    # the flagged first run read the table in place; its re-run on 'bf16x3' materialised the matrix, as ever
    assert c1[H2] >= 1 and c1["feature_store_direct_materialized"] >= 1, c1


def train_step(world):
    switch(True)
    world.mode(None, train=True)
    try:
        s0, s1 = world.eager_step("rounded", "f32", IMAGES), world.eager_step("rounded", "bf16", IMAGES)
    finally:
        world.mode(None, train=False)
    assert steps_equal(s0, s1)
    want = {"feature_store_direct": 0, "feature_store_direct_train": 0, "feature_store_direct_materialized": s1[4]}
    assert {k: s1[3][k] for k in KEYS} == want, s1[3]


def setter_refusal(world):
    """DFOL_FEATURES_ROWS_BF16_H2 in front of a first layer that is not DFOL_DENSE_F16X2 (the bf16 mode's): refused with the reason."""
    switch(True)
    os.environ["DFOL_NATIVE"] = "1"
    world.mode("bf16", train=False)
    pbs_dev = [pb.to_cuda(DEV) for pb in world.host_batches("rounded", "bf16", IMAGES, kind="exist")]
    real = _lib.call

    def call(name, *args):
        if name == "dfol_run_program":                                   # (the bf16 mode's own run: its scene struct names DFOL_FEATURES_ROWS_BF16)
            scene = args[1]._obj
            assert scene.feature_form == native_exec.FEATURES_ROWS_BF16 and scene.src_row and scene.box6
            scene.feature_form = native_exec.FEATURES_ROWS_BF16_H2
        return real(name, *args)
    _lib.call = call
    try:
        with torch.no_grad():
            world.model(pbs_dev[:1], False)
        raise AssertionError("not refused")
    except _lib.DfolError as e:
        assert "DFOL_DENSE_F16X2" in str(e) and "(DFOL_FEATURES_ROWS_BF16_H2)" in str(e), str(e)
    finally:
        _lib.call = real
        world.mode(None, train=False)
    assert native_exec.DENSE_F16X2 != native_exec.DENSE_BF16


def main(directory):
    assert os.environ.get("DFOL_DENSE_WIDE") == "2"
    for k in ("DFOL_NATIVE", "DFOL_DENSE_MATH", "DFOL_STORE_BF16_DIRECT"):
        os.environ.pop(k, None)
    world = World(directory)
    report = {}
    for name, fn in (("inference_on", lambda: inference(world, True)), ("inference_off", lambda: inference(world, False)),
                     ("graphed", lambda: graphed(world)), ("range_rerun", lambda: range_rerun(world)), ("train_step", lambda: train_step(world)),
                     ("setter_refusal", lambda: setter_refusal(world))):
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
