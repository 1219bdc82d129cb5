"""GPU tests of the train step over a `direct=True` feature store (interpreter.featurize_scene -> visual_oracle.StoreRowsLinear: the
featurizer's first layer reads the store's rows through src_row, forward and weight gradient) against the same step over a plain store, which
gathers the [O, F + 6] matrix.  Every comparison is bit equality: loss, every parameter's gradient, the weights after the Adam step.

One child process runs all cases (tests/_train_store_direct_worker.py, DFOL_DENSE_WIDE=2: the library reads the switch once per process, and
a batch of a few dozen rows is not the wide kernel's without it); the tests read its report.  The model is narrow - 260 features -> 260, a
weight the split kernels take - over a store of 8 images of 3 - 12 objects, 5 questions with one image asked twice.
`feature_store_direct` counts every batch whose featurizer read the store in place, `feature_store_direct_train` those of them that train.

In `mlp_math: bf16` the indexed weight gradient has its kernel (tests/test_wgrad_rows_gpu.py), but the forward product over indexed rows exists
in the two-piece fp16 arithmetic only (store_layers_of): there the route steps aside and the step is the matrix route's, which is what the
bf16 test pins down - equal bits, counted as materialised."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ALL_EQUAL = ("loss_equal", "grads_equal", "weights_equal")
W1 = ["_featurizer._featurizer_network._network.1.bias", "_featurizer._featurizer_network._network.1.weight"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    env = dict(os.environ, DFOL_DENSE_WIDE="2")
    env.pop("DFOL_NATIVE", None)
    env.pop("DFOL_DENSE_MATH", None)
    out = subprocess.run([sys.executable, os.path.join(HERE, "_train_store_direct_worker.py"), str(tmp_path_factory.mktemp("train_direct"))], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_direct_train_step_equals_the_matrix_route(report):
    r = report["default"]
    assert all(r[k] for k in ALL_EQUAL), r
    assert r["featurizer_grads"] == W1 and r["weights_moved"], r


def test_direct_train_step_is_counted(report):
    r = report["default"]
    n = r["batches"]
    assert n >= 1
    assert r["direct_counts"] == {"feature_store_direct_train": n, "feature_store_direct_materialized": 0, "feature_store_direct": n}, r
    assert r["plain_counts"] == {"feature_store_direct_train": 0, "feature_store_direct_materialized": 0, "feature_store_direct": 0}, r


def test_bf16_mode_keeps_the_matrix_routes_bits(report):
    r = report["bf16"]
    assert all(r[k] for k in ALL_EQUAL) and r["featurizer_grads"] == W1 and r["weights_moved"], r
    assert r["direct_counts"] == {"feature_store_direct_train": 0, "feature_store_direct_materialized": r["batches"], "feature_store_direct": 0}, r


def test_graphed_train_step_replays_the_route(report):
    g = report["graphed"]
    assert g["capture_counts"]["feature_store_direct_train"] >= 2 and g["capture_counts"]["feature_store_direct_materialized"] == 0, g      # warm-up and capture
    assert g["batches_differ"], g
    assert [r["batch"] for r in g["replays"]] == [0, 1, 0]
    for r in g["replays"]:
        assert all(r[k] for k in ALL_EQUAL), r


def test_active_dropout_steps_aside(report):
    r = report["dropout"]
    assert r["direct_counts"] == {"feature_store_direct_train": 0, "feature_store_direct_materialized": r["batches"], "feature_store_direct": 0}, r


def test_frozen_featurizer_keeps_the_inference_route(report):
    r = report["frozen"]
    assert all(r[k] for k in ALL_EQUAL) and r["featurizer_grads"] == [] and r["weights_moved"], r
    assert r["direct_counts"] == {"feature_store_direct_train": 0, "feature_store_direct_materialized": 0, "feature_store_direct": r["batches"]}, r


def test_two_layer_featurizer_trains_on_the_route(report):
    r = report["two_layer"]
    assert all(r[k] for k in ALL_EQUAL) and r["weights_moved"], r
    assert r["featurizer_grads"] == W1 + [W1[0].replace(".1.", ".4."), W1[1].replace(".1.", ".4.")], r
    assert r["direct_counts"] == {"feature_store_direct_train": r["batches"], "feature_store_direct_materialized": 0, "feature_store_direct": r["batches"]}, r
