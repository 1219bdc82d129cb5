"""GPU tests of the route DFOL_STORE_BF16_TRAIN=1 opens: a model in the default arithmetic (two fp16 pieces forward, three bf16 pieces in the
weight gradient) whose featurizer TRAINS reads a bf16 feature store's rows in place - forward through dfol_linear_wide_rows_bf16t_f16_h2_f32,
first-layer weight gradient through dfol_linear_wgrad_bias_rows_bf16t_x3 - eagerly and in a captured train step, against an fp32 store over
chunk files whose features are bf16 values already, so the two stores hold the same numbers and every comparison is bit equality: the loss, every
gradient, every parameter after Adam.  With the switch unset, and with it set under an active Dropout, DFOL_WGRAD_MATH=f32, `mlp_math: bf16`
or a frozen featurizer, every route and counter is what it was.

One child process runs all cases (tests/_store_bf16_train_route_worker.py, DFOL_DENSE_WIDE=2: the library reads that switch once per process,
and a batch of a few dozen rows is not the wide kernel's without it) on the synthetic-model construction of tests/test_store_bf16_gpu.py; the
tests read its report."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    env = dict(os.environ)
    env["DFOL_DENSE_WIDE"] = "2"
    for k in ("DFOL_NATIVE", "DFOL_DENSE_MATH", "DFOL_WGRAD_MATH", "DFOL_STORE_BF16_DIRECT", "DFOL_STORE_BF16_TRAIN"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(HERE, "_store_bf16_train_route_worker.py"), str(tmp_path_factory.mktemp("bf16_train_route"))],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_switch_set_train_step_reads_the_table_in_place_with_the_fp32_stores_bits(report):
    """feature_store_direct == feature_store_direct_train == feature_store_direct_train_bf16_x3 == batches, feature_store_direct_materialized == 0,
    a non-zero Adam step and a gradient for the featurizer."""
    assert report["switch_set"] == "ok", report["switch_set"]


def test_switch_unset_materialises_as_before_with_the_same_bits(report):
    assert report["switch_unset"] == "ok", report["switch_unset"]


def test_graphed_train_step_replays_new_scenes_through_rows_out(report):
    """Captured over one scene, refilled through store.rows(..., out=) and replayed in the order 0, 1, 0: each replay is the fp32 store's eager
    step; the capture counted no materialised batch."""
    assert report["graphed"] == "ok", report["graphed"]


def test_graphed_train_step_over_files_of_fp16_values(report):
    """The same with scenes [0, 1, 2, 1] / [3, 4, 5, 4] over chunk files without image 1's 2^17: the certified forward inside the capture."""
    assert report["graphed_f16"] == "ok", report["graphed_f16"]


def test_active_dropout_keeps_the_matrix_under_the_switch(report):
    assert report["keeps_dropout"] == "ok", report["keeps_dropout"]


def test_fp32_pipe_weight_gradient_keeps_the_matrix_under_the_switch(report):
    assert report["keeps_wgrad_f32"] == "ok", report["keeps_wgrad_f32"]


def test_bf16_mode_keeps_its_own_in_place_route_under_the_switch(report):
    assert report["keeps_bf16_mode"] == "ok", report["keeps_bf16_mode"]


def test_frozen_featurizer_keeps_the_inference_routing_under_the_switch(report):
    assert report["keeps_inference"] == "ok", report["keeps_inference"]


def test_certified_and_uncertified_forward_give_the_same_step(report):
    """A store of fp16 values with its certificate forced True (two products forward) and False (three): the fp32 store's step both times."""
    assert report["certificate"] == "ok", report["certificate"]
