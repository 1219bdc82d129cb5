"""GPU tests of the route DFOL_STORE_BF16_DIRECT=1 opens: a model in the default arithmetic (two fp16 pieces, three products) whose featurizer
reads a bf16 feature store's rows in place on the inference path - Python loop, native executor, captured forward, range re-run - against an fp32
store over chunk files whose features are bf16 values already, so the two stores hold the same numbers and every comparison is bit equality.
With the switch unset the same calls count the materialised matrix, as before.

One child process runs all cases (tests/_store_bf16_direct_route_worker.py, DFOL_DENSE_WIDE=2: the library reads that switch once per process,
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
    for k in ("DFOL_NATIVE", "DFOL_DENSE_MATH", "DFOL_STORE_BF16_DIRECT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(HERE, "_store_bf16_direct_route_worker.py"), str(tmp_path_factory.mktemp("bf16_direct_route"))],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_switch_on_inference_reads_the_table_in_place_with_the_fp32_stores_bits(report):
    """DFOL_NATIVE 1 and 0, shared scenes on and off, `exist` and `verify_rel`: equal log-probabilities and answers;
    feature_store_direct == feature_store_direct_bf16_h2 == batches, feature_store_direct_materialized == 0."""
    assert report["inference_on"] == "ok", report["inference_on"]


def test_switch_unset_materialises_as_before_with_the_same_bits(report):
    assert report["inference_off"] == "ok", report["inference_off"]


def test_graphed_forward_serves_a_second_scene_through_rows_out(report):
    assert report["graphed"] == "ok", report["graphed"]


def test_range_rerun_from_the_in_place_kernels_flag(report):
    """Image 1 holds 2^17: the in-place kernel raises the flag, the batch runs again on 'bf16x3' over the materialised matrix and gives the fp32
    store's bits, with `fallback:range_rerun` counted."""
    assert report["range_rerun"] == "ok", report["range_rerun"]


def test_train_step_keeps_its_route_under_the_switch(report):
    assert report["train_step"] == "ok", report["train_step"]


def test_new_setter_refuses_another_first_layer(report):
    assert report["setter_refusal"] == "ok", report["setter_refusal"]
