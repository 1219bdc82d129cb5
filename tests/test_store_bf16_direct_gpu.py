"""GPU tests of the default arithmetic's product over a bf16 feature store's rows in place: dfol_linear_wide_rows_bf16t_h2_f32
(csrc/dfol_dense_wide.hip, BF16T).  The yardstick is code that existed before it, never the kernel itself: `_lib.linear_wide`
(dfol_linear_wide_h2_f32) over `table.float()[src_row]`, compared as uint32 bit patterns - no tolerance is involved.

One child process runs every case (tests/_store_bf16_direct_worker.py, DFOL_DENSE_WIDE=2: the library reads the switch once per process); the
tests read its report.  Shapes: M in {1, 127, 128, 129, 300} x N in {257, 300, 512} x K in {128, 132, 164, 2048} (132 and 164: the K % 8 == 4
tail) x row stride in {K, K + 4} x the base offset by 0 and 4 elements (the one 16-byte load and the two 8-byte loads), all four activations
with and without bias and into a column slice of a wider matrix, the index patterns identity / reversed / one row M times, more 128-row blocks
than CUs, and table rows beyond a 4 GB byte offset.  Values: random bf16 with zeros and -0, magnitudes near 2^-20 (a non-zero low fp16 piece),
and a table holding 2^17 - the range word must equal the yardstick route's and the outputs its bits, NaN included."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def report():
    env = dict(os.environ)
    env["DFOL_DENSE_WIDE"] = "2"
    env.pop("DFOL_DENSE_MATH", None)
    out = subprocess.run([sys.executable, os.path.join(HERE, "_store_bf16_direct_worker.py")], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_every_shape_stride_and_base_offset_has_the_yardsticks_bits(report):
    r = report["shapes"]
    assert r["cases"] == 5 * 3 * 4 * 2 * 2 and r["failed"] == 0, json.dumps(r["failures"])


def test_every_activation_bias_slice_and_index_pattern(report):
    r = report["activations"]
    assert r["cases"] == 4 * 2 * 2 * 3 * 3 and r["failed"] == 0, json.dumps(r["failures"])


def test_tiny_values_and_a_value_beyond_fp16s_range(report):
    """A low piece that is not zero; and 2^17: the in-place kernel raises DFOL_RANGE_X_OVERFLOW exactly where the yardstick route does and its
    outputs - NaN included - have the same bits."""
    r = report["values"]
    assert r["cases"] == 2 * 4 * 3 and r["failed"] == 0, json.dumps(r["failures"])


def test_a_workgroup_crosses_a_row_block(report):
    assert report["blocks"]["equal"] and report["blocks"]["finite"] and report["blocks"]["M"] % 128 == 5, report["blocks"]


def test_table_rows_beyond_a_four_gigabyte_offset(report):
    assert report["beyond_4gb"] == {"past": True, "equal": True, "finite": True}


def test_certificate_of_a_table_of_fp16_values(report):
    """dfol_store_bf16_is_f16: true for a table drawn from {0, +-[2^-10, 2^10]}; false after planting 2^-20 (1 + 2^-7), 2^17, inf or NaN, one at a
    time, at the first and at the last element."""
    c = report["certificate"]
    assert c.pop("clean") is True and c.pop("empty") is True
    assert len(c) == 8 and all(v is False for v in c.values()), c


def test_two_products_on_a_certified_table_have_the_yardsticks_bits(report):
    r = report["two_products"]
    assert r["cases"] == 5 * 3 * 4 * 2 * 2 and r["failed"] == 0, json.dumps(r["failures"])
    r = report["two_products_activations"]
    assert r["cases"] == 4 * 2 * 2 * 3 * 3 and r["failed"] == 0, json.dumps(r["failures"])


def test_a_request_for_two_products_on_an_uncertified_store_runs_three(report):
    r = report["uncertified_request"]
    assert r["cases"] == 2 * 4 * 3 and r["failed"] == 0, json.dumps(r["failures"])


def test_refusals_come_before_any_launch_with_a_message(report):
    assert all(v is True for v in report["refusals"].values()), report["refusals"]
    assert report["supported"] == [True, True, False, False, False, True]
