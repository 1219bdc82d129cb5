"""CPU tests of the bf16 feature store's host half (feature_store.DeviceFeatureStore(feature_dtype="bf16")): the rounding rule restated in
numpy - what tests/test_store_bf16_gpu.py compares dfol_store_round_bf16 with - against torch's own conversion, the byte accounting of the
layout, and the option's refusals that need no device."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import _lib  # noqa: E402
from dfol_vqa_amd.data import DeviceFeatureStore  # noqa: E402
from dfol_vqa_amd.feature_store import StoreLayout  # noqa: E402
from test_feature_store import write_chunks  # noqa: E402


def rne_bf16(x):
    """fp32 array -> the uint16 bit patterns of its elements rounded to bfloat16, to nearest, ties to even: add 0x7fff plus the kept part's last
    bit to the word and keep the top half.  The carry does the rest - into the exponent, and from the largest finite values into inf."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen_bf16(h):
    """uint16 bfloat16 bit patterns -> the fp32 values they stand for (exact)."""
    return (np.asarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32)


def rounding_inputs(seed=0, n=4000):
    """Ties both ways (the kept part even: down; odd: up), +-0, subnormals (fp32 ones, and ones bf16 still holds), the largest finite bf16,
    values that round up to inf, and a few thousand random values over the whole exponent range.  All finite."""
    words = [0x3F800000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,      # 1.0, ties to even / to odd + 1, just off a tie
             0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00010000, 0x807F8000,
             0x7F7F0000, 0xFF7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7FFFFF]
    rng = np.random.RandomState(seed)
    rand = rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    rand = rand[(rand & 0x7F800000) != 0x7F800000]                   # (no inf, no NaN)
    return np.concatenate([np.array(words, np.uint32), rand]).view(np.float32)


def test_the_restatement_is_torchs_conversion():
    x = rounding_inputs()
    assert np.isfinite(x).all() and x.size > 3000
    mine = rne_bf16(x)
    theirs = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(mine, theirs)
    # what the cases are there for
    one = lambda w: int(rne_bf16(np.array([w], np.uint32).view(np.float32))[0])
    assert one(0x3F808000) == 0x3F80 and one(0x3F818000) == 0x3F82            # ties: to the even neighbour, down and up
    assert one(0x7F7F0000) == 0x7F7F and one(0x7F7F8000) == 0x7F80 and one(0xFF7FFFFF) == 0xFF80      # the largest finite bf16 stays, beyond it: inf
    assert one(0x80000000) == 0x8000 and one(0x00008000) == 0x0000 and one(0x00018000) == 0x0002     # -0 kept; subnormal ties to even
    assert np.array_equal(rne_bf16(widen_bf16(mine)), mine)                 # a bf16 value rounds to itself


def test_layout_counts_the_bytes_actually_held(tmp_path):
    chunks, info = write_chunks(tmp_path, feature_dim=8, max_obj=6, counts=[1, 6, 4, 2, 6, 3], per_chunk=3)
    f32 = StoreLayout(str(tmp_path), "objs", chunks, info)
    bf16 = StoreLayout(str(tmp_path), "objs", chunks, info, feature_itemsize=2)
    other = 4 * (6 * 4 + 2)                                              # boxes and (W, H) stay fp32
    assert f32.row_bytes == 4 * 6 * 8 + other and bf16.row_bytes == 2 * 6 * 8 + other
    assert bf16.chunk_bytes == [3 * bf16.row_bytes] * 2
    # a budget that admits one fp32 chunk admits the chunks the bf16 store's own bytes give
    budget = f32.chunk_bytes[0]
    assert len(f32.index("a", budget)[2]) - 1 == 1
    assert len(bf16.index("b", budget)[2]) - 1 == budget // bf16.chunk_bytes[0] == 1
    assert len(bf16.index("c", 2 * bf16.chunk_bytes[0])[2]) - 1 == 2 and len(f32.index("d", 2 * bf16.chunk_bytes[0])[2]) - 1 == 1


def test_option_refusals_without_a_device(tmp_path):
    chunks, info = write_chunks(tmp_path, feature_dim=8)
    with pytest.raises(_lib.DfolError, match="featurized=True"):
        DeviceFeatureStore(str(tmp_path), "objs", chunks, info, "cuda:0", featurized=True, feature_dtype="bf16")
    with pytest.raises(_lib.DfolError, match="feature_dtype must be"):
        DeviceFeatureStore(str(tmp_path), "objs", chunks, info, "cuda:0", feature_dtype="f16")
