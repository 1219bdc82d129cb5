"""The dropout mask rule on the host: the numpy restatement of csrc/dfol_dropout.hip (tests/dropout_rule.py) against the published
Philox4x32-10 known-answer vectors, and the statistics a mask must have.  Seeds and sizes are fixed: nothing here is random between runs."""

import numpy as np
import pytest

from tests import dropout_rule as R

# Random123 (Salmon et al., SC'11), kat_vectors: philox4x32, 10 rounds: counter, key -> output
KNOWN_ANSWERS = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
ROWS, COLS = 1024, 1024                     # 2^20 elements
N = ROWS * COLS
SEED = 20240613
PS = (0.1, 0.2, 0.5)
SITES = (0, 1, 5)


def test_philox_known_answers():
    for counter, key, out in KNOWN_ANSWERS:
        assert tuple(int(w) for w in R.philox4x32_10(counter, key)) == out
    # vectorised over counters: the same words as one at a time
    c = np.array([k[0] for k in KNOWN_ANSWERS[:1] * 3], dtype=np.uint64).T
    got = R.philox4x32_10(tuple(c), KNOWN_ANSWERS[0][1])
    assert all(tuple(int(w[i]) for w in got) == KNOWN_ANSWERS[0][2] for i in range(3))


def test_host_generator_of_the_library_agrees():
    from dfol_vqa_amd import _lib
    for counter, key, out in KNOWN_ANSWERS:
        assert _lib.philox4x32_10(counter, key) == out
    for seed, rank in ((7, 0), (7, 1), (2 ** 63 + 5, 3)):
        rec = _lib._dropout_record(seed, rank)
        k0, k1 = R.stream_key(seed, 0, rank)
        assert rec[0] & 0xFFFFFFFFFFFFFFFF == seed and rec[1] == 0 and rec[3] == rank
        assert rec[2] & 0xFFFFFFFFFFFFFFFF == k0 | (k1 << 32)


def test_threshold_and_scale():
    assert R.threshold(0.5) == 2 ** 31 and R.threshold(0.0) == 0
    assert R.threshold(0.1) == int(np.float32(0.1).astype(np.float64) * 2 ** 32)        # the fp32 value of p, floor of an exact product
    assert R.scale(0.5) == np.float32(2.0) and R.scale(0.2).dtype == np.float32


def test_rows_are_64_bit():
    key = R.stream_key(SEED, 1)
    lo = R.words(2, 8, 0, key, row0=3)
    hi = R.words(2, 8, 0, key, row0=3 + 2 ** 32)             # the same low word, another high word: other masks
    assert not np.array_equal(lo, hi)
    w = R.philox4x32_10((3, 1, 1, 0), key)                    # row 3 + 2^32, group 1, site 0
    assert [int(v) for v in w] == [int(v) for v in hi[0, 4:8]]


def test_tail_uses_the_leading_words():
    key = R.stream_key(SEED, 1)
    assert np.array_equal(R.words(5, 7, 2, key), R.words(5, 8, 2, key)[:, :7])


@pytest.mark.parametrize("p", PS)
def test_kept_share(p):
    key = R.stream_key(SEED, 1)
    for site in SITES:
        kept = R.keep_mask(ROWS, COLS, p, site, key).mean()
        sigma = np.sqrt(p * (1 - p) / N)
        assert abs(kept - (1 - p)) < 5 * sigma, (p, site, kept)


@pytest.mark.parametrize("p", PS)
def test_masks_of_sites_steps_and_ranks_differ(p):
    base = R.keep_mask(ROWS, COLS, p, 0, R.stream_key(SEED, 1, 0))
    others = {"site": R.keep_mask(ROWS, COLS, p, 1, R.stream_key(SEED, 1, 0)),
              "step": R.keep_mask(ROWS, COLS, p, 0, R.stream_key(SEED, 2, 0)),
              "rank": R.keep_mask(ROWS, COLS, p, 0, R.stream_key(SEED, 1, 1))}
    q = 2 * p * (1 - p)                                       # two independent masks differ where exactly one of them keeps
    sigma = np.sqrt(q * (1 - q) / N)
    for what, m in others.items():
        share = (m != base).mean()
        assert abs(share - q) < 5 * sigma, (p, what, share, q)


def _lag1(m, axis):
    a = m.astype(np.float64)
    a -= a.mean()
    x, y = (a[:-1], a[1:]) if axis == 0 else (a[:, :-1], a[:, 1:])
    return float((x * y).mean() / a.var()), x.size


@pytest.mark.parametrize("p", PS)
def test_no_lag1_correlation(p):
    key = R.stream_key(SEED, 1)
    for site in SITES:
        m = R.keep_mask(ROWS, COLS, p, site, key)
        for half in (m[:ROWS // 2], m[ROWS // 2:]):
            for axis in (0, 1):
                r, n = _lag1(half, axis)
                assert abs(r) < 5 / np.sqrt(n), (p, site, axis, r)
