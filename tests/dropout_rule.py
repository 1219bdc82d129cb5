"""The dropout mask rule of csrc/dfol_dropout.hip restated in numpy, for the tests (host only: no device, no library).

    Philox4x32-10: ten rounds of (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), the key bumped by
    (0x9E3779B9, 0xBB67AE85) between rounds.
    key(seed, step, rank) = the first two words of Philox(counter = (step_lo, step_hi, rank, 0), key = (seed_lo, seed_hi)).
    The elements (row, 4g .. 4g + 3) of site s use the four words of Philox(counter = (row_lo, row_hi, g, s), key); element j is kept iff
    word[j] >= floor(p 2^32) as unsigned 64-bit values, p the fp32 value of the probability; kept values are scaled by fp32 1 / (1 - p).
"""

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two -> four uint32 arrays, broadcast together."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.uint64(int(v) & 0xFFFFFFFF) for v in key)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return [v.astype(np.uint32) for v in c]


def stream_key(seed, step, rank=0):
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((step & 0xFFFFFFFF, step >> 32, int(rank), 0), (seed & 0xFFFFFFFF, seed >> 32))
    return int(w[0]), int(w[1])


def threshold(p):
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def words(rows, cols, site, key, row0=0):
    """uint32 [rows, cols]: the word each element's keep test reads; row0: the (64-bit) number of the first row."""
    groups = (cols + 3) // 4
    r = np.arange(rows, dtype=np.uint64) + np.uint64(row0)
    w = philox4x32_10(((r & MASK32)[:, None], (r >> np.uint64(32))[:, None], np.arange(groups, dtype=np.uint64)[None, :], site), key)
    return np.stack(w, axis=-1).reshape(rows, 4 * groups)[:, :cols]


def keep_mask(rows, cols, p, site, key, row0=0):
    return words(rows, cols, site, key, row0).astype(np.uint64) >= np.uint64(threshold(p))


def apply(x, p, site, key):
    """The kernel's result on a float32 matrix: kept elements times fp32 1 / (1 - p), dropped ones +0.0 by selection."""
    x = np.asarray(x, np.float32)
    keep = keep_mask(x.shape[0], x.shape[1], p, site, key)
    with np.errstate(all="ignore"):
        return np.where(keep, x * scale(p), np.float32(0.0)).astype(np.float32)
