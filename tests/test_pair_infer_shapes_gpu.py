"""The inference pair kernels (_lib.PAIR_KINDS: csrc/dfol_pair_h2.hip f16x2 / f16, dfol_pair_split.hip bf16x3, dfol_pair.hip packed,
dfol_dense.hip plain) against a vectorised float64 restatement on images of many tiles, with `req_tile` as a real map and with strided
operands; and the range of the epilogue's reciprocal pair decode (dfol_common.h: dfol_offdiag_slot_rcp, DFOL_OFFDIAG_RCP_MAX_N).

Shapes (object counts per image; widths 256 -> 300, 50 concepts, the weight scales of test_kernels_gpu.test_pair_ll_kernels_against_torch):
  cross     [33, 17, 1, 64, 2, 65], K = 2: the 32-wide / 64-wide block edges of the block kernels at, on and one past; pair rows of 16, 32 and 64
            slots under the 32-slot wavefronts of the h2 / split kernels; NS = 68 (no multiple of 8) and 72 (> max_n; fp32 and bf16 tiles)
  workload  [100, 57, 100, 2], NS = 104: 39 tiles of 256 slots per image; K = 3 and K = 26 (more request rows than the h2 kernel stages)
  big       [300, 12], NS = 300, K = 1

Tolerances are the project's: 2e-5 max(1, max |ref|) of test_pair_ll_kernels_against_torch for fp32 tiles, the 6 sigma + n32 rule of
test_pair_f16_gpu.test_accuracy_against_float64 (that file's error_model) for the one-product kernel, bf16 tiles = the fp32 tiles rounded to
nearest even and within 2^-8 |ref| + 1e-6.  Written cells are compared as boolean masks against the off-diagonal n x n cells of the requested
tiles, so a value in a wrong cell shows twice: as a cell written that should keep the -30 fill, and as a cell left unwritten.

The CPU-side tests (no `gpu` mark) hold the reference against the looped one of test_kernels_gpu, the shapes against what they are for, and
the decode against the integer division on the host."""

import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HID1, C = 256, 50
FILL = -30.0
SHAPES = {"cross": [33, 17, 1, 64, 2, 65], "workload": [100, 57, 100, 2], "big": [300, 12]}
COMMON_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dfol_vqa_amd", "csrc", "dfol_common.h")
H2_STAGE_FLOATS = 8192                                # csrc/dfol_pair_h2.hip: STAGE_FLOATS; SR = STAGE_FLOATS / (16 NB16) - 2 staged request rows


def rcp_max_n():
    with open(COMMON_H) as f:
        return int(re.search(r"#define\s+DFOL_OFFDIAG_RCP_MAX_N\s+(\d+)", f.read()).group(1))


def staged_rows(hid2):
    return H2_STAGE_FLOATS // (16 * ((hid2 + 15) // 16)) - 2


# ---- inputs (host side, fp32) ---------------------------------------------------------------------------------------------------------
def make_weights(hid2, seed):
    rng = np.random.RandomState(seed)
    w2 = np.zeros(((hid2 + 31) // 32 * 32, HID1), np.float32)
    w2[:hid2] = rng.normal(size=(hid2, HID1)).astype(np.float32) / np.sqrt(HID1)
    w = dict(hid2=hid2, wg=rng.uniform(-0.5, 0.5, (HID1, 4)).astype(np.float32), w2=w2, b2=rng.normal(size=hid2).astype(np.float32),
             emb=(rng.normal(size=(C, hid2)) / np.sqrt(hid2)).astype(np.float32), be=rng.normal(size=C).astype(np.float32))
    w["host"] = dict(w2=w2[:hid2].astype(np.float64))            # (what test_pair_f16_gpu.error_model reads)
    return w


def make_scene(n_list, K, seed, drop_q=()):
    """Object counts n_list, K request rows: random concepts, -1 in a fifth of the slots when K > 1 and in every slot of the images drop_q
    (every other image of two or more objects keeps a request), random orientations, the identity tile map."""
    rng = np.random.RandomState(seed)
    Q, O = len(n_list), int(sum(n_list))
    off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int32)
    uv = rng.uniform(-1, 1, (O, 2 * HID1)).astype(np.float32)
    pos = rng.uniform(0.05, 0.9, (O, 4)).astype(np.float32)
    req_col = rng.randint(0, C, (K, Q)).astype(np.int32)
    keep = req_col[0].copy()
    if K > 1:
        req_col[rng.uniform(size=(K, Q)) < 0.2] = -1
        lost = (req_col < 0).all(0)
        req_col[0, lost] = keep[lost]
        if not (req_col < 0).any():
            req_col[K - 1, 0] = -1
    for q in drop_q:
        req_col[:, q] = -1
    orient = (rng.uniform(size=(K, Q)) < 0.5).astype(np.uint8)
    if K * Q > 1:
        requested = np.argwhere(req_col >= 0)
        orient[tuple(requested[0])], orient[tuple(requested[-1])] = 0, 1
    return dict(n=list(n_list), K=K, Q=Q, O=O, off=off, uv=uv, pos=pos, req_col=req_col, orient=orient,
                req_tile=np.arange(K * Q, dtype=np.int32).reshape(K, Q), max_n=int(max(n_list)))


def permuted(sc, spare=3, seed=99):
    """The scene with K Q distinct tile indices in a fixed random order out of a buffer of K Q + spare tiles."""
    T = sc["K"] * sc["Q"] + spare
    req_tile = np.random.RandomState(seed).permutation(T)[:sc["K"] * sc["Q"]].astype(np.int32).reshape(sc["K"], sc["Q"])
    return {**sc, "req_tile": req_tile}, T


# ---- the float64 reference, vectorised ---------------------------------------------------------------------------------------------------
def reference64(w, sc, model=False):
    """The pair formula in float64 from the unrounded fp32 inputs, all ordered pairs of an image at once (the formula of
    test_kernels_gpu._pair_ref64 and test_pair_f16_gpu.reference64): per written cell (tile, row, column) and ll = LogSigmoid(x).
    model=True adds what test_pair_f16_gpu.error_model reads: the activations A [pairs, HID1] and per cell g_j = E_cj h_j (1 - h_j), the
    LogSigmoid's slope and the cell's row of A."""
    hid2 = w["hid2"]
    wg, w2, b2 = w["wg"].astype(np.float64), w["w2"][:hid2].astype(np.float64), w["b2"].astype(np.float64)
    emb, be = w["emb"].astype(np.float64), w["be"].astype(np.float64)
    uv, pos = sc["uv"].astype(np.float64), sc["pos"].astype(np.float64)
    cells, ll, G, slope, pair_of, A, rows_a = [], [], [], [], [], [], 0
    for q, n in enumerate(sc["n"]):
        ks = np.nonzero(sc["req_col"][:, q] >= 0)[0]
        if n < 2 or len(ks) == 0:
            continue
        s, o = np.nonzero(~np.eye(n, dtype=bool))                       # every (s, o), s != o, subject-major
        p = pos[sc["off"][q]:sc["off"][q] + n]
        dx = p[s, 0] + p[s, 2] / 2 - p[o, 0] - p[o, 2] / 2
        dy = p[s, 1] + p[s, 3] / 2 - p[o, 1] - p[o, 3] / 2
        dist = np.sqrt(dx * dx + dy * dy)
        geo = np.stack([dist, np.arcsin(dy / np.maximum(dist, 1e-10)), np.sign(p[o, 0] - p[s, 0]), np.sign(p[o, 1] - p[s, 1])], 1)
        rows = uv[sc["off"][q]:sc["off"][q] + n]
        z = rows[s, :HID1] + rows[o, HID1:] + geo @ wg.T
        a = np.where(z > 0, z, np.expm1(z))
        hid = 1.0 / (1.0 + np.exp(-(a @ w2.T + b2)))
        cols = sc["req_col"][ks, q]
        x = hid @ emb[cols].T + be[cols]                                 # [pairs, requests]
        for j, k in enumerate(ks):
            flip = bool(sc["orient"][k, q])
            cells.append(np.stack([np.full(len(s), sc["req_tile"][k, q]), o if flip else s, s if flip else o], 1))
            ll.append(np.minimum(x[:, j], 0.0) - np.log1p(np.exp(-np.abs(x[:, j]))))
            if model:
                G.append(emb[cols[j]] * hid * (1.0 - hid))
                slope.append(1.0 / (1.0 + np.exp(x[:, j])))
                pair_of.append(rows_a + np.arange(len(s)))
        if model:
            A.append(a)
            rows_a += len(s)
    out = dict(cells=np.concatenate(cells), ll=np.concatenate(ll))
    if model:
        out.update(G=np.concatenate(G), slope=np.concatenate(slope), pair_of=np.concatenate(pair_of), A=np.concatenate(A))
    return out


def dense(ref, T, NS):
    out = np.full((T, NS, NS), FILL)
    t, r, c = ref["cells"].T
    out[t, r, c] = ref["ll"]
    return out


def expected_mask(sc, T, NS):
    """The cells a launch must write, from the requests alone: off the diagonal of the n x n corner of every requested tile."""
    mask = np.zeros((T, NS, NS), bool)
    for q, n in enumerate(sc["n"]):
        for k in range(sc["K"]):
            if sc["req_col"][k, q] >= 0 and n >= 2:
                mask[sc["req_tile"][k, q], :n, :n] |= ~np.eye(n, dtype=bool)
    return mask


def reference_tiles(ref, sc, T, NS):
    """-> (dense float64 tiles, mask of written cells); the reference's own cells are exactly the expected ones, each once."""
    count = np.zeros((T, NS, NS), np.int64)
    np.add.at(count, tuple(ref["cells"].T), 1)
    mask = expected_mask(sc, T, NS)
    assert np.array_equal(count, mask.astype(np.int64)), "the reference writes other cells than the requests name"
    return dense(ref, T, NS), mask


@functools.lru_cache(maxsize=None)
def reference_self_check():
    """The vectorised reference against the looped test_kernels_gpu._pair_ref64 on [7, 1, 13, 2] to 1e-12 - before any launch relies on it."""
    from test_kernels_gpu import _pair_ref64
    w = make_weights(300, 5)
    sc = make_scene([7, 1, 13, 2], 3, 6, drop_q=(3,))
    sc, T = permuted(sc, spare=0, seed=7)                                # (the looped one allocates K Q tiles: a permutation without spares)
    NS = 16
    looped = _pair_ref64(sc["n"], sc["off"], sc["uv"], sc["pos"], w["wg"], w["w2"], w["b2"], w["emb"], w["be"], sc["req_col"], sc["req_tile"],
                         sc["orient"], HID1, 300, sc["K"], NS)
    mine, mask = reference_tiles(reference64(w, sc), sc, T, NS)
    assert mask.sum() > 300 and (sc["orient"][sc["req_col"] >= 0] == 1).any() and (sc["orient"][sc["req_col"] >= 0] == 0).any()
    diff = np.abs(mine - looped).max()
    assert diff <= 1e-12, diff
    return True


def test_vectorised_reference_matches_the_looped_one():
    assert reference_self_check()


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(name):
    """cross: image 4 (two objects) without a request; workload3 / workload26: K = 3 / 26; big: K = 1."""
    if name == "cross":
        return make_scene(SHAPES["cross"], 2, 31, drop_q=(4,))
    if name == "workload3":
        return make_scene(SHAPES["workload"], 3, 32)
    if name == "workload26":
        return make_scene(SHAPES["workload"], 26, 33)
    assert name == "big"
    return make_scene(SHAPES["big"], 1, 34)


NS_OF = {"cross": (68, 72), "workload3": (104,), "workload26": (104,), "big": (300,)}


def test_the_shapes_cover_what_they_are_for():
    cross, w3, w26, big = scene("cross"), scene("workload3"), scene("workload26"), scene("big")
    assert cross["n"] == [33, 17, 1, 64, 2, 65] and cross["K"] == 2 and cross["max_n"] == 65
    assert w3["n"] == w26["n"] == [100, 57, 100, 2] and w3["K"] == 3 and big["n"] == [300, 12] and big["K"] == 1
    for sc in (cross, w3, w26):
        asked = sc["req_col"] >= 0
        assert (~asked).any() and set(map(int, sc["orient"][asked])) == {0, 1}            # a -1 request; both orientations among the requested tiles
    assert not (cross["req_col"][:, 4] >= 0).any()                              # one image with no request ...
    assert all((sc["req_col"][:, q] >= 0).any() for sc in (cross, w3, w26, big) for q, n in enumerate(sc["n"]) if n >= 2 and not (sc is cross and q == 4))
    assert -(-100 * 99 // 256) == 39 > 8                                        # tiles of 256 slots per image on workload
    for sc in (cross, w3):
        rows = [n - 1 for n in sc["n"] if n >= 2]
        assert any(32 % r != 0 for r in rows) and any(r < 32 for r in rows)     # wavefronts that start mid-row; rows shorter than a wavefront
    assert {33, 64, 65} <= set(cross["n"])                                      # one past the 32-wide block edge; on and one past the 64-wide one
    assert 68 % 8 != 0 and 68 % 4 == 0 and all(ns > cross["max_n"] for ns in NS_OF["cross"]) and 104 > w3["max_n"]
    assert staged_rows(300) == 24 and w26["K"] == 26 > staged_rows(300) and w3["K"] < staged_rows(300)
    assert [(h + 15) // 16 for h in (270, 288, 300, 320)] == [17, 18, 19, 20]   # the h2 kernel's four NB16 arms
    assert 1 in cross["n"] and 2 in cross["n"] and 2 in w3["n"]
    for name in ("cross", "workload3"):                                         # the permuted map: distinct tiles, three of them spare, not the identity
        sc, T = permuted(scene(name))
        assert T == sc["K"] * sc["Q"] + 3 and len(set(sc["req_tile"].ravel())) == sc["K"] * sc["Q"] and sc["req_tile"].max() < T
        assert not np.array_equal(sc["req_tile"], scene(name)["req_tile"])


def test_the_reciprocal_decode_on_the_host():
    """dfol_offdiag_slot_rcp restated in float32 NumPy - (float)e + 0.5f, times a reciprocal, truncated - with the correctly rounded
    reciprocal and with it one ulp up and one ulp down, against the integer division, for every pair of an image of n objects up to the bound
    the launchers enforce.  (It backs the derivation in dfol_common.h - the arithmetic, not the hardware's reciprocal.)"""
    bound = rcp_max_n()
    assert 300 < bound <= 1672                                                  # (1672: the derivation's own limit)
    for n in (2, 3, 33, 65, 100, 300, bound):
        m = n - 1
        e = np.arange(n * m, dtype=np.int64)
        s_int = e // m
        x = e.astype(np.float32) + np.float32(0.5)
        assert x.dtype == np.float32 and np.array_equal(x.astype(np.float64), e + 0.5)
        r0 = np.float32(1.0) / np.float32(m)
        for r in (r0, np.nextafter(r0, np.float32(0)), np.nextafter(r0, np.float32(2))):
            p = x * np.float32(r)
            assert p.dtype == np.float32
            s = p.astype(np.int32).astype(np.int64)                             # (truncation, as the kernel's (int))
            assert np.array_equal(s, s_int), (n, float(r), int((s != s_int).sum()))
            oo = e - s * m
            o = oo + (oo >= s)
            assert ((o != s) & (o >= 0) & (o < n)).all()


# ---- GPU side -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from dfol_vqa_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    assert reference_self_check()
    return _lib


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_DEVICE_WEIGHTS = {}


def device_weights(L, w, kind):
    """The weights on the device with the second layer in the form of `kind` (a key of _lib.PAIR_KINDS), built once."""
    key = (id(w), kind)
    if key not in _DEVICE_WEIGHTS:
        row = L.PAIR_KINDS[kind]
        w2 = dev(w["w2"])
        _DEVICE_WEIGHTS[key] = dict(wg=dev(w["wg"]), b2=dev(w["b2"]), emb=dev(w["emb"]), be=dev(w["be"]),
                                    image=w2 if row.pack is None else getattr(L, row.pack)(w2, w["hid2"]))
    return _DEVICE_WEIGHTS[key]


@functools.lru_cache(maxsize=None)
def weights(hid2=300):
    return make_weights(hid2, 1000 + hid2)


def launch(L, kind, w, sc, T, NS, bf16=False, tiles_per_wg=None, uv=None, pos=None, max_n=None, tiles=None):
    """One launch of `kind` into T tiles of NS x NS filled with -30; uv / pos: device tensors instead of the scene's (for the two fp16 kinds
    uv is then taken as already in the kernel's units); tiles: the caller's buffer instead.  -> the tiles (device)."""
    row, d = L.PAIR_KINDS[kind], device_weights(L, w, kind)
    if tiles is None:
        tiles = torch.full((T, NS, NS), FILL, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
    extra = dict(uv_prescaled=True) if (uv is not None and row.ln2_units) else {}
    uv_d, pos_d = dev(sc["uv"]) if uv is None else uv, dev(sc["pos"]) if pos is None else pos
    tail = (d["emb"], d["be"], dev(np.asarray(sc["n"], np.int32)), dev(sc["off"]), sc["max_n"] if max_n is None else max_n, dev(sc["req_col"]),
            dev(sc["req_tile"]), dev(sc["orient"]), tiles)
    old = os.environ.get("DFOL_PAIR_TILES")
    if tiles_per_wg is not None:
        os.environ["DFOL_PAIR_TILES"] = str(tiles_per_wg)          # (read by the launcher at every call)
    try:
        if row.pack is None:
            getattr(L, row.launch)(uv_d, HID1, pos_d, d["wg"], d["image"], d["b2"], *tail, hid2=w["hid2"])
        else:
            getattr(L, row.launch)(uv_d, HID1, pos_d, d["wg"], d["image"], d["b2"], w["hid2"], *tail, **extra)
        torch.cuda.synchronize()
    finally:
        if tiles_per_wg is not None:
            if old is None:
                os.environ.pop("DFOL_PAIR_TILES", None)
            else:
                os.environ["DFOL_PAIR_TILES"] = old
    return tiles


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def check_written(what, tiles, mask):
    """Written cells (bits other than the fill's) are exactly `mask`: nothing beside it, nothing of it left out."""
    fill = bits(torch.full((1,), FILL, dtype=tiles.dtype))[0]
    written = bits(tiles) != fill
    stray, missing = int((written & ~mask).sum()), int((mask & ~written).sum())
    assert stray == 0 and missing == 0, "%s: %d cells written that must keep the fill, %d of %d cells not written" % (what, stray, missing, int(mask.sum()))


def check_f32(what, tiles, refd, mask):
    """fp32 tiles of a full-precision kind: the written cells, and max |got - ref| <= 2e-5 max(1, max |ref|) over them."""
    check_written(what, tiles, mask)
    err = np.abs(tiles.cpu().numpy().astype(np.float64) - refd)[mask].max()
    bound = 2e-5 * max(1.0, np.abs(refd[mask]).max())
    print("pair shapes %s: max |got - ref64| %.3e (bound %.3e)" % (what, err, bound))
    assert err <= bound, (what, err, bound)
    return err


def check_bf16(what, tiles16, tiles32, refd, mask):
    """bf16 tiles: the fp32 tiles of the same kernel rounded to nearest even, bit for bit; within 2^-8 |ref| + 1e-6 of float64."""
    check_written(what, tiles16, mask)
    assert np.array_equal(bits(tiles16), bits(tiles32.to(torch.bfloat16))), what + ": not the fp32 tiles rounded to nearest even"
    err = np.abs(tiles16.float().cpu().numpy().astype(np.float64) - refd)[mask]
    print("pair shapes %s: max |got - ref64| / (2^-8 |ref| + 1e-6) %.3f" % (what, (err / (2.0 ** -8 * np.abs(refd[mask]) + 1e-6)).max()))
    assert np.all(err <= 2.0 ** -8 * np.abs(refd[mask]) + 1e-6), what


def check_h1(what, tiles, ref, sigma, n32, mask):
    """The one-product kernel: the written cells, and |got - ref| <= 6 sigma + n32 in each (test_pair_f16_gpu.test_accuracy_against_float64:
    sigma from its error_model, n32 = the f16x2 kernel's largest error on the same inputs)."""
    check_written(what, tiles, mask)
    t, r, c = ref["cells"].T
    e1 = np.abs(tiles.cpu().numpy().astype(np.float64)[t, r, c] - ref["ll"])
    ratio = (e1 / (6 * sigma + n32)).max()
    print("pair shapes %s: max |got - ref64| %.3e, max |e| / (6 sigma + n32) %.3f (n32 %.3e, rms sigma %.3e)"
          % (what, e1.max(), ratio, n32, np.sqrt((sigma ** 2).mean())))
    bad = e1 > 6 * sigma + n32
    assert not bad.any(), "%s: %d of %d cells beyond 6 sigma + n32, worst ratio %.2f" % (what, int(bad.sum()), len(e1), ratio)


@pytest.fixture(scope="module")
def refs():
    """(scene name, hid2) -> (weights, scene, reference): computed once, never written to afterwards.  The one-product kernel's error model
    (sigma per cell) is kept beside it where that kernel runs: every case of 300 hidden units but K = 26."""
    assert reference_self_check()
    cache = {}

    def get(name, hid2=300):
        if (name, hid2) not in cache:
            from test_pair_f16_gpu import error_model
            w, sc = weights(hid2), scene(name)
            with_model = hid2 == 300 and name != "workload26"
            ref = reference64(w, sc, model=with_model)
            sigma = error_model(w, ref)[0] if with_model else None
            for key in ("G", "A", "slope", "pair_of"):                          # (hundreds of MB on `big`: only sigma is kept)
                ref.pop(key, None)
            cache[(name, hid2)] = (w, sc, ref, sigma)
        return cache[(name, hid2)]
    return get


def _run_case(L, refs, name, kind, hid2=300, with_bf16=False):
    """Every NS of the case; fp32 tiles (and bf16 ones) against float64; the two fp16 kinds at one tile per workgroup and at the default."""
    w, sc, ref, sigma = refs(name, hid2)
    T = sc["K"] * sc["Q"]
    fp16_kind = kind in ("f16x2", "f16")
    for NS in NS_OF[name]:
        refd, mask = reference_tiles(ref, sc, T, NS)
        n32 = None
        if kind == "f16":
            # (the allowance comes from the f16x2 kernel, so that kernel is held to its own bound first: a fault the two kernels share -
            # they share their epilogue - must not widen the one-product kernel's allowance until it hides itself)
            n32 = check_f32("%s f16x2 hid2=%d NS=%d (the yardstick of f16)" % (name, hid2, NS), launch(L, "f16x2", w, sc, T, NS), refd, mask)
        for tpw in ((1, None) if fp16_kind and name != "big" else (None,)):
            what = "%s %s hid2=%d NS=%d tiles/wg=%s" % (name, kind, hid2, NS, "default" if tpw is None else tpw)
            t32 = launch(L, kind, w, sc, T, NS, tiles_per_wg=tpw)
            if kind == "f16":
                check_h1(what, t32, ref, sigma, n32, mask)
            else:
                check_f32(what, t32, refd, mask)
            if with_bf16 and NS % 8 == 0 and L.PAIR_KINDS[kind].bf16_tiles:
                check_bf16(what + " bf16", launch(L, kind, w, sc, T, NS, bf16=True, tiles_per_wg=tpw), t32, refd, mask)


KINDS = ("plain", "packed", "bf16x3", "f16x2", "f16")


@pytest.mark.gpu
def test_the_kinds_are_the_table(L):
    assert set(KINDS) == set(L.PAIR_KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_cross(L, refs, kind):
    """[33, 17, 1, 64, 2, 65], K = 2, NS = 68 (fp32 tiles) and 72 (fp32 and bf16 tiles): every kind against float64."""
    _run_case(L, refs, "cross", kind, with_bf16=True)


@pytest.mark.gpu
@pytest.mark.parametrize("hid2", [270, 288, 320])
def test_cross_h2_widths(L, refs, hid2):
    """The f16x2 kernel's NB16 = 17, 18 and 20 arms on the cross shape."""
    _run_case(L, refs, "cross", "f16x2", hid2=hid2, with_bf16=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_workload(L, refs, kind):
    """[100, 57, 100, 2], NS = 104, K = 3 with orientations: 39 tiles per 100-object image."""
    _run_case(L, refs, "workload3", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f16x2", "bf16x3"])
def test_workload_more_requests_than_staged_rows(L, refs, kind):
    """The workload shape with K = 26 request rows: two more than the f16x2 kernel stages in LDS at 300 hidden units."""
    _run_case(L, refs, "workload26", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f16x2", "bf16x3", "packed", "f16"])
def test_big(L, refs, kind):
    """[300, 12], NS = 300, K = 1: 89 700 pairs of one image (351 tiles); the one-product kind too, its error model being quick enough here."""
    _run_case(L, refs, "big", kind)


MAP_CASES = [("cross", "f16x2"), ("cross", "bf16x3"), ("workload3", "f16x2")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", MAP_CASES)
def test_req_tile_is_a_map(L, refs, name, kind):
    """req_tile = K Q distinct indices in random order into a buffer of K Q + 3 tiles, NS > max_n: the values land where the map says, against
    the float64 reference placed through the same map; the three spare tiles keep the fill."""
    w, sc0, ref0, _ = refs(name)
    sc, T = permuted(sc0)
    NS = NS_OF[name][-1]
    ref = dict(cells=ref0["cells"].copy(), ll=ref0["ll"])
    ref["cells"][:, 0] = sc["req_tile"].ravel()[ref0["cells"][:, 0]]            # (the identity map numbers tile k Q + q)
    refd, mask = reference_tiles(ref, sc, T, NS)
    spare = sorted(set(range(T)) - set(sc["req_tile"].ravel().tolist()))
    assert len(spare) == 3 and not mask[spare].any()
    check_f32("%s %s permuted req_tile NS=%d" % (name, kind, NS), launch(L, kind, w, sc, T, NS), refd, mask)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", MAP_CASES)
def test_strided_operands(L, refs, name, kind):
    """uv = the first 512 columns of a [O, 520] matrix (row stride 520: a multiple of 4, base 16-byte aligned), pos = the first four columns
    of a [O, 6] matrix, the other columns NaN: the tiles are bit for bit those of the contiguous call.  (The wrappers take such views: _dp
    hands the pointer and the row stride on; no refusal to assert.  The fp16 kinds get uv already in their units - the wrapper's own scaling
    would make a contiguous copy.)"""
    w, sc, ref, _ = refs(name)
    T, NS = sc["K"] * sc["Q"], NS_OF[name][-1]
    uv = dev(sc["uv"])
    if L.PAIR_KINDS[kind].ln2_units:
        uv = uv * L.LOG2E
    pos = dev(sc["pos"])
    uv_wide = torch.full((sc["O"], 2 * HID1 + 8), float("nan"), device="cuda")
    pos_wide = torch.full((sc["O"], 6), float("nan"), device="cuda")
    uv_wide[:, :2 * HID1], pos_wide[:, :4] = uv, pos
    uv_view, pos_view = uv_wide[:, :2 * HID1], pos_wide[:, :4]
    assert uv_view.stride(0) == 520 and pos_view.stride(0) == 6 and uv_view.data_ptr() % 16 == 0 and not uv_view.is_contiguous()
    flat = launch(L, kind, w, sc, T, NS, uv=uv, pos=pos)
    strided = launch(L, kind, w, sc, T, NS, uv=uv_view, pos=pos_view)
    refd, mask = reference_tiles(ref, sc, T, NS)
    check_f32("%s %s contiguous, prescaled NS=%d" % (name, kind, NS), flat, refd, mask)
    assert np.array_equal(bits(flat), bits(strided)), "%d values differ from the contiguous call's" % int((bits(flat) != bits(strided)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f16x2", "f16", "bf16x3"])
def test_max_n_above_the_decode_range_is_refused(L, kind):
    """max_n = DFOL_OFFDIAG_RCP_MAX_N + 1 raises before any launch and writes nothing (one image of two objects, one request, tiles of the
    matching NS).  Nothing runs AT the bound: it rests on the derivation in dfol_common.h."""
    bound = rcp_max_n()
    w = weights(300)
    sc = make_scene([2], 1, 40)
    NS = (bound + 1 + 3) // 4 * 4
    tiles = torch.full((1, NS, NS), FILL, device="cuda")
    with pytest.raises(L.DfolError, match="max_n=%d" % (bound + 1)):
        launch(L, kind, w, sc, 1, NS, max_n=bound + 1, tiles=tiles)
    torch.cuda.synchronize()
    assert bool((tiles == FILL).all())
