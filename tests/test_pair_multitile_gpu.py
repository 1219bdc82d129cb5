"""The fp16x2 pair kernel with several pair tiles per workgroup (csrc/dfol_pair_h2.hip, DFOL_PAIR_TILES): every tile is computed by the
same instructions in the same K order whatever the number of tiles a workgroup runs, so the relation tiles must be BITWISE those of one
tile per workgroup - at the bench shape, on ragged shared scenes with several requested columns, with 1- and 2-object images, images
without a requested column and tile counts that are not a multiple of the tiles per workgroup."""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HID1, HID2, C = 256, 300, 333


@pytest.fixture(scope="module")
def L():
    from dfol_vqa_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return _lib


@pytest.fixture(scope="module")
def weights(L):
    g = torch.Generator().manual_seed(7)
    dev = torch.device("cuda")
    wg = (torch.randn(HID1, 4, generator=g) * 0.3).to(dev)
    w2 = torch.zeros(320, HID1)
    w2[:HID2] = torch.randn(HID2, HID1, generator=g) / 16
    b2 = torch.randn(HID2, generator=g).to(dev)
    emb = (torch.randn(C, HID2, generator=g) / 17).to(dev)
    be = torch.randn(C, generator=g).to(dev)
    return wg, L.pair_pack_w2_h2(w2.to(dev), HID2), b2, emb, be


def _scene(n_list, K, seed, drop_q=(), orient=False):
    """Inputs of one launch: object counts n_list, K requested columns per image (-1 for the images in drop_q and some random slots)."""
    rng = np.random.RandomState(seed)
    dev = torch.device("cuda")
    Q, O = len(n_list), int(sum(n_list))
    off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int32)
    uv = torch.from_numpy(rng.randn(max(O, 1), 2 * HID1).astype(np.float32) * 0.5).to(dev)
    pos = torch.from_numpy(rng.rand(max(O, 1), 4).astype(np.float32) * 0.5 + 0.05).to(dev)
    req_col = rng.randint(0, C, size=(K, Q)).astype(np.int32)
    if K > 1:
        req_col[rng.rand(K, Q) < 0.2] = -1
    for q in drop_q:
        req_col[:, q] = -1
    req_tile = np.arange(K * Q, dtype=np.int32).reshape(K, Q)
    req_orient = torch.from_numpy(rng.randint(0, 2, size=(K, Q)).astype(np.uint8)).to(dev) if orient else None
    return dict(uv=uv, pos=pos, n_obj=torch.from_numpy(np.asarray(n_list, np.int32)).to(dev), off=torch.from_numpy(off).to(dev),
                max_n=int(max(n_list)), req_col=torch.from_numpy(req_col).to(dev), req_tile=torch.from_numpy(req_tile).to(dev),
                req_orient=req_orient, K=K, Q=Q)


def _run(L, weights, s, tiles_per_wg, bf16=False):
    wg, w2h, b2, emb, be = weights
    NS = (s["max_n"] + 7) // 8 * 8
    tiles = torch.full((s["K"] * s["Q"], NS, NS), -30.0, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
    old = os.environ.get("DFOL_PAIR_TILES")
    os.environ["DFOL_PAIR_TILES"] = str(tiles_per_wg)          # (read by the launcher at every call)
    try:
        L.pair_ll_h2(s["uv"], HID1, s["pos"], wg, w2h, b2, HID2, emb, be, s["n_obj"], s["off"], s["max_n"], s["req_col"], s["req_tile"],
                     s["req_orient"], tiles)
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop("DFOL_PAIR_TILES", None)
        else:
            os.environ["DFOL_PAIR_TILES"] = old
    return tiles.view(torch.int16 if bf16 else torch.int32).cpu().numpy()


def _same_bits(L, weights, s, bf16=False):
    ref = _run(L, weights, s, 1, bf16)
    assert (ref != _run(L, weights, {**s, "req_col": torch.full_like(s["req_col"], -1)}, 1, bf16)).any(), "the launch wrote nothing"
    for t in (2, 3, 8):
        got = _run(L, weights, s, t, bf16)
        assert np.array_equal(ref, got), "T = %d: %d of %d values differ from T = 1" % (t, int((ref != got).sum()), ref.size)


def test_multitile_bench_shape(L, weights):
    _same_bits(L, weights, _scene([100] * 256, 1, seed=1))


def test_multitile_ragged_shared_scenes(L, weights):
    # c3: ragged 10..100 objects, 8 questions per image (one image per question slot here), K > 1 columns, both orientations
    rng = np.random.RandomState(3)
    n_list = list(np.repeat(rng.randint(10, 101, size=12), 8))
    _same_bits(L, weights, _scene(n_list, 3, seed=4, orient=True))


def test_multitile_edge_images(L, weights):
    # 1- and 2-object images (npairs 0 and 2), images without a requested column, and 3 + 2 x 7 + ... tiles: no multiple of 2, 3 or 8
    n_list = [40, 1, 2, 40, 7, 1, 40, 2, 33, 40, 17]
    _same_bits(L, weights, _scene(n_list, 2, seed=5, drop_q=(3, 8)))
    _same_bits(L, weights, _scene(n_list, 1, seed=6, drop_q=(0, 4, 10)))


def test_multitile_bf16_tiles(L, weights):
    rng = np.random.RandomState(8)
    _same_bits(L, weights, _scene(list(rng.randint(1, 101, size=40)), 2, seed=9), bf16=True)


def test_default_is_deterministic(L, weights):
    wg, w2h, b2, emb, be = weights
    s = _scene([100] * 64 + [57] * 9, 1, seed=10)
    default = os.environ.pop("DFOL_PAIR_TILES", None)
    try:
        outs = []
        for _ in range(3):
            tiles = torch.full((s["Q"], 104, 104), -30.0, device="cuda")
            L.pair_ll_h2(s["uv"], HID1, s["pos"], wg, w2h, b2, HID2, emb, be, s["n_obj"], s["off"], s["max_n"], s["req_col"], s["req_tile"],
                         None, tiles)
            outs.append(tiles.view(torch.int32).cpu().numpy())
    finally:
        if default is not None:
            os.environ["DFOL_PAIR_TILES"] = default
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    assert np.array_equal(outs[0], _run(L, weights, s, 1))
