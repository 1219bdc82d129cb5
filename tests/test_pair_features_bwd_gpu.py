"""GPU test of dfol_pair_features_bwd_f32 (csrc/dfol_dropout.hip): the pair matrix's backward without atomics, against float64 index_add_."""

import numpy as np
import pytest
import torch

from dfol_vqa_amd import _lib
from dfol_vqa_amd import ops as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_LIST = [3, 0, 1, 37, 2, 1, 3]                       # ragged: images of 0, 1, 2, 3 and 37 objects


def geometry(n_list):
    n = np.asarray(n_list, np.int64)
    obj_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    pair_off = np.concatenate([[0], np.cumsum(n * (n - 1))]).astype(np.int64)
    ind_s, ind_o = [], []
    for q, k in enumerate(n_list):                    # fol_types.BatchWorld.pair_index: row pair_off + s (n - 1) + (o < s ? o : o - 1)
        for s in range(k):
            for o in range(k):
                if o != s:
                    ind_s.append(obj_off[q] + s)
                    ind_o.append(obj_off[q] + o)
    return obj_off, pair_off, np.asarray(ind_s, np.int64), np.asarray(ind_o, np.int64)


@pytest.mark.parametrize("D", [10, 516])
@pytest.mark.parametrize("pad", [0, 3])
def test_ordered_backward_equals_float64_index_add(D, pad):
    obj_off, pair_off, ind_s, ind_o = geometry(N_LIST)
    O, pairs, Q, max_n = int(obj_off[-1]), int(pair_off[-1]), len(N_LIST), max(N_LIST)
    assert len(ind_s) == pairs
    gen = torch.Generator().manual_seed(D + pad)
    buf = torch.randn(pairs, 2 * D + 4 + pad, generator=gen) * torch.exp(2 * torch.randn(pairs, 1, generator=gen))
    g = buf[:, :2 * D + 4]                             # pad = 3: rows of another stride
    ref = torch.zeros(O, D, dtype=torch.float64)
    mag = torch.zeros(O, D, dtype=torch.float64)
    for ind, cols in ((ind_s, slice(0, D)), (ind_o, slice(D, 2 * D))):
        ref.index_add_(0, torch.from_numpy(ind), g[:, cols].double())
        mag.index_add_(0, torch.from_numpy(ind), g[:, cols].double().abs())
    dev = lambda a: torch.from_numpy(a).to(DEV)
    args = (D, dev(obj_off), dev(pair_off), Q, max_n, O)
    gd = buf.to(DEV)[:, :2 * D + 4]
    got = _lib.pair_features_bwd(gd, *args)
    again = _lib.pair_features_bwd(gd, *args)
    assert tuple(got.shape) == (O, D)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), again.cpu().numpy().view(np.uint32))
    n_of = np.repeat(np.asarray(N_LIST), N_LIST)                                 # each object's image size
    bound = torch.from_numpy(np.maximum(n_of - 1, 0).astype(np.float64))[:, None] * 2.0 ** -23 * mag
    err = (got.cpu().double() - ref).abs()
    print("D=%d pad=%d: max error %.3g, max bound %.3g" % (D, pad, float(err.max()), float(bound.max())))
    assert bool((err <= bound).all())
    lone = np.nonzero(n_of == 1)[0]
    assert len(lone) == 2 and bool((got[torch.from_numpy(lone).to(DEV)] == 0).all())     # an image of one object: a written zero row


def test_autograd_route():
    """ops.pair_features(ordered=True) under autograd gives index_add_'s gradient (to rounding) and repeats bit for bit; ordered=False keeps
    index_add_ (the dropout-0 full-table route's bits are not this pull request's to change)."""
    D = 12
    obj_off, pair_off, ind_s, ind_o = geometry(N_LIST)
    O, pairs = int(obj_off[-1]), int(pair_off[-1])
    dev = lambda a: torch.from_numpy(a).to(DEV)
    gen = torch.Generator().manual_seed(2)
    obj = torch.randn(O, D, generator=gen).to(DEV).requires_grad_(True)
    w = torch.randn(pairs, 2 * D + 4, generator=gen).to(DEV)
    index = lambda: (dev(ind_s), dev(ind_o))
    grads = []
    _lib.PATH_COUNTS.clear()
    for ordered in (True, True, False):
        pair = L.pair_features(obj, D, dev(obj_off), dev(pair_off), len(N_LIST), max(N_LIST), pairs, pair_index=index, ordered=ordered)
        (g,) = torch.autograd.grad((pair * w).sum(), obj)
        grads.append(g)
    assert _lib.PATH_COUNTS["pair_features_bwd_ordered"] == 2
    assert torch.equal(grads[0], grads[1])
    assert torch.allclose(grads[0], grads[2], rtol=1e-5, atol=1e-5)


def test_guards():
    h = _lib.load()
    assert h.dfol_pair_features_bwd_f32(None, 24, 10, None, None, 0, 5, None, 10, None) == 0        # no images: no launch
    assert h.dfol_pair_features_bwd_f32(None, 19, 10, None, None, 1, 5, None, 10, None) != 0 and b"pair_features_bwd" in h.dfol_last_error()
    assert h.dfol_pair_features_bwd_f32(None, 24, 0, None, None, 1, 5, None, 10, None) != 0
    with pytest.raises(_lib.DfolError):
        _lib.pair_features_bwd(torch.zeros(6, 19, device=DEV), 10, None, None, 1, 3, 3)
