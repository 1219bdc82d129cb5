"""The listed pairs' kernels of the scene-graph step (csrc/dfol_scene_pairs.hip) on the GPU: dfol_scene_pair_rows_f32 against index_select / sign
(bit for bit) and a float64 restatement of distance and angle, dfol_scene_pair_rows_bwd_f32 against a float64 sum of the same blocks, and the
registered operator under torch.library.opcheck.

Bounds.  Distance and angle: four times the largest error the tensor-op expression of interpreter.build_scene_graph (fp32, the same inputs,
computed here on the CPU) shows against the float64 restatement over the case, plus one ulp of the value - the factor allows for the device's
asinf / sqrtf against torch's.  Boxes of the toleranced cases keep |dy| / dist <= 0.99: asin is ill-conditioned at +-1 and the bound must not
hide that.  The exact cases draw boxes on a 2^-6 grid, where every sum of the centre differences is exact in fp32 (off the grid the reference's
own expression x + w / 2 - x - w / 2 does not return 0 either).  Backward: every element within n 2^-23 sum|g| of its segment, n the segment's
length - the bound of a sequential fp32 sum."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import _lib, data, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def draw(O, D, P, seed):
    """obj [O, D] with boxes (x, y, w, h) in the last four columns and P pairs of distinct objects whose centre offsets keep |dy| / dist <= 0.99.
    One object: its box on the 2^-6 grid, every pair the object with itself."""
    for attempt in range(50):
        rng = np.random.RandomState(seed + 1000 * attempt)
        obj = rng.normal(size=(O, D)).astype(np.float32)
        if O == 1:
            obj[:, D - 4:] = rng.randint(0, 65, size=(1, 4)) / 64.0
            return obj, np.zeros(P, np.int32), np.zeros(P, np.int32)
        obj[:, D - 4:] = rng.uniform(0.0, 1.0, size=(O, 4))
        b = obj[:, D - 4:].astype(np.float64)
        cx, cy = b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2
        dx, dy = cx[:, None] - cx[None, :], cy[:, None] - cy[None, :]
        dist = np.hypot(dx, dy)
        ok = (np.abs(dy) <= 0.99 * dist) & (dist > 1e-3)
        np.fill_diagonal(ok, False)
        cand = np.argwhere(ok)
        if len(cand):
            pick = cand[rng.randint(len(cand), size=P)]
            return obj, pick[:, 0].astype(np.int32), pick[:, 1].astype(np.int32)
    raise AssertionError("no well-conditioned pair found")


def geometry64(obj, s, o):
    D = obj.shape[1]
    ps, po = obj[s, D - 4:].astype(np.float64), obj[o, D - 4:].astype(np.float64)
    dx = ps[:, 0] + ps[:, 2] / 2 - po[:, 0] - po[:, 2] / 2
    dy = ps[:, 1] + ps[:, 3] / 2 - po[:, 1] - po[:, 3] / 2
    dist = np.sqrt(dx * dx + dy * dy)
    return dist, np.arcsin(dy / np.maximum(dist, 1e-10))


def run(obj, s, o):
    return _lib.scene_pair_rows(torch.as_tensor(obj).to(DEV), torch.as_tensor(s).to(DEV), torch.as_tensor(o).to(DEV)).cpu()


@pytest.mark.parametrize("D", [8, 10, 516])
@pytest.mark.parametrize("O", [1, 3, 130])
@pytest.mark.parametrize("P", [1, 64, 65, 257])
def test_forward(D, O, P):
    obj, s, o = draw(O, D, P, seed=D + 7 * O + 13 * P)
    got = run(obj, s, o)
    assert tuple(got.shape) == (P, 2 * D + 4)
    t = torch.as_tensor(obj)
    want = ops.scene_pair_rows_reference(t, torch.as_tensor(s.astype(np.int64)), torch.as_tensor(o.astype(np.int64)))     # the parent's expression, fp32
    assert torch.equal(got[:, :2 * D], want[:, :2 * D]), "gathered columns"
    assert torch.equal(got[:, 2 * D + 2:], want[:, 2 * D + 2:]), "sign columns"
    if O == 1:                                                       # s == o on the grid: exact
        assert not got[:, 2 * D:].any() and not want[:, 2 * D:].any()
        return
    dist64, ang64 = geometry64(obj, s, o)
    assert (np.abs(np.sin(ang64)) <= 0.99 + 1e-9).all()
    for col, r64, name in ((2 * D, dist64, "dist"), (2 * D + 1, ang64, "angle")):
        g, w = got[:, col].double().numpy(), want[:, col].double().numpy()
        own, err = np.abs(w - r64).max(), np.abs(g - r64)
        ulp = np.spacing(np.abs(r64).astype(np.float32)).astype(np.float64)
        print("D %d O %d P %d %s: kernel error %.3g, the fp32 tensor-op expression's %.3g" % (D, O, P, name, err.max(), own))
        assert (err <= 4 * own + ulp).all(), (name, err.max(), own)


def test_no_pairs_returns_an_empty_matrix():
    obj = torch.zeros(5, 12, device=DEV)
    e = torch.zeros(0, dtype=torch.int32, device=DEV)
    assert tuple(_lib.scene_pair_rows(obj, e, e).shape) == (0, 28)
    csr = tuple(torch.as_tensor(a).to(DEV) for a in data.scene_pair_csr([], [], 5))
    out = ops.scene_pair_rows(obj.requires_grad_(True), e, e, csr)
    assert tuple(out.shape) == (0, 28)


def test_exact_cases():
    D = 12
    rng = np.random.RandomState(3)
    obj = rng.normal(size=(6, D)).astype(np.float32)
    # boxes on a 2^-6 grid (x, y, w, h): 0 and 1 side by side at one height, 2 above 3 at one x, 4 anywhere
    obj[:, D - 4:] = np.asarray([[8, 16, 4, 6], [40, 16, 4, 6], [20, 4, 10, 2], [20, 50, 10, 2], [33, 7, 5, 9], [1, 2, 3, 4]], np.float32) / 64.0
    s = np.asarray([4, 0, 1, 2, 3, 5], np.int32)
    o = np.asarray([4, 1, 0, 3, 2, 5], np.int32)
    got = run(obj, s, o)[:, 2 * D:].numpy()
    half_pi = np.float32(np.pi / 2)
    want = np.asarray([[0, 0, 0, 0],                                 # s == o
                       [0.5, 0, 1, 0], [0.5, 0, -1, 0],              # purely horizontal: dy = 0, the distance is |dx|, the angle asin(0)
                       [46 / 64.0, -half_pi, 0, 1], [46 / 64.0, half_pi, 0, -1],      # purely vertical: dx = 0, asin(-+1)
                       [0, 0, 0, 0]], np.float32)
    assert np.array_equal(got, want), (got, want)
    # an index outside [0, O) handed to the raw entry point: clamped to the first / last row, no fault
    t = torch.as_tensor(obj).to(DEV)
    bad_s = torch.as_tensor(np.asarray([-5, 900, 2], np.int32)).to(DEV)
    bad_o = torch.as_tensor(np.asarray([1, -1, 6], np.int32)).to(DEV)
    clamped = run(obj, np.asarray([0, 5, 2], np.int32), np.asarray([1, 0, 5], np.int32))
    assert torch.equal(_lib.scene_pair_rows(t, bad_s, bad_o).cpu(), clamped)


def backward_case(O, D, s, o, seed):
    rng = np.random.RandomState(seed)
    P = len(s)
    g = rng.normal(size=(P, 2 * D + 4)).astype(np.float32)
    seg_off, slot = data.scene_pair_csr(s, o, O)
    dev = lambda a: torch.as_tensor(a).to(DEV)
    runs = [_lib.scene_pair_rows_bwd(dev(g), D, dev(seg_off), dev(slot), O).cpu().numpy() for _ in range(2)]
    assert np.array_equal(runs[0].view(np.uint8), runs[1].view(np.uint8)), "two runs, other bits"
    want, mass, n = np.zeros((O, D)), np.zeros((O, D)), np.zeros(O)
    for p in range(P):
        for t, block in ((s[p], g[p, :D]), (o[p], g[p, D:2 * D])):
            want[t] += block.astype(np.float64)
            mass[t] += np.abs(block.astype(np.float64))
            n[t] += 1
    err = np.abs(runs[0].astype(np.float64) - want)
    assert (err <= n[:, None] * 2.0 ** -23 * mass).all(), (err.max(), (n[:, None] * 2.0 ** -23 * mass).max())
    return runs[0], n


@pytest.mark.parametrize("D", [8, 10, 516])
def test_backward(D):
    O, P = 130, 257
    rng = np.random.RandomState(D)
    s, o = rng.randint(0, O - 2, size=P).astype(np.int32), rng.randint(0, O - 2, size=P).astype(np.int32)
    s[5] = o[5] = 17                                                 # one object as subject and object of the same pair
    got, n = backward_case(O, D, s, o, seed=D + 1)
    assert (n[O - 2:] == 0).all() and not got[O - 2:].any()          # objects no pair names: exact zeros
    assert np.array_equal(got[O - 2:].view(np.uint32), np.zeros((2, D), np.uint32))
    # one object the subject of all 257 pairs: a segment of 257 entries (514 with s == o) summed in the list's order
    got, n = backward_case(3, D, np.full(P, 1, np.int32), rng.randint(0, 3, size=P).astype(np.int32), seed=D + 2)
    assert n[1] >= 257
    backward_case(1, D, np.zeros(64, np.int32), np.zeros(64, np.int32), seed=D + 3)


def test_autograd_front_and_opcheck():
    from dfol_vqa_amd import torch_ops  # noqa: F401
    O, D, P = 9, 10, 21
    obj, s, o = draw(O, D, P, seed=11)
    dev = lambda a: torch.as_tensor(a).to(DEV)
    csr = tuple(dev(a) for a in data.scene_pair_csr(s, o, O))
    x = dev(obj).requires_grad_(True)
    before = ops.PATH_COUNTS["scene_pair_rows_hip"]
    rows = ops.scene_pair_rows(x, dev(s), dev(o), csr)
    assert ops.PATH_COUNTS["scene_pair_rows_hip"] == before + 1
    g = torch.as_tensor(np.random.RandomState(2).normal(size=(P, 2 * D + 4)).astype(np.float32)).to(DEV)
    rows.backward(g)
    want = _lib.scene_pair_rows_bwd(g, D, csr[0], csr[1], O)
    assert torch.equal(x.grad, want)
    torch.library.opcheck(torch.ops.dfol.scene_pair_rows.default, (dev(obj).requires_grad_(True), dev(s), dev(o)) + csr,
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration", "test_aot_dispatch_dynamic"))
    torch.library.opcheck(torch.ops.dfol.scene_pair_rows_bwd.default, (g, csr[0], csr[1], O, D), test_utils=("test_schema", "test_faketensor"))
