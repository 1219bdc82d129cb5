"""ops.scene_bce on the GPU (csrc/dfol_scene.hip): the fused weighted BCE of all concept columns, its metric sums and its three gradients,
against the float64 restatement of the reference's expressions (tests/scene_util.py).

Rule (golden_util.check_gradient): per element of dh, dE and db  |g - r64| <= 8 own s,  s = |r64| + 1e-3 max|r64|,
own = max(2^-20, max|r32 - r64| / s) with r32 the same restatement in float32; the loss by the same formula with s = sum |terms|.  num and
den are sums of weights that are multiples of 1/8 over index sets: exact in fp32, compared exactly (no log-likelihood lies within 1e-4 of thr).
Shapes: row tails of the 64-row block (1, 37, 130), K tail and K padding (H = 20, 300), column tails of the 32-column tile and of the forward's
256-column slab (1, 33, 333, 2002), more than one slab of row blocks in the column kernel (M = 130 at C = 33), more forward workgroups than
the 256 lanes of the partial-sum pass take in one step (M = 16400 at C = 1: 257).

Observed on an MI355X (pytest -s prints every figure): max |g - r64| / s between 1e-7 and 1.1e-4 over all cases; at |z| <= 20 the float32
restatement's own distance `own` reaches 1e-3 .. 1e6 wherever a logit beyond ~16 makes its rounded 1 - p zero, so those bounds are loose and
test_moderate_logits (|z| <= 8: `own` 1e-6 .. 6e-4, the kernels at up to 0.46 of the bound - db at 130 x 300 x 333) is the tighter check."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
import scene_util as su  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    import __graft_entry__ as g
    g.build()
    from dfol_vqa_amd import ops
    return ops


def dev(x):
    return None if x is None else torch.as_tensor(x).cuda()


def run(O, case, grad=True):
    """-> (loss, num, den, dh, dE [C, H], db [C] or None) as numpy, the gradients gathered from the embedding layer's full-size ones (whose
    other rows must be exactly 0)."""
    h, w, t, wt, cols = dev(case["h"]), dev(case["emb_w"]), dev(case["target"]), dev(case["weight"]), dev(case["cols"])
    b = dev(case["emb_b"])
    if grad:
        h.requires_grad_(True)
        w.requires_grad_(True)
        if b is not None:
            b.requires_grad_(True)
    before = O.PATH_COUNTS["scene_bce_hip"]
    loss, num, den = O.scene_bce(h, w, b, cols, t, wt, case["thr"])
    assert O.PATH_COUNTS["scene_bce_hip"] == before + 1
    assert not num.requires_grad and not den.requires_grad
    out = [loss.item(), num.item(), den.item()]
    if not grad:
        return out + [None, None, None]
    loss.backward()
    idx = cols.to(torch.int64)
    rest = torch.ones(w.shape[0], dtype=torch.bool, device="cuda")
    rest[idx] = False
    assert not w.grad[rest].any() and not torch.signbit(w.grad[rest]).any()
    if b is not None:
        assert not b.grad[rest].any()
    return out + [h.grad.cpu().numpy(), w.grad[idx].cpu().numpy(), None if b is None else b.grad[idx].cpu().numpy()]


def check(O, case, r64, what):
    r32 = su.restate(case["h"], case["emb_w"], case["emb_b"], case["cols"], case["target"], case["weight"], case["thr"], torch.float32)
    for r in (r32, r64):                                            # the yardsticks themselves are finite on |z| <= 20
        assert all(np.all(np.isfinite(v)) for v in r.values() if v is not None), what
    loss, num, den, dh, dE, db = run(O, case)
    su.check_loss(loss, r32, r64, what)
    assert num == float(r64["num"]) and den == float(r64["den"]), (what, num, den, float(r64["num"]), float(r64["den"]))
    gu.check_gradient(dh, r32["dh"], r64["dh"], what + " dh")
    gu.check_gradient(dE, r32["dE"], r64["dE"], what + " dE")
    if db is not None:
        gu.check_gradient(db, r32["db"], r64["db"], what + " db")
    return loss, num, den, dh, dE, db


SHAPES = [(M, H, C) for M in (1, 37, 130) for H in (20, 300) for C in (1, 33, 333)] + [(37, 300, 2002), (16400, 20, 1)]


@pytest.mark.parametrize("M,H,C", SHAPES)
def test_shapes(O, M, H, C):
    """Every shape with a bias and thr = 0.5 (the reference's: no log-likelihood exceeds it), and without one at a negative thr."""
    bias = (M + H + C) % 2 == 0
    thr = 0.5 if bias else -0.7
    case, r64 = su.make_case(M, H, C, bias=bias, thr=thr, seed=M * 7 + H + C)
    _, num, den, _, _, _ = check(O, case, r64, "M=%d H=%d C=%d bias=%s thr=%g" % (M, H, C, bias, thr))
    if thr < 0 and M * C >= 300:
        assert 0 < num < den                                        # the negative threshold puts predictions on both sides


@pytest.mark.parametrize("M,H,C,bias", [(37, 20, 33, True), (130, 300, 333, True), (130, 20, 33, False), (5, 300, 2002, False),
                                        (16400, 20, 1, True)])
def test_moderate_logits(O, M, H, C, bias):
    """|z| <= 8: there the float32 restatement itself is a tight yardstick (beyond |z| ~ 16 its rounded 1 - p makes `own` large and the bound of
    the |z| <= 20 cases loose), so the kernel is held to 8 x fp32-class noise."""
    case, r64 = su.make_case(M, H, C, bias=bias, thr=-0.7, seed=31 + M + C, z_max=8.0)
    check(O, case, r64, "moderate M=%d H=%d C=%d" % (M, H, C))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("thr", [0.5, -0.7])
def test_bias_and_threshold(O, bias, thr):
    case, r64 = su.make_case(37, 300, 33, bias=bias, thr=thr, seed=11)
    check(O, case, r64, "bias=%s thr=%g" % (bias, thr))


@pytest.mark.parametrize("targets", ["zeros", "ones", "mixed"])
def test_targets(O, targets):
    case, r64 = su.make_case(130, 20, 33, targets=targets, thr=-0.7, seed=5)
    check(O, case, r64, "targets=" + targets)


def test_zero_weight_rows_and_columns(O):
    """Whole rows and columns of zero weight: their dh rows and dE / db entries are exactly +0."""
    rows, cs = (0, 36, 70), (0, 31, 32)
    case, r64 = su.make_case(130, 300, 33, thr=-0.7, seed=3, zero_rows=rows, zero_cols=cs)
    _, _, _, dh, dE, db = check(O, case, r64, "zero weights")
    for g in (dh[list(rows)], dE[list(cs)], db[list(cs)]):
        assert not g.any() and not np.signbit(g).any()
    assert dh[1].any() and dE[1].any() and db[1]


def test_saturated(O):
    """z = +-(200 and more) in one row (through one scaled coordinate of that row of h) and in two columns (through one scaled coordinate of
    two rows of emb_w), everything within fp16 range: the loss terms there are 100 w and 0 as binary_cross_entropy's clamp gives them, and
    the gradient there is exactly 0."""
    M, H, C = 37, 20, 33
    case, _ = su.make_case(M, H - 2, C, thr=-0.7, seed=9)           # two more coordinates carry the saturation; the other logits stay as drawn
    cols = case["cols"]
    h = case["h"] = np.concatenate([case["h"], np.zeros((M, 2), np.float32)], 1)
    e = case["emb_w"] = np.concatenate([case["emb_w"], np.zeros((case["emb_w"].shape[0], 2), np.float32)], 1)
    r0, c0, c1, ka, kb = 5, 3, 17, H - 2, H - 1
    rng = np.random.RandomState(1)
    h[:, kb] = 1.0
    h[r0, ka] = 50.0
    e[cols, ka] = np.where(rng.uniform(size=C) < 0.5, 4.5, -4.5).astype(np.float32)
    e[cols[c0], ka], e[cols[c1], ka] = 4.5, -4.5
    e[cols[c0], kb], e[cols[c1], kb] = 230.0, -230.0
    r64 = su.restate(h, e, case["emb_b"], cols, case["target"], case["weight"], case["thr"], torch.float64)
    z = r64["z"]
    sat = np.zeros((M, C), bool)
    sat[r0, :] = True
    sat[:, [c0, c1]] = True
    assert np.abs(z[sat]).min() >= 200 and np.abs(z[~sat]).max() <= 20
    loss, num, den, dh, dE, db = check(O, case, r64, "saturated")
    assert not dh[r0].any() and not dE[[c0, c1]].any() and not db[[c0, c1]].any()
    # with weight on the saturated cells alone the loss is the sum of 100 w over the wrong-side cells: multiples of 12.5, exact in fp32
    only = dict(case, weight=np.where(sat, case["weight"], 0.0).astype(np.float32))
    wrong = sat & ((z > 0) != (case["target"] > 0))
    got = run(O, only, grad=False)[0]
    assert got == float((100.0 * only["weight"].astype(np.float64))[wrong].sum()) and got > 0


def test_two_runs_same_bits(O):
    for (M, H, C) in ((130, 300, 333), (16400, 20, 1), (37, 300, 2002)):
        case, _ = su.make_case(M, H, C, thr=-0.7, seed=21)
        a, b = run(O, case), run(O, case)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x), np.asarray(y)), (M, H, C)
        assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes()


@pytest.mark.parametrize("M,C", [(0, 33), (37, 0), (0, 0)])
def test_empty(O, M, C):
    """M = 0 (no objects, or P = 0 listed pairs) and C = 0: zero sums, zero gradients, no launch error."""
    case, _ = su.make_case(M, 300, C, seed=2)
    loss, num, den, dh, dE, db = run(O, case)
    torch.cuda.synchronize()
    assert (loss, num, den) == (0.0, 0.0, 0.0)
    assert dh.shape == (M, 300) and dE.shape == (C, 300) and not dh.any() and not dE.any() and not db.any()


def test_declined_shape_takes_the_tensor_route(O):
    """H = 324 is beyond dfol_scene_bce_supported: the tensor-op route serves it; on a shape both serve the two routes agree within the rule."""
    from dfol_vqa_amd import _lib
    assert _lib.scene_bce_supported(37, 300, 33) and _lib.scene_bce_supported(0, 1, 0) and _lib.scene_bce_supported(37, 320, 2335)
    assert not _lib.scene_bce_supported(37, 324, 33) and not _lib.scene_bce_supported(37, 0, 33)
    case, r64 = su.make_case(37, 324, 33, thr=-0.7, seed=4)
    r32 = su.restate(case["h"], case["emb_w"], case["emb_b"], case["cols"], case["target"], case["weight"], case["thr"], torch.float32)
    args = [dev(case[k]) for k in ("h", "emb_w", "emb_b", "cols", "target", "weight")]
    args[0].requires_grad_(True)
    before = O.PATH_COUNTS["scene_bce_torch"]
    loss, num, den = O.scene_bce(*args, case["thr"])
    assert O.PATH_COUNTS["scene_bce_torch"] == before + 1
    loss.backward()
    su.check_loss(loss.item(), r32, r64, "declined")
    assert num.item() == float(r64["num"]) and den.item() == float(r64["den"])
    gu.check_gradient(args[0].grad.cpu().numpy(), r32["dh"], r64["dh"], "declined dh")
    # a shape both routes serve
    case, r64 = su.make_case(37, 300, 33, thr=-0.7, seed=4)
    r32 = su.restate(case["h"], case["emb_w"], case["emb_b"], case["cols"], case["target"], case["weight"], case["thr"], torch.float32)
    hip = run(O, case)
    args = [dev(case[k]) for k in ("h", "emb_w", "emb_b", "cols", "target", "weight")]
    args[0].requires_grad_(True)
    loss, num, den = O.scene_bce_reference(*args, case["thr"])
    loss.backward()
    su.check_loss(loss.item(), r32, r64, "tensor route")
    su.check_loss(hip[0], r32, r64, "kernel route")
    assert (num.item(), den.item()) == (hip[1], hip[2])
    gu.check_gradient(args[0].grad.cpu().numpy(), r32["dh"], r64["dh"], "tensor route dh")
    gu.check_gradient(hip[3], r32["dh"], r64["dh"], "kernel route dh")


def test_repeated_columns_are_refused(O):
    case, _ = su.make_case(5, 20, 4, seed=1)
    cols = dev(np.asarray([3, 9, 3, 1], np.int32))
    with pytest.raises(O.DfolError):
        O.scene_bce(dev(case["h"]), dev(case["emb_w"]), None, cols, dev(case["target"]), dev(case["weight"]), 0.5)


def test_range_word(O):
    """An embedding row beyond fp16's range is reported through the range word, not answered with."""
    from dfol_vqa_amd import _lib
    case, _ = su.make_case(37, 20, 33, seed=6)
    watch = _lib.RangeWatch("cuda")
    run(O, case, grad=False)
    assert watch.finish()(throw=False) == 0
    case["emb_w"][case["cols"][7], 3] = 1.0e5
    watch = _lib.RangeWatch("cuda")
    run(O, case, grad=False)
    assert watch.finish()(throw=False) & _lib.RANGE_X_OVERFLOW
    _lib.range_status_off()


def test_opcheck(O):
    case, _ = su.make_case(37, 20, 33, seed=8)
    g = lambda t: t.requires_grad_(True)
    utils = ("test_schema", "test_faketensor", "test_autograd_registration", "test_aot_dispatch_dynamic")
    for b in (g(dev(case["emb_b"])), None):
        torch.library.opcheck(torch.ops.dfol.scene_bce.default, (g(dev(case["h"])), g(dev(case["emb_w"])), b, dev(case["cols"]), dev(case["target"]),
                                                                 dev(case["weight"]), 0.5), test_utils=utils)
