"""The pair train streams (csrc/dfol_pair_train.hip: pair_hidden1_fwd, pair_hidden1_bwd in its 1024-thread, 512-thread and rebuilt-z forms,
pair_logit_fwd, pair_logit_bwd and its sums form) off the shapes of their first test: images beyond 128 objects, the edges of the batched walk,
the widest and the narrowest hidden layers, 0-row predicates and row counts around one trip of the logit backward.

1. hidden1, float64 reference = autograd of ELU(U[s] + V[o] + geo @ Wg^T) on the kernel's own geometry (itself checked against float64, the angle
   through its sine).  One batch of ragged images per row of H1_GRID:
     HID1  n_list             rebuilt-z  reaches
      256  [129, 1, 2, 200]   no         1024-thread form for the whole batch, its n = 1 and n = 2 images too; the last object slot partly filled
      256  [256, 130]         no         1024-thread form at the guard's maximum: all 16 slots of all 16 groups hold an object
      256  [32, 33, 2]        yes        walk<1> full, walk<2> with ONE object in its second batch, the smallest image that has pairs
      256  [64, 65, 17, 16]   yes        walk<2> full, walk<3> by one object; the forward's two-subject shortcut (n - 1 >= 16) on both sides
      256  [96, 97, 1]        yes        walk<3> full with an even n (two subjects per pass), walk<4> by one object with an odd n
      256  [128, 127]         yes        walk<4> full; the rebuilt-z form at exactly 144 KB of LDS
      512  [64, 5]            yes        512-thread form at its maximum (4 groups)
      512  [65, 128]          no         1024-thread form with 8 groups up to its maximum
     1024  [32, 3]            yes        forward with one row slot per workgroup; 2 groups; the rebuilt-z form at exactly 144 KB
     1024  [33, 64]           no         1024-thread form with 4 groups up to its maximum
       16  [40, 1, 7]         yes        the narrowest width: 4 lanes per row, 128 groups
   Which form ran is asserted, never assumed: both share one entry point, so every row asserts dfol_pair_hidden1_bwd_recompute_supported(max_n,
   HID1) - the condition of the 512-thread choice - to be what the row was written for.  U and V are the two halves of a joined [O, 2 HID1]
   buffer, pos a column slice with NaN in the spare columns.  bf16 storage on the HID1 = 256 rows and on 512 x [64, 5]: the forward is the
   fp32 result rounded to nearest even and the backward the fp32-storage kernel on the widened values, both bit for bit.
2. DFOL_H1B_THREADS=1024 (read once per process: one fresh child, this file run as a program) on HID1 = 256, n_list = [1, 2, 17, 100, 36], fp32
   and bf16 storage.  The bf16-storage kernel differentiates through the STORED z and dZ, so its float64 reference is the same sums over the
   stored values.  That the switch took effect shows in the bits: 16 groups' partial sums add up in another order than the 512-thread form's 8.
3. logit forward / backward, float64 autograd of (sigmoid(P2) * E[rep]).sum(1) + be[rep], at HID2 = 512 (8 row groups), 260 (65 lanes per row, 15
   row groups, 49 idle threads), 16 (the vector path's minimum, 256 row groups), 12 and 511 (the generic kernels; 511: odd, all 8 lane strides),
   300; predicates of [0, 1, 15, 16, 17, T - 1, T, T + 1, 0, 3 T + 5] rows at HID2 = 300 and 16 (T = 8 row groups' worth of rows in flight: one
   trip of pair_logit_bwd4_kernel), of [1, 0, 40, 257] rows elsewhere.  P2 and E are column slices with NaN behind them.  The vector kernel and
   the generic one share an entry point too; that HID2 = 16, 260, 300 took the vector kernel shows in dE and dbe being bit-equal to the sums
   form's, which has no other kernel.
4. The Python guard against the entry points' own (nothing is launched: Q = 0 / P = 0 return after the size checks), and the refusals.

Bounds are test_fused_pair_training_kernels_against_autograd's: z and x rtol = atol = 2e-5, dP2 rtol 2e-5 atol 2e-6, every sum 5e-5 max(1, max|ref|).
Every case also evaluates the same formula in float32 on the CPU (index_add_) and prints its error against the same bound; a (case, quantity)
listed in FALLBACK would be held to 8 x that float32 error instead (golden_util.check_gradient's factor).
dB2 of the sums form against the float64 column sums of the materialised dP2: N 2^-24 / (1 - N 2^-24) sum|dP2| for a predicate of N rows, the bound of
a float32 sum of N terms in any order.

Every check prints its worst ratio error / bound (pytest -s).  MI355X; every bit-for-bit comparison held, every row ran the form it was written
for, and no bound had to fall back to the 8 x float32 rule (FALLBACK is empty; the float32 restatement itself stays below 0.21 of every bound):
     HID1  n_list             form           z      dU     dV     dWg
      256  [129, 1, 2, 200]   1024-thread    0.019  0.003  0.009  0.016
      256  [256, 130]         1024-thread    0.018  0.004  0.014  0.024
      256  [32, 33, 2]        512, rebuilt   0.015  0.002  0.004  0.006
      256  [64, 65, 17, 16]   512, rebuilt   0.020  0.003  0.007  0.007
      256  [96, 97, 1]        512, rebuilt   0.016  0.002  0.007  0.013
      256  [128, 127]         512, rebuilt   0.020  0.003  0.008  0.022
      512  [64, 5]            512, rebuilt   0.017  0.002  0.006  0.014
      512  [65, 128]          1024-thread    0.021  0.002  0.009  0.017
     1024  [32, 3]            512, rebuilt   0.015  0.002  0.004  0.011
     1024  [33, 64]           1024-thread    0.020  0.003  0.006  0.014
       16  [40, 1, 7]         512, rebuilt   0.011  0.003  0.004  0.002
      256  [1, 2, 17, 100, 36]  forced 1024  0.016  0.003  0.007  0.009     bf16 storage, on the stored values: dU 0.002, dV 0.003, dWg 0.008
     HID2    x      dP2    dE     dbe    dB2 (sums form)    bf16 x error against 2 x the fp32-storage kernel's + 1e-6
      300  0.026  0.056  0.005  0.005  0.099
       16  0.007  0.061  0.009  0.004  0.089              3.4e-07 against 2 x 3.3e-07 + 1e-6
      512  0.040  0.062  0.003  0.001    -                1.4e-06 against 2 x 1.2e-06 + 1e-6
      260  0.023  0.058  0.002  0.001  0.024              8.9e-07 against 2 x 8.3e-07 + 1e-6
       12  0.008  0.035  0.002  0.003    -
      511  0.032  0.056  0.003  0.002    -
No kernel bug was found, and the Python guard agrees with the entry points at every size tried.  Three mutants of csrc/dfol_pair_train.hip, each
built on a scratch copy and run once against this file (none reads or writes out of bounds):
  * the `o != s` test of the BATCH = 1 loop of pair_hidden1_bwd_kernel dropped wherever the diagonal's row index still lies inside the image
    (s + 1 < n; dropped outright, the last subject would read one row past its image): the backward test of exactly the four 1024-thread rows
    and the forced-form test fail, 5 of 51;
  * the `s < n` guard of `consume` in `walk` made always true: the backward test of exactly the four rows with an odd n under walk<1> or walk<3>
    fails (256 x [64, 65, 17, 16], 512 x [64, 5], 1024 x [32, 3], 16 x [40, 1, 7]), 4 of 51;
  * `min(sA + 1, n - 1)` of the forward made `sA`: the forward test of all eleven rows fails (each has an image of 17 objects or more), with it
    their backward tests (the stored z is wrong) and the forced-form test, 23 of 51.
"""

import contextlib
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from dfol_vqa_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64, BF, I32 = torch.float32, torch.float64, torch.bfloat16, torch.int32

#           HID1  n_list            rebuilt-z form (= the 512-thread form)
H1_GRID = [(256, [129, 1, 2, 200], False),
           (256, [256, 130], False),
           (256, [32, 33, 2], True),
           (256, [64, 65, 17, 16], True),
           (256, [96, 97, 1], True),
           (256, [128, 127], True),
           (512, [64, 5], True),
           (512, [65, 128], False),
           (1024, [32, 3], True),
           (1024, [33, 64], False),
           (16, [40, 1, 7], True)]
H1_IDS = ["%d-%s" % (h, "_".join(str(n) for n in ns)) for h, ns, _ in H1_GRID]
H1_BF16 = [0, 1, 2, 3, 4, 5, 6]
FORCED = (256, [1, 2, 17, 100, 36])

LOGIT_SHORT = [1, 0, 40, 257]
LOGIT_GRID = [300, 16, 512, 260, 12, 511]        # HID2; 300 and 16 with _trip_counts
LOGIT_BF16 = [512, 260, 16]
LOGIT_SUMS = [16, 260, 300]

# (case id, quantity) -> the bound is 8 x the float32 restatement's own error instead of the project's.  None was needed.
FALLBACK = set()

_H1, _LOGIT = {}, {}


class _Case(object):
    pass


@pytest.fixture(scope="module", autouse=True)
def _free_cases():
    yield
    _H1.clear()
    _LOGIT.clear()


@contextlib.contextmanager
def _entry_points(monkeypatch):
    """The entry points _lib.call is given inside the block."""
    names, real = [], _lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    try:
        yield names
    finally:
        monkeypatch.setattr(_lib, "call", real)


def _report(case, what, ratio, ratio32):
    print("pair-train %-22s %-4s %.3f of its bound (float32 on the CPU: %.3f)%s"
          % (case, what, ratio, ratio32, "  [8 x float32 bound]" if (case, what) in FALLBACK else ""))


def _sum_ratio(case, what, got, r64, r32):
    """max|got - r64| over the sums' bound 5e-5 max(1, max|r64|), resp. over 8 max|r32 - r64| for a (case, quantity) of FALLBACK."""
    got, r64, r32 = (np.asarray(a, np.float64) for a in (got, r64, r32))
    assert got.shape == r64.shape and np.isfinite(got).all(), (case, what)
    top = np.abs(r64).max() if r64.size else 0.0
    e32 = np.abs(r32 - r64).max() if r64.size else 0.0
    project = 5e-5 * max(1.0, top)
    bound = 8.0 * e32 if (case, what) in FALLBACK else project
    ratio = (np.abs(got - r64).max() if r64.size else 0.0) / bound
    _report(case, what, ratio, e32 / project)
    return ratio


def _close_ratio(case, what, got, r64, r32, rtol, atol):
    """max of |got - r64| / (atol + rtol |r64|): numpy.allclose as a ratio."""
    got, r64, r32 = (np.asarray(a, np.float64) for a in (got, r64, r32))
    assert got.shape == r64.shape and np.isfinite(got).all(), (case, what)
    if not r64.size:
        return 0.0
    tol = atol + rtol * np.abs(r64)
    ratio32 = (np.abs(r32 - r64) / tol).max()
    if (case, what) in FALLBACK:
        tol = np.maximum(tol, 8.0 * np.abs(r32 - r64).max())
    ratio = (np.abs(got - r64) / tol).max()
    _report(case, what, ratio, ratio32)
    return ratio


# ---------------------------------------------------------------------------------------------------
# 1. hidden1: operands, the float64 reference, the float32 restatement
# ---------------------------------------------------------------------------------------------------
def _hidden1_operands(hid1, n_list):
    """Seeded by the shape alone: the forced-form child and its parent build the same arrays."""
    c = _Case()
    c.id = "%d-%s" % (hid1, "_".join(str(k) for k in n_list))
    rng = np.random.RandomState(sum(n_list) + hid1)
    n = np.asarray(n_list, np.int64)
    c.hid1, c.n, c.Q, c.max_n = hid1, n, len(n_list), int(n.max())
    c.O, c.pairs = int(n.sum()), int((n * (n - 1)).sum())
    c.obj_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    c.pair_off = np.concatenate([[0], np.cumsum(n * (n - 1))]).astype(np.int64)
    s_idx, o_idx = [], []
    for q, k in enumerate(n_list):
        s, o = np.nonzero(~np.eye(k, dtype=bool))
        s_idx.append(s + c.obj_off[q]), o_idx.append(o + c.obj_off[q])
    c.s_idx, c.o_idx = torch.as_tensor(np.concatenate(s_idx)), torch.as_tensor(np.concatenate(o_idx))
    c.U_h = torch.as_tensor(rng.normal(size=(c.O, hid1)).astype(np.float32))
    c.V_h = torch.as_tensor(rng.normal(size=(c.O, hid1)).astype(np.float32))
    c.pos_h = torch.as_tensor(rng.uniform(0.05, 0.9, (c.O, 4)).astype(np.float32))
    c.Wg_h = torch.as_tensor(rng.normal(size=(hid1, 4)).astype(np.float32) * 0.5)
    c.gz_h = torch.as_tensor(rng.standard_normal(size=(c.pairs, hid1)).astype(np.float32))
    c.UV = torch.cat([c.U_h, c.V_h], 1).to(DEV)                     # the joined U|V product's layout: row stride 2 HID1
    c.U, c.V = c.UV[:, :hid1], c.UV[:, hid1:]
    c.posbuf = torch.full((c.O, 6), float("nan"), dtype=F32, device=DEV)
    c.posbuf[:, 1:5] = c.pos_h.to(DEV)
    c.pos = c.posbuf[:, 1:5]                                        # a strided view, like obj[:, D - 4:]
    c.Wg, c.gz = c.Wg_h.to(DEV), c.gz_h.to(DEV)
    c.geom = (torch.as_tensor(c.obj_off).to(DEV), torch.as_tensor(c.pair_off).to(DEV), torch.as_tensor(n.astype(np.int32)).to(DEV))
    return c


def _geometry_failures(c, geo):
    """The kernel's [pairs, 4] geometry against float64, the angle through its sine (asin is ill-conditioned at +-1)."""
    p64 = c.pos_h.numpy().astype(np.float64)
    ps, po = p64[c.s_idx.numpy()], p64[c.o_idx.numpy()]
    dx = ps[:, 0] + ps[:, 2] / 2.0 - po[:, 0] - po[:, 2] / 2.0
    dy = ps[:, 1] + ps[:, 3] / 2.0 - po[:, 1] - po[:, 3] / 2.0
    dist = np.sqrt(dx * dx + dy * dy)
    bad = []
    if not np.isfinite(geo).all():
        bad.append("not finite")
    if not np.allclose(geo[:, 0], dist, rtol=1e-5, atol=1e-6):
        bad.append("distance")
    # (dy is a float32 difference of coordinates of order 1: its rounding, 2e-7 at most, is divided by the distance)
    if not (np.abs(np.sin(geo[:, 1]) - dy / np.maximum(dist, 1e-10)) <= 2e-6 + 2e-7 / np.maximum(dist, 1e-10)).all():
        bad.append("angle")
    if not (np.array_equal(geo[:, 2], np.sign(po[:, 0] - ps[:, 0])) and np.array_equal(geo[:, 3], np.sign(po[:, 1] - ps[:, 1]))):
        bad.append("signs")
    return bad


def _hidden1_autograd(c, geo, dtype):
    """(z, dU, dV, dWg) of z = ELU(U[s] + V[o] + geo @ Wg^T) under the upstream gradient gz, in `dtype` on the CPU.  float64: torch autograd.
    float32: the same formula written out with index_add_ (the restatement whose own error the FALLBACK rule takes)."""
    if dtype == F64:
        U, V, W = (t.double().requires_grad_(True) for t in (c.U_h, c.V_h, c.Wg_h))
        z = torch.nn.functional.elu(U[c.s_idx] + V[c.o_idx] + geo.double() @ W.t())
        z.backward(c.gz_h.double())
        return z.detach(), U.grad, V.grad, W.grad
    g = geo.to(dtype)
    z = torch.nn.functional.elu(c.U_h[c.s_idx] + c.V_h[c.o_idx] + g @ c.Wg_h.t())
    return (z,) + _hidden1_sums(c, c.gz_h, z, g, dtype)


def _hidden1_sums(c, dz, z, geo, dtype):
    """The backward as the kernel states it, from STORED z and dZ: dpre = dZ * (z > 0 ? 1 : z + 1), summed by subject, by object, against geo."""
    dz, z, geo = dz.to(dtype), z.to(dtype), geo.to(dtype)
    dpre = dz * torch.where(z > 0, torch.ones_like(z), z + 1)
    du = torch.zeros(c.O, c.hid1, dtype=dtype).index_add_(0, c.s_idx, dpre)
    dv = torch.zeros(c.O, c.hid1, dtype=dtype).index_add_(0, c.o_idx, dpre)
    return du, dv, dpre.t() @ geo


def _hidden1_case(hid1, n_list):
    """Operands, the forward kernel's z and geo (fp32 storage), the float64 reference and the float32 restatement; the forward's figures."""
    c = _hidden1_operands(hid1, n_list)
    c.z, c.geo = _lib.pair_hidden1_fwd(c.U, c.V, c.pos, c.Wg, c.geom[0], c.geom[1], c.geom[2], c.max_n, c.pairs)
    geo = c.geo.cpu()
    c.geometry_failures = _geometry_failures(c, geo.numpy().astype(np.float64))
    z64, du64, dv64, dw64 = _hidden1_autograd(c, geo, F64)
    z32, du32, dv32, dw32 = _hidden1_autograd(c, geo, F32)
    c.z_ratio = _close_ratio(c.id, "z", c.z.cpu().numpy(), z64.numpy(), z32.numpy(), 2e-5, 2e-5)
    c.r64 = {"dU": du64.numpy(), "dV": dv64.numpy(), "dWg": dw64.numpy()}
    c.r32 = {"dU": du32.numpy(), "dV": dv32.numpy(), "dWg": dw32.numpy()}
    return c


def _h1(i):
    if i not in _H1:
        _H1[i] = _hidden1_case(H1_GRID[i][0], H1_GRID[i][1])
    return _H1[i]


def _hidden1_bwd(c, dz, z, **kw):
    return _lib.pair_hidden1_bwd(dz, z, c.geo, c.geom[0], c.geom[1], c.geom[2], c.max_n, c.O, **kw)


def _hidden1_ratios(c, grads, r64=None, r32=None, tag=""):
    r64, r32 = r64 or c.r64, r32 or c.r32
    return {k: _sum_ratio(c.id + tag, k, g.cpu().numpy(), r64[k], r32[k]) for k, g in zip(("dU", "dV", "dWg"), grads)}


def _one_object_rows_are_zero(c, du, dv):
    rows = [int(c.obj_off[q]) for q in range(c.Q) if c.n[q] == 1]
    return all(not bool(du[r].any()) and not bool(dv[r].any()) for r in rows)


@pytest.mark.parametrize("i", range(len(H1_GRID)), ids=H1_IDS)
def test_hidden1_forward_against_float64(i):
    c = _h1(i)
    assert c.z.shape == (c.pairs, c.hid1) and c.geo.shape == (c.pairs, 4)
    assert not c.geometry_failures, c.geometry_failures
    assert c.z_ratio <= 1.0
    assert bool(c.posbuf[:, 0].isnan().all()) and bool(c.posbuf[:, 5].isnan().all())


@pytest.mark.parametrize("i", range(len(H1_GRID)), ids=H1_IDS)
def test_hidden1_backward_against_float64(i, monkeypatch):
    """dU, dV, dWg against float64; twice, bit-identical; zero rows for one-object images; the form the row was written for; where z is
    rebuilt, that form into a joined [O, 2 HID1] buffer equals the reading form bit for bit."""
    monkeypatch.delenv("DFOL_H1B_RECOMPUTE", raising=False)
    c = _h1(i)
    hid1, _, rebuilt = H1_GRID[i]
    assert bool(_lib.load().dfol_pair_hidden1_bwd_recompute_supported(c.max_n, hid1)) == rebuilt
    assert _lib.pair_train_supported(hid1, 300, c.max_n)
    with _entry_points(monkeypatch) as names:
        du, dv, dw = _hidden1_bwd(c, c.gz, c.z)
        du2, dv2, dw2 = _hidden1_bwd(c, c.gz, c.z)
    assert names == ["dfol_pair_hidden1_bwd_f32"] * 2
    ratios = _hidden1_ratios(c, (du, dv, dw))
    assert max(ratios.values()) <= 1.0, ratios
    assert torch.equal(du, du2) and torch.equal(dv, dv2) and torch.equal(dw, dw2)          # no atomics: bitwise repeatable
    assert _one_object_rows_are_zero(c, du, dv)
    uvw = (c.U, c.V, c.Wg)
    assert _lib.hidden1_recompute(uvw, c.gz, c.max_n, hid1) == rebuilt
    if rebuilt:
        with _entry_points(monkeypatch) as names:
            duv, none, dw3 = _hidden1_bwd(c, c.gz, None, joined=True, uvw=uvw)
        assert names == ["dfol_pair_hidden1_bwd_recompute_f32"]
        assert none is None and torch.equal(duv[:, :hid1], du) and torch.equal(duv[:, hid1:], dv) and torch.equal(dw3, dw)


@pytest.mark.parametrize("i", H1_BF16, ids=[H1_IDS[i] for i in H1_BF16])
def test_hidden1_bf16_storage_equals_fp32_storage_on_the_same_values(i, monkeypatch):
    """test_bf16_storage_stream_kernels_equal_fp32_storage_kernels_on_the_same_values's policy; both storages take the same form at a shape."""
    c = _h1(i)
    with _entry_points(monkeypatch) as names:
        zb, geob = _lib.pair_hidden1_fwd(c.U, c.V, c.pos, c.Wg, c.geom[0], c.geom[1], c.geom[2], c.max_n, c.pairs, store=BF)
        dzb = c.gz.to(BF)
        got = _hidden1_bwd(c, dzb, zb)
        want = _hidden1_bwd(c, dzb.float(), zb.float())
    assert names == ["dfol_pair_hidden1_fwd_bf16", "dfol_pair_hidden1_bwd_bf16", "dfol_pair_hidden1_bwd_f32"]
    assert zb.dtype == BF and torch.equal(zb, c.z.to(BF)) and torch.equal(geob, c.geo)        # the fp32 value, rounded to nearest even
    for a, b in zip(got, want):
        assert torch.equal(a, b)                                                              # same fp32 arithmetic on the same values
    assert _one_object_rows_are_zero(c, got[0], got[1])


# ---------------------------------------------------------------------------------------------------
# 2. DFOL_H1B_THREADS=1024 in a fresh child
# ---------------------------------------------------------------------------------------------------
def _digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _forced_figures():
    """FORCED in this process, whatever form it takes: every figure the parent asserts on."""
    c = _hidden1_case(*FORCED)
    out = {"threads": os.environ.get("DFOL_H1B_THREADS"), "geometry_failures": c.geometry_failures, "z": c.z_ratio}
    g32 = _hidden1_bwd(c, c.gz, c.z)
    again = _hidden1_bwd(c, c.gz, c.z)
    out["fp32"] = _hidden1_ratios(c, g32)
    out["repeatable"] = all(torch.equal(a, b) for a, b in zip(g32, again))
    out["zero_rows"] = _one_object_rows_are_zero(c, g32[0], g32[1])
    out["digest"] = _digest(g32)
    zb, geob = _lib.pair_hidden1_fwd(c.U, c.V, c.pos, c.Wg, c.geom[0], c.geom[1], c.geom[2], c.max_n, c.pairs, store=BF)
    dzb = c.gz.to(BF)
    gb = _hidden1_bwd(c, dzb, zb)
    wide = _hidden1_bwd(c, dzb.float(), zb.float())
    out["bf16_forward_is_rounded_fp32"] = bool(torch.equal(zb, c.z.to(BF)) and torch.equal(geob, c.geo))
    out["bf16_equals_fp32_storage"] = all(torch.equal(a, b) for a, b in zip(gb, wide))
    # the bf16-storage kernel's sums are those of the STORED values: float64 and float32 of exactly these
    stored = (dzb.cpu(), zb.cpu(), c.geo.cpu())
    r64 = dict(zip(("dU", "dV", "dWg"), (t.numpy() for t in _hidden1_sums(c, *stored, F64))))
    r32 = dict(zip(("dU", "dV", "dWg"), (t.numpy() for t in _hidden1_sums(c, *stored, F32))))
    out["bf16"] = _hidden1_ratios(c, gb, r64, r32, tag=" bf16")
    out["bf16_zero_rows"] = _one_object_rows_are_zero(c, gb[0], gb[1])
    return out


def test_forced_1024_thread_form_on_small_ragged_images(monkeypatch):
    monkeypatch.delenv("DFOL_H1B_THREADS", raising=False)
    env = dict(os.environ, DFOL_H1B_THREADS="1024")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "forced-1024"], env=env, cwd=ROOT, timeout=300, stdout=subprocess.PIPE)
    lines = child.stdout.decode().splitlines()
    print("\n".join(lines))
    assert child.returncode == 0 and lines, child.returncode
    out = json.loads(lines[-1])
    assert out["threads"] == "1024" and not out["geometry_failures"], out
    assert out["z"] <= 1.0 and max(out["fp32"].values()) <= 1.0 and max(out["bf16"].values()) <= 1.0, out
    assert out["repeatable"] and out["zero_rows"] and out["bf16_zero_rows"], out
    assert out["bf16_forward_is_rounded_fp32"] and out["bf16_equals_fp32_storage"], out
    # the same arrays in this process, where nothing is forced: the 512-thread form (8 groups), the same sums in another order
    hid1, n_list = FORCED
    assert _lib.load().dfol_pair_hidden1_bwd_recompute_supported(max(n_list), hid1) == 1
    c = _hidden1_operands(hid1, n_list)
    c.z, c.geo = _lib.pair_hidden1_fwd(c.U, c.V, c.pos, c.Wg, c.geom[0], c.geom[1], c.geom[2], c.max_n, c.pairs)
    assert _digest(_hidden1_bwd(c, c.gz, c.z)) != out["digest"]


# ---------------------------------------------------------------------------------------------------
# 3. logit forward / backward
# ---------------------------------------------------------------------------------------------------
def _trip_counts(hid2):
    """Row counts around one trip of pair_logit_bwd4_kernel: RF rows in flight for each of RG row groups (the documented rule)."""
    trip = 8 * (1024 // (hid2 // 4))
    return [0, 1, 15, 16, 17, trip - 1, trip, trip + 1, 0, 3 * trip + 5]


def _behind_nan(t, extra=4):
    """t as a column slice of a buffer `extra` columns wider, NaN behind the slice -> (buffer, slice)."""
    buf = torch.full((t.shape[0], t.shape[1] + extra), float("nan"), dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf, buf[:, :t.shape[1]]


def _logit_sums32(c, p2, dtype=F32):
    h = torch.sigmoid(p2.to(dtype))
    E, be, gx = c.E_h.to(dtype), c.be_h.to(dtype), c.gx_h.to(dtype)
    x = (h * E[c.rep]).sum(1) + be[c.rep]
    dp2 = gx[:, None] * E[c.rep] * h * (1 - h)
    de = torch.zeros(c.P, c.hid2, dtype=dtype).index_add_(0, c.rep, gx[:, None] * h)
    dbe = torch.zeros(c.P, dtype=dtype).index_add_(0, c.rep, gx)
    return {"x": x.numpy(), "dP2": dp2.numpy(), "dE": de.numpy(), "dbe": dbe.numpy()}


def _logit(hid2):
    if hid2 in _LOGIT:
        return _LOGIT[hid2]
    c = _Case()
    c.id, c.hid2 = "logit-%d" % hid2, hid2
    c.counts = _trip_counts(hid2) if hid2 in (300, 16) else LOGIT_SHORT
    if hid2 == 300:
        assert c.counts[6] == 104
    rng = np.random.RandomState(7000 + hid2)
    c.P, c.rows = len(c.counts), int(sum(c.counts))
    c.rep = torch.as_tensor(np.repeat(np.arange(c.P), c.counts))
    c.P2_h = torch.as_tensor(rng.normal(size=(c.rows, hid2)).astype(np.float32) * 2)
    c.E_h = torch.as_tensor(rng.normal(size=(c.P, hid2)).astype(np.float32) * 0.3)
    c.be_h = torch.as_tensor(rng.normal(size=c.P).astype(np.float32))
    c.gx_h = torch.as_tensor(rng.normal(size=c.rows).astype(np.float32))
    c.p2buf, c.p2 = _behind_nan(c.P2_h)
    c.ebuf, c.E = _behind_nan(c.E_h)
    c.be, c.gx = c.be_h.to(DEV), c.gx_h.to(DEV)
    c.pred_off = torch.as_tensor(np.concatenate([[0], np.cumsum(c.counts)]).astype(np.int64)).to(DEV)
    P2, E, be = (t.double().requires_grad_(True) for t in (c.P2_h, c.E_h, c.be_h))
    x = (torch.sigmoid(P2) * E[c.rep]).sum(1) + be[c.rep]
    x.backward(c.gx_h.double())
    c.r64 = {"x": x.detach().numpy(), "dP2": P2.grad.numpy(), "dE": E.grad.numpy(), "dbe": be.grad.numpy()}
    c.r32 = _logit_sums32(c, c.P2_h)
    _LOGIT[hid2] = c
    return c


def _fills_intact(c):
    return bool(c.p2buf[:, c.hid2:].isnan().all()) and bool(c.ebuf[:, c.hid2:].isnan().all())


@pytest.mark.parametrize("hid2", LOGIT_GRID)
def test_logit_forward_and_backward_against_float64(hid2, monkeypatch):
    c = _logit(hid2)
    assert _lib.pair_train_supported(256, hid2, 100)
    with _entry_points(monkeypatch) as names:
        x = _lib.pair_logit_fwd(c.p2, c.E, c.be, c.pred_off, max(c.counts))
        dp2, de, dbe = _lib.pair_logit_bwd(c.gx, c.p2, c.E, c.pred_off)
        dp2n, den, none = _lib.pair_logit_bwd(c.gx, c.p2, c.E, c.pred_off, need_bias=False)
    assert names == ["dfol_pair_logit_fwd_f32", "dfol_pair_logit_bwd_f32", "dfol_pair_logit_bwd_f32"]
    assert x.shape == (c.rows,) and dp2.shape == (c.rows, hid2) and de.shape == (c.P, hid2) and dbe.shape == (c.P,)
    ratios = {"x": _close_ratio(c.id, "x", x.cpu().numpy(), c.r64["x"], c.r32["x"], 2e-5, 2e-5),
              "dP2": _close_ratio(c.id, "dP2", dp2.cpu().numpy(), c.r64["dP2"], c.r32["dP2"], 2e-5, 2e-6),
              "dE": _sum_ratio(c.id, "dE", de.cpu().numpy(), c.r64["dE"], c.r32["dE"]),
              "dbe": _sum_ratio(c.id, "dbe", dbe.cpu().numpy(), c.r64["dbe"], c.r32["dbe"])}
    assert max(ratios.values()) <= 1.0, ratios
    empty = [p for p in range(c.P) if c.counts[p] == 0]
    assert empty
    for p in empty:                                              # (their neighbours' x and dP2 are held to float64 above)
        assert not bool(de[p].any()) and float(dbe[p]) == 0.0, p
    assert none is None and torch.equal(dp2n, dp2) and torch.equal(den, de)
    assert _fills_intact(c)


@pytest.mark.parametrize("hid2", LOGIT_BF16)
def test_logit_bf16_storage_equals_fp32_storage_on_the_same_values(hid2, monkeypatch):
    """dP2: the fp32-storage result rounded to nearest even; dE and dbe: the fp32-storage kernel on the widened values, bit for bit; the forward
    (another summation order) within twice the fp32-storage kernel's own error against float64."""
    c = _logit(hid2)
    p2buf, p2b = _behind_nan((c.P2_h * 1.5).to(BF))
    wide = p2b.float()
    with _entry_points(monkeypatch) as names:
        xb = _lib.pair_logit_fwd(p2b, c.E, c.be, c.pred_off, max(c.counts))
        x32 = _lib.pair_logit_fwd(wide, c.E, c.be, c.pred_off, max(c.counts))
        dpb, deb, dbb = _lib.pair_logit_bwd(c.gx, p2b, c.E, c.pred_off)
        dp32, de32, db32 = _lib.pair_logit_bwd(c.gx, wide, c.E, c.pred_off)
    assert names == ["dfol_pair_logit_fwd_bf16", "dfol_pair_logit_fwd_f32", "dfol_pair_logit_bwd_bf16", "dfol_pair_logit_bwd_f32"]
    assert dpb.dtype == BF and torch.equal(dpb, dp32.to(BF)) and torch.equal(deb, de32) and torch.equal(dbb, db32)
    ref = (torch.sigmoid(wide.cpu().double()) * c.E_h.double()[c.rep]).sum(1) + c.be_h.double()[c.rep]
    eb, e32 = float((xb.cpu().double() - ref).abs().max()), float((x32.cpu().double() - ref).abs().max())
    print("pair-train %-22s bf16 x: %.3g against 2 x %.3g + 1e-6" % (c.id, eb, e32))
    assert eb <= 2 * e32 + 1e-6
    for p in (p for p in range(c.P) if c.counts[p] == 0):
        assert not bool(deb[p].any()) and float(dbb[p]) == 0.0, p
    assert bool(p2buf[:, hid2:].isnan().all()) and _fills_intact(c)


@pytest.mark.parametrize("hid2", LOGIT_SUMS)
def test_logit_sums_form_equals_the_materialised_backward(hid2, monkeypatch):
    """pair_head_sums (pair_logit_bwd4_kernel without dP2, with dB2): dE and dbe bit-equal to pair_logit_bwd's, dB2 the column sums of its dP2."""
    c = _logit(hid2)
    E = c.E.contiguous()
    with _entry_points(monkeypatch) as names:
        dp2, de, dbe = _lib.pair_logit_bwd(c.gx, c.p2, c.E, c.pred_off)
        des, dbes, db2 = _lib.pair_head_sums(c.gx, c.p2, E, c.pred_off)
        desn, none, db2n = _lib.pair_head_sums(c.gx, c.p2, E, c.pred_off, need_bias=False)
    assert names == ["dfol_pair_logit_bwd_f32"] + ["dfol_pair_logit_bwd_sums_f32"] * 2
    assert torch.equal(des, de) and torch.equal(dbes, dbe)
    assert none is None and torch.equal(desn, de) and torch.equal(db2n, db2)
    d64 = dp2.cpu().double()
    exact = torch.zeros(c.P, hid2, dtype=F64).index_add_(0, c.rep, d64)
    mag = torch.zeros(c.P, hid2, dtype=F64).index_add_(0, c.rep, d64.abs())
    nu = torch.as_tensor(c.counts, dtype=F64)[:, None] * 2.0 ** -24
    bound = nu / (1.0 - nu) * mag
    err = (db2.cpu().double() - exact).abs()
    assert bool((err <= bound).all())
    print("pair-train %-22s dB2  %.3f of its bound" % (c.id, float((err / bound.clamp(min=1e-300)).max())))
    for p in (p for p in range(c.P) if c.counts[p] == 0):
        assert not bool(db2[p].any()), p
    assert _fills_intact(c)


# ---------------------------------------------------------------------------------------------------
# 4. the guards (nothing here launches a kernel)
# ---------------------------------------------------------------------------------------------------
def _accepts(name, *args):
    try:
        _lib.call(name, *args)
    except _lib.DfolError:
        return False
    return True


def _entry_points_accept(hid1, hid2, max_n):
    """The size checks of the four entry points, which all come before `if (Q == 0) return` resp. `if (P == 0) return`: no operand is touched."""
    ld = (hid1 + 3) // 4 * 4                                     # (a legal row stride whatever the width: only the width's own check refuses)
    return (_accepts("dfol_pair_hidden1_fwd_f32", None, ld, None, ld, None, 4, None, None, None, None, 0, max_n, hid1, None, None, None)
            and _accepts("dfol_pair_hidden1_bwd_f32", None, None, None, None, None, None, 0, max_n, hid1, None, ld, None, ld, None, None)
            and _accepts("dfol_pair_logit_fwd_f32", None, hid2, hid2, None, hid2, None, None, 0, 0, 0, None, None)
            and _accepts("dfol_pair_logit_bwd_f32", None, None, hid2, hid2, None, hid2, None, 0, None, hid2, None, hid2, None, None))


@pytest.mark.parametrize("hid1", [12, 16, 20, 256, 512, 1024, 2048])
def test_python_guard_agrees_with_the_entry_points(hid1):
    edge = 16 * (1024 // (hid1 // 4))
    for hid2 in (512, 516):
        for max_n in (edge, edge + 1):
            assert _lib.pair_train_supported(hid1, hid2, max_n) == _entry_points_accept(hid1, hid2, max_n), (hid1, hid2, max_n)
    assert _lib.pair_train_supported(hid1, 512, edge) == (hid1 in (16, 256, 512, 1024))
    assert not _lib.pair_train_supported(hid1, 512, edge + 1) and not _lib.pair_train_supported(hid1, 516, edge)


def test_rebuilt_z_form_guard_values():
    ok = _lib.load().dfol_pair_hidden1_bwd_recompute_supported
    for max_n, hid1 in [(128, 256), (64, 512), (32, 1024), (2048, 16), (1, 256)]:
        assert ok(max_n, hid1) == 1, (max_n, hid1)
    for max_n, hid1 in [(129, 256), (65, 512), (33, 1024), (2049, 16), (8, 20), (8, 12), (8, 2048)]:
        assert ok(max_n, hid1) == 0, (max_n, hid1)


def _refused(words, fn):
    with pytest.raises(_lib.DfolError) as err:
        fn()
    for w in words:
        assert w in str(err.value), str(err.value)


def test_unsupported_sizes_raise_and_launch_nothing():
    """A DfolError that names the size, through _lib.call, before any launch: the outputs handed in stay as they were."""
    n_list = [3, 2]
    c = _hidden1_operands(256, n_list)
    z = torch.full((c.pairs, 256), float("nan"), device=DEV)
    geo = torch.full((c.pairs, 4), float("nan"), device=DEV)
    _refused(["max_n=257"], lambda: _hidden1_bwd_claiming(c, 257, z, geo))
    du = torch.full((c.O, 256), float("nan"), device=DEV)
    dv, part = du.clone(), torch.full((c.Q, 256, 4), float("nan"), device=DEV)
    _refused(["HID1=256", "max_n=129"], lambda: _lib.call(
        "dfol_pair_hidden1_bwd_recompute_f32", _lib._ptr(c.gz, F32), _lib._dp(c.U), c.U.stride(0), _lib._dp(c.V), c.V.stride(0), _lib._ptr(c.Wg, F32),
        _lib._ptr(geo, F32), _lib._ptr(c.geom[0], I32), _lib._ptr(c.geom[1], torch.int64), _lib._ptr(c.geom[2], I32), c.Q, 129, 256, _lib._dp(du),
        du.stride(0), _lib._dp(dv), dv.stride(0), _lib._ptr(part), _lib._stream()))
    assert bool(du.isnan().all()) and bool(dv.isnan().all()) and bool(part.isnan().all())
    # HID1 = 20: five lanes per row
    c20 = _hidden1_operands(20, n_list)
    _refused(["HID1=20"], lambda: _lib.pair_hidden1_fwd(c20.U, c20.V, c20.pos, c20.Wg, c20.geom[0], c20.geom[1], c20.geom[2], c20.max_n, c20.pairs))
    z20, geo20 = torch.zeros(c20.pairs, 20, device=DEV), torch.zeros(c20.pairs, 4, device=DEV)
    _refused(["HID1=20"], lambda: _lib.pair_hidden1_bwd(c20.gz, z20, geo20, c20.geom[0], c20.geom[1], c20.geom[2], c20.max_n, c20.O))
    assert not _lib.hidden1_recompute((c20.U, c20.V, c20.Wg), c20.gz, c20.max_n, 20)
    # HID2 = 516
    p2 = torch.zeros(8, 516, device=DEV)
    E, be = torch.zeros(1, 516, device=DEV), torch.zeros(1, device=DEV)
    off = torch.as_tensor(np.array([0, 8], np.int64)).to(DEV)
    _refused(["HID2=516"], lambda: _lib.pair_logit_fwd(p2, E, be, off, 8))
    _refused(["HID2=516"], lambda: _lib.pair_logit_bwd(torch.zeros(8, device=DEV), p2, E, off))
    _refused(["HID2=516"], lambda: _lib.pair_head_sums(torch.zeros(8, device=DEV), p2, E, off))
    _refused(["HID2=516"], lambda: _lib.pair_logit_fwd(p2.to(BF), E, be, off, 8))
    _refused(["HID2=12"], lambda: _lib.pair_logit_fwd(p2[:, :12].contiguous().to(BF), E[:, :12].contiguous(), be, off, 8))     # (bf16 storage: the vector kernels only)
    torch.cuda.synchronize()


def _hidden1_bwd_claiming(c, max_n, z, geo):
    return _lib.pair_hidden1_bwd(c.gz, z, geo, c.geom[0], c.geom[1], c.geom[2], max_n, c.O)


if __name__ == "__main__":                                        # the child of test_forced_1024_thread_form_on_small_ragged_images
    assert sys.argv[1:] == ["forced-1024"], sys.argv
    print(json.dumps(_forced_figures()))
