"""dfol_modulate_bwd_f32 (csrc/dfol_logic.hip; the backward of apply_modulations, one launch per calibrated operator in the calibrator phases) off
the one shape of test_kernels_gpu.test_modulate_backward_kernel_against_autograd (NS = 32, n <= 30).  The kernel is one wavefront per predicate
with a `for (c = lane; c < NS; c += 64)` loop and four wave sums:

      NS    passes of the column loop
       4    one, 60 lanes idle
      64    exactly one
      65    one plus one lane
     104    two (the workload's 100 objects, padded)
     260    five, the last with a tail of 4

Called through _lib.modulate_bwd and through the autograd Function of ops.modulate.  Reference: ops._modulate_reference under torch autograd in
float64 on the CPU; the same in float32 is the reference's own noise, own = |ref32 - ref64|.

Inputs: att = -|N(0, 2)| with one cell at exactly 0.0 (log 1: log_not at its clamp) and one at -80, both in the predicate whose image fills the
row (the -80 in its last column); mods ~ U(0.02, 0.98); g ~ N(0, 1); NaN in every padding cell (columns >= n) of att and of g_out as the kernel
sees them.  (The reference gets finite padding: torch.where's backward multiplies a NaN by the zero it hands the unselected branch.)

Bounds.  g_att is elementwise: |got - ref64| <= 8 own + 2e-5 max(1, |ref64|) (2e-5: the bar of the existing test; 8: grad_close's K).  g_mods is
four sums per predicate: |got - ref64| <= 8 own + 2e-5 A + 1e-7 with A the float64 sum of the addends' magnitudes.  With att <= 0 every addend
of sums 1, 2, 3 has the sign of g and of sum 0 the sign of -g (rt in [0, 1], ru <= 0, a <= 0, log_not(a) <= 0), so the float64 reference with
|g| as cotangent returns A up to sign; the CPU test asserts that sign pattern.  The kernel's accumulation adds at most (NS / 64 + 6) 2^-24 < 1e-6
of A; the 2e-5 covers the transcendentals.  The CPU test also asserts own <= the bar in every entry of the main cases (seeds chosen for it), so
the whole bound is never more than 9 bars.

The clamp corners (d = 0, d = 1, c = 0, and d = 1 with att = -80 so that S <= eps) are a case of their own at NS = 104, held to the existing
test's tolerance unchanged: 2e-5 abs + rel on g_att, 2e-4 on g_mods."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import ops  # noqa: E402

# name -> (NS, objects per question, predicates per question, seed)
MAIN = {
    "ns4": (4, [1, 4, 3, 2], [2, 1, 3, 1], 41),
    "ns64": (64, [1, 64, 37, 63, 5], [1, 3, 2, 1, 2], 42),
    "ns65": (65, [1, 65, 63, 64, 30], [2, 1, 3, 1, 2], 43),
    "ns104": (104, [1, 104, 63, 64, 65, 100, 90], [1, 2, 3, 1, 2, 1, 2], 44),
    "ns260": (260, [1, 260, 63, 64, 65, 129, 256, 200], [1, 2, 1, 3, 1, 2, 1, 1], 45),
}
CORNERS = {"ns104_corners": (104, [104, 70, 1, 65, 100, 33], [2, 1, 3, 1, 2, 1], 46)}
CASES = dict(MAIN, **CORNERS)
BAR, K = 2e-5, 8.0
_CACHE = {}


def _reference(att, mods, g, valid, dt):
    a = torch.tensor(att, dtype=dt, requires_grad=True)
    m = torch.tensor(mods, dtype=dt, requires_grad=True)
    out = ops._modulate_reference(a, m, torch.from_numpy(valid))
    ga, gm = torch.autograd.grad(out, (a, m), torch.tensor(g, dtype=dt))
    return ga.numpy().astype(np.float64), gm.numpy().astype(np.float64)


def case(name):
    """The inputs (as the kernel gets them: NaN padding) and the float64 / float32 references, once per case."""
    if name in _CACHE:
        return _CACHE[name]
    NS, n_list, k_list, seed = CASES[name]
    rng = np.random.RandomState(seed)
    pq = np.repeat(np.arange(len(n_list)), k_list).astype(np.int32)
    P = len(pq)
    n_p = np.asarray(n_list)[pq]
    valid = np.arange(NS)[None, :] < n_p[:, None]
    att = (-np.abs(rng.normal(size=(P, NS))) * 2).astype(np.float32)
    mods = rng.uniform(0.02, 0.98, size=(P, 4)).astype(np.float32)
    g = rng.normal(size=(P, NS)).astype(np.float32)
    full = int(np.nonzero(n_p == NS)[0][0])                       # a predicate whose image fills the row
    att[full, 0], att[full, NS - 1] = 0.0, -80.0
    corners = None
    if name in CORNERS:
        rows = [int(p) for p in np.nonzero(n_p >= 65)[0][:4]]      # every corner row runs the second pass of the column loop
        assert len(rows) == 4
        mods[rows[0], 3], mods[rows[1], 3], mods[rows[2], 2] = 0.0, 1.0, 0.0
        mods[rows[3], 3], mods[rows[3], 0] = 1.0, 0.9              # d = 1 and alpha = 9: at att = -80, e^t = 0 and e^u = eps, so S <= eps
        att[rows[3], [2, 64]] = -80.0
        corners = rows
    ref_att, ref_g = np.where(valid, att, np.float32(-1.0)), np.where(valid, g, np.float32(0.0))
    ga64, gm64 = _reference(ref_att, mods, ref_g, valid, torch.float64)
    ga32, gm32 = _reference(ref_att, mods, ref_g, valid, torch.float32)
    _, gm_abs = _reference(ref_att, mods, np.abs(ref_g), valid, torch.float64)
    c = dict(name=name, NS=NS, P=P, pq=pq, n=np.asarray(n_list, np.int32), n_p=n_p, valid=valid, mods=mods, corners=corners,
             att=np.where(valid, att, np.float32(np.nan)), g=np.where(valid, g, np.float32(np.nan)),
             ga64=ga64, gm64=gm64, own_a=np.abs(ga32 - ga64), own_m=np.abs(gm32 - gm64), gm_abs=gm_abs, A=np.abs(gm_abs))
    _CACHE[name] = c
    return c


def bar_att(c):
    return BAR * np.maximum(1.0, np.abs(c["ga64"]))


def bar_mods(c):
    return BAR * c["A"] + 1e-7


# ---- the generated inputs (no GPU) -----------------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_they_are_for():
    assert sorted(CASES[k][0] for k in MAIN) == [4, 64, 65, 104, 260] and CASES["ns104_corners"][0] == 104
    for name, (NS, n_list, k_list, _) in CASES.items():
        c = case(name)
        assert len(n_list) == len(k_list) <= 8 and max(n_list) == NS and set(k_list) == {1, 2, 3}
        assert (np.diff(c["pq"]) >= 0).all() and np.bincount(c["pq"]).tolist() == k_list           # sorted, many-to-one
        assert np.isnan(c["att"][~c["valid"]]).all() and np.isnan(c["g"][~c["valid"]]).all()
        assert np.isfinite(c["att"][c["valid"]]).all() and (c["att"][c["valid"]] <= 0).all()
        assert (c["att"][c["valid"]] == 0.0).sum() >= 1 and (c["att"][c["valid"]] == -80.0).sum() >= 1
        if name in MAIN:
            assert {1, NS} <= set(n_list) and (NS <= 64 or {63, 64, 65} <= set(n_list)), name
            assert c["mods"].min() >= 0.02 and c["mods"].max() <= 0.98
            if NS > 64:                                            # the -80 sits in a later pass of the column loop
                assert (c["att"][:, 64:][c["valid"][:, 64:]] == -80.0).any()
    c = case("ns104_corners")
    r = c["corners"]
    assert [c["mods"][r[0], 3], c["mods"][r[1], 3], c["mods"][r[2], 2], c["mods"][r[3], 3]] == [0.0, 1.0, 0.0, 1.0]
    assert (c["n_p"][r] >= 65).all() and c["att"][r[3], 64] == -80.0 and c["att"][r[3], 2] == -80.0
    t = 10.0 * c["mods"][r[3], 0] * -80.0 + np.log(10.0 * c["mods"][r[3], 2])
    assert np.exp(np.float32(t)) == 0.0                            # e^t underflows in float32: S = e^u = the clamp of slog(1 - d)


def test_the_sign_pattern_behind_A():
    """With |g| as cotangent, sum 0 is <= 0 and sums 1, 2, 3 are >= 0 in every predicate - every addend of a sum has one sign, so |that sum| is
    the sum of the addends' magnitudes - and A bounds the gradient itself."""
    for name in CASES:
        c = case(name)
        assert (c["gm_abs"][:, 0] <= 0).all() and (c["gm_abs"][:, 1:] >= 0).all(), name
        assert (np.abs(c["gm64"]) <= c["A"] * (1 + 1e-12) + 1e-300).all(), name
        assert (c["A"] > 0).any(axis=0).all(), name


@pytest.mark.parametrize("name", list(MAIN))
def test_the_references_own_noise_stays_under_the_bar(name):
    """own <= the bar in every entry of the main cases: 8 own + bar is then at most 9 bars, and own cannot hide a failure."""
    c = case(name)
    ra, rm = (c["own_a"] / bar_att(c))[c["valid"]].max(), (c["own_m"] / bar_mods(c)).max()
    print("  %s: own / bar  g_att %.3f  g_mods %.3f" % (name, ra, rm))
    assert ra <= 1.0 and rm <= 1.0, (name, ra, rm)
    assert not c["own_a"][~c["valid"]].any() and not c["ga64"][~c["valid"]].any()        # the reference's padding is 0


# ---- the kernel --------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def run(c):
    """-> (g_att, g_mods) of the direct call, after the padding, repeat and autograd assertions every case shares."""
    from dfol_vqa_amd import _lib
    _lib.load()
    pq, n_obj = dev(c["pq"]), dev(c["n"])
    ga, gm = _lib.modulate_bwd(dev(c["g"]), dev(c["att"]), dev(c["mods"]), pq, n_obj)
    ga2, gm2 = _lib.modulate_bwd(dev(c["g"]), dev(c["att"]), dev(c["mods"]), pq, n_obj)
    a32, m32 = dev(c["att"]).requires_grad_(True), dev(c["mods"]).requires_grad_(True)
    fa, fm = torch.autograd.grad(ops.modulate(a32, m32, pq, n_obj), (a32, m32), dev(c["g"]))
    torch.cuda.synchronize()
    ga, gm, ga2, gm2, fa, fm = (t.cpu().numpy() for t in (ga, gm, ga2, gm2, fa, fm))
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    assert not bits(ga)[~c["valid"]].any(), (c["name"], "g_att padding is not +0")
    assert np.isfinite(gm).all() and np.isfinite(ga).all(), c["name"]
    assert np.array_equal(bits(ga), bits(ga2)) and np.array_equal(bits(gm), bits(gm2)), (c["name"], "two runs differ")
    assert np.array_equal(bits(ga), bits(fa)) and np.array_equal(bits(gm), bits(fm)), (c["name"], "ops.modulate's autograd differs")
    return ga.astype(np.float64), gm.astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MAIN))
def test_kernel_against_float64_autograd(name):
    c = case(name)
    ga, gm = run(c)
    err_a, err_m = np.abs(ga - c["ga64"]), np.abs(gm - c["gm64"])
    bound_a, bound_m = K * c["own_a"] + bar_att(c), K * c["own_m"] + bar_mods(c)
    i, j = np.unravel_index(np.argmax(err_a / bound_a), err_a.shape), np.unravel_index(np.argmax(err_m / bound_m), err_m.shape)
    print("  %s: g_att largest err %.3g (bound there %.3g, |ref| %.3g), worst err / bound %.3f at %s;  g_mods largest err %.3g (A there %.3g), "
          "worst err / bound %.3f at %s (err %.3g, bound %.3g)" % (name, err_a.max(), bound_a.flat[np.argmax(err_a)], np.abs(c["ga64"]).flat[np.argmax(err_a)],
                                                                  (err_a / bound_a).max(), i, err_m.max(), c["A"].flat[np.argmax(err_m)],
                                                                  (err_m / bound_m).max(), j, err_m[j], bound_m[j]))
    assert (err_a <= bound_a).all(), (name, "g_att", i, ga[i], c["ga64"][i], bound_a[i])
    assert (err_m <= bound_m).all(), (name, "g_mods", j, gm[j], c["gm64"][j], bound_m[j])


@pytest.mark.gpu
def test_clamp_corners():
    c = case("ns104_corners")
    ga, gm = run(c)
    err_a, err_m = np.abs(ga - c["ga64"]), np.abs(gm - c["gm64"])
    print("  corners: g_att largest err %.3g, g_mods largest err %.3g (largest |g_mods| %.3g)" % (err_a.max(), err_m.max(), np.abs(c["gm64"]).max()))
    assert (err_a <= 2e-5 + 2e-5 * np.abs(c["ga64"])).all(), err_a.max()
    assert (err_m <= 2e-4 + 2e-4 * np.abs(c["gm64"])).all(), err_m.max()
