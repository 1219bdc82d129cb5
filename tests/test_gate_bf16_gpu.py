"""The one-launch gated Relate on bf16 tiles (dfol_relate_one_gate_fwd_bf16, csrc/dfol_logic_gate.hip) off one shape: against
the float64 gated cell of tests/gate_util.py evaluated on the tile AFTER bf16 rounding (rounded on the host, widened exactly - the kernel's
arithmetic is fp32 on exactly those values), under the tolerance policy tests/test_gate_native_gpu.py applies to the fp32 one-launch kernel
against the same restatement, and against that fp32 kernel on the widened tile (another order of the sum over rows: the policy's slack, not
bits).

Dispatch arms (NS / 8 column groups -> lanes per row LPR, rounded up to a power of two):
    NS 8 -> 1 | 16 -> 2 | 24 -> 4 (one idle lane group reading the clamped column) | 40 -> 8 | 104 -> 16 | 256 -> 32."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as U  # noqa: E402
import test_gate_native_gpu as TN  # noqa: E402  (restate_one: the float64 restatement of the one-posterior launch)
from dfol_vqa_amd import _lib  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu
dev = TN.dev
DEV = TN.DEV

# name: (NS, objects per image, predicates per image, negation, inactive rows)
SHAPES = {
    "ns8_lpr1_lone": (8, [7], [1], False, False),                      # P = 1: the lone predicate's literal FOR_ALL branch
    "ns16_lpr2_P3": (16, [16, 1, 5], [1, 1, 1], True, False),          # n = 1: an empty sum; n = 5 < NS - 8: a lane group of padding only
    "ns24_lpr4_P5": (24, [24, 13], [3, 2], True, True),                # 3 column groups on 4 lanes per row; partial last workgroup
    "ns40_lpr8_P9": (40, [40, 1, 27, 33], [3, 2, 2, 2], True, True),   # 5 groups on 8 lanes; three workgroups, the last with one predicate
    "ns104_lpr16_P3": (104, [104, 90, 57], [1, 1, 1], False, True),    # 13 groups on 16 lanes
    "ns256_lpr32_P5": (256, [256, 200, 3], [2, 2, 1], True, False),    # the full width: 2 rows per iteration
}
_CACHE = {}


def round_bf16(a):
    """float32 -> the bfloat16 value, widened back exactly (round to nearest even, on the host)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).to(torch.float32).numpy()


def problem(name):
    """Inputs of one shape, the tile rounded to bf16, and the restatement on the rounded tile in float32 and float64 (once, shared, never modified)."""
    if name in _CACHE:
        return _CACHE[name]
    NS, n_list, k_list, with_neg, with_inactive = SHAPES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    pq = np.repeat(np.arange(len(n_list)), k_list).astype(np.int32)
    P, Q = len(pq), len(n_list)
    pr = dict(NS=NS, n=np.asarray(n_list, np.int32), pq=pq, P=P, Q=Q, lone=(P == 1))
    prev, x, T = np.zeros((Q, NS), np.float32), np.zeros((P, NS), np.float32), np.full((P, NS, NS), -30, np.float32)
    for q, n in enumerate(n_list):
        prev[q, :n] = np.minimum(syn.table_log_likelihood(rng, (n,), "unif") * 0.3, 0)
    for p in range(P):
        n = n_list[pq[p]]
        x[p, :n] = np.minimum(syn.table_log_likelihood(rng, (n,), "unif") * 0.3, 0)
        t = syn.table_log_likelihood(rng, (n, n), "mix10")
        t[np.arange(n), np.arange(n)] = -30
        T[p, :n, :n] = t
    pr["neg"] = (np.arange(P) % 2 == 1).astype(np.uint8) if with_neg else None
    pr["active"] = (np.arange(P) != 1).astype(np.uint8) if with_inactive else None
    pr["W"] = rng.uniform(-0.7, 0.7, (2, 6, 2)).astype(np.float32)
    pr["c"] = rng.uniform(-0.7, 0.7, (2, 6)).astype(np.float32)
    op = dict(pr=pr, x=x, prev=prev, T_raw=T, T=round_bf16(T),                                    # T: what the kernel reads, as float32
              quant=(np.arange(P) % 2 == 0).astype(np.float32) if P > 1 else np.zeros(1, np.float32),      # EXISTS and FOR_ALL mixed
              flag=((np.arange(P) + NS // 8) % 2).astype(np.uint8) if P > 1 else np.ones(1, np.uint8))    # x on either axis
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        op[tag] = TN.restate_one(op, dt)
    op["swapped"] = TN.restate_one(op, torch.float64, swap=True)
    _CACHE[name] = op
    return op


def run_bf16(op):
    pr = op["pr"]
    gs, go = (_lib.gate_params(dev(pr["W"][k]), dev(pr["c"][k])) for k in (0, 1))
    tile = dev(op["T_raw"]).to(torch.bfloat16)                     # torch's device rounding: the same round-to-nearest-even
    return _lib.relate_one_gate_fwd_bf16(dev(op["x"]), dev(op["prev"]), tile, dev(pr["pq"]), dev(pr["n"]), dev(op["quant"]), dev(op["flag"]), gs, go,
                                         dev(pr["neg"]), dev(pr["active"]), lone_forall_identity=pr["lone"])


def test_the_cases_cover_what_they_are_for():
    ops_ = [problem(n) for n in SHAPES]
    assert [o["pr"]["NS"] for o in ops_] == [8, 16, 24, 40, 104, 256] and [o["pr"]["P"] for o in ops_] == [1, 3, 5, 9, 3, 5]
    lpr = lambda ns: 1 << max(0, (ns // 8 - 1).bit_length())
    assert [lpr(o["pr"]["NS"]) for o in ops_] == [1, 2, 4, 8, 16, 32]
    assert all(len(set(o["flag"])) == 2 and len(set(o["quant"])) == 2 for o in ops_ if o["pr"]["P"] > 1)            # mixed within every launch
    assert ops_[0]["pr"]["lone"] and ops_[0]["quant"][0] == 0
    assert any(o["pr"]["neg"] is not None and o["pr"]["neg"].any() for o in ops_) and any(o["pr"]["active"] is not None for o in ops_)
    for o in ops_:
        n, NS = o["pr"]["n"], o["pr"]["NS"]
        assert (n == NS).any() or NS == 8
        assert not np.array_equal(o["pr"]["W"][0], o["pr"]["W"][1]) and not np.array_equal(o["pr"]["c"][0], o["pr"]["c"][1])
        assert not np.array_equal(o["T"], o["T_raw"])             # the rounding is not the identity on these tiles
        assert np.array_equal(dev(o["T_raw"]).to(torch.bfloat16).float().cpu().numpy(), o["T"])      # host and device round alike
    assert any((o["pr"]["n"] == 1).any() for o in ops_) and any(((o["pr"]["n"] < o["pr"]["NS"] - 8) & (o["pr"]["n"] > 1)).any() for o in ops_)
    assert any(len(o["pr"]["pq"]) > len(set(o["pr"]["pq"])) for o in ops_)                                          # many-to-one pred_q


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_against_the_float64_restatement_on_the_rounded_tile(name):
    op = problem(name)
    pr = op["pr"]
    with torch.no_grad():
        out = run_bf16(op)
        again = run_bf16(op)
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.cpu().numpy().view(np.uint32))           # two launches, the same bits
    print(name, "max |dp| vs fp64", np.abs(np.exp(got) - np.exp(op["f64"])).max(), "restatement's own fp32", np.abs(np.exp(op["f32"]) - np.exp(op["f64"])).max())
    U.check_logprob(got, op["f32"], op["f64"], name)
    for p in range(pr["P"]):
        assert not got[p, pr["n"][pr["pq"][p]]:].view(np.uint32).any(), (name, p, "padding")  # exactly +0
    if pr["active"] is not None:                                   # a no-op row is prev's row, bit for bit
        p = int(np.nonzero(pr["active"] == 0)[0][0])
        q, n = pr["pq"][p], pr["n"][pr["pq"][p]]
        assert np.array_equal(got[p, :n].view(np.uint32), op["prev"][q, :n].view(np.uint32))
    # inner and outer gate exchanged lies outside the bound: the bound tells the two apart (CPU, the restatement alone)
    with pytest.raises(AssertionError):
        U.check_logprob(op["swapped"], op["f32"], op["f64"], name + " with the gates swapped")


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_against_the_fp32_kernel_on_the_widened_tile(name):
    """The fp32 one-launch kernel on the widened tile computes the same terms, joined in another order (a lane of the bf16 kernel owns 8 columns,
    so other rows share a lane): each lies within policy (ii) of the float64 value, so within twice that of each other - the bound
    test_gate_native_gpu.test_kernel_against_the_generic_route states for two routes to one value."""
    op = problem(name)
    with torch.no_grad():
        b16 = run_bf16(op).cpu().numpy()
        f32 = TN.run_one(op).cpu().numpy()                         # op["T"]: the widened tile
    U.check_logprob(f32, op["f32"], op["f64"], name + " fp32 kernel")
    err = np.abs(np.exp(b16) - np.exp(f32)).max()
    own = np.abs(np.exp(op["f32"]) - np.exp(op["f64"])).max()
    print(name, "bf16 kernel vs fp32 kernel max |dp|", err, "bound", 2 * (2.0 * own + 1e-6))
    assert err <= 2 * (2.0 * own + 1e-6), (name, err, own)


def test_refusals_reach_no_launch():
    SENTINEL = 12345.0
    gs = go = torch.zeros(18, device=DEV)

    def raw(NS, P=3):
        """The C entry point itself, over buffers large enough for the call it refuses."""
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
        out = torch.full((P, NS), SENTINEL, device=DEV)
        t = [z(P, NS), z(P, NS), z(P, NS, NS, dt=torch.bfloat16), z(P, dt=torch.int32), z(P, dt=torch.int32), z(P), z(P, dt=torch.uint8)]
        with pytest.raises(_lib.DfolError, match="relate_one_gate_fwd_bf16"):
            _lib.call("dfol_relate_one_gate_fwd_bf16", *[a.data_ptr() for a in t], None, 0, None, P, NS, 0, gs.data_ptr(), go.data_ptr(), out.data_ptr(),
                      _lib._stream())
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), NS

    raw(12)
    raw(264)
    op = problem("ns16_lpr2_P3")
    pr = op["pr"]
    args = lambda tile: (dev(op["x"]), dev(op["prev"]), tile, dev(pr["pq"]), dev(pr["n"]), dev(op["quant"]), dev(op["flag"]), gs, go)
    with pytest.raises(_lib.DfolError, match="bfloat16"):
        _lib.relate_one_gate_fwd_bf16(*args(dev(op["T"])))         # an fp32 tile handed to the bf16 wrapper
    for NS in (12, 264):
        with pytest.raises(_lib.DfolError, match="NS=%d" % NS):
            _lib.relate_one_gate_fwd_bf16(*args(torch.zeros(3, NS, NS, dtype=torch.bfloat16, device=DEV)))
    with pytest.raises(_lib.DfolError):                            # and the fp32 wrapper keeps refusing the bf16 tile
        _lib.relate_one_gate_fwd(*args(dev(op["T"]).to(torch.bfloat16)))
    # P == 0: an empty result, no launch
    e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=DEV)
    out = _lib.relate_one_gate_fwd_bf16(e(0, 16), dev(op["prev"]), e(0, 16, 16, dt=torch.bfloat16), e(0, dt=torch.int32), dev(pr["n"]), e(0), e(0, dt=torch.uint8),
                                        gs, go)
    assert tuple(out.shape) == (0, 16)
    torch.cuda.synchronize()
