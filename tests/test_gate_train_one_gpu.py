"""The one-posterior gated Relate of the train step (DFOL_GATE_TRAIN=1): dfol_relate_keep_gate_fwd_f32 and
dfol_relate_keep_gate_bwd_f32 (csrc/dfol_logic_gate.hip) against the float64 restatement of tests/gate_util.py and its torch autograd, and
against the generic gated route (gate, gate, relate_gate_fwd(want), gate) they replace.

The problems are test_gate_native_gpu.one_problem's, subject flags mixed within the launch.  Those kernels read the tile with prev's objects
along rows; the train step's tile holds SUBJECTS along rows for every predicate, so the kernels here get the transpose of T where the flag is
set.  With S that tile:  flag set -> post_s of t_relate_gate(a = x, b = prev, l = S);  clear -> post_o of t_relate_gate(a = prev, b = x, l = S).

Dispatch arms (NS / 4 column groups -> lanes per row; NS > 256 -> the plain workgroup kernel): the shapes of test_trainable_gate_gpu.SHAPES,
NS 4 -> LPR 1 | 8 -> 2 | 12, 16 -> 4 | 20, 32 -> 8 | 36, 64 -> 16 | 68, 128 -> 32 | 132, 256 -> 64 | 260 -> plain.  The backward is one
kernel for every NS <= 1024."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gate_util as GU  # noqa: E402
import golden_util as U  # noqa: E402
import test_gate_native_gpu as GN  # noqa: E402
import test_trainable_gate_gpu as TG  # noqa: E402
from dfol_vqa_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu
dev = TG.dev
_CACHE = {}
LEAVES = ("x", "prev", "S", "W", "c")


def keep_problem(name):
    """one_problem(name) with the subject-row tile S, the restatement's kept posterior and its gradients (cotangent: the problem's own random one,
    zero on padding) in float32 and float64; computed once, shared, never modified."""
    if name in _CACHE:
        return _CACHE[name]
    op = GN.one_problem(name)
    pr = op["pr"]
    f = op["flag"].astype(bool)
    kp = dict(op=op, pr=pr, S=np.ascontiguousarray(np.where(f[:, None, None], op["T"].transpose(0, 2, 1), op["T"])), cot=pr["cot"][1])
    live = np.ones(pr["P"], bool) if pr["active"] is None else pr["active"].astype(bool)
    kp["live"] = live
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        kp[tag] = restate_keep(kp, dt, kp["cot"])
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):                      # the cotangent of the live rows alone
        kp[tag + "_live"] = kp[tag]["g"] if live.all() else restate_keep(kp, dt, kp["cot"] * live[:, None])["g"]
    _CACHE[name] = kp
    return kp


def restate_keep(kp, dt, cot):
    op, pr = kp["op"], kp["pr"]
    src = {"x": op["x"], "prev": op["prev"], "S": kp["S"], "W": pr["W"], "c": pr["c"]}
    lv = {k: torch.tensor(src[k], dtype=dt, requires_grad=True) for k in LEAVES}
    any_neg = pr["neg"] is not None
    rows = []
    for p in range(pr["P"]):
        q = pr["pq"][p]
        n = pr["n"][q]
        x, prev, S = lv["x"][p, :n], lv["prev"][q, :n], lv["S"][p, :n, :n]
        if pr["active"] is not None and not pr["active"][p]:
            post = prev
        else:
            ng, qp = (float(pr["neg"][p]) if any_neg else 0.0), op["quant"][p]
            gates = (lv["W"][0], lv["c"][0], lv["W"][1], lv["c"][1])
            if op["flag"][p]:
                post = GU.t_relate_gate(x, prev, S, qp, qp, ng, any_neg, *gates, lone_forall_identity=pr["lone"])[0]
            else:
                post = GU.t_relate_gate(prev, x, S, qp, qp, ng, any_neg, *gates, lone_forall_identity=pr["lone"])[1]
        rows.append(torch.cat([post, torch.zeros(pr["NS"] - n, dtype=dt)]))
    out = torch.stack(rows)
    g = torch.autograd.grad((out * torch.tensor(cot, dtype=dt)).sum(), [lv[k] for k in LEAVES], allow_unused=True)
    return {"out": out.detach().numpy(), "g": {k: (np.zeros(lv[k].shape) if v is None else v.numpy().astype(np.float64)) for k, v in zip(LEAVES, g)}}


def owned_masks(kp):
    pr = kp["pr"]
    col = np.arange(pr["NS"])
    prev = col[None, :] < pr["n"][:, None]                                   # [Q, NS]
    x = (col[None, :] < pr["n"][pr["pq"]][:, None]) & kp["live"][:, None]      # [P, NS]: a no-op predicate's posterior does not see x
    tile = x[:, :, None] & x[:, None, :] & ~np.eye(pr["NS"], dtype=bool)[None]
    return x, prev, tile


def launch_args(kp, tile=None, flag=None):
    op, pr = kp["op"], kp["pr"]
    return (dev(op["x"]), dev(op["prev"]), dev(kp["S"]) if tile is None else tile, dev(pr["pq"]), dev(pr["n"]), dev(op["quant"]),
            dev(op["flag"]) if flag is None else flag)


def run_fwd(kp, **kw):
    pr = kp["pr"]
    gs, go = (_lib.gate_params(dev(pr["W"][k]), dev(pr["c"][k])) for k in (0, 1))
    return _lib.relate_keep_gate_fwd(*launch_args(kp, **kw), gs, go, dev(pr["neg"]), dev(pr["active"]), lone_forall_identity=pr["lone"])


def run_autograd(kp, cot):
    """ops.relate_keep_gate and its backward -> {leaf name: gradient}."""
    op, pr = kp["op"], kp["pr"]
    x, prev, S = (torch.tensor(a, device=TG.DEV, requires_grad=True) for a in (op["x"], op["prev"], kp["S"]))
    Ws, cs, Wo, co = TG.gate_tensors(pr, grad=True)
    pq = dev(pr["pq"])
    pq._dfol_sorted = True                                        # (np.repeat of arange: non-decreasing)
    out = ops.relate_keep_gate(x, prev, S, pq, dev(pr["n"]), dev(op["quant"]), dev(op["flag"]), Ws, cs, Wo, co, dev(pr["neg"]), dev(pr["active"]),
                               lone_forall_identity=pr["lone"])
    (out * dev(cot)).sum().backward()
    g = lambda t: t.grad.cpu().numpy()
    return out.detach(), {"x": g(x), "prev": g(prev), "S": g(S), "W": np.stack([g(Ws), g(Wo)]), "c": np.stack([g(cs), g(co)])}


def check_all(got, r32, r64, kp, what):
    o_x, o_prev, o_tile = owned_masks(kp)
    U.check_gradient(got["x"], r32["x"], r64["x"], what + " d x", owned=o_x)
    U.check_gradient(got["prev"], r32["prev"], r64["prev"], what + " d prev", owned=o_prev)
    U.check_gradient(got["S"], r32["S"], r64["S"], what + " d tile", owned=o_tile)
    for k in (0, 1):
        U.check_gradient(got["W"][k], r32["W"][k], r64["W"][k], "%s d W%d" % (what, k))
        U.check_gradient(got["c"][k], r32["c"][k], r64["c"][k], "%s d c%d" % (what, k))


def test_the_cases_cover_what_they_are_for():
    kps = [keep_problem(n) for n in TG.SHAPES]
    assert sorted({k["pr"]["NS"] for k in kps}) == [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260]
    assert any(len(set(k["op"]["flag"])) == 2 for k in kps) and any(len(set(k["op"]["quant"])) == 2 for k in kps)      # mixed within a launch
    assert {int(v) for k in kps for v in k["op"]["flag"]} == {0, 1} and {float(v) for k in kps for v in k["op"]["quant"]} == {0.0, 1.0}
    assert any(k["pr"]["neg"] is not None and k["pr"]["neg"].any() for k in kps) and any(not k["live"].all() for k in kps)
    assert any(k["pr"]["P"] == 1 and k["op"]["quant"][0] == 0 for k in kps) and any(k["pr"]["P"] == 5 for k in kps)      # the literal branch; P % 4 != 0
    assert any((k["pr"]["n"] == 1).any() for k in kps) and any((k["pr"]["n"] % 4 != 0).any() for k in kps)
    assert any(len(k["pr"]["pq"]) > len(set(k["pr"]["pq"])) for k in kps)                                               # many-to-one pred_q
    assert {TG.SHAPES[n][5] for n in TG.SHAPES} == {0.7, 4.0}
    for k in kps:                                                 # the subject-row tile differs from the prev-row one where a flag is set
        if k["op"]["flag"].any() and k["pr"]["n"].max() > 1:
            assert not np.array_equal(k["S"], k["op"]["T"])
        np.testing.assert_allclose(k["f64"]["out"], k["op"]["f64"], rtol=0, atol=1e-12)      # the same restatement as the inference kernel's


@pytest.mark.parametrize("name", list(TG.SHAPES))
def test_forward_against_the_float64_restatement(name):
    kp = keep_problem(name)
    op, pr = kp["op"], kp["pr"]
    with torch.no_grad():
        got = run_fwd(kp).cpu().numpy()
        again = run_fwd(kp).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))                          # two launches, the same bits
    U.check_logprob(got, kp["f32"]["out"], kp["f64"]["out"], name)
    for p in range(pr["P"]):
        assert not got[p, pr["n"][pr["pq"][p]]:].view(np.uint32).any(), (name, p, "padding")  # exactly +0
    for p in np.nonzero(~kp["live"])[0]:                           # a no-op row is prev's row, bit for bit
        q, n = pr["pq"][p], pr["n"][pr["pq"][p]]
        assert np.array_equal(got[p, :n].view(np.uint32), op["prev"][q, :n].view(np.uint32))
    # inner and outer gate exchanged lies outside the bound: the bound tells the two apart (CPU, the restatement alone)
    with pytest.raises(AssertionError):
        U.check_logprob(op["swapped"], kp["f32"]["out"], kp["f64"]["out"], name + " with the gates swapped")


@pytest.mark.parametrize("name", list(TG.SHAPES))
def test_backward_against_the_float64_restatement(name):
    """The bounds of test_trainable_gate_gpu.test_backward_against_the_float64_restatement (golden_util.check_gradient, K = 8 times the
    formula's own float32 noise, floor 2^-20; the parameter gradients against the tensor's scale).  Cells nobody owns are +0."""
    kp = keep_problem(name)
    out, got = run_autograd(kp, kp["cot"])
    U.check_logprob(out.cpu().numpy(), kp["f32"]["out"], kp["f64"]["out"], name + " forward under autograd")
    check_all(got, kp["f32"]["g"], kp["f64"]["g"], kp, name)


@pytest.mark.parametrize("name", list(TG.SHAPES))
def test_backward_against_the_generic_route(name):
    """gate, gate, ops.relate_gate_fwd(want), gate under autograd on the same inputs, one question per predicate, and the one-launch pair: both
    within the bound of the same float64 gradients (another summation order: no bit equality).  A no-op row of the generic cell is the wanted
    side's own prior - x where x is the subject - and the interpreter's mask puts prev back; the one-launch kernel writes prev at once
    (test_gate_native_gpu says the same of the forward).  So the cotangent here is the problem's on the live rows and zero on the no-op rows:
    what the two routes share."""
    kp = keep_problem(name)
    op, pr = kp["op"], kp["pr"]
    cot = kp["cot"] * kp["live"][:, None]
    _, one = run_autograd(kp, cot)
    P = pr["P"]
    x, prev, S = (torch.tensor(a, device=TG.DEV, requires_grad=True) for a in (op["x"], op["prev"], kp["S"]))
    Ws, cs, Wo, co = TG.gate_tensors(pr, grad=True)
    quant, g = dev(op["quant"]), dev(op["flag"].astype(np.float32))
    prev_p = prev[torch.tensor(pr["pq"].astype(np.int64), device=TG.DEV)]
    prior_s, _ = ops.gate(x, prev_p, quant, quant, g)
    prior_o, _ = ops.gate(prev_p, x, quant, quant, g)
    want = dev(np.where(op["flag"] > 0, _lib.WANT_SUBJECT, _lib.WANT_OBJECT).astype(np.uint8))
    ident = dev(np.arange(P, dtype=np.int32))
    ident._dfol_sorted = True
    ps, po = ops.relate_gate_fwd(prior_s, prior_o, S, ident, dev(pr["n"][pr["pq"]]), quant, quant, Ws, cs, Wo, co, dev(pr["neg"]), dev(pr["active"]),
                                 want=want, lone_forall_identity=pr["lone"])
    kept, _ = ops.gate(ps, po, quant, quant, g)
    (kept * dev(cot)).sum().backward()
    t = lambda v: v.grad.cpu().numpy()
    generic = {"x": t(x), "prev": t(prev), "S": t(S), "W": np.stack([t(Ws), t(Wo)]), "c": np.stack([t(cs), t(co)])}
    o_x, o_prev, o_tile = owned_masks(kp)
    for what, got in (("one launch", one), ("generic route", generic)):
        r32, r64 = kp["f32_live"], kp["f64_live"]
        U.check_gradient(got["x"], r32["x"], r64["x"], "%s %s d x" % (name, what), owned=o_x, signed_zero_ok=True)
        U.check_gradient(got["prev"], r32["prev"], r64["prev"], "%s %s d prev" % (name, what), owned=o_prev, signed_zero_ok=True)
        U.check_gradient(got["S"], r32["S"], r64["S"], "%s %s d tile" % (name, what), owned=o_tile, signed_zero_ok=True)
        for k in (0, 1):
            U.check_gradient(got["W"][k], r32["W"][k], r64["W"][k], "%s %s d W%d" % (name, what, k))
            U.check_gradient(got["c"][k], r32["c"][k], r64["c"][k], "%s %s d c%d" % (name, what, k))


def test_parameter_gradients_repeat_bit_for_bit():
    for name in ("ns36_lpr16", "ns12_lpr4_manytoone"):
        kp = keep_problem(name)
        runs = []
        for _ in range(2):
            _, got = run_autograd(kp, kp["cot"])
            runs.append(np.concatenate([got[k].reshape(-1) for k in LEAVES]).view(np.uint32))
            assert got["W"][0].any() and got["W"][1].any() and got["c"][0].any() and got["c"][1].any()
        assert np.array_equal(runs[0], runs[1])


def test_refusals():
    """None reaches a launch: 1028 object slots in the backward, a bf16 tile, a flag count that is not P."""
    kp = keep_problem("ns8_lone")
    pr = kp["pr"]
    gs, go = (_lib.gate_params(dev(pr["W"][k]), dev(pr["c"][k])) for k in (0, 1))
    with pytest.raises(_lib.DfolError, match="fp32 tiles"):
        run_fwd(kp, tile=dev(kp["S"]).to(torch.bfloat16))
    with pytest.raises(_lib.DfolError, match="subject flags"):
        run_fwd(kp, flag=dev(np.ones(3, np.uint8)))
    NS = 1028
    z = lambda *s: torch.zeros(*s, device=TG.DEV)
    one = torch.ones(1, dtype=torch.uint8, device=TG.DEV)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=TG.DEV)
    with pytest.raises(_lib.DfolError, match="at most 1024"):
        _lib.relate_keep_gate_bwd(z(1, NS), z(1, NS), z(1, NS), z(1, NS, NS), i32(0), i32(NS), z(1), one, gs, go, None, None, True)
    with pytest.raises(_lib.DfolError, match="fp32 tiles"):
        _lib.relate_keep_gate_bwd(z(1, 8), z(1, 8), z(1, 8), z(1, 8, 8).to(torch.bfloat16), i32(0), i32(7), z(1), one, gs, go, None, None, True)
    with pytest.raises(_lib.DfolError, match="subject flags"):
        _lib.relate_keep_gate_bwd(z(1, 8), z(1, 8), z(1, 8), z(1, 8, 8), i32(0), i32(7), z(1), torch.ones(2, dtype=torch.uint8, device=TG.DEV), gs, go,
                                  None, None, True)
    torch.cuda.synchronize()
