"""The ungated Relate computes ONE body (csrc/dfol_logic.hip): dfol_relate_keep_fwd_f32 is dfol_relate_fwd_f32's fused body with
prev's quantifier on both sides and exactly one side wanted.  For NS > 256 that is shared code (relate_big_cols / relate_big_rows); for
NS <= 256 relate_keep_fwd_kernel is written out beside relate_fwd_kernel, and this file is what keeps the two from drifting apart.  So

    _lib.relate_keep_fwd(x, prev, S, ..., flag)
    _lib.relate_fwd on the same subject-row tile, one question per predicate, both quantifiers prev's, `want` asking for x's side only
        (flag 1: prior_s = x, prior_o = prev;  flag 0: prior_s = prev, prior_o = x)

return THE SAME BITS on every live cell and +0 on padding.  No tolerance appears in this file.

Every predicate is active (the two kernels' no-op rows differ by design: prev's row against the wanted side's prior).  x, prev and S carry NaN in
every padding cell and a live value on S's diagonal (test_relate_train_one_gpu.poisoned, whose generator makes the inputs).

Kinds: FOR_ALL; negated FOR_ALL; FOR_ALL with one term below log 1e-20, which sends both kernels from the transcendental-free sweep to the clamping
loop; EXISTS with one entry of prev above 0, which sends both from the complement form to the clamping loop.  EXISTS on its complement form is left
out on purpose: the two-posterior kernel combines a row's partials through LDS, the kept one by the DPP group OR, so their bits may differ by design
(each is held to the float64 restatement elsewhere).  Sizes: NS 8 (two lanes per row), 40 (sixteen), 260 (the plain kernels), one image at n = NS
and one below; both flag values in every case."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_relate_train_one_gpu as T  # noqa: E402
from dfol_vqa_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
dev = T.dev

SIZES = {8: [8, 5], 40: [40, 33], 260: [260, 131]}
KINDS = ("forall", "forall_negated", "forall_at_the_clamp", "exists_prev_above_log1")


def problem(NS, kind):
    """test_relate_train_one_gpu's generator on a shape of this file (two predicates per image, flags 0 and 1 in each; no restatement: the kernels
    are compared with each other), then the kind's edit."""
    quants = "exists" if kind.startswith("exists") else "forall"
    kp = T.make_problem("one_body_ns%d_%s" % (NS, quants), (NS, SIZES[NS], [2, 2], False, False, quants, "mixed"), restate=False)
    if kind == "forall_negated":                       # every predicate negated; l <= -3 keeps l' = log(1 - e^l) and its sums off the clamp
        kp["neg"] = np.ones(kp["P"], np.uint8)
        kp["S"] = -(3.0 + np.abs(kp["S"])).astype(np.float32)
    elif kind == "forall_at_the_clamp":                # one live off-diagonal term below log(1e-20) = -46.05: in row 0 and in column 1
        kp["S"][:, 0, 1] = -50.0
    elif kind == "exists_prev_above_log1":             # a probability above 1 in the prior the aggregate reads
        kp["prev"][:, 2] = 0.25
    return kp


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("NS", sorted(SIZES))
def test_kept_posterior_is_the_two_posterior_body(NS, kind):
    kp = problem(NS, kind)
    assert set(kp["flag"]) == {0, 1} and kp["live"].all() and (kp["n"] > 2).all() and kp["n"].max() == NS and kp["n"].min() < NS
    x, prev, S = (dev(a) for a in T.poisoned(kp))
    pq, n, quant, flag, neg, active = T.device_args(kp)
    assert active is None
    with torch.no_grad():
        kept = _lib.relate_keep_fwd(x, prev, S, pq, n, quant, flag, neg, active)
        prev_p = prev[pq.long()]
        is_s = flag.bool()[:, None]
        ident = torch.arange(kp["P"], dtype=torch.int32, device=x.device)
        want = dev(np.where(kp["flag"] > 0, _lib.WANT_SUBJECT, _lib.WANT_OBJECT).astype(np.uint8))
        post_s, post_o = _lib.relate_fwd(torch.where(is_s, x, prev_p).contiguous(), torch.where(is_s, prev_p, x).contiguous(), S, ident, n[pq.long()],
                                         quant, quant, neg, None, want=want)
        both = torch.where(is_s, post_s, post_o)
    kept, both = kept.cpu().numpy(), both.cpu().numpy()
    assert np.isfinite(kept).all()
    for p in range(kp["P"]):
        m = kp["n"][kp["pq"][p]]
        assert not kept[p, m:].view(np.uint32).any() and not both[p, m:].view(np.uint32).any(), (p, "padding is not +0")
        assert kept[p, :m].any(), (p, "the posterior is all zero: nothing was computed")
    diff = kept.view(np.uint32) != both.view(np.uint32)
    assert not diff.any(), "%d cells differ in bits, first at %s" % (int(diff.sum()), tuple(np.argwhere(diff)[0]))
