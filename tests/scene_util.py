"""Float64 restatement of the scene-graph supervision, for the tests of ops.scene_bce (oracle/ is closed to additions).

What is restated, in torch CPU tensor ops and their autograd:
  * ClassifierOracle.compute_all_log_likelihood, classifier_oracle.py:139-143: LogSigmoid of the embedding layer over the attribute (relation)
    index rows, z = h E[cols]^T + b[cols];
  * the loss, trainer.py:235-256: binary_cross_entropy(exp(lp), target, weight = weight, reduction = 'sum') (its clamp of the logs at -100);
  * the metric, trainer.py:265-275: a = [lp > thr]; numerator sum w [(t + a) > 0] [t != a], denominator sum w [(t + a) > 0].
The same code in float32 is the yardstick of rounding noise (golden_util.check_gradient)."""

import numpy as np
import torch

F = torch.nn.functional


def restate(h, emb_w, emb_b, cols, target, weight, thr, dtype):
    """-> dict(loss, num, den, dh, dE [C, H], db [C] or None, lp, abs_terms) of numpy float64 arrays, computed in `dtype` on the CPU."""
    h, emb_w, target, weight = (torch.as_tensor(np.asarray(x)).to(dtype) for x in (h, emb_w, target, weight))
    idx = torch.as_tensor(np.asarray(cols)).to(torch.int64)
    h.requires_grad_(True)
    E = emb_w[idx].clone().requires_grad_(True)
    b = None if emb_b is None else torch.as_tensor(np.asarray(emb_b)).to(dtype)[idx].clone().requires_grad_(True)
    z = h @ E.t()
    if b is not None:
        z = z + b
    lp = F.logsigmoid(z)                                            # classifier_oracle.py:139-143
    p = lp.exp()
    loss = F.binary_cross_entropy(p, target, weight=weight, reduction="sum")        # trainer.py:235-256
    out = {"z": z, "lp": lp}
    if h.numel() and idx.numel():
        grads = torch.autograd.grad(loss, [h, E] + ([b] if b is not None else []))
    else:
        grads = [torch.zeros_like(h), torch.zeros_like(E)] + ([torch.zeros_like(b)] if b is not None else [])
    out["dh"], out["dE"] = grads[0], grads[1]
    out["db"] = grads[2] if b is not None else None
    with torch.no_grad():
        a = (lp > thr).to(dtype)                                    # trainer.py:265-275
        either = ((target + a) > 0).to(dtype)
        out["num"] = (weight * either * (target != a).to(dtype)).sum()
        out["den"] = (weight * either).sum()
        terms = F.binary_cross_entropy(p, target, weight=weight, reduction="none")
        out["abs_terms"] = terms.abs().sum()
    out["loss"] = loss
    return {k: (None if v is None else v.detach().to(torch.float64).numpy()) for k, v in out.items()}


def check_loss(got, r32, r64, what, K=8.0):
    """|got - r64| <= K own s with s = sum |terms| in float64 and own = max(2^-20, |r32 - r64| / s): check_gradient's rule for the scalar."""
    s = float(r64["abs_terms"]) + 1e-30
    own = max(2.0 ** -20, abs(float(r32["loss"]) - float(r64["loss"])) / s)
    err = abs(float(got) - float(r64["loss"]))
    print("%s: loss %.9g f64 %.9g  own %.3g  ratio %.3g" % (what, float(got), float(r64["loss"]), own, err / (own * s)))
    assert np.isfinite(float(got)), what
    assert err <= K * own * s, "%s: loss %.9g against %.9g, %.3g of the allowed %.3g" % (what, float(got), float(r64["loss"]), err, K * own * s)


def make_case(M, H, C, bias=True, targets="mixed", thr=0.5, seed=0, C_all=2335, zero_rows=(), zero_cols=(), z_max=19.0):
    """fp32 inputs as numpy arrays: h in (0, 1) (a Sigmoid output), emb_w [C_all, H] with logits spread over |z| <= z_max, cols a shuffled
    non-contiguous subset, weights multiples of 1/8 (sums of them are exact in fp32), no log-likelihood within 1e-4 of thr in float64."""
    for attempt in range(300):
        rng = np.random.RandomState(seed + 7919 * attempt)
        h = rng.uniform(0.02, 0.98, size=(M, H)).astype(np.float32)
        emb_w = (rng.normal(size=(C_all, H)) * 6.0 / np.sqrt(0.33 * H)).astype(np.float32)
        emb_b = rng.normal(size=C_all).astype(np.float32) if bias else None
        cols = rng.permutation(C_all)[:C].astype(np.int32)
        z = h.astype(np.float64) @ emb_w[cols].astype(np.float64).T + (emb_b[cols].astype(np.float64) if bias else 0.0)
        top = np.abs(z).max() if z.size else 0.0
        if top > z_max:
            emb_w = (emb_w * (z_max / top)).astype(np.float32)
            if bias:
                emb_b = (emb_b * (z_max / top)).astype(np.float32)
            z = h.astype(np.float64) @ emb_w[cols].astype(np.float64).T + (emb_b[cols].astype(np.float64) if bias else 0.0)
        if z.size and np.abs(np.minimum(z, 0.0) - np.log1p(np.exp(-np.abs(z))) - thr).min() < 1e-4 + 1e-9:
            continue                                                # a log-likelihood too near thr: redraw (the exact test follows below)
        if targets == "zeros":
            t = np.zeros((M, C), np.float32)
        elif targets == "ones":
            t = np.ones((M, C), np.float32)
        else:
            t = (rng.uniform(size=(M, C)) < 0.3).astype(np.float32)
        w = (rng.randint(0, 17, size=(M, C)) / 8.0).astype(np.float32)
        for r in zero_rows:
            w[r, :] = 0.0
        for c in zero_cols:
            w[:, c] = 0.0
        r64 = restate(h, emb_w, emb_b, cols, t, w, thr, torch.float64)
        if r64["z"].size == 0 or (np.abs(r64["lp"] - thr).min() >= 1e-4 and np.abs(r64["z"]).max() <= 20.0):
            return dict(h=h, emb_w=emb_w, emb_b=emb_b, cols=cols, target=t, weight=w, thr=thr), r64
    raise AssertionError("no tie-free case found")
