#!/usr/bin/env python3
"""Accuracy of the fused pair kernel's two arithmetic modes (f16x2: dfol_pair_ll_h2_f32, f16: dfol_pair_ll_h1_f32) against a float64
evaluation of the pair formula at the bench shape (256 images x N objects, one relation column per image, full widths), with the error
model of tests/test_pair_f16_gpu.py: per cell sigma^2 = sum_j (E_cj h_j (1 - h_j))^2 sum_k (a_k W_jk)^2 x 2 (2^-11)^2 / 3, and the
correlation-aware sigma_mean of the mean error.  The float64 side runs in torch on the GPU, one image at a time.  Runs on the GPU box.

    python tools/lab/pair_f16_accuracy.py [--objects 100] [--images 256]

Weight and input scales are those of the tests (randn / 16 W2, 0.5 randn U | V, positions in (0.05, 0.55))."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
HID1, HID2, C = 256, 300, 333
EPS = 2.0 ** -11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=100)
    ap.add_argument("--images", type=int, default=256)
    args = ap.parse_args()
    from dfol_vqa_amd import _lib as L
    L.load()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(7)
    wg = torch.randn(HID1, 4, generator=g) * 0.3
    w2 = torch.zeros(320, HID1)
    w2[:HID2] = torch.randn(HID2, HID1, generator=g) / 16
    b2 = torch.randn(HID2, generator=g)
    emb = torch.randn(C, HID2, generator=g) / 17
    be = torch.randn(C, generator=g)
    rng = np.random.RandomState(11)
    Q, n = args.images, args.objects
    O = Q * n
    uv = torch.from_numpy(rng.randn(O, 2 * HID1).astype(np.float32) * 0.5).to(dev)
    pos = torch.from_numpy(rng.rand(O, 4).astype(np.float32) * 0.5 + 0.05).to(dev)
    cols = rng.randint(0, C, size=(1, Q)).astype(np.int32)
    n_obj = torch.full((Q,), n, dtype=torch.int32, device=dev)
    off = torch.arange(Q + 1, dtype=torch.int32, device=dev) * n
    req_col, req_tile = torch.from_numpy(cols).to(dev), torch.arange(Q, dtype=torch.int32, device=dev).reshape(1, Q)
    NS = (n + 7) // 8 * 8
    w2d = w2.to(dev)
    got = {}
    for kind, fn, img in (("f16", L.pair_ll_h1, L.pair_pack_w2_h1(w2d, HID2)), ("f16x2", L.pair_ll_h2, L.pair_pack_w2_h2(w2d, HID2))):
        tiles = torch.full((Q, NS, NS), -30.0, device=dev)
        fn(uv, HID1, pos, wg.to(dev), img, b2.to(dev), HID2, emb.to(dev), be.to(dev), n_obj, off, n, req_col, req_tile, None, tiles)
        torch.cuda.synchronize()
        got[kind] = tiles.double()

    d = lambda t: t.to(dev).double()
    Wg, W, B2, E, BE = d(wg), d(w2[:HID2]), d(b2), d(emb), d(be)
    ii, jj = torch.nonzero(~torch.eye(n, dtype=torch.bool, device=dev), as_tuple=True)          # subject, object
    acc = {k: dict(max=0.0, sq=0.0, sum=0.0, r6=0.0, e=[]) for k in got}
    sig_sq, var_c, cells = 0.0, 0.0, 0
    dmat = torch.zeros(HID2, HID1, dtype=torch.float64, device=dev)
    sigmas = []
    for q in range(Q):
        p, u = pos[q * n:(q + 1) * n].double(), uv[q * n:(q + 1) * n].double()
        x1, y1, w1, h1 = (p[ii, k] for k in range(4))
        x2, y2, w2_, h2 = (p[jj, k] for k in range(4))
        dx, dy = x1 + w1 / 2 - x2 - w2_ / 2, y1 + h1 / 2 - y2 - h2 / 2
        dist = torch.sqrt(dx * dx + dy * dy)
        geo = torch.stack([dist, torch.asin(dy / dist.clamp(min=1e-10)), torch.sign(x2 - x1), torch.sign(y2 - y1)], 1)
        z = u[ii, :HID1] + u[jj, HID1:] + geo @ Wg.T
        a = torch.where(z > 0, z, torch.expm1(z))
        hid = torch.sigmoid(a @ W.T + B2)
        c = int(cols[0, q])
        x = hid @ E[c] + BE[c]
        ll = x.clamp(max=0) - torch.log1p(torch.exp(-x.abs()))
        G = E[c] * hid * (1 - hid)
        sigma = torch.sqrt((G ** 2 * ((a ** 2) @ (W ** 2).T)).sum(1) * 2.0 * EPS ** 2 / 3.0)
        Gs = G * torch.sigmoid(-x)[:, None]
        var_c += float((((Gs @ W) * a) ** 2).sum())
        dmat += Gs.T @ a
        sig_sq += float((sigma ** 2).sum())
        cells += len(x)
        sigmas.append(sigma)
        for k in got:
            e = got[k][q][ii, jj] - ll
            acc[k]["e"].append(e)
    sigma = torch.cat(sigmas)
    sigma_mean = np.sqrt(EPS ** 2 / 3.0 * (var_c + float(((dmat * W) ** 2).sum())) / cells)
    e2 = torch.cat(acc["f16x2"]["e"])
    n32 = float(e2.abs().max())
    out = {"objects": n, "images": Q, "cells": cells, "rms_sigma": float(np.sqrt(sig_sq / cells)), "sigma_mean": float(sigma_mean),
           "mean_bound_6_sigma_mean_over_sqrt_cells": float(6 * sigma_mean / np.sqrt(cells)), "n32": n32}
    for k in got:
        e = torch.cat(acc[k]["e"])
        out[k] = {"max": float(e.abs().max()), "rms": float(torch.sqrt((e ** 2).mean())), "mean": float(e.mean()),
                  "max_over_6sigma": float((e.abs() / (6 * sigma)).max()), "max_over_6sigma_plus_n32": float((e.abs() / (6 * sigma + n32)).max()),
                  "rms_over_rms_sigma": float(torch.sqrt((e ** 2).mean()) / np.sqrt(sig_sq / cells))}
    out["differing_values"] = int((got["f16"] != got["f16x2"]).sum())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
