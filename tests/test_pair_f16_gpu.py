"""The opt-in one-product mode of the fused pair kernel (`pair_math: f16`, csrc/dfol_pair_h2.hip with one piece per operand:
dfol_pair_ll_h1_f32 on the dfol_pair_pack_w2_f16 image): accuracy against float64 with a bound derived from fp16's rounding, independence
of the tiles per workgroup, the packed image, the saturation report, the interpreter's two routes, and a train step that ignores the key.

Kernel-level tests run the full model widths (256 -> 300, 333 concepts) on tiny scenes, shape R: object counts [1, 2, 16, 17, 23, 5, 33] -
images without pairs, partial last tiles, five tiles at the 33-object image (no multiple of the tiles per workgroup), workgroups that
straddle images."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

HID1, HID2, C = 256, 300, 333
R = [1, 2, 16, 17, 23, 5, 33]
EPS = 2.0 ** -11                                    # fp16: 11 significand bits, relative rounding error at most 2^-11 (round to nearest)


@pytest.fixture(scope="module")
def L():
    from dfol_vqa_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return _lib


@pytest.fixture(scope="module")
def weights(L):
    """The weight scales of tests/test_pair_multitile_gpu.py; both packed images of the same W2."""
    g = torch.Generator().manual_seed(7)
    dev = torch.device("cuda")
    wg = torch.randn(HID1, 4, generator=g) * 0.3
    w2 = torch.zeros(320, HID1)
    w2[:HID2] = torch.randn(HID2, HID1, generator=g) / 16
    b2 = torch.randn(HID2, generator=g)
    emb = torch.randn(C, HID2, generator=g) / 17
    be = torch.randn(C, generator=g)
    host = dict(wg=wg.numpy().astype(np.float64), w2=w2[:HID2].numpy().astype(np.float64), b2=b2.numpy().astype(np.float64),
                emb=emb.numpy().astype(np.float64), be=be.numpy().astype(np.float64))
    w2d = w2.to(dev)
    return dict(wg=wg.to(dev), w2=w2d, h1=L.pair_pack_w2_h1(w2d, HID2), h2=L.pair_pack_w2_h2(w2d, HID2), b2=b2.to(dev), emb=emb.to(dev),
                be=be.to(dev), host=host)


def _scene(n_list, K, seed, orient=False):
    rng = np.random.RandomState(seed)
    dev = torch.device("cuda")
    Q, O = len(n_list), int(sum(n_list))
    off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int32)
    uv = rng.randn(O, 2 * HID1).astype(np.float32) * 0.5
    pos = rng.rand(O, 4).astype(np.float32) * 0.5 + 0.05
    req_col = rng.randint(0, C, size=(K, Q)).astype(np.int32)
    if K > 1:
        req_col[rng.rand(K, Q) < 0.2] = -1
        req_col[0, 4], req_col[1, 6] = -1, -1                   # (some -1 requests whatever the seed; the largest image keeps two columns)
        req_col[0, 6] = abs(req_col[0, 6])
    req_tile = np.arange(K * Q, dtype=np.int32).reshape(K, Q)
    ori = rng.randint(0, 2, size=(K, Q)).astype(np.uint8) if orient else None
    t = lambda a: torch.from_numpy(a).to(dev)
    return dict(uv=t(uv), pos=t(pos), n_obj=t(np.asarray(n_list, np.int32)), off=t(off), max_n=int(max(n_list)), req_col=t(req_col),
                req_tile=t(req_tile), req_orient=None if ori is None else t(ori), K=K, Q=Q,
                host=dict(uv=uv, pos=pos, off=off, n=list(n_list), req_col=req_col, ori=ori))


def _run(L, w, s, kernel="h1", tiles_per_wg=None, bf16=False):
    NS = (s["max_n"] + 7) // 8 * 8
    tiles = torch.full((s["K"] * s["Q"], NS, NS), -30.0, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
    old = os.environ.get("DFOL_PAIR_TILES")
    if tiles_per_wg is not None:
        os.environ["DFOL_PAIR_TILES"] = str(tiles_per_wg)      # (read by the launcher at every call)
    try:
        fn, img = (L.pair_ll_h1, w["h1"]) if kernel == "h1" else (L.pair_ll_h2, w["h2"])
        fn(s["uv"], HID1, s["pos"], w["wg"], img, w["b2"], HID2, w["emb"], w["be"], s["n_obj"], s["off"], s["max_n"], s["req_col"],
           s["req_tile"], s["req_orient"], tiles)
        torch.cuda.synchronize()
    finally:
        if tiles_per_wg is not None:
            if old is None:
                os.environ.pop("DFOL_PAIR_TILES", None)
            else:
                os.environ["DFOL_PAIR_TILES"] = old
    return tiles


def reference64(w, s):
    """The pair formula in float64 from the unrounded inputs (classifier_oracle.py:145-156 over the pair features of
    batch_gqa_boxfeatures_pipeline.py:263-279): per written cell its position in the tiles, ll = LogSigmoid(x), and the quantities of the
    error model - the activations a [pairs, HID1], and per cell g_j = E_cj h_j (1 - h_j) = d x / d pre2_j and the LogSigmoid's slope."""
    h, hs = w["host"], s["host"]
    NS = (s["max_n"] + 7) // 8 * 8
    cells, ll, G, slope, pair_of, A = [], [], [], [], [], []
    for q, n in enumerate(hs["n"]):
        f = int(hs["off"][q])
        for sub in range(n):
            for ob in range(n):
                if sub == ob:
                    continue
                x1, y1, w1, h1 = hs["pos"][f + sub].astype(np.float64)
                x2, y2, w2_, h2 = hs["pos"][f + ob].astype(np.float64)
                dx, dy = x1 + w1 / 2 - x2 - w2_ / 2, y1 + h1 / 2 - y2 - h2 / 2
                dist = np.sqrt(dx * dx + dy * dy)
                geo = np.array([dist, np.arcsin(dy / max(dist, 1e-10)), np.sign(x2 - x1), np.sign(y2 - y1)])
                z = hs["uv"][f + sub, :HID1].astype(np.float64) + hs["uv"][f + ob, HID1:].astype(np.float64) + h["wg"] @ geo
                a = np.where(z > 0, z, np.expm1(z))
                hid = 1.0 / (1.0 + np.exp(-(h["w2"] @ a + h["b2"])))
                wrote = False
                for k in range(s["K"]):
                    c = int(hs["req_col"][k, q])
                    if c < 0:
                        continue
                    x = hid @ h["emb"][c] + h["be"][c]
                    flip = hs["ori"] is not None and hs["ori"][k, q]
                    cells.append((k * s["Q"] + q, ob, sub) if flip else (k * s["Q"] + q, sub, ob))
                    ll.append(min(x, 0.0) - np.log1p(np.exp(-abs(x))))
                    G.append(h["emb"][c] * hid * (1.0 - hid))
                    slope.append(1.0 / (1.0 + np.exp(x)))           # d LogSigmoid / dx = Sigmoid(-x), in (0, 1)
                    pair_of.append(len(A))
                    wrote = True
                if wrote:
                    A.append(a)
    return dict(cells=np.asarray(cells), ll=np.asarray(ll), G=np.asarray(G), slope=np.asarray(slope), pair_of=np.asarray(pair_of),
                A=np.asarray(A), NS=NS)


def error_model(w, ref):
    """One fp16 rounding per operand, relative error uniform within half an ulp at most: variance <= (2^-11)^2 / 3 of the operand's square.

    sigma (per cell, of the LOGIT): sigma^2 = sum_j (E_cj h_j (1 - h_j))^2 sum_k (a_k W_jk)^2 x 2 (2^-11)^2 / 3 - every product a_k W_jk
    carries the two roundings, taken as independent across the 256 x 300 products of a cell.

    sigma_mean: the standard deviation of the MEAN error over the cells times sqrt(cells), under the same rounding model but with the one
    thing the per-cell formula may ignore and a mean over cells may not: a rounded VALUE is shared by all the products it enters.  The
    rounding of W_jk is the same number in every cell, that of a pair's activation a_k is shared by the K cells of the pair and the 300
    columns j, so the errors of different cells are correlated and the mean's variance is NOT mean(sigma^2) / cells.  With the mean's
    sensitivities  c_pk = sum_{cells of pair p} s_c sum_j g_cj W_jk  (to the relative rounding of a_pk; s_c = the LogSigmoid's slope, the
    mean is taken over ll) and  d_jk = sum_cells s_c g_cj a_pk  (to that of W_jk):
        var(sum of errors) = (2^-11)^2 / 3 x (sum_pk (c_pk a_pk)^2 + sum_jk (d_jk W_jk)^2),  sigma_mean = sqrt(var / cells).
    For independent cells this is the root mean square of sigma (times the slopes).

    How far the two readings are apart on this file's cases (float64, host side only; the test prints both): K1, 2096 cells - rms sigma
    5.80e-5 (times the slopes 2.16e-5), sigma_mean 1.02e-4: the mean's bound 6 sigma_mean / sqrt(cells) is 1.34e-5 where the naive
    6 rms sigma / sqrt(cells) would be 7.6e-6 (1.8 x wider; 4.7 x the independent-cells value with the slopes).  K3, 4726 cells - rms sigma
    5.87e-5 (3.37e-5), sigma_mean 1.51e-4: 1.32e-5 against 5.1e-6 (2.6 x; 4.5 x).  The shared roundings cost the mean test that factor of
    its power against a bias; a bias of one sigma per cell (5.8e-5) is still 4 x beyond the bound."""
    W, A, G = w["host"]["w2"], ref["A"], ref["G"]
    a_of_cell = A[ref["pair_of"]]
    sigma = np.sqrt((G ** 2 * ((a_of_cell ** 2) @ (W ** 2).T)).sum(1) * 2.0 * EPS ** 2 / 3.0)
    Gs = G * ref["slope"][:, None]
    Gp = np.zeros((A.shape[0], HID2))
    np.add.at(Gp, ref["pair_of"], Gs)
    c = Gp @ W                                                   # [pairs, HID1]
    d = Gs.T @ a_of_cell                                         # [HID2, HID1]
    var_sum = EPS ** 2 / 3.0 * (((c * A) ** 2).sum() + ((d * W) ** 2).sum())
    return sigma, np.sqrt(var_sum / len(sigma))


@pytest.fixture(scope="module")
def cases(L, weights):
    """The accuracy cases, their float64 references and error models: computed once."""
    out = {}
    for name, K, seed, orient in (("K1", 1, 11, False), ("K3", 3, 12, True)):
        s = _scene(R, K, seed, orient)
        ref = reference64(weights, s)
        out[name] = (s, ref) + error_model(weights, ref)
    return out


@pytest.mark.parametrize("name", ["K1", "K3"])
def test_accuracy_against_float64(L, weights, cases, name):
    """|ll_f16 - ll_64| <= 6 sigma + n32 in every written cell (sigma: error_model; n32: the largest error of the EXISTING f16x2 kernel
    against the same float64 values on the same inputs - that kernel's own rounding, the float32 epilogue and store - so the allowance
    comes from the parent's kernel), |mean error| <= 6 sigma_mean / sqrt(cells), at least one value differs from the f16x2 kernel's, and
    the cells nobody writes keep the fill."""
    s, ref, sigma, sigma_mean = cases[name]
    got = _run(L, weights, s, "h1").cpu().numpy().astype(np.float64)
    got2 = _run(L, weights, s, "h2").cpu().numpy().astype(np.float64)
    t, r, c = ref["cells"].T
    n_cells = len(t)
    assert n_cells >= 2000 and len(set(map(tuple, ref["cells"]))) == n_cells
    e1, e2 = got[t, r, c] - ref["ll"], got2[t, r, c] - ref["ll"]
    n32 = np.abs(e2).max()
    ratio = (np.abs(e1) / (6 * sigma + n32)).max()
    print("pair f16 %s: cells %d  f16 max %.3e rms %.3e  f16x2 max (n32) %.3e rms %.3e  max |e| / (6 sigma + n32) %.3f  max |e| / 6 sigma %.3f  "
          "mean e %.3e  6 sigma_mean / sqrt(cells) %.3e  rms sigma %.3e" %
          (name, n_cells, np.abs(e1).max(), np.sqrt((e1 ** 2).mean()), n32, np.sqrt((e2 ** 2).mean()), ratio, (np.abs(e1) / (6 * sigma)).max(),
           e1.mean(), 6 * sigma_mean / np.sqrt(n_cells), np.sqrt((sigma ** 2).mean())))
    assert n32 < 1e-5, n32                                       # (the yardstick itself is sane)
    bad = np.abs(e1) > 6 * sigma + n32
    assert not bad.any(), "%d of %d cells beyond 6 sigma + n32, worst ratio %.2f" % (int(bad.sum()), n_cells, ratio)
    assert abs(e1.mean()) <= 6 * sigma_mean / np.sqrt(n_cells), (e1.mean(), sigma_mean / np.sqrt(n_cells))
    assert (got[t, r, c] != got2[t, r, c]).any(), "the one-product kernel returned the f16x2 kernel's bits: the lo pieces are still there"
    untouched = np.ones(got.shape, bool)
    untouched[t, r, c] = False
    assert (got[untouched] == -30.0).all() and untouched.sum() > n_cells


@pytest.mark.parametrize("bf16", [False, True])
def test_tiles_per_workgroup_change_no_bit(L, weights, bf16):
    s = _scene(R, 3, 21, orient=True)
    view = torch.int16 if bf16 else torch.int32
    ref = _run(L, weights, s, "h1", 1, bf16).view(view).cpu().numpy()
    none = _run(L, weights, {**s, "req_col": torch.full_like(s["req_col"], -1)}, "h1", 1, bf16).view(view).cpu().numpy()
    assert (ref != none).any(), "the launch wrote nothing"
    for t in (3, 4):
        got = _run(L, weights, s, "h1", t, bf16).view(view).cpu().numpy()
        assert np.array_equal(ref, got), "T = %d: %d of %d values differ from T = 1" % (t, int((ref != got).sum()), ref.size)
    if bf16:                                                     # the bf16 tiles are the fp32 tiles rounded to nearest even
        f32 = _run(L, weights, s, "h1", 1, False)
        assert np.array_equal(f32.to(torch.bfloat16).view(torch.int16).cpu().numpy(), ref)


def test_packed_image(L, weights):
    """The one-piece image is the hi-piece half of the two-piece image, chunk by chunk and bit for bit, followed by the same 640-word tail."""
    h1, h2 = weights["h1"].view(torch.int16).cpu().numpy(), weights["h2"].view(torch.int16).cpu().numpy()
    lib = L.load()
    assert lib.dfol_pair_w2_f16_bytes(HID1) == h1.size * 2 == (HID1 // 32) * 320 * 4 * 16 + 640 * 4
    assert lib.dfol_pair_w2_f16x2_bytes(HID1) == h2.size * 2
    nchunk, half = HID1 // 32, 320 * 4 * 8                       # fp16 values of one piece of one chunk
    c1, c2 = h1[:nchunk * half].reshape(nchunk, half), h2[:nchunk * 2 * half].reshape(nchunk, 2, half)
    assert np.array_equal(c1, c2[:, 0])
    assert c2[:, 1].any()                                        # (the lo pieces exist in the two-piece image and are not copied)
    assert np.array_equal(h1[nchunk * half:], h2[nchunk * 2 * half:]) and h1[nchunk * half:].size == 640 * 2
    # the weight without its padding rows gives the same image (rows >= HID2 are zero in it either way)
    assert torch.equal(L.pair_pack_w2_h1(weights["w2"][:HID2].contiguous()), weights["h1"])


@pytest.mark.parametrize("hid1", [256, 96])
def test_saturation_is_still_reported(L, hid1):
    """The inputs of test_kernels_gpu.test_pair_h2_saturation_flag through the new entry point: DFOL_RANGE_PAIR_SATURATED exactly when a
    first-layer sum may pass the saturation point (or is NaN), clear on ordinary inputs, on large negative sums, without a status word."""
    rng = np.random.RandomState(5)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    hid2, K, n_list = 300, 1, [9, 1, 12, 37]
    Q, O, NS, Cn = len(n_list), sum(n_list), 40, 8
    off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int32)
    pos = rng.uniform(0.05, 0.9, (O, 4)).astype(np.float32)
    wg = rng.uniform(-0.5, 0.5, (hid1, 4)).astype(np.float32)
    w2 = np.zeros((320, hid1), np.float32)
    w2[:hid2] = rng.normal(size=(hid2, hid1)).astype(np.float32) / np.sqrt(hid1)
    packed = L.pair_pack_w2_h1(dev(w2), hid2)
    b2 = dev(rng.normal(size=hid2).astype(np.float32))
    E, be = dev((rng.normal(size=(Cn, hid2)) / np.sqrt(hid2)).astype(np.float32)), dev(rng.normal(size=Cn).astype(np.float32))
    req_col, req_tile = dev(rng.randint(0, Cn, (K, Q)).astype(np.int32)), dev(np.arange(K * Q, dtype=np.int32).reshape(K, Q))
    word = torch.zeros(1, dtype=torch.int32, device="cuda")

    def flagged(uv, with_word=True):
        word.zero_()
        L.load().dfol_set_range_status(word.data_ptr() if with_word else None)
        try:
            t = torch.full((K * Q, NS, NS), -30.0, device="cuda")
            L.pair_ll_h1(dev(uv), hid1, dev(pos), dev(wg), packed, b2, hid2, E, be, dev(np.array(n_list, np.int32)), dev(off), max(n_list),
                         req_col, req_tile, None, t, uv_prescaled=True)      # (the values below are in the kernel's units of 1 / ln 2)
        finally:
            L.load().dfol_set_range_status(None)
        return int(word.item())

    base = rng.uniform(-1, 1, (O, 2 * hid1)).astype(np.float32)
    assert flagged(base) == 0
    neg = base.copy(); neg[:, 3] = -5.0e5
    assert flagged(neg) == 0
    lone = base.copy(); lone[int(off[1])] = 9.0e4
    assert flagged(lone) == 0
    for k in (0, hid1 - 1, hid1 // 2 + 1):
        hot = base.copy()
        hot[int(off[3]) + 5, k] = 4.0e4
        hot[int(off[3]) + 20, hid1 + k] = 3.0e4
        assert flagged(hot) == L.RANGE_PAIR_SATURATED, k
        assert flagged(hot, with_word=False) == 0
        under = hot.copy(); under[int(off[3]) + 20, hid1 + k] = 1.0e4
        assert flagged(under) == 0, k
        apart = base.copy()
        apart[int(off[3]) + 5, k] = 4.0e4
        apart[int(off[2]) + 2, hid1 + k] = 3.0e4
        assert flagged(apart) == 0, k
    nan = base.copy(); nan[int(off[2]) + 7, hid1 + 9] = np.nan
    assert flagged(nan) == L.RANGE_PAIR_SATURATED


# ---- through the interpreter ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """Full-size models from configs with `pair_math: f16` (fp32 and bf16 relation tiles) and without the key, the same seeded weights."""
    from dfol_vqa_amd import experiment
    from dfol_vqa_amd import synthetic as syn
    from test_interpreter_gpu import DEV
    paths, names = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("pair_f16")))
    ont = experiment.build_ontology(syn.reference_config(paths))
    out = {}
    for key, over in (("f16", dict(pair_math="f16")), ("f16_bf16tiles", dict(pair_math="f16", relation_tile_dtype="bf16")), ("default", {})):
        model = experiment.build_model(syn.reference_config(paths, **over), ont)
        syn.load_seeded_weights(model, 23)
        out[key] = model.to(DEV).eval()
    return out, ont, names, paths


def _questions(names, n_list):
    """select -> filter -> relate -> exist on ragged images (one of ONE object); the last question ends with a verify_rel instead (a
    ProgramBatch holds one terminal operator: it is collated on its own)."""
    from dfol_vqa_amd import synthetic as syn
    nouns, attrs, rels = names["nouns"][:8], names["attributes"][:6], names["relations"][:5]
    qs = []
    for i, n in enumerate(n_list):
        br, last = syn.three_hop_program(i, nouns, attrs, rels)
        if i == len(n_list) - 1:
            br, last = [[syn.op("select", nouns[1]), syn.op("filter", attrs[2])]], syn.op("verify_rel", rels[1], True, nouns[3])
        qs.append(syn.question(i, br, last, "yes" if i % 2 else "no", syn.feature_scene(4200 + i, n, 2048)))
    return qs


def _collate(ont, qs, shared=False):
    from test_interpreter_gpu import DEV, TableCollater
    groups = [[q for q in qs if q["program"]["last_op"]["operator"] == kind] for kind in ("exist", "verify_rel")]
    return [pb.to_cuda(DEV) for g in groups if g for pb in TableCollater(2 if len(g) > 2 else 1, ont, "X", share_scenes=shared).collate([dict(q) for q in g])]


def _both_routes(model, pbs_of, monkeypatch):
    from dfol_vqa_amd import _lib
    out = []
    for native in ("1", "0"):
        monkeypatch.setenv("DFOL_NATIVE", native)
        pbs = pbs_of()
        _lib.PATH_COUNTS.clear()
        with torch.no_grad():
            out.append(model(pbs, False))
        assert _lib.PATH_COUNTS.get("native_program", 0) == (len(pbs) if native == "1" else 0), dict(_lib.PATH_COUNTS)
    assert torch.equal(out[0]["log_probability"], out[1]["log_probability"])
    assert out[0]["answer"] == out[1]["answer"] and out[0]["answer_log_probability"] == out[1]["answer_log_probability"]
    return out[0]


@pytest.mark.parametrize("shared", [False, True])
def test_through_the_interpreter(models, shared, monkeypatch):
    """`pair_math: f16` from the config to the kernel: the Python loop and the native executor agree bit for bit and every batch runs on
    the executor; the tiles the forward produced are those of a direct pair_ll_h1 call on the same U | V (and not the f16x2 kernel's);
    the model without the key still answers with the f16x2 kernel's bits; `relation_tile_dtype: bf16` with the key runs on the executor."""
    from dfol_vqa_amd import _lib, ops
    by_key, ont, names, _ = models
    monkeypatch.delenv("DFOL_PAIR_MATH", raising=False)
    n_list = [3, 20, 1, 7, 12, 16, 9, 5] if not shared else [8, 16, 1, 8, 16, 1, 8, 16]      # (bf16 tiles need NS % 8 == 0: see below)
    qs = _questions(names, n_list)
    if shared:
        images = [qs[i]["scene"] for i in range(3)]
        for i, q in enumerate(qs):
            q["image_id"], q["scene"] = "img%d" % (i % 3), images[i % 3]

    def pbs_of():
        return _collate(ont, qs, shared)

    calls = []
    real_h1, real_h2 = ops.pair_ll_h1, ops.pair_ll_h2

    def spy_h1(*args, **kw):
        out = real_h1(*args, **kw)
        calls.append(("h1", args, kw, out.clone()))
        return out

    def spy_h2(*args, **kw):
        calls.append(("h2", args, kw, None))
        return real_h2(*args, **kw)

    monkeypatch.setattr(ops, "pair_ll_h1", spy_h1)
    monkeypatch.setattr(ops, "pair_ll_h2", spy_h2)
    res = _both_routes(by_key["f16"], pbs_of, monkeypatch)
    assert by_key["f16"]._oracle._pair_kind() == "f16x2"          # (outside a forward the key is not in force: the scope is the forward's)
    with _lib.pair_math_scope("f16"):
        assert by_key["f16"]._oracle._pair_kind() == "f16"
    assert calls and all(c[0] == "h1" for c in calls), [c[0] for c in calls]       # the Python loop's launches (the executor calls C directly)
    # The direct call takes nothing from the host layer but U | V and the requests: the image is packed here from the model's own W2, so
    # a forward that handed the kernel another image (or another kernel this image) would not reproduce.  The EXECUTOR's tiles are not
    # visible from here; they are covered by its final log-probabilities being the Python loop's bit for bit (_both_routes).
    lin2 = [m for m in by_key["f16"]._oracle._relation_network._network if isinstance(m, torch.nn.Linear)][1]
    fresh = _lib.pair_pack_w2_h1(lin2.weight.detach().contiguous(), lin2.weight.shape[0])
    differs = False
    for _, args, kw, produced in calls:
        uv, hid1, pos, wg, img, b2, hid2, ew, eb, n_obj, off, max_n, rc, rt, ro, tiles = args[:16]
        assert torch.equal(fresh.view(torch.int16), img.view(torch.int16))
        again = real_h1(uv, hid1, pos, wg, fresh, b2, hid2, ew, eb, n_obj, off, max_n, rc, rt, ro, torch.full_like(tiles, -30.0), **kw)
        assert torch.equal(again.view(torch.int32), produced.view(torch.int32))
        img2 = by_key["f16"]._oracle._pair_image("f16x2").image
        two = real_h2(uv, hid1, pos, wg, img2, b2, hid2, ew, eb, n_obj, off, max_n, rc, rt, ro, torch.full_like(tiles, -30.0), **kw)
        differs |= not torch.equal(two, produced)
        assert (two - produced).abs().max().item() < 1e-2
    assert differs
    # the same weights without the key: the default kernel, and (almost surely) other bits than the reduced mode's
    calls.clear()
    ref = _both_routes(by_key["default"], pbs_of, monkeypatch)
    assert calls and all(c[0] == "h2" for c in calls)
    assert (ref["log_probability"] - res["log_probability"]).abs().max().item() < 1e-2
    # bf16 relation tiles together with the key: on the executor, bit for bit the Python loop
    calls.clear()
    bf = _both_routes(by_key["f16_bf16tiles"], pbs_of, monkeypatch)
    assert calls and all(c[0] == "h1" for c in calls)
    if shared:                                                   # NS = 16: bf16 tiles are in use
        assert any(c[3].dtype == torch.bfloat16 for c in calls)
    assert (bf["log_probability"] - res["log_probability"]).abs().max().item() <= 5e-2


def test_training_ignores_the_key(models, monkeypatch):
    """One train_batch (4 questions x 6..9 objects, full widths, every weight trains): bit-identical loss, gradients and updated weights
    with `pair_math: f16` and without it - the pair branch of a train step stays on the f16x2 image and its fused forward."""
    from dfol_vqa_amd import _lib, experiment, training
    from dfol_vqa_amd import synthetic as syn
    from test_interpreter_gpu import DEV
    _, ont, names, paths = models
    monkeypatch.delenv("DFOL_PAIR_MATH", raising=False)
    qs = _questions(names, [6, 9, 7, 8])
    out = {}
    for key in ("default", "f16"):
        model = experiment.build_model(syn.reference_config(paths, **({"pair_math": "f16"} if key == "f16" else {})), ont)
        syn.load_seeded_weights(model, 23)
        model = model.to(DEV).train()
        assert getattr(model, "_pair_math", None) == (None if key == "default" else "f16")
        for prm in model.parameters():
            prm.requires_grad_(prm.dtype.is_floating_point and prm is not model._global_step)
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
        pbs = _collate(ont, qs)
        _lib.PATH_COUNTS.clear()
        loss, _ = training.train_batch(model, opt, pbs, clip_norm=0.65)
        counts = {k: v for k, v in _lib.PATH_COUNTS.items() if k.startswith("pair_") or k.startswith("fused_")}
        out[key] = (loss, {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None},
                    {k: p.detach().clone() for k, p in model.named_parameters()}, counts)
    (l0, g0, p0, c0), (l1, g1, p1, c1) = out["default"], out["f16"]
    assert c0 == c1 and c0.get("pair_forward_fused", 0) >= 1, (c0, c1)      # the same route: the fused forward on the f16x2 image
    assert l0 == l1 and np.isfinite(l0), (l0, l1)
    assert set(g0) == set(g1) and len(g0) >= 8
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


def test_both_images_stay_packed_inside_the_scope(models, monkeypatch):
    """Inside a `pair_math: f16` scope the train gate asks for the f16x2 image between requests for the f16 one: W2 is packed once per
    arithmetic, not once per switch, and clearing `_w2_cache` drops every entry."""
    from dfol_vqa_amd import _lib, ops
    oracle = models[0]["f16"]._oracle
    monkeypatch.delenv("DFOL_PAIR_MATH", raising=False)
    packs = []
    for name in ("pair_pack_w2_h1", "pair_pack_w2_h2"):             # (visual_oracle packs through `ops`)
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _name=name, **k: (packs.append(_name), _real(*a, **k))[1])
    oracle._w2_cache = None
    with _lib.pair_math_scope("f16"):
        first = oracle._pair_image()
        two = oracle._pair_image("f16x2")
        for _ in range(3):
            assert oracle._pair_image().image is first.image and oracle._pair_image("f16x2").image is two.image
    assert (first.kind, two.kind) == ("f16", "f16x2") and sorted(packs) == ["pair_pack_w2_h1", "pair_pack_w2_h2"], packs
    oracle._w2_cache = None
    assert oracle._pair_image().kind == "f16x2"
    assert [(math, img.kind) for math, img in oracle._w2_cache[1].items()] == [("f16x2", "f16x2")]      # exactly one entry: the f16x2 image


# ---- every form of the second layer through the one launch path -----------------------------------------------------------------------------
# kind -> (pair_math scope, DFOL_PAIR_PACKED, the _lib wrapper that launches it, the _lib wrapper that packs its image, U | V prescaled by log2 e);
# written out here, not read from _lib.PAIR_KINDS: the table is what is under test
FORMS = {"f16x2": ("f16x2", None, "pair_ll_h2", "pair_pack_w2_h2", True), "f16": ("f16", None, "pair_ll_h1", "pair_pack_w2_h1", True),
         "bf16x3": ("bf16x3", None, "pair_ll_split", "pair_pack_w2_split", False), "packed": ("f32", None, "pair_ll_packed", "pair_pack_w2", False),
         "plain": ("f32", "0", "pair_ll", None, False)}


def test_every_kind_launches_its_own_wrapper(models, monkeypatch):
    """One shared-scene batch of three images with 1, 2 and 9 objects (no pair; the smallest image with an ordered pair; 72 pairs, so a
    workgroup's 256 slots straddle images), two relation columns per image, in each of the five kinds in turn: the tiles _launch_pairs
    writes are bit for bit those of the kind's _lib wrapper called directly on an image packed here from the model's own W2; the
    executor's log-probabilities are the Python loop's bit for bit; the executor's model struct carries the header's code of the kind."""
    import re
    from dfol_vqa_amd import _lib, native_exec
    from dfol_vqa_amd import synthetic as syn
    from test_interpreter_gpu import DEV, TableCollater
    by_key, ont, names, _ = models
    model = by_key["default"]
    oracle = model._oracle
    monkeypatch.delenv("DFOL_PAIR_MATH", raising=False)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dfol_vqa.h")).read()
    codes = {name.lower(): int(value) for name, value in re.findall(r"#define\s+DFOL_PAIR_([A-Z0-9]+)\s+(\d+)", header)}
    assert set(codes) == set(FORMS)
    nouns, attrs, rels = names["nouns"][:4], names["attributes"][:3], names["relations"][:2]
    scenes = [syn.feature_scene(4300 + i, n, 2048) for i, n in enumerate((1, 2, 9))]
    qs = []
    for i in range(6):                                           # two questions per image, one relation each: K = 2 distinct requests per image
        br = [[syn.op("select", nouns[i % 4]), syn.op("filter", attrs[i % 3]), syn.op("relate", rels[i // 3], True, nouns[(i + 1) % 4])]]
        qs.append(dict(syn.question(i, br, syn.op("exist"), "yes" if i % 2 else "no", scenes[i % 3]), image_id="img%d" % (i % 3)))

    def pbs_of():
        return [pb.to_cuda(DEV) for pb in TableCollater(1, ont, "X", share_scenes=True).collate([dict(q) for q in qs])]

    launches = []
    real_launch = oracle._launch_pairs

    def spy(world, req_col, req_tile, tiles, req_orient=None):
        real_launch(world, req_col, req_tile, tiles, req_orient)
        launches.append((world, req_col, req_tile, req_orient, tiles.clone()))

    monkeypatch.setattr(oracle, "_launch_pairs", spy)
    lin1, lin2 = [m for m in oracle._relation_network._network if isinstance(m, torch.nn.Linear)]
    w1, w2 = lin1.weight.detach(), lin2.weight.detach()
    D = (w1.shape[1] - 4) // 2
    assert tuple(w2.shape) == (HID2, HID1)
    wg, b2 = w1[:, 2 * D:].contiguous(), lin2.bias.detach().contiguous()
    w2_padded = torch.zeros(320, HID1, device=w2.device)
    w2_padded[:HID2] = w2
    emb = oracle._embedding_network.linear

    def forget():                                                # (neither cache is keyed by DFOL_PAIR_PACKED)
        oracle._w2_cache = None
        model.__dict__.pop("_native_model", None)

    results = {}
    try:
        for kind, (math, packed_env, launch, pack, prescaled) in FORMS.items():
            if packed_env is not None:
                monkeypatch.setenv("DFOL_PAIR_PACKED", packed_env)
            forget()
            del launches[:]
            with _lib.pair_math_scope(math):
                results[kind] = _both_routes(model, pbs_of, monkeypatch)["log_probability"]
                assert oracle._pair_kind() == kind
                assert native_exec.native_model(model).struct.pair_kind == codes[kind], kind
            assert len(launches) == 1, (kind, len(launches))     # the Python loop's one launch (the executor calls C directly)
            world, rc, rt, ro, produced = launches[0]
            assert tuple(rc.shape) == (2, 3) and world._img_n_list == [1, 2, 9] and produced.dtype == torch.float32
            head = (world._uv, HID1, world._obj[:, D - 4:], wg)
            rest = (emb.weight, emb.bias, world._img_n_obj, world._obj_off, 9, rc, rt, ro, torch.full_like(produced, -30.0), -30.0)
            if pack is None:
                again = _lib.pair_ll(*head, w2_padded, b2, *rest, hid2=HID2)
            else:
                image = getattr(_lib, pack)(w2_padded, HID2)
                again = getattr(_lib, launch)(*head, image, b2, HID2, *rest, **({"uv_prescaled": True} if prescaled else {}))
            assert torch.equal(again.view(torch.int32), produced.view(torch.int32)), kind
            wrote = (produced != -30.0).flatten(1).sum(1).cpu().numpy()[rt.cpu().numpy()]          # [K, images]
            assert (wrote[:, 0] == 0).all() and (wrote[:, 1] == 2).all() and (wrote[:, 2] == 72).all(), (kind, wrote)
    finally:
        monkeypatch.delenv("DFOL_PAIR_PACKED", raising=False)
        forget()
    # the arithmetics are different kernels: the reduced mode and the default do not answer with the same bits, and all stay close
    assert not torch.equal(results["f16"], results["f16x2"])
    for kind, lp in results.items():
        assert (lp - results["packed"]).abs().max().item() < 1e-2, kind
