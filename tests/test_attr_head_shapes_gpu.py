"""The fused attribute head (csrc/dfol_pair_h2.hip: attr_head_h2_kernel, dfol_attr_head_h2_f32) off the one shape tests/test_attr_head_gpu.py
runs it at (256 -> 300): all four compiled instantiations (NB16 = 17 .. 20) at their lower edges and full, one to eight W2 chunks, 0 to 15
padding columns, every staging depth (SR = 28, 26, 24, 23), more than 256 images, four request windows, batches of 1 / 128 / 129 objects,
images without objects, strided inputs, no embedding bias, another default, guarded outputs and inputs, the range flag, the refusals.

The rule is test_attr_head_gpu.py's: the head (L.attr_head_h2 over L.linear_act(x, w1, b1, ACT_NONE)) and the route it replaces (two
L.linear_act layers, L.attr_ll) are both compared with the float64 value of the same fp32 inputs (oracle/dfol_oracle.py's formulas).
  * owned cells whose float64 value is >= -5:   |head - f64| <= 2 max|present - f64| + 1e-6
  * ALL owned cells (below -5 LogSigmoid is the identity to rounding, so the head has to follow the logit as well as the present route
    does):                                      |head - f64| <= 2 max|present - f64| + 1e-6 max(1, |f64|)
  * cells nobody owns (columns >= n, no-op tokens, requests on images without objects) hold default_ll, bit for bit.
Every case also asserts its own worth (an owned cell exists, at least 90 % of the owned cells are >= -5), that the status word stays clean
for inputs in range, and that the first-layer rows and embedding rows may be followed by NaN: pre1 is always rows [0, O) of a buffer one
row longer, the embedding table rows [0, C) of one a row longer (slots past the last object repeat it, they do not read on).

Where the present route's second layer is the plain fp32 kernel (HID1 HID2 < 65536: every shape below but 256 -> 300 / 304 / 320) it has
fewer and exacter accumulation steps to err in than the full-size network, while the head's two-piece fp16 operands keep their error per
term.  The factor 2 holds all the same: NO shape needed the operand-model term of DESIGN 3.4, and none is in the bounds.

Largest observed max|head - f64| / max|present - f64| (cells >= -5) per (HID1, HID2) over all scenes of 100 cells or more, MI355X:
  ( 32, 257)  1.32      ( 64, 272)  1.18      ( 96, 273)  1.28      (160, 288)  1.08      (224, 289)  1.31
  (256, 304)  1.41      (128, 305)  1.46      (256, 320)  1.27      (256, 300)  1.37 (many small images, its one scene here)
with both errors between 1.2e-7 and 4.9e-7.  The one-object batch has three owned cells: 1.7e-8 against 7.6e-8 at (32, 257), 7.4e-8 against
1.8e-7 at (256, 320) - ratios 4.55 and 2.47 that the rule's absolute 1e-6 carries, as it is there to do.
Every case prints its figures (pytest -s)."""

import contextlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import dfol_oracle as orc  # noqa: E402
from test_attr_head_gpu import _smoke_model  # noqa: E402

pytestmark = pytest.mark.gpu

D, C = 36, 97
#          HID1 HID2    chunks, instantiation, padding columns, staging depth
SHAPES = [(32, 257),    # 1, <17>, 15, SR 28
          (64, 272),    # 2, <17>,  0
          (96, 273),    # 3, <18>, 15, SR 26
          (160, 288),   # 5, <18>,  0
          (224, 289),   # 7, <19>, 15, SR 24
          (256, 304),   # 8, <19>,  0
          (128, 305),   # 4, <20>, 15, SR 23
          (256, 320)]   # 8, <20>,  0: the packed image's whole 320 rows
FULL_SIZE = (256, 300)  # test_attr_head_gpu.py's, for the scene it has not seen either
RAGGED = [1, 2, 37, 100, 1, 1, 2, 100, 37, 1, 2, 2, 100, 37, 37, 1, 100, 2, 1, 37]
GUARD = 8                                                    # NaN rows in front of and behind a guarded output

RATIOS = {}


def _sr(hid2):
    """Embedding rows the kernel's 8192-float staging area holds beside the bias and the multiplier row."""
    return 8192 // ((hid2 + 15) // 16 * 16) - 2


def _host_weights(hid1, hid2):
    """fp32 weights of order one at every width: pre-activations ~ N(0, 1), logits ~ N(-1, 1.2)."""
    g = torch.Generator().manual_seed(1000 * hid1 + hid2)
    w1 = torch.randn(hid1, D, generator=g) / np.sqrt(D)
    b1 = torch.randn(hid1, generator=g) * 0.1
    w2 = torch.randn(hid2, hid1, generator=g) / np.sqrt(hid1)
    b2 = torch.randn(hid2, generator=g) * 0.5
    emb = torch.randn(C, hid2, generator=g) / 17
    be = torch.randn(C, generator=g) - 1.0
    return w1, b1, w2, b2, emb, be


def _requests(n_list, per_image, seed, noop=0.0, repeat=False, sort=False):
    """test_attr_head_gpu.py's: per_image predicates for every image, the images once per token list (NOT sorted by image) unless sort."""
    rng = np.random.RandomState(seed)
    pq, col = [], []
    for k in range(per_image):
        for q in range(len(n_list)):
            pq.append(q)
            col.append(-1 if rng.rand() < noop else (7 if repeat and k % 2 == 0 else int(rng.randint(0, C))))
    pq, col = np.asarray(pq, np.int32), np.asarray(col, np.int32)
    if sort:
        order = np.argsort(pq, kind="stable")
        pq, col = pq[order], col[order]
    return pq, col


def _reference(hw, x, n_list, pq, col, NS, edit=None, bias=True):
    """-> float64 blocks [P, NS] with NaN in the cells no object owns.  Host only."""
    w1, b1, w2, b2, emb, be = (t.numpy().astype(np.float64) for t in hw)
    z1 = orc._linear(x.astype(np.float64), w1, b1)
    if edit is not None:
        z1[edit[0], edit[1]] = edit[2]
    a = orc._elu(z1)
    h = orc._sigmoid(orc._linear(a, w2, b2))
    off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int64)
    ref = np.full((len(pq), NS), np.nan)
    for p in range(len(pq)):
        n = n_list[pq[p]]
        if col[p] >= 0 and n > 0:
            rows = slice(off[pq[p]], off[pq[p]] + n)
            ref[p, :n] = orc._log_sigmoid(h[rows] @ emb[col[p]] + (be[col[p]] if bias else 0.0))
    return ref


class _Case(object):
    pass


@pytest.fixture(scope="module")
def L():
    from dfol_vqa_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return _lib


@pytest.fixture(scope="module")
def bank(L):
    """shape -> (host weights, the same on the device + the packed second layer), made once per shape."""
    made = {}

    def get(shape):
        if shape not in made:
            hw = _host_weights(*shape)
            dw = tuple(t.cuda() for t in hw)
            made[shape] = (hw, dw + (L.pair_pack_w2_h2(dw[2], shape[1]),))
        return made[shape]
    return get


@contextlib.contextmanager
def _range_word(L):
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = L.load()
    try:
        lib.dfol_set_range_status(word.data_ptr())
        yield word
    finally:
        lib.dfol_set_range_status(None)


def _launch(L, c, guard=False):
    """The head on the case's device tensors -> (blocks [P, NS] as numpy, the status word).  guard: through the C entry point into rows
    [GUARD, GUARD + P) of a NaN-filled buffer, whose other rows must stay NaN and whose own rows must all be written."""
    P = c.pq_d.numel()
    with _range_word(L) as word:
        if guard:
            buf = torch.full((P + 2 * GUARD, c.NS), float("nan"), device="cuda")
            L.call("dfol_attr_head_h2_f32", c.pre1.data_ptr(), c.pre1.stride(0), c.pre1.shape[1], c.w2h.data_ptr(), c.b2.data_ptr(), c.shape[1],
                   c.emb.data_ptr(), c.emb.stride(0), None if c.be is None else c.be.data_ptr(), c.off_d.data_ptr(), c.off_d.numel() - 1,
                   c.pre1.shape[0], c.pq_d.data_ptr(), c.col_d.data_ptr(), P, c.NS, c.default, buf[GUARD:].data_ptr(), L._stream())
            torch.cuda.synchronize()
            assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + P:]).all(), "a write outside ll[P, NS]"
            new = buf[GUARD:GUARD + P]
            assert not torch.isnan(new).any(), "a cell was not written (or the kernel produced a NaN)"
        else:
            new = L.attr_head_h2(c.pre1, c.w2h, c.b2, c.shape[1], c.emb, c.be, c.off_d, c.pq_d, c.col_d, c.NS, c.default)
        flag = int(word.item())
    return new.cpu().numpy(), flag


def _run(L, bank, shape, n_list, pq, col, seed, guard=False, default=-30.0, pad1=0, pade=0, bias=True, edit=None):
    """Both routes and float64 for one scene.  pre1 = rows [0, O), columns [0, HID1) of a NaN-filled [O + 1, HID1 + pad1] buffer, the
    embedding table rows [0, C), columns [0, HID2) of a NaN-filled [C + 1, HID2 + pade] one.  edit = (row, k, value) sets one first-layer
    pre-activation, for every route."""
    hid1, hid2 = shape
    hw, (w1, b1, w2, b2, emb, be, w2h) = bank(shape)
    rng = np.random.RandomState(seed)
    c = _Case()
    c.shape, c.n_list, c.pq, c.col, c.default = shape, list(n_list), pq, col, default
    O = int(sum(n_list))
    c.NS = max(4, (max(n_list) + 3) // 4 * 4)
    x = rng.randn(O, D).astype(np.float32)
    c.ref = _reference(hw, x, n_list, pq, col, c.NS, edit, bias)
    xd = torch.from_numpy(x).cuda()
    off = np.concatenate([[0], np.cumsum(n_list)]).astype(np.int32)
    c.off_d, c.pq_d, c.col_d = (torch.from_numpy(a).cuda() for a in (off, pq, col))
    pbuf = torch.full((O + 1, hid1 + pad1), float("nan"), device="cuda")
    c.pre1 = pbuf[:O, :hid1]
    c.pre1.copy_(L.linear_act(xd, w1, b1, L.ACT_NONE))
    ebuf = torch.full((C + 1, hid2 + pade), float("nan"), device="cuda")
    c.emb = ebuf[:C, :hid2]
    c.emb.copy_(emb)
    c.be, c.b2, c.w2h = (be if bias else None), b2, w2h
    h1 = L.linear_act(xd, w1, b1, L.ACT_ELU)
    if edit is not None:
        c.pre1[edit[0], edit[1]] = edit[2]
        h1[edit[0], edit[1]] = edit[2] if edit[2] > 0 else float(np.expm1(edit[2]))
    hidden = L.linear_act(h1, w2, b2, L.ACT_SIGMOID)
    c.old = L.attr_ll(hidden, c.emb, c.be, c.off_d, c.pq_d, c.col_d, c.NS, default).cpu().numpy()
    c.new, c.flag = _launch(L, c, guard)
    return c


def _check(name, c):
    old, new, ref = c.old, c.new, c.ref
    owned = ~np.isnan(ref)
    assert owned.any(), "no requested cell"
    # cells no object owns: the default, bit for bit
    dflt = np.float32(c.default).view(np.int32)
    assert (new[~owned].view(np.int32) == dflt).all() and (old[~owned].view(np.int32) == dflt).all()
    assert np.isfinite(new[owned]).all()
    assert c.flag == 0, "inputs in range left %d in the status word" % c.flag
    hi = owned & (np.nan_to_num(ref, nan=-np.inf) >= -5.0)
    assert hi.sum() >= 0.9 * owned.sum(), "only %d of %d owned cells have a float64 value >= -5" % (hi.sum(), owned.sum())
    d_old, d_new = np.abs(old - ref), np.abs(new - ref)
    e_old, e_new = d_old[hi].max(), d_new[hi].max()
    e_old_all, e_new_all = d_old[owned].max(), d_new[owned].max()
    ratio = e_new / e_old
    RATIOS[c.shape] = max(RATIOS.get(c.shape, 0.0), ratio)
    print("attr_head %3d -> %3d %-30s cells %7d (>= -5: %7d)  max |err| vs float64: present %.3e  fused %.3e  ratio %5.2f (shape's largest %5.2f)"
          "   all cells: present %.3e  fused %.3e"
          % (c.shape[0], c.shape[1], name, int(owned.sum()), int(hi.sum()), e_old, e_new, ratio, RATIOS[c.shape], e_old_all, e_new_all))
    assert (d_new[hi] <= 2.0 * e_old + 1e-6).all(), (name, c.shape, e_old, e_new)
    assert (d_new[owned] <= 2.0 * e_old_all + 1e-6 * np.maximum(1.0, np.abs(ref[owned]))).all(), (name, c.shape, e_old_all, e_new_all)


def _same_request_same_bits(c):
    """Which entries are staged depends on the order of an atomicAdd: every repeat of one (image, column) request holds the same bits."""
    first, repeats = {}, 0
    for p in range(len(c.pq)):
        key = (int(c.pq[p]), int(c.col[p]))
        if key in first:
            repeats += 1
            assert np.array_equal(c.new[first[key]].view(np.int32), c.new[p].view(np.int32)), key
        else:
            first[key] = p
    return repeats


@pytest.mark.parametrize("shape", SHAPES)
def test_ragged_images(L, bank, shape):
    # images of 1, 2, 37 and 100 objects: tiles over many images, images that start mid-tile, a last partial tile (O = 598: five workgroups)
    pq, col = _requests(RAGGED, 2, seed=3)
    _check("ragged 1/2/37/100", _run(L, bank, shape, RAGGED, pq, col, seed=4))
    pq, col = _requests(RAGGED, 2, seed=5, sort=True)
    _check("ragged, sorted requests", _run(L, bank, shape, RAGGED, pq, col, seed=4))


@pytest.mark.parametrize("shape", SHAPES)
def test_more_requests_than_the_staging_area(L, bank, shape):
    # SR + 6 predicates on every image: the first SR entries of a tile are staged, the others read their embedding row from global memory
    n_list = [100, 28, 100]
    pq, col = _requests(n_list, _sr(shape[1]) + 6, seed=8, repeat=True)
    c = _run(L, bank, shape, n_list, pq, col, seed=9)
    _check("%d predicates per image" % (_sr(shape[1]) + 6), c)
    assert _same_request_same_bits(c) >= 3 * (_sr(shape[1]) // 2)


@pytest.mark.parametrize("shape", [(64, 272), (256, 320), FULL_SIZE])
def test_many_small_images(L, bank, shape):
    # 600 images of 1 - 3 objects (the first 200 of one: 128 images in the first tile), three predicates each: the image-count loop makes
    # three trips (Q > 257), P = 1800 is four request windows, the first tile has 128 entries in each of the first three
    n_list = [1] * 200 + [int(n) for n in np.random.RandomState(20).randint(1, 4, 400)]
    pq, col = _requests(n_list, 3, seed=21)
    _check("600 images of 1-3, 3 / image", _run(L, bank, shape, n_list, pq, col, seed=22, guard=True))


@pytest.mark.parametrize("n_list", [[1], [128], [100, 29], [127, 1, 1]], ids=lambda n: "-".join(map(str, n)))
@pytest.mark.parametrize("shape", [(32, 257), (256, 320)])
def test_batch_edges(L, bank, shape, n_list):
    # one object (127 slots repeat it), a full tile, 129 objects (a second workgroup that owns one), images that end with the tile
    pq, col = _requests(n_list, 3, seed=30)
    _check("objects " + "+".join(map(str, n_list)), _run(L, bank, shape, n_list, pq, col, seed=31))


@pytest.mark.parametrize("shape", SHAPES)
def test_images_without_objects(L, bank, shape):
    n_list = [5, 0, 0, 40, 0, 100, 0]
    pq, col = _requests(n_list, 2, seed=40)
    c = _run(L, bank, shape, n_list, pq, col, seed=41)
    empty = np.asarray([n_list[q] == 0 for q in pq])
    assert empty.sum() == 8 and (col[empty] >= 0).all() and np.isnan(c.ref[empty]).all()      # (their rows are checked as cells nobody owns)
    _check("images without objects", c)


def test_strides_no_bias_another_default(L, bank):
    # rows of both inputs followed by NaN (ld_pre1 = HID1 + 4, ld_e = HID2 + 3), enough predicates for both embedding-row paths
    shape = (96, 273)
    n_list = [100, 28, 100, 1, 2, 37]
    pq, col = _requests(n_list, _sr(shape[1]) + 6, seed=50)
    col[-1] = C - 1                                                       # the table's last row, read from global memory
    c = _run(L, bank, shape, n_list, pq, col, seed=51, pad1=4, pade=3, default=-7.5)
    assert c.pre1.stride(0) == shape[0] + 4 and c.emb.stride(0) == shape[1] + 3
    _check("strided, default -7.5", c)
    c = _run(L, bank, shape, n_list, pq, col, seed=51, pad1=4, pade=3, default=-7.5, bias=False)
    _check("strided, no embedding bias", c)


@pytest.mark.parametrize("shape", [(32, 257), (256, 320)])
def test_guarded_output(L, bank, shape):
    pq, col = _requests(RAGGED, 2, seed=60, noop=0.2)
    assert (col < 0).any()
    _check("guarded output", _run(L, bank, shape, RAGGED, pq, col, seed=61, guard=True))


@pytest.mark.parametrize("shape", [(64, 272), (128, 305)])
def test_range_flag(L, bank, shape):
    """DFOL_RANGE_X_OVERFLOW for an activation beyond the fp16 range or a NaN, in the last chunk's last column too; not for -1e6 (ELU: -1)."""
    n_list = [5, 9, 37]
    pq, col = _requests(n_list, 2, seed=70)
    c = _run(L, bank, shape, n_list, pq, col, seed=71)
    _check("range flag: in range", c)                                     # (asserts the clean word)
    keep = c.pre1[20, shape[0] - 1].item()
    c.pre1[20, shape[0] - 1] = 1.0e6
    assert _launch(L, c)[1] & L.RANGE_X_OVERFLOW
    c.pre1[20, shape[0] - 1] = keep
    assert _launch(L, c)[1] == 0
    c.pre1[3, 1] = float("nan")
    assert _launch(L, c)[1] & L.RANGE_X_OVERFLOW
    _check("range flag: -1e6", _run(L, bank, shape, n_list, pq, col, seed=71, edit=(20, shape[0] - 1, -1.0e6)))


def test_loud_errors(L, bank):
    """Sizes the kernel was not built for are refused before any launch, and attr_head_supported (what the callers ask) says the same."""
    for shape in SHAPES + [FULL_SIZE]:
        assert L.attr_head_supported(*shape)
    n_list = [5, 9]
    pq, col = _requests(n_list, 1, seed=80)
    c = _run(L, bank, (64, 272), n_list, pq, col, seed=81)
    wide = torch.zeros(14, 292, device="cuda")
    odd = torch.zeros(14, 66, device="cuda")
    big = torch.zeros(L.load().dfol_pair_w2_f16x2_bytes(288) // 2, dtype=torch.float16, device="cuda")
    ewide = torch.zeros(C, 324, device="cuda")
    b2 = torch.zeros(324, device="cuda")
    #        pre1               HID2  NS
    cases = {"HID1 = 48": (wide[:, :48], 272, 12), "HID1 = 288": (wide[:, :288], 272, 12), "HID2 = 256": (c.pre1, 256, 12),
             "HID2 = 321": (c.pre1, 321, 12), "ld_pre1 = HID1 + 2": (odd[:, :64], 272, 12),
             "NS = 6": (c.pre1, 272, 6)}
    for what, (hid1, hid2) in {"HID1 = 48": (48, 272), "HID1 = 288": (288, 272), "HID2 = 256": (64, 256), "HID2 = 321": (64, 321)}.items():
        assert not L.attr_head_supported(hid1, hid2), what
    for what, (pre1, hid2, NS) in cases.items():
        ll = torch.full((2, 12), float("nan"), device="cuda")
        with pytest.raises(L.DfolError):
            L.call("dfol_attr_head_h2_f32", pre1.data_ptr(), pre1.stride(0), pre1.shape[1], big.data_ptr(), b2.data_ptr(), hid2, ewide.data_ptr(),
                   ewide.stride(0), None, c.off_d.data_ptr(), 2, 14, c.pq_d.data_ptr(), c.col_d.data_ptr(), 2, NS, -30.0, ll.data_ptr(), L._stream())
        torch.cuda.synchronize()
        assert torch.isnan(ll).all(), what + ": refused, yet something was written"


def test_reduced_width_model_takes_the_head(L, monkeypatch):
    """test_interpreter_routes_with_and_without_the_head's model with the attribute network at 516 -> 128 -> 288 (the config's
    attribute_network_layers_config and word_embedding_dim): the Python operator loop and the native executor both take the head, agree bit
    for bit, match the float64 oracle to 1e-5 in probability and give the table route's (DFOL_ATTR_HEAD=0) answers."""
    from dfol_vqa_amd import native_plan as NP
    from dfol_vqa_amd import synthetic as syn
    full = syn.reference_config
    monkeypatch.setattr(syn, "reference_config", lambda paths, **over: full(paths, attribute_network_layers_config=[128], word_embedding_dim=288, **over))
    model, collater, qs, oont, dev = _smoke_model()
    lin1, lin2 = [m for m in model._oracle._attribute_network._network if isinstance(m, torch.nn.Linear)]
    assert tuple(lin1.weight.shape) == (128, 516) and tuple(lin2.weight.shape) == (288, 128)
    weights = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if k.startswith("_featurizer.") or k.startswith("_oracle.")}
    ref = orc.run_questions(oont, qs, [q["scene"] for q in qs], np.float64, weights=weights)
    got = {}
    for head in ("1", "0"):
        for native in ("1", "0"):
            monkeypatch.setenv("DFOL_ATTR_HEAD", head)
            monkeypatch.setenv("DFOL_NATIVE", native)
            pbs = collater.collate([dict(q) for q in qs])
            for pb in pbs:
                pb.create_sparse_tensors()
            L.PATH_COUNTS.clear()
            on_dev = [pb.to_cuda(dev) for pb in pbs]
            with torch.no_grad():
                res = model(on_dev, False)
            routes = dict(L.PATH_COUNTS)
            assert routes.get("native_program" if native == "1" else "python_program", 0) >= 1, routes
            if native == "1":                                  # the executor's plan takes the head's instruction, or the table route's
                ops = np.concatenate([pb._native_plan.instrs[:, 0] for pb in on_dev])
                assert bool((ops == NP.OP_ATTR_HEAD).any()) == (head == "1") and bool((ops == NP.OP_ATTR_LL).any()) == (head == "0")
            else:
                assert (routes.get("attr_head", 0) >= 1) == (head == "1"), routes
            lp = res["log_probability"].cpu().numpy()
            assert np.abs(np.exp(lp) - np.exp(ref["log_probability"])).max() < 1e-5, (head, native)
            assert res["answer"] == ref["answer"]
            got[head, native] = (lp, res["answer"])
    assert np.array_equal(got["1", "1"][0].view(np.int32), got["1", "0"][0].view(np.int32))
    assert np.array_equal(got["0", "1"][0].view(np.int32), got["0", "0"][0].view(np.int32))
    assert got["1", "1"][1] == got["0", "1"][1]
    print("attr_head 128 -> 288 interpreter: max |d log_probability| head vs table route %.3e" % np.abs(got["1", "1"][0] - got["0", "1"][0]).max())
