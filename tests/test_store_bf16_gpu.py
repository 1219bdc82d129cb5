"""GPU tests of the bf16 feature store (DeviceFeatureStore(feature_dtype="bf16"), csrc/dfol_store.hip) and the two kernels that read its
table in place in the bf16 arithmetic: dfol_linear_act_rows_bf16t_f32 (csrc/dfol_dense_split.hip, MODE 3) and dfol_linear_wgrad_bias_rows_bf16t
(csrc/dfol_dense_wgrad.hip).  Every comparison is bit equality, and every reference is a kernel that existed before the store did, over
`table.float()[src_row]` or over an fp32 store: the table holds what those kernels round an fp32 feature to, so nothing may differ.

Tables hold NaN wherever the index does not point - unnamed rows, padding columns, the weight gradient's workspace - so a read outside the
named rows shows in the result."""

import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dfol_vqa_amd as D  # noqa: E402,F401
from dfol_vqa_amd import _lib, data, experiment, training  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from dfol_vqa_amd.feature_store import StoreLayout, StoreRows  # noqa: E402
from dfol_vqa_amd.interpreter import GraphedForward  # noqa: E402
from test_feature_store import write_chunks  # noqa: E402
from test_store_bf16 import rne_bf16, rounding_inputs, widen_bf16  # noqa: E402
from test_wgrad_rows_gpu import PATTERNS, SHAPES, first_growth, index_of  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAN = float("nan")
BF16 = torch.bfloat16
ACTS = (_lib.ACT_NONE, _lib.ACT_SIGMOID, _lib.ACT_ELU, _lib.ACT_LOGSIGMOID)
KEYS = ("feature_store_direct", "feature_store_direct_train", "feature_store_direct_materialized")


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def bits16(t):
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16)


def counts_of(fn):
    before = dict(_lib.PATH_COUNTS)
    out = fn()
    return out, {k: _lib.PATH_COUNTS.get(k, 0) - before.get(k, 0) for k in KEYS + ("native_program", "python_program")}


# ---- 1. rounding ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [None, 1, 7])
def test_round_kernel_is_round_to_nearest_even(n):
    x = rounding_inputs()[:n]
    dst = torch.full((x.size + 2,), NAN, dtype=BF16, device=DEV)
    _lib.store_round_bf16(torch.from_numpy(x.copy()).to(DEV), dst[:x.size])
    got = bits16(dst)
    assert np.array_equal(got[:x.size], rne_bf16(x))
    assert np.isnan(widen_bf16(got[x.size:])).all()                     # nothing written past n, an odd count included


# ---- 2. gather --------------------------------------------------------------------------------------------------------------------------
G_COUNTS = [1, 6, 3, 2, 6, 5]                                            # 1 object, max_obj objects, odd counts (both output-row alignments)


@pytest.fixture(scope="module", params=[12, 1028], ids=lambda f: "F%d" % f)
def stores(request, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bf16_store"))
    F = request.param                                                    # (1028: 257 pieces per row - the four-in-flight loop and its tail)
    chunks, info = write_chunks(d, feature_dim=F, max_obj=6, counts=G_COUNTS, per_chunk=4, seed=3)
    f32 = data.DeviceFeatureStore(d, "objs", chunks, info, DEV)
    b16 = data.DeviceFeatureStore(d, "objs", chunks, info, DEV, feature_dtype="bf16")
    named = torch.zeros(b16.S, 6, dtype=torch.bool)
    for k, n in enumerate(G_COUNTS):
        named[k, :n] = True
    b16.features[~named.to(DEV)] = NAN                                    # every row no image names (objects past the count, slots without an image)
    return d, chunks, info, f32, b16, F


def test_store_bookkeeping(stores):
    d, chunks, info, f32, b16, F = stores
    lay = StoreLayout(d, "objs", chunks, info, feature_itemsize=2)
    assert b16.features.dtype == BF16 and tuple(b16.features.shape) == (8, 6, F) and b16.boxes.dtype == b16.sizes.dtype == torch.float32
    assert b16.direct and not b16.featurized and b16.feature_dtype == "bf16" and f32.feature_dtype == "f32" and not f32.direct
    assert b16.nbytes == sum(lay.chunk_bytes) == 8 * (2 * 6 * F + 4 * (6 * 4 + 2)) and f32.nbytes == 8 * 4 * (6 * F + 6 * 4 + 2)
    # under a budget that admits one whole fp32 chunk the bf16 store holds the chunks its own per-chunk bytes give
    budget = StoreLayout(d, "objs", chunks, info).chunk_bytes[0]
    want = 0
    while want < chunks and sum(lay.chunk_bytes[:want + 1]) <= budget:
        want += 1
    part = data.DeviceFeatureStore(d, "objs", chunks, info, DEV, max_bytes=budget, feature_dtype="bf16")
    assert part.resident_chunks == want >= 1 and part.nbytes == sum(lay.chunk_bytes[:want])
    assert data.DeviceFeatureStore(d, "objs", chunks, info, DEV, max_bytes=budget).resident_chunks == 1
    with pytest.raises(_lib.DfolError, match="not built"):
        b16.featurize(None)


def test_materialize_equals_the_fp32_stores_rounded(stores):
    d, chunks, info, f32, b16, F = stores
    images = ["img%03d" % k for k in (1, 0, 2, 5, 1, 3, 4)]
    ref32, ref16 = f32.index.ref(images), b16.index.ref(images)
    want = f32.gather(ref32)
    got = b16.rows(ref16).materialize()
    assert isinstance(b16.rows(ref16), StoreRows) and tuple(got.shape) == tuple(want.shape) == (sum(G_COUNTS[k] for k in (1, 0, 2, 5, 1, 3, 4)), F + 6)
    w = want.cpu().numpy()
    w[:, :F] = widen_bf16(rne_bf16(w[:, :F]))
    assert np.array_equal(bits(got), w.view(np.uint32))                  # (the box columns: equal bits outright)
    assert np.array_equal(bits(got[:, F:]), bits(want[:, F:]))
    assert np.array_equal(bits(b16.gather(ref16)), bits(got))
    # rows of an odd stride: all four store alignments; the padding column is left alone
    wide = torch.full((got.shape[0], F + 7), -7.5, device=DEV)
    assert b16.gather(ref16, out=wide) is wide
    assert np.array_equal(bits(wide[:, :F + 6]), bits(got)) and bool((wide[:, F + 6] == -7.5).all())


def test_f_not_a_multiple_of_four_is_refused(tmp_path):
    chunks, info = write_chunks(tmp_path, feature_dim=6)
    with pytest.raises(_lib.DfolError, match=r"F % 4 == 0"):
        data.DeviceFeatureStore(str(tmp_path), "objs", chunks, info, DEV, feature_dtype="bf16")


# ---- 3. forward product -----------------------------------------------------------------------------------------------------------------
def bf16_table(R, K, ld, named, g):
    """[R, ld] bfloat16, NaN everywhere but the first K columns of the rows `named`."""
    table = torch.full((R, ld), NAN, dtype=BF16)
    table[named, :K] = torch.randn(named.numel(), K, generator=g).to(BF16)
    return table.to(DEV)


def forward_case(M, N, K, ld, pattern, act, seed, R=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    R = R or 2 * M + 5
    idx = index_of(pattern, M, R, g)
    table = bf16_table(R, K, ld, torch.unique(idx.long()), g)
    idx = idx.to(DEV)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    where = (M, N, K, ld, pattern, act)
    assert _lib.linear_rows_bf16t_supported(N, K, ld), where
    with _lib.dense_math("bf16"):
        want = _lib.linear_act_split(table.float()[idx.long()][:, :K].contiguous(), W, b, act)
        out = torch.full((M, N), NAN, device=DEV)
        got = _lib.linear_rows_bf16t(table[:, :K], idx, W, b, act, out)
    assert bool(torch.isfinite(want).all()) and np.array_equal(bits(want), bits(got)), where


@pytest.mark.parametrize("K", [36, 128, 2048])
@pytest.mark.parametrize("N", [44, 128, 300, 512])
def test_rows_product_equals_the_matrix_product(N, K):
    for p, M in enumerate((1, 63, 64, 65, 129, 200)):                    # 64-row blocks
        forward_case(M, N, K, K if p % 2 else K + 8, PATTERNS[p % len(PATTERNS)], _lib.ACT_SIGMOID, 100 * M + p)


def test_rows_product_every_activation_and_index_pattern():
    for act in ACTS:
        forward_case(129, 300, 128, 136, "repeats", act, 7 + act)
    for pattern in PATTERNS:                                             # (first_last names the table's last row)
        forward_case(65, 128, 36, 44, pattern, _lib.ACT_ELU, 31)


def test_rows_product_on_128_row_blocks():
    M = 16384 + 5                                                         # 129 x 4 blocks of 128 rows: the kernel's other block height
    forward_case(M, 512, 128, 128, "descending", _lib.ACT_SIGMOID, 5, R=M + 77)
    forward_case(M, 512, 128, 136, "repeats", _lib.ACT_NONE, 6, R=M + 77)


def test_rows_product_beyond_a_four_gigabyte_offset():
    K, N = 2048, 128
    R = (1 << 32) // (2 * K) + 9                                          # the last rows lie past 2^32 bytes
    table = torch.empty((R, K), dtype=BF16, device=DEV)                   # uninitialised: only the named rows are written
    g = torch.Generator(device="cpu").manual_seed(11)
    idx = torch.tensor([R - 1, 5, R - 3, 5, R - 1, 0, R - 2], dtype=torch.int32)
    assert (R - 3) * 2 * K >= 1 << 32
    named = torch.unique(idx.long())
    table[named.to(DEV)] = torch.randn(named.numel(), K, generator=g).to(BF16).to(DEV)
    W, b, idx = (torch.randn(N, K, generator=g) / K ** 0.5).to(DEV), torch.randn(N, generator=g).to(DEV), idx.to(DEV)
    with _lib.dense_math("bf16"):
        want = _lib.linear_act_split(table[idx.long()].float(), W, b, _lib.ACT_SIGMOID)
        got = _lib.linear_rows_bf16t(table, idx, W, b, _lib.ACT_SIGMOID)
    assert bool(torch.isfinite(want).all()) and np.array_equal(bits(want), bits(got))


def test_rows_product_empty_and_refusals():
    g = torch.Generator(device="cpu").manual_seed(2)
    table = bf16_table(9, 40, 48, torch.arange(9), g)
    W, idx = torch.randn(16, 40).to(DEV), torch.arange(4, dtype=torch.int32, device=DEV)
    y = torch.full((4, 16), -7.5, device=DEV)
    lib, st = _lib.load(), _lib._stream()
    assert lib.dfol_linear_act_rows_bf16t_f32(None, 48, None, None, None, None, 16, 0, 16, 40, 0, st) == 0           # M = 0: no launch, no pointer read
    assert tuple(_lib.linear_rows_bf16t(table[:, :40], idx[:0], W, None, 0).shape) == (0, 16)
    packed = _lib.linear_pack_w_split(W, False, 1)

    def refused(tab_ptr, ld, K, what):
        with pytest.raises(_lib.DfolError, match=what):
            _lib.call("dfol_linear_act_rows_bf16t_f32", tab_ptr, ld, idx.data_ptr(), packed.data_ptr(), None, y.data_ptr(), 16, 4, 16, K, 0, st)

    refused(table.data_ptr(), 48, 38, "multiple of 4")
    refused(table.data_ptr(), 46, 40, "8-byte aligned")
    refused(table.data_ptr(), 36, 40, "cover K")
    refused(table.data_ptr() + 2, 48, 40, "8-byte")
    assert not _lib.linear_rows_bf16t_supported(16, 38, 48) and not _lib.linear_rows_bf16t_supported(16, 40, 46)
    assert not _lib.linear_rows_bf16t_supported(16, 40, 36) and _lib.linear_rows_bf16t_supported(16, 40, 48)
    with pytest.raises(_lib.DfolError, match="bfloat16"):
        _lib.linear_rows_bf16t(table.float()[:, :40], idx, W, None, 0)
    torch.cuda.synchronize()
    assert bool((y == -7.5).all())                                        # nothing was launched


# ---- 4. weight gradient -----------------------------------------------------------------------------------------------------------------
def wgrad_case(M, N, K, pattern, want_db, seed):
    """dfol_linear_wgrad_bias_bf16 over the gathered, widened rows against dfol_linear_wgrad_bias_rows_bf16t over the table: NaN workspace,
    NaN results, NaN in every unnamed table row, in the table's padding and in the gathered matrix's six extra columns."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    R, ld = 8 * M + 3, K + 12
    idx = index_of(pattern, M, R, g)
    table = bf16_table(R, K, ld, torch.unique(idx.long()), g)
    dy = (torch.randn(M, N, generator=g) * 0.1).to(DEV)
    idx = idx.to(DEV)
    mat = torch.full((M, K + 6), NAN, device=DEV)
    mat[:, :K] = table.float()[idx.long(), :K]
    lib, out = _lib.load(), []
    where = (M, N, K, pattern, want_db)
    assert _lib.linear_wgrad_rows_supported(N, K, N, ld, bf16_table=True), where
    for rows_form in (False, True):
        ws = torch.full((lib.dfol_linear_wgrad_workspace(M, N, K),), NAN, device=DEV)
        dw = torch.full((N, K), NAN, device=DEV)
        db = torch.full((N,), NAN, device=DEV) if want_db else None
        tail = (M, N, K, ws.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(), _lib._stream())
        if rows_form:
            _lib.call("dfol_linear_wgrad_bias_rows_bf16t", dy.data_ptr(), N, table.data_ptr(), ld, idx.data_ptr(), *tail)
        else:
            _lib.call("dfol_linear_wgrad_bias_bf16", dy.data_ptr(), N, mat.data_ptr(), K + 6, *tail)
        out.append((dw, db))
    (dw0, db0), (dw1, db1) = out
    assert bool(torch.isfinite(dw0).all()) and np.array_equal(bits(dw0), bits(dw1)), where
    if want_db:
        assert bool(torch.isfinite(db0).all()) and np.array_equal(bits(db0), bits(db1)), where


@pytest.mark.parametrize("shape", SHAPES + [(512, 2048)], ids=lambda s: "%dx%d" % s)
def test_rows_wgrad_equals_the_matrix_wgrad(shape):
    N, K = shape
    # around the 16-row MFMA step; 20 and 27: the range ends inside the eight rows of a lane of the first / second half; more slabs than one row gets
    Ms = (257,) if shape == (512, 2048) else (1, 15, 16, 17, 20, 27, 257, first_growth(N, K) + 2)
    for M in Ms:
        for p, pattern in enumerate(PATTERNS):
            wgrad_case(M, N, K, pattern, (M + p) % 2 == 0, 1000 * M + p)


def test_rows_wgrad_host_wrapper():
    M, N, K = 300, 256, 260
    assert N * K >= _lib.SPLIT_MIN_WEIGHT
    g = torch.Generator(device="cpu").manual_seed(9)
    idx = index_of("repeats", M, 1000, g)
    table = bf16_table(1000, K, K, torch.unique(idx.long()), g)
    dy, idx = (torch.randn(M, N, generator=g) * 0.1).to(DEV), idx.to(DEV)
    with _lib.dense_math("bf16"):
        dw0, db0 = _lib.linear_wgrad(dy, table.float()[idx.long()], bias=True)
        dw1, db1 = _lib.linear_wgrad_rows(dy, table, idx, bias=True)
        dw, db = _lib.linear_wgrad_rows(dy[:0], table, idx[:0], bias=True)
    assert np.array_equal(bits(dw0), bits(dw1)) and np.array_equal(bits(db0), bits(db1))
    assert tuple(dw.shape) == (N, K) and not bool(dw.any()) and not bool(db.any())
    with pytest.raises(_lib.DfolError, match="needs the bf16 mode"):     # another arithmetic gets the gathered matrix, never this table
        with _lib.dense_math("f16x2"):
            _lib.linear_wgrad_rows(dy, table, idx)
    with pytest.raises(_lib.DfolError, match=r"ld_table % 4"):
        _lib.call("dfol_linear_wgrad_bias_rows_bf16t", dy.data_ptr(), N, table.data_ptr(), K + 2, idx.data_ptr(), M, N, K, dy.data_ptr(), dy.data_ptr(), None,
                  _lib._stream())
    assert not _lib.linear_wgrad_rows_supported(N, K, N, K + 2, bf16_table=True) and not _lib.linear_wgrad_rows_supported(N, 258, N, 260, bf16_table=True)


# ---- 5. / 6. end to end -----------------------------------------------------------------------------------------------------------------
MAX_OBJ = 40
E_COUNTS = [40, 10, 25, 40, 10, 25, 13, 37]       # images 0-2 and 3-5 have the same object counts: a second scene for a captured batch
IMAGES = [6, 1, 6, 3, 0]                          # 13 .. 40 objects, one image asked twice
CLIP = 0.65


class World(object):
    """The full-size synthetic model in training form (nothing frozen, dropout 0) over chunk files of ordinary fp32 features (`plain`) and of
    features that are bf16 values already (`rounded`), each behind an fp32 store with direct=False and a bf16 store."""

    def __init__(self, directory):
        self.paths, self.names = syn.write_synthetic_ontology(os.path.join(directory, "ontology"))
        over = dict(freeze_featurizer=False, freeze_attribute_network=False, freeze_relation_network=False, freeze_embedding_network=False, dropout=0.0)
        self.cfg = syn.reference_config(self.paths, **over)
        self.ont = experiment.build_ontology(self.cfg)
        torch.manual_seed(0)
        self.model = experiment.build_model(self.cfg, self.ont)
        with torch.no_grad():
            self.model._oracle._embedding_network.linear.weight.normal_(0.0, 0.1)
            self.model._oracle._embedding_network.linear.bias.fill_(-2.0)
        self.model = self.model.to(DEV)
        self.state0 = copy.deepcopy(self.model.state_dict())
        with open(self.paths["attribute_file"]) as f:
            self.cats = json.load(f)
        self.dirs, self.stores = {}, {}
        for name in ("plain", "rounded"):
            d = os.path.join(directory, name)
            os.makedirs(d)
            chunks, info = write_chunks(d, feature_dim=2048, max_obj=MAX_OBJ, counts=E_COUNTS, per_chunk=4, seed=17)
            if name == "rounded":
                for c in range(chunks):
                    z = dict(np.load(os.path.join(d, "objs_%d.npz" % c)))
                    z["features"] = widen_bf16(rne_bf16(z["features"])).reshape(z["features"].shape)
                    if c == 0:
                        z["features"][1, 3, 7] = 2.0 ** 17            # image 1: one feature beyond fp16's 65504 (a bf16 value)
                    np.savez(os.path.join(d, "objs_%d.npz" % c), **z)
            self.dirs[name] = (d, chunks, info)
            self.stores[name, "f32"] = data.DeviceFeatureStore(d, "objs", chunks, info, DEV)
            self.stores[name, "bf16"] = data.DeviceFeatureStore(d, "objs", chunks, info, DEV, feature_dtype="bf16")

    def host_batches(self, name, dtype, images, kind="verify_rel", share=False, seed=61):
        d, chunks, info = self.dirs[name]
        qs = syn.full_size_questions(kind, len(images), 10, MAX_OBJ, self.names, self.cats, seed, with_scene=False)
        for q, im in zip(qs, images):
            q["image_id"] = "img%03d" % im
        pbs = data.BatchGQABoxFeaturesCollator(d, "objs", chunks, info, self.ont, 2, device_store=self.stores[name, dtype].index,
                                               share_scenes=share).collate([dict(q) for q in qs])
        for pb in pbs:
            pb.create_sparse_tensors()
        return pbs

    def mode(self, math, train, dropout=0.0, overflow="raise"):
        self.model._mlp_math, self.model._range_overflow = math, overflow
        self.model.train(train)
        for m in self.model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = dropout

    def infer(self, name, dtype, images, **kw):
        pbs = self.host_batches(name, dtype, images, **kw)
        with torch.no_grad():
            res = self.model([pb.to_cuda(DEV) for pb in pbs], False)
        return len(pbs), res["log_probability"].cpu().numpy().copy(), res["answer"]

    def reset(self, opt=None):
        with torch.no_grad():
            self.model.load_state_dict(self.state0)
            for st in ([] if opt is None else opt.state.values()):
                for v in st.values():
                    if isinstance(v, torch.Tensor):
                        v.zero_()
        if opt is None:
            for p in self.model.parameters():
                p.grad = None

    def adam(self):
        return torch.optim.Adam([p for p in self.model.parameters() if p.requires_grad], lr=1e-3, capturable=True)

    def snapshot(self, grads):
        return {k: (p.grad if grads else p).detach().cpu().numpy().copy() for k, p in self.model.named_parameters() if not grads or p.grad is not None}

    def eager_step(self, name, dtype, images):
        self.reset()
        dev = [pb.to_cuda(DEV) for pb in self.host_batches(name, dtype, images)]
        (loss, _), counts = counts_of(lambda: training.train_batch(self.model, self.adam(), dev, clip_norm=CLIP, sync_loss=False))
        return np.float64(float(loss)), self.snapshot(True), self.snapshot(False), counts, len(dev)


def same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


def steps_equal(s0, s1):
    return s0[0].tobytes() == s1[0].tobytes() and bool(np.isfinite(s0[0])) and same(s0[1], s1[1]) and same(s0[2], s1[2])


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    saved = {k: os.environ.pop(k, None) for k in ("DFOL_NATIVE", "DFOL_DENSE_MATH")}
    yield World(str(tmp_path_factory.mktemp("bf16_world")))
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("share", [False, True])
def test_bf16_mode_inference_has_the_fp32_stores_bits(world, share, native, monkeypatch):
    monkeypatch.setenv("DFOL_NATIVE", native)
    world.mode("bf16", train=False)
    for kind in ("exist", "verify_rel"):
        (n0, lp0, a0), c0 = counts_of(lambda: world.infer("plain", "f32", IMAGES, kind=kind, share=share))
        (n1, lp1, a1), c1 = counts_of(lambda: world.infer("plain", "bf16", IMAGES, kind=kind, share=share))
        where = (kind, share, native, c0, c1)
        assert n0 == n1 and bool(np.isfinite(lp0).all()) and np.array_equal(lp0.view(np.uint32), lp1.view(np.uint32)) and a0 == a1, where
        assert c0["feature_store_direct"] == c0["feature_store_direct_materialized"] == 0, where
        assert c1["feature_store_direct"] == n1 and c1["feature_store_direct_materialized"] == c1["feature_store_direct_train"] == 0, where
        assert c1["native_program" if native == "1" else "python_program"] == n1 and c0["native_program"] == c1["native_program"], where


def test_bf16_mode_graphed_forward_serves_a_second_scene(world, monkeypatch):
    monkeypatch.setenv("DFOL_NATIVE", "1")
    world.mode("bf16", train=False)
    store = world.stores["plain", "bf16"]
    scenes = ([0, 1, 2, 1], [3, 4, 5, 4])
    host = [world.host_batches("plain", "bf16", ims, kind="exist", seed=77) for ims in scenes]
    with torch.no_grad():
        want = [world.infer("plain", "f32", ims, kind="exist", seed=77) for ims in scenes]
    assert not np.array_equal(want[0][1].view(np.uint32), want[1][1].view(np.uint32))
    dev = [pb.to_cuda(DEV) for pb in host[0]]
    assert all(isinstance(pb._object_features, StoreRows) for pb in dev)
    g, c = counts_of(lambda: GraphedForward(world.model, dev))
    assert c["feature_store_direct"] > 0 and c["feature_store_direct_materialized"] == 0, c
    for k in (0, 1):
        for pb, pb2 in zip(dev, host[k]):
            assert store.rows(pb2._object_features, out=pb._object_features) is pb._object_features
        r = g()
        assert np.array_equal(bits(r["log_probability"]), want[k][1].view(np.uint32)) and r["answer"] == want[k][2], k


def test_bf16_mode_train_step_has_the_fp32_stores_bits(world):
    world.mode("bf16", train=True)
    s0 = world.eager_step("plain", "f32", IMAGES)
    s1 = world.eager_step("plain", "bf16", IMAGES)
    n = s1[4]
    assert steps_equal(s0, s1)
    assert not same(s1[2], {k: v.cpu().numpy() for k, v in world.state0.items() if k in s1[2]})          # a non-zero Adam step
    assert any(k.startswith("_featurizer") for k in s1[1])
    assert {k: s1[3][k] for k in KEYS} == {"feature_store_direct": n, "feature_store_direct_train": n, "feature_store_direct_materialized": 0}, s1[3]
    assert {k: s0[3][k] for k in KEYS} == {"feature_store_direct": 0, "feature_store_direct_train": 0, "feature_store_direct_materialized": 0}, s0[3]


def test_bf16_mode_graphed_train_step_replays_new_scenes(world):
    world.mode("bf16", train=True)
    batches = ([0, 1, 2, 1], [3, 4, 5, 4])
    eager = [world.eager_step("plain", "f32", ims) for ims in batches]
    assert eager[0][0].tobytes() != eager[1][0].tobytes()
    host = [world.host_batches("plain", "bf16", ims) for ims in batches]
    store = world.stores["plain", "bf16"]
    world.reset()
    opt = world.adam()
    dev = [pb.to_cuda(DEV) for pb in host[0]]
    step, c = counts_of(lambda: training.GraphedTrainStep(world.model, opt, dev, CLIP, warmup=1))
    assert c["feature_store_direct_train"] >= 2 and c["feature_store_direct_materialized"] == 0, c
    for k in (0, 1, 0):
        for pb, pb2 in zip(dev, host[k]):
            assert store.rows(pb2._object_features, out=pb._object_features) is pb._object_features
        world.reset(opt)
        loss, _ = step()
        torch.cuda.synchronize()
        assert steps_equal((np.float64(float(loss)), world.snapshot(True), world.snapshot(False)), eager[k]), k


def test_other_arithmetics_get_the_matrix_of_the_rounded_features(world, monkeypatch):
    """Chunk files whose features are bf16 values already: the bf16 store then holds what the fp32 store holds, and every route outside
    `mlp_math: bf16` - here the default f16x2 - must give the fp32 store's bits from the materialised matrix."""
    monkeypatch.setenv("DFOL_NATIVE", "1")
    images = [6, 2, 6, 3, 0]                                              # (not image 1: its out-of-range feature is the next test's)
    world.mode(None, train=False)
    (n0, lp0, a0), c0 = counts_of(lambda: world.infer("rounded", "f32", images))
    (n1, lp1, a1), c1 = counts_of(lambda: world.infer("rounded", "bf16", images))
    assert n0 == n1 and bool(np.isfinite(lp0).all()) and np.array_equal(lp0.view(np.uint32), lp1.view(np.uint32)) and a0 == a1
    assert c1["feature_store_direct_materialized"] == n1 and c1["feature_store_direct"] == 0 and c0["feature_store_direct_materialized"] == 0, (c0, c1)
    world.mode(None, train=True)
    s0, s1 = world.eager_step("rounded", "f32", images), world.eager_step("rounded", "bf16", images)
    assert steps_equal(s0, s1)
    assert {k: s1[3][k] for k in KEYS} == {"feature_store_direct": 0, "feature_store_direct_train": 0, "feature_store_direct_materialized": s1[4]}, s1[3]


def test_range_rerun_over_a_bf16_store(world, monkeypatch):
    monkeypatch.setenv("DFOL_NATIVE", "1")
    images = [1, 2, 1, 0]                                                 # image 1 holds 2^17
    world.mode(None, train=False, overflow="rerun")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                   # (the rerun says so once per route)
        before = _lib.PATH_COUNTS["fallback:range_rerun"]
        (n0, lp0, a0), c0 = counts_of(lambda: world.infer("rounded", "f32", images))
        (n1, lp1, a1), c1 = counts_of(lambda: world.infer("rounded", "bf16", images))
    world.mode(None, train=False)
    assert _lib.PATH_COUNTS["fallback:range_rerun"] >= before + 2         # both stores' batches left fp16's range and ran again
    assert n0 == n1 and bool(np.isfinite(lp0).all()) and np.array_equal(lp0.view(np.uint32), lp1.view(np.uint32)) and a0 == a1
    assert c1["feature_store_direct"] == 0 and c1["feature_store_direct_materialized"] >= n1, c1


def test_active_dropout_trains_over_the_materialised_matrix(world):
    world.mode("bf16", train=True, dropout=0.1)
    s = world.eager_step("plain", "bf16", IMAGES)
    world.mode("bf16", train=True)
    assert bool(np.isfinite(s[0]))
    assert {k: s[3][k] for k in KEYS} == {"feature_store_direct": 0, "feature_store_direct_train": 0, "feature_store_direct_materialized": s[4]}, s[3]


def test_bf16_rows_in_front_of_another_first_layer_are_refused(world):
    """DFOL_FEATURES_ROWS_BF16 with a model whose first featurizer layer is not DFOL_DENSE_BF16: the executor says why and runs nothing."""
    from dfol_vqa_amd import native_exec
    world.mode(None, train=False)                                         # f16x2: the executor's first layer is DFOL_DENSE_F16X2
    pbs = world.host_batches("plain", "bf16", IMAGES, kind="exist")
    real = _lib.call

    def call(name, *args):                                                # hand the executor the bf16 index form in its own run's scene struct
        if name == "dfol_run_program":
            rows, scene = pbs_dev[0]._object_features, args[1]._obj
            scene.feature_form, scene.src_row, scene.box6 = native_exec.FEATURES_ROWS_BF16, rows.src_row.data_ptr(), rows.box6.data_ptr()
        return real(name, *args)
    pbs_dev = [pb.to_cuda(DEV) for pb in pbs]
    os.environ["DFOL_NATIVE"] = "1"
    _lib.call = call
    try:
        with pytest.raises(_lib.DfolError, match="DFOL_DENSE_BF16"), torch.no_grad():
            world.model(pbs_dev[:1], False)
    finally:
        _lib.call = real
        os.environ.pop("DFOL_NATIVE", None)
    assert native_exec.DENSE_BF16 == 3
