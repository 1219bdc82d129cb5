"""A gated model over bf16 relation tiles (`trainable_gate: True` with `relation_tile_dtype: bf16`, DFOL_GATE_NATIVE=1 DFOL_GATE_BF16=1; DESIGN.md
3.7, 4): the native executor against the Python operator loop under the same switches, bit for bit - both run dfol_relate_one_gate_fwd_bf16 on
tiles the pair kernel wrote as bf16 - per question, on shared scenes and calibrated; the batches that keep fp32 tiles (NS % 8 != 0, a
choose_rel) against the same model with fp32 tile storage, bit for bit; the refusal with the switch off; and bf16 against fp32 tiles under the
bound tests/test_native_gpu.py::test_native_bf16_relation_tiles states for that comparison of the ungated model (|d log p| <= 5e-2)."""

import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import _lib, native_exec, ops  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from test_native_gpu import ALL_KINDS, TableCollater, _FullCalibrationCollater, same_results  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16_VS_F32_BOUND = 5e-2                # test_native_gpu.test_native_bf16_relation_tiles: the same model and batch on bf16 and on fp32 tiles
_MODELS = {}


def soft_product_gates(model, seed=11):
    """Every gate tensor its own values, around the gate that IS the ungated cell's product (alpha0..2 -> 0, alpha3..5 -> 1: G(a, b) = a + b): biases
    -+6 with noise, weights U(-0.7, 0.7).  Gates drawn around zero put a floor of ~0.3 under every element's probability, and an EXISTS over 40
    objects then answers log p = 0 exactly whatever the tiles hold - a batch on which bf16 and fp32 tiles could not be told apart."""
    rng = np.random.RandomState(seed)
    named = [(k, p) for k, p in model.named_parameters() if "_nlg" in k]
    assert len(named) >= 32
    with torch.no_grad():
        for k, p in named:
            v = rng.uniform(-0.7, 0.7, tuple(p.shape)).astype(np.float32)
            if k.endswith(".bias"):
                v += np.asarray([-6, -6, -6, 6, 6, 6], np.float32)
            p.copy_(torch.from_numpy(v))
    flat = [p.detach().cpu().numpy().tobytes() for _, p in named]
    assert len(set(flat)) == len(flat)                            # gate_s and gate_o of every cell differ: swapping them changes the answer


def build(tmp_path_factory, calibrated):
    """The seeded full-size model through experiment's config route with both keys set (hid2 = 300 > 256: the packed pair kernels write bf16 tiles)."""
    if calibrated not in _MODELS:
        from dfol_vqa_amd import experiment
        paths, names = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("gate_bf16")))
        cfg = syn.reference_config(paths, trainable_gate=True, relation_tile_dtype="bf16", activate_attention_transfer=calibrated)
        ont = experiment.build_ontology(cfg)
        torch.manual_seed(5)
        model = experiment.build_model(cfg, ont)
        syn.load_seeded_weights(model, 23)
        if calibrated:
            with torch.no_grad():                                  # (the reference initialises the output layer's weight to zero)
                out = model._ops['filter']._filter._attention_output_network[0]
                out.weight.normal_(0.0, 0.5)
                out.bias.normal_(0.0, 0.5)
        soft_product_gates(model)
        with open(paths["attribute_file"]) as f:
            categories = json.load(f)
        model = model.to(DEV).eval()
        assert model._oracle._tile_dtype == torch.bfloat16 and model._gated()
        lin = [m for m in model._oracle._relation_network._network if isinstance(m, torch.nn.Linear)]
        assert _lib.pair_tiles_bf16_ok(lin[0].out_features, lin[1].out_features)
        _MODELS[calibrated] = (model, ont, names, categories)
    return _MODELS[calibrated]


@pytest.fixture(scope="module")
def gated(tmp_path_factory):
    return build(tmp_path_factory, False)


def questions(kind, n_lo, n_hi, names, categories, shared=False, count=8):
    qs = syn.full_size_questions(kind, count, n_lo, n_hi, names, categories, 1700 + ALL_KINDS.index(kind))
    qs[0]["scene"] = syn.feature_scene(qs[0]["question_id"], n_hi, 2048)       # (the largest image fixes NS)
    if shared:
        for i, q in enumerate(qs):
            q["image_id"], q["scene"] = "img%d" % (i % 3), qs[i % 3]["scene"]
    return qs


class Spy(object):
    """What the Python loop did: the dtype of every prefetched tile set, and the calls of the two one-launch gated wrappers."""

    def __init__(self, model, monkeypatch):
        self.dtypes, self.bf16_calls, self.f32_calls = [], 0, 0
        oracle = model._oracle
        remember = oracle._remember_tiles

        def spy_remember(world, low, toks, entry):
            self.dtypes.append(entry[0].dtype)
            return remember(world, low, toks, entry)

        b16, f32 = ops.relate_one_gate_fwd_bf16, ops.relate_one_gate_fwd

        def spy_b16(*a, **k):
            self.bf16_calls += 1
            return b16(*a, **k)

        def spy_f32(*a, **k):
            self.f32_calls += 1
            return f32(*a, **k)

        monkeypatch.setattr(oracle, "_remember_tiles", spy_remember, raising=False)
        monkeypatch.setattr(ops, "relate_one_gate_fwd_bf16", spy_b16)
        monkeypatch.setattr(ops, "relate_one_gate_fwd", spy_f32)


def forward(model, qs, native, monkeypatch, collater, switch=True, **kw):
    """One forward under DFOL_GATE_NATIVE=1 and (switch) DFOL_GATE_BF16=1 -> (results, route counters, batch count)."""
    monkeypatch.setenv("DFOL_GATE_NATIVE", "1")
    monkeypatch.setenv("DFOL_NATIVE", native)
    if switch:
        monkeypatch.setenv("DFOL_GATE_BF16", "1")
    else:
        monkeypatch.delenv("DFOL_GATE_BF16", raising=False)
    pbs = collater.collate([dict(q) for q in qs])
    for pb in pbs:
        pb.create_sparse_tensors()
    pbs = [pb.to_cuda(DEV) for pb in pbs]
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        res = model(pbs, False, **kw)
    return res, dict(_lib.PATH_COUNTS), len(pbs)


def both(model, qs, monkeypatch, make_collater, **kw):
    nat, c_nat, n = forward(model, qs, "1", monkeypatch, make_collater(), **kw)
    assert c_nat.get("native_program", 0) == n and not c_nat.get("python_program") and not c_nat.get("fallback:trainable_gate"), c_nat
    py, c_py, n = forward(model, qs, "0", monkeypatch, make_collater(), **kw)
    assert c_py.get("python_program", 0) == n and not c_py.get("native_program"), c_py
    return nat, py, c_py


def with_fp32_tiles(model, fn):
    """fn() on the same model with `relation_tile_dtype` left at fp32."""
    model._oracle._tile_dtype = torch.float32
    try:
        return fn()
    finally:
        model._oracle._tile_dtype = torch.bfloat16


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("kind,n_lo,n_hi", [("exist", 40, 40), ("verify_rel", 33, 40)])
def test_executor_equals_python_loop_on_bf16_tiles(gated, kind, n_lo, n_hi, shared, monkeypatch):
    model, ont, names, categories = gated
    qs = questions(kind, n_lo, n_hi, names, categories, shared)
    spy = Spy(model, monkeypatch)
    make = lambda: TableCollater(1, ont, "X", share_scenes=True) if shared else TableCollater(1, ont, "X")
    nat, py, counts = both(model, qs, monkeypatch, make)
    same_results(nat, py, "gated bf16 tiles %s shared=%s" % (kind, shared))
    assert bool(torch.isfinite(nat["log_probability"]).all())
    assert spy.dtypes and all(d == torch.bfloat16 for d in spy.dtypes), spy.dtypes             # the prefetched tiles are bfloat16
    assert spy.bf16_calls >= 1 and spy.f32_calls == 0
    assert counts.get("relate_one_gate_bf16", 0) == spy.bf16_calls                              # counted once per hop
    # bf16 against fp32 tiles: the bound of the ungated model's comparison; not the same bits (the tiles really were rounded)
    f32, c32, n = with_fp32_tiles(model, lambda: forward(model, qs, "1", monkeypatch, make()))
    assert c32.get("native_program", 0) == n
    d = (f32["log_probability"] - nat["log_probability"]).abs().max().item()
    print("log p on bf16 tiles", nat["log_probability"].cpu().numpy().ravel()[:8])
    print("gated %s shared=%s: max |d log p| bf16 vs fp32 tiles = %.3g (bound %g)" % (kind, shared, d, BF16_VS_F32_BOUND))
    assert not torch.equal(f32["log_probability"], nat["log_probability"])
    assert d <= BF16_VS_F32_BOUND


@pytest.mark.parametrize("kind,n_lo,n_hi", [("exist", 30, 36), ("choose_rel", 40, 40)])
def test_batches_that_keep_fp32_tiles(gated, kind, n_lo, n_hi, monkeypatch):
    """NS = 36 is no multiple of 8, and choose_rel's two-posterior cell reads fp32: fp32 tiles and the fp32 gated kernels, the bits of the same
    model with fp32 tile storage."""
    model, ont, names, categories = gated
    qs = questions(kind, n_lo, n_hi, names, categories)
    spy = Spy(model, monkeypatch)
    make = lambda: TableCollater(1, ont, "X")
    nat, py, counts = both(model, qs, monkeypatch, make)
    same_results(nat, py, "gated, fp32 fallback %s" % kind)
    assert spy.dtypes and all(d == torch.float32 for d in spy.dtypes), spy.dtypes
    assert spy.bf16_calls == 0 and not counts.get("relate_one_gate_bf16")
    assert spy.f32_calls >= (1 if kind == "exist" else 0)
    f32_nat, f32_py, _ = with_fp32_tiles(model, lambda: both(model, qs, monkeypatch, make))
    same_results(nat, f32_nat, "fp32 fallback against fp32 storage (executor) %s" % kind)
    same_results(py, f32_py, "fp32 fallback against fp32 storage (Python loop) %s" % kind)


@pytest.mark.parametrize("native", ["0", "1"])
def test_switch_off_keeps_the_refusal(gated, native, monkeypatch):
    """DFOL_GATE_BF16 unset: the two config keys do not combine (the executor has no plan and the Python loop raises), as before."""
    model, ont, names, categories = gated
    qs = questions("exist", 40, 40, names, categories)           # (the batch of the test above: it has relate hops)
    with pytest.raises(_lib.DfolError, match="bf16"):
        forward(model, qs, native, monkeypatch, TableCollater(1, ont, "X"), switch=False)
    # DFOL_GATE_BF16 without DFOL_GATE_NATIVE has no effect: the generic gated route does what it does with neither set, to the bit
    monkeypatch.delenv("DFOL_GATE_NATIVE")
    monkeypatch.setenv("DFOL_NATIVE", native)
    outcome = []
    for value in (None, "1"):
        monkeypatch.delenv("DFOL_GATE_BF16", raising=False) if value is None else monkeypatch.setenv("DFOL_GATE_BF16", value)
        pbs = [pb.to_cuda(DEV) for pb in TableCollater(1, ont, "X").collate([dict(q) for q in qs])]
        _lib.PATH_COUNTS.clear()
        try:
            with torch.no_grad():
                outcome.append(model(pbs, False)["log_probability"].clone())
        except _lib.DfolError as e:
            outcome.append(str(e))
        assert not _lib.PATH_COUNTS.get("relate_one_gate_bf16") and not _lib.PATH_COUNTS.get("native_program")
    a, b = outcome
    assert type(a) is type(b) and (a == b if isinstance(a, str) else torch.equal(a, b)), outcome
    torch.cuda.synchronize()


def test_one_calibrated_batch(tmp_path_factory, monkeypatch):
    model, ont, names, categories = build(tmp_path_factory, True)
    assert model._has_modulator and native_exec.calibrator(model) is not None and native_exec.gate_slots(model)
    qs = questions("verify_rel", 33, 40, names, categories)
    spy = Spy(model, monkeypatch)
    nat, py, counts = both(model, qs, monkeypatch, lambda: _FullCalibrationCollater(1, ont))
    same_results(nat, py, "calibrated gated bf16 tiles")
    assert spy.dtypes and all(d == torch.bfloat16 for d in spy.dtypes) and counts.get("relate_one_gate_bf16", 0) == spy.bf16_calls >= 1
    off, _, _ = forward(model, qs, "1", monkeypatch, _FullCalibrationCollater(1, ont), modulator_switch=False)
    assert not torch.equal(off["log_probability"], nat["log_probability"])        # the calibrator is not the identity
