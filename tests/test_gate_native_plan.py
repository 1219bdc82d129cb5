"""Host logic of the gated model on the native executor (DFOL_GATE_NATIVE=1) - no GPU: a gated spec lowers to the gated
opcodes, every instruction names the gates of the cell the Python loop runs for that operator, the subject flags travel in the blob, and with
the switch unset the interpreter announces the fallback as before.  The executor itself is compared with the Python loop on the GPU
(tests/test_gate_native_gpu.py)."""

import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import _lib, native_exec  # noqa: E402
from dfol_vqa_amd import native_plan as NP  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from test_native_plan import KINDS, FeatureCollater  # noqa: E402

UNGATED = (NP.OP_FILTER, NP.OP_RELATE_ONE, NP.OP_RELATE)
GATED = (NP.OP_FILTER_GATE, NP.OP_RELATE_ONE_GATE, NP.OP_RELATE_GATE)
SLOT_AT = {NP.OP_FILTER_GATE: 8, NP.OP_RELATE_ONE_GATE: 13, NP.OP_RELATE_GATE: 15}


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """A gated and an ungated model on the CPU (reduced widths: only the modules matter here), the ontology, and the two specs."""
    from dfol_vqa_amd import experiment
    paths, names = syn.write_synthetic_ontology(str(tmp_path_factory.mktemp("gate_plan")))
    with open(paths["attribute_file"]) as f:
        categories = json.load(f)
    models = {}
    for gated in (False, True):
        cfg = syn.reference_config(paths, trainable_gate=gated, box_features_dim=16, oracle_input_dim=12, attribute_network_layers_config=[8],
                                   relation_network_layers_config=[8])
        ont = experiment.build_ontology(cfg)
        models[gated] = experiment.build_model(cfg, ont).eval()
    slots = native_exec.gate_slots(models[True])
    spec = lambda gates, **kw: NP.ModelSpec([12], [8, 300], 8, 16, True, 0.0, ont._relation_index, gates=gates, **kw)
    return ont, names, categories, models, slots, spec


def plan_of(ont, spec, qs):
    for q in qs:
        q["scene"]["X"] = q["scene"]["X"][:, -22:]
    pbs = FeatureCollater(1, ont, spec).collate(qs)
    assert len(pbs) == 1
    return pbs[0], pbs[0]._native_plan


def test_gate_slots_follow_the_modules(setup):
    ont, names, categories, models, slots, spec = setup
    assert native_exec.gate_slots(models[False]) is None
    model = models[True]
    cells = native_exec.gated_cells(model)
    # every gated cell of the model has a slot, in named_modules() order, a relate cell owns two rows
    assert [p for p, _ in cells] == [n[:-len("._blc")] for n, m in model.named_modules() if n.endswith("._blc")]
    at = 0
    for path, cell in cells:
        assert slots[path] == at and model.get_submodule(path)._blc is cell
        at += cell._arity
    assert at == sum(1 for k in model.state_dict() if k.endswith("._linear.weight") and "_nlg" in k)
    for path in ("_ops.select._filter", "_ops.filter._filter", "_ops.relate._gqa_select._filter", "_ops.relate._relate", "_ops.verify_attrs._filter",
                 "_ops.choose_rel._gqa_select._filter", "_ops.choose_rel._relate", "_ops.verify_rel._gqa_relate._gqa_select._filter",
                 "_ops.verify_rel._gqa_relate._relate", "_ops.query_attr._gqa_choose_attr._filter", "_ops.all_different._gqa_all_same._filter",
                 "_ops.two_different._gqa_two_same._filter", "_ops.compare._filter"):
        assert path in slots, path
    assert len(set(slots.values())) == len(slots)


@pytest.mark.parametrize("kind", KINDS)
def test_gated_spec_emits_gated_opcodes_only(setup, kind):
    ont, names, categories, models, slots, spec = setup
    qs = syn.full_size_questions(kind, 7, 5, 12, names, categories, 3 + KINDS.index(kind))
    _, plan = plan_of(ont, spec(slots), qs)
    assert isinstance(plan, NP.NativePlan), kind
    ops = [int(x) for x in plan.instrs[:, 0]]
    assert not any(o in UNGATED for o in ops) and any(o in GATED for o in ops), (kind, ops)
    n_gates = max(slots.values()) + 2
    for row in plan.instrs:
        at = SLOT_AT.get(int(row[0]))
        if at is not None:
            arity = 1 if int(row[0]) == NP.OP_FILTER_GATE else 2
            assert 0 <= row[at] and row[at] + arity <= n_gates, row
    # the same batch under the ungated spec: the same launches with the ungated opcodes, nothing else moved
    _, plain = plan_of(ont, spec(None), syn.full_size_questions(kind, 7, 5, 12, names, categories, 3 + KINDS.index(kind)))
    back = {g: u for g, u in zip(GATED, UNGATED)}
    assert [back.get(o, o) for o in ops] == [int(x) for x in plain.instrs[:, 0]]
    assert plan.key != plain.key


def gated_rows(plan):
    return [row for row in plan.instrs if int(row[0]) in GATED]


def test_every_instruction_names_its_operators_own_cell(setup):
    ont, names, categories, models, slots, spec = setup
    nouns, attrs, rels = names["nouns"][:4], names["attributes"][:4], names["relations"][:3]
    S = lambda path: slots["_ops." + path]
    # select -> filter -> relate (subject flags MIXED over the batch) -> verify_attrs
    flags = [True, False, False, True, True]
    qs = [syn.question(i, [[syn.op("select", nouns[i % 4]), syn.op("filter", attrs[i % 4]), syn.op("relate", rels[i % 3], flags[i], nouns[(i + 1) % 4])]],
                       syn.op("verify_attrs", [attrs[0], attrs[1]]), "yes", syn.feature_scene(i, 3 + i, 16)) for i in range(5)]
    pb, plan = plan_of(ont, spec(slots), qs)
    rows = gated_rows(plan)
    assert [(int(r[0]), int(r[SLOT_AT[int(r[0])]])) for r in rows] == [
        (NP.OP_FILTER_GATE, S("select._filter")), (NP.OP_FILTER_GATE, S("filter._filter")), (NP.OP_FILTER_GATE, S("relate._gqa_select._filter")),
        (NP.OP_RELATE_ONE_GATE, S("relate._relate")), (NP.OP_FILTER_GATE, S("verify_attrs._filter"))]
    rel = rows[3]
    assert int(rel[11]) == NP.TILE_F32 and rel[12] >= 0 and rel[12] % 16 == 0
    assert list(plan.blob[int(rel[12]):int(rel[12]) + 5]) == [1 if f else 0 for f in flags]        # x_is_subject = the program's flags
    program_flags = [op for op in pb._op_batch_list if op._op_name == "relate"][0]._arguments[1]
    assert [1 if f else 0 for f in program_flags] == [1 if f else 0 for f in flags]
    # select -> choose_rel: its own select's filter, and the generic two-posterior cell of ITS RelateBatch
    qs = [syn.question(10 + i, [[syn.op("select", nouns[i % 4])]], syn.op("choose_rel", [rels[0], rels[1]], bool(i % 2), nouns[(i + 2) % 4]), "yes",
                       syn.feature_scene(10 + i, 4 + i, 16)) for i in range(3)]
    rows = gated_rows(plan_of(ont, spec(slots), qs)[1])
    assert [(int(r[0]), int(r[SLOT_AT[int(r[0])]])) for r in rows] == [
        (NP.OP_FILTER_GATE, S("select._filter")), (NP.OP_FILTER_GATE, S("choose_rel._gqa_select._filter")), (NP.OP_RELATE_GATE, S("choose_rel._relate"))]
    # select -> verify_rel: the second operator that holds a relate
    qs = [syn.question(20 + i, [[syn.op("select", nouns[i % 4])]], syn.op("verify_rel", rels[i % 3], bool(i % 2), nouns[(i + 1) % 4]), "yes",
                       syn.feature_scene(20 + i, 4 + i, 16)) for i in range(3)]
    rows = gated_rows(plan_of(ont, spec(slots), qs)[1])
    assert [(int(r[0]), int(r[SLOT_AT[int(r[0])]])) for r in rows] == [
        (NP.OP_FILTER_GATE, S("select._filter")), (NP.OP_FILTER_GATE, S("verify_rel._gqa_relate._gqa_select._filter")),
        (NP.OP_RELATE_ONE_GATE, S("verify_rel._gqa_relate._relate"))]
    assert S("verify_rel._gqa_relate._relate") != S("relate._relate") != S("choose_rel._relate")


def test_spec_key_and_bf16(setup):
    ont, names, categories, models, slots, spec = setup
    assert spec(slots).key() != spec(None).key()
    moved = dict(slots)
    a, b = "_ops.select._filter", "_ops.filter._filter"
    moved[a], moved[b] = moved[b], moved[a]
    assert spec(moved).key() != spec(slots).key()                 # the map itself is part of the key
    # bf16 tiles and gates do not combine: no plan (the Python loop raises the DfolError of the combination)
    qs = syn.full_size_questions("verify_rel", 3, 8, 8, names, categories, 14)
    assert plan_of(ont, spec(slots, tile_bf16=True), qs)[1] is None
    qs = syn.full_size_questions("verify_rel", 3, 8, 8, names, categories, 14)
    assert isinstance(plan_of(ont, spec(None, tile_bf16=True), qs)[1], NP.NativePlan)
    # a model whose cell the plan names is missing from the map steps aside instead of running another cell's gates
    short = {k: v for k, v in slots.items() if k != "_ops.verify_rel._gqa_relate._relate"}
    qs = syn.full_size_questions("verify_rel", 3, 8, 8, names, categories, 14)
    assert plan_of(ont, spec(short), qs)[1] is None


def test_switch_unset_keeps_the_fallback(setup, monkeypatch):
    ont, names, categories, models, slots, spec = setup
    monkeypatch.delenv("DFOL_GATE_NATIVE", raising=False)
    monkeypatch.setenv("DFOL_NATIVE", "1")
    assert not _lib.gate_native()
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        assert models[True]._native_spec(False, True, False) is None
    assert _lib.PATH_COUNTS.get("fallback:trainable_gate", 0) == 1
    for value, on in (("0", False), ("1", True)):
        monkeypatch.setenv("DFOL_GATE_NATIVE", value)             # read when the forward starts
        assert _lib.gate_native() is on
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        models[True]._native_spec(False, True, False)
    assert not _lib.PATH_COUNTS.get("fallback:trainable_gate")    # switched on: no fallback is announced
    monkeypatch.delenv("DFOL_GATE_NATIVE")
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        models[False]._native_spec(False, True, False)
    assert not _lib.PATH_COUNTS.get("fallback:trainable_gate")    # an ungated model never does
