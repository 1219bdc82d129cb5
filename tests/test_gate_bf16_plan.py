"""Host logic of the gated model over bf16 relation tiles (DFOL_GATE_NATIVE=1 with DFOL_GATE_BF16=1) - no GPU: the spec
field that lets gates and `tile_bf16` combine, the gated one-posterior opcode carrying the bf16 tile dtype over a half-size tile workspace,
the batches that keep fp32 tiles, the switch, and the entry point's argument checks (none of which touches a device).  The kernel and the
routes are compared on the GPU (tests/test_gate_bf16_gpu.py, tests/test_gate_bf16_route_gpu.py)."""

import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import _lib  # noqa: E402
from dfol_vqa_amd import native_plan as NP  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from test_gate_native_plan import plan_of, setup  # noqa: E402,F401  (the gated / ungated CPU models, the slots and the spec factory)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dfol_relate_one_gate_fwd_bf16"


def questions(names, categories, kind, n_list, seed=14):
    qs = syn.full_size_questions(kind, len(n_list), 5, 9, names, categories, seed)
    for q, n in zip(qs, n_list):
        q["scene"] = {"n": n, "X": syn.feature_scene(q["question_id"], n, 16)["X"]}
    return qs


def rows_of(plan, opcode):
    return [row for row in plan.instrs if int(row[0]) == opcode]


def test_on_spec_lowers_to_the_gated_opcode_over_bf16_tiles(setup):
    ont, names, categories, models, slots, spec = setup
    n_list = [16, 5, 11]                                          # NS = 16
    on = plan_of(ont, spec(slots, tile_bf16=True, gate_bf16=True), questions(names, categories, "verify_rel", n_list))[1]
    assert isinstance(on, NP.NativePlan)
    rel = rows_of(on, NP.OP_RELATE_ONE_GATE)
    assert len(rel) >= 1 and all(int(r[11]) == NP.TILE_BF16 for r in rel)
    assert not rows_of(on, NP.OP_RELATE_ONE) and not rows_of(on, NP.OP_RELATE_GATE) and not rows_of(on, NP.OP_RELATE)
    pair = rows_of(on, NP.OP_PAIR_LL)
    assert len(pair) == 1 and int(pair[0][11]) == NP.TILE_BF16    # the pair kernel writes what the relate reads
    # the tile workspace: NS * NS / 2 words per predicate, filled with two bf16 -30 per word; the fp32 plan of the same batch holds twice that
    NS, preds = 16, sum(int(r[8]) for r in rel)
    fills = [r for r in rows_of(on, NP.OP_FILL) if int(r[3]) == NP._NEG30_BF16X2]
    assert len(fills) == 1 and int(fills[0][2]) == preds * NS * NS // 2
    f32 = plan_of(ont, spec(slots), questions(names, categories, "verify_rel", n_list))[1]
    rel32 = rows_of(f32, NP.OP_RELATE_ONE_GATE)
    assert [int(r[8]) for r in rel32] == [int(r[8]) for r in rel] and all(int(r[11]) == NP.TILE_F32 for r in rel32)
    assert sorted(int(r[2]) for r in rows_of(f32, NP.OP_FILL))[-1] == preds * NS * NS
    assert [int(x) for x in on.instrs[:, 0]] == [int(x) for x in f32.instrs[:, 0]]      # nothing else moved
    # the gate slots and the subject flags are the fp32 plan's
    assert [(int(r[12]) >= 0, int(r[13])) for r in rel] == [(int(r[12]) >= 0, int(r[13])) for r in rel32]


def test_field_off_yields_no_plan_and_the_keys_differ(setup):
    ont, names, categories, models, slots, spec = setup
    off, on = spec(slots, tile_bf16=True), spec(slots, tile_bf16=True, gate_bf16=True)
    assert off.gate_bf16 is False and on.gate_bf16 is True
    assert plan_of(ont, off, questions(names, categories, "verify_rel", [8, 8, 8]))[1] is None
    assert plan_of(ont, spec(slots, tile_bf16=True, gate_bf16=False), questions(names, categories, "verify_rel", [8, 8, 8]))[1] is None
    assert off.key() != on.key()
    assert spec(slots, gate_bf16=True).key() != spec(slots).key()
    plan = plan_of(ont, on, questions(names, categories, "verify_rel", [8, 8, 8]))[1]
    assert isinstance(plan, NP.NativePlan) and plan.key == on.key()


def test_batches_that_keep_fp32_tiles(setup):
    ont, names, categories, models, slots, spec = setup
    on = spec(slots, tile_bf16=True, gate_bf16=True)
    # NS = 12: not a multiple of 8
    plan = plan_of(ont, on, questions(names, categories, "verify_rel", [9, 5, 12]))[1]
    rel = rows_of(plan, NP.OP_RELATE_ONE_GATE)
    assert len(rel) >= 1 and all(int(r[11]) == NP.TILE_F32 for r in rel)
    assert all(int(r[11]) == NP.TILE_F32 for r in rows_of(plan, NP.OP_PAIR_LL))
    # a choose_rel in the batch (NS = 8): the two-posterior gated cell, fp32 tiles throughout
    plan = plan_of(ont, on, questions(names, categories, "choose_rel", [8, 5, 7]))[1]
    assert isinstance(plan, NP.NativePlan) and len(rows_of(plan, NP.OP_RELATE_GATE)) >= 1
    assert all(int(r[11]) == NP.TILE_F32 for r in rows_of(plan, NP.OP_PAIR_LL) + rows_of(plan, NP.OP_RELATE_ONE_GATE))
    assert not [r for r in rows_of(plan, NP.OP_FILL) if int(r[3]) == NP._NEG30_BF16X2]


def test_the_switch_needs_both_variables(monkeypatch):
    for native, bf16, want in ((None, None, False), ("1", None, False), (None, "1", False), ("1", "0", False), ("0", "1", False), ("1", "1", True)):
        for k, v in (("DFOL_GATE_NATIVE", native), ("DFOL_GATE_BF16", bf16)):
            monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)
        assert _lib.gate_bf16() is want, (native, bf16)           # read when asked: no import-time state


def test_model_spec_takes_the_field_from_the_switch(setup, monkeypatch):
    ont, names, categories, models, slots, spec = setup
    assert spec(slots).gate_bf16 is False                         # default off
    src = open(os.path.join(ROOT, "dfol_vqa_amd", "native_exec.py")).read()
    assert re.search(r"gate_bf16\s*=\s*_lib\.gate_bf16\(\)", src)


@pytest.fixture(scope="module")
def handle():
    import __graft_entry__ as g
    g.build()
    return _lib.load()


def test_entry_point_is_exported_declared_and_bound(handle):
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfol_vqa.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, text, flags=re.S)
    assert m and "const uint16_t* tile" in m.group(1)
    assert len(_lib.SIGNATURES[NAME]) == len(_lib.SIGNATURES["dfol_relate_one_gate_fwd_f32"]) == len(m.group(1).split(","))
    assert handle.dfol_abi_version() == 4 == _lib.ABI_VERSION      # (the entry point itself was a pure addition under 3)


def test_entry_point_refuses_bad_sizes_without_a_device(handle):
    fn = getattr(handle, NAME)
    args = lambda P, NS: (None, None, None, None, None, None, None, None, 0, None, P, NS, 0, None, None, None, None)
    for NS in (12, 264, 0, 4):
        assert fn(*args(3, NS)) != 0 and b"relate_one_gate_fwd_bf16" in handle.dfol_last_error(), NS
    assert fn(*args(0, 16)) == 0                                  # P == 0: nothing to do, before any pointer is looked at
    assert fn(*args(3, 16)) != 0 and b"null pointer" in handle.dfol_last_error()


def test_wrapper_refusals_before_any_launch():
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)

    def run(tile, flags=3):
        P, NS = tile.shape[0], tile.shape[1]
        return _lib.relate_one_gate_fwd_bf16(z(P, NS), z(P, NS), tile, z(P, dt=torch.int32), z(P, dt=torch.int32), z(P), z(flags, dt=torch.uint8),
                                             z(18), z(18))

    with pytest.raises(_lib.DfolError, match="bfloat16"):
        run(z(3, 16, 16))                                         # an fp32 tile
    with pytest.raises(_lib.DfolError, match="NS=12"):
        run(z(3, 12, 12, dt=torch.bfloat16))
    with pytest.raises(_lib.DfolError, match="NS=264"):
        run(z(3, 264, 264, dt=torch.bfloat16))
    with pytest.raises(_lib.DfolError, match="subject flags"):
        run(z(3, 16, 16, dt=torch.bfloat16), flags=2)
    with pytest.raises(_lib.DfolError):                           # the fp32 wrappers keep refusing a bf16 tile
        _lib.relate_one_gate_fwd(z(3, 16), z(3, 16), z(3, 16, 16, dt=torch.bfloat16), z(3, dt=torch.int32), z(3, dt=torch.int32), z(3),
                                 z(3, dt=torch.uint8), z(18), z(18))
    from dfol_vqa_amd import ops
    assert ops.relate_one_gate_fwd_bf16 is _lib.relate_one_gate_fwd_bf16 and ops.gate_bf16 is _lib.gate_bf16

