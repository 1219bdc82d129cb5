"""The table of the fused pair kernel's second-layer forms (_lib.PAIR_KINDS) on the host side (no GPU): its codes against the header,
its wrapper names against the module, the entry points the wrappers name against the header, and the two rules derived from it -
pair_kind_for and pair_tiles_bf16_ok - against expectations written out from the rules they replace."""

import itertools
import os
import re
import types

import pytest
import torch

from dfol_vqa_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfol_vqa.h")).read(), flags=re.S)
KINDS = ("f16x2", "f16", "bf16x3", "packed", "plain")
SHAPES = ((256, 300), (256, 320), (256, 256), (128, 300), (8, 8), (272, 300))          # (HID1, HID2)


def test_codes_are_the_headers():
    assert tuple(_lib.PAIR_KINDS) == KINDS
    defines = {name.lower(): int(value) for name, value in re.findall(r"#define\s+DFOL_PAIR_([A-Z0-9]+)\s+(\d+)", HEADER)}
    assert {k: row.code for k, row in _lib.PAIR_KINDS.items()} == defines


def test_wrappers_exist_and_name_declared_entry_points(monkeypatch):
    """Every pack / launch name is a callable of _lib, and - with the two helpers replaced by recorders - every wrapper hands its helper an
    entry point the header declares, the row's dtype and (launch) a prescale flag that follows the row's units and `uv_prescaled`."""
    declared = set(re.findall(r"\b(dfol_[a-z0-9_]+)\s*\(", HEADER))
    seen = []
    monkeypatch.setattr(_lib, "_pair_pack", lambda entry, dtype, nbytes, w2, hid2: seen.append((entry, dtype)))
    monkeypatch.setattr(_lib, "_pair_ll_image", lambda entry, dtype, scale_uv, *rest: seen.append((entry, dtype, scale_uv, len(rest))))
    monkeypatch.setattr(_lib, "load", lambda: types.SimpleNamespace(dfol_pair_w2_f16x2_bytes=lambda hid1: 0, dfol_pair_w2_f16_bytes=lambda hid1: 0))
    entries = set()
    for kind, row in _lib.PAIR_KINDS.items():
        assert callable(getattr(_lib, row.launch)), kind
        if kind == "plain":
            assert row.pack is None and row.launch == "pair_ll" and not row.bf16_tiles and not row.ln2_units
            continue
        assert callable(getattr(_lib, row.pack)) and row.bf16_tiles, kind
        del seen[:]
        getattr(_lib, row.pack)(torch.zeros(320, 256), 300)
        getattr(_lib, row.launch)(*range(16))
        (pack_entry, pack_dtype), (entry, dtype, scale_uv, n_rest) = seen
        assert pack_entry in declared and entry in declared and pack_dtype == dtype == row.dtype, (kind, seen)
        assert n_rest == 17 and scale_uv == row.ln2_units, (kind, seen)          # (16 positional arguments and default_ll)
        if row.ln2_units:
            del seen[:]
            getattr(_lib, row.launch)(*range(16), uv_prescaled=True)
            assert seen[0][2] is False
        entries |= {pack_entry, entry}
    assert len(entries) == 8


# Read off ClassifierOracle._padded_second_layer as it stood before the table: W2 is packed when HID1 % 16 == 0, HID1 <= 256, HID2 <= 320 and
# DFOL_PAIR_PACKED is not "0", else "plain"; a packed W2 of the split kernels' shapes (HID1 % 32 == 0, 0 < HID1 <= 256, 256 < HID2 <= 320)
# under any arithmetic but "f32" takes that arithmetic's own image, else "packed".
FULL = {"f16x2": "f16x2", "bf16x3": "bf16x3", "f32": "packed", "f16": "f16"}
EXPECTED = {(256, 300): FULL, (256, 320): FULL, (128, 300): FULL,
            (256, 256): dict.fromkeys(FULL, "packed"), (8, 8): dict.fromkeys(FULL, "plain"), (272, 300): dict.fromkeys(FULL, "plain")}


@pytest.mark.parametrize("packed_env", [None, "0"])
def test_pair_kind_for(monkeypatch, packed_env):
    monkeypatch.delenv("DFOL_PAIR_PACKED", raising=False)
    if packed_env is not None:
        monkeypatch.setenv("DFOL_PAIR_PACKED", packed_env)
    assert set(FULL) == set(_lib.PAIR_MATH_MODES)
    for math, (hid1, hid2) in itertools.product(_lib.PAIR_MATH_MODES, SHAPES):
        want = "plain" if packed_env == "0" else EXPECTED[(hid1, hid2)][math]
        assert _lib.pair_kind_for(math, hid1, hid2) == want, (math, hid1, hid2, packed_env)


@pytest.mark.parametrize("packed_env", [None, "0"])
def test_pair_tiles_bf16_ok(monkeypatch, packed_env):
    """Against native_exec.model_spec's expression as it stood before the table."""
    monkeypatch.delenv("DFOL_PAIR_PACKED", raising=False)
    if packed_env is not None:
        monkeypatch.setenv("DFOL_PAIR_PACKED", packed_env)
    for hid1, hid2 in SHAPES:
        want = 256 < hid2 <= 320 and hid1 <= 256 and hid1 % 16 == 0 and os.environ.get("DFOL_PAIR_PACKED", "1") != "0"
        assert _lib.pair_tiles_bf16_ok(hid1, hid2) is want, (hid1, hid2, packed_env)
    assert [s for s in SHAPES if _lib.pair_tiles_bf16_ok(*s)] == ([] if packed_env == "0" else [(256, 300), (256, 320), (128, 300)])
