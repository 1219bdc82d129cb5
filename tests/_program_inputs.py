"""What the no-device tests of dfol_run_program's inputs share: the header's struct fields by name, and an EMPTY program (n_instr = 0: nothing is
launched, no device is touched) run over a real ProgramModel / ProgramScene with the fields under test set."""

import ctypes
import os
import re

from dfol_vqa_amd import _lib, native_exec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("DFOL_FEATURES_MATRIX", "DFOL_FEATURES_ROWS_F32", "DFOL_FEATURES_ROWS_BF16", "DFOL_FEATURES_ROWS_BF16_H2", "DFOL_FEATURES_ROWS_BF16_H2_F16",
         "DFOL_FEATURES_CACHED")


def header():
    with open(os.path.join(ROOT, "include", "dfol_vqa.h")) as f:
        return f.read()


def header_fields(struct):
    """The field names of `typedef struct { ... } <struct>;` in the header's order."""
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    body = text[:text.index("} %s;" % struct)].rsplit("typedef struct {", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if decl:
            first, rest = decl.split(",")[0], decl.split(",")[1:]
            names += [re.sub(r"\[\d+\]", "", n.strip().lstrip("*")) for n in [first.replace("*", " ").split()[-1]] + rest]
    return names


def assert_forms_and_layout():
    """The header declares the six DFOL_FEATURES_* constants with native_exec's values, and both ctypes structs carry the header's fields in order."""
    text = header()
    for value, name in enumerate(FORMS):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
        assert getattr(native_exec, name[len("DFOL_"):]) == value, name
    for struct, mirror in (("DfolProgramScene", native_exec.ProgramScene), ("DfolProgramModel", native_exec.ProgramModel)):
        assert [n for n, _ in mirror._fields_] == header_fields(struct), struct
    assert [n for n, _ in native_exec.ProgramScene._fields_][-6:] == ["feature_form", "src_row", "box6", "cache", "ld_cache", "cache_cols"]
    assert [n for n, _ in native_exec.ProgramModel._fields_][-2:] == ["gates", "n_gates"]


def run_empty(model=(), **scene):
    """-> (return code, dfol_last_error()) of an empty program over a scene with `scene`'s fields and a model with `model`'s (a dict); the
    instruction table, blob and workspace are fake non-null addresses that an empty program never reads."""
    h = _lib.load()
    m, sc = native_exec.ProgramModel(), native_exec.ProgramScene()
    sc.NS = 4
    for k, v in dict(model).items():
        setattr(m, k, v)
    for k, v in scene.items():
        setattr(sc, k, v)
    rc = h.dfol_run_program(ctypes.byref(m), ctypes.byref(sc), 8, 0, 8, 8, None)
    return rc, h.dfol_last_error()
