"""The `pair_math` switch of the fused pair kernel on the host side (no GPU): the config key, and the precedence of a
pair_math_scope over DFOL_PAIR_MATH over the default rule."""

import pytest

from dfol_vqa_amd import _lib


@pytest.fixture()
def no_env(monkeypatch):
    monkeypatch.delenv("DFOL_PAIR_MATH", raising=False)
    monkeypatch.delenv("DFOL_DENSE_MATH", raising=False)
    return monkeypatch


def test_pair_math_config_key(tmp_path):
    """`pair_math: f16x2 | f16` is recorded on the interpreter, an absent key records nothing, anything else is rejected with the allowed
    values in the message."""
    from dfol_vqa_amd import experiment
    from dfol_vqa_amd import synthetic as syn
    paths, _ = syn.write_synthetic_ontology(str(tmp_path))
    cfg = syn.reference_config(paths)
    ont = experiment.build_ontology(cfg)
    assert getattr(experiment.build_model(dict(cfg), ont), "_pair_math", None) is None
    assert experiment.build_model(dict(cfg, pair_math="f16"), ont)._pair_math == "f16"
    assert experiment.build_model(dict(cfg, pair_math="f16x2"), ont)._pair_math == "f16x2"
    for bad in ("bf16", "fp16x3", ""):
        with pytest.raises(ValueError) as err:
            experiment.build_model(dict(cfg, pair_math=bad), ont)
        assert "f16x2" in str(err.value) and "f16 " in str(err.value)
    # mlp_math: bf16 does not imply the reduced pair mode
    assert getattr(experiment.build_model(dict(cfg, mlp_math="bf16"), ont), "_pair_math", None) is None


def test_absent_key_keeps_todays_rule(no_env):
    """Without scope and environment variable: bf16x3 follows the dense math, every other dense mode (bf16 included) keeps f16x2."""
    assert _lib.pair_math() == "f16x2"
    for dense, want in (("f16x2", "f16x2"), ("bf16x3", "bf16x3"), ("f32", "f16x2"), ("bf16", "f16x2")):
        with _lib.dense_math(dense):
            assert _lib.pair_math() == want, dense
            with _lib.pair_math_scope(None):                     # (a model without the key enters the scope with None: no change)
                assert _lib.pair_math() == want, dense


def test_precedence_scope_over_environment_over_default(no_env):
    no_env.setenv("DFOL_PAIR_MATH", "f16")
    assert _lib.pair_math() == "f16"                             # the environment variable is accepted ...
    with _lib.dense_math("bf16x3"):
        assert _lib.pair_math() == "f16"                         # ... and beats the rule
    with _lib.pair_math_scope("f16x2"):
        assert _lib.pair_math() == "f16x2"                       # a scope beats the environment
        with _lib.pair_math_scope("f16"):
            assert _lib.pair_math() == "f16"
            with _lib.pair_math_scope(None):
                assert _lib.pair_math() == "f16"
        assert _lib.pair_math() == "f16x2"                       # scopes nest and restore
    assert _lib.pair_math() == "f16"
    no_env.setenv("DFOL_PAIR_MATH", "bf16x3")
    with _lib.pair_math_scope("f16"):
        assert _lib.pair_math() == "f16"
    no_env.delenv("DFOL_PAIR_MATH")
    with _lib.pair_math_scope("f16"):
        with _lib.dense_math("bf16"):
            assert _lib.pair_math() == "f16"
    assert _lib.pair_math() == "f16x2"


def test_unknown_modes_are_refused(no_env):
    with pytest.raises(_lib.DfolError):
        _lib.pair_math_scope("fp8")
    no_env.setenv("DFOL_PAIR_MATH", "f8")
    with pytest.raises(_lib.DfolError) as err:
        _lib.pair_math()
    assert "f16x2" in str(err.value) and "f16:" in str(err.value)


def test_scope_restores_after_an_exception(no_env):
    with pytest.raises(RuntimeError):
        with _lib.pair_math_scope("f16"):
            raise RuntimeError("x")
    assert _lib.pair_math() == "f16x2"
