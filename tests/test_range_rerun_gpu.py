"""`range_overflow: rerun` (interpreter.range_rerun): an inference forward that left fp16's range in the default two-piece fp16 arithmetic is run
again on "bf16x3" - dense layers and pair kernel - instead of raising.  The yardstick throughout is what the SAME model returns for the SAME batch
with `mlp_math: bf16x3` under the default `raise`: bit for bit (the re-run is that forward), and for the overflowing batch against the oracle.
Through forward, forward_async().result(), GraphedForward.__call__ / submit + collect and ReplayLanes, with the executor on and off."""

import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
from dfol_vqa_amd import _lib  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402
from oracle import dfol_oracle as orc  # noqa: E402
from test_interpreter_gpu import DEV, TableCollater  # noqa: E402

gpu = pytest.mark.gpu
KINDS = ["exist", "verify_rel"]                                  # (verify_rel: the terminal operator itself reads relation tiles)
SEED = 21


@pytest.fixture(scope="module")
def full(tmp_path_factory):
    from dfol_vqa_amd import experiment
    d = str(tmp_path_factory.mktemp("range_rerun"))
    paths, names = syn.write_synthetic_ontology(d)
    cfg = syn.reference_config(paths)
    ont = experiment.build_ontology(cfg)
    model = experiment.build_model(cfg, ont)
    syn.load_seeded_weights(model, 23)
    with open(paths["attribute_file"]) as f:
        categories = json.load(f)
    oont = orc.Ontology(paths["attribute_file"], paths["class_file"], paths["vocabulary_file"], paths["relation_file"])
    return model.to(DEV).eval(), ont, oont, names, categories


def questions(full, kind, edit=None):
    """Four ragged 10..20-object questions; edit: the value of feature 100 of object 3 of question 1 (1e5: beyond fp16; NaN: beyond everything)."""
    qs = syn.full_size_questions(kind, 4, 10, 20, full[3], full[4], SEED)
    if edit is not None:
        qs = [dict(q, scene=dict(q["scene"], X=q["scene"]["X"].copy())) for q in qs]
        qs[1]["scene"]["X"][3, 100] = edit
    return qs


def upload(full, qs):
    return [pb.to_cuda(DEV) for pb in TableCollater(1, full[1], "X").collate([dict(q) for q in qs])]


class mode(object):
    """with mode(model, _range_overflow="rerun", ...): the model's switches inside the block, put back on the way out."""

    def __init__(self, model, **kw):
        self.model, self.kw = model, kw

    def __enter__(self):
        self.saved = {k: (k in self.model.__dict__, self.model.__dict__.get(k)) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.model, k, v)

    def __exit__(self, *exc):
        for k, (had, v) in self.saved.items():
            if had:
                self.model.__dict__[k] = v
            else:
                self.model.__dict__.pop(k, None)
        return False


def snapshot(res):
    """A result dict, detached from whatever the next forward or replay refills."""
    return {"log_probability": res["log_probability"].detach().cpu().clone(), "answer": [list(a) if isinstance(a, list) else a for a in res["answer"]],
            "answer_log_probability": [list(a) if isinstance(a, list) else a for a in res["answer_log_probability"]], "type": res["type"],
            "keys": sorted(k for k in res if not k.startswith("_")), "dtype": res["log_probability"].dtype}


def same(got, want, what):
    got = snapshot(got)
    assert torch.equal(got["log_probability"], want["log_probability"]), (what, got["log_probability"], want["log_probability"])
    assert got["answer"] == want["answer"] and got["answer_log_probability"] == want["answer_log_probability"], what
    assert got["keys"] == want["keys"] and got["dtype"] == want["dtype"] and int(got["type"]) == int(want["type"]), what


_REF = {}


def reference(model, pbs, key, math):
    """The model's plain forward (`raise`) of the batch in dense arithmetic `math` (None: the default), computed once per key and left alone."""
    key = key + (math, os.environ.get("DFOL_NATIVE", "1"))
    if key not in _REF:
        with mode(model, _range_overflow="raise", _mlp_math=math), torch.no_grad():
            _REF[key] = snapshot(model(pbs, False))
    return _REF[key]


def reruns():
    return _lib.PATH_COUNTS.get("range_rerun", 0)


def entry(model, pbs, how):
    with torch.no_grad():
        return model(pbs, False) if how == "forward" else model.forward_async(pbs, False).result()


@gpu
@pytest.mark.parametrize("how", ["forward", "forward_async"])
@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("kind", KINDS)
def test_rerun_returns_the_wide_range_answer(full, kind, native, how, monkeypatch):
    """A feature of 1e5 (the batch test_fp16_range_overflow_raises_instead_of_nan raises for): under `rerun` the forward returns, finite and bit
    for bit, what the model returns for that batch with `mlp_math: bf16x3`; one re-run is counted (and announced) per forward; the clean batch
    before and after is what it is under `raise`, with no re-run."""
    model = full[0]
    monkeypatch.setenv("DFOL_NATIVE", native)
    good, bad = upload(full, questions(full, kind)), upload(full, questions(full, kind, 1.0e5))
    clean = reference(model, good, (kind, "good"), None)
    wide = reference(model, bad, (kind, "bad"), "bf16x3")
    assert bool(torch.isfinite(wide["log_probability"]).all())
    _lib._WARNED.discard("range_rerun")
    with mode(model, _range_overflow="rerun"):
        n0 = reruns()
        same(entry(model, good, how), clean, "clean before")
        assert reruns() == n0
        with pytest.warns(RuntimeWarning, match="range_rerun.*fp16 range exceeded"):
            got = entry(model, bad, how)
        assert reruns() == n0 + 1 and _lib.PATH_COUNTS["fallback:range_rerun"] >= 1
        assert bool(torch.isfinite(got["log_probability"]).all())
        same(got, wide, "bad batch")
        same(entry(model, bad, how), wide, "bad batch again")
        assert reruns() == n0 + 2
        same(entry(model, good, how), clean, "clean after")
        assert reruns() == n0 + 2
        assert "_mlp_math" not in model.__dict__ or model.__dict__["_mlp_math"] is None      # (the re-run's modes do not outlive it)
    with pytest.raises(_lib.DfolError, match="fp16 range"):       # the switch, not the code around it: `raise` still raises
        entry(model, bad, how)


class saturating(object):
    """The model of test_pair_kernel_saturation_raises: first relation layer weight and bias x 1e6 inside the block (first-layer sums of ~3e5)."""

    def __init__(self, model):
        from torch import nn
        self.lin1 = [m for m in model._oracle._relation_network._network if isinstance(m, nn.Linear)][0]

    def __enter__(self):
        with torch.no_grad():
            self.saved = self.lin1.weight.clone(), self.lin1.bias.clone()
            self.lin1.weight.mul_(1.0e6)
            self.lin1.bias.mul_(1.0e6)

    def __exit__(self, *exc):
        with torch.no_grad():
            self.lin1.weight.copy_(self.saved[0])
            self.lin1.bias.copy_(self.saved[1])
        return False


@gpu
@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("kind", KINDS)
def test_rerun_recovers_a_saturated_pair_kernel(full, kind, native, monkeypatch):
    """DFOL_RANGE_PAIR_SATURATED: the saturating model under `rerun` returns what an explicit bf16x3 forward of it returns; the unscaled model
    afterwards is bit-equal to before."""
    model = full[0]
    monkeypatch.setenv("DFOL_NATIVE", native)
    pbs = upload(full, questions(full, kind))
    clean = reference(model, pbs, (kind, "good"), None)
    with saturating(model):
        with mode(model, _range_overflow="raise", _mlp_math="bf16x3"), torch.no_grad():
            wide = snapshot(model(pbs, False))
        with mode(model, _range_overflow="rerun"):
            n0 = reruns()
            for how in ("forward", "forward_async"):
                same(entry(model, pbs, how), wide, "saturated " + how)
            assert reruns() == n0 + 2
    with mode(model, _range_overflow="rerun"):
        n0 = reruns()
        same(entry(model, pbs, "forward"), clean, "unscaled afterwards")
        assert reruns() == n0


@gpu
@pytest.mark.parametrize("native", ["1", "0"])
def test_rerun_forces_the_pair_scope(full, native, monkeypatch):
    """`pair_math: f16` on the saturating model: the one-product kernel saturates as the default does, and a re-run that left the model's pair
    mode in place would saturate again (and raise).  The re-run sets the pair arithmetic itself: no error, the explicit bf16x3 result."""
    model = full[0]
    monkeypatch.setenv("DFOL_NATIVE", native)
    pbs = upload(full, questions(full, "verify_rel"))
    with saturating(model):
        with mode(model, _range_overflow="raise", _mlp_math="bf16x3"), torch.no_grad():
            wide = snapshot(model(pbs, False))
        with mode(model, _pair_math="f16"):
            with pytest.raises(_lib.DfolError, match="saturation"):
                entry(model, pbs, "forward")
            with mode(model, _range_overflow="rerun"):
                n0 = reruns()
                same(entry(model, pbs, "forward"), wide, "pair_math f16")
                assert reruns() == n0 + 1
            assert model._pair_math == "f16"


def oracle_runs(full, qs):
    model, oont = full[0], full[2]
    weights = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items() if k.startswith("_featurizer.") or k.startswith("_oracle.")}
    plain = [{k: v for k, v in q.items() if k != "scene"} for q in qs]
    scenes = [q["scene"] for q in qs]
    return (orc.run_questions(oont, plain, scenes, np.float32, weights=weights),
            orc.run_questions(oont, plain, scenes, np.float64, weights=weights))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_rerun_agrees_with_the_oracle(full, kind):
    """The overflowing batch's re-run against the oracle in fp32 and fp64 on the same inputs (the reference accepts any fp32 feature), at
    check_logprob's defaults; answers as the fp64 oracle's."""
    model = full[0]
    qs = questions(full, kind, 1.0e5)
    r32, r64 = oracle_runs(full, qs)
    assert np.all(np.isfinite(r32["log_probability"])) and np.all(np.isfinite(r64["log_probability"]))
    with mode(model, _range_overflow="rerun"):
        n0 = reruns()
        got = entry(model, upload(full, qs), "forward")
        assert reruns() == n0 + 1
    gu.check_logprob(got["log_probability"].cpu().numpy(), r32["log_probability"], r64["log_probability"], "rerun " + kind)


@gpu
@pytest.mark.parametrize("how", ["forward", "forward_async"])
def test_unrecoverable_input_still_raises(full, how):
    """A NaN feature is beyond every arithmetic: the re-run's log-probabilities are not finite, and the forward raises today's text plus a note
    that the re-run did not help.  The next clean batch is what it always was."""
    model = full[0]
    good, bad = upload(full, questions(full, "exist")), upload(full, questions(full, "exist", float("nan")))
    clean = reference(model, good, ("exist", "good"), None)
    with mode(model, _range_overflow="rerun"):
        n0 = reruns()
        with pytest.raises(_lib.DfolError, match="fp16 range exceeded.*did not help"):
            entry(model, bad, how)
        assert reruns() == n0 + 1
        same(entry(model, good, how), clean, "clean after NaN")
        assert reruns() == n0 + 1


def put(pbs, src):
    for pb, s in zip(pbs, src):
        pb._object_features.copy_(s._object_features)


@gpu
def test_graph_replay_reruns_eagerly(full):
    """A GraphedForward captured over the clean batch; the overflowing features copied into its ProgramBatches: __call__ and submit + collect return
    the explicit bf16x3 result of those features (collect: log-probabilities on the host), the clean features copied back replay bit-equal to the
    first replay.  Two replays in flight, the flagged one first and clean features copied in behind it: its features are gone, collect raises and
    says why; the second ticket returns the clean result."""
    from dfol_vqa_amd.interpreter import GraphedForward
    model = full[0]
    good, bad = upload(full, questions(full, "verify_rel")), upload(full, questions(full, "verify_rel", 1.0e5))
    pbs = upload(full, questions(full, "verify_rel"))
    wide = reference(model, bad, ("verify_rel", "bad"), "bf16x3")
    with mode(model, _range_overflow="rerun"):
        g = GraphedForward(model, pbs)
        res = g()
        first = snapshot(res)
        same(res, reference(model, good, ("verify_rel", "good"), None), "first replay")
        n0 = reruns()
        put(pbs, bad)
        same(g(), wide, "__call__")
        got = g.collect(g.submit())
        assert got["log_probability"].device.type == "cpu"
        same(got, wide, "submit + collect")
        assert reruns() == n0 + 2
        put(pbs, good)
        same(g(), first, "clean features back")
        got = g.collect(g.submit())
        assert got["log_probability"].device.type == "cpu"
        same(got, first, "clean features back, collect")
        assert reruns() == n0 + 2
        put(pbs, bad)
        t0 = g.submit(depth=2)
        put(pbs, good)
        t1 = g.submit(depth=2)
        with pytest.raises(_lib.DfolError, match="fp16 range exceeded.*later submit"):
            g.collect(t0)
        same(g.collect(t1), first, "the ticket behind the flagged one")
        assert reruns() == n0 + 2


@gpu
def test_lanes_rerun_their_own_batch(full):
    """ReplayLanes of two lanes: overflowing features on lane 0, clean ones on lane 1.  Each collect returns its own batch's result - lane 0 the
    bf16x3 result, lane 1 bit-equal to the clean reference - and one re-run is counted."""
    from dfol_vqa_amd.interpreter import ReplayLanes
    model = full[0]
    good, bad = upload(full, questions(full, "verify_rel")), upload(full, questions(full, "verify_rel", 1.0e5))
    clean = reference(model, good, ("verify_rel", "good"), None)
    wide = reference(model, bad, ("verify_rel", "bad"), "bf16x3")
    with mode(model, _range_overflow="rerun"):
        lanes = ReplayLanes(model, [upload(full, questions(full, "verify_rel")), upload(full, questions(full, "verify_rel"))])
        torch.cuda.synchronize()
        n0 = reruns()
        t0 = lanes.submit(lambda lane_pbs: put(lane_pbs, bad))
        t1 = lanes.submit(lambda lane_pbs: put(lane_pbs, good))
        r0, r1 = lanes.collect(t0), lanes.collect(t1)
        same(r0, wide, "lane 0")
        same(r1, clean, "lane 1")
        assert reruns() == n0 + 1
        t0 = lanes.submit(lambda lane_pbs: put(lane_pbs, good))   # lane 0 again, clean: nothing of the re-run stays behind
        same(lanes.collect(t0), clean, "lane 0 afterwards")
        assert reruns() == n0 + 1


def test_default_unchanged(tmp_path):
    """No GPU: `range_overflow` defaults to raise, `rerun` sets it, anything else is a ValueError; the check closure called the old way raises
    the text range_message gives, and hands its flags back only when asked to."""
    from dfol_vqa_amd import experiment
    paths, names = syn.write_synthetic_ontology(str(tmp_path))
    cfg = syn.reference_config(paths)
    ont = experiment.build_ontology(cfg)
    assert "range_overflow" not in cfg
    assert experiment.build_model(cfg, ont)._range_overflow == "raise"
    assert experiment.build_model(dict(cfg, range_overflow="rerun"), ont)._range_overflow == "rerun"
    assert experiment.build_model(dict(cfg, range_overflow="raise"), ont)._range_overflow == "raise"
    with pytest.raises(ValueError, match="range_overflow"):
        experiment.build_model(dict(cfg, range_overflow="maybe"), ont)

    class FakeWord(object):                                      # (what the closure does with a non-zero word: clear it)
        zeroed = 0

        def zero_(self):
            FakeWord.zeroed += 1

    watch = _lib.RangeWatch.__new__(_lib.RangeWatch)
    watch.word, watch.device, watch._outer = FakeWord(), torch.device("cpu"), None
    check = fake_finish(watch)
    assert check.range_check is True
    assert check(False, 0) is None
    for flags, word in ((_lib.RANGE_X_OVERFLOW, "65504"), (_lib.RANGE_PAIR_SATURATED, "saturation"), (3, "65504.*saturation")):
        with pytest.raises(_lib.DfolError, match=word) as err:
            check(False, flags)
        assert str(err.value) == _lib.range_message(flags) and "bf16x3" in str(err.value)
        with pytest.raises(_lib.DfolError):
            check(sync=False, value=flags)
        assert check(False, flags, False) == flags
    assert check(False, 0, False) == 0


def fake_finish(watch):
    """RangeWatch.finish() with the device taken out of it: a host word that is never copied into, no status pointer, no event."""
    import unittest.mock as mock
    lib = mock.Mock()
    host = torch.zeros(1, dtype=torch.int32)
    host.copy_ = lambda *a, **k: host
    with mock.patch.object(_lib, "load", lambda: lib), mock.patch.object(_lib, "_range_host", lambda: host), \
            mock.patch.object(_lib, "capturing", lambda: True):
        return watch.finish()
