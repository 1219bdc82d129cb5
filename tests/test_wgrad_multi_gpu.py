"""Several readers' weight gradient in one pass (csrc/dfol_pair_wgrad.hip: pair_wgrad_fused_kernel<CPT, false, false, MULTI> behind
dfol_pair_wgrad_fused_multi_f32, its scale from dfol_pair_wgrad_multi_scale_f32) against float64:  dW2 = sum_k dpre2_k^T Z,
dpre2_k[r][j] = dx_k[r] E_k[p(r)][j] h (1 - h), h = Sigmoid(pre2[r][j]).

Shapes: (HID2, HID1) = (300, 256) [three columns per thread], (304, 256), (64, 128), (320, 252) [four]; ragged images of 1..9 objects and one of
40, i.e. predicates of 0, 2, 6, 12, 20, 30, 42, 56, 72 and 1560 pair rows - boundaries inside an octet, several boundaries inside one 32-row step,
M = 1800 (no multiple of 32, eight slabs); a second batch of M = 260: just over one slab of 256 rows, so two workgroups and the reduce run.
Strided operands: pre2, Z and the embedding rows are column slices with NaN behind them, dx rows are 8 floats apart from M.

The tolerance is not invented here.  The readers one by one through dfol_pair_wgrad_fused_f32 (each with its own scale), summed, are today's
answer; the kernel's error model is max(2^-23 |a|, 2^-39 x largest row bound) per element.  The one pass must stay within TWICE the summed single
passes' largest error against float64 plus one fp32 ulp of the element (the factor 2: one common scale in place of nr separate ones).  One
reader given the same scale must give dfol_pair_wgrad_fused_f32's bits; two runs of anything must be bitwise equal.

Every case prints both measured errors (pytest -s)."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dfol_vqa_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64

SHAPES = [(300, 256), (304, 256), (64, 128), (320, 252)]
BATCHES = {"ragged": [3, 1, 2, 4, 5, 40, 6, 1, 7, 8, 9],       # 6, 0, 2, 12, 20, 1560, 30, 0, 42, 56, 72 rows: M = 1800
           "two_slabs": [5, 2, 3, 9, 1, 4, 8, 6, 7, 5]}       # M = 260: one slab of 256 rows and four more
# readers: (scale of dx, kind); "idle": zero rows for every other question
READERS = {1: [(1.0, "dense")],
           2: [(1.0, "dense"), (2.0 ** -10, "dense")],
           3: [(1.0, "dense"), (0.0, "dense"), (2.0 ** 10, "idle")],
           4: [(1.0, "dense"), (2.0 ** -10, "idle"), (3.0, "dense"), (0.0, "dense")],
           6: [(1.0, "dense"), (2.0 ** -10, "dense"), (0.5, "idle"), (2.0 ** 10, "dense"), (0.0, "dense"), (7.0, "idle")]}

_cache = {}


def _inputs(h2, h1, batch, nr):
    key = (h2, h1, batch, nr)
    if key in _cache:
        return _cache[key]
    g = torch.Generator(device="cpu").manual_seed(1000 * h2 + 10 * h1 + nr + (7 if batch == "ragged" else 0))
    rows = [n * (n - 1) for n in BATCHES[batch]]
    P, M = len(rows), sum(rows)
    pred_off = torch.tensor([0] + list(torch.tensor(rows).cumsum(0)), dtype=I64)
    row_pred = torch.repeat_interleave(torch.arange(P, dtype=I32), torch.tensor(rows))
    nan = float("nan")
    p2 = torch.full((M, h2 + 4), nan)
    p2[:, :h2] = 2.0 * torch.randn(M, h2, generator=g)
    z = torch.full((M, h1 + 4), nan)
    z[:, :h1] = torch.nn.functional.elu(torch.randn(M, h1, generator=g))
    E = torch.full((nr, P, h2 + 4), nan)
    E[:, :, :h2] = 0.3 * torch.randn(nr, P, h2, generator=g)
    dx = torch.full((nr, M + 8), nan)
    for k, (sc, kind) in enumerate(READERS[nr]):
        d = sc * torch.randn(M, generator=g)
        if kind == "idle":
            d = d * (row_pred % 2 == 0).float()
        dx[k, :M] = d
    t = dict(P=P, M=M, h2=h2, h1=h1, nr=nr, pred_off=pred_off.to(DEV), row_pred=row_pred.to(DEV), p2=p2.to(DEV)[:, :h2], z=z.to(DEV)[:, :h1],
             E=E.to(DEV), dx=dx.to(DEV))
    # float64 on the device: sum_k dpre2_k^T Z
    h = torch.sigmoid(t["p2"].double())
    coef = torch.zeros(M, h2, dtype=F64, device=DEV)
    for k in range(nr):
        coef += t["dx"][k, :M].double()[:, None] * t["E"][k, :, :h2].double().index_select(0, t["row_pred"].long())
    t["ref"] = (coef * h * (1.0 - h)).t() @ t["z"].double()
    _cache[key] = t
    return t


def _scale(t, k0, nr):
    """{S, 1 / S, bound} of readers k0 .. k0 + nr - 1, from the device"""
    emax = t["E"][k0:k0 + nr, :, :t["h2"]].abs().amax(2).contiguous()
    scale = torch.empty(4, dtype=F32, device=DEV)
    dx = t["dx"][k0:]
    L.call("dfol_pair_wgrad_multi_scale_f32", dx.data_ptr(), dx.stride(0), nr, t["row_pred"].data_ptr(), emax.data_ptr(), t["P"], t["M"],
           scale.data_ptr(), L._stream())
    return scale


def _multi(t, k0, nr, scale, bad=()):
    M, h2, h1 = t["M"], t["h2"], t["h1"]
    a = dict(nr=nr, h2=h2, dx_stride=t["dx"].stride(0))
    a.update(dict(bad))
    ws = torch.empty(L.load().dfol_pair_wgrad_fused_workspace(M, h2, h1), dtype=F32, device=DEV)
    dw = torch.full((h2, h1), float("nan"), dtype=F32, device=DEV)
    dx, E = t["dx"][k0:], t["E"][k0:]
    L.call("dfol_pair_wgrad_fused_multi_f32", t["p2"].data_ptr(), t["p2"].stride(0), dx.data_ptr(), a["dx_stride"], a["nr"], t["row_pred"].data_ptr(),
           t["pred_off"].data_ptr(), E.data_ptr(), E.stride(1), t["P"], scale.data_ptr(), t["z"].data_ptr(), t["z"].stride(0), M, a["h2"], h1,
           ws.data_ptr(), dw.data_ptr(), L._stream())
    return dw


def _single(t, k, scale):
    M, h2, h1 = t["M"], t["h2"], t["h1"]
    ws = torch.empty(L.load().dfol_pair_wgrad_fused_workspace(M, h2, h1), dtype=F32, device=DEV)
    dw = torch.full((h2, h1), float("nan"), dtype=F32, device=DEV)
    L.call("dfol_pair_wgrad_fused_f32", t["p2"].data_ptr(), t["p2"].stride(0), t["dx"][k].data_ptr(), t["row_pred"].data_ptr(), t["pred_off"].data_ptr(),
           t["E"][k].data_ptr(), t["E"].stride(1), scale.data_ptr(), t["z"].data_ptr(), t["z"].stride(0), M, h2, h1, ws.data_ptr(), dw.data_ptr(),
           L._stream())
    return dw


def _singles_summed(t):
    key = "singles"
    if key not in t:
        dw = None
        for k in range(t["nr"]):
            one = _single(t, k, _scale(t, k, 1))
            dw = one if dw is None else dw + one             # (the order and arithmetic of today's route: _HeadUse.backward adds the readers' shares)
        t[key] = dw
    return t[key]


def _ulp(x):
    """one fp32 ulp of |x| (x float64)"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def _check(t, got, what):
    ref = t["ref"]
    assert torch.isfinite(got).all(), what
    err_single = (_singles_summed(t).double() - ref).abs().max().item()
    err = (got.double() - ref).abs()
    print("%s  HID2 %3d HID1 %3d M %4d readers %d:  multi %.3e   singles summed %.3e   (max |dW2| %.3e)"
          % (what, t["h2"], t["h1"], t["M"], t["nr"], err.max().item(), err_single, ref.abs().max().item()))
    assert bool((err <= 2.0 * err_single + _ulp(ref)).all()), (what, err.max().item(), err_single)


@pytest.mark.parametrize("nr", [1, 2, 3, 4])
@pytest.mark.parametrize("h2,h1", SHAPES)
def test_one_pass_against_float64_and_the_readers_one_by_one(h2, h1, nr):
    t = _inputs(h2, h1, "ragged", nr)
    scale = _scale(t, 0, nr)
    got = _multi(t, 0, nr, scale)
    _check(t, got, "ragged   ")
    assert torch.equal(got, _multi(t, 0, nr, scale)), "two runs differ"
    if nr == 1:
        assert torch.equal(got, _single(t, 0, scale)), "one reader, the same scale: not the bits of dfol_pair_wgrad_fused_f32"


@pytest.mark.parametrize("nr", [1, 3, 4])
@pytest.mark.parametrize("h2,h1", [(300, 256), (64, 128)])
def test_just_over_one_slab(h2, h1, nr):
    t = _inputs(h2, h1, "two_slabs", nr)
    scale = _scale(t, 0, nr)
    got = _multi(t, 0, nr, scale)
    _check(t, got, "two slabs")
    assert torch.equal(got, _multi(t, 0, nr, scale)), "two runs differ"
    if nr == 1:
        assert torch.equal(got, _single(t, 0, scale))


@pytest.mark.parametrize("h2,h1", [(300, 256), (320, 252)])
def test_six_readers_through_the_binding(h2, h1):
    t = _inputs(h2, h1, "ragged", 6)
    M = t["M"]
    args = ([t["dx"][k, :M] for k in range(6)], t["p2"], t["z"], [t["E"][k, :, :h2] for k in range(6)], t["pred_off"], t["row_pred"])
    got = L.pair_wgrad_multi(*args)
    _check(t, got, "binding  ")
    assert torch.equal(got, L.pair_wgrad_multi(*args)), "two runs differ"


def test_scale_is_the_power_of_two_of_the_largest_row_bound():
    t = _inputs(64, 128, "ragged", 4)
    s = _scale(t, 0, 4).cpu()
    emax = t["E"][:, :, :64].abs().amax(2)
    bound = sum(t["dx"][k, :t["M"]].abs() * emax[k].index_select(0, t["row_pred"].long()) * 0.25 for k in range(4)).max().item()
    assert abs(s[2].item() - bound) <= 1e-6 * bound
    assert s[0].item() * s[1].item() == 1.0 and 2.0 ** 13 <= s[0].item() * s[2].item() < 2.0 ** 14


def test_bad_arguments_are_errors_not_launches():
    t = _inputs(64, 128, "two_slabs", 4)
    scale = _scale(t, 0, 4)
    for bad in (dict(nr=0), dict(nr=5), dict(h2=324), dict(dx_stride=t["M"] - 1)):
        with pytest.raises(L.DfolError) as e:
            _multi(t, 0, 4, scale, bad)
        assert "pair_wgrad_fused_multi" in str(e.value), str(e.value)
