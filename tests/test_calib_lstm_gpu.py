"""The calibration LSTM kernels (csrc/dfol_calib.h) off their one shape.

Every calibrated forward runs eight LSTM cells through three pieces of device code: the grid kernel (lc_stage + lc_units) behind dfol_lstm_cell_f32 /
_tokens_f32 / _train_f32, the walk kernel's cell (lc_wide inside calib_walk_kernel) and the pointwise kernels (dfol_lstm_pointwise_f32,
dfol_lstm_cell_bwd_f32).  The rest of the suite runs them at LSTMCell(318 -> 50) and LSTMCell(30 -> 6) only, where the second weight load of a K
slice, the walk's second column pass, empty / unequal K slices and H < 8 never execute.  Here: the widths at which each loop takes another path,
against the cell's formula in float64, with torch's own fp32 cell as the measure of fp32 rounding noise (the rule of
test_kernels_gpu.py::test_calibration_lstm_cell_equals_torch:  e_kernel <= 4 e_torch_fp32 + 2e-6), the bitwise relations include/dfol_vqa.h
promises between the entry points, and the routes a model takes beyond the kernels' size limits (KX + H <= 496 for the cell,
KX + 9 H + 2 <= 1024 for the walk)."""

import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
from dfol_vqa_amd import native_exec, native_plan  # noqa: E402
from dfol_vqa_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

# (KX, H): what the shape reaches (K = KX + H is cut into 16 slices, a thread holds LC_MAXK = 24 weights of its slice at a time; a workgroup owns
# 16 rows x 8 hidden units)
SHAPES = [
    (318, 50),     # K = 368: the shape of every other test (control)
    (1, 1),        # K = 2: 14 empty slices, one hidden unit, every load clamped to K - 1
    (5, 3),        # K = 8: K < 16, H < 8
    (17, 8),       # K = 25: slices of unequal length, exactly one unit block
    (334, 50),     # K = 384: the longest slice is still 24 - one load
    (335, 50),     # K = 385: one slice of 25 - the second load, of a single weight
    (318, 72),     # K = 390: second load; 4H = 288 > 256 (the walk kernel's second column pass)
    (396, 100),    # K = 496: the cell's limit, slices of 31
    (446, 50),     # K = 496: the limit with a wide input
    (96, 200),     # K = 296: 25 unit blocks, 4H = 800
]
ROWS = (1, 15, 16, 17, 100)          # (a workgroup owns 16 rows: nothing larger reaches other code)
MAX_ROWS = max(ROWS)
GUARD = 64                           # floats behind every output that must stay untouched
RATIOS = {}                          # shape -> largest e_kernel / (4 e_ref + 2e-6) seen


@pytest.fixture(scope="module")
def L():
    from dfol_vqa_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    return _lib


_CASES = {}


def case(KX, H):
    """Seeded inputs of one shape at MAX_ROWS rows (a test takes the first `rows` of them) and the float64 cell on them, computed once."""
    hit = _CASES.get((KX, H))
    if hit is not None:
        return hit
    g = torch.Generator().manual_seed(1000 * KX + H)
    rnd = lambda *s: torch.randn(*s, generator=g)
    K = KX + H
    c = dict(KX=KX, H=H,
             w_ih=(rnd(4 * H, KX) / math.sqrt(K)).cuda(), w_hh=(rnd(4 * H, H) / math.sqrt(K)).cuda(),     # gate pre-activations of order one
             b_ih=(rnd(4 * H) * 0.5).cuda(), b_hh=(rnd(4 * H) * 0.5).cuda(),
             x=rnd(MAX_ROWS, KX).cuda(), h=(rnd(MAX_ROWS, H) * 0.5).cuda(), c=rnd(MAX_ROWS, H).cuda())
    c["wt"] = (c["w_ih"].t().contiguous(), c["w_hh"].t().contiguous())
    c["ref64"] = {}
    _CASES[(KX, H)] = c
    return c


def cell_formula(x, h, c, w_ih, w_hh, b_ih, b_hh, dtype):
    """nn.LSTMCell's formula (gate order i, f, g, o) in `dtype` -> h', c', activated gates [rows, 4H]."""
    x, h, c, w_ih, w_hh = (t.to(dtype) for t in (x, h, c, w_ih, w_hh))
    gates = x @ w_ih.t() + h @ w_hh.t()
    if b_ih is not None:
        gates = gates + b_ih.to(dtype)
    if b_hh is not None:
        gates = gates + b_hh.to(dtype)
    i, f, gg, o = gates.chunk(4, 1)
    i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
    c_new = f * c + i * gg
    return o * torch.tanh(c_new), c_new, torch.cat([i, f, gg, o], 1)


def ref64(cs, use_ih=True, use_hh=True):
    """The float64 cell of a case at MAX_ROWS rows (rows are independent: a test slices it), shared and left unchanged."""
    key = (use_ih, use_hh)
    if key not in cs["ref64"]:
        cs["ref64"][key] = cell_formula(cs["x"], cs["h"], cs["c"], cs["w_ih"], cs["w_hh"], cs["b_ih"] if use_ih else None,
                                        cs["b_hh"] if use_hh else None, torch.float64)
    return cs["ref64"][key]


def torch_cell(cs, rows, use_ih=True, use_hh=True):
    """torch's own fp32 nn.LSTMCell on the first `rows` rows (a missing bias as zeros: adding 0 is exact)."""
    cell = torch.nn.LSTMCell(cs["KX"], cs["H"]).cuda()
    z = torch.zeros_like(cs["b_ih"])
    cell.load_state_dict({"weight_ih": cs["w_ih"], "weight_hh": cs["w_hh"], "bias_ih": cs["b_ih"] if use_ih else z, "bias_hh": cs["b_hh"] if use_hh else z})
    with torch.no_grad():
        return cell(cs["x"][:rows], (cs["h"][:rows], cs["c"][:rows]))


def nan_out(rows, width):
    """An output buffer pre-filled with NaN (an unwritten element cannot pass) with GUARD floats behind it (a write past the end shows)."""
    buf = torch.full((rows * width + GUARD,), float("nan"), device="cuda")
    return buf, buf[:rows * width].view(rows, width)


def ptr(t):
    return None if t is None else t.data_ptr()


def run_cell(L, cs, rows, x=None, h=None, b_ih="own", b_hh="own", entry="cell", tokens=None):
    """One of the three entry points of the grid kernel, through the C ABI, on the first `rows` rows -> (h', c'[, gates])."""
    H, KX, wt = cs["H"], cs["KX"], cs["wt"]
    x = cs["x"][:rows] if x is None else x
    h = cs["h"][:rows] if h is None else h
    b_ih = cs["b_ih"] if isinstance(b_ih, str) else b_ih
    b_hh = cs["b_hh"] if isinstance(b_hh, str) else b_hh
    c = cs["c"][:rows]
    assert c.is_contiguous() and x.stride(1) == 1 and h.stride(1) == 1 and tuple(h.shape) == (rows, H)
    bufs = [nan_out(rows, H), nan_out(rows, H)]
    tail = [h.data_ptr(), h.stride(0), c.data_ptr(), wt[0].data_ptr(), wt[0].stride(0), wt[1].data_ptr(), wt[1].stride(0), ptr(b_ih), ptr(b_hh), rows, H,
            bufs[0][1].data_ptr(), bufs[1][1].data_ptr()]
    if entry == "tokens":
        head, table, idx = tokens
        assert head.numel() + table.shape[1] == KX and idx.numel() == rows and idx.dtype == torch.int32
        L.call("dfol_lstm_cell_tokens_f32", ptr(head), head.numel(), ptr(table), table.shape[1], idx.data_ptr(), *tail, L._stream())
    elif entry == "train":
        assert tuple(x.shape) == (rows, KX)
        bufs.append(nan_out(rows, 4 * H))
        L.call("dfol_lstm_cell_train_f32", x.data_ptr(), x.stride(0), KX, *tail, bufs[2][1].data_ptr(), L._stream())
    else:
        assert tuple(x.shape) == (rows, KX)
        L.call("dfol_lstm_cell_f32", x.data_ptr(), x.stride(0), KX, *tail, L._stream())
    for buf, view in bufs:
        assert torch.isnan(buf[view.numel():]).all(), "a write behind the output"
    return tuple(view for _, view in bufs)


def within(got, r32, r64, what, shape=None, scale=1.0):
    """The project's rule: max |got - fp64| <= 4 max |torch fp32 - fp64| + 2e-6 (per tensor; `scale`: the gradient tests divide by max |fp64|)."""
    e = (got.double() - r64).abs().max().item() / scale
    e_ref = (r32.double() - r64).abs().max().item() / scale
    bound = 4 * e_ref + 2e-6
    if shape is not None and e == e:
        RATIOS[shape] = max(RATIOS.get(shape, 0.0), e / bound)
    assert not torch.isnan(got).any(), (what, "NaN: an element was not written, or the kernel produced one")
    assert e <= bound, (what, "e_kernel %.3g, e_ref %.3g, ratio %.3f" % (e, e_ref, e / bound))
    return e / bound


# ---- forward accuracy --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("KX,H", SHAPES)
def test_cell_forward_against_float64(L, KX, H):
    """dfol_lstm_cell_f32 at every shape and row count into NaN-filled buffers: e_kernel <= 4 e_ref + 2e-6 per output tensor, e against the
    float64 formula, e_ref torch's own fp32 nn.LSTMCell on the same inputs."""
    cs = case(KX, H)
    h64, c64, _ = ref64(cs)
    for rows in ROWS:
        hy, cy = run_cell(L, cs, rows)
        h32, c32 = torch_cell(cs, rows)
        within(hy, h32, h64[:rows], ("h", KX, H, rows), (KX, H))
        within(cy, c32, c64[:rows], ("c", KX, H, rows), (KX, H))
    print("lstm_cell (%d, %d): largest e_kernel / (4 e_ref + 2e-6) = %.3f" % (KX, H, RATIOS[(KX, H)]))


# ---- the bitwise relations of include/dfol_vqa.h ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("KX,H", SHAPES)
def test_train_entry_point_gives_the_cells_bits_and_the_activated_gates(L, KX, H):
    """dfol_lstm_cell_train_f32: h' and c' bit for bit dfol_lstm_cell_f32's; its gates are the ACTIVATED gates (sigmoid i, sigmoid f, tanh g,
    sigmoid o) of the float64 formula to the rule (e_ref: the formula in torch fp32 - nn.LSTMCell does not hand its gates out)."""
    cs = case(KX, H)
    g64 = ref64(cs)[2]
    for rows in ROWS:
        hy, cy = run_cell(L, cs, rows)
        hy2, cy2, gates = run_cell(L, cs, rows, entry="train")
        assert torch.equal(hy, hy2) and torch.equal(cy, cy2), (KX, H, rows)
        g32 = cell_formula(cs["x"][:rows], cs["h"][:rows], cs["c"][:rows], cs["w_ih"], cs["w_hh"], cs["b_ih"], cs["b_hh"], torch.float32)[2]
        within(gates, g32, g64[:rows], ("gates", KX, H, rows), (KX, H))


@pytest.mark.parametrize("KX,H", SHAPES)
def test_token_form_equals_features_then_cell(L, KX, H):
    """dfol_lstm_cell_tokens_f32 == dfol_calib_features_f32 + dfol_lstm_cell_f32 bit for bit: no-op tokens (idx < 0 -> zero rows), and the
    degenerate splits n_head = 0 and E = 0 of KX = n_head + E."""
    cs = case(KX, H)
    g = torch.Generator().manual_seed(7 * KX + H)
    splits = [(0, KX), (KX, 0)] + ([(min(18, KX - 1), KX - min(18, KX - 1))] if KX >= 2 else [])
    T = 7
    for n_head, E in splits:
        head = (torch.randn(n_head, generator=g) * 0.7).cuda()
        table = (torch.randn(T, E, generator=g) * 0.7).cuda()
        for rows in ROWS:
            idx = ((torch.arange(rows) * 3) % (T + 1) - 1).to(torch.int32).cuda()          # -1 (no-op token) first, then rows of the table
            xb, x = nan_out(rows, KX)
            L.call("dfol_calib_features_f32", ptr(head), n_head, ptr(table), E, idx.data_ptr(), rows, x.data_ptr(), L._stream())
            assert torch.isnan(xb[x.numel():]).all() and (x[idx < 0] == 0).all() and not torch.isnan(x).any()
            hy, cy = run_cell(L, cs, rows, x=x)
            hy2, cy2 = run_cell(L, cs, rows, entry="tokens", tokens=(head, table, idx))
            assert torch.equal(hy, hy2) and torch.equal(cy, cy2), (KX, H, n_head, E, rows)


@pytest.mark.parametrize("KX,H", SHAPES)
def test_strided_inputs_give_the_contiguous_bits(L, KX, H):
    """x as a column window of a wider tensor (ld_x > KX) and h as one (ld_h > H): the bits of the contiguous call, for the plain, the train and
    (h only) the token entry point."""
    cs = case(KX, H)
    for rows in ROWS:
        wide_x = torch.full((rows, KX + 13), 1e30, device="cuda")
        wide_h = torch.full((rows, H + 7), 1e30, device="cuda")
        wide_x[:, 5:5 + KX] = cs["x"][:rows]
        wide_h[:, 3:3 + H] = cs["h"][:rows]
        xs, hs = wide_x[:, 5:5 + KX], wide_h[:, 3:3 + H]
        base = run_cell(L, cs, rows)
        for x, h in ((xs, None), (None, hs), (xs, hs)):
            got = run_cell(L, cs, rows, x=x, h=h)
            assert torch.equal(base[0], got[0]) and torch.equal(base[1], got[1]), (KX, H, rows, x is not None, h is not None)
        tr = run_cell(L, cs, rows, x=xs, h=hs, entry="train")
        tr0 = run_cell(L, cs, rows, entry="train")
        assert all(torch.equal(a, b) for a, b in zip(tr, tr0)) and torch.equal(tr[0], base[0]), (KX, H, rows)
        head, table = torch.zeros(0, device="cuda"), cs["x"][:rows].contiguous()                 # row p of the table is row p of x
        idx = torch.arange(rows, dtype=torch.int32, device="cuda")
        tk = run_cell(L, cs, rows, h=hs, entry="tokens", tokens=(head, table, idx))
        assert torch.equal(tk[0], base[0]) and torch.equal(tk[1], base[1]), (KX, H, rows)


@pytest.mark.parametrize("KX,H", SHAPES)
def test_null_biases_count_as_zero(L, KX, H):
    """b_ih NULL, b_hh NULL and both NULL: the float64 formula with the missing bias as zero, to the rule."""
    cs = case(KX, H)
    for use_ih, use_hh in ((False, True), (True, False), (False, False)):
        h64, c64, _ = ref64(cs, use_ih, use_hh)
        for rows in (17, 100):
            hy, cy = run_cell(L, cs, rows, b_ih="own" if use_ih else None, b_hh="own" if use_hh else None)
            h32, c32 = torch_cell(cs, rows, use_ih, use_hh)
            within(hy, h32, h64[:rows], ("h", KX, H, rows, use_ih, use_hh), (KX, H))
            within(cy, c32, c64[:rows], ("c", KX, H, rows, use_ih, use_hh), (KX, H))


# ---- backward --------------------------------------------------------------------------------------------------------------------------------------
def _pointwise(z, c_prev):
    i, f, gg, o = z.chunk(4, 1)
    i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
    c_new = f * c_prev + i * gg
    return o * torch.tanh(c_new), c_new, torch.cat([i, f, gg, o], 1)


@pytest.mark.parametrize("H", [1, 3, 72, 200])
@pytest.mark.parametrize("which", ["h", "c", "both"])
def test_pointwise_backward_against_float64_autograd(L, H, which):
    """dfol_lstm_cell_bwd_f32 (from the activated gates, c and c' to d_gates w.r.t. the PRE-activations and d_c) with a gradient through h' only
    (d_cy NULL), through c' only (d_hy NULL) and through both, against float64 autograd through the pointwise stage.  The kernel's inputs are the
    float64 stage's values rounded to fp32; the measure of fp32 noise is torch's fp32 autograd through the same stage, the rule the project's:
    e / max|g64| <= 4 e_ref / max|g64| + 2e-6."""
    g = torch.Generator().manual_seed(31 * H + len(which))
    for rows in (1, 17, 100):
        z32, c32 = torch.randn(rows, 4 * H, generator=g).cuda(), torch.randn(rows, H, generator=g).cuda()
        gh, gc = torch.randn(rows, H, generator=g).cuda(), torch.randn(rows, H, generator=g).cuda()
        grads = {}
        for dt in (torch.float64, torch.float32):
            z, c = z32.to(dt).requires_grad_(True), c32.to(dt).requires_grad_(True)
            hy, cy, act = _pointwise(z, c)
            loss = ((hy * gh.to(dt)).sum() if which != "c" else 0) + ((cy * gc.to(dt)).sum() if which != "h" else 0)
            grads[dt] = torch.autograd.grad(loss, (z, c))
            if dt == torch.float64:
                act64, cy64 = act.detach(), cy.detach()
        db, dgates = nan_out(rows, 4 * H)
        cb, dc = nan_out(rows, H)
        act32, cy32 = act64.float().contiguous(), cy64.float().contiguous()
        L.call("dfol_lstm_cell_bwd_f32", act32.data_ptr(), c32.data_ptr(), cy32.data_ptr(),
               ptr(gh if which != "c" else None), ptr(gc if which != "h" else None), rows, H, dgates.data_ptr(), dc.data_ptr(), L._stream())
        assert torch.isnan(db[dgates.numel():]).all() and torch.isnan(cb[dc.numel():]).all()
        for got, r32, r64, name in ((dgates, grads[torch.float32][0], grads[torch.float64][0], "d_gates"), (dc, grads[torch.float32][1], grads[torch.float64][1], "d_c")):
            within(got, r32, r64, (name, H, rows, which), scale=r64.abs().max().item() + 1e-12)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("KX,H", [(5, 3), (318, 72), (396, 100)])
def test_module_gradients_against_float64(L, KX, H, bias):
    """CalibrationLSTMCell with gradients (dfol_lstm_cell_train_f32, then dfol_lstm_cell_bwd_f32 + the dense / weight-gradient kernels): every
    gradient - x, h, c, both weights, both biases - against the float64 cell, torch's fp32 cell as the measure (the loop and the rule of
    test_calibration_lstm_cell_equals_torch), with a gradient through both outputs and through one."""
    from dfol_vqa_amd.visual_oracle import CalibrationLSTMCell
    cs = case(KX, H)
    sd = {"weight_ih": cs["w_ih"], "weight_hh": cs["w_hh"]}
    if bias:
        sd.update(bias_ih=cs["b_ih"], bias_hh=cs["b_hh"])
    cells = {"mine": (CalibrationLSTMCell(KX, H, bias=bias).cuda(), torch.float32), "ref": (torch.nn.LSTMCell(KX, H, bias=bias).cuda(), torch.float32),
             "ref64": (torch.nn.LSTMCell(KX, H, bias=bias).cuda().double(), torch.float64)}
    for cell, dt in cells.values():
        cell.load_state_dict({k: v.to(dt) for k, v in sd.items()})
    g = torch.Generator().manual_seed(KX + H)
    for rows, which in ((37, "both"), (16, "h"), (5, "c")):
        gh, gc = torch.randn(rows, H, generator=g).cuda(), torch.randn(rows, H, generator=g).cuda()
        grads = {}
        L.PATH_COUNTS.clear()
        for tag, (cell, dt) in cells.items():
            cell.zero_grad()
            x, h, c = (cs[k][:rows].detach().to(dt).requires_grad_(True) for k in ("x", "h", "c"))
            hy, cy = cell(x, (h, c))
            loss = ((hy * gh.to(dt)).sum() if which != "c" else 0) + ((cy * gc.to(dt)).sum() if which != "h" else 0)
            loss.backward()
            grads[tag] = [x.grad, h.grad, c.grad, cell.weight_ih.grad, cell.weight_hh.grad] + ([cell.bias_ih.grad, cell.bias_hh.grad] if bias else [])
        assert not any(k.startswith("fallback:") for k in L.PATH_COUNTS), dict(L.PATH_COUNTS)      # (these widths run on this library's kernels)
        for name, gm, gr, g64 in zip(("x", "h", "c", "w_ih", "w_hh", "b_ih", "b_hh"), grads["mine"], grads["ref"], grads["ref64"]):
            within(gm, gr, g64, (name, KX, H, bias, rows, which), scale=g64.abs().max().item() + 1e-12)


# ---- beyond the cell's limit: KX + H > 496 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("KX,H", [(318, 200), (768 + 18, 50)])
def test_wider_cells_take_the_pointwise_route(L, KX, H):
    """attention_transfer_state_dim: 200 and a 768-wide token embedding do not fit the one-launch cell: without gradients CalibrationLSTMCell runs
    two dense products + dfol_lstm_pointwise_f32 (route counter `lstm_pointwise`) and equals float64 to the rule; with gradients it is torch's own
    cell (announced as a fallback) and gives its gradients."""
    from dfol_vqa_amd.visual_oracle import CalibrationLSTMCell
    assert KX + H > 496
    cs = case(KX, H)
    sd = {"weight_ih": cs["w_ih"], "weight_hh": cs["w_hh"], "bias_ih": cs["b_ih"], "bias_hh": cs["b_hh"]}
    mine, ref = CalibrationLSTMCell(KX, H).cuda(), torch.nn.LSTMCell(KX, H).cuda()
    mine.load_state_dict(sd)
    ref.load_state_dict(sd)
    h64, c64, _ = ref64(cs)
    for rows in ROWS:
        x, h, c = cs["x"][:rows], cs["h"][:rows], cs["c"][:rows]
        L.PATH_COUNTS.clear()
        with torch.no_grad():
            hy, cy = mine(x, (h, c))
            h32, c32 = ref(x, (h, c))
        assert L.PATH_COUNTS.get("lstm_pointwise", 0) == 1, dict(L.PATH_COUNTS)
        r = max(within(hy, h32, h64[:rows], ("h", KX, H, rows), (KX, H)), within(cy, c32, c64[:rows], ("c", KX, H, rows), (KX, H)))
    print("pointwise route (%d, %d): largest e / (4 e_ref + 2e-6) = %.3f (last row count %.3f)" % (KX, H, RATIOS[(KX, H)], r))
    # with gradients: torch's cell
    ref64_cell = torch.nn.LSTMCell(KX, H).cuda().double()
    ref64_cell.load_state_dict({k: v.double() for k, v in sd.items()})
    rows = 17
    g = torch.Generator().manual_seed(3)
    gh, gc = torch.randn(rows, H, generator=g).cuda(), torch.randn(rows, H, generator=g).cuda()
    grads = {}
    L.PATH_COUNTS.clear()
    for tag, cell, dt in (("mine", mine, torch.float32), ("ref", ref, torch.float32), ("ref64", ref64_cell, torch.float64)):
        cell.zero_grad()
        x, h, c = (cs[k][:rows].detach().to(dt).requires_grad_(True) for k in ("x", "h", "c"))
        hy, cy = cell(x, (h, c))
        ((hy * gh.to(dt)).sum() + (cy * gc.to(dt)).sum()).backward()
        grads[tag] = [x.grad, h.grad, c.grad, cell.weight_ih.grad, cell.weight_hh.grad, cell.bias_ih.grad, cell.bias_hh.grad]
    assert L.PATH_COUNTS.get("fallback:calibration LSTM cell (training)", 0) == 1 and "lstm_pointwise" not in L.PATH_COUNTS, dict(L.PATH_COUNTS)
    for name, gm, gr, g64 in zip(("x", "h", "c", "w_ih", "w_hh", "b_ih", "b_hh"), grads["mine"], grads["ref"], grads["ref64"]):
        within(gm, gr, g64, (name, KX, H, "torch's cell"), scale=g64.abs().max().item() + 1e-12)


# ---- whole models: the walk kernel and the routing at other state widths -------------------------------------------------------------------------
from test_interpreter_gpu import DEV  # noqa: E402
from test_native_gpu import _FullCalibrationCollater, both_routes, same_results  # noqa: E402


class _Float64Cell(torch.nn.LSTMCell):
    """nn.LSTMCell's formula in float64 on fp32 parameters and states (the twin's yardstick cell: no code of this library)."""

    def forward(self, x, state):
        hy, cy, _ = cell_formula(x, state[0], state[1], self.weight_ih, self.weight_hh, self.bias_ih, self.bias_hh, torch.float64)
        return hy.float(), cy.float()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """The full-size synthetic calibrated model (as test_native_gpu.py's calibrated_full) at another attention_transfer_state_dim, built once per
    width; cell=...: the twin whose two LSTM cells are that class instead of CalibrationLSTMCell, with the same state_dict."""
    from dfol_vqa_amd import experiment
    d = str(tmp_path_factory.mktemp("calib_widths"))
    paths, names = syn.write_synthetic_ontology(d)
    with open(paths["attribute_file"]) as f:
        categories = json.load(f)
    built = {}

    def get(S, cell=None):
        if (S, cell) in built:
            return built[(S, cell)]
        cfg = syn.reference_config(paths, activate_attention_transfer=True, attention_transfer_state_dim=S)
        ont = experiment.build_ontology(cfg)
        own = experiment.CalibrationLSTMCell
        try:
            if cell is not None:
                experiment.CalibrationLSTMCell = cell
            torch.manual_seed(5)
            model = experiment.build_model(cfg, ont)
        finally:
            experiment.CalibrationLSTMCell = own
        if cell is None:
            syn.load_seeded_weights(model, 23)
            with torch.no_grad():                                # (the reference initialises the output layer's weight to zero: every modulation would be Sigmoid(bias))
                out = model._ops['filter']._filter._attention_output_network[0]
                out.weight.normal_(0.0, 0.5)
                out.bias.normal_(0.0, 0.5)
        else:
            model.load_state_dict(get(S)[0].state_dict())
        built[(S, cell)] = (model.to(DEV).eval(), ont)
        return built[(S, cell)]

    return get, names, categories


def _questions(kind, names, categories):
    return syn.full_size_questions(kind, 6, 3, 20, names, categories, 4100 + len(kind))


def _forward(model, ont, qs):
    pbs = [pb.to_cuda(DEV) for pb in _FullCalibrationCollater(1, ont).collate([dict(q) for q in qs])]
    from dfol_vqa_amd import _lib
    _lib.PATH_COUNTS.clear()
    with torch.no_grad():
        res = model(pbs, False)
    return res, pbs, dict(_lib.PATH_COUNTS)


def _walk_on_and_off(model, ont, qs, monkeypatch):
    monkeypatch.setenv("DFOL_NATIVE", "1")
    out = {}
    for walk in ("1", "0"):
        monkeypatch.setenv("DFOL_CALIB_WALK", walk)
        res, pbs, counts = _forward(model, ont, qs)
        assert counts.get("native_program", 0) == len(pbs), counts
        out[walk] = (res, [int(x) for pb in pbs for x in pb._native_plan.instrs[:, 0]])
    return out


@pytest.mark.parametrize("kind", ["exist", "choose_rel"])
def test_state_width_72_second_load_and_second_column_pass(models, kind, monkeypatch):
    """S = 72 (K = 390, 4S = 288): the cell's second weight load and the walk's second column pass are both live.  DFOL_CALIB_WALK=1 gives the bits
    of the separate launches, the plan holds OP_CALIB_WALK only under 1, and the executor equals the Python operator loop bit for bit."""
    get, names, categories = models
    model, ont = get(72)
    assert native_exec.calibrator(model) is not None
    qs = _questions(kind, names, categories)
    out = _walk_on_and_off(model, ont, qs, monkeypatch)
    assert native_plan.OP_CALIB_WALK in out["1"][1] and native_plan.OP_CALIB_WALK not in out["0"][1]
    same_results(out["1"][0], out["0"][0], "S = 72, walk " + kind)
    nat, py = both_routes(model, ont, qs, monkeypatch=monkeypatch, collater=_FullCalibrationCollater(1, ont))
    same_results(nat, py, "S = 72 " + kind)
    same_results(nat, out["0"][0], "S = 72 " + kind)


@pytest.mark.parametrize("kind", ["exist", "choose_rel"])
def test_state_width_100_fits_the_cell_but_not_the_walk(models, kind, monkeypatch):
    """S = 100 (K = 418 <= 496, 318 + 900 + 2 > 1024): under DFOL_CALIB_WALK=1 the plan keeps the separate launches (no OP_CALIB_WALK), the forward
    runs on the executor and gives the bits of DFOL_CALIB_WALK=0 and of the Python loop."""
    get, names, categories = models
    model, ont = get(100)
    assert native_exec.calibrator(model) is not None
    qs = _questions(kind, names, categories)
    out = _walk_on_and_off(model, ont, qs, monkeypatch)
    assert native_plan.OP_CALIB_WALK not in out["1"][1] and out["1"][1] == out["0"][1]
    assert out["1"][1].count(native_plan.OP_LSTM_CELL) >= 4
    same_results(out["1"][0], out["0"][0], "S = 100, walk " + kind)
    nat, py = both_routes(model, ont, qs, monkeypatch=monkeypatch, collater=_FullCalibrationCollater(1, ont))
    same_results(nat, py, "S = 100 " + kind)


@pytest.mark.parametrize("kind", ["exist", "choose_rel"])
def test_state_width_200_runs_on_the_pointwise_route(models, kind, monkeypatch):
    """S = 200 (K = 518): nothing fits.  Under DFOL_NATIVE=1 and =0 the calibrated forward runs - on the Python operator loop, its cells as two dense
    products + dfol_lstm_pointwise_f32 - and its log-probabilities pass check_logprob against a twin model whose two cells are plain
    torch.nn.LSTMCell in fp32 and the cell's formula in float64, with the same state_dict."""
    get, names, categories = models
    model, ont = get(200)
    qs = _questions(kind, names, categories)
    lp = {}
    for native in ("1", "0"):
        monkeypatch.setenv("DFOL_NATIVE", native)
        res, pbs, counts = _forward(model, ont, qs)
        assert counts.get("native_program", 0) == 0 and counts.get("python_program", 0) == len(pbs) and counts.get("lstm_pointwise", 0) >= 4, counts
        lp[native] = res
    same_results(lp["1"], lp["0"], "S = 200 " + kind)
    assert native_exec.calibrator(model) is None and native_exec.model_spec(model, calibrate=True) is None      # (the executor steps aside)
    refs = {}
    for tag, cell in (("f32", torch.nn.LSTMCell), ("f64", _Float64Cell)):
        twin, _ = get(200, cell)
        res, pbs, counts = _forward(twin, ont, qs)
        assert counts.get("lstm_pointwise", 0) == 0 and counts.get("native_program", 0) == 0, counts
        refs[tag] = res["log_probability"].cpu().numpy()
    gu.check_logprob(lp["1"]["log_probability"].cpu().numpy(), refs["f32"], refs["f64"], "S = 200 " + kind)
