"""GPU tests of the dropout kernel (csrc/dfol_dropout.hip) against the numpy restatement of its mask rule (tests/dropout_rule.py)."""

import numpy as np
import pytest
import torch

from dfol_vqa_amd import _lib
from dfol_vqa_amd import ops as L
from tests import dropout_rule as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 91


def bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)).view(np.uint32)


def current_key():
    """(k0, k1) read back from the device state, and the state's step."""
    rec = _lib.dropout_state(DEV).cpu().numpy().view(np.uint64)
    return (int(rec[2]) & 0xFFFFFFFF, int(rec[2]) >> 32), int(rec[1])


@pytest.fixture()
def stream():
    """A freshly seeded stream, advanced twice: the key is step 2's, by the kernel's own advance."""
    _lib.seed_dropout(SEED, rank=3)
    key0, step0 = current_key()
    assert step0 == 0 and key0 == R.stream_key(SEED, 0, 3)
    _lib.dropout_advance(DEV)
    _lib.dropout_advance(DEV)
    key, step = current_key()
    assert step == 2 and key == R.stream_key(SEED, 2, 3)
    yield key
    _lib.seed_dropout(torch.initial_seed())


# views: (buffer shape, row slice start, column slice start, rows, cols).  1 x 1: one lane; 3 x 7: a tail group only after one full group, 8 lanes
# a row; 257 x 301: more than one workgroup's rows in a launch of 4-row wavefronts... and a tail of one; 64 x 1036: the pair matrix's width, a wavefront a
# row; [129, 2048] of [129, 2054]: the featurizer's view - every other row only 8-byte aligned; a view from column 1: 4-byte aligned rows
CASES = [((1, 1), 0, 1, 1), ((3, 7), 0, 3, 7), ((257, 301), 0, 257, 301), ((64, 1036), 0, 64, 1036), ((129, 2054), 0, 129, 2048),
         ((33, 70), 1, 33, 66), ((33, 71), 1, 33, 70)]


@pytest.mark.parametrize("shape,col0,rows,cols", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("p", [0.2, 0.5])
def test_kernel_equals_the_host_rule(stream, shape, col0, rows, cols, p):
    g = torch.Generator().manual_seed(rows * 131 + cols)
    buf = torch.randn(shape, generator=g)
    want = R.apply(buf[:, col0:col0 + cols].numpy(), p, site=4, key=stream)
    dev = buf.to(DEV)
    x = dev[:, col0:col0 + cols]
    y = _lib.dropout(x, p, _lib.dropout_key(DEV), 4)                          # out of place, into a fresh matrix
    assert np.array_equal(bits(y), bits(want))
    assert np.array_equal(_lib.dropout_mask((rows, cols), p, 4, DEV).cpu().numpy(), R.keep_mask(rows, cols, p, 4, stream))
    out = torch.full(shape, -7.0, device=DEV)                                 # out of place, into a view of the same strides
    _lib.dropout(x, p, _lib.dropout_key(DEV), 4, out=out[:, col0:col0 + cols])
    assert np.array_equal(bits(out[:, col0:col0 + cols].contiguous()), bits(want))
    _lib.dropout(x, p, _lib.dropout_key(DEV), 4, out=x)                       # in place
    assert np.array_equal(bits(x.contiguous()), bits(want))
    keep = np.ones(shape, bool)
    keep[:, col0:col0 + cols] = False
    assert np.array_equal(bits(dev)[keep], bits(buf)[keep]) and bool((out.cpu().numpy()[keep] == -7.0).all()), "columns outside the view"


def test_dropped_elements_are_zero_under_inf_and_nan(stream):
    x = torch.full((40, 37), float("inf"))
    x[::2] = float("nan")
    x[1::4] = -float("inf")
    y = _lib.dropout(x.to(DEV), 0.5, _lib.dropout_key(DEV), 0).cpu().numpy()
    keep = R.keep_mask(40, 37, 0.5, 0, stream)
    assert 0.3 < keep.mean() < 0.7
    assert np.array_equal(y[~keep].view(np.uint32), np.zeros(int((~keep).sum()), np.uint32))       # +0.0, bit for bit
    assert np.array_equal(bits(y[keep]), bits((x.numpy() * R.scale(0.5))[keep]))


def test_backward_regenerates_the_forwards_mask(stream):
    """ops.dropout under autograd: the backward is mask * scale * g bit for bit, and a backward that runs after a SECOND forward (the step has
    advanced, the site counter restarted) still uses the first forward's mask."""
    p = 0.2
    x = torch.randn(50, 301, generator=torch.Generator().manual_seed(5)).to(DEV).requires_grad_(True)
    g = torch.randn(50, 301, generator=torch.Generator().manual_seed(6)).to(DEV)
    _lib.PATH_COUNTS.clear()
    _lib.dropout_forward_begins()
    y0 = L.dropout(x, p)
    y1 = L.dropout(x, p)                                                    # site 1 of the same forward
    key1, step1 = current_key()
    assert step1 == 3 and key1 == R.stream_key(SEED, 3, 3)                   # the forward's first Dropout advanced the step, once
    m0, m1 = R.keep_mask(50, 301, p, 0, key1), R.keep_mask(50, 301, p, 1, key1)
    assert not np.array_equal(m0, m1)
    assert np.array_equal(bits(y0), bits(R.apply(x.detach().cpu().numpy(), p, 0, key1)))
    assert np.array_equal(bits(y1), bits(R.apply(x.detach().cpu().numpy(), p, 1, key1)))
    _lib.dropout_forward_begins()                                           # a later forward: a new step, sites from zero again
    y2 = L.dropout(x, p)
    key2, step2 = current_key()
    assert step2 == 4 and key2 != key1
    assert np.array_equal(bits(y2), bits(R.apply(x.detach().cpu().numpy(), p, 0, key2)))
    (gx,) = torch.autograd.grad(y1, x, g)                                   # the first forward's site 1, after the second forward
    want = np.where(m1, g.cpu().numpy() * R.scale(p), np.float32(0.0)).astype(np.float32)
    assert np.array_equal(bits(gx), bits(want))
    (gx0,) = torch.autograd.grad(y0, x, g[:, ::1].t().contiguous().t())      # a gradient of another memory layout
    assert np.array_equal(bits(gx0), bits(np.where(m0, g.cpu().numpy() * R.scale(p), np.float32(0.0)).astype(np.float32)))
    assert _lib.PATH_COUNTS["dropout"] == 5                                  # three forwards, two backwards


def test_p_zero_and_eval_launch_nothing(stream):
    from dfol_vqa_amd.visual_oracle import RegularMLP
    torch.manual_seed(0)
    net = RegularMLP(24, 5, [16], 0.2).to(DEV)
    zero = RegularMLP(24, 5, [16], 0.0).to(DEV).train()
    zero.load_state_dict(net.state_dict())
    x = torch.randn(19, 24, device=DEV)
    _lib.PATH_COUNTS.clear()
    _, step = current_key()
    with torch.no_grad():
        a = net.eval()(x)
        b = zero(x)
        assert L.dropout(x, 0.0) is x
    assert _lib.PATH_COUNTS["dropout"] == 0 and current_key()[1] == step
    assert np.array_equal(bits(a), bits(b))
    _lib.dropout_forward_begins()
    trace = _lib.DROPOUT_TRACE = []
    try:
        with torch.no_grad():
            c = net.train()(x)                                              # train() with p > 0 drops during inference too, as the reference does
    finally:
        _lib.DROPOUT_TRACE = None
    assert trace == [(0, (19, 24), 0.2), (1, (19, 16), 0.2)] and _lib.PATH_COUNTS["dropout"] == 2 and current_key()[1] == step + 1
    assert not np.array_equal(bits(c), bits(a))
    # ... and is the two layers on the masked inputs: restated with the kernel's own masks and the library's dense layers
    key = current_key()[0]
    lin1, lin2 = net._network[1], net._network[4]
    with torch.no_grad():
        h = _lib.linear_act(torch.from_numpy(R.apply(x.cpu().numpy(), 0.2, 0, key)).to(DEV), lin1.weight, lin1.bias, _lib.ACT_ELU)
        want = _lib.linear_act(torch.from_numpy(R.apply(h.cpu().numpy(), 0.2, 1, key)).to(DEV), lin2.weight, lin2.bias, _lib.ACT_SIGMOID)
    assert np.array_equal(bits(c), bits(want))


def test_guards():
    h = _lib.load()
    x = torch.zeros(4, 8, device=DEV)
    key = _lib.dropout_key(DEV)
    assert h.dfol_dropout_f32(None, 8, None, 8, 0, 8, 0.5, None, 0, None) == 0                       # no rows: no launch, no error
    for rows, cols, ld, p in ((-1, 8, 8, 0.5), (4, 0, 8, 0.5), (4, 8, 7, 0.5), (4, 8, 8, 1.0), (4, 8, 8, -0.1)):
        assert h.dfol_dropout_f32(x.data_ptr(), ld, x.data_ptr(), ld, rows, cols, p, key.data_ptr(), 0, None) != 0
        assert b"dropout" in h.dfol_last_error()
    with pytest.raises(_lib.DfolError):
        _lib.dropout(torch.zeros(4, 8), 0.5, key, 0)                                                 # no CPU fallback
    with pytest.raises(_lib.DfolError):
        _lib.dropout(x.t(), 0.5, key, 0)                                                             # unit column stride
    with pytest.raises(_lib.DfolError):
        L.dropout(x, 1.0)
