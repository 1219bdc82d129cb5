"""The size limits of the calibration LSTM kernels, without a GPU: the two queries (dfol_lstm_cell_supported, dfol_calib_walk_supported) state the
rules the kernels' LDS tiling sets (csrc/dfol_calib.h: lc_lds_floats, lc_wide_lds_floats), and the cell's entry point refuses what the query refuses.
Argument errors are reported before any device call, so rows = 0 with null pointers asks the entry point for its verdict alone."""

import pytest

KXS = (1, 30, 318, 446, 447, 786)
HS = (1, 6, 50, 72, 78, 79, 100, 200)


@pytest.fixture(scope="module")
def h():
    import __graft_entry__ as g
    g.build()
    from dfol_vqa_amd import _lib
    return _lib.load()


def cell_rc(h, KX, H):
    """dfol_lstm_cell_f32 on zero rows: its size checks and nothing else."""
    return h.dfol_lstm_cell_f32(None, KX, KX, None, H, None, None, 4 * H, None, 4 * H, None, None, 0, H, None, None, None)


@pytest.mark.parametrize("KX,H", [(446, 50), (396, 100)])
def test_cell_takes_the_widths_at_its_limit(h, KX, H):
    assert cell_rc(h, KX, H) == 0


@pytest.mark.parametrize("KX,H", [(447, 50), (318, 200)])
def test_cell_refuses_wider_with_a_message(h, KX, H):
    assert cell_rc(h, KX, H) != 0
    assert b"staging buffer" in h.dfol_last_error()


def test_queries_state_the_kernels_rules(h):
    for KX in KXS:
        for H in HS:
            assert bool(h.dfol_lstm_cell_supported(KX, H)) == (KX + H <= 496), (KX, H)
            assert bool(h.dfol_calib_walk_supported(KX, H)) == (KX + 9 * H + 2 <= 1024), (KX, H)


def test_cell_query_agrees_with_the_entry_point(h):
    for KX in KXS:
        for H in HS:
            assert (cell_rc(h, KX, H) == 0) == bool(h.dfol_lstm_cell_supported(KX, H)), (KX, H)


def test_python_wrappers_answer_like_the_library():
    from dfol_vqa_amd import _lib
    assert _lib.lstm_cell_supported(318, 50) and _lib.lstm_cell_supported(396, 100) and not _lib.lstm_cell_supported(318, 200)
    assert _lib.calib_walk_supported(318, 72) and not _lib.calib_walk_supported(318, 100)
