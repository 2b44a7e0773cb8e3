"""sl_emd_cells_device without a GPU: the symbol, its argument checks (all of which
return before any launch) and the keyword errors of the Python paths on top of it."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from safelife_amd import _lib
    return _lib, _lib.lib()


def test_constants_match_the_header():
    import os
    import re
    from safelife_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                               "include", "safelife_hip.h")).read()
    for name in ("SL_EMD_DEVICE_MAX_CELLS", "SL_EMD_ST_BADCELL", "SL_EMD_ST_TOOBIG",
                 "SL_EMD_ST_PIVOTS"):
        m = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, header)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert _lib.SL_EMD_DEVICE_MAX_CELLS >= 256
    assert len({_lib.SL_EMD_ST_BADCELL, _lib.SL_EMD_ST_TOOBIG, _lib.SL_EMD_ST_PIVOTS}) == 3
    assert "int sl_emd_cells_device(" in header


def test_argument_checks_return_before_any_launch(lib):
    _lib, L = lib
    assert hasattr(L, "sl_emd_cells_device")
    buf = np.zeros(16, np.int64)                 # a non-null address; never dereferenced
    a = buf.ctypes.data
    f = L.sl_emd_cells_device
    assert f(None, None, None, None, None, 0, None, 4, 4, 1.0, None, None, None) == _lib.SL_OK
    assert f(a, a, a, a, a, 0, a, 4, 4, 1.0, a, a, None) == _lib.SL_OK
    assert f(a, a, a, a, a, -1, a, 4, 4, 1.0, a, a, None) == _lib.SL_EINVAL
    assert f(a, a, a, a, a, 0, a, 0, 4, 1.0, a, a, None) == _lib.SL_EINVAL
    assert f(a, a, a, a, a, 0, a, 4, 0, 1.0, a, a, None) == _lib.SL_EINVAL
    assert f(a, a, a, a, a, 1, a, 4, -3, 1.0, a, a, None) == _lib.SL_EINVAL
    assert f(a, a, a, a, a, 2 ** 31, a, 4, 4, 1.0, a, a, None) == _lib.SL_EINVAL
    for null in range(9):                        # each pointer in turn, nprob = 1
        if null == 5:
            continue
        args = [a, a, a, a, a, 1, a, 4, 4, 1.0, a, a, None]
        slot = null if null < 5 else {6: 6, 7: 10, 8: 11}[null]
        args[slot] = None
        assert f(*args) == _lib.SL_EINVAL, slot
    assert (buf == 0).all()


def test_unknown_emd_keyword():
    from safelife_amd.side_effects import side_effect_score, side_effect_scores
    boards = np.zeros((1, 4, 4), np.uint16)
    with pytest.raises(ValueError, match="emd"):
        side_effect_scores(boards, boards, [1], 0.0, 2, emd="bogus")
    with pytest.raises(ValueError, match="emd"):
        side_effect_scores(boards, boards, [1], 0.0, 2, problems="device", emd="bogus")

    class Game:
        _init_data = {"board": boards[0]}
        board, num_steps, spawn_prob = boards[0], 1, 0.0
    with pytest.raises(ValueError, match="emd"):
        side_effect_score(Game(), 2, emd="bogus")


def test_device_emd_needs_device_problems():
    from safelife_amd.side_effects import side_effect_score, side_effect_scores
    boards = np.zeros((1, 4, 4), np.uint16)
    with pytest.raises(ValueError, match="problems='device'"):
        side_effect_scores(boards, boards, [1], 0.0, 2, emd="device")
    with pytest.raises(ValueError, match="problems='device'"):
        side_effect_scores(boards, boards, [1], 0.0, 2, problems="host", emd="device")

    class Game:
        _init_data = {"board": boards[0]}
        board, num_steps, spawn_prob = boards[0], 1, 0.0
    with pytest.raises(ValueError, match="problems='device'"):
        side_effect_score(Game(), 2, problems="host", emd="device")


def test_node_counts_of_hand_made_problems():
    """emd_problem_nodes: supply bins + demand bins + the threshold column."""
    from safelife_amd.side_effects import emd_problem_nodes
    p = np.array([1.0, 0.0, 2.0, 0.5, 0.5, 0.0, 0.0, 3.0])
    q = np.array([0.0, 1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 3.0])
    #            one supply + one demand, equal      | 2 supplies + threshold | none
    offsets = [0, 2, 3, 5, 5, 7, 8]
    assert emd_problem_nodes(p, q, offsets).tolist() == [2, 0, 3, 0, 0, 0]
