"""(CPU) The host side of the band rollout of boards past 64 rows or columns (kernel="wide",
SL_KERNEL_WIDE in sl_side_effect_densities_k): the constant, the answers of
sl_side_effect_kernel and sl_side_effect_kernel_auto (unchanged: the kernel is opt-in), the
entry's checks that need no device, and -- with the oracle alone -- that the inputs of
tests/test_gpu_rollout_wide.py (tests/rollout_wide_inputs.py) reach every seam between two
bands of 32 rows, both wraps and both outcomes of a spawn draw.  No GPU.

Conditions, not measurements: an input that stops meeting one no longer tests the seams.
"""
import os
import re

import numpy as np
import pytest

import oracle
import rollout_mid_inputs as mi
import rollout_wide_inputs as wi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOUP_SHAPES = [(33, 65), (96, 96), (128, 127)]


@pytest.fixture(scope="module")
def L():
    from safelife_amd import _lib
    return _lib, _lib.lib()


def test_wide_constant_matches_the_header(L):
    _lib, _ = L
    assert _lib.SL_KERNEL_WIDE == 5
    text = open(os.path.join(REPO, "include", "safelife_hip.h")).read()
    assert int(re.search(r"^#define\s+SL_KERNEL_WIDE\s+(\d+)", text, re.M).group(1)) == 5


def test_both_entries_answer_generic_on_wide_shapes(L):
    _lib, lib = L
    for shape in wi.SHAPES:
        for mode in (_lib.SL_RNG_PHILOX, _lib.SL_RNG_STREAM):
            assert lib.sl_side_effect_kernel(*shape, mode) == _lib.SL_KERNEL_GENERIC, shape
            assert lib.sl_side_effect_kernel_auto(*shape, mode) == _lib.SL_KERNEL_GENERIC, shape


def test_both_entries_answer_as_before_elsewhere(L):
    _lib, lib = L
    P, St = _lib.SL_RNG_PHILOX, _lib.SL_RNG_STREAM
    for shape in ((64, 64), (25, 25)):
        assert lib.sl_side_effect_kernel(*shape, P) == _lib.SL_KERNEL_FAST, shape
        assert lib.sl_side_effect_kernel_auto(*shape, P) == _lib.SL_KERNEL_FAST, shape
    assert lib.sl_side_effect_kernel(48, 48, P) == _lib.SL_KERNEL_GENERIC
    assert lib.sl_side_effect_kernel_auto(48, 48, P) == _lib.SL_KERNEL_MID
    assert lib.sl_side_effect_kernel(128, 128, P) == _lib.SL_KERNEL_GENERIC
    assert lib.sl_side_effect_kernel_auto(128, 128, P) == _lib.SL_KERNEL_BANDS
    for shape in ((64, 64), (25, 25), (48, 48), (128, 128)):
        assert lib.sl_side_effect_kernel(*shape, St) == _lib.SL_KERNEL_GENERIC, shape
        assert lib.sl_side_effect_kernel_auto(*shape, St) == _lib.SL_KERNEL_GENERIC, shape


def _densities_k_without_episodes(lib, _lib, shape, kernel):
    h, w = shape
    return lib.sl_side_effect_densities_k(None, None, None, None, None, 0, h, w, 3,
                                          _lib.SL_RNG_PHILOX, 1, 0, None, None, 16, None, None,
                                          None, None, None, None, 0, None, kernel, None)


def test_the_entry_knows_wide_and_no_kernel_6(L):
    """E = 0: the checks that need no device."""
    _lib, lib = L
    for shape in ((65, 65), (40, 128), (2, 66)):
        assert _densities_k_without_episodes(lib, _lib, shape, _lib.SL_KERNEL_WIDE) == _lib.SL_OK
        assert _densities_k_without_episodes(lib, _lib, shape, 6) == _lib.SL_EINVAL


def test_the_shapes_are_the_issue_s():
    assert wi.SHAPES == [(2, 66), (7, 65), (32, 128), (33, 65), (40, 128), (64, 127), (65, 2),
                         (65, 65), (96, 96), (97, 3), (100, 100), (128, 127)]
    assert wi.SEAM_SHAPES == [(33, 65), (65, 65), (100, 100), (128, 127)]
    assert wi.PALETTE_K == {(65, 2): 6, (97, 3): 11}
    assert (wi.STEPS, wi.SPAWN, wi.IDS) == (mi.STEPS, mi.SPAWN, mi.IDS)
    assert wi.S == 9 and wi.SEED == 77
    # the mid tests' module keeps its own seam rows and seeds
    assert mi.seam_rows(40) == (31, 32, 39, 0) and mi.PALETTE_K == {(33, 2): 2, (64, 2): 3}


def test_seam_rows():
    assert wi.seam_rows(2) == (1, 0) and wi.seam_rows(32) == (31, 0)
    assert wi.seam_rows(33) == (31, 32, 32, 0)
    assert wi.seam_rows(100) == (31, 32, 63, 64, 95, 96, 99, 0)
    assert wi.seam_rows(128) == (31, 32, 63, 64, 95, 96, 127, 0)


def _check_reaches_the_seams(case, shape):
    H, W = shape
    rows, cols, spawned, stayed = wi.coverage(case)
    # a cell changes, in a sampled advance, in every row next to a row seam and in both
    # columns of the wrap
    assert not [r for r in wi.seam_rows(H) if r not in rows], sorted(rows)
    assert not [c for c in (0, W - 1) if c not in cols], sorted(cols)
    # at 0 < p < 1, next to each row seam, an eligible cell spawns and one does not
    for a, b in wi.seam_pairs(H):
        assert {a, b} & spawned and {a, b} & stayed, (a, b, spawned, stayed)


@pytest.mark.parametrize("shape", wi.SHAPES, ids=lambda s: "%dx%d" % s)
def test_palette_inputs_reach_the_seams(shape):
    case = wi.palette_case(shape)
    assert case[0].shape == (7,) + shape
    k = wi.PALETTE_K.get(shape, 0)
    rng = np.random.RandomState(100 * shape[0] + shape[1] + 10000 * k)
    assert np.array_equal(case[0], wi.bits_helpers()._palette_boards(rng, 7, *shape))
    _check_reaches_the_seams(case, shape)


@pytest.mark.parametrize("shape", sorted(wi.PALETTE_K), ids=lambda s: "%dx%d" % s)
def test_palette_k_is_the_first_that_reaches_the_seams(shape):
    saved = dict(wi.PALETTE_K)
    try:
        for k in range(saved[shape]):
            wi.PALETTE_K[shape] = k
            with pytest.raises(AssertionError):
                _check_reaches_the_seams(wi.palette_case(shape), shape)
    finally:
        wi.PALETTE_K.clear()
        wi.PALETTE_K.update(saved)


@pytest.mark.parametrize("shape", wi.SHAPES, ids=lambda s: "%dx%d" % s)
def test_palette_inputs_keep_to_128_keys(shape):
    """(oracle) no episode with more density keys than the max_keys = 128 of the GPU test."""
    init, final, steps, sp, ids = wi.palette_case(shape)
    for e in range(len(init)):
        ina, act = oracle.side_effect_densities(init[e], final[e], int(steps[e]),
                                                np.float32(sp[e]), wi.S, rng="philox",
                                                seed=wi.SEED, env_id=int(ids[e]))
        assert 0 < len(set(ina) | set(act)) <= 128, (e, len(set(ina) | set(act)))


@pytest.mark.parametrize("shape", wi.SEAM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_seam_inputs_reach_the_seams(shape):
    _check_reaches_the_seams(wi.seam_case(shape), shape)


@pytest.mark.parametrize("shape", wi.SEAM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_seam_board_is_as_described(shape):
    H, W = shape
    NB = wi.bands(H)
    b = wi.seam_board(shape)
    if H >= 34:                 # the mid inputs' board, whole, under what was added
        m = mi.seam_board(shape)
        assert np.array_equal(b[m != 0], m[m != 0])
        assert int(((b != 0) & (m == 0)).sum()) == 5 * (NB - 2)
    life = {(int(y), int(x)) for y, x in zip(*((b == wi.LIFE).nonzero()))}
    ys, xs = (b == wi.SPAWNER).nonzero()
    for a, _ in wi.seam_pairs(H):
        # a blinker across the seam, and spawners within two cells of it on both sides
        assert [c for c in range(W) if all(((a + d) % H, c) in life for d in range(3))], a
        assert [y for y in ys if y == a] and [y for y in ys if y == (a + 2) % H], a
    assert all((16, c) in life for c in (W - 1, 0, 1))
    assert W - 1 in xs.tolist()
    assert int((b != 0).sum()) == 9 + 5 + 5 * (NB - 2)


@pytest.mark.parametrize("shape", SOUP_SHAPES, ids=lambda s: "%dx%d" % s)
def test_soup_case_keeps_to_its_values_and_keys(shape):
    """At most 40 distinct cell values, and (oracle) no episode with more keys than the
    max_keys = 256 the GPU test gives it."""
    init, final, steps, sp, ids = wi.soup_case(shape)
    assert init.shape == (5,) + shape
    assert len(np.unique(init)) <= 41                   # 40 values and empty
    assert ((init & 0x7000) != 0).any() and ((init & 0x80) != 0).any()
    for e in range(len(init)):
        ina, act = oracle.side_effect_densities(init[e], final[e], int(steps[e]),
                                                np.float32(sp[e]), wi.S, rng="philox",
                                                seed=wi.SEED, env_id=int(ids[e]))
        assert 8 < len(set(ina) | set(act)) <= 256, (e, len(set(ina) | set(act)))
