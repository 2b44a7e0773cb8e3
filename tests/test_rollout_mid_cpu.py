"""(CPU) The host side of the one-wave rollout of boards of 33 to 64 rows (kernel="mid",
SL_KERNEL_MID): the constant, the answers of sl_side_effect_kernel (unchanged) and of
sl_side_effect_kernel_auto (SL_KERNEL_MID or SL_KERNEL_GENERIC on mid shapes of at least
32 columns with Philox draws, as DESIGN.md states), and -- with the oracle alone -- that
the inputs of tests/test_gpu_rollout_mid.py (tests/rollout_mid_inputs.py) reach the seam
between the two halves of the rows, both wraps and both outcomes of a spawn draw.  No GPU.

Conditions, not measurements: an input that stops meeting one no longer tests the seams.
"""
import os
import re

import numpy as np
import pytest

import oracle
import rollout_mid_inputs as mi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO_SHAPES = [(33, 32), (48, 48), (64, 63), (35, 64)]


@pytest.fixture(scope="module")
def L():
    from safelife_amd import _lib
    return _lib, _lib.lib()


def test_mid_constant_matches_the_header(L):
    _lib, _ = L
    assert _lib.SL_KERNEL_MID == 4
    text = open(os.path.join(REPO, "include", "safelife_hip.h")).read()
    assert int(re.search(r"^#define\s+SL_KERNEL_MID\s+(\d+)", text, re.M).group(1)) == 4


def test_one_wave_entry_keeps_its_answers(L):
    _lib, lib = L
    for shape in ((33, 20), (48, 48), (64, 48), (40, 70), (65, 40)):
        for mode in (_lib.SL_RNG_PHILOX, _lib.SL_RNG_STREAM):
            assert lib.sl_side_effect_kernel(*shape, mode) == _lib.SL_KERNEL_GENERIC, shape


def test_auto_on_mid_shapes(L):
    _lib, lib = L
    P, St = _lib.SL_RNG_PHILOX, _lib.SL_RNG_STREAM
    got = {lib.sl_side_effect_kernel_auto(*shape, P) for shape in AUTO_SHAPES}
    assert len(got) == 1, got
    assert got <= {_lib.SL_KERNEL_MID, _lib.SL_KERNEL_GENERIC}, got
    for shape in AUTO_SHAPES:
        assert lib.sl_side_effect_kernel_auto(*shape, St) == _lib.SL_KERNEL_GENERIC, shape
    # narrower than half a wave's lanes, or no mid shape at all
    for shape in ((33, 20), (48, 31), (40, 70), (65, 40)):
        for mode in (P, St):
            assert lib.sl_side_effect_kernel_auto(*shape, mode) == _lib.SL_KERNEL_GENERIC, shape


def test_auto_elsewhere_is_unchanged(L):
    _lib, lib = L
    P, St = _lib.SL_RNG_PHILOX, _lib.SL_RNG_STREAM
    for shape in ((64, 64), (25, 25)):
        assert lib.sl_side_effect_kernel_auto(*shape, P) == _lib.SL_KERNEL_FAST, shape
        assert lib.sl_side_effect_kernel_auto(*shape, St) == _lib.SL_KERNEL_GENERIC, shape
    assert lib.sl_side_effect_kernel_auto(128, 128, P) in (_lib.SL_KERNEL_BANDS,
                                                           _lib.SL_KERNEL_GENERIC)
    assert lib.sl_side_effect_kernel_auto(128, 128, St) == _lib.SL_KERNEL_GENERIC


def test_auto_at_48_is_what_design_states(L):
    _lib, lib = L
    got = lib.sl_side_effect_kernel_auto(48, 48, _lib.SL_RNG_PHILOX)
    assert got in (_lib.SL_KERNEL_MID, _lib.SL_KERNEL_GENERIC)
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.findall(r"`sl_side_effect_kernel_auto\(48, 48, SL_RNG_PHILOX\)`\s+returns\s+"
                   r"`SL_KERNEL_(MID|GENERIC)`", text)
    assert len(m) == 1, m
    assert got == {"MID": _lib.SL_KERNEL_MID, "GENERIC": _lib.SL_KERNEL_GENERIC}[m[0]]


def test_env_step_family_does_not_know_mid(L):
    _lib, lib = L
    assert lib.sl_env_step_family(48, 48, _lib.SL_KERNEL_MID) == _lib.SL_EINVAL


def test_the_shapes_are_the_issue_s():
    assert mi.SHAPES == [(33, 2), (33, 33), (34, 7), (40, 21), (48, 48), (47, 64), (63, 64),
                         (64, 63), (64, 2)]
    assert mi.SEAM_SHAPES == [(40, 21), (47, 64), (64, 63)]
    assert mi.STEPS == [0, 1, 3, 11, 0, 2, 6]
    assert mi.SPAWN == [0.0, 0.3, 1.0, 0.3, 1.0, 0.0, 0.3]
    assert max(mi.IDS) == 4000000000 and mi.S == 9 and mi.SEED == 77


def _check_rows_and_columns(case, shape):
    H, W = shape
    rows, cols, spawned, stayed = mi.coverage(case)
    # a cell changes, in a sampled advance, in every row next to a row seam and in both
    # columns of the wrap
    assert not [r for r in mi.seam_rows(H) if r not in rows], sorted(rows)
    assert not [c for c in (0, W - 1) if c not in cols], sorted(cols)
    return spawned, stayed


@pytest.mark.parametrize("shape", mi.SHAPES, ids=lambda s: "%dx%d" % s)
def test_palette_inputs_reach_the_seams(shape):
    case = mi.palette_case(shape)
    assert case[0].shape == (7,) + shape
    spawned, stayed = _check_rows_and_columns(case, shape)
    # at 0 < p < 1, next to each row seam, an eligible cell spawns and one does not
    for a, b in ((31, 32), (shape[0] - 1, 0)):
        assert {a, b} & spawned and {a, b} & stayed, (a, b, spawned, stayed)


@pytest.mark.parametrize("shape", mi.SEAM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_seam_inputs_reach_the_seams(shape):
    H, W = shape
    case = mi.seam_case(shape)
    spawned, stayed = _check_rows_and_columns(case, shape)
    # the seam board has spawners at both row seams: both outcomes on at least one side
    # of each
    for a, b in ((31, 32), (H - 1, 0)):
        assert {a, b} & spawned and {a, b} & stayed, (a, b, spawned, stayed)


@pytest.mark.parametrize("shape", mi.SEAM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_seam_board_is_as_described(shape):
    H, W = shape
    b = mi.seam_board(shape)
    life = {(int(y), int(x)) for y, x in zip(*((b == mi.LIFE).nonzero()))}
    for r0 in (31, H - 1):
        assert [c for c in range(W) if all(((r0 + d) % H, c) in life for d in range(3))], r0
    assert all((16, c) in life for c in (W - 1, 0, 1))
    ys, xs = (b == mi.SPAWNER).nonzero()
    for seam in (31.5, H - 0.5):
        assert [y for y in ys if abs(y - seam) <= 2 or abs(y + H - seam) <= 2], seam
    assert W - 1 in xs.tolist()
    assert int((b != 0).sum()) == 9 + 5


@pytest.mark.parametrize("shape", [(33, 33), (47, 64), (64, 63)], ids=lambda s: "%dx%d" % s)
def test_soup_case_keeps_to_its_values_and_keys(shape):
    """At most 40 distinct cell values, and (oracle) no episode with more keys than the
    max_keys = 256 the GPU test gives it."""
    init, final, steps, sp, ids = mi.soup_case(shape)
    assert init.shape == (5,) + shape
    assert len(np.unique(init)) <= 41                   # 40 values and empty
    assert ((init & 0x7000) != 0).any() and ((init & 0x80) != 0).any()
    for e in range(len(init)):
        ina, act = oracle.side_effect_densities(init[e], final[e], int(steps[e]),
                                                np.float32(sp[e]), mi.S, rng="philox",
                                                seed=mi.SEED, env_id=int(ids[e]))
        assert 8 < len(set(ina) | set(act)) <= 256, (e, len(set(ina) | set(act)))
