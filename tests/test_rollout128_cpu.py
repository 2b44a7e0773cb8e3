"""(CPU) The 128x128 band rollout's host side: which kernel SL_KERNEL_AUTO launches
(sl_side_effect_kernel_auto), the SL_KERNEL_BANDS constant, and -- with the oracle alone --
that the inputs of tests/test_gpu_rollout_bands128.py (tests/rollout128_inputs.py) reach
the band seams and both outcomes of a spawn draw.  No GPU.

Conditions, not measurements: an input that stops meeting one no longer tests the seams.
"""
import os
import re

import pytest

import rollout128_inputs as ri

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from safelife_amd import _lib
    return _lib, _lib.lib()


def test_auto_kernel_entry(L):
    _lib, lib = L
    P, St = _lib.SL_RNG_PHILOX, _lib.SL_RNG_STREAM
    assert hasattr(lib, "sl_side_effect_kernel_auto")
    for shape in ((64, 64), (25, 25), (2, 2), (32, 64), (33, 20), (20, 65)):
        for mode in (P, St):
            assert (lib.sl_side_effect_kernel_auto(*shape, mode) ==
                    lib.sl_side_effect_kernel(*shape, mode)), (shape, mode)
    assert lib.sl_side_effect_kernel_auto(128, 128, St) == _lib.SL_KERNEL_GENERIC
    # the one-wave entry keeps its answer
    assert lib.sl_side_effect_kernel(128, 128, P) == _lib.SL_KERNEL_GENERIC


def test_auto_at_128_is_what_design_states(L):
    _lib, lib = L
    got = lib.sl_side_effect_kernel_auto(128, 128, _lib.SL_RNG_PHILOX)
    assert got in (_lib.SL_KERNEL_BANDS, _lib.SL_KERNEL_GENERIC)
    text = open(os.path.join(REPO, "DESIGN.md")).read()
    m = re.findall(r"`sl_side_effect_kernel_auto\(128, 128, SL_RNG_PHILOX\)`\s+returns\s+"
                   r"`SL_KERNEL_(BANDS|GENERIC)`", text)
    assert len(m) == 1, m
    assert got == {"BANDS": _lib.SL_KERNEL_BANDS, "GENERIC": _lib.SL_KERNEL_GENERIC}[m[0]]


def test_bands_constant_matches_the_header(L):
    _lib, _ = L
    assert _lib.SL_KERNEL_BANDS == 3
    text = open(os.path.join(REPO, "include", "safelife_hip.h")).read()
    assert int(re.search(r"^#define\s+SL_KERNEL_BANDS\s+(\d+)", text, re.M).group(1)) == 3
    assert "int sl_side_effect_kernel_auto(int H, int W, int rng_mode);" in text


@pytest.mark.parametrize("name", ["palette", "seam"])
def test_gpu_inputs_reach_the_seams(name):
    case = ri.palette_case() if name == "palette" else ri.seam_case()
    init = case[0]
    assert init.shape[1:] == (128, 128) and len(init) <= 7
    assert max(case[2]) <= 11 and max(case[4]) <= 4000000000
    rows, cols, spawned, stayed = ri.coverage(case)
    # a cell changes, in a sampled advance, in every row next to a seam and in both
    # columns of the wrap
    assert not [r for r in ri.SEAM_ROWS if r not in rows], sorted(rows)
    assert not [c for c in ri.SEAM_COLS if c not in cols], sorted(cols)
    # at 0 < p < 1, next to a seam, an eligible cell spawns and one does not
    assert spawned and stayed, (spawned, stayed)
    if name == "seam":
        # the seam board has a spawner at every seam: both outcomes on at least one
        # side of each
        for a, b in ((31, 32), (63, 64), (95, 96), (127, 0)):
            assert {a, b} & spawned and {a, b} & stayed, (a, b, spawned, stayed)


def test_palette_case_is_the_issue_s():
    init, final, steps, sp, ids = ri.palette_case()
    assert steps == [0, 1, 3, 11, 0, 2, 6]
    assert sp == [0.0, 0.3, 1.0, 0.3, 1.0, 0.0, 0.3]
    assert max(ids) == 4000000000
    assert 0.40 < float((init == 0).mean()) < 0.50
    assert ((init & 0x7000) != 0).any()             # bits 12-14
    from safelife_amd.cell_types import CELL_TYPE_NAMES
    for v, nm in CELL_TYPE_NAMES:
        assert ((init & 0xF1FF) == int(v)).any(), nm


def test_seam_board_is_as_described():
    b = ri.seam_board()
    life = {(int(y), int(x)) for y, x in zip(*((b == ri.LIFE).nonzero()))}
    for r0 in (31, 63, 95, 127):
        assert [c for c in range(128)
                if all(((r0 + d) % 128, c) in life for d in range(3))], r0
    assert all((16, c) in life for c in (127, 0, 1))
    sp = [int(y) for y in (b == ri.SPAWNER).nonzero()[0]]
    for seam in (31.5, 63.5, 95.5, 127.5):
        assert [y for y in sp if abs(y - seam) <= 2 or abs(y + 128 - seam) <= 2], seam
    assert int((b != 0).sum()) == 15 + 5
