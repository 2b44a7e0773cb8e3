"""Inputs of the tests of the band rollout of boards past 64 rows or columns
(tests/test_gpu_rollout_wide.py; kernel="wide": k_rollout_bits_wide,
sl_rollout_bits_wide.hip), built here so that tests/test_rollout_wide_cpu.py can check with
the oracle alone that they exercise what they are there for: every seam between two bands
of 32 rows (32k-1 | 32k), the wrap of the rows (H-1|0), the wrap of the columns (W-1|0),
and spawn draws that go both ways next to every row seam.

The cases, the coverage walk and the seam board's pieces are those of
tests/rollout_mid_inputs.py, the palette boards, the roll of the final boards and the oracle
comparison those of tests/test_gpu_rollout_bits.py (both loaded from their files, not
copied).  The mid inputs are loaded as a module of this file's own, so that its seam rows
and its table of generator seeds can be these boards' without touching the module the mid
tests import.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _mid_inputs():
    spec = importlib.util.spec_from_file_location(
        "rollout_mid_inputs_for_wide", os.path.join(HERE, "rollout_mid_inputs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_mid = _mid_inputs()

SEED, S = _mid.SEED, _mid.S                 # 77, 9
STEPS, SPAWN, IDS = _mid.STEPS, _mid.SPAWN, _mid.IDS
SEAM_STEPS, SEAM_SPAWN, SEAM_IDS = _mid.SEAM_STEPS, _mid.SEAM_SPAWN, _mid.SEAM_IDS
LIFE, SPAWNER = _mid.LIFE, _mid.SPAWNER
bits_helpers = _mid.bits_helpers

# NB = 1 (up and dn from the wave itself): 2x66, 7x65, 32x128; one real row in the last band
# at NB = 2, 3, 4: 33x65, 65x2 and 65x65, 97x3; full last bands: 32x128, 64x127, 96x96,
# 128x127; odd W with nl < 64: 7x65, 33x65, 65x65, 97x3; odd W with nl = 64 (the copy word
# in lane 63): 64x127, 128x127; W = 2 (a lane is its own column neighbour): 65x2; full
# width: 32x128, 40x128; uint16 loads at every odd W, dword loads at every even W
SHAPES = [(2, 66), (7, 65), (32, 128), (33, 65), (40, 128), (64, 127), (65, 2), (65, 65),
          (96, 96), (97, 3), (100, 100), (128, 127)]
SEAM_SHAPES = [(33, 65), (65, 65), (100, 100), (128, 127)]

# the boards' generator seed is 100 H + W + 10000 k, k the first at which the boards meet
# the seam conditions of test_rollout_wide_cpu.py: 0 but for the narrow boards, where few
# cells lie next to a seam
PALETTE_K = {(65, 2): 6, (97, 3): 11}
_mid.PALETTE_K = PALETTE_K


def bands(H):
    return (H + 31) // 32


def seam_pairs(H):
    """The row pairs a halo row crosses: every band seam, then the wrap."""
    return [(32 * k - 1, 32 * k) for k in range(1, bands(H))] + [(H - 1, 0)]


def seam_rows(H):
    return tuple(r for pair in seam_pairs(H) for r in pair)


_mid.seam_rows = seam_rows                  # coverage() keeps the spawn outcomes of these rows
coverage = _mid.coverage
palette_case = _mid.palette_case            # (with PALETTE_K above)
soup_case = _mid.soup_case


def seam_board(shape):
    """seam_board of the mid inputs -- a blinker across rows 31|32, one across the row wrap,
    one across the column wrap, spawners within two cells of both row seams and one in
    column W-1 -- with its rows taken modulo H (at H = 33 row 33 is row 0), and for every
    further band seam 32k-1 | 32k, k = 2 .. NB-1, 20 (k-1) columns to the right of the first
    seam's: a blinker across it (rows 32k-1 .. 32k+1) and a spawner pair, one in row 32k-1
    and one in row 32k+1."""
    H, W = shape
    b = np.zeros((H, W), dtype=np.uint16)
    for k in range(1, bands(H)):
        dc = 20 * (k - 1)
        for d in range(3):
            b[(32 * k - 1 + d) % H, 3 + dc] = LIFE
        b[32 * k - 1, 6 + dc] = SPAWNER
        b[(32 * k + 1) % H, 12 + dc] = SPAWNER
    for d in range(3):
        b[(H - 1 + d) % H, 9] = LIFE
        b[16, (W - 1 + d) % W] = LIFE
    for r, c in ((H - 1, 14), (1, 17), (24, W - 1)):
        b[r, c] = SPAWNER
    return b


def seam_case(shape):
    h = bits_helpers()
    rng = np.random.RandomState(_mid.SEAM_RNG)
    init = np.stack([seam_board(shape)] * len(SEAM_STEPS))
    final = h._rolled(rng, init)
    return init, final, SEAM_STEPS, SEAM_SPAWN, SEAM_IDS
