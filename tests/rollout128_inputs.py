"""Inputs of the 128x128 band-rollout tests (tests/test_gpu_rollout_bands128.py), built
here so that tests/test_rollout128_cpu.py can check with the oracle alone that they
exercise what they are there for: the seams between the four bands of 32 rows (rows 31|32,
63|64, 95|96 and the wrap 127|0), the wrap of the columns (127|0), and spawn draws that go
both ways next to a seam.

The palette boards, the roll of the final boards and the oracle comparison are those of
tests/test_gpu_rollout_bits.py (loaded from the file, not copied).
"""
import importlib.util
import os

import numpy as np

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
N = 128
SEED = 77                   # the Philox seed of every call
S = 9                       # num_samples
SEAM_ROWS = (31, 32, 63, 64, 95, 96, 127, 0)
SEAM_COLS = (0, 127)

# the palette case: seven episodes, the schedule of test_gpu_rollout_bits.py
PALETTE_RNG = 128 * 100 + 128
STEPS = [0, 1, 3, 11, 0, 2, 6]
SPAWN = [0.0, 0.3, 1.0, 0.3, 1.0, 0.0, 0.3]
IDS = [3, 1000, 7, 65536, 12, 4000000000, 99]

# the seam case: one hand-made board, three episodes of it
SEAM_RNG = 5
SEAM_STEPS = [0, 4, 11]
SEAM_SPAWN = [0.3, 0.3, 0.3]
SEAM_IDS = [8, 70000, 3999999999]

LIFE = 9                    # alive | destructible
SPAWNER = 0x98 | 0x400      # frozen | spawning | destructible, green


def bits_helpers():
    """tests/test_gpu_rollout_bits.py as a module (its palette, _rolled, _check_vs_oracle and
    the episode-log helpers)."""
    spec = importlib.util.spec_from_file_location(
        "rollout_bits_helpers", os.path.join(HERE, "test_gpu_rollout_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def palette_case():
    """(init, final, steps, spawn_prob, env_ids): every cell type, bits 12-14, 45 % empty."""
    h = bits_helpers()
    rng = np.random.RandomState(PALETTE_RNG)
    init = h._palette_boards(rng, len(STEPS), N, N)
    final = h._rolled(rng, init)
    return init, final, STEPS, SPAWN, IDS


def seam_board():
    """Empty but for a blinker across each band seam (rows 31-33, 63-65, 95-97, 127-1), one
    across the column wrap (columns 127-1), and a spawner within two cells of each seam:
    in the last row of a band (31), in the first (64), one row off (94), on the wrap (127),
    and one in column 127 whose block reaches column 0."""
    b = np.zeros((N, N), dtype=np.uint16)
    for r0, c in ((31, 20), (63, 50), (95, 80), (127, 110)):
        for d in range(3):
            b[(r0 + d) % N, c] = LIFE
    for d in range(3):
        b[16, (127 + d) % N] = LIFE
    for r, c in ((31, 40), (64, 70), (94, 100), (127, 10), (50, 127)):
        b[r, c] = SPAWNER
    return b


def seam_case():
    h = bits_helpers()
    rng = np.random.RandomState(SEAM_RNG)
    init = np.stack([seam_board()] * len(SEAM_STEPS))
    final = h._rolled(rng, init)
    return init, final, SEAM_STEPS, SEAM_SPAWN, SEAM_IDS


def coverage(case, num_samples=S, seed=SEED):
    """The oracle's rollouts of a case.  Returns (rows, cols, spawned, stayed): the rows and
    columns in which a cell changed in a sampled advance, and the seam rows in which, in an
    episode with 0 < p < 1, an eligible cell spawned / did not spawn (an eligible cell is
    one that p = 1 and p = 0 advance differently)."""
    init, final, steps, sp, ids = case
    rows, cols, spawned, stayed = set(), set(), set(), set()
    for e in range(len(init)):
        p = np.float32(sp[e])
        for which, b, first in ((0, init[e], int(steps[e])), (1, final[e], 0)):
            b = np.array(b, dtype=np.uint16)
            for t in range(first + num_samples):
                kw = dict(rng=oracle.RNG_PHILOX, seed=seed, env_id=int(ids[e]), step=t,
                          tensor=4 + which)
                new = oracle.advance(b, p, **kw)[0]
                if t >= first:
                    ys, xs = np.nonzero(new != b)
                    rows |= set(ys.tolist())
                    cols |= set(xs.tolist())
                if 0.0 < p < 1.0:
                    always = oracle.advance(b, 1.0, **kw)[0]
                    never = oracle.advance(b, 0.0, **kw)[0]
                    elig = always != never
                    spawned |= set(np.nonzero(elig & (new == always))[0].tolist())
                    stayed |= set(np.nonzero(elig & (new == never))[0].tolist())
                b = new
    seam = set(SEAM_ROWS)
    return rows, cols, spawned & seam, stayed & seam
