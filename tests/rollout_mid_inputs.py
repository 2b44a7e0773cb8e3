"""Inputs of the tests of the one-wave rollout of boards of 33 to 64 rows
(tests/test_gpu_rollout_mid.py; kernel="mid": k_rollout_bits_mid, sl_rollout_bits_mid.hip),
built here so that tests/test_rollout_mid_cpu.py can check with the oracle alone that they
exercise what they are there for: the seam between the two halves of the rows (31|32), the
wrap of the rows (H-1|0), the wrap of the columns (W-1|0), and spawn draws that go both
ways next to a row seam.

The palette boards, the roll of the final boards and the oracle comparison are those of
tests/test_gpu_rollout_bits.py (loaded from the file, not copied).
"""
import importlib.util
import os

import numpy as np

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 77                   # the Philox seed of every call
S = 9                       # num_samples

# H - 33 = 0 (one upper row) at W = 2 and odd W; nl odd (7 -> 4, 21 -> 11); odd and even W;
# W = 2 (a lane is its own column neighbour) at both ends of H; full width; H = 64 at odd W
SHAPES = [(33, 2), (33, 33), (34, 7), (40, 21), (48, 48), (47, 64), (63, 64), (64, 63), (64, 2)]
SEAM_SHAPES = [(40, 21), (47, 64), (64, 63)]

# the palette case: seven episodes, the schedule of test_gpu_rollout_bits.py
STEPS = [0, 1, 3, 11, 0, 2, 6]
SPAWN = [0.0, 0.3, 1.0, 0.3, 1.0, 0.0, 0.3]
IDS = [3, 1000, 7, 65536, 12, 4000000000, 99]
# the boards' generator seed is 100 H + W (test_gpu_rollout_bits.py) + 10000 k, k the first
# at which the boards meet the seam conditions of test_rollout_mid_cpu.py: 0 but for the
# two-column boards, where few cells lie next to a seam
PALETTE_K = {(33, 2): 2, (64, 2): 3}

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


def seam_rows(H):
    return (31, 32, H - 1, 0)


def palette_case(shape):
    """(init, final, steps, spawn_prob, env_ids): every cell type, bits 12-14, 45 % empty."""
    H, W = shape
    h = bits_helpers()
    rng = np.random.RandomState(100 * H + W + 10000 * PALETTE_K.get(shape, 0))
    init = h._palette_boards(rng, len(STEPS), H, W)
    final = h._rolled(rng, init)
    return init, final, STEPS, SPAWN, IDS


def seam_board(shape):
    """Empty but for a blinker across rows 31|32 (rows 31-33), one across the row wrap (rows
    H-1, 0, 1), one across the column wrap (columns W-1, 0, 1), and spawners within two
    cells of each row seam -- in row 31, in row 33 (one row off), in row H-1 and in row 1 --
    and one in column W-1 whose block reaches column 0."""
    H, W = shape
    b = np.zeros((H, W), dtype=np.uint16)
    for r0, c in ((31, 3), (H - 1, 9)):
        for d in range(3):
            b[(r0 + d) % H, c] = LIFE
    for d in range(3):
        b[16, (W - 1 + d) % W] = LIFE
    for r, c in ((31, 6), (33, 12), (H - 1, 14), (1, 17), (24, W - 1)):
        b[r, c] = SPAWNER
    return b


def seam_case(shape):
    h = bits_helpers()
    rng = np.random.RandomState(SEAM_RNG)
    init = np.stack([seam_board(shape)] * len(SEAM_STEPS))
    final = h._rolled(rng, init)
    return init, final, SEAM_STEPS, SEAM_SPAWN, SEAM_IDS


def soup_case(shape, E=5, values=40):
    """E boards of 16-bit cells restricted to `values` distinct values (any bit pattern,
    spawners and bits 12-14 as they fall), half of them empty: more would exceed max_keys
    on boards this large."""
    H, W = shape
    rng = np.random.RandomState(7000 + 100 * H + W)
    pal = rng.randint(1, 65536, size=values).astype(np.uint16)
    init = pal[rng.randint(0, values, size=(E, H, W))]
    init[rng.rand(E, H, W) < 0.5] = 0
    init = init.astype(np.uint16)
    final = bits_helpers()._rolled(rng, init)
    return init, final, [0, 3, 11, 1, 6][:E], [0.3, 0.0, 1.0, 0.3, 0.3][:E], \
        [5, 6, 900, 4000000000, 31][:E]


def coverage(case, num_samples=S, seed=SEED):
    """The oracle's rollouts of a case.  Returns (rows, cols, spawned, stayed): the rows and
    columns in which a cell changed in a sampled advance, and the seam rows in which, in an
    episode with 0 < p < 1, an eligible cell spawned / did not spawn (an eligible cell is
    one that p = 1 and p = 0 advance differently)."""
    init, final, steps, sp, ids = case
    H = init.shape[1]
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
    seam = set(seam_rows(H))
    return rows, cols, spawned & seam, stayed & seam
