"""Cases and data of the tests of the bit-sliced step kernel for boards of 33 to 64 rows
(k_env_step_mid): shared by tests/test_mid_boards_cpu.py, which checks on the oracle that
each case exercises what it is there for, and tests/test_gpu_mid_boards.py, which runs
them on the device with the same seeds.
"""
import numpy as np

import feature_pools as fp

MID = "mid"

# the smallest shapes at which each part of the geometry can go wrong
CASES = [
    # one real row in the upper half; the odd-W column-0 copy
    fp.Case("mid-33x33", (33, 33), MID, "fast", n_exits=8, toggles=True, period=1, view=(9, 9),
            B=25, seed=40),
    # nl = 1: a lane is its own left and right neighbour
    fp.Case("mid-33x2", (33, 2), MID, "fast", n_exits=1, period=0, B=26, seed=41),
    # odd W at nearly full width
    fp.Case("mid-34x63", (34, 63), MID, "fast", n_exits=2, period=16, view=(33, 33),
            remove_white=False, B=27, seed=42),
    # nl = 32: the permute wrap is the whole wave; odd H (half a spawn block in the last row)
    fp.Case("mid-47x64", (47, 64), MID, "fast", n_exits=2, toggles=True, period=4, min_perf=0.5,
            B=26, seed=43),
    # full height: the wrap must equal the 64x64 layout's; odd W
    fp.Case("mid-64x63", (64, 63), MID, "fast", n_exits=8, exit_rows=(31, 32, 63, 0),
            view=(8, 12), B=25, seed=44),
    # odd H at full width
    fp.Case("mid-63x64", (63, 64), MID, "fast", n_exits=1, period=4, min_perf=0.01, B=27,
            seed=45),
    # narrow: 20 of 64 lanes hold cells
    fp.Case("mid-40x20", (40, 20), MID, "fast", n_exits=2, period=1, B=26, seed=46),
    # full height, few lanes
    fp.Case("mid-64x34", (64, 34), MID, "fast", n_exits=2, toggles=True, B=25, seed=47),
]
STREAM_CASES = [
    fp.Case("mid-33x33-stream", (33, 33), MID, "fast", n_exits=8, toggles=True, period=1,
            view=(9, 9), B=25, rng="stream", seed=48),
    fp.Case("mid-47x64-stream", (47, 64), MID, "fast", n_exits=2, toggles=True, period=4,
            min_perf=0.5, B=26, rng="stream", seed=49),
]
ALL_CASES = CASES + STREAM_CASES
CASE_IDS = [c.name for c in ALL_CASES]

SOUP_SHAPES = [(33, 33), (47, 64), (64, 63)]
USED_BITS = 0b1000111111111111          # bits 0-11 and 15


def soup_levels(H, W, K=9):
    """K levels whose board and goals are random over all 16 cell bits, spawners
    included: the three kinds of random board the advance's known-answer fixture
    (advance_known_answers.npz) is made of -- all used bits; a life-like soup with sparse
    special cells; every bit pattern -- thinned to a random density; p in {0, 0.3, 1}.
    (Of the board's exit bits all but a few are cleared: see below.)"""
    rng = np.random.RandomState(H * 1000 + W)

    def soup(i):
        mode = i % 3
        if mode == 0:
            b = rng.randint(0, 1 << 16, size=(H, W)).astype(np.uint16) & np.uint16(USED_BITS)
        elif mode == 1:
            b = np.where(rng.rand(H, W) < 0.5, 9, 1).astype(np.uint16)
            b |= (rng.randint(0, 8, size=(H, W)) << 9).astype(np.uint16)
            special = rng.rand(H, W) < 0.1
            b[special] |= rng.choice([16, 32, 64, 128, 152, 256, 4, 32768],
                                     size=special.sum()).astype(np.uint16)
        else:
            b = rng.randint(0, 1 << 16, size=(H, W)).astype(np.uint16)
        return (b * (rng.rand(H, W) < rng.uniform(0.05, 0.95))).astype(np.uint16)

    out = []
    for k in range(K):
        board, goals = soup(k), soup(k + 1)
        # a level holds at most eight exits (LevelPool): the board keeps bit 8 on the
        # first six cells that drew it, next to the exit placed below
        ey, ex = np.nonzero(board & 0x100)
        board[ey[6:], ex[6:]] &= np.uint16(0xFEFF)
        ax, ay = int(rng.randint(W)), int(rng.randint(H))
        board[ay, ax] = 122                                     # the agent
        board[(ay + H // 2) % H, (ax + W // 2) % W] = 272       # an exit
        out.append({"board": board, "goals": goals, "agent_loc": np.array([ax, ay]),
                    "orientation": int(rng.randint(4)), "spawn_prob": (0.0, 0.3, 1.0)[k % 3],
                    "min_performance": 0.01})
    return out
