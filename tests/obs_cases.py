"""Cases and states of the tests of the stand-alone observation kernels behind sl_env_obs
(k_env_obs_packed, k_env_obs_channels<1|2|4> and the LDS-staged k_env_obs; sl_env.hip,
sl_obs.h): shared by tests/test_obs_cases_cpu.py, which checks on the oracle that the
cases exercise what they are there for, and tests/test_gpu_obs_matrix.py, which runs them
on the device with the same seeds.  tests/golden/make_golden.py (gen_obs) builds the
states of tests/golden/obs_views.npz from FIXTURE_SPECS.

A case is a board shape, B, a view shape, an element mode, a channel list,
remove_white_goals, whether the output starts one element past an aligned address, and a
seed.  The seed makes B explicit states: board and goals random over all 16 bits and
thinned to a random density, an agent cell and an exit list of 0 to 8 cells.  The exit
list is explicit (the kernels read exit_y / exit_x, in list order) and of a STYLE that
env b of a case picks by (seed + b): none, eight random cells, several cells that clip
onto one border cell of the view, a cell for each view corner, cells at wrapped distance
exactly -(H // 2) and -(W // 2), or cells inside the view with random ones after them.
"""
import os
import re

import numpy as np

import oracle

MODES = ("packed", "uint16", "uint8", "float32", "bfloat16")
ESZ = {"packed": 2, "uint16": 2, "uint8": 1, "float32": 4, "bfloat16": 2}
# an element's 1, as the raw bits the kernels store
ONE = {"uint16": 1, "uint8": 1, "float32": 0x3F800000, "bfloat16": 0x3F80}
MAX_EXITS = 8
RAINBOW = 0x0E00

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "safelife-k2_amd", "csrc")


def _constant(fname, name):
    text = open(os.path.join(_SRC, fname)).read()
    return int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text).group(1))


WAVE_MAX_CELLS = _constant("sl_obs.h", "kObsMaxCells")     # last size of the wave kernels
MAX_CELLS = _constant("sl_env.hip", "kMaxCells")           # last size obs_args accepts

CHANNEL_LISTS = [
    tuple(range(15)),
    tuple(range(16)),
    (15,),
    (0,),
    (3, 0, 9, 14),
    (5, 5, 2),                       # a repeated channel
    tuple(range(15, -1, -1)),
]


# ----------------------------------------------------------------------------- states
def exit_targets(H, W, vh, vw, y0, x0):
    """For every board cell: the flat view index an exit on it is moved to
    (helper_utils.py:64-72), and whether the clip moved it."""
    jy = (np.arange(H) - y0 + H // 2) % H - H // 2 + vh // 2
    jx = (np.arange(W) - x0 + W // 2) % W - W // 2 + vw // 2
    cy, cx = np.clip(jy, 0, vh - 1), np.clip(jx, 0, vw - 1)
    return cy[:, None] * vw + cx[None, :], (cy != jy)[:, None] | (cx != jx)[None, :]


def _soup(rng, H, W):
    b = rng.randint(0, 1 << 16, size=(H, W)).astype(np.uint16)
    return (b * (rng.rand(H, W) < rng.uniform(0.05, 0.95))).astype(np.uint16)


def _random_cells(rng, H, W, n, taken=()):
    taken = set(taken)
    cells = [(int(c // W), int(c % W)) for c in rng.permutation(H * W)[:n + len(taken)]]
    return [c for c in cells if c not in taken][:n]


STYLES = ("none", "full", "stack", "corners", "half", "inside")


def place_exits(rng, style, H, W, vh, vw, y0, x0):
    """The exit list of one env, [(iy, ix)], distinct cells in list order."""
    tgt, clipped = exit_targets(H, W, vh, vw, y0, x0)
    if style == "none":
        return []
    if style == "full":
        return _random_cells(rng, H, W, MAX_EXITS)
    if style == "stack":
        # two or three cells that clip onto one border cell (where the view leaves any)
        groups = {}
        for y, x in zip(*np.nonzero(clipped)):
            groups.setdefault(int(tgt[y, x]), []).append((int(y), int(x)))
        groups = [g for _, g in sorted(groups.items()) if len(g) >= 2]
        if not groups:
            return _random_cells(rng, H, W, 3)
        g = groups[rng.randint(len(groups))]
        n = min(len(g), 2 + rng.randint(2))
        pick = [g[i] for i in rng.permutation(len(g))[:n]]
        return pick + _random_cells(rng, H, W, rng.randint(3), pick)
    if style == "corners":
        out = []
        for corner in (0, vw - 1, (vh - 1) * vw, vh * vw - 1):
            cells = [(int(y), int(x)) for y, x in zip(*np.nonzero(tgt == corner))
                     if (int(y), int(x)) not in out]
            if cells:
                out.append(cells[rng.randint(len(cells))])
        return out
    if style == "half":
        a = ((y0 - H // 2) % H, int(rng.randint(W)))
        b = (int(rng.randint(H)), (x0 - W // 2) % W)
        return [a] if a == b else [a, b]
    if style == "inside":
        cells = [(int(y), int(x)) for y, x in zip(*np.nonzero(~clipped))]
        pick = [cells[i] for i in rng.permutation(len(cells))[:1 + rng.randint(2)]]
        return pick + _random_cells(rng, H, W, rng.randint(4), pick)
    raise ValueError(style)


def make_state(rng, shape, view, style):
    """One state: board, goals, agent cell and exit list.  The exit cells get board
    values of their own and empty goals, so that exits sharing a target differ."""
    H, W = shape
    board, goals = _soup(rng, H, W), _soup(rng, H, W)
    ax, ay = int(rng.randint(W)), int(rng.randint(H))
    exits = place_exits(rng, style, H, W, view[0], view[1], ay, ax)
    if style in ("stack", "corners"):
        vals = rng.permutation(np.arange(1, 1 << 16))[:len(exits)]
        for (y, x), v in zip(exits, vals):
            board[y, x], goals[y, x] = v, 0
    return {"board": board, "goals": goals, "ax": ax, "ay": ay, "exits": exits}


def make_states(case):
    """The B states of a case, stacked the way SafeLifeVecEnv.set_state takes them, and
    the per-env exit lists for the oracle."""
    rng = np.random.RandomState(case.seed)
    B, (H, W) = case.B, case.shape
    sts = [make_state(rng, case.shape, case.view, STYLES[(case.seed + b) % len(STYLES)])
           for b in range(B)]
    ey = np.zeros((B, MAX_EXITS), np.int16)
    ex = np.zeros((B, MAX_EXITS), np.int16)
    for b, s in enumerate(sts):
        for k, (y, x) in enumerate(s["exits"]):
            ey[b, k], ex[b, k] = y, x
    return {"board": np.stack([s["board"] for s in sts]),
            "goals": np.stack([s["goals"] for s in sts]),
            "agent_x": np.array([s["ax"] for s in sts], np.int32),
            "agent_y": np.array([s["ay"] for s in sts], np.int32),
            "exit_count": np.array([len(s["exits"]) for s in sts], np.int32),
            "exit_y": ey, "exit_x": ex, "exits": [s["exits"] for s in sts]}


# ------------------------------------------------------------------------------ cases
class ObsCase:
    def __init__(self, name, shape, B, view, mode, channels, remove_white, offset, seed):
        self.name, self.shape, self.B, self.view = name, tuple(shape), B, tuple(view)
        self.mode, self.remove_white, self.offset, self.seed = mode, remove_white, offset, seed
        self.channels = None if mode == "packed" else tuple(channels)

    nv = property(lambda s: s.view[0] * s.view[1])
    esz = property(lambda s: ESZ[s.mode])
    nch = property(lambda s: len(s.channels) if s.channels else 1)
    # bytes per env, and the bytes between a 16-byte aligned address and the output
    env_bytes = property(lambda s: s.nv * s.nch * s.esz)
    out_shift = property(lambda s: s.esz if s.offset else 0)

    @property
    def kernel(self):
        """launch_obs's choice (sl_env.hip), restated for the cases' own bookkeeping."""
        if self.mode == "packed" and self.nv <= WAVE_MAX_CELLS:
            return "wave-packed"
        if self.out_shift % 16 == 0 and self.nv <= WAVE_MAX_CELLS:
            return "chunk"
        return "fallback"

    def env_parts(self, b):
        """Env b's output bytes [base, end) cut at the 16-byte boundaries, as
        obs_store_channels cuts them: (head bytes, whole chunks, tail bytes, whether the
        env's bytes contain a boundary strictly inside)."""
        base = self.out_shift + b * self.env_bytes
        end = base + self.env_bytes
        c0, c1 = (base + 15) // 16 * 16, end // 16 * 16
        head = min(c0, end) - base
        tail = end - c1 if c1 >= c0 else 0
        return head, max(0, (c1 - c0) // 16), tail, base < (base // 16 + 1) * 16 < end

    def __repr__(self):
        return self.name


BOARDS = [(2, 2), (5, 9), (25, 25), (33, 40), (64, 64), (9, 70), (128, 128)]
_SIDE = int(round(MAX_CELLS ** 0.5))
VIEWS = [
    # small and degenerate
    (1, 1), (1, 64), (64, 1), (2, 3), (8, 12), (9, 9), (33, 31),
    # wide
    (7, 64), (3, 65), (5, 130),
    # around the wave kernels' limit: 4 095, 4 096 (their last size), 4 160 cells
    (65, 63), (64, 64), (64, 65),
    # the largest obs_args accepts
    (_SIDE, MAX_CELLS // _SIDE),
]


def _curated():
    cases, n = [], 0

    def add(shape, view, mode, chans, offset):
        nonlocal n
        name = "%03d-%dx%d-v%dx%d-%s%s%s" % ((n,) + shape + view + (
            mode, "" if mode == "packed" else "-c" + "".join("%x" % c for c in chans),
            "-off" if offset else ""))
        cases.append(ObsCase(name, shape, 5 + n % 3, view, mode, chans, bool((n // 3) % 2),
                             offset, 7000 + n))
        n += 1

    # every view in every mode, aligned and offset; the boards and channel lists cycle,
    # so that each view meets all seven boards
    for vi, view in enumerate(VIEWS):
        for mi, mode in enumerate(MODES):
            for off in (False, True):
                k = vi + 2 * mi + off
                add(BOARDS[k % len(BOARDS)], view, mode, CHANNEL_LISTS[(k + vi) % len(CHANNEL_LISTS)],
                    off)
    # every channel list in every channel mode, aligned and offset
    for li, chans in enumerate(CHANNEL_LISTS):
        for mi, mode in enumerate(MODES[1:]):
            for off in (False, True):
                k = li + mi + off
                add(BOARDS[(2 * k + 1) % len(BOARDS)], ((33, 31), (8, 12), (7, 64))[k % 3], mode,
                    chans, off)
    # an env of less than 16 bytes, in every channel mode: 1 to 16 elements per env
    for mi, mode in enumerate(MODES[1:]):
        for vi, view in enumerate(((1, 1), (2, 3), (1, 2))):
            for li, chans in enumerate(((5, 5, 2), (0,), (15,), (3, 0, 9, 14))):
                add(BOARDS[(mi + vi + li) % len(BOARDS)], view, mode, chans, False)
    # 243 bytes per env: with those above, uint8 heads of every length from 0 to 15
    add((25, 25), (9, 9), "uint8", (5, 5, 2), False)
    return cases


CURATED = _curated()

SWEEP_SIDES = (1, 2, 3, 7, 8, 15, 16, 31, 33, 63, 64, 65, 100)
SWEEP_MAX_CELLS = 4200


def sweep_cases(n=200, seed=20261):
    """n random cases of B = 5 on boards of at most 40 x 40."""
    rng = np.random.RandomState(seed)
    cases = []
    for i in range(n):
        shape = (int(rng.randint(2, 41)), int(rng.randint(2, 41)))
        while True:
            view = (int(rng.choice(SWEEP_SIDES)), int(rng.choice(SWEEP_SIDES)))
            if view[0] * view[1] <= SWEEP_MAX_CELLS:
                break
        mode = MODES[rng.randint(len(MODES))]
        chans = tuple(int(c) for c in rng.randint(0, 16, size=rng.randint(1, 17)))
        off, rw = bool(rng.randint(2)), bool(rng.randint(2))
        cases.append(ObsCase("sweep%03d" % i, shape, 5, view, mode, chans, rw, off, 9000 + i))
    return cases


SWEEP = sweep_cases()


def expected(case, st):
    """oracle.make_obs of every env of a case: [B, vh, vw(, nch)] int64."""
    return np.stack([
        oracle.make_obs(st["board"][b], st["goals"][b], int(st["agent_x"][b]),
                        int(st["agent_y"][b]), st["exits"][b], case.view, case.channels,
                        case.remove_white).astype(np.int64) for b in range(case.B)])


# ------------------------------------------------- the reference-captured fixture's states
# (board shape, view, remove_white_goals, output_channels, exit style, exits kept: None =
# all the style gives).  tests/golden/make_golden.py (gen_obs) records what the reference
# returns for them.
FIXTURE_SPECS = [
    # views of more than twice the board
    ((2, 2), (9, 9), True, None, "full", 4),
    ((2, 2), (9, 9), False, tuple(range(15)), "none", None),
    ((3, 5), (1, 64), True, None, "half", None),
    ((3, 5), (1, 64), False, (15,), "full", None),
    # 1x1, 1xN, Nx1 and even views
    ((5, 9), (1, 1), True, None, "full", None),
    ((5, 9), (1, 1), False, (3, 0, 9, 14), "inside", 1),
    ((6, 8), (1, 12), True, None, "stack", None),
    ((6, 8), (12, 1), False, None, "corners", None),
    ((8, 8), (4, 4), True, None, "corners", None),
    ((8, 8), (2, 6), False, tuple(range(16)), "stack", None),
    ((10, 10), (8, 12), True, None, "half", None),
    ((16, 16), (6, 6), False, None, "full", None),
    # 0, 1 and 8 exits
    ((7, 12), (5, 5), True, None, "none", None),
    ((7, 12), (5, 5), False, None, "inside", 1),
    ((12, 7), (5, 7), True, None, "full", None),
    # two and three exits clipped onto one border cell
    ((16, 16), (5, 5), True, None, "stack", None),
    ((16, 16), (5, 5), False, None, "stack", None),
    ((12, 12), (3, 9), True, None, "stack", None),
    ((12, 12), (9, 3), False, (5, 5, 2), "stack", None),
    ((15, 11), (7, 5), True, None, "stack", None),
    ((11, 15), (4, 6), False, None, "stack", None),
    # an exit in each view corner
    ((16, 16), (9, 9), True, None, "corners", None),
    ((13, 16), (6, 5), False, None, "corners", None),
    ((16, 13), (15, 15), True, tuple(range(15)), "corners", None),
    # wrapped distance exactly H/2 and W/2 on even boards
    ((8, 8), (9, 9), True, None, "half", None),
    ((8, 8), (7, 7), False, None, "half", None),
    ((10, 6), (15, 15), True, None, "half", None),
    ((6, 10), (5, 5), False, tuple(range(15, -1, -1)), "half", None),
    ((16, 16), (16, 16), True, None, "half", None),
    ((16, 16), (17, 17), False, None, "half", None),
    # odd boards, views of the board's size and one past it
    ((9, 9), (9, 9), True, None, "full", None),
    ((9, 9), (10, 10), False, None, "inside", None),
    ((7, 7), (15, 15), True, None, "stack", None),
    ((5, 9), (33, 31), False, None, "full", None),
    ((15, 15), (15, 15), True, tuple(range(15)), "inside", None),
    ((15, 15), (15, 15), False, tuple(range(16)), "full", None),
    ((3, 3), (2, 2), True, None, "full", None),
    ((4, 3), (3, 4), False, (0,), "corners", None),
    # the two larger boards
    ((9, 70), (3, 65), True, None, "stack", None),
    ((33, 40), (15, 15), False, None, "corners", None),
]


def fixture_states(seed=4242):
    out = []
    for i, (shape, view, rw, chans, style, keep) in enumerate(FIXTURE_SPECS):
        s = make_state(np.random.RandomState(seed + i), shape, view, style)
        if keep is not None:
            s["exits"] = s["exits"][:keep]
        s.update(view=view, remove_white=rw, channels=chans, style=style)
        out.append(s)
    return out
