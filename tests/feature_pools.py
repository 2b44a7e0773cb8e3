"""Synthetic feature levels and pools of any board shape, for the tests of everything
around the rule: several exits, crates, toggles, bonus periods, odd and non-square
boards.  Plain data built from safelife_amd.cell_types by a seeded generator.

``build_level`` places, around an agent, the things each feature needs within reach:

* exits (1..8): optionally one right of the agent, optionally two side by side in one
  row, the rest on free cells (or on the rows given by ``exit_rows``);
* a pushable crate above the agent, a pullable one to its left, and more of both
  scattered; with ``seam`` the agent starts at x = 0, y = 1, so that the push
  and the pull carry those crates across the wrap seam of either axis;
* toggle targets below the agent (a coloured tree, a coloured hard spawner or a
  fountain) and scattered: cells that are neither empty nor destructible;
* walls, life of several colours, destructible spawners;
* goals: colour cells, white cells, and a live blinker so that the goals move.

``CASES`` is the matrix the CPU coverage test and the GPU tests share.
"""
import numpy as np

from safelife_amd.cell_types import CellTypes as CT

import oracle

MAX_EXITS = 8
COLORS = [int(CT.color_r), int(CT.color_g), int(CT.color_b),
          int(CT.color_r | CT.color_g), int(CT.color_g | CT.color_b), int(CT.rainbow_color)]


def _put(board, y, x, v, force=False):
    H, W = board.shape
    y, x = y % H, x % W
    if force or board[y, x] == 0:
        board[y, x] = v
        return True
    return False


def build_level(rng, H, W, n_exits=1, *, variant=0, seam=False, exit_rows=None,
                n_crates=4, n_walls=4, n_life=8, n_spawners=1, n_targets=3, n_goals=6,
                spawn_prob=0.3, min_performance=-1.0):
    """One level as a dict (the npz schema of a saved level).  ``variant`` (0..3) picks
    what stands next to the agent; ``seam`` puts the agent at x = 0, y = 1."""
    if not 1 <= n_exits <= MAX_EXITS:
        raise ValueError("n_exits must be in 1..%d" % MAX_EXITS)
    cells = H * W
    board = np.zeros((H, W), np.uint16)
    goals = np.zeros((H, W), np.uint16)
    ax, ay = (0, 1 % H) if seam else (int(rng.randint(W)), int(rng.randint(H)))
    board[ay, ax] = CT.player | (CT.color_b if variant & 1 else 0)
    exits = 0
    # an exit right of the agent (variants 0, 2); two exits side by side (variants 0, 1)
    if variant in (0, 2) and exits < n_exits and cells > 4:
        exits += _put(board, ay, ax + 1, CT.level_exit)
    if cells >= 20:
        _put(board, ay - 1, ax, CT.frozen | CT.pushable)                 # push it up
        _put(board, ay, ax - 1, CT.frozen | CT.pullable)                 # pull it right
        below = (CT.tree | CT.color_g, CT.hard_spawner | CT.color_b,
                 CT.fountain | CT.color_r, CT.crate)[variant]
        _put(board, ay + 1, ax, below)
    free = [(int(y), int(x)) for y, x in zip(*np.nonzero(board == 0))]
    rng.shuffle(free)

    def take(row=None):
        for i, (y, x) in enumerate(free):
            if board[y, x] == 0 and (row is None or y == row):
                free.pop(i)
                return y, x
        return None

    if variant in (0, 1) and n_exits - exits >= 2 and W >= 4:
        far = lambda x: min((x - ax) % W, (ax - x) % W) >= W // 3     # out of most views
        for y, x in [p for p in free if far(p[1])] + list(free):
            if board[y, x] == 0 and board[y, (x + 1) % W] == 0:
                board[y, x] = board[y, (x + 1) % W] = CT.level_exit
                exits += 2
                break
    rows = list(exit_rows) if exit_rows is not None else []
    while exits < n_exits:
        p = take(rows.pop(0) % H if rows else None)
        if p is None:
            break
        board[p] = CT.level_exit
        exits += 1
    kinds = [(n_crates, lambda i: CT.frozen | (CT.pushable, CT.pullable, CT.movable)[i % 3]),
             (n_walls, lambda i: CT.wall | (COLORS[i % 6] if i % 2 else 0)),
             (n_targets, lambda i: (CT.tree | COLORS[i % 5], CT.hard_spawner | COLORS[(i + 2) % 5],
                                    CT.fountain, CT.ice_cube)[i % 4]),
             (n_spawners, lambda i: CT.spawner | COLORS[(i + 1) % 5]),
             (n_life, lambda i: CT.life | COLORS[1 + i % 4] * (i % 4 != 3) if variant >= 2
              else CT.life | COLORS[i % 5] * (i % 4 != 3))]
    for n, val in kinds:
        for i in range(n):
            p = take()
            if p is not None and len(free) > cells // 3:
                board[p] = val(i)
    # (variants 2 and 3 have no goals and no red life: nothing to complete, so can_exit holds
    # under any min_performance until something red is born)
    if variant >= 2:
        n_goals = 0
    for i in range(n_goals):
        y, x = int(rng.randint(H)), int(rng.randint(W))
        goals[y, x] = COLORS[i % 6]
    if H >= 5 and W >= 5 and variant < 2:       # a live blinker: the goals advance too
        y, x = int(rng.randint(H)), int(rng.randint(W))
        for d in (-1, 0, 1):
            goals[y, (x + d) % W] = CT.life | CT.color_g
    return {"board": board, "goals": goals, "agent_loc": np.array([ax, ay]),
            "orientation": int(rng.randint(4)), "spawn_prob": float(spawn_prob),
            "min_performance": float(min_performance)}


def build_levels(seed, K, H, W, n_exits, **kw):
    """K level dicts; level k has variant k % 4 and, for odd k // 4 or k == 1, the agent on
    the seam.  ``n_exits`` is one count or a sequence cycled over the levels."""
    rng = np.random.RandomState(seed)
    ne = [n_exits] if np.isscalar(n_exits) else list(n_exits)
    scale = max(1, (H * W) // 120)
    dens = dict(n_crates=3 * scale, n_walls=2 * scale, n_life=5 * scale,
                n_spawners=max(1, scale // 2), n_targets=2 * scale, n_goals=4 * scale)
    if H * W < 20:
        dens = dict(n_crates=0, n_walls=0, n_life=1, n_spawners=0, n_targets=0, n_goals=1)
    dens.update(kw)
    return [build_level(rng, H, W, min(ne[k % len(ne)], max(1, H * W // 3)), variant=k % 4,
                        seam=(k % 4 == 1 or (k // 4) % 2 == 1), **dens) for k in range(K)]


def feature_pool(seed, K, H, W, n_exits, **kw):
    """A safelife_amd.LevelPool of K feature levels, and the same levels for the oracle."""
    from safelife_amd import LevelPool
    ds = build_levels(seed, K, H, W, n_exits, **kw)
    return LevelPool.from_levels(ds), oracle_levels(ds)


def oracle_levels(ds):
    return [oracle.Level(d["board"], d["goals"], d["agent_loc"], d["orientation"],
                         d["spawn_prob"], d["min_performance"]) for d in ds]


# --------------------------------------------------------------------------- the matrix
class Case:
    """One case of the matrix: a board shape, the kernel that must run it and the
    settings around the rule."""

    def __init__(self, name, shape, family, kernel="auto", n_exits=1, toggles=False, period=4,
                 remove_white=True, view=(9, 9), penalty=0.7, min_perf=-1.0, B=26, T=60,
                 board_mode="auto", channels=None, obs_dtype="uint16", rng="philox",
                 exit_rows=None, K=8, seed=0, planes=None, time_limit=20, pseed=None):
        self.name, self.shape, self.family, self.kernel = name, shape, family, kernel
        self.n_exits, self.toggles, self.period = n_exits, toggles, period
        self.remove_white, self.view, self.penalty, self.min_perf = remove_white, view, penalty, min_perf
        self.B, self.T, self.board_mode, self.channels = B, T, board_mode, channels
        self.obs_dtype, self.rng, self.exit_rows, self.K = obs_dtype, rng, exit_rows, K
        self.seed = seed
        self.planes = planes            # 64x64: must planes_ok bit 6 be set (True) / clear (False)
        self.time_limit = time_limit
        # the Philox seed (levels' order, rolls, spawns): chosen on the CPU so that the
        # case meets its coverage conditions (tests/test_feature_matrix_cpu.py)
        self.pseed = seed + 5 if pseed is None else pseed

    @property
    def multi_exit(self):
        return self.n_exits > 1

    def level_dicts(self):
        H, W = self.shape
        kw = {}
        if self.exit_rows is not None:
            kw["exit_rows"] = self.exit_rows
        # levels with the wrapper's min_performance in force only (min_perf >= 0 cases:
        # can_exit is then sometimes false at an exit)
        return build_levels(1000 + self.seed, self.K, H, W, self.n_exits, **kw)

    def env_kw(self):
        """Settings shared by SafeLifeVecEnv and OracleEnv."""
        return dict(time_limit=self.time_limit, view_shape=self.view,
                    output_channels=self.channels, remove_white_goals=self.remove_white,
                    movement_bonus_period=self.period, penalty_coef=self.penalty,
                    min_performance=self.min_perf, can_toggle_powers=self.toggles,
                    can_toggle_colors=self.toggles)

    def actions(self):
        """[T, B] actions: uniform over the nine, with a seek share decided per step."""
        rng = np.random.RandomState(77 + self.seed)
        return rng.randint(0, 9, size=(self.T, self.B)).astype(np.int32), \
            rng.random_sample((self.T, self.B))

    SEEK = 0.3


def seek_action(env, u):
    """A move towards env's first exit (as the goldens' seek policy), or None."""
    if not env.exits:
        return None
    H, W = env.board.shape
    x0, y0 = env.agent_loc
    ey, ex = env.exits[0]
    dy = (ey - y0 + H // 2) % H - H // 2
    dx = (ex - x0 + W // 2) % W - W // 2
    opts = ([1] if dy < 0 else []) + ([3] if dy > 0 else []) + ([2] if dx > 0 else []) + \
        ([4] if dx < 0 else [])
    if not opts:
        return None
    return opts[int(u * 7919) % len(opts)]


G, S4, S1, U64, P64, B128 = "generic", "small-seg4", "small", "bits64-uint16", "bits64-planes", "bits128"

CASES = [
    # generic only: kernel="generic", and AUTO above the small kernel's 32 x 64
    Case("g-2x2", (2, 2), G, "generic", n_exits=1, period=0, view=(9, 9), B=26, K=4),
    Case("g-5x9", (5, 9), G, "generic", n_exits=2, toggles=True, period=1, view=(15, 15),
         remove_white=False, penalty=0.0, min_perf=0.5, seed=1),
    Case("g-33x40", (33, 40), G, "auto", n_exits=8, period=16, view=(33, 33), min_perf=0.01,
         B=25, seed=2),
    Case("g-9x70", (9, 70), G, "auto", n_exits=2, toggles=True, period=4, view=(8, 12),
         penalty=0.0, B=27, seed=3),
    # small kernel, four envs per wave (W <= 32)
    Case("s4-7x29", (7, 29), S4, "fast", n_exits=8, toggles=True, period=1, view=(9, 9),
         remove_white=False, B=26, seed=4),
    Case("s4-20x28", (20, 28), S4, "fast", n_exits=2, period=16, view=(8, 12), penalty=0.0,
         min_perf=0.5, B=30, seed=5),
    Case("s4-32x32", (32, 32), S4, "fast", n_exits=1, toggles=True, period=0, view=(33, 33),
         min_perf=0.01, B=34, seed=6),
    Case("s4-7x29-stream", (7, 29), S4, "fast", n_exits=3, period=4, view=(9, 9), B=26,
         rng="stream", seed=7),
    # small kernel, one env per wave (32 < W <= 64)
    Case("s1-17x40", (17, 40), S1, "fast", n_exits=8, period=0, view=(8, 12),
         remove_white=False, min_perf=0.01, B=25, seed=8),
    Case("s1-32x63", (32, 63), S1, "fast", n_exits=2, toggles=True, period=16, view=(33, 33),
         penalty=0.0, B=26, seed=9),
    Case("s1-17x40-p1", (17, 40), S1, "fast", n_exits=1, period=1, view=(9, 9), min_perf=0.5,
         B=27, seed=10),
    Case("s1-17x40-stream", (17, 40), S1, "fast", n_exits=3, period=4, view=(9, 9), B=25,
         rng="stream", seed=11),
    # 64x64, the uint16-board kernel
    Case("u64-packed", (64, 64), U64, "fast", n_exits=8, toggles=True, period=1, view=(33, 33),
         board_mode="uint16", planes=False, B=24, seed=12, pseed=217),
    Case("u64-chan-u8", (64, 64), U64, "fast", n_exits=2, period=0, view=(8, 12),
         remove_white=False, board_mode="uint16", channels=tuple(range(15)), obs_dtype="uint8",
         penalty=0.0, min_perf=0.5, planes=False, B=24, seed=13),
    Case("u64-chan-bf16", (64, 64), U64, "fast", n_exits=1, period=16, view=(9, 9),
         board_mode="uint16", channels=(0, 3, 8, 9, 12, 14), obs_dtype="bfloat16",
         min_perf=0.01, planes=False, B=24, seed=14, pseed=119),
    Case("u64-p4", (64, 64), U64, "fast", n_exits=2, period=4, view=(9, 9), board_mode="uint16",
         planes=False, B=24, seed=15),
    # 64x64, the plane kernel (default board mode, Philox, no capture)
    Case("p64-toggles", (64, 64), P64, "auto", n_exits=8, toggles=True, period=4, view=(33, 33),
         min_perf=0.01, planes=True, B=24, seed=12),
    Case("p64-chan", (64, 64), P64, "auto", n_exits=2, period=1, view=(8, 12),
         remove_white=False, channels=tuple(range(15)), obs_dtype="uint8", penalty=0.0,
         planes=True, B=24, seed=13),
    Case("p64-p0", (64, 64), P64, "auto", n_exits=1, period=0, view=(9, 9), min_perf=0.5,
         planes=True, B=24, seed=14, pseed=619),
    Case("p64-p16", (64, 64), P64, "auto", n_exits=2, period=16, view=(9, 9), planes=True, B=24,
         seed=15),
    # 128x128: exits in different 32-row bands and on the band-edge rows 31 / 32
    Case("b128-8", (128, 128), B128, "fast", n_exits=8, toggles=True, period=1, view=(33, 33),
         remove_white=False, min_perf=0.01, B=12, T=40, K=4, time_limit=13, seed=16,
         exit_rows=(31, 32, 63, 64, 95, 96, 127, 0), pseed=2721),
    Case("b128-2", (128, 128), B128, "fast", n_exits=2, period=0, view=(8, 12), penalty=0.0,
         min_perf=0.5, B=12, T=40, K=4, time_limit=13, seed=17, exit_rows=(31, 32), pseed=122),
    Case("b128-1", (128, 128), B128, "auto", n_exits=1, period=16, view=(9, 9), B=12, T=40, K=4, time_limit=13,
         seed=18, exit_rows=(96,), pseed=123),
    Case("b128-p4", (128, 128), B128, "auto", n_exits=2, period=4, view=(9, 9), B=12, T=40, K=4, time_limit=13,
         seed=19, exit_rows=(32, 95), pseed=1224),
]
CASE_IDS = [c.name for c in CASES]


class TracingOracleEnv(oracle.OracleEnv):
    """OracleEnv that counts what a case is there to exercise (it changes nothing)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.n = dict(push_seam=0, pull_seam=0, toggle_power=0, toggle_color=0, exit_resets=0,
                      resets=0, clipped_same=0, exit_in_view=0, can_exit_false=0)

    def _move_agent(self, dy, dx=0):
        b = self.board
        H, W = b.shape
        x0, y0 = self.agent_loc
        x1, y1 = self._relative_loc(dy, dx)
        x2, y2 = self._relative_loc(-dy, -dx)
        x3, y3 = self._relative_loc(dy * 2)
        ahead, behind, far = int(b[y1, x1]), int(b[y2, x2]), int(b[y3, x3])
        if (ahead & oracle.EXIT) and not self._can_exit():
            self.n["can_exit_false"] += 1
        r = super()._move_agent(dy, dx)
        moved = self.agent_loc == (x1, y1) and (x0, y0) != (x1, y1)

        def seam(pa, pb):
            return abs(pa[0] - pb[0]) > 1 or abs(pa[1] - pb[1]) > 1
        if moved and ahead and (ahead & oracle.PUSHABLE) and far == 0 and seam((x1, y1), (x3, y3)) \
                and min(H, W) > 2:
            self.n["push_seam"] += 1
        if moved and (behind & oracle.PULLABLE) and seam((x2, y2), (x0, y0)) and min(H, W) > 2:
            self.n["pull_seam"] += 1
        return r

    def _execute_action(self, name):
        x0, y0 = self.agent_loc
        before = int(self.board[y0, x0])
        r = super()._execute_action(name)
        if name.startswith("TOGGLE"):
            diff = before ^ int(self.board[y0, x0])
            self.n["toggle_power"] += bool(diff & (oracle.ALIVE | oracle.INHIBITING |
                                                   oracle.PRESERVING | oracle.SPAWNING))
            self.n["toggle_color"] += bool(diff & oracle.RAINBOW)
        return r

    def obs(self):
        h, w = self.view_shape
        bh, bw = self.board.shape
        x0, y0 = self.agent_loc
        seen = {}
        for iy, ix in self.exits:
            jy = (iy - y0 + bh // 2) % bh - bh // 2 + h // 2
            jx = (ix - x0 + bw // 2) % bw - bw // 2 + w // 2
            inside = 0 <= jy < h and 0 <= jx < w
            self.n["exit_in_view"] += inside
            cell = (min(max(jy, 0), h - 1), min(max(jx, 0), w - 1))
            self.n["clipped_same"] += cell in seen      # (two exits inside never share one)
            seen[cell] = inside
        return super().obs()

    def reset(self):
        if self.episodes:
            self.n["resets"] += 1
            self.n["exit_resets"] += bool(self.game_over)
        return super().reset()


def oracle_envs(case, levels, cls=oracle.OracleEnv, stream=None):
    """The oracle's envs of a case, as the device pool hands out levels (Philox cases:
    random order, rolled; replay cases: pool order, one shared stream)."""
    kw = case.env_kw()
    if case.channels is None:
        kw["output_channels"] = None
    if case.rng == "stream":
        return [cls(lambda ep, e=e: levels[(e + ep * case.B) % len(levels)], env_id=e,
                    rng="stream", stream=stream, **kw) for e in range(case.B)]
    return [cls(oracle.pool_level_fn(levels, e, seed=case.pseed, n_total=case.B,
                                     random_order=True, augment=True),
                env_id=e, rng="philox", seed=case.pseed, **kw) for e in range(case.B)]


def case_action(case, env, a, u):
    """The action env takes: the drawn one, or with share SEEK a move towards its exit."""
    if u < case.SEEK:
        s = seek_action(env, u / case.SEEK)
        if s is not None:
            return s
    return int(a)


class SharedStream:
    """One uniform stream consumed env after env, board then goals (replay order)."""

    def __init__(self, s):
        self.s, self.pos = s, 0

    def take(self, n):
        out = self.s[self.pos:self.pos + n]
        self.pos += n
        return out
