"""The 64x64 plane step's action on four cells (csrc/sl_action4.h in sl_planes64_step.inc):
the wave gathers the agent's cell, the one in front, the one behind and the one two ahead
from the staged planes, takes their EXIT bits from the record's exit list, and decides the
action wave-uniformly -- no overlay, no search.

64 envs, time limit 40, 90 steps, against oracle twins of envs 0-39 step by step: reward,
done, flags, scalars, agent and orientation every step, board and goals every third.  The c3
pool runs k_env_planes64_s6 (asserted through sl_env_step_plan before and after), the c4 pool
the coloured five-wave instance.

The actions come from the oracle twins alone (drive): envs 8-63 play at random, envs 0-7
walk by a breadth-first search over the twin's empty cells toward the exit.  The pools put
the exit some 60 cells from the agent, out of reach within the time limit, so at steps 0 and
45 the walkers are set down three cells left of their exit through state_dict /
load_state_dict (the plan check still passes): even ones before two empty cells, odd ones
before a crate and an empty cell, which they push into the empty cell and then into the
exit.  The first time the exits are closed (min_performance 0.01: the walk into one is
refused); at step 30 the batch's min_performance drops to 0, every env resets at step 40, and
the second time the exits are open and entered.  The twins (envs 0-39) count what act_core's
branches did and where the agent stood: each case at least once, rows and columns 0, 1, 62
and 63 included, facing each way (the front, behind and two-ahead cells wrap in each
direction).  The seeds were chosen with the oracle alone (oracle_counts below runs the same
drive without a GPU).
"""
import ctypes
from collections import deque

import numpy as np
import pytest

import oracle
from agent_planes_util import C3, C4, SEED, levels_of, make_venv, pool, twins
import test_gpu_planes64_split as split

pytestmark = pytest.mark.gpu
B, T = 64, 90
WALKERS, TWINS = 8, 40
OPEN_AT, PLACE_AT = 30, (0, 45)
CRATE = 0x8014
EXIT, PUSHABLE, PULLABLE, DESTR = 0x0100, 0x0004, 0x8000, 0x0008
DIRS = ((-1, 0), (0, 1), (1, 0), (0, -1))          # MOVE UP, RIGHT, DOWN, LEFT: actions 1-4
CASES = ("move into empty", "open exit entered", "closed exit refused", "push into empty",
         "push into exit", "push blocked", "pull", "toggle create", "toggle destroy")
EDGES = (0, 1, 62, 63)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _first_move(board, start, goal):
    """First direction of a shortest path from start to goal over empty cells (the goal may
    hold anything), or None."""
    if start == goal:
        return None
    H, W = board.shape
    free = board == 0
    prev = {start: None}
    q = deque([start])
    while q:
        y, x = q.popleft()
        for d, (dy, dx) in enumerate(DIRS):
            n = ((y + dy) % H, (x + dx) % W)
            if n in prev or not (free[n] or n == goal):
                continue
            prev[n] = ((y, x), d)
            if n == goal:
                while prev[n][0] != start:
                    n = prev[n][0]
                return prev[n][1]
            q.append(n)
    return None


def _walker_action(o, rng):
    ax, ay = o.agent_loc
    # a crate on the right with the exit behind it or one further: push
    if o.board[ay, (ax + 1) % 64] & PUSHABLE and any(
            ey == ay and (ex - ax) % 64 in (2, 3) for ey, ex in o.exits):
        return 2
    for ey, ex in o.exits:
        m = _first_move(o.board, (ay, ax), (ey, ex))
        if m is not None:
            return 1 + m
    return int(rng.randint(0, 9))


def set_down(board, e):
    """Walker e three cells left of the (first) exit of `board`, edited in place: before two
    empty cells (e even) or a crate and an empty cell.  Returns the agent's (x, y)."""
    ys, xs = np.nonzero(board & EXIT)
    ey, ex = int(ys[0]), int(xs[0])
    ay, ax = (int(v[0]) for v in np.nonzero(board & 0x0002))
    agent = board[ay, ax]
    board[ay, ax] = 0
    board[ey, (ex - 1) % 64] = 0
    board[ey, (ex - 2) % 64] = CRATE if e & 1 else 0
    board[ey, (ex - 3) % 64] = agent
    return (ex - 3) % 64, ey


def _count(o, a, counts, edges):
    """What action a is about to do on twin o, read from its board (before the step)."""
    if o.game_over or a == 0:
        return
    b = o.board
    H, W = b.shape
    x0, y0 = o.agent_loc
    dy, dx = DIRS[(a - 1) & 3]
    c1 = int(b[(y0 + dy) % H, (x0 + dx) % W])
    c2 = int(b[(y0 - dy) % H, (x0 - dx) % W])
    c3 = int(b[(y0 + 2 * dy) % H, (x0 + 2 * dx) % W])
    if y0 in EDGES:
        edges.add(("row", y0, (a - 1) & 3))
    if x0 in EDGES:
        edges.add(("col", x0, (a - 1) & 3))
    if a <= 4:
        moved = False
        if c1 == 0:
            counts["move into empty"] += 1
            moved = True
        elif c1 & EXIT:
            counts["open exit entered" if o._can_exit() else "closed exit refused"] += 1
        elif c1 & PUSHABLE:
            if c3 == 0:
                counts["push into empty"] += 1
                moved = True
            elif c3 & EXIT:
                counts["push into exit"] += 1
                moved = True
            else:
                counts["push blocked"] += 1
        if moved and c2 & PULLABLE:
            counts["pull"] += 1
    elif c1 == 0:
        counts["toggle create"] += 1
    elif c1 & DESTR:
        counts["toggle destroy"] += 1


def _set_down_twins(oenvs):
    for e in range(WALKERS):
        oenvs[e].agent_loc = set_down(oenvs[e].board, e)
    return oenvs


def drive(oenvs, seed, step=None, switch=None, place=_set_down_twins):
    """T steps of the twins with the actions described above; step(oenvs, acts, t) takes the
    same step elsewhere and checks it against the twins (it steps them), switch() opens the
    exits there, place(oenvs) sets the walkers down there and returns the twins."""
    rng = np.random.RandomState(seed)
    counts, edges = dict.fromkeys(CASES, 0), set()
    for t in range(T):
        if t == OPEN_AT:
            for o in oenvs.values():
                o.wrapper_min_performance = 0.0
            if switch is not None:
                switch()
        if t in PLACE_AT:
            oenvs = place(oenvs)
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        for e in range(WALKERS):
            acts[e] = _walker_action(oenvs[e], rng)
        for e, o in oenvs.items():
            _count(o, int(acts[e]), counts, edges)
        if step is not None:
            step(oenvs, acts, t)
        else:
            for e, o in oenvs.items():
                o.step(int(acts[e]))
    return counts, edges


def check_counts(counts, edges):
    print(counts, len(edges))
    for k in CASES:
        assert counts[k] >= 1, (k, counts)
    # the agent acted in each edge row and column, facing each way
    for kind in ("row", "col"):
        for v in EDGES:
            assert {d for k, w, d in edges if (k, w) == (kind, v)} == {0, 1, 2, 3}, (kind, v)


def oracle_counts(path, seed):
    """The drive on freshly reset oracles alone (no GPU): how the seeds were chosen."""
    levels = levels_of(pool(path))
    oenvs = {}
    for e in range(TWINS):
        o = oracle.OracleEnv(oracle.pool_level_fn(levels, e, seed=SEED, n_total=B,
                                                  random_order=True, augment=True),
                             env_id=e, rng="philox", seed=SEED, time_limit=40,
                             view_shape=(33, 33), output_channels=None, penalty_coef=1.0,
                             min_performance=0.01)
        o.reset()
        oenvs[e] = o
    return drive(oenvs, seed)


def _plan(venv):
    from safelife_amd import _lib
    cfg = venv._fill_cfg()
    venv._fill_obs_cfg(cfg, None)
    out = _lib.StepPlan()
    rc = _lib.lib().sl_env_step_plan(ctypes.byref(venv._state),
                                     ctypes.byref(venv._pool_dev["struct"]), ctypes.byref(cfg),
                                     venv.flags.data_ptr(), ctypes.byref(out))
    assert rc == _lib.SL_OK
    return out


def _run(torch, dev, path, seed, kernel64):
    from safelife_amd import _lib
    p = pool(path)
    venv = make_venv(dev, p, B)
    venv.reset()

    def on_kernel():
        pl = _plan(venv)
        assert (pl.kernel64, pl.keep) == (kernel64, _lib.SL_PLAN_KEEP_C3), (pl.kernel64, pl.keep)
        assert (pl.stored, pl.derived) == (0x061D, 0x8100)

    def place(_):
        sd = venv.state_dict()
        board = sd["board"].cpu().numpy()
        for e in range(WALKERS):
            x, y = set_down(board[e], e)
            sd["agent_x"][e], sd["agent_y"][e] = x, y
        sd["board"] = torch.from_numpy(board).to(dev)
        venv.load_state_dict(sd)
        on_kernel()
        oenvs = twins(venv, p, list(range(TWINS)))
        for o in oenvs.values():        # (the batch's, where the exits have been opened)
            o.wrapper_min_performance = venv.min_performance
        return oenvs

    def step(oenvs, acts, t):
        venv.step_async(torch.from_numpy(acts).to(dev))
        split._vs_oracle(venv, oenvs, acts, t, t % 3 == 2 or t == T - 1)

    def switch():
        venv.min_performance = 0.0

    on_kernel()
    counts, edges = drive({}, seed, step, switch, place)
    on_kernel()
    check_counts(counts, edges)


def test_c3_six_wave_split_instance(torch_dev):
    from safelife_amd import _lib
    torch, dev = torch_dev
    _run(torch, dev, C3, 407, _lib.SL_PLAN_K64_S6)


def test_c4_coloured_five_wave_instance(torch_dev):
    from safelife_amd import _lib
    torch, dev = torch_dev
    _run(torch, dev, C4, 402, _lib.SL_PLAN_K64_PLANES)
