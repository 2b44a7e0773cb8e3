"""Shared by the agent-plane tests (sl_env_state.agent_planes: the 64x64 plane kernels
build cell bits 1, 5 and 6 from the agent's position instead of storing their planes):
pools, hand-built levels, and the oracle twins of a few envs of a batch."""
import os

import numpy as np

import oracle

POOLS = os.path.join(os.path.dirname(__file__), "golden", "pools")
C3 = os.path.join(POOLS, "c3_prune_still_64.npz")
C4 = os.path.join(POOLS, "c4_append_still_64.npz")

PLAYER, WALL, CRATE, EXIT, LIFE = 0x7A, 0x10, 0x14, 0x110, 0x09
FOUNTAIN, PARASITE = 0x30, 0x55
SEED = 23


def pool(path):
    from safelife_amd import LevelPool
    return LevelPool.load(path)


def with_cell(p, value):
    """Pool p with one free cell of each level, away from the agent, set to `value`."""
    from safelife_amd import LevelPool
    b = p.board.copy()
    for k in range(p.K):
        free = b[k] == 0
        ay, ax = int(p.agent_y[k]), int(p.agent_x[k])
        free[max(ay - 4, 0):ay + 5, max(ax - 4, 0):ax + 5] = False
        ys, xs = np.nonzero(free)
        b[k, ys[len(ys) // 2], xs[len(xs) // 2]] = value
    return LevelPool(b, p.goals, np.stack([p.agent_x, p.agent_y], 1), p.orientation,
                     p.spawn_prob, p.min_performance)


def hand_level(ay, ax, extra=()):
    """An open 64x64 level: the agent at (ay, ax), a few live cells far from every path
    the tests walk, a red goal patch and an exit; `extra`: ((y, x, value), ...)."""
    board = np.zeros((64, 64), np.uint16)
    goals = np.zeros((64, 64), np.uint16)
    for y, x in ((20, 20), (20, 21), (21, 20), (21, 21), (40, 10), (40, 11), (40, 12)):
        board[y, x] = LIFE | 0x400            # a block and a blinker, green
    goals[10:12, 40:42] = 0x200
    board[50, 50] = EXIT
    for y, x, v in extra:
        board[y % 64, x % 64] = v
    board[ay, ax] = PLAYER
    return {"board": board, "goals": goals, "agent_loc": (ax, ay), "orientation": 1,
            "spawn_prob": 0.0, "min_performance": 0.5}


def levels_of(p):
    return [oracle.Level(p.board[k], p.goals[k], (p.agent_x[k], p.agent_y[k]),
                         p.orientation[k], p.spawn_prob[k], p.min_performance[k])
            for k in range(p.K)]


def env_state(venv, e):
    s = {"board": venv.board[e].cpu().numpy(), "goals": venv.goals[e].cpu().numpy(),
         "start_board": venv.start_board[e].cpu().numpy()}
    for k, t in venv.st_t.items():
        s[k] = t[e].cpu().numpy()
    return s


def make_venv(dev, p, B, *, time_limit=40, view=(33, 33), channels=None, dtype="uint16",
              compute_obs=False, board_mode="planes", random_order=True, augment=True, **kw):
    from safelife_amd import SafeLifeVecEnv
    return SafeLifeVecEnv(p, B, dev, board_mode=board_mode, rng="philox", seed=SEED,
                          kernel="fast", compute_obs=compute_obs,
                          level_order="random" if random_order else "sequential",
                          augment_roll=augment, obs_dtype=dtype, time_limit=time_limit,
                          view_shape=view, output_channels=channels, penalty_coef=1.0,
                          min_performance=0.01, **kw)


def twins(venv, p, sample, *, time_limit=40, view=(33, 33), channels=None, random_order=True,
          augment=True, **kw):
    """OracleEnvs continuing envs `sample` of venv from its current state."""
    levels = levels_of(p)
    out = {}
    for e in sample:
        o = oracle.OracleEnv(oracle.pool_level_fn(levels, e, seed=SEED, n_total=venv.B,
                                                  random_order=random_order, augment=augment),
                             env_id=e, rng="philox", seed=SEED, time_limit=time_limit,
                             view_shape=view, output_channels=channels, penalty_coef=1.0,
                             min_performance=0.01, **kw)
        o.load_state(env_state(venv, e), venv._step_index)
        out[e] = o
    return out


def check_step(venv, oenvs, acts, ctx, obs=None):
    """The step `acts` just taken by venv, taken by the oracle twins: reward, done, flags,
    the scalars and the completed board and goals, bit for bit (and the views `obs`).
    Returns the number of twins that finished."""
    vr, vd, vf = (t.cpu().numpy() for t in (venv.reward, venv.done, venv.flags))
    board, goals = venv.board.cpu().numpy(), venv.goals.cpu().numpy()
    st = {k: venv.st_t[k].cpu().numpy() for k in
          ("agent_x", "agent_y", "orientation", "old_points", "side_effect", "baseline",
           "episode_length")}
    n_done = 0
    for e, o in oenvs.items():
        ob, r, dn, info = o.step(int(acts[e]))
        c = (ctx, e)
        assert vr[e] == r, (c, vr[e], r)
        assert bool(vd[e]) == dn, c
        assert bool(vf[e] & 1) == bool(info["times_up"]), c
        assert bool(vf[e] & 2) == bool(info["game_over"]), c
        assert np.array_equal(board[e], o.board), c
        assert np.array_equal(goals[e], o.goals), c
        assert (st["agent_x"][e], st["agent_y"][e]) == o.agent_loc, c
        assert st["orientation"][e] == o.orientation, c
        assert st["old_points"][e] == o.old_points, c
        assert st["side_effect"][e] == o.last_side_effect, c
        assert st["baseline"][e] == o.baseline, c
        assert st["episode_length"][e] == o.episode_length, c
        if obs is not None:
            assert np.array_equal(obs[e], ob), c
        n_done += int(dn or (vf[e] & 4) != 0)
    return n_done
