"""The premise of sl_env_state.agent_planes, from the oracle alone (CPU), and the host
function that declares it.

Premise: on the still-life pools the cell bits agent (1), preserving (5) and inhibiting
(6) are set in exactly one board cell, the agent's, after every step and every reset --
so the 64x64 plane kernels may build those three planes from the agent's position
instead of storing them.  Checked on the oracle's PPO chain (random rolls, random level
order, uniform random actions, a short time limit so episodes end by the limit and by
exits), for every env after every step, and on the frame a finished env leaves before
its reset.

Host function: vec_env.agent_planes on hand-built pools.
"""
import numpy as np
import pytest

import oracle
from agent_planes_util import (C3, C4, FOUNTAIN, PARASITE, PLAYER, hand_level, levels_of,
                               pool)

MASK = 0x0062


def _assert_agent_cell(board, ax, ay, ctx):
    ys, xs = np.nonzero(board & MASK)
    assert len(ys) == 1, (ctx, len(ys))
    assert (int(ys[0]), int(xs[0])) == (ay, ax), (ctx, ys[0], xs[0], ay, ax)
    assert board[ay, ax] & MASK == MASK, (ctx, hex(int(board[ay, ax])))


@pytest.mark.parametrize("path", [C3, C4], ids=["c3", "c4"])
def test_oracle_keeps_agent_bits_on_the_agent_cell(path):
    levels = levels_of(pool(path))
    B, T = 24, 2000
    cb = oracle.CpuBatch(levels, B, time_limit=25, view_shape=(15, 15), penalty_coef=1.0,
                         min_performance=0.01, seed=7, level_order="random",
                         augment_roll=True)
    cb.reset()
    for e in range(B):
        s = cb.scalars(e)
        _assert_agent_cell(cb.board(e), s["agent_x"], s["agent_y"], ("reset", e))
    rng = np.random.RandomState(3)
    episodes = 0
    for t in range(T):
        cb.step(rng.randint(0, 9, size=B).astype(np.int32))
        for e in range(B):
            s = cb.scalars(e)
            _assert_agent_cell(cb.board(e), s["agent_x"], s["agent_y"], (t, e))
        episodes = sum(cb.scalars(e)["episodes"] for e in range(B))
    assert episodes >= B * (T // 26)          # resets happened throughout


@pytest.mark.parametrize("path", [C3, C4], ids=["c3", "c4"])
def test_finished_env_keeps_agent_bits_before_its_reset(path):
    """The board an env holds when its episode ends (by the time limit or through an
    exit), before the reset: what a batch without auto-reset keeps stepping."""
    levels = levels_of(pool(path))
    rng = np.random.RandomState(5)
    ended = 0
    for e in range(4):
        o = oracle.OracleEnv(oracle.pool_level_fn(levels, e, seed=7, random_order=True,
                                                  augment=True),
                             env_id=e, rng="philox", seed=7, time_limit=20, view_shape=(15, 15),
                             output_channels=None, penalty_coef=1.0, min_performance=0.01)
        o.reset()
        for t in range(300):
            before = o.episodes
            ax, ay = o.agent_loc
            o.step(int(rng.randint(0, 9)))
            if o.episodes != before:          # the frame before the reset
                fb = o.last_frame[1]
                ys, xs = np.nonzero(fb & MASK)
                assert len(ys) == 1 and fb[ys[0], xs[0]] & MASK == MASK, (e, t)
                # (the agent moved at most one cell in its last step)
                d = min((ys[0] - ay) % 64, (ay - ys[0]) % 64) + \
                    min((xs[0] - ax) % 64, (ax - xs[0]) % 64)
                assert d <= 1, (e, t, d)
                ended += 1
            _assert_agent_cell(o.board, o.agent_loc[0], o.agent_loc[1], (e, t))
    assert ended >= 40


def _pool_of(levels):
    from safelife_amd import LevelPool
    return LevelPool.from_levels(levels)


def _mask(p, **kw):
    from safelife_amd.vec_env import agent_planes
    return agent_planes(p.board, p.agent_x, p.agent_y, **kw)


def test_host_mask_on_the_reference_pools():
    assert _mask(pool(C3)) == 0x62
    assert _mask(pool(C4)) == 0x62


def test_host_mask_on_hand_built_pools():
    plain = [hand_level(0, 0), hand_level(31, 63), hand_level(63, 63)]
    assert _mask(_pool_of(plain)) == 0x62
    # a fountain holds preserving, a parasite inhibiting: in one level of three is enough
    assert _mask(_pool_of(plain + [hand_level(5, 5, ((30, 30, FOUNTAIN),))])) == 0x42
    assert _mask(_pool_of(plain + [hand_level(5, 5, ((30, 30, PARASITE),))])) == 0x22
    assert _mask(_pool_of(plain + [hand_level(5, 5, ((30, 30, FOUNTAIN),
                                                      (33, 33, PARASITE)))])) == 0x02
    # two agent cells; the agent bit missing at agent_loc; the agent elsewhere
    assert _mask(_pool_of(plain + [hand_level(5, 5, ((30, 30, PLAYER),))])) == 0
    lv = hand_level(5, 5)
    lv["board"][5, 5] = PLAYER & ~0x02
    assert _mask(_pool_of(plain + [lv])) == 0x60
    lv = hand_level(5, 5)
    lv["agent_loc"] = (6, 5)
    assert _mask(_pool_of(plain + [lv])) == 0
    # an agent's cell that is not frozen could be changed by the rule
    lv = hand_level(5, 5)
    lv["board"][5, 5] = PLAYER & ~0x10
    assert _mask(_pool_of(plain + [lv])) == 0
    # toggled powers can set preserving and inhibiting anywhere (0x00E1)
    assert _mask(_pool_of(plain), can_toggle_powers=True) == 0x02
    assert _mask(pool(C3), can_toggle_powers=True) == 0x02
