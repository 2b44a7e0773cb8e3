"""sl_env_state.goals_gray only ever narrows: a pool with coloured goals (set_pool,
PoolFeeder.swap) and goals written from outside the kernels (write_goals, a game's goals
setter, set_state) clear it, after which the batch steps like the oracle again -- with a
green goal under a live green cell, which scores +5 where a black or white one scores 0;
a state_dict round trip keeps the flag only where both sides have it."""
import numpy as np
import pytest

from agent_planes_util import C3, C4, check_step, make_venv, pool, twins

import oracle

pytestmark = pytest.mark.gpu
B = 64
SAMPLE = [0, 1, 31, 63]
GREEN_LIFE, GREEN = 0x0401, 0x0400      # alive + green of the cell bits 0, 9-11


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _steps(torch, dev, venv, rng, n, oenvs=None, ctx=None):
    n_done = 0
    for t in range(n):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step_async(torch.from_numpy(acts).to(dev))
        if oenvs is not None:
            n_done += check_step(venv, oenvs, acts, (ctx, t))
    return n_done


@pytest.mark.parametrize("how", ["set_pool", "feeder"])
def test_pool_with_coloured_goals_narrows_the_flag(torch_dev, how):
    torch, dev = torch_dev
    from safelife_amd.pool_feed import PoolFeeder, npz_level_source
    c3, c4 = pool(C3), pool(C4)
    venv = make_venv(dev, c3, B)
    venv.reset()
    rng = np.random.RandomState(41)
    _steps(torch, dev, venv, rng, 20)
    assert venv._state.goals_gray == 1
    assert int(((venv.planes_ok & 64) != 0).sum().item()) > B // 2
    if how == "set_pool":
        venv.set_pool(c4)
    else:
        feeder = PoolFeeder(npz_level_source(C4, repeat=False), pool_size=c4.K, device=dev)
        try:
            assert feeder.swap(venv, block=True, timeout=60)
        finally:
            feeder.close()
    assert venv._state.goals_gray == 0
    oenvs = twins(venv, c4, SAMPLE)
    before = {e: o.episodes for e, o in oenvs.items()}
    n_done = 0
    for t in range(60):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step_async(torch.from_numpy(acts).to(dev))
        n_done += check_step(venv, oenvs, acts, (how, t))
        assert venv._state.goals_gray == 0
    assert n_done >= len(SAMPLE)
    assert all(o.episodes > before[e] for e, o in oenvs.items())   # resets drew c4 levels
    # a gray pool again does not bring the flag back: running envs keep their goals
    venv.set_pool(c3)
    assert venv._state.goals_gray == 0


def _green_cell(venv):
    """(env, y, x) of a live green cell that outlives a step, away from the env's agent."""
    boards = venv.board.cpu().numpy()
    ax, ay = venv.st_t["agent_x"].cpu().numpy(), venv.st_t["agent_y"].cpu().numpy()
    for e in range(B):
        nxt = oracle.advance(boards[e], 0.0)[0]
        ys, xs = np.nonzero(((boards[e] & 0x0E01) == GREEN_LIFE) & ((nxt & 0x0E01) == GREEN_LIFE))
        far = (np.abs(ys - ay[e]) > 3) & (np.abs(xs - ax[e]) > 3)
        if far.any():
            return e, int(ys[far][0]), int(xs[far][0])
    raise AssertionError("no env with a live green cell")


@pytest.mark.parametrize("how", ["write_goals", "game_setter", "set_state"])
def test_outside_goal_write_clears_the_flag(torch_dev, how):
    torch, dev = torch_dev
    from safelife_amd.env import SafeLifeGame
    p = pool(C3)
    venv = make_venv(dev, p, B)
    venv.reset()
    rng = np.random.RandomState(42)
    _steps(torch, dev, venv, rng, 3)
    assert venv._state.goals_gray == 1
    assert int(((venv.planes_ok & 64) != 0).sum().item()) > B // 2
    e, y, x = _green_cell(venv)
    goals = venv.goals.cpu().numpy().copy()
    assert (goals[e, y, x] >> 9) & 7 in (0, 7)
    # (its other bits stay: a live goal cell killed here would be born again, black)
    goals[e, y, x] = (int(goals[e, y, x]) & 0xF1FF) | GREEN
    if how == "write_goals":
        venv.write_goals(e, goals[e])
    elif how == "game_setter":
        SafeLifeGame(venv, e).goals = goals[e]
    else:
        sc = {k: t.cpu().numpy() for k, t in venv.st_t.items()}
        venv.set_state(venv.board.cpu().numpy(), goals, venv.start_board.cpu().numpy(), **sc)
    assert venv._state.goals_gray == 0
    oenvs = twins(venv, p, sorted({0, e, B - 1}))
    acts = np.zeros(B, np.int32)              # nobody acts: the green cell stays
    venv.step_async(torch.from_numpy(acts).to(dev))
    check_step(venv, oenvs, acts, how)
    o = oenvs[e]
    assert o.board[y, x] & 0x0E01 == GREEN_LIFE
    blank = o.goals.copy()
    assert (o.goals[y, x] >> 9) & 7 == 2      # still green
    blank[y, x] &= 0xF1FF
    assert oracle.points(o.board, o.goals) - oracle.points(o.board, blank) == 5
    assert int(venv.st_t["old_points"][e].item()) == oracle.points(o.board, o.goals)
    _steps(torch, dev, venv, rng, 30, oenvs, how)
    assert venv._state.goals_gray == 0


def test_state_dict_round_trip_keeps_the_flag_where_both_have_it(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    a = make_venv(dev, p, B)
    a.reset()
    rng = np.random.RandomState(43)
    _steps(torch, dev, a, rng, 10)
    sd = a.state_dict()
    assert int(sd["goals_gray"]) == 1
    _steps(torch, dev, a, rng, 5)
    a.load_state_dict(sd)
    assert a._state.goals_gray == 1
    oenvs = twins(a, p, SAMPLE)
    assert _steps(torch, dev, a, rng, 50, oenvs, "restored") >= len(SAMPLE)
    # a snapshot of goals not known to be gray; a dict from before the field
    sd0 = dict(sd, goals_gray=torch.tensor(0, dtype=torch.int32))
    a.load_state_dict(sd0)
    assert a._state.goals_gray == 0
    b = make_venv(dev, p, B)
    b.reset()
    del sd0["goals_gray"]
    b.load_state_dict(sd0)
    assert b._state.goals_gray == 0
    # a batch that lost the flag does not get it back from a snapshot that has it
    a.load_state_dict(sd)
    assert a._state.goals_gray == 0
