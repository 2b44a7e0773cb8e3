"""Env step against OracleEnv over the feature matrix of tests/feature_pools.py: odd and
non-square boards in every kernel family, 1 / 2 / 8 exits, toggles, bonus periods 0 / 1 /
4 / 16, remove_white_goals, even and over-wide views, can_exit sometimes false.

Every env, after every step: reward (== on float64), done, info flags, board, goals,
view, agent, orientation, old_points, side_effect and the exit list.  Philox cases draw
levels in random order with toroidal rolls (oracle.pool_level_fn); the two replay cases
share one stream with the oracle.  tests/test_feature_matrix_cpu.py checks on the CPU
that each case exercises its features with these very seeds and actions.

The three reference-captured feature fixtures (tests/golden/feat_*.npz) are replayed
through SafeLifeVecEnv as well, which ties the device path to the reference directly.
"""
import glob
import os

import numpy as np
import pytest

import oracle
import feature_pools as fp

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _views(torch, t):
    """Host array of a view tensor: packed uint16 as it is, channels as 0/1 (bf16 by bits)."""
    if t.dtype == torch.bfloat16:
        t = t.view(torch.uint16)
    a = t.cpu().numpy()
    return a if a.ndim == 3 else (a != 0).astype(np.uint16)


def _check_env(venv, st, board, goals, views, e, o, ctx):
    assert np.array_equal(board[e], o.board), ctx
    assert np.array_equal(goals[e], o.goals), ctx
    assert np.array_equal(views[e], o.obs()), ctx
    assert (int(st["agent_x"][e]), int(st["agent_y"][e])) == o.agent_loc, ctx
    assert int(st["orientation"][e]) == o.orientation, ctx
    assert int(st["old_points"][e]) == o.old_points, ctx
    assert int(st["side_effect"][e]) == o.last_side_effect, ctx
    n = int(st["exit_count"][e])
    assert n == len(o.exits), ctx
    got = list(zip(st["exit_y"][e][:n].tolist(), st["exit_x"][e][:n].tolist()))
    assert got == o.exits, (ctx, got, o.exits)


STATE_KEYS = ("agent_x", "agent_y", "orientation", "old_points", "side_effect", "exit_count",
              "exit_y", "exit_x")


@pytest.mark.parametrize("case", fp.CASES, ids=fp.CASE_IDS)
def test_env_step_vs_oracle(torch_dev, case):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool
    from safelife_amd.vec_env import zero_planes
    ds = case.level_dicts()
    pool, levels = LevelPool.from_levels(ds), fp.oracle_levels(ds)
    B = case.B
    if case.shape[1] <= 32:
        assert B % 4 != 0                  # the last wave of four envs keeps empty segments
    kw = case.env_kw()
    kw["obs_dtype"] = case.obs_dtype
    if case.rng == "stream":
        draws = np.random.RandomState(case.seed).random_sample(400000)
        venv = SafeLifeVecEnv(pool, B, dev, rng="stream", spawn_stream=draws, kernel=case.kernel,
                              board_mode=case.board_mode, **kw)
        oenvs = fp.oracle_envs(case, levels, stream=fp.SharedStream(draws))
    else:
        venv = SafeLifeVecEnv(pool, B, dev, rng="philox", seed=case.pseed, kernel=case.kernel,
                              board_mode=case.board_mode, level_order="random",
                              augment_roll=True, **kw)
        oenvs = fp.oracle_envs(case, levels)
    if case.planes and case.toggles:
        bits = int(np.bitwise_or.reduce(pool.board.reshape(-1)))
        assert venv._state.board_zero == zero_planes(bits, True, True), hex(venv._state.board_zero)

    def state():
        # (sync_board completes the uint16 boards without counting as a caller's read,
        # which would take board_mode="auto" out of plane mode for the next steps)
        venv.sync_board()
        st = {k: venv.st_t[k].cpu().numpy() for k in STATE_KEYS}
        return st, venv._board.cpu().numpy(), venv.goals.cpu().numpy()

    views = _views(torch, venv.reset())
    for o in oenvs:
        o.reset()
    st, board, goals = state()
    for e, o in enumerate(oenvs):
        _check_env(venv, st, board, goals, views, e, o, (case.name, "reset", e))
    acts, us = case.actions()
    n_plane = 0
    for t in range(case.T):
        a = np.array([fp.case_action(case, o, acts[t, e], us[t, e])
                      for e, o in enumerate(oenvs)], np.int32)
        vo, vr, vd, info = venv.step(torch.from_numpy(a).to(dev))
        views, vr, vd = _views(torch, vo), vr.cpu().numpy(), vd.cpu().numpy()
        flags = venv.flags.cpu().numpy()
        if case.planes is not None:
            # which 64x64 kernel ran: the plane kernel leaves bit 6 set on every env it
            # did not reset, the uint16-board kernel on none
            pok = venv.planes_ok.cpu().numpy()
            if case.planes:
                kept = (flags & 4) == 0
                assert ((pok[kept] & 64) != 0).all(), (case.name, t)
                n_plane += int(kept.sum())
            else:
                assert ((pok & 64) == 0).all(), (case.name, t)
        st, board, goals = state()
        for e, o in enumerate(oenvs):
            _, r, dn, oi = o.step(int(a[e]))
            ctx = (case.name, t, e)
            assert vr[e] == r, (ctx, vr[e], r)
            assert bool(vd[e]) == dn, ctx
            assert bool(flags[e] & 1) == bool(oi["times_up"]), ctx
            assert bool(flags[e] & 2) == bool(oi["game_over"]), ctx
            assert bool(flags[e] & 4) == bool(oi["times_up"] or oi["game_over"]), ctx
            _check_env(venv, st, board, goals, views, e, o, ctx)
    if case.planes:
        assert n_plane > case.T * B // 2
        assert venv._state.board_zero == zero_planes(
            int(np.bitwise_or.reduce(pool.board.reshape(-1))), case.toggles, case.toggles)
    if case.rng == "stream":
        assert not venv.stream_error()


# ------------------------------------------------- the reference's feature fixtures
def _feat_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "feat_*.npz")))


@pytest.mark.parametrize("kernel", ["fast", "generic"])
@pytest.mark.parametrize("path", _feat_files(), ids=lambda p: os.path.basename(p)[5:-4])
def test_env_feature_golden_trajectory(torch_dev, path, kernel):
    """The reference-captured feature trajectories (13x22 with toggles and period 1, 21x9
    with 8 exits and period 16, 10x10 with an 8x12 view) at B=1, reference-order spawn
    stream, through the small kernel (all three shapes fit it) and the per-cell kernel."""
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool
    d = np.load(path)
    penalty, min_perf, seed, vh, vw, time_limit = d["cfg"]
    powers, colors, period, remove_white = (int(v) for v in d["cfg_extra"])
    pool = LevelPool.from_levels([{
        "board": d["level_board"], "goals": d["level_goals"], "agent_loc": d["level_agent_loc"],
        "orientation": d["level_orientation"], "spawn_prob": d["level_spawn_prob"],
        "min_performance": d["level_min_performance"]}])
    stream = np.random.RandomState(int(seed)).random_sample(400000)
    env = SafeLifeVecEnv(pool, 1, dev, time_limit=int(time_limit), view_shape=(int(vh), int(vw)),
                         output_channels=None, penalty_coef=float(penalty),
                         min_performance=float(min_perf), rng="stream", spawn_stream=stream,
                         movement_bonus_period=period, remove_white_goals=bool(remove_white),
                         can_toggle_powers=bool(powers), can_toggle_colors=bool(colors),
                         kernel=kernel)
    obs = env.reset().cpu().numpy()
    assert np.array_equal(obs[0], d["obs0"])
    actions = torch.from_numpy(d["action"].astype(np.int32)).to(dev)
    for t in range(len(d["action"])):
        obs, r, done, info = env.step(actions[t:t + 1])
        ctx = (os.path.basename(path), kernel, t)
        assert r.item() == d["reward"][t], (ctx, r.item(), d["reward"][t])
        assert bool(done.item()) == bool(d["done"][t]), ctx
        assert bool(info["times_up"].item()) == bool(d["times_up"][t]), ctx
        assert bool(info["game_over"].item()) == bool(d["game_over"][t]), ctx
        st = env.state
        assert (st["agent_x"].item(), st["agent_y"].item()) == tuple(d["agent_loc"][t]), ctx
        assert st["orientation"].item() == d["orientation"][t], ctx
        assert st["old_points"].item() == d["points"][t], ctx
        assert st["side_effect"].item() == d["side_effect"][t], ctx
        assert np.array_equal(env.board[0].cpu().numpy(), d["board"][t]), ctx
        assert np.array_equal(env.goals[0].cpu().numpy(), d["goals"][t]), ctx
        assert np.array_equal(obs[0].cpu().numpy(), d["obs"][t]), ctx
    assert not env.stream_error()
