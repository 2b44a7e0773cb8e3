"""Pin the CPU oracle (oracle/) against golden vectors captured from the reference.

CPU-only.  These tests are what makes the oracle trustworthy as the checker of
the HIP path (tests/test_gpu_*.py).
"""
import glob
import os

import numpy as np
import pytest

import oracle

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def test_g1_advance_known_answers():
    d = np.load(os.path.join(GOLDEN, "advance_known_answers.npz"))
    off = 0
    for (H, W), p in zip(d["shapes"], d["spawn_prob"]):
        n = H * W
        bi = d["boards_in"][off:off + n].reshape(H, W)
        bo = d["boards_out"][off:off + n].reshape(H, W)
        off += n
        out, _ = oracle.advance(bi, p)
        assert np.array_equal(out, bo), (H, W, p)


def test_g2_reference_stream():
    d = np.load(os.path.join(GOLDEN, "advance_stream.npz"))
    keys = sorted({k.rsplit("_", 1)[0] for k in d.files if k.endswith("_board0")})
    assert len(keys) >= 12
    for key in keys:
        s = int(key.split("_")[0][1:])
        rng = oracle.RefStreamRNG()
        rng.seed(s)
        b, g = d[key + "_board0"], d[key + "_goals0"]
        for t in range(d[key + "_boards"].shape[0]):
            nb, ng = d[key + "_counts"][t]
            assert oracle.count_eligible(b) == nb
            b, _ = oracle.advance(b, 0.3, rng.take(nb))
            assert oracle.count_eligible(g) == ng
            g, _ = oracle.advance(g, 0.3, rng.take(ng))
            assert np.array_equal(b, d[key + "_boards"][t]), (key, t)
            assert np.array_equal(g, d[key + "_goals"][t]), (key, t)


def test_g1_128_known_answers():
    """G1 at 128x128 (C5's board size), captured from the reference."""
    d = np.load(os.path.join(GOLDEN, "advance_known_answers_128.npz"))
    assert len(d["boards_in"]) >= 50
    for b, want, p in zip(d["boards_in"], d["boards_out"], d["spawn_prob"]):
        got, _ = oracle.advance(b, p, np.zeros(b.size), 0)
        assert np.array_equal(got, want), p


def test_g2_128_reference_stream():
    """G2 at 128x128: C5 navigation levels advanced 30 times after speedups.seed(s)."""
    d = np.load(os.path.join(GOLDEN, "advance_stream_128.npz"))
    keys = sorted({k.rsplit("_", 1)[0] for k in d.files if k.endswith("_board0")})
    assert len(keys) >= 2
    for key in keys:
        rng = oracle.RefStreamRNG()
        rng.seed(int(key.split("_")[0][1:]))
        p = float(d[key + "_p"])
        b, g = d[key + "_board0"], d[key + "_goals0"]
        for t in range(d[key + "_boards"].shape[0]):
            b, _ = oracle.advance(b, p, rng.take(oracle.count_eligible(b)))
            g, _ = oracle.advance(g, p, rng.take(oracle.count_eligible(g)))
            assert np.array_equal(b, d[key + "_boards"][t]), (key, t)
            assert np.array_equal(g, d[key + "_goals"][t]), (key, t)


def _traj_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "traj_*.npz")))


def make_oracle_env(d, rng=None):
    penalty, min_perf, seed, vh, vw, time_limit = d["cfg"]
    lvl = oracle.Level(d["level_board"], d["level_goals"], d["level_agent_loc"],
                       d["level_orientation"], d["level_spawn_prob"],
                       d["level_min_performance"])
    if rng is None:
        rng = oracle.RefStreamRNG()
        rng.seed(int(seed))
    return oracle.OracleEnv(lambda ep: lvl, time_limit=int(time_limit),
                            view_shape=(int(vh), int(vw)), output_channels=None,
                            penalty_coef=float(penalty), min_performance=float(min_perf),
                            rng="stream", stream=rng)


@pytest.mark.parametrize("path", _traj_files(), ids=lambda p: os.path.basename(p)[5:-4])
def test_g3_trajectory(path):
    d = np.load(path)
    env = make_oracle_env(d)
    obs = env.reset()
    assert np.array_equal(obs, d["obs0"])
    T = len(d["action"])
    for t in range(T):
        obs, r, done, info = env.step(int(d["action"][t]))
        ctx = (os.path.basename(path), t)
        assert r == d["reward"][t], ctx          # bit-exact float64
        assert done == d["done"][t], ctx
        assert info["times_up"] == d["times_up"][t], ctx
        assert tuple(env.agent_loc) == tuple(d["agent_loc"][t]), ctx
        assert env.orientation == d["orientation"][t], ctx
        assert np.array_equal(env.board, d["board"][t]), ctx
        assert np.array_equal(env.goals, d["goals"][t]), ctx
        assert np.array_equal(obs, d["obs"][t]), ctx
        assert env.old_points == d["points"][t], ctx
        assert tuple(env._perf_ratio()) == tuple(d["perf"][t]), ctx
        assert env.last_side_effect == d["side_effect"][t], ctx


def _feat_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "feat_*.npz")))


def make_feat_oracle_env(d, cls=oracle.OracleEnv):
    env = make_oracle_env(d)
    powers, colors, period, remove_white = (int(v) for v in d["cfg_extra"])
    kw = dict(time_limit=env.time_limit, view_shape=env.view_shape, output_channels=None,
              penalty_coef=env.penalty_coef, min_performance=env.wrapper_min_performance,
              rng="stream", stream=env.stream, movement_bonus_period=period,
              remove_white_goals=bool(remove_white), can_toggle_powers=bool(powers),
              can_toggle_colors=bool(colors))
    return cls(env.level_fn, **kw)


def _check_traj_step(env, d, t, obs, r, done, info, ctx):
    assert r == d["reward"][t], ctx          # bit-exact float64
    assert done == d["done"][t], ctx
    assert info["times_up"] == d["times_up"][t], ctx
    assert tuple(env.agent_loc) == tuple(d["agent_loc"][t]), ctx
    assert env.orientation == d["orientation"][t], ctx
    assert np.array_equal(env.board, d["board"][t]), ctx
    assert np.array_equal(env.goals, d["goals"][t]), ctx
    assert np.array_equal(obs, d["obs"][t]), ctx
    assert env.old_points == d["points"][t], ctx
    assert env.last_side_effect == d["side_effect"][t], ctx


@pytest.mark.parametrize("path", _feat_files(), ids=lambda p: os.path.basename(p)[5:-4])
def test_g8_feature_trajectory(path):
    """Reference-captured trajectories on what the traj_* fixtures hold fixed: H != W,
    3 / 8 / 2 exits (np.nonzero order, two exits clipped to one view cell, all exits
    recoloured), toggles on, bonus periods 1 / 16 / 3, remove_white_goals off, an even
    non-square view and a view wider than twice the board.  The oracle follows the
    reference stream; every recorded quantity at every step."""
    d = np.load(path)
    assert len(_feat_files()) == 3
    env = make_feat_oracle_env(d)
    obs = env.reset()
    assert np.array_equal(obs, d["obs0"])
    for t in range(len(d["action"])):
        obs, r, done, info = env.step(int(d["action"][t]))
        ctx = (os.path.basename(path), t)
        _check_traj_step(env, d, t, obs, r, done, info, ctx)
        assert tuple(env._perf_ratio()) == tuple(d["perf"][t]), ctx


def test_g8_feature_trajectories_exercise_their_features():
    """The fixtures hold what they are for: game-over and time-limit resets, toggles that
    change the agent's power and colour bits, two exits clipped to one view cell, crates
    moved across the seam, an exit refused by can_exit."""
    import feature_pools
    seen = {}
    for path in _feat_files():
        d = np.load(path)
        env = make_feat_oracle_env(d, cls=feature_pools.TracingOracleEnv)
        env.reset()
        for a in d["action"]:
            env.step(int(a))
        seen[os.path.basename(path)[5:-4]] = (env.n, int(d["game_over"].sum()),
                                              int(d["times_up"].sum()))
    n, go, tu = seen["13x22_toggles"]
    assert tu >= 2 and n["toggle_power"] >= 1 and n["toggle_color"] >= 1, seen
    assert n["clipped_same"] >= 1 and n["push_seam"] >= 1, seen
    # (a 33x33 view holds every cell of a 21x9 board: its exits are always in view)
    n, go, tu = seen["21x9_exits8"]
    assert go >= 5 and n["exit_in_view"] >= 1 and n["pull_seam"] >= 1, seen
    n, go, tu = seen["10x10_view8x12"]
    assert go >= 1 and tu >= 1 and n["toggle_power"] >= 1 and n["toggle_color"] >= 1, seen
    assert n["can_exit_false"] >= 1, seen


def test_g8_cpu_batch_follows_reference_trajectory():
    """CpuBatch (sl_cpu_step.c) against the reference fixture itself where it can: the
    21x9 level has 8 exits and no spawner, so no uniform is ever drawn and the Philox-only
    CpuBatch replays the reference's trajectory (view 33x33, bonus period 16,
    remove_white_goals off).  CpuBatch's config takes neither can_toggle_powers nor
    can_toggle_colors and has no replay stream, so the two toggle fixtures (whose levels
    spawn) are out of its reach; its other settings meet the oracle in
    tests/test_feature_matrix_cpu.py."""
    d = np.load(os.path.join(GOLDEN, "feat_21x9_exits8.npz"))
    assert not ((d["level_board"] | d["level_goals"]) & oracle.SPAWNING).any()
    penalty, min_perf, seed, vh, vw, time_limit = d["cfg"]
    powers, colors, period, remove_white = (int(v) for v in d["cfg_extra"])
    assert not powers and not colors
    lvl = oracle.Level(d["level_board"], d["level_goals"], d["level_agent_loc"],
                       d["level_orientation"], d["level_spawn_prob"], d["level_min_performance"])
    cb = oracle.CpuBatch([lvl], 1, time_limit=int(time_limit), view_shape=(int(vh), int(vw)),
                         remove_white_goals=bool(remove_white), movement_bonus_period=period,
                         penalty_coef=float(penalty), min_performance=float(min_perf), obs=True)
    cb.reset()
    for t in range(len(d["action"])):
        o, r, dn = cb.step(np.array([d["action"][t]], np.int32), threads=1)
        ctx = t
        assert r[0] == d["reward"][t], ctx
        assert bool(dn[0]) == bool(d["done"][t]), ctx
        assert np.array_equal(cb.board(0), d["board"][t]), ctx
        assert np.array_equal(cb.board(0, 1), d["goals"][t]), ctx
        assert np.array_equal(o[0], d["obs"][t]), ctx
        s = cb.scalars(0)
        assert (s["agent_x"], s["agent_y"]) == tuple(d["agent_loc"][t]), ctx
        assert s["orientation"] == d["orientation"][t], ctx
        assert s["old_points"] == d["points"][t], ctx
        assert s["side_effect"] == d["side_effect"][t], ctx


def test_obs_channels_match_packed():
    d = np.load(_traj_files()[0])
    env = make_oracle_env(d)
    env.output_channels = tuple(range(15))
    o = env.reset()
    packed = (o.astype(np.uint32) << np.arange(15)).sum(-1)
    assert np.array_equal(packed, d["obs0"] & 0x7FFF)


def test_philox_known_values():
    # Philox4x32-10 published known-answer vectors (Random123 kat_vectors):
    # counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
    import ctypes
    out = (ctypes.c_uint32 * 4)()
    oracle.lib().orc_philox4x32.argtypes = [ctypes.c_void_p] + [ctypes.c_uint32] * 4 + [ctypes.c_uint64]
    oracle.lib().orc_philox4x32(out, 0, 0, 0, 0, 0)
    assert [hex(v) for v in out] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    oracle.lib().orc_philox4x32(out, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF,
                                0xFFFFFFFFFFFFFFFF)
    assert [hex(v) for v in out] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]


def test_symmetry_deterministic():
    """The rule commutes with toroidal roll / transpose / flips (p in {0,1})."""
    rng = np.random.RandomState(3)
    for _ in range(40):
        H, W = rng.randint(3, 20, size=2)
        b = rng.randint(0, 1 << 16, size=(H, W)).astype(np.uint16)
        b = (b * (rng.rand(H, W) < 0.5)).astype(np.uint16)
        for p in (0.0, 1.0):
            out, _ = oracle.advance(b, p)
            dy, dx = rng.randint(0, H), rng.randint(0, W)
            r, _ = oracle.advance(np.roll(b, (dy, dx), (0, 1)), p)
            assert np.array_equal(r, np.roll(out, (dy, dx), (0, 1)))
            t, _ = oracle.advance(np.ascontiguousarray(b.T), p)
            assert np.array_equal(t, out.T)
            f, _ = oracle.advance(np.ascontiguousarray(b[::-1]), p)
            assert np.array_equal(f, out[::-1])


def test_g5_side_effect_densities():
    """The oracle's rollout + density restatement reproduces the reference's
    _add_cell_distribution maps captured in densities.npz (replay RNG)."""
    d = np.load(os.path.join(GOLDEN, "densities.npz"))
    for j in range(2):
        stream = oracle.RefStreamRNG()
        stream.seed(11 + j)
        board = d["l%d_board" % j]
        ina, act = oracle.side_effect_densities(board, np.roll(board, 1, axis=1), 7,
                                                float(d["l%d_spawn" % j]), 20, rng="stream",
                                                stream=stream)
        for nm, got in (("inaction", ina), ("action", act)):
            keys = d["l%d_%s_keys" % (j, nm)].tolist()
            assert sorted(got) == keys, (j, nm)
            for k, ref in zip(keys, d["l%d_%s_dens" % (j, nm)]):
                assert np.array_equal(got[k], ref), (j, nm, k)
