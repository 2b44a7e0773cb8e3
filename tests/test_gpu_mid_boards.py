"""The bit-sliced step kernel for boards of 33 to 64 rows and up to 64 columns
(k_env_step_mid, sl_bits_mid.hip; GeoMid, sl_bits_geo.h) on the device.

1. against OracleEnv on the shapes of tests/mid_boards_cases.py, every env after every
   step (the checks of test_gpu_feature_matrix.py), Philox and replay;
2. against the per-cell kernel on dense soups over all 16 cell bits;
3. batches of 1 and 3 envs;
4. what kernel="auto" picks, and that auto, fast and generic agree;
5. the pre-reset frame of a capture.
Every comparison is == or array_equal.  tests/test_mid_boards_cpu.py checks on the CPU
that the cases exercise the geometry's seams with these very seeds.
"""
import ctypes

import numpy as np
import pytest

import oracle
import feature_pools as fp
import mid_boards_cases as mc
from test_gpu_feature_matrix import STATE_KEYS, _check_env, _views

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _run_case_vs_oracle(torch, dev, case, B=None, **venv_kw):
    from safelife_amd import SafeLifeVecEnv, LevelPool
    ds = case.level_dicts()
    pool, levels = LevelPool.from_levels(ds), fp.oracle_levels(ds)
    if B is not None:
        case = fp.Case(case.name, case.shape, case.family, case.kernel, n_exits=case.n_exits,
                       toggles=case.toggles, period=case.period, remove_white=case.remove_white,
                       view=case.view, penalty=case.penalty, min_perf=case.min_perf, B=B,
                       T=case.T, rng=case.rng, exit_rows=case.exit_rows, seed=case.seed,
                       time_limit=case.time_limit, pseed=case.pseed)
    B = case.B
    kw = case.env_kw()
    kw.update(venv_kw)
    if case.rng == "stream":
        draws = np.random.RandomState(case.seed).random_sample(400000)
        if "spawn_stream" not in venv_kw:
            kw["spawn_stream"] = draws
        venv = SafeLifeVecEnv(pool, B, dev, rng="stream", kernel=case.kernel, **kw)
        oenvs = fp.oracle_envs(case, levels, stream=fp.SharedStream(draws))
    else:
        venv = SafeLifeVecEnv(pool, B, dev, rng="philox", seed=case.pseed, kernel=case.kernel,
                              level_order="random", augment_roll=True, **kw)
        oenvs = fp.oracle_envs(case, levels)
    assert venv.kernel_family == "mid"

    def state():
        st = {k: venv.st_t[k].cpu().numpy() for k in STATE_KEYS}
        return st, venv._board.cpu().numpy(), venv.goals.cpu().numpy()

    views = _views(torch, venv.reset())
    for o in oenvs:
        o.reset()
    st, board, goals = state()
    for e, o in enumerate(oenvs):
        _check_env(venv, st, board, goals, views, e, o, (case.name, "reset", e))
    acts, us = case.actions()
    for t in range(case.T):
        a = np.array([fp.case_action(case, o, acts[t, e], us[t, e])
                      for e, o in enumerate(oenvs)], np.int32)
        vo, vr, vd, info = venv.step(torch.from_numpy(a).to(dev))
        views, vr, vd = _views(torch, vo), vr.cpu().numpy(), vd.cpu().numpy()
        flags = venv.flags.cpu().numpy()
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
    if case.rng == "stream":
        assert not venv.stream_error()
    return venv


# ------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("case", mc.ALL_CASES, ids=mc.CASE_IDS)
def test_mid_env_step_vs_oracle(torch_dev, case):
    torch, dev = torch_dev
    assert case.B % 4 != 0 and 25 <= case.B <= 27
    _run_case_vs_oracle(torch, dev, case)


def test_mid_env_step_vs_oracle_device_generator(torch_dev):
    """33x33 replay with the stream generated on the device: the ring form the pool's
    single threshold selects (a bit ring), against the same seeded stream on the host."""
    torch, dev = torch_dev
    case = mc.STREAM_CASES[0]
    venv = _run_case_vs_oracle(torch, dev, case, spawn_stream=None, seed=case.seed)
    assert venv.mt is not None


# ------------------------------------------------------------------ 2. dense soups
def _compare_state(e1, e2, ctx):
    assert np.array_equal(e1.board.cpu().numpy(), e2.board.cpu().numpy()), ctx
    assert np.array_equal(e1.goals.cpu().numpy(), e2.goals.cpu().numpy()), ctx
    for k in e1.st_t:
        assert np.array_equal(e1.st_t[k].cpu().numpy(), e2.st_t[k].cpu().numpy()), (ctx, k)


@pytest.mark.parametrize("rng_mode", ["philox", "stream"])
@pytest.mark.parametrize("shape", mc.SOUP_SHAPES, ids=["%dx%d" % s for s in mc.SOUP_SHAPES])
def test_mid_kernel_vs_generic_on_soups(torch_dev, shape, rng_mode):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool
    H, W = shape
    pool = LevelPool.from_levels(mc.soup_levels(H, W))
    B, T = 64, 40
    kw = dict(time_limit=11, view_shape=(9, 9), output_channels=None, penalty_coef=0.7,
              min_performance=0.01, seed=5, level_order="random", augment_roll=True,
              can_toggle_powers=True, can_toggle_colors=True)
    if rng_mode == "stream":
        kw.update(rng="stream", spawn_stream=np.random.RandomState(9).random_sample(6000000))
    else:
        kw.update(rng="philox")
    fast = SafeLifeVecEnv(pool, B, dev, kernel="fast", **kw)
    gen = SafeLifeVecEnv(pool, B, dev, kernel="generic", **kw)
    assert (fast.kernel_family, gen.kernel_family) == ("mid", "generic")
    assert torch.equal(fast.reset(), gen.reset())
    rng = np.random.RandomState(H * 100 + W)
    resets = 0
    for t in range(T):
        a = torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev)
        o1, r1, d1, _ = fast.step(a)
        o2, r2, d2, _ = gen.step(a)
        assert torch.equal(r1, r2), (t, (r1 - r2).abs().max().item())
        assert torch.equal(d1, d2), t
        assert torch.equal(fast.flags, gen.flags), t
        assert torch.equal(o1, o2), t
        _compare_state(fast, gen, t)
        resets += int(((fast.flags & 4) != 0).sum().item())
    assert resets >= B
    if rng_mode == "stream":
        assert not fast.stream_error() and not gen.stream_error()


# ------------------------------------------------------------------ 3. tiny batches
@pytest.mark.parametrize("B", [1, 3])
def test_mid_tiny_batches_vs_oracle(torch_dev, B):
    torch, dev = torch_dev
    _run_case_vs_oracle(torch, dev, mc.CASES[0], B=B)


# ------------------------------------------------------------------ 4. kernel="auto"
def test_auto_takes_the_mid_kernel(torch_dev):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool
    pool = LevelPool.from_levels(fp.build_levels(7, 8, 48, 48, 2))
    wide = LevelPool.from_levels(fp.build_levels(7, 4, 40, 70, 2))
    kw = dict(time_limit=15, view_shape=(9, 9), output_channels=None, rng="philox", seed=3,
              level_order="random", augment_roll=True)
    envs = {k: SafeLifeVecEnv(pool, 26, dev, kernel=k, **kw) for k in ("auto", "fast", "generic")}
    assert envs["auto"].kernel_family == "mid"
    assert envs["fast"].kernel_family == "mid"
    assert envs["generic"].kernel_family == "generic"
    assert SafeLifeVecEnv(wide, 4, dev, kernel="auto", **kw).kernel_family == "generic"
    for v in envs.values():
        v.reset()
    rng = np.random.RandomState(1)
    for t in range(30):
        a = torch.from_numpy(rng.randint(0, 9, size=26).astype(np.int32)).to(dev)
        out = {k: v.step(a) for k, v in envs.items()}
        for k in ("fast", "generic"):
            assert torch.equal(out["auto"][1], out[k][1]), (t, k)
            assert torch.equal(envs["auto"].board, envs[k].board), (t, k)
            assert torch.equal(envs["auto"].goals, envs[k].goals), (t, k)


# ------------------------------------------------------------------ 5. capture
def test_mid_capture_pre_reset_frame(torch_dev, tmp_path):
    """With a recorder attached at 40x40 the frame copied before the reset is the
    finished episode's last board (the oracle restatement of test_gpu_feed_record.py);
    stepping on after detaching stays on the oracle."""
    torch, dev = torch_dev
    import os
    from safelife_amd import SafeLifeVecEnv, LevelPool
    from safelife_amd.recorder import TrajectoryRecorder
    from test_gpu_feed_record import _exit_next_to_agent, _expected_recordings
    levels = _exit_next_to_agent(fp.oracle_levels(fp.build_levels(11, 6, 40, 40, 1)))
    pool = LevelPool.from_levels([{"board": lv.board, "goals": lv.goals,
                                   "agent_loc": lv.agent_loc, "orientation": lv.orientation,
                                   "spawn_prob": lv.spawn_prob,
                                   "min_performance": lv.min_performance} for lv in levels])
    B, T, freq = 8, 50, 2
    env_ids = [0, 3, 7]
    kw = dict(time_limit=13, view_shape=(5, 5), output_channels=None, penalty_coef=1.0,
              min_performance=-1.0)
    venv = SafeLifeVecEnv(pool, B, dev, rng="philox", seed=6, kernel="fast", **kw)
    assert venv.kernel_family == "mid"
    venv.reset()
    rec = TrajectoryRecorder(venv, str(tmp_path / "ep-{env}-{episode_num}"), env_ids=env_ids,
                             video_recording_freq=freq, ring=16)
    rng = np.random.RandomState(2)
    acts = rng.choice(9, size=(T + 10, B),
                      p=[.04, .06, .5, .06, .06, .07, .07, .07, .07]).astype(np.int32)
    overs = 0
    for t in range(T):
        venv.step(torch.from_numpy(acts[t]).to(dev))
        overs += int(((venv.flags & 2) != 0).sum().item())
    files = rec.close()
    assert overs > 0
    exp = _expected_recordings(levels, env_ids, B, T, acts, kw, freq)
    for e in env_ids:
        mine = [f for f in files if os.path.basename(f).startswith("ep-%d-" % e)]
        mine.sort(key=lambda f: int(os.path.basename(f)[:-4].split("-")[2]))
        assert [int(os.path.basename(f)[:-4].split("-")[2]) for f in mine] == \
            [n for n, _ in exp[e]], e
        for f, (num, frames) in zip(mine, exp[e]):
            z = np.load(f)
            assert np.array_equal(z["orientation"], [fr[0] for fr in frames]), (e, num)
            assert np.array_equal(z["board"], np.stack([fr[1] for fr in frames])), (e, num)
            assert np.array_equal(z["goals"], np.stack([fr[2] for fr in frames])), (e, num)
    # detached: the resets are the step kernel's own again
    oenvs = [oracle.OracleEnv(oracle.pool_level_fn(levels, e, n_total=B), env_id=e,
                              rng="philox", seed=6, **kw) for e in range(B)]
    for o in oenvs:
        o.reset()
    for t in range(T + 10):
        if t >= T:
            venv.step(torch.from_numpy(acts[t]).to(dev))
        for e, o in enumerate(oenvs):
            o.step(int(acts[t, e]))
    board = venv.board.cpu().numpy()
    for e, o in enumerate(oenvs):
        assert np.array_equal(board[e], o.board), e


def test_c_abi_family_and_toobig(torch_dev):
    """sl_env_step itself: SL_KERNEL_FAST steps a 48x48 state and still rejects 40x70."""
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool, _lib
    wide = LevelPool.from_levels(fp.build_levels(7, 4, 40, 70, 2))
    env = SafeLifeVecEnv(wide, 4, dev, kernel="fast", output_channels=None)
    env.reset()
    with pytest.raises(RuntimeError):
        env.step(torch.zeros(4, dtype=torch.int32, device=dev))
    assert _lib.lib().sl_env_step_family(40, 70, _lib.SL_KERNEL_FAST) == _lib.SL_ETOOBIG
    assert ctypes.c_int(_lib.lib().sl_env_step_family(48, 48, _lib.SL_KERNEL_FAST)).value == \
        _lib.SL_FAMILY_MID
