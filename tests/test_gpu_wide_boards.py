"""The opt-in bit-sliced step kernel for boards of up to 128 x 128 with more than 64 rows or
more than 64 columns (k_env_step_wide, sl_bits_wide.hip; GeoWide, sl_bits_geo.h) on the
device.

1. against OracleEnv on the shapes of tests/wide_boards_cases.py, every env after every
   step (the checks of test_gpu_feature_matrix.py), episode ends and resets included;
2. against the per-cell kernel on dense soups over all 16 cell bits;
3. the dispatch: auto and generic stay generic, wide is wide, and what wide rejects;
4. the frames of a capture, against the per-cell kernel's.
Every comparison is == or array_equal.  tests/test_wide_boards_cpu.py checks on the CPU
that the cases exercise the geometry's seams with these very seeds.
"""
import os

import numpy as np
import pytest

import feature_pools as fp
import wide_boards_cases as wc
from test_gpu_feature_matrix import STATE_KEYS, _check_env, _views

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


# ------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("case", wc.CASES, ids=wc.CASE_IDS)
def test_wide_env_step_vs_oracle(torch_dev, case):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool
    ds = case.level_dicts()
    pool, levels = LevelPool.from_levels(ds), fp.oracle_levels(ds)
    venv = SafeLifeVecEnv(pool, case.B, dev, rng="philox", seed=case.pseed, kernel=case.kernel,
                          level_order="random", augment_roll=True, **case.env_kw())
    oenvs = fp.oracle_envs(case, levels)
    assert venv.kernel_family == "wide"

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
    resets = 0
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
        resets += int((flags & 4 != 0).sum())
    assert resets >= 1, case.name


# ------------------------------------------------------------------ 2. dense soups
@pytest.mark.parametrize("shape", wc.SOUP_SHAPES, ids=["%dx%d" % s for s in wc.SOUP_SHAPES])
def test_wide_kernel_vs_generic_on_soups(torch_dev, shape):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool
    H, W = shape
    pool = LevelPool.from_levels(wc.soup_levels(H, W))
    B, T = 18, 20
    kw = dict(time_limit=11, view_shape=(9, 9), output_channels=None, penalty_coef=0.7,
              min_performance=0.01, seed=5, level_order="random", augment_roll=True,
              can_toggle_powers=True, can_toggle_colors=True, rng="philox")
    wide = SafeLifeVecEnv(pool, B, dev, kernel="wide", **kw)
    gen = SafeLifeVecEnv(pool, B, dev, kernel="generic", **kw)
    assert (wide.kernel_family, gen.kernel_family) == ("wide", "generic")
    assert torch.equal(wide.reset(), gen.reset())
    rng = np.random.RandomState(H * 100 + W)
    resets = 0
    for t in range(T):
        a = torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev)
        o1, r1, d1, _ = wide.step(a)
        o2, r2, d2, _ = gen.step(a)
        assert torch.equal(r1, r2), (t, (r1 - r2).abs().max().item())
        assert torch.equal(d1, d2), t
        assert torch.equal(wide.flags, gen.flags), t
        assert torch.equal(o1, o2), t
        assert torch.equal(wide.board, gen.board), t
        assert torch.equal(wide.goals, gen.goals), t
        for k in wide.st_t:
            assert torch.equal(wide.st_t[k], gen.st_t[k]), (t, k)
        resets += int(((wide.flags & 4) != 0).sum().item())
    assert resets >= B


# ------------------------------------------------------------------ 3. dispatch
def test_dispatch_and_what_wide_rejects(torch_dev):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool, _lib
    pool = LevelPool.from_levels(fp.build_levels(7, 4, 65, 65, 2))
    kw = dict(time_limit=15, view_shape=(9, 9), output_channels=None, seed=3)
    fam = {k: SafeLifeVecEnv(pool, 4, dev, kernel=k, rng="philox", **kw).kernel_family
           for k in ("auto", "generic", "wide")}
    assert fam == {"auto": "generic", "generic": "generic", "wide": "wide"}
    code = r"code %d\)" % _lib.SL_ETOOBIG
    small = LevelPool.from_levels(fp.build_levels(7, 4, 48, 48, 2))
    with pytest.raises(RuntimeError, match=code):
        env = SafeLifeVecEnv(small, 4, dev, kernel="wide", rng="philox", **kw)
        env.reset()
        env.step(torch.zeros(4, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match=code):
        env = SafeLifeVecEnv(pool, 4, dev, kernel="wide", rng="stream",
                             spawn_stream=np.random.RandomState(0).random_sample(100000), **kw)
        env.reset()
        env.step(torch.zeros(4, dtype=torch.int32, device=dev))


# ------------------------------------------------------------------ 4. capture
def test_wide_capture_frames_equal_generic(torch_dev, tmp_path):
    """A recorder on env 0 at 65x65: the same episodes with the same frames (the one copied
    before the reset included) under kernel="wide" as under kernel="generic"."""
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool
    from safelife_amd.recorder import TrajectoryRecorder
    pool = LevelPool.from_levels(fp.build_levels(11, 6, 65, 65, 2))
    B, T = 8, 40
    kw = dict(time_limit=13, view_shape=(5, 5), output_channels=None, penalty_coef=1.0,
              min_performance=-1.0, rng="philox", seed=6)
    acts = np.random.RandomState(2).randint(0, 9, size=(T, B)).astype(np.int32)
    out = {}
    for kernel in ("wide", "generic"):
        venv = SafeLifeVecEnv(pool, B, dev, kernel=kernel, **kw)
        assert venv.kernel_family == kernel
        venv.reset()
        rec = TrajectoryRecorder(venv, str(tmp_path / kernel / "ep-{env}-{episode_num}"),
                                 env_ids=[0], video_recording_freq=1, ring=16)
        for t in range(T):
            venv.step(torch.from_numpy(acts[t]).to(dev))
        files = sorted(rec.close())
        out[kernel] = {os.path.basename(f): np.load(f) for f in files}
    assert len(out["wide"]) >= 2 and sorted(out["wide"]) == sorted(out["generic"])
    for name, z in out["wide"].items():
        g = out["generic"][name]
        assert sorted(z.files) == sorted(g.files), name
        for k in z.files:
            assert np.array_equal(z[k], g[k]), (name, k)
