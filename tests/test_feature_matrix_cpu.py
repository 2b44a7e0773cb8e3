"""(CPU) The feature matrix of tests/feature_pools.py, run by the oracle alone: every case
exercises what it is there for, with the seeds, T and action mix the GPU tests use
(tests/test_gpu_feature_matrix.py).  And the compiled chain (CpuBatch, sl_cpu_step.c)
against the oracle over the same cases.

Conditions, not measurements: a case that stops meeting one no longer tests its feature.
"""
import numpy as np
import pytest

import oracle
import feature_pools as fp


def run_oracle_case(case):
    """The case's trajectory on TracingOracleEnv's; returns (envs, levels, done counts)."""
    levels = fp.oracle_levels(case.level_dicts())
    stream = fp.SharedStream(np.random.RandomState(case.seed).random_sample(400000))
    envs = fp.oracle_envs(case, levels, cls=fp.TracingOracleEnv, stream=stream)
    for o in envs:
        o.reset()
    acts, us = case.actions()
    for t in range(case.T):
        for e, o in enumerate(envs):
            o.step(fp.case_action(case, o, acts[t, e], us[t, e]))
    return envs, levels


def _view_covers_board(case):
    return case.view[0] >= case.shape[0] and case.view[1] >= case.shape[1]


@pytest.mark.parametrize("case", fp.CASES, ids=fp.CASE_IDS)
def test_case_exercises_its_features(case):
    envs, levels = run_oracle_case(case)
    total = {k: sum(o.n[k] for o in envs) for k in envs[0].n}
    ctx = (case.name, total)
    for lv in levels:
        assert 1 <= int(((lv.board & oracle.EXIT) != 0).sum()) <= fp.MAX_EXITS
    if case.shape != (2, 2):
        assert max(int(((lv.board & oracle.EXIT) != 0).sum()) for lv in levels) == case.n_exits
    # every env resets at least twice; at least one reset is a game over through an exit
    assert min(o.n["resets"] for o in envs) >= 2, ctx
    assert total["exit_resets"] >= 1, ctx
    if case.shape[0] * case.shape[1] >= 20:       # (a 2x2 board has no room for a crate)
        assert total["push_seam"] >= 1 and total["pull_seam"] >= 1, ctx
    if case.toggles:
        assert total["toggle_power"] >= 1 and total["toggle_color"] >= 1, ctx
    else:
        assert total["toggle_power"] == 0 and total["toggle_color"] == 0, ctx
    if case.multi_exit:
        assert total["exit_in_view"] >= 1, ctx
        if not _view_covers_board(case):          # (a view holding the whole board never clips)
            assert total["clipped_same"] >= 1, ctx
    if case.min_perf >= 0:                        # can_exit is sometimes false at an exit
        assert total["can_exit_false"] >= 1, ctx
    if case.multi_exit and case.rng == "philox":
        # augment_roll: some rolled level's np.nonzero exit order is not the unrolled one
        differs = 0
        for e in range(case.B):
            fn = oracle.pool_level_fn(levels, e, seed=case.pseed, n_total=case.B,
                                      random_order=True, augment=True)
            plain = oracle.pool_level_fn(levels, e, seed=case.pseed, n_total=case.B,
                                         random_order=True, augment=False)
            for ep in range(3):
                r, u = fn(ep), plain(ep)
                H, W = u.board.shape
                dy = (r.agent_loc[1] - u.agent_loc[1]) % H
                dx = (r.agent_loc[0] - u.agent_loc[0]) % W
                uy, ux = np.nonzero(u.board & oracle.EXIT)
                moved = list(zip(((uy + dy) % H).tolist(), ((ux + dx) % W).tolist()))
                ry, rx = np.nonzero(r.board & oracle.EXIT)
                differs += moved != list(zip(ry.tolist(), rx.tolist()))
        assert differs >= 1, ctx


def test_matrix_covers_every_setting_in_every_family():
    """Each setting of the issue's list appears on at least one shape of every kernel
    family (not a full product)."""
    fams = sorted({c.family for c in fp.CASES})
    assert len(fams) == 6
    for fam in fams:
        cs = [c for c in fp.CASES if c.family == fam]
        have = lambda f: {f(c) for c in cs}
        assert have(lambda c: c.n_exits) >= {1, 2, 8}, fam
        assert have(lambda c: c.toggles) == {False, True}, fam
        assert have(lambda c: c.period) >= {0, 1, 4, 16}, fam
        assert have(lambda c: c.remove_white) == {False, True}, fam
        assert have(lambda c: c.view) >= {(9, 9), (8, 12), (33, 33)}, fam
        assert have(lambda c: c.penalty) >= {0.0, 0.7}, fam
        assert have(lambda c: c.min_perf) >= {-1.0, 0.01, 0.5}, fam
    assert any(c.shape == (5, 9) and c.view == (15, 15) for c in fp.CASES)
    assert sum(c.rng == "stream" for c in fp.CASES) == 2


@pytest.mark.parametrize("case", [c for c in fp.CASES if c.rng == "philox"],
                         ids=[c.name for c in fp.CASES if c.rng == "philox"])
def test_cpu_batch_vs_oracle_on_case(case):
    """CpuBatch against OracleEnv on the case's pool, order, rolls, view, bonus period,
    remove_white_goals, penalty and min_performance: reward, done, board, goals, packed
    view, agent, orientation, points, side effect, exit count at every step.  CpuBatch's
    config has no can_toggle_powers / can_toggle_colors, so both sides run with the
    toggles off here (the toggles meet the reference in test_oracle.py's fixtures)."""
    levels = fp.oracle_levels(case.level_dicts())
    kw = case.env_kw()
    kw.update(can_toggle_powers=False, can_toggle_colors=False, output_channels=None)
    B = min(case.B, 8)
    oenvs = [oracle.OracleEnv(oracle.pool_level_fn(levels, e, seed=case.pseed, n_total=B,
                                                   random_order=True, augment=True),
                              env_id=e, rng="philox", seed=case.pseed, **kw) for e in range(B)]
    cb = oracle.CpuBatch(levels, B, time_limit=case.time_limit, view_shape=case.view,
                         remove_white_goals=case.remove_white, movement_bonus_period=case.period,
                         penalty_coef=case.penalty, min_performance=case.min_perf,
                         seed=case.pseed, level_order="random", augment_roll=True, obs=True)
    cb.reset()
    for o in oenvs:
        o.reset()
    acts, us = case.actions()
    for t in range(case.T):
        a = np.array([fp.case_action(case, o, acts[t, e], us[t, e])
                      for e, o in enumerate(oenvs)], np.int32)
        obs, r, d = cb.step(a, threads=2)
        for e, o in enumerate(oenvs):
            oo, rr, dd, _ = o.step(int(a[e]))
            ctx = (case.name, t, e)
            assert r[e] == rr, (ctx, r[e], rr)
            assert bool(d[e]) == dd, ctx
            assert np.array_equal(cb.board(e), o.board), ctx
            assert np.array_equal(cb.board(e, 1), o.goals), ctx
            assert np.array_equal(obs[e], oo), ctx
            s = cb.scalars(e)
            assert (s["agent_x"], s["agent_y"]) == o.agent_loc, ctx
            assert s["orientation"] == o.orientation, ctx
            assert s["old_points"] == o.old_points, ctx
            assert s["side_effect"] == o.last_side_effect, ctx
            assert s["exit_count"] == len(o.exits), ctx
