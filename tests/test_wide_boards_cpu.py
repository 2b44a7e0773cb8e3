"""(CPU) The opt-in step kernel for boards of up to 128 x 128 with more than 64 rows or
more than 64 columns (SL_KERNEL_WIDE, SL_FAMILY_WIDE): the dispatch table of
sl_env_step_family over every shape up to 130 x 130, the plan of such a step
(sl_env_step_plan), and the GPU cases of tests/wide_boards_cases.py run by the oracle
alone, to see that each exercises the seams of the kernel's layout (rows H-1 | 0, columns
W-1 | 0, spawns, resets) with the seeds, T and action mix tests/test_gpu_wide_boards.py uses.

Conditions, not measurements: a case that stops meeting one no longer tests its feature.
"""
import ctypes

import numpy as np
import pytest

import oracle
import feature_pools as fp
import wide_boards_cases as wc
from test_step_plan_cpu import CAPTURE, P, cfg, plan, pool, replay, state, views  # noqa: F401


@pytest.fixture(scope="module")
def L():
    from safelife_amd import _lib
    _lib.build()
    return _lib.lib()


def _lib():
    from safelife_amd import _lib
    return _lib


def _wide(H, W):
    return 2 <= H <= 128 and 2 <= W <= 128 and (H > 64 or W > 64) and (H, W) != (128, 128)


# ------------------------------------------------------------------ dispatch table
def test_constants():
    lib = _lib()
    assert (lib.SL_KERNEL_WIDE, lib.SL_FAMILY_WIDE) == (5, 6)
    assert lib.FAMILY_NAMES[lib.SL_FAMILY_WIDE] == "wide"


def test_family_table_wide(L):
    lib = _lib()
    fam = L.sl_env_step_family
    n = 0
    for H in range(1, 131):
        for W in range(1, 131):
            want = lib.SL_FAMILY_WIDE if _wide(H, W) else lib.SL_ETOOBIG
            assert fam(H, W, lib.SL_KERNEL_WIDE) == want, (H, W)
            n += want == lib.SL_FAMILY_WIDE
    assert n == 127 * 127 - 63 * 63 - 1
    for shape in ((80, 80), (96, 96), (100, 100), (40, 128), (128, 64), (65, 128), (3, 65),
                  (65, 2), (2, 65), (128, 127), (127, 128)):
        assert fam(shape[0], shape[1], lib.SL_KERNEL_WIDE) == lib.SL_FAMILY_WIDE, shape
    for shape in ((128, 128), (64, 64), (48, 48), (1, 65), (65, 1), (129, 2), (2, 129), (32, 64)):
        assert fam(shape[0], shape[1], lib.SL_KERNEL_WIDE) == lib.SL_ETOOBIG, shape
    assert fam(0, 70, lib.SL_KERNEL_WIDE) == lib.SL_EINVAL
    assert fam(70, -1, lib.SL_KERNEL_WIDE) == lib.SL_EINVAL
    assert lib.env_step_family(96, 96, lib.SL_KERNEL_WIDE) == "wide"
    with pytest.raises(RuntimeError, match=r"code -3"):
        lib.env_step_family(48, 48, lib.SL_KERNEL_WIDE)


def test_no_other_request_answers_wide(L):
    lib = _lib()
    fam = L.sl_env_step_family
    for kernel in (lib.SL_KERNEL_AUTO, lib.SL_KERNEL_FAST, lib.SL_KERNEL_GENERIC):
        for H in range(1, 131):
            for W in range(1, 131):
                assert fam(H, W, kernel) != lib.SL_FAMILY_WIDE, (H, W, kernel)


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("shape", [(65, 65), (96, 96), (40, 128), (128, 64), (3, 65)])
def test_plan_of_a_wide_step(L, shape):
    lib = _lib()
    H, W = shape
    st = state(H, W)
    for with_views in (False, True):
        kw = views(lib.SL_OBS_PACKED, 9, 9) if with_views else {}
        want_obs = lib.SL_PLAN_OBS_SEPARATE if with_views else lib.SL_PLAN_OBS_NONE
        for auto_reset in (0, 1):
            for cap in (False, True):
                if cap and not auto_reset:
                    continue            # (a capture needs auto-reset: SL_EINVAL for any family)
                c = cfg(kernel=lib.SL_KERNEL_WIDE, auto_reset=auto_reset, **kw)
                if cap:
                    c.capture = ctypes.addressof(CAPTURE)
                rc, p = plan(L, st, c, pool(H, W) if auto_reset else None)
                assert rc == lib.SL_OK, (shape, with_views, auto_reset, cap)
                assert p.family == lib.SL_FAMILY_WIDE
                assert (p.plane_mode, p.demote_first, p.kernel64, p.view_kind) == (0, 0, 0, 0)
                assert p.obs == want_obs
                assert p.resets == (lib.SL_PLAN_RESETS_SCAN if auto_reset
                                    else lib.SL_PLAN_RESETS_NONE)
                assert p.capture == int(cap) and p.replay == 0


def test_plan_rejects_stream_and_other_shapes(L):
    lib = _lib()
    assert plan(L, state(65, 65), replay(kernel=lib.SL_KERNEL_WIDE))[0] == lib.SL_ETOOBIG
    assert plan(L, state(96, 96), replay(kernel=lib.SL_KERNEL_WIDE))[0] == lib.SL_ETOOBIG
    for H, W in ((128, 128), (64, 64), (48, 48)):
        st = state(H, W, planes=P + 0x300000, planes_ok=P + 0x400000)
        assert plan(L, st, cfg(kernel=lib.SL_KERNEL_WIDE))[0] == lib.SL_ETOOBIG, (H, W)
    # the other requests plan such a shape as before
    assert plan(L, state(65, 65), cfg())[1].family == lib.SL_FAMILY_GENERIC
    assert plan(L, state(65, 65), cfg(kernel=lib.SL_KERNEL_FAST))[0] == lib.SL_ETOOBIG


# ------------------------------------------------------------------ case coverage
class EdgeTracer(fp.TracingOracleEnv):
    """TracingOracleEnv that also counts what the banded layout is there to get right:
    cells born or dying on the board's first and last row and column, and spawns."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.n.update(row_first=0, row_last=0, col_first=0, col_last=0, spawns=0, spawners=0)

    def _advance(self, x, tensor):
        out = super()._advance(x, tensor)
        if tensor == 0:
            alive = (x & oracle.ALIVE) != 0
            flip = alive != ((out & oracle.ALIVE) != 0)
            self.n["row_first"] += bool(flip[0].any())
            self.n["row_last"] += bool(flip[-1].any())
            self.n["col_first"] += bool(flip[:, 0].any())
            self.n["col_last"] += bool(flip[:, -1].any())
            # a cell the advance made alive with other than three living neighbours was
            # no birth of the rule: it spawned
            nb = sum(np.roll(np.roll(alive, dy, 0), dx, 1).astype(np.int32)
                     for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
            self.n["spawns"] += bool((flip & ~alive & (nb != 3)).any())
            self.n["spawners"] += bool((x & oracle.SPAWNING).any())
        return out


def _run(case):
    levels = fp.oracle_levels(case.level_dicts())
    envs = fp.oracle_envs(case, levels, cls=EdgeTracer)
    for o in envs:
        o.reset()
    acts, us = case.actions()
    for t in range(case.T):
        for e, o in enumerate(envs):
            o.step(fp.case_action(case, o, acts[t, e], us[t, e]))
    return envs


def test_the_cases_are_the_issues():
    assert [c.shape for c in wc.CASES] == [(3, 65), (65, 2), (64, 66), (65, 65), (96, 127),
                                           (97, 128), (128, 127), (127, 128), (100, 20)]
    by = {c.shape: c for c in wc.CASES}
    c = by[(65, 65)]
    assert c.n_exits > 1 and c.toggles and c.period == 1 and c.view == (9, 9)
    assert by[(96, 127)].exit_rows == (0, 31, 32, 95)
    assert by[(97, 128)].min_perf == 0.5
    assert wc.SOUP_SHAPES == [(3, 65), (65, 65), (97, 128)]


@pytest.mark.parametrize("case", wc.CASES, ids=wc.CASE_IDS)
def test_wide_case_exercises_the_seams(case):
    H, W = case.shape
    assert _wide(H, W)
    assert (case.family, case.kernel, case.rng) == ("wide", "wide", "philox")
    assert 8 <= case.B <= 16 and case.T == 30
    envs = _run(case)
    total = {k: sum(o.n[k] for o in envs) for k in envs[0].n}
    ctx = (case.name, total)
    assert total["row_first"] >= 1 and total["row_last"] >= 1, ctx
    assert total["col_first"] >= 1 and total["col_last"] >= 1, ctx
    if total["spawners"]:
        assert total["spawns"] >= 1, ctx
    assert total["resets"] >= 1, ctx


@pytest.mark.parametrize("shape", wc.SOUP_SHAPES, ids=["%dx%d" % s for s in wc.SOUP_SHAPES])
def test_soups_change_on_every_seam_at_step_one(shape):
    """The dense soups of the wide-against-generic test: the first advance changes a cell
    in the first and last row of every band and in columns 0, W-1 of some level."""
    H, W = shape
    rows, cols = set(), set()
    for d in wc.soup_levels(H, W):
        after, _ = oracle.advance(d["board"], d["spawn_prob"],
                                  np.random.RandomState(0).random_sample(2 * H * W))
        diff = after != d["board"]
        rows |= set(np.nonzero(diff.any(1))[0].tolist())
        cols |= set(np.nonzero(diff.any(0))[0].tolist())
    seams = {0, H - 1} | {r for t in range(1, (H + 31) // 32) for r in (32 * t - 1, 32 * t)}
    assert seams <= rows, sorted(rows)
    assert {0, W - 1} <= cols, sorted(cols)
