"""(CPU) The step kernel for boards of 33 to 64 rows: the dispatch table of
sl_env_step_family over every shape up to 130 x 130, and the GPU cases of
tests/mid_boards_cases.py run by the oracle alone, to see that each exercises the seams of
the kernel's layout (rows 31 | 32, rows H-1 | 0, columns W-1 | 0) with the seeds, T and
action mix tests/test_gpu_mid_boards.py uses.

Conditions, not measurements: a case that stops meeting one no longer tests its feature.
"""
import numpy as np
import pytest

import oracle
import feature_pools as fp
import mid_boards_cases as mc


# ------------------------------------------------------------------ dispatch table
def _family():
    from safelife_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "sl_env_step_family")
    return _lib, L.sl_env_step_family


def _expected(_lib, H, W):
    """the bit-sliced family of H x W, or None"""
    if (H, W) == (64, 64):
        return _lib.SL_FAMILY_BITS64
    if (H, W) == (128, 128):
        return _lib.SL_FAMILY_BITS128
    if 2 <= H <= 32 and 2 <= W <= 32:
        return _lib.SL_FAMILY_SMALL_SEG4
    if 2 <= H <= 32 and 2 <= W <= 64:
        return _lib.SL_FAMILY_SMALL
    if 33 <= H <= 64 and 2 <= W <= 64:
        return _lib.SL_FAMILY_MID
    return None


def test_family_table():
    _lib, fam = _family()
    assert [_lib.SL_FAMILY_GENERIC, _lib.SL_FAMILY_SMALL_SEG4, _lib.SL_FAMILY_SMALL,
            _lib.SL_FAMILY_MID, _lib.SL_FAMILY_BITS64, _lib.SL_FAMILY_BITS128] == list(range(6))
    n_mid = 0
    for H in range(1, 131):
        for W in range(1, 131):
            want = _expected(_lib, H, W)
            auto = fam(H, W, _lib.SL_KERNEL_AUTO)
            fast = fam(H, W, _lib.SL_KERNEL_FAST)
            assert fam(H, W, _lib.SL_KERNEL_GENERIC) == _lib.SL_FAMILY_GENERIC, (H, W)
            assert fast == (_lib.SL_ETOOBIG if want is None else want), (H, W, fast)
            # AUTO may leave part of the mid range on the per-cell kernel (where a
            # measurement says so); everywhere else it is FAST's answer or generic
            if want == _lib.SL_FAMILY_MID:
                assert auto in (_lib.SL_FAMILY_MID, _lib.SL_FAMILY_GENERIC), (H, W, auto)
                n_mid += auto == _lib.SL_FAMILY_MID
            else:
                assert auto == (_lib.SL_FAMILY_GENERIC if want is None else want), (H, W, auto)
    assert n_mid > 0
    # the shapes named where the kernel was asked for, and the rejected one the C ABI
    # test relies on
    for shape in ((33, 40), (40, 40), (48, 48), (50, 50), (64, 48), (35, 64), (33, 2), (64, 63)):
        assert fam(shape[0], shape[1], _lib.SL_KERNEL_FAST) == _lib.SL_FAMILY_MID, shape
    assert fam(40, 70, _lib.SL_KERNEL_FAST) == _lib.SL_ETOOBIG
    assert fam(40, 70, _lib.SL_KERNEL_AUTO) == _lib.SL_FAMILY_GENERIC


def test_family_rejects_bad_arguments():
    _lib, fam = _family()
    assert fam(0, 5, _lib.SL_KERNEL_AUTO) == _lib.SL_EINVAL
    assert fam(5, -1, _lib.SL_KERNEL_AUTO) == _lib.SL_EINVAL
    assert fam(48, 48, _lib.SL_KERNEL_BANDS) == _lib.SL_EINVAL
    assert fam(48, 48, 17) == _lib.SL_EINVAL
    assert _lib.env_step_family(48, 48, _lib.SL_KERNEL_FAST) == "mid"
    assert _lib.env_step_family(40, 70) == "generic"
    with pytest.raises(RuntimeError):
        _lib.env_step_family(40, 70, _lib.SL_KERNEL_FAST)


# ------------------------------------------------------------------ case coverage
class SeamTracer(fp.TracingOracleEnv):
    """TracingOracleEnv that also counts what the split layout is there to get right."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.n.update(time_resets=0, spawn_low=0, spawn_high=0, cross_mid=0, cross_wrap=0,
                      both_edge_columns=0)

    def _advance(self, x, tensor):
        out = super()._advance(x, tensor)
        if tensor == 0:
            # a cell the advance made alive with other than three living neighbours was
            # no birth of the rule: it spawned
            alive = (x & oracle.ALIVE) != 0
            nb = sum(np.roll(np.roll(alive, dy, 0), dx, 1).astype(np.int32)
                     for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))
            spawned = ~alive & ((out & oracle.ALIVE) != 0) & (nb != 3)
            self.n["spawn_low"] += bool(spawned[:32].any())
            self.n["spawn_high"] += bool(spawned[32:].any())
        return out

    def step(self, action):
        H, W = self.board.shape
        x0, y0 = self.agent_loc
        before, ep0 = self.board.copy(), self.episodes
        out = super().step(action)
        after = self.last_frame[1]                    # the board before any reset
        diff = before != after
        self.n["both_edge_columns"] += bool(diff[:, 0].any() and diff[:, W - 1].any())
        if self.episodes != ep0:                      # reset: the agent is the new level's
            self.n["time_resets"] += bool(out[3]["times_up"]) and not out[3]["game_over"]
            return out
        x1, y1 = self.agent_loc
        self.n["cross_mid"] += {y0, y1} == {31, 32}
        self.n["cross_wrap"] += {y0, y1} == {0, H - 1}
        return out


def _run(case):
    levels = fp.oracle_levels(case.level_dicts())
    stream = fp.SharedStream(np.random.RandomState(case.seed).random_sample(400000))
    envs = fp.oracle_envs(case, levels, cls=SeamTracer, stream=stream)
    for o in envs:
        o.reset()
    acts, us = case.actions()
    for t in range(case.T):
        for e, o in enumerate(envs):
            o.step(fp.case_action(case, o, acts[t, e], us[t, e]))
    return envs


@pytest.mark.parametrize("case", mc.ALL_CASES, ids=mc.CASE_IDS)
def test_mid_case_exercises_the_seams(case):
    H, W = case.shape
    assert 33 <= H <= 64 and 2 <= W <= 64 and (H, W) != (64, 64)
    assert 25 <= case.B <= 27 and case.T == 60 and case.time_limit == 20
    envs = _run(case)
    total = {k: sum(o.n[k] for o in envs) for k in envs[0].n}
    ctx = (case.name, total)
    assert total["time_resets"] >= 1 and total["exit_resets"] >= 1, ctx
    assert total["spawn_low"] >= 1 and total["spawn_high"] >= 1, ctx
    assert total["cross_mid"] >= 1 and total["cross_wrap"] >= 1, ctx
    if W > 2:       # (the tracer counts no seam push on a board two cells wide)
        assert total["push_seam"] + total["pull_seam"] >= 1, ctx
    if W & 1:
        assert total["both_edge_columns"] >= 1, ctx


@pytest.mark.parametrize("shape", mc.SOUP_SHAPES, ids=["%dx%d" % s for s in mc.SOUP_SHAPES])
def test_soups_change_on_every_seam_at_step_one(shape):
    """The dense soups of the fast-against-generic test: the first advance changes a cell
    in each of rows 0, 31, 32, H-1 and columns 0, W-1 of some level."""
    H, W = shape
    rows, cols = set(), set()
    for d in mc.soup_levels(H, W):
        after, _ = oracle.advance(d["board"], d["spawn_prob"],
                                  np.random.RandomState(0).random_sample(2 * H * W))
        diff = after != d["board"]
        rows |= set(np.nonzero(diff.any(1))[0].tolist())
        cols |= set(np.nonzero(diff.any(0))[0].tolist())
    assert {0, 31, 32, H - 1} <= rows, sorted(rows)
    assert {0, W - 1} <= cols, sorted(cols)
