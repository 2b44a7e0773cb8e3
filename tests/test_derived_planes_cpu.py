"""The premise of sl_env_state.derived_planes, from the oracle alone (CPU), the host
function that declares it, how writes from outside narrow it, and the step plan's public
record of it.

Premise: on the still-life pools cell bit 15 equals cell bit 2 in every cell (only a crate
carries either), and the cells with the exit bit (8) are exactly the env's exit list, after
every step and every reset -- so the 64x64 plane kernels may rebuild those two planes from
plane 2 and from the list instead of loading and storing them.  Checked on the oracle's PPO
chain (random rolls, random level order, uniform random actions, a short time limit so
episodes end by the limit and by exits).
"""
import ctypes

import numpy as np
import pytest

import oracle
from agent_planes_util import C3, C4, CRATE, EXIT, hand_level, levels_of, pool

B, T, LIMIT = 6, 130, 40
P = 0x7F0000001000          # a 16-byte aligned non-NULL "device" address


@pytest.mark.parametrize("path", [C3, C4], ids=["c3", "c4"])
def test_oracle_keeps_the_derived_planes(path):
    levels = levels_of(pool(path))
    cb = oracle.CpuBatch(levels, B, time_limit=LIMIT, view_shape=(15, 15), penalty_coef=1.0,
                         min_performance=0.01, seed=7, level_order="random",
                         augment_roll=True)
    cb.reset()
    rng = np.random.RandomState(3)

    def check(ctx):
        for e in range(B):
            b, s0 = cb.board(e), cb.board(e, 2)
            c = (ctx, e)
            assert np.array_equal((b >> 2) & 1, (b >> 15) & 1), c
            # the exit list is the start board's exits in np.nonzero order (the reset)
            assert np.array_equal((b & 0x100) != 0, (s0 & 0x100) != 0), c
            n = int(((b & 0x100) != 0).sum())
            assert n == cb.scalars(e)["exit_count"] and 1 <= n <= 8, c
            # bit 15 rebuilt from bit 2, bit 8 from the list: the same board, cell for cell
            # (and so the same scores: nothing further to compare)
            r = (b & ~np.uint16(0x8100)) | ((b & 4) << 13) | (s0 & 0x100)
            assert np.array_equal(r, b), c

    check("reset")
    for t in range(T):
        cb.step(rng.randint(0, 9, size=B).astype(np.int32))
        check(t)
    assert sum(cb.scalars(e)["episodes"] for e in range(B)) >= B * (T // (LIMIT + 1))


# ---- the host mask ------------------------------------------------------------------------
def _pool_of(levels):
    from safelife_amd import LevelPool
    return LevelPool.from_levels(levels)


def _mask(p, **kw):
    from safelife_amd.vec_env import derived_planes
    return derived_planes(p.board, **kw)


def test_host_mask_on_the_reference_pools():
    assert _mask(pool(C3)) == 0x8100
    assert _mask(pool(C4)) == 0x8100
    # a power toggle can give the agent bit 2 without bit 15
    assert _mask(pool(C3), can_toggle_powers=True) == 0x0100


def test_host_mask_on_hand_built_pools():
    plain = [hand_level(0, 0), hand_level(31, 63, ((30, 30, CRATE | 0x8000),))]
    assert _mask(_pool_of(plain)) == 0x8100
    # a bit-2 cell that lacks bit 15, and the converse, in one level of three
    assert _mask(_pool_of(plain + [hand_level(5, 5, ((30, 30, CRATE),))])) == 0x0100
    assert _mask(_pool_of(plain + [hand_level(5, 5, ((30, 30, 0x8010),))])) == 0x0100
    # eight exits fill the list (hand_level has one at (50, 50)); nine do not fit it
    eight = tuple((2, 2 * k, EXIT) for k in range(7))
    assert _mask(_pool_of(plain + [hand_level(5, 5, eight)])) == 0x8100
    # (a LevelPool refuses such a level; the mask is asked of the boards themselves)
    from safelife_amd.vec_env import derived_planes
    nine = np.stack([lv["board"] for lv in plain + [hand_level(5, 5, eight + ((4, 4, EXIT),))]])
    assert derived_planes(nine) == 0x8000
    assert _mask(_pool_of(plain), can_toggle_powers=True) == 0x0100
    # an exit the rule or the action could change: not frozen, pushable, pullable,
    # destructible
    for bad in (0x0100, EXIT | 0x0004, EXIT | 0x8000, EXIT | 0x0008):
        lv = hand_level(5, 5)
        lv["board"][50, 50] = bad
        flag = 0x8000 if (bad >> 2) & 1 == (bad >> 15) & 1 else 0
        assert _mask(_pool_of(plain + [lv])) == flag, hex(bad)


# ---- set, narrowed, cleared: the flag on a batch without a device ------------------------------
class _Batch:
    """The flag's owner, SafeLifeVecEnv's own methods, on a bare sl_env_state: the sync
    and the planes_ok write they make first are counted, not run."""

    def __init__(self, derived, ctp=False):
        from safelife_amd import _lib
        from safelife_amd.vec_env import SafeLifeVecEnv as V
        self._state = _lib.EnvState(derived_planes=derived, planes_live=1)
        self.can_toggle_powers = ctp
        self.demotions = 0
        self._derived_planes = V._derived_planes.__get__(self)
        self._narrow_derived_planes = V._narrow_derived_planes.__get__(self)

    def sync_board(self):
        self.demotions += 1

    def _pok_clear(self, bits):
        from safelife_amd import _lib
        assert bits == _lib.SL_POK_BOARD


def test_flag_is_narrowed_never_widened():
    c3 = pool(C3)
    lone = _pool_of([hand_level(5, 5, ((30, 30, CRATE),))])
    nine = hand_level(5, 5, tuple((2, 2 * k, EXIT) for k in range(8)))["board"][None]
    v = _Batch(0x8100)
    assert v._derived_planes(c3) == 0x8100
    v._narrow_derived_planes(v._derived_planes(c3))         # the same property: nothing moves
    assert (v._state.derived_planes, v.demotions, v._state.planes_live) == (0x8100, 0, 1)
    v._narrow_derived_planes(v._derived_planes(lone))       # boards leave the planes first
    assert (v._state.derived_planes, v.demotions, v._state.planes_live) == (0x0100, 1, 0)
    v._narrow_derived_planes(v._derived_planes(c3))         # ... and the bit never returns
    assert (v._state.derived_planes, v.demotions) == (0x0100, 1)
    from safelife_amd.vec_env import derived_planes
    v._narrow_derived_planes(derived_planes(nine))
    assert (v._state.derived_planes, v.demotions) == (0, 2)
    v = _Batch(0x8100)
    v._narrow_derived_planes()                              # a board written from outside
    assert (v._state.derived_planes, v.demotions) == (0, 1)
    assert _Batch(0x8100, ctp=True)._derived_planes(c3) == 0x0100


# ---- the step plan ------------------------------------------------------------------------------
def _plan(**kw):
    from safelife_amd import _lib
    _lib.build()
    L = _lib.lib()
    d = dict(planes=P + 0x300000, board_planes=P + 0x300000, planes_ok=P + 0x400000,
             board_zero=0x7880, agent_planes=0x0062, goals_gray=1, derived_planes=0x8100)
    d.update(kw)
    st = _lib.EnvState(B=8, H=64, W=64, board=P, goals=P + 0x100000, start_board=P + 0x200000,
                       **d)
    c = _lib.EnvCfg(time_limit=1000, rng_mode=_lib.SL_RNG_PHILOX, kernel=_lib.SL_KERNEL_AUTO,
                    scratch=P + 0x700000, auto_reset=1)
    pl = _lib.LevelPool(K=4, H=64, W=64, board=P, goals=P)
    out = _lib.StepPlan()
    assert L.sl_env_step_plan(ctypes.byref(st), ctypes.byref(pl), ctypes.byref(c), P,
                              ctypes.byref(out)) == _lib.SL_OK
    return out


def test_plan_names_the_stored_and_derived_planes():
    """Six stored planes -- twelve words, three DMA groups -- only with all three masks."""
    from safelife_amd import _lib
    p = _plan()
    assert (p.kernel64, p.keep) == (_lib.SL_PLAN_K64_S6, _lib.SL_PLAN_KEEP_C3)
    assert (p.stored, p.derived) == (0x061D, 0x8100)
    # the flag is read at run time: a batch without it, or with half of it, keeps its
    # kernel and stores both planes
    for flag, derived, stored in ((0, 0, 0x871D), (0x8000, 0, 0x871D), (0x0100, 0, 0x871D)):
        p = _plan(derived_planes=flag)
        assert (p.kernel64, p.keep) == (_lib.SL_PLAN_K64_S6, _lib.SL_PLAN_KEEP_C3)
        assert (p.stored, p.derived) == (stored, derived)
    # bits outside 0x8100 are ignored; so is a plane no board holds
    assert (_plan(derived_planes=0xFFFF).stored, _plan(derived_planes=0xFFFF).derived) == (
        0x061D, 0x8100)
    p = _plan(board_zero=0x7880 | 0x8000)
    assert (p.keep, p.stored, p.derived) == (_lib.SL_PLAN_KEEP_RUNTIME, 0x061D, 0x0100)
    # other agent planes, other kept planes: the run-time class, the flag still honoured
    p = _plan(agent_planes=0x0060)
    assert (p.keep, p.stored, p.derived) == (_lib.SL_PLAN_KEEP_RUNTIME, 0x061F, 0x8100)
    p = _plan(board_zero=0)
    assert (p.keep, p.stored, p.derived) == (_lib.SL_PLAN_KEEP_ALL, 0x7E9D, 0x8100)
    # not in plane mode: nothing is stored in planes, nothing derived
    p = _plan(board_planes=None)
    assert (p.plane_mode, p.stored, p.derived) == (0, 0, 0)
