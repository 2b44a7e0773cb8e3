"""What sl_env_step decides before its first launch (plan_step, csrc/sl_env_step.hip),
read through sl_env_step_plan on host-built structs: no GPU, no launch, and the pointers
are made-up addresses the plan only tests for NULL and alignment."""
import ctypes

import pytest

from safelife_amd import _lib
from safelife_amd._lib import (SL_OK, SL_EINVAL, SL_ETOOBIG, SL_KERNEL_AUTO, SL_KERNEL_GENERIC,
                               SL_KERNEL_FAST, SL_KERNEL_BANDS, SL_KERNEL_MID)

P = 0x7F0000001000          # a 16-byte aligned non-NULL "device" address
KEEP_C3, AGENT_C3 = 0x877F, 0x0062
K_FUSED_CHAN_CELLS = 1096   # sl_obs.h kFusedChanCells


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def state(H, W, B=8, **kw):
    st = _lib.EnvState(B=B, H=H, W=W, board=P, goals=P + 0x100000, start_board=P + 0x200000)
    for k, v in kw.items():
        setattr(st, k, v)
    return st


def planes64_state(**kw):
    """64x64 with the board in half 0 of the goals mirror: C3 planes, gray goals."""
    d = dict(planes=P + 0x300000, board_planes=P + 0x300000, planes_ok=P + 0x400000,
             board_zero=~KEEP_C3 & 0xFFFF, agent_planes=AGENT_C3, goals_gray=1)
    d.update(kw)
    return state(64, 64, **d)


def planes128_state(**kw):
    d = dict(planes=P + 0x300000, board_planes=P + 0x500000, planes_ok=P + 0x400000,
             elig_planes=P + 0x600000)
    d.update(kw)
    return state(128, 128, **d)


def pool(H, W, K=4):
    return _lib.LevelPool(K=K, H=H, W=W, board=P, goals=P)


def cfg(**kw):
    c = _lib.EnvCfg(time_limit=1000, rng_mode=_lib.SL_RNG_PHILOX, kernel=SL_KERNEL_AUTO,
                    scratch=P + 0x700000)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def replay(**kw):
    d = dict(rng_mode=_lib.SL_RNG_STREAM, draws=P, n_draws=64, stream_pos=P + 0x800000)
    d.update(kw)
    return cfg(**d)


def views(mode, vh, vw, out=P + 0x900000, nch=0):
    d = dict(obs_out=out, obs_mode=mode, obs_vh=vh, obs_vw=vw, obs_nch=nch)
    if nch:
        d["obs_channels"] = (ctypes.c_int32 * 16)(*range(nch))
    return d


CAPTURE = _lib.Capture(n=1, env=P, flags=P)


def captured(**kw):
    return dict(capture=ctypes.addressof(CAPTURE), **kw)


def plan(L, st, c, pl=None, flags=P):
    """(return code, sl_step_plan) for this state, cfg, pool and info_flags."""
    out = _lib.StepPlan()
    rc = L.sl_env_step_plan(ctypes.byref(st), ctypes.byref(pl) if pl is not None else None,
                            ctypes.byref(c), flags, ctypes.byref(out))
    return rc, out


def ok(L, st, c, pl=None, flags=P):
    rc, p = plan(L, st, c, pl, flags)
    assert rc == SL_OK
    return p


def test_family_is_sl_env_step_family(L):
    """Every shape up to 130 x 130 and the three step kernel requests: the plan's family is
    sl_env_step_family's answer, its error the plan's; shapes no state may have (a side
    below 2, more than 16 384 cells) are SL_EINVAL before any family is asked."""
    out = _lib.StepPlan()
    c = cfg()
    for kernel in (SL_KERNEL_AUTO, SL_KERNEL_GENERIC, SL_KERNEL_FAST):
        c.kernel = kernel
        for H in range(1, 131):
            for W in range(1, 131):
                st = state(H, W, planes=P, planes_ok=P)
                rc = L.sl_env_step_plan(ctypes.byref(st), None, ctypes.byref(c), None,
                                        ctypes.byref(out))
                fam = L.sl_env_step_family(H, W, kernel)
                if H < 2 or W < 2 or H * W > 16384:
                    assert rc == SL_EINVAL, (H, W, kernel)
                elif fam < 0:
                    assert rc == fam, (H, W, kernel)
                else:
                    assert rc == SL_OK and out.family == fam, (H, W, kernel)


def test_128_without_goals_mirror(L):
    st = state(128, 128)
    assert ok(L, st, cfg()).family == _lib.SL_FAMILY_GENERIC
    assert ok(L, st, cfg(kernel=SL_KERNEL_GENERIC)).family == _lib.SL_FAMILY_GENERIC
    assert plan(L, st, cfg(kernel=SL_KERNEL_FAST))[0] == SL_ETOOBIG
    assert ok(L, planes128_state(), cfg(kernel=SL_KERNEL_FAST)).family == _lib.SL_FAMILY_BITS128


def test_empty_state(L):
    p = ok(L, state(64, 64, B=0), cfg(rng_mode=7))      # (nothing past the pool is validated)
    assert p.empty == 1
    assert ok(L, state(64, 64), cfg()).empty == 0


# ---- 64 x 64: the plane instance ------------------------------------------------------
def plan64(L, waves=0, st=None, pl=True, **kw):
    st = st if st is not None else planes64_state()
    return ok(L, st, cfg(auto_reset=1 if pl else 0, planes64_waves=waves, **kw),
              pool(64, 64) if pl else None)


@pytest.mark.parametrize("waves", [0, 6])
def test_planes64_split_pair(L, waves):
    p = plan64(L, waves)
    assert p.family == _lib.SL_FAMILY_BITS64 and p.plane_mode == 1 and p.demote_first == 0
    assert (p.kernel64, p.keep, p.view_kind) == (_lib.SL_PLAN_K64_S6, _lib.SL_PLAN_KEEP_C3, 0)
    assert p.resets == _lib.SL_PLAN_RESETS_SPLIT_TAIL64 and p.obs == _lib.SL_PLAN_OBS_NONE
    assert p.replay == 0 and p.capture == 0


def test_planes64_unsplit_and_five_waves(L):
    p = plan64(L, _lib.SL_PLANES64_W6_UNSPLIT)
    assert (p.kernel64, p.resets) == (_lib.SL_PLAN_K64_W6, _lib.SL_PLAN_RESETS_LIST64)
    p = plan64(L, 5)
    assert (p.kernel64, p.view_kind, p.resets) == (_lib.SL_PLAN_K64_GRAY, 0,
                                                  _lib.SL_PLAN_RESETS_LIST64)
    # the hand-over records need 16-byte aligned scratch; without auto-reset nothing splits
    p = plan64(L, scratch=P + 0x700008)
    assert (p.kernel64, p.resets) == (_lib.SL_PLAN_K64_W6, _lib.SL_PLAN_RESETS_LIST64)
    p = plan64(L, pl=False)
    assert (p.kernel64, p.resets) == (_lib.SL_PLAN_K64_W6, _lib.SL_PLAN_RESETS_NONE)


def test_planes64_capture_demotes(L):
    p = plan64(L, **captured())
    assert p.capture == 1 and p.plane_mode == 0 and p.demote_first == 1
    assert (p.kernel64, p.keep) == (_lib.SL_PLAN_K64_BITS64, _lib.SL_PLAN_KEEP_RUNTIME)
    assert p.resets == _lib.SL_PLAN_RESETS_LIST64


def test_planes64_keep_classes(L):
    p = plan64(L, st=planes64_state(agent_planes=0x0060))
    assert (p.kernel64, p.keep, p.plane_mode) == (_lib.SL_PLAN_K64_PLANES,
                                                 _lib.SL_PLAN_KEEP_RUNTIME, 1)
    p = plan64(L, st=planes64_state(goals_gray=0))
    assert (p.kernel64, p.keep, p.view_kind) == (_lib.SL_PLAN_K64_PLANES, _lib.SL_PLAN_KEEP_C3, 0)
    assert p.resets == _lib.SL_PLAN_RESETS_LIST64
    p = plan64(L, st=planes64_state(board_zero=0, goals_gray=1))
    assert (p.kernel64, p.keep) == (_lib.SL_PLAN_K64_PLANES, _lib.SL_PLAN_KEEP_ALL)
    p = plan64(L, st=planes64_state(board_zero=0x8000))
    assert (p.kernel64, p.keep) == (_lib.SL_PLAN_K64_PLANES, _lib.SL_PLAN_KEEP_RUNTIME)


def test_bits64_without_planes(L):
    """A 64x64 state without board planes: the uint16 kernel, nothing to demote."""
    p = ok(L, state(64, 64), cfg(auto_reset=1), pool(64, 64))
    assert (p.kernel64, p.plane_mode, p.demote_first) == (_lib.SL_PLAN_K64_BITS64, 0, 0)
    assert p.resets == _lib.SL_PLAN_RESETS_LIST64
    p = ok(L, planes64_state(), cfg(kernel=SL_KERNEL_GENERIC))
    assert (p.family, p.kernel64, p.demote_first) == (_lib.SL_FAMILY_GENERIC, 0, 1)


# ---- 64 x 64: views ---------------------------------------------------------------------
def test_views64_packed_fused(L):
    p = plan64(L, **views(_lib.SL_OBS_PACKED, 33, 33))
    assert p.obs == _lib.SL_PLAN_OBS_FUSED64 and p.plane_mode == 1 and p.view_kind == 1
    assert (p.kernel64, p.resets) == (_lib.SL_PLAN_K64_GRAY, _lib.SL_PLAN_RESETS_LIST64)
    p = plan64(L, st=planes64_state(goals_gray=0), **views(_lib.SL_OBS_PACKED, 33, 33))
    assert (p.kernel64, p.keep, p.view_kind) == (_lib.SL_PLAN_K64_PLANES, _lib.SL_PLAN_KEEP_C3, 1)


def test_views64_channels(L):
    p = plan64(L, **views(_lib.SL_OBS_CHANNELS_U8, 33, 33, nch=15))
    assert (p.obs, p.plane_mode) == (_lib.SL_PLAN_OBS_FUSED64, 1)
    assert (p.kernel64, p.keep, p.view_kind) == (_lib.SL_PLAN_K64_CHAN, _lib.SL_PLAN_KEEP_C3, 3)
    assert plan64(L, **views(_lib.SL_OBS_CHANNELS_F32, 33, 33, nch=2)).view_kind == 4
    for mode in (_lib.SL_OBS_CHANNELS, _lib.SL_OBS_CHANNELS_BF16):
        assert plan64(L, **views(mode, 33, 33, nch=2)).view_kind == 2
    # one cell too many for the step kernel's view masks: 33 x 34 + 2 > kFusedChanCells
    assert 33 * 33 + 2 <= K_FUSED_CHAN_CELLS < 33 * 34 + 2
    for v in (views(_lib.SL_OBS_CHANNELS_U8, 33, 34, nch=15),
              views(_lib.SL_OBS_CHANNELS_U8, 33, 33, out=P + 0x900002, nch=15)):
        p = plan64(L, **v)
        assert (p.obs, p.plane_mode, p.demote_first) == (_lib.SL_PLAN_OBS_SEPARATE, 0, 1)
        assert (p.kernel64, p.view_kind) == (_lib.SL_PLAN_K64_BITS64, 0)


def test_views64_replay(L):
    p = ok(L, planes64_state(), replay(auto_reset=1, **views(_lib.SL_OBS_PACKED, 33, 33)),
           pool(64, 64))
    assert (p.replay, p.plane_mode, p.demote_first) == (1, 0, 1)
    assert (p.obs, p.kernel64, p.view_kind) == (_lib.SL_PLAN_OBS_FUSED64,
                                               _lib.SL_PLAN_K64_BITS64, 1)


# ---- 128 x 128 --------------------------------------------------------------------------
def test_128_views(L):
    pl = pool(128, 128)
    p = ok(L, planes128_state(), cfg(auto_reset=1), pl)
    assert (p.family, p.plane_mode, p.obs) == (_lib.SL_FAMILY_BITS128, 1, _lib.SL_PLAN_OBS_NONE)
    assert (p.resets, p.kernel64) == (_lib.SL_PLAN_RESETS_LIST128, 0)
    p = ok(L, planes128_state(), cfg(auto_reset=1, **views(_lib.SL_OBS_PACKED, 96, 96)), pl)
    assert (p.obs, p.plane_mode, p.demote_first, p.view_kind) == (_lib.SL_PLAN_OBS_FUSED128,
                                                                 1, 0, 1)
    p = ok(L, planes128_state(), cfg(auto_reset=1, **views(_lib.SL_OBS_PACKED, 97, 96)), pl)
    assert (p.obs, p.plane_mode, p.demote_first, p.view_kind) == (_lib.SL_PLAN_OBS_SEPARATE,
                                                                 0, 1, 0)
    p = ok(L, planes128_state(), cfg(auto_reset=1, **views(_lib.SL_OBS_CHANNELS_U8, 9, 9, nch=3)),
           pl)
    assert (p.obs, p.plane_mode) == (_lib.SL_PLAN_OBS_SEPARATE, 0)


def test_128_plane_mode_conditions(L):
    assert ok(L, planes128_state(), replay()).plane_mode == 1
    p = ok(L, planes128_state(elig_planes=None), replay())
    assert (p.plane_mode, p.demote_first) == (0, 1)
    p = ok(L, planes128_state(), cfg(board_mode=_lib.SL_BOARD_UINT16))
    assert (p.plane_mode, p.demote_first) == (0, 1)
    p = ok(L, planes128_state(), cfg(auto_reset=1, **captured()), pool(128, 128))
    assert (p.plane_mode, p.demote_first, p.resets) == (0, 1, _lib.SL_PLAN_RESETS_LIST128)
    # no board planes: nothing to keep, nothing to demote
    p = ok(L, planes128_state(board_planes=None), cfg())
    assert (p.family, p.plane_mode, p.demote_first) == (_lib.SL_FAMILY_BITS128, 0, 0)


# ---- small, mid, generic ------------------------------------------------------------------
@pytest.mark.parametrize("H,W,family", [(9, 9, _lib.SL_FAMILY_SMALL_SEG4),
                                        (20, 40, _lib.SL_FAMILY_SMALL),
                                        (40, 40, _lib.SL_FAMILY_MID)])
def test_small_and_mid_resets(L, H, W, family):
    st = state(H, W)
    p = ok(L, st, cfg(auto_reset=1), pool(H, W))
    assert (p.family, p.resets, p.kernel64) == (family, _lib.SL_PLAN_RESETS_IN_KERNEL, 0)
    p = ok(L, st, cfg(auto_reset=1, **captured()), pool(H, W))
    assert (p.resets, p.capture) == (_lib.SL_PLAN_RESETS_SCAN, 1)
    assert plan(L, st, cfg(auto_reset=1), pool(H + 1, W))[0] == SL_EINVAL
    p = ok(L, st, cfg(), pool(H, W))
    assert p.resets == _lib.SL_PLAN_RESETS_NONE
    p = ok(L, st, cfg(**views(_lib.SL_OBS_PACKED, 5, 5)))
    assert (p.obs, p.view_kind) == (_lib.SL_PLAN_OBS_SEPARATE, 0)


def test_generic_resets(L):
    p = ok(L, state(70, 70), cfg(auto_reset=1), pool(70, 70))
    assert (p.family, p.resets) == (_lib.SL_FAMILY_GENERIC, _lib.SL_PLAN_RESETS_SCAN)
    p = ok(L, state(64, 64), cfg(auto_reset=1, kernel=SL_KERNEL_GENERIC), pool(64, 64))
    assert (p.family, p.resets, p.kernel64) == (_lib.SL_FAMILY_GENERIC,
                                                _lib.SL_PLAN_RESETS_SCAN, 0)


def test_stream_phases(L):
    for phase in (0, 1, 2):
        p = ok(L, state(40, 40), replay(stream_phase=phase, stream_base=P))
        assert (p.replay, p.stream_phase) == (1, phase)


# ---- validation: sl_env_step's codes ------------------------------------------------------
def test_validation_codes(L):
    st = state(40, 40)
    bad = [cfg(bonus_period=-1), cfg(bonus_period=_lib.SL_BONUS_PERIOD_MAX + 1),
           cfg(bonus_period=4),                                   # no table
           cfg(bonus_period=4, bonus_table=P, bonus_len=0),
           cfg(scratch=None),
           cfg(rng_mode=2),
           cfg(stream_phase=1),                                   # a phase without replay
           replay(stream_phase=3), replay(stream_phase=-1),
           replay(stream_phase=2),                                # phase 2 without a base
           replay(stream_pos=None),
           replay(draws=None),                                    # draws promised, none given
           cfg(board_mode=2), cfg(planes64_waves=4), cfg(planes64_waves=-5),
           cfg(kernel=SL_KERNEL_MID), cfg(kernel=SL_KERNEL_BANDS), cfg(kernel=9),
           cfg(**captured()),                                     # a capture without auto-reset
           cfg(**views(_lib.SL_OBS_PACKED, 0, 5)), cfg(**views(9, 5, 5)),
           cfg(**views(_lib.SL_OBS_CHANNELS, 5, 5, nch=0))]
    for c in bad:
        assert plan(L, st, c, pool(40, 40))[0] == SL_EINVAL
    assert plan(L, st, replay(draws=None, n_draws=0))[0] == SL_OK
    # auto-reset: a pool of the state's shape with levels, and info_flags
    assert plan(L, st, cfg(auto_reset=1))[0] == SL_EINVAL
    assert plan(L, st, cfg(auto_reset=1), pool(40, 40, K=0))[0] == SL_EINVAL
    assert plan(L, st, cfg(auto_reset=1), pool(40, 40), flags=None)[0] == SL_EINVAL
    # a capture needs info_flags (without auto-reset nothing else asks for them), its env
    # list and its flags
    assert plan(L, st, cfg(auto_reset=1, **captured()), pool(40, 40))[0] == SL_OK
    assert plan(L, st, cfg(auto_reset=1, **captured()), pool(40, 40), flags=None)[0] == SL_EINVAL
    noenv = _lib.Capture(n=1, flags=P)
    assert plan(L, st, cfg(auto_reset=1, capture=ctypes.addressof(noenv)),
                pool(40, 40))[0] == SL_EINVAL
    none = _lib.Capture(n=0)
    assert ok(L, st, cfg(capture=ctypes.addressof(none))).capture == 0
    # a bad state; no state, cfg or result
    assert plan(L, state(40, 40, board=None), cfg())[0] == SL_EINVAL
    assert plan(L, state(40, 40, B=-1), cfg())[0] == SL_EINVAL
    out = _lib.StepPlan()
    assert L.sl_env_step_plan(None, None, ctypes.byref(cfg()), None, ctypes.byref(out)) == SL_EINVAL
    assert L.sl_env_step_plan(ctypes.byref(st), None, None, None, ctypes.byref(out)) == SL_EINVAL
    assert L.sl_env_step_plan(ctypes.byref(st), None, ctypes.byref(cfg()), None, None) == SL_EINVAL
    # SL_KERNEL_FAST where no bit-sliced kernel takes the shape; the earlier error wins
    assert plan(L, state(70, 70), cfg(kernel=SL_KERNEL_FAST))[0] == SL_ETOOBIG
    assert plan(L, state(70, 70), cfg(kernel=SL_KERNEL_FAST, rng_mode=2))[0] == SL_EINVAL
    assert plan(L, state(70, 70), cfg(kernel=SL_KERNEL_FAST, board_mode=2))[0] == SL_ETOOBIG
