"""sl_env_cfg.obs_fuse / SL_OBS_FUSE_CHAN128 in the plan of a step (plan_step,
csrc/sl_env_step.hip), read through sl_env_step_plan on host-built structs as
test_step_plan_cpu.py does: with the bit set a 128x128 plane state keeps the board in planes
over a step with channel views (SL_PLAN_OBS_FUSED128, view_kind 2-4) inside the writer's
limits; outside them, with the bit clear and for every other family the plan is what it is
without the field."""
import ctypes

import pytest

from safelife_amd import _lib
from safelife_amd._lib import SL_OK

P = 0x7F0000001000          # a 16-byte aligned non-NULL "device" address
KEEP_C3, AGENT_C3 = 0x877F, 0x0062
FUSE = _lib.SL_OBS_FUSE_CHAN128
CHANNEL_MODES = [(_lib.SL_OBS_CHANNELS, 2), (_lib.SL_OBS_CHANNELS_U8, 3),
                 (_lib.SL_OBS_CHANNELS_F32, 4), (_lib.SL_OBS_CHANNELS_BF16, 2)]
PLAN_FIELDS = [n for n, _ in _lib.StepPlan._fields_]


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
    c = _lib.EnvCfg(time_limit=1000, rng_mode=_lib.SL_RNG_PHILOX, kernel=_lib.SL_KERNEL_AUTO,
                    scratch=P + 0x700000, auto_reset=1)
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


def ok(L, st, c, pl):
    out = _lib.StepPlan()
    rc = L.sl_env_step_plan(ctypes.byref(st), ctypes.byref(pl), ctypes.byref(c), P,
                            ctypes.byref(out))
    assert rc == SL_OK
    return out


def fields(p):
    return tuple(getattr(p, n) for n in PLAN_FIELDS)


def separate(p):
    return ((p.obs, p.plane_mode, p.demote_first, p.view_kind)
            == (_lib.SL_PLAN_OBS_SEPARATE, 0, 1, 0))


def test_constants_and_field():
    assert FUSE == 1
    assert _lib.SL_FUSE_CHAN128_MAX_CELLS >= 33 * 33      # the benchmark's view fits
    assert _lib.EnvCfg._fields_[-1][0] == "obs_fuse"
    assert _lib.EnvCfg().obs_fuse == 0


@pytest.mark.parametrize("mode,kind", CHANNEL_MODES)
def test_channel_modes_fuse(L, mode, kind):
    pl = pool(128, 128)
    for vh, vw, nch in ((33, 33, 15), (15, 15, 15), (9, 9, 3), (1, 1, 1), (96, 11, 15),
                        (5, 128, 16)):
        p = ok(L, planes128_state(), cfg(obs_fuse=FUSE, **views(mode, vh, vw, nch=nch)), pl)
        assert p.family == _lib.SL_FAMILY_BITS128
        assert (p.obs, p.plane_mode, p.demote_first) == (_lib.SL_PLAN_OBS_FUSED128, 1, 0)
        assert p.view_kind == kind
        assert (p.resets, p.kernel64) == (_lib.SL_PLAN_RESETS_LIST128, 0)
        # bit clear: today's plan
        assert separate(ok(L, planes128_state(), cfg(**views(mode, vh, vw, nch=nch)), pl))


def test_replay_needs_draw_planes(L):
    pl = pool(128, 128)
    v = views(_lib.SL_OBS_CHANNELS, 33, 33, nch=15)
    p = ok(L, planes128_state(), replay(obs_fuse=FUSE, **v), pl)
    assert (p.replay, p.obs, p.plane_mode, p.demote_first, p.view_kind) == (
        1, _lib.SL_PLAN_OBS_FUSED128, 1, 0, 2)
    p = ok(L, planes128_state(elig_planes=None), replay(obs_fuse=FUSE, **v), pl)
    assert p.replay == 1 and separate(p)


def test_outside_the_limits_is_separate(L):
    pl = pool(128, 128)
    U8 = _lib.SL_OBS_CHANNELS_U8
    limit = _lib.SL_FUSE_CHAN128_MAX_CELLS
    assert 96 * 42 <= limit < 96 * 43 and 43 <= 128
    cases = [
        (planes128_state(), cfg(obs_fuse=FUSE, **views(U8, 97, 11, nch=3))),          # rows
        (planes128_state(), cfg(obs_fuse=FUSE, **views(U8, 9, 9, out=P + 0x900002, nch=3))),
        (planes128_state(), cfg(obs_fuse=FUSE, **views(U8, 9, 9, out=P + 0x900008, nch=3))),
        (planes128_state(), cfg(obs_fuse=FUSE, **views(U8, 96, 43, nch=3))),          # cells
        (planes128_state(), cfg(obs_fuse=FUSE, **views(U8, 5, 129, nch=3))),          # columns
        (planes128_state(), cfg(obs_fuse=FUSE, board_mode=_lib.SL_BOARD_UINT16,
                                **views(U8, 9, 9, nch=3))),
    ]
    for st, c in cases:
        assert separate(ok(L, st, c, pl))
    # the cell limit itself still fuses
    p = ok(L, planes128_state(), cfg(obs_fuse=FUSE, **views(U8, 96, 42, nch=3)), pl)
    assert (p.obs, p.plane_mode) == (_lib.SL_PLAN_OBS_FUSED128, 1)
    # no board planes: nothing to keep and nothing to demote, the views are separate
    p = ok(L, planes128_state(board_planes=None),
           cfg(obs_fuse=FUSE, **views(U8, 9, 9, nch=3)), pl)
    assert (p.family, p.obs, p.plane_mode, p.demote_first, p.view_kind) == (
        _lib.SL_FAMILY_BITS128, _lib.SL_PLAN_OBS_SEPARATE, 0, 0, 0)
    # a capture takes the board out of planes, as it does with packed views
    cap = _lib.Capture(n=1, env=P, flags=P)
    p = ok(L, planes128_state(),
           cfg(obs_fuse=FUSE, capture=ctypes.addressof(cap), **views(U8, 9, 9, nch=3)), pl)
    assert separate(p)


def test_bit_clear_is_todays_plan(L):
    """The very case of test_step_plan_cpu.py::test_128_views."""
    p = ok(L, planes128_state(), cfg(**views(_lib.SL_OBS_CHANNELS_U8, 9, 9, nch=3)),
           pool(128, 128))
    assert (p.obs, p.plane_mode) == (_lib.SL_PLAN_OBS_SEPARATE, 0)
    assert separate(p)


def test_packed_views_unchanged_by_the_bit(L):
    pl = pool(128, 128)
    for vh, vw in ((33, 33), (96, 96), (97, 96), (96, 128)):
        for mk in (cfg, replay):
            a = ok(L, planes128_state(), mk(**views(_lib.SL_OBS_PACKED, vh, vw)), pl)
            b = ok(L, planes128_state(), mk(obs_fuse=FUSE, **views(_lib.SL_OBS_PACKED, vh, vw)),
                   pl)
            assert fields(a) == fields(b)
    p = ok(L, planes128_state(), cfg(obs_fuse=FUSE, **views(_lib.SL_OBS_PACKED, 96, 96)), pl)
    assert (p.obs, p.plane_mode, p.demote_first, p.view_kind) == (_lib.SL_PLAN_OBS_FUSED128,
                                                                 1, 0, 1)
    # no views at all
    a, b = ok(L, planes128_state(), cfg(), pl), ok(L, planes128_state(), cfg(obs_fuse=FUSE), pl)
    assert fields(a) == fields(b) and a.obs == _lib.SL_PLAN_OBS_NONE


def test_other_families_ignore_the_bit(L):
    modes = [m for m, _ in CHANNEL_MODES] + [_lib.SL_OBS_PACKED]
    for mode in modes:
        nch = 0 if mode == _lib.SL_OBS_PACKED else 15
        for vh, vw in ((33, 33), (33, 34), (9, 9)):
            v = views(mode, vh, vw, nch=nch)
            a = ok(L, planes64_state(), cfg(**v), pool(64, 64))
            b = ok(L, planes64_state(), cfg(obs_fuse=FUSE, **v), pool(64, 64))
            assert fields(a) == fields(b)
        for H, W in ((9, 9), (20, 40), (40, 40), (70, 70)):
            v = views(mode, 5, 5, nch=nch)
            a = ok(L, state(H, W), cfg(**v), pool(H, W))
            b = ok(L, state(H, W), cfg(obs_fuse=FUSE, **v), pool(H, W))
            assert fields(a) == fields(b) and b.obs == _lib.SL_PLAN_OBS_SEPARATE
    p = ok(L, planes64_state(), cfg(obs_fuse=FUSE, **views(_lib.SL_OBS_CHANNELS_U8, 33, 33,
                                                          nch=15)), pool(64, 64))
    assert (p.obs, p.kernel64, p.view_kind) == (_lib.SL_PLAN_OBS_FUSED64, _lib.SL_PLAN_K64_CHAN, 3)
    # a 128x128 state on the generic kernel
    p = ok(L, planes128_state(), cfg(obs_fuse=FUSE, kernel=_lib.SL_KERNEL_GENERIC,
                                     **views(_lib.SL_OBS_CHANNELS_U8, 9, 9, nch=3)),
           pool(128, 128))
    assert (p.family, p.obs, p.plane_mode) == (_lib.SL_FAMILY_GENERIC,
                                               _lib.SL_PLAN_OBS_SEPARATE, 0)
