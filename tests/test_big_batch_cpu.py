"""(CPU) The cases of tests/big_batch_cases.py do what they claim: by arithmetic alone every
case's batch crosses the boundaries it names and its envs of interest are distinct envs of
the batch; every step case's shape gets the kernel family and the plan it names
(sl_env_step_family, sl_env_step_plan on host-built structs); and, on the oracle, with the
global env ids, seeds, clocks and actions tests/test_gpu_big_batch.py uses, every compared
env resets at least twice within T and the envs of a pool with spawners draw.

Conditions, not measurements: a case that stops meeting one no longer tests its feature.
"""
import numpy as np
import pytest

import oracle
import feature_pools as fp
import obs_cases as oc
import big_batch_cases as bb

IDS_OBS = [c.name for c in bb.OBS_CASES]
IDS_STEP = [c.name for c in bb.STEP_CASES]


@pytest.fixture(scope="module")
def L():
    from safelife_amd import _lib
    _lib.build()
    return _lib.lib()


def _check_arithmetic(case):
    for X, ids in case.interest().items():
        assert (case.B - 1) * case.env_bytes >= X, (case, X)
        assert len(set(ids)) == len(ids) == 4 and all(0 <= e < case.B for e in ids), (case, X)
        below, at, nxt, last = ids
        assert (below + 1) * case.env_bytes <= X, (case, X)            # wholly below
        assert at * case.env_bytes <= X < (at + 1) * case.env_bytes    # holds X, or starts at it
        assert nxt == at + 1 and nxt * case.env_bytes > X and last == case.B - 1


# --------------------------------------------------------------- stand-alone observations
def test_the_obs_cases_are_the_issues():
    assert {c.name: c.env_bytes for c in bb.OBS_CASES} == bb.OBS_ENV_BYTES
    assert {c.name: c.small.kernel for c in bb.OBS_CASES} == bb.OBS_KERNELS
    by = {c.name: c for c in bb.OBS_CASES}
    assert oc.WAVE_MAX_CELLS == 4096 and bb.MAXV == 64
    for c in bb.OBS_CASES:
        assert c.small.shape in ((5, 9), (2, 2)) and c.small.shape in oc.BOARDS
        assert c.small.B == bb.PERIOD == 7 and c.small.nv <= oc.WAVE_MAX_CELLS
        want = (bb.P31, bb.P32, bb.P33) if c.name == "chan-f32" else (bb.P31, bb.P32)
        assert c.boundaries == want
    assert by["bench-f32"].small.view == (33, 33) and by["bench-f32"].small.nch == 15
    assert by["fallback-f32"].small.channels == by["fallback-u8"].small.channels == (3, 0, 9, 14)
    assert by["fallback-f32"].small.out_shift == 4 and by["fallback-u8"].small.out_shift == 1
    # the f32 case's elements no longer count in an int
    assert by["chan-f32"].numel > 1 << 31


@pytest.mark.parametrize("case", bb.OBS_CASES, ids=IDS_OBS)
def test_obs_case_crosses_its_boundaries(case):
    _check_arithmetic(case)
    assert case.B == max(case.boundaries) // case.env_bytes + bb.EXTRA
    assert case.footprint() <= bb.FOOTPRINT_CAP
    # every exit style occurs among the PERIOD states, so in every group of the batch
    assert {oc.STYLES[(case.small.seed + b) % len(oc.STYLES)] for b in range(bb.PERIOD)} \
        == set(oc.STYLES)
    # bench-f32: the 16-byte head of an env's bytes differs from env to env
    if case.name == "bench-f32":
        heads = {case.small.env_parts(b)[0] for es in case.interest().values() for b in es}
        assert len(heads) > 1


# ------------------------------------------------------------------------- step families
def test_the_step_cases_are_the_issues(L):
    env_bytes = {c.name: c.env_bytes for c in bb.STEP_CASES}
    H, W = bb.seg4_largest()
    assert (H, W) == (32, 32)
    assert env_bytes == dict(bb.STEP_ENV_BYTES, **{"seg4": H * W * 2, "seg4-tail": H * W * 2})
    by = {c.name: c for c in bb.STEP_CASES}
    assert by["bits128"].boundaries == (bb.P31, bb.P32)
    assert by["planes64-chan-f32"].boundaries == (bb.P31, bb.P32)
    assert by["planes64-chan-f32"].B == 65740
    assert all(c.boundaries == (bb.P31,) for c in bb.STEP_CASES
               if c.name not in ("bits128", "planes64-chan-f32"))
    assert by["seg4"].B % 4 == 0 and by["seg4-tail"].B % 4 == 1
    assert [c.name for c in bb.STEP_CASES if c.rng == "stream"] == ["bits128-replay"]
    for c in bb.STEP_CASES:
        assert 8 <= c.T <= 16
        if c.tensor == "views":
            # the boards stay below the views' last boundary (packed views are smaller than
            # a 64x64 board: there the boards cross 2^31 and 2^32 as well)
            assert c.compute_obs
            assert (c.B * c.shape[0] * c.shape[1] * 2 < max(c.boundaries)) \
                == (c.name != "planes64-packed")


@pytest.mark.parametrize("case", bb.STEP_CASES, ids=IDS_STEP)
def test_step_case_crosses_its_boundaries(case):
    _check_arithmetic(case)
    assert case.B % case.group == case.ragged
    assert case.footprint() <= bb.FOOTPRINT_CAP
    for lo in case.twins():
        assert 0 <= lo and lo + bb.TWIN <= case.B
    if case.twins():
        covered = {e for lo in case.twins() for e in range(lo, lo + bb.TWIN)}
        assert set(case.anchors()) <= covered and case.twins()[-1] + bb.TWIN == case.B
        assert len(case.twins()) == len(case.boundaries)


@pytest.mark.parametrize("case", bb.STEP_CASES, ids=IDS_STEP)
def test_step_case_gets_its_family_and_plan(L, case):
    from safelife_amd import _lib
    kernel = {"generic": _lib.SL_KERNEL_GENERIC, "fast": _lib.SL_KERNEL_FAST,
              "wide": _lib.SL_KERNEL_WIDE}[case.kernel]
    H, W = case.shape
    assert _lib.env_step_family(H, W, kernel) == case.family
    facts = bb.plan_facts(bb.host_plan(case))
    assert {k: facts[k] for k in case.plan} == case.plan, (case, facts)
    assert facts["replay"] == int(case.rng == "stream")


@pytest.mark.parametrize("case", bb.STEP_CASES, ids=IDS_STEP)
def test_step_case_resets_twice_and_draws(case):
    levels = fp.oracle_levels(case.level_dicts())
    spawners = any(((lv.board | lv.goals) & oracle.SPAWNING).any() for lv in levels)
    assert spawners == (case.pool not in ("c3", "c4c3"))
    stream = fp.SharedStream(np.random.RandomState(1).random_sample(1 << 22))
    envs = {e: case.oracle_env(levels, e, stream=stream, cls=fp.TracingOracleEnv)
            for e in case.anchors()}
    assert len(envs) == 3 * len(case.boundaries) + 1        # (B - 1 is every boundary's)
    for e, o in envs.items():
        o.reset()
        o.episode_length = int(case.clock(e))
    draws = 0
    for t in range(case.T):
        acts = case.actions(t)
        for e, o in envs.items():
            draws += oracle.count_eligible(o.board) + oracle.count_eligible(o.goals)
            o.step(int(acts[e]))
    for e, o in envs.items():
        assert o.n["resets"] >= 2, (case, e, o.n)
    if spawners:
        assert draws >= 1, case
