"""sl_env_step's launch sequence (run_step, csrc/sl_env_step.hip) in every kernel family and
both rng modes: the event pair round the step kernel is recorded -- the generic replay
path included -- and a step split over the replay phases 1 and 2 equals the whole step."""
import ctypes

import pytest
import torch

import step_cases
from safelife_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def events():
    """A fresh pair per test: sl_event_elapsed_ms fails on an event that was never
    recorded, so a sequence that skips ev_begin or ev_end cannot pass on a stale one."""
    L = _lib.lib()
    evs = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in evs:
        assert L.sl_event_create(ctypes.byref(e)) == _lib.SL_OK
    yield evs
    for e in evs:
        L.sl_event_destroy(e)


def timed_step(env, events, actions):
    """One step between the two events; the elapsed time sl_event_elapsed_ms reports."""
    env._cfg.ev_begin, env._cfg.ev_end = events[0].value, events[1].value
    env.step_async(actions)
    env._cfg.ev_begin = env._cfg.ev_end = None
    torch.cuda.synchronize()
    ms = ctypes.c_float(-1.0)
    assert _lib.lib().sl_event_elapsed_ms(events[0], events[1], ctypes.byref(ms)) == _lib.SL_OK
    return ms.value


def actions(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, 9, (step_cases.B,), dtype=torch.int32, device=DEV, generator=g)


@pytest.mark.parametrize("name,H,W,family,rng", step_cases.CASES, ids=step_cases.CASE_IDS)
def test_events_recorded(events, name, H, W, family, rng):
    env = step_cases.make_env(H, W, rng)
    assert env.kernel_family == family
    if rng == "stream":
        assert env._may_spawn       # the step below is a replay step
    ms = timed_step(env, events, actions(H))
    assert ms >= 0.0
    assert not env.stream_error()


def test_events_split_pair(events):
    """64x64 plane mode on C3 planes with gray goals: the six-wave kernel, whose epilogue
    and resets run in a tail kernel after ev_end."""
    env = step_cases.c3_env()
    assert timed_step(env, events, actions(3)) >= 0.0


def test_shard_phases_equal_whole_step(events):
    """40x40 replay: phase 1 (actions, counts, total) then phase 2 from a base of 0 gives
    the boards and rewards of the whole step on a twin env."""
    from safelife_amd import dist as sdist
    whole = step_cases.make_env(40, 40, "stream")
    shard = step_cases.make_env(40, 40, "stream", stream_exchange=sdist.StreamExchange(device=DEV))
    a = actions(40)
    whole.step_async(a)
    assert timed_step(shard, events, a) >= 0.0      # (phase 1 records neither, phase 2 both)
    assert int(whole.stream_pos.item()) > 0         # the step drew
    assert torch.equal(shard.stream_pos, whole.stream_pos)
    assert torch.equal(shard.board, whole.board)
    assert torch.equal(shard.goals, whole.goals)
    assert torch.equal(shard.reward, whole.reward)
    assert torch.equal(shard.done, whole.done)
    assert not whole.stream_error() and not shard.stream_error()
