"""The split six-wave 64x64 plane step (sl_bits.hip): k_env_planes64_s6 ends each wave after
its plane stores with a 32-byte hand-over record, and k_env_epilogue_reset64 runs the
epilogue one lane per env and resets the finished envs wave by wave.  Taken by a C3 / C4
batch with gray goals, no views, auto-reset from a pool and no capture; every other case
keeps k_env_planes64_w6 (or its neighbours) and k_env_reset_list.

Against the oracle step by step, bit for bit beside the five-wave twin (planes64_waves=5,
epilogue in the wave) and the unsplit six-wave kernel (planes64_waves=-6), at batch sizes
that leave the tail kernel a partial wave and a partial block, with all 64 envs of a wave
finishing on one step and with exactly one, with the episode outputs, through the
fall-backs, and after writes from outside.

c3 pool, time limit 40, 90 steps: every env resets at least twice.  The library exposes
no record of which kernel a step dispatched: _takes_split checks the state the dispatch
reads.
"""
import numpy as np
import pytest

from agent_planes_util import C3, make_venv, pool, twins

import oracle

pytestmark = pytest.mark.gpu
B, T = 64, 90
SAMPLE = [0, 1, 31, 47, 63]
OUTPUTS = ("reward", "done", "flags", "ep_len", "ep_rew")
SCALARS = ("agent_x", "agent_y", "orientation", "old_points", "side_effect", "baseline",
           "episode_length", "episode_reward", "num_steps", "game_over")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _takes_split(venv):
    """The state and settings launch_step_bits sends to the split pair."""
    s = venv._state
    return (s.goals_gray == 1 and s.agent_planes == 0x62 and s.board_zero == 0x7880
            and venv.planes64_waves == 6 and venv.auto_reset and not venv.compute_obs
            and venv._recorder is None)


def _acts(torch, dev, rng, n=B):
    acts = rng.randint(0, 9, size=n).astype(np.int32)
    return acts, torch.from_numpy(acts).to(dev)


def _vs_oracle(venv, oenvs, acts, t, boards, auto_reset=True, ep_out=None):
    """The step just taken by venv, taken by the oracle twins: outputs, scalars, score and
    possible; with `boards` the board, goals and start board.  Without auto-reset a twin
    is dropped when its episode ends (the oracle resets itself).  Returns ended twins."""
    vr, vd, vf = (x.cpu().numpy() for x in (venv.reward, venv.done, venv.flags))
    st = {k: venv.st_t[k].cpu().numpy() for k in SCALARS + ("score", "possible")}
    if boards:
        board, goals, start = (x.cpu().numpy() for x in
                               (venv.board, venv.goals, venv.start_board))
    if ep_out is not None:
        el, er = (x.cpu().numpy() for x in ep_out)
    n_ended = 0
    for e, o in list(oenvs.items()):
        _, r, dn, info = o.step(int(acts[e]))
        c = (t, e)
        ended = bool(info["times_up"] or info["game_over"])
        n_ended += ended
        assert vr[e] == r, (c, vr[e], r)
        assert bool(vd[e]) == (dn if auto_reset else ended), c
        assert bool(vf[e] & 1) == bool(info["times_up"]), c
        assert bool(vf[e] & 2) == bool(info["game_over"]), c
        assert bool(vf[e] & 4) == (auto_reset and ended), c
        if ep_out is not None:
            assert el[e] == (info["episode_length"] if ended else 0), c
            assert er[e] == (info["episode_reward"] if ended else 0), c
        if ended and not auto_reset:
            del oenvs[e]
            continue
        assert (st["agent_x"][e], st["agent_y"][e]) == o.agent_loc, c
        assert st["orientation"][e] == o.orientation, c
        assert st["old_points"][e] == o.old_points, c
        assert st["side_effect"][e] == o.last_side_effect, c
        assert st["baseline"][e] == o.baseline, c
        assert st["episode_length"][e] == o.episode_length, c
        assert st["episode_reward"][e] == int(o.episode_reward), c
        assert st["num_steps"][e] == o.num_steps, c
        assert bool(st["game_over"][e]) == bool(o.game_over), c
        assert (st["score"][e], st["possible"][e]) == oracle.perf_terms(o.board, o.goals), c
        if boards:
            assert np.array_equal(board[e], o.board), c
            assert np.array_equal(goals[e], o.goals), c
            assert np.array_equal(start[e], o.init_board), c
    return n_ended


def _run_vs_oracle(torch, dev, venv, p, n, seed, sample=SAMPLE, auto_reset=True, **kw):
    oenvs = twins(venv, p, sample, **kw)
    rng = np.random.RandomState(seed)
    n_ended = 0
    for t in range(n):
        acts, a = _acts(torch, dev, rng, venv.B)
        venv.step_async(a)
        n_ended += _vs_oracle(venv, oenvs, acts, t, t % 3 == 2 or t == n - 1, auto_reset)
    return n_ended


def _same(torch, a, b, t, boards):
    for k in OUTPUTS:
        assert torch.equal(getattr(a, k), getattr(b, k)), (t, k)
    for k in a.st_t:
        assert torch.equal(a.st_t[k], b.st_t[k]), (t, k)
    assert torch.equal(a.planes_ok, b.planes_ok), t
    if boards:
        assert torch.equal(a.board, b.board), t
        assert torch.equal(a.goals, b.goals), t
        assert torch.equal(a.start_board, b.start_board), t


def test_split_path_vs_oracle(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    venv = make_venv(dev, p, B)
    venv.reset()
    assert _takes_split(venv)
    assert _run_vs_oracle(torch, dev, venv, p, T, 51) >= 2 * len(SAMPLE)
    assert _takes_split(venv)
    # no list on this path: both parities' lengths stay zero
    assert int(venv.scratch[8 * B + 2:8 * B + 4].abs().sum().item()) == 0


def test_identical_to_the_five_wave_twin_and_the_unsplit_kernel(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    a = make_venv(dev, p, B)
    others = [make_venv(dev, p, B, planes64_waves=w) for w in (5, -6)]
    for v in [a] + others:
        v.reset()
    assert _takes_split(a) and not any(_takes_split(v) for v in others)
    rng = np.random.RandomState(52)
    n_reset = torch.zeros(B, dtype=torch.int64, device=dev)
    for t in range(T):
        _, acts = _acts(torch, dev, rng)
        for v in [a] + others:
            v.step_async(acts)
        for v in others:        # (a board read marks the env's planes_ok: scalars first)
            _same(torch, a, v, t, False)
        if t % 3 == 2 or t == T - 1:
            for v in others:
                assert torch.equal(a.board, v.board), t
                assert torch.equal(a.goals, v.goals), t
                assert torch.equal(a.start_board, v.start_board), t
        n_reset += (a.flags & 4) != 0
    assert int(n_reset.min().item()) >= 2


@pytest.mark.parametrize("n", [70, 257, 1])
def test_batch_sizes_partial_wave_and_block(torch_dev, n):
    """70: a full wave and a wave of six lanes; 257: a second block of one lane; 1."""
    torch, dev = torch_dev
    p = pool(C3)
    a, b = make_venv(dev, p, n), make_venv(dev, p, n, planes64_waves=-6)
    a.reset()
    b.reset()
    assert _takes_split(a)
    sample = sorted({0, min(63, n - 1), min(64, n - 1), n - 1})
    oenvs = twins(a, p, sample)
    rng = np.random.RandomState(53)
    n_ended = 0
    for t in range(T):
        acts, ad = _acts(torch, dev, rng, n)
        a.step_async(ad)
        b.step_async(ad)
        boards = t % 3 == 2 or t == T - 1
        _same(torch, a, b, t, boards)
        n_ended += _vs_oracle(a, oenvs, acts, t, boards)
    assert n_ended >= 2 * len(sample)


@pytest.mark.parametrize("early", [None, 37])
def test_simultaneous_resets_in_one_wave(torch_dev, early):
    """Episode clocks unstaggered: all 64 envs of the one wave finish on step 41 (64 resets
    in that wave); with env 37's clock 20 ahead, exactly that lane finishes first."""
    torch, dev = torch_dev
    p = pool(C3)
    a, b = make_venv(dev, p, B), make_venv(dev, p, B, planes64_waves=-6)
    a.reset()
    b.reset()
    if early is not None:
        for v in (a, b):
            v.st_t["episode_length"][early] = 20
    oenvs = twins(a, p, sorted(set(SAMPLE + [37])))
    rng = np.random.RandomState(54)
    counts, first = [], None
    for t in range(T):
        acts, ad = _acts(torch, dev, rng)
        a.step_async(ad)
        b.step_async(ad)
        boards = t % 3 == 2 or t == T - 1
        _same(torch, a, b, t, boards)
        _vs_oracle(a, oenvs, acts, t, boards)
        r = (a.flags & 4) != 0
        counts.append(int(r.sum().item()))
        if first is None and counts[-1]:
            first = r.nonzero().reshape(-1).tolist()
    if early is None:
        assert B in counts, counts
    else:
        assert first == [early] and B - 1 in counts, (first, counts)


def test_episode_outputs_and_counters(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    n = 8
    venv = make_venv(dev, p, n)
    venv.reset()
    assert _takes_split(venv)
    oenvs = twins(venv, p, list(range(n)))
    el = torch.full((n,), -1, dtype=torch.int32, device=dev)
    er = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rng = np.random.RandomState(55)
    for t in range(T):
        acts, ad = _acts(torch, dev, rng, n)
        venv.step_async(ad, ep_len_out=el, ep_rew_out=er)
        _vs_oracle(venv, oenvs, acts, t, t == T - 1, ep_out=(el, er))
    c = venv.sync_counters()
    assert c.episodes_started == sum(o.episodes for o in oenvs.values())
    assert c.episodes_completed == sum(o.completed for o in oenvs.values())
    assert c.episodes_completed >= 2 * n


def test_fallback_without_auto_reset(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    venv = make_venv(dev, p, B, auto_reset=False)
    venv.reset()
    assert not _takes_split(venv)
    assert _run_vs_oracle(torch, dev, venv, p, 45, 56, auto_reset=False) == len(SAMPLE)


def test_fallback_with_a_capture(torch_dev, tmp_path):
    torch, dev = torch_dev
    from safelife_amd.recorder import TrajectoryRecorder
    p = pool(C3)
    venv = make_venv(dev, p, B)
    venv.reset()
    rng = np.random.RandomState(57)
    for t in range(5):                           # split steps, then captured ones
        venv.step_async(_acts(torch, dev, rng)[1])
    rec = TrajectoryRecorder(venv, str(tmp_path / "ep-{env}-{episode_num}"), env_ids=[1, 5],
                             video_recording_freq=1, ring=8)
    assert not _takes_split(venv)
    assert _run_vs_oracle(torch, dev, venv, p, 45, 58) >= len(SAMPLE)
    rec.close()
    assert _takes_split(venv)                    # ... and split steps again
    assert _run_vs_oracle(torch, dev, venv, p, 45, 59) >= len(SAMPLE)


def test_fallback_with_packed_views(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    kw = dict(view=(33, 33), channels=None, remove_white_goals=False)
    venv = make_venv(dev, p, B, compute_obs=True, **kw)
    venv.reset()
    assert not _takes_split(venv)
    oenvs = twins(venv, p, SAMPLE, **kw)
    rng = np.random.RandomState(60)
    n_ended = 0
    for t in range(T):
        acts, ad = _acts(torch, dev, rng)
        obs = venv.step(ad)[0].cpu().numpy()
        n_ended += _vs_oracle(venv, oenvs, acts, t, t % 3 == 2)
        for e, o in oenvs.items():
            assert np.array_equal(obs[e], o.obs()), (t, e)
    assert n_ended >= 2 * len(SAMPLE)


@pytest.mark.parametrize("how", ["set_pool", "load_state_dict"])
def test_reentry_after_a_write_from_outside(torch_dev, how):
    """The step after set_pool / load_state_dict enters the split kernel from the uint16
    board and reads the start board from HBM (start_roll = -1)."""
    torch, dev = torch_dev
    p = pool(C3)
    venv = make_venv(dev, p, B)
    venv.reset()
    rng = np.random.RandomState(61)
    for t in range(7):
        venv.step_async(_acts(torch, dev, rng)[1])
    if how == "set_pool":
        venv.set_pool(pool(C3))
    else:
        venv.load_state_dict(venv.state_dict())
    assert _takes_split(venv)
    assert bool((venv.st_t["start_roll"] == -1).all().item())
    assert _run_vs_oracle(torch, dev, venv, p, T, 62) >= 2 * len(SAMPLE)
    assert _takes_split(venv)
