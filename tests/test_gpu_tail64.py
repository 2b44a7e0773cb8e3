"""The tail of the split six-wave 64x64 plane step (sl_bits.hip k_env_epilogue_reset64) after
it stopped writing the exits' colour into the stale uint16 board and stopped reading the
position ring: the step wave (k_env_planes64_s6) hands the movement-bonus distance over in
the env's hand-over record, and the board's exits are the planes' alone until
k_board_sync64 completes the uint16 board.

Against the oracle step by step with the board read after every step (each read runs
k_board_sync64) over a run in which the exits' colour flips both ways; bit for bit beside
the five-wave twin (planes64_waves=5) and the unsplit six-wave kernel (planes64_waves=-6),
whose epilogue still runs in the step's wave; with bonus periods 1, 4 and
SL_BONUS_PERIOD_MAX under an action script that walks agents across the torus edge, rewards
compared as doubles bit for bit; at batch sizes 1, 70 and 257, with unstaggered episode
clocks and with one clock ahead.

c3 pool, time limit 40, 90 steps, 64 envs unless said: every env resets at least twice.
"""
import numpy as np
import pytest

from agent_planes_util import C3, make_venv, pool, twins
from test_gpu_planes64_split import _acts, _same, _takes_split, _vs_oracle

import oracle

pytestmark = pytest.mark.gpu
B, T = 64, 90
PERIOD_MAX = 16     # SL_BONUS_PERIOD_MAX


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_board_after_every_step_with_the_exit_colour_flipping(torch_dev):
    """The uint16 board completed by k_board_sync64 after every step, against the oracle's:
    the exit cells carry the colour the step wave gave plane 9, and that colour changes both
    ways inside an episode of a compared env (seeded actions; asserted)."""
    torch, dev = torch_dev
    p = pool(C3)
    venv = make_venv(dev, p, B)
    venv.reset()
    assert _takes_split(venv)
    sample = [0, 8, 16, 20, 48, 63]
    oenvs = twins(venv, p, sample)
    rng = np.random.RandomState(71)
    red = oracle.LEVEL_EXIT | oracle.COLOR_R
    prev = {}
    opened = closed = n_ended = 0
    for t in range(T):
        acts, ad = _acts(torch, dev, rng)
        episodes = {e: o.episodes for e, o in oenvs.items()}
        venv.step_async(ad)
        n_ended += _vs_oracle(venv, oenvs, acts, t, True)
        board = venv.board.cpu().numpy()        # (compared with the oracle's just above)
        for e, o in oenvs.items():
            vals = {int(board[e][y, x]) for y, x in o.exits}
            assert len(o.exits) >= 1 and vals <= {red, oracle.LEVEL_EXIT} and len(vals) == 1, (t, e)
            can = vals == {red}
            if o.episodes == episodes[e] and e in prev and prev[e] != can:
                opened += can
                closed += not can
            prev[e] = can
        assert _takes_split(venv)
    assert opened >= 1 and closed >= 1, (opened, closed)
    assert n_ended >= 2 * len(sample)


def _left_acts(torch, dev, rng, n=B):
    """Mostly MOVE LEFT: agents cross the torus edge within an episode."""
    acts = rng.randint(0, 9, size=n)
    acts = np.where(rng.rand(n) < 0.75, 4, acts).astype(np.int32)
    return acts, torch.from_numpy(acts).to(dev)


@pytest.mark.parametrize("period", [1, 4, PERIOD_MAX])
def test_ring_regimes_rewards_bit_for_bit(torch_dev, period):
    """The distance handed over instead of the ring gather: a filling ring (the first
    `period` steps after a reset), a full ring wrapping its head, agents across the torus
    edge (abs(ax - px) > 40, asserted, with a full ring and -- period > 1 -- a filling one);
    rewards against the oracle's and the unsplit kernel's as doubles, bit for bit."""
    torch, dev = torch_dev
    p = pool(C3)
    kw = dict(movement_bonus_period=period)
    a, b = make_venv(dev, p, B, **kw), make_venv(dev, p, B, planes64_waves=-6, **kw)
    a.reset()
    b.reset()
    assert _takes_split(a) and not _takes_split(b)
    sample = [0, 12, 14, 24, 27, 40, 63]
    oenvs = twins(a, p, sample, **kw)
    rng = np.random.RandomState(72)
    far_full = far_filling = n_ended = 0
    for t in range(T):
        acts, ad = _left_acts(torch, dev, rng)
        oldest = {e: (o.prior[0][0], len(o.prior)) for e, o in oenvs.items()}
        a.step_async(ad)
        b.step_async(ad)
        boards = t % 3 == 2 or t == T - 1
        _same(torch, a, b, t, boards)
        assert torch.equal(a.reward.view(torch.int64), b.reward.view(torch.int64)), t
        ax = a.st_t["agent_x"].cpu().numpy()
        episodes = {e: o.episodes for e, o in oenvs.items()}
        # (the oracle twins step inside _vs_oracle; its reward check is ==, the bits here)
        n_ended += _vs_oracle(a, oenvs, acts, t, boards)
        for e, o in oenvs.items():
            px, ln = oldest[e]
            if o.episodes == episodes[e] and abs(int(ax[e]) - px) > 40:
                far_full += ln >= period
                far_filling += ln < period
        st = {k: a.st_t[k].cpu().numpy() for k in ("prior_len", "prior_head", "prior_x", "prior_y")}
        for e, o in oenvs.items():
            ring = [(int(st["prior_x"][e][(st["prior_head"][e] + k) % period]),
                     int(st["prior_y"][e][(st["prior_head"][e] + k) % period]))
                    for k in range(int(st["prior_len"][e]))]
            assert ring == [tuple(q) for q in o.prior], (t, e)
    assert far_full >= 1, far_full
    assert period == 1 or far_filling >= 1, far_filling
    assert n_ended >= 2 * len(sample)


def test_rewards_are_the_oracles_doubles(torch_dev):
    """reward_out against the oracle's float, compared as bit patterns, every env."""
    torch, dev = torch_dev
    p = pool(C3)
    n = 16
    kw = dict(movement_bonus_period=PERIOD_MAX)
    venv = make_venv(dev, p, n, **kw)
    venv.reset()
    assert _takes_split(venv)
    oenvs = twins(venv, p, list(range(n)), **kw)
    rng = np.random.RandomState(73)
    for t in range(T):
        acts, ad = _left_acts(torch, dev, rng, n)
        venv.step_async(ad)
        vr = venv.reward.cpu().numpy()
        for e, o in oenvs.items():
            r = o.step(int(acts[e]))[1]
            assert _bits(vr[e]) == _bits(r), (t, e, vr[e], r)


def test_identical_to_the_twin_kernels(torch_dev):
    """Beside the five-wave twin and the forced unsplit kernel (their epilogue runs in the
    step's wave, exits stored and ring read as before): outputs and scalars each step,
    boards, goals and start boards every third."""
    torch, dev = torch_dev
    p = pool(C3)
    a = make_venv(dev, p, B)
    others = [make_venv(dev, p, B, planes64_waves=w) for w in (5, -6)]
    for v in [a] + others:
        v.reset()
    assert _takes_split(a) and not any(_takes_split(v) for v in others)
    rng = np.random.RandomState(74)
    n_reset = torch.zeros(B, dtype=torch.int64, device=dev)
    for t in range(T):
        _, ad = _left_acts(torch, dev, rng)
        for v in [a] + others:
            v.step_async(ad)
        for v in others:
            _same(torch, a, v, t, False)
            assert torch.equal(a.reward.view(torch.int64), v.reward.view(torch.int64)), t
        if t % 3 == 2 or t == T - 1:
            for v in others:
                assert torch.equal(a.board, v.board), t
                assert torch.equal(a.goals, v.goals), t
                assert torch.equal(a.start_board, v.start_board), t
        n_reset += (a.flags & 4) != 0
    assert int(n_reset.min().item()) >= 2


def _episode_run(torch, dev, p, n, seed, clocks=None):
    """n envs beside the unsplit kernel and oracle twins, with the episode outputs; returns
    the per-step counts of envs reset and the envs of the first step with any."""
    a, b = make_venv(dev, p, n), make_venv(dev, p, n, planes64_waves=-6)
    a.reset()
    b.reset()
    assert _takes_split(a)
    for e, c in (clocks or {}).items():
        for v in (a, b):
            v.st_t["episode_length"][e] = c
    sample = sorted({0, min(37, n - 1), min(63, n - 1), min(64, n - 1), n - 1})
    oenvs = twins(a, p, sample)
    outs = [tuple(torch.full((n,), -1, dtype=torch.int32, device=dev) for _ in range(2))
            for _ in range(2)]
    rng = np.random.RandomState(seed)
    counts, first, n_ended = [], None, 0
    for t in range(T):
        acts, ad = _acts(torch, dev, rng, n)
        for v, (el, er) in zip((a, b), outs):
            v.step_async(ad, ep_len_out=el, ep_rew_out=er)
        boards = t % 3 == 2 or t == T - 1
        _same(torch, a, b, t, boards)
        for x, y in zip(*outs):
            assert torch.equal(x, y), t
        n_ended += _vs_oracle(a, oenvs, acts, t, boards, ep_out=outs[0])
        r = (a.flags & 4) != 0
        counts.append(int(r.sum().item()))
        if first is None and counts[-1]:
            first = r.nonzero().reshape(-1).tolist()
    assert n_ended >= 2 * len(sample)
    ca, cb = a.sync_counters(), b.sync_counters()
    assert ca.episodes_started == cb.episodes_started == n + sum(counts)
    assert ca.episodes_completed == cb.episodes_completed == sum(counts)
    return counts, first


@pytest.mark.parametrize("n", [1, 70, 257])
def test_batch_sizes(torch_dev, n):
    """1; 70: a full wave and one of six lanes; 257: a second block of one lane."""
    torch, dev = torch_dev
    _episode_run(torch, dev, pool(C3), n, 75)


@pytest.mark.parametrize("early", [None, 37])
def test_clocks_unstaggered_and_one_ahead(torch_dev, early):
    """All 64 envs of the one wave finish on one step; with env 37's clock 20 ahead,
    exactly that lane finishes first."""
    torch, dev = torch_dev
    counts, first = _episode_run(torch, dev, pool(C3), B, 76,
                                 clocks=None if early is None else {early: 20})
    if early is None:
        assert B in counts, counts
    else:
        assert first == [early] and B - 1 in counts, (first, counts)
