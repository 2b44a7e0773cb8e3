"""The 64x64 plane step with derived planes (sl_env_state.derived_planes 0x8100): plane 15
is rebuilt from plane 2 and plane 8 from the env's exit list, neither is loaded or stored,
and a C3 / C4 batch reads twelve plane words (three DMA groups) where it read sixteen.

Against oracle twins step by step, bit for bit beside a twin whose flag is forced to 0 (all
sixteen words stored) or to half of it, beside the five-wave and the unsplit six-wave
kernels, at batch sizes that leave partial waves and blocks, through hand-built levels on
which the agent walks into an exit, pushes a crate, pulls one and pushes one into an exit
(scripted actions, so each case happens on a known step), after writes from outside that
narrow the flag, with packed and uint8 channel views, on c4, round a capture and without
auto-reset.

c3 pool, time limit 40, 90 steps: every env resets at least twice.  The exit closed, open
and changing colour is test_exit_closed_open_and_recoloured: three hand-built levels on
which can_exit is known from the scores, with scripted actions.
"""
import numpy as np
import pytest

import test_gpu_planes64_split as split
from agent_planes_util import (C3, C4, EXIT, WALL, hand_level, make_venv, pool, twins,
                               with_cell)

pytestmark = pytest.mark.gpu
B, T = 64, 90
SAMPLE = split.SAMPLE
CRATE = 0x8014              # CellTypes.crate: pushable (2), pullable (15), frozen, destructible


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _venv(dev, p, n=B, derived=None, **kw):
    v = make_venv(dev, p, n, **kw)
    if derived is not None:             # (before the first reset: no board is in planes)
        v._state.derived_planes &= derived
    v.reset()
    return v


def _derives(venv, mask=0x8100):
    s = venv._state
    return s.derived_planes == mask and s.agent_planes == 0x62 and s.board_zero == 0x7880


def _lockstep(torch, dev, a, others, p, n, seed, sample=SAMPLE, **kw):
    """a against oracle twins, the others bit for bit beside a."""
    oenvs = twins(a, p, sample, **kw)
    rng = np.random.RandomState(seed)
    n_ended = 0
    for t in range(n):
        acts, ad = split._acts(torch, dev, rng, a.B)
        for v in [a] + others:
            v.step_async(ad)
        boards = t % 3 == 2 or t == n - 1
        for v in others:        # (a board read marks the env's planes_ok: scalars first)
            split._same(torch, a, v, t, False)
        for v in others if boards else ():
            assert torch.equal(a.board, v.board), t
            assert torch.equal(a.goals, v.goals), t
            assert torch.equal(a.start_board, v.start_board), t
        n_ended += split._vs_oracle(a, oenvs, acts, t, boards)
    return n_ended


def test_c3_vs_oracle_and_the_synced_board(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    venv = _venv(dev, p)
    assert _derives(venv) and split._takes_split(venv)
    assert split._run_vs_oracle(torch, dev, venv, p, T, 71) >= 2 * len(SAMPLE)
    assert _derives(venv)
    # the completed uint16 board carries the two planes no step stored
    b = venv.board.cpu().numpy()
    assert ((b & 0x0100) != 0).reshape(B, -1).sum(1).min() >= 1
    assert ((b & 0x8000) != 0).any()
    assert np.array_equal((b >> 15) & 1, (b >> 2) & 1)


@pytest.mark.parametrize("mask", [0, 0x8000, 0x0100])
def test_identical_to_a_twin_that_stores_the_planes(torch_dev, mask):
    torch, dev = torch_dev
    p = pool(C3)
    a, b = _venv(dev, p), _venv(dev, p, derived=mask)
    assert _derives(a) and _derives(b, mask)
    assert _lockstep(torch, dev, a, [b], p, T, 72) >= 2 * len(SAMPLE)


def test_identical_to_the_five_wave_and_the_unsplit_kernel(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    a = _venv(dev, p)
    others = [_venv(dev, p, planes64_waves=w) for w in (5, -6)]
    assert all(_derives(v) for v in [a] + others)
    assert _lockstep(torch, dev, a, others, p, T, 73) >= 2 * len(SAMPLE)


@pytest.mark.parametrize("n", [70, 257, 1])
def test_batch_sizes(torch_dev, n):
    torch, dev = torch_dev
    p = pool(C3)
    a, b = _venv(dev, p, n), _venv(dev, p, n, derived=0)
    sample = sorted({0, min(63, n - 1), min(64, n - 1), n - 1})
    assert _lockstep(torch, dev, a, [b], p, T, 74, sample=sample) >= 2 * len(sample)


def _scripted_pool():
    """One level per case, the agent at (30, 30) facing right; action 2 walks right."""
    from safelife_amd import LevelPool
    cases = [((30, 31, EXIT),),                         # into the exit (closed or open)
             ((30, 31, CRATE),),                        # pushes the crate, four cells
             ((30, 29, CRATE),),                        # pulls it along
             ((30, 31, CRATE), (30, 32, EXIT)),         # pushes it into the exit
             ((30, 31, CRATE), (30, 32, WALL)),         # cannot push it
             ((30, 29, CRATE), (30, 31, CRATE))]        # pushes one, pulls the other
    return LevelPool.from_levels([hand_level(30, 30, c) for c in cases])


@pytest.mark.parametrize("mask", [0x8100, 0])
def test_crate_and_exit_actions(torch_dev, mask):
    torch, dev = torch_dev
    p = _scripted_pool()
    n = p.K
    kw = dict(random_order=False, augment=False)
    venv = _venv(dev, p, n, derived=mask, **kw)
    assert venv._state.derived_planes == mask and venv._state.agent_planes == 0x62
    oenvs = twins(venv, p, list(range(n)), **kw)
    rng = np.random.RandomState(75)
    for t in range(T):
        # right four times, back left twice (pulling what was pushed), then anything; the
        # same again after every reset (time limit 40)
        k = t % 41
        acts = (np.full(n, 2 if k < 4 else 4, np.int32) if k < 6
                else rng.randint(0, 9, size=n).astype(np.int32))
        venv.step_async(torch.from_numpy(acts).to(dev))
        split._vs_oracle(venv, oenvs, acts, t, True)
        if t == 0:
            b = venv.board.cpu().numpy()
            assert b[1, 30, 32] == CRATE and b[1, 30, 31] & 0x02          # pushed
            assert b[2, 30, 30] == CRATE and b[2, 30, 31] & 0x02          # pulled
            assert b[3, 30, 31] & 0x02 and not (b[3] == CRATE).any()      # gone into the exit
            assert b[3, 30, 32] & 0x0100
            assert b[4, 30, 31] == CRATE and b[4, 30, 30] & 0x02          # blocked
            assert b[5, 30, 32] == CRATE and b[5, 30, 30] == CRATE
            assert b[0, 30, 31] & 0x0100                                  # the exit stays


def _exit_pool():
    """Three levels, the agent at (30, 30) facing right, time limit 40, min_performance 0.01:
    0  an empty red goal cell: completed 0 of 1, the exit at (30, 31) is closed;
    1  no goals, no life: completed 0 of 0, the exit at (30, 31) is open;
    2  a red block on red goals, all of the level's score in the baseline: 0 of 0, the exit
       at (30, 33) is open until the agent destroys a cell of the block (-1 of 0: closed)."""
    from safelife_amd import LevelPool
    from agent_planes_util import LIFE, PLAYER
    out = []
    for k, ex in enumerate(((30, 31), (30, 31), (30, 33))):
        lv = hand_level(30, 30)
        b, g = np.zeros((64, 64), np.uint16), np.zeros((64, 64), np.uint16)
        b[30, 30] = PLAYER
        b[ex] = EXIT
        if k == 0:
            g[29, 40] = 0x0200
        if k == 2:
            for y, x in ((28, 31), (28, 32), (29, 31), (29, 32)):
                b[y, x] = LIFE | 0x0200
                g[y, x] = 0x0200
        # a crate and a green block far from the agent's path: with them the pool holds
        # the C3 planes (board_zero 0x7880) and the batch runs the kKeepC3 instances
        b[45, 45] = CRATE
        for y, x in ((50, 10), (50, 11), (51, 10), (51, 11)):
            b[y, x] = LIFE | 0x0400
        lv["board"], lv["goals"] = b, g
        out.append(lv)
    return LevelPool.from_levels(out)


@pytest.mark.parametrize("mask", [0x8100, 0])
def test_exit_closed_open_and_recoloured(torch_dev, mask):
    """The action tests EXIT on a cell whose bit 8 is rebuilt from the list; plane 9 is
    recoloured while plane 8 is not stored; the sync puts bit 8 back."""
    torch, dev = torch_dev
    p = _exit_pool()
    kw = dict(random_order=False, augment=False)
    venv = _venv(dev, p, 3, derived=mask, **kw)
    assert _derives(venv, mask) and venv._state.goals_gray == 0
    b = venv.board.cpu().numpy()
    assert (b[0, 30, 31], b[1, 30, 31], b[2, 30, 33]) == (0x0110, 0x0310, 0x0310)
    oenvs = twins(venv, p, [0, 1, 2], **kw)
    script = [(2, 2, 2), (0, 0, 5), (0, 0, 2), (0, 0, 2)]
    rng = np.random.RandomState(87)
    for t in range(45):
        acts = (np.array(script[t], np.int32) if t < len(script)
                else rng.randint(0, 9, size=3).astype(np.int32))
        venv.step_async(torch.from_numpy(acts).to(dev))
        split._vs_oracle(venv, oenvs, acts, t, True)
        if t >= len(script):
            continue
        b = venv.board.cpu().numpy()
        r, f = venv.reward.cpu().numpy(), venv.flags.cpu().numpy()
        ax = venv.st_t["agent_x"].cpu().numpy()
        if t == 0:
            # closed: the agent stays, no game over, the movement bonus alone, the exit black
            assert ax[0] == 30 and f[0] == 0 and 0 <= r[0] < 0.5 and b[0, 30, 31] == 0x0110
            assert not bool(venv.st_t["game_over"][0].item())
            # open: reward 1 (and the bonus), game over, reset onto the same level, whose
            # exit the reset coloured again
            assert r[1] >= 1.0 and f[1] & 2 and f[1] & 4
            assert ax[1] == 30 and b[1, 30, 31] == 0x0310 and b[1, 30, 30] & 0x02
            assert b[2, 30, 33] == 0x0310 and ax[2] == 31
        if t == 1:      # a cell of the block destroyed: plane 9 of the exit cleared
            assert b[2, 29, 31] == 0 and b[2, 30, 33] == 0x0110
        if t == 3:      # ... and the agent stands before the now closed exit
            assert ax[2] == 32 and f[2] == 0 and b[2, 30, 33] == 0x0110


def test_writes_from_outside_narrow_the_flag(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    rng = np.random.RandomState(76)

    def steps(v, n):
        for _ in range(n):
            v.step_async(split._acts(torch, dev, rng)[1])

    # write_board with a lone bit-2 cell
    venv = _venv(dev, p)
    steps(venv, 7)
    cells = venv.board[3].cpu().numpy().copy()
    ys, xs = np.nonzero(cells == 0)
    cells[ys[0], xs[0]] = 0x0014
    venv.write_board(3, cells)
    assert venv._state.derived_planes == 0 and not _derives(venv)
    assert split._run_vs_oracle(torch, dev, venv, p, 45, 77, sample=[0, 3, 63]) >= 3
    # set_state
    venv = _venv(dev, p)
    steps(venv, 7)
    venv.set_state(venv.board.cpu().numpy(), venv.goals.cpu().numpy(),
                   venv.start_board.cpu().numpy())
    assert venv._state.derived_planes == 0
    assert split._run_vs_oracle(torch, dev, venv, p, 45, 78) >= len(SAMPLE)
    # load_state_dict: the snapshot's own flag, ANDed with the batch's; none without one
    venv = _venv(dev, p)
    steps(venv, 7)
    sd = venv.state_dict()
    assert int(sd["derived_planes"]) == 0x8100
    venv.load_state_dict(dict(sd, derived_planes=torch.tensor(0x0100, dtype=torch.int32)))
    assert venv._state.derived_planes == 0x0100
    assert split._run_vs_oracle(torch, dev, venv, p, 45, 79) >= len(SAMPLE)
    del sd["derived_planes"]
    venv.load_state_dict(sd)
    assert venv._state.derived_planes == 0
    # set_pool to a pool without the property: running envs keep their boards
    venv = _venv(dev, p)
    steps(venv, 7)
    q = with_cell(p, 0x0014)
    venv.set_pool(q)
    assert venv._state.derived_planes == 0x0100 and venv._state.agent_planes == 0x62
    assert split._run_vs_oracle(torch, dev, venv, q, T, 80) >= 2 * len(SAMPLE)
    venv.set_pool(p)                                    # never widened again
    assert venv._state.derived_planes == 0x0100


@pytest.mark.parametrize("channels,dtype", [(None, "uint16"), (tuple(range(15)), "uint8")],
                         ids=["packed", "u8"])
def test_views(torch_dev, channels, dtype):
    torch, dev = torch_dev
    p = pool(C3)
    kw = dict(view=(33, 33), channels=channels, remove_white_goals=False)
    a = _venv(dev, p, compute_obs=True, dtype=dtype, **kw)
    b = _venv(dev, p, derived=0, compute_obs=True, dtype=dtype, **kw)
    assert _derives(a)
    oenvs = twins(a, p, SAMPLE, **kw)
    rng = np.random.RandomState(81)
    n_ended = 0
    for t in range(T):
        acts, ad = split._acts(torch, dev, rng)
        obs = a.step(ad)[0]
        assert torch.equal(obs, b.step(ad)[0]), t
        obs = obs.cpu().numpy()
        n_ended += split._vs_oracle(a, oenvs, acts, t, t % 3 == 2)
        for e, o in oenvs.items():
            assert np.array_equal(obs[e], o.obs()), (t, e)
    assert n_ended >= 2 * len(SAMPLE)


def test_c4(torch_dev):
    torch, dev = torch_dev
    p = pool(C4)
    a, b = _venv(dev, p), _venv(dev, p, derived=0)
    assert _derives(a)
    assert _lockstep(torch, dev, a, [b], p, T, 82) >= 2 * len(SAMPLE)


def test_a_capture_attached_and_closed(torch_dev, tmp_path):
    torch, dev = torch_dev
    from safelife_amd.recorder import TrajectoryRecorder
    p = pool(C3)
    venv = _venv(dev, p)
    rng = np.random.RandomState(83)
    for t in range(5):
        venv.step_async(split._acts(torch, dev, rng)[1])
    rec = TrajectoryRecorder(venv, str(tmp_path / "ep-{env}-{episode_num}"), env_ids=[1, 5],
                             video_recording_freq=1, ring=8)
    assert split._run_vs_oracle(torch, dev, venv, p, 45, 84) >= len(SAMPLE)
    rec.close()
    assert _derives(venv) and split._takes_split(venv)
    assert split._run_vs_oracle(torch, dev, venv, p, 45, 85) >= len(SAMPLE)


def test_without_auto_reset(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    venv = _venv(dev, p, auto_reset=False)
    assert _derives(venv)
    assert split._run_vs_oracle(torch, dev, venv, p, 45, 86, auto_reset=False) == len(SAMPLE)
