"""The six-wave 64x64 plane kernel (k_env_planes64_w6, sl_bits.hip: C3 / C4 planes, gray
goals, no views; a 6 KiB buffer) against the oracle step by step, beside its five-wave
twin (SafeLifeVecEnv(planes64_waves=5): k_env_planes64_gray<0x877F, 0>), and the batches
that must not take it.

c3 with random rolls and a time limit of 40 over 90 steps: every env resets at least twice,
and the step after each reset enters plane mode from the uint16 board -- in this kernel
in two passes of 32 rows through the 4 KiB the buffer has for it.  A start board the
kernel reads from HBM (start_roll = -1) is staged the same way; of the writes from
outside, load_state_dict and set_pool leave the batch on this kernel (they keep
agent_planes and goals_gray), set_state and write_board take it to the run-time-mask
kernel (agent_planes = 0) -- both kinds are stepped against the oracle here.

The library exposes no record of which kernel a step dispatched: the dispatch cases
check the state the dispatch reads (goals_gray, agent_planes, board_zero) and the
results.
"""
import numpy as np
import pytest

from agent_planes_util import C3, C4, check_step, make_venv, pool, twins

import oracle

pytestmark = pytest.mark.gpu
B, T = 64, 90
SAMPLE = [0, 1, 31, 47, 63]
POK_BOARD_PLANES = 64
OUTPUTS = ("reward", "done", "flags")


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _takes_w6(venv):
    """The state launch_step_bits sends to k_env_planes64_w6 (no views, Philox)."""
    s = venv._state
    return (s.goals_gray == 1 and s.agent_planes == 0x62 and s.board_zero == 0x7880
            and venv.planes64_waves == 6)


def _check_scores(venv, oenvs, ctx):
    score, possible = (venv.st_t[k].cpu().numpy() for k in ("score", "possible"))
    for e, o in oenvs.items():
        assert (score[e], possible[e]) == oracle.perf_terms(o.board, o.goals), (ctx, e)


def _acts(torch, dev, rng):
    acts = rng.randint(0, 9, size=B).astype(np.int32)
    return acts, torch.from_numpy(acts).to(dev)


def _steps_vs_oracle(torch, dev, venv, p, n, seed, **kw):
    """n steps of venv beside oracle twins of SAMPLE continuing from its state."""
    oenvs = twins(venv, p, SAMPLE, **kw)
    rng = np.random.RandomState(seed)
    n_done = n_planes = 0
    for t in range(n):
        acts, a = _acts(torch, dev, rng)
        venv.step_async(a)
        n_planes += int(((venv.planes_ok & POK_BOARD_PLANES) != 0).sum().item())
        n_done += check_step(venv, oenvs, acts, t)
        _check_scores(venv, oenvs, t)
    return n_done, n_planes


def test_c3_steps_vs_oracle(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    venv = make_venv(dev, p, B)
    venv.reset()
    assert _takes_w6(venv)
    n_done, n_planes = _steps_vs_oracle(torch, dev, venv, p, T, 41)
    assert n_done >= 2 * len(SAMPLE)          # (time limit 40: two resets each at least)
    assert n_planes > B * T * 3 // 4          # most envs hold SL_POK_BOARD_PLANES
    assert _takes_w6(venv)


def test_identical_to_the_five_wave_twin(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    a, b = make_venv(dev, p, B), make_venv(dev, p, B, planes64_waves=5)
    a.reset()
    b.reset()
    assert _takes_w6(a) and not _takes_w6(b)
    rng = np.random.RandomState(42)
    n_reset = torch.zeros(B, dtype=torch.int64, device=dev)
    for t in range(T):
        _, acts = _acts(torch, dev, rng)
        a.step_async(acts)
        b.step_async(acts)
        for k in OUTPUTS:
            assert torch.equal(getattr(a, k), getattr(b, k)), (t, k)
        for k in a.st_t:
            assert torch.equal(a.st_t[k], b.st_t[k]), (t, k)
        assert torch.equal(a.planes_ok, b.planes_ok), t
        n_reset += (a.flags & 4) != 0
        if t % 3 == 2 or t == T - 1:       # (the steps between run with no sync at all)
            assert torch.equal(a.board, b.board), t
            assert torch.equal(a.goals, b.goals), t
            assert torch.equal(a.start_board, b.start_board), t
    assert int(n_reset.min().item()) >= 2


@pytest.mark.parametrize("how", ["load_state_dict", "set_pool", "set_state", "write_board"])
def test_caller_written_start_boards_vs_oracle(torch_dev, how):
    torch, dev = torch_dev
    p = pool(C3)
    venv = make_venv(dev, p, B)
    venv.reset()
    rng = np.random.RandomState(43)
    for t in range(7):
        venv.step_async(_acts(torch, dev, rng)[1])
    if how == "load_state_dict":       # every env: uint16 entry and start board from HBM
        venv.load_state_dict(venv.state_dict())
    elif how == "set_pool":            # running episodes: start boards from HBM
        venv.set_pool(pool(C3))
    elif how == "set_state":
        st = {k: v.cpu().numpy() for k, v in venv.st_t.items()}
        venv.set_state(venv.board.cpu().numpy(), venv.goals.cpu().numpy(),
                       venv.start_board.cpu().numpy(), **st)
    else:
        venv.write_board(5, venv.board[5].clone())
    on_w6 = how in ("load_state_dict", "set_pool")
    assert _takes_w6(venv) == on_w6
    if how != "write_board":
        assert bool((venv.st_t["start_roll"] == -1).all().item())
    n_done, _ = _steps_vs_oracle(torch, dev, venv, p, T, 44)
    assert n_done >= 2 * len(SAMPLE)
    assert _takes_w6(venv) == on_w6


def test_step_into_plane_mode_after_uint16_steps(torch_dev):
    """board_mode="auto": a caller's read makes the next steps uint16-mode steps (planes
    demoted); the plane step after them enters from the uint16 board, every env at once.
    Beside a batch that never leaves uint16 mode."""
    torch, dev = torch_dev
    p = pool(C3)
    a = make_venv(dev, p, B, board_mode="auto")
    b = make_venv(dev, p, B, board_mode="uint16")
    a.reset()
    b.reset()
    assert _takes_w6(a)
    rng = np.random.RandomState(45)
    in_planes = []
    for t in range(24):
        _, acts = _acts(torch, dev, rng)
        a.step_async(acts)
        b.step_async(acts)
        for k in OUTPUTS:
            assert torch.equal(getattr(a, k), getattr(b, k)), (t, k)
        in_planes.append(int(((a.planes_ok & POK_BOARD_PLANES) != 0).sum().item()))
        if t in (5, 15):
            assert torch.equal(a.board, b.board), t          # a caller's read
    # plane steps, uint16 steps after each read, and plane steps again after those
    assert in_planes[5] > B // 2 and in_planes[7] == 0, in_planes
    assert in_planes[14] > B // 2 and in_planes[17] == 0 and in_planes[23] > B // 2, in_planes
    assert torch.equal(a.board, b.board) and torch.equal(a.goals, b.goals)
    for k in a.st_t:
        if k != "start_roll":
            assert torch.equal(a.st_t[k], b.st_t[k]), k


def _one_red_goal(p):
    from safelife_amd import LevelPool
    g = p.goals.copy()
    g[p.K // 2, 17, 5] = 0x0200
    return LevelPool(p.board, g, np.stack([p.agent_x, p.agent_y], 1), p.orientation,
                     p.spawn_prob, p.min_performance)


@pytest.mark.parametrize("which", ["c4", "c3-one-red"])
def test_coloured_goals_do_not_take_it(torch_dev, which):
    torch, dev = torch_dev
    p = pool(C4) if which == "c4" else _one_red_goal(pool(C3))
    venv = make_venv(dev, p, B)
    venv.reset()
    assert venv._state.goals_gray == 0 and not _takes_w6(venv)
    n_done, n_planes = _steps_vs_oracle(torch, dev, venv, p, T, 46)
    assert n_done >= len(SAMPLE)
    assert n_planes > B * T * 3 // 4
    assert venv._state.goals_gray == 0


def test_packed_views_keep_the_gray_view_kernel(torch_dev):
    """With packed views the dispatch stays at k_env_planes64_gray<0x877F, 1>: views and
    results against the oracle, with the six-wave default and with the switch at five."""
    torch, dev = torch_dev
    p = pool(C3)
    kw = dict(view=(33, 33), channels=None, remove_white_goals=False)
    a = make_venv(dev, p, B, compute_obs=True, **kw)
    b = make_venv(dev, p, B, compute_obs=True, planes64_waves=5, **kw)
    obs = a.reset().cpu().numpy()
    b.reset()
    oenvs = twins(a, p, SAMPLE, **kw)
    for e in SAMPLE:
        assert np.array_equal(obs[e], oenvs[e].obs()), e
    rng = np.random.RandomState(47)
    n_done = 0
    for t in range(T):
        acts, ad = _acts(torch, dev, rng)
        obs, _, _, _ = a.step(ad)
        obs2, _, _, _ = b.step(ad)
        assert torch.equal(obs, obs2), t
        assert torch.equal(a.reward, b.reward), t
        n_done += check_step(a, oenvs, acts, t, obs=obs.cpu().numpy())
    assert n_done >= len(SAMPLE)
