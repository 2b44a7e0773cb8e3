"""The 64x64 plane kernel (k_env_step_bits64_planes without views, sl_bits.hip) against
the oracle directly, once per instantiation: the C3 pool (kept planes 0x877F, fixed at
compile time), the C3 levels with spawners, blue life and movable blocks (the mask at
run time) and a pool whose boards together hold every cell bit (all 16 planes).

Short episodes (time_limit 13) over 40 steps cover resets, the step into plane mode
after each of them (the uint16 board transposed on entry), goals off their fixed
point and the exits' recolouring.  The board and the goals are read after every step:
under board_mode="planes" a read completes the uint16 board and the next step is a
plane step again.  Boards, goals and dones bit for bit, rewards with ``==``.
"""
import os

import numpy as np
import pytest

import oracle

POOLS = os.path.join(os.path.dirname(__file__), "golden", "pools")
C3 = os.path.join(POOLS, "c3_prune_still_64.npz")
pytestmark = pytest.mark.gpu

B, T, SEED = 96, 40, 29
SAMPLE = [0, 1, 63, 64, 95]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _spawner_pool():
    """The C3 levels with spawners, blue cells and pushable / pullable blocks sprinkled in
    (planes 2, 7, 11, 15 come and go; the zero-plane mask must follow)."""
    from safelife_amd import LevelPool
    p = LevelPool.load(C3)
    rng = np.random.RandomState(4)
    b = p.board.copy()
    for k in range(p.K):
        ay, ax = p.agent_y[k], p.agent_x[k]
        free = (b[k] == 0)
        free[max(ay - 3, 0):ay + 4, max(ax - 3, 0):ax + 4] = False
        ys, xs = np.nonzero(free)
        pick = rng.choice(len(ys), size=min(40, len(ys)), replace=False)
        for n, i in enumerate(pick):
            kind = n % 4
            b[k, ys[i], xs[i]] = (152 | (3 << 9) if kind == 0 else      # spawner, blue-ish
                                  1 | 8 | (4 << 9) if kind == 1 else    # alive blue life
                                  4 if kind == 2 else 0x8000 | 16)      # pushable / pullable
    return LevelPool(b, p.goals, np.stack([p.agent_x, p.agent_y], 1), p.orientation,
                     p.spawn_prob, p.min_performance)


def _all_bits_pool():
    """The spawner pool with the cell bits no cell type uses (12-14) set on its walls:
    every plane is kept."""
    p = _spawner_pool()
    walls = (p.board & 0x10) != 0
    p.board[walls] |= np.uint16(0x7000)
    return p


def _c3_pool():
    from safelife_amd import LevelPool
    return LevelPool.load(C3)


def _levels(pool):
    return [oracle.Level(pool.board[k], pool.goals[k], (pool.agent_x[k], pool.agent_y[k]),
                         pool.orientation[k], pool.spawn_prob[k], pool.min_performance[k])
            for k in range(pool.K)]


def _env_state(venv, e):
    s = {"board": venv.board[e].cpu().numpy(), "goals": venv.goals[e].cpu().numpy(),
         "start_board": venv.start_board[e].cpu().numpy()}
    for k, t in venv.st_t.items():
        s[k] = t[e].cpu().numpy()
    return s


@pytest.mark.parametrize("name,make,zero", [("c3", _c3_pool, 0x7880),
                                            ("spawners", _spawner_pool, 0x7000),
                                            ("all_bits", _all_bits_pool, 0x0000)])
def test_plane_kernel64_vs_oracle(torch_dev, name, make, zero):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv
    pool = make()
    levels = _levels(pool)
    kw = dict(time_limit=13, view_shape=(33, 33), output_channels=None, penalty_coef=1.0,
              min_performance=0.01)
    venv = SafeLifeVecEnv(pool, B, dev, board_mode="planes", rng="philox", seed=SEED,
                          kernel="fast", compute_obs=False, level_order="random",
                          augment_roll=True, **kw)
    venv.reset()
    assert venv.board_planes is not None
    # the instantiation: the kept planes fixed at compile time, at run time, all of them
    assert venv._state.board_zero == zero, hex(venv._state.board_zero)
    oenvs = {}
    for e in SAMPLE:
        o = oracle.OracleEnv(oracle.pool_level_fn(levels, e, seed=SEED, random_order=True,
                                                  augment=True),
                             env_id=e, rng="philox", seed=SEED, **kw)
        o.load_state(_env_state(venv, e), venv._step_index)
        oenvs[e] = o
    rng = np.random.RandomState(12)
    n_done = 0
    vd = None
    n_plane_steps = 0
    for t in range(T):
        if t > 0:
            # the reads below left the planes in place: the next step is a plane step again
            # for every env but those the last step reset (a reset writes the uint16 board;
            # such an env enters plane mode anew).  All episodes start together, so the
            # time limit resets the whole batch at once every 13th step: on every other
            # step more than half of the batch is in planes.
            inp = ((venv.planes_ok & 64) != 0).cpu().numpy()
            kept = ~vd.astype(bool)
            assert inp[kept].all(), (t, int(inp.sum()), int(kept.sum()))
            if kept.sum() > B // 2:
                assert inp.sum() > B // 2, (t, int(inp.sum()))
                n_plane_steps += 1
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step_async(torch.from_numpy(acts).to(dev))
        vr, vd = venv.reward.cpu().numpy(), venv.done.cpu().numpy()
        board, goals = venv.board.cpu().numpy(), venv.goals.cpu().numpy()
        for e in SAMPLE:
            _, r, dn, _ = oenvs[e].step(int(acts[e]))
            ctx = (name, t, e)
            assert vr[e] == r, (ctx, vr[e], r)
            assert bool(vd[e]) == dn, ctx
            assert np.array_equal(board[e], oenvs[e].board), ctx
            assert np.array_equal(goals[e], oenvs[e].goals), ctx
            n_done += int(dn)
    assert n_done >= 2 * len(SAMPLE)         # every sampled env went through resets
    assert n_plane_steps >= T - 1 - T // 13  # all but the steps after the time limit's resets
    assert venv._state.board_zero == zero    # the mask (the instantiation) held throughout
