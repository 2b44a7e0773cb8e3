"""Channel views written by the 64x64 plane kernel (k_env_planes64_chan, sl_bits.hip): a
step with output_channels=(...) keeps the board in bit planes and writes the views from
them, where it used to demote every board to uint16 first.

Setup of test_gpu_planes64_oracle.py (B=96, T=40, seed 29, time_limit 13, its three
pools: the C3 planes fixed at compile time, the run-time mask, all 16 planes), with a
4x4 white goal patch near every level's agent start so that remove_white_goals and the
goal colours' add into planes 12-15 show in every view of an episode's first steps.

1. parity with the oracle per instantiation (keep mask x element size), the view also
   against the stand-alone view kernel (observe()) for the whole batch;
2. the feature: after a channel-view step the boards are still in planes (planes_ok bit
   6, no sync: bit 7 clear) -- fails on a build that demotes for channel views;
3. views the step kernel cannot fuse (40x40, an unaligned output) demote as before;
4. view-less, packed-view and channel-view steps mixed, against a uint16-mode twin.
"""
import os

import numpy as np
import pytest

import oracle

POOLS = os.path.join(os.path.dirname(__file__), "golden", "pools")
C3 = os.path.join(POOLS, "c3_prune_still_64.npz")

B, T, SEED, TL = 96, 40, 29, 13
SAMPLE = [0, 1, 63, 64, 95]
WHITE_GOAL = 0x0E00 | 0x10
BOARD_STEPS = (9, 19, 29, T - 1)       # where the board is read: most steps run without


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _with_goal_patch(p):
    """The pool with a 4x4 white goal patch at (+3, +3) from each level's agent start
    (wrapped): inside every view of at least 15x15 at each episode start, whatever the
    roll."""
    from safelife_amd import LevelPool
    g = p.goals.copy()
    for k in range(p.K):
        ys = (int(p.agent_y[k]) + 3 + np.arange(4)) % p.H
        xs = (int(p.agent_x[k]) + 3 + np.arange(4)) % p.W
        g[k][ys[:, None], xs[None, :]] = WHITE_GOAL
    return LevelPool(p.board, g, np.stack([p.agent_x, p.agent_y], 1), p.orientation,
                     p.spawn_prob, p.min_performance)


def _spawner_pool_plain():
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


def _spawner_pool():
    return _with_goal_patch(_spawner_pool_plain())


def _all_bits_pool():
    """The spawner pool with the cell bits no cell type uses (12-14) set on its walls:
    every plane is kept."""
    p = _spawner_pool_plain()
    walls = (p.board & 0x10) != 0
    p.board[walls] |= np.uint16(0x7000)
    return _with_goal_patch(p)


def _c3_pool():
    from safelife_amd import LevelPool
    return _with_goal_patch(LevelPool.load(C3))


MAKE = {"c3": (_c3_pool, 0x7880), "spawners": (_spawner_pool, 0x7000),
        "all_bits": (_all_bits_pool, 0x0000)}


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


def _kw(view, channels, remove_white):
    return dict(time_limit=TL, view_shape=view, output_channels=channels,
                remove_white_goals=remove_white, penalty_coef=1.0, min_performance=0.01)


def _venv(dev, pool, view, channels, dtype, remove_white, board_mode="planes",
          compute_obs=True, seed=SEED):
    from safelife_amd import SafeLifeVecEnv
    return SafeLifeVecEnv(pool, B, dev, board_mode=board_mode, rng="philox", seed=seed,
                          kernel="fast", compute_obs=compute_obs, level_order="random",
                          augment_roll=True, obs_dtype=dtype,
                          **_kw(view, channels, remove_white))


def _oracle_env(levels, e, view, channels, remove_white):
    return oracle.OracleEnv(oracle.pool_level_fn(levels, e, seed=SEED, random_order=True,
                                                 augment=True),
                            env_id=e, rng="philox", seed=SEED,
                            **_kw(view, channels, remove_white))


def _bytes(torch, t):
    return t.contiguous().view(torch.uint8)


def _nonzero(torch, t):
    """Host 0/1 array of a view tensor of any element type (bf16 by its bits)."""
    if t.dtype == torch.bfloat16:
        t = t.view(torch.uint16)
    return (t.cpu().numpy() != 0).astype(np.uint16)


@pytest.mark.parametrize("name", ["c3", "spawners", "all_bits"])
def test_oracle_alone_every_sampled_env_resets_twice(name):
    """(CPU) With the goal patches in place and the exact parameters of the GPU cases, the
    oracle alone takes every sampled env through resets: n_done >= 2 per env."""
    levels = _levels(MAKE[name][0]())
    rng = np.random.RandomState(12)
    acts = [rng.randint(0, 9, size=B).astype(np.int32) for _ in range(T)]
    n_done = 0
    for e in SAMPLE:
        o = _oracle_env(levels, e, (33, 33), tuple(range(15)), True)
        o.reset()
        for t in range(T):
            n_done += int(o.step(int(acts[t][e]))[2])
    assert n_done >= 2 * len(SAMPLE), n_done


CASES = [
    ("c3", (33, 33), tuple(range(15)), "uint16", False),
    ("c3", (33, 33), tuple(range(15)), "uint8", True),
    ("spawners", (15, 15), tuple(range(15)), "bfloat16", False),
    ("spawners", (33, 33), (0, 3, 5, 9, 10, 11), "uint16", True),
    ("all_bits", (33, 33), tuple(range(16)), "float32", False),
    ("all_bits", (7, 64), (1, 4, 2, 12, 13, 14, 15, 0), "uint8", False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,view,channels,dtype,remove_white", CASES,
                         ids=["%s-%dx%d-%dch-%s" % (c[0], c[1][0], c[1][1], len(c[2]), c[3])
                              for c in CASES])
def test_plane_channel_views_vs_oracle(torch_dev, name, view, channels, dtype, remove_white):
    torch, dev = torch_dev
    make, zero = MAKE[name]
    pool = make()
    levels = _levels(pool)
    venv = _venv(dev, pool, view, channels, dtype, remove_white)
    obs = venv.reset()
    assert venv.board_planes is not None
    assert venv._state.board_zero == zero, hex(venv._state.board_zero)
    oenvs = {}
    for e in SAMPLE:
        o = _oracle_env(levels, e, view, channels, remove_white)
        o.load_state(_env_state(venv, e), venv._step_index)
        oenvs[e] = o
    got = _nonzero(torch, obs)
    for e in SAMPLE:
        assert np.array_equal(got[e], oenvs[e].obs()), (name, "reset", e)
    ref = torch.zeros_like(venv.obs)
    rng = np.random.RandomState(12)
    n_done = 0
    for t in range(T):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        obs, vr, vd, _ = venv.step(torch.from_numpy(acts).to(dev))
        # the fused view equals the stand-alone view kernel's, every env, every byte
        venv.observe(out=ref)
        assert torch.equal(_bytes(torch, obs), _bytes(torch, ref)), (name, t)
        got = _nonzero(torch, obs)
        vr, vd = vr.cpu().numpy(), vd.cpu().numpy()
        read = t in BOARD_STEPS
        if read:
            board, goals = venv.board.cpu().numpy(), venv.goals.cpu().numpy()
        for e in SAMPLE:
            o, r, dn, _ = oenvs[e].step(int(acts[e]))
            ctx = (name, t, e)
            assert vr[e] == r, (ctx, vr[e], r)
            assert bool(vd[e]) == dn, ctx
            assert np.array_equal(got[e], o), ctx
            if read:
                assert np.array_equal(board[e], oenvs[e].board), ctx
                assert np.array_equal(goals[e], oenvs[e].goals), ctx
            n_done += int(dn)
    assert n_done >= 2 * len(SAMPLE)         # every sampled env went through resets
    assert venv._state.board_zero == zero    # the mask (the instantiation) held throughout


def _run_and_check_planes(torch, dev, venv, steps, expect_planes):
    """`steps` channel-view steps into a caller's buffer; after each, planes_ok of the envs
    the step did not reset.  Returns the number of steps on which more than half of the
    batch was not reset."""
    venv.reset()
    out = torch.zeros_like(venv.obs)
    rng = np.random.RandomState(12)
    n_most = 0
    for t in range(steps):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step_async(torch.from_numpy(acts).to(dev), obs_out=out)
        pok = venv.planes_ok.cpu().numpy()
        kept = (venv.flags.cpu().numpy() & 4) == 0          # not reset by this step
        if expect_planes:
            assert ((pok[kept] & 64) != 0).all(), (t, int(((pok & 64) != 0).sum()), int(kept.sum()))
            if kept.sum() > B // 2:
                # they held planes before the step, and no sync ran
                assert ((pok[kept] & 128) == 0).all(), t
                n_most += 1
        else:
            assert ((pok & 64) == 0).all(), t
    return n_most


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["uint16", "uint8", "bfloat16", "float32"])
def test_channel_view_steps_stay_in_planes(torch_dev, dtype):
    torch, dev = torch_dev
    venv = _venv(dev, _c3_pool(), (33, 33), tuple(range(15)), dtype, True, compute_obs=False)
    n_most = _run_and_check_planes(torch, dev, venv, 20, True)
    assert n_most >= 20 - 1 - 20 // TL


@pytest.mark.gpu
def test_channel_view_steps_stay_in_planes_auto_mode(torch_dev):
    """The default board_mode with no board read: the same."""
    torch, dev = torch_dev
    venv = _venv(dev, _c3_pool(), (33, 33), tuple(range(15)), "uint16", True,
                 board_mode="auto", compute_obs=False)
    assert _run_and_check_planes(torch, dev, venv, 20, True) >= 20 - 1 - 20 // TL


@pytest.mark.gpu
def test_uint16_board_mode_keeps_out_of_planes(torch_dev):
    """Control: board_mode="uint16" never enters plane mode."""
    torch, dev = torch_dev
    venv = _venv(dev, _c3_pool(), (33, 33), tuple(range(15)), "uint16", True,
                 board_mode="uint16", compute_obs=False)
    _run_and_check_planes(torch, dev, venv, 20, False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["view40", "unaligned"])
def test_unfusable_channel_views_demote_as_before(torch_dev, kind):
    """A 40x40 channel view (more cells than the kernel's mask array) and an output that is
    not 16-byte aligned: the uint16 path, views equal to observe(), no board in planes."""
    torch, dev = torch_dev
    view = (40, 40) if kind == "view40" else (33, 33)
    venv = _venv(dev, _spawner_pool(), view, tuple(range(15)), "uint8", True, compute_obs=False)
    venv.reset()
    n = venv.obs.numel()
    big = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    at = 16 if kind == "view40" else 1            # an odd element offset of a larger buffer
    out = big[at:at + n].view(venv.obs.shape)
    assert (out.data_ptr() % 16 != 0) == (kind == "unaligned")
    ref = torch.zeros_like(venv.obs)
    rng = np.random.RandomState(12)
    for t in range(12):
        acts = torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev)
        if t % 4 != 3:                            # plane steps in between: boards in planes
            venv.step_async(acts)
            assert int(((venv.planes_ok & 64) != 0).sum().item()) > 0, t
            continue
        venv.step_async(acts, obs_out=out)
        assert int(((venv.planes_ok & 64) != 0).sum().item()) == 0, t
        venv.observe(out=ref)
        assert torch.equal(out, ref), t
        assert not big[:at].any() and not big[at + n:].any(), t     # nothing beside the view


def _packed_step(venv, acts, out):
    """One step of `venv` writing packed views (output_channels=None) into `out`."""
    from safelife_amd import _lib
    saved = (venv.obs_mode, venv.output_channels, venv.obs)
    venv.obs_mode, venv.output_channels, venv.obs = _lib.SL_OBS_PACKED, None, out
    try:
        venv.step_async(acts, obs_out=out)
    finally:
        venv.obs_mode, venv.output_channels, venv.obs = saved


def _same_state(a, b, ctx):
    assert np.array_equal(a.board.cpu().numpy(), b.board.cpu().numpy()), ctx
    assert np.array_equal(a.goals.cpu().numpy(), b.goals.cpu().numpy()), ctx
    for k in a.st_t:
        assert np.array_equal(a.st_t[k].cpu().numpy(), b.st_t[k].cpu().numpy()), (ctx, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", [("spawners", "uint16"), ("c3", "uint8")])
def test_mixed_view_steps_match_uint16_mode(torch_dev, name, dtype):
    """View-less, packed-view and channel-view steps in turn: the plane-mode batch never
    leaves the planes and equals a board_mode="uint16" twin, outputs every step, state at
    the end.  (The packed steps borrow the view settings of a second env built with
    output_channels=None.)"""
    torch, dev = torch_dev
    pool = MAKE[name][0]()
    args = ((33, 33), tuple(range(15)), dtype, True)
    a = _venv(dev, pool, *args, board_mode="planes", compute_obs=False, seed=31)
    b = _venv(dev, pool, *args, board_mode="uint16", compute_obs=False, seed=31)
    p = _venv(dev, pool, (33, 33), None, "uint16", True, board_mode="uint16",
              compute_obs=False, seed=31)
    a.reset()
    b.reset()
    ch_a, ch_b = torch.zeros_like(a.obs), torch.zeros_like(b.obs)
    pk_a, pk_b = torch.zeros_like(p.obs), torch.zeros_like(p.obs)
    rng = np.random.RandomState(6)
    for t in range(30):
        acts = torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev)
        if t % 3 == 0:
            a.step_async(acts)
            b.step_async(acts)
        elif t % 3 == 1:
            _packed_step(a, acts, pk_a)
            _packed_step(b, acts, pk_b)
            assert torch.equal(pk_a, pk_b), t
        else:
            a.step_async(acts, obs_out=ch_a)
            b.step_async(acts, obs_out=ch_b)
            assert torch.equal(_bytes(torch, ch_a), _bytes(torch, ch_b)), t
        for x, y in ((a.reward, b.reward), (a.done, b.done), (a.flags, b.flags),
                     (a.ep_len, b.ep_len), (a.ep_rew, b.ep_rew)):
            assert torch.equal(x, y), t
        kept = (a.flags.cpu().numpy() & 4) == 0
        assert ((a.planes_ok.cpu().numpy()[kept] & 64) != 0).all(), t
        assert int(((b.planes_ok & 64) != 0).sum().item()) == 0, t
    _same_state(a, b, "end")
