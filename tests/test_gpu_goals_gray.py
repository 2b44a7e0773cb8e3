"""The 64x64 plane kernel for gray goals (k_env_planes64_gray; sl_env_state.goals_gray: every
goal cell black or white, so the scores read no goal colour and the packed views one
plane of three) against the oracle, step by step, and the batches that must not take it.

c3 with random rolls and a time limit of 40 (resets, and the step after each, whose
goals are not yet at their fixed point, many times over).  That the colour loads are
really gone is shown by overwriting the mirror's colour words of envs whose goals are at
their fixed point with random bits: a kernel that read them would score and reward from
them (rows 1-6 of the point table), this one stays bit-exact.
"""
import numpy as np
import pytest

from agent_planes_util import C3, C4, check_step, make_venv, pool, twins

import oracle

pytestmark = pytest.mark.gpu
B, T = 64, 90
SAMPLE = [0, 1, 31, 47, 63]
POK_MIRROR_FIXED = 2 | 4          # SL_POK_GOALS_MIRROR | SL_POK_GOALS_FIXED
POK_BOARD_PLANES = 64
COLOUR_WORDS = [9, 10, 11, 25, 26, 27]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _mixed(a, b):
    from safelife_amd import LevelPool
    cat = lambda k: np.concatenate([getattr(a, k), getattr(b, k)])
    return LevelPool(cat("board"), cat("goals"),
                     np.stack([cat("agent_x"), cat("agent_y")], 1), cat("orientation"),
                     cat("spawn_prob"), cat("min_performance"))


def _one_red_goal(p):
    from safelife_amd import LevelPool
    g = p.goals.copy()
    g[p.K // 2, 17, 5] = 0x0200
    return LevelPool(p.board, g, np.stack([p.agent_x, p.agent_y], 1), p.orientation,
                     p.spawn_prob, p.min_performance)


def _check_scores(venv, oenvs, ctx):
    score, possible = (venv.st_t[k].cpu().numpy() for k in ("score", "possible"))
    for e, o in oenvs.items():
        assert (score[e], possible[e]) == oracle.perf_terms(o.board, o.goals), (ctx, e)


def _run(torch, dev, p, gray, **kw):
    venv = make_venv(dev, p, B, **kw)
    venv.reset()
    assert venv._state.goals_gray == gray
    assert venv._state.agent_planes == 0x62 and venv._state.board_zero == 0x7880
    oenvs = twins(venv, p, SAMPLE, **kw)
    rng = np.random.RandomState(31)
    n_done = n_planes = 0
    for t in range(T):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step_async(torch.from_numpy(acts).to(dev))
        n_planes += int(((venv.planes_ok & POK_BOARD_PLANES) != 0).sum().item())
        n_done += check_step(venv, oenvs, acts, t)
        _check_scores(venv, oenvs, t)
        assert venv._state.goals_gray == gray, t
    assert n_done >= len(SAMPLE)
    assert n_planes > B * T * 3 // 4          # most envs hold SL_POK_BOARD_PLANES
    return venv


def test_c3_steps_vs_oracle(torch_dev):
    torch, dev = torch_dev
    _run(torch, dev, pool(C3), 1)


def test_mirror_colour_words_are_not_read(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    venv = make_venv(dev, p, B)
    venv.reset()
    assert venv._state.goals_gray == 1
    rng = np.random.RandomState(32)
    for t in range(4):
        venv.step_async(torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev))
    gen = torch.Generator(device="cpu").manual_seed(5)

    def poison():
        fixed = ((venv.planes_ok & POK_MIRROR_FIXED) == POK_MIRROR_FIXED).nonzero().flatten()
        junk = torch.randint(-2 ** 31, 2 ** 31, (len(fixed), len(COLOUR_WORDS), 64),
                             generator=gen, dtype=torch.int64).to(torch.int32).to(dev)
        for i, q in enumerate(COLOUR_WORDS):
            venv.planes[fixed, 1, q, :] = junk[:, i].to(venv.planes.dtype)
        return fixed.cpu().numpy().tolist()

    fixed = poison()
    assert len(fixed) >= B // 2, len(fixed)
    sample = fixed[:2] + fixed[len(fixed) // 2:len(fixed) // 2 + 1] + fixed[-2:]
    oenvs = twins(venv, p, sample)
    n_done = n_poisoned = 0
    for t in range(T):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step_async(torch.from_numpy(acts).to(dev))
        n_done += check_step(venv, oenvs, acts, t)
        _check_scores(venv, oenvs, t)
        if t % 8 == 7:      # (a reset rewrote its env's mirror: poison the new episodes too)
            n_poisoned += len(set(poison()) & set(sample))
    assert n_done >= len(sample)
    assert n_poisoned >= len(sample)
    assert venv._state.goals_gray == 1


@pytest.mark.parametrize("rw", [True, False], ids=["less-white", "with-white"])
def test_packed_views_vs_oracle(torch_dev, rw):
    torch, dev = torch_dev
    p = pool(C3)
    kw = dict(view=(33, 33), channels=None, remove_white_goals=rw)
    venv = make_venv(dev, p, B, compute_obs=True, **kw)
    obs = venv.reset().cpu().numpy()
    assert venv._state.goals_gray == 1
    oenvs = twins(venv, p, SAMPLE, **kw)
    for e in SAMPLE:
        assert np.array_equal(obs[e], oenvs[e].obs()), e
    twin = None
    if not rw:              # beside a batch that keeps its board as uint16 cells
        twin = make_venv(dev, p, B, compute_obs=True, board_mode="uint16", **kw)
        twin.reset()
    rng = np.random.RandomState(33)
    n_done = n_planes = 0
    for t in range(T):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        obs, _, _, _ = venv.step(torch.from_numpy(acts).to(dev))
        n_planes += int(((venv.planes_ok & POK_BOARD_PLANES) != 0).sum().item())
        n_done += check_step(venv, oenvs, acts, (rw, t), obs=obs.cpu().numpy())
        if twin is not None:
            obs2, _, _, _ = twin.step(torch.from_numpy(acts).to(dev))
            assert torch.equal(obs, obs2), t
            assert torch.equal(venv.reward, twin.reward), t
    assert n_done >= len(SAMPLE)
    assert n_planes > B * T * 3 // 4
    if twin is not None:
        assert torch.equal(venv.board, twin.board) and torch.equal(venv.goals, twin.goals)


@pytest.mark.parametrize("which", ["c4", "c3+c4", "c3-one-red"])
def test_coloured_goals_keep_loading(torch_dev, which):
    torch, dev = torch_dev
    p = {"c4": lambda: pool(C4), "c3+c4": lambda: _mixed(pool(C3), pool(C4)),
         "c3-one-red": lambda: _one_red_goal(pool(C3))}[which]()
    _run(torch, dev, p, 0)
