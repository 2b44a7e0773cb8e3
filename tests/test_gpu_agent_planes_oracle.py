"""The 64x64 plane kernel with the agent's planes implied (sl_env_state.agent_planes
0x62: cell bits 1, 5, 6 built from the agent's position, not stored) against the oracle,
step by step: reward, done, flags, scores, goals and the completed board.

The c3 and c4 pools with random rolls and a time limit of 40 (resets and re-entries into
plane mode many times), and hand-built levels with the agent on the corners of the
lane / word / bit selection of the implied words -- (0,0), (31,63), (32,0), (63,63), an
odd and an even column -- walked across the row-31/32 seam and both torus wraps, pushing
crates across them.
"""
import numpy as np
import pytest

from agent_planes_util import (C3, C4, CRATE, check_step, hand_level, make_venv, pool,
                               twins)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


@pytest.mark.parametrize("path", [C3, C4], ids=["c3", "c4"])
def test_pool_steps_vs_oracle(torch_dev, path):
    torch, dev = torch_dev
    B, T, sample = 96, 100, [0, 1, 47, 64, 95]
    p = pool(path)
    venv = make_venv(dev, p, B)
    venv.reset()
    assert venv._state.agent_planes == 0x62 and venv._state.board_zero == 0x7880
    oenvs = twins(venv, p, sample)
    rng = np.random.RandomState(12)
    n_done = n_planes = 0
    for t in range(T):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step_async(torch.from_numpy(acts).to(dev))
        n_planes += int(((venv.planes_ok & 64) != 0).sum().item())
        n_done += check_step(venv, oenvs, acts, t)
        assert venv._state.agent_planes == 0x62 and venv._state.board_zero == 0x7880
    assert n_done >= 2 * len(sample)
    assert n_planes > B * T * 3 // 4          # the steps were plane steps


def _seam_levels():
    return [
        hand_level(0, 0, ((63, 0, CRATE), (0, 63, CRATE))),       # up / left: both wraps
        hand_level(31, 63, ((32, 63, CRATE), (31, 0, CRATE))),    # down: the seam; right: wrap
        hand_level(32, 0, ((31, 0, CRATE), (32, 63, CRATE))),     # up: the seam; left: wrap
        hand_level(63, 63, ((0, 63, CRATE), (63, 0, CRATE))),     # down / right: both wraps
        hand_level(10, 7, ((10, 8, CRATE),)),                     # an odd column
        hand_level(10, 8, ((10, 7, CRATE),)),                     # an even column
    ]


# 1-4 move up / right / down / left, 5-8 toggle the cell ahead; every agent first pushes
# its crates across a seam or a wrap, walks a loop over them, then builds and destroys
SCRIPT = [1, 1, 3, 3, 3, 3, 1, 1,  4, 4, 2, 2, 2, 2, 4, 4,  3, 2, 2, 1, 4, 4,
          5, 1, 6, 2, 7, 3, 8, 4, 5, 5, 0, 6, 6]


def test_hand_built_levels_on_the_seams(torch_dev):
    torch, dev = torch_dev
    from safelife_amd import LevelPool
    B, T = 64, 90
    p = LevelPool.from_levels(_seam_levels())
    sample = [0, 1, 2, 3, 4, 5, 63]
    venv = make_venv(dev, p, B, random_order=False, augment=False)
    venv.reset()
    assert venv._state.agent_planes == 0x62
    oenvs = twins(venv, p, sample, random_order=False, augment=False)
    rng = np.random.RandomState(8)
    n_done = 0
    for t in range(T):
        if t < len(SCRIPT):
            acts = np.full(B, SCRIPT[t], np.int32)
        else:
            acts = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step_async(torch.from_numpy(acts).to(dev))
        # every env is in planes but those the step reset (all of them at the time limit)
        assert bool((((venv.planes_ok & 64) != 0) | ((venv.flags & 4) != 0)).all().item()), t
        n_done += check_step(venv, oenvs, acts, t)
    assert n_done >= len(sample)
    assert venv._state.agent_planes == 0x62
