"""Batches whose agent planes are not 0x62 take the plane kernel's run-time instance (or
no implied plane at all), each against the oracle: a pool with a fountain (mask 0x42),
a level with two agent cells (mask 0), can_toggle_powers (mask 0x02)."""
import numpy as np
import pytest

from agent_planes_util import (C3, FOUNTAIN, PLAYER, check_step, make_venv, pool, twins,
                               with_cell)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _run(torch, dev, p, mask, zero, **kw):
    B, T, sample = 64, 90, [0, 1, 31, 63]
    venv = make_venv(dev, p, B, **kw)
    venv.reset()
    assert venv._state.agent_planes == mask, hex(venv._state.agent_planes)
    assert venv._state.board_zero == zero, hex(venv._state.board_zero)
    oenvs = twins(venv, p, sample, **kw)
    rng = np.random.RandomState(14)
    n_done = n_planes = 0
    for t in range(T):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step_async(torch.from_numpy(acts).to(dev))
        n_planes += int(((venv.planes_ok & 64) != 0).sum().item())
        n_done += check_step(venv, oenvs, acts, t)
    assert n_done >= len(sample)
    assert n_planes > B * T * 3 // 4
    assert venv._state.agent_planes == mask and venv._state.board_zero == zero


def test_fountain_pool(torch_dev):
    torch, dev = torch_dev
    _run(torch, dev, with_cell(pool(C3), FOUNTAIN), 0x42, 0x7880)


def test_two_agent_cells(torch_dev):
    torch, dev = torch_dev
    _run(torch, dev, with_cell(pool(C3), PLAYER), 0x00, 0x7880)


def test_can_toggle_powers(torch_dev):
    torch, dev = torch_dev
    # (toggled powers take cell bits 0, 5, 6, 7 out of board_zero: 0x7880 & ~0x00E1)
    _run(torch, dev, pool(C3), 0x02, 0x7800, can_toggle_powers=True)
