"""Writes from outside the kernels narrow sl_env_state.agent_planes: a board with a
second preserving cell written mid-run (write_board, set_state) takes the envs out of
plane mode and the mask down, after which the batch steps like a uint16-mode twin; a
state_dict round trip keeps the mask."""
import numpy as np
import pytest

from agent_planes_util import C3, FOUNTAIN, check_step, make_venv, pool, twins

pytestmark = pytest.mark.gpu
B = 64


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _step_both(torch, dev, a, b, rng, ctx):
    acts = torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev)
    a.step_async(acts)
    b.step_async(acts)
    for x, y in ((a.reward, b.reward), (a.done, b.done), (a.flags, b.flags),
                 (a.ep_len, b.ep_len), (a.ep_rew, b.ep_rew)):
        assert torch.equal(x, y), ctx


def _same_state(torch, a, b, ctx):
    assert torch.equal(a.board, b.board), ctx
    assert torch.equal(a.goals, b.goals), ctx
    for k in a.st_t:
        assert torch.equal(a.st_t[k], b.st_t[k]), (ctx, k)


def _with_fountain(board, ay, ax):
    out = board.copy()
    ys, xs = np.nonzero(out == 0)
    far = (np.abs(ys - ay) > 4) & (np.abs(xs - ax) > 4)
    out[ys[far][0], xs[far][0]] = FOUNTAIN
    return out


@pytest.mark.parametrize("how", ["write_board", "set_state"])
def test_outside_board_write_narrows_the_mask(torch_dev, how):
    torch, dev = torch_dev
    p = pool(C3)
    a = make_venv(dev, p, B)
    b = make_venv(dev, p, B, board_mode="uint16")
    a.reset()
    b.reset()
    rng = np.random.RandomState(21)
    for t in range(12):
        _step_both(torch, dev, a, b, rng, t)
    assert a._state.agent_planes == 0x62
    assert int(((a.planes_ok & 64) != 0).sum().item()) > B // 2
    _same_state(torch, a, b, "before")
    boards = a.board.cpu().numpy()
    ax, ay = a.st_t["agent_x"].cpu().numpy(), a.st_t["agent_y"].cpu().numpy()
    if how == "write_board":
        for v in (a, b):
            v.write_board(5, _with_fountain(boards[5], ay[5], ax[5]))
    else:
        new = np.stack([_with_fountain(boards[e], ay[e], ax[e]) for e in range(B)])
        for v in (a, b):
            sc = {k: t.cpu().numpy() for k, t in v.st_t.items()}
            v.set_state(new, v.goals.cpu().numpy(), v.start_board.cpu().numpy(), **sc)
    assert a._state.agent_planes == 0, hex(a._state.agent_planes)
    assert a._state.board_zero == 0x7880
    assert int(((a.planes_ok & 64) != 0).sum().item()) == 0      # every env left the planes
    for t in range(45):
        _step_both(torch, dev, a, b, rng, (how, t))
        if t % 9 == 0:
            _same_state(torch, a, b, (how, t))
    assert int(((a.planes_ok & 64) != 0).sum().item()) > B // 2  # (in planes again)
    assert a._state.agent_planes == 0
    _same_state(torch, a, b, (how, "end"))


def test_state_dict_round_trip_keeps_the_mask(torch_dev):
    torch, dev = torch_dev
    p = pool(C3)
    a = make_venv(dev, p, B)
    a.reset()
    rng = np.random.RandomState(22)
    for t in range(10):
        a.step_async(torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev))
    sd = a.state_dict()
    assert sd["agent_planes"] == 0x62
    for t in range(5):
        a.step_async(torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev))
    a.load_state_dict(sd)
    assert a._state.agent_planes == 0x62 and a._state.board_zero == 0x7880
    assert int(((a.planes_ok & 64) != 0).sum().item()) == 0
    sample = [0, 1, 33, 63]
    oenvs = twins(a, p, sample)
    n_planes = 0
    for t in range(50):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        a.step_async(torch.from_numpy(acts).to(dev))
        n_planes += int(((a.planes_ok & 64) != 0).sum().item())
        check_step(a, oenvs, acts, t)
    assert n_planes > B * 50 * 3 // 4
    # a snapshot of boards under a narrower mask narrows this batch's
    sd["agent_planes"] = 0x02
    a.load_state_dict(sd)
    assert a._state.agent_planes == 0x02
    del sd["agent_planes"]                     # (a dict from before the field: none kept)
    a.load_state_dict(sd)
    assert a._state.agent_planes == 0
