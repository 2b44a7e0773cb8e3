"""Views written by the plane kernels from the implied layout (the agent's planes built
from its position, sl_env_state.agent_planes 0x62) against the oracle: packed views and
15-channel views (uint16, uint8), the views of envs reset by the step included."""
import numpy as np
import pytest

from agent_planes_util import C3, C4, check_step, make_venv, pool, twins

pytestmark = pytest.mark.gpu

CASES = [("c3", C3, None, "uint16"), ("c4", C4, None, "uint16"),
         ("c3", C3, tuple(range(15)), "uint16"), ("c4", C4, tuple(range(15)), "uint8")]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


@pytest.mark.parametrize("name,path,channels,dtype", CASES,
                         ids=["%s-%s-%s" % (c[0], "packed" if c[2] is None else "15ch", c[3])
                              for c in CASES])
def test_views_vs_oracle(torch_dev, name, path, channels, dtype):
    torch, dev = torch_dev
    B, T, sample = 64, 90, [0, 1, 31, 63]
    p = pool(path)
    kw = dict(view=(33, 33), channels=channels)
    venv = make_venv(dev, p, B, dtype=dtype, compute_obs=True, **kw)
    obs = venv.reset().cpu().numpy()
    assert venv._state.agent_planes == 0x62 and venv._state.board_zero == 0x7880
    oenvs = twins(venv, p, sample, **kw)
    for e in sample:
        assert np.array_equal(obs[e] != 0 if channels else obs[e], oenvs[e].obs()), e
    rng = np.random.RandomState(16)
    n_done = n_planes = 0
    for t in range(T):
        acts = rng.randint(0, 9, size=B).astype(np.int32)
        obs, _, _, info = venv.step(torch.from_numpy(acts).to(dev))
        n_planes += int(((venv.planes_ok & 64) != 0).sum().item())
        got = obs.cpu().numpy()
        if channels:
            got = (got != 0).astype(np.uint16)
        n_done += check_step(venv, oenvs, acts, (name, t), obs=got)
    assert n_done >= 2 * len(sample)          # views of envs the step reset were compared
    assert n_planes > B * T * 3 // 4          # written from the planes
    assert venv._state.agent_planes == 0x62
