"""The 128x128 band rollout (kernel="bands": k_rollout_bands128, sl_rollout_bits128.hip)
against the oracle and against the per-cell kernels, and the episode log on the C5 pool.
Everything is compared exactly: the density maps are integer counts divided by num_samples
in the same division.

The inputs come from tests/rollout128_inputs.py; tests/test_rollout128_cpu.py checks with
the oracle alone that they reach every band seam and both outcomes of a spawn draw.
"""
import os

import numpy as np
import pytest

import rollout128_inputs as ri

POOLS = os.path.join(os.path.dirname(__file__), "golden", "pools")
pytestmark = pytest.mark.gpu

H = ri.bits_helpers()


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _same(a, b):
    assert len(a) == len(b)
    for e in range(len(a)):
        for x, y in zip(a[e], b[e]):
            assert sorted(x) == sorted(y), e
            for k in y:
                assert np.array_equal(x[k], y[k]), (e, k)


def test_bands_rollout_vs_oracle(torch_dev):
    """Palette boards (every cell type, bits 12-14, 45 % empty): num_steps 0 and up, env ids
    far apart, and the never / draw / always branches of the spawn draw."""
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = ri.palette_case()
    got = side_effect_densities(init, final, steps, sp, ri.S, rng="philox", seed=ri.SEED,
                                max_keys=128, kernel="bands", env_ids=ids)
    H._check_vs_oracle(got, init, final, steps, sp, ri.S, ids, seed=ri.SEED)


def test_seam_board_bands_generic_oracle(torch_dev):
    """Blinkers across every band seam and the column wrap, a spawner at each seam."""
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = ri.seam_case()
    kw = dict(rng="philox", seed=ri.SEED, max_keys=128, env_ids=ids)
    bands = side_effect_densities(init, final, steps, sp, ri.S, kernel="bands", **kw)
    gen = side_effect_densities(init, final, steps, sp, ri.S, kernel="generic", **kw)
    _same(bands, gen)
    H._check_vs_oracle(bands, init, final, steps, sp, ri.S, ids, seed=ri.SEED)


def test_bands_equals_generic_on_c5_pool(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    board = np.load(os.path.join(POOLS, "c5_navigation_128.npz"))["board"]
    E = 5
    init = np.ascontiguousarray(board[np.arange(E) % len(board)])
    rng = np.random.RandomState(4)
    final = H._rolled(rng, init)
    steps, sp, ids = [0, 3, 11, 1, 6], [0.3] * E, [5, 6, 900, 2, 31]
    kw = dict(rng="philox", seed=ri.SEED, max_keys=128, env_ids=ids)
    bands = side_effect_densities(init, final, steps, sp, ri.S, kernel="bands", **kw)
    gen = side_effect_densities(init, final, steps, sp, ri.S, kernel="generic", **kw)
    _same(bands, gen)
    auto = side_effect_densities(init, final, steps, sp, ri.S, kernel="auto", **kw)
    _same(auto, gen)
    H._check_vs_oracle(bands, init, final, steps, sp, ri.S, ids, seed=ri.SEED)


def test_key_overflow_raises_the_same_on_bands_and_generic(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    init, final = ri.palette_case()[:2]
    msgs = []
    for kernel in ("bands", "generic"):
        with pytest.raises(ValueError) as ei:
            side_effect_densities(init[:1], final[:1], [2], 0.3, 4, rng="philox", seed=1,
                                  max_keys=8, kernel=kernel)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]


@pytest.mark.parametrize("shape", [(64, 64), (33, 20)], ids=lambda s: "%dx%d" % s)
def test_forced_bands_raises_off_128(torch_dev, shape):
    from safelife_amd.side_effects import side_effect_densities
    h, w = shape
    rng = np.random.RandomState(h)
    init = H._palette_boards(rng, 2, h, w)
    final = H._rolled(rng, init)
    with pytest.raises(RuntimeError):
        side_effect_densities(init, final, [1, 2], 0.3, 3, rng="philox", seed=2,
                              kernel="bands")


def _map_functional(a, b, **_):
    """Stands in for the EMD of two density maps: a position-weighted sum, exact and
    deterministic, that moves when any cell of either map does (densities are multiples of
    1 / num_samples, the weights are distinct)."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    w = np.sqrt(np.arange(1.0, a.size + 1.0)).reshape(a.shape)
    return float((a * w).sum() - 2.0 * (b * w).sum())


def test_episode_log_c5_vs_oracle(torch_dev, monkeypatch):
    """EpisodeLog on the C5 pool (its flush scores through kernel='auto') against the
    oracle's density maps, record by record.

    The earth mover's distance is host code that this comparison runs identically on both
    sides (log and oracle maps); on 128x128 maps around spawners it moves thousands of cells
    and takes seconds per key, 156 s for this test with the real EMD (it passed so).  The rollout is what is under test, so both sides get the same cheap exact
    functional of the two maps in its place; the real EMD through the log is
    test_gpu_rollout_bits.py::test_episode_log_64_spawners_vs_oracle."""
    torch, dev = torch_dev
    from safelife_amd import LevelPool, side_effects
    monkeypatch.setattr(side_effects, "earth_mover_distance", _map_functional)
    pool = LevelPool.load(os.path.join(POOLS, "c5_navigation_128.npz"))
    records, oenvs = H._run_logged(torch, dev, pool, 4, 10, 40, ring=64)
    H._check_records(records, oenvs)
