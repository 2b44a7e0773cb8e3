"""The one-wave rollout of boards of 33 to 64 rows (kernel="mid": k_rollout_bits_mid,
sl_rollout_bits_mid.hip) against the oracle and against the per-cell kernels, its dispatch,
and the side-effect scores and the episode log on top of it at 40x40.  Everything is
compared exactly: the density maps are integer counts divided by num_samples in the same
division, and the EMD is the same arithmetic on both sides.

The inputs come from tests/rollout_mid_inputs.py; tests/test_rollout_mid_cpu.py checks with
the oracle alone that they reach the seam between the two halves of the rows, both wraps
and both outcomes of a spawn draw.
"""
import ctypes

import numpy as np
import pytest

import feature_pools as fp
import rollout_mid_inputs as mi

pytestmark = pytest.mark.gpu

H = mi.bits_helpers()


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


# ------------------------------------------------------- oracle and generic kernel
@pytest.mark.parametrize("shape", mi.SHAPES, ids=lambda s: "%dx%d" % s)
def test_mid_rollout_vs_oracle(torch_dev, shape):
    """Palette boards (every cell type, bits 12-14, 45 % empty): num_steps 0 and up, env ids
    far apart, and the never / draw / always branches of the spawn draw; one upper row,
    H = 64, odd W (the column-0 copy word), W = 2, full width, an odd number of lanes."""
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = mi.palette_case(shape)
    got = side_effect_densities(init, final, steps, sp, mi.S, rng="philox", seed=mi.SEED,
                                max_keys=128, kernel="mid", env_ids=ids)
    H._check_vs_oracle(got, init, final, steps, sp, mi.S, ids, seed=mi.SEED)


@pytest.mark.parametrize("shape", mi.SEAM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_seam_board_mid_vs_oracle(torch_dev, shape):
    """Blinkers across rows 31|32, the row wrap and the column wrap, spawners at the row
    seams and in the last column."""
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = mi.seam_case(shape)
    got = side_effect_densities(init, final, steps, sp, mi.S, rng="philox", seed=mi.SEED,
                                max_keys=128, kernel="mid", env_ids=ids)
    H._check_vs_oracle(got, init, final, steps, sp, mi.S, ids, seed=mi.SEED)


@pytest.mark.parametrize("shape", [(33, 33), (47, 64), (64, 63)], ids=lambda s: "%dx%d" % s)
def test_mid_equals_generic_on_soups(torch_dev, shape):
    """16-bit soups of at most 40 distinct values, E = 5: the same bytes from both kernels."""
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = mi.soup_case(shape)
    kw = dict(rng="philox", seed=mi.SEED, max_keys=256, env_ids=ids)
    mid = side_effect_densities(init, final, steps, sp, mi.S, kernel="mid", **kw)
    gen = side_effect_densities(init, final, steps, sp, mi.S, kernel="generic", **kw)
    assert len(mid) == 5 and any(len(m[0]) > 8 for m in mid)
    _same(mid, gen)


def test_one_episode_without_steps(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    init, final, _, _, _ = mi.palette_case((40, 21))
    got = side_effect_densities(init[:1], final[:1], [0], [0.3], mi.S, rng="philox",
                                seed=mi.SEED, max_keys=128, kernel="mid", env_ids=[12])
    assert len(got) == 1
    H._check_vs_oracle(got, init[:1], final[:1], [0], [0.3], mi.S, [12], seed=mi.SEED)


# ------------------------------------------------------------------------ overflow
def test_key_overflow_raises_the_same_on_mid_and_generic(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    init, final = mi.palette_case((48, 48))[:2]
    msgs = []
    for kernel in ("mid", "generic"):
        with pytest.raises(ValueError) as ei:
            side_effect_densities(init[:1], final[:1], [2], 0.3, 4, rng="philox", seed=1,
                                  max_keys=8, kernel=kernel)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]


# ------------------------------------------------------------------------ dispatch
@pytest.mark.parametrize("shape", [(32, 32), (64, 64), (128, 128), (40, 70)],
                         ids=lambda s: "%dx%d" % s)
def test_forced_mid_raises_off_its_shapes(torch_dev, shape):
    from safelife_amd.side_effects import side_effect_densities
    h, w = shape
    rng = np.random.RandomState(h)
    init = H._palette_boards(rng, 2, h, w)
    final = H._rolled(rng, init)
    with pytest.raises(RuntimeError):
        side_effect_densities(init, final, [1, 2], 0.3, 3, rng="philox", seed=2, kernel="mid")


def test_forced_mid_raises_in_stream_mode(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    rng = np.random.RandomState(3)
    init = H._palette_boards(rng, 1, 48, 48)
    final = H._rolled(rng, init)
    stream = rng.random_sample(200000)
    with pytest.raises(RuntimeError):
        side_effect_densities(init, final, [1], 0.3, 3, rng="stream", spawn_stream=stream,
                              kernel="mid")
    # ... where the per-cell kernels serve the call
    out = side_effect_densities(init, final, [1], 0.3, 3, rng="stream", spawn_stream=stream,
                                kernel="generic")
    assert len(out) == 1 and out[0][0]


def test_fast_still_raises_and_auto_gives_the_generic_bytes_at_48(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = mi.palette_case((48, 48))
    init, final, steps, sp, ids = init[:3], final[:3], steps[1:4], sp[1:4], ids[1:4]
    kw = dict(rng="philox", seed=mi.SEED, max_keys=128, env_ids=ids)
    with pytest.raises(RuntimeError):
        side_effect_densities(init, final, steps, sp, mi.S, kernel="fast", **kw)
    auto = side_effect_densities(init, final, steps, sp, mi.S, kernel="auto", **kw)
    gen = side_effect_densities(init, final, steps, sp, mi.S, kernel="generic", **kw)
    _same(auto, gen)


def test_c_entry_takes_a_narrow_board_when_asked(torch_dev):
    """sl_side_effect_densities_k itself with SL_KERNEL_MID at 33x20, a shape SL_KERNEL_AUTO
    leaves to the per-cell kernels: SL_OK, and the keys and maps of SL_KERNEL_GENERIC."""
    torch, dev = torch_dev
    from safelife_amd import _lib
    L = _lib.lib()
    E, h, w, mk, S = 2, 33, 20, 64, 5
    assert L.sl_side_effect_kernel_auto(h, w, _lib.SL_RNG_PHILOX) == _lib.SL_KERNEL_GENERIC
    rng = np.random.RandomState(33)
    init = H._palette_boards(rng, E, h, w)
    b0 = torch.from_numpy(init).to(dev)
    b1 = torch.from_numpy(H._rolled(rng, init)).to(dev)
    steps_h = np.array([2, 5], dtype=np.int32)
    steps_d = torch.from_numpy(steps_h.copy()).to(dev)
    sp = torch.tensor([0.3, 1.0], dtype=torch.float32, device=dev)
    nbytes = ctypes.c_int64()
    assert L.sl_side_effect_workspace(E, h, w, ctypes.byref(nbytes)) == _lib.SL_OK
    res = {}
    for kernel in (_lib.SL_KERNEL_MID, _lib.SL_KERNEL_GENERIC):
        keys = torch.zeros((E, mk), dtype=torch.uint16, device=dev)
        n_keys = torch.zeros(E, dtype=torch.int32, device=dev)
        present = torch.zeros((E, mk), dtype=torch.int32, device=dev)
        ina = torch.empty((E, mk, h, w), dtype=torch.float64, device=dev)
        act = torch.empty_like(ina)
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        rc = L.sl_side_effect_densities_k(
            b0.data_ptr(), b1.data_ptr(), steps_d.data_ptr(),
            steps_h.ctypes.data_as(ctypes.c_void_p), sp.data_ptr(), E, h, w, S,
            _lib.SL_RNG_PHILOX, 9, 40, None, None, mk, keys.data_ptr(), n_keys.data_ptr(),
            present.data_ptr(), ina.data_ptr(), act.data_ptr(), ws.data_ptr(),
            int(nbytes.value), None, kernel, _lib.stream_ptr(dev))
        assert rc == _lib.SL_OK, (kernel, rc)
        torch.cuda.synchronize()
        nk = n_keys.cpu().numpy()
        assert (nk > 0).all() and (nk <= mk).all()
        res[kernel] = [(nk[e], keys[e, :nk[e]].cpu().numpy(), present[e, :nk[e]].cpu().numpy(),
                        ina[e, :nk[e]].cpu().numpy(), act[e, :nk[e]].cpu().numpy())
                       for e in range(E)]
    for m, g in zip(res[_lib.SL_KERNEL_MID], res[_lib.SL_KERNEL_GENERIC]):
        for x, y in zip(m, g):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------- end to end, 40x40
def _levels40(K=4):
    # tests/mid_boards_cases.py builds its levels so (Case.level_dicts)
    return fp.build_levels(1061, K, 40, 40, 2)


def test_scores_on_the_device_equal_the_host_path(torch_dev):
    from safelife_amd.side_effects import side_effect_scores
    ds = _levels40()
    init = np.stack([d["board"] for d in ds])
    final = init.copy()
    for b in final:                      # a local change: six living cells less
        yy, xx = np.nonzero((b & 1) != 0)
        b[yy[:6], xx[:6]] = 0
    steps, sp, ids = [3, 0, 7, 12], [0.3, 0.3, 0.0, 1.0], [4, 90000, 17, 4000000000]
    kw = dict(rng="philox", seed=mi.SEED, env_ids=ids, max_keys=64)
    dev = side_effect_scores(init, final, steps, sp, 20, problems="device", emd="device",
                             kernel="mid", **kw)
    host = side_effect_scores(init, final, steps, sp, 20, kernel="generic", **kw)
    assert len(dev) == len(host) == 4
    for d, h in zip(dev, host):
        assert d and sorted(d) == sorted(h)
        for k in h:
            assert d[k][0] == h[k][0], k                         # the EMD: the same bits
            # the inaction sum: 1600 non-negative doubles in another order than np.sum's,
            # each order within 1600 * 2^-53 (1.8e-13) of the exact sum, relatively
            assert abs(d[k][1] - h[k][1]) <= 4e-13 * abs(h[k][1]), k


def test_episode_log_40_vs_oracle(torch_dev):
    """EpisodeLog over a 40x40 pool with rollout_kw = {kernel: 'mid'} against the oracle's
    records (the loop of test_gpu_rollout_bits.py's _run_logged, which cannot pass the
    keyword)."""
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, EpisodeLog, LevelPool
    ds = _levels40()
    pool, levels = LevelPool.from_levels(ds), fp.oracle_levels(ds)
    B, T = 4, 40
    kw = dict(time_limit=10, view_shape=(15, 15), output_channels=None, penalty_coef=1.0,
              min_performance=0.01)
    venv = SafeLifeVecEnv(pool, B, dev, rng="philox", seed=21, **kw)
    oenvs = []
    for e in range(B):
        o = H._LoggedOracle(lambda ep, e=e: levels[(e + ep * B) % len(levels)], env_id=e,
                            rng="philox", seed=21, **kw)
        o.finished = []
        oenvs.append(o)
    venv.reset()
    for o in oenvs:
        o.reset()
    with pytest.raises(ValueError):                      # the seed is the log's own
        EpisodeLog(venv, rollout_kw={"seed": 1})
    log = EpisodeLog(venv, num_samples=20, side_effect_seed=5, ring=16,
                     other_episode_data={"coef": 0.25}, rollout_kw={"kernel": "mid"})
    records = []
    rng = np.random.RandomState(6)
    for t in range(T):
        a = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step(torch.from_numpy(a).to(dev))
        for e in range(B):
            oenvs[e].step(int(a[e]))
    records += log.close()
    H._check_records(records, oenvs)
