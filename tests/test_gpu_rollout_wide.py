"""The band rollout of boards past 64 rows or columns (kernel="wide": k_rollout_bits_wide,
sl_rollout_bits_wide.hip) against the oracle and against the per-cell kernels, its dispatch,
and the side-effect scores and the episode log on top of it at 70x70.  Everything is
compared exactly: the density maps are integer counts divided by num_samples in the same
division, and the EMD is the same arithmetic on both sides.

The inputs come from tests/rollout_wide_inputs.py; tests/test_rollout_wide_cpu.py checks
with the oracle alone that they reach every seam between two bands of rows, both wraps and
both outcomes of a spawn draw.
"""
import ctypes

import numpy as np
import pytest

import feature_pools as fp
import rollout_wide_inputs as wi

pytestmark = pytest.mark.gpu

H = wi.bits_helpers()


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
@pytest.mark.parametrize("shape", wi.SHAPES, ids=lambda s: "%dx%d" % s)
def test_wide_rollout_vs_oracle(torch_dev, shape):
    """Palette boards (every cell type, bits 12-14, 45 % empty): num_steps 0 and up, env ids
    far apart, and the never / draw / always branches of the spawn draw; one to four bands,
    one real row in the last band, odd W (the column-0 copy word, in lane 63 too), W = 2,
    full width, both load paths."""
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = wi.palette_case(shape)
    got = side_effect_densities(init, final, steps, sp, wi.S, rng="philox", seed=wi.SEED,
                                max_keys=128, kernel="wide", env_ids=ids)
    H._check_vs_oracle(got, init, final, steps, sp, wi.S, ids, seed=wi.SEED)


@pytest.mark.parametrize("shape", wi.SEAM_SHAPES, ids=lambda s: "%dx%d" % s)
def test_seam_board_wide_vs_oracle(torch_dev, shape):
    """Blinkers across every band seam, the row wrap and the column wrap, spawners at the
    row seams and in the last column."""
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = wi.seam_case(shape)
    got = side_effect_densities(init, final, steps, sp, wi.S, rng="philox", seed=wi.SEED,
                                max_keys=128, kernel="wide", env_ids=ids)
    H._check_vs_oracle(got, init, final, steps, sp, wi.S, ids, seed=wi.SEED)


@pytest.mark.parametrize("shape", [(33, 65), (96, 96), (128, 127)], ids=lambda s: "%dx%d" % s)
def test_wide_equals_generic_on_soups(torch_dev, shape):
    """16-bit soups of at most 40 distinct values, E = 5: the same bytes from both kernels."""
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = wi.soup_case(shape)
    kw = dict(rng="philox", seed=wi.SEED, max_keys=256, env_ids=ids)
    wide = side_effect_densities(init, final, steps, sp, wi.S, kernel="wide", **kw)
    gen = side_effect_densities(init, final, steps, sp, wi.S, kernel="generic", **kw)
    assert len(wide) == 5 and any(len(m[0]) > 8 for m in wide)
    _same(wide, gen)


def test_one_episode_without_steps(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    init, final, _, _, _ = wi.palette_case((65, 65))
    got = side_effect_densities(init[:1], final[:1], [0], [0.3], wi.S, rng="philox",
                                seed=wi.SEED, max_keys=128, kernel="wide", env_ids=[12])
    assert len(got) == 1
    H._check_vs_oracle(got, init[:1], final[:1], [0], [0.3], wi.S, [12], seed=wi.SEED)


# ------------------------------------------------------------------------ overflow
def test_key_overflow_raises_the_same_on_wide_and_generic(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    rng = np.random.RandomState(7070)
    init = H._palette_boards(rng, 1, 70, 70)
    final = H._rolled(rng, init)
    msgs = []
    for kernel in ("wide", "generic"):
        with pytest.raises(ValueError) as ei:
            side_effect_densities(init, final, [2], 0.3, 4, rng="philox", seed=1,
                                  max_keys=8, kernel=kernel)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]


# ------------------------------------------------------------------------ dispatch
@pytest.mark.parametrize("shape", [(32, 32), (48, 48), (64, 64), (128, 128)],
                         ids=lambda s: "%dx%d" % s)
def test_forced_wide_raises_off_its_shapes(torch_dev, shape):
    from safelife_amd.side_effects import side_effect_densities
    h, w = shape
    rng = np.random.RandomState(h)
    init = H._palette_boards(rng, 2, h, w)
    final = H._rolled(rng, init)
    with pytest.raises(RuntimeError):
        side_effect_densities(init, final, [1, 2], 0.3, 3, rng="philox", seed=2, kernel="wide")


def test_forced_wide_raises_in_stream_mode(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    rng = np.random.RandomState(3)
    init = H._palette_boards(rng, 1, 65, 65)
    final = H._rolled(rng, init)
    stream = rng.random_sample(400000)
    with pytest.raises(RuntimeError):
        side_effect_densities(init, final, [1], 0.3, 3, rng="stream", spawn_stream=stream,
                              kernel="wide")
    # ... where the per-cell kernels serve the call
    out = side_effect_densities(init, final, [1], 0.3, 3, rng="stream", spawn_stream=stream,
                                kernel="generic")
    assert len(out) == 1 and out[0][0]


def test_auto_gives_the_generic_bytes_at_65(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    init, final, steps, sp, ids = wi.palette_case((65, 65))
    init, final, steps, sp, ids = init[:3], final[:3], steps[1:4], sp[1:4], ids[1:4]
    kw = dict(rng="philox", seed=wi.SEED, max_keys=128, env_ids=ids)
    auto = side_effect_densities(init, final, steps, sp, wi.S, kernel="auto", **kw)
    gen = side_effect_densities(init, final, steps, sp, wi.S, kernel="generic", **kw)
    _same(auto, gen)


def test_c_entry_takes_boards_at_an_address_that_is_2_mod_4(torch_dev):
    """sl_side_effect_densities_k itself with SL_KERNEL_WIDE at 65x3, the boards a uint16
    view one element into a larger tensor (the kernel has no alignment rule): SL_OK, and
    the keys and maps of SL_KERNEL_GENERIC."""
    torch, dev = torch_dev
    from safelife_amd import _lib
    L = _lib.lib()
    E, h, w, mk, S = 2, 65, 3, 64, 5
    rng = np.random.RandomState(653)
    init = H._palette_boards(rng, E, h, w)
    final = H._rolled(rng, init)
    n = E * h * w
    boards = []
    for src in (init, final):
        big = torch.zeros(n + 3, dtype=torch.uint16, device=dev)
        view = big[1:1 + n]
        view.copy_(torch.from_numpy(src.reshape(-1)).to(dev))
        assert view.data_ptr() % 4 == 2
        boards.append((big, view))
    b0, b1 = boards[0][1], boards[1][1]
    steps_h = np.array([2, 5], dtype=np.int32)
    steps_d = torch.from_numpy(steps_h.copy()).to(dev)
    sp = torch.tensor([0.3, 1.0], dtype=torch.float32, device=dev)
    nbytes = ctypes.c_int64()
    assert L.sl_side_effect_workspace(E, h, w, ctypes.byref(nbytes)) == _lib.SL_OK
    res = {}
    for kernel in (_lib.SL_KERNEL_WIDE, _lib.SL_KERNEL_GENERIC):
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
    for m, g in zip(res[_lib.SL_KERNEL_WIDE], res[_lib.SL_KERNEL_GENERIC]):
        for x, y in zip(m, g):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------- end to end, 70x70
def _levels70(K=4):
    return fp.build_levels(1071, K, 70, 70, 2)


def test_scores_on_the_device_equal_the_host_path(torch_dev):
    from safelife_amd.side_effects import side_effect_scores
    ds = _levels70()
    init = np.stack([d["board"] for d in ds])
    final = init.copy()
    for b in final:                      # a local change: six living cells less
        yy, xx = np.nonzero((b & 1) != 0)
        b[yy[:6], xx[:6]] = 0
    steps, sp, ids = [3, 0, 7, 12], [0.3, 0.3, 0.0, 1.0], [4, 90000, 17, 4000000000]
    kw = dict(rng="philox", seed=wi.SEED, env_ids=ids, max_keys=64)
    dev = side_effect_scores(init, final, steps, sp, 20, problems="device", emd="device",
                             kernel="wide", **kw)
    host = side_effect_scores(init, final, steps, sp, 20, kernel="generic", **kw)
    assert len(dev) == len(host) == 4
    for d, h in zip(dev, host):
        assert d and sorted(d) == sorted(h)
        for k in h:
            assert d[k][0] == h[k][0], k                         # the EMD: the same bits
            # the inaction sum: 4900 non-negative doubles in another order than np.sum's,
            # each order within 4900 * 2^-53 (5.4e-13) of the exact sum, relatively
            assert abs(d[k][1] - h[k][1]) <= 4900 * 2.0 ** -53 * 2 * abs(h[k][1]), k


def test_episode_log_70_vs_oracle(torch_dev):
    """EpisodeLog with rollout_kw = {kernel: 'wide'} over a 70x70 pool stepped by the wide
    step kernel, against the oracle's records."""
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, EpisodeLog, LevelPool
    ds = _levels70()
    pool, levels = LevelPool.from_levels(ds), fp.oracle_levels(ds)
    B, T = 4, 40
    kw = dict(time_limit=10, view_shape=(15, 15), output_channels=None, penalty_coef=1.0,
              min_performance=0.01)
    venv = SafeLifeVecEnv(pool, B, dev, rng="philox", seed=21, kernel="wide", **kw)
    oenvs = []
    for e in range(B):
        o = H._LoggedOracle(lambda ep, e=e: levels[(e + ep * B) % len(levels)], env_id=e,
                            rng="philox", seed=21, **kw)
        o.finished = []
        oenvs.append(o)
    venv.reset()
    for o in oenvs:
        o.reset()
    log = EpisodeLog(venv, num_samples=20, side_effect_seed=5, ring=16,
                     other_episode_data={"coef": 0.25}, rollout_kw={"kernel": "wide"})
    records = []
    rng = np.random.RandomState(6)
    for t in range(T):
        a = rng.randint(0, 9, size=B).astype(np.int32)
        venv.step(torch.from_numpy(a).to(dev))
        for e in range(B):
            oenvs[e].step(int(a[e]))
    records += log.close()
    H._check_records(records, oenvs)
