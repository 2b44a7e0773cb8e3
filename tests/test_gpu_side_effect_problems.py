"""The EMD problems built on the device (sl_side_effect_problems.hip) and the paths on top
of them: the two kernels on synthetic maps against numpy, side_effect_scores(...,
problems="device") against "host" on real rollouts, and EpisodeLog(scoring="device")
against "host".

Cells, coordinates, densities, offsets and EMDs are compared exactly.  The inaction map's
sum is compared with np.sum within relative 2 * hw * 2**-53: any two summation orders of
hw non-negative doubles differ by at most that (each of the at most hw - 1 additions of
either order rounds by at most 2**-53 of a partial sum, and no partial sum exceeds the
total).
"""
import ctypes
import os

import numpy as np
import pytest

import oracle

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
POOLS = os.path.join(GOLDEN, "pools")
pytestmark = pytest.mark.gpu

SEED = 77


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _mass_close(got, want, hw):
    return abs(got - want) <= 2.0 * hw * 2.0 ** -53 * abs(want)


# ------------------------------------------------------- kernels on synthetic maps
E, MK, NKEYS = 3, 4, [0, 2, 4]
TIE = 1e-3 * 1.0                              # the threshold of a problem whose gmax is 1.0


def _synthetic(H, W):
    """inaction, action [E, MK, H, W]: rows at or above n_keys[e] are NaN (never read);
    episode 1: identical maps, then one map all zero; episode 2: changed cells in every
    wave and chunk with cell 0 and cell hw - 1, the threshold tie, two dense random maps,
    and a sparse action map over an all-zero inaction map."""
    hw = H * W
    rng = np.random.RandomState(1000 * H + W)
    ina = np.full((E, MK, hw), np.nan)
    act = np.full((E, MK, hw), np.nan)

    def dens():                               # multiples of 1/8 with many exact zeros
        return rng.randint(0, 9, size=hw) / 8.0 * (rng.rand(hw) < 0.6)

    ina[1, 0] = act[1, 0] = dens()
    ina[1, 1], act[1, 1] = dens(), 0.0
    ina[1, 1, hw - 1] = 0.5
    a = dens()
    b = a.copy()
    cells = sorted(set(range(0, hw, 37)) | {0, hw - 1})       # one in every 64 cells
    b[cells] = a[cells] + 0.25 + 0.5 * rng.rand(len(cells))
    ina[2, 0], act[2, 0] = a, b
    a = dens()
    b = a.copy()
    one, tie, above = (1, 2, 4) if hw < 300 else (hw // 2 + 3, 70, hw - 67)
    a[[one, tie, above]] = [1.0, TIE, np.nextafter(TIE, 1.0)]
    b[[one, tie, above]] = 0.0
    ina[2, 1], act[2, 1] = a, b
    ina[2, 2], act[2, 2] = rng.rand(hw), rng.rand(hw)
    ina[2, 3], act[2, 3] = 0.0, dens()
    act[2, 3, 0] = 1.0
    return ina.reshape(E, MK, H, W), act.reshape(E, MK, H, W)


def _reference(ina, act):
    """numpy on the same arrays: per read slot the cells of earth_mover_distance."""
    H, W = ina.shape[2:]
    counts, mass, p, q, ys, xs = [], [], [], [], [], []
    for e in range(E):
        for k in range(MK):
            if k >= NKEYS[e]:
                counts.append(0)
                mass.append(0.0)
                continue
            a, b = ina[e, k], act[e, k]
            gap = np.abs(a - b)
            yy, xx = np.nonzero(gap > 1e-3 * gap.max())
            counts.append(len(yy))
            mass.append(np.sum(a))
            p.append(a[yy, xx])
            q.append(b[yy, xx])
            ys.append(yy)
            xs.append(xx)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return (offsets, np.array(mass), np.concatenate(p), np.concatenate(q),
            np.concatenate(ys).astype(np.int32), np.concatenate(xs).astype(np.int32))


def _run_kernels(torch, dev, ina, act, cap_short=0):
    """Both entry points on the given maps.  The four output buffers hold
    total - cap_short cells and one canary word each, which is returned as well."""
    from safelife_amd import _lib
    L = _lib.lib()
    H, W = ina.shape[2:]
    n = E * MK
    ina_d, act_d = torch.from_numpy(ina).to(dev), torch.from_numpy(act).to(dev)
    nk = torch.tensor(NKEYS, dtype=torch.int32, device=dev)
    nbytes = ctypes.c_int64()
    _lib.check(L.sl_side_effect_problems_workspace(E, MK, ctypes.byref(nbytes)), "workspace")
    assert nbytes.value % 8 == 0
    ws = torch.zeros(nbytes.value // 8, dtype=torch.int64, device=dev)
    offsets = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    mass = torch.full((n,), -7.0, dtype=torch.float64, device=dev)
    stream = _lib.stream_ptr(dev)
    _lib.check(L.sl_side_effect_problem_counts(
        ina_d.data_ptr(), act_d.data_ptr(), nk.data_ptr(), E, MK, H, W, offsets.data_ptr(),
        mass.data_ptr(), ws.data_ptr(), nbytes.value, stream), "counts")
    off_h = offsets.cpu().numpy()
    cap = int(off_h[n]) - cap_short
    p = torch.full((cap + 1,), -5.0, dtype=torch.float64, device=dev)
    q = torch.full((cap + 1,), -5.0, dtype=torch.float64, device=dev)
    ys = torch.full((cap + 1,), -5, dtype=torch.int32, device=dev)
    xs = torch.full((cap + 1,), -5, dtype=torch.int32, device=dev)
    _lib.check(L.sl_side_effect_problem_cells(
        ina_d.data_ptr(), act_d.data_ptr(), nk.data_ptr(), E, MK, H, W, offsets.data_ptr(),
        p.data_ptr(), q.data_ptr(), ys.data_ptr(), xs.data_ptr(), cap, ws.data_ptr(),
        nbytes.value, stream), "cells")
    torch.cuda.synchronize()
    return off_h, mass.cpu().numpy(), [t.cpu().numpy() for t in (p, q, ys, xs)]


SHAPES = [(2, 3), (25, 25), (64, 64), (128, 128)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def synthetic(request):
    ina, act = _synthetic(*request.param)
    return ina, act, _reference(ina, act)


def test_synthetic_cases_hold_what_they_should(synthetic):
    """The inputs themselves: the tie is exact, every wave of every chunk has a cell."""
    ina, act, (offsets, mass, p, q, ys, xs) = synthetic
    H, W = ina.shape[2:]
    hw = H * W
    counts = np.diff(offsets).reshape(E, MK)
    assert (counts[0] == 0).all() and (counts[1, 2:] == 0).all()
    assert counts[1, 0] == 0 and counts[1, 1] > 0 and counts[2, 3] > 0
    assert np.isnan(ina[0]).all() and np.isnan(act[1, 2:]).all()
    lo = offsets[2 * MK]
    cell = ys[lo:offsets[2 * MK + 1]].astype(np.int64) * W + xs[lo:offsets[2 * MK + 1]]
    assert cell[0] == 0 and cell[-1] == hw - 1
    assert set(cell // 64) == set(range((hw + 63) // 64))
    a, b = ina[2, 1].ravel(), act[2, 1].ravel()
    gaps = np.sort(a - b)[-3:]
    assert gaps[2] == 1.0 and gaps[0] == 1e-3 * 1.0 and gaps[1] == np.nextafter(gaps[0], 1.0)
    assert counts[2, 1] == 2                  # the tie itself is not selected
    assert counts[2, 2] > 0.9 * hw


def test_kernels_equal_numpy(torch_dev, synthetic):
    torch, dev = torch_dev
    ina, act, (offsets, mass, p, q, ys, xs) = synthetic
    hw = ina.shape[2] * ina.shape[3]
    off_d, mass_d, (p_d, q_d, ys_d, xs_d) = _run_kernels(torch, dev, ina, act)
    assert np.array_equal(off_d, offsets)
    total = int(offsets[-1])
    assert np.array_equal(ys_d[:total], ys) and np.array_equal(xs_d[:total], xs)
    assert np.array_equal(p_d[:total].view(np.uint64), p.view(np.uint64))
    assert np.array_equal(q_d[:total].view(np.uint64), q.view(np.uint64))
    assert p_d[total] == -5.0 and q_d[total] == -5.0 and ys_d[total] == -5 and xs_d[total] == -5
    for i in range(E * MK):
        print(i, repr(float(mass_d[i])), repr(float(mass[i])))
        if i % MK >= NKEYS[i // MK]:
            assert mass_d[i] == 0.0, i
        else:
            assert _mass_close(mass_d[i], mass[i], hw), (i, mass_d[i], mass[i])


@pytest.mark.parametrize("short", ["one", "half"])
def test_fill_stores_nothing_at_or_beyond_cap(torch_dev, short):
    """cap = total - 1 drops the last cell of the last problem; cap = total // 2 falls
    inside the dense problem, so whole waves, chunks and later problems lie beyond it."""
    torch, dev = torch_dev
    ina, act = _synthetic(25, 25)
    offsets, mass, p, q, ys, xs = _reference(ina, act)
    total = int(offsets[-1])
    cap = total - 1 if short == "one" else total // 2
    assert offsets[2 * MK + 2] < cap < offsets[2 * MK + 3] or short == "one"
    off_d, _, (p_d, q_d, ys_d, xs_d) = _run_kernels(torch, dev, ina, act, cap_short=total - cap)
    assert np.array_equal(off_d, offsets) and len(p_d) == cap + 1
    # the canary word behind each buffer, where the first cell beyond cap would have gone
    assert p_d[cap] == -5.0 and q_d[cap] == -5.0 and ys_d[cap] == -5 and xs_d[cap] == -5
    assert np.array_equal(p_d[:cap], p[:cap]) and np.array_equal(q_d[:cap], q[:cap])
    assert np.array_equal(ys_d[:cap], ys[:cap]) and np.array_equal(xs_d[:cap], xs[:cap])


# ------------------------------------------------- device against host on rollouts
N_EP = 5
STEPS = [2, 0, 5, 1, 12]
IDS = [40, 2, 77, 5, 4000000000]
SAMPLES = 6
LIFE = 1


def _episodes(name):
    """The pool's first levels as five finished episodes.  The final board is the start
    board after num_steps oracle advances (Philox, the episode's spawn probability) in
    which, at the third advance from the end at the latest, something took a handful of
    living cells away next to each other -- what an agent does -- so that the action run
    differs from the inaction run around that place.

    The 128x128 navigation levels hold hundreds of spawners; with their spawn probability
    (0.3) the two runs draw apart and differ in 5 000 and more cells per episode, an exact
    transport of minutes on the host for every mode compared.  There the episodes run
    with spawn probability 0.0: the problems stay those of a local change (hundreds of
    cells), and what is compared -- selection, order, doubles, EMD -- is the same code.
    test_problems_reproduce_the_host_selection runs that pool at 0.3 as well."""
    board = np.load(os.path.join(POOLS, name + ".npz"))["board"]
    sp = 0.0 if board.shape[1] == 128 else 0.3
    init = np.ascontiguousarray(board[np.arange(N_EP) % len(board)])
    final = []
    for e in range(N_EP):
        b = init[e]
        for t in range(STEPS[e]):
            if t == max(0, STEPS[e] - 3):
                b = _take_life(b)
            b, _ = oracle.advance(b, sp, rng=oracle.RNG_PHILOX, seed=9, env_id=e, step=t,
                                  tensor=0)
        if STEPS[e] == 0:
            b = _take_life(b)
        final.append(b)
    return init, np.stack(final), [sp] * N_EP


def _take_life(board):
    """The board without the (up to) six living cells nearest to its first one."""
    b = board.copy()
    yy, xx = np.nonzero((b & LIFE) != 0)
    near = np.argsort(np.abs(yy - yy[0]) + np.abs(xx - xx[0]), kind="stable")[:6]
    b[yy[near], xx[near]] = 0
    return b


POOL_NAMES = ["c2_append_still_25", "c3_prune_still_64", "c5_navigation_128"]


@pytest.fixture(scope="module", params=POOL_NAMES)
def rollouts(request, torch_dev):
    """One pool's episodes with the host path's scores, computed once."""
    from safelife_amd.side_effects import side_effect_scores
    init, final, sp = _episodes(request.param)
    kw = dict(rng="philox", seed=SEED, env_ids=IDS)
    host = side_effect_scores(init, final, STEPS, sp, SAMPLES, **kw)
    return init, final, sp, kw, host


def _same_scores(dev_scores, host_scores, hw):
    assert len(dev_scores) == len(host_scores)
    for e, (d, h) in enumerate(zip(dev_scores, host_scores)):
        assert sorted(d) == sorted(h), e
        assert list(d) == list(h), e          # the YAML text follows this order
        for key in h:
            print(e, key, repr(d[key][0]), repr(h[key][0]), repr(float(d[key][1])),
                  repr(float(h[key][1])))
            assert d[key][0] == h[key][0], (e, key)
            assert _mass_close(d[key][1], h[key][1], hw), (e, key, d[key][1], h[key][1])


def test_device_scores_equal_host_scores(torch_dev, rollouts):
    from safelife_amd.side_effects import side_effect_scores
    init, final, sp, kw, host = rollouts
    hw = init.shape[1] * init.shape[2]
    assert any(v[0] > 0 for h in host for v in h.values())      # the two runs do differ
    dev = side_effect_scores(init, final, STEPS, sp, SAMPLES, problems="device", **kw)
    _same_scores(dev, host, hw)


def test_device_scores_honour_include_and_exclude(torch_dev, rollouts):
    from safelife_amd.side_effects import side_effect_scores
    init, final, sp, kw, host = rollouts
    hw = init.shape[1] * init.shape[2]
    keys = sorted(set(k for h in host for k in h))
    assert len(keys) >= 2
    inc, exc = keys[::2] + [60000], keys[:1]
    for sel in (dict(include=inc), dict(exclude=exc), dict(include=inc, exclude=exc)):
        want = [{k: v for k, v in h.items()
                 if ("include" not in sel or k in sel["include"])
                 and ("exclude" not in sel or k not in sel["exclude"])} for h in host]
        got = side_effect_scores(init, final, STEPS, sp, SAMPLES, problems="device", **kw, **sel)
        for g, w in zip(got, want):
            assert sorted(g) == sorted(w)
        _same_scores([{k: g[k] for k in w} for g, w in zip(got, want)], want, hw)


@pytest.mark.parametrize("name", POOL_NAMES)
def test_problems_reproduce_the_host_selection(torch_dev, name):
    """side_effect_problems against earth_mover_distance's selection on the dense maps of
    side_effect_densities, at the pools' own spawn probability (no EMD is solved)."""
    from safelife_amd.side_effects import side_effect_densities, side_effect_problems
    init, final, _ = _episodes(name)
    H, W = init.shape[1:]
    kw = dict(rng="philox", seed=SEED, env_ids=IDS)
    dense = side_effect_densities(init, final, STEPS, 0.3, SAMPLES, **kw)
    probs = side_effect_problems(init, final, STEPS, 0.3, SAMPLES, **kw)
    assert len(probs) == N_EP
    zeros = np.zeros((H, W))
    cells = 0
    for e, (ina, act) in enumerate(dense):
        assert sorted(probs[e]) == sorted(set(ina) | set(act)), e
        for key, (p, q, ys, xs, mass) in probs[e].items():
            a, b = ina.get(key, zeros), act.get(key, zeros)
            gap = np.abs(a - b)
            yy, xx = np.nonzero(gap > 1e-3 * np.max(gap))
            assert np.array_equal(ys, yy) and np.array_equal(xs, xx), (e, key)
            assert ys.dtype == np.int32 and xs.dtype == np.int32
            assert np.array_equal(p, a[yy, xx]) and np.array_equal(q, b[yy, xx]), (e, key)
            assert _mass_close(mass, np.sum(a), H * W), (e, key, mass, np.sum(a))
            cells += len(yy)
    assert cells > 0


def test_device_problems_raise_the_max_keys_error(torch_dev):
    from safelife_amd.side_effects import side_effect_densities, side_effect_scores
    rng = np.random.RandomState(8)
    b = rng.randint(0, 65536, size=(1, 32, 32)).astype(np.uint16)
    args = (b, np.roll(b, 1, 2), [2], 0.3, 4)
    with pytest.raises(ValueError) as host:
        side_effect_densities(*args, rng="philox", seed=1, max_keys=8)
    with pytest.raises(ValueError) as dev:
        side_effect_scores(*args, rng="philox", seed=1, max_keys=8, problems="device")
    assert str(host.value) == str(dev.value)


# ----------------------------------------------------------------- episode log
def _logged(torch, dev, scoring, path):
    from safelife_amd import SafeLifeVecEnv, EpisodeLog, LevelPool
    pool = LevelPool.load(os.path.join(POOLS, "c2_append_still_25.npz"))
    B = 8
    venv = SafeLifeVecEnv(pool, B, dev, rng="philox", seed=21, time_limit=10,
                          view_shape=(15, 15), output_channels=None, penalty_coef=1.0,
                          min_performance=0.01)
    venv.reset()
    log = EpisodeLog(venv, log_file=path, num_samples=4, side_effect_seed=5, ring=8,
                     other_episode_data={"coef": 0.25}, scoring=scoring)
    assert ("board" in log._host) == (scoring == "host")
    assert ("start" in log._host) == (scoring == "host")
    rng = np.random.RandomState(6)
    for t in range(25):
        venv.step(torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev))
    records = log.close()
    return records


def test_episode_log_device_scoring_equals_host_scoring(torch_dev, tmp_path):
    torch, dev = torch_dev
    from safelife_amd.benchmarking import load_benchmarks
    paths = {s: str(tmp_path / ("%s.yaml" % s)) for s in ("host", "device")}
    host = _logged(torch, dev, "host", paths["host"])
    devr = _logged(torch, dev, "device", paths["device"])
    assert len(host) == len(devr) >= 16       # two time limits of 8 envs in 25 steps
    hw = 25 * 25
    scored = 0
    for n, (h, d) in enumerate(zip(host, devr)):
        assert list(h) == list(d), n
        for key in h:
            if key in ("start_board", "final_board"):
                assert h[key].dtype == d[key].dtype and np.array_equal(h[key], d[key]), (n, key)
            elif key != "side effects":
                assert h[key] == d[key] and type(h[key]) is type(d[key]), (n, key)
        _same_scores([d["side effects"]], [h["side effects"]], hw)
        scored += sum(v[0] > 0 for v in h["side effects"].values())
    assert scored > 0
    a, b = load_benchmarks(paths["host"]), load_benchmarks(paths["device"])
    assert sorted(a) == sorted(b) and len(a["length"]) == len(host)
    for key in a:
        if key != "side effects":
            assert np.array_equal(a[key], b[key]), key
    assert sorted(a["side effects"]) == sorted(b["side effects"])
    for cell, arr in a["side effects"].items():
        # (with num_samples = 4 every density is a multiple of 1/4 and the sums are exact
        # in any order, so the two-decimal text of the masses is the same as well)
        assert np.array_equal(arr, b["side effects"][cell]), cell
    assert open(paths["host"]).read() == open(paths["device"]).read()
