"""The EMD solved on the device (k_emd_cells, sl_emd_device.hip) against the host solver
(sl_emd_cells, through sl_emd_cells_batch, which returns exactly its values) on the same
arrays.  Every comparison is of the doubles' bits: the arithmetic around the transport is
the same IEEE operations in the same order, and the integer transport has one optimum.

Grids 5x7 (odd, where the wrap makes the ground distance asymmetric), 25x25 and 64x64;
cell counts 1, 2, 3, 17, 63, 64, 65, 200 and SL_EMD_DEVICE_MAX_CELLS of distinct cells --
on 5x7 the counts above its 35 cells do not exist, and 35 (every cell) runs instead.

No problem here may end at the pivot cap (status SL_EMD_ST_PIVOTS): a cap that swallowed
test problems would hide a wrong solver behind the host fallback.  ``_device`` asserts
that for every launch of this file, and that only the problems built to be too big fall
back by size.  It also prints the largest pivots / (n + m) it saw.
"""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
POOLS = os.path.join(GOLDEN, "pools")
pytestmark = pytest.mark.gpu

GRIDS = [(5, 7), (25, 25), (64, 64)]
COUNTS = [1, 2, 3, 17, 63, 64, 65, 200]          # and MAX_CELLS, appended in _random_bank
FORMS = ["p_heavier", "q_heavier", "equal_sums"]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _max_cells():
    from safelife_amd import _lib
    return _lib.SL_EMD_DEVICE_MAX_CELLS


def _cells(rng, H, W, c):
    cells = np.sort(rng.choice(H * W, c, replace=False))
    return (cells // W).astype(np.int32), (cells % W).astype(np.int32)


def _random_problem(rng, H, W, c, form):
    ys, xs = _cells(rng, H, W, c)
    if form == "equal_sums":
        # the same multiset of masses on two disjoint halves of the cells (the odd cell
        # out carries p == q): nothing pre-flows between the halves, the integer masses
        # are the same numbers on both sides, and no threshold column appears
        h = c // 2
        vals = 0.25 + rng.rand(h)
        p, q = np.zeros(c), np.zeros(c)
        order = rng.permutation(c)
        p[order[:h]] = vals
        q[order[h:2 * h]] = rng.permutation(vals)
        if c % 2:
            p[order[-1]] = q[order[-1]] = 0.5
        return p, q, ys, xs
    p, q = 0.1 + rng.rand(c), 0.1 + rng.rand(c)
    if form == "p_heavier":
        p *= 1.5 * q.sum() / p.sum()
    else:
        q *= 1.5 * p.sum() / q.sum()
    return p, q, ys, xs


def _pack(problems):
    """Concatenated p, q, ys, xs and the offsets of a list of (p, q, ys, xs)."""
    sizes = [len(pr[0]) for pr in problems]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)

    def cat(k, dt):
        return np.ascontiguousarray(np.concatenate(
            [np.asarray(pr[k], dtype=dt) for pr in problems] + [np.zeros(0, dt)]))
    return cat(0, np.float64), cat(1, np.float64), cat(2, np.int32), cat(3, np.int32), offsets


def _host(problems, H, W, penalty=1.0):
    from safelife_amd import _lib
    from safelife_amd.side_effects import ground_distance_table
    p, q, ys, xs, offsets = _pack(problems)
    out = np.zeros(len(problems))
    if len(problems):
        table = ground_distance_table(H, W)
        pad = [np.concatenate([a, np.zeros(1, a.dtype)]) for a in (p, q, ys, xs)]
        _lib.check(_lib.lib().sl_emd_cells_batch(
            *(a.ctypes.data for a in pad), offsets.ctypes.data, len(problems),
            table.ctypes.data, H, W, float(penalty), out.ctypes.data, 8), "batch")
    return out


def _device(torch, dev, problems, H, W, penalty=1.0, too_big=()):
    """(out, status) of one launch; asserts the cap and size conditions of this file."""
    from safelife_amd import _lib
    from safelife_amd.side_effects import (emd_cells_device, emd_problem_nodes,
                                           ground_distance_table)
    p, q, ys, xs, offsets = _pack(problems)
    table = torch.from_numpy(ground_distance_table(H, W)).to(dev)
    out, status = emd_cells_device(*(torch.from_numpy(a).to(dev) for a in (p, q, ys, xs, offsets)),
                                   table, penalty)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert out.dtype == np.float64 and status.dtype == np.int32
    assert out.shape == status.shape == (len(problems),)
    assert not (status == _lib.SL_EMD_ST_PIVOTS).any(), np.nonzero(status == -3)[0][:10]
    assert sorted(np.nonzero(status == _lib.SL_EMD_ST_TOOBIG)[0]) == sorted(too_big)
    nodes = emd_problem_nodes(p, q, offsets)
    ok = (status > 0) & (nodes > 0)
    if ok.any():
        ratio = status[ok] / nodes[ok]
        print("largest pivots/(n+m): %.3f (problem %d of %d, %d nodes)"
              % (ratio.max(), np.nonzero(ok)[0][ratio.argmax()], len(problems),
                 nodes[ok][ratio.argmax()]))
    return out, status


def _same_bits(got, want):
    bad = np.nonzero(got.view(np.int64) != want.view(np.int64))[0]
    assert len(bad) == 0, [(int(i), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]]


# ------------------------------------------------------------------ random problems
@pytest.fixture(scope="module", params=GRIDS, ids=lambda s: "%dx%d" % s)
def random_bank(request):
    """Per grid every count in every form, with the host's distances (penalty 1 and -1),
    computed once."""
    H, W = request.param
    rng = np.random.RandomState(100 * H + W)
    counts = [c for c in COUNTS + [_max_cells()] if c <= H * W]
    if H * W < COUNTS[-1]:
        counts.append(H * W)
    problems, labels = [], []
    for c in counts:
        for form in FORMS:
            problems.append(_random_problem(rng, H, W, c, form))
            labels.append((c, form))
    return H, W, problems, labels, _host(problems, H, W), _host(problems, H, W, -1.0)


def test_random_problems_are_the_forms_they_claim(random_bank):
    from safelife_amd.side_effects import emd_problem_nodes
    H, W, problems, labels, host, _ = random_bank
    assert len(problems) >= 15
    for (p, q, ys, xs), (c, form), h in zip(problems, labels, host):
        assert len(p) == c and len(set(zip(ys.tolist(), xs.tolist()))) == c
        if form == "p_heavier":
            assert p.sum() > q.sum()
        elif form == "q_heavier":
            assert q.sum() > p.sum()
        else:
            both = np.minimum(p, q)
            scale = 1e6 / max(p.sum(), q.sum())
            ip, iq = np.floor((p - both) * scale + 0.5), np.floor((q - both) * scale + 0.5)
            assert ip.sum() == iq.sum()
            # no threshold column: as many demand bins as supply bins
            assert emd_problem_nodes(p, q, [0, c])[0] == 2 * (c // 2)
        assert h > 0 or c == 1, (c, form)


def test_random_problems_equal_the_host(torch_dev, random_bank):
    torch, dev = torch_dev
    H, W, problems, labels, host, _ = random_bank
    out, status = _device(torch, dev, problems, H, W)
    for lab, o, h, s in zip(labels, out, host, status):
        print(lab, int(s), repr(float(o)), repr(float(h)))
    assert (status >= 0).all()
    _same_bits(out, host)


def test_extra_mass_penalty_minus_one(torch_dev, random_bank):
    torch, dev = torch_dev
    H, W, problems, labels, host, host_m1 = random_bank
    assert (host_m1 != host).any()
    out, status = _device(torch, dev, problems, H, W, penalty=-1.0)
    assert (status >= 0).all()
    _same_bits(out, host_m1)


# ---------------------------------------------------------------- degenerate cases
def _assignment(rng, H, W, k):
    """Unit masses on k cells against unit masses on k other cells: ties everywhere."""
    ys, xs = _cells(rng, H, W, 2 * k)
    side = rng.permutation(2 * k) < k
    return side.astype(float), (~side).astype(float), ys, xs


@pytest.fixture(scope="module")
def degenerate_bank():
    H, W = 25, 25
    rng = np.random.RandomState(5)
    problems, labels = [], []
    for k in (2, 31, 128):
        problems.append(_assignment(rng, H, W, k))
        labels.append("assignment%d" % k)
    p, q, ys, xs = _random_problem(rng, H, W, 40, "p_heavier")
    q[::3] = p[::3]                                        # the pre-flow removes both sides
    problems.append((p, q, ys, xs))
    labels.append("some_equal_bins")
    p, q, ys, xs = _random_problem(rng, H, W, 30, "p_heavier")
    problems.append((p, np.zeros(30), ys, xs))
    labels.append("q_zero")
    problems.append((p, p.copy(), ys, xs))
    labels.append("p_equals_q")
    problems.append((np.zeros(30), np.zeros(30), ys, xs))
    labels.append("all_zero")
    problems.append((np.array([0.75]), np.array([0.25]), ys[:1], xs[:1]))
    labels.append("one_cell")
    return H, W, problems, labels, _host(problems, H, W), _host(problems, H, W, -1.0)


def test_degenerate_problems_equal_the_host(torch_dev, degenerate_bank):
    torch, dev = torch_dev
    H, W, problems, labels, host, host_m1 = degenerate_bank
    want = dict(zip(labels, host))
    assert want["p_equals_q"] == 0.0 and want["all_zero"] == 0.0 and want["q_zero"] > 0.0
    assert want["one_cell"] == 0.5 and want["assignment128"] > 0.0
    assert len(problems[2][0]) == _max_cells()            # 128 against 128 fills the limit
    for penalty, ref in ((1.0, host), (-1.0, host_m1)):
        out, status = _device(torch, dev, problems, H, W, penalty=penalty)
        for lab, o, h, s in zip(labels, out, ref, status):
            print(penalty, lab, int(s), repr(float(o)), repr(float(h)))
        assert (status >= 0).all()
        _same_bits(out, ref)
        got = dict(zip(labels, status))
        # decided without a transport: no pivots
        assert got["q_zero"] == got["p_equals_q"] == got["all_zero"] == got["one_cell"] == 0
        assert got["assignment31"] > 0


# --------------------------------------------------------------------- batch shape
def test_no_problem_and_one_problem(torch_dev):
    torch, dev = torch_dev
    out, status = _device(torch, dev, [], 25, 25)
    assert out.shape == (0,)
    rng = np.random.RandomState(11)
    one = [_random_problem(rng, 25, 25, 9, "q_heavier")]
    out, status = _device(torch, dev, one, 25, 25)
    assert status[0] >= 0
    _same_bits(out, _host(one, 25, 25))
    out, status = _device(torch, dev, [(np.zeros(0),) * 2 + (np.zeros(0, np.int32),) * 2], 25, 25)
    assert out[0] == 0.0 and status[0] == 0 and not np.signbit(out[0])


def test_three_thousand_mixed_problems_in_one_launch(torch_dev):
    """Every third problem is empty; one problem recurs at several positions."""
    torch, dev = torch_dev
    H, W = 25, 25
    rng = np.random.RandomState(12)
    empty = (np.zeros(0), np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32))
    again = _random_problem(rng, H, W, 23, "p_heavier")
    at = [1, 64, 1000, 2999]
    problems = []
    for i in range(3000):
        if i in at:
            problems.append(again)
        elif i % 3 == 0:
            problems.append(empty)
        else:
            problems.append(_random_problem(rng, H, W, int(rng.randint(1, 41)),
                                            FORMS[int(rng.randint(3))]))
    out, status = _device(torch, dev, problems, H, W)
    assert (status >= 0).all()
    _same_bits(out, _host(problems, H, W))
    assert len(set(out[at].view(np.int64).tolist())) == 1 and out[at[0]] > 0
    assert len(set(status[at].tolist())) == 1
    assert (out[[i for i in range(0, 3000, 3) if i not in at]] == 0.0).all()


# ------------------------------------------------------------------------ fallback
def test_a_problem_above_the_limit_is_left_alone(torch_dev):
    from safelife_amd import _lib
    torch, dev = torch_dev
    H, W = 64, 64
    rng = np.random.RandomState(13)
    problems = [_random_problem(rng, H, W, c, "p_heavier") for c in (5, 12)]
    problems.append(_random_problem(rng, H, W, _max_cells() + 1, "p_heavier"))
    problems += [_random_problem(rng, H, W, c, "q_heavier") for c in (7, 1)]
    out, status = _device(torch, dev, problems, H, W, too_big=[2])
    assert status[2] == _lib.SL_EMD_ST_TOOBIG and out[2] == 0.0
    keep = [0, 1, 3, 4]
    assert (status[keep] >= 0).all()
    _same_bits(out[keep], _host([problems[i] for i in keep], H, W))


def test_a_cell_off_the_board_is_reported_not_read(torch_dev):
    """A row equal to H (and, in another problem, a negative column).  k_emd_cells checks
    every coordinate of a problem and leaves before its first table access (the loop over
    the cells ends in ``if (__any(bad)) ... return`` ahead of the maxC loop, the first
    reader of the table), so nothing is read outside the table."""
    from safelife_amd import _lib
    torch, dev = torch_dev
    H, W = 25, 25
    rng = np.random.RandomState(14)
    problems = [_random_problem(rng, H, W, c, "p_heavier") for c in (6, 70, 8, 9)]
    good = [problems[0], problems[3]]
    problems[1][2][69] = H
    problems[2][3][0] = -1
    from safelife_amd.side_effects import emd_cells_device, ground_distance_table
    p, q, ys, xs, offsets = _pack(problems)
    table = torch.from_numpy(ground_distance_table(H, W)).to(dev)
    out, status = emd_cells_device(*(torch.from_numpy(a).to(dev) for a in (p, q, ys, xs, offsets)),
                                   table)
    torch.cuda.synchronize()
    out, status = out.cpu().numpy(), status.cpu().numpy()
    assert status[1] == status[2] == _lib.SL_EMD_ST_BADCELL and out[1] == out[2] == 0.0
    assert status[0] >= 0 and status[3] >= 0
    _same_bits(out[[0, 3]], _host(good, H, W))


# ---------------------------------------------------------------------- end to end
LIFE = 1
STEPS, SAMPLES, SEED = 20, 20, 31


def _episodes(name):
    """Three levels of a pool; the final board is the start board without the six living
    cells nearest to its first one."""
    board = np.load(os.path.join(POOLS, name + ".npz"))["board"]
    init = np.ascontiguousarray(board[:3])
    final = init.copy()
    for b in final:
        yy, xx = np.nonzero((b & LIFE) != 0)
        near = np.argsort(np.abs(yy - yy[0]) + np.abs(xx - xx[0]), kind="stable")[:6]
        b[yy[near], xx[near]] = 0
    return init, final


@pytest.fixture(scope="module", params=["c3_prune_still_64", "c2_append_still_25"])
def rollouts(request, torch_dev):
    from safelife_amd.side_effects import side_effect_scores
    init, final = _episodes(request.param)
    kw = dict(rng="philox", seed=SEED, env_ids=[3, 50, 7], problems="device")
    host = side_effect_scores(init, final, [STEPS] * 3, 0.3, SAMPLES, emd="host", **kw)
    return init, final, kw, host


def _same_scores(got, want):
    assert len(got) == len(want)
    for e, (g, w) in enumerate(zip(got, want)):
        assert list(g) == list(w), e                      # key for key, in the same order
        for key in w:
            print(e, key, repr(g[key][0]), repr(w[key][0]))
            assert np.float64(g[key][0]).view(np.int64) == np.float64(w[key][0]).view(np.int64)
            assert np.float64(g[key][1]).view(np.int64) == np.float64(w[key][1]).view(np.int64)
            assert type(g[key][0]) is type(w[key][0]) and type(g[key][1]) is type(w[key][1])


def test_scores_with_the_device_emd_equal_the_host_emd(torch_dev, rollouts):
    from safelife_amd.side_effects import side_effect_scores
    init, final, kw, host = rollouts
    assert any(v[0] > 0 for h in host for v in h.values())
    dev = side_effect_scores(init, final, [STEPS] * 3, 0.3, SAMPLES, emd="device", **kw)
    _same_scores(dev, host)
    keys = sorted(set(k for h in host for k in h))
    assert len(keys) >= 2
    for sel in (dict(include=keys[::2] + [60000]), dict(exclude=keys[:1])):
        want = [{k: v for k, v in h.items()
                 if k in sel.get("include", keys) and k not in sel.get("exclude", ())}
                for h in host]
        got = side_effect_scores(init, final, [STEPS] * 3, 0.3, SAMPLES, emd="device", **kw, **sel)
        for g, w in zip(got, want):
            assert sorted(g) == sorted(w)
        assert [list(g) for g in got] == [
            list(h) for h in side_effect_scores(init, final, [STEPS] * 3, 0.3, SAMPLES,
                                                emd="host", **kw, **sel)]
        _same_scores([{k: g[k] for k in w} for g, w in zip(got, want)], want)


def test_python_fallback_solves_what_the_kernel_left(torch_dev, rollouts, monkeypatch):
    """The kernel's answer for every slot is replaced by "too many cells" (what a problem
    of more than SL_EMD_DEVICE_MAX_CELLS cells gets): the scores are then the host's."""
    from safelife_amd import _lib, side_effects
    init, final, kw, host = rollouts
    real = side_effects._emd_device_launch
    calls = []

    def too_big(p, q, ys, xs, offsets, nprob, table, H, W, penalty, out, status):
        real(p, q, ys, xs, offsets, nprob, table, H, W, penalty, out, status)
        calls.append(nprob)
        status.fill_(_lib.SL_EMD_ST_TOOBIG)
        out.fill_(float("nan"))                           # a value nobody may use

    monkeypatch.setattr(side_effects, "_emd_device_launch", too_big)
    got = side_effects.side_effect_scores(init, final, [STEPS] * 3, 0.3, SAMPLES, emd="device",
                                          **kw)
    assert calls == [3 * 64]
    _same_scores(got, host)


# --------------------------------------------------------------------- episode log
def _logged(torch, dev, emd, path):
    from safelife_amd import SafeLifeVecEnv, EpisodeLog, LevelPool
    pool = LevelPool.load(os.path.join(POOLS, "c2_append_still_25.npz"))
    B = 8
    venv = SafeLifeVecEnv(pool, B, dev, rng="philox", seed=21, time_limit=10,
                          view_shape=(15, 15), output_channels=None, penalty_coef=1.0,
                          min_performance=0.01)
    venv.reset()
    log = EpisodeLog(venv, log_file=path, num_samples=4, side_effect_seed=5, ring=8,
                     scoring="device", emd=emd)
    rng = np.random.RandomState(6)
    for t in range(12):
        venv.step(torch.from_numpy(rng.randint(0, 9, size=B).astype(np.int32)).to(dev))
    return log.close()


def test_episode_log_device_emd_equals_host_emd(torch_dev, tmp_path):
    torch, dev = torch_dev
    paths = {s: str(tmp_path / ("%s.yaml" % s)) for s in ("host", "device")}
    host = _logged(torch, dev, "host", paths["host"])
    devr = _logged(torch, dev, "device", paths["device"])
    assert len(host) == len(devr) >= 8
    _same_scores([d["side effects"] for d in devr], [h["side effects"] for h in host])
    assert sum(v[0] > 0 for h in host for v in h["side effects"].values()) > 0
    assert open(paths["host"]).read() == open(paths["device"]).read()
