"""CPU-side checks of the device-built EMD problems (no GPU): sl_emd_cells_batch against
a loop of sl_emd_cells, the argument checks of the four new entry points, their ctypes
signatures against the header, and the two new keywords' error paths."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "safelife_hip.h")
NEW = ("sl_side_effect_problems_workspace", "sl_side_effect_problem_counts",
       "sl_side_effect_problem_cells", "sl_emd_cells_batch")


@pytest.fixture(scope="module")
def lib():
    from safelife_amd import _lib
    _lib.build()
    return _lib.lib()


# ------------------------------------------------------------------ batch EMD
def _random_problems(H, W, seed):
    """About 40 problems: 0, 1, 2, ... up to 300 cells, empty ones first, in the middle
    and last; cells are distinct, row-major, masses non-negative with exact zeros."""
    rng = np.random.RandomState(seed)
    hw = H * W
    sizes = [0, 0, 1, 2, 3] + [int(rng.randint(0, min(hw, 120) + 1)) for _ in range(28)]
    sizes[len(sizes) // 2] = 0
    sizes += [min(hw, 300), min(hw, 299), 1, 0, 2, 0]
    p, q, ys, xs = [], [], [], []
    for n in sizes:
        cells = np.sort(rng.choice(hw, size=n, replace=False))
        a, b = rng.rand(n) * (rng.rand(n) < 0.7), rng.rand(n) * (rng.rand(n) < 0.7)
        p.append(a)
        q.append(b)
        ys.append(cells // W)
        xs.append(cells % W)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return (np.concatenate(p), np.concatenate(q), np.concatenate(ys).astype(np.int32),
            np.concatenate(xs).astype(np.int32), offs)


@pytest.fixture(scope="module", params=[(25, 25), (9, 21)], ids=["25x25", "9x21"])
def problems(request, lib):
    """The problems of one table with the single-call results, computed once."""
    from safelife_amd.side_effects import ground_distance_table
    H, W = request.param
    p, q, ys, xs, offs = _random_problems(H, W, seed=H * 100 + W)
    table = ground_distance_table(H, W)
    single = np.zeros(len(offs) - 1)
    for i in range(len(single)):
        lo, n = int(offs[i]), int(offs[i + 1] - offs[i])
        out = ctypes.c_double(-1.0)
        assert lib.sl_emd_cells(p[lo:].ctypes.data, q[lo:].ctypes.data, ys[lo:].ctypes.data,
                                xs[lo:].ctypes.data, n, table.ctypes.data, H, W, 1.0,
                                ctypes.byref(out)) == 0
        single[i] = out.value
    return H, W, p, q, ys, xs, offs, table, single


@pytest.mark.parametrize("nthreads", [1, 3, 16])
def test_batch_emd_equals_single_emd(lib, problems, nthreads):
    H, W, p, q, ys, xs, offs, table, single = problems
    nprob = len(offs) - 1
    assert 38 <= nprob <= 45 and offs[1] == 0 and offs[-1] == offs[-2]
    assert np.diff(offs).max() == min(H * W, 300) and (single > 0).sum() > 20
    out = np.full(nprob, -1.0)
    rc = lib.sl_emd_cells_batch(p.ctypes.data, q.ctypes.data, ys.ctypes.data, xs.ctypes.data,
                                offs.ctypes.data, nprob, table.ctypes.data, H, W, 1.0,
                                out.ctypes.data, nthreads)
    assert rc == 0
    assert np.array_equal(out.view(np.uint64), single.view(np.uint64))
    assert (out[np.diff(offs) == 0] == 0.0).all()


# ------------------------------------------------------------- argument checks
def _bufs():
    """Host buffers standing in for device memory: a rejected call must not touch them,
    and no call below may get past its checks."""
    return {k: np.zeros(64, dtype=np.float64) for k in
            ("ina", "act", "nk", "off", "mass", "ws", "p", "q", "ys", "xs")}


def _counts_args(b, **kw):
    a = dict(ina=b["ina"].ctypes.data, act=b["act"].ctypes.data, nk=b["nk"].ctypes.data, E=1,
             mk=4, H=2, W=3, off=b["off"].ctypes.data, mass=b["mass"].ctypes.data,
             ws=b["ws"].ctypes.data, wsb=9 * 8, stream=None)
    a.update(kw)
    return [a[k] for k in ("ina", "act", "nk", "E", "mk", "H", "W", "off", "mass", "ws", "wsb",
                           "stream")]


def _cells_args(b, **kw):
    a = dict(ina=b["ina"].ctypes.data, act=b["act"].ctypes.data, nk=b["nk"].ctypes.data, E=1,
             mk=4, H=2, W=3, off=b["off"].ctypes.data, p=b["p"].ctypes.data,
             q=b["q"].ctypes.data, ys=b["ys"].ctypes.data, xs=b["xs"].ctypes.data, cap=8,
             ws=b["ws"].ctypes.data, wsb=9 * 8, stream=None)
    a.update(kw)
    return [a[k] for k in ("ina", "act", "nk", "E", "mk", "H", "W", "off", "p", "q", "ys", "xs",
                           "cap", "ws", "wsb", "stream")]


BAD_SHAPES = [dict(E=-1), dict(H=1), dict(W=1), dict(H=256, W=129), dict(mk=0), dict(mk=1025),
              dict(wsb=9 * 8 - 1), dict(ws=None)]


def test_workspace_size_and_checks(lib):
    from safelife_amd import _lib
    n = ctypes.c_int64(-1)
    assert lib.sl_side_effect_problems_workspace(3, 4, ctypes.byref(n)) == _lib.SL_OK
    assert n.value == (2 * 12 + 1) * 8           # counts + trailing zero, thresholds
    assert lib.sl_side_effect_problems_workspace(0, 4, ctypes.byref(n)) == _lib.SL_OK
    for E, mk in ((-1, 4), (1, 0), (1, 1025)):
        assert lib.sl_side_effect_problems_workspace(E, mk, ctypes.byref(n)) == _lib.SL_EINVAL
    assert lib.sl_side_effect_problems_workspace(1, 4, None) == _lib.SL_EINVAL


def test_problem_counts_rejects_bad_arguments(lib):
    from safelife_amd import _lib
    b = _bufs()
    for bad in BAD_SHAPES + [dict(ina=None), dict(act=None), dict(nk=None), dict(off=None),
                             dict(mass=None)]:
        assert lib.sl_side_effect_problem_counts(*_counts_args(b, **bad)) == _lib.SL_EINVAL, bad
    # hw == 32768 passes the shape check (and then fails on the short workspace only)
    assert lib.sl_side_effect_problem_counts(*_counts_args(b, H=256, W=128, wsb=0)) \
        == _lib.SL_EINVAL
    assert lib.sl_side_effect_problem_counts(*_counts_args(b, E=0, wsb=8)) == _lib.SL_OK
    assert all((v == 0).all() for v in b.values())


def test_problem_cells_rejects_bad_arguments(lib):
    from safelife_amd import _lib
    b = _bufs()
    for bad in BAD_SHAPES + [dict(cap=-1), dict(ina=None), dict(act=None), dict(nk=None),
                             dict(off=None), dict(p=None), dict(q=None), dict(ys=None),
                             dict(xs=None)]:
        assert lib.sl_side_effect_problem_cells(*_cells_args(b, **bad)) == _lib.SL_EINVAL, bad
    assert lib.sl_side_effect_problem_cells(*_cells_args(b, E=0, wsb=8)) == _lib.SL_OK
    assert all((v == 0).all() for v in b.values())


def test_emd_batch_rejects_bad_arguments(lib):
    from safelife_amd import _lib
    from safelife_amd.side_effects import ground_distance_table
    table = ground_distance_table(3, 3)
    p, q = np.array([1.0, 0.0]), np.array([0.0, 1.0])
    ys, xs = np.array([0, 1], np.int32), np.array([0, 2], np.int32)
    offs, out = np.array([0, 2], np.int64), np.zeros(1)

    def call(**kw):
        a = dict(p=p.ctypes.data, q=q.ctypes.data, ys=ys.ctypes.data, xs=xs.ctypes.data,
                 offs=offs.ctypes.data, nprob=1, table=table.ctypes.data, H=3, W=3, pen=1.0,
                 out=out.ctypes.data, nthreads=2)
        a.update(kw)
        return lib.sl_emd_cells_batch(*[a[k] for k in (
            "p", "q", "ys", "xs", "offs", "nprob", "table", "H", "W", "pen", "out", "nthreads")])

    assert call() == _lib.SL_OK and out[0] > 0
    for bad in (dict(nthreads=0), dict(nthreads=-3), dict(nprob=-1), dict(p=None), dict(q=None),
                dict(ys=None), dict(xs=None), dict(offs=None), dict(table=None), dict(out=None),
                dict(H=0), dict(W=0)):
        assert call(**bad) == _lib.SL_EINVAL, bad
    # null pointers are rejected as well when no problem has a cell
    none = np.array([0, 0], np.int64)
    assert call(offs=none.ctypes.data) == _lib.SL_OK and out[0] == 0.0
    for name in ("p", "q", "ys", "xs", "table", "out"):
        assert call(offs=none.ctypes.data, **{name: None}) == _lib.SL_EINVAL, name
    down = np.array([2, 0], np.int64)
    assert call(offs=down.ctypes.data) == _lib.SL_EINVAL
    assert call(nprob=0, out=None, offs=None) == _lib.SL_OK
    # a cell outside the board is sl_emd_cells' own error, passed on
    far = np.array([0, 3], np.int32)
    assert call(ys=far.ctypes.data) == _lib.SL_EINVAL


# ------------------------------------------------------------------ signatures
_CTYPE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


def _header_signature(name):
    """ctypes argument types of `name` as include/safelife_hip.h declares it: every
    pointer is a void pointer (or POINTER(c_int64) where _lib passes byref)."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        if "*" in arg:
            out.append("pointer")
        else:
            out.append(_CTYPE[arg.replace("const ", "").rsplit(" ", 1)[0]])
    return out


def test_lib_declares_the_headers_signatures(lib):
    for name in NEW:
        fn = getattr(lib, name)
        want = _header_signature(name)
        assert fn.restype is ctypes.c_int, name
        assert len(fn.argtypes) == len(want), name
        for got, w in zip(fn.argtypes, want):
            if w == "pointer":
                assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, got)
            else:
                assert got is w, (name, got, w)


def test_header_cites_the_reference_lines():
    text = open(HEADER).read()
    for name in NEW[1:]:
        comment = text[:text.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "side_effects.py:36-56" in comment, name


# ------------------------------------------------------------------ key order
def _hand_made_problems(keys, present):
    """A _Problems of one 4x4 episode: key slot k holds k + 1 cells (mass k + 0.5)."""
    from safelife_amd.side_effects import _Problems
    n, mk = len(keys), len(keys) + 2
    pr = _Problems()
    pr.E, pr.H, pr.W, pr.max_keys = 1, 4, 4, mk
    pr.n_keys = np.array([n], np.int32)
    pr.keys = np.zeros((1, mk), np.uint16)
    pr.keys[0, :n] = keys
    pr.present = np.zeros((1, mk), np.int32)
    pr.present[0, :n] = present
    sizes = [k + 1 for k in range(n)] + [0, 0]
    pr.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pr.mass = np.array([k + 0.5 for k in range(n)] + [0.0, 0.0])
    cells = np.concatenate([np.arange(m) for m in sizes]).astype(np.int32)
    pr.ys, pr.xs = cells // 4, cells % 4
    rng = np.random.RandomState(2)
    pr.p, pr.q = rng.randint(0, 5, len(cells)) / 4.0, rng.randint(0, 5, len(cells)) / 4.0
    return pr


# found by search: with these keys (and the present bits below) a union of two sets grown
# key by key iterates in another order than the union of two sets sized from dicts
KEY_SETS = [
    [9, 521, 784, 1033, 1545, 1688, 2569, 3081, 3593, 32788],
    [9, 122, 529, 784, 1041, 1545, 2057, 3593],
    [1, 16, 17, 25, 122, 521, 529, 1041, 1545, 1553, 2057, 3593],
    [20758, 21244, 30404, 32104, 41994, 42614, 43568, 45892, 46885, 52417, 55027, 57044],
]


@pytest.mark.parametrize("keys", KEY_SETS, ids=lambda k: "%dkeys" % len(k))
def test_device_scores_list_keys_in_the_host_order(lib, keys):
    """The result dict's key order is what EpisodeLog writes under 'side effects:'.  The
    host path iterates set(ina) | set(act) of two dicts filled in slot order; a set built
    another way can iterate differently from about five keys on, so the device path's
    order is compared with that expression, with include and exclude as well."""
    from safelife_amd.side_effects import _scores_from_problems, emd_cells, \
        ground_distance_table
    present = [(1, 2, 3, 3, 2, 1, 3)[k % 7] for k in range(len(keys))]
    pr = _hand_made_problems(keys, present)
    ina = {int(k): None for k, b in zip(keys, present) if b & 1}
    act = {int(k): None for k, b in zip(keys, present) if b & 2}
    table = ground_distance_table(4, 4)
    for include, exclude in ((None, None), (keys[::2] + [7], None), (None, keys[1::3]),
                             (keys[1:], keys[4:6])):
        want = set(ina) | set(act)
        if include is not None:
            want &= set(include)
        if exclude is not None:
            want -= set(exclude)
        got, = _scores_from_problems(pr, include, exclude)
        assert list(got) == list(want), (include, exclude)
        assert len(got) >= 3
        for key, (emd, mass) in got.items():
            k = keys.index(key)
            lo, hi = pr.offsets[k], pr.offsets[k + 1]
            assert mass == k + 0.5
            assert emd == emd_cells(pr.p[lo:hi], pr.q[lo:hi], pr.ys[lo:hi], pr.xs[lo:hi], table)


def test_key_order_cases_tell_set_constructions_apart():
    """Every case above iterates differently when the sets are grown from generators
    instead of sized from dicts: the cases can see the difference."""
    differ = 0
    for keys in KEY_SETS:
        present = [(1, 2, 3, 3, 2, 1, 3)[k % 7] for k in range(len(keys))]
        ina = {int(k): None for k, b in zip(keys, present) if b & 1}
        act = {int(k): None for k, b in zip(keys, present) if b & 2}
        grown = (set(int(k) for k, b in zip(keys, present) if b & 1)
                 | set(int(k) for k, b in zip(keys, present) if b & 2))
        differ += list(set(ina) | set(act)) != list(grown)
    assert differ == len(KEY_SETS)


# -------------------------------------------------------------- keyword errors
def test_unknown_problems_keyword():
    from safelife_amd.side_effects import side_effect_score, side_effect_scores
    boards = np.zeros((1, 4, 4), np.uint16)
    with pytest.raises(ValueError, match="problems"):
        side_effect_scores(boards, boards, [1], 0.0, 2, problems="nope")

    class Game:
        _init_data = {"board": boards[0]}
        board, num_steps, spawn_prob = boards[0], 1, 0.0
    with pytest.raises(ValueError, match="problems"):
        side_effect_score(Game(), 2, problems="nope")


def test_unknown_scoring_keyword():
    from safelife_amd.episode_log import EpisodeLog

    class Env:
        auto_reset = True
        _recorder = None
    with pytest.raises(ValueError, match="scoring"):
        EpisodeLog(Env(), scoring="nope")
