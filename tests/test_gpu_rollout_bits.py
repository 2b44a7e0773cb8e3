"""The bit-sliced side-effect rollout (sl_rollout_bits.hip) and the episode log on top of
it, against the oracle.  Everything is compared exactly: the density maps are integer
counts divided by num_samples in the same division, and the EMD is the same host code
on both sides.
"""
import importlib.util
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


def _planes64_helpers():
    spec = importlib.util.spec_from_file_location(
        "planes64_oracle_helpers", os.path.join(os.path.dirname(__file__),
                                                "test_gpu_planes64_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ boards
def _palette():
    """At most 40 cell values: every reference cell type (colours cycling through all
    eight), life in every colour, an agent, and cells with the bits 12-14 no type uses."""
    from safelife_amd.cell_types import CELL_TYPE_NAMES
    vals = []
    for n, (v, _) in enumerate(CELL_TYPE_NAMES[1:]):        # (empty is drawn separately)
        vals.append(int(v) | ((n % 8) << 9))
    vals += [9 | (c << 9) for c in range(8)]                # life x colours
    vals += [122, 122 | (2 << 9)]                           # the agent (player)
    vals += [16, 0x1000 | 9, 0x2000 | 16, 0x4000 | 1]      # plain wall; bits 12-14
    vals = sorted(set(vals))
    assert len(vals) <= 40
    return np.array(vals, dtype=np.uint16)


def _palette_boards(rng, E, H, W):
    pal = _palette()
    b = pal[rng.randint(0, len(pal), size=(E, H, W))]
    b[rng.rand(E, H, W) < 0.45] = 0
    return b.astype(np.uint16)


def _rolled(rng, init):
    return np.stack([np.roll(b, (rng.randint(3), rng.randint(3)), (0, 1)) for b in init])


def _check_vs_oracle(got, init, final, steps, sp, S, ids, seed=SEED):
    for e in range(len(init)):
        ina, act = oracle.side_effect_densities(init[e], final[e], int(steps[e]),
                                                np.float32(sp[e]), S, rng="philox", seed=seed,
                                                env_id=int(ids[e]))
        for nm, g, r in (("inaction", got[e][0], ina), ("action", got[e][1], act)):
            assert sorted(g) == sorted(r), (e, nm)
            for k in r:
                assert np.array_equal(g[k], r[k]), (e, nm, k)


STEPS = [0, 1, 3, 11, 0, 2, 6]
SPAWN = [0.0, 0.3, 1.0, 0.3, 1.0, 0.0, 0.3]
IDS = [3, 1000, 7, 65536, 12, 4000000000, 99]
SHAPES = [(2, 2), (2, 3), (7, 9), (25, 25), (26, 26), (32, 64), (31, 63), (64, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_fast_rollout_vs_oracle(torch_dev, shape):
    """kernel='fast' per episode against the oracle: num_steps 0 and up, env ids far
    apart, and the never / draw / always branches of the spawn draw; odd W (the column-0
    copy word), W = 2 (a lane that is its own neighbour), H = 32 and rows < 32."""
    from safelife_amd.side_effects import side_effect_densities
    H, W = shape
    rng = np.random.RandomState(100 * H + W)
    kinds = [_palette_boards(rng, 7, H, W)]
    if H <= 32 and W <= 32:        # any 16-bit cell: keys <= cells <= 1024
        kinds.append(rng.randint(0, 65536, size=(7, H, W)).astype(np.uint16))
    for init in kinds:
        final = _rolled(rng, init)
        got = side_effect_densities(init, final, STEPS, SPAWN, 9, rng="philox", seed=SEED,
                                    max_keys=1024, kernel="fast", env_ids=IDS)
        _check_vs_oracle(got, init, final, STEPS, SPAWN, 9, IDS)


def _pool_boards(name):
    if name == "spawners64":
        return _planes64_helpers()._spawner_pool().board
    return np.load(os.path.join(POOLS, name + ".npz"))["board"]


@pytest.mark.parametrize("name", ["c3_prune_still_64", "c4_append_still_64", "spawners64"])
def test_fast_equals_generic_on_pools(torch_dev, name):
    from safelife_amd.side_effects import side_effect_densities
    board = _pool_boards(name)
    E = 5
    init = np.ascontiguousarray(board[np.arange(E) % len(board)])
    rng = np.random.RandomState(4)
    final = _rolled(rng, init)
    steps, sp, ids = [0, 3, 11, 1, 6], [0.3] * E, [5, 6, 900, 2, 31]
    kw = dict(rng="philox", seed=SEED, env_ids=ids)
    fast = side_effect_densities(init, final, steps, sp, 9, kernel="fast", **kw)
    gen = side_effect_densities(init, final, steps, sp, 9, kernel="generic", **kw)
    for e in range(E):
        for f, g in zip(fast[e], gen[e]):
            assert sorted(f) == sorted(g), e
            for k in g:
                assert np.array_equal(f[k], g[k]), (e, k)
    _check_vs_oracle(fast, init, final, steps, sp, 9, ids)


def test_key_overflow_raises_on_both_kernels(torch_dev):
    from safelife_amd.side_effects import side_effect_densities
    rng = np.random.RandomState(8)
    b = rng.randint(0, 65536, size=(1, 32, 32)).astype(np.uint16)
    msgs = []
    for kernel in ("fast", "generic"):
        with pytest.raises(ValueError) as ei:
            side_effect_densities(b, np.roll(b, 1, 2), [2], 0.3, 4, rng="philox", seed=1,
                                  max_keys=8, kernel=kernel)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1]


@pytest.mark.parametrize("shape", [(128, 128), (33, 20)], ids=lambda s: "%dx%d" % s)
def test_forced_fast_raises_where_no_rollout_exists(torch_dev, shape):
    from safelife_amd.side_effects import side_effect_densities
    H, W = shape
    rng = np.random.RandomState(H)
    init = _palette_boards(rng, 2, H, W)
    final = _rolled(rng, init)
    args = (init, final, [1, 2], 0.3, 3)
    with pytest.raises(RuntimeError):
        side_effect_densities(*args, rng="philox", seed=2, kernel="fast")
    auto = side_effect_densities(*args, rng="philox", seed=2, kernel="auto", env_ids=[9, 4])
    gen = side_effect_densities(*args, rng="philox", seed=2, kernel="generic", env_ids=[9, 4])
    for e in range(2):
        for a, g in zip(auto[e], gen[e]):
            assert sorted(a) == sorted(g)
            for k in g:
                assert np.array_equal(a[k], g[k])
    _check_vs_oracle(auto, init, final, [1, 2], [0.3, 0.3], 3, [9, 4], seed=2)


class _Game:
    def __init__(self, init, board, num_steps, spawn_prob):
        self._init_data = {"board": init}
        self.board, self.num_steps, self.spawn_prob = board, num_steps, spawn_prob


def test_side_effect_scores_batch_equals_singles(torch_dev):
    from safelife_amd.side_effects import side_effect_scores, side_effect_score
    rng = np.random.RandomState(3)
    init = _palette_boards(rng, 4, 25, 25)
    final = _rolled(rng, init)
    steps, sp, ids = [2, 0, 5, 1], [0.3, 0.0, 1.0, 0.3], [40, 2, 77, 5]
    batch = side_effect_scores(init, final, steps, sp, 6, rng="philox", seed=SEED, env_ids=ids)
    assert len(batch) == 4
    for e in range(4):
        one = side_effect_score(_Game(init[e], final[e], steps[e], sp[e]), 6, rng="philox",
                                seed=SEED, env_ids=[ids[e]])
        assert one and one == batch[e], e


# ------------------------------------------------------------------ episode log
class _LoggedOracle(oracle.OracleEnv):
    """OracleEnv that keeps what log_episode would read, taken just before each reset."""

    def reset(self):
        if getattr(self, "episode_completed", False):
            completed, possible = self._perf_ratio()
            self.finished.append(dict(
                length=int(self.episode_length), reward=int(self.episode_reward),
                performance=[completed, possible, max(0.0, float(self.min_performance))],
                start=self.init_board.copy(), final=self.board.copy(),
                num_steps=int(self.num_steps), spawn_prob=float(self.spawn_prob)))
        return super().reset()


def _levels(pool):
    return [oracle.Level(pool.board[k], pool.goals[k], (pool.agent_x[k], pool.agent_y[k]),
                         pool.orientation[k], pool.spawn_prob[k], pool.min_performance[k])
            for k in range(pool.K)]


def _run_logged(torch, dev, pool, B, time_limit, T, ring, log_file=None, samples=20):
    from safelife_amd import SafeLifeVecEnv, EpisodeLog
    levels = _levels(pool)
    kw = dict(time_limit=time_limit, view_shape=(15, 15), output_channels=None,
              penalty_coef=1.0, min_performance=0.01)
    venv = SafeLifeVecEnv(pool, B, dev, rng="philox", seed=21, **kw)
    plain = SafeLifeVecEnv(pool, B, dev, rng="philox", seed=21, **kw)
    oenvs = []
    for e in range(B):
        o = _LoggedOracle(lambda ep, e=e: levels[(e + ep * B) % len(levels)], env_id=e,
                          rng="philox", seed=21, **kw)
        o.finished = []
        oenvs.append(o)
    venv.reset()
    plain.reset()
    for o in oenvs:
        o.reset()
    log = EpisodeLog(venv, log_file=log_file, num_samples=samples, side_effect_seed=5, ring=ring,
                     other_episode_data={"coef": 0.25})
    records = []
    rng = np.random.RandomState(6)
    for t in range(T):
        a = rng.randint(0, 9, size=B).astype(np.int32)
        at = torch.from_numpy(a).to(dev)
        if t == 17:                 # a flush by hand between the ones the ring forces
            records += log.flush()
        _, r1, d1, _ = venv.step(at)
        _, r2, d2, _ = plain.step(at)
        assert torch.equal(r1, r2) and torch.equal(d1, d2), t
        for e in range(B):
            oenvs[e].step(int(a[e]))
    records += log.close()
    assert venv._recorder is None
    assert np.array_equal(venv.board.cpu().numpy(), plain.board.cpu().numpy())
    assert np.array_equal(venv.goals.cpu().numpy(), plain.goals.cpu().numpy())
    return records, oenvs


def _check_records(records, oenvs, samples=20):
    from safelife_amd.side_effects import earth_mover_distance
    B = len(oenvs)
    by_env = {e: [r for r in records if r["env"] == e] for e in range(B)}
    assert sum(len(o.finished) for o in oenvs) == len(records) > B
    for e, o in enumerate(oenvs):
        assert len(by_env[e]) == len(o.finished), e
        for n, (rec, ref) in enumerate(zip(by_env[e], o.finished)):
            ctx = (e, n)
            assert rec["episode"] == n + 1, ctx
            assert rec["length"] == ref["length"], ctx
            assert rec["reward"] == ref["reward"], ctx
            assert rec["performance"] == ref["performance"], (ctx, rec["performance"])
            assert rec["initial green"] == int(np.sum((ref["start"] | 8) == (9 | 0x400))), ctx
            assert np.array_equal(rec["start_board"], ref["start"]), ctx
            assert np.array_equal(rec["final_board"], ref["final"]), ctx
            assert rec["num_steps"] == ref["num_steps"], ctx
            assert rec["other"] == {"coef": 0.25}, ctx
            ina, act = oracle.side_effect_densities(
                ref["start"], ref["final"], ref["num_steps"], np.float32(ref["spawn_prob"]),
                samples, rng="philox", seed=5, env_id=e)
            zeros = np.zeros(ref["start"].shape)
            want = {k: [earth_mover_distance(ina.get(k, zeros), act.get(k, zeros)),
                        np.sum(ina.get(k, zeros))] for k in set(ina) | set(act)}
            assert rec["side effects"] == want, ctx


def test_episode_log_c2_vs_oracle(torch_dev, tmp_path):
    torch, dev = torch_dev
    from safelife_amd import LevelPool
    from safelife_amd.benchmarking import load_benchmarks
    pool = LevelPool.load(os.path.join(POOLS, "c2_append_still_25.npz"))
    path = str(tmp_path / "log.yaml")
    # a ring of 4 steps forces flushes mid-run
    records, oenvs = _run_logged(torch, dev, pool, 6, 12, 40, ring=4, log_file=path)
    _check_records(records, oenvs)
    data = load_benchmarks(path)
    assert len(data["length"]) == len(records)
    assert sorted(data["length"].tolist()) == sorted(r["length"] for r in records)
    assert data["performance"].shape == (len(records), 3)
    assert open(path).read().count("# SafeLife benchmark data") == 1
    for arr in data["side effects"].values():
        assert arr.shape == (len(records), 2)


def test_episode_log_64_spawners_vs_oracle(torch_dev):
    torch, dev = torch_dev
    pool = _planes64_helpers()._spawner_pool()
    records, oenvs = _run_logged(torch, dev, pool, 4, 10, 40, ring=64)
    _check_records(records, oenvs)


def test_one_recorder_at_a_time(torch_dev, tmp_path):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool, EpisodeLog
    from safelife_amd.recorder import TrajectoryRecorder
    pool = LevelPool.load(os.path.join(POOLS, "c2_append_still_25.npz"))
    venv = SafeLifeVecEnv(pool, 2, dev, rng="philox", seed=1, time_limit=5,
                          output_channels=None)
    venv.reset()
    log = EpisodeLog(venv, record_side_effects=False)
    with pytest.raises(ValueError):
        TrajectoryRecorder(venv, str(tmp_path / "v{env}_{episode_num}"))
    with pytest.raises(ValueError):
        EpisodeLog(venv)
    log.close()
    rec = TrajectoryRecorder(venv, str(tmp_path / "v{env}_{episode_num}"))
    with pytest.raises(ValueError):
        EpisodeLog(venv)
    rec.close()
    noreset = SafeLifeVecEnv(pool, 2, dev, rng="philox", seed=1, auto_reset=False,
                             output_channels=None)
    with pytest.raises(ValueError):
        EpisodeLog(noreset)
