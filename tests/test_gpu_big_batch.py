"""Every kernel family past a 2 GiB and a 4 GiB tensor offset (f32 views: 8 GiB, where an
int element index overflows as well), over the cases of tests/big_batch_cases.py.  The
rest of the suite stops short of 2^31 bytes in every tensor it compares; a byte offset or
an element index formed in 32 bits would corrupt exactly the envs above that line.

Stand-alone views (sl_env_obs: k_env_obs_packed, k_env_obs_channels<1|2|4>, k_env_obs):
the B states repeat with period 7, one observe() writes into a guarded buffer, the first
7 envs are compared with oracle.make_obs byte for byte and every later group of 7 with the
first, on the device, slab by slab: all B envs are checked, and the guards.

Step families: the whole B-env batch beside 64-env twins whose global env ids (env0,
n_total_envs) are those of a slice around each boundary and of the batch's end.  Philox
draws, level choice and rolls key on the global id, so a twin computes at low addresses --
the paths the small-B oracle tests pin -- what the slice must hold.  After every step:
rewards, dones, flags, board, goals, start board, views and every st_t key, torch.equal.
As an anchor that does not lean on the shard mechanism the envs of interest of every
boundary are also handed to oracle.OracleEnv (load_state) and followed ==.  Episode clocks
are staggered, so every step resets a fifth of the batch and every compared env resets at
least twice within T.  The replay case has no twins (a shard's draws start where all envs
before it end); its envs of interest take their draws at the offsets the scan left in
scratch [2B, 4B), as tests/test_gpu_bench_regime.py does.

Memory: the largest case holds 43 GB (the table's arithmetic: StepBig.footprint); a case
skips only when the device reports less free memory than 1.25 times its footprint.
Every comparison is ==, array_equal or torch.equal.
"""
import ctypes

import numpy as np
import pytest

import obs_cases as oc
import feature_pools as fp
import big_batch_cases as bb
from test_gpu_bench_regime import _OffsetStream
from test_gpu_headline import _env_state
from test_gpu_obs_matrix import FILL, blank_level, expected_bits, raw_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    import safelife_amd  # noqa: F401
    return torch, torch.device("cuda:0")


def _need(torch, case):
    """Skip when the device cannot hold the case (never on an MI355X with nothing else
    resident: the largest footprint is below 48 GiB)."""
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    want = case.footprint()
    assert want <= bb.FOOTPRINT_CAP
    free = torch.cuda.mem_get_info()[0]
    if free < 1.25 * want:
        pytest.skip("%s needs 1.25 x %d bytes, the device reports %d free" % (case, want, free))
    print("%s: B = %d, footprint %.2f GiB" % (case, case.B, want / 2.0 ** 30))


def _ints(torch, t):
    """A tensor's elements as signed integers of their own size (a view)."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# --------------------------------------------------------------- stand-alone observations
@pytest.mark.parametrize("case", bb.OBS_CASES, ids=[c.name for c in bb.OBS_CASES])
def test_observe_past_the_boundaries(torch_dev, case):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool
    _need(torch, case)
    small, B, P = case.small, case.B, bb.PERIOD
    venv = SafeLifeVecEnv(LevelPool.from_levels([blank_level(small.shape)]), B, dev,
                          view_shape=small.view, output_channels=small.channels,
                          obs_dtype="uint16" if small.mode == "packed" else small.mode,
                          remove_white_goals=small.remove_white, compute_obs=False)
    big, st = bb.tiled_states(case)
    venv.set_state(big["board"], big["goals"], big["board"],
                   **{k: big[k] for k in ("agent_x", "agent_y", "exit_count", "exit_y", "exit_x")})
    # an output like venv.obs inside a buffer of FILL bytes: at the buffer's start (16-byte
    # aligned) or one element in, and one guard element after it
    n, esz = venv.obs.numel(), venv.obs.element_size()
    assert esz == small.esz and n == case.numel and n * esz == B * case.env_bytes
    assert (B - 1) * case.env_bytes >= max(case.boundaries)
    raw = torch.full(((n + 2) * esz,), FILL, dtype=torch.uint8, device=dev).view(venv.obs.dtype)
    lo = 1 if small.offset else 0
    out = raw[lo:lo + n].view(venv.obs.shape)
    assert out.data_ptr() % 16 == small.out_shift
    got = venv.observe(out=out)
    torch.cuda.synchronize()
    assert got is out and venv._step_index == 0
    # 1. the first P envs against the oracle
    have, want = raw_bits(torch, out[:P]), expected_bits(small, st)
    assert have.shape == want.shape
    assert np.array_equal(have, want), (case, np.argwhere(have != want)[0])
    # 2. every later group of P envs against the first, slab by slab
    flat = _ints(torch, out).view(B, -1)
    ref = flat[:P]
    step = max(1, bb.SLAB // (P * case.env_bytes)) * P
    for b0 in range(P, B, step):
        chunk = flat[b0:min(b0 + step, B)]
        full = chunk.shape[0] // P
        groups = chunk[:full * P].view(full, P, -1)
        if not torch.equal(groups, ref.unsqueeze(0).expand_as(groups)):
            bad = (groups != ref.unsqueeze(0)).flatten(1).any(1).nonzero()[0].item()
            envs = (chunk[bad * P:bad * P + P] != ref).any(1).nonzero().flatten() + b0 + bad * P
            pytest.fail("%s: env %d (byte offset %d) differs from env %d" % (
                case, envs[0].item(), envs[0].item() * case.env_bytes, envs[0].item() % P))
        tail = chunk[full * P:]
        assert torch.equal(tail, ref[:tail.shape[0]]), (case, "the ragged last group")
    # 3. the guards
    fill = int.from_bytes(bytes([FILL]) * esz, "little")
    assert raw[lo + n:].numel() == 2 - lo
    assert (raw_bits(torch, raw[:lo]) == fill).all(), (case, "wrote before its output")
    assert (raw_bits(torch, raw[lo + n:]) == fill).all(), (case, "wrote past its output")


# ------------------------------------------------------------------------- step families
def _plan(venv):
    from safelife_amd import _lib
    cfg = venv._fill_cfg()
    venv._fill_obs_cfg(cfg, venv.obs if venv.compute_obs else None)
    out = _lib.StepPlan()
    rc = _lib.lib().sl_env_step_plan(ctypes.byref(venv._state),
                                     ctypes.byref(venv._pool_dev["struct"]), ctypes.byref(cfg),
                                     venv.flags.data_ptr(), ctypes.byref(out))
    assert rc == _lib.SL_OK
    return bb.plan_facts(out)


def _same_slice(torch, whole, twin, lo, ctx, views):
    hi = lo + twin.B
    for k in ("reward", "done", "flags", "ep_len", "ep_rew"):
        assert torch.equal(getattr(whole, k)[lo:hi], getattr(twin, k)), (ctx, k)
    assert torch.equal(whole.board[lo:hi], twin.board), (ctx, "board")
    assert torch.equal(whole.goals[lo:hi], twin.goals), (ctx, "goals")
    assert torch.equal(whole.start_board[lo:hi], twin.start_board), (ctx, "start_board")
    if views:
        assert torch.equal(_ints(torch, whole.obs[lo:hi]), _ints(torch, twin.obs)), (ctx, "views")
    for k in whole.st_t:
        assert torch.equal(whole.st_t[k][lo:hi], twin.st_t[k]), (ctx, k)


def _view_bits(case, o_obs):
    o_obs = np.asarray(o_obs).astype(np.int64)
    return o_obs if case.channels is None else o_obs * oc.ONE[case.mode]


@pytest.mark.parametrize("case", bb.STEP_CASES, ids=[c.name for c in bb.STEP_CASES])
def test_step_past_the_boundaries(torch_dev, case):
    torch, dev = torch_dev
    from safelife_amd import SafeLifeVecEnv, LevelPool
    _need(torch, case)
    B, T = case.B, case.T
    ds = case.level_dicts()
    pool, levels = LevelPool.from_levels(ds), fp.oracle_levels(ds)
    replay = case.rng == "stream"
    kw = case.venv_kw()
    stream = None
    if replay:
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        stream = torch.rand(case.stream_draws(), dtype=torch.float64, device=dev, generator=g)
        kw["spawn_stream"] = stream
    whole = SafeLifeVecEnv(pool, B, dev, **kw)
    twins = [(lo, SafeLifeVecEnv(pool, bb.TWIN, dev, env0=lo, n_total_envs=B, **kw))
             for lo in case.twins()]
    assert whole.kernel_family == case.family
    tensor = whole.obs if case.tensor == "views" else whole._board
    assert tensor.numel() * tensor.element_size() == B * case.env_bytes
    assert (B - 1) * case.env_bytes >= max(case.boundaries)
    for lo, v in [(0, whole)] + twins:
        v.reset()
        ids = torch.arange(lo, lo + v.B, device=dev, dtype=torch.int32)
        v.st_t["episode_length"].copy_(case.clock(ids))
    facts = _plan(whole)
    assert {k: facts[k] for k in case.plan} == case.plan, (case, facts)
    for lo, v in twins:
        assert _plan(v) == facts
        _same_slice(torch, whole, v, lo, (case, "reset", lo), case.compute_obs)
    # the oracle's envs: the state after the reset, which a fresh oracle env must share
    anchors, oenvs, ostreams = case.anchors(), {}, {}
    for e in anchors:
        ostreams[e] = _OffsetStream(stream) if replay else None
        o = case.oracle_env(levels, e, stream=ostreams[e])
        s = _env_state(whole, e)
        fresh = case.oracle_env(levels, e)
        fresh.reset()
        assert np.array_equal(s["board"], fresh.board) and np.array_equal(s["goals"], fresh.goals), e
        assert np.array_equal(s["start_board"], fresh.init_board), e
        o.load_state(s, whole._step_index)
        oenvs[e] = o
    resets = {e: 0 for e in anchors}
    slice_resets = torch.zeros(B, dtype=torch.int32, device=dev)
    n_draws = 0
    for t in range(T):
        acts = case.actions(t)
        a = torch.from_numpy(acts).to(dev)
        if replay:
            whole.stream_pos.zero_()
        vo, vr, vd, info = whole.step(a)
        for lo, v in twins:
            v.step(a[lo:lo + v.B])
            _same_slice(torch, whole, v, lo, (case, t, lo), case.compute_obs)
        slice_resets += info["reset"].to(torch.int32)
        rs, vr, vd = info["reset"].cpu().numpy(), vr.cpu().numpy(), vd.cpu().numpy()
        board, goals = whole.board, whole.goals
        if replay:
            offs = whole.scratch[2 * B:4 * B].cpu().numpy()
            end = int(whole.stream_pos.item())
            nxt = lambda k: int(offs[k]) if k < 2 * B else end          # noqa: E731
            for e in anchors:
                ostreams[e].arm(int(offs[2 * e]), int(offs[2 * e + 1]), nxt(2 * e + 2))
                n_draws += nxt(2 * e + 2) - int(offs[2 * e])
        for e in anchors:
            oo, r, dn, _ = oenvs[e].step(int(acts[e]))
            ctx = (case, t, e)
            resets[e] += int(rs[e])
            assert vr[e] == r, (ctx, vr[e], r)
            assert bool(vd[e]) == dn, ctx
            assert np.array_equal(board[e].cpu().numpy(), oenvs[e].board), ctx
            assert np.array_equal(goals[e].cpu().numpy(), oenvs[e].goals), ctx
            if case.compute_obs:
                assert np.array_equal(raw_bits(torch, vo[e]), _view_bits(case, oo)), ctx
            if replay:
                assert not ostreams[e].bounds, ("draws left unconsumed", ctx)
    assert min(resets.values()) >= 2, resets
    for lo, v in twins:
        assert int(slice_resets[lo:lo + v.B].min().item()) >= 2, (case, lo)
    if replay:
        assert not whole.stream_error() and n_draws > 0
