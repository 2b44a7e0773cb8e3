"""Cases of the tests that run every kernel family past a 2 GiB, 4 GiB (and, for f32 views,
8 GiB) tensor offset: shared by tests/test_big_batch_cpu.py, which checks by arithmetic and
on the oracle that each case does what it claims, and tests/test_gpu_big_batch.py, which
runs them on the device with the same seeds.

A case names a kernel family, a board shape, an env configuration, the tensor whose offsets
are under test with its bytes per env, and the boundaries (byte offsets from the tensor's
first element) it must cross.  B is derived: boundary // bytes_per_env + EXTRA, rounded up
to the family's env group (the four-envs-per-wave kernel; one case keeps a ragged tail).
For a boundary X the envs of interest are k - 1, k, k + 1 and B - 1 with k = X // bytes_per_env:
k - 1 is the last env wholly below X, k holds X (or starts at it, k - 1 and k then being
the envs either side), k + 1 is the next one.
"""
import ctypes
import os

import numpy as np

import feature_pools as fp
import obs_cases as oc

P31, P32, P33 = 1 << 31, 1 << 32, 1 << 33
EXTRA = 8                    # envs past the env that holds the largest boundary
PERIOD = 7                   # stand-alone views: env b holds state b % PERIOD
TWIN = 64                    # envs of a low-address twin of a slice of the batch
SLAB = 256 << 20             # bytes of output compared at a time
FOOTPRINT_CAP = 48 << 30     # a case's own tensors, by the table's arithmetic

POOLS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pools")
POOL_FILES = {"c5": ("c5_navigation_128.npz",), "c3": ("c3_prune_still_64.npz",),
              "c4c3": ("c4_append_still_64.npz", "c3_prune_still_64.npz")}
LEVEL_KEYS = ("board", "goals", "agent_loc", "orientation", "spawn_prob", "min_performance")


def batch_size(boundaries, env_bytes, group=1, ragged=0):
    B = max(boundaries) // env_bytes + EXTRA
    return -(-B // group) * group + ragged


def envs_of_interest(boundary, env_bytes, B):
    k = boundary // env_bytes
    return [k - 1, k, k + 1, B - 1]


# ------------------------------------------------------------- stand-alone observations
class ObsBig:
    """One sl_env_obs case: `small` is the PERIOD-env obs_cases.ObsCase whose states the B
    envs repeat; the output [B, view(, channels)] is the tensor under test."""

    def __init__(self, name, shape, view, mode, channels, offset, boundaries, seed):
        self.name, self.boundaries = name, tuple(boundaries)
        self.small = oc.ObsCase(name, shape, PERIOD, view, mode, channels, False, offset, seed)
        self.env_bytes = self.small.env_bytes
        self.B = batch_size(boundaries, self.env_bytes)

    @property
    def numel(self):
        return self.B * self.env_bytes // self.small.esz

    def interest(self):
        return {X: envs_of_interest(X, self.env_bytes, self.B) for X in self.boundaries}

    def footprint(self):
        """The env's own view tensor, the guarded output and a slab's comparison."""
        H, W = self.small.shape
        return self.B * (2 * self.env_bytes + 6 * H * W + STATE_BYTES) + 2 * SLAB

    def __repr__(self):
        return self.name


MAXV = int(round(oc.WAVE_MAX_CELLS ** 0.5))        # 64 x 64: the wave kernels' largest view
assert MAXV * MAXV == oc.WAVE_MAX_CELLS
ALL16 = tuple(range(16))
BENCH_VIEW, BENCH_CH = (33, 33), tuple(range(15))  # bench.py's views

OBS_CASES = [
    ObsBig("packed", (5, 9), (MAXV, MAXV), "packed", None, False, (P31, P32), 8101),
    ObsBig("chan-u8", (2, 2), (MAXV, MAXV), "uint8", ALL16, False, (P31, P32), 8102),
    ObsBig("chan-u16", (5, 9), (MAXV, MAXV), "uint16", ALL16, False, (P31, P32), 8103),
    ObsBig("chan-bf16", (2, 2), (MAXV, MAXV), "bfloat16", ALL16, False, (P31, P32), 8104),
    # 2^33 bytes of f32: where an int element index overflows
    ObsBig("chan-f32", (5, 9), (MAXV, MAXV), "float32", ALL16, False, (P31, P32, P33), 8105),
    # the LDS-staged fallback: the output starts one element past an aligned address
    ObsBig("fallback-f32", (2, 2), (MAXV, MAXV), "float32", (3, 0, 9, 14), True, (P31, P32), 8106),
    ObsBig("fallback-u8", (5, 9), (MAXV, MAXV), "uint8", (3, 0, 9, 14), True, (P31, P32), 8107),
    # the benchmark's f32 views: 65 340 bytes per env, the 16-byte head / tail split differs
    # from env to env
    ObsBig("bench-f32", (5, 9), BENCH_VIEW, "float32", BENCH_CH, False, (P31, P32), 8108),
]
OBS_KERNELS = {"packed": "wave-packed", "chan-u8": "chunk", "chan-u16": "chunk",
               "chan-bf16": "chunk", "chan-f32": "chunk", "fallback-f32": "fallback",
               "fallback-u8": "fallback", "bench-f32": "chunk"}
OBS_ENV_BYTES = {"packed": 8192, "chan-u8": 65536, "chan-u16": 131072, "chan-bf16": 131072,
                 "chan-f32": 262144, "fallback-f32": 65536, "fallback-u8": 16384,
                 "bench-f32": 65340}


def tiled_states(case):
    """The B states of a stand-alone case: state b % PERIOD of the small case's, stacked
    as SafeLifeVecEnv.set_state takes them; and the small case's own states."""
    st = oc.make_states(case.small)
    idx = np.arange(case.B) % PERIOD
    big = {k: st[k][idx] for k in ("board", "goals", "agent_x", "agent_y", "exit_count",
                                   "exit_y", "exit_x")}
    return big, st


# ----------------------------------------------------------------------- step families
# bytes per env of the state besides the three uint16 tensors and the planes: st_t (25
# tensors), planes_ok, and the step's own inputs and outputs (actions, reward, done, flags,
# ep_len, ep_rew, 8 scratch words)
STATE_BYTES = 248 + 4 + 86


def seg4_largest():
    """The largest shape sl_env_step_family answers small-seg4 for (most cells, then most
    rows), asked of the library itself."""
    from safelife_amd import _lib
    fam = _lib.lib().sl_env_step_family
    shapes = [(H * W, H, W) for H in range(2, 131) for W in range(2, 131)
              if fam(H, W, _lib.SL_KERNEL_FAST) == _lib.SL_FAMILY_SMALL_SEG4]
    return max(shapes)[1:]


class StepBig:
    """One step case.  `tensor` is "board" (board, goals and start board, H * W * 2 bytes per
    env each) or "views" (the step's view output); `plan` names what sl_env_step_plan must
    answer for it (SL_PLAN_* / SL_FAMILY_* names without the prefix)."""

    def __init__(self, name, family, kernel, shape, pool, tensor, boundaries, plan, seed,
                 view=(1, 1), channels=None, obs_dtype="uint16", compute_obs=False,
                 board_mode="auto", fuse128=False, rng="philox", group=1, ragged=0, T=12,
                 time_limit=4):
        self.name, self.family, self.kernel, self._shape = name, family, kernel, shape
        self.pool, self.tensor, self.boundaries, self.plan = pool, tensor, tuple(boundaries), plan
        self.seed, self.view, self.channels, self.obs_dtype = seed, view, channels, obs_dtype
        self.compute_obs, self.board_mode, self.fuse128, self.rng = compute_obs, board_mode, fuse128, rng
        self.group, self.ragged, self.T, self.time_limit = group, ragged, T, time_limit

    @property
    def shape(self):
        return seg4_largest() if self._shape == "seg4" else self._shape

    @property
    def mode(self):
        return "packed" if self.channels is None else self.obs_dtype

    @property
    def view_bytes(self):
        nch = len(self.channels) if self.channels else 1
        return self.view[0] * self.view[1] * nch * oc.ESZ[self.mode]

    @property
    def env_bytes(self):
        H, W = self.shape
        return H * W * 2 if self.tensor == "board" else self.view_bytes

    @property
    def B(self):
        return batch_size(self.boundaries, self.env_bytes, self.group, self.ragged)

    def interest(self):
        return {X: envs_of_interest(X, self.env_bytes, self.B) for X in self.boundaries}

    def anchors(self):
        """The envs handed to the oracle: every env of interest."""
        return sorted({e for es in self.interest().values() for e in es})

    def twins(self):
        """First global env id of each TWIN-env twin: around each boundary (from TWIN / 2
        envs before its first env of interest, or the batch's last TWIN envs where that
        would pass the end), and the batch's last TWIN envs.  Replay has none: a shard's draws start where all envs before it
        end, which only the whole batch knows."""
        if self.rng == "stream":
            return []
        los = [min(es[0] - TWIN // 2, self.B - TWIN) for es in self.interest().values()]
        return sorted(set(los + [self.B - TWIN]))

    def per_env_bytes(self):
        H, W = self.shape
        n = 6 * H * W + STATE_BYTES + self.view_bytes
        if (H, W) == (64, 64):
            n += 16384                               # planes: the goals mirror and the board
        if (H, W) == (128, 128):
            n += 65536 + (4096 if self.rng == "stream" else 0)
        return n

    def stream_draws(self):
        H, W = self.shape
        return min(self.B * H * W // 4, 1 << 28) if self.rng == "stream" else 0

    def footprint(self):
        return (self.B + TWIN * len(self.twins())) * self.per_env_bytes() + 8 * self.stream_draws()

    # ---- levels
    def level_dicts(self):
        if self.pool in POOL_FILES:
            out = []
            for f in POOL_FILES[self.pool]:
                with np.load(os.path.join(POOLS, f)) as d:
                    out += [{k: d[k][i] for k in LEVEL_KEYS} for i in range(d["board"].shape[0])]
            return out
        H, W = self.shape
        return fp.build_levels(3000 + self.seed, 4, H, W, 2)

    def env_kw(self):
        """Settings shared by SafeLifeVecEnv and OracleEnv."""
        return dict(time_limit=self.time_limit, view_shape=self.view, output_channels=self.channels,
                    penalty_coef=1.0, min_performance=0.01)

    def venv_kw(self):
        return dict(self.env_kw(), rng=self.rng, seed=self.seed, level_order="random",
                    augment_roll=True, kernel=self.kernel, obs_dtype=self.obs_dtype,
                    compute_obs=self.compute_obs, board_mode=self.board_mode,
                    fuse_channel_views128=self.fuse128)

    def actions(self, t):
        """Step t's actions of all B envs, keyed by the global env id."""
        return np.random.RandomState(self.seed * 1000 + t).randint(0, 9, size=self.B).astype(np.int32)

    def clock(self, e):
        """The episode clock env e (global id, or an array of them) starts with: staggered,
        so that every step resets a fifth of the batch and every env resets twice within T."""
        return e % (self.time_limit + 1)

    def oracle_env(self, levels, e, stream=None, cls=None):
        import oracle
        cls = cls or oracle.OracleEnv
        return cls(oracle.pool_level_fn(levels, e, seed=self.seed, n_total=self.B,
                                        random_order=True, augment=True),
                   env_id=e, rng=self.rng, seed=self.seed, stream=stream, **self.env_kw())

    def __repr__(self):
        return self.name


C3GRAY = dict(family="bits64", kernel="fast", shape=(64, 64), board_mode="planes")
STEP_CASES = [
    StepBig("bits128", "bits128", "fast", (128, 128), "c5", "board", (P31, P32),
            dict(family="BITS128", plane_mode=1, obs="NONE", resets="LIST128"), 31,
            board_mode="planes"),
    StepBig("bits128-replay", "bits128", "fast", (128, 128), "c5", "board", (P31,),
            dict(family="BITS128", plane_mode=1, obs="NONE", resets="LIST128", replay=1), 32,
            board_mode="planes", rng="stream"),
    StepBig("wide", "wide", "wide", (128, 127), "feature", "board", (P31,),
            dict(family="WIDE", obs="NONE", resets="SCAN"), 33),
    StepBig("generic", "generic", "generic", (128, 127), "feature", "board", (P31,),
            dict(family="GENERIC", obs="NONE", resets="SCAN"), 33),
    # C3, gray goals, no views: k_env_planes64_s6 + k_env_epilogue_reset64
    StepBig("bits64-planes-s6", pool="c3", tensor="board", boundaries=(P31,), seed=35,
            plan=dict(family="BITS64", plane_mode=1, kernel64="S6", keep="C3", obs="NONE",
                      resets="SPLIT_TAIL64"), **C3GRAY),
    # the C4 + C3 mix: every stored plane, coloured goals, k_env_reset_list
    StepBig("bits64-planes-all", "bits64", "fast", (64, 64), "c4c3", "board", (P31,),
            dict(family="BITS64", plane_mode=1, kernel64="PLANES", obs="NONE", resets="LIST64"),
            36, board_mode="planes"),
    # the kernel that steps on the uint16 board (k_env_step_bits64)
    StepBig("bits64-uint16", "bits64", "fast", (64, 64), "c4c3", "board", (P31,),
            dict(family="BITS64", plane_mode=0, kernel64="BITS64", obs="NONE", resets="LIST64"),
            37, board_mode="uint16"),
    StepBig("mid", "mid", "fast", (64, 62), "feature", "board", (P31,),
            dict(family="MID", obs="NONE", resets="IN_KERNEL"), 38),
    StepBig("small", "small", "fast", (32, 64), "feature", "board", (P31,),
            dict(family="SMALL", obs="NONE", resets="IN_KERNEL"), 39),
    StepBig("seg4", "small-seg4", "fast", "seg4", "feature", "board", (P31,),
            dict(family="SMALL_SEG4", obs="NONE", resets="IN_KERNEL"), 40, group=4),
    # ... and a batch whose last wave holds one env
    StepBig("seg4-tail", "small-seg4", "fast", "seg4", "feature", "board", (P31,),
            dict(family="SMALL_SEG4", obs="NONE", resets="IN_KERNEL"), 41, group=4, ragged=1),
    # ---- the view output past the boundary, the boards below it
    StepBig("planes64-chan-f32", "bits64", "fast", (64, 64), "c3", "views", (P31, P32),
            dict(family="BITS64", plane_mode=1, kernel64="CHAN", obs="FUSED64", resets="LIST64",
                 view_kind=4), 42, view=BENCH_VIEW, channels=BENCH_CH, obs_dtype="float32",
            compute_obs=True, board_mode="planes"),
    StepBig("planes64-packed", "bits64", "fast", (64, 64), "c3", "views", (P31,),
            dict(family="BITS64", plane_mode=1, kernel64="GRAY", obs="FUSED64", resets="LIST64",
                 view_kind=1), 43, view=BENCH_VIEW, compute_obs=True, board_mode="planes"),
    # k_env_bits128_chan + k_env_obs_reset_list_chan
    StepBig("bits128-chan-f32", "bits128", "fast", (128, 128), "c5", "views", (P31,),
            dict(family="BITS128", plane_mode=1, obs="FUSED128", resets="LIST128", view_kind=4),
            44, view=BENCH_VIEW, channels=BENCH_CH, obs_dtype="float32", compute_obs=True,
            board_mode="planes", fuse128=True),
    # the separate observation kernel after the step
    StepBig("wide-chan-u8", "wide", "wide", (65, 65), "feature", "views", (P31,),
            dict(family="WIDE", obs="SEPARATE", resets="SCAN"), 45, view=BENCH_VIEW,
            channels=BENCH_CH, obs_dtype="uint8", compute_obs=True),
]
STEP_ENV_BYTES = {"bits128": 32768, "bits128-replay": 32768, "wide": 32512, "generic": 32512,
                  "bits64-planes-s6": 8192, "bits64-planes-all": 8192, "bits64-uint16": 8192,
                  "mid": 7936, "small": 4096, "planes64-chan-f32": 65340,
                  "planes64-packed": 2178, "bits128-chan-f32": 65340, "wide-chan-u8": 16335}


# ------------------------------------------------------------------ the plan, on the host
_P = 0x7F0000001000          # a 16-byte aligned made-up "device" address


def host_plan(case):
    """sl_env_step_plan for a case on host-built structs, as SafeLifeVecEnv fills them from
    the case's pool (no GPU: the plan only tests pointers for NULL and alignment)."""
    from safelife_amd import _lib, vec_env as ve
    ds = case.level_dicts()
    board = np.stack([d["board"] for d in ds])
    goals = np.stack([d["goals"] for d in ds])
    al = np.stack([np.asarray(d["agent_loc"]) for d in ds])
    H, W = case.shape
    st = _lib.EnvState(B=case.B, H=H, W=W, board=_P, goals=_P + 0x100000,
                       start_board=_P + 0x200000)
    if (H, W) in ((64, 64), (128, 128)):
        st.planes, st.planes_ok = _P + 0x300000, _P + 0x400000
        st.board_zero = ve.zero_planes(int(np.bitwise_or.reduce(board.reshape(-1))))
    if (H, W) == (64, 64):
        st.board_planes = st.planes
        st.agent_planes = ve.agent_planes(board, al[:, 0] % W, al[:, 1] % H)
        st.goals_gray = ve.goals_gray(goals)
        st.derived_planes = ve.derived_planes(board)
    if (H, W) == (128, 128):
        st.board_planes = _P + 0x500000
        if case.rng == "stream":
            st.elig_planes = _P + 0x600000
    kernels = {"auto": _lib.SL_KERNEL_AUTO, "generic": _lib.SL_KERNEL_GENERIC,
               "fast": _lib.SL_KERNEL_FAST, "wide": _lib.SL_KERNEL_WIDE}
    c = _lib.EnvCfg(time_limit=case.time_limit, auto_reset=1, kernel=kernels[case.kernel],
                    rng_mode=_lib.SL_RNG_STREAM if case.rng == "stream" else _lib.SL_RNG_PHILOX,
                    scratch=_P + 0x700000, bonus_table=_P + 0x800000, bonus_len=H + W + 6,
                    bonus_period=4, planes64_waves=6,
                    board_mode=_lib.SL_BOARD_UINT16 if case.board_mode == "uint16"
                    else _lib.SL_BOARD_AUTO,
                    obs_fuse=_lib.SL_OBS_FUSE_CHAN128 if case.fuse128 else 0)
    if case.rng == "stream":
        c.draws, c.n_draws, c.stream_pos = _P + 0x900000, 64, _P + 0xA00000
    if case.compute_obs:
        modes = {"packed": _lib.SL_OBS_PACKED, "uint16": _lib.SL_OBS_CHANNELS,
                 "uint8": _lib.SL_OBS_CHANNELS_U8, "float32": _lib.SL_OBS_CHANNELS_F32,
                 "bfloat16": _lib.SL_OBS_CHANNELS_BF16}
        c.obs_out, c.obs_mode = _P + 0xB00000, modes[case.mode]
        c.obs_vh, c.obs_vw, c.obs_remove_white = case.view[0], case.view[1], 1
        c.obs_nch = len(case.channels or ())
        for k, ch in enumerate(case.channels or ()):
            c.obs_channels[k] = ch
    pl = _lib.LevelPool(K=len(ds), H=H, W=W, board=_P, goals=_P)
    out = _lib.StepPlan()
    rc = _lib.lib().sl_env_step_plan(ctypes.byref(st), ctypes.byref(pl), ctypes.byref(c), _P,
                                     ctypes.byref(out))
    assert rc == _lib.SL_OK, (case, rc)
    return out


def plan_facts(p):
    """An sl_step_plan as the names the cases use."""
    from safelife_amd import _lib

    def name(prefix, v):
        return next(k[len(prefix):] for k in dir(_lib) if k.startswith(prefix)
                    and getattr(_lib, k) == v)
    return dict(family=name("SL_FAMILY_", p.family), plane_mode=p.plane_mode, replay=p.replay,
                kernel64=name("SL_PLAN_K64_", p.kernel64), keep=name("SL_PLAN_KEEP_", p.keep),
                obs=name("SL_PLAN_OBS_", p.obs), resets=name("SL_PLAN_RESETS_", p.resets),
                view_kind=p.view_kind)
