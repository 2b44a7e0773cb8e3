// sl_bits_mid.hip -- the bit-sliced fused env-step kernel for boards of 33 to 64 rows
// and 2 to 64 columns, 64x64 aside (40x40, 48x48, 50x50, 64x48, 35x64: sizes the
// proc-gen curricula and the interactive game use between the small kernel's 32 rows
// and the 64x64 kernels).
//
// Same semantics as k_env_step_small (sl_bits_small.hip), and so as k_env_action +
// k_env_step_generic (sl_env.hip); the layout is GeoMid's (sl_bits_geo.h):
//
//  * one wave64 per env; lane l = 2j + h holds the column pair (2j, 2j+1),
//    j < nl = ceil(W / 2), over rows 32h .. 32h+31, of which rows < H are real;
//  * the uint16 board stays in HBM and only changed rows are stored; no plane mode and
//    no fused views (sl_env_obs writes the views after the step);
//  * only the board is staged in LDS (rows of 64 u16, 128 H bytes: 8 KiB at most), for
//    the action, which runs on lane 0 against it (act_core<64>) and puts its edits
//    there before the rows become planes.  Goals and start board go from HBM straight
//    into the lanes' registers, one dword a row where W is even (two u16 where it is
//    odd): nothing reads them at random, and a stage for each would cost 24 KiB a wave
//    at 64 rows, two waves per SIMD fewer than the registers allow;
//  * scores, changed rows, epilogue and the reset of a finished env by its own wave
//    are the small kernel's.
// Philox draws, or the reference's stream order after a replay prologue
// (k_stream_prologue_mid).
#include "sl_bits_small.h"

using namespace sl;
using namespace sl::fast;
using namespace sl::bits;

namespace {

constexpr int kMinH = 33, kMaxH = 64, kMaxW = 64;

#ifndef SL_MID_MINW
#define SL_MID_MINW 3        // waves per SIMD the register budget is sized for
#endif

// (the row loads from HBM, hbm_rows, and mask_planes: sl_bits_small.h)

// Per-half OR of a row mask: the rows (bit y = row 32h + y) any lane of this lane's
// parity has set -- quad xor 2, then two row rotations keep the parity.  lo: rows 0-31,
// hi: rows 32-63 (both wave-uniform).
struct HalfRows {
    u32 lo, hi;
    __device__ __forceinline__ u32 any() const { return lo | hi; }
};
__device__ __forceinline__ HalfRows half_rows(u32 m) {
    u32 x = m | dpp<0x4E>(m);             // quad_perm [2,3,0,1]
    x |= dpp<0x124>(x);                   // row_ror:4
    x |= dpp<0x128>(x);                   // row_ror:8
    const auto rl = [x](int l) { return (u32)__builtin_amdgcn_readlane((int)x, l); };
    return HalfRows{rl(0) | rl(16) | rl(32) | rl(48), rl(1) | rl(17) | rl(33) | rl(49)};
}

// the rows of r (this lane's half) of the lane's column pair, from the dwords D
__device__ __forceinline__ void store_rows(uint16_t *t, const u32 D[32], HalfRows r, int h,
                                           bool active, bool odd_last, int W, int row0, int c0) {
    const u32 mine = h ? r.hi : r.lo, anyr = r.any();
    uint16_t *p = t + (active ? row0 * W + c0 : 0);
#pragma unroll
    for (int y = 0; y < 32; y++)
        if ((anyr >> y) & 1u) {                    // (wave-uniform: most rows are skipped)
            if (((mine >> y) & 1u) && active) {
                p[y * W] = (uint16_t)D[y];
                if (!odd_last) p[y * W + 1] = (uint16_t)(D[y] >> 16);
            }
        }
}

// MODE: SPAWN_PHILOX, or SPAWN_STREAM (replay: k_env_action has run the action and
// k_stream_prologue_mid sized the draws; the step reads act[b] and each tensor's first
// uniform from the scratch words)
template <int MODE>
__global__ void __launch_bounds__(64, SL_MID_MINW)
k_env_step_mid(SmallKArgs ka) {
    const sl_env_state &st = ka.st;
    const StepArgs &a = ka.a;
    const int32_t *__restrict__ actions = ka.actions;
    const int ctp = ka.ctp, ctc = ka.ctc;
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x, h = lane & 1, j = lane >> 1, row0 = 32 * h;
    const int H = st.H, W = st.W, nl = (W + 1) >> 1;
    // the board: H rows of 32 dwords (dynamic: 6 KiB at 48 rows)
    extern __shared__ __attribute__((aligned(16))) u32 dyn_stage[];
    lds_u32 *buf = (lds_u32 *)dyn_stage;
    const bool active = j < nl;
    GeoMid<MODE> geo = mid_geo<MODE>(lane, H, W);
    int64_t pos_b, pos_g;
    geo.src = stream_src<MODE>(a, ka.scratch, st.B, b, pos_b, pos_g);
    const int c0 = 2 * j, c1 = geo.odd_last ? 0 : 2 * j + 1;
    // valid cells per word: real rows of real columns
    const u32 wm0 = active ? geo.mh : 0u, wm1 = (active && !geo.odd_last) ? geo.mh : 0u;
    const u32 lm = wm0;       // ... of the loaded planes: the column-0 copy counts

    const int64_t off = b * (int64_t)H * W;
    const u32 V = load_record(st, actions, b, lane);
    u32 PB[32], PG[32];
    hbm_rows(st.goals + off, H, W, active, row0, c0, c1, PG);
    {
        const uint16_t *src[1] = {st.board + off};
        lds_u16 *dst[1] = {(lds_u16 *)dyn_stage};
        // rows of odd boards end in the column-0 copy; the rest of a row stays unread
        stage_tensors<1>(src, dst, H * W, W, lane);
    }

    const SpawnCtx sc = spawn_ctx(a, b, rec(V, R_SPAWN));

    // ---- goals: rule, then store the changed rows
    transpose32(PG);
    mask_planes(PG, lm);
    u32 cg[2];
    geo.pos = pos_g;
    rule_planes(PG, cg, geo, sc, 1u);
    const HalfRows rg = half_rows((cg[0] & wm0) | (cg[1] & wm1));
    u32 gcol[3][2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        gcol[k][0] = PL(PG, 9 + k, 0) & wm0;
        gcol[k][1] = PL(PG, 9 + k, 1) & wm1;
    }
    if (rg.any()) {
        transpose32(PG);
        store_rows(st.goals + off, PG, rg, h, active, geo.odd_last, W, row0, c0);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- board: the action reads the staged cells, then the rows become planes
    // (kept copy of the 64x64 kernels' action prologue: see step_env, sl_bits.hip)
    wait_lgkm();
    OverlayT<SmallCells> ov;
    ov.src.buf = buf;
    ov.n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        ov.idx[k] = 0;
        ov.val[k] = 0;
    }
    RecEnv env{st, b, rec(V, R_GO), rec(V, R_AX), rec(V, R_AY), rec(V, R_SCORE),
               rec(V, R_BASE), rec(V, R_POSS), rec_f64(V, R_MP)};
    int act_reward = 0;
    if (MODE == SPAWN_STREAM) {        // k_env_action ran the action (no edits left)
        act_reward = (int)scratch_of(ka.scratch, st.B).act[b];
    } else {
        if (lane == 0) act_reward = act_core<64>(env, rec(V, R_ACT), H, W, ctp, ctc, ov);
        act_reward = __builtin_amdgcn_readfirstlane(act_reward);
    }
    // the action's cell edits go straight into the staged board (lane 0; the wave's LDS
    // operations run in order, so the row reads below see them), the column-0 copy of
    // an odd board too; erow = the rows holding an edit, 64 of them here
    u32 elo = 0, ehi = 0;
    if (lane == 0) {
        lds_u16 *cells = (lds_u16 *)dyn_stage;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < ov.n) {
                const int i = ov.idx[k];
                cells[i] = (uint16_t)ov.val[k];
                if ((W & 1) && (i & 63) == 0) cells[i + W] = (uint16_t)ov.val[k];
                const int r = i >> 6;
                if (r < 32) elo |= 1u << r;
                else ehi |= 1u << (r - 32);
            }
    }
    elo = (u32)__builtin_amdgcn_readfirstlane((int)elo);
    ehi = (u32)__builtin_amdgcn_readfirstlane((int)ehi);
    const RecFields fl = rec_fields(a, V, __builtin_amdgcn_readfirstlane(env.go),
                                    __builtin_amdgcn_readfirstlane(env.ax),
                                    __builtin_amdgcn_readfirstlane(env.ay));
    lds_rows((const lds_u16 *)dyn_stage, H, active, j, PB, row0);
    // the start board's rows are on their way while the rule runs
    u32 PS[32];
    hbm_rows(st.start_board + off, H, W, active, row0, c0, c1, PS);
    transpose32(PB);
    u32 cb[2];
    geo.pos = pos_b;
    rule_planes(PB, cb, geo, sc, 0u);
    __builtin_amdgcn_sched_barrier(0);

    // ---- scores over the real cells of the new board and goals
    transpose32(PS);
#pragma unroll
    for (int p = 0; p < 16; p++) {
        PL(PB, p, 0) &= wm0;
        PL(PB, p, 1) &= wm1;
        PL(PS, p, 0) &= wm0;
        PL(PS, p, 1) &= wm1;
    }
    int pts, scr, pos, side;
    score_planes(PB, gcol, PS, &pts, &scr, &pos, &side);
    const ScoreTotals tot = score_totals(pts, scr, pos, side);
    __builtin_amdgcn_sched_barrier(0);

    // ---- changed rows, exits in the colour the epilogue gives them
    HalfRows rb = half_rows((cb[0] & wm0) | (cb[1] & wm1));
    rb.lo |= elo;
    rb.hi |= ehi;
    if (rb.any()) {
        (void)recolour_exits(PB, can_exit_now(fl.min_performance(), tot.score, fl.baseline(),
                                              tot.possible));
        transpose32(PB);
        store_rows(st.board + off, PB, rb, h, active, geo.odd_last, W, row0, c0);
    }
    int rs = 0;
    if (lane == 0) {
        const SmallKArgs &k = kargs();
        rs = epilogue_core(k.st, k.a, b, fl, act_reward, tot.points, tot.score, tot.possible,
                           tot.side, k.reward_out, k.done_out, k.flags_out, k.ep_len_out,
                           k.ep_rew_out)
                 ? 1 : 0;
    }
    rs = __builtin_amdgcn_readfirstlane(rs);
    if (rs) {
        const SmallKArgs &k = kargs();
        if (k.pool.K > 0) {
            wait_vm();         // this step's stores to the env have completed
            small_reset(k.st, k.pool, k.ra, b, lane);
        }
    }
}

// Replay-mode count of env b (SL_RNG_STREAM), one wave, after k_env_action (one lane
// per env) has applied the actions -- state and cell edits in HBM, rewards in scratch
// act[] -- so the board read here is the acted-on one: the eligible cells of the
// board and of the goals (scratch counts[2b], [2b+1]; sl_exclusive_scan_i64 turns them
// into each tensor's first uniform).  k_stream_prologue_small's work on GeoMid; nothing
// reads a cell at random here, so both tensors come straight from HBM.  A tensor without
// spawners is not read.
__global__ void __launch_bounds__(64)
k_stream_prologue_mid(SmallKArgs ka) {
    const sl_env_state &st = ka.st;
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x, h = lane & 1, j = lane >> 1;
    const int H = st.H, W = st.W, nl = (W + 1) >> 1;
    const bool active = j < nl;
    const int64_t off = b * (int64_t)H * W;
    const u32 V = load_record(st, ka.actions, b, lane);
    const Scratch w = scratch_of(ka.scratch, st.B);
    // no spawner in the tensor (spawn_flags, set at reset; toggling powers can make
    // one on the board): no draws
    const int spf = rec(V, R_SPF) | (ka.ctp ? 1 : 0);
    int n[2] = {0, 0};
    SpawnCtx sc{0u, 0u, 0ull, 0.0};
#pragma unroll
    for (int t = 0; t < 2; t++) {
        if ((spf >> t) & 1) {
            GeoMid<SPAWN_COUNT> geo = mid_geo<SPAWN_COUNT>(lane, H, W);
            u32 P[32];
            hbm_rows((t ? st.goals : st.board) + off, H, W, active, 32 * h, 2 * j,
                     geo.odd_last ? 0 : 2 * j + 1, P);
            __builtin_amdgcn_sched_barrier(0);
            transpose32(P);
            mask_planes(P, active ? geo.mh : 0u);
            __builtin_amdgcn_sched_barrier(0);
            u32 ch[2];
            rule_planes(P, ch, geo, sc, (u32)t);
            n[t] = wave_total(geo.count);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (lane == 0) {
        w.counts[2 * b] = n[0];
        w.counts[2 * b + 1] = n[1];
    }
}

}  // namespace

namespace sl {

bool mid_shape(int H, int W) {
    return H >= kMinH && H <= kMaxH && W >= 2 && W <= kMaxW && !(H == 64 && W == 64);
}

namespace {
// replay: the actions (k_env_action, one lane per env), then each env's eligible counts
int counts_mid(const StepCall &c) {
    const sl_env_state &st = *c.st;
    const int rc = launch_env_action(st, c.actions, c.ctp, c.ctc,
                                     scratch_of(c.fx.scratch, st.B).act, c.s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_stream_prologue_mid, dim3((unsigned)st.B), dim3(64), 0, c.s,
                       small_kargs(c));
    return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
}

int step_mid(const StepCall &c) {
    const sl_env_state &st = *c.st;
    const size_t lds = (size_t)st.H * 32 * sizeof(uint32_t);
    const dim3 grid((unsigned)st.B);
    if (c.plan.replay)
        hipLaunchKernelGGL(k_env_step_mid<SPAWN_STREAM>, grid, dim3(64), lds, c.s, small_kargs(c));
    else
        hipLaunchKernelGGL(k_env_step_mid<SPAWN_PHILOX>, grid, dim3(64), lds, c.s, small_kargs(c));
    return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
}
}  // namespace

const StepHooks &hooks_mid() {
    static const StepHooks h = {counts_mid, nullptr, step_mid, reset_scan, false};
    return h;
}

}  // namespace sl
