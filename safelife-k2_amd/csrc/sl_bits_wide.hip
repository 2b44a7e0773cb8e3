// sl_bits_wide.hip -- the bit-sliced env-step kernel for the boards of up to 128 x 128
// that no other bit-sliced kernel takes: more than 64 rows or more than 64 columns,
// 128x128 aside (80x80, 96x96, 100x100, 40x128, 128x64).  Opt-in: SL_KERNEL_WIDE.
//
// Same semantics as k_env_step_generic (sl_env.hip), whose place in the generic family's
// launch sequence it takes: k_env_action has run before it (state and cell edits in HBM,
// the reward in scratch act[b]) and k_env_reset_scan follows it.  The layout is GeoWide's
// (sl_bits_geo.h), the 128x128 kernel's bands with the mid kernel's columns:
//
//  * one wave64 per env; lane j < nl = ceil(W / 2) holds the column pair (2j, 2j+1), for
//    odd W the last pair's word 1 is a copy of column 0; lanes >= nl hold no cells;
//  * the rows are NB = ceil(H / 32) bands of 32, processed in order: a band's 32 row
//    loads (one dword a lane a row where W is even, two u16 where it is odd; rows past H
//    repeat the last row and are cleared once the rows are planes), transposed into 16
//    planes x 2 words; the rule with the rows just outside the band as halo words; the
//    scores; the stores of the changed rows;
//  * every band sees the pre-step board: a band's upper halo is the previous band's last
//    row, kept from its load, its lower halo the next band's first row, not yet written;
//    band 0's upper halo is row H - 1, read up front, and the last band's lower halo row 0,
//    kept from band 0's load (at NB = 1 both come from the band itself);
//  * per band the goals advance first (their colour planes stay for the scores), then the
//    board; the start board is read band by band for the side-effect term, every cell bit
//    compared;
//  * uint16 board, goals and start board stay in HBM: no mirrors, no plane mode, no LDS;
//  * exits are rewritten by the epilogue after the row stores have completed.
// Philox draws only: replay (SL_RNG_STREAM) is SL_ETOOBIG in the plan.
#include "sl_bits_small.h"

using namespace sl;
using namespace sl::fast;
using namespace sl::bits;

namespace {

#ifndef SL_WIDE_MINW
#define SL_WIDE_MINW 3        // waves per SIMD the register budget is sized for
#endif

// the rows of `rows` (wave-uniform, bit y = row row0 + y < H) of the lane's column pair,
// from the dwords D
__device__ __forceinline__ void store_rows(uint16_t *t, const u32 D[32], u32 rows, int W,
                                           int row0, bool active, bool odd_last, int c0) {
    if (!(W & 1) && !((uintptr_t)t & 3)) {
        u32 *p = reinterpret_cast<u32 *>(t + row0 * W + c0);
        const u32 s = (u32)W >> 1;
#pragma unroll
        for (int y = 0; y < 32; y++)
            if ((rows >> y) & 1u) {                    // (wave-uniform: most rows are skipped)
                if (active) p[(u32)y * s] = D[y];
            }
    } else {
        uint16_t *p = t + row0 * W + c0;
#pragma unroll
        for (int y = 0; y < 32; y++)
            if ((rows >> y) & 1u) {
                if (active) {
                    p[(u32)(y * W)] = (uint16_t)D[y];
                    if (!odd_last) p[(u32)(y * W) + 1u] = (uint16_t)(D[y] >> 16);
                }
            }
    }
}

// The board's width, re-read from the kernel arguments where a band's row offsets are
// formed: left to itself the compiler forms the 32 offsets y W of every load and store
// phase once, ahead of the band loop, and holds them -- a hundred scalar registers,
// spilled -- through every rule.
__device__ __forceinline__ int width_now() { return kargs().st.W; }

// MODE: SPAWN_PHILOX
template <int MODE>
__global__ void __launch_bounds__(64, SL_WIDE_MINW)
k_env_step_wide(SmallKArgs ka) {
    const sl_env_state &st = ka.st;
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const int H = st.H, W = st.W, nl = (W + 1) >> 1, NB = (H + 31) >> 5;
    const bool active = lane < nl, odd_last = (W & 1) && lane == nl - 1;
    // (lanes past the board read column pair 0 and store nothing)
    const int c0 = active ? 2 * lane : 0, c1 = odd_last ? 0 : c0 + 1;
    const int64_t off = b * (int64_t)H * W;

    const u32 V = load_record(st, ka.actions, b, lane);
    const SpawnCtx sc = spawn_ctx(ka.a, b, rec(V, R_SPAWN));
    // the halo rows kept across the bands: the row above the next band, and row 0
    u32 upg = hbm_row(st.goals + off, W, H - 1, c0, c1);
    u32 upb = hbm_row(st.board + off, W, H - 1, c0, c1);
    u32 g0 = 0u, b0 = 0u;
    int points = 0, score = 0, possible = 0, side = 0;     // (wave-uniform)
#pragma unroll 1
    for (int t = 0; t < NB; t++) {
        const int row0 = 32 * t;
        // (the tensors' pointers are re-read per band, not held in SGPRs through the rule)
        const sl_env_state &ks = kargs().st;
        uint16_t *gb = ks.board + off, *gg = ks.goals + off;
        const uint16_t *gs = ks.start_board + off;
        const bool last_band = t == NB - 1;
        GeoWide<MODE> geo = wide_geo<MODE>(lane, H, W, row0);
        // valid cells per word: real rows of real columns; of the loaded planes the
        // column-0 copy counts (lm)
        const u32 lm = active ? geo.mh : 0u;
        const u32 wm0 = lm, wm1 = odd_last ? 0u : lm;
        const u32 real = (u32)__builtin_amdgcn_readfirstlane((int)geo.mh);

        // ---- goals: rule, then store the changed rows; their colours stay for the scores
        u32 gcol[3][2];
        {
            u32 G[32];
            hbm_rows(gg, H, width_now(), active, row0, c0, c1, G);
            const u32 dn = last_band ? 0u : hbm_row(gg, W, row0 + 32, c0, c1);
            if (t == 0) g0 = G[0];
            const u32 below = last_band ? g0 : dn, bottom = G[31];
            transpose32(G);
            mask_planes(G, lm);
            geo.hv = HaloView{active ? upg : 0u, active ? below : 0u};
            upg = bottom;
            u32 cg[2];
            rule_planes(G, cg, geo, sc, 1u);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                gcol[k][0] = PL(G, 9 + k, 0) & wm0;
                gcol[k][1] = PL(G, 9 + k, 1) & wm1;
            }
            const u32 rg = wave_or((cg[0] & wm0) | (cg[1] & wm1)) & real;
            if (rg) {
                transpose32(G);
                store_rows(gg, G, rg, width_now(), row0, active, odd_last, c0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);

        // ---- board: rule, scores against the goals' colours and the start board, then
        // the changed rows
        u32 P[32], S[32];
        hbm_rows(gb, H, width_now(), active, row0, c0, c1, P);
        const u32 dn = last_band ? 0u : hbm_row(gb, W, row0 + 32, c0, c1);
        // the start board's rows are on their way while the rule runs
        hbm_rows(gs, H, width_now(), active, row0, c0, c1, S);
        if (t == 0) b0 = P[0];
        const u32 below = last_band ? b0 : dn, bottom = P[31];
        transpose32(P);
        mask_planes(P, lm);
        geo.hv = HaloView{active ? upb : 0u, active ? below : 0u};
        upb = bottom;
        u32 cb[2];
        rule_planes(P, cb, geo, sc, 0u);
        __builtin_amdgcn_sched_barrier(0);

        transpose32(S);
#pragma unroll
        for (int p = 0; p < 16; p++) {
            PL(P, p, 0) &= wm0;
            PL(P, p, 1) &= wm1;
            PL(S, p, 0) &= wm0;
            PL(S, p, 1) &= wm1;
        }
        int pts, scr, pos, sde;
        score_planes(P, gcol, S, &pts, &scr, &pos, &sde);
        const ScoreTotals tot = score_totals(pts, scr, pos, sde);
        points += tot.points;
        score += tot.score;
        possible += tot.possible;
        side += tot.side;
        __builtin_amdgcn_sched_barrier(0);

        const u32 rb = wave_or((cb[0] & wm0) | (cb[1] & wm1)) & real;
        if (rb) {
            transpose32(P);
            store_rows(gb, P, rb, width_now(), row0, active, odd_last, c0);
        }
    }
    // the epilogue's inputs, loaded now (in flight with the row stores) rather than held
    // through the bands: the action's reward, the record again (L2) and the bonus term
    const SmallKArgs &k = kargs();
    const int act_reward = (int)scratch_of(k.scratch, k.st.B).act[b];
    const u32 VE = load_record(k.st, k.actions, b, lane_now());
    const RecFields fl = rec_fields(k.a, VE, rec(VE, R_GO), rec(VE, R_AX), rec(VE, R_AY));
    wait_vm();              // row stores land before the epilogue rewrites the exits
    if (lane_now() == 0)
        (void)epilogue_core(k.st, k.a, b, fl, act_reward, points, score, possible, side,
                            k.reward_out, k.done_out, k.flags_out, k.ep_len_out, k.ep_rew_out);
}

}  // namespace

namespace sl {

bool wide_shape(int H, int W) {
    return H >= 2 && H <= 128 && W >= 2 && W <= 128 && (H > 64 || W > 64) &&
           !(H == 128 && W == 128);
}

namespace {
// the action of every env ahead of the step kernel, one lane each (k_env_action)
int action_wide(const StepCall &c) {
    const sl_env_state &st = *c.st;
    return launch_env_action(st, c.actions, c.ctp, c.ctc, scratch_of(c.fx.scratch, st.B).act, c.s);
}

int step_wide(const StepCall &c) {
    hipLaunchKernelGGL(k_env_step_wide<SPAWN_PHILOX>, dim3((unsigned)c.st->B), dim3(64), 0, c.s,
                       small_kargs(c));
    return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
}
}  // namespace

// (no replay: plan_step answers SL_RNG_STREAM with SL_ETOOBIG, so `counts` is never called)
const StepHooks &hooks_wide() {
    static const StepHooks h = {nullptr, action_wide, step_wide, reset_scan, false};
    return h;
}

}  // namespace sl
