// sl_bits_small.h -- what the one-wave-per-env step kernels with the uint16 board in
// HBM share (sl_bits_small.hip: boards up to 32 rows; sl_bits_mid.hip: 33 to 64 rows;
// sl_bits_wide.hip: past 64 rows or columns): the LDS stage of a tensor as rows of 64 u16,
// the row loads from HBM, the kernels' argument struct, and the reset of a finished env by
// its own wave.
#pragma once
#include "sl_bits_geo.h"
#include "sl_env_step.h"

namespace sl {
namespace bits {

typedef __attribute__((address_space(3))) u32 lds_u32;
typedef __attribute__((address_space(3))) const uint16_t lds_cu16;

// unedited cells for the action, from the staged board: row y is 32 dwords, and the
// action indexes cell (y, x) as y * 64 + x (act_core<64>)
struct SmallCells {
    const lds_u32 *buf;
    __device__ __forceinline__ uint32_t operator()(int i) const {
        return reinterpret_cast<lds_cu16 *>(buf)[i];
    }
};

// Board, goals and start board are staged in LDS as rows of 64 u16 (cell (y, x) at
// y * 64 + x), each tensor read by the whole wave with coalesced u16 loads (cells
// lane + 64 k), eight per lane and tensor in flight at once.  For odd W column 0 is
// also written at x = W, so the last lane's second word reads as its copy.
constexpr int kGroup = 8;

template <int NTEN = 3>
__device__ __forceinline__ void stage_tensors(const uint16_t *const src[NTEN],
                                              lds_u16 *const dst[NTEN], int HW, int W, int lane) {
    const int dy = 64 / W, dx = 64 - dy * W;
    int y = lane / W, x = lane - (lane / W) * W;
    for (int i0 = lane; i0 < HW; i0 += 64 * kGroup) {
        uint32_t v[NTEN][kGroup];
        int pos[kGroup];
#pragma unroll
        for (int g = 0; g < kGroup; g++) {
            const int i = i0 + 64 * g;
            pos[g] = -1;
            if (i < HW) {
#pragma unroll
                for (int t = 0; t < NTEN; t++) v[t][g] = src[t][i];
                pos[g] = y * 64 + x + ((x == 0 && (W & 1)) ? 0x10000 : 0);
            }
            y += dy;
            x += dx;
            if (x >= W) {
                x -= W;
                y++;
            }
        }
#pragma unroll
        for (int g = 0; g < kGroup; g++)
            if (pos[g] >= 0) {
                const int p = pos[g] & 0xFFFF;
#pragma unroll
                for (int t = 0; t < NTEN; t++) {
                    dst[t][p] = (uint16_t)v[t][g];
                    if (pos[g] >> 16) dst[t][p + W] = (uint16_t)v[t][g];    // column-0 copy
                }
            }
    }
}

// the lane's dwords D[y] = cell(row0 + y, 2j) | cell(row0 + y, 2j + 1) << 16 of a staged
// tensor (0 outside the board); row0 = 0 where a lane holds every row
__device__ __forceinline__ void lds_rows(const lds_u16 *t, int H, bool active, int j, u32 D[32],
                                         int row0 = 0) {
    const lds_u32 *p = reinterpret_cast<const lds_u32 *>(t) + row0 * 32 + j;
#pragma unroll
    for (int y = 0; y < 32; y++) D[y] = (active && row0 + y < H) ? p[y * 32] : 0u;
}

// The lane's dwords D[y] = cell(row0 + y, c0) | cell(row0 + y, c1) << 16 of a tensor in
// HBM (t: the env's cells, row stride W).  c1 = c0 + 1, or 0 for the column-0 copy of an
// odd board.  Even W with t on a dword boundary: one load a row.  No load is predicated
// (32 predicates would cost the kernel its scalar registers): rows past the board
// repeat its last row and lanes past it read column pair 0, and the caller clears
// what is no cell once the rows are planes (mask_planes).
__device__ __forceinline__ void hbm_rows(const uint16_t *__restrict__ t, int H, int W,
                                         bool active, int row0, int c0, int c1, u32 D[32]) {
    const int last = min(32, H - row0) - 1;            // this half's last real row, >= 0
    const int a0 = active ? c0 : 0, a1 = active ? c1 : 0;
    if (!(W & 1) && !((uintptr_t)t & 3)) {
        const u32 *p = reinterpret_cast<const u32 *>(t + row0 * W + a0);
        const int s = W >> 1;
#pragma unroll
        for (int y = 0; y < 32; y++) D[y] = p[min(y, last) * s];
    } else {
        const uint16_t *p = t + row0 * W;
#pragma unroll
        for (int y = 0; y < 32; y++) {
            const int r = min(y, last) * W;
            D[y] = (u32)p[r + a0] | ((u32)p[r + a1] << 16);
        }
    }
}
// both words of every plane to the lane's real rows (m = 0 for a lane past the board)
__device__ __forceinline__ void mask_planes(u32 P[32], u32 m) {
#pragma unroll
    for (int k = 0; k < 32; k++) P[k] &= m;
}

// all kernel arguments in one struct at kernarg offset 0: the epilogue re-reads its
// ~20 pointers where it runs (kargs()), so they are not held in SGPRs through the step
struct SmallKArgs {
    sl_env_state st;
    StepArgs a;
    const int32_t *actions;
    int ctp, ctc;
    double *reward_out;
    uint8_t *done_out, *flags_out;
    int32_t *ep_len_out, *ep_rew_out;
    sl_level_pool pool;       // auto-reset source (K == 0: no reset here)
    ResetArgs ra;
    int64_t *scratch;         // sl_env_cfg.scratch (replay mode: act, offsets, err)
};

// a call's arguments; the pool only where the step kernel itself resets finished envs
inline SmallKArgs small_kargs(const StepCall &c) {
    sl_level_pool pool = c.fx.pool;
    if (c.plan.resets != SL_PLAN_RESETS_IN_KERNEL) pool.K = 0;
    return SmallKArgs{*c.st, c.a, c.actions, c.ctp, c.ctc, c.reward, c.done, c.flags, c.ep_len,
                      c.ep_rew, pool, c.fx.ra, c.fx.scratch};
}

__device__ __forceinline__ const SmallKArgs &kargs() {
    auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return *(const SmallKArgs *)kp;
}

// SafeLifeEnv.reset (safelife_env.py:188-198) of env b by its own wave, right after
// the step that ended the episode (ContinuingEnv + run_agents' reset-on-done): the
// same result as reset_one (sl_env.hip).  Pass 1 sums points / baseline / possible
// over the level (a roll permutes cells, so the level's own order is used) and lists
// the exits of the ROLLED board in np.nonzero order (row-major chunks of 64 cells, a
// ballot prefix count within a chunk); pass 2 copies the rolled level into board
// (exits coloured), goals and start board.
__device__ __forceinline__ void small_reset(const sl_env_state &st, const sl_level_pool &pool,
                                            const ResetArgs &ra, int64_t b, int lane) {
    const int H = st.H, W = st.W, hw = H * W;
    int li = 0, dy = 0, dx = 0;
    if (lane == 0) {
        const LevelChoice c = choose_level(pool, ra, ra.env0 + (uint32_t)b, st.episodes[b], H, W);
        li = c.idx;
        dy = c.dy;
        dx = c.dx;
    }
    li = __builtin_amdgcn_readfirstlane(li);
    dy = __builtin_amdgcn_readfirstlane(dy);
    dx = __builtin_amdgcn_readfirstlane(dx);
    const uint16_t *lb = pool.board + (int64_t)li * hw, *lg = pool.goals + (int64_t)li * hw;
    const int dy64 = 64 / W, dx64 = 64 - dy64 * W;
    const uint64_t below = (1ull << lane) - 1ull;
    int p = 0, q = 0, r = 0, spb = 0, n_exit = 0;
    {
        int y = lane / W, x = lane - (lane / W) * W;
        for (int i0 = 0; i0 < hw; i0 += 64) {
            const int i = i0 + lane;
            bool ex = false;
            if (i < hw) {
                const int src = fast::wrap1(y - dy, H) * W + fast::wrap1(x - dx, W);
                const uint32_t vb = lb[src], vg = lg[src];
                int pp, qq, rr;
                cell_scores(vb, vg, &pp, &qq, &rr);
                p += pp;
                q += qq;
                r += rr;
                spb |= ((vb & SPAWN) ? 1 : 0) | ((vg & SPAWN) ? 2 : 0);
                ex = (vb & EXIT) != 0;
            }
            const uint64_t m = __ballot(ex);
            const int rank = __builtin_popcountll(m & below);
            if (ex && n_exit + rank < SL_MAX_EXITS) {
                st.exit_y[b * SL_MAX_EXITS + n_exit + rank] = (int16_t)y;
                st.exit_x[b * SL_MAX_EXITS + n_exit + rank] = (int16_t)x;
            }
            n_exit += __builtin_popcountll(m);
            y += dy64;
            x += dx64;
            if (x >= W) {
                x -= W;
                y++;
            }
        }
    }
    p = wave_total(p);
    q = wave_total(q);
    r = wave_total(r);
    spb = (int)wave_or((u32)spb);
    int ev = 0;
    if (lane == 0) {
        ev = reset_scalars(st, pool, ra, b, li, dy, dx, p, q, r, spb);
        st.exit_count[b] = n_exit;
        for (int e = n_exit; e < SL_MAX_EXITS; e++) {
            st.exit_y[b * SL_MAX_EXITS + e] = 0;
            st.exit_x[b * SL_MAX_EXITS + e] = 0;
        }
    }
    ev = __builtin_amdgcn_readfirstlane(ev);
    const int64_t off = b * (int64_t)hw;
    uint16_t *gb = st.board + off, *gg = st.goals + off, *gs = st.start_board + off;
    int y = lane / W, x = lane - (lane / W) * W;
    for (int i = lane; i < hw; i += 64) {
        const int src = fast::wrap1(y - dy, H) * W + fast::wrap1(x - dx, W);
        const uint16_t vb = lb[src];
        gs[i] = vb;
        gb[i] = (vb & EXIT) ? (uint16_t)ev : vb;
        gg[i] = lg[src];
        y += dy64;
        x += dx64;
        if (x >= W) {
            x -= W;
            y++;
        }
    }
}

}  // namespace bits
}  // namespace sl
