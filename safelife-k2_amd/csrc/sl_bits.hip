// sl_bits.hip -- the bit-sliced fused env-step kernel for 64x64 boards.
//
// Same semantics as k_env_action + k_env_step_generic (sl_env.hip); different data
// layout, chosen for CDNA4's VALU-issue limit:
//
//  * one wave64 per env; lane l owns the column pair (2j, 2j+1), j = l >> 1, for
//    the 32-row half h = l & 1 (rows 32h .. 32h+31);
//  * each lane loads its 32 dwords D[y] = cell(32h+y, 2j) | cell(32h+y, 2j+1) << 16
//    (every load instruction covers two full 128-byte rows) and transposes them in
//    registers (32x32 bit transpose: 2 v_perm stages + 3 bfi stages, 256 VALU
//    ops), giving 16 bit planes x 2 words: plane k, word w, bit y = bit k of
//    cell(32h + y, 2j + w);
//  * the rule (advance_board.c:34-120) is then evaluated as
//    bitwise logic on 32 cells per operation: vertical neighbours are funnel
//    shifts (v_alignbit) against the other half's word (DPP quad_perm lane swap),
//    horizontal neighbours are the lane's other word or a 2-lane whole-wave DPP
//    rotation (wave_ror:1 / wave_rol:1, wrapping at W = 64), the 3x3 alive count
//    is a bit-sliced adder and the >= 2 tests are majority functions -- about
//    120 VALU ops per 32 cells against ~1300 for the packed two-cells-per-register
//    form;
//  * points, performance score, possible score and side effects
//    (safelife_game.py:590-631, env_wrappers.py:319-342) are recomputed in full
//    every step from the new planes with bitwise masks and v_bcnt;
//  * the new planes are transposed back and only the rows that changed are
//    stored (a wave-wide OR of the per-column change masks picks them).
// The action (execute_action / move_agent, safelife_game.py:308-393) runs on lane
// 0 while the column loads are in flight; its cell edits are broadcast and
// written into the planes before the rule.  Envs that finish are queued; a second
// kernel (k_env_reset_list) resets exactly those, one wave each, so the step
// kernel carries no reset code (128 VGPRs, 4 waves/SIMD, no spills).  The <true>
// instantiation also writes the packed observation (write_obs, 130 VGPRs, 3 waves).
#include "sl_bits_geo.h"
#include "sl_env_step.h"
#include "sl_action4.h"

using namespace sl;
using namespace sl::fast;
using namespace sl::bits;

namespace {

constexpr int kMinWaves = 4;      // waves per SIMD the register budget is sized for
constexpr int kMinWavesObs = 3;   // the same for the instantiations that write views or
                                  // replay the reference stream

constexpr int N = 64;        // rows = columns = lanes

// ---------------------------------------------------------------- LDS staging
// A wave's 8 KiB LDS buffer holds one 64x64 board, row-major, with the 16-byte
// chunks of rows 32..63 rotated by 4 chunks so that the even (rows 0..31) and odd
// (rows 32..63) lanes of a column-pair read fall in different banks.
typedef __attribute__((address_space(3))) u32 lds_u32;

__device__ __forceinline__ void dma_board(const uint16_t *__restrict__ src, lds_u32 *buf,
                                          int lane) {
    const char *s = reinterpret_cast<const char *>(src);
#pragma unroll
    for (int k = 0; k < 8; k++) {          // 8 x (64 lanes x 16 B), LDS chunk q = 64k + lane
        const int q = k * 64 + lane, row = q >> 3, pos = q & 7;
        const int c = (pos - ((row >> 5) << 2)) & 7;
        __builtin_amdgcn_global_load_lds((const void *)(s + row * 128 + c * 16),
                                         (__attribute__((address_space(3))) void *)(buf + k * 256),
                                         16, 0, 2);
    }
}

// the lane's 32 dwords (rows 32h + y, column pair j) from the staged board
__device__ __forceinline__ void read_pairs(const lds_u32 *buf, int lane, u32 D[32]) {
    const int h = lane & 1, j = lane >> 1;
    const lds_u32 *p = buf + h * 1024 + ((j + 16 * h) & 31);
#pragma unroll
    for (int y = 0; y < 32; y++) D[y] = p[y * 32];
}

// The start-board planes the side-effect term needs (0, 2, 7-15), from the level
// pool's precomputed bit planes: the start board of an env reset from the pool is
// level li rolled by (dy, dx) (sl_env_state.start_roll).  Column c of the start
// board is level column c - dx; its 64-bit row column rotated by dy gives rows
// 32h .. 32h+31 as one funnel shift.  The pool stays in L2 / the Infinity Cache,
// so this costs no HBM traffic and no transpose.  The level's planes 0-3 and 6-15
// (7 KiB, seven 1 KiB DMA rows) are copied into the wave's board buffer as soon as
// the board has been read out of it, so their (queueing-dominated) latency runs
// under the action and the rule (issued at scoring time, it was ~40% of a wave's
// life; held in registers instead, it spills).
// KEEP: the planes any board (and so any start board) can hold; a row whose two planes
// the scores do not need (1, 3, 6 are never read) or no board holds is not copied
// PACK: the copied rows lie one after the other in LDS (the six-wave kernel's 6 KiB
// buffer: KEEP 0x877F copies 5 of the 7 rows, 5 KiB), not each in its own slot
constexpr int pool_row_plane(int k) { return k < 2 ? 2 * k : 2 * k + 2; }   // row k: planes p0, p0 + 1
constexpr bool pool_row_copied(u32 keep, int k) {
    return (((keep & 0xFF85u) >> pool_row_plane(k)) & 3u) != 0u;             // planes 0, 2, 7-15
}
constexpr int pool_row_slot(u32 keep, bool pack, int k) {
    if (!pack) return k;
    int n = 0;
    for (int i = 0; i < k; i++) n += pool_row_copied(keep, i) ? 1 : 0;
    return n;
}
// dwords of LDS the copied rows take
constexpr int pool_rows_dwords(u32 keep, bool pack) {
    int top = 0;
    for (int k = 0; k < 7; k++)
        if (pool_row_copied(keep, k)) top = pool_row_slot(keep, pack, k) + 1;
    return top * 256;
}
template <u32 KEEP = 0xFFFFu, bool PACK = false>
__device__ __forceinline__ void pool_dma(const sl_level_pool &pool, int li, lds_u32 *buf,
                                         int lane) {
    const char *pl = reinterpret_cast<const char *>(pool.board_planes + (int64_t)li * 16 * N);
    constexpr u32 need = KEEP & 0xFF85u;         // planes 0, 2, 7-15
#pragma unroll
    for (int k = 0; k < 7; k++) {       // LDS row k <- planes (0,1), (2,3), (6,7) .. (14,15)
        const int p0 = k < 2 ? 2 * k : 2 * k + 2;
        if (!((need >> p0) & 3u)) continue;
        const int slot = PACK ? pool_row_slot(KEEP, true, k) : k;
        __builtin_amdgcn_global_load_lds((const void *)(pl + p0 * N * 8 + lane * 16),
                                         (__attribute__((address_space(3))) void *)(buf + slot * 256),
                                         16, 0, 0);
    }
}
template <u32 KEEP = 0xFFFFu>
__device__ __forceinline__ void pool_planes_lds(const lds_u32 *buf, int dy, int dx, int lane,
                                                u32 S[32]) {
    const int c0 = (2 * (lane >> 1) - dx) & 63, c1 = (c0 + 1) & 63;
    const int r = (32 * (lane & 1) - dy) & 63;
    const bool lo_first = r < 32;
    const u32 sh = (u32)(r & 31);
#pragma unroll
    for (int p = 0; p < 16; p++) {
        if (p == 1 || (p >= 3 && p <= 6) || !((KEEP >> p) & 1u)) {
            PL(S, p, 0) = 0u;
            PL(S, p, 1) = 0u;
            continue;
        }
        const int slot = p < 4 ? p : p - 2;             // LDS plane slot
        const lds_u32 *q = buf + slot * 128;            // 64 columns x 2 dwords
        const u32 a0 = q[2 * c0], a1 = q[2 * c0 + 1], b0 = q[2 * c1], b1 = q[2 * c1 + 1];
        PL(S, p, 0) = lo_first ? __builtin_amdgcn_alignbit(a1, a0, sh)
                               : __builtin_amdgcn_alignbit(a0, a1, sh);
        PL(S, p, 1) = lo_first ? __builtin_amdgcn_alignbit(b1, b0, sh)
                               : __builtin_amdgcn_alignbit(b0, b1, sh);
    }
}
// The same from pool_dma<KEEP, true>'s packed rows, for the column word W alone (the
// other word of S is left as it is): the six-wave kernel scores one word at a time.
template <u32 KEEP, int W>
__device__ __forceinline__ void pool_planes_lds_word(const lds_u32 *buf, int dy, int dx,
                                                     int lane, u32 S[32]) {
    const int c = (2 * (lane >> 1) + W - dx) & 63;
    const int r = (32 * (lane & 1) - dy) & 63;
    const bool lo_first = r < 32;
    const u32 sh = (u32)(r & 31);
#pragma unroll
    for (int p = 0; p < 16; p++) {
        if (p == 1 || (p >= 3 && p <= 6) || !((KEEP >> p) & 1u)) {
            PL(S, p, W) = 0u;
            continue;
        }
        const int row = p < 4 ? p >> 1 : (p >> 1) - 1;                  // pool_dma's row k
        const int slot = 2 * pool_row_slot(KEEP, true, row) + (p & 1);  // LDS plane slot
        const lds_u32 *q = buf + slot * 128;            // 64 columns x 2 dwords
        const u32 a0 = q[2 * c], a1 = q[2 * c + 1];
        PL(S, p, W) = lo_first ? __builtin_amdgcn_alignbit(a1, a0, sh)
                               : __builtin_amdgcn_alignbit(a0, a1, sh);
    }
}

// A uint16 board through a buffer of 4 KiB (the six-wave kernel's): two passes of 32 rows,
// each DMA'd to the start of the buffer (row-major, no rotation: within a half the 32
// lanes that read it take 32 consecutive dwords of each row) and read by the lanes of
// that half -- read_pairs' dwords.  A DMA's data is waited for (vmcnt) before it is read,
// and a half's reads are retired (lgkmcnt) before the next DMA overwrites it, the
// caller's earlier reads of the buffer included.
__device__ __forceinline__ void board_pairs_halves(const uint16_t *__restrict__ src, lds_u32 *buf,
                                                   int lane, u32 D[32]) {
    const int h = lane & 1, j = lane >> 1;
    // the lane's source offset, computed here: shared with the kernel's first DMAs it is
    // held from there through the rule, and at 80 registers spilled round the draw loop
    int l16 = lane * 16;
    asm volatile("" : "+v"(l16));
    const char *s = reinterpret_cast<const char *>(src) + l16;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        wait_lgkm();
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < 4; k++)        // 4 x (64 lanes x 16 B): rows 32 half + 8k .. + 7
            __builtin_amdgcn_global_load_lds((const void *)(s + half * 4096 + k * 1024),
                                             (__attribute__((address_space(3))) void *)(buf + k * 256),
                                             16, 0, 2);
        wait_vm();
        if (h == half) {
#pragma unroll
            for (int y = 0; y < 32; y++) D[y] = buf[y * 32 + j];
        }
    }
    wait_lgkm();
}


// unedited cells for the action, from the staged board (dma_board's layout)
typedef __attribute__((address_space(3))) const uint16_t lds_cu16;
struct LdsCells {
    const lds_u32 *buf;
    __device__ __forceinline__ uint32_t operator()(int i) const {
        const int row = i >> 6, col = i & 63;
        const int pos = ((col >> 3) + ((row >> 5) << 2)) & 7;
        return reinterpret_cast<lds_cu16 *>(buf)[row * 64 + pos * 8 + (col & 7)];
    }
};

// The action's cell edits (wave-uniform (flat index, value) pairs) written into the
// planes on the lane holding each cell; returns the row pairs (bit y: rows y, y + 32)
// holding an edit, whose stores are then forced.
__device__ __forceinline__ u32 mux_edits(u32 P[32], int ne, const int eidx[4], const u32 eval[4],
                                         int lane) {
    u32 erow = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < ne) {
            const int y = eidx[k] >> 6, x = eidx[k] & 63;
            const int tl = 2 * (x >> 1) + (y >> 5);            // lane holding the cell
            const u32 bit = 1u << (y & 31);
            const u32 m0 = (lane == tl && !(x & 1)) ? bit : 0u;
            const u32 m1 = (lane == tl && (x & 1)) ? bit : 0u;
            erow |= bit;
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const u32 v = ((eval[k] >> p) & 1u) ? ~0u : 0u;
                PL(P, p, 0) = mux(m0, v, PL(P, p, 0));
                PL(P, p, 1) = mux(m1, v, PL(P, p, 1));
            }
        }
    }
    return erow;
}
// The same for the plane step's four fixed slots (sl_action4.h): slot k is written where bit
// k of `changed` is set; the four cells are distinct, so the order does not matter.
__device__ __forceinline__ void mux_edits4(u32 P[32], u32 changed, const int eidx[4],
                                           const u32 eval[4], int lane) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if ((changed >> k) & 1u) {
            const int y = eidx[k] >> 6, x = eidx[k] & 63;
            const int tl = 2 * (x >> 1) + (y >> 5);            // lane holding the cell
            const u32 bit = 1u << (y & 31);
            const u32 m0 = (lane == tl && !(x & 1)) ? bit : 0u;
            const u32 m1 = (lane == tl && (x & 1)) ? bit : 0u;
#pragma unroll
            for (int p = 0; p < 16; p++) {
                const u32 v = ((eval[k] >> p) & 1u) ? ~0u : 0u;
                PL(P, p, 0) = mux(m0, v, PL(P, p, 0));
                PL(P, p, 1) = mux(m1, v, PL(P, p, 1));
            }
        }
    }
}

// SafeLifeEnv.reset (safelife_env.py:188-198) of env b by one wave, right after the
// step that finished the episode (ContinuingEnv + run_agents' reset-on-done).
// Same result as reset_one (sl_env.hip): the rolled level is copied into board,
// goals and start board; points, perf baseline and possible are the bit-sliced sums
// over it; the exit list is collected row by row in np.nonzero order.
__device__ __forceinline__ void wave_reset(const sl_env_state &st, const sl_level_pool &pool,
                                        const ResetArgs &ra, int64_t b, int lane) {
    const int ep = __builtin_amdgcn_readfirstlane(st.episodes[b]);
    const LevelChoice lc = choose_level_wave(pool, ra, ra.env0 + (uint32_t)b, ep, N, N, lane);
    const int li = lc.idx, dy = lc.dy, dx = lc.dx;
    const LevelScalars ls = level_scalars(pool, li);     // in flight with the gathers
    const int h = lane & 1, j = lane >> 1;
    const uint16_t *lb = pool.board + (int64_t)li * (N * N), *lg = pool.goals + (int64_t)li * (N * N);
    const int c0 = (2 * j - dx) & 63, c1 = (2 * j + 1 - dx) & 63;
    const int64_t off = b * (int64_t)(N * N);
    const int lane_off = h * 1024 + j;
    u32 *gs = reinterpret_cast<u32 *>(st.start_board + off) + lane_off;
    u32 *gg = reinterpret_cast<u32 *>(st.goals + off) + lane_off;
    u32 *gb = reinterpret_cast<u32 *>(st.board + off) + lane_off;
    // the lane's 32 dwords of a rolled pool level (all gathers in flight at once:
    // this runs in its own kernel, registers are plentiful)
    auto rolled = [&](const uint16_t *lv, u32 D[32]) {
#pragma unroll
        for (int y = 0; y < 32; y++) {
            const int sr = ((32 * h + y - dy) & 63) * N;
            D[y] = (u32)lv[sr + c0] | ((u32)lv[sr + c1] << 16);
        }
    };
    // both gathers in flight together; the board's rows serve the start board (as
    // loaded), the sums (transposed copy) and the board itself (exits coloured)
    u32 P[32], D[32];
    rolled(lg, P);
    rolled(lb, D);
    // goals: copy, then keep their colour planes for the sums
#pragma unroll
    for (int y = 0; y < 32; y++) gg[y * 32] = P[y];
    transpose32(P);
    u32 *mg = st.planes ? st.planes + b * 4096 + 2048 + lane : nullptr;
    if (mg) {      // the goals' bit-plane mirror
#pragma unroll
        for (int q = 0; q < 32; q++) mg[q * 64] = P[q];
    }
    u32 gcol[3][2];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        gcol[k][0] = PL(P, 9 + k, 0);
        gcol[k][1] = PL(P, 9 + k, 1);
    }
    const bool sg = __ballot((PL(P, 7, 0) | PL(P, 7, 1)) != 0u) != 0ull;
    // start board: copy, then the sums over the initial board and goals
#pragma unroll
    for (int y = 0; y < 32; y++) {
        gs[y * 32] = D[y];
        P[y] = D[y];
    }
    transpose32(P);
    int pts, scr, pos, side;
    score_planes(P, gcol, P, &pts, &scr, &pos, &side);
    const ScoreTotals t = score_totals(pts, scr, pos, 0);     // (no side effects yet)
    const bool sb = __ballot((PL(P, 7, 0) | PL(P, 7, 1)) != 0u) != 0ull;
    int ev = 0;
    if (lane == 0)
        ev = reset_scalars_from(st, ra, b, li, dy, dx, ls, ep, t.points, t.score, t.possible,
                                (sb ? 1 : 0) | (sg ? 2 : 0));
    ev = __builtin_amdgcn_readfirstlane(ev);
    const u32 ex0 = PL(P, 8, 0), ex1 = PL(P, 8, 1);       // exit planes
    // the board: the start board with its exits coloured (update_exit_colors)
    {
#pragma unroll
        for (int y = 0; y < 32; y++) {
            u32 d = D[y];
            if (d & (u32)EXIT) d = (d & 0xFFFF0000u) | (u32)ev;
            if (d & ((u32)EXIT << 16)) d = (d & 0x0000FFFFu) | ((u32)ev << 16);
            gb[y * 32] = d;
        }
    }
    // exits in np.nonzero (row-major) order: repeatedly take the wave-wide smallest
    // key row * 64 + column among the lanes' remaining exit bits (one round per exit)
    const int n_exit = wave_total(__builtin_popcount(ex0) + __builtin_popcount(ex1));
    {
        u32 e0 = ex0, e1 = ex1;
        const int kmax = n_exit < SL_MAX_EXITS ? n_exit : SL_MAX_EXITS;   // uniform
        for (int k = 0; k < kmax; k++) {
            const u32 k0 = e0 ? (u32)((32 * h + __builtin_ctz(e0)) * N + 2 * j) : 0xFFFFu;
            const u32 k1 = e1 ? (u32)((32 * h + __builtin_ctz(e1)) * N + 2 * j + 1) : 0xFFFFu;
            u32 m = k0 < k1 ? k0 : k1;
            m = min(m, dpp<0xB1>(m));
            m = min(m, dpp<0x4E>(m));
            m = min(m, dpp<0x141>(m));
            m = min(m, dpp<0x140>(m));
            const u32 key = min(min((u32)__builtin_amdgcn_readlane((int)m, 0),
                                    (u32)__builtin_amdgcn_readlane((int)m, 16)),
                                min((u32)__builtin_amdgcn_readlane((int)m, 32),
                                    (u32)__builtin_amdgcn_readlane((int)m, 48)));
            if (k0 == key) e0 &= e0 - 1;
            if (k1 == key) e1 &= e1 - 1;
            if (lane == 0) {
                st.exit_y[b * SL_MAX_EXITS + k] = (int16_t)(key >> 6);
                st.exit_x[b * SL_MAX_EXITS + k] = (int16_t)(key & 63);
            }
        }
    }
    if (lane == 0) {
        if (mg) st.planes_ok[b] = SL_POK_GOALS_MIRROR;   // after reset_scalars cleared it
        st.exit_count[b] = n_exit;
        for (int e = n_exit; e < SL_MAX_EXITS; e++) {
            st.exit_y[b * SL_MAX_EXITS + e] = 0;
            st.exit_x[b * SL_MAX_EXITS + e] = 0;
        }
    }
}

// all kernel arguments of k_env_step_bits64 in one struct at kernarg offset 0, so a
// phase can re-read one late through kernarg() (write_obs)
struct StepKArgs {
    sl_env_state st;
    StepArgs a;
    FastExtra fx;
    const int32_t *actions;
    int ctp, ctc;
    double *reward_out;
    uint8_t *done_out, *flags_out;
    int32_t *ep_len_out, *ep_rew_out;
};

// the kernel's arguments through a pointer the compiler cannot see as invariant: a
// field read through it is loaded where it is used, not hoisted into the SGPRs that
// the whole kernel then has to keep
__device__ __forceinline__ const StepKArgs &kernarg() {
    auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return *(const StepKArgs *)kp;
}

// ---------------------------------------------------------------- fused observation
// SafeLifeEnv.get_obs + recenter_view (safelife_env.py:125-155, helper_utils.py:41-74)
// of the board the kernel holds on chip, packed (output_channels=None): the same
// values k_env_obs_packed (sl_env.hip) computes from HBM after the step.  A view
// cell is board + ((goals & COLORS) << 3) (white goals optionally removed), i.e. the
// goal colour planes added into planes 12-14.  Board bits 12-14 are unused by every
// cell type, so (wave-uniform check) the planes are overwritten with the goal colours
// and ONE transpose yields both the board rows (masked with ~0x7000 per cell for the
// HBM store) and the view-form rows, which go to the wave's LDS buffer in dma_board's
// layout; a board with any of those bits set takes a bit-sliced add and two more
// transposes instead.  Each view cell is then one u16 LDS read.  Envs reset after the
// step get their view written by the reset-list kernel after their reset.
__device__ __forceinline__ void lds_put_board(lds_u32 *buf, int lane, const u32 D[32]) {
    const int h = lane & 1, j = lane >> 1;
    lds_u32 *p = buf + h * 1024 + ((j + 16 * h) & 31);
#pragma unroll
    for (int y = 0; y < 32; y++) p[y * 32] = D[y];
}

__device__ __forceinline__ int lds_cell_idx(int row, int col) {
    return row * 64 + ((col + 32 * (row >> 5)) & 63);
}

typedef __attribute__((address_space(3))) uint16_t lds_u16;

// Per-half OR: bit y of the result is set when any lane of this lane's parity (rows
// 32 (lane & 1) + y) has it -- quad xor 2, then two row rotations keep the parity
__device__ __forceinline__ uint64_t changed_rows64(u32 cl) {
    u32 x = cl | dpp<0x4E>(cl);           // quad_perm [2,3,0,1]
    x |= dpp<0x124>(x);                   // row_ror:4
    x |= dpp<0x128>(x);                   // row_ror:8
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)x, 0) | (u32)__builtin_amdgcn_readlane((int)x, 16) |
                   (u32)__builtin_amdgcn_readlane((int)x, 32) | (u32)__builtin_amdgcn_readlane((int)x, 48);
    const u32 hi = (u32)__builtin_amdgcn_readlane((int)x, 1) | (u32)__builtin_amdgcn_readlane((int)x, 17) |
                   (u32)__builtin_amdgcn_readlane((int)x, 33) | (u32)__builtin_amdgcn_readlane((int)x, 49);
    return ((uint64_t)hi << 32) | lo;
}

// The rows of M (bit r = row r) stored from the LDS board (lds_put_board's layout:
// chunk c of row r at chunk (c + 4 (r >> 5)) & 7), ANDed with `keep`: slot s = lane >> 3
// of each store instruction takes the s-th listed row, lane & 7 its 16-byte chunk.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_rows(lds_u32 *buf, uint8_t *rowlist, u32 *gb0, uint64_t M,
                                           u32 keep, int lane) {
    typedef __attribute__((address_space(3))) uint8_t lds_u8;
    typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
    lds_u8 *rl = (lds_u8 *)rowlist;
    if ((M >> lane) & 1ull) rl[lanes_below(M)] = (uint8_t)lane;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int n = __builtin_popcountll(M);
    const int c = lane & 7;
    for (int s = lane >> 3; s < n; s += 8) {
        const int row = rl[s];
        u32x4 v = *(const lds_u32x4 *)(buf + row * 32 + (((c + 4 * (row >> 5)) & 7) << 2));
        v &= keep;
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(gb0) + row * 8 + c);
    }
}

// exit y (R_EY) or x (R_EX) number e of the record, e = this lane's own index
__device__ __forceinline__ int lane_exit(const RecFields &fl, int e, int field) {
    const u32 w = (u32)__builtin_amdgcn_ds_bpermute(4 * (field + (e >> 1)), (int)fl.V);
    return (int)(int16_t)(w >> (16 * (e & 1)));
}

__device__ __forceinline__ void write_obs(lds_u32 *buf, const FastExtra &fx, const RecFields &fl,
                                          int64_t b, int lane) {
    lds_u16 *cells = reinterpret_cast<lds_u16 *>(buf);
    (void)fx;
    const FastExtra &lfx = kernarg().fx;     // read late: no SGPRs held through the step
    const int vh = lfx.obs_vh, vw = lfx.obs_vw;
    const int nv = vh * vw;
    const int ty = fl.ay - vh / 2, tx = fl.ax - vw / 2;
    // exits onto their clipped view positions: lane k < ne handles exit k (values read
    // before any is moved); the last in np.nonzero order wins a shared target
    const int ne = min(fl.exit_count(), SL_MAX_EXITS);
    int tgt = -1;
    u32 val = 0u;
    const int iy = lane_exit(fl, lane & 7, R_EY), ix = lane_exit(fl, lane & 7, R_EX);  // all lanes
    if (lane < ne) {
        int jy = ((iy - fl.ay + N / 2) & (N - 1)) - N / 2;
        int jx = ((ix - fl.ax + N / 2) & (N - 1)) - N / 2;
        jy = min(max(jy + vh / 2, 0), vh - 1);
        jx = min(max(jx + vw / 2, 0), vw - 1);
        tgt = jy * vw + jx;
        val = cells[lds_cell_idx(iy, ix)];
        // a view no larger than the board shows each board cell at most once: the
        // exits are moved in the LDS board itself and the gather needs no per-cell test
        tgt = lds_cell_idx((ty + jy) & (N - 1), (tx + jx) & (N - 1)) | (tgt << 12);
    }
    const bool small = vh <= N && vw <= N;
    if (small)
        for (int k = 0; k < ne; k++)            // one store instruction per exit, in order
            if (lane == k) cells[tgt & 4095] = (uint16_t)val;
    uint16_t *o = lfx.obs_out + b * (int64_t)nv;
    const int dr = 64 / vw, dc = 64 - dr * vw;
    if (small) {
        // two cells per store (global_store_dword, 4-B aligned in the whole obs array;
        // an env starting mid-dword stores its first cell alone, an odd remainder its
        // last): 9 store instructions per lane instead of 17 (+1 %, tools/ab/c3p_dword.py)
        const int s0 = (int)((b * (int64_t)nv) & 1);     // env starts mid-dword
        const int np = (nv - s0) >> 1;
        if (s0 && lane == 0) o[0] = cells[lds_cell_idx(ty & (N - 1), tx & (N - 1))];
        if (((nv - s0) & 1) && lane == 1)
            o[nv - 1] = cells[lds_cell_idx((ty + vh - 1) & (N - 1), (tx + vw - 1) & (N - 1))];
        uint32_t *o32 = reinterpret_cast<uint32_t *>(o + s0);
        const int c0 = s0 + 2 * lane;
        int rr = c0 / vw, cc = c0 - rr * vw;
        const int d2r = 128 / vw, d2c = 128 - d2r * vw;
        for (int p = lane; p < np; p += 64) {
            const int r1 = cc + 1 == vw ? rr + 1 : rr, c1 = cc + 1 == vw ? 0 : cc + 1;
            const uint32_t v0 = cells[lds_cell_idx((ty + rr) & (N - 1), (tx + cc) & (N - 1))];
            const uint32_t v1 = cells[lds_cell_idx((ty + r1) & (N - 1), (tx + c1) & (N - 1))];
            o32[p] = v0 | (v1 << 16);
            rr += d2r;
            cc += d2c;
            if (cc >= vw) {
                cc -= vw;
                rr++;
            }
        }
    } else {
        int r = lane / vw, c = lane - r * vw;
        for (int i = lane; i < nv; i += 64) {
            u32 v = cells[lds_cell_idx((ty + r) & (N - 1), (tx + c) & (N - 1))];
            for (int k = 0; k < ne; k++)
                if (i == (__builtin_amdgcn_readlane(tgt, k) >> 12))
                    v = (u32)__builtin_amdgcn_readlane((int)val, k);
            o[i] = (uint16_t)v;
            r += dr;
            c += dc;
            if (c >= vw) {
                c -= vw;
                r++;
            }
        }
    }
}

// Fused channel views (output_channels = a channel list: the reference's default
// 15 channels, safelife_env.py:79,150-154) of the view-form board in LDS (the same
// board write_obs reads, exits moved in place; views no larger than the board): each
// view cell's channel mask goes to the wave's mask array, then the env's output
// bytes leave as 16-byte chunks (obs_store_channels, sl_obs.h) -- no re-read of the
// state from HBM as the separate k_env_obs_channels needs.
template <int ESZ>
__device__ __forceinline__ void write_obs_channels(lds_u32 *buf, uint16_t *vm, const RecFields &fl,
                                                   int64_t b, int lane) {
    lds_u16 *cells = reinterpret_cast<lds_u16 *>(buf);
    const FastExtra &lfx = kernarg().fx;     // read late: no SGPRs held through the step
    const int vh = lfx.obs_vh, vw = lfx.obs_vw;
    const int nv = vh * vw;
    const int ty = fl.ay - vh / 2, tx = fl.ax - vw / 2;
    const int ne = min(fl.exit_count(), SL_MAX_EXITS);
    int tgt = -1;
    u32 val = 0u;
    const int iy = lane_exit(fl, lane & 7, R_EY), ix = lane_exit(fl, lane & 7, R_EX);
    if (lane < ne) {
        int jy = ((iy - fl.ay + N / 2) & (N - 1)) - N / 2;
        int jx = ((ix - fl.ax + N / 2) & (N - 1)) - N / 2;
        jy = min(max(jy + vh / 2, 0), vh - 1);
        jx = min(max(jx + vw / 2, 0), vw - 1);
        val = cells[lds_cell_idx(iy, ix)];
        tgt = lds_cell_idx((ty + jy) & (N - 1), (tx + jx) & (N - 1));
    }
    for (int k = 0; k < ne; k++)              // in np.nonzero order: the last one wins
        if (lane == k) cells[tgt] = (uint16_t)val;
    const sl::obs::ChanMap cm{lfx.obs_chpack, lfx.obs_nch};
    const bool id = cm.ident();
    const int dr = 64 / vw, dc = 64 - dr * vw;
    int r = lane / vw, c = lane - r * vw;
    for (int i = lane; i < nv; i += 64) {
        vm[i] = (uint16_t)cm.mask(cells[lds_cell_idx((ty + r) & (N - 1), (tx + c) & (N - 1))], id);
        r += dr;
        c += dc;
        if (c >= vw) {
            c -= vw;
            r++;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    sl::obs::obs_store_channels<ESZ>(vm, nv, cm.nch, lfx.obs_one, b, lane,
                                     reinterpret_cast<uint8_t *>(lfx.obs_out));
}

// the instantiations' view modes: 0 none, 1 packed, 2 channels of 2-byte elements (u16,
// bf16), 3 of 1-byte (u8), 4 of 4-byte (f32)
constexpr int obs_esz(int OBS) { return OBS == 3 ? 1 : (OBS == 4 ? 4 : 2); }

// What an env's step needs first, issued ahead: the per-env record (lane k = field k)
// and the goals' three colour planes from the mirror (speculative: used when the
// mirror is valid).  The board itself is DMA'd into the wave's LDS buffer.
// NG: the colour planes loaded, 3, or fewer for gray goals (sl_env_state.goals_gray, the
// three planes equal): 1 (plane 9 alone; the others 0) or 0 (no load; all 0).
struct Pre {
    u32 V;
    u32 g[3][2];
};

template <int NG = 3>
__device__ __forceinline__ void issue_pre(const sl_env_state &st, const int32_t *actions,
                                          int64_t b, int lane, Pre &p) {
    p.V = load_record(st, actions, b, lane);
    if (NG < 3) {
#pragma unroll
        for (int k = 0; k < 3; k++) p.g[k][0] = p.g[k][1] = 0u;
    }
    if (NG > 0 && st.planes) {
        const u32 *mg = st.planes + b * 4096 + 2048 + lane;
#pragma unroll
        for (int k = 0; k < NG; k++) {
            p.g[k][0] = mg[(9 + k) * 64];
            p.g[k][1] = mg[(25 + k) * 64];
        }
    }
}

// The goals' step of the two 64x64 kernels, for goals not at their fixed point (the
// callers skip those: (pok & kPokGoalsSkip) == kPokGoalsSkip).  The goals come from their
// bit-plane mirror mg when it is valid (pok has SL_POK_GOALS_MIRROR; mg may be null: no
// mirror), else from the cells gg,
// transposed; after the rule the mirror takes the words whose 32 cells changed (all of
// them if rebuilt), gcol the new colour planes and gg the changed rows.  Returns the
// goals' planes_ok bits after the step (pok without a mirror); the caller stores them.
// PIN: rule_planes'.
template <bool PIN, int MODE>
__device__ __forceinline__ int goals_step64(u32 *gg, u32 *mg, int pok, int lane,
                                            const SpawnCtx &sc, const StreamSrc &ssrc,
                                            int64_t pos_g, u32 gcol[3][2]) {
    int ok = pok;
    u32 PG[32];
    if (pok & SL_POK_GOALS_MIRROR) {
#pragma unroll
        for (int q = 0; q < 32; q++) PG[q] = mg[q * 64];    // goal planes
    } else {
        load_pairs_nt<32>(gg, PG);                              // goal cells
        transpose32(PG);
    }
    u32 cg[2];
    rule_planes<PIN>(PG, cg, Geo64<MODE>{lane, ssrc, pos_g, 0}, sc, 1u);
    const u32 rg = wave_or(cg[0] | cg[1]);
    if (mg) {
        const bool all = !(pok & SL_POK_GOALS_MIRROR);
#pragma unroll
        for (int w = 0; w < 2; w++)
            if (all || cg[w])
#pragma unroll
                for (int k = 0; k < 16; k++) mg[(k + 16 * w) * 64] = PL(PG, k, w);
        const bool fixed = rg == 0 && __ballot((PL(PG, 7, 0) | PL(PG, 7, 1)) != 0u) == 0ull;
        ok = SL_POK_GOALS_MIRROR | (fixed ? SL_POK_GOALS_FIXED : 0);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        gcol[k][0] = PL(PG, 9 + k, 0);
        gcol[k][1] = PL(PG, 9 + k, 1);
    }
    if (rg) {
        transpose32(PG);
#pragma unroll
        for (int y = 0; y < 32; y++)
            if ((rg >> y) & 1u) __builtin_nontemporal_store(PG[y], &gg[y * 32]);
    }
    return ok;
}

// One env-step of env b.  `pre` holds b's record and goal colour planes and b's board
// is in flight into `buf` (issued by the caller).  MODE: SPAWN_PHILOX, or SPAWN_STREAM
// (replay: k_env_action has run the action and k_stream_prologue64 sized the draws; the step reads
// act[b] and each tensor's first uniform from the scratch words).
template <int OBS, int MODE>
__device__ __forceinline__ void step_env(const sl_env_state &st, const StepArgs &a,
                                         const FastExtra &fx, int64_t b, int lane, lds_u32 *buf,
                                         uint16_t *vm, uint8_t *rowlist,
                                         const int32_t *__restrict__ actions,
                                         int ctp, int ctc, double *reward_out, uint8_t *done_out,
                                         uint8_t *flags_out, int32_t *ep_len_out,
                                         int32_t *ep_rew_out, const Pre &pre) {
    constexpr bool VIEW = OBS != 0, CH = OBS >= 2;
    const int64_t off = b * (int64_t)(N * N);
    const int lane_off = (lane & 1) * 1024 + (lane >> 1);     // dwords: row 32h, column pair j
    u32 *gb = reinterpret_cast<u32 *>(st.board + off) + lane_off;
    u32 *gg = reinterpret_cast<u32 *>(st.goals + off) + lane_off;
    // bit-plane mirrors (sl_env_state.planes): read instead of u16 + transpose when valid
    // goals mirror, word-major: word q of lane l at planes[b*4096 + 2048 + q*64 + l]
    // (the goals rarely change, so it saves their transpose at almost no write cost;
    // a board mirror would be rewritten every step and does not pay)
    u32 *mg = st.planes ? st.planes + b * 4096 + 2048 + lane : nullptr;
    const u32 V = pre.V;
    // goals: a goals board without spawners that came through a step unchanged is at
    // a fixed point of the (then deterministic) rule and never changes again
    // (SL_POK_GOALS_FIXED); such envs read only the three colour planes of the mirror,
    // which are speculatively in flight before the record says which case holds
    u32 gcol[3][2];                    // goal colour planes, kept for the scores
#pragma unroll
    for (int k = 0; k < 3; k++) {
        gcol[k][0] = pre.g[k][0];
        gcol[k][1] = pre.g[k][1];
    }
    const int pok = (mg && st.planes_ok) ? rec(V, R_POK) & kPokGoalsSkip : 0;

    const SpawnCtx sc = spawn_ctx(a, b, rec(V, R_SPAWN));
    int64_t pos_b, pos_g;
    const StreamSrc ssrc = stream_src<MODE>(a, fx.scratch, st.B, b, pos_b, pos_g);

    // ---- goals
    if ((pok & kPokGoalsSkip) != kPokGoalsSkip) {
        const int ok = goals_step64<false, MODE>(gg, mg, pok, lane, sc, ssrc, pos_g, gcol);
        if (ok != pok && lane == 0) st.planes_ok[b] = ok;
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---- board: from LDS; the start board comes from the level pool (cache) when
    // the env was reset from it, else from HBM through the same LDS buffer
    int roll = -1;
    if (fx.pool.K > 0 && fx.pool.board_planes && st.start_roll) roll = rec(V, R_ROLL);
    wait_vm();

    // the action (lane 0), on the staged board and the record.  (Kept copy: this
    // prologue is written out here, in the plane kernel and in k_env_step_small.  A
    // force-inlined sl_bits.h helper templated on the cell source -- building the
    // overlay and RecEnv, returning RecFields, edits through out-parameters; or taking
    // a caller-built RecEnv and returning only the reward -- left k_env_step_bits64<0,
    // SPAWN_PHILOX> with 64 spilled VGPRs and 132 B of scratch.)
    OverlayT<LdsCells> ov;
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
        act_reward = (int)scratch_of(fx.scratch, st.B).act[b];
    } else {
        if (lane == 0) act_reward = act_core(env, rec(V, R_ACT), N, N, ctp, ctc, ov);
        act_reward = __builtin_amdgcn_readfirstlane(act_reward);
    }
    const int ne = __builtin_amdgcn_readfirstlane(ov.n);
    int eidx[4];
    u32 eval[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        eidx[k] = __builtin_amdgcn_readfirstlane(ov.idx[k]);
        eval[k] = (u32)__builtin_amdgcn_readfirstlane((int)ov.val[k]);
    }
    const RecFields fl = rec_fields(a, V, __builtin_amdgcn_readfirstlane(env.go),
                                    __builtin_amdgcn_readfirstlane(env.ax),
                                    __builtin_amdgcn_readfirstlane(env.ay));

    u32 PB[32];
    read_pairs(buf, lane, PB);
    wait_lgkm();
    if (roll < 0) dma_board(st.start_board + off, buf, lane);
    else pool_dma(fx.pool, rec(V, R_LI), buf, lane);
    transpose32(PB);
    const u32 erow = mux_edits(PB, ne, eidx, eval, lane);
    u32 cb[2];
    rule_planes(PB, cb, Geo64<MODE>{lane, ssrc, pos_b, 0}, sc, 0u);
    __builtin_amdgcn_sched_barrier(0);
    // fused views: board bits 12-14 are unused by every cell type, so (wave-uniform
    // check) the goal colours go into planes 12-14 now -- the scores read them there
    // and the goal planes die before the scoring -- and ONE transpose later yields
    // both the board rows and the view rows
    const bool hi = VIEW && __ballot((PL(PB, 12, 0) | PL(PB, 13, 0) | PL(PB, 14, 0) |
                                      PL(PB, 12, 1) | PL(PB, 13, 1) | PL(PB, 14, 1)) != 0u) != 0ull;
    if (VIEW && !hi) {
        const int obs_rw = kernarg().fx.obs_rw;
#pragma unroll
        for (int w = 0; w < 2; w++) {
            const u32 white = obs_rw ? (gcol[0][w] & gcol[1][w] & gcol[2][w]) : 0u;
#pragma unroll
            for (int k = 0; k < 3; k++) PL(PB, 12 + k, w) = gcol[k][w] & ~white;
        }
    }

    // ---- scores over the new board and goals
    u32 PS[32];
    wait_vm();
    if (roll >= 0) {
        pool_planes_lds(buf, roll >> 16, roll & 0xFFFF, lane, PS);
    } else {
        read_pairs(buf, lane, PS);
        transpose32(PS);
    }
    int pts, scr, pos, side;
    if (VIEW && !hi) score_planes<true>(PB, gcol, PS, &pts, &scr, &pos, &side);
    else score_planes(PB, gcol, PS, &pts, &scr, &pos, &side);
    // totals: reduced before the board store so the scoring is not sunk past it
    const ScoreTotals tot = score_totals(pts, scr, pos, side);
    __builtin_amdgcn_sched_barrier(0);

    // ---- write back the changed rows of the board, exits already in the colour the
    // epilogue gives them (update_exit_colors), so its exit writes and these row
    // stores carry the same values and need no ordering
    const u32 rb = wave_or(cb[0] | cb[1]) | erow;
    if (rb || VIEW) {
        (void)recolour_exits(PB, can_exit_now(fl.min_performance(), tot.score, fl.baseline(),
                                              tot.possible));
        transpose32(PB);
        if (VIEW && !hi) {
            lds_put_board(buf, lane, PB);      // the start board in buf has been read out
            // the changed rows from the LDS board (which the views read anyway), 8 whole
            // rows per store; planes 12-14 hold the goal colours: the store masks them
            // out again.  (From registers a store writes rows y and 32 + y together:
            // same box, packed views 264.5 vs 258.9 M env-steps/s, tools/ab/c3_rowlist.py;
            // without views the LDS round trip costs more than the bytes it saves,
            // 344.6 vs 356.7 M, so that path keeps the register stores below.)
            if (rb) {
                uint64_t M = changed_rows64(cb[0] | cb[1]);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (k < ne) M |= 1ull << (eidx[k] >> 6);
                store_rows(buf, rowlist, reinterpret_cast<u32 *>(st.board + off), M, 0x8FFF8FFFu,
                           lane);
            }
        } else if (rb) {
#pragma unroll
            for (int y = 0; y < 32; y++)
                if ((rb >> y) & 1u) __builtin_nontemporal_store(PB[y], &gb[y * 32]);
        }
    }
    if (VIEW && !hi) {
        __builtin_amdgcn_sched_barrier(0);
        if (CH) write_obs_channels<obs_esz(OBS)>(buf, vm, fl, b, lane);
        else write_obs(buf, fx, fl, b, lane);
        __builtin_amdgcn_sched_barrier(0);
    }
    int reset = 0;
    if (lane == 0)
        reset = epilogue_core(st, a, b, fl, act_reward, tot.points, tot.score, tot.possible,
                              tot.side, reward_out, done_out, flags_out, ep_len_out, ep_rew_out);
    reset = __builtin_amdgcn_readfirstlane(reset);
    if (VIEW && hi && !(fx.fuse_reset && reset)) {
        // a board using bits 12-14 (no cell type does): the view from the stored state
        // once everything has landed -- the action's writes, this step's goal and row
        // stores and the epilogue's exit cells (this wave's own stores) -- as
        // k_env_obs_packed computes it; an env reset after the step gets its view from
        // the reset-list kernel instead
        wait_vm();
        const FastExtra &lfx = kernarg().fx;
        sl::obs::ObsArgs oa{};
        oa.vh = lfx.obs_vh;
        oa.vw = lfx.obs_vw;
        oa.remove_white = lfx.obs_rw;
        oa.mode = lfx.obs_mode;
        oa.nch = lfx.obs_nch;
        if (CH)
            sl::obs::obs_channels_wave<obs_esz(OBS)>(
                st, oa, sl::obs::ChanMap{lfx.obs_chpack, lfx.obs_nch}, lfx.obs_one, b, lane, vm,
                reinterpret_cast<uint8_t *>(lfx.obs_out));
        else
            sl::obs::obs_packed_wave(st, oa, b, lane, lfx.obs_out);
    }
    // queue the env for the reset kernel (k_env_reset_list)
    if (fx.fuse_reset && reset && lane == 0) queue_reset(fx.scratch, st.B, a.step, b);
}

// OBS: also write the observation (fx.obs_out): 1 packed, 2-4 channel views
// (obs_esz); MODE: see step_env
template <int OBS, int MODE>
__global__ void __launch_bounds__(64, (OBS || MODE == SPAWN_STREAM) ? kMinWavesObs : kMinWaves)
k_env_step_bits64(StepKArgs ka) {
    const int64_t b = blockIdx.x;          // one wave per env
    const int lane = threadIdx.x;
    __shared__ __attribute__((aligned(16))) u32 stage[N * N / 2];
    // channel views: the view's channel masks (write_obs_channels)
    __shared__ __attribute__((aligned(16))) uint16_t vmask[OBS >= 2 ? sl::obs::kFusedChanCells : 2];
    __shared__ uint8_t rowlist[OBS ? 64 : 1];   // changed rows by rank (store_rows)
    lds_u32 *buf = (lds_u32 *)&stage[0];
    Pre pre;
    issue_pre(ka.st, ka.actions, b, lane, pre);
    dma_board(ka.st.board + b * (int64_t)(N * N), buf, lane);
    step_env<OBS, MODE>(ka.st, ka.a, ka.fx, b, lane, buf, vmask, rowlist, ka.actions, ka.ctp, ka.ctc,
                        ka.reward_out, ka.done_out, ka.flags_out, ka.ep_len_out, ka.ep_rew_out,
                        pre);
}

// ---------------------------------------------------------------- plane mode
// The 64x64 board kept in bit planes across steps (round 6; the 128x128 kernel's
// round-5 design, sl_bits128.hip): half 0 of the goals mirror (sl_env_state.planes:
// word q of lane l at planes[b*4096 + q*64 + l] = plane q & 15 of column 2 (l >> 1) +
// (q >> 4), rows 32 (l & 1) .. +31; half 1 keeps the goals).  A Philox step without
// capture (sl_env_state.board_planes == planes; without views, or with views it writes
// from the planes itself: packed, or channel views, k_env_planes64_chan) DMA's the plane words into
// the wave's buffer at once -- as the uint16 board was -- runs the action on them, and
// stores only the words that changed; no transposes.  Planes in
// sl_env_state.board_zero (all zero in every board of the batch, for good: the C3 / C4
// pools never use cell bits 7 and 11-14) are neither loaded nor stored, nor are the
// planes in sl_env_state.agent_planes (one cell each, the agent's: built from its
// position) or in sl_env_state.derived_planes (plane 15, a copy of plane 2; plane 8, the
// env's exit list), and the stored ones are packed (PlaneSlots): on C3 / C4 3 of the 8 KiB
// are read.  SL_POK_BOARD_PLANES: the
// planes hold the board; SL_POK_BOARD_FULL: so does the uint16 board (a sync wrote it),
// which a plane step otherwise leaves stale (exits aside: the epilogue writes them in
// both).

// The stored planes packed word after word: word q (plane q & 15 of column word q >> 4)
// at position pos(q), the number of stored words below it, so the stored words come
// first and one DMA instruction of 16 B per lane moves four of them (4-B DMAs word by
// word ran 12 % slower).  Two masks: the planes a board can HOLD (~board_zero: the
// others are zero in registers too) and, among them, the planes that are STORED: held
// and not in sl_env_state.agent_planes.  An agent plane holds one cell, the agent's, whose
// position is in the env's record: its words are built from (R_AY, R_AX), never loaded
// or stored (C3 / C4: planes 1, 5 and 6; 16 of 32 words are stored, four DMA
// instructions with no padding).  The layout follows board_zero and agent_planes, which
// change only after every board has left the planes.
// the instantiations: every plane, the C3 / C4 pools' planes (cell bits 0-6, 8-10, 15,
// of which the agent's 1, 5, 6 are implied), and any other masks at run time
constexpr u32 kKeepAll = 0xFFFFu, kKeepC3 = 0x877Fu, kAgentC3 = 0x0062u;
// Derived planes (sl_env_state.derived_planes): planes a board holds that are neither
// loaded nor stored but rebuilt in registers once the stored words are read -- plane 15, a
// copy of plane 2 (only the crate carries either bit; taken after mux_edits, so the action's
// edits reach both), and plane 8, one bit per exit of the record's exit list (at most
// SL_MAX_EXITS, built as agent_words builds the agent's).  The stored words are packed
// without them: C3 / C4 12 words, three DMA groups, instead of 16 and four.  As with the
// other two masks the layout changes only after every board has left the planes.
constexpr u32 kDerivable = 0x8100u;
// the derived planes a state's flag stands for: both, or none (a batch with half the
// property stores both planes)
__host__ __device__ constexpr u32 derived_eff(u32 derived) {
    return (derived & kDerivable) == kDerivable ? kDerivable : 0u;
}
// K16: the held planes, fixed at compile time; 0: from board_zero.  DM: the derived planes,
// fixed at compile time (the kKeepC3 instances: 0x8100, and 0 in their k_env_p64_stored16
// twins; every position a constant in both); -1: from derived_planes
template <u32 K16, int DM = -1>
struct PlaneSlots {
    // kKeepC3 fixes the agent planes too (the dispatch checks both); the other two
    // take them at run time
    static constexpr bool kFixed = K16 == kKeepC3;
    u32 keep;           // bit q: word q is held (K16 == 0)
    u32 store;          // bit q: word q has a position in the layout (!kFixed)
    u32 drv_;           // bit p: plane p (of kDerivable, in the layout) is derived (DM < 0)
    __device__ __forceinline__ u32 drv16() const { return DM >= 0 ? (u32)DM : drv_; }
    __device__ __forceinline__ u32 keep32() const { return K16 ? K16 * 0x10001u : keep; }
    __device__ __forceinline__ u32 store32() const {
        return kFixed ? (K16 & ~kAgentC3) * 0x10001u : store;
    }
    static constexpr bool late(int q) { return (kDerivable >> (q & 15)) & 1u; }
    __device__ __forceinline__ bool kept(int q) const { return (keep32() >> q) & 1u; }
    __device__ __forceinline__ bool laid(int q) const { return (store32() >> q) & 1u; }
    // loaded and stored: held, not the agent's and not derived
    __device__ __forceinline__ bool stored(int q) const {
        return laid(q) && !(late(q) && ((drv16() >> (q & 15)) & 1u));
    }
    __device__ __forceinline__ u32 stored32() const { return store32() & ~(drv16() * 0x10001u); }
    // the agent planes (held, not stored or derived)
    __device__ __forceinline__ u32 agent16() const {
        return kFixed ? kAgentC3 : (keep32() & ~store32()) & 0xFFFFu;
    }
    // (at run time recomputed where used: two SALU, not 32 positions held in SGPRs all
    // kernel long; with kFixed and DM a constant)
    __device__ __forceinline__ int pos(int q) const {
        const u32 below = (1u << q) - 1u;
        if (kFixed && DM >= 0) return __builtin_popcount(stored32() & below);
        u32 k = stored32();
        asm volatile("" : "+s"(k));
        return __builtin_popcount(k & below);
    }
    __device__ __forceinline__ int stored16() const {
        return __builtin_popcount(stored32() & 0xFFFFu);
    }
    static __device__ __forceinline__ PlaneSlots of(u32 zero, u32 agent, u32 derived) {
        const u32 k = ~zero & 0xFFFFu;
        const u32 s = kFixed ? (K16 & ~kAgentC3) : ((K16 ? K16 : k) & ~agent);
        return PlaneSlots{k * 0x10001u, (k & ~agent) * 0x10001u, derived_eff(derived) & s};
    }
};
// this lane's two words of the exit plane: one bit per exit of the record's list
__device__ __forceinline__ void exit_words(u32 V, int lane, u32 ew[2]) {
    const RecFields fl{V, 0, 0, 0, 0.0};
    const int n = min(fl.exit_count(), SL_MAX_EXITS);
    ew[0] = ew[1] = 0u;
#pragma unroll 1
    for (int e = 0; e < n; e++) {
        const int y = fl.exit_y(e), x = fl.exit_x(e);
        const u32 bit = lane == 2 * (x >> 1) + (y >> 5) ? 1u << (y & 31) : 0u;
        if (x & 1) ew[1] |= bit;
        else ew[0] |= bit;
    }
}
// this lane's two words of an agent plane: the one bit of cell (ay, ax)
__device__ __forceinline__ void agent_words(int ay, int ax, int lane, u32 aw[2]) {
    const u32 bit = lane == 2 * (ax >> 1) + (ay >> 5) ? 1u << (ay & 31) : 0u;
    aw[0] = (ax & 1) ? 0u : bit;
    aw[1] = (ax & 1) ? bit : 0u;
}
// the plane kernel's waves per SIMD: five (96 VGPRs; 20 x 8 KiB is the CU's LDS) where
// the instantiation fits that budget without spills -- the C3 / C4 planes without views
// (its 10 planes never held are 20 registers fewer); the others spill there (13-24
// VGPRs) and stay at four
constexpr int kMinWavesPlanes = 5;
constexpr int planes_min_waves(u32 k16, int obs) {
    return (obs == 0 && k16 == kKeepC3) ? kMinWavesPlanes : kMinWaves;
}

// the stored plane words of an env, DMA'd into the wave's buffer in their packed order
// (position p of lane l at buf[p * 64 + l]); no registers held while they are in flight
template <u32 K16, int DM>
__device__ __forceinline__ void dma_planes(const u32 *__restrict__ bp, PlaneSlots<K16, DM> ps,
                                           lds_u32 *buf, int lane) {
    const int groups = (2 * ps.stored16() + 3) >> 2;
    const char *s = reinterpret_cast<const char *>(bp);
#pragma unroll
    for (int g = 0; g < 8; g++)
        if (g < groups)
            __builtin_amdgcn_global_load_lds((const void *)(s + g * 1024 + lane * 16),
                                             (__attribute__((address_space(3))) void *)(buf + g * 256),
                                             16, 0, 2);
}

// The cells act_core can read around (y0, x0) -- the row within +-2 columns, the
// column within +-2 rows: near_cell_index(k) -- gathered from the staged planes by
// lanes 0..8 at once (16 LDS reads for the wave, not 16 per cell on the action's lane),
// then read by the lane-0 action with v_readlane (whatever the exec mask)
__device__ __forceinline__ int near_cell_index(int k, int y0, int x0) {
    const int dy = k < 5 ? 0 : (k == 5 ? -1 : k == 6 ? 1 : k == 7 ? -2 : 2);
    const int dx = k >= 5 || k == 0 ? 0 : (k == 1 ? -1 : k == 2 ? 1 : k == 3 ? -2 : 2);
    return ((y0 + dy) & 63) * 64 + ((x0 + dx) & 63);
}
struct NearCells {
    int y0, x0;
    u32 v;              // lane k: cell near_cell_index(k)
    __device__ __forceinline__ uint32_t operator()(int i) const {
        const int dy = (((i >> 6) - y0 + 32) & 63) - 32, dx = (((i & 63) - x0 + 32) & 63) - 32;
        const int k = dy == 0 ? (dx == 0 ? 0 : dx == -1 ? 1 : dx == 1 ? 2 : dx == -2 ? 3 : 4)
                              : (dy == -1 ? 5 : dy == 1 ? 6 : dy == -2 ? 7 : 8);
        return (u32)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(k));
    }
};
// cell i from the staged planes (this lane's; of the planes not stored, the derived ones
// are rebuilt from plane 2 and the record's exit list -- the action tests EXIT on these
// cells and moves crates whole -- and the agent planes are 0: the caller adds them to the
// agent's cell)
template <u32 K16, int DM>
__device__ __forceinline__ u32 lds_plane_cell(const lds_u32 *buf, PlaneSlots<K16, DM> ps, u32 V,
                                              int i) {
    const int y = i >> 6, x = i & 63;
    const lds_u32 *q = buf + 2 * (x >> 1) + (y >> 5);
    const u32 r = (u32)(y & 31);
    const int w = 16 * (x & 1);
    u32 v = 0;
#pragma unroll
    for (int p = 0; p < 16; p++) {
        const int pw = ps.pos(p) + (w ? ps.stored16() : 0);
        if (ps.stored(p)) v |= ((q[pw * 64] >> r) & 1u) << p;
    }
    if (ps.drv16() & 0x8000u) v |= (v & 4u) << 13;
    if (ps.drv16() & 0x0100u) {
        const RecFields fl{V, 0, 0, 0, 0.0};
        const int n = min(fl.exit_count(), SL_MAX_EXITS);
#pragma unroll 1
        for (int e = 0; e < n; e++)
            if (i == fl.exit_y(e) * 64 + fl.exit_x(e)) v |= 0x0100u;
    }
    return v;
}

// Cell i from the staged planes: its stored planes' bits, and plane 15 rebuilt from plane 2
// where it is derived (the action moves crates whole).  Not in the value: the agent planes
// (the caller adds them to the agent's cell) and a derived exit plane (the caller takes the
// bit from the record's exit list).  Every lane may read its own cell.
template <u32 K16, int DM>
__device__ __forceinline__ u32 lds_plane_cell_stored(const lds_u32 *buf, PlaneSlots<K16, DM> ps,
                                                     int i) {
    const int y = i >> 6, x = i & 63;
    const lds_u32 *q = buf + 2 * (x >> 1) + (y >> 5);
    const u32 r = (u32)(y & 31);
    const int w = 16 * (x & 1);
    u32 v = 0;
#pragma unroll
    for (int p = 0; p < 16; p++) {
        const int pw = ps.pos(p) + (w ? ps.stored16() : 0);
        if (ps.stored(p)) v |= ((q[pw * 64] >> r) & 1u) << p;
    }
    if (ps.drv16() & 0x8000u) v |= (v & 4u) << 13;
    return v;
}

// The step itself is sl_planes64_step.inc, shared with k_env_planes64_chan below.  The
// kKeepC3 instances have the derived planes compiled in as well (DM 0x8100: twelve stored
// words, every position a constant); a C3 batch without them runs k_env_p64_stored16.
constexpr int planes_dm(u32 k16) { return k16 == kKeepC3 ? (int)kDerivable : -1; }
// OBS: 0 no views, 1 packed views
template <u32 K16, int OBS>
__global__ void __launch_bounds__(64, planes_min_waves(K16, OBS))
k_env_step_bits64_planes(StepKArgs ka) {
    __shared__ __attribute__((aligned(16))) u32 stage[N * N / 2];
    uint16_t *const vm = nullptr;
    constexpr bool GRAY = false, W6 = false, SPLIT_EPI = false;
    constexpr int DM = planes_dm(K16);
#include "sl_planes64_step.inc"
}

// The same for a batch whose goals are all black or white (sl_env_state.goals_gray): the
// step reads no goal colour plane from the mirror (OBS 0: six loads and six registers
// fewer, 1 536 of the step's bytes per env) or one of the three (OBS 1, for the view; none
// with white goals removed).  Instantiated for the C3 / C4 planes only: batches with
// other plane masks keep loading the colours, gray goals or not.  (Named apart from
// k_env_step_*, as k_env_planes64_chan is; tests/test_kernel_resources_gray.py.)
template <u32 K16, int OBS>
__global__ void __launch_bounds__(64, planes_min_waves(K16, OBS))
k_env_planes64_gray(StepKArgs ka) {
    static_assert(OBS <= 1, "channel views load the three colour planes");
    __shared__ __attribute__((aligned(16))) u32 stage[N * N / 2];
    uint16_t *const vm = nullptr;
    constexpr bool GRAY = true, W6 = false, SPLIT_EPI = false;
    constexpr int DM = planes_dm(K16);
#include "sl_planes64_step.inc"
}

// k_env_planes64_gray<K16, 0> at six waves per SIMD: at most 80 VGPRs and a buffer of
// 6 KiB (24 waves x 6 KiB = 144 of the CU's 160 KiB).  The buffer holds the 4 KiB of stored
// plane words, then the 5 KiB of start-plane rows the scores need, packed; the two cold
// entries that stage a whole uint16 board (the step after a reset or a host write, and a
// caller-written start board) take it in two halves (board_pairs_halves).  Same loads,
// same stores, same results.  Only the C3 / C4 planes are instantiated.  (Named apart
// from k_env_step_* and k_env_planes64_gray, whose resource tests count by name;
// tests/test_kernel_resources_w6.py.)
constexpr int kMinWavesW6 = 6;
constexpr int kStageDwW6 = 1536;
template <u32 K16>
__global__ void __launch_bounds__(64, kMinWavesW6)
k_env_planes64_w6(StepKArgs ka) {
    __shared__ __attribute__((aligned(16))) u32 stage[kStageDwW6];
    uint16_t *const vm = nullptr;
    constexpr int OBS = 0;
    constexpr bool GRAY = true, W6 = true, SPLIT_EPI = false;
    constexpr int DM = planes_dm(K16);
#include "sl_planes64_step.inc"
}

// k_env_planes64_w6 without its one-lane tail: after the plane stores lane 0 writes the
// env's hand-over record (Handover, sl_bits.h) and the wave ends; the epilogue and the
// resets run in k_env_epilogue_reset64 below, launched right after.  Same registers and
// buffer; launched only with auto-reset from a pool (SL_PLAN_K64_S6).  (Named apart from
// k_env_planes64_w6, whose resource test counts by name;
// tests/test_kernel_resources_split.py.)
template <u32 K16>
__global__ void __launch_bounds__(64, kMinWavesW6)
k_env_planes64_s6(StepKArgs ka) {
    __shared__ __attribute__((aligned(16))) u32 stage[kStageDwW6];
    uint16_t *const vm = nullptr;
    constexpr int OBS = 0;
    constexpr bool GRAY = true, W6 = true, SPLIT_EPI = true;
    constexpr int DM = planes_dm(K16);
#include "sl_planes64_step.inc"
}

// The epilogue of every env k_env_planes64_s6 stepped, one lane per env (in the step's
// wave it ran on lane 0 while 63 lanes idled and the wave held its registers and LDS), then
// the resets of the envs that finished: each wave ballots the lanes whose env finished,
// and the block's four waves take its finished envs in turn, all 64 lanes resetting one
// env (wave_reset, as k_env_reset_list runs it).  No list in memory and no shared counter;
// the reset-list lengths stay zero, and the other step parity's is zeroed as
// k_env_reset_list does.
constexpr int kTailThreads = 256;
__global__ void __launch_bounds__(kTailThreads)
k_env_epilogue_reset64(sl_env_state st, StepArgs a, sl_level_pool pool, ResetArgs ra,
                       int64_t *scratch, double *reward_out, uint8_t *done_out,
                       uint8_t *flags_out, int32_t *ep_len_out, int32_t *ep_rew_out) {
    const int64_t b = (int64_t)blockIdx.x * kTailThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (b == 0) scratch[8 * st.B + 2 + ((a.step + 1) & 1)] = 0;
    bool reset = false;
    if (b < st.B) {
        const Handover h = get_handover(handover_of(scratch, st.B), b);
        const HandFields f{{st, b, a.bonus_table}, h.go, h.ax, h.ay, h.dist};
        reset = epilogue_core(st, a, b, f, h.act_reward, h.points, h.score, h.possible, h.side,
                              reward_out, done_out, flags_out, ep_len_out, ep_rew_out);
    }
    // the block's finished envs, dealt round its four waves in env order: two in one
    // wave's 64 (a few waves every step at 65 536 envs) do not wait for each other
    __shared__ uint64_t finished[kTailThreads / 64];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t mine = __ballot(reset);
    if (lane == 0) finished[wave] = mine;
    // the epilogue's stores before the resets' to the same words (the env's scalars; no
    // board cell: HandFields has no exits), which other lanes -- of any wave of the block --
    // issue: retired at workgroup scope (the block's waves store through one CU to one L2; a
    // device-scope fence in every wave, with its L2 write-back, cost more than the step
    // kernel gained)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    const int64_t b0 = (int64_t)blockIdx.x * kTailThreads;
    int i = 0;
#pragma unroll 1
    for (int q = 0; q < kTailThreads / 64; q++) {
        const uint64_t f = finished[q];
        uint64_t todo = ((uint64_t)(u32)__builtin_amdgcn_readfirstlane((int)(f >> 32)) << 32) |
                        (u32)__builtin_amdgcn_readfirstlane((int)f);
        while (todo) {
            const int k = __builtin_ctzll(todo);
            todo &= todo - 1;
            if ((i++ & (kTailThreads / 64 - 1)) == wave) wave_reset(st, pool, ra, b0 + 64 * q + k, lane);
        }
    }
}

// Plane mode with channel views of ESZ-byte elements (1: u8, 2: u16 / bf16, 4: f32): the
// board stays in planes on the steps the reference's PPO takes (output_channels =
// range(15)).  stage + vmask = 10 384 B a wave, 15 waves in the CU's 160 KiB as
// k_env_step_bits64<2..4, 0> has.  (Named apart from k_env_step_*: the step kernels'
// resource test counts those by name; tests/test_kernel_resources_chan.py covers these.)
template <u32 K16, int ESZ>
__global__ void __launch_bounds__(64, kMinWaves)
k_env_planes64_chan(StepKArgs ka) {
    constexpr int OBS = ESZ == 1 ? 3 : (ESZ == 4 ? 4 : 2);      // obs_esz(OBS) == ESZ
    __shared__ __attribute__((aligned(16))) u32 stage[N * N / 2];
    __shared__ __attribute__((aligned(16))) uint16_t vmask[sl::obs::kFusedChanCells];
    uint16_t *const vm = vmask;
    constexpr bool GRAY = false, W6 = false, SPLIT_EPI = false;
    constexpr int DM = planes_dm(K16);
#include "sl_planes64_step.inc"
}

// The kKeepC3 instances for a batch whose flag does not stand for both derived planes (DM 0:
// all sixteen words stored, the code those instances were before derived planes): can_toggle_powers, a
// pool with a bit-2 cell that lacks bit 15, a state built without the flag.  KIND: 0
// k_env_step_bits64_planes<kKeepC3, OBS>, 1 k_env_planes64_gray<kKeepC3, OBS>, 2
// k_env_planes64_w6, 3 k_env_planes64_s6, 4 k_env_planes64_chan<kKeepC3, obs_esz(OBS)>.
// (One name apart from all of theirs: the resource tests count those by name.)
constexpr int stored16_min_waves(int kind, int obs) {
    return kind == 2 || kind == 3 ? kMinWavesW6 : (kind == 4 ? kMinWaves : planes_min_waves(kKeepC3, obs));
}
template <int KIND, int OBS>
__global__ void __launch_bounds__(64, stored16_min_waves(KIND, OBS))
k_env_p64_stored16(StepKArgs ka) {
    constexpr u32 K16 = kKeepC3;
    constexpr int DM = 0;
    constexpr bool GRAY = KIND >= 1 && KIND <= 3, W6 = KIND == 2 || KIND == 3, SPLIT_EPI = KIND == 3;
    __shared__ __attribute__((aligned(16))) u32 stage[W6 ? kStageDwW6 : N * N / 2];
    __shared__ __attribute__((aligned(16))) uint16_t vmask[OBS >= 2 ? sl::obs::kFusedChanCells : 2];
    uint16_t *const vm = OBS >= 2 ? vmask : nullptr;
#include "sl_planes64_step.inc"
}

// sl_env_board_sync for 64x64 boards in planes: one wave per env
__global__ void __launch_bounds__(64) k_board_sync64(sl_env_state st, int demote) {
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const int pok = __builtin_amdgcn_readfirstlane(st.planes_ok[b]);
    if (!(pok & SL_POK_BOARD_PLANES)) return;
    if (!(pok & SL_POK_BOARD_FULL)) {
        const PlaneSlots<0> ps = PlaneSlots<0>::of(st.board_zero, st.agent_planes,
                                                   st.derived_planes);
        const u32 *bp = st.planes + b * 4096 + lane;
        u32 P[32];
#pragma unroll
        for (int q = 0; q < 32; q++) P[q] = ps.stored(q) ? bp[ps.pos(q) * 64] : 0u;
        // the agent planes: their one cell, from the agent's position
        u32 aw[2];
        agent_words(__builtin_amdgcn_readfirstlane(st.agent_y[b]),
                    __builtin_amdgcn_readfirstlane(st.agent_x[b]), lane, aw);
#pragma unroll
        for (int q = 0; q < 32; q++)
            if ((ps.agent16() >> (q & 15)) & 1u) P[q] = aw[q >> 4];
        // the derived planes: the crate's second bit, and the exits of the env's list
        if (ps.drv16() & 0x8000u) {
            PL(P, 15, 0) = PL(P, 2, 0);
            PL(P, 15, 1) = PL(P, 2, 1);
        }
        if (ps.drv16() & 0x0100u) {
            const int n = min(__builtin_amdgcn_readfirstlane(st.exit_count[b]), SL_MAX_EXITS);
            PL(P, 8, 0) = PL(P, 8, 1) = 0u;
            for (int e = 0; e < n; e++) {
                const int y = __builtin_amdgcn_readfirstlane(st.exit_y[b * SL_MAX_EXITS + e]);
                const int x = __builtin_amdgcn_readfirstlane(st.exit_x[b * SL_MAX_EXITS + e]);
                const u32 bit = lane == 2 * (x >> 1) + (y >> 5) ? 1u << (y & 31) : 0u;
                if (x & 1) PL(P, 8, 1) |= bit;
                else PL(P, 8, 0) |= bit;
            }
        }
        transpose32(P);
        u32 *gb = reinterpret_cast<u32 *>(st.board + b * (int64_t)(N * N)) + (lane & 1) * 1024 +
                  (lane >> 1);
#pragma unroll
        for (int y = 0; y < 32; y++) gb[y * 32] = P[y];
    }
    if (lane == 0)
        st.planes_ok[b] = demote ? pok & ~(SL_POK_BOARD_PLANES | SL_POK_BOARD_FULL)
                                 : pok | SL_POK_BOARD_FULL;
}

// Replay-mode count of env b (SL_RNG_STREAM), one wave, after k_env_action (one lane
// per env) has applied the actions -- state and cell edits in HBM, rewards in scratch
// act[] -- so the board read here is the acted-on one: the eligible cells, i.e. the
// uniforms the step will draw, of the board and of the goals (scratch counts[2b],
// [2b+1]; sl_exclusive_scan_i64 turns them into each tensor's first uniform).  The work
// of k_env_count (sl_env.hip) on the bit-sliced rule.  (The action ran on lane 0 of
// this wave before: one wave per env for a one-lane latency chain made this launch
// cost as much as a quarter of the step on boards without spawners.)
__global__ void __launch_bounds__(64)
k_stream_prologue64(StepKArgs ka) {
    const sl_env_state &st = ka.st;
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t off = b * (int64_t)(N * N);
    const int lane_off = (lane & 1) * 1024 + (lane >> 1);
    const u32 V = load_record(st, ka.actions, b, lane);
    const Scratch w = scratch_of(ka.fx.scratch, st.B);
    // a board or goals without spawners (spawn_flags, set at reset: no rule or action
    // creates one) draws nothing: its count is 0 without a read
    const int spf = rec(V, R_SPF) | (ka.ctp ? 1 : 0);     // toggling powers can make one
    SpawnCtx sc{0u, 0u, 0ull, 0.0};
    u32 P[32], ch[2];
    int nb = 0;
    if (spf & 1) {
        load_pairs_nt<32>(reinterpret_cast<const u32 *>(st.board + off) + lane_off, P);
        transpose32(P);
        Geo64<SPAWN_COUNT> gbd{lane, StreamSrc{nullptr, 0, nullptr}, 0, 0};
        rule_planes(P, ch, gbd, sc, 0u);
        nb = wave_total(gbd.count);
    }
    // goals at their fixed point (SL_POK_GOALS_FIXED) hold no spawner: no draws
    const int pok = (st.planes && st.planes_ok) ? rec(V, R_POK) & kPokGoalsSkip : 0;
    int ng = 0;
    if ((pok & kPokGoalsSkip) != kPokGoalsSkip && (spf & 2)) {
        if (pok & SL_POK_GOALS_MIRROR) {
            const u32 *mg = st.planes + b * 4096 + 2048 + lane;
#pragma unroll
            for (int q = 0; q < 32; q++) P[q] = mg[q * 64];
        } else {
            load_pairs_nt<32>(reinterpret_cast<const u32 *>(st.goals + off) + lane_off, P);
            transpose32(P);
        }
        Geo64<SPAWN_COUNT> ggl{lane, StreamSrc{nullptr, 0, nullptr}, 0, 0};
        rule_planes(P, ch, ggl, sc, 1u);
        ng = wave_total(ggl.count);
    }
    if (lane == 0) {
        w.counts[2 * b] = nb;
        w.counts[2 * b + 1] = ng;
    }
}

// Resets the envs the step kernel queued (one wave per env, grid-stride over the
// list).  Also zeroes the other step parity's list length for the next step.
// With obs_out, each reset env's packed view is then written from the new episode
// (the step kernel wrote the views of all other envs).
__global__ void __launch_bounds__(64)
k_env_reset_list(sl_env_state st, sl_level_pool pool, ResetArgs ra, int64_t *scratch,
                 uint32_t step, sl::obs::ObsArgs oa, uint64_t chpack, uint32_t one,
                 uint16_t *obs_out) {
    // channel views of the reset envs: their masks
    __shared__ __attribute__((aligned(16))) uint16_t vmask[sl::obs::kFusedChanCells];
    int64_t *cnt = scratch + 8 * st.B + 2;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[(step + 1) & 1] = 0;
    const int32_t *list = reset_list(scratch);
    // the first entry is loaded together with the length (grid <= B <= list size; the
    // value is used only when the entry is in the list)
    const int first = list[blockIdx.x];
    const int n = (int)__builtin_amdgcn_readfirstlane((int)cnt[step & 1]);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t b = __builtin_amdgcn_readfirstlane(i == (int)blockIdx.x ? first : list[i]);
        wave_reset(st, pool, ra, b, threadIdx.x);
        if (obs_out) {
            wait_vm();      // the reset's stores have landed (no stale lines: this wave
                            // alone touches env b, and L1 starts clean each launch)
            const sl::obs::ChanMap cm{chpack, oa.nch};
            uint8_t *o8 = reinterpret_cast<uint8_t *>(obs_out);
            if (oa.mode == SL_OBS_PACKED)
                sl::obs::obs_packed_wave(st, oa, b, threadIdx.x, obs_out);
            else if (oa.mode == SL_OBS_CHANNELS_U8)
                sl::obs::obs_channels_wave<1>(st, oa, cm, one, b, threadIdx.x, vmask, o8);
            else if (oa.mode == SL_OBS_CHANNELS_F32)
                sl::obs::obs_channels_wave<4>(st, oa, cm, one, b, threadIdx.x, vmask, o8);
            else
                sl::obs::obs_channels_wave<2>(st, oa, cm, one, b, threadIdx.x, vmask, o8);
        }
    }
}

template <int MODE>
void launch_bits64(int kind, unsigned grid, const StepKArgs &ka, hipStream_t s) {
    switch (kind) {
    case 0: hipLaunchKernelGGL((k_env_step_bits64<0, MODE>), dim3(grid), dim3(64), 0, s, ka); break;
    case 1: hipLaunchKernelGGL((k_env_step_bits64<1, MODE>), dim3(grid), dim3(64), 0, s, ka); break;
    case 2: hipLaunchKernelGGL((k_env_step_bits64<2, MODE>), dim3(grid), dim3(64), 0, s, ka); break;
    case 3: hipLaunchKernelGGL((k_env_step_bits64<3, MODE>), dim3(grid), dim3(64), 0, s, ka); break;
    default: hipLaunchKernelGGL((k_env_step_bits64<4, MODE>), dim3(grid), dim3(64), 0, s, ka); break;
    }
}

template <u32 K16>
void launch_planes64_chan_k(int esz, unsigned grid, const StepKArgs &ka, hipStream_t s) {
    switch (esz) {
    case 1: hipLaunchKernelGGL((k_env_planes64_chan<K16, 1>), dim3(grid), dim3(64), 0, s, ka); break;
    case 4: hipLaunchKernelGGL((k_env_planes64_chan<K16, 4>), dim3(grid), dim3(64), 0, s, ka); break;
    default: hipLaunchKernelGGL((k_env_planes64_chan<K16, 2>), dim3(grid), dim3(64), 0, s, ka); break;
    }
}

// the plane kernel with channel views: by the keep class (SL_PLAN_KEEP_*) and element size
void launch_planes64_chan(int keep, int esz, unsigned grid, const StepKArgs &ka, hipStream_t s) {
    switch (keep) {
    case SL_PLAN_KEEP_C3: launch_planes64_chan_k<kKeepC3>(esz, grid, ka, s); break;
    case SL_PLAN_KEEP_ALL: launch_planes64_chan_k<kKeepAll>(esz, grid, ka, s); break;
    default: launch_planes64_chan_k<0>(esz, grid, ka, s); break;
    }
}

template <u32 K16>
void launch_planes64_k(int obs, unsigned grid, const StepKArgs &ka, hipStream_t s) {
    if (obs)
        hipLaunchKernelGGL((k_env_step_bits64_planes<K16, 1>), dim3(grid), dim3(64), 0, s, ka);
    else
        hipLaunchKernelGGL((k_env_step_bits64_planes<K16, 0>), dim3(grid), dim3(64), 0, s, ka);
}

// the plane kernel without views or with packed ones
void launch_planes64(int keep, int obs, unsigned grid, const StepKArgs &ka, hipStream_t s) {
    switch (keep) {
    case SL_PLAN_KEEP_C3: launch_planes64_k<kKeepC3>(obs, grid, ka, s); break;
    case SL_PLAN_KEEP_ALL: launch_planes64_k<kKeepAll>(obs, grid, ka, s); break;
    default: launch_planes64_k<0>(obs, grid, ka, s); break;
    }
}

StepKArgs kargs_of(const StepCall &c) {
    return StepKArgs{*c.st, c.a, c.fx, c.actions, c.ctp, c.ctc, c.reward, c.done, c.flags,
                     c.ep_len, c.ep_rew};
}

// replay: the actions (k_env_action, one lane per env), then each env's eligible counts
int counts64(const StepCall &c) {
    const sl_env_state &st = *c.st;
    const int rc = launch_env_action(st, c.actions, c.ctp, c.ctc,
                                     scratch_of(c.fx.scratch, st.B).act, c.s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_stream_prologue64, dim3((unsigned)st.B), dim3(64), 0, c.s, kargs_of(c));
    return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
}

// the kKeepC3 instance the plan names, for a plan without derived planes: its
// k_env_p64_stored16 twin
#define SL_STORED16(KIND, OBS) \
    hipLaunchKernelGGL((k_env_p64_stored16<KIND, OBS>), dim3(grid), dim3(64), 0, s, ka)
bool launch_stored16(const StepPlan &p, unsigned grid, const StepKArgs &ka, hipStream_t s) {
    switch (p.kernel64) {
    case SL_PLAN_K64_PLANES:
        if (p.view_kind) SL_STORED16(0, 1);
        else SL_STORED16(0, 0);
        return true;
    case SL_PLAN_K64_GRAY:
        if (p.view_kind) SL_STORED16(1, 1);
        else SL_STORED16(1, 0);
        return true;
    case SL_PLAN_K64_W6: SL_STORED16(2, 0); return true;
    case SL_PLAN_K64_S6: SL_STORED16(3, 0); return true;
    case SL_PLAN_K64_CHAN:
        if (p.view_kind == 3) SL_STORED16(4, 3);
        else if (p.view_kind == 4) SL_STORED16(4, 4);
        else SL_STORED16(4, 2);
        return true;
    default: return false;
    }
}
#undef SL_STORED16

// the step kernel: the instance the plan names
int step64(const StepCall &c) {
    const StepPlan &p = c.plan;
    const unsigned grid = (unsigned)c.st->B;
    const StepKArgs ka = kargs_of(c);
    hipStream_t s = c.s;
    // the one place the derived planes choose a kernel: the plan's `derived` (both planes or
    // none in the kKeepC3 class, whose instances have 0x8100 compiled in)
    if (p.keep == SL_PLAN_KEEP_C3 && p.derived == 0 && launch_stored16(p, grid, ka, s))
        return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
    switch (p.kernel64) {
    case SL_PLAN_K64_BITS64:
        if (p.replay) launch_bits64<SPAWN_STREAM>(p.view_kind, grid, ka, s);
        else launch_bits64<SPAWN_PHILOX>(p.view_kind, grid, ka, s);
        break;
    case SL_PLAN_K64_PLANES: launch_planes64(p.keep, p.view_kind, grid, ka, s); break;
    case SL_PLAN_K64_CHAN: launch_planes64_chan(p.keep, obs_esz(p.view_kind), grid, ka, s); break;
    case SL_PLAN_K64_GRAY:       // goals all black or white: the instances that skip their colours
        if (p.view_kind)
            hipLaunchKernelGGL((k_env_planes64_gray<kKeepC3, 1>), dim3(grid), dim3(64), 0, s, ka);
        else                     // (sl_env_cfg.planes64_waves 5: the five-wave twin)
            hipLaunchKernelGGL((k_env_planes64_gray<kKeepC3, 0>), dim3(grid), dim3(64), 0, s, ka);
        break;
    case SL_PLAN_K64_S6:
        hipLaunchKernelGGL((k_env_planes64_s6<kKeepC3>), dim3(grid), dim3(64), 0, s, ka);
        break;
    case SL_PLAN_K64_W6:
        hipLaunchKernelGGL((k_env_planes64_w6<kKeepC3>), dim3(grid), dim3(64), 0, s, ka);
        break;
    default: return SL_EINVAL;
    }
    return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
}

// the finished envs: the split pair's tail (the epilogue of every env, then the resets),
// or the resets of the envs the step kernel listed, with their views
int resets64(const StepCall &c) {
    const sl_env_state &st = *c.st;
    const FastExtra &fx = c.fx;
    if (c.plan.resets == SL_PLAN_RESETS_SPLIT_TAIL64) {
        const unsigned tgrid = (unsigned)((st.B + kTailThreads - 1) / kTailThreads);
        hipLaunchKernelGGL(k_env_epilogue_reset64, dim3(tgrid), dim3(kTailThreads), 0, c.s, st, c.a,
                           fx.pool, fx.ra, fx.scratch, c.reward, c.done, c.flags, c.ep_len,
                           c.ep_rew);
    } else {
        const unsigned grid = (unsigned)(st.B < 512 ? st.B : 512);
        hipLaunchKernelGGL(k_env_reset_list, dim3(grid), dim3(64), 0, c.s, st, fx.pool, fx.ra,
                           fx.scratch, c.a.step, c.plan.oa, fx.obs_chpack, fx.obs_one, fx.obs_out);
    }
    return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
}

}  // namespace

namespace sl {

bool planes64_shape(const sl_env_state &st) {
    return st.H == N && st.W == N && st.planes && st.planes_ok && st.board_planes == st.planes;
}

int sync_board_planes64(const sl_env_state &st, int demote, hipStream_t s) {
    if (!planes64_shape(st) || st.B <= 0) return SL_OK;
    hipLaunchKernelGGL(k_board_sync64, dim3((unsigned)st.B), dim3(64), 0, s, st, demote);
    return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
}

int planes64_keep(const sl_env_state &st) {
    const u32 keep = ~st.board_zero & 0xFFFFu;
    // the <kKeepC3, *> instances fix the agent planes as well: a batch holding those
    // planes whose agent planes differ takes the run-time instance
    if (keep == kKeepC3) return st.agent_planes == kAgentC3 ? SL_PLAN_KEEP_C3 : SL_PLAN_KEEP_RUNTIME;
    return keep == kKeepAll ? SL_PLAN_KEEP_ALL : SL_PLAN_KEEP_RUNTIME;
}

const StepHooks &hooks_64() {
    static const StepHooks h = {counts64, nullptr, step64, resets64, false};
    return h;
}

}  // namespace sl
