// sl_rollout_bits_wide.hip -- the side-effect rollouts (side_effects.py:131-139) of the
// boards of up to 128 x 128 with more than 64 rows or more than 64 columns, 128x128 aside
// (wide_shape: 80x80, 96x96, 100x100, 40x128, 128x64), on the bit-sliced rule: one
// workgroup of NB = ceil(H / 32) wave64 per board, the board held in registers for the
// whole rollout, one launch per pass (SL_KERNEL_WIDE).
//
// The boards, their advance counts, the Philox key (cell block, env id, the board's own
// advance index, 4 + which) and the two passes are those of sl_rollout_bits.hip (the loop
// itself is shared: rollout<PASS>, sl_rollout_bits_dev.h), so the boards are those of
// k_rollout_advance bit for bit.  The layout is the wide step kernel's (GeoWide,
// sl_bits_geo.h; sl_bits_wide.hip) with the bands side by side, as in the 128x128 band
// rollout, instead of one after another: wave t holds band t (rows 32t .. 32t + 31) as 16
// planes x 2 words, lane j < nl = ceil(W / 2) the column pair 2j, 2j + 1, from its one load
// to the end.  For odd W the last pair's word 1 is a copy of column 0; lanes >= nl and the
// rows past H - 1 in the last band hold zeros.  The step kernel loads its board anew every
// step; here it is loaded once, so the column-0 copy is kept up by LayWide::after_step.
//
// What a band needs from its neighbours is one row each (GeoWide's HaloView).  Per advance
// every wave gathers its row 0 and its last real row (geo.sd: row 31 but in the last band)
// from the planes into cell-pair dwords, writes them to an LDS halo buffer, and after one
// workgroup barrier reads `up` from band (t + NB - 1) % NB's last real row and `dn` from
// band (t + 1) % NB's row 0 (row H - 1 wraps to row 0; at NB = 1 the wave reads its own
// rows), so every wave advances the pre-step board.  The rows are gathered after the
// copy-word refresh of the previous advance, so the last lane's upper half is column 0 of
// the halo row.  All waves of a workgroup work on one board and run the same number of
// advances, so the barrier is uniform.
//
// What holds no cell stays 0 through the rule itself; after_step does not mask.  In a row
// past H - 1 every neighbour word is masked with mh (GeoWide::vert; mh is wave-uniform, so
// the words that come through horiz are masked too), so the alive count there is 0 and no
// cell is born; nothing alive is there to die; and GeoWide::spawn masks the eligible cells
// with mh.  A lane >= nl permutes with itself and reads its own halo rows: all of its
// inputs are 0, and of all-zero inputs the rule changes nothing.  (The step kernel masks
// after the rule because its loads repeat the last row; the loads here leave such rows 0.)
//
// LDS per workgroup: the 8 KiB key bitmap (pass 0; pass 1: the episode's key list) that
// the waves share, and the two halo buffers (2 x NB x 2 x 64 dwords: 1 to 4 KiB).  Pass 0
// ORs keys into the shared bitmap with LDS atomics; pass 1's adds go to cells no other
// lane of any wave holds.
#include "sl_rollout_bits_dev.h"

using namespace sl;
using namespace sl::bits;

namespace {

typedef __attribute__((address_space(3))) u32 lds_u32;

// wave `band` of the workgroup holds rows 32 band .. 32 band + 31, lane j < nl columns 2j,
// 2j + 1 (GeoWide)
template <int NB>
struct LayWide {
    static constexpr int kThreads = 64 * NB;
    static constexpr int kHaloWords = NB * 2 * 64;  // one halo buffer: per band its row 0
                                                    // and its last real row
    int lane, band, W;
    u32 wm0, wm1;        // real rows of real columns (the odd-W copy word counts nothing)
    bool odd, odd_last;
    lds_u32 *halo;       // [2][NB][2][64]
    __device__ __forceinline__ u32 valid(int w) const { return w ? wm1 : wm0; }
    __device__ __forceinline__ int cell(int y, int w) const {
        return (32 * band + y) * W + 2 * lane + w;
    }
    // The halo exchange of advance `it`.  Two buffers alternate by the advance's parity,
    // so one barrier per advance is enough (Lay128::before_step, sl_rollout_bits128.hip).
    __device__ __forceinline__ void before_step(const u32 *P, GeoWide<SPAWN_PHILOX> &geo,
                                                int it) const {
        u32 r0 = 0u, rl = 0u;           // bit k + 16 w = bit k of cell (row, 2 lane + w)
        const u32 sh = 31u - (u32)geo.sd;
#pragma unroll
        for (int k = 0; k < 32; k++) r0 = __builtin_amdgcn_alignbit(P[k], r0, 1);
#pragma unroll
        for (int k = 31; k >= 0; k--) rl = __builtin_amdgcn_alignbit(rl, P[k] << sh, 31);
        lds_u32 *h = halo + (it & 1) * kHaloWords;
        h[(2 * band) * 64 + lane] = r0;
        h[(2 * band + 1) * 64 + lane] = rl;
        __syncthreads();
        const int above = band == 0 ? NB - 1 : band - 1, below = band == NB - 1 ? 0 : band + 1;
        geo.hv.up = h[(2 * above + 1) * 64 + lane];
        geo.hv.dn = h[(2 * below) * 64 + lane];
    }
    // odd W: the last pair's word 1 is a copy of the band's column 0 (word 0 of lane 0);
    // what the rule computed for it is replaced by the new column 0
    __device__ __forceinline__ void after_step(u32 *P) const {
        if (odd) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const u32 c0 = (u32)__builtin_amdgcn_readlane((int)PL(P, k, 0), 0);
                PL(P, k, 1) = odd_last ? c0 : PL(P, k, 1);
            }
        }
    }
};

template <int PASS, int NB>
__global__ void __launch_bounds__(64 * NB)
k_rollout_bits_wide(RolloutArgs a) {
    __shared__ u32 lds[kBitmapWords];
    __shared__ u32 halo_[2 * LayWide<NB>::kHaloWords];
    const int64_t bi = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int band = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int H = a.H, W = a.W;
    GeoWide<SPAWN_PHILOX> geo = wide_geo<SPAWN_PHILOX>(lane, H, W, 32 * band);
    const bool active = lane < geo.nl;
    const uint16_t *src = ((bi & 1) ? a.final_board : a.init_board) + (bi >> 1) * (int64_t)(H * W);
    // the lane's dwords D[y] = cell(32 band + y, 2j) | cell(32 band + y, 2j + 1) << 16,
    // column 0 again in the odd-W copy word, 0 outside the board
    const int c0 = 2 * lane, c1 = geo.odd_last ? 0 : c0 + 1;
    const int rows = active ? min(32, H - 32 * band) : 0;      // this band's real rows
    u32 P[32];
#pragma unroll
    for (int y = 0; y < 32; y++) {
        P[y] = 0u;
        if (y < rows) P[y] = hbm_row(src, W, 32 * band + y, c0, c1);
    }
    transpose32(P);
    LayWide<NB> lay;
    lay.lane = lane;
    lay.band = band;
    lay.W = W;
    lay.wm0 = active ? geo.mh : 0u;
    lay.wm1 = (active && !geo.odd_last) ? geo.mh : 0u;
    lay.odd = (W & 1) != 0;
    lay.odd_last = geo.odd_last;
    lay.halo = (lds_u32 *)halo_;
    rollout<PASS>(P, geo, lay, a, bi, lds);
}

template <int NB>
int launch_nb(const RolloutArgs &a, int64_t E, int pass, hipStream_t s) {
    const dim3 grid((unsigned)(2 * E)), block(64 * NB);
    if (pass == 0) hipLaunchKernelGGL((k_rollout_bits_wide<0, NB>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_rollout_bits_wide<1, NB>), grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

// wide_shape's range (sl_bits_wide.hip)
bool sl::rollout_wide_shape(int H, int W) { return wide_shape(H, W); }

int sl::launch_rollout_wide(const RolloutArgs &a, int64_t E, int pass, hipStream_t s) {
    if (!rollout_wide_shape(a.H, a.W) || E < 1 || 2 * E > 0x7FFFFFFF) return -1;
    switch ((a.H + 31) >> 5) {          // bands = waves per workgroup
    case 1: return launch_nb<1>(a, E, pass, s);
    case 2: return launch_nb<2>(a, E, pass, s);
    case 3: return launch_nb<3>(a, E, pass, s);
    default: return launch_nb<4>(a, E, pass, s);
    }
}
