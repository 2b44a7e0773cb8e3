// sl_rollout_bits_mid.hip -- the side-effect rollouts (side_effects.py:131-139) of boards
// of 33 to 64 rows and 2 to 64 columns, 64x64 aside, on the bit-sliced rule: one wave64
// per board, the board held in registers as 16 bit planes x 2 words for the whole
// rollout, one launch per pass (SL_KERNEL_MID).
//
// The boards, their advance counts, the Philox key (cell block, env id, the board's own
// advance index, 4 + which) and the two passes are those of sl_rollout_bits.hip (the loop
// itself is shared: rollout<PASS>, sl_rollout_bits_dev.h), so the boards are those of
// k_rollout_advance bit for bit.  The layout is the mid step kernel's (GeoMid,
// sl_bits_geo.h; sl_bits_mid.hip): lane l = 2j + h holds the column pair (2j, 2j + 1),
// j < nl = ceil(W / 2), over rows 32h .. 32h + 31, of which rows < H are real.  The step
// kernel loads the board anew every step; here it is loaded once, so the column-0 copy
// of an odd board is kept up by LayMid::after_step.
#include "sl_rollout_bits_dev.h"

using namespace sl;
using namespace sl::bits;

namespace {

// the mid layout (GeoMid): lane l = 2j + h, j < ceil(W / 2), holds columns 2j, 2j + 1 over
// rows 32h .. 32h + 31
struct LayMid {
    static constexpr int kThreads = 64;
    int lane, W;
    u32 wm0, wm1;        // real rows of real columns (the odd-W copy word counts nothing;
                         // nor do the upper word's bits >= H - 32, which the rule keeps 0)
    bool odd, odd_last;
    __device__ __forceinline__ u32 valid(int w) const { return w ? wm1 : wm0; }
    __device__ __forceinline__ int cell(int y, int w) const {
        return (32 * (lane & 1) + y) * W + 2 * (lane >> 1) + w;
    }
    template <class Geo>
    __device__ __forceinline__ void before_step(const u32 *, Geo &, int) const {}
    // odd W: the last pair's word 1 is a copy of column 0 of the same half (word 0 of
    // lane h); what the rule computed for it is replaced by the new column 0
    __device__ __forceinline__ void after_step(u32 *P) const {
        if (odd) {
            const bool hi = (lane & 1) != 0;
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const u32 lo0 = (u32)__builtin_amdgcn_readlane((int)PL(P, k, 0), 0);
                const u32 hi0 = (u32)__builtin_amdgcn_readlane((int)PL(P, k, 0), 1);
                PL(P, k, 1) = odd_last ? (hi ? hi0 : lo0) : PL(P, k, 1);
            }
        }
    }
};

template <int PASS>
__global__ void __launch_bounds__(64)
k_rollout_bits_mid(RolloutArgs a) {
    __shared__ u32 lds[kBitmapWords];
    const int64_t bi = blockIdx.x;
    const int lane = threadIdx.x, h = lane & 1, j = lane >> 1;
    const int H = a.H, W = a.W;
    GeoMid<SPAWN_PHILOX> geo = mid_geo<SPAWN_PHILOX>(lane, H, W);
    const bool active = j < geo.nl;
    const uint16_t *src = ((bi & 1) ? a.final_board : a.init_board) + (bi >> 1) * (int64_t)(H * W);
    // the lane's dwords D[y] = cell(32h + y, 2j) | cell(32h + y, 2j + 1) << 16, column 0
    // again in the odd-W copy word, 0 outside the board (uint16 reads: no alignment rule)
    const int x0 = 2 * j, x1 = geo.odd_last ? 0 : 2 * j + 1;
    const int rows = active ? min(32, H - 32 * h) : 0;     // this half's real rows
    const uint16_t *p = src + 32 * h * W;
    u32 P[32];
#pragma unroll
    for (int y = 0; y < 32; y++) {
        P[y] = 0u;
        if (y < rows) P[y] = (u32)p[y * W + x0] | ((u32)p[y * W + x1] << 16);
    }
    transpose32(P);
    LayMid lay;
    lay.lane = lane;
    lay.W = W;
    lay.wm0 = active ? geo.mh : 0u;
    lay.wm1 = (active && !geo.odd_last) ? geo.mh : 0u;
    lay.odd = (W & 1) != 0;
    lay.odd_last = geo.odd_last;
    rollout<PASS>(P, geo, lay, a, bi, lds);
}

}  // namespace

// mid_shape's range (sl_bits_mid.hip)
bool sl::rollout_mid_shape(int H, int W) {
    return H >= 33 && H <= 64 && W >= 2 && W <= 64 && !(H == 64 && W == 64);
}

int sl::launch_rollout_mid(const RolloutArgs &a, int64_t E, int pass, hipStream_t s) {
    if (!rollout_mid_shape(a.H, a.W) || E < 1 || 2 * E > 0x7FFFFFFF) return -1;
    const dim3 grid((unsigned)(2 * E)), block(64);
    if (pass == 0) hipLaunchKernelGGL(k_rollout_bits_mid<0>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_rollout_bits_mid<1>, grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
