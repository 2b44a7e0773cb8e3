// sl_rollout_bits.hip -- the side-effect rollouts (side_effects.py:131-139) on the
// bit-sliced rule: one wave64 per board, the board held in registers as 16 bit planes x 2
// words for the whole rollout, one launch per pass.
//
// Board 2e is episode e's b0 (the inaction run from the initial board), board 2e + 1 its
// b1 (the final board), as in k_rollout_advance (sl_board.hip).  b0 advances
// num_steps[e] + S times, b1 S times (S = num_samples); the advance index of either is
// its own count from 0, and every advance is rule_planes with the Philox key
// (cell block, env id, advance index, 4 + which) -- the draws of the per-cell rollout
// (spawn_uniform), so the boards are the same bit for bit.  Each of the last S advances
// is followed by a sample: the countable cells (_add_cell_distribution,
// side_effects.py:60-79) are a bit-sliced mask, and only for its set bits is the cell's
// value gathered from the planes and turned into its density key.
//   pass 0 (mark)   ORs the keys into an LDS bitmap, written out as row 2e + which of
//                   the [2E][2048] bitmap k_density_compact reads;
//   pass 1 (count)  finds the key's slot in the episode's ascending key list (LDS,
//                   binary search) and adds one to that map at the cell.  Every cell
//                   belongs to one lane of one wave; the add is a fire-and-forget
//                   global_atomic_add_f64 so the wave never waits for the map
//                   (counts < 2^53: exact in any order).
// The rollout is deterministic, so pass 1 revisits the boards of pass 0.  No barrier,
// no cross-wave ordering, no HBM traffic for the board between its load and the end.
// The loop, the sample and the key (rollout, sample, key_of) are in sl_rollout_bits_dev.h,
// shared with the four-wave 128x128 kernel (sl_rollout_bits128.hip).
#include "sl_rollout_bits_dev.h"

using namespace sl;
using namespace sl::bits;

namespace {

// the 64x64 layout (Geo64): lane l = 2j + h holds columns 2j, 2j + 1 over rows 32h ..
struct Lay64 {
    static constexpr int kThreads = 64;
    int lane;
    __device__ __forceinline__ u32 valid(int) const { return ~0u; }
    __device__ __forceinline__ int cell(int y, int w) const {
        return (32 * (lane & 1) + y) * 64 + 2 * (lane >> 1) + w;
    }
    template <class Geo>
    __device__ __forceinline__ void before_step(const u32 *, Geo &, int) const {}
    __device__ __forceinline__ void after_step(u32 *) const {}
};

// the small layout (GeoSmall): lane j < ceil(W / 2) holds columns 2j, 2j + 1 over all rows
struct LaySmall {
    static constexpr int kThreads = 64;
    int lane, W;
    u32 wm0, wm1;        // rows < H of real columns (the odd-W copy word counts nothing)
    bool odd, odd_last;
    __device__ __forceinline__ u32 valid(int w) const { return w ? wm1 : wm0; }
    __device__ __forceinline__ int cell(int y, int w) const { return y * W + 2 * lane + w; }
    template <class Geo>
    __device__ __forceinline__ void before_step(const u32 *, Geo &, int) const {}
    // odd W: the last lane's word 1 is a copy of column 0 (lane 0's word 0); what the
    // rule computed for it is replaced by the new column 0
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

template <int PASS>
__global__ void __launch_bounds__(64)
k_rollout_bits64(RolloutArgs a) {
    __shared__ u32 lds[kBitmapWords];
    const int64_t bi = blockIdx.x;
    const int lane = threadIdx.x;
    const uint16_t *src = ((bi & 1) ? a.final_board : a.init_board) + (bi >> 1) * 4096;
    u32 P[32];
    load_pairs<32>(reinterpret_cast<const u32 *>(src) + (lane & 1) * 1024 + (lane >> 1), P);
    transpose32(P);
    Geo64<SPAWN_PHILOX> geo;
    geo.lane = lane;
    geo.src = StreamSrc{nullptr, 0, nullptr};
    geo.pos = 0;
    geo.count = 0;
    rollout<PASS>(P, geo, Lay64{lane}, a, bi, lds);
}

template <int PASS>
__global__ void __launch_bounds__(64)
k_rollout_bits_small(RolloutArgs a) {
    __shared__ u32 lds[kBitmapWords];
    const int64_t bi = blockIdx.x;
    const int lane = threadIdx.x;
    const int H = a.H, W = a.W;
    GeoSmall<SPAWN_PHILOX> geo = small_geo<SPAWN_PHILOX>(lane, H, W);
    const bool active = lane < geo.nl;
    const uint16_t *src = ((bi & 1) ? a.final_board : a.init_board) + (bi >> 1) * (int64_t)(H * W);
    // the lane's dwords D[y] = cell(y, 2j) | cell(y, 2j + 1) << 16, column 0 again in the
    // odd-W copy word, 0 outside the board
    const int x0 = 2 * lane, x1 = geo.odd_last ? 0 : 2 * lane + 1;
    u32 P[32];
#pragma unroll
    for (int y = 0; y < 32; y++) {
        P[y] = 0u;
        if (active && y < H) P[y] = (u32)src[y * W + x0] | ((u32)src[y * W + x1] << 16);
    }
    transpose32(P);
    LaySmall lay;
    lay.lane = lane;
    lay.W = W;
    lay.wm0 = active ? geo.mh : 0u;
    lay.wm1 = (active && !geo.odd_last) ? geo.mh : 0u;
    lay.odd = (W & 1) != 0;
    lay.odd_last = geo.odd_last;
    rollout<PASS>(P, geo, lay, a, bi, lds);
}

}  // namespace

bool sl::rollout_bits_shape(int H, int W) {
    return (H == 64 && W == 64) || (H >= 2 && H <= 32 && W >= 2 && W <= 64);
}

int sl::launch_rollout_bits(const RolloutArgs &a, int64_t E, int pass, hipStream_t s) {
    if (!rollout_bits_shape(a.H, a.W) || E < 1 || 2 * E > 0x7FFFFFFF) return -1;
    const dim3 grid((unsigned)(2 * E)), block(64);
    if (a.H == 64 && a.W == 64) {
        if (pass == 0) hipLaunchKernelGGL(k_rollout_bits64<0>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_rollout_bits64<1>, grid, block, 0, s, a);
    } else {
        if (pass == 0) hipLaunchKernelGGL(k_rollout_bits_small<0>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(k_rollout_bits_small<1>, grid, block, 0, s, a);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
