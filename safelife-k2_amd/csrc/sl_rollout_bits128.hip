// sl_rollout_bits128.hip -- the side-effect rollouts (side_effects.py:131-139) of 128x128
// boards on the bit-sliced rule: one workgroup of four wave64 per board, the board held
// in registers for the whole rollout, one launch per pass (SL_KERNEL_BANDS).
//
// The boards, their advance counts, the Philox key (cell block, env id, the board's own
// advance index, 4 + which) and the two passes are those of sl_rollout_bits.hip (the loop
// itself is shared: rollout<PASS>, sl_rollout_bits_dev.h), so the boards are those of
// k_rollout_advance bit for bit.  The layout is the 128x128 step kernel's (sl_bits128.hip)
// with the four bands side by side instead of one after another: wave t holds band t
// (rows 32t .. 32t + 31) as 16 planes x 2 words, lane j the column pair 2j, 2j + 1, from
// its one load (32 row dwords, transposed) to the end.
//
// What a band needs from its neighbours is one row each (GeoBand's HaloView).  Per
// advance every wave gathers its rows 0 and 31 from the planes into cell-pair dwords,
// writes them to an LDS halo buffer, and after one workgroup barrier reads `up` from
// wave (t + 3) & 3's row 31 and `dn` from wave (t + 1) & 3's row 0 (row 127 wraps to row
// 0), so every wave advances the pre-step board.  All four waves work on one board and
// run the same number of advances, so the barrier is uniform.
//
// LDS per workgroup: the 8 KiB key bitmap (pass 0; pass 1: the episode's key list) that
// the four waves share, one compact_draws slot array per wave (4 x 2 KiB), and the two
// halo buffers (2 x 2 KiB).  Pass 0 ORs keys into the shared bitmap with LDS atomics;
// pass 1's adds go to cells no other lane of any wave holds.
#include "sl_rollout_bits_dev.h"

using namespace sl;
using namespace sl::bits;

namespace {

constexpr int N = 128;                  // rows = columns
constexpr int NB = N / 32;              // bands = waves per workgroup
constexpr int RS = N / 2;               // dwords per row
constexpr int kHaloWords = NB * 2 * 64; // one halo buffer: per band its rows 0 and 31

typedef __attribute__((address_space(3))) u32 lds_u32;

// wave `band` of the workgroup holds rows 32 band .. 32 band + 31, lane j columns 2j, 2j + 1
struct Lay128 {
    static constexpr int kThreads = 64 * NB;
    int lane, band;
    lds_u32 *halo;                      // [2][NB][2][64]
    __device__ __forceinline__ u32 valid(int) const { return ~0u; }
    __device__ __forceinline__ int cell(int y, int w) const {
        return (32 * band + y) * N + 2 * lane + w;
    }
    // The halo exchange of advance `it`.  Two buffers alternate by the advance's parity,
    // so one barrier per advance is enough: a wave that runs ahead after the barrier
    // writes the other buffer, and it can write this one again only at advance it + 2,
    // after the barrier of advance it + 1 -- which every wave reaches only once it has
    // read its halo rows of advance `it`.
    __device__ __forceinline__ void before_step(const u32 *P, GeoBand<SPAWN_PHILOX> &geo,
                                                int it) const {
        u32 r0 = 0u, r31 = 0u;          // bit k + 16 w = bit k of cell (row, 2 lane + w)
#pragma unroll
        for (int k = 0; k < 32; k++) r0 = __builtin_amdgcn_alignbit(P[k], r0, 1);
#pragma unroll
        for (int k = 31; k >= 0; k--) r31 = __builtin_amdgcn_alignbit(r31, P[k], 31);
        lds_u32 *h = halo + (it & 1) * kHaloWords;
        h[(2 * band) * 64 + lane] = r0;
        h[(2 * band + 1) * 64 + lane] = r31;
        __syncthreads();
        geo.hv.up = h[(2 * ((band + NB - 1) & (NB - 1)) + 1) * 64 + lane];
        geo.hv.dn = h[(2 * ((band + 1) & (NB - 1))) * 64 + lane];
    }
    __device__ __forceinline__ void after_step(u32 *) const {}
};

template <int PASS>
__global__ void __launch_bounds__(64 * NB)
k_rollout_bands128(RolloutArgs a) {
    __shared__ u32 lds[kBitmapWords];
    __shared__ uint16_t slots_[NB * kDrawSlots];
    __shared__ u32 halo_[2 * kHaloWords];
    const int64_t bi = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int band = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint16_t *src = ((bi & 1) ? a.final_board : a.init_board) + (bi >> 1) * (N * N);
    u32 P[32];
    load_pairs<RS>(reinterpret_cast<const u32 *>(src) + band * 32 * RS + lane, P);
    transpose32(P);
    GeoBand<SPAWN_PHILOX> geo{lane, 32 * band, HaloView{0u, 0u}, StreamSrc{nullptr, 0, nullptr},
                              0, 0, 0, (lds_u16 *)slots_ + band * kDrawSlots};
    rollout<PASS>(P, geo, Lay128{lane, band, (lds_u32 *)halo_}, a, bi, lds);
}

}  // namespace

bool sl::rollout_bands_shape(int H, int W) { return H == N && W == N; }

int sl::launch_rollout_bands(const RolloutArgs &a, int64_t E, int pass, hipStream_t s) {
    if (!rollout_bands_shape(a.H, a.W) || E < 1 || 2 * E > 0x7FFFFFFF) return -1;
    const dim3 grid((unsigned)(2 * E)), block(64 * NB);
    if (pass == 0) hipLaunchKernelGGL(k_rollout_bands128<0>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_rollout_bands128<1>, grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}
