// sl_rollout_bits_dev.h -- the device code the bit-sliced side-effect rollout kernels
// share (sl_rollout_bits.hip: one wave per board; sl_rollout_bits128.hip: four waves per
// 128x128 board): the density key, the sample after an advance, and the rollout loop.
//
// A kernel supplies the planes P of the calling wave, the geometry policy of rule_planes
// (sl_bits_geo.h) and a layout policy Lay:
//   Lay::kThreads          threads of the workgroup (they share the LDS bitmap / key list);
//   lay.valid(w)           the rows of word w that are board cells;
//   lay.cell(y, w)         the board's cell index of bit y of word w;
//   lay.before_step(P, geo, it)   what the geometry needs before advance `it` (the band
//                          kernel's halo exchange; may hold a workgroup barrier, so every
//                          wave of a workgroup runs the same number of advances);
//   lay.after_step(P)      fix-ups of the planes after an advance.
#pragma once
#include "sl_bits_geo.h"
#include "sl_rollout_bits.h"

namespace sl {
namespace bits {

constexpr int kBitmapWords = 2048;      // 65536 keys, one bit each

// the density key of a counted cell (density_key, sl_board.hip; c is never 0 here)
__device__ __forceinline__ u32 key_of(u32 c) {
    u32 m = c & ~DESTR & 0xFFFFu;
    const u32 base = m & ~COLORS;
    if (base == ALIVE || base == (FROZEN | SPAWN)) m |= DESTR;
    return m;
}

template <int PASS, class Lay>
__device__ __forceinline__ void sample(const u32 P[32], const Lay &lay, u32 *lds, int nk,
                                       double *dens, int hw) {
#pragma unroll
    for (int w = 0; w < 2; w++) {
        u32 nz = 0u;        // c & ~DESTR != 0
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k != 3) nz |= PL(P, k, w);
        // (c & (FROZEN | DESTR | MOVABLE)) == FROZEN
        const u32 fixed = PL(P, 4, w) & ~(PL(P, 3, w) | PL(P, 2, w) | PL(P, 15, w));
        u32 m = nz & ~fixed & ~PL(P, 1, w) & lay.valid(w);
        while (m) {
            const int y = __builtin_ctz(m);
            m &= m - 1;
            u32 c = 0u;
#pragma unroll
            for (int k = 0; k < 16; k++) c |= ((PL(P, k, w) >> y) & 1u) << k;
            const u32 key = key_of(c);
            if (PASS == 0) {
                atomicOr(&lds[key >> 5], 1u << (key & 31));
            } else {
                const uint16_t *kl = reinterpret_cast<const uint16_t *>(lds);
                int lo = 0, hi = nk - 1;             // keys ascending
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (kl[mid] < key) lo = mid + 1;
                    else hi = mid;
                }
                if (nk > 0 && kl[lo] == key)         // else: key overflow (n_keys > max_keys)
                    atomicAdd(&dens[(int64_t)lo * hw + lay.cell(y, w)], 1.0);
            }
        }
    }
}

// The rollout of board bi by the workgroup's waves, each on its own planes P: lds is the
// workgroup's 8 KiB (pass 0: the key bitmap; pass 1: the episode's key list).
template <int PASS, class Geo, class Lay>
__device__ __forceinline__ void rollout(u32 P[32], Geo &geo, const Lay &lay,
                                        const RolloutArgs &a, int64_t bi, u32 *lds) {
    const int64_t e = bi >> 1;
    const int which = (int)(bi & 1);
    const int tid = threadIdx.x;
    const int hw = a.H * a.W;
    const int st = __builtin_amdgcn_readfirstlane(a.steps[e]);
    const int first = which == 0 ? st : 0, n_adv = first + a.S;
    int nk = 0;
    double *dens = nullptr;
    if (PASS == 0) {
        for (int i = tid; i < kBitmapWords; i += Lay::kThreads) lds[i] = 0u;
    } else {
        nk = __builtin_amdgcn_readfirstlane(a.n_keys[e]);
        nk = nk < a.max_keys ? nk : a.max_keys;
        uint16_t *kl = reinterpret_cast<uint16_t *>(lds);
        for (int k = tid; k < nk; k += Lay::kThreads) kl[k] = a.keys[e * a.max_keys + k];
        dens = (which == 0 ? a.inaction : a.action) + e * (int64_t)a.max_keys * hw;
    }
    __syncthreads();        // the LDS fill, before any wave of the workgroup samples
    SpawnCtx sc;
    sc.gid = a.env_ids ? a.env_ids[e] : a.env0 + (uint32_t)e;
    sc.gid = (uint32_t)__builtin_amdgcn_readfirstlane((int)sc.gid);
    sc.seed = a.seed;
    set_spawn_prob(sc, a.spawn_prob[e]);
    const u32 tensor = 4u + (u32)which;
#pragma unroll 1
    for (int it = 0; it < n_adv; it++) {
        sc.step = (uint32_t)it;
        u32 chg[2];
        lay.before_step(P, geo, it);
        rule_planes(P, chg, geo, sc, tensor);
        lay.after_step(P);
        if (it >= first) sample<PASS>(P, lay, lds, nk, dens, hw);
    }
    if (PASS == 0) {
        __syncthreads();    // every wave's keys are in the bitmap
        uint32_t *row = a.bitmap + bi * kBitmapWords;
        for (int i = tid; i < kBitmapWords; i += Lay::kThreads) row[i] = lds[i];
    }
}

}  // namespace bits
}  // namespace sl
