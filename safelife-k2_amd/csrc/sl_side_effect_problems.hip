// sl_side_effect_problems.hip -- the EMD problems of side_effect_score, cut from the
// dense density maps on the device (gfx950).
//
// earth_mover_distance (side_effects.py:36-43) keeps, of two [H, W] maps a and b, the
// cells with |a - b| > 1e-3 * max |a - b|, in row-major order; only those few cells go
// to the EMD.  Here that selection runs on the maps sl_side_effect_densities_k left in
// device memory, so that a caller copies a few KB per problem instead of both maps.
//
// A problem is one (episode e, key slot k), index e * max_keys + k, with
// k < min(n_keys[e], max_keys); the other slots are never read and have 0 cells and
// mass 0.  A key absent from one run is an all-zero map (sl_side_effect_densities_k
// zeroes both tensors), so `present` is not consulted.
//
//   sl_side_effect_problem_counts   k_problem_count (one workgroup per slot), then
//                                   sl_exclusive_scan_i64 over the counts
//   sl_side_effect_problem_cells    k_problem_fill  (one workgroup per slot; slots with
//                                   no cell leave at once)
//
// The grand total: the count array has one trailing zero (written by workgroup 0 of
// k_problem_count) and the scan runs over all E * max_keys + 1 entries, so its last
// output, offsets[E * max_keys], is the number of cells of all problems.
//
// Arithmetic: gap = |a - b| (one subtraction, one fabs), gmax its maximum (order-free,
// hence exact), thr = 1e-3 * gmax (one multiplication), selected iff gap > thr: the
// IEEE operations numpy performs.  The file is built with -ffp-contract=off (Makefile
// FLAGS), so none of them is fused.  The fill pass compares against the stored thr.
//
// mass = sum of a, in this fixed order: thread t of the 256 adds cells t, t + 256,
// t + 512, ... in ascending order into one accumulator starting at 0.0; each wave then
// combines its 64 accumulators by a butterfly (lane l adds lane l ^ 32, then ^ 16, ^ 8,
// ^ 4, ^ 2, ^ 1: every lane ends with the same value); thread 0 adds the four wave sums
// in wave order.  It differs from numpy's pairwise sum by rounding only.
//
// Each problem's maps are read twice by the count pass and once by the fill pass, 8
// bytes per lane, coalesced; a pair of maps (64 KiB at 64x64, 256 KiB at 128x128) stays
// in L2 between the reads.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/safelife_hip.h"

namespace {

constexpr int NT = 256;                      // four waves per problem
constexpr int kMaxCells = 32768;             // hw limit of the density entry points

struct Problem {
    const double *a, *b;                     // inaction, action maps; null: empty slot
};

__device__ __forceinline__ Problem problem_maps(const double *inaction, const double *action,
                                                const int32_t *n_keys, int max_keys, int hw) {
    const int64_t prob = blockIdx.x;
    const int64_t e = prob / max_keys;
    const int k = (int)(prob - e * max_keys);
    const int nk = n_keys[e] < max_keys ? n_keys[e] : max_keys;
    if (k >= nk) return Problem{nullptr, nullptr};
    return Problem{inaction + prob * hw, action + prob * hw};
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ double wave_add(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(NT)
k_problem_count(const double *__restrict__ inaction, const double *__restrict__ action,
                const int32_t *__restrict__ n_keys, int max_keys, int hw, int64_t nprob,
                int64_t *__restrict__ count, double *__restrict__ thr_out,
                double *__restrict__ mass_out) {
    __shared__ double w_max[NT / 64], w_sum[NT / 64];
    __shared__ int w_cnt[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t prob = blockIdx.x;
    if (prob == 0 && tid == 0) count[nprob] = 0;         // the scan's trailing zero
    const Problem P = problem_maps(inaction, action, n_keys, max_keys, hw);
    if (!P.a) {                                          // uniform over the workgroup
        if (tid == 0) {
            count[prob] = 0;
            thr_out[prob] = 0.0;
            mass_out[prob] = 0.0;
        }
        return;
    }
    double gmax = 0.0, sum = 0.0;
    for (int i = tid; i < hw; i += NT) {
        const double av = P.a[i], bv = P.b[i];
        gmax = fmax(gmax, fabs(av - bv));
        sum += av;
    }
    gmax = wave_max(gmax);
    sum = wave_add(sum);
    if (lane == 0) {
        w_max[wid] = gmax;
        w_sum[wid] = sum;
    }
    __syncthreads();
    gmax = fmax(fmax(w_max[0], w_max[1]), fmax(w_max[2], w_max[3]));
    const double thr = 1e-3 * gmax;
    int n = 0;
    for (int i = tid; i < hw; i += NT) n += fabs(P.a[i] - P.b[i]) > thr;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) w_cnt[wid] = n;
    __syncthreads();
    if (tid == 0) {
        count[prob] = (int64_t)w_cnt[0] + w_cnt[1] + w_cnt[2] + w_cnt[3];
        thr_out[prob] = thr;
        mass_out[prob] = ((w_sum[0] + w_sum[1]) + w_sum[2]) + w_sum[3];
    }
}

__global__ void __launch_bounds__(NT)
k_problem_fill(const double *__restrict__ inaction, const double *__restrict__ action,
               const int32_t *__restrict__ n_keys, int max_keys, int hw, int W,
               const int64_t *__restrict__ offsets, const double *__restrict__ thr_in,
               double *__restrict__ p, double *__restrict__ q, int32_t *__restrict__ ys,
               int32_t *__restrict__ xs, int64_t cap) {
    __shared__ int w_tot[NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t prob = blockIdx.x;
    const int64_t base = offsets[prob];
    if (offsets[prob + 1] == base) return;               // no cell: uniform exit
    const Problem P = problem_maps(inaction, action, n_keys, max_keys, hw);
    if (!P.a) return;
    const double thr = thr_in[prob];
    int64_t running = base;                              // cells of the chunks before
    for (int c0 = 0; c0 < hw; c0 += NT) {
        const int i = c0 + tid;
        double av = 0.0, bv = 0.0;
        bool sel = false;
        if (i < hw) {
            av = P.a[i];
            bv = P.b[i];
            sel = fabs(av - bv) > thr;
        }
        // stable rank: lanes below in the wave, waves below in the workgroup
        const unsigned long long m = __ballot(sel);
        const int below = (int)__builtin_amdgcn_mbcnt_hi(
            (unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) w_tot[wid] = __popcll(m);
        __syncthreads();
        int pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; w++) {
            const int t = w_tot[w];
            pre += w < wid ? t : 0;
            tot += t;
        }
        __syncthreads();
        const int64_t at = running + pre + below;
        if (sel && at >= 0 && at < cap) {
            const int y = i / W;
            p[at] = av;
            q[at] = bv;
            ys[at] = y;
            xs[at] = i - y * W;
        }
        running += tot;
    }
}

// the checks both entry points share; *nprob = E * max_keys
int check_shape(int64_t E, int max_keys, int H, int W, int64_t *nprob) {
    if (E < 0 || H < 2 || W < 2 || max_keys < 1 || max_keys > 1024) return SL_EINVAL;
    if ((int64_t)H * W > kMaxCells) return SL_EINVAL;
    if (E > (int64_t)0x7FFFFFFE / max_keys) return SL_EINVAL;   // one workgroup per slot
    *nprob = E * max_keys;
    return SL_OK;
}

bool workspace_ok(const void *workspace, int64_t workspace_bytes, int64_t E, int max_keys) {
    int64_t need;
    if (sl_side_effect_problems_workspace(E, max_keys, &need) != SL_OK) return false;
    return workspace && (((uintptr_t)workspace) & 7) == 0 && workspace_bytes >= need;
}

}  // namespace

// workspace: int64 count[E * max_keys + 1], then double thr[E * max_keys]
extern "C" int sl_side_effect_problems_workspace(int64_t E, int max_keys, int64_t *bytes) {
    if (E < 0 || max_keys < 1 || max_keys > 1024 || !bytes) return SL_EINVAL;
    if (E > (int64_t)0x7FFFFFFE / max_keys) return SL_EINVAL;
    *bytes = (2 * E * max_keys + 1) * 8;
    return SL_OK;
}

extern "C" int sl_side_effect_problem_counts(const double *inaction, const double *action,
                                             const int32_t *n_keys, int64_t E, int max_keys,
                                             int H, int W, int64_t *offsets, double *mass,
                                             void *workspace, int64_t workspace_bytes,
                                             void *stream) {
    int64_t nprob;
    if (check_shape(E, max_keys, H, W, &nprob) != SL_OK) return SL_EINVAL;
    if (!inaction || !action || !n_keys || !offsets || !mass ||
        !workspace_ok(workspace, workspace_bytes, E, max_keys))
        return SL_EINVAL;
    if (E == 0) return SL_OK;
    hipStream_t s = (hipStream_t)stream;
    int64_t *count = (int64_t *)workspace;
    double *thr = (double *)(count + nprob + 1);
    hipLaunchKernelGGL(k_problem_count, dim3((unsigned)nprob), dim3(NT), 0, s, inaction, action,
                       n_keys, max_keys, H * W, nprob, count, thr, mass);
    if (hipGetLastError() != hipSuccess) return SL_EHIP;
    return sl_exclusive_scan_i64(count, offsets, nprob + 1, nullptr, nullptr, stream);
}

extern "C" int sl_side_effect_problem_cells(const double *inaction, const double *action,
                                            const int32_t *n_keys, int64_t E, int max_keys,
                                            int H, int W, const int64_t *offsets, double *p,
                                            double *q, int32_t *ys, int32_t *xs, int64_t cap,
                                            void *workspace, int64_t workspace_bytes,
                                            void *stream) {
    int64_t nprob;
    if (check_shape(E, max_keys, H, W, &nprob) != SL_OK || cap < 0) return SL_EINVAL;
    if (!inaction || !action || !n_keys || !offsets || !p || !q || !ys || !xs ||
        !workspace_ok(workspace, workspace_bytes, E, max_keys))
        return SL_EINVAL;
    if (E == 0) return SL_OK;
    const double *thr = (const double *)((const int64_t *)workspace + nprob + 1);
    hipLaunchKernelGGL(k_problem_fill, dim3((unsigned)nprob), dim3(NT), 0, (hipStream_t)stream,
                       inaction, action, n_keys, max_keys, H * W, W, offsets, thr, p, q, ys, xs,
                       cap);
    return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
}
