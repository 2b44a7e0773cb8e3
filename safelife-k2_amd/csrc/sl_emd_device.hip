// sl_emd_device.hip -- the earth mover's distances of side_effect_score solved on the
// device (gfx950): sl_emd_cells (sl_emd.cpp) restated for one wave per problem.
//
// The inputs are what k_problem_fill (sl_side_effect_problems.hip) leaves in device
// memory: per problem a run of cells (p, q, ys, xs) delimited by `offsets`.  Every
// floating-point step around the transport is the host's, in the host's order: the two
// sums in index order, the pre-flow, 1e6 / maxSum and 1e6 / maxC, floor(x * norm + 0.5),
// (double)c / PQnorm / Cnorm, + (maxSum - minSum) * penalty.  The file is built with
// -ffp-contract=off (Makefile FLAGS), so no product is fused into a sum.  The transport
// itself is an integer problem with one optimum, whatever exact method finds it, so the
// result is the host's bit for bit.
//
// k_emd_cells: one workgroup of one wave per problem.
//   setup      coordinates checked against the board before any table read
//              (SL_EMD_ST_BADCELL); p, q staged in LDS; every lane forms sumP / sumQ by
//              the same serial additions; maxC = max of table[offset(i, j)] over all
//              ordered pairs of cells; integer masses; the heavier side supplies and
//              its excess goes to a threshold column at cost 0; supplies and demands
//              are compacted in cell order (ballot ranks).
//   simplex    the host's perturbation (K = n + 1, +1 per supply, +n on the last
//              demand) and north-west-corner tree, kept as parent pointers: per node
//              its parent, depth, potential, and the flow and cost of the edge to its
//              parent.  A pivot prices all n * m reduced costs across the lanes (full
//              Dantzig pricing, wave argmin, ties to the lowest cell index); lane 0
//              walks both ends of the entering cell up to their common ancestor, takes
//              theta and the leaving edge from the edges that lose flow, moves theta
//              round the cycle and reverses the parent pointers from the entering end
//              to the leaving edge; then all nodes recompute depth and potential from
//              their parents in sweeps until a sweep changes nothing.
//   result     the final tree's flows for the unperturbed masses (levels from the
//              deepest up, each node adding its balance to its parent's), the sum of
//              flow * cost in int64, back to doubles.
//
// Integer cost of a pair: floor(table[.] * Cnorm + 0.5) <= 1e6, computed from the table
// where it is needed, or read from an LDS copy when n * m <= kStage.  Potentials,
// reduced costs and flows are int64 throughout.
//
// Bounds.  Every loop is bounded before it starts: the cell loops by
// SL_EMD_DEVICE_MAX_CELLS, tree walks and sweeps by the node count n + m, the pivot loop
// by kPivotCapMult * (n + m) (SL_EMD_ST_PIVOTS beyond it).  A tree that fails one of the
// checks the host answers with -1 ("cannot happen": an incomplete north-west tree, a walk
// that does not meet, a negative final flow) is reported as SL_EMD_ST_PIVOTS as well, so
// that the host solves that problem and speaks for itself.
//
// LDS per problem: 4 int32 and 3 int64 arrays of kNodes = 264 entries (10 560 B) plus the
// staged costs (4 096 B): 14 656 B, eleven problems per CU.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/safelife_hip.h"

namespace {

constexpr int kMaxCells = SL_EMD_DEVICE_MAX_CELLS;
constexpr int kNodes = 264;                  // >= kMaxCells + 1 (the threshold column)
constexpr int kStage = 1024;                 // staged integer costs (n * m at most)
constexpr int kPivotCapMult = 25;            // pivots allowed per node: 8 x the largest
                                             // seen, 3.11
constexpr int kMaxSide = 32768;              // H, W: a cell packs into 16 + 15 bits

static_assert(kMaxCells % 64 == 0 && kNodes >= kMaxCells + 1, "node arrays too short");

__device__ __forceinline__ void wave_sync() { __syncthreads(); }    // workgroup = one wave

__device__ __forceinline__ int lanes_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                          __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ long long wave_add_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(64)
k_emd_cells(const double *__restrict__ p, const double *__restrict__ q,
            const int32_t *__restrict__ ys, const int32_t *__restrict__ xs,
            const int64_t *__restrict__ offsets, const double *__restrict__ table, int H, int W,
            double penalty, double *__restrict__ out, int32_t *__restrict__ status) {
    __shared__ int s_par[kNodes], s_dep[kNodes], s_eco[kNodes], s_yx[kNodes], s_cst[kStage];
    __shared__ long long s_pot[kNodes], s_flw[kNodes], s_mas[kNodes];
    __shared__ int s_fail;
    const int lane = threadIdx.x;
    const int64_t prob = blockIdx.x;
    const int64_t base = offsets[prob];
    const int64_t cnt = offsets[prob + 1] - base;
    if (cnt == 0 || cnt < 0 || cnt > kMaxCells) {        // uniform over the wave
        if (lane == 0) {
            out[prob] = 0.0;
            status[prob] = cnt == 0 ? 0 : SL_EMD_ST_TOOBIG;
        }
        return;
    }
    const int c = (int)cnt;
    const int tw = 2 * W - 1;
    // ---- cells: coordinates first; no table access before every one is on the board
    int *cyx = s_par;                                    // the cells' packed coordinates
    bool bad = false;
    for (int k = 0; k < kMaxCells; k += 64) {
        const int i = k + lane;
        if (i < c) {
            const int y = ys[base + i], x = xs[base + i];
            const bool off_board = y < 0 || y >= H || x < 0 || x >= W;
            bad |= off_board;
            cyx[i] = off_board ? 0 : (y << 16) | x;
            s_pot[i] = __double_as_longlong(p[base + i]);
            s_flw[i] = __double_as_longlong(q[base + i]);
        }
    }
    if (__any(bad)) {
        if (lane == 0) {
            out[prob] = 0.0;
            status[prob] = SL_EMD_ST_BADCELL;
        }
        return;
    }
    wave_sync();
    // ---- the sums of the histograms as given, in index order (every lane the same)
    double sumP = 0.0, sumQ = 0.0;
    for (int i = 0; i < c; i++) {
        sumP += __longlong_as_double(s_pot[i]);
        sumQ += __longlong_as_double(s_flw[i]);
    }
    // ---- the largest ground distance over all ordered pairs of the cells
    double maxC = 0.0;
    {
        const int qi = 64 / c, rj = 64 % c;
        int i = lane / c, j = lane % c;
        const int pairs = c * c;
        for (int e = lane; e < pairs; e += 64) {
            const int a = cyx[i], b = cyx[j];
            const int64_t o = (int64_t)((a >> 16) - (b >> 16) + H - 1) * tw +
                              ((a & 0xFFFF) - (b & 0xFFFF) + W - 1);
            const double t = table[o];
            maxC = maxC < t ? t : maxC;
            i += qi;
            j += rj;
            if (j >= c) {
                j -= c;
                i++;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double t = __shfl_xor(maxC, o, 64);
            maxC = maxC < t ? t : maxC;
        }
    }
    const double minSum = sumQ < sumP ? sumQ : sumP, maxSum = sumP < sumQ ? sumQ : sumP;
    if (penalty == -1.0) penalty = maxC;
    double dist = 0.0;
    int pivots = 0;
    bool failed = false;
    if (maxSum > 0.0 && maxC > 0.0) {
        const double PQnorm = 1000000.0 / maxSum, Cnorm = 1000000.0 / maxC;
        // ---- pre-flow at equal bins, then fixed point (each lane its own cells)
        long long sP = 0, sQ = 0;
        for (int k = 0; k < kMaxCells; k += 64) {
            const int i = k + lane;
            if (i < c) {
                double P = __longlong_as_double(s_pot[i]), Q = __longlong_as_double(s_flw[i]);
                if (P < Q) {
                    Q -= P;
                    P = 0.0;
                } else {
                    P -= Q;
                    Q = 0.0;
                }
                const long long iP = (long long)floor(P * PQnorm + 0.5);
                const long long iQ = (long long)floor(Q * PQnorm + 0.5);
                s_pot[i] = iP;
                s_flw[i] = iQ;
                sP += iP;
                sQ += iQ;
            }
        }
        sP = wave_add_i64(sP);
        sQ = wave_add_i64(sQ);
        // ---- the heavier side supplies (C as given, supply bin first)
        const bool swap = sQ > sP;
        const long long excess = sP > sQ ? sP - sQ : sQ - sP;
        wave_sync();
        int n = 0, m = 0;
        for (int k = 0; k < kMaxCells; k += 64) {
            const int i = k + lane;
            const long long S = i < c ? (swap ? s_flw[i] : s_pot[i]) : 0;
            const long long D = i < c ? (swap ? s_pot[i] : s_flw[i]) : 0;
            n += __popcll(__ballot(S > 0));
            m += __popcll(__ballot(D > 0));
        }
        int nS = 0, nD = 0;
        for (int k = 0; k < kMaxCells; k += 64) {
            const int i = k + lane;
            const long long S = i < c ? (swap ? s_flw[i] : s_pot[i]) : 0;
            const long long D = i < c ? (swap ? s_pot[i] : s_flw[i]) : 0;
            const bool isS = S > 0, isD = D > 0;
            const unsigned long long bS = __ballot(isS), bD = __ballot(isD);
            if (isS) {
                const int r = nS + lanes_below(bS);
                s_mas[r] = S;
                s_yx[r] = cyx[i];
            }
            if (isD) {
                const int r = n + nD + lanes_below(bD);
                s_mas[r] = D;
                s_yx[r] = cyx[i];
            }
            nS += __popcll(bS);
            nD += __popcll(bD);
        }
        if (excess > 0) {                                // the threshold node
            if (lane == 0) {
                s_mas[n + m] = excess;
                s_yx[n + m] = -1;
            }
            m++;
        }
        wave_sync();                                     // cyx (s_par) is free from here
        if (n > 0 && m > 0) {
            const int N = n + m;
            bool staged = false;
            // the fixed-point cost of a supply bin against a demand bin (packed cells)
            auto cost_cells = [&](int yi, int yj) -> int {
                if (yj < 0) return 0;                    // the threshold column
                const int64_t o = (int64_t)((yi >> 16) - (yj >> 16) + H - 1) * tw +
                                  ((yi & 0xFFFF) - (yj & 0xFFFF) + W - 1);
                return (int)(long long)floor(table[o] * Cnorm + 0.5);
            };
            auto cost = [&](int i, int j) -> int {
                return staged ? s_cst[i * m + j] : cost_cells(s_yx[i], s_yx[n + j]);
            };
            const int cells = n * m;
            const int qi = 64 / m, rj = 64 % m;          // a lane's step through the cells
            if (cells <= kStage) {
                int i = lane / m, j = lane % m;
                for (int e = lane; e < cells; e += 64) {
                    s_cst[e] = cost_cells(s_yx[i], s_yx[n + j]);
                    i += qi;
                    j += rj;
                    if (j >= m) {
                        j -= m;
                        i++;
                    }
                }
                staged = true;
            }
            if (lane == 0) s_fail = 0;
            wave_sync();
            // ---- north-west corner on the perturbed masses: a tree rooted at row 0
            if (lane == 0) {
                const long long K = n + 1;
                int i = 0, j = 0, made = 0;
                long long rs = K * s_mas[0] + 1;
                long long rd = K * s_mas[n] + (m == 1 ? n : 0);
                bool col_is_new = true;                  // which end of the cell joins
                s_par[0] = -1;
                s_dep[0] = 0;
                s_pot[0] = 0;
                s_flw[0] = 0;
                s_eco[0] = 0;
                for (int step = 0; step < N - 1 && i < n && j < m; step++) {
                    const long long f = rs < rd ? rs : rd;
                    const int v = col_is_new ? n + j : i, u = col_is_new ? i : n + j;
                    const int cc = cost(i, j);
                    s_par[v] = u;
                    s_dep[v] = s_dep[u] + 1;
                    s_eco[v] = cc;
                    s_pot[v] = cc - s_pot[u];
                    s_flw[v] = f;
                    made++;
                    rs -= f;
                    rd -= f;
                    if (rs == 0 && i < n - 1) {
                        i++;
                        rs = K * s_mas[i] + 1;
                        col_is_new = false;
                    } else {
                        j++;
                        if (j < m) rd = K * s_mas[n + j] + (j == m - 1 ? n : 0);
                        col_is_new = true;
                    }
                }
                if (made != N - 1 || i != n - 1 || j != m) s_fail = 1;
            }
            wave_sync();
            failed = s_fail != 0;
            // ---- pivots
            const int cap = kPivotCapMult * N;
            bool optimal = false;
            for (int piv = 0; piv <= cap && !failed; piv++) {
                // pricing: the most negative reduced cost, ties to the lowest cell
                long long best = 0;
                int be = 0x7FFFFFFF;
                {
                    int i = lane / m, j = lane % m;
                    for (int e = lane; e < cells; e += 64) {
                        const long long rc = (long long)cost(i, j) - s_pot[i] - s_pot[n + j];
                        if (rc < best) {
                            best = rc;
                            be = e;
                        }
                        i += qi;
                        j += rj;
                        if (j >= m) {
                            j -= m;
                            i++;
                        }
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const long long orc = __shfl_xor(best, o, 64);
                    const int oe = __shfl_xor(be, o, 64);
                    if (orc < best || (orc == best && oe < be)) {
                        best = orc;
                        be = oe;
                    }
                }
                if (best >= 0) {
                    optimal = true;
                    pivots = piv;
                    break;
                }
                if (piv == cap) break;
                const int bi = be / m, bj = be - bi * m;
                if (lane == 0) {
                    const int a = bi, b = n + bj;
                    // the cycle: both ends up to their common ancestor; counted from
                    // either end, the 1st, 3rd, ... edges lose flow
                    int ua = a, ub = b, ka = 0, kb = 0, leave = -1;
                    bool on_a = true;
                    long long theta = 0x7FFFFFFFFFFFFFFFLL;
                    for (int s = 0; s < N && ua != ub; s++) {
                        const int da = s_dep[ua], db = s_dep[ub];
                        if (da >= db) {
                            if (!(ka & 1) && s_flw[ua] < theta) {
                                theta = s_flw[ua];
                                leave = ua;
                                on_a = true;
                            }
                            ka++;
                        }
                        if (db >= da) {
                            if (!(kb & 1) && s_flw[ub] < theta) {
                                theta = s_flw[ub];
                                leave = ub;
                                on_a = false;
                            }
                            kb++;
                        }
                        if (da >= db) ua = s_par[ua];
                        if (db >= da) ub = s_par[ub];
                        if (ua < 0 || ub < 0) break;
                    }
                    if (ua != ub || ua < 0 || leave < 0) {
                        s_fail = 1;
                    } else {
                        const int top = ua;
                        int v = a;
                        for (int s = 0; s < N && v != top && v >= 0; s++) {
                            s_flw[v] += (s & 1) ? theta : -theta;
                            v = s_par[v];
                        }
                        v = b;
                        for (int s = 0; s < N && v != top && v >= 0; s++) {
                            s_flw[v] += (s & 1) ? theta : -theta;
                            v = s_par[v];
                        }
                        // the entering edge takes the leaving edge's place: the parent
                        // pointers from the entering end down to the leaving edge turn
                        // round, each edge's flow and cost moving to its other end
                        int prev = on_a ? b : a, pc = cost(bi, bj);
                        long long pf = theta;
                        v = on_a ? a : b;
                        for (int s = 0; s < N; s++) {
                            const int nxt = s_par[v], vc = s_eco[v];
                            const long long vf = s_flw[v];
                            s_par[v] = prev;
                            s_flw[v] = pf;
                            s_eco[v] = pc;
                            if (v == leave || nxt < 0) break;
                            prev = v;
                            pf = vf;
                            pc = vc;
                            v = nxt;
                        }
                    }
                }
                wave_sync();
                failed = s_fail != 0;
                // depth and potential of the re-hung nodes: every node from its parent,
                // until a sweep changes nothing (the root stays 0 / 0)
                for (int sweep = 0; sweep < N && !failed; sweep++) {
                    bool changed = false;
                    for (int k = 0; k < kNodes; k += 64) {
                        const int v = k + lane;
                        if (v > 0 && v < N) {
                            const int u = s_par[v];
                            const int nd = s_dep[u] + 1;
                            const long long np = (long long)s_eco[v] - s_pot[u];
                            if (nd != s_dep[v] || np != s_pot[v]) {
                                s_dep[v] = nd;
                                s_pot[v] = np;
                                changed = true;
                            }
                        }
                    }
                    wave_sync();
                    if (!__any(changed)) break;
                }
            }
            if (!optimal) failed = true;
            if (!failed) {
                // ---- the optimal tree's flows for the unperturbed masses
                int maxd = 0;
                for (int k = 0; k < kNodes; k += 64) {
                    const int v = k + lane;
                    if (v < N) {
                        s_pot[v] = v < n ? s_mas[v] : -s_mas[v];         // the balances
                        maxd = s_dep[v] > maxd ? s_dep[v] : maxd;
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const int t = __shfl_xor(maxd, o, 64);
                    maxd = t > maxd ? t : maxd;
                }
                maxd = maxd < N ? maxd : N - 1;
                wave_sync();
                for (int d = maxd; d > 0; d--) {         // children before parents
                    for (int k = 0; k < kNodes; k += 64) {
                        const int v = k + lane;
                        if (v > 0 && v < N && s_dep[v] == d) {
                            const long long bal = s_pot[v];
                            s_flw[v] = v < n ? bal : -bal;
                            atomicAdd((unsigned long long *)&s_pot[s_par[v]],
                                      (unsigned long long)bal);
                        }
                    }
                    wave_sync();
                }
                long long total = 0;
                bool negative = false;
                for (int k = 0; k < kNodes; k += 64) {
                    const int v = k + lane;
                    if (v > 0 && v < N) {
                        negative |= s_flw[v] < 0;
                        total += s_flw[v] * s_eco[v];
                    }
                }
                total = wave_add_i64(total);
                if (__any(negative)) {
                    failed = true;
                } else {
                    dist = (double)total;
                    dist = dist / PQnorm;
                    dist = dist / Cnorm;
                }
            }
        }
    }
    dist += (maxSum - minSum) * penalty;
    if (lane == 0) {
        out[prob] = failed ? 0.0 : dist;
        status[prob] = failed ? SL_EMD_ST_PIVOTS : pivots;
    }
}

}  // namespace

extern "C" int sl_emd_cells_device(const double *p, const double *q, const int32_t *ys,
                                   const int32_t *xs, const int64_t *offsets, int64_t nprob,
                                   const double *cost_table, int H, int W,
                                   double extra_mass_penalty, double *out, int32_t *status,
                                   void *stream) {
    if (nprob < 0 || H < 1 || W < 1 || H > kMaxSide || W > kMaxSide) return SL_EINVAL;
    if (nprob == 0) return SL_OK;
    if (!p || !q || !ys || !xs || !offsets || !cost_table || !out || !status) return SL_EINVAL;
    if (nprob > (int64_t)0x7FFFFFFF) return SL_EINVAL;   // one workgroup per problem
    hipLaunchKernelGGL(k_emd_cells, dim3((unsigned)nprob), dim3(64), 0, (hipStream_t)stream, p,
                       q, ys, xs, offsets, cost_table, H, W, extra_mass_penalty, out, status);
    return hipGetLastError() == hipSuccess ? SL_OK : SL_EHIP;
}
