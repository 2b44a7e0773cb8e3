// sl_bits_geo.h -- the geometry policies of rule_planes (sl_bits.h) for the layouts more
// than one file uses: Geo64 (64x64 boards: sl_bits.hip, sl_rollout_bits.hip), GeoSmall
// (boards up to 32 rows x 64 columns: sl_bits_small.hip, sl_rollout_bits.hip), GeoMid
// (33 to 64 rows, up to 64 columns: sl_bits_mid.hip; here so that the side-effect rollout
// can take it), GeoBand with its HaloView (128x128 boards in bands of 32 rows:
// sl_bits128.hip, sl_rollout_bits128.hip) and GeoWide (bands of 32 rows of any board of up
// to 128 x 128: sl_bits_wide.hip).
#pragma once
#include "sl_bits.h"

namespace sl {
namespace bits {

// Neighbourhood of the 64x64 layout: lane l holds columns 2j, 2j+1 (j = l >> 1) over
// rows 32h .. 32h+31 (h = l & 1).  Column 2j - 1 is word 1 of lane l - 2 and column
// 2j + 2 word 0 of lane l + 2 (the 64-lane rotation wraps at W = 64); the rows
// around a word come from the other half's word (lane l ^ 1), which also supplies
// the wrap at H = 64.
template <int MODE>
struct Geo64 {
    static constexpr int N = 64;        // rows = columns = lanes
    int lane;
    StreamSrc src;     // SPAWN_STREAM: the supplied uniforms; pos = this tensor's first
    int64_t pos;
    int count;         // SPAWN_COUNT: this lane's eligible cells
    template <class F>
    __device__ __forceinline__ V3 vert(const u32 *P, int w, F f) const {
        const u32 x = f(P, w);
        return vert_with(x, lane_x1(x));
    }
    __device__ __forceinline__ H3 horiz(u32 w0, u32 w1) const {
        return H3{lane_m1(lane_m1(w1)), lane_p1(lane_p1(w0))};
    }
    __device__ __forceinline__ bool halo_spawn() const { return false; }
    // the 2x2 spawn block of rows 32h + y, y + 1 (y even) of the lane's column pair
    __device__ __forceinline__ u32 block(int y) const {
        return (u32)(((32 * (lane & 1) + y) >> 1) * (N / 2) + (lane >> 1));
    }
    // spawners are rare on these boards: per-lane Philox draws, no LDS list
    __device__ __forceinline__ void spawn(const u32 elig[2], u32 sp[2], const SpawnCtx &sc,
                                          u32 tensor) {
        if (MODE == SPAWN_PHILOX) {
            philox_spawn(*this, elig, sp, sc, tensor);
        } else if (MODE == SPAWN_STREAM) {
            (void)stream_draws<true>(elig, sp, sc.thr, src, pos, lane);
        } else {
            count += __builtin_popcount(elig[0]) + __builtin_popcount(elig[1]);
        }
    }
};

// Boards up to 32 rows x 64 columns: lane j < nl = ceil(W / 2) holds the column pair
// (2j, 2j+1) over all rows.  Vertical neighbours are rotations within the low H bits,
// horizontal ones come through ds_bpermute, which wraps at W for any W; for odd W the
// last lane's second word is a copy of column 0.
template <int MODE>
struct GeoSmall {
    int lane, H, W, nl;
    u32 mh;                  // the low H bits
    int src_l, src_r;        // lanes holding columns 2j - 1 and 2j + 2
    bool odd_last;           // this lane's word 1 is the column-0 copy (odd W)
    StreamSrc src;           // SPAWN_STREAM: the supplied uniforms from this tensor's first
    int64_t pos;
    int count;               // SPAWN_COUNT: this lane's eligible cells
    template <class F>
    __device__ __forceinline__ V3 vert(const u32 *P, int w, F f) const {
        const u32 x = f(P, w);
        return V3{((x << 1) | (x >> (H - 1))) & mh, ((x >> 1) | ((x & 1u) << (H - 1))) & mh};
    }
    __device__ __forceinline__ H3 horiz(u32 w0, u32 w1) const {
        const u32 right_col = odd_last ? w0 : w1;          // this lane's last real column
        return H3{(u32)__builtin_amdgcn_ds_bpermute(4 * src_l, (int)right_col),
                  (u32)__builtin_amdgcn_ds_bpermute(4 * src_r, (int)w0)};
    }
    __device__ __forceinline__ bool halo_spawn() const { return false; }
    // the 2x2 spawn block of rows y, y + 1 (y even) of the lane's column pair
    __device__ __forceinline__ u32 block(int y) const { return (u32)((y >> 1) * nl + lane); }
    // (the column-0 copy's draws are discarded with the rest of that word; in replay
    // mode it draws nothing, so it cannot shift the real cells' ranks)
    __device__ __forceinline__ void spawn(const u32 elig[2], u32 sp[2], const SpawnCtx &sc,
                                          u32 tensor) {
        const u32 e[2] = {elig[0], odd_last ? 0u : elig[1]};
        if (MODE == SPAWN_PHILOX) {
            philox_spawn(*this, elig, sp, sc, tensor);
        } else if (MODE == SPAWN_STREAM) {
            (void)stream_draws<false>(e, sp, sc.thr, src, pos, lane);
        } else {
            count += __builtin_popcount(e[0]) + __builtin_popcount(e[1]);
        }
    }
};

// the geometry of lane `lane` on an H x W board (lanes >= ceil(W / 2) hold nothing)
template <int MODE>
__device__ __forceinline__ GeoSmall<MODE> small_geo(int lane, int H, int W) {
    GeoSmall<MODE> g;
    const int nl = (W + 1) >> 1;
    const bool active = lane < nl;
    g.lane = lane;
    g.H = H;
    g.W = W;
    g.nl = nl;
    g.mh = H == 32 ? ~0u : ((1u << H) - 1u);
    g.src_l = active ? (lane == 0 ? nl - 1 : lane - 1) : lane;
    g.src_r = active ? (lane + 1 == nl ? 0 : lane + 1) : lane;
    g.odd_last = (W & 1) && lane == nl - 1;
    g.src = StreamSrc{nullptr, 0, nullptr};
    g.pos = 0;
    g.count = 0;
    return g;
}

// Boards of 33 to 64 rows and up to 64 columns: Geo64's split of the rows over lane
// parity with GeoSmall's columns.  Lane l = 2j + h holds the column pair (2j, 2j+1),
// j < nl = ceil(W / 2), over rows 32h .. 32h+31: the lower half's 32 rows are all
// real, the upper half's are its low H - 32 bits (mh), and the bits above them hold
// no cell: every neighbour word is masked, so they stay clear through the rule.  The
// rows around a word come from the other half's word (lane l ^ 1) with the torus wrap
// at H: above row 0 is row H - 1 (the partner's bit H - 33), below row 31 is row 32
// (its bit 0), above row 32 is row 31 (its bit 31), and below row H - 1 is row 0 (its
// bit 0, entering at this word's bit H - 33).  At H = 64 this is Geo64's vert_with.
// Columns come through ds_bpermute from lanes l -+ 2, wrapping at 2 nl; for odd W the
// last pair's word 1 is a copy of column 0 (GeoSmall).
template <int MODE>
struct GeoMid {
    int lane, H, W, nl;
    u32 mh;                  // this word's real rows
    int su;                  // the partner's bit that is the row above this word's row 0
    int sd;                  // this word's last real row: the partner's bit 0 lies below it
    int src_l, src_r;        // lanes holding columns 2j - 1 and 2j + 2 of this half
    bool odd_last;           // this lane's word 1 is the column-0 copy (odd W)
    StreamSrc src;           // SPAWN_STREAM: the supplied uniforms from this tensor's first
    int64_t pos;
    int count;               // SPAWN_COUNT: this lane's eligible cells
    template <class F>
    __device__ __forceinline__ V3 vert(const u32 *P, int w, F f) const {
        const u32 x = f(P, w);
        const u32 o = lane_x1(x);
        return V3{((x << 1) | ((o >> su) & 1u)) & mh, ((x >> 1) | ((o & 1u) << sd)) & mh};
    }
    __device__ __forceinline__ H3 horiz(u32 w0, u32 w1) const {
        const u32 right_col = odd_last ? w0 : w1;          // this lane's last real column
        return H3{(u32)__builtin_amdgcn_ds_bpermute(4 * src_l, (int)right_col),
                  (u32)__builtin_amdgcn_ds_bpermute(4 * src_r, (int)w0)};
    }
    __device__ __forceinline__ bool halo_spawn() const { return false; }
    // the 2x2 spawn block of rows 32h + y, y + 1 (y even) of the lane's column pair
    __device__ __forceinline__ u32 block(int y) const {
        return (u32)(((32 * (lane & 1) + y) >> 1) * nl + (lane >> 1));
    }
    // only real cells draw: no row past H - 1, nothing in the column-0 copy (in replay
    // mode it would shift the real cells' ranks); lanes past the board hold zeros
    __device__ __forceinline__ void spawn(const u32 elig[2], u32 sp[2], const SpawnCtx &sc,
                                          u32 tensor) {
        const u32 e[2] = {elig[0] & mh, odd_last ? 0u : elig[1] & mh};
        if (MODE == SPAWN_PHILOX) {
            philox_spawn(*this, e, sp, sc, tensor);
        } else if (MODE == SPAWN_STREAM) {
            (void)stream_draws<true>(e, sp, sc.thr, src, pos, lane);
        } else {
            count += __builtin_popcount(e[0]) + __builtin_popcount(e[1]);
        }
    }
};

// the geometry of lane `lane` on an H x W board, 33 <= H <= 64 (lanes >= 2 ceil(W / 2)
// hold nothing)
template <int MODE>
__device__ __forceinline__ GeoMid<MODE> mid_geo(int lane, int H, int W) {
    GeoMid<MODE> g;
    const int nl = (W + 1) >> 1, h = lane & 1, j = lane >> 1;
    const bool active = j < nl;
    g.lane = lane;
    g.H = H;
    g.W = W;
    g.nl = nl;
    g.mh = (h && H < 64) ? ((1u << (H - 32)) - 1u) : ~0u;
    g.su = h ? 31 : H - 33;
    g.sd = h ? H - 33 : 31;
    g.src_l = active ? (j == 0 ? 2 * (nl - 1) + h : lane - 2) : lane;
    g.src_r = active ? (j + 1 == nl ? h : lane + 2) : lane;
    g.odd_last = (W & 1) && j == nl - 1;
    g.src = StreamSrc{nullptr, 0, nullptr};
    g.pos = 0;
    g.count = 0;
    return g;
}

// The rows just outside a band as "planes": element p is a word with bit 31 = bit p
// of the row above's cell pair and bit 0 = bit p of the row below's, computed where
// the rule uses it (two registers live instead of the full 32-word array).
struct HaloView {
    u32 up, dn;
    __device__ __forceinline__ u32 operator[](int p) const {
        return ((up >> p) << 31) | ((dn >> p) & 1u);
    }
};

// Neighbourhood of a band word of a 128x128 board (one wave64 per band of 32 rows, lane
// j owns the column pair 2j, 2j + 1): columns from the neighbouring lanes (2j - 1 is word
// 1 of lane j - 1, 2j + 2 word 0 of lane j + 1), rows outside the band from the halo
// (plane k, word w: bit 31 = row 32t - 1, bit 0 = row 32t + 32).
template <int MODE>
struct GeoBand {
    static constexpr int N = 128;       // rows = columns
    int lane, row0;
    HaloView hv;
    StreamSrc src;     // SPAWN_STREAM: the supplied uniforms; pos = the band's first,
    int64_t pos;       // used = how many the band consumed
    int used;
    int count;         // SPAWN_COUNT: this lane's eligible cells
    lds_u16 *slots;    // SPAWN_PHILOX: compact_draws' queue (kDrawSlots)
    u32 e[2];          // SPAWN_COUNT: the band's eligible cells; SPAWN_DECIDED: the
                       // cells k_stream_draw128 decided spawn
    template <class F>
    __device__ __forceinline__ V3 vert(const u32 *P, int w, F f) const {
        return vert_with(f(P, w), f(hv, w));
    }
    __device__ __forceinline__ H3 horiz(u32 w0, u32 w1) const {
        return H3{lane_m1(w1), lane_p1(w0)};
    }
    __device__ __forceinline__ bool halo_spawn() const {
        return (PL(hv, 7, 0) | PL(hv, 7, 1)) != 0u;
    }
    // the 2x2 spawn block of band rows y, y + 1 (y even) of the lane's column pair
    __device__ __forceinline__ u32 block(int y) const {
        return block_of(lane, y);
    }
    __device__ __forceinline__ u32 block_of(int l, int y) const {
        return (u32)(((row0 + y) >> 1) * (N / 2) + l);
    }
    __device__ __forceinline__ void spawn(const u32 elig[2], u32 sp[2], const SpawnCtx &sc,
                                          u32 tensor) {
        if (MODE == SPAWN_PHILOX) {
            philox_spawn_compact(*this, elig, sp, sc, tensor, slots);
        } else if (MODE == SPAWN_STREAM) {
            used = stream_draws<false>(elig, sp, sc.thr, src, pos, lane);
        } else if (MODE == SPAWN_DECIDED) {
            sp[0] = elig[0] & e[0];
            sp[1] = elig[1] & e[1];
        } else {
            count += __builtin_popcount(elig[0]) + __builtin_popcount(elig[1]);
            e[0] = elig[0];
            e[1] = elig[1];
        }
    }
};

// Boards of up to 128 x 128 that no other layout takes (more than 64 rows or more than 64
// columns, 128x128 aside: sl_bits_wide.hip): GeoBand's bands of 32 rows with GeoSmall's
// columns.  Lane j < nl = ceil(W / 2) holds the column pair (2j, 2j+1) of the band's rows;
// columns come through ds_bpermute from lanes j -+ 1 modulo nl, and for odd W the last
// pair's word 1 is a copy of column 0 (at nl = 64 the permute is GeoBand's whole-wave
// rotation).  The rows just outside the band come from the halo, wrapping at H: the last
// band holds n = H - 32 (NB - 1) real rows (mh), its other bits hold no cell and every
// neighbour word is masked, and its lower halo -- row 0 -- enters below row n - 1 (sd), not
// below bit 31.  Philox draws only (replay is open: DESIGN.md 10).
template <int MODE>
struct GeoWide {
    static_assert(MODE == SPAWN_PHILOX, "GeoWide draws with Philox only");
    int lane, nl, row0;      // row0: the band's first row
    u32 mh;                  // the band's real rows
    int sd;                  // the band's last real row: the lower halo lies below it
    int src_l, src_r;        // lanes holding columns 2j - 1 and 2j + 2
    bool odd_last;           // this lane's word 1 is the column-0 copy (odd W)
    HaloView hv;
    template <class F>
    __device__ __forceinline__ V3 vert(const u32 *P, int w, F f) const {
        const u32 x = f(P, w), o = f(hv, w);
        return V3{__builtin_amdgcn_alignbit(x, o, 31u) & mh, ((x >> 1) | ((o & 1u) << sd)) & mh};
    }
    __device__ __forceinline__ H3 horiz(u32 w0, u32 w1) const {
        const u32 right_col = odd_last ? w0 : w1;          // this lane's last real column
        return H3{(u32)__builtin_amdgcn_ds_bpermute(4 * src_l, (int)right_col),
                  (u32)__builtin_amdgcn_ds_bpermute(4 * src_r, (int)w0)};
    }
    __device__ __forceinline__ bool halo_spawn() const {
        return (PL(hv, 7, 0) | PL(hv, 7, 1)) != 0u;
    }
    // the 2x2 spawn block of band rows y, y + 1 (y even) of the lane's column pair
    __device__ __forceinline__ u32 block(int y) const {
        return (u32)(((row0 + y) >> 1) * nl + lane);
    }
    // only real cells draw: no row past H - 1, nothing in the column-0 copy; lanes past
    // the board hold zeros
    __device__ __forceinline__ void spawn(const u32 elig[2], u32 sp[2], const SpawnCtx &sc,
                                          u32 tensor) {
        const u32 e[2] = {elig[0] & mh, odd_last ? 0u : elig[1] & mh};
        philox_spawn(*this, e, sp, sc, tensor);
    }
};

// row r of a tensor in HBM as the lane's dword in GeoWide's columns (a0, a1: the lane's
// columns): one dword where W is even and the tensor's address a multiple of 4, else two
// uint16 (sl_bits_wide.hip, sl_rollout_bits_wide.hip)
__device__ __forceinline__ u32 hbm_row(const uint16_t *__restrict__ t, int W, int r, int a0,
                                       int a1) {
    if (!(W & 1) && !((uintptr_t)t & 3)) return reinterpret_cast<const u32 *>(t + r * W + a0)[0];
    return (u32)t[r * W + a0] | ((u32)t[r * W + a1] << 16);
}

// the geometry of lane `lane` in the band of rows row0 .. row0 + 31 of an H x W board
// (lanes >= ceil(W / 2) hold nothing); the caller sets the halo
template <int MODE>
__device__ __forceinline__ GeoWide<MODE> wide_geo(int lane, int H, int W, int row0) {
    GeoWide<MODE> g;
    const int nl = (W + 1) >> 1, n = min(32, H - row0);
    const bool active = lane < nl;
    g.lane = lane;
    g.nl = nl;
    g.row0 = row0;
    g.mh = n == 32 ? ~0u : ((1u << n) - 1u);
    g.sd = n - 1;
    g.src_l = active ? (lane == 0 ? nl - 1 : lane - 1) : lane;
    g.src_r = active ? (lane + 1 == nl ? 0 : lane + 1) : lane;
    g.odd_last = (W & 1) && lane == nl - 1;
    g.hv = HaloView{0u, 0u};
    return g;
}

}  // namespace bits
}  // namespace sl
