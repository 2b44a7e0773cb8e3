// sl_rollout_bits.h -- launcher of the bit-sliced side-effect rollout kernels
// (sl_rollout_bits.hip, sl_rollout_bits_mid.hip, sl_rollout_bits128.hip,
// sl_rollout_bits_wide.hip), called by sl_side_effect_densities_k (sl_board.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sl {

struct RolloutArgs {
    const uint16_t *init_board, *final_board;   // dev [E, H, W]
    const int32_t *steps;                       // dev [E]
    const float *spawn_prob;                    // dev [E]
    const uint32_t *env_ids;                    // dev [E] or NULL: env0 + e
    uint32_t env0;
    uint64_t seed;
    int32_t S, H, W;                            // S = num_samples
    uint32_t *bitmap;                           // dev [2E][2048]: pass 0 writes every word
    const uint16_t *keys;                       // pass 1: dev [E, max_keys] ascending
    const int32_t *n_keys;                      // pass 1: dev [E]
    int32_t max_keys;
    double *inaction, *action;                  // pass 1: dev [E, max_keys, H, W] counts
};

// a bit-sliced rollout exists for this shape (Philox draws only)
bool rollout_bits_shape(int H, int W);

// pass 0: mark every sampled key; pass 1: count every sampled cell into its key's map.
// One launch of 2E single-wave workgroups each.
int launch_rollout_bits(const RolloutArgs &a, int64_t E, int pass, hipStream_t s);

// the four-wave band rollout (sl_rollout_bits128.hip) exists for this shape: 128x128,
// Philox draws only
bool rollout_bands_shape(int H, int W);

// the same two passes, one launch of 2E four-wave workgroups each; the boards are read
// as dwords (4-byte aligned)
int launch_rollout_bands(const RolloutArgs &a, int64_t E, int pass, hipStream_t s);

// the one-wave rollout of boards of 33 to 64 rows (sl_rollout_bits_mid.hip) exists for
// this shape: 33 <= H <= 64, 2 <= W <= 64, not 64x64 (mid_shape's range), Philox draws only
bool rollout_mid_shape(int H, int W);

// the same two passes, one launch of 2E single-wave workgroups each; the boards are read
// as uint16 (no alignment rule)
int launch_rollout_mid(const RolloutArgs &a, int64_t E, int pass, hipStream_t s);

// the band rollout of boards past 64 rows or columns (sl_rollout_bits_wide.hip) exists for
// this shape: wide_shape (sl_bits_wide.hip; declared in sl_env_common.h too) -- 2 <= H, W
// <= 128, H > 64 or W > 64, not 128x128 -- Philox draws only
bool wide_shape(int H, int W);
bool rollout_wide_shape(int H, int W);

// the same two passes, one launch of 2E workgroups of ceil(H / 32) waves each; the boards
// are read as dwords where W is even and the address a multiple of 4, else as uint16 (no
// alignment rule)
int launch_rollout_wide(const RolloutArgs &a, int64_t E, int pass, hipStream_t s);

}  // namespace sl
