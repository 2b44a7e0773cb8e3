/*
 * safelife_hip.h -- C ABI of the MI355X (gfx950) SafeLife stepper.
 *
 * Plain pointers and sizes only; every pointer argument marked "dev" is device
 * memory on the current HIP device, every call is stream-ordered on `stream`
 * (a hipStream_t passed as void*, NULL = default stream) and returns 0 or a
 * negative SL_E* code.  No global state: two streams may run independent
 * batches concurrently.  Layouts are row-major uint16 [B, H, W] boards
 * (bit layout of safelife_game.py:74-120 / speedups_src/constants.h:4-25).
 *
 * Reference interfaces each entry point replaces:
 *   sl_advance          speedups.advance_board(board, spawn_prob=0.3)
 *                       /root/reference/safelife/speedups_src/module.c:19-44
 *                       (batched over B boards; the reference does one per call)
 *   sl_count_eligible   the draw count of one advance_board call
 *                       (random_float() calls, advance_board.c:110) -- used to
 *                       place each board's draws in the reference stream
 *                       (speedups.seed / random.c:28-52)
 *   sl_env_step         SafeLifeEnv.step (safelife_env.py:157-186) under the
 *                       PPO chain MovementBonusWrapper -> SimpleSideEffectPenalty
 *                       -> ContinuingEnv (training/safelife_ppo.py:128-139,
 *                       env_wrappers.py:67-88,319-346,298-303) for B envs at once,
 *                       as driven by PPO.run_agents (training/ppo.py:436-452)
 *   sl_env_reset        SafeLifeEnv.reset (safelife_env.py:188-198) + the
 *                       wrappers' resets (env_wrappers.py:90-94,313-317) for the
 *                       envs selected by a mask, from a device level pool
 *                       (the level_iterator / safelife_loader contract,
 *                       file_finder.py:143-201)
 *   sl_env_obs          SafeLifeEnv.get_obs (safelife_env.py:125-155) +
 *                       recenter_view (helper_utils.py:41-74)
 *   sl_side_effect_densities  side_effect_score's rollout + density maps
 *                       (side_effects.py:59-92,131-139), batched over episodes
 *   sl_side_effect_problem_counts / _cells  earth_mover_distance's changed-cell
 *                       selection (side_effects.py:36-43) on those maps, on the device
 *   sl_level_pool_prepare  derived pool data for the device level pool
 *                       (levels as loaded by safelife_game.py:184-212)
 *   sl_sample_actions   np.random.choice(len(policy), p=policy) per env in
 *                       PPO.run_agents (training/ppo.py:440)
 *   sl_gae              returns + advantages of PPO.gen_training_batch
 *                       (training/ppo.py:487-503)
 */
#ifndef SAFELIFE_HIP_H
#define SAFELIFE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SL_OK 0
#define SL_EINVAL (-1)      /* bad shape or argument */
#define SL_EHIP (-2)        /* HIP runtime / launch error */
#define SL_ETOOBIG (-3)     /* board too large for the selected kernel */

#define SL_RNG_STREAM 0     /* replay a supplied uniform stream (reference order) */
#define SL_RNG_PHILOX 1     /* counter-based Philox4x32-10 (production): the four
                               cells of a 2x2 block share one evaluation,
                               counter (block, env, step, tensor), 32-bit words */

#define SL_KERNEL_AUTO 0     /* bit-sliced kernels for 128x128 and for boards of
                                up to 64 rows x 64 columns (both RNG modes; replay adds an
                                action kernel, a count kernel and a scan per
                                step), the generic
                                kernel for other shapes                      */
#define SL_KERNEL_GENERIC 1  /* LDS-staged per-cell kernel, any shape        */
#define SL_KERNEL_FAST 2     /* require the fast kernel (error if none)      */
#define SL_KERNEL_BANDS 3    /* bit-sliced rollout, one four-wave workgroup per
                                board: Philox draws on 128x128 boards;
                                SL_ETOOBIG elsewhere.  Accepted by
                                sl_side_effect_densities_k only
                                (sl_env_cfg.kernel: SL_EINVAL)                */
#define SL_KERNEL_MID 4      /* bit-sliced rollout, one wave per board, of boards
                                of 33 to 64 rows and 2 to 64 columns, 64x64
                                aside: Philox draws; SL_ETOOBIG elsewhere.
                                Accepted by sl_side_effect_densities_k only
                                (sl_env_cfg.kernel: SL_EINVAL)                */
#define SL_KERNEL_WIDE 5     /* the bit-sliced step kernel, and the bit-sliced
                                side-effect rollout, for boards of up to
                                128 x 128 with more than 64 rows or more than 64
                                columns, 128x128 aside (80x80, 96x96, 40x128):
                                Philox draws; SL_ETOOBIG for every other shape
                                and for SL_RNG_STREAM.  Opt-in: AUTO and FAST
                                never pick it.  Accepted by sl_env_cfg.kernel,
                                sl_env_step_family and
                                sl_side_effect_densities_k                    */

/* the step kernel families of sl_env_step (sl_env_step_family) */
#define SL_FAMILY_GENERIC 0     /* k_env_action + the per-cell kernel, any shape      */
#define SL_FAMILY_SMALL_SEG4 1  /* bit-sliced, H <= 32, W <= 32: four envs per wave   */
#define SL_FAMILY_SMALL 2       /* bit-sliced, H <= 32, 32 < W <= 64                  */
#define SL_FAMILY_MID 3         /* bit-sliced, 33 <= H <= 64, W <= 64, 64x64 aside    */
#define SL_FAMILY_BITS64 4      /* bit-sliced 64x64 kernels                           */
#define SL_FAMILY_BITS128 5     /* bit-sliced 128x128 kernels                         */
#define SL_FAMILY_WIDE 6        /* bit-sliced, H <= 128, W <= 128, H > 64 or W > 64,
                                   128x128 aside: k_env_action + k_env_step_wide; only
                                   under SL_KERNEL_WIDE                               */

/* bits of the replay stream's error flag (scratch word 8B, sl_env_cfg.scratch) */
#define SL_STREAM_ERR_RANGE 1      /* the supplied stream ran out, or the device
                                      generator could not serve a step's draw range
                                      (ring too small, or rewound): re-seed / enlarge */
#define SL_STREAM_ERR_THRESHOLD 2  /* a bit ring (sl_mt19937.bit_ring) served an env
                                      whose spawn threshold is not the ring's */

/* sl_env_cfg.board_mode: a 128x128 step without capture -- with no views, or with
 * packed views of at most 96 rows -- keeps the board in sl_env_state.board_planes
 * (SL_BOARD_AUTO) and writes only a few uint16 rows; a caller that reads the uint16
 * board after (nearly) every step asks for it whole instead (SL_BOARD_UINT16: the step
 * kernel writes every changed row, and no sync is needed before a read) */
#define SL_BOARD_AUTO 0
#define SL_BOARD_UINT16 1

/* sl_env_cfg.planes64_waves, beside 0, 5 and 6: the six-wave 64x64 plane kernel with its
 * epilogue in the wave and the reset list, where the default splits them off */
#define SL_PLANES64_W6_UNSPLIT (-6)

/* sl_env_cfg.obs_fuse bits: views the step kernel is asked to write beyond its defaults.
 * SL_OBS_FUSE_CHAN128: the 128x128 step kernel also writes channel views (SL_OBS_CHANNELS*)
 * from the board planes, so the board stays in planes over such steps.  Taken only for a
 * view of at most 96 rows, 128 columns and SL_FUSE_CHAN128_MAX_CELLS cells (the writer of the
 * reset envs' views stages one env's view in LDS) into a 16-byte aligned obs_out; any other
 * view is the observation kernel's, as with the bit clear.  Every other family ignores it. */
#define SL_OBS_FUSE_CHAN128 1
#define SL_FUSE_CHAN128_MAX_CELLS 4096

#define SL_MAX_EXITS 8      /* exits tracked per env (benchmark levels have 1) */
#define SL_BONUS_PERIOD_MAX 16

#define SL_OBS_NONE 0
#define SL_OBS_PACKED 1     /* uint16 [B, vh, vw]           (output_channels=None) */
#define SL_OBS_CHANNELS 2   /* uint16 [B, vh, vw, nch]      (output_channels=(...)) */
#define SL_OBS_CHANNELS_U8 3 /* uint8 [B, vh, vw, nch]      (same values, 1 byte)  */
#define SL_OBS_CHANNELS_F32 4 /* float [B, vh, vw, nch]     0.0 / 1.0: the policy's
                                 layer0 (training/safelife_ppo.py:147-152)        */
#define SL_OBS_CHANNELS_BF16 5 /* bfloat16 [B, vh, vw, nch] 0.0 / 1.0             */

/* Library / device info. */
const char *sl_version(void);
const char *sl_build_id(void);   /* hash of the sources this library was built from */
int sl_device_arch(char *buf, int len);   /* e.g. "gfx950" */

/* Timing events (hipEvent_t as void*) for in-process kernel timing. */
int sl_event_create(void **ev);
int sl_event_destroy(void *ev);
int sl_event_elapsed_ms(void *begin, void *end, float *ms);   /* after completion */
/* Bandwidth reference for roofline reporting (not on the env path): copies n16
 * 16-byte words src -> dst (dev, 16-B aligned) with a grid-stride vector kernel
 * (1024 workgroups, one load per lane per iteration) -- what a plain streaming
 * read+write of the same bytes draws on this GPU. */
int sl_copy16(const void *src, void *dst, int64_t n16, void *stream);

/* ---------------------------------------------------------------- boards -- */

/*
 * Advance B independent boards one step: out[b] = rule(in[b]).
 *   in, out      dev uint16 [B,H,W]; must not alias.  H, W >= 2.
 *   spawn_prob   dev float [B] or NULL (then spawn_prob_scalar for all boards);
 *                each draw u spawns iff u < (double)spawn_prob (a C float, as
 *                the reference parses it with format "f", module.c:22-24).
 *   rng_mode     SL_RNG_STREAM: board b consumes draws[draw_offsets[b] + k] for
 *                its k-th eligible cell in row-major order (draws/draw_offsets
 *                may be NULL when no board can draw: p <= 0 or p >= 1 decide
 *                without a draw).  SL_RNG_PHILOX: u = philox(seed; cell, env0+b,
 *                step, tensor).
 */
int sl_advance(const uint16_t *in, uint16_t *out, int64_t B, int H, int W,
               const float *spawn_prob, float spawn_prob_scalar, int rng_mode,
               uint64_t seed, uint32_t env0, uint32_t step, uint32_t tensor,
               const double *draws, const int64_t *draw_offsets, void *stream);

/* counts[b] = number of uniform draws board b consumes in one advance. */
int sl_count_eligible(const uint16_t *in, int64_t *counts, int64_t B, int H, int W,
                      void *stream);

/*
 * HOST advance of one board (no GPU; csrc/sl_host.cpp): speedups.advance_board's
 * numpy path (module.c:19-44 for a numpy board).
 *   in, out      host uint16 [H,W], row-major, must not alias; 2 <= H, 2 <= W <= 512.
 *   draws        the caller's next n_draws spawn uniforms in reference order (one
 *                per eligible cell, row-major, random.c:47-52).
 * Returns the uniforms consumed (>= 0); -(needed + 1) when the board needs more
 * than n_draws (out unspecified: call again with `needed`); with out == NULL, the
 * number of eligible cells; INT64_MIN for a bad shape.  Thread-safe.
 */
int64_t sl_host_advance(const uint16_t *in, uint16_t *out, int64_t H, int64_t W,
                        float spawn_prob, const double *draws, int64_t n_draws);

/* out[i] = base + sum_{j<i} in[j]; *total_out (dev, may be NULL) = base + sum. */
int sl_exclusive_scan_i64(const int64_t *in, int64_t *out, int64_t n,
                          const int64_t *base, int64_t *total_out, void *stream);

/* -------------------------------------------- seeded reference stream -- */

/*
 * The reference's spawn stream on the device: numpy's legacy RandomState(seed)
 * .random_sample() -- MT19937 seeded by init_genrand, doubles (a >> 5, b >> 6) / 2^53
 * from consecutive outputs -- which speedups.seed(seed) makes the reference draw
 * from in 10 000-double chunks (speedups_src/random.c:14-26,28-44,47-52,
 * module.c:246-253).  Draw d lands in ring[d & (ring_draws - 1)].
 *
 * The stream is cut into blocks of 624 * rounds raw outputs (312 * rounds draws);
 * block q is generated by chain q mod n_chains, whose state then jumps n_chains
 * blocks ahead (x^(n_chains * block) mod the characteristic polynomial, applied
 * to the block's own first raw words).  All buffers are caller-allocated device
 * memory:
 *   chains   uint32 [n_chains, 624]          the MT state of each chain's next block
 *   prefix   uint32 [n_chains, SL_MT_PREFIX] scratch
 *   polys    uint32 [log2(n_chains) + 1, SL_MT_POLY_WORDS] jump polynomials
 *   ctl      int64 [SL_MT_CTL_WORDS] (8): [0] next block to generate, [1] a done
 *            counter, [2] error flags (bit0: a fill asked for a range the ring or
 *            the chains cannot serve), [3] the first block, [4] the next block whose
 *            chain has to jump, [5] a done counter, [6] and [7] the last fill's draw
 *            range [lo, hi) (written by every fill, read by the look-ahead)
 * n_chains is a power of two (one fill generates at most n_chains blocks), rounds
 * >= 33, ring_draws a power of two >= 2 blocks.
 */
#define SL_MT_PREFIX 21216       /* 34 x 624 raw words */
#define SL_MT_CTL_WORDS 8
#define SL_MT_POLY_WORDS 640
typedef struct sl_mt19937 {
    int32_t n_chains;
    int32_t rounds;
    int64_t ring_draws;
    double *ring;
    uint32_t *chains;
    uint32_t *prefix;
    uint32_t *polys;
    int64_t *ctl;                   /* dev int64 [SL_MT_CTL_WORDS] */
    /* look-ahead (sl_mt19937_lookahead): after each fill, the blocks of the next
     * fill's likely range are generated on this second stream, beside the step that
     * consumes the current range; the next fill waits for them.  NULL = off.  The
     * event handles and the flag are the library's. */
    void *ahead_stream;
    void *ev_fill, *ev_ahead;
    int32_t ahead_pending;
    /* bit ring (round 5): bit_ring != 0 makes `ring` a ring of decisions -- draw d is
     * bit (d & 31) of uint32 word (d & (ring_draws - 1)) >> 5 of ring (read as
     * uint32_t, ring_draws / 8 bytes), set iff the draw's double is < bits_thr -- for
     * batches whose envs all spawn with that one threshold (double)(float)p: the
     * replay kernels need only u < p, and the ring then holds 1/64 of the bytes.
     * rounds must be a multiple of 4 (a block's draws fill whole words).  A step in
     * which an env that draws has another threshold sets bit 1 of the stream error
     * flag (SL_STREAM_ERR_THRESHOLD; bit 0 stays the ring's range error).
     * bit_ring == 0 (a zeroed struct): a ring of doubles, bits_thr unused. */
    int32_t bit_ring;
    double bits_thr;
} sl_mt19937;

/* Seed: the stream of RandomState(seed), positioned so that draws from first_draw
 * on can be generated (host polynomial work, then device init; synchronises
 * `stream`).  Re-seed to move the position backwards. */
int sl_mt19937_seed(sl_mt19937 *mt, uint32_t seed, int64_t first_draw, void *stream);
/* Generate every not yet generated block holding a draw below *hi (dev int64);
 * *lo (dev) is the first draw the caller will read.  err (dev int64, may be NULL)
 * is OR-ed with 1 when the range cannot be served (re-seed).  With the look-ahead
 * on, `stream` first waits for the last fill's look-ahead, and after the fill the
 * blocks of [*hi, *hi + 1.25 (*hi - *lo)) (capped by the ring) are generated on the
 * look-ahead stream; mt's flag is updated (mt is const for the device state only). */
int sl_mt19937_fill(const sl_mt19937 *mt, const int64_t *lo, const int64_t *hi, int64_t *err,
                    void *stream);
/* Turn the look-ahead on (ahead_stream = a hipStream_t) or off (NULL); creates /
 * keeps the two events.  sl_mt19937_release destroys them (the device buffers are
 * the caller's). */
int sl_mt19937_lookahead(sl_mt19937 *mt, void *ahead_stream);
int sl_mt19937_release(sl_mt19937 *mt);
/* Host reference pieces (no GPU): the seeded window, x^n mod phi, a jump of a
 * window by a polynomial, and n draws from a window (tests; seeding). */
int sl_mt19937_host_window(uint32_t seed, uint32_t *window624);
int sl_mt19937_host_jump_poly(uint64_t n, uint32_t *poly);
int sl_mt19937_host_jump(const uint32_t *window_in, const uint32_t *poly, uint32_t *window_out);
int sl_mt19937_host_draws(const uint32_t *window, int64_t n, double *out);

/* ------------------------------------------------------- side effects -- */

/*
 * The rollout + density half of side_effect_score (side_effects.py:59-92,
 * 131-139) for E finished episodes at once.  Per episode e: b0 = init_board[e]
 * is advanced num_steps[e] times, then num_samples times alternately with
 * b1 = final_board[e] (b0 then b1, the reference's order); after each of those
 * advances both boards are added to their cell-type density maps
 * (_add_cell_distribution), which are finally divided by num_samples.
 *   num_steps_dev / num_steps_host  the same [E] values, device and host copy
 *   spawn_prob     dev float [E]
 *   rng_mode       SL_RNG_STREAM: E must be 1; draws are consumed from
 *                  draws[*stream_pos] on in the reference's order (advanced);
 *                  SL_RNG_PHILOX: u = philox(seed; cell, env0 + e, advance
 *                  index of that board, 4 + (0: b0, 1: b1)).
 *   keys           dev uint16 [E, max_keys]: the union of both maps' cell-type
 *                  keys, ascending; n_keys dev [E] its size (> max_keys means
 *                  the maps are incomplete: raise max_keys); present dev
 *                  [E, max_keys]: bit0 key occurs in the inaction map (b0),
 *                  bit1 in the action map (b1)
 *   inaction, action  dev double [E, max_keys, H, W] densities per key
 *   workspace      dev scratch of sl_side_effect_workspace() bytes
 * max_keys <= 1024.  The earth mover's distance over the maps
 * (side_effects.py:12-56, third-party pyemd) is host code above this call.
 */
/*
 * Earth mover's distance of side_effect_score (host code; no GPU needed).
 * Replaces pyemd.emd(a[changed], b[changed], dist, extra_mass_penalty) at
 * /root/reference/safelife/side_effects.py:56 (its caller's cell selection and
 * ground distance: side_effects.py:36-55).
 *   p, q         host double [n]: the two densities at the n selected cells
 *   ys, xs       host int32 [n]: the cells' row / column on an H x W board
 *   cost_table   host double [2H-1][2W-1]: ground distance between two cells by their
 *                signed offset (y_i - y_j + H - 1, x_i - x_j + W - 1)
 *   extra_mass_penalty  per unit of |sum p - sum q|; -1: the largest distance used
 *   out          the distance (FastEMD emd_hat semantics, see sl_emd.cpp)
 */
int sl_emd_cells(const double *p, const double *q, const int32_t *ys, const int32_t *xs,
                 int64_t n, const double *cost_table, int H, int W,
                 double extra_mass_penalty, double *out);

int sl_side_effect_workspace(int64_t E, int H, int W, int64_t *bytes);
int sl_side_effect_densities(const uint16_t *init_board, const uint16_t *final_board,
                             const int32_t *num_steps_dev, const int32_t *num_steps_host,
                             const float *spawn_prob, int64_t E, int H, int W,
                             int num_samples, int rng_mode, uint64_t seed, uint32_t env0,
                             const double *draws, int64_t *stream_pos, int max_keys,
                             uint16_t *keys, int32_t *n_keys, int32_t *present,
                             double *inaction, double *action, void *workspace,
                             int64_t workspace_bytes, void *stream);
/*
 * The same with a choice of kernel and per-episode Philox ids.
 *   env_ids  dev uint32 [E] or NULL: episode e draws as env env_ids[e] (NULL: env0 + e),
 *            so a batch of finished episodes keeps each episode's own id whatever
 *            batch it lands in (ignored by SL_RNG_STREAM)
 *   kernel   SL_KERNEL_GENERIC: one per-cell LDS launch per advance plus one mark /
 *            count launch per sample, any shape up to 32768 cells;
 *            SL_KERNEL_FAST: the bit-sliced rollout, one wave per board and one launch
 *            per pass (four launches per call) -- Philox draws on 64x64 boards and on
 *            boards of H <= 32, W <= 64; SL_ETOOBIG elsewhere;
 *            SL_KERNEL_BANDS: the bit-sliced rollout of 128x128 boards, one workgroup
 *            of four waves per board (a wave per band of 32 rows, the band in
 *            registers, one halo row each way through LDS per advance), the same four
 *            launches per call -- Philox draws on 128x128 boards; SL_ETOOBIG elsewhere;
 *            SL_KERNEL_MID: the bit-sliced rollout of boards of 33 to 64 rows and 2 to 64
 *            columns, 64x64 aside (the shapes of the mid env step), one wave per board:
 *            lane 2j + h holds columns 2j, 2j + 1 over rows 32h .. 32h + 31, the same
 *            four launches per call -- Philox draws on those shapes, read as uint16 (no
 *            alignment rule); SL_ETOOBIG elsewhere, stream mode included.  SL_KERNEL_FAST
 *            keeps its shape set and is SL_ETOOBIG on these boards;
 *            SL_KERNEL_WIDE: the bit-sliced rollout of boards of up to 128 x 128 with more
 *            than 64 rows or more than 64 columns, 128x128 aside (the shapes of the wide
 *            env step), one workgroup of ceil(H / 32) waves per board: a wave per band of
 *            32 rows, lane j the columns 2j, 2j + 1, the band in registers, one halo row
 *            each way through LDS per advance, the same four launches per call -- Philox
 *            draws on those shapes, read as dwords where W is even and the address a
 *            multiple of 4 and as uint16 otherwise (no alignment rule); SL_ETOOBIG
 *            elsewhere, stream mode included.  Opt-in: SL_KERNEL_AUTO never picks it;
 *            SL_KERNEL_AUTO: what sl_side_effect_kernel_auto names: FAST where it
 *            exists, BANDS on 128x128 boards with Philox draws, else GENERIC.  On the
 *            MID shapes of at least 32 columns (at least half of the wave's lanes hold
 *            cells) with Philox draws it names MID, by the measurement of DESIGN.md 6.4
 *            (one constant, kAutoTakesMidRollout); narrower MID shapes stay on GENERIC
 *            under AUTO in this version and are served by SL_KERNEL_MID when asked for.
 *            The 64x64 and 128x128 kernels load dwords: such boards at an address that
 *            is no multiple of 4 go to GENERIC under AUTO and are SL_EINVAL under FAST
 *            or BANDS.
 * All kernels give the same bytes.  sl_side_effect_densities is
 * _k(..., NULL, SL_KERNEL_AUTO, stream).
 */
int sl_side_effect_densities_k(const uint16_t *init_board, const uint16_t *final_board,
                               const int32_t *num_steps_dev, const int32_t *num_steps_host,
                               const float *spawn_prob, int64_t E, int H, int W,
                               int num_samples, int rng_mode, uint64_t seed, uint32_t env0,
                               const double *draws, int64_t *stream_pos, int max_keys,
                               uint16_t *keys, int32_t *n_keys, int32_t *present,
                               double *inaction, double *action, void *workspace,
                               int64_t workspace_bytes, const uint32_t *env_ids, int kernel,
                               void *stream);
/* SL_KERNEL_FAST if SL_KERNEL_AUTO takes the one-wave rollout for such a call, else
 * SL_KERNEL_GENERIC (host only; no GPU needed) */
int sl_side_effect_kernel(int H, int W, int rng_mode);
/* the kernel SL_KERNEL_AUTO launches for such a call: SL_KERNEL_GENERIC, SL_KERNEL_FAST,
 * SL_KERNEL_BANDS or SL_KERNEL_MID (host only; no GPU needed; boards the dword loads cannot take,
 * see above, go to GENERIC all the same) */
int sl_side_effect_kernel_auto(int H, int W, int rng_mode);

/*
 * The EMD problems of side_effect_score, cut from the dense maps on the device
 * (earth_mover_distance's cell selection, side_effects.py:36-56: the cells where the
 * two maps differ by more than 1e-3 of their largest difference, row-major).
 * inaction / action / n_keys are what sl_side_effect_densities_k wrote.  Problem
 * e * max_keys + k is episode e's key slot k, for k < min(n_keys[e], max_keys); the
 * other slots are never read and have 0 cells and mass 0.  H, W >= 2, H * W <= 32768,
 * 1 <= max_keys <= 1024; E == 0 is SL_OK and touches nothing.
 *
 * sl_side_effect_problem_counts (side_effects.py:36-41): per problem the number of
 * selected cells -- |a - b| > 1e-3 * max |a - b|, strictly, the IEEE operations numpy
 * performs; none when the maps are equal -- scanned into
 *   offsets  dev int64 [E * max_keys + 1]: problem i owns cells offsets[i] ..
 *            offsets[i + 1]; the last entry is the total (the scan runs over the counts
 *            plus one trailing zero)
 *   mass     dev double [E * max_keys]: the inaction map's sum (side_effects.py:158's
 *            np.sum up to summation order: per-thread strided sums, a wave butterfly,
 *            four wave sums in order; see sl_side_effect_problems.hip)
 *   workspace  dev scratch of sl_side_effect_problems_workspace() bytes, 8-byte aligned;
 *            keeps each problem's threshold for the fill pass
 *
 * sl_side_effect_problem_cells (side_effects.py:41,56): with the same maps, offsets and
 * workspace, stores problem i's cells in row-major order at offsets[i] + rank:
 *   p, q     dev double [cap]: the inaction / action density at the cell
 *   ys, xs   dev int32 [cap]: its row and column
 *   cap      the buffers' length (the total of offsets); nothing is stored at or
 *            beyond cap
 */
int sl_side_effect_problems_workspace(int64_t E, int max_keys, int64_t *bytes);
int sl_side_effect_problem_counts(const double *inaction, const double *action,
                                  const int32_t *n_keys, int64_t E, int max_keys, int H, int W,
                                  int64_t *offsets, double *mass, void *workspace,
                                  int64_t workspace_bytes, void *stream);
int sl_side_effect_problem_cells(const double *inaction, const double *action,
                                 const int32_t *n_keys, int64_t E, int max_keys, int H, int W,
                                 const int64_t *offsets, double *p, double *q, int32_t *ys,
                                 int32_t *xs, int64_t cap, void *workspace,
                                 int64_t workspace_bytes, void *stream);
/*
 * nprob earth mover's distances at once (host code; no GPU needed): problem i is the
 * cells offsets[i] .. offsets[i + 1] of p, q, ys, xs (host arrays; offsets host int64
 * [nprob + 1], non-decreasing), and out[i] (host double [nprob]) is exactly what
 * sl_emd_cells returns for that slice (side_effects.py:36-56), 0 for an empty one.
 * Runs on min(nthreads, nprob) std::threads (the caller's included), nthreads >= 1;
 * nprob == 0 is SL_OK; otherwise every pointer must be non-null, also when no problem has
 * a cell.  Returns the code of the lowest-numbered failing problem (SL_ETOOBIG: out of
 * memory); a thread that cannot be started is done without.
 */
int sl_emd_cells_batch(const double *p, const double *q, const int32_t *ys, const int32_t *xs,
                       const int64_t *offsets, int64_t nprob, const double *cost_table,
                       int H, int W, double extra_mass_penalty, double *out, int nthreads);
/*
 * The same distances solved on the device (k_emd_cells, sl_emd_device.hip: one wave per
 * problem): what pyemd.emd returns at the reference's side_effects.py:56 for each
 * problem's cells, bit for bit what sl_emd_cells returns for them -- the same IEEE
 * double operations in the same order around an integer transport problem whose optimum
 * does not depend on the method.  All pointers are device pointers: p, q, ys, xs and
 * offsets (int64 [nprob + 1]) as sl_side_effect_problem_cells leaves them, cost_table
 * double [2H-1][2W-1], out double [nprob], status int32 [nprob].
 *   status[i] >= 0  solved: out[i] is the distance and status[i] the number of simplex
 *                   pivots it took (0 also for a problem without cells, out[i] = 0.0,
 *                   and for the cases decided without a transport)
 *   status[i] <  0  not solved, out[i] = 0.0:
 *     SL_EMD_ST_BADCELL  a cell off the board (sl_emd_cells: SL_EINVAL); checked before
 *                        any table read
 *     SL_EMD_ST_TOOBIG   more than SL_EMD_DEVICE_MAX_CELLS cells (or a negative count):
 *                        not attempted; the limit is what one wave's share of LDS holds
 *                        (14 656 B per problem)
 *     SL_EMD_ST_PIVOTS   the pivot cap (a fixed multiple of the transport's node count)
 *                        ran out, or a consistency check of the tree failed
 *   A caller solves the TOOBIG and PIVOTS problems with sl_emd_cells_batch.
 * nprob == 0 is SL_OK without a launch; nprob < 0, H or W < 1 or > 32768, nprob > 2^31 - 1
 * or a null pointer with nprob > 0 is SL_EINVAL before any launch.
 */
#define SL_EMD_DEVICE_MAX_CELLS 256
#define SL_EMD_ST_BADCELL (-1)
#define SL_EMD_ST_TOOBIG (-2)
#define SL_EMD_ST_PIVOTS (-3)
int sl_emd_cells_device(const double *p, const double *q, const int32_t *ys, const int32_t *xs,
                        const int64_t *offsets, int64_t nprob, const double *cost_table,
                        int H, int W, double extra_mass_penalty, double *out, int32_t *status,
                        void *stream);

/* ------------------------------------------------------------------ envs -- */

/* Per-env state, structure of arrays, all dev pointers, length B unless noted. */
typedef struct sl_env_state {
    int64_t B;
    int32_t H, W;
    uint16_t *board;          /* [B,H,W]  game.board                          */
    uint16_t *goals;          /* [B,H,W]  game.goals                          */
    uint16_t *start_board;    /* [B,H,W]  game._init_data['board']            */
    int32_t *agent_x, *agent_y, *orientation;
    int32_t *game_over;
    int32_t *episode_length;
    int32_t *episode_reward;  /* SafeLifeEnv's own (integer) reward sum       */
    int32_t *old_points;      /* SafeLifeEnv._old_game_value                  */
    int32_t *baseline;        /* perf baseline over _init_data (per episode)  */
    int32_t *score;           /* current perf score (unit rewards)            */
    int32_t *possible;        /* perf possible score                          */
    int32_t *side_effect;     /* SimpleSideEffectPenalty.last_side_effect     */
    float *spawn_prob;
    double *min_performance;  /* game.min_performance                         */
    int32_t *prior_x;         /* [B, SL_BONUS_PERIOD_MAX] position ring        */
    int32_t *prior_y;
    int32_t *prior_len;       /* entries in the ring (deque length)           */
    int32_t *prior_head;      /* index of the oldest entry                    */
    int32_t *exit_count;
    int16_t *exit_y, *exit_x; /* [B, SL_MAX_EXITS], np.nonzero order          */
    int32_t *level_index;     /* level of the current episode                 */
    int32_t *episodes;        /* episodes started by this env                 */
    int32_t *num_steps;       /* game.num_steps                               */
    int32_t *spawn_flags;     /* bit0: board, bit1: goals may hold a spawning
                                 cell (set at reset; spawning bits are never
                                 created by the rule or the actions -- except a
                                 power toggle, which the kernels allow for -- only
                                 moved).  The replay prologues skip the eligible
                                 count of a tensor whose bit is clear: a caller
                                 writing state sets both bits.
                                 128x128 boards only (0 on other shapes):
                                 bit2: the start board may use cell bits 12-14
                                 (no cell type does; set at reset from the level):
                                 the 128x128 kernel keeps no start planes for them
                                 and takes such an env's exact side-effect term in
                                 a second pass.  A caller writing start boards
                                 sets it where they carry those bits.
                                 bit3: a goal cell uses bits other than alive,
                                 destructible, frozen and colours (set at reset):
                                 with bits 1 and 3 clear the 128x128 kernel keeps
                                 the goals' six planes in the mirror and reads
                                 them from there.                              */
    int32_t *start_roll;      /* (dy << 16) | dx: start_board[b] equals pool
                                 level level_index[b] rolled by (dy, dx) (set by
                                 every reset); -1: start_board was written by
                                 the caller.  Lets the 64x64 kernel read the
                                 start board from the cache-resident pool.     */
    uint32_t *planes;         /* bit-plane mirror of the goals kept by the
                                 bit-sliced kernels, or NULL (then 128x128
                                 boards take the generic kernel).
                                 64x64: [B,2,32,64], half 1 (half 0 reserved):
                                 [b][1][q][lane], word q = plane q & 15 of
                                 column 2(lane>>1) + (q>>4), rows
                                 32(lane&1)..+31 (sl_bits.hip).
                                 128x128: [B,4,32,64], [b][t][q][lane], word q
                                 = plane q & 15 of column 2 lane + (q>>4),
                                 rows 32t..32t+31 (sl_bits128.hip).
                                 Derived data, never read unless planes_ok
                                 has SL_POK_GOALS_MIRROR.                      */
    int32_t *planes_ok;       /* [B] which of the derived copies above and below
                                 are valid: SL_POK_* bits (sl_planes_ok_bits,
                                 after this struct).  Zero-init.               */
    uint32_t *elig_planes;    /* replay mode, 128x128, [B][1024] words: the
                                 draw planes [tensor][band t][word w][lane] (bit
                                 y of word w of lane j = cell (32t + y, 2j + w)).
                                 The step kernel leaves the advanced board's
                                 eligible cells in tensor 0's (SL_POK_ELIG);
                                 the next step's count patches the rows its
                                 action edited and counts them; the draw pass
                                 replaces each drawing tensor's eligible cells
                                 with those whose uniforms spawn, before the
                                 step kernel runs.  Or NULL (the step kernel
                                 then ranks and draws itself)                  */
    uint32_t *board_planes;   /* 128x128, or NULL: [B,4,32,64] u32 in the goals
                                 mirror's layout ([b][t][q][lane], word q =
                                 plane q & 15 of column 2 lane + (q >> 4), rows
                                 32t..32t+31).  When set, a step of the fast
                                 kernel without capture -- Philox or replay with
                                 draw planes; no obs_out, or packed views of at
                                 most 96 rows (with SL_OBS_FUSE_CHAN128 also
                                 channel views), which it writes from the planes;
                                 sl_env_cfg.board_mode SL_BOARD_AUTO -- keeps
                                 the board here (SL_POK_BOARD_PLANES) and writes of
                                 the uint16 board only its band-edge rows (32t,
                                 32t + 31) and the cells the action and exits
                                 edit: SL_POK_BOARD_FULL then says the uint16
                                 board is complete.  sl_env_board_sync completes it (a
                                 per-env no-op for envs not in planes or
                                 already complete); the library's other entry
                                 points that read or write st->board do so
                                 themselves.  A caller that writes the uint16
                                 board: see sl_planes_ok_bits.
                                 64x64: board_planes == planes puts
                                 the board's planes in half 0 of the goals
                                 mirror (Philox steps without capture: with no
                                 obs_out, with packed views, or with channel
                                 views of at most 64x64 and 1094 cells into a
                                 16-byte aligned obs_out, all written from the
                                 planes; SL_POK_BOARD_FULL only after a sync). */
    uint32_t board_zero;      /* plane mode (64x64, 128x128): cell bits (planes) that are
                                 0 in every board of the batch and that no rule,
                                 action or reset can set (the caller's promise:
                                 none in its levels or written boards, not
                                 LIFE / COLOR_R, not toggled powers / colours);
                                 their planes are neither loaded nor stored.
                                 To widen it, complete the board first
                                 (sl_env_board_sync) and clear SL_POK_BOARD.
                                 0 = every plane.                              */
    int32_t planes_live;      /* host flag, kept by the library: a plane-mode
                                 step set it (some board may be in planes);
                                 a demotion clears it.  While 0 the syncs the
                                 entry points run are skipped.  Zero-init; a
                                 caller stepping a slice (a copy of this
                                 struct) ORs the slice's flag back in.         */
    uint32_t agent_planes;    /* 64x64 plane mode: cell bits (planes) that, in every
                                 board of the batch and for good, are set in the
                                 agent's cell (agent_y, agent_x) and in no other
                                 (the caller's promise: in its levels and written
                                 boards they sit on the agent's cell alone, that
                                 cell is frozen, and no birth, spawn, exit or
                                 allowed toggle sets them).  Their planes are
                                 neither loaded nor stored: the kernels build them
                                 from the agent's position, and sl_env_board_sync
                                 puts them into the completed uint16 board.  Never
                                 overlaps board_zero.  Changes as board_zero does:
                                 complete the board first and clear SL_POK_BOARD;
                                 clearing bits is always safe then.  0 = none.
                                 128x128 kernels ignore it.                     */
    uint32_t goals_gray;      /* 64x64 plane mode, 0 or 1: every goal cell of every
                                 env of the batch has its three colour bits (9, 10,
                                 11) equal -- black or white -- and stays so: the
                                 rule computes each colour plane by the same function
                                 of the same-numbered plane, actions never edit
                                 goals, and resets draw from a pool of which the
                                 same holds (the caller's promise).  Rows black and
                                 white of the point table are equal and neither
                                 counts as possible, so with the C3 / C4 planes and
                                 agent planes (board_zero, agent_planes) the step
                                 without views reads no goal colour from the mirror
                                 and the step with packed views one plane of three;
                                 other plane masks and channel views keep loading
                                 all three.  The mirror is still written in full
                                 (resets, the goals' own step): only reads are
                                 skipped.  Set by the caller from its pool, cleared
                                 by the caller -- never by the library -- before a
                                 pool with a coloured goal cell is admitted or the
                                 goals are written from outside (besides clearing
                                 SL_POK_GOALS); needs no board sync and no
                                 planes_ok change; never set again while envs run
                                 whose goals are not known.  0 = goals of any
                                 colour.  128x128 kernels ignore it.             */
    uint32_t derived_planes;  /* 64x64 plane mode: cell bits (planes), of 8 and 15
                                 (mask 0x8100), that every board of the batch holds
                                 but that follow from the rest of the env's state,
                                 for good (the caller's promise, for its levels and
                                 written boards):
                                 bit 15: plane 15 equals plane 2 in every cell (only
                                 a crate carries either bit; actions move whole cells
                                 or write LIFE | colour, the rule clears both
                                 together; needs can_toggle_powers == 0, or the agent
                                 can take bit 2 alone);
                                 bit 8: the cells with EXIT are exactly the env's
                                 exit list (exit_y, exit_x, exit_count <=
                                 SL_MAX_EXITS; an exit is frozen, never pushed,
                                 made or destroyed).
                                 Their planes are neither loaded nor stored: the
                                 kernels rebuild them in registers, and
                                 sl_env_board_sync puts them into the completed
                                 uint16 board.  The stored words are packed
                                 without them, so the flag changes the layout: it
                                 changes as agent_planes does (complete the board
                                 first and clear SL_POK_BOARD; clearing bits is
                                 always safe then).  The kernels derive both
                                 planes or neither: one bit alone counts as none.
                                 Bits outside 0x8100, in board_zero or in
                                 agent_planes are ignored.  0 = none.  128x128
                                 kernels ignore it.                              */
} sl_env_state;

/*
 * The bits of sl_env_state.planes_ok[b]: which derived copies of env b's state are
 * valid.  "Step" is a step of the bit-sliced 64x64 / 128x128 kernels; the per-cell
 * kernels (sl_env_action and sl_env_advance, and sl_env_step on other shapes or with
 * SL_KERNEL_GENERIC) keep no copies and store 0.  Every reset rewrites the word (it
 * writes the uint16 board and goals): 64x64 to SL_POK_GOALS_MIRROR (it rebuilds the
 * mirror), 128x128 to SL_POK_GOALS_LEVEL.
 *
 * SL_POK_GOALS_MIRROR  64x64, 128x128.  `planes` mirrors the goals.  Set by the 64x64
 *     reset and by a step that advanced the goals (it rebuilds a stale mirror).
 * SL_POK_GOALS_FIXED   64x64, 128x128.  The goals hold no spawner and came through a
 *     step unchanged: the rule is skipped from then on.  Set by that step.
 * SL_POK_GOALS_SIX     128x128.  The mirror holds all six goal planes (spawn_flags
 *     bits 1 and 3 clear), not only the colours.  Set by the step that (re)built it.
 * SL_POK_GOALS_LEVEL   128x128.  The goals are still the pool level's: their colours
 *     come from the pool's goal_planes.  Set by the reset, cleared by the first step
 *     that changes the goals.
 * SL_POK_ELIG          128x128 replay with elig_planes.  The board's draw planes hold
 *     its eligible cells as the last step left them.  Set by a decided replay step,
 *     cleared by every other step.
 * SL_POK_BOARD_PLANES  64x64, 128x128.  board_planes hold the board.  Set by a
 *     plane-mode step; cleared (after completing the uint16 board) by every library
 *     entry point that writes it: a step in another mode, sl_env_action,
 *     sl_env_advance.
 * SL_POK_BOARD_FULL    64x64, 128x128; with SL_POK_BOARD_PLANES.  The uint16 board is
 *     complete too (else only its band-edge rows and exit cells).  Set by
 *     sl_env_board_sync and by a 128x128 step into plane mode, cleared by the next
 *     plane-mode step.
 * SL_POK_BOARD_LO12    128x128 decided replay; with SL_POK_BOARD_PLANES.  Board planes
 *     12-14 are zero and not kept.  Set by the step into plane mode that found them
 *     zero.
 *
 * A caller that writes state from outside the library:
 *   - the goals: clear SL_POK_GOALS, and sl_env_state.goals_gray unless every cell
 *     written is black or white (see there);
 *   - the uint16 board: complete it first (sl_env_board_sync), write, then clear
 *     SL_POK_ELIG | SL_POK_BOARD (and widen board_zero first if the cells written use
 *     planes in it: see there);
 *   - everything (a restored checkpoint): store 0.
 */
enum sl_planes_ok_bits {
    SL_POK_GOALS_MIRROR = 2,
    SL_POK_GOALS_FIXED = 4,
    SL_POK_ELIG = 8,
    SL_POK_GOALS_SIX = 16,
    SL_POK_GOALS_LEVEL = 32,
    SL_POK_BOARD_PLANES = 64,
    SL_POK_BOARD_FULL = 128,
    SL_POK_BOARD_LO12 = 256,
    SL_POK_GOALS = SL_POK_GOALS_MIRROR | SL_POK_GOALS_FIXED | SL_POK_GOALS_SIX |
                   SL_POK_GOALS_LEVEL,
    SL_POK_BOARD = SL_POK_BOARD_PLANES | SL_POK_BOARD_FULL | SL_POK_BOARD_LO12
};

/* A device-resident level pool (the level_iterator's levels). */
typedef struct sl_level_pool {
    int32_t K, H, W;
    const uint16_t *board;    /* [K,H,W] as stored (exits uncoloured)         */
    const uint16_t *goals;    /* [K,H,W]                                      */
    const int32_t *agent_x, *agent_y, *orientation;
    const float *spawn_prob;
    const double *min_performance;  /* the level's own value (used for the
                                       reset-time exit colour only)           */
    uint64_t *board_planes;   /* bit planes of the pool boards, or NULL
                                 (sl_level_pool_prepare; the bit-sliced kernels'
                                 start-board source):
                                 64x64 pools: uint64 [K,16,W], element [k][p][x]
                                 bit y = bit p of board[k][y][x];
                                 128x128 pools: uint32 [K,16,4,W] (8*K*16*W
                                 bytes), element [k][p][q][x] bit r = bit p of
                                 board[k][32q + r][x]                          */
    uint32_t *goal_planes;    /* 128x128 pools: the goals' colour planes, uint32
                                 [K,3,4,W], element [k][c][q][x] bit r = bit 9+c
                                 of goals[k][32q + r][x]; or NULL.  The 128x128
                                 kernel scores goals still as the level had them
                                 from here (cache-resident) instead of the
                                 env's mirror (sl_level_pool_prepare fills it) */
} sl_level_pool;

/* Fill pool->board_planes (caller-allocated, dev, layout above; H must be 64 or
 * 128) from pool->board.  Derived data only; the reference keeps levels as npz
 * (safelife_game.py:184-194). */
int sl_level_pool_prepare(sl_level_pool *pool, void *stream);

/*
 * Trajectory capture (SafeLifeRecorder, /root/reference/safelife/env_wrappers.py:97-136):
 * sl_env_step copies the state of n chosen envs twice per step -- right after the
 * board advance, before any reset (the frame the reference captures after
 * env.step), and after the step's resets (the first frame of the next episode,
 * meaningful where flags & 4).  Copies only; the stepping itself is unchanged.
 * env and flags are required; every other target is a dev pointer or NULL, and a
 * NULL target is not copied (with all three reset_* NULL the second copy is skipped).
 */
typedef struct sl_capture {
    int32_t n;                    /* envs recorded (0: none)                       */
    const int32_t *env;           /* dev [n] env indices (required)                */
    uint16_t *board, *goals;      /* dev [n, H, W] or NULL  after the advance      */
    int32_t *orientation;         /* dev [n] or NULL                                */
    uint8_t *flags;               /* dev [n]  the step's info flags (required)     */
    uint16_t *reset_board, *reset_goals;   /* dev [n, H, W] or NULL  after the resets */
    int32_t *reset_orientation;   /* dev [n] or NULL                                */
    /* the finished episode's record (EpisodeLog), each dev or NULL; copied with the
       frame after the advance, before any reset overwrites them */
    uint16_t *start_board;        /* dev [n, H, W]                                  */
    int32_t *score, *possible;    /* dev [n]  performance_ratio() returns            */
    int32_t *baseline;            /*          (score - baseline, possible - baseline) */
    int32_t *num_steps;           /* dev [n]  board advances of the episode         */
    float *spawn_prob;            /* dev [n]                                        */
    double *min_performance;      /* dev [n]                                        */
    int32_t *episode_length, *episode_reward, *level_index;   /* dev [n]            */
} sl_capture;

typedef struct sl_env_cfg {
    int32_t time_limit;             /* SafeLifeEnv.time_limit (1000)          */
    int32_t auto_reset;             /* 1: ContinuingEnv + caller reset-on-done */
    int32_t can_toggle_powers, can_toggle_colors;
    double penalty_coef;            /* SimpleSideEffectPenalty (scheduled)    */
    double wrapper_min_performance; /* SimpleSideEffectPenalty.min_performance;
                                       applied at reset (NaN = keep level's)  */
    const double *bonus_table;      /* dev [bonus_len]: movement_bonus *
                                       (d/period)**power for integer d        */
    int32_t bonus_len;
    int32_t bonus_period;           /* movement_bonus_period (<= 16; 0 = off) */
    int32_t rng_mode;               /* SL_RNG_*                               */
    uint64_t seed;
    uint32_t step;                  /* batched-step index (Philox counter)     */
    uint32_t env0;                  /* global id of env 0 (multi-GPU shards)   */
    const double *draws;            /* SL_RNG_STREAM: dev uniform stream       */
    int64_t n_draws;
    int64_t *stream_pos;            /* dev [1]: next unread draw (advanced)    */
    int64_t *scratch;               /* dev [8*B + 16] workspace, zeroed once
                                     * before the first step (layout:
                                     * sl_env_common.h Scratch).  With auto_reset the
                                     * 64x64 / 128x128 kernels queue finished envs
                                     * in per-parity lists (words 8B+2, 8B+3) that
                                     * stay valid only over consecutive steps
                                     * (step, step+1, ...) with auto_reset set: zero
                                     * words 8B+2..8B+3 again after any other
                                     * sequence (rewound step index, auto_reset
                                     * toggled, state written by the caller)     */
    int32_t level_mode;             /* 0: level = (env0+b + episodes*n_total)%K,
                                       1: Philox-random level                  */
    int32_t n_total_envs;           /* envs across all shards                  */
    int32_t augment_roll;           /* 1: random toroidal roll per episode     */
    void *ev_begin, *ev_end;        /* optional hipEvent_t pair recorded right
                                       before and after the board-advance (step)
                                       kernel's launch (profiling; an event record
                                       holds the next dispatch until written)  */
    int32_t kernel;                 /* SL_KERNEL_*: which advance kernel       */
    void *obs_out;                  /* dev: sl_env_step also writes every env's
                                       observation after the step (auto-resets
                                       included), exactly as sl_env_obs with the
                                       fields below would; NULL = no observation.
                                       The 64x64 kernels write packed views, and
                                       channel views of at most 64x64 and 1094
                                       cells into a 16-byte aligned obs_out, from
                                       the board they hold on chip (no re-read;
                                       in plane mode from the planes, which stay).
                                       The 128x128 kernel writes packed views of at
                                       most 96 rows from the board planes, and with
                                       obs_fuse & SL_OBS_FUSE_CHAN128 channel views
                                       of at most 96 rows and
                                       SL_FUSE_CHAN128_MAX_CELLS cells into a
                                       16-byte aligned obs_out                  */
    int32_t obs_mode, obs_vh, obs_vw, obs_remove_white, obs_nch;
    int32_t obs_channels[16];
    const sl_capture *capture;      /* host pointer or NULL: trajectory capture
                                       (needs auto_reset and info_flags)      */
    int32_t stream_phase;           /* SL_RNG_STREAM with the batch split over
                                       shards (SURVEY §8(e) collective 3: the
                                       reference's one stream runs env after env
                                       over ALL shards, training/ppo.py:436-452):
                                       0 = the whole step, this batch alone;
                                       1 = count phase: the actions, then each
                                       env's eligible cells; *stream_pos = this
                                       batch's draw total (no draw, no advance);
                                       2 = draw phase (after a phase-1 call on the
                                       same state): this batch's draws start at
                                       *stream_base -- the global position plus
                                       the totals of the shards before it --, the
                                       step completes, *stream_pos = *stream_base
                                       + the batch's total                     */
    const int64_t *stream_base;     /* dev [1]: phase 2's first uniform        */
    const sl_mt19937 *mt;           /* SL_RNG_STREAM: host pointer or NULL.  When
                                       set, the draws come from this device
                                       generator's ring (draws / n_draws are not
                                       read): after the offsets scan each step
                                       fills it for the step's range, so the
                                       stream is RandomState(seed) from
                                       *stream_pos on with no host buffer      */
    int32_t board_mode;             /* SL_BOARD_*: where a 128x128 step leaves the
                                       board (sl_env_state.board_planes)       */
    int32_t planes64_waves;         /* 64x64 plane mode, C3 / C4 planes, gray goals,
                                       no views: 0 or 6, the kernel sized for six
                                       waves per SIMD; 5, its five-wave twin (same
                                       results; kept for comparison).  With
                                       auto_reset from a pool (and no capture) the
                                       six-wave kernel ends each wave after its plane
                                       stores and a second kernel runs the epilogue
                                       one lane per env and resets the finished envs
                                       (the 32 B per env handed over lie in scratch
                                       words [4B, 8B), which must be 16-byte aligned);
                                       SL_PLANES64_W6_UNSPLIT keeps the six-wave
                                       kernel with the epilogue in the wave and the
                                       reset list (same results; for comparison) */
    int32_t obs_fuse;               /* SL_OBS_FUSE_* bits; 0: the defaults     */
} sl_env_cfg;

/*
 * One env-step for all B envs (in place on `st`).
 *   actions     dev int32 [B], 0..8 (safelife_env.py:61-71)
 *   reward      dev double [B]      chain reward (float64, as Python computes it)
 *   done        dev uint8 [B]       done as returned to the caller (times_up)
 *   info_flags  dev uint8 [B] or NULL: bit0 times_up, bit1 game_over,
 *               bit2 env was reset this step
 *   ep_len, ep_reward  dev int32 [B] or NULL: finished-episode length / reward
 * With cfg->auto_reset the done/game-over envs are reset from `pool` before
 * returning (so the next sl_env_obs sees the new episode); the 64x64 kernel
 * does this inside the step kernel, the other paths with a second kernel.
 */
int sl_env_step(sl_env_state *st, const sl_level_pool *pool, const int32_t *actions,
                const sl_env_cfg *cfg, double *reward, uint8_t *done,
                uint8_t *info_flags, int32_t *ep_len, int32_t *ep_reward,
                void *stream);

/* which step kernel family sl_env_step runs for this shape and request:
   SL_FAMILY_GENERIC, _SMALL_SEG4, _SMALL, _MID, _BITS64, _BITS128; SL_ETOOBIG where
   kernel == SL_KERNEL_FAST and no bit-sliced kernel takes H x W; SL_EINVAL otherwise bad
   (host only; no GPU needed).  kernel == SL_KERNEL_WIDE: SL_FAMILY_WIDE where 2 <= H <= 128,
   2 <= W <= 128, H > 64 or W > 64 and not 128x128, SL_ETOOBIG for every other shape with
   H, W >= 1; no other request answers SL_FAMILY_WIDE.  sl_env_step takes its kernel from this very function; a
   128x128 state without the goals mirror (sl_env_state.planes) goes to the generic kernel
   under SL_KERNEL_AUTO and is SL_ETOOBIG under SL_KERNEL_FAST all the same. */
int sl_env_step_family(int H, int W, int kernel);

/* sl_step_plan.obs: who writes the step's views */
#define SL_PLAN_OBS_NONE 0
#define SL_PLAN_OBS_FUSED64 1    /* the 64x64 step kernel (and its reset list)          */
#define SL_PLAN_OBS_FUSED128 2   /* the 128x128 step kernel, then the reset envs' views:
                                    packed views (k_env_step_bits128_view), or with
                                    SL_OBS_FUSE_CHAN128 channel views (view_kind 2-4:
                                    k_env_bits128_chan), both from the board planes     */
#define SL_PLAN_OBS_SEPARATE 3   /* the observation kernel over all envs, after resets  */
/* sl_step_plan.resets: who resets the finished envs */
#define SL_PLAN_RESETS_NONE 0
#define SL_PLAN_RESETS_IN_KERNEL 1   /* the small / mid step kernel, each wave its own   */
#define SL_PLAN_RESETS_LIST64 2      /* k_env_reset_list over the step kernel's list     */
#define SL_PLAN_RESETS_SPLIT_TAIL64 3 /* k_env_epilogue_reset64 after k_env_planes64_s6  */
#define SL_PLAN_RESETS_LIST128 4     /* k_env_reset_list_wide over the step kernel's list */
#define SL_PLAN_RESETS_SCAN 5        /* k_env_reset_scan over the step's flags           */
/* sl_step_plan.kernel64: the 64x64 instance family (0 for every other family) */
#define SL_PLAN_K64_NONE 0
#define SL_PLAN_K64_BITS64 1   /* k_env_step_bits64<view_kind, spawn mode>               */
#define SL_PLAN_K64_PLANES 2   /* k_env_step_bits64_planes<keep, view_kind>              */
#define SL_PLAN_K64_GRAY 3     /* k_env_planes64_gray<C3, view_kind>                     */
#define SL_PLAN_K64_W6 4       /* k_env_planes64_w6<C3>                                  */
#define SL_PLAN_K64_S6 5       /* k_env_planes64_s6<C3>, then the split tail             */
#define SL_PLAN_K64_CHAN 6     /* k_env_planes64_chan<keep, element size of view_kind>   */
/* sl_step_plan.keep: the plane instances' class of kept board planes */
#define SL_PLAN_KEEP_RUNTIME 0 /* from board_zero / agent_planes at run time             */
#define SL_PLAN_KEEP_C3 1      /* planes 0x877F with agent planes 0x0062, compiled in    */
#define SL_PLAN_KEEP_ALL 2     /* all sixteen                                            */

/* What sl_env_step would run for this state, pool, cfg and info_flags: every decision it
 * takes before its first launch.  Host only; no GPU needed, nothing is launched and no
 * device pointer is read (sl_env_step itself runs from this plan). */
typedef struct sl_step_plan {
    int32_t empty;          /* 1: the state holds no env; nothing runs, nothing else is set */
    int32_t family;         /* SL_FAMILY_*: sl_env_step_family's answer, or generic for a
                               128x128 state without the goals mirror                     */
    int32_t replay;         /* SL_RNG_STREAM                                              */
    int32_t stream_phase;   /* sl_env_cfg.stream_phase                                    */
    int32_t plane_mode;     /* the step keeps the board in sl_env_state.board_planes      */
    int32_t demote_first;   /* boards in planes are completed and the planes marked stale
                               before the step                                            */
    int32_t obs;            /* SL_PLAN_OBS_*                                              */
    int32_t resets;         /* SL_PLAN_RESETS_*                                           */
    int32_t capture;        /* 1: sl_env_cfg.capture is taken (small / mid resets then move
                               to the scan, after the first frame)                        */
    int32_t kernel64;       /* SL_PLAN_K64_*                                              */
    int32_t keep;           /* SL_PLAN_KEEP_* (kernel64 PLANES, GRAY, W6, S6, CHAN)       */
    int32_t view_kind;      /* views the step kernel writes: 0 none, 1 packed, 2 u16 / bf16
                               channels, 3 u8 channels, 4 f32 channels                    */
    int32_t stored;         /* 64x64 plane mode: the board planes the step loads and stores
                               (held, not the agent's, not derived); 0x061D for the C3 / C4
                               planes with agent planes 0x0062 and derived planes 0x8100   */
    int32_t derived;        /* 64x64 plane mode: the planes of sl_env_state.derived_planes
                               the step rebuilds in registers (0x8100 less board_zero, or 0) */
} sl_step_plan;

/* Same return codes as sl_env_step for anything it rejects before launching
 * (actions, reward and done aside, which the plan does not need). */
int sl_env_step_plan(const sl_env_state *st, const sl_level_pool *pool, const sl_env_cfg *cfg,
                     const uint8_t *info_flags, sl_step_plan *out);

/* Complete the uint16 board of every env whose board lives in st->board_planes
 * (SL_POK_BOARD_PLANES without SL_POK_BOARD_FULL): needed before reading st->board directly after
 * steps that kept the board in planes.  No-op without board_planes. */
int sl_env_board_sync(sl_env_state *st, void *stream);

/* Reset the envs with mask[b] != 0 (mask NULL = all) from `pool`. */
int sl_env_reset(sl_env_state *st, const sl_level_pool *pool, const uint8_t *mask,
                 const sl_env_cfg *cfg, void *stream);

/*
 * Observations centred on each agent.
 *   obs_mode SL_OBS_PACKED: out uint16 [B,vh,vw]; SL_OBS_CHANNELS: uint16
 *   [B,vh,vw,nch] with channel k = bit channels[k]; SL_OBS_CHANNELS_U8: uint8;
 *   SL_OBS_CHANNELS_F32 / _BF16: the same bits as 0.0 / 1.0 floats.
 *   channels: host int array [nch] (<= 16) -- copied into kernel arguments.
 */
int sl_env_obs(const sl_env_state *st, int vh, int vw, int remove_white_goals,
               int obs_mode, const int32_t *channels, int nch, void *out,
               void *stream);

/* ------------------------------------------------- game-level pieces -- */
/*
 * The SafeLifeGame methods sl_env_step fuses, one at a time, for callers that drive
 * the game directly (/root/reference/safelife/safelife_game.py).  A state struct
 * whose pointers are offset by i0 envs (B = n) addresses envs [i0, i0 + n).
 *
 * sl_env_action       execute_action / move_agent / relative_loc
 *                     (safelife_game.py:294-393) for actions 0..8 of
 *                     safelife_env.py:61-71: the board cells, agent, orientation
 *                     and game_over in place.  act: dev int64 [4*B]: act[b] = the
 *                     action's reward (points_on_level_exit), act[B+b], [2B+b],
 *                     [3B+b] = its change to points / perf score / side effects.
 *                     The exit check reads score / possible (sl_env_rescore).
 * sl_env_advance      SafeLifeGame.advance_board (safelife_game.py:657-660): per env
 *                     num_steps += 1, board then goals advanced.  RNG from cfg
 *                     (rng_mode, seed, step, env0, draws / n_draws / stream_pos:
 *                     replay consumes env after env, board then goals, exactly as
 *                     two speedups.advance_board calls per env do), cfg->scratch
 *                     as for sl_env_step; the other cfg fields are not read.
 * sl_env_rescore      current_points (safelife_game.py:590-599) -> points (dev
 *                     int32 [B] or NULL) and performance_ratio's score terms
 *                     (:601-631) -> st->score, st->possible, for the current board.
 * sl_env_exit_colors  mode 0: update_exit_colors (safelife_game.py:528-537) from
 *                     st->score / possible / baseline / min_performance;
 *                     mode 1: exit cells set back to their start-board values.
 */
int sl_env_action(sl_env_state *st, const int32_t *actions, int can_toggle_powers,
                  int can_toggle_colors, int64_t *act, void *stream);
int sl_env_advance(sl_env_state *st, const sl_env_cfg *cfg, void *stream);
int sl_env_rescore(sl_env_state *st, int32_t *points, void *stream);
int sl_env_exit_colors(sl_env_state *st, int mode, void *stream);

/* ------------------------------------------------------- PPO caller -- */

/*
 * actions[b] = np.random.choice(A, p=probs[b]) (numpy's legacy RandomState.choice:
 * p taken as float64, cdf = cumsum(p) / cdf[-1], index = #{k : cdf[k] <= u}).
 *   probs       dev float32 (probs_f64 = 0) or float64 [B, ld], first A used
 *   rng_mode    SL_RNG_STREAM: u = uniforms[b] (dev double [B], e.g. the global
 *               numpy stream); SL_RNG_PHILOX: u = philox(seed; 0, env0 + b, step, 2)
 *   atol        numpy's tolerance on |sum(p) - 1| (sqrt(eps) of float64, or of
 *               the probabilities' dtype when larger)
 *   err         dev uint8 [B] or NULL: bit0 some p < 0, bit1 |kahan_sum(p) - 1|
 *               > atol -- the ValueErrors numpy raises; the caller raises them
 */
int sl_sample_actions(const void *probs, int probs_f64, int64_t B, int A, int64_t ld,
                      int rng_mode, const double *uniforms, uint64_t seed, uint32_t env0,
                      uint32_t step, double atol, int32_t *actions, uint8_t *err,
                      void *stream);

/*
 * Discounted returns and GAE advantages over a rollout of T steps x N envs with G
 * discount factors, in the reference's dtypes and evaluation order:
 *   rewards      dev double [T, N]   (clipped to +-reward_clip when > 0)
 *   end_episode  dev uint8 [T, N]
 *   values       dev float [T+1, N, G]
 *   gamma, lmda  dev float [G]       (lmda = the reference's lmda * gamma, float32)
 *   returns, advantages  dev double [T, N, G]
 */
int sl_gae(const double *rewards, const uint8_t *end_episode, const float *values,
           const float *gamma, const float *lmda, int G, int T, int64_t N,
           double reward_clip, double *returns, double *advantages, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SAFELIFE_HIP_H */
