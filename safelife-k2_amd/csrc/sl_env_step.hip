// sl_env_step.hip -- sl_env_step: decide, then do.  Host code only; the kernels live
// with their families (sl_env.hip, sl_bits_small.hip, sl_bits_mid.hip, sl_bits.hip,
// sl_bits128.hip, sl_bits_wide.hip) and are reached through each family's StepHooks (sl_env_step.h).
//
//   plan_step   every decision of a step as a pure function of (state, pool, cfg,
//               info_flags): the kernel family, replay and its phase, plane mode and
//               whether boards in planes are demoted first, who writes the views
//               (SL_PLAN_OBS_*), who resets the finished envs (SL_PLAN_RESETS_*), the
//               capture, and the 64x64 instance (SL_PLAN_K64_*, SL_PLAN_KEEP_*).
//               sl_env_step_plan exposes it; nothing else computes these facts.
//   run_step    the one launch sequence, the same for every family:
//                 1 demote boards in planes           (plan.demote_first)
//                 2 mark the state's planes live      (plane mode, not phase 1)
//                 3 replay: counts (not in phase 2) -> stream_offsets -> phase 1 ends
//                 4 pre-step
//                 5 ev_begin   6 the step kernel   7 ev_end
//                 8 capture, the frame before the resets
//                 9 resets by plan.resets
//                10 views by plan.obs
//                11 capture, the frame after the resets
#include "sl_env_step.h"

using namespace sl;

namespace {

// Whether SL_KERNEL_AUTO takes the 33-to-64-row kernel where it exists.  Set by the A/B of
// DESIGN.md 6.3 (profiles/mid_boards_ab.json): at 33x40, 48x48 and 64x48 it is more
// than twice the per-cell kernel.
constexpr bool kAutoTakesMid = true;

// the step kernels' view mode (k_env_step_bits64's OBS)
int view_kind_of(int obs_mode) {
    switch (obs_mode) {
    case SL_OBS_PACKED: return 1;
    case SL_OBS_CHANNELS_U8: return 3;
    case SL_OBS_CHANNELS_F32: return 4;
    default: return 2;               // u16 and bf16 channels
    }
}

}  // namespace

extern "C" int sl_env_step_family(int H, int W, int kernel) {
    if (H < 1 || W < 1) return SL_EINVAL;
    // opt-in: the one request that answers SL_FAMILY_WIDE, and nothing else
    if (kernel == SL_KERNEL_WIDE) return wide_shape(H, W) ? SL_FAMILY_WIDE : SL_ETOOBIG;
    if (kernel != SL_KERNEL_AUTO && kernel != SL_KERNEL_GENERIC && kernel != SL_KERNEL_FAST)
        return SL_EINVAL;
    if (kernel != SL_KERNEL_GENERIC) {
        if (H == 64 && W == 64) return SL_FAMILY_BITS64;
        if (H == 128 && W == 128) return SL_FAMILY_BITS128;
        if (small_seg4_shape(H, W)) return SL_FAMILY_SMALL_SEG4;
        if (small_shape(H, W)) return SL_FAMILY_SMALL;
        if (mid_shape(H, W) && (kAutoTakesMid || kernel == SL_KERNEL_FAST)) return SL_FAMILY_MID;
    }
    return kernel == SL_KERNEL_FAST ? SL_ETOOBIG : SL_FAMILY_GENERIC;
}

int sl::plan_step(const sl_env_state &st, const sl_level_pool *pool, const sl_env_cfg &cfg,
                  const uint8_t *info_flags, StepPlan *out) {
    StepPlan p{};
    if (!state_ok(&st) || !cfg.scratch) return SL_EINVAL;
    if (cfg.bonus_period < 0 || cfg.bonus_period > SL_BONUS_PERIOD_MAX) return SL_EINVAL;
    if (cfg.bonus_period > 0 && (!cfg.bonus_table || cfg.bonus_len < 1)) return SL_EINVAL;
    if (cfg.auto_reset && (!pool || !info_flags || pool->K <= 0 || pool->H != st.H ||
                           pool->W != st.W))
        return SL_EINVAL;
    if (st.B == 0) {
        p.empty = 1;
        *out = p;
        return SL_OK;
    }
    if (cfg.rng_mode != SL_RNG_STREAM && cfg.rng_mode != SL_RNG_PHILOX) return SL_EINVAL;
    const bool replay = cfg.rng_mode == SL_RNG_STREAM;
    // (the device generator's ring stands in for cfg.draws: step_args)
    if (replay && (!cfg.stream_pos ||
                   (cfg.mt ? !cfg.mt->ring : (!cfg.draws && cfg.n_draws > 0))))
        return SL_EINVAL;
    if (cfg.stream_phase < 0 || cfg.stream_phase > 2 || (cfg.stream_phase && !replay) ||
        (cfg.stream_phase == 2 && !cfg.stream_base))
        return SL_EINVAL;
    p.replay = replay;
    p.stream_phase = cfg.stream_phase;
    // the kernel family is sl_env_step_family's answer (SL_KERNEL_BANDS and SL_KERNEL_MID
    // name side-effect rollout kernels, no step kernel: SL_EINVAL); the 128x128 kernel
    // needs the state's goals mirror as well
    p.family = sl_env_step_family(st.H, st.W, cfg.kernel);
    if (p.family < 0) return p.family;
    if (p.family == SL_FAMILY_BITS128 && !bits128_shape(st)) {
        if (cfg.kernel == SL_KERNEL_FAST) return SL_ETOOBIG;
        p.family = SL_FAMILY_GENERIC;
    }
    // (the wide kernel draws with Philox only: replay is open)
    if (p.family == SL_FAMILY_WIDE && replay) return SL_ETOOBIG;
    const bool fast = p.family == SL_FAMILY_BITS64, fast128 = p.family == SL_FAMILY_BITS128;
    // every one-wave kernel with the uint16 board in HBM, which resets its own finished envs
    const bool small = p.family == SL_FAMILY_MID || p.family == SL_FAMILY_SMALL ||
                       p.family == SL_FAMILY_SMALL_SEG4;
    p.cap = (cfg.capture && cfg.capture->n > 0) ? cfg.capture : nullptr;
    // (env and flags are needed; every other target may be NULL and is then not copied)
    if (p.cap && (!p.cap->env || !p.cap->flags || !info_flags || !cfg.auto_reset))
        return SL_EINVAL;
    p.capture = p.cap ? 1 : 0;
    if (cfg.obs_out) {
        const int rc = obs_args(cfg.obs_vh, cfg.obs_vw, cfg.obs_remove_white, cfg.obs_mode,
                                cfg.obs_channels, cfg.obs_nch, &p.oa);
        if (rc) return rc;
    }
    if (cfg.board_mode != SL_BOARD_AUTO && cfg.board_mode != SL_BOARD_UINT16) return SL_EINVAL;
    if (cfg.planes64_waves != 0 && cfg.planes64_waves != 5 && cfg.planes64_waves != 6 &&
        cfg.planes64_waves != SL_PLANES64_W6_UNSPLIT)
        return SL_EINVAL;
    if ((small || p.family == SL_FAMILY_WIDE) && st.B > 0x7FFFFFFF) return SL_EINVAL;

    // Views.  The 128x128 kernel writes packed views of at most kViewMaxRows128 rows from
    // the board planes (channel views: below); the 64x64 kernels write packed views, and channel views of up
    // to kFusedChanCells cells into a 16-byte aligned array (one wave writes its env's
    // 16-byte chunks from the view masks it builds in LDS); everything else is the
    // observation kernel's, after the resets.
    const bool planes128 = st.board_planes && st.planes_ok && st.H == 128 && st.W == 128;
    const bool planes64 = planes64_shape(st);
    // a board stays in planes over a step without capture whose draws the plane kernels
    // know (128x128 replay: with draw planes, the decided form; 64x64: Philox only)
    const bool planes_can = !p.cap && cfg.board_mode != SL_BOARD_UINT16;
    // ... and, asked to (SL_OBS_FUSE_CHAN128), channel views of at most
    // SL_FUSE_CHAN128_MAX_CELLS cells into a 16-byte aligned array: the limits of the wave
    // writer that gives the reset envs their views (launch_obs_reset_list)
    static_assert(SL_FUSE_CHAN128_MAX_CELLS <= obs::kObsMaxCells, "the reset envs' writer");
    const bool chan128 = (cfg.obs_fuse & SL_OBS_FUSE_CHAN128) && p.oa.mode != SL_OBS_PACKED &&
                         p.oa.vh * p.oa.vw <= SL_FUSE_CHAN128_MAX_CELLS &&
                         (((uintptr_t)cfg.obs_out) & 15) == 0;
    const bool fuse128 = fast128 && planes128 && planes_can && cfg.obs_out &&
                         (!replay || st.elig_planes) &&
                         (p.oa.mode == SL_OBS_PACKED || chan128) &&
                         p.oa.vh <= kViewMaxRows128 && p.oa.vw <= 128;
    const bool fuse64 =
        fast && cfg.obs_out &&
        ((p.oa.mode == SL_OBS_PACKED && p.oa.vh * p.oa.vw <= obs::kObsMaxCells) ||
         (p.oa.mode != SL_OBS_PACKED && p.oa.vh <= 64 && p.oa.vw <= 64 &&
          p.oa.vh * p.oa.vw + 2 <= obs::kFusedChanCells && (((uintptr_t)cfg.obs_out) & 15) == 0));
    p.obs = !cfg.obs_out ? SL_PLAN_OBS_NONE
            : fuse128    ? SL_PLAN_OBS_FUSED128
            : fuse64     ? SL_PLAN_OBS_FUSED64
                         : SL_PLAN_OBS_SEPARATE;
    const bool views_ok = p.obs != SL_PLAN_OBS_SEPARATE;    // none, or the step kernel's own
    if (fast128 && planes128)
        p.plane_mode = planes_can && views_ok && (!replay || st.elig_planes);
    else if (fast && planes64)
        p.plane_mode = planes_can && views_ok && !replay;
    p.demote_first = (planes128 || planes64) && !p.plane_mode;
    p.view_kind = (p.obs == SL_PLAN_OBS_FUSED64 || p.obs == SL_PLAN_OBS_FUSED128)
                      ? view_kind_of(p.oa.mode) : 0;

    // the 64x64 instance.  The <C3> instances fix the agent planes as well; gray goals
    // (all black or white) take the instances that skip their colours, without views the
    // six-wave one -- split from its epilogue and resets (k_env_planes64_s6 +
    // k_env_epilogue_reset64) when it resets from a pool and the hand-over records in
    // scratch are 16-byte aligned; planes64_waves 5 and -6 ask for the unsplit twins
    if (fast && !p.plane_mode) {
        p.kernel64 = SL_PLAN_K64_BITS64;
    } else if (fast) {
        p.keep = planes64_keep(st);
        // (the derived planes -- both or none -- make no class of their own: a C3 batch
        // without them runs the same instances compiled to store all sixteen words)
        const uint32_t laid = ~st.board_zero & ~st.agent_planes & 0xFFFFu;
        p.derived = (int32_t)(((st.derived_planes & 0x8100u) == 0x8100u ? 0x8100u : 0u) & laid);
        p.stored = (int32_t)(laid & ~(uint32_t)p.derived);
        const bool gray = p.keep == SL_PLAN_KEEP_C3 && st.goals_gray;
        if (p.view_kind >= 2) p.kernel64 = SL_PLAN_K64_CHAN;
        else if (!gray) p.kernel64 = SL_PLAN_K64_PLANES;
        else if (p.view_kind || cfg.planes64_waves == 5) p.kernel64 = SL_PLAN_K64_GRAY;
        else if (cfg.planes64_waves != SL_PLANES64_W6_UNSPLIT && cfg.auto_reset &&
                 (reinterpret_cast<uintptr_t>(cfg.scratch) & 15) == 0 &&
                 (cfg.bonus_period == 0 || cfg.bonus_len <= kHandDistMax))
            p.kernel64 = SL_PLAN_K64_S6;
        else p.kernel64 = SL_PLAN_K64_W6;
    }

    // Resets.  The small-board kernels reset finished envs inside the step; with a
    // capture those run in the follow-up scan so the pre-reset frame can be copied first.
    // The 64x64 / 128x128 kernels list the finished envs and a second kernel resets them
    // after that frame, so they keep the list (and its per-parity lengths, which only the
    // reset-list kernel clears) going through captured steps.  The wide kernel stands in
    // the generic family's sequence: the scan, with or without a capture.
    p.resets = !cfg.auto_reset                    ? SL_PLAN_RESETS_NONE
               : small                            ? (p.cap ? SL_PLAN_RESETS_SCAN : SL_PLAN_RESETS_IN_KERNEL)
               : p.kernel64 == SL_PLAN_K64_S6     ? SL_PLAN_RESETS_SPLIT_TAIL64
               : fast                             ? SL_PLAN_RESETS_LIST64
               : fast128                          ? SL_PLAN_RESETS_LIST128
                                                  : SL_PLAN_RESETS_SCAN;
    *out = p;
    return SL_OK;
}

extern "C" int sl_env_step_plan(const sl_env_state *st, const sl_level_pool *pool,
                                const sl_env_cfg *cfg, const uint8_t *info_flags,
                                sl_step_plan *out) {
    if (!st || !cfg || !out) return SL_EINVAL;
    StepPlan p;
    const int rc = plan_step(*st, pool, *cfg, info_flags, &p);
    if (!rc) *out = p;
    return rc;
}

namespace {

const StepHooks &hooks_of(int family) {
    switch (family) {
    case SL_FAMILY_BITS64: return hooks_64();
    case SL_FAMILY_BITS128: return hooks_128();
    case SL_FAMILY_MID: return hooks_mid();
    case SL_FAMILY_WIDE: return hooks_wide();
    case SL_FAMILY_GENERIC: return hooks_generic();
    default: return hooks_small();
    }
}

void step_args(const sl_env_cfg &cfg, StepArgs &a) {
    a.time_limit = cfg.time_limit;
    a.auto_reset = cfg.auto_reset;
    a.bonus_len = cfg.bonus_len;
    a.bonus_period = cfg.bonus_period;
    a.penalty_coef = cfg.penalty_coef;
    a.bonus_table = cfg.bonus_table;
    a.seed = cfg.seed;
    a.step = cfg.step;
    a.env0 = cfg.env0;
    a.draws = cfg.draws;
    a.n_draws = cfg.n_draws;
    if (cfg.rng_mode == SL_RNG_STREAM && cfg.mt) draws_from_ring(a, *cfg.mt);
}

// the bit-sliced kernels' extra arguments, from cfg and the plan
void fast_extra(const sl_env_cfg &cfg, const sl_level_pool *pool, const StepPlan &p,
                FastExtra &fx) {
    fx.pool = pool ? *pool : sl_level_pool{};
    fx.ra = reset_args(&cfg);
    fx.fuse_reset = p.resets != SL_PLAN_RESETS_NONE && p.resets != SL_PLAN_RESETS_SCAN;
    fx.scratch = cfg.scratch;
    fx.ev_begin = cfg.ev_begin;
    fx.ev_end = cfg.ev_end;
    fx.capture = p.cap;
    fx.stream = p.replay;
    fx.stream_pos = cfg.stream_pos;
    fx.stream_phase = cfg.stream_phase;
    fx.stream_base = cfg.stream_base;
    fx.mt = p.replay ? cfg.mt : nullptr;
    if (fx.mt && fx.mt->bit_ring) fx.bits_thr = fx.mt->bits_thr;
    fx.plane_mode = p.plane_mode;
    fx.obs_out = p.view_kind ? (uint16_t *)cfg.obs_out : nullptr;
    fx.obs_vh = cfg.obs_vh;
    fx.obs_vw = cfg.obs_vw;
    fx.obs_rw = cfg.obs_remove_white;
    fx.obs_mode = SL_OBS_PACKED;
    fx.obs_nch = 0;
    fx.obs_chpack = 0;
    fx.obs_one = 1u;
    if (cfg.obs_out) {
        fx.obs_mode = p.oa.mode;
        fx.obs_nch = p.oa.nch;
        for (int k = 0; k < p.oa.nch; k++) fx.obs_chpack |= (uint64_t)p.oa.ch[k] << (4 * k);
        fx.obs_one = p.oa.mode == SL_OBS_CHANNELS_F32 ? 0x3F800000u
                     : p.oa.mode == SL_OBS_CHANNELS_BF16 ? 0x3F80u : 1u;
    }
}

int run_step(const StepCall &c, const StepHooks &h) {
    const StepPlan &p = c.plan;
    sl_env_state *st = c.st;
    int rc;
    if (p.demote_first && (rc = demote_planes(st, c.s))) return rc;
    // (a plane-mode step below leaves boards in planes)
    if (p.plane_mode && p.stream_phase != 1) st->planes_live = 1;
    if (p.replay) {
        if (p.stream_phase != 2 && (rc = h.counts(c))) return rc;
        rc = stream_offsets(*st, c.fx, h.counts_check_thr, c.s);
        if (rc || p.stream_phase == 1) return rc;
    }
    if (h.pre_step && (rc = h.pre_step(c))) return rc;
    if (c.fx.ev_begin) (void)hipEventRecord((hipEvent_t)c.fx.ev_begin, c.s);
    if ((rc = h.step(c))) return rc;
    if (c.fx.ev_end) (void)hipEventRecord((hipEvent_t)c.fx.ev_end, c.s);
    if (p.cap && (rc = launch_capture(*st, *p.cap, c.flags, 0, c.s))) return rc;
    if (p.resets > SL_PLAN_RESETS_IN_KERNEL && (rc = h.resets(c))) return rc;
    // FUSED64: the reset-list kernel wrote the views of the envs it reset.  FUSED128: the
    // step kernel wrote every view from the planes; the envs the reset-list kernel
    // reset get theirs from the new episode's uint16 board
    if (p.obs == SL_PLAN_OBS_FUSED128 && p.resets == SL_PLAN_RESETS_LIST128)
        rc = launch_obs_reset_list(*st, p.oa, c.fx.obs_out, c.fx.scratch, c.a.step, c.s);
    else if (p.obs == SL_PLAN_OBS_SEPARATE)
        rc = launch_obs(*st, p.oa, c.obs_out, c.s);
    if (rc || !p.cap) return rc;
    return launch_capture(*st, *p.cap, c.flags, 1, c.s);
}

}  // namespace

extern "C" int sl_env_step(sl_env_state *st, const sl_level_pool *pool, const int32_t *actions,
                           const sl_env_cfg *cfg, double *reward, uint8_t *done,
                           uint8_t *info_flags, int32_t *ep_len, int32_t *ep_reward,
                           void *stream) {
    if (!st || !cfg || !actions || !reward || !done) return SL_EINVAL;
    StepCall c;
    const int rc = plan_step(*st, pool, *cfg, info_flags, &c.plan);
    if (rc || c.plan.empty) return rc;
    c.st = st;
    step_args(*cfg, c.a);
    fast_extra(*cfg, pool, c.plan, c.fx);
    c.actions = actions;
    c.ctp = cfg->can_toggle_powers;
    c.ctc = cfg->can_toggle_colors;
    c.reward = reward;
    c.done = done;
    c.flags = info_flags;
    c.ep_len = ep_len;
    c.ep_rew = ep_reward;
    c.obs_out = cfg->obs_out;
    c.s = (hipStream_t)stream;
    return run_step(c, hooks_of(c.plan.family));
}
