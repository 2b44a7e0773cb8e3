// sl_env_step.h -- sl_env_step in two halves (sl_env_step.hip): the plan of a step,
// decided once by a pure host function, and the one launch sequence that runs it
// through the hooks each kernel family exports.
#pragma once
#include "sl_obs.h"

namespace sl {

// Everything sl_env_step decides before its first launch (plan_step): the public
// sl_step_plan (include/safelife_hip.h) plus what only the library can use.
struct StepPlan : sl_step_plan {
    obs::ObsArgs oa;            // the step's views (obs != SL_PLAN_OBS_NONE)
    const sl_capture *cap;      // the capture, or NULL
};

// Validates as sl_env_step does (same codes, same precedence) and fills *out.  Host
// only: no HIP call, no device pointer dereferenced (pointers are tested for NULL and
// alignment).  out->empty: a state without envs, nothing else is filled in.
int plan_step(const sl_env_state &st, const sl_level_pool *pool, const sl_env_cfg &cfg,
              const uint8_t *info_flags, StepPlan *out);

// the operands of one sl_env_step call, bundled once for the hooks
struct StepCall {
    sl_env_state *st;
    StepArgs a;
    FastExtra fx;
    const int32_t *actions;
    int ctp, ctc;
    double *reward;
    uint8_t *done, *flags;
    int32_t *ep_len, *ep_rew;
    void *obs_out;              // sl_env_cfg.obs_out (fx.obs_out: only when the step kernel writes)
    hipStream_t s;
    StepPlan plan;
};

// What a kernel family contributes to the sequence (run_step, sl_env_step.hip); a
// family without a piece leaves its hook NULL.
struct StepHooks {
    int (*counts)(const StepCall &);    // replay: the actions, then each env's eligible counts
    int (*pre_step)(const StepCall &);  // launches between the offsets scan and ev_begin
    int (*step)(const StepCall &);      // the step kernel, between ev_begin and ev_end
    int (*resets)(const StepCall &);    // plan.resets beyond SL_PLAN_RESETS_IN_KERNEL
    bool counts_check_thr;              // `counts` checks the bit ring's threshold itself
                                        // (stream_offsets then launches no k_bits_thr_check)
};
const StepHooks &hooks_generic();   // sl_env.hip
const StepHooks &hooks_small();     // sl_bits_small.hip (both small families)
const StepHooks &hooks_mid();       // sl_bits_mid.hip
const StepHooks &hooks_64();        // sl_bits.hip
const StepHooks &hooks_128();       // sl_bits128.hip
const StepHooks &hooks_wide();      // sl_bits_wide.hip

// k_env_reset_scan over all envs: SL_PLAN_RESETS_SCAN (sl_env.hip)
int reset_scan(const StepCall &c);
// the SL_PLAN_KEEP_* class of a 64x64 plane state's board_zero / agent_planes (sl_bits.hip;
// derived_planes is a run-time flag of every class)
int planes64_keep(const sl_env_state &st);

// host pieces of sl_env.hip the plan and the sequence use
bool state_ok(const sl_env_state *st);
ResetArgs reset_args(const sl_env_cfg *cfg);
int obs_args(int vh, int vw, int remove_white, int mode, const int32_t *channels, int nch,
             obs::ObsArgs *a);
int launch_obs(const sl_env_state &st, const obs::ObsArgs &a, void *out, hipStream_t s);
// the views of the envs the 128x128 reset-list kernel reset this step (packed, or channel
// views of at most obs::kObsMaxCells cells into a 16-byte aligned array)
int launch_obs_reset_list(const sl_env_state &st, const obs::ObsArgs &a, void *out,
                          const int64_t *scratch, uint32_t step, hipStream_t s);
// complete the uint16 board of a state whose boards live in planes and mark them stale
int demote_planes(sl_env_state *st, hipStream_t s);
// replay draws from the device generator's ring (sl_env_cfg.mt) instead of cfg->draws
void draws_from_ring(StepArgs &a, const sl_mt19937 &mt);

}  // namespace sl
