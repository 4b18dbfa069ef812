/*
 * pom_step_mixed.h — pom_batch_step_mixed's kernel (include/pom_batch.h PomMixedStepSpec): ONE tick of a range of whole tiles in which
 * the agents of simple_mask play agents::SimpleAgent and the others take the caller's moves, with the observation of the state the
 * tick leaves written by the same launch, plain or as fogged views.
 *
 * It joins three things that pom_step_kernel has in separate instantiations (and says so: its static_assert on OBS and POLICY): the
 * fused policy of pom_step_kernel<POLICY> (pom_policy_prepare_*, pom_policy_wave, the agents' memory), the explicit moves of the
 * one-tick quad kernels (a dword per lane, fetched while the record is on its way) and the fused export of the OBS / VIEW ones
 * (pom_observe_tile over staging rows behind the record) — with the mask of pom_rollout_policy.h: actor = the env plays this tick, the
 * agent is in the mask, and it is alive.  One wavefront per tile of 16 envs, lane m of an env's quad is agent m.
 *   1  the record (load_tile16_x4), and while it is on its way the lane's two memory dwords and, for an agent outside the mask, its
 *      move moves[tile * 64 + lane];
 *   2  POM_RESET_AT_START: finished envs restart (restart_column, or pom_boardgen_wave with fresh boards), all four agents' memory
 *      becomes zero;
 *   3  the policy, skipped as a whole when the mask is 0 (wave-uniform): every lane goes into pom_policy_wave, the actors come out with
 *      a move and their memory moved on; the memory leaves for global memory here, it is not carried through the tick;
 *   4  the move select, one v_cndmask: mask bit ? the policy's move (IDLE for a dead agent) : the caller's;
 *   5  the tick, its bookkeeping and, with POM_RESET_AT_END, the finishing tick's restart — as pom_step_kernel, line for line;
 *   6  the record out (store_tile16_x4), then OBS: pom_observe_tile, then the wavefront's counters.
 * The agents' memory may be absent (nullptr) when the mask is 0: nothing of it is then read or written.
 *
 * EVENTS (pom_batch_step_events, pom_step_events.h): the same kernel, line for line, which also says what the tick did.  Behind 2 every
 * lane keeps its agent's two words of S0 (and, when the wood count is asked for, the wood bits of its share of the boards); behind the
 * tick's epilogue and BEFORE 5's restart at the end it reads the same of S1 and stores one event word per lane, the owner lanes the
 * env's outcome word and wood count.  The body is shared (pom_step_mixed_body.inc, included by both); pom_batch_step_mixed's kernels are what
 * they were before EVENTS existed, instruction for instruction.
 *
 * LDS: the policy's 44 overlay rows (danger map 32, cell sets 12) and the export's staging rows (38) lie over the SAME rows behind the
 * record, which are also the tick's scratch rows: the policy is over before the tick begins and the tick is over before the export
 * begins, so the largest of the three sizes the tile — max(LDS_ROWS, POM_REC_DWORDS + 44) rows, what the fused policy kernel has.
 */
#ifndef POM_STEP_MIXED_H_
#define POM_STEP_MIXED_H_

#include "pom_device.h"
#include "pom_step_events.h"

struct MixedStepParams {
    uint32_t* state;
    const uint32_t* snap;
    const int32_t* moves;  /* device int32[n][4], indexed by env; read for the agents outside simple_mask only (nullptr if there are none) */
    uint32_t* agent_mem;   /* [2][4 * n_pad]; nullptr only with simple_mask == 0 on a handle that has none */
    uint32_t* episode;
    uint32_t* terminal;
    int64_t* wave_counters;
    int64_t n, n_pad, env_offset;
    int64_t block0;        /* the launch covers tiles block0 .. block0 + gridDim.x - 1 */
    uint64_t seed, board_seed;
    uint32_t tick;         /* keys the SimpleAgent draw: the spec's, not the handle's */
    int32_t simple_mask, mode, auto_reset, max_steps;
    /* OBS / VIEW: as StepParams */
    void* obs_planes;
    int32_t* obs_agent_attrs;
    int32_t* obs_env_attrs;
    int32_t* obs_viewer_attrs;
    int32_t obs_dtype, obs_per_agent, obs_view_radius;
    /* the COMPACT kernels only (PomCompactViewSpec): ObserveParams' view_compact.  It lies in what was the struct's tail padding: no
     * kernel argument moves, StepEventsOut behind it included */
    int32_t obs_view_compact;
};
static_assert(sizeof(MixedStepParams) == 176, "obs_view_compact fills the tail padding");

#define POM_STEP_MIXED_COMPACT 0
template <bool FRESH, bool ATEND, bool OBS, bool VIEW>
__global__ __launch_bounds__(64, 4) void pom_step_mixed_kernel(MixedStepParams p)
{
#define POM_STEP_MIXED_EVENTS 0
#include "pom_step_mixed_body.inc"
#undef POM_STEP_MIXED_EVENTS
}

/* pom_batch_step_events' kernel: the same, with the events (pom_step_events.h) */
template <bool FRESH, bool ATEND, bool OBS, bool VIEW>
__global__ __launch_bounds__(64, 4) void pom_step_events_kernel(MixedStepParams p, StepEventsOut eo)
{
#define POM_STEP_MIXED_EVENTS 1
#include "pom_step_mixed_body.inc"
#undef POM_STEP_MIXED_EVENTS
}
#undef POM_STEP_MIXED_COMPACT

/* COMPACT: the two kernels once more with the compact views (pom_batch.h PomCompactViewSpec) as their observation — the body's one
 * other way out, pom_observe_tile_compact.  Kernels of their own, by name: the text of the sixteen above is what it was */
#define POM_STEP_MIXED_COMPACT 1
template <bool FRESH, bool ATEND>
__global__ __launch_bounds__(64, 4) void pom_step_mixed_compact_kernel(MixedStepParams p)
{
    constexpr bool OBS = true, VIEW = true;
#define POM_STEP_MIXED_EVENTS 0
#include "pom_step_mixed_body.inc"
#undef POM_STEP_MIXED_EVENTS
}
template <bool FRESH, bool ATEND>
__global__ __launch_bounds__(64, 4) void pom_step_events_compact_kernel(MixedStepParams p, StepEventsOut eo)
{
    constexpr bool OBS = true, VIEW = true;
#define POM_STEP_MIXED_EVENTS 1
#include "pom_step_mixed_body.inc"
#undef POM_STEP_MIXED_EVENTS
}
#undef POM_STEP_MIXED_COMPACT

#endif /* POM_STEP_MIXED_H_ */
