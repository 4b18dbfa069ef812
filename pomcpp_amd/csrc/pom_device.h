/*
 * pom_device.h — what a kernel of this library is made of, for every unit that defines one: the runtime, the C-ABI's constants and
 * the device-side parts.  It defines no __global__ function, so a unit that includes it emits nothing but its own kernels:
 *   pom_tile.h         the LDS tile: its rows, LdsEnv, the record's loads and stores, restart_column(s) / column_to_record,
 *                      lane_from_tile, pom_boardgen_wave, pom_xcd_tile_order
 *   pom_step_body.h    the tick (PomStepper), pom_policy_body.h SimpleAgent for one agent, pom_boardgen_body.h the board generator
 *   pom_policy_wave.h  SimpleAgent for a wavefront: PolicyStore, the cooperative searches, pom_policy_wave
 *   pom_observe.h      the observation export of a tile in LDS: ObserveParams .. pom_observe_tile
 *   pom_chain_visit.h  the chained launches' hand-off, device side: pom_chain_enter / pom_chain_leave
 * The core unit's kernels: pom_kernels.h.
 */
#ifndef POM_DEVICE_H_
#define POM_DEVICE_H_

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "pom_batch.h"
#include "pom_boardgen_body.h"
#include "pom_packed.h"
#include "pom_policy_body.h"
#include "pom_step_body.h"
#include "pom_tile.h"
#include "pom_policy_wave.h"
#include "pom_observe.h"
#include "pom_chain_visit.h"

/* occupancy target of the quad kernel: 4 wavefronts per SIMD = 16 per CU = every one of 65,536 envs' wavefronts resident at
 * once.  The kernel needs 120-128 VGPRs; the target keeps the compiler from drifting past 128 (which would drop a whole
 * round's worth of wavefronts to a second round) — at the price of a spill or two if it ever has to.  History: an early
 * 157-VGPR version capped at 128 spilled 60 B/lane and ran 12 % slower than uncapped (profiles/r01_quad.txt); since the tile
 * mirrors the whole record the kernel fits. */
#ifndef POM_QUAD_WAVES
#define POM_QUAD_WAVES 4
#endif
/* wavefronts per workgroup.  Every wavefront works on a tile of its own in its own slice of the workgroup's LDS and never
 * synchronises with the others; more than one per workgroup only means fewer workgroups for the dispatcher to place. */
#ifndef POM_WPB
#define POM_WPB 1
#endif

/* The step kernels' parameters (pom_step_kernel, pom_kernels.h).  They stand here because the handle keeps copies of them (pom_host.h
 * PomChain), so every unit that knows the handle knows them. */
struct StepParams {
    uint32_t* state;
    const uint32_t* snap;
    const int32_t* moves; /* device int32[n][4], or nullptr: synthetic stream */
    int64_t* wave_counters;
    int64_t n, n_pad, env_offset;
    uint64_t seed;
    uint32_t tick0;            /* the launch's first tick is tick0 + *tick_base */
    const uint32_t* tick_base; /* a device word: 0 for a launch of its own, the chunk's first tick for a node of a replayed graph (pom_issue.h) */
    int32_t dist, ticks, mode, auto_reset, max_steps;
    int64_t block0, block_end; /* this launch covers tiles block0 .. block_end - 1 (sub-batch of a split step) */
    uint32_t* terminal;  /* auto_reset == POM_RESET_AT_END: the last finished episode's final record per env, array of structs */
    uint32_t* agent_mem; /* POLICY instantiation: SimpleAgent memory, [2][4 * n_pad] */
    uint32_t* episode;   /* games started so far per env (fresh boards: keys the next board) */
    uint64_t board_seed;
    int32_t fresh;       /* a restarting env gets the next board of pom_boardgen.h instead of its snapshot */
    /* CHAIN instantiation (pom_chain.h): launches of one queue that do NOT wait for each other — a tile's tick waits for the
     * same tile's previous tick instead.  Per tile one 64-bit word: bits 63..36 visits begun (tickets), 35..32 1 + the XCD
     * that stored the tile last (0: none yet), 27..0 visits stored.  The j-th visitor of a tile plays tick tick0 + (j - chain_seq0)
     * once the word says j visits are stored; which launch a visitor belongs to does not matter. */
    unsigned long long* tile_seq;
    uint32_t* chain_err; /* a device word of POM_CHAIN_E_* flags, read back by the host after the next join (chain_settle) */
    uint32_t chain_seq0;
    uint32_t tape_len;         /* CHAIN with explicit moves: `moves` is a tape int32[tape_len][n][4], the visit at distance d from
                                  chain_seq0 plays tick d of it (0: `moves` is one tick's Move[4] array or nullptr) */
    uint32_t chain_rot; /* chained: the launch's workgroups take their XCD's tiles starting this many positions in (< tiles per XCD; launch_many_chain) */
    uint64_t chain_wait_limit; /* how long a wavefront waits for the visit before its own, in ticks of the 100 MHz wall clock */
    /* OBS instantiation (pom_batch_step_device_observe): the planes / attributes of the state the tick leaves behind, written by
     * the same launch while the tile is still in LDS (pom_batch.h pom_batch_observe for the layout) */
    void* obs_planes;
    int32_t* obs_agent_attrs;
    int32_t* obs_env_attrs;
    int32_t obs_dtype, obs_per_agent;
    /* VIEW instantiation (pom_batch_step_device_observe_view): the four agents' fogged views instead (pom_batch.h PomViewSpec) */
    int32_t* obs_viewer_attrs;
    int32_t obs_view_radius;
#if defined(POM_DIAG)
    long long* diag; /* POM_PH_N accumulators per wavefront, diagnostic build only */
#endif
#if defined(POM_TRUNC)
    int32_t trunc; /* the tick stops after this phase (POM_CUT in pom_step_body.h); environment POM_TRUNC_AT, default: all of it */
#endif
};

#endif /* POM_DEVICE_H_ */
