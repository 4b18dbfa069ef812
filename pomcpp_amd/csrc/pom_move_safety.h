/*
 * pom_move_safety.h — pom_batch_move_safety's kernel (include/pom_batch.h PomMoveSafetySpec): which of an agent's six moves does it
 * survive, and from which is there somewhere to walk to?  Every candidate of every asked agent of every env in ONE launch, the batch
 * untouched.
 *
 * It joins three things that exist: the forecast's several-tick loop on a tile that never leaves LDS (pom_forecast.h: tick 1 with
 * given moves, then IDLE), the rollout's grid of (tile, variant) wavefronts with its early exit by ballot (pom_rollout.h), and the
 * policy's flood-fill step on 121-bit cell sets spread over a quad, one 32-cell word per lane (pom_quad_neighbours,
 * pom_policy_body.h; PomQuadLanes, pom_policy_wave.h).  One wavefront per (tile of 16 envs, variant), variant = (agent of the mask,
 * candidate move): load_tile16_x4, lane_from_tile, then up to K times PomStepper::step_packed and, per env, the quad's four lanes
 * build the set of free cells from the env's board bytes in LDS and let the set of cells a walker can have reached grow by one step.
 * Nothing of the batch is written: no record, no counter, no ticket word, no restart.  The owner lane of every env stores one byte
 * per output.
 *
 * LDS: the tick's LDS_ROWS rows and nothing more (no staging rows: both answers are registers).
 *
 * Grid: pom_rollout.h's — one dimension, workgroup b = v * tiles8 + slot with tiles8 the tile count rounded up to a multiple of 8, so
 * that b % 8 == slot % 8 and all variants of a tile run on one XCD (pom_xcd_tile_order).  Slots >= tiles exit.
 */
#ifndef POM_MOVE_SAFETY_H_
#define POM_MOVE_SAFETY_H_

#include "pom_policy_body.h"

/* ---- the two set functions, for the device and for the host (tests/emul/pom_move_safety_emul.cpp) ---- */

/* Word m (cells 32m .. 32m+31) of Free: the cells whose code is passage or a power-up (IS_WALKABLE, bboard.hpp:81-84) — the
 * classification and the gathering of pom_policy_prepare_fill's "walkable" set (pom_policy_body.h), without its agent set.
 * P: uint32_t cells4(int k), the codes of cells 4k .. 4k+3, a byte each; k up to 31 must be readable (what lies past cell 120 is
 * masked here). */
template <class P>
POM_HD uint32_t pom_free_word(const P& p, int m)
{
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        uint32_t w0, g0, w1, g1;
        pom_cells_walk_agent(p.cells4(8 * m + i), w0, g0);
        pom_cells_walk_agent(p.cells4(8 * m + i + 1), w1, g1);
        w |= pom_gather_flags(w1, pom_gather_flags(w0, 0u, 0), 1) << (4 * i);
    }
    return m == 3 ? w & 0x01FFFFFFu : w; /* 121 = 96 + 25 */
}

/* R_t from R_{t-1}: the set and its four neighbours on the board (the policy's dilation, pom_quad_neighbours), cut to the free cells.
 * Q: what "one word per lane" is (pom_policy_body.h). */
template <class Q>
POM_HD typename Q::W pom_escape_grow(const Q& q, typename Q::W reach, typename Q::W free_cells)
{
    return (reach | pom_quad_neighbours(q, reach)) & free_cells;
}

#if defined(__HIPCC__) /* ---- the kernel ---- */

#include "pom_device.h"
#include "pom_policy_wave.h"

struct MoveSafetyParams {
    const uint32_t* state;
    const int32_t* moves; /* device int32[n][4], the others' moves of tick 1, or nullptr: IDLE */
    int8_t* death_tick;   /* nullable: int8 [n][4][6] */
    int8_t* escape_tick;  /* nullable: int8 [n][4][6]; one of the two is given */
    int64_t n;
    int32_t horizon;      /* 1 .. POM_FORECAST_MAX_TICKS */
    int32_t agent_mask;   /* 1 .. 15 */
    uint32_t tiles, tiles8; /* tiles of 16 envs; the same rounded up to a multiple of 8: the grid is variants * tiles8 */
};

/* the board of the quad's env as pom_free_word reads it: cell c at byte c * 16 of the env's column (LdsEnv::b, pom_tile.h) */
struct MoveSafetyCells {
    const uint8_t* b;
    __device__ uint32_t cells4(int k) const
    {
        const uint8_t* q = b + 64 * k;
        return (uint32_t)q[0] | ((uint32_t)q[16] << 8) | ((uint32_t)q[32] << 16) | ((uint32_t)q[48] << 24);
    }
};

static_assert(POM_FORECAST_MAX_TICKS < 128, "a tick fits the int8 outputs");

__global__ __launch_bounds__(64, POM_QUAD_WAVES) void pom_move_safety_kernel(MoveSafetyParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[LDS_ROWS * 16];
    const int lane = threadIdx.x;
    const uint32_t variant = blockIdx.x / p.tiles8, slot = blockIdx.x - variant * p.tiles8;
    if (slot >= p.tiles) return; /* a workgroup of the padding */
    const int64_t tile_id = pom_xcd_tile_order(slot, p.tiles);
    /* the HBM layout is 16-env tiles whatever the handle's launch shape; the buffers hold n_pad columns, so a last, short tile is
     * loaded whole */
    load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    /* the variant: candidate `cand` of the (variant / 6)-th agent of the mask — uniform: scalar code */
    const int nth = (int)(variant / 6u), cand = (int)(variant - 6u * (uint32_t)nth);
    int agent = 0;
    for (int a = 0, seen = 0; a < 4; a++) {
        if ((p.agent_mask >> a) & 1) {
            if (seen == nth) agent = a;
            seen++;
        }
    }
    /* the tick: lane -> (env lane / 4, member lane % 4) as in pom_step_kernel<16, 4> */
    const int ec = lane >> 2, member = lane & 3;
    const int64_t e = tile_id * 16 + ec;
    const bool valid = e < p.n; /* the lanes of an env past the batch's end step nothing and write nothing */
    /* tick 1's moves do not depend on the record: fetch them while it is on its way.  Lane m reads agent m's (dead agents' entries
     * included, as pom_batch_step_device reads them); the candidate takes the place of its agent's */
    int mine = POM_MOVE_IDLE;
    if (p.moves && valid) mine = p.moves[e * 4 + member];
    mine = member == agent ? cand : mine;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the DMA rows have landed (one wavefront per workgroup: no barrier) */
    uint32_t* t = tile + ec;
    PomLane L;
    int time_step = 0;
    uint32_t status = 0;
    lane_from_tile(L, time_step, status, t, 16);
    pom_lane_diag_off(L);
    LdsEnv<16, 4> acc(tile, ec, member);
    PomStepper<LdsEnv<16, 4>> stepper(acc, L);
    const PomQuadLanes Q(member);
    const MoveSafetyCells cells{acc.b};
    const bool want_escape = p.escape_tick != nullptr;

    /* both answers, the same in the quad's four lanes: -1 dead before the first tick, 0 not (yet) dead / not (yet) without a way out */
    int death = ag_dead(sel4(agent, L.a0)) ? -1 : 0, escape = death;
    uint32_t reach = 0u; /* R, this lane's word of it */
    /* the moves, a nibble per agent, exchanged within the quad; ticks 2 .. K are all-IDLE: the packed word of four IDLE moves is 0 */
    static_assert(POM_MOVE_IDLE == 0, "the packed all-IDLE word");
    uint32_t mvp = stepper.pack_moves_quad(mine);
    const int K = p.horizon;
    POM_NOUNROLL
    for (int tk = 1; tk <= K; tk++) {
        /* an env is played on while its answer is open.  R = {} is absorbing and means the agent is dead (its own cell is free while
         * it lives), so with escape_tick that is "R not empty yet", without it "not dead yet".  A wavefront whose agent was dead at
         * S_0 in all its envs plays no tick */
        const bool open = valid && (want_escape ? escape : death) == 0; /* the quad's four lanes agree */
        if (__ballot(open) == 0) break;
        if (open) {
            /* bare bboard::Step as in POM_MODE_RAW: no timeStep++, no done / max_steps logic, a finished env is played like any other */
            stepper.step_packed(mvp);
            mvp = 0u;
            const int a0 = sel4(agent, L.a0);
            const bool alive = !ag_dead(a0);
            death = ((int)(death == 0) & (int)!alive) ? tk : death;
            if (want_escape) {
                obs_lds_order(); /* the lanes' board writes are in the tile: no read below may be scheduled earlier */
                const uint32_t own = alive ? Q.bit(ag_y(a0) * POM_N + ag_x(a0)) : 0u;
                /* R_1 = where the agent stands after its move; from then on one step of growth on this tick's free cells */
                reach = tk == 1 ? own : pom_escape_grow(Q, reach, pom_free_word(cells, member) | own);
                if (!Q.any(reach)) escape = tk;
                obs_lds_order(); /* ... and the next tick's accesses stay behind the reads */
            }
        }
    }

    /* out: a byte per env and output from the env's owner lane, [e][agent][cand]: 16 bytes per wavefront, stride 24 */
    if (valid && member == 0) {
        const int64_t at = e * 24 + agent * 6 + cand;
        if (p.death_tick) p.death_tick[at] = (int8_t)death;
        if (want_escape) p.escape_tick[at] = (int8_t)escape;
    }
}

#endif /* __HIPCC__ */

#endif /* POM_MOVE_SAFETY_H_ */
