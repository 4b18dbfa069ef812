/*
 * pom_rollout.h — pom_batch_rollout's kernel (include/pom_batch.h PomRolloutSpec): how does the game end?  R random playouts of every
 * env to a finished game or a horizon of K ticks, the batch untouched.
 *
 * It joins three things that exist: the forecast's several-tick loop on a tile that never leaves LDS (pom_forecast.h), the quad
 * path of pom_step_kernel that draws the pom_rng.h move stream in the kernel (lane m of the quad works out agent m's 16 bits), and
 * Environment::Step's bookkeeping (pom_env_epilogue, pom_step_body.h).  One wavefront per (tile of 16 envs, sample): load_tile16_x4,
 * lane_from_tile, then up to K times draw, PomStepper::step_packed, timeStep++, epilogue — an env that is done is not stepped
 * (environment.cpp:125-128), and the wavefront leaves the loop when a ballot shows all of its envs done.  Nothing of the batch is
 * written: no record, no counter, no ticket word, no restart.  The owner lane of every env writes one result word.
 *
 * LDS: the tick's LDS_ROWS rows and nothing more (no staging rows: the result is a register).
 *
 * Grid: one dimension, workgroup b = r * tiles8 + slot with tiles8 the tile count rounded up to a multiple of 8, so that
 * b % 8 == slot % 8 and all samples of a tile run on one XCD (pom_xcd_tile_order): the L2 that got the tile's record with the first
 * sample serves the others.  That is an argument, not a measurement, and nothing of the result depends on it.  Slots >= tiles exit.
 */
#ifndef POM_ROLLOUT_H_
#define POM_ROLLOUT_H_

#include "pom_device.h"
#include "pom_result_word.h" /* pom_rollout_word */

struct RolloutParams {
    const uint32_t* state;
    const int32_t* moves; /* device int32[n][4], tick 1 of every sample, or nullptr: tick 1 is drawn like the others */
    uint32_t* result;     /* uint32 [samples][n] */
    int64_t n, env_offset;
    uint64_t seed;
    int32_t horizon;      /* 1 .. POM_ROLLOUT_MAX_TICKS */
    int32_t dist, max_steps;
    uint32_t tiles, tiles8; /* tiles of 16 envs; the same rounded up to a multiple of 8: the grid is samples * tiles8 */
};

static_assert(POM_ROLLOUT_MAX_TICKS < (1 << 16), "the tick count has 16 bits of the result word");

__global__ __launch_bounds__(64, POM_QUAD_WAVES) void pom_rollout_kernel(RolloutParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[LDS_ROWS * 16];
    const int lane = threadIdx.x;
    const uint32_t sample = blockIdx.x / p.tiles8, slot = blockIdx.x - sample * p.tiles8;
    if (slot >= p.tiles) return; /* a workgroup of the padding */
    const int64_t tile_id = pom_xcd_tile_order(slot, p.tiles);
    /* the HBM layout is 16-env tiles whatever the handle's launch shape; the buffers hold n_pad columns, so a last, short tile is
     * loaded whole */
    load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    /* the tick: lane -> (env lane / 4, member lane % 4) as in pom_step_kernel<16, 4> */
    const int ec = lane >> 2, member = lane & 3;
    const int64_t e = tile_id * 16 + ec;
    const bool valid = e < p.n;
    const uint32_t env_key = (uint32_t)(p.env_offset + e); /* the env's number in the whole job: what its move draws are keyed by */
    const uint64_t seed_r = pom_splitmix64(p.seed + sample); /* uniform: scalar code */
    /* tick 1's moves do not depend on the record: fetch them while it is on its way (dead agents' entries included) */
    int first = POM_MOVE_IDLE;
    if (p.moves && valid) first = p.moves[e * 4 + member];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the DMA rows have landed (one wavefront per workgroup: no barrier) */
    uint32_t* t = tile + ec;
    PomLane L;
    int time_step = 0;
    uint32_t status = 0;
    lane_from_tile(L, time_step, status, t, 16);
    pom_lane_diag_off(L);
    LdsEnv<16, 4> acc(tile, ec, member);
    PomStepper<LdsEnv<16, 4>> stepper(acc, L);

    /* done: the record's own bit (never set on a RAW handle), later the epilogue's; the lanes of an env past the batch's end count
     * as done from the start */
    bool done = !valid || (status & POM_ST_DONE);
    uint32_t ub = 0; /* the flags the played ticks raise; the env's own (the record's) are not the rollout's */
    int length = 0;
    const int K = p.horizon;
    POM_NOUNROLL
    for (int tk = 1; tk <= K; tk++) {
        if (__ballot(!done) == 0) break; /* random play ends games fast: most wavefronts leave long before K */
        if (!done) { /* the quad's four lanes agree */
            int mine = first;
            if (tk > 1 || !p.moves) {
                const uint32_t r = pom_rng_draw_half(seed_r, env_key, (uint32_t)(tk - 1), member >> 1); /* lane m needs agent m's 16 bits only */
                mine = pom_rng_pick((r >> (16 * (member & 1))) & 0xFFFFu, p.dist);
            }
            const uint32_t mvp = stepper.pack_moves_quad(mine);
            L.ub = 0;
            stepper.step_packed(mvp);
            ub |= L.ub;
            /* Environment::Step's bookkeeping whatever the handle's mode (environment.cpp:148-168) */
            time_step++;
            status = pom_env_epilogue(L, time_step, p.max_steps, status & ~(uint32_t)POM_ST_RESTARTED);
            length = tk;
            done = (status & POM_ST_DONE) != 0;
        }
    }

    /* out: one dword per env from its owner lane, 16 consecutive dwords per wavefront; a last, short tile writes its envs only */
    if (valid && member == 0) p.result[(int64_t)sample * p.n + e] = pom_rollout_word(L, status, ub != 0, (uint32_t)length);
}

#endif /* POM_ROLLOUT_H_ */
