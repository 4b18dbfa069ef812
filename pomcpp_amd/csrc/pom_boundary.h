/*
 * pom_boundary.h — the kernels at the boundary between the caller's States and the device's records: upload, download, the
 * one-State call, status and results, snapshot.  What a field's bits are and what upload refuses is pom_packed.h's business;
 * nothing here restates it.  Part of pom_kernels.h (included from there, after the tick and its helpers).
 */
#ifndef POM_BOUNDARY_H_
#define POM_BOUNDARY_H_

#include "pom_device.h"

__global__ void pom_pack_kernel(const int32_t* __restrict__ aos, int64_t first, int64_t count, uint32_t* state, uint32_t* snap,
                                int64_t np, int* first_bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int32_t* st = aos + i * (POM_STATE_BYTES / 4);
    const int lane = (int)((first + i) & 15);
    uint32_t* col = state + pom_rec_col(first + i);
    const int64_t rs = POM_TILE_ENVS; /* row stride of a column */
    int bad = pom_pack_state(st, col, rs, lane);
    for (int k = 0; k < POM_MAX_BOMBS; k++) bad |= pom_pack_live_bomb_bad(st, k);
    if (bad) {
        atomicMin(first_bad, (int)(i > INT_MAX - 1 ? INT_MAX - 1 : i));
        for (int c = 0; c < 4 * POM_REC_BOARD_DWORDS; c++) pom_rec_set_cell(col, rs, c, 0, lane); /* inert blank board ... */
        for (int d = POM_REC_TIMESTEP; d < POM_REC_DWORDS; d++) col[d * rs] = 0;
        pom_rec_set_meta(col, rs, 0u, (uint32_t)POM_ST_DONE << 8); /* ... that is never stepped in ENV mode */
    }
    /* the snapshot is array-of-structs (restart_column): a dense record, the column as it stands (a refused env's stays finished) */
    pom_col_to_rec(snap + (first + i) * POM_REC_DWORDS, col - lane, lane, false);
}

__global__ void pom_unpack_kernel(const uint32_t* __restrict__ state, int64_t first, int64_t count, int64_t np, int32_t* aos)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    pom_unpack_state(state + pom_rec_col(first + i), POM_TILE_ENVS, aos + i * (POM_STATE_BYTES / 4), (int)((first + i) & 15));
}

/* ---------------------------------------------------------------------------------------------
 * ONE State, one tick, one launch: the literal `bboard::Step(State*, Move*)` (POM_MODE_RAW) and `Environment::Step`'s tick +
 * bookkeeping (POM_MODE_ENV; environment.cpp:123-169) for callers that hold a single host State (pom_step, pom_env_step).
 * `io` is pinned host memory the device reads and writes directly — no staging copies, no second and third launch:
 *   dwords   0..250  in:  the State (include/pom_state.h)        252..255  in:  Move[4]
 *   dwords 256..506  out: the State after the tick               508..511  out: done, winner, draw, ubflags
 *   dword  512       out: 1 if the State is outside the representable game states (nothing else is written then)
 *   dword  513       out: `seq`, written LAST (system-scope release): the host polls it
 *   dwords 514..516  in:  mode, max_steps, seq of this request
 * One wavefront: all 64 lanes fetch and pack (pom_pack_lane: a few record items per lane), the quad of lanes 0..3 plays the
 * tick with the same PomStepper as pom_step_kernel, all lanes unpack (pom_unpack_lane) and write back.
 * ------------------------------------------------------------------------------------------- */
struct StepOneParams {
    int32_t* io_base;  /* POM_ONE_SLOTS pages of POM_ONE_PAGE_DWORDS dwords each */
    uint64_t slots;    /* bit s: slot s holds a request; workgroup b serves the b-th set bit */
};
/* a slot's page: the layout above, then the request's own parameters — one launch serves whatever requests are pending, each
 * with its own mode (pom_step / pom_env_step), bound and sequence number */
enum { POM_ONE_MOVES = 252, POM_ONE_OUT = 256, POM_ONE_STATUS = 508, POM_ONE_BAD = 512, POM_ONE_SEQ = 513, POM_ONE_MODE = 514,
       POM_ONE_MAX_STEPS = 515, POM_ONE_REQ = 516, POM_ONE_PAGE_DWORDS = 1024, POM_ONE_SLOTS = 64 };

__global__ __launch_bounds__(64) void pom_step_one_kernel(StepOneParams q)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[LDS_ROWS * 16];
    __shared__ int32_t aos[256];
    const int lane = threadIdx.x;
    /* which slot: the blockIdx-th set bit of the request mask (wave-uniform) */
    uint64_t slot_bits = q.slots;
    for (unsigned b = 0; b < blockIdx.x; b++) slot_bits &= slot_bits - 1;
    struct { int32_t* io; int32_t mode, max_steps; uint32_t seq; } p;
    p.io = q.io_base + (int64_t)(__ffsll((unsigned long long)slot_bits) - 1) * POM_ONE_PAGE_DWORDS;
    p.mode = p.io[POM_ONE_MODE];
    p.max_steps = p.io[POM_ONE_MAX_STEPS];
    p.seq = (uint32_t)p.io[POM_ONE_REQ];
#pragma unroll
    for (int k = 0; k < 4; k++) aos[lane + 64 * k] = p.io[lane + 64 * k]; /* State + Move[4]: four 256-B reads of host memory */
    for (int k = lane; k < LDS_ROWS * 16; k += 64) tile[k] = 0u;           /* columns 1..15 stay blank and are never stepped */
    __syncthreads();
    if (__ballot(pom_pack_lane(aos, tile, lane) != 0)) { /* the caller's State is left alone; pom_step reports POM_E_UNREPRESENTABLE */
        if (lane == 0) {
            p.io[POM_ONE_BAD] = 1;
            __threadfence_system();
            __hip_atomic_store(reinterpret_cast<uint32_t*>(p.io) + POM_ONE_SEQ, p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }
    __syncthreads();

    /* the tick: lane -> (env lane / 4, member lane % 4) as in pom_step_kernel<16, 4>; env 0 is the only one there is */
    const int ec = lane >> 2, member = lane & 3;
    uint32_t* t = tile + ec;
    PomLane L;
    int time_step = 0;
    uint32_t status = 0;
    lane_from_tile(L, time_step, status, t, 16);
    pom_lane_diag_off(L);
    LdsEnv<16, 4> acc(tile, ec, member);
    PomStepper<LdsEnv<16, 4>> stepper(acc, L);
    const bool env_mode = p.mode == POM_MODE_ENV;
    if (ec == 0) {
        const uint32_t mvp = stepper.pack_moves_quad(aos[POM_ONE_MOVES + member]);
        L.ub = 0;
        stepper.step_packed(mvp);
        if (env_mode) {
            time_step++;
            status = pom_env_epilogue(L, time_step, p.max_steps, status);
        }
        if (member == 0) { /* the register-resident rows */
            t[POM_REC_TIMESTEP * 16] = (uint32_t)time_step;
#pragma unroll
            for (int k = 0; k < 8; k++) t[(POM_REC_AGENTS + k) * 16] = pom_lane_agent_word(L, status, k, (k & 1) ? t[(POM_REC_AGENTS + k) * 16] : 0u);
        }
    }
    __syncthreads();

    /* unpack column 0 straight into host memory */
    pom_unpack_lane(tile, p.io + POM_ONE_OUT, lane);
    if (lane == POM_LANE_SCALARS) {
        const PomStatus s = pom_status_decode(pom_rec_meta2(tile, 16));
        p.io[POM_ONE_STATUS + 0] = s.done;
        p.io[POM_ONE_STATUS + 1] = s.winner;
        p.io[POM_ONE_STATUS + 2] = s.draw;
        p.io[POM_ONE_STATUS + 3] = s.ubflags;
        p.io[POM_ONE_BAD] = 0;
    }
    __threadfence_system(); /* every lane's stores have left before ... */
    __syncthreads();
    if (lane == 0) /* ... the word the host is polling changes */
        __hip_atomic_store(reinterpret_cast<uint32_t*>(p.io) + POM_ONE_SEQ, p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

/* out: 6 arrays of `count` int32: done, winner, draw, alive, timeStep, ubflags */
__global__ void pom_status_kernel(const uint32_t* __restrict__ state, int64_t first, int64_t count, int64_t np, int32_t* out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t* col = state + pom_rec_col(first + i);
    const PomStatus s = pom_status_decode(pom_rec_meta2(col, POM_TILE_ENVS));
    out[0 * count + i] = s.done;
    out[1 * count + i] = s.winner;
    out[2 * count + i] = s.draw;
    out[3 * count + i] = pom_sext8(pom_rec_meta(col, POM_TILE_ENVS));
    out[4 * count + i] = (int32_t)col[POM_REC_TIMESTEP * POM_TILE_ENVS];
    out[5 * count + i] = s.ubflags;
}

/* POM_RESET_AT_END: out = 5 arrays of `count` int32: finished (the state's "restarted" mark), then winner, draw, length, alive
 * of the terminal record (array of structs; all-zero = no episode finished yet) */
__global__ void pom_results_kernel(const uint32_t* __restrict__ state, const uint32_t* __restrict__ terminal, int64_t first, int64_t count,
                                   int64_t np, int32_t* out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint32_t now = (pom_rec_meta2(state + pom_rec_col(first + i), POM_TILE_ENVS) >> 8) & 0xFF;
    const uint32_t* rec = terminal + (first + i) * POM_REC_DWORDS;
    const PomStatus s = pom_status_decode(pom_rec_meta2(rec, 1));
    out[0 * count + i] = (now & POM_ST_RESTARTED) ? 1 : 0;
    out[1 * count + i] = s.winner;
    out[2 * count + i] = s.draw;
    out[3 * count + i] = (int32_t)rec[POM_REC_TIMESTEP];
    out[4 * count + i] = s.done ? pom_sext8(pom_rec_meta(rec, 1)) : 0;
}

__global__ void pom_unpack_aos_kernel(const uint32_t* __restrict__ recs, int64_t first, int64_t count, int32_t* aos)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    pom_unpack_state(recs + (first + i) * POM_REC_DWORDS, 1, aos + i * (POM_STATE_BYTES / 4));
}

/* every column into its snapshot record (array of structs, restart_column); a snapshot starts an episode: status and flags clear */
__global__ void pom_snapshot_kernel(const uint32_t* __restrict__ state, uint32_t* snap, int64_t np)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= np) return;
    pom_col_to_rec(snap + e * POM_REC_DWORDS, state + (e >> 4) * POM_TILE_DWORDS, (int)(e & 15), true);
}

#endif /* POM_BOUNDARY_H_ */
