/*
 * pom_expand.h — pom_batch_expand's kernel (include/pom_batch.h PomExpandSpec): for a device-side list, env first + j becomes the
 * successor of env src[j] under moves[j] — the copy of pom_batch_copy_envs (flags 0) and one tick, in ONE launch — with a result
 * word per child (pom_batch_rollout's format) and, optionally, the observation of the tiles touched.
 *
 * One wavefront per DESTINATION tile, a quad per env, as the one-tick step kernels:
 *   1  the list's entries, then the destination tile into LDS as it stands (load_tile16_x4);
 *   2  the source columns of the tile's jobs over it — the gather of PomGather16 (pom_rollout_policy.h): lane l moves the items
 *      of column l & 15, has ONE source address, and all its loads are in flight before the first wait.  Only columns with a job that
 *      copies (src != destination) are loaded and stored.  Where the 16 sources are the 16 envs of one tile in order (pom_sources_one_tile)
 *      the source tile is loaded as a tile;
 *   3  the children's agent memory and episode counter — the source's: loaded with the gather, stored as soon as it has arrived (no
 *      index is both read and written, see below, so their place in the order does not matter; here nothing is carried through the tick);
 *   4  the tick for the job quads only (PomStepper<LdsEnv<16, 4>>, pom_tile_env_tick), as the handle's mode says; no
 *      restart is ever played;
 *   5  the register rows back into the columns that were ticked;
 *   6  the whole tile out (store_tile16_x4);
 *   7  the result words from the owner lanes;
 *   8  POM_RESET_AT_END: the children's terminal records — the source's — child after child by the whole wavefront;
 *   9  OBS: pom_observe_tile over the staging rows behind the record;
 *  10  the wavefront's counters, returnless atomics as in pom_step_kernel.
 *
 * Aliasing (the argument of pom_copy.h's one-pass shortcut).  A job is refused when its source lies inside [first, first + count) and
 * is not its own destination, so a source column is never a column some job writes: every source is either outside the range, or an
 * identity entry — which only its own quad reads, out of its own tile.  Every byte this kernel stores into a column that is not a
 * played destination is the byte it loaded from there, so a wavefront that reads a source column out of a tile another wavefront is
 * rewriting sees the same bytes before, during and after that store.  The side arrays follow: entries are read at sources and
 * written at copied destinations, and no index is both.
 *
 * LDS: LDS_ROWS rows (7,424 B); OBS: the staging area of the fused export lies over the tick's scratch rows (the tick is over when
 * the observation begins), max(LDS_ROWS, POM_REC_DWORDS + the staging rows).
 */
#ifndef POM_EXPAND_H_
#define POM_EXPAND_H_

#include "pom_rollout_policy.h"

struct ExpandParams {
    uint32_t* state;
    const int64_t* src;        /* device int64[count] */
    const int32_t* moves;      /* device int32[count][4], a row per job */
    uint32_t* result;          /* device uint32[count], or nullptr */
    int64_t first, count, n, n_pad;
    int64_t tile0;             /* first destination tile; the grid covers tiles tile0 .. tile0 + gridDim.x - 1 */
    uint32_t* agent_mem;       /* [2][4 * n_pad] or nullptr (no SimpleAgent memory allocated) */
    uint32_t* episode;         /* [n_pad] */
    uint32_t* terminal;        /* [n_pad][80] or nullptr (not POM_RESET_AT_END) */
    int64_t* wave_counters;
    int32_t mode, max_steps;
    ObserveParams obs;         /* OBS: pom_batch_observe's own arguments (observe_params), its outputs sized for the whole batch */
};

/* is entry s of the list a job for destination d: a source of the batch that is not another slot of the range */
__device__ __forceinline__ bool pom_expand_job(const ExpandParams& p, int64_t s, int64_t d)
{
    return s >= 0 && s < p.n && !(s >= p.first && s < p.first + p.count && s != d);
}

template <bool OBS>
__global__ __launch_bounds__(64, 4) void pom_expand_kernel(ExpandParams p)
{
    constexpr int OBS_ROWS = (obs_stage_vecs(OBS_PASS_ENVS_FUSED) * 16 + 63) / 64;
    constexpr int ROWS = OBS && POM_REC_DWORDS + OBS_ROWS > LDS_ROWS ? POM_REC_DWORDS + OBS_ROWS : LDS_ROWS;
    __shared__ __attribute__((aligned(16))) uint32_t tile[ROWS * 16];
    const int lane = threadIdx.x;
    const int64_t tile_id = p.tile0 + pom_xcd_tile_order(blockIdx.x, gridDim.x);
    /* the list's entries of this tile, twice: the one this lane's quad plays, and the one whose column this lane helps to move — asked
     * for BEFORE the tile, so that waiting for them (in-order vmcnt) does not wait for the tile */
    const int ec = lane >> 2, member = lane & 3, col = lane & 15;
    const int64_t d = tile_id * 16 + ec, dc = tile_id * 16 + col;
    const int64_t j = d - p.first, jc = dc - p.first;
    const bool in_range = j >= 0 && j < p.count;
    const int64_t s = in_range ? p.src[j] : -1, sc = jc >= 0 && jc < p.count ? p.src[jc] : -1;
    load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    const bool job = pom_expand_job(p, s, d), copy = job && s != d;
    const bool copyc = pom_expand_job(p, sc, dc) && sc != dc;
    /* neither the moves nor the side arrays depend on the record: fetch them while it is on its way */
    int mine = POM_MOVE_IDLE;
    if (job) mine = p.moves[j * 4 + member]; /* (dead agents' entries included) */
    uint32_t m0 = 0, m1 = 0, ep = 0;
    if (copy) {
        if (p.agent_mem) {
            m0 = p.agent_mem[s * 4 + member];
            m1 = p.agent_mem[4 * p.n_pad + s * 4 + member];
        }
        if (member == 0) ep = p.episode[s];
    }
    /* the 16 sources are the 16 envs of one other tile, in order: loaded as a tile below.  Else the gather's load half (PomGather16,
     * pom_rollout_policy.h) here and its store half behind the wait: every load (these, the move, the side arrays) is issued before the
     * ONE wait that also covers the tile's DMA rows, and only then may a column be laid over the tile.  A column without a copying job
     * is neither loaded nor stored */
    const int64_t t0 = pom_sources_one_tile(sc, copyc, lane);
    const bool gather = copyc && t0 < 0;
    PomGather16 g;
    g.load(p.state, sc, gather, lane);
    /* the destination tile's DMA rows have landed (one wavefront per workgroup: no barrier) — before any column is laid over them */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("" : "+v"(mine)); /* (the move is looked at from here on: nothing of the tick's packing waits for it earlier) */
    if (t0 >= 0) {
        load_tile16_x4(p.state + t0 * POM_TILE_DWORDS, tile, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (gather) g.store(tile, lane);
    /* the children's agent memory and episode counter: their source's */
    if (copy) {
        if (p.agent_mem) {
            p.agent_mem[d * 4 + member] = m0;
            p.agent_mem[4 * p.n_pad + d * 4 + member] = m1;
        }
        if (member == 0) p.episode[d] = ep;
    }
    asm volatile("" ::: "memory"); /* other lanes wrote this lane's column: no read of it may be scheduled earlier */

    PomLane L;
    int time_step = 0;
    uint32_t status = 0;
    uint32_t* const t = tile + ec;
    lane_from_tile(L, time_step, status, t, 16);
    pom_lane_diag_off(L);
    const bool env_mode = p.mode == POM_MODE_ENV;
    /* POM_MODE_ENV: a finished source gives an unticked copy (environment.cpp:125-128) */
    const bool active = job && !(env_mode && (status & POM_ST_DONE));
    bool newly_done = false, new_ub = false;
    if (active) { /* the quad's four lanes agree */
        LdsEnv<16, 4> acc(tile, ec, member);
        PomStepper<LdsEnv<16, 4>> stepper(acc, L);
        const uint32_t rec_ub = L.ub; /* the record's flags: this tick's are added to them */
        status = pom_tile_env_tick(stepper, L, mine, tile, ec, member, env_mode, p.max_steps, status & ~(uint32_t)POM_ST_RESTARTED);
        new_ub = L.ub != 0;
        L.ub |= rec_ub;
        newly_done = env_mode && (status & POM_ST_DONE) != 0;
        /* the register-resident rows back into the column: the played destinations only, every other column leaves as it came */
        if (member == 0) {
#pragma unroll
            for (int k = 0; k < 8; k++) t[(POM_REC_AGENTS + k) * 16] = pom_lane_agent_word(L, status, k, (k & 1) ? t[(POM_REC_AGENTS + k) * 16] : 0u);
        }
    }
    asm volatile("" ::: "memory");
    {
        int lane_late = lane; /* (a lane id the compiler cannot see through: the store addresses are worked out here, not carried through the tick) */
        asm volatile("" : "+v"(lane_late));
        store_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane_late);
    }
    /* the result word, pom_batch_rollout's: one dword per entry of the list from its owner lane; POM_RO_NONE without a job */
    if (p.result && in_range && member == 0) p.result[j] = job ? pom_rollout_word(L, status, new_ub, active ? 1u : 0u) : (uint32_t)POM_RO_NONE;
    /* POM_RESET_AT_END: the children's terminal records are their sources', one child after the other by the whole wavefront */
    if (p.terminal) {
        uint64_t todo = __ballot(copy && member == 0);
        while (todo) {
            const int ec_u = (__builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1)) >> 2;
            todo &= todo - 1;
            const int64_t d_u = tile_id * 16 + ec_u, s_u = p.src[d_u - p.first];
            const uint32_t* from = p.terminal + s_u * POM_REC_DWORDS;
            uint32_t* to = p.terminal + d_u * POM_REC_DWORDS;
            to[lane] = from[lane];
            if (lane + 64 < POM_REC_DWORDS) to[lane + 64] = from[lane + 64];
        }
    }
    if (OBS) {
        /* the observation of what lies in the tile now, while the record's stores are on their way (they have been read out of LDS
         * into registers; the staging area lies behind the record rows) */
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pom_observe_tile<OBS_PASS_ENVS_FUSED, false>(p.obs, tile, reinterpret_cast<uint4*>(tile + POM_REC_DWORDS * 16), tile_id, lane);
    }
    /* expansion ticks are steps of the batch; no restart is ever played */
    const long long c_steps = __popcll(__ballot(active && member == 0)), c_episodes = __popcll(__ballot(newly_done && member == 0)),
                    c_ub = __popcll(__ballot(new_ub && member == 0));
    if (lane == 0) {
        unsigned long long* wc = reinterpret_cast<unsigned long long*>(p.wave_counters + tile_id * POM_CNT_N);
        if (c_steps) __hip_atomic_fetch_add(&wc[POM_CNT_STEPS], (unsigned long long)c_steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c_episodes) __hip_atomic_fetch_add(&wc[POM_CNT_EPISODES], (unsigned long long)c_episodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c_ub) __hip_atomic_fetch_add(&wc[POM_CNT_UB_TICKS], (unsigned long long)c_ub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

#endif /* POM_EXPAND_H_ */
