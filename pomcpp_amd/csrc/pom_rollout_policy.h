/*
 * pom_rollout_policy.h — pom_batch_rollout_policy's kernel (include/pom_batch.h PomRolloutPolicySpec): R playouts of every env in
 * which the agents of simple_mask play agents::SimpleAgent, the others the pom_rng.h move stream, and tick 1 may be fixed per agent;
 * the batch untouched.
 *
 * It joins pom_rollout_kernel (pom_rollout.h: the K-tick loop on a tile that never leaves LDS, the ballot exit, Environment::Step's
 * bookkeeping, the result word) with the policy of pom_step_kernel<POLICY> (pom_policy_body.h, pom_policy_wave.h: pom_policy_prepare_*, pom_policy_wave, the
 * danger map and the cell sets laid over the tick's scratch rows).  One wavefront per (tile of 16 envs, sample); lane m of an env's
 * quad is agent m.  The agents' memory is two dwords per lane, loaded once and never stored to global memory: every sample plays on
 * with its own copy.
 *
 * The wavefront's floods run cooperatively (pom_coop_forward / pom_coop_backward deal the jobs to all 16 quads), so EVERY lane enters
 * pom_policy_wave on every tick the wavefront plays — with actor = false for finished envs, lanes past the batch's end, dead agents
 * and agents outside simple_mask.  Only the wave-uniform ballot exit skips it.
 *
 * POLICY = false (simple_mask == 0): an instantiation without any of the policy — pom_rollout_kernel with a per-agent first tick.
 *
 * LDS: max(LDS_ROWS, POM_REC_DWORDS + 44) rows: the danger map (32 rows of bytes) and the cell sets (12 rows) lie where the tick keeps
 * its bomb destinations and explosion frames — the policy of a tick is over before its tick begins.  Behind them 12 rows, three
 * dwords per lane: the agent's memory and its move of tick 1 wait there through the tick (in registers they cost 12 spilled VGPRs
 * at 4 wavefronts per SIMD).  8,704 B per wavefront: the 16 wavefronts of a CU fit.  128 VGPRs, no scratch.
 *
 * Grid: as pom_rollout_kernel — workgroup b = r * tiles8 + slot, all samples of a tile on one XCD; slots >= tiles exit.
 *
 * JOBS = true (pom_batch_rollout_jobs, PomRolloutJobsSpec): the same playouts for a device-side list of jobs instead of the batch's
 * envs in order.  One wavefront per (group of 16 consecutive jobs, sample); job 16 g + ec belongs to quad ec.  Only the front and the
 * indices differ:
 *   the load   the LDS tile is put together from 16 different columns of the state buffer: column src & 15 of tile src >> 4 becomes
 *              column ec (PomGather16 below: one source address per lane, every lane issues all its loads, for all 16 columns at once,
 *              before anything waits; pom_copy_gather_kernel moves its columns one after another and waits for each).  The bytes go
 *              through registers (an LDS-DMA of one byte per lane is not something this project has measured), and so do the dwords:
 *              a lane without a job stores zeros with the same instructions.  Where the 16 sources are the 16 envs of one tile in
 *              order (pom_sources_one_tile) the tile is loaded as the other kernels load it, load_tile16_x4 — every group of a move
 *              table (BatchEnvironment.move_table) whose batch is a multiple of 16 envs is of that kind.
 *   no job     an entry with src outside [0, n) and the slots past the list's end: a blank record (zeros), its lanes done from the
 *              start; they still enter pom_policy_wave with actor = false.  The owner lane writes the word 0 for an entry of the list.
 *   indices    the agents' memory and the draws' key are the SOURCE env's (env_offset + src: jobs of one source play under common
 *              random numbers), the moves of tick 1 and the result word the job's.
 * The two instances without JOBS were, instruction for instruction, what they had been before the parameter existed
 * (profiles/rollout_jobs_kernel_resources.txt).
 */
#ifndef POM_ROLLOUT_POLICY_H_
#define POM_ROLLOUT_POLICY_H_

#include "pom_rollout.h"

struct RolloutPolicyParams {
    const uint32_t* state;
    const int32_t* moves;      /* device int32[n][4]: tick 1 of the agents in first_mask; nullptr when first_mask == 0 */
    const uint32_t* agent_mem; /* [2][4 * n_pad], or nullptr: fresh agents (no memory allocated, or POM_ROLLOUT_FRESH_AGENTS) */
    uint32_t* result;          /* uint32 [samples][n] */
    int64_t n, n_pad, env_offset;
    uint64_t seed;
    int32_t horizon;           /* 1 .. POM_ROLLOUT_MAX_TICKS */
    int32_t dist, max_steps;
    int32_t simple_mask, first_mask;
    uint32_t tiles, tiles8;    /* tiles of 16 envs; the same rounded up to a multiple of 8: the grid is samples * tiles8 */
};

/* JOBS: `tiles` / `tiles8` count groups of 16 jobs, `moves` is int32[jobs][4] and `result` uint32 [samples][jobs] */
struct RolloutJobsParams : RolloutPolicyParams {
    const int64_t* src;        /* device int64[jobs]: job j plays env src[j]; outside [0, n): no job */
    int64_t jobs;
};

enum { RP_ROWS = POM_REC_DWORDS + 44 > LDS_ROWS ? POM_REC_DWORDS + 44 : LDS_ROWS, RP_PARK_ROWS = 3 * 4 };

/* The column gather of the list-driven kernels: column `col` = lane & 15 of the LDS tile becomes a copy of env s's column of the state
 * buffer.  Lane l moves the items of column l & 15 — board bytes k = (l >> 4) + 4 t, t = 0 .. 30, and dwords 31 + (l >> 4) + 4 t,
 * t = 0 .. 12 — so a lane has ONE source address and all its loads are immediates behind it.  Two halves, because a caller may have
 * other loads to issue and one wait to share between them: load() issues all of a lane's loads and waits for none (a lane whose `ok`
 * is false loads nothing and holds a blank record, zeros), store() lays what has arrived over the tile. */
struct PomGather16 {
    static constexpr int NB = POM_COL_BOARD_ITEMS / 4, ND = (POM_REC_DWORDS - POM_REC_TIMESTEP + 3) / 4; /* 31 byte loads, 13 dword loads */
    static_assert(POM_COL_BOARD_ITEMS % 4 == 0 && POM_TILE_ENVS == 16, "64 lanes take 4 items of each of the 16 columns at a time");
    uint32_t b[NB], d[ND];

    /* the last round of dwords is short (row 79 only): the lanes that have an item in it; sub = lane >> 4, which of a round's four items */
    static __device__ __forceinline__ bool last(int sub) { return sub < (POM_REC_DWORDS - POM_REC_TIMESTEP) - 4 * (ND - 1); }

    __device__ __forceinline__ void load(const uint32_t* state, int64_t s, bool ok, int lane)
    {
        const int sub = lane >> 4;
        const uint32_t* const src_tile = state + (ok ? s >> 4 : 0) * POM_TILE_DWORDS;
        const int src_col = ok ? (int)(s & 15) : 0;
        const uint8_t* const gb = reinterpret_cast<const uint8_t*>(src_tile) + sub * 16 + src_col; /* byte k * 16 + src_col, k = sub + 4 t */
        const uint32_t* const gd = src_tile + (POM_REC_TIMESTEP + sub) * 16 + src_col;             /* dword (31 + sub + 4 t) * 16 + src_col */
#pragma unroll
        for (int t = 0; t < NB; t++) b[t] = 0;
#pragma unroll
        for (int t = 0; t < ND; t++) d[t] = 0;
        if (ok) {
#pragma unroll
            for (int t = 0; t < ND - 1; t++) d[t] = gd[t * 64];
            if (last(sub)) d[ND - 1] = gd[(ND - 1) * 64];
#pragma unroll
            for (int t = 0; t < NB; t++) b[t] = gb[t * 64];
        }
    }

    __device__ __forceinline__ void store(uint32_t* tile, int lane) const
    {
        uint8_t* const lb = reinterpret_cast<uint8_t*>(tile) + lane; /* byte k * 16 + col, k = sub + 4 t */
        uint32_t* const ld = tile + POM_REC_TIMESTEP * 16 + lane;     /* dword (31 + sub + 4 t) * 16 + col */
#pragma unroll
        for (int t = 0; t < ND - 1; t++) ld[t * 64] = d[t];
        if (last(lane >> 4)) ld[(ND - 1) * 64] = d[ND - 1];
#pragma unroll
        for (int t = 0; t < NB; t++) lb[t * 64] = (uint8_t)b[t];
    }
};

/* The front of the JOBS kernel: the whole tile gathered, a blank record where `ok` is false.  All of a lane's loads are issued before
 * the first of them is waited for. */
__device__ __forceinline__ void pom_gather_tile16(const uint32_t* state, int64_t s, bool ok, uint32_t* tile, int lane)
{
    PomGather16 g;
    g.load(state, s, ok, lane);
    g.store(tile, lane);
}

/* Are the 16 sources of a group (lane l holds the one of column l & 15, `ok`: it is one) the 16 envs of one tile, in order?  The tile's
 * number, or -1.  Wave-uniform: a ballot.  Such a group is loaded as a tile (load_tile16_x4) instead of gathered. */
__device__ __forceinline__ int64_t pom_sources_one_tile(int64_t s, bool ok, int lane)
{
    const int64_t t0 = __builtin_amdgcn_readfirstlane((int)((ok ? s : 0) >> 4));
    return __ballot(ok && s == t0 * 16 + (lane & 15)) == ~0ull ? t0 : -1;
}

/* One tick of Environment::Step for a quad whose record lies in an LDS tile, timeStep included: the moves packed, the tick, and, with
 * `env`, the bookkeeping whatever the handle's mode (environment.cpp:148-168).  timeStep is looked at here only: read back from the
 * tile (env column `ec`) and counted there by the owner lane (`member` 0) instead of living in a register through the tick.  L.ub is left
 * holding the flags this tick raised.  Returns the status byte after the tick. */
template <class Stepper>
__device__ __forceinline__ uint32_t pom_tile_env_tick(Stepper& stepper, PomLane& L, int mine, uint32_t* tile, int ec, int member, bool env,
                                                      int32_t max_steps, uint32_t status)
{
    const uint32_t mvp = stepper.pack_moves_quad(mine);
    L.ub = 0;
    stepper.step_packed(mvp);
    if (!env) return status;
    uint32_t* const ts = tile + ec + POM_REC_TIMESTEP * 16; /* (worked out behind the tick, not carried through it) */
    const int time_step = (int)*ts + 1;
    if (member == 0) *ts = (uint32_t)time_step;
    return pom_env_epilogue(L, time_step, max_steps, status);
}

template <bool JOBS>
struct RolloutParamsOf { typedef RolloutPolicyParams type; };
template <>
struct RolloutParamsOf<true> { typedef RolloutJobsParams type; };

template <bool POLICY, bool JOBS = false>
__global__ __launch_bounds__(64, 4) void pom_rollout_policy_kernel(typename RolloutParamsOf<JOBS>::type p)
{
    /* POLICY: behind the tile three dwords per lane that are parked through the tick: the agent's memory and its move of tick 1 */
    __shared__ __attribute__((aligned(16))) uint32_t tile[(POLICY ? RP_ROWS + RP_PARK_ROWS : LDS_ROWS) * 16];
    const int lane = threadIdx.x;
    const uint32_t sample = blockIdx.x / p.tiles8, slot = blockIdx.x - sample * p.tiles8;
    if (slot >= p.tiles) return; /* a workgroup of the padding */
    const int64_t tile_id = pom_xcd_tile_order(slot, p.tiles); /* JOBS: the group of 16 jobs */
    /* lane -> (env lane / 4, agent lane % 4) */
    const int ec = lane >> 2, member = lane & 3;
    int64_t e;        /* the env this lane plays: its record, its agents' memory, the key of its draws (JOBS: 0 where there is no job) */
    int64_t slot_out; /* where its moves of tick 1 and its result word are: the env, or the job */
    bool valid;       /* there is a game to play */
    uint32_t env_key = 0; /* JOBS: the env's number in the whole job, what its draws are keyed by (per lane; else key0 + ec below) */
    if constexpr (JOBS) {
        /* the list's entries of this group, twice: the one this lane's quad plays, and the one whose column this lane helps to move */
        const int64_t j0 = tile_id * 16, jc = j0 + (lane & 15);
        slot_out = j0 + ec;
        const int64_t s = slot_out < p.jobs ? p.src[slot_out] : -1, sc = jc < p.jobs ? p.src[jc] : -1;
        valid = s >= 0 && s < p.n;
        e = valid ? s : 0;
        const bool okc = sc >= 0 && sc < p.n;
        const int64_t t0 = pom_sources_one_tile(sc, okc, lane);
        if (t0 >= 0) load_tile16_x4(p.state + t0 * POM_TILE_DWORDS, tile, lane);
        else pom_gather_tile16(p.state, sc, okc, tile, lane);
        env_key = (uint32_t)(p.env_offset + e);
    } else {
        load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
        e = tile_id * 16 + ec;
        slot_out = e;
        valid = e < p.n;
    }
    const uint32_t key0 = (uint32_t)(p.env_offset + tile_id * 16); /* + ec: the env's number in the whole job, what its draws are keyed by */
    const uint64_t seed_r = pom_splitmix64(p.seed + sample); /* uniform: scalar code */
    /* neither tick 1's moves nor the agents' memory depend on the record: fetch them while it is on its way */
    int first = POM_MOVE_IDLE;
    if (((p.first_mask >> member) & 1) && valid) first = p.moves[slot_out * 4 + member]; /* (dead agents' entries included) */
    if (POLICY) {
        /* this lane's agent's memory: this sample's own copy, never stored to global memory (the buffers hold n_pad columns) */
        uint32_t m0 = 0, m1 = 0;
        if (p.agent_mem) {
            if constexpr (JOBS) {
                if (valid) {
                    m0 = p.agent_mem[e * 4 + member];
                    m1 = p.agent_mem[4 * p.n_pad + e * 4 + member];
                }
            } else {
                m0 = p.agent_mem[tile_id * 64 + lane];
                m1 = p.agent_mem[4 * p.n_pad + tile_id * 64 + lane];
            }
        }
        uint32_t* park = tile + RP_ROWS * 16 + lane; /* (rows no DMA touches) */
        park[0] = m0;
        park[64] = m1;
        park[128] = (uint32_t)first;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the DMA rows have landed (one wavefront per workgroup: no barrier) */
    PomLane L;
    /* the playout's state beside the tile and L, one register: the status byte, bit 8 = a played tick raised a flag, bits 16.. = ticks played */
    uint32_t run = 0;
    {
        int time_step = 0; /* lives in the tile: the owner lane counts it there */
        lane_from_tile(L, time_step, run, tile + ec, 16);
        run &= 0xFFu & ~(uint32_t)POM_ST_RESTARTED;
        if (!valid) run |= POM_ST_DONE; /* the lanes of an env past the batch's end count as done from the start; they write nothing */
    }
    pom_lane_diag_off(L);

    const int K = p.horizon;
    POM_NOUNROLL
    for (int tk = 1; tk <= K; tk++) {
        if (__ballot(!(run & POM_ST_DONE)) == 0) break; /* wave-uniform: the one exit that may skip the policy */
        /* a lane id and a view of the tile that the compiler cannot see through, made anew for the policy and for the tick: what is
         * derived from them is worked out where it is used, not before the loop and carried through every tick (the fresh-view trick of
         * pom_step_kernel<POLICY>) */
        int ln = lane;
        uint32_t* tp = tile;
        if (POLICY) asm volatile("" : "+v"(ln), "+v"(tp));
        const int ec_p = ln >> 2, member_p = ln & 3;
        const bool done = (run & POM_ST_DONE) != 0;
        const bool simple = POLICY && ((p.simple_mask >> member_p) & 1);        /* this lane's agent plays SimpleAgent */
        const bool fixed = tk == 1 && ((p.first_mask >> member_p) & 1);         /* ... and this tick's move is the caller's */
        /* agent m's 16 bits of the tick's draw: SimpleAgent's one random choice, or the stream's move */
        const uint32_t r = pom_rng_draw_half(seed_r, JOBS ? env_key : key0 + (uint32_t)ec_p, (uint32_t)(tk - 1), member_p >> 1);
        const uint32_t r16 = (r >> (16 * (member_p & 1))) & 0xFFFFu;
        int mine = first;
        if (POLICY) {
            uint8_t* const danger = reinterpret_cast<uint8_t*>(tp + POM_REC_DWORDS * 16);
            uint32_t* const sets = tp + (POM_REC_DWORDS + 32) * 16;
            LdsEnv<16, 4> accp(tp, ec_p, member_p);
            uint32_t* const park = tp + RP_ROWS * 16 + ln;
            uint32_t m0 = park[0], m1 = park[64]; /* the memory does not stay in registers through the tick */
            PolicyStore st{tp, tp + ec_p, danger + ec_p, sets + ec_p, member_p};
            const PomPolicyEnv E{{L.a0[0], L.a0[1], L.a0[2], L.a0[3]}, {accp.ag1(0), accp.ag1(1), accp.ag1(2), accp.ag1(3)}, L.bIdx, L.bCnt};
            if (!done) { /* all four lanes of the env, dead agents' lanes included */
                pom_policy_prepare_clear(st);
                pom_policy_prepare_fill(st, E);
                pom_policy_prepare_safe(st);
            }
            /* act() is only asked of live agents (environment.cpp:139-146); the wavefront's searches run together: EVERY lane goes in */
            const bool actor = !done && simple && !ag_dead(sel4(member_p, L.a0));
#if defined(POM_DIAG)
            long long pt_last = 0, pt_acc[POM_PP_N];
            mine = pom_policy_wave(st, E, member_p, m0, m1, actor, (int)((r16 * 5u) >> 16), sets, ln, pt_last, pt_acc);
#else
            mine = pom_policy_wave(st, E, member_p, m0, m1, actor, (int)((r16 * 5u) >> 16), sets, ln);
#endif
            park[0] = m0;
            park[64] = m1;
            /* the caller's move of tick 1: a SimpleAgent overridden here has been asked all the same, its memory has moved on */
            if (fixed) mine = (int)park[128];
        }
        if (!done) { /* the quad's four lanes agree */
            if (!fixed && !simple) mine = pom_rng_pick(r16, p.dist); /* the stream's move (dead agents get theirs too) */
            int ln2 = lane;
            uint32_t* t2 = tile;
            if (POLICY) asm volatile("" : "+v"(ln2), "+v"(t2));
            const int ec2 = ln2 >> 2, member2 = ln2 & 3;
            LdsEnv<16, 4> acc2(t2, ec2, member2);
            PomStepper<LdsEnv<16, 4>> stepper2(acc2, L);
            const uint32_t status = pom_tile_env_tick(stepper2, L, mine, t2, ec2, member2, true, p.max_steps, run & 0xFFu);
            run = status | (run & 0x100u) | (L.ub ? 0x100u : 0u) | ((uint32_t)tk << 16);
        }
    }

    /* out: pom_rollout_kernel's word, one dword per env from its owner lane */
    if (valid && member == 0) {
        const uint32_t word = pom_rollout_word(L, run & 0xFFu, (run & 0x100u) != 0, run >> 16);
        if constexpr (JOBS) p.result[(int64_t)sample * p.jobs + slot_out] = word;
        else p.result[(int64_t)sample * p.n + e] = word;
    }
    if constexpr (JOBS) /* an entry of the list without a job: POM_RO_NONE */
        if (!valid && member == 0 && slot_out < p.jobs) p.result[(int64_t)sample * p.jobs + slot_out] = (uint32_t)POM_RO_NONE;
}

#endif /* POM_ROLLOUT_POLICY_H_ */
