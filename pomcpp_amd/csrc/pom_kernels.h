/*
 * pom_kernels.h — the gfx950 kernels of the batched Pommerman stepper (device side only; the host runtime that launches
 * them is pom_issue.h, the C-ABI of include/pom_batch.h is pom_batch.hip).  Written for MI355X only: 64-lane wavefronts,
 * one wavefront per workgroup, each env's board / bomb queue / flame queue in a column of the wavefront's LDS tile
 * ([row][lane]: every per-lane dynamic index is an LDS address, no shuffles, no scratch).
 *
 * The tick itself is pom_step_body.h; the kernels here are the data movement around it:
 *   HBM (packed records in 16-env tiles, pom_packed.h) -> LDS tile + VGPRs -> tick(s) -> HBM,
 * the SimpleAgent policy kernel, the observation export, the board generator and counters.  This file holds the core unit's
 * __global__ kernels and their parameter structs, and only pom_batch.hip includes it; what the kernels are made of, and what the
 * kernel families of the other units are made of too, is pom_device.h and the parts it lists.  pom_boundary.h (the pack / unpack
 * between the boundary's 1004-byte States and the tiles, the one-State call, the status extraction and the snapshot) is included
 * below, where its kernels always stood.
 */
#ifndef POM_KERNELS_H_
#define POM_KERNELS_H_

#include "pom_device.h"

/* POLICY: the moves are not read but decided here — lane m of an env's quad is agent m and runs SimpleAgent::act
 * (pom_policy_body.h) on the tile the tick is about to work on: Environment::Step with four SimpleAgents in ONE kernel, one
 * record load per tick instead of two and no Move[4] round trip (pom_batch_step_simple). */
/* SINGLE: the launch plays exactly one tick (p.ticks == 1: every launch of the bench, of an RL loop, of the explicit-move
 * steps) — an instantiation without the tick loop, so that nothing is kept alive "for the next tick". */
/* CHAIN: a launch of a queue without barriers between its packets (pom_chain.h): the wavefront first waits until its tile's
 * previous tick has been stored (StepParams.tile_seq), fetches the record past the vector cache, and publishes the tile when
 * its own stores have arrived.  A launch then no longer lasts as long as its slowest wavefront: the next launch's
 * wavefronts start on the tiles that are ready. */
extern "C" __device__ uint64_t pom_dispatch_id(void) __asm("llvm.amdgcn.dispatch.id"); /* the AQL packet's index in its queue */

/* pom_rng_pick (pom_rng.h; the same values) where `dist` is wave-uniform: the stress distribution's compare chain behind a BRANCH —
 * as a select (what the compiler makes of the host's form) every tick of every distribution pays for both picks.  The quad step
 * kernels use this; the one-lane-per-env kernels and the rollouts (pom_rollout.h) keep the select form */
__device__ __forceinline__ int pom_rng_pick_uniform(uint32_t r16, int dist)
{
    int mv;
    if (dist == POM_DIST_STRESS) {
        mv = pom_rng_pick(r16, POM_DIST_STRESS);
        asm volatile("" : "+v"(mv)); /* (nothing to execute: a block with it in is not folded into selects) */
    } else {
        mv = pom_rng_pick(r16, dist); /* (its uniform pick: the stress side folds away behind the branch) */
    }
    return mv;
}

/* OBS: the launch also writes the observation of the state it leaves behind (pom_observe_tile) — an RL tick is then one launch
 * and one read of the record instead of two of each. */
/* VIEW (with OBS): the observation is the four agents' fogged views (PomViewSpec) — an instantiation of its own, not a branch in the
 * OBS one. */
template <int EPW, int G, bool FRESH, bool POLICY = false, bool ATEND = false, bool SINGLE = false, bool CHAIN = false, bool OBS = false,
          bool VIEW = false>
__global__ __launch_bounds__(64 * POM_WPB, (POLICY ? 4 : G == 4 ? POM_QUAD_WAVES : EPW == 16 ? 3 : EPW == 32 ? 2 : 1)) void pom_step_kernel(StepParams p)
{
    static_assert(!CHAIN || SINGLE, "chained launches play one tick each");
    static_assert(!OBS || (SINGLE && !CHAIN && !POLICY && POM_WPB == 1), "the fused observation exists for the one-tick explicit-move shape");
    static_assert(!VIEW || OBS, "the fogged views are a kind of fused observation");
    /* the one-tick kernels' ticket, hand-on and wave-counter adds are issued as plain one-lane atomics (pom_one_lane_address) */
    constexpr bool ONE_LANE_ATOMICS = SINGLE && !(POM_TAKE_OUT & 8);
    static_assert(!SINGLE || G == 4, "the one-tick instantiation exists for the quad shape");
    static_assert(G == 1 || (G == 4 && EPW == 16), "a quad per env needs 16 envs per wavefront");
    static_assert(!POLICY || G == 4, "the policy runs one agent per lane of the quad");
    static_assert(!ATEND || G == 4, "the end-of-tick reset is built for the quad shape only");
    /* POLICY: the danger map (32 rows of bytes) and the cell sets (12 rows) live where the tick keeps its bomb destinations
     * and explosion frames — the policy of a tick is over before its tick begins.  139 rows = 8,896 B: 17 wavefronts per
     * CU would fit, 16 (all of 65,536 envs resident at once) are needed. */
    /* OBS: the staging area — one env's planes (1,936 + 16 B) or four envs' code planes (2,420 B: 38 rows) — lies over the same
     * scratch rows — the tick is over when the observation begins */
    constexpr int OBS_ROWS = (obs_stage_vecs(OBS_PASS_ENVS_FUSED) * 16 + EPW * 4 - 1) / (EPW * 4);
    constexpr int OVERLAY = POLICY ? 44 : OBS ? OBS_ROWS : 0; /* rows behind the record that the policy / the export use when the tick does not */
    constexpr int ROWS = POM_REC_DWORDS + OVERLAY > LDS_ROWS ? POM_REC_DWORDS + OVERLAY : LDS_ROWS;
    static_assert(ROWS >= LDS_ROWS, "the tick's scratch rows fit under the overlay");
    __shared__ __attribute__((aligned(16))) uint32_t tiles_[POM_WPB][ROWS * EPW];
    uint32_t* const tile = tiles_[POM_WPB == 1 ? 0 : threadIdx.x >> 6];
    uint8_t* const danger = reinterpret_cast<uint8_t*>(tile + POM_REC_DWORDS * EPW);
    uint32_t* const sets = tile + (POM_REC_DWORDS + 32) * EPW;
    const int lane = threadIdx.x & 63;
    int64_t tile_local; /* in XCD-aware order (pom_xcd_tile_order), or, chained, by the XCD the workgroup is on */
    uint32_t chain_xcd = 0;
    if (CHAIN) {
        /* the XCD the workgroup IS on decides its tile (launches of different queues start their round-robin at different
         * XCDs): XCD x plays tiles x * q .. x * q + q - 1, its k-th workgroup (workgroup ids x0, x0 + 8, ...) the k-th of them.
         * The grid is padded to a multiple of 8 workgroups.  chain_rot rotates that order within the XCD (a bijection: still every
         * tile once per launch). */
        chain_xcd = pom_chain_xcd();
        const int64_t q = gridDim.x / 8;
        int64_t k_in_xcd = (int64_t)(blockIdx.x / 8) + p.chain_rot;
        if (k_in_xcd >= q) k_in_xcd -= q;
        tile_local = (int64_t)chain_xcd * q + k_in_xcd;
        if (chain_xcd >= 8u) { /* not the machine this was written for: nothing is stepped, no ticket is drawn (the verify pass reports it) */
            if (lane == 0) __hip_atomic_fetch_or(p.chain_err, (uint32_t)POM_CHAIN_E_XCD, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        if (POM_WPB == 1 && p.block0 + tile_local >= p.block_end) return; /* a workgroup of the padding */
    } else {
#if defined(POM_NO_XCD_REMAP)
    tile_local = blockIdx.x;
#else
    { /* pom_xcd_tile_order(blockIdx.x, gridDim.x), written out: the call, inlined, leaves the same tiles but not the same instructions
         in the tick behind it (signed for unsigned minima in 23 of the 27 instantiations), and this kernel's code is kept as measured */
        const int64_t b = blockIdx.x, nb = gridDim.x, q = nb / 8, r = nb % 8, x = b % 8;
        tile_local = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
    }
#endif
    }
    if (POM_WPB > 1) {
        tile_local = tile_local * POM_WPB + (threadIdx.x >> 6);
        if (p.block0 + tile_local >= p.block_end) return; /* the last workgroup of a launch may be short of tiles */
    }
    const int64_t tile_id = p.block0 + tile_local;
    const int64_t np = p.n_pad;
    const bool env_mode = p.mode == POM_MODE_ENV;
    /* data movement: lane -> (env el, row group sub) so that one DMA / store instruction covers 64/EPW rows */
    const int el = lane % EPW, sub = lane / EPW;
    const int64_t e_d = tile_id * EPW + el;
    uint32_t* col_d = p.state + pom_rec_col(e_d); /* buffers hold n_pad columns: in range for every lane */
    /* the tick: G = 1: the lanes with sub == 0 own env el; G = 4: lane -> (env lane/4, member lane%4), all lanes run */
    const int ec = G == 1 ? el : lane >> 2;
    const int member = G == 1 ? 0 : lane & 3;
    const int64_t e = tile_id * EPW + ec;
    const bool owner = G == 1 ? sub == 0 : member == 0; /* the lane that speaks for env e (register rows, counters) */
    const bool runs = G == 1 ? sub == 0 : true;         /* the lanes that execute env e's tick */
    const bool valid = runs && e < p.n;
    const uint32_t env_key = (uint32_t)(p.env_offset + e); /* the env's number in the whole job: what its move draws are keyed by */
    uint32_t* t = tile + ec;

#if defined(POM_DIAG)
    const long long t_begin = (long long)clock64();
#endif
    long long c_steps = 0, c_episodes = 0, c_resets = 0, c_ub = 0;

    /* the launch's first tick: asked for BEFORE the record, so that waiting for it (in-order vmcnt) does not wait for the record */
    uint32_t tick0 = CHAIN ? p.tick0 : p.tick0 + *p.tick_base; /* (graphs replay sub-batch launches, never chained ones) */
    PomChainVisit cv; /* CHAIN: this wavefront's visit of its tile */
    if (CHAIN) {
        unsigned long long* const word = p.tile_seq + tile_id * POM_CHAIN_WORD_STRIDE;
        if (!pom_chain_enter<ONE_LANE_ATOMICS>(word, chain_xcd, p.chain_seq0, p.tape_len, p.chain_wait_limit, p.chain_err, lane, cv)) return;
        tick0 += (uint32_t)cv.dist;
        /* the loads below are issued after the word has been seen: the record they fetch is the stored one */
        load_tile16_x4<POM_REC_DWORDS, 16>(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    } else if (EPW == 16) load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane); /* 16-byte pieces, 7 instructions of 1 KB */
    else load_tile<EPW>(col_d, POM_TILE_ENVS, tile, sub);
    uint32_t m0 = 0, m1 = 0; /* POLICY: this lane's agent's memory */
    if (POLICY) {
        m0 = pom_load_shared<CHAIN>(p.agent_mem + tile_id * 64 + lane);
        m1 = pom_load_shared<CHAIN>(p.agent_mem + 4 * np + tile_id * 64 + lane);
    }
    /* the first tick's moves do not depend on the record: hash / fetch them while the record is on its way */
    uint64_t draw0 = 0;
    int4 moves0 = make_int4(0, 0, 0, 0);
    int mine0 = POM_MOVE_IDLE; /* the one-tick quad kernels: lane m's agent's move, the one value that is carried to the tick */
    /* explicit moves come one tick per launch: the several-tick quad kernel never sees any (step_kernel) */
    constexpr bool TAKES_MOVES = SINGLE || G == 1;
    constexpr bool QUAD1 = SINGLE && G == 4;
    if (!POLICY) {
        if (TAKES_MOVES && p.moves) { /* wave-uniform, and a branch: the side not taken costs nothing */
            /* chained: tick `chain_dist` of the caller's move tape (pom_batch_step_device_many) */
            if (QUAD1) { /* the quad's lanes take a dword each of their env's Move[4] */
                /* Move[4] of env e = tile_id * 16 + lane / 4, agent lane % 4: the tile's 64 moves lie one behind the other */
                const int32_t* const mt = p.moves + ((CHAIN ? (int64_t)cv.dist * p.n : (int64_t)0) + tile_id * EPW) * 4;
                if (valid) mine0 = *reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(mt) + 4u * (uint32_t)lane);
            } else if (valid) moves0 = reinterpret_cast<const int4*>(p.moves)[(CHAIN ? (int64_t)cv.dist * p.n : (int64_t)0) + e];
        } else {
            if (G == 4 && !SINGLE) { /* several ticks per launch: the draw is made where it is used, nothing to carry */
            } else if (G == 4) { /* lane m needs agent m's 16 bits only */
                mine0 = pom_rng_pick_uniform((pom_rng_draw_half(p.seed, env_key, tick0, member >> 1) >> (16 * (member & 1))) & 0xFFFFu, p.dist);
            } else draw0 = pom_rng_draw(p.seed, env_key, tick0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the DMA rows have landed (one wavefront per workgroup: no barrier) */
    PomLane L;
    int time_step = 0;
    uint32_t status = 0;
    /* the one-tick kernels that restart at the start of the tick look at the status byte alone first: whether an env restarts is
     * known before its register rows are unpacked, and they are unpacked ONCE, behind the restarts — not a second time in the
     * wavefronts that restart somebody (about half of them) */
    constexpr bool UNPACK_LATE = SINGLE && !ATEND;
    if (UNPACK_LATE) status = t[(POM_REC_AGENTS + 3) * EPW] >> 24; /* (as pom_lane_load reads it) */
    else lane_from_tile(L, time_step, status, t, EPW);
    bool restarted = false;

    LdsEnv<EPW, G> acc(tile, ec, member);
    PomStepper<LdsEnv<EPW, G>> stepper(acc, L);
#if defined(POM_TRUNC)
    L.trunc = p.trunc;
#endif
#if defined(POM_DIAG)
#pragma unroll /* (every loop over the phase clocks: an index the compiler does not resolve puts them into scratch) */
    for (int k = 0; k < POM_PH_N; k++) L.t_acc[k] = 0;
    L.t_last = t_begin;
    POM_STAMP(L, POM_PH_LOAD);
#endif

    const int n_ticks = SINGLE ? 1 : p.ticks;
    for (int tk = 0; tk < n_ticks; tk++) {
        if (ATEND) {
            /* POM_RESET_AT_END (a separate instantiation): nobody is finished when a tick begins; see the end of the tick */
        } else if (FRESH) { /* a separate instantiation: the replay kernel carries none of this */
            /* fresh boards: a finished env starts its next game on the board (board_seed, env, games played) of
             * pom_boardgen.h, drawn into its tile column by the whole wavefront, one restarting env after the other —
             * the one place, first tick included */
            const bool reload = valid && env_mode && p.auto_reset == POM_RESET_AT_START && (status & POM_ST_DONE);
            uint64_t todo = __ballot(reload && owner);
            while (todo) {
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1); /* an owner lane */
                todo &= todo - 1;
                const int ec_u = G == 1 ? src : src >> 2;
                uint32_t ep = 0;
                if (lane == src) {
                    ep = pom_load_shared<CHAIN>(p.episode + e) + 1u;
                    p.episode[e] = ep;
                }
                ep = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)ep, src));
                const uint32_t key = pom_board_key(p.board_seed, (uint32_t)(p.env_offset + tile_id * EPW + ec_u), ep);
                pom_boardgen_wave<EPW, POM_REC_DWORDS>(tile, ec_u, (uint32_t)__builtin_amdgcn_readfirstlane((int)key), lane);
            }
            asm volatile("" ::: "memory"); /* other lanes wrote this lane's column: no read of it may be scheduled earlier */
            if (!UNPACK_LATE && reload) lane_from_tile(L, time_step, status, t, EPW); /* the register-resident rows, from the new record */
            restarted = reload;
            c_resets += __popcll(__ballot(reload && owner));
        } else {
            /* a finished env restarts from its snapshot (tick 0: as the record says; later ticks of a launch: as the epilogue
             * found), by the whole wavefront: one env's record, or those of up to four envs with their loads in flight together
             * (restart_columns) */
            const bool reload = valid && env_mode && p.auto_reset == POM_RESET_AT_START && (status & POM_ST_DONE);
            const uint64_t todo = __ballot(reload && owner);
            if (todo) {
                c_resets += __popcll(todo);
                int lane_now = lane; /* (as at the end of the tick: addresses worked out where they are used — a launch of several ticks
                                        would carry them from tick to tick) */
                if (!SINGLE) asm volatile("" : "+v"(lane_now));
                restart_columns<EPW, POM_REC_DWORDS, G == 1 ? 1 : 4>(tile, todo, p.snap + tile_id * EPW * POM_REC_DWORDS, lane_now);
                asm volatile("" ::: "memory"); /* other lanes wrote this lane's column: no read of it may be scheduled earlier */
                if (!UNPACK_LATE && reload) lane_from_tile(L, time_step, status, t, EPW); /* the register-resident rows, from the new record */
            }
            restarted = reload;
        }
        if (UNPACK_LATE) lane_from_tile(L, time_step, status, t, EPW); /* every lane's register rows, restarted or not */
        const bool active = valid && !(env_mode && (status & POM_ST_DONE));
        bool newly_done = false, new_ub = false;
        int mv_own = POM_MOVE_IDLE;
        if (POLICY) {
            if (tk > 0) { /* the memory does not stay in registers through the tick */
                m0 = p.agent_mem[tile_id * 64 + lane];
                m1 = p.agent_mem[4 * np + tile_id * 64 + lane];
            }
            if (restarted) m0 = m1 = 0; /* a new game gets fresh agents */
            restarted = false;
            PolicyStore st{tile, t, danger + ec, sets + ec, member};
#if defined(POM_TRUNC)
            st.trunc = p.trunc; /* cuts -4 .. -1: none of the policy, + clear, + fill, + safe (act and the tick skipped); 0: the whole policy */
            if (active) {
                if (p.trunc > -4) pom_policy_prepare_clear(st);
                if (p.trunc > -3) pom_policy_prepare_fill(st, PomPolicyEnv{{L.a0[0], L.a0[1], L.a0[2], L.a0[3]}, {acc.ag1(0), acc.ag1(1), acc.ag1(2), acc.ag1(3)}, L.bIdx, L.bCnt});
                if (p.trunc > -2) pom_policy_prepare_safe(st);
            }
            if (p.trunc > -1)
#else
            if (active) { /* all four lanes of the env, dead agents' lanes included */
                pom_policy_prepare_clear(st);
                pom_policy_prepare_fill(st, PomPolicyEnv{{L.a0[0], L.a0[1], L.a0[2], L.a0[3]}, {acc.ag1(0), acc.ag1(1), acc.ag1(2), acc.ag1(3)}, L.bIdx, L.bCnt});
                pom_policy_prepare_safe(st);
            }
#endif
            { /* act() is only asked of live agents (environment.cpp:139-146); the wavefront's searches run together: every lane goes in */
                const PomPolicyEnv E{{L.a0[0], L.a0[1], L.a0[2], L.a0[3]}, {acc.ag1(0), acc.ag1(1), acc.ag1(2), acc.ag1(3)}, L.bIdx, L.bCnt};
                const uint32_t r = pom_rng_draw_half(p.seed, env_key, tick0 + (uint32_t)tk, member >> 1);
                const bool actor = active && !ag_dead(sel4(member, L.a0));
#if defined(POM_DIAG)
                long long pt_last = 0, pt_acc[POM_PP_N];
                mv_own = pom_policy_wave(st, E, member, m0, m1, actor, (int)((((r >> (16 * (member & 1))) & 0xFFFFu) * 5u) >> 16), sets, lane, pt_last, pt_acc);
#else
                mv_own = pom_policy_wave(st, E, member, m0, m1, actor, (int)((((r >> (16 * (member & 1))) & 0xFFFFu) * 5u) >> 16), sets, lane);
#endif
            }
            p.agent_mem[tile_id * 64 + lane] = m0;
            p.agent_mem[4 * np + tile_id * 64 + lane] = m1;
        }
        if (active) {
            /* the moves, a nibble per agent.  With a quad per env lane m works out agent m's and the quad exchanges them */
            uint32_t mvp;
            if (G == 4) {
                int mine;
                if (POLICY) {
                    mine = mv_own;
                } else if (SINGLE) { /* explicit or drawn: chosen while the record was on its way */
                    mine = mine0;
                } else {
                    const uint32_t r = pom_rng_draw_half(p.seed, env_key, tick0 + (uint32_t)tk, member >> 1);
                    mine = pom_rng_pick_uniform((r >> (16 * (member & 1))) & 0xFFFFu, p.dist);
                }
                mvp = stepper.pack_moves_quad(mine);
            } else {
                int mv[4];
                if (p.moves) {
                    mv[0] = moves0.x; mv[1] = moves0.y; mv[2] = moves0.z; mv[3] = moves0.w;
                } else {
                    const uint64_t r = tk == 0 ? draw0 : pom_rng_draw(p.seed, env_key, tick0 + (uint32_t)tk);
#pragma unroll
                    for (int i = 0; i < 4; i++) mv[i] = pom_rng_pick((uint32_t)(r >> (16 * i)) & 0xFFFFu, p.dist);
                }
                mvp = stepper.pack_moves(mv);
            }
            L.ub = 0; /* this tick's flags; the record's (in the top bytes of two agent words, untouched by the tick) are added afterwards */
            status &= ~(uint32_t)POM_ST_RESTARTED;
            POM_STAMP(L, POM_PH_RESTART); /* diagnostic builds: the restarts and the move draw */
#if defined(POM_TRUNC)
            if (p.trunc <= 0) {
            } else
#endif
            if (POLICY) {
                /* a fresh view of the tile for the tick: keeps the compiler from computing the tick's addresses before the
                 * policy and carrying them through it (the fused kernel otherwise wants 170 VGPRs) */
                uint32_t* t2 = tile;
                asm volatile("" : "+v"(t2));
                LdsEnv<EPW, G> acc2(t2, ec, member);
                PomStepper<LdsEnv<EPW, G>> stepper2(acc2, L);
                stepper2.step_packed(mvp);
            } else {
                stepper.step_packed(mvp);
            }
            new_ub = L.ub != 0;
            L.ub |= (t[(POM_REC_AGENTS + 5) * EPW] >> 24) | ((t[(POM_REC_AGENTS + 7) * EPW] >> 24) << 8);
            if (env_mode) {
                /* timeStep is looked at here only: read back from the tile instead of living in a register through the tick */
                time_step = (int)t[POM_REC_TIMESTEP * EPW] + 1;
                if (owner) t[POM_REC_TIMESTEP * EPW] = (uint32_t)time_step;
                status = pom_env_epilogue(L, time_step, p.max_steps, status);
                newly_done = (status & POM_ST_DONE) != 0;
            }
        }
        c_steps += __popcll(__ballot(active && owner));
        c_episodes += __popcll(__ballot(newly_done && owner));
        c_ub += __popcll(__ballot(new_ub && owner));
        if (ATEND) {
            /* The tick that finishes an episode also starts the next one: the final record goes to the terminal buffer, the
             * env's column is replaced by its start state (snapshot record, or the next generated board), the agents' memory
             * is wiped.  What the caller reads next — state, observation, status — is the new episode's first state, marked
             * POM_ST_RESTARTED; the move it then supplies is a move for THAT state. */
            uint64_t todo = __ballot(newly_done && owner);
            if (todo) {
                c_resets += __popcll(todo);
                if (newly_done && owner) { /* the register-resident rows of the final record (timeStep is in the tile already) */
#pragma unroll
                    for (int k = 0; k < 8; k++) t[(POM_REC_AGENTS + k) * EPW] = pom_lane_agent_word(L, status, k, t[(POM_REC_AGENTS + k) * EPW]);
                }
                asm volatile("" ::: "memory");
                int lane_end = lane; /* (a lane id the compiler cannot see through: the global addresses below are worked out here, not at
                                        the top of the kernel and carried through the tick) */
                asm volatile("" : "+v"(lane_end));
                const uint64_t finished = todo;
                do {
                    const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1); /* an owner lane */
                    todo &= todo - 1;
                    const int ec_u = G == 1 ? src : src >> 2;
                    const int64_t e_u = tile_id * EPW + ec_u;
                    uint32_t* tr = p.terminal + e_u * POM_REC_DWORDS;
                    column_to_record<EPW>(tile, ec_u, tr, lane_end);
                    if (FRESH) {
                        uint32_t ep = 0;
                        if (lane == src) {
                            ep = pom_load_shared<CHAIN>(p.episode + e_u) + 1u;
                            p.episode[e_u] = ep;
                        }
                        ep = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)ep, src));
                        const uint32_t key = pom_board_key(p.board_seed, (uint32_t)(p.env_offset + e_u), ep);
                        pom_boardgen_wave<EPW, POM_REC_DWORDS>(tile, ec_u, (uint32_t)__builtin_amdgcn_readfirstlane((int)key), lane_end);
                    }
                } while (todo);
                /* the final records have been read out of the tile: the start states of all of them, their loads in flight together */
                if (!FRESH) restart_columns<EPW, POM_REC_DWORDS, G == 1 ? 1 : 4>(tile, finished, p.snap + tile_id * EPW * POM_REC_DWORDS, lane_end);
                asm volatile("" ::: "memory");
                if (newly_done && runs) {
                    lane_from_tile(L, time_step, status, t, EPW);
                    status |= POM_ST_RESTARTED;
                    if (POLICY) { /* a new game gets fresh agents */
                        int lane_here = lane; /* (a lane id the compiler cannot see through: the two addresses are worked out here, not carried through the tick) */
                        asm volatile("" : "+v"(lane_here));
                        p.agent_mem[tile_id * 64 + lane_here] = 0u;
                        p.agent_mem[4 * np + tile_id * 64 + lane_here] = 0u;
                    }
                }
            }
        }
        POM_STAMP(L, POM_PH_EPILOGUE);
    }

    /* write back: the owner puts the register-resident rows into the tile, then the whole record leaves in row groups */
    if (owner) { /* (timeStep went into the tile with the tick's epilogue) */
#pragma unroll
        for (int k = 0; k < 8; k++) t[(POM_REC_AGENTS + k) * EPW] = pom_lane_agent_word(L, status, k, (k & 1) ? t[(POM_REC_AGENTS + k) * EPW] : 0u);
    }
    if (EPW == 16) {
        /* the store addresses are functions of the lane id and the arguments only: left alone the compiler computes them at
         * the top of the kernel and keeps 14 registers alive (or spilled) through the whole tick — hand it a lane id it cannot
         * see through, so that they are computed here */
        int lane_late = lane;
        asm volatile("" : "+v"(lane_late));
        /* chained: with the non-temporal hint (-2.5 % per step: the stores are acknowledged sooner and the wavefront's slot is free
         * sooner; on the sub-batch kernels' stores, or on the loads, the hint gains nothing or loses) */
        store_tile16_x4<CHAIN>(p.state + tile_id * POM_TILE_DWORDS, tile, lane_late);
    } else {
        store_tile<EPW>(col_d, POM_TILE_ENVS, tile, sub, el);
    }
    if (OBS) {
        /* the observation of what the tick left in the tile, while the record's stores are on their way (they have been read out
         * of LDS into registers; the staging area lies behind the record rows) */
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const ObserveParams op{nullptr, p.n, p.n_pad, 0, p.obs_planes, p.obs_agent_attrs, p.obs_env_attrs, p.obs_dtype, p.obs_per_agent,
                               VIEW ? p.obs_viewer_attrs : nullptr, VIEW ? p.obs_view_radius : 0};
        pom_observe_tile<OBS_PASS_ENVS_FUSED, VIEW>(op, tile, reinterpret_cast<uint4*>(tile + POM_REC_DWORDS * EPW), tile_id, lane);
    }
    if (CHAIN) { /* the record's stores have been acknowledged by the L2 before the word that hands the tile on is written */
        pom_chain_leave<ONE_LANE_ATOMICS>(p.tile_seq + tile_id * POM_CHAIN_WORD_STRIDE, lane, cv);
#if defined(POM_CHAIN_DIAG)
        if (lane == 0) { /* per tile, summed over launches: cycles to the ticket, cycles polling, cycles in all, polls */
            unsigned long long* d = p.tile_seq + (p.block_end - p.block0) * POM_CHAIN_WORD_STRIDE + 68 * tile_id;
            d[4 + 2 * (cv.visit & 31)] = (unsigned long long)cv.rt0; /* the last 32 visits: start and end on the 100 MHz clock */
            d[5 + 2 * (cv.visit & 31)] = (unsigned long long)wall_clock64();
            d[0] += (unsigned long long)(cv.t1 - cv.t0);
            d[1] += (unsigned long long)(cv.t2 - cv.t1);
            d[2] += (unsigned long long)((long long)__builtin_readcyclecounter() - cv.t0);
            d[3] += (unsigned long long)cv.polls;
        }
#endif
    }

#if defined(POM_DIAG)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    POM_STAMP(L, POM_PH_STORE);
    if (p.diag) { /* one slot per wavefront: no contended atomics that would distort the timing.  Phases entered by some envs
                     only (the blast engines) are booked by the lanes inside; everybody else books the same time on the phase
                     around them — so the wavefront reports the lane that spent the most time inside */
        long long inside = 0;
#pragma unroll
        for (int k = POM_PH_X_SCAN; k <= POM_PH_X_SHORT; k++) inside += L.t_acc[k];
        long long best = inside;
        for (int o = 32; o > 0; o >>= 1) {
            const long long w = __shfl_xor(best, o);
            best = w > best ? w : best;
        }
        const uint64_t who = __ballot(inside == best);
        if (lane == __ffsll((unsigned long long)who) - 1)
#pragma unroll
            for (int k = 0; k < POM_PH_N; k++) p.diag[tile_id * POM_PH_N + k] += L.t_acc[k];
    }
#endif
    if (lane == 0) {
        /* each wavefront owns its slot, so nothing contends; the adds are returnless atomics only because those are
         * fire-and-forget — a load / add / store would keep the finished wavefront alive for a global round trip */
        auto* wc = pom_one_lane_address<ONE_LANE_ATOMICS>(reinterpret_cast<unsigned long long*>(p.wave_counters + tile_id * POM_CNT_N));
        __hip_atomic_fetch_add(&wc[POM_CNT_STEPS], (unsigned long long)c_steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c_episodes) __hip_atomic_fetch_add(&wc[POM_CNT_EPISODES], (unsigned long long)c_episodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c_resets) __hip_atomic_fetch_add(&wc[POM_CNT_RESETS], (unsigned long long)c_resets, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c_ub) __hip_atomic_fetch_add(&wc[POM_CNT_UB_TICKS], (unsigned long long)c_ub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

/* The hand-off by itself (pom_chain_litmus, tests): the same tile choice, ticket, wait, sc1 DMA load, non-temporal store and
 * publication as the CHAIN step kernels, with a "tick" whose result gives every stale or torn read away — visit v of a tile must
 * find ALL 1,312 dwords of the record equal to v (the j-th dword XOR-tagged with its index, so that a record of another tile or a
 * shifted piece cannot pass either) and leaves them at v + 1.  out[0]: records that were not what the visit before left (counted
 * per wavefront), out[1]: dwords that differed, out[2]: visits played. */
struct LitmusParams {
    uint32_t* data;              /* tiles x POM_TILE_DWORDS */
    unsigned long long* tile_seq;
    uint32_t* err;
    unsigned long long* out;
    int64_t tiles;
    uint32_t chain_seq0;
    uint64_t wait_limit;
};
__global__ __launch_bounds__(64) void pom_chain_litmus_kernel(LitmusParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POM_REC_DWORDS * 16];
    const int lane = threadIdx.x;
    const uint32_t xcd = pom_chain_xcd();
    if (xcd >= 8u) return;
    const int64_t tile_id = (int64_t)xcd * (gridDim.x / 8) + blockIdx.x / 8;
    if (tile_id >= p.tiles) return;
    unsigned long long* const word = p.tile_seq + tile_id * POM_CHAIN_WORD_STRIDE;
    PomChainVisit cv;
    if (!pom_chain_enter(word, xcd, p.chain_seq0, 0u, p.wait_limit, p.err, lane, cv)) return;
    load_tile16_x4<POM_REC_DWORDS, 16>(p.data + tile_id * POM_TILE_DWORDS, tile, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t expect = p.chain_seq0 + (uint32_t)cv.dist; /* = this visit's number: as many visits are stored */
    const uint32_t tag = (uint32_t)tile_id * 2654435761u;
    int bad = 0;
#pragma unroll 4
    for (int k = lane; k < POM_TILE_DWORDS; k += 64) {
        bad += tile[k] != (expect ^ (tag + (uint32_t)k));
        tile[k] = (expect + 1u) ^ (tag + (uint32_t)k);
    }
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    store_tile16_x4<true>(p.data + tile_id * POM_TILE_DWORDS, tile, lane);
    pom_chain_leave(word, lane, cv);
    if (lane == 0) {
        if (bad) {
            atomicAdd(p.out + 0, 1ull);
            atomicAdd(p.out + 1, (unsigned long long)bad);
        }
        atomicAdd(p.out + 2, 1ull);
    }
}

/* chained launches, before the first one: which XCD does workgroup b of a small grid land on?  (pom_chain.h checks that it is the
 * round-robin over eight XCDs the tile choice assumes — a partitioned device, or another chip, is not) */
__global__ void pom_chain_probe_kernel(uint32_t* xcd_of_block)
{
    const uint32_t x = pom_chain_xcd();
    if (threadIdx.x == 0) xcd_of_block[blockIdx.x] = x;
}

/* chained launches, after a join: every tile must have drawn exactly `visits` tickets, and have stored as many visits — or be
 * poisoned (a visitor could not play: POM_CHAIN_POISON), in which case (tile, visits really stored) goes onto the list the host
 * replays from (chain_settle).  aux[0]: the POM_CHAIN_E_* flags, aux[1]: length of the list, list: aux + 2, two dwords per entry. */
__global__ void pom_chain_verify_kernel(const unsigned long long* tile_seq, int64_t tiles, uint32_t visits, uint32_t* aux)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tiles) return;
    const unsigned long long w = tile_seq[t * POM_CHAIN_WORD_STRIDE];
    const uint32_t stored = (uint32_t)w & POM_CHAIN_COUNT_MASK;
    if ((uint32_t)(w >> POM_CHAIN_TICKET_SHIFT) != visits) atomicOr(aux, (uint32_t)POM_CHAIN_E_UNEVEN);
    if ((uint32_t)w & POM_CHAIN_POISON) {
        const uint32_t k = atomicAdd(aux + 1, 1u);
        aux[2 + 2 * k] = (uint32_t)t;
        aux[3 + 2 * k] = stored;
        if (stored >= visits) atomicOr(aux, (uint32_t)POM_CHAIN_E_UNEVEN); /* poisoned means: at least one visit not played */
    } else if (stored != visits) {
        atomicOr(aux, (uint32_t)POM_CHAIN_E_UNEVEN);
    }
}

/* ---------------------------------------------------------------------------------------------
 * SimpleAgent policy (pom_policy_body.h): one lane per AGENT, the quad 4e..4e+3 = the four agents of env e,
 * 16 envs per wavefront.  The wavefront DMAs record rows 0..63 (board, meta, agents, bombs: 0..61) of its 16 envs into a shared
 * tile; per env the four lanes together prepare a danger map ([128][16] bytes) and three cell sets.  The reachability
 * questions are flood fills on 121-bit cell sets in registers, so a wavefront needs only 9 KB of LDS (17 wavefronts per CU).  Output:
 * Move[4] per env into the handle's move buffer, agent memory (2 dwords per agent) updated in place.  A finished env that the
 * next step will restart is read from its snapshot column — or, with fresh boards, drawn here exactly as the tick will draw
 * it — and gets fresh (zero) agent memory, so policy and tick see the same game.
 * ------------------------------------------------------------------------------------------- */
enum { POL_ROWS = POM_REC_FLAMES, POL_LOAD_ROWS = 64 }; /* the policy reads rows 0..59 (board, timeStep, agents, bombs); they arrive 16 rows per instruction */
static_assert(POL_ROWS <= POL_LOAD_ROWS && POL_LOAD_ROWS <= POM_REC_DWORDS, "policy rows");


struct PolicyParams {
    const uint32_t* state;
    const uint32_t* snap;
    uint32_t* agent_mem; /* [2][4 * n_pad] */
    int32_t* moves;      /* [n_pad][4] */
    int64_t n, n_pad, env_offset, block0;
    uint64_t seed;
    uint32_t tick;
    int32_t mode, auto_reset;
    const uint32_t* episode; /* fresh boards: a restarting env is judged on the board the tick will generate for it */
    uint64_t board_seed;
    int32_t fresh;
#if defined(POM_DIAG)
    long long* diag; /* POM_PP_N accumulators per wavefront, diagnostic build only */
#endif
};

__global__ __launch_bounds__(64) void pom_policy_kernel(PolicyParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POL_LOAD_ROWS * 16];
    __shared__ uint8_t danger[128 * 16]; /* 121 cells; the safe-set pass reads whole 32-cell words */
    __shared__ uint32_t sets[12 * 16];
    const int lane = threadIdx.x;
    const int64_t np = p.n_pad;
    const int64_t tile_local = pom_xcd_tile_order(blockIdx.x, gridDim.x);
    const int64_t tile_id = p.block0 + tile_local;
    const bool env_mode = p.mode == POM_MODE_ENV;
#if defined(POM_DIAG)
    long long t_last = (long long)clock64(), t_acc[POM_PP_N] = {0, 0, 0, 0, 0, 0, 0};
#endif
    load_tile16_x4<POL_LOAD_ROWS>(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    /* the policy: lane -> (env lane/4, agent lane%4) */
    const int ec = lane >> 2, id = lane & 3;
    const int64_t e = tile_id * 16 + ec;
    const int64_t slot = e * 4 + id; /* = tile_id * 64 + lane */
    uint32_t m0 = p.agent_mem[slot], m1 = p.agent_mem[4 * np + slot];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    /* an env the tick is about to restart is judged on the board it will restart on: its snapshot record (array of structs,
     * fetched by the whole wavefront: restart_column) or, with fresh boards, the board the tick kernel is about to draw for it
     * (the tick counts the episode) */
    const bool restart = e < p.n && env_mode && p.auto_reset == POM_RESET_AT_START && ((pom_rec_meta2(tile + ec, 16) >> 8) & POM_ST_DONE);
    if (restart) m0 = m1 = 0; /* a new game gets fresh agents */
    {
        uint64_t todo = __ballot(restart && id == 0);
        if (p.fresh) {
            while (todo) {
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
                todo &= todo - 1;
                const int ec_u = src >> 2;
                const uint32_t ep = p.episode[tile_id * 16 + ec_u] + 1u;
                const uint32_t key = pom_board_key(p.board_seed, (uint32_t)(p.env_offset + tile_id * 16 + ec_u),
                                                   (uint32_t)__builtin_amdgcn_readfirstlane((int)ep));
                pom_boardgen_wave<16, POL_ROWS>(tile, ec_u, (uint32_t)__builtin_amdgcn_readfirstlane((int)key), lane);
            }
        } else if (todo) { /* the records of up to four envs with their loads in flight together */
            restart_columns<16, POL_ROWS, 4>(tile, todo, p.snap + tile_id * 16 * POM_REC_DWORDS, lane);
        }
        asm volatile("" ::: "memory");
    }
    const uint32_t* t = tile + ec;
    PomPolicyEnv E;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        E.a0[i] = (int)t[(POM_REC_AGENTS + 2 * i) * 16];
        E.a1[i] = (int)t[(POM_REC_AGENTS + 2 * i + 1) * 16];
    }
    const uint32_t meta = pom_rec_meta(t, 16), meta2 = pom_rec_meta2(t, 16);
    E.bIdx = (int)((meta >> 8) & 0xFF);
    E.bCnt = (int)((meta >> 16) & 0xFF);
    const bool frozen = env_mode && ((meta2 >> 8) & POM_ST_DONE); /* finished and not restarted: Environment::Step returns */
    int mv = POM_MOVE_IDLE;
    PolicyStore st{tile, t, danger + ec, sets + ec, id};
    POM_PSTAMP(POM_PP_LOAD);
    if (e < p.n && !frozen) { /* all four lanes of the env, dead agents' lanes included */
        pom_policy_prepare_clear(st);
        pom_policy_prepare_fill(st, E);
        pom_policy_prepare_safe(st);
    }
    POM_PSTAMP(POM_PP_PREPARE);
    { /* act() is only asked of live agents (environment.cpp:139-146); the wavefront's searches run together: every lane goes in */
        const bool actor = e < p.n && !frozen && !ag_dead(sel4(id, E.a0));
        const uint32_t r = pom_rng_draw_half(p.seed, (uint32_t)(p.env_offset + e), p.tick, id >> 1);
        const int draw = (int)((((r >> (16 * (id & 1))) & 0xFFFFu) * 5u) >> 16);
#if defined(POM_DIAG)
        mv = pom_policy_wave(st, E, id, m0, m1, actor, draw, sets, lane, t_last, t_acc);
#else
        mv = pom_policy_wave(st, E, id, m0, m1, actor, draw, sets, lane);
#endif
    }
    p.moves[slot] = mv;
    p.agent_mem[slot] = m0;
    p.agent_mem[4 * np + slot] = m1;
#if defined(POM_DIAG)
    POM_PSTAMP(POM_PP_STORE);
    /* a lane that skipped a phase books the wavefront's time on its next stamp: per phase, the lanes that ran it agree, so
     * take the largest (an idle wavefront's act phases read 0) */
    for (int k = 0; k < POM_PP_N; k++) {
        long long v = t_acc[k];
        for (int o = 32; o > 0; o >>= 1) {
            const long long w = __shfl_xor(v, o);
            v = w > v ? w : v;
        }
        t_acc[k] = v;
    }
    if (lane == 0 && p.diag)
        for (int k = 0; k < POM_PP_N; k++) p.diag[tile_id * POM_PP_N + k] += t_acc[k];
#endif
}

/* the stand-alone export (pom_batch_observe; VIEW: pom_batch_observe_view, the same with the fogged views of PomViewSpec on the
 * way out): a tile into LDS, then pom_observe_tile */
template <bool VIEW>
__device__ __forceinline__ void pom_observe_alone(const ObserveParams& p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POM_REC_DWORDS * 16];
    __shared__ uint4 stage[obs_stage_vecs(OBS_PASS_ENVS_ALONE)];
    const int lane = threadIdx.x;
    const int64_t tile_local = pom_xcd_tile_order(blockIdx.x, gridDim.x);
    const int64_t tile_id = p.block0 + tile_local;
    load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    /* The builtin, not inline asm: the compiler's own wait-count bookkeeping must SEE that the LDS-DMA rows have landed before the
     * pass loop begins — otherwise it assumes at the loop's head that they may still be in flight and puts an s_waitcnt vmcnt(0) in
     * front of the first tile read of EVERY pass, which (stores count in vmcnt too) waits for the previous pass's global stores:
     * 31 of a wavefront's 58 k cycles, profiles/r04_observe_pmc.txt.  0x0F70: vmcnt(0), the other counters left alone. */
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("" ::: "memory");
    pom_observe_tile<OBS_PASS_ENVS_ALONE, VIEW>(p, tile, stage, tile_id, lane);
}
__global__ __launch_bounds__(64) void pom_observe_kernel(ObserveParams p) { pom_observe_alone<false>(p); }
__global__ __launch_bounds__(64) void pom_observe_view_kernel(ObserveParams p) { pom_observe_alone<true>(p); }
/* pom_batch_observe_view with a PomCompactViewSpec: the same, with pom_observe_tile_compact as the way out.  A kernel of its own and
 * not a branch in the one above, which stays what it was */
__global__ __launch_bounds__(64) void pom_observe_compact_kernel(ObserveParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POM_REC_DWORDS * 16];
    __shared__ uint4 stage[obs_stage_vecs(OBS_PASS_ENVS_ALONE)];
    const int lane = threadIdx.x;
    const int64_t tile_id = p.block0 + pom_xcd_tile_order(blockIdx.x, gridDim.x);
    load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    __builtin_amdgcn_s_waitcnt(0x0F70); /* as pom_observe_alone */
    asm volatile("" ::: "memory");
    pom_observe_tile_compact(p, tile, stage, tile_id, lane);
}

/* every env's first board (episode 0) into its state and snapshot columns, through an LDS tile so that the records leave in
 * the tick's coalesced row groups */
__global__ __launch_bounds__(64) void pom_generate_kernel(uint32_t* state, uint32_t* snap, uint32_t* episode, int64_t n, int64_t np,
                                                          int64_t env_offset, uint64_t board_seed)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POM_REC_DWORDS * 16];
    const int lane = threadIdx.x;
    const int64_t tile_id = blockIdx.x;
    if (tile_id * 16 + 16 > n) { /* the last, partial tile: its unused columns leave as blank records */
        for (int k = lane; k < POM_REC_DWORDS * 4; k += 64) reinterpret_cast<uint4*>(tile)[k] = make_uint4(0, 0, 0, 0);
        __syncthreads();
    }
    for (int ec = 0; ec < 16 && tile_id * 16 + ec < n; ec++)
        pom_boardgen_wave<16, POM_REC_DWORDS>(tile, ec, pom_board_key(board_seed, (uint32_t)(env_offset + tile_id * 16 + ec), 0u), lane);
    if (tile_id * 16 + lane < n && lane < 16) episode[tile_id * 16 + lane] = 0u;
    __syncthreads();
    /* whole tiles: the buffers hold n_pad columns; columns past n are blank records here, as after creation */
    store_tile16_x4(state + tile_id * POM_TILE_DWORDS, tile, lane);
    for (int ec = 0; ec < 16; ec++) { /* the snapshot: array of structs (restart_column); columns past n are blank like the state's */
        column_to_record<16>(tile, ec, snap + (tile_id * 16 + ec) * POM_REC_DWORDS, lane);
    }
}

/* ---- boundary kernels: States in and out, the one-State call, status, snapshot */
#include "pom_boundary.h"

__global__ __launch_bounds__(1024) void pom_reduce_counters_kernel(const int64_t* __restrict__ wc, int64_t n_waves, int64_t* out)
{
    /* one workgroup of 1,024 lanes: 4,096 wavefront slots are four independent 32-byte loads per lane (the kernel sits at
     * the end of a caller's timed region, after the sub-streams' join: a 256-lane loop of 16 dependent trips took 5-10 us) */
    __shared__ long long part[POM_CNT_N][16];
    long long acc[POM_CNT_N] = {0, 0, 0, 0};
    for (int64_t w = threadIdx.x; w < n_waves; w += blockDim.x) {
        const longlong2 lo = *reinterpret_cast<const longlong2*>(wc + w * POM_CNT_N);
        const longlong2 hi = *reinterpret_cast<const longlong2*>(wc + w * POM_CNT_N + 2);
        acc[0] += lo.x; acc[1] += lo.y; acc[2] += hi.x; acc[3] += hi.y;
    }
    static_assert(POM_CNT_N == 4, "two 16-byte loads per slot");
    for (int k = 0; k < POM_CNT_N; k++)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < POM_CNT_N; k++) part[k][threadIdx.x >> 6] = acc[k];
    __syncthreads();
    if (threadIdx.x < POM_CNT_N) {
        long long t = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); i++) t += part[threadIdx.x][i];
        out[threadIdx.x] = t;
    }
}

#endif /* POM_KERNELS_H_ */
