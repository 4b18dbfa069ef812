/*
 * pom_step_mixed_body.inc — the body of the mixed step's kernel, included by pom_step_mixed.h once for each of its two __global__
 * functions: pom_step_mixed_kernel (POM_STEP_MIXED_EVENTS 0) and pom_step_events_kernel (1, with the StepEventsOut eo beside p).  It
 * is an include and not a function that both call because the compiler does not give an inlined __device__ function's kernel the
 * instructions it gives the same text written in the kernel (a handful differ, scripts/compare_kernel_isa.py), and
 * pom_batch_step_mixed's kernels stay what they were.  No include guard: it is meant to be included twice.
 */
    static_assert(!VIEW || OBS, "the fogged views are a kind of fused observation");
    constexpr int EPW = 16;
    constexpr int OBS_ROWS = (obs_stage_vecs(OBS_PASS_ENVS_FUSED) * 16 + 63) / 64;
    constexpr int OVERLAY = OBS && OBS_ROWS > 44 ? OBS_ROWS : 44; /* the policy's rows and the export's staging rows, one over the other */
    constexpr int ROWS = POM_REC_DWORDS + OVERLAY > LDS_ROWS ? POM_REC_DWORDS + OVERLAY : LDS_ROWS;
    __shared__ __attribute__((aligned(16))) uint32_t tile[ROWS * EPW];
    /* & 63, as pom_step_kernel has it: the compiler works out the value ranges of the shared bodies' arguments over ALL their callers
     * before it inlines them, and a caller that hands the fogged export a lane id of 0..1023 changes the code of the VIEW step kernels
     * (a 16-bit division where they had an 8-bit one) */
    const int lane = threadIdx.x & 63;
    const int64_t tile_id = p.block0 + pom_xcd_tile_order(blockIdx.x, gridDim.x);
    const int64_t np = p.n_pad;
    const bool env_mode = p.mode == POM_MODE_ENV;
    /* lane -> (env lane / 4, agent lane % 4) */
    const int ec = lane >> 2, member = lane & 3;
    const int64_t e = tile_id * EPW + ec;
    const bool owner = member == 0;
    const bool valid = e < p.n;
    const uint32_t env_key = (uint32_t)(p.env_offset + e); /* the env's number in the whole job: what its draw is keyed by */
    uint32_t* t = tile + ec;
    uint8_t* const danger = reinterpret_cast<uint8_t*>(tile + POM_REC_DWORDS * EPW);
    uint32_t* const sets = tile + (POM_REC_DWORDS + 32) * EPW;
    const bool simple = (p.simple_mask >> member) & 1; /* this lane's agent plays SimpleAgent */
    const bool has_mem = p.agent_mem != nullptr;       /* wave-uniform */

    long long c_steps = 0, c_episodes = 0, c_resets = 0, c_ub = 0;

    load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    /* neither the memory nor the caller's move depends on the record: fetch them while it is on its way (the buffers hold n_pad
     * columns of memory; the moves are the caller's n rows) */
    uint32_t m0 = 0, m1 = 0;
    if (has_mem) {
        m0 = p.agent_mem[tile_id * 64 + lane];
        m1 = p.agent_mem[4 * np + tile_id * 64 + lane];
    }
    int mine0 = POM_MOVE_IDLE;
    if (valid && !simple) mine0 = p.moves[tile_id * 64 + lane]; /* Move[4] of env e, agent lane % 4: dead agents' entries included */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the DMA rows have landed (one wavefront per workgroup: no barrier) */
    PomLane L;
    int time_step = 0;
    uint32_t status = 0;
    /* as pom_step_kernel: where restarts happen at the start of the tick the status byte alone is looked at first, and the register
     * rows are unpacked once, behind the restarts */
    constexpr bool UNPACK_LATE = !ATEND;
    if (UNPACK_LATE) status = t[(POM_REC_AGENTS + 3) * EPW] >> 24; /* (as pom_lane_load reads it) */
    else lane_from_tile(L, time_step, status, t, EPW);
    pom_lane_diag_off(L);
    bool restarted = false;

    if (ATEND) {
        /* POM_RESET_AT_END: nobody is finished when a tick begins; see the end of the tick */
    } else if (FRESH) {
        /* a finished env starts its next game on the board (board_seed, env, games played), drawn into its column by the whole wavefront */
        const bool reload = valid && env_mode && p.auto_reset == POM_RESET_AT_START && (status & POM_ST_DONE);
        uint64_t todo = __ballot(reload && owner);
        while (todo) {
            const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1); /* an owner lane */
            todo &= todo - 1;
            const int ec_u = src >> 2;
            uint32_t ep = 0;
            if (lane == src) {
                ep = p.episode[e] + 1u;
                p.episode[e] = ep;
            }
            ep = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)ep, src));
            const uint32_t key = pom_board_key(p.board_seed, (uint32_t)(p.env_offset + tile_id * EPW + ec_u), ep);
            pom_boardgen_wave<EPW, POM_REC_DWORDS>(tile, ec_u, (uint32_t)__builtin_amdgcn_readfirstlane((int)key), lane);
        }
        asm volatile("" ::: "memory"); /* other lanes wrote this lane's column: no read of it may be scheduled earlier */
        restarted = reload;
        c_resets += __popcll(__ballot(reload && owner));
    } else {
        /* a finished env restarts from its snapshot, one restarting env after the other, by the whole wavefront */
        const bool reload = valid && env_mode && p.auto_reset == POM_RESET_AT_START && (status & POM_ST_DONE);
        uint64_t todo = __ballot(reload && owner);
        if (todo) {
            c_resets += __popcll(todo);
            do {
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1); /* an owner lane */
                todo &= todo - 1;
                const int ec_u = src >> 2;
                restart_column<EPW>(tile, ec_u, p.snap + (tile_id * EPW + ec_u) * POM_REC_DWORDS, lane);
            } while (todo);
            asm volatile("" ::: "memory"); /* other lanes wrote this lane's column: no read of it may be scheduled earlier */
        }
        restarted = reload;
    }
    if (UNPACK_LATE) lane_from_tile(L, time_step, status, t, EPW); /* every lane's register rows, restarted or not */
    const bool active = valid && !(env_mode && (status & POM_ST_DONE));
    bool newly_done = false, new_ub = false;
#if POM_STEP_MIXED_EVENTS
    /* S0 is what stands in the tile now.  The lane's agent's two words, and the tile's wood cells if they are asked for (wave-uniform) */
    const int ev_a0 = sel4(member, L.a0), ev_a1 = (int)t[(POM_REC_AGENTS + 1 + 2 * member) * EPW];
    const uint32_t ev_wood = eo.wood ? pom_wood_bits(tile, lane) : 0u;
#endif

    /* the moves: the policy's for the mask's agents, the caller's for the others */
    int mine = mine0;
    if (has_mem) {
        if (restarted) m0 = m1 = 0; /* a new game gets fresh agents: all four, in the mask or not */
        if (p.simple_mask) { /* wave-uniform: with nobody to ask the whole policy is skipped */
            LdsEnv<EPW, 4> accp(tile, ec, member);
            PolicyStore st{tile, t, danger + ec, sets + ec, member};
            const PomPolicyEnv E{{L.a0[0], L.a0[1], L.a0[2], L.a0[3]}, {accp.ag1(0), accp.ag1(1), accp.ag1(2), accp.ag1(3)}, L.bIdx, L.bCnt};
            if (active) { /* all four lanes of the env, dead agents' lanes and those outside the mask included: the env's map is theirs too */
                pom_policy_prepare_clear(st);
                pom_policy_prepare_fill(st, E);
                pom_policy_prepare_safe(st);
            }
            /* act() is only asked of live agents (environment.cpp:139-146), and here only of the mask's; the wavefront's searches run
             * together: every lane goes in */
            const uint32_t r = pom_rng_draw_half(p.seed, env_key, p.tick, member >> 1);
            const bool actor = active && simple && !ag_dead(sel4(member, L.a0));
#if defined(POM_DIAG)
            long long pt_last = 0, pt_acc[POM_PP_N];
            const int mv_own = pom_policy_wave(st, E, member, m0, m1, actor, (int)((((r >> (16 * (member & 1))) & 0xFFFFu) * 5u) >> 16), sets, lane, pt_last, pt_acc);
#else
            const int mv_own = pom_policy_wave(st, E, member, m0, m1, actor, (int)((((r >> (16 * (member & 1))) & 0xFFFFu) * 5u) >> 16), sets, lane);
#endif
            if (simple) mine = mv_own; /* (IDLE for a dead agent of the mask) */
        }
        /* the memory does not stay in registers through the tick */
        p.agent_mem[tile_id * 64 + lane] = m0;
        p.agent_mem[4 * np + tile_id * 64 + lane] = m1;
    }
    if (active) {
        /* a fresh view of the tile for the tick: keeps the compiler from computing the tick's addresses before the policy and carrying
         * them through it (as pom_step_kernel<POLICY>) */
        uint32_t* t2 = tile;
        asm volatile("" : "+v"(t2));
        LdsEnv<EPW, 4> acc2(t2, ec, member);
        PomStepper<LdsEnv<EPW, 4>> stepper2(acc2, L);
        const uint32_t mvp = stepper2.pack_moves_quad(mine);
        L.ub = 0; /* this tick's flags; the record's (in the top bytes of two agent words, untouched by the tick) are added afterwards */
        status &= ~(uint32_t)POM_ST_RESTARTED;
        stepper2.step_packed(mvp);
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
#if POM_STEP_MIXED_EVENTS
    /* S1 is what stands in the tile and in L now: the restart at the end has not happened yet.  (The agents' second words and the
     * board were written by whichever lane of the quad the tick gave the work to: no read of them may be scheduled earlier) */
    asm volatile("" ::: "memory");
    uint32_t ev_word = ag_dead(ev_a0) ? 0u : (uint32_t)POM_EV_ALIVE; /* an env that is not ticked */
    if (active)
        ev_word = pom_event_word(ev_a0, ev_a1, sel4(member, L.a0), (int)t[(POM_REC_AGENTS + 1 + 2 * member) * EPW],
                                 PomStepper<LdsEnv<EPW, 4>>::clamp_move(mine), member, restarted, newly_done, status, new_ub);
    if (valid) eo.events[tile_id * 64 + lane] = ev_word;
    if (eo.outcome && valid && owner) {
        const uint32_t ts = t[POM_REC_TIMESTEP * EPW];
        eo.outcome[e] = pom_rollout_word(L, status, new_ub, ts < 65535u ? ts : 65535u);
    }
    if (eo.wood) { /* wave-uniform: every lane scans, whatever its env did (an env that is not ticked burns nothing) */
        const uint32_t burnt = pom_wood_burnt(ev_wood, pom_wood_bits(tile, lane), ec);
        if (valid && owner) eo.wood[e] = (uint8_t)burnt;
    }
#endif
    if (ATEND) {
        /* the tick that finishes an episode also starts the next one (pom_step_kernel): the final record goes to the terminal buffer, the
         * env's column is replaced by its start state, the agents' memory is wiped, the env is marked POM_ST_RESTARTED */
        uint64_t todo = __ballot(newly_done && owner);
        if (todo) {
            c_resets += __popcll(todo);
            if (newly_done && owner) { /* the register-resident rows of the final record (timeStep is in the tile already) */
#pragma unroll
                for (int k = 0; k < 8; k++) t[(POM_REC_AGENTS + k) * EPW] = pom_lane_agent_word(L, status, k, t[(POM_REC_AGENTS + k) * EPW]);
            }
            asm volatile("" ::: "memory");
            int lane_end = lane; /* (a lane id the compiler cannot see through: the global addresses below are worked out here) */
            asm volatile("" : "+v"(lane_end));
            do {
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1); /* an owner lane */
                todo &= todo - 1;
                const int ec_u = src >> 2;
                const int64_t e_u = tile_id * EPW + ec_u;
                column_to_record<EPW>(tile, ec_u, p.terminal + e_u * POM_REC_DWORDS, lane_end);
                if (FRESH) {
                    uint32_t ep = 0;
                    if (lane == src) {
                        ep = p.episode[e_u] + 1u;
                        p.episode[e_u] = ep;
                    }
                    ep = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)ep, src));
                    const uint32_t key = pom_board_key(p.board_seed, (uint32_t)(p.env_offset + e_u), ep);
                    pom_boardgen_wave<EPW, POM_REC_DWORDS>(tile, ec_u, (uint32_t)__builtin_amdgcn_readfirstlane((int)key), lane_end);
                } else {
                    restart_column<EPW>(tile, ec_u, p.snap + e_u * POM_REC_DWORDS, lane_end);
                }
            } while (todo);
            asm volatile("" ::: "memory");
            if (newly_done) {
                lane_from_tile(L, time_step, status, t, EPW);
                status |= POM_ST_RESTARTED;
                if (has_mem) { /* a new game gets fresh agents: all four */
                    p.agent_mem[tile_id * 64 + lane_end] = 0u;
                    p.agent_mem[4 * np + tile_id * 64 + lane_end] = 0u;
                }
            }
        }
    }

    /* write back: the owner puts the register-resident rows into the tile, then the whole record leaves in row groups */
    if (owner) { /* (timeStep went into the tile with the tick's epilogue) */
#pragma unroll
        for (int k = 0; k < 8; k++) t[(POM_REC_AGENTS + k) * EPW] = pom_lane_agent_word(L, status, k, (k & 1) ? t[(POM_REC_AGENTS + k) * EPW] : 0u);
    }
    {
        int lane_late = lane; /* (a lane id the compiler cannot see through: the store addresses are worked out here, not carried through the tick) */
        asm volatile("" : "+v"(lane_late));
        store_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane_late);
    }
    if (OBS) {
        /* the observation of what the tick left in the tile, while the record's stores are on their way (they have been read out of LDS
         * into registers; the staging area lies behind the record rows, where the policy's maps were) */
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#if POM_STEP_MIXED_COMPACT
        const ObserveParams opc{nullptr, p.n, p.n_pad, 0, p.obs_planes, nullptr, p.obs_env_attrs, p.obs_dtype, 1, p.obs_viewer_attrs, p.obs_view_radius,
                                p.obs_view_compact};
        pom_observe_tile_compact(opc, tile, reinterpret_cast<uint4*>(tile + POM_REC_DWORDS * EPW), tile_id, lane);
#else
        const ObserveParams op{nullptr, p.n, p.n_pad, 0, p.obs_planes, p.obs_agent_attrs, p.obs_env_attrs, p.obs_dtype, p.obs_per_agent,
                               VIEW ? p.obs_viewer_attrs : nullptr, VIEW ? p.obs_view_radius : 0};
        pom_observe_tile<OBS_PASS_ENVS_FUSED, VIEW>(op, tile, reinterpret_cast<uint4*>(tile + POM_REC_DWORDS * EPW), tile_id, lane);
#endif
    }
    if (lane == 0) { /* each wavefront owns its slot; returnless atomics because those are fire-and-forget (pom_step_kernel) */
        unsigned long long* wc = reinterpret_cast<unsigned long long*>(p.wave_counters + tile_id * POM_CNT_N);
        __hip_atomic_fetch_add(&wc[POM_CNT_STEPS], (unsigned long long)c_steps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c_episodes) __hip_atomic_fetch_add(&wc[POM_CNT_EPISODES], (unsigned long long)c_episodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c_resets) __hip_atomic_fetch_add(&wc[POM_CNT_RESETS], (unsigned long long)c_resets, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c_ub) __hip_atomic_fetch_add(&wc[POM_CNT_UB_TICKS], (unsigned long long)c_ub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
