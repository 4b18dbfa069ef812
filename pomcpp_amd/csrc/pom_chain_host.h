/*
 * pom_chain_host.h — the host half of chained launches (pom_chain.h says what they are and sets them up): a several-tick call as
 * chained launches (launch_many_chain), and the check and recovery behind them (chain_settle), which every call that reads or
 * changes the batch goes through (quiesce, pom_handle.h).
 */
#ifndef POM_CHAIN_HOST_H_
#define POM_CHAIN_HOST_H_

#include "pom_issue.h"

#ifndef POM_CHAIN_LONG_CALL
#define POM_CHAIN_LONG_CALL 50
#endif

/* The check behind chained launches, and the recovery (pom_chain.h).  Joins the streams, lists the tiles some visitor could not
 * play (poisoned: their records stand on the last tick they really played), waits for the answer, and plays the missing ticks of
 * each such tile again — ordinary one-tile, one-tick launches of the twin kernel without the chain, with the parameters the
 * chained call was launched with (the log), on the caller's stream.  Afterwards every tile stands on the tick the host thinks it
 * does.  Costs one synchronisation of the caller's stream; free while there have been no chained launches since the last one. */
static int chain_settle(PomBatch* h)
{
    PomChain* c = &h->chain;
    if (!c->unverified || !c->ok) return POM_OK;
    if (int jr = join_parts(h)) return jr;
    const int64_t tiles = c->tiles;
    HIPCHK(hipMemsetAsync(c->aux + 1, 0, 4, h->stream));
    pom_chain_verify_kernel<<<dim3((unsigned)((tiles + 255) / 256)), dim3(256), 0, h->stream>>>(c->tile_seq, tiles, c->visits, c->aux);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->aux_host, c->aux, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    c->unverified = false;
    c->stat_settles++;
    const uint32_t flags = c->aux_host[0], bad = c->aux_host[1];
    if (!flags && !bad) {
        c->log.clear();
        return POM_OK;
    }
    if ((flags & POM_CHAIN_E_UNEVEN) || bad > (uint32_t)tiles) { /* not a tile left behind: launches that did not cover the tiles as assumed */
        c->ok = false;
        c->log.clear();
        snprintf(g_err, sizeof g_err, "chained launches did not visit every tile once (flags %u): the batch is in an undefined state — upload again "
                 "or destroy it; the handle launches sub-batches from here on", flags);
        return POM_E_HIP;
    }
    uint32_t* const list = new (std::nothrow) uint32_t[(size_t)2 * bad + 2]; /* (nothing may throw across the C boundary) */
    if (!list) {
        c->unverified = true; /* nothing has been replayed: the next call tries again */
        snprintf(g_err, sizeof g_err, "out of host memory while catching up tiles left behind by chained launches");
        return POM_E_NOMEM;
    }
    struct Free {
        uint32_t* p;
        ~Free() { delete[] p; }
    } free_list{list};
    /* from here on a failing runtime call leaves tiles half caught up: the handle says so instead of pretending otherwise (a retry
     * would replay from the old counts and play ticks twice) */
    struct Undefined {
        PomChain* c;
        bool armed;
        ~Undefined()
        {
            if (armed) {
                c->ok = false;
                c->log.clear();
            }
        }
    } undefined{c, true};
    if (bad) HIPCHK(hipMemcpy(list, c->aux + 2, (size_t)bad * 8, hipMemcpyDeviceToHost));
    if (getenv("POM_CHAIN_VERBOSE"))
        fprintf(stderr, "pom: chained launches left %u tile(s) behind (flags %u: %s%s%s); replaying their ticks\n", bad, flags,
                (flags & POM_CHAIN_E_TIMEOUT) ? "a wavefront waited out its limit " : "", (flags & POM_CHAIN_E_XCD) ? "a tile changed its XCD " : "",
                (flags & POM_CHAIN_E_TAPE) ? "a ticket outside the move tape" : "");
    PomRun replay; /* one launch of one tile */
    replay.grid = 1;
    replay.st = h->stream;
    replay.count = 1;
    for (uint32_t k = 0; k < bad; k++) {
        const uint32_t tile = list[2 * k], stored = list[2 * k + 1];
        for (uint32_t v = stored; v != c->visits; v++) {
            const PomChainCall* call = nullptr;
            for (const PomChainCall& e : c->log)
                if (v - e.visit0 < e.launches) call = &e;
            if (!call) { /* cannot happen: every chained launch since the last settle is in the log */
                snprintf(g_err, sizeof g_err, "a tile left behind by chained launches cannot be replayed: the batch is in an undefined state");
                return POM_E_HIP;
            }
            StepParams& q = replay.p;
            q = call->p;
            const uint32_t d = v - q.chain_seq0; /* visits after the call's first */
            q.block0 = tile;
            q.block_end = (int64_t)tile + 1;
            q.ticks = 1;
            q.tick0 += d;
            q.tick_base = h->tick_words + PomBatch::MAX_PARTS;
            if (q.moves) q.moves += (int64_t)d * q.n * 4;
            q.tile_seq = nullptr;
            q.chain_err = nullptr;
            q.chain_seq0 = 0;
            q.tape_len = 0;
            replay.kernel = step_kernel(h, call->policy, 1, false, false); /* the chained kernel's twin */
            int queued = 0;
            HIPCHK(issue_run(h, replay, 0, 1, false, &queued));
            c->stat_ticks_replayed++;
        }
        c->stat_tiles_recovered++;
    }
    /* the words start over: every tile is level again; only now are the flags that asked for this forgotten */
    HIPCHK(hipMemsetAsync(c->tile_seq, 0, (size_t)tiles * 8 * POM_CHAIN_WORD_STRIDE, h->stream));
    HIPCHK(hipMemsetAsync(c->aux, 0, 4, h->stream));
    undefined.armed = false;
    c->visits = 0;
    c->log.clear();
    if (flags & (POM_CHAIN_E_XCD | POM_CHAIN_E_TAPE)) c->ok = false; /* structural, not a matter of timing: no more chained launches on this handle */
    return POM_OK;
}

/* chain_setup for a handle (pom_batch_create, or the first chained call of a handle that was not created for them); where chained
 * launches cannot be had the handle launches sub-batches, and POM_CHAIN_VERBOSE says so */
static bool chain_setup_for(PomBatch* h)
{
    const bool ok = chain_setup(&h->chain, h->n_pad / h->epw, h->stream);
    if (!ok && getenv("POM_CHAIN_VERBOSE"))
        fprintf(stderr, "pom: chained launches are not available on this device (allocation failed or the workgroup -> XCD probe did not find the "
                        "eight-XCD round-robin); launching sub-batches\n");
    return ok;
}

/* POM_ISSUE_CHAIN (pom_chain.h): `launches` one-tick launches, each over the WHOLE batch, dealt round-robin to the handle's
 * streams; the tiles' ticket words order the ticks.  p0.moves != nullptr: a move tape of `launches` ticks.  *used = false: not
 * available for this handle, nothing was launched, the caller takes the ordinary path. */
static int launch_many_chain(PomBatch* h, const StepParams& p0, int launches, bool policy, bool* used)
{
    *used = false;
    PomChain* c = &h->chain;
    const int64_t tiles = h->n_pad / h->epw;
    if (!c->tried) { /* a handle that was not created for chained launches (pom_batch_set_streams made them possible later) */
        if (int jr = join_parts(h)) return jr;
        chain_setup_for(h);
    }
    if (!c->ok) return POM_OK;
    /* the fields of the tile words must not run into each other: after 2^27 visits (20 minutes of stepping) the words start over.
     * (POM_CHAIN_RESET_AT: a smaller number, so that tests get to see it happen).  The log of calls is bounded the same way. */
    static const uint64_t reset_at = getenv("POM_CHAIN_RESET_AT") ? (uint64_t)atoll(getenv("POM_CHAIN_RESET_AT")) : (uint64_t)(1u << 27);
    if ((uint64_t)c->visits + (uint64_t)launches >= (reset_at < (1u << 27) && reset_at > 0 ? reset_at : (uint64_t)(1u << 27)) || c->log.size() >= 256) {
        if (int sr = chain_settle(h)) return sr;
        if (!c->ok) return POM_OK;
        if (int jr = join_parts(h)) return jr;
        HIPCHK(hipMemsetAsync(c->tile_seq, 0, (size_t)tiles * 8 * POM_CHAIN_WORD_STRIDE, h->stream));
        c->visits = 0;
    }
    StepParams p = p0; /* the same for every launch of the call: which tick a wavefront plays follows from its ticket */
    p.block0 = 0;
    p.block_end = tiles;
    p.ticks = 1;
    p.tile_seq = c->tile_seq;
    p.chain_err = c->aux;
    p.chain_seq0 = c->visits;
    p.tape_len = p.moves ? (uint32_t)launches : 0u;
    p.chain_wait_limit = c->wait_limit;
    const PomStepKernel kernel = step_kernel(h, policy, 1, true, false);
    /* Launches in flight together must be interchangeable — "the j-th visitor of a tile plays the tile's j-th tick" holds only
     * if every launch would play that tick the same way: the same kernel, seed, move distribution, mode ... and the same offset
     * between ticks and visits.  A call that differs in any of that from the chained launches still in flight waits for them
     * (tests/test_gpu_chain.py: random sequences of calls with a seed of their own each).  A move tape belongs to its call: the
     * launches of a tape call never overlap another call's (and the tape was written on the caller's stream: the fork below
     * orders this call's launches behind it). */
    StepParams key = p;
    key.tick0 = p.tick0 - p.chain_seq0;
    key.chain_seq0 = 0;
    const bool continues = !p.moves && kernel == c->last_kernel && memcmp(&key, &c->last_key, sizeof key) == 0;
    if (h->forked && h->last_kind == POM_KIND_CHAIN && !continues)
        if (int jr = join_parts(h)) return jr;
    if (p.moves && h->forked)
        if (int jr = join_parts(h)) return jr;
    c->last_key = key;
    c->last_kernel = kernel;
    if (int rc = fork_parts(h, POM_KIND_CHAIN)) return rc;
    /* how many streams: a third launch in flight pays once the pipeline runs and costs while it fills and drains.  65,536 envs, us
     * per step on two / three streams at the round-4 kernels (with the rotation below on two): 30 ticks 10.47 / 11.13, 40 ticks
     * 10.20 / 10.76, 60 ticks 10.05 / 9.72, 100 ticks 9.79 / 9.64, 300 ticks 9.7 / 9.0.  Any mix is fine: the tickets order the
     * ticks, not the streams. */
    const int use = !h->chain_auto ? h->chain_parts : launches >= POM_CHAIN_LONG_CALL ? 3 : 2;
    /* On two streams, where one launch fills the chip's wavefront slots exactly (65,536 envs: 4,096 tiles, 16 slots on each of 256
     * CUs), every launch takes its XCD's tiles starting a sixteenth of them BEHIND where the launch before it started (a rotation
     * of the workgroup -> tile map: still every tile once per launch, still on its XCD).  With the same order in every launch the
     * two launches in flight meet on the same tiles more often than they must — the later visitor spins in a slot for the rest of
     * the earlier one's tick; short calls: 20 ticks 11.65 -> 11.31 us per step (ten runs each, medians; another box 11.75 -> 11.16),
     * 10 ticks 13.44 -> 13.08, 39 ticks unchanged.  Not on three streams (long calls: 9.0 -> 9.8 - 11.0 us, the launches there trail
     * each other by a whole cycle and the common order is what keeps them apart) and not at other sizes (32,768 and 16,384 envs: no
     * effect; 131,072: worse).  profiles/r04_chain_rotation.txt.  POM_CHAIN_ROT_DIV: the divisor (0: off). */
    static const int rot_div = getenv("POM_CHAIN_ROT_DIV") ? atoi(getenv("POM_CHAIN_ROT_DIV")) : 16;
    const uint32_t per_xcd = (uint32_t)(((tiles + POM_WPB - 1) / POM_WPB + 7) / 8);
    const bool fills_the_chip = c->wave_slots > 0 && tiles <= c->wave_slots && tiles * 4 >= (int64_t)c->wave_slots * 3;
    const uint32_t back = (use == 2 && fills_the_chip && rot_div > 0) ? per_xcd / (uint32_t)rot_div : 0u;
    h->chain_last_use = use;
    PomRun runs[PomBatch::MAX_PARTS];
    for (int r = 0; r < use; r++) { /* the call's launch i goes to stream (turn + i) % use: run r holds launches r, r + use, ... */
        runs[r].kernel = kernel;
        runs[r].grid = per_xcd * 8; /* a multiple of 8: every XCD gets as many workgroups as it has tiles */
        runs[r].part = (int)((c->turn + (uint32_t)r) % (uint32_t)use);
        runs[r].st = part_stream(h, runs[r].part, use);
        runs[r].p = p;
        runs[r].first = r;
        runs[r].stride = use;
        runs[r].count = launches > r ? (launches - r + use - 1) / use : 0;
        runs[r].rot0 = c->visits;
        runs[r].rot_mul = per_xcd - back;
        runs[r].rot_mod = back ? per_xcd : 0u;
    }
    /* Who issues: with the helper threads (the ones sub-batch launches use: created on first use, spinning for a millisecond after
     * pom_batch_fork / a job; issue_runs).  A launch costs the host 2.5 - 3 us, sometimes 6 - 9: with one thread a 20-step call is
     * queued in 50 - 60 us on most runs and in 120 - 180 us on one in five, late enough for the device to wait for its launches
     * (profiles/r05_issue_helpers.txt).  Any interleaving is fine: the tiles' tickets order the ticks, not the launches' order. */
    static const bool helpers_on = !(getenv("POM_CHAIN_HELPERS") && atoi(getenv("POM_CHAIN_HELPERS")) == 0);
    const bool helpers = helpers_on && !h->profiling && use >= 2 && launches >= 3 * use && !h->issuers_failed;
    hipError_t err = hipSuccess;
    const int issued = issue_runs(h, runs, use, helpers, &err);
    c->turn += (uint32_t)issued;
    /* what was issued is accounted for even if a launch failed half-way: the tiles' words, the log and the host's tick agree */
    if (issued > 0) {
        if (continues && !c->log.empty() && c->log.back().visit0 + c->log.back().launches == c->visits && c->log.back().policy == policy) {
            c->log.back().launches += (uint32_t)issued; /* the same play goes on: one entry */
        } else {
            PomChainCall e;
            e.visit0 = c->visits;
            e.launches = (uint32_t)issued;
            e.p = p;
            e.policy = policy;
            c->log.push_back(e);
        }
        c->visits += (uint32_t)issued;
        c->stat_launches += issued;
        c->unverified = true;
        h->tick += (uint64_t)issued;
    }
    *used = true;
    if (err != hipSuccess) {
        snprintf(g_err, sizeof g_err, "pom_step_kernel launch: %s (%d of the call's %d ticks were queued and will be played; the rest were not)",
                 hipGetErrorString(err), issued, launches);
        return POM_E_HIP;
    }
    return POM_OK;
}

#endif /* POM_CHAIN_HOST_H_ */
