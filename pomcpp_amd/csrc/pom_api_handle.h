/*
 * pom_api_handle.h — the entry points that make, describe and configure a handle rather than touch its games: the options checked
 * and the launch shape decided (create_plan), pom_batch_create / _destroy, the stream calls (fork, flush, sync, stream, set_streams),
 * the tick, and what the handle reports about its shape.
 */
#ifndef POM_API_HANDLE_H_
#define POM_API_HANDLE_H_

#include "pom_chain_host.h"

/* What pom_batch_create decides before it touches the runtime: the options as understood (a shorter struct_size is a prefix, the rest
 * zero) and the launch shape that follows from them and from the tuning overrides of the environment. */
struct PomPlan {
    PomBatchOptions o;
    int64_t n_pad;
    int epw;
    bool quad;
    int parts, main_part, issue_mode, chain_parts;
    bool fuse_policy, chain_auto;
};

/* Fills *pl from the arguments of pom_batch_create, or refuses them (POM_E_ARG, by that name).  No runtime call: a bad option is
 * refused as such on a machine without a device too. */
static int create_plan(PomBatch** out, int64_t n_envs, const PomBatchOptions* opts, PomPlan* pl)
{
    static const char who[] = "pom_batch_create";
    if (!out || n_envs <= 0 || n_envs > (int64_t)1 << 30) return refuse(who, "bad arguments");
    *out = nullptr; /* whatever follows: no handle unless the call succeeds */
    PomBatchOptions& o = pl->o;
    memset(&o, 0, sizeof o);
    o.mode = POM_MODE_ENV;
    if (opts) {
        if (opts->struct_size <= 0 || opts->struct_size > (int)sizeof o) return refuse(who, "options struct_size %d not understood", opts->struct_size);
        memcpy(&o, opts, (size_t)opts->struct_size);
    }
    if (o.mode != POM_MODE_RAW && o.mode != POM_MODE_ENV) return refuse(who, "bad mode %d", o.mode);
    if (o.auto_reset < POM_RESET_OFF || o.auto_reset > POM_RESET_AT_END)
        return refuse(who, "auto_reset must be 0 (off), 1 (at the start of the next tick) or 2 (at the end of the tick)");
    pl->n_pad = (n_envs + 63) / 64 * 64;
    /* Kernel shape.  Default: the quad kernel (16 envs per wavefront, 4 adjacent lanes per env) — fastest at every batch
     * size measured (profiles/r01_quad.txt).  The one-lane-per-env variants (64 / 32 / 16 envs per wavefront) stay
     * selectable; all produce identical results. */
    pl->epw = 16;
    pl->quad = true;
    if (o.lanes_per_env != 0 && o.lanes_per_env != 1 && o.lanes_per_env != 4) return refuse(who, "lanes_per_env must be 0, 1 or 4");
    if (o.envs_per_wave != 0 && o.envs_per_wave != 16 && o.envs_per_wave != 32 && o.envs_per_wave != 64)
        return refuse(who, "envs_per_wave must be 0, 16, 32 or 64");
    if (o.envs_per_wave != 0) {
        pl->epw = o.envs_per_wave;
        pl->quad = pl->epw == 16 && o.lanes_per_env != 1;
    } else if (o.lanes_per_env == 1) {
        pl->quad = false;
        pl->epw = pl->n_pad <= 8192 ? 16 : 32;
    }
    if (o.lanes_per_env == 4 && !pl->quad) return refuse(who, "lanes_per_env 4 needs envs_per_wave 16 (or 0)");
    if (const char* ev = getenv("POM_EPW")) { /* tuning overrides for sweeps */
        const int v = atoi(ev);
        if (v == 16 || v == 32 || v == 64) {
            pl->epw = v;
            pl->quad = false;
        }
    }
    if (const char* ev = getenv("POM_QUAD")) pl->quad = atoi(ev) != 0 && pl->epw == 16;
    /* sub-batches per step: part 0 on the caller's stream, the others on internal streams.  Measured on MI355X at 65,536
     * envs: one launch 26.4 us, two parts 22.3, three 20.4; FOUR concurrent streams of one process serialize on this stack
     * (36 us; profiles/r01_streams.txt), and other streams of the process (RCCL) count against that budget, so the default
     * stays at three only for batches where it matters and a caller can measure (pom_batch_set_streams, as bench.py does). */
    pl->parts = pl->n_pad >= 49152 ? 3 : pl->n_pad >= 8192 ? 2 : 1;
    if (o.streams >= 1 && o.streams <= PomBatch::MAX_PARTS) pl->parts = o.streams;
    else if (o.streams != 0) return refuse(who, "streams must be 0..%d", (int)PomBatch::MAX_PARTS);
    /* policy and tick in one kernel: faster at every batch size since the wavefront-cooperative searches (round 3: 33.7 / 39.0 /
     * 55.7 / 109.5 us per step fused against 42.2 / 47.9 / 62.8 / 112.8 as two kernels at 32,768 .. 262,144 envs).  Round 1
     * measured the two kernels 3 % ahead at 262,144 envs (profiles/r01_fuse.txt). */
    pl->fuse_policy = true;
    if (const char* ev = getenv("POM_FUSE")) pl->fuse_policy = atoi(ev) != 0;
    pl->main_part = 1;
    if (const char* ev = getenv("POM_MAIN_PART")) pl->main_part = atoi(ev) != 0;
    if (o.issue_mode < POM_ISSUE_AUTO || o.issue_mode > POM_ISSUE_CHAIN) return refuse(who, "issue_mode must be one of POM_ISSUE_*");
    /* AUTO: chained launches where they pay (measured up to 131,072 envs, even at 262,144: scripts/experiments/chain/sizes.sh)
     * and can be had (the one-tick replay shape: pom_handle.h runs_chain); the helper threads otherwise */
    pl->issue_mode = o.issue_mode != POM_ISSUE_AUTO ? o.issue_mode : (pl->quad && pl->n_pad <= 196608) ? POM_ISSUE_CHAIN : POM_ISSUE_THREADS;
    if (const char* ev = getenv("POM_ISSUE")) {
        if (!strcmp(ev, "direct")) pl->issue_mode = POM_ISSUE_DIRECT;
        else if (!strcmp(ev, "threads")) pl->issue_mode = POM_ISSUE_THREADS;
        else if (!strcmp(ev, "graph")) pl->issue_mode = POM_ISSUE_GRAPH;
        else if (!strcmp(ev, "chain")) pl->issue_mode = POM_ISSUE_CHAIN;
    }
    if (const char* ev = getenv("POM_STREAMS")) {
        const int v = atoi(ev);
        if (v >= 1 && v <= PomBatch::MAX_PARTS) pl->parts = v;
    }
    if ((int64_t)pl->parts > pl->n_pad / pl->epw) pl->parts = (int)(pl->n_pad / pl->epw);
    /* chained launches rotate over two streams (short calls) or three (long ones) unless the caller asked for a number (options /
     * POM_STREAMS / pom_batch_set_streams: then that many; one stream = launches in a row, nothing to chain) */
    pl->chain_auto = !(o.streams >= 1 || getenv("POM_STREAMS"));
    pl->chain_parts = pl->chain_auto ? 3 : pl->parts;
    if (const char* ev = getenv("POM_CHAIN_STREAMS")) {
        const int v = atoi(ev);
        if (v >= 1 && v <= PomBatch::MAX_PARTS) {
            pl->chain_parts = v;
            pl->chain_auto = false;
        }
    }
    if (o.auto_reset == POM_RESET_AT_END && !pl->quad)
        return refuse(who, "auto_reset = POM_RESET_AT_END is built for the default kernel shape (envs_per_wave 16, lanes_per_env 4) only");
    return POM_OK;
}

extern "C" {

const char* pom_last_error(void) { return g_err; }

int pom_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pom_batch_destroy(PomBatch* h)
{
    if (int rc = check_call(h, "pom_batch_destroy")) return rc;
    stop_issuers(h);
    (void)hipSetDevice(h->device);
    for (int k = 0; k < PomBatch::MAX_PARTS; k++)
        if (h->sub[k]) (void)hipStreamSynchronize(h->sub[k]);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    chain_destroy(&h->chain); /* after the streams have drained: launches in flight still use the tiles' words */
    drop_graphs(h);
    for (int k = 0; k < PomBatch::MAX_PARTS; k++) {
        if (h->sub[k]) (void)hipStreamDestroy(h->sub[k]);
        if (h->ev_join[k]) (void)hipEventDestroy(h->ev_join[k]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (int k = 0; k < 2 * PomBatch::PROF_RING; k++)
        if (h->prof_ev[k]) (void)hipEventDestroy(h->prof_ev[k]);
    (void)hipFree(h->state);
    (void)hipFree(h->snap);
    (void)hipFree(h->terminal);
    (void)hipFree(h->moves_dev);
    (void)hipFree(h->agent_mem);
    (void)hipFree(h->episode);
    (void)hipFree(h->staging);
    (void)hipFree(h->copy_scratch);
    (void)hipFree(h->copy_idx);
    (void)hipFree(h->wave_counters);
    (void)hipFree(h->totals_dev);
    (void)hipFree(h->first_bad);
    (void)hipFree(h->tick_words);
    if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return POM_OK;
}

int pom_batch_create(PomBatch** out, int64_t n_envs, const PomBatchOptions* opts)
{
    PomPlan pl;
    if (int rc = create_plan(out, n_envs, opts, &pl)) return rc;
    const PomBatchOptions& o = pl.o;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (o.device < 0 || o.device >= ndev) {
        snprintf(g_err, sizeof g_err, "pom_batch_create: device %d of %d", o.device, ndev);
        return POM_E_HIP;
    }
    HIPCHK(hipSetDevice(o.device));
    PomBatch* h = new (std::nothrow) PomBatch();
    if (!h) return POM_E_NOMEM;
    struct Guard { /* whatever fails from here on: the handle and what it holds so far are released */
        PomBatch* h;
        ~Guard()
        {
            if (h) pom_batch_destroy(h);
        }
    } guard{h};
    h->device = o.device;
    h->n = n_envs;
    h->n_pad = pl.n_pad;
    h->n_waves = h->n_pad / 16;
    h->epw = pl.epw;
    h->quad = pl.quad;
    h->parts = pl.parts;
    h->main_part = pl.main_part;
    h->issue_mode = pl.issue_mode;
    h->chain_parts = pl.chain_parts;
    h->chain_auto = pl.chain_auto;
    h->fuse_policy = pl.fuse_policy;
    h->mode = o.mode;
    h->auto_reset = o.auto_reset;
    h->max_steps = o.max_steps;
    h->env_offset = o.env_offset;
    h->fresh = o.fresh_boards != 0;
    h->board_seed = o.board_seed;
    h->staging_envs = h->n_pad < 16384 ? h->n_pad : 16384;
    if (o.stream) {
        h->stream = (hipStream_t)o.stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            set_err("hipStreamCreate", e);
            return POM_E_HIP;
        }
        h->own_stream = true;
    }
    if (ensure_sub_streams(h, streams_for(h, 0)) != POM_OK) return POM_E_HIP; /* what its usual launches need; the rest when first needed */
    /* the handle's arrays.  Zeroed: all-zero records are inert blank boards; padded envs are marked finished */
    const size_t rec_bytes = (size_t)POM_REC_DWORDS * 4 * (size_t)h->n_pad;
    const struct {
        void** ptr;
        size_t bytes;
        bool zeroed;
    } arrays[] = {
        {(void**)&h->state, rec_bytes, true},
        {(void**)&h->snap, rec_bytes, true},
        {(void**)&h->moves_dev, (size_t)h->n_pad * 16, true},
        {(void**)&h->staging, (size_t)h->staging_envs * POM_STATE_BYTES, false},
        {(void**)&h->wave_counters, (size_t)h->n_waves * POM_CNT_N * 8, true},
        {(void**)&h->totals_dev, POM_CNT_N * 8, false},
        {(void**)&h->first_bad, sizeof(int), false},
        {(void**)&h->episode, (size_t)h->n_pad * 4, true},
        {(void**)&h->tick_words, (PomBatch::MAX_PARTS + 1) * sizeof(uint32_t), true},
        {(void**)&h->terminal, h->auto_reset == POM_RESET_AT_END ? rec_bytes : 0, true},
    };
    for (const auto& a : arrays) {
        if (!a.bytes) continue;
        const hipError_t e = hipMalloc(a.ptr, a.bytes);
        if (e != hipSuccess) {
            set_err("hipMalloc", e);
            return e == hipErrorOutOfMemory ? POM_E_NOMEM : POM_E_HIP;
        }
    }
    hipError_t e = hipSuccess;
    for (const auto& a : arrays)
        if (a.bytes && a.zeroed && e == hipSuccess) e = hipMemsetAsync(*a.ptr, 0, a.bytes, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        set_err("initial memset", e);
        return POM_E_HIP;
    }
    /* chained launches: the tiles' words and the probe of the workgroup -> XCD pattern, here rather than in the first step (the
     * probe synchronises the stream); where they cannot be had the handle launches sub-batches */
    if (chains(h)) chain_setup_for(h);
    guard.h = nullptr;
    *out = h;
    return POM_OK;
}

int64_t pom_batch_size(const PomBatch* h) { return h ? h->n : -1; }

int pom_batch_set_streams(PomBatch* h, int32_t streams)
{
    static const char who[] = "pom_batch_set_streams";
    if (int rc = begin_call(h, who, POM_SETTLED, streams < 1 || streams > PomBatch::MAX_PARTS ? "streams must be 1..8" : nullptr)) return rc;
    const int64_t tiles = h->n_pad / h->epw;
    const int want = (int64_t)streams > tiles ? (int)tiles : streams;
    if (int er = ensure_sub_streams(h, streams)) return er;
    h->parts = want;
    h->chain_parts = streams; /* chained launches cover all tiles: their stream count is not bounded by the tiles */
    h->chain_auto = false;
    return POM_OK;
}
static_assert(PomBatch::MAX_PARTS == 8, "pom_batch_set_streams says so in its refusal");

int pom_batch_set_tick(PomBatch* h, int64_t tick)
{
    if (int rc = check_call(h, "pom_batch_set_tick", tick < 0 ? "tick must be >= 0" : nullptr)) return rc;
    h->tick = (uint64_t)tick;
    return POM_OK;
}

int pom_batch_stream(PomBatch* h, void** stream)
{
    if (int rc = check_call(h, "pom_batch_stream", !stream ? "stream is NULL" : nullptr)) return rc;
    *stream = (void*)h->stream;
    return POM_OK;
}

int pom_batch_fork(PomBatch* h)
{
    if (int rc = begin_call(h, "pom_batch_fork", POM_AS_IS)) return rc;
    for (int k = 0; k < PomBatch::MAX_PARTS; k++) /* the issuing threads of multi-tick calls: work is coming, stay awake for it */
        if (h->issuers[k]) {
            h->issuers[k]->posted.fetch_add(1, std::memory_order_release);
            h->issuers[k]->cv.notify_all();
        }
    return fork_parts(h, 0);
}

int pom_batch_flush(PomBatch* h) { return begin_call(h, "pom_batch_flush", POM_JOINED); }

int pom_batch_sync(PomBatch* h)
{
    if (int rc = begin_call(h, "pom_batch_sync", POM_SETTLED)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return POM_OK;
}

int pom_batch_launch_shape(PomBatch* h, int32_t* envs_per_wave, int32_t* lanes_per_env, int32_t* launches_per_step)
{
    if (int rc = check_call(h, "pom_batch_launch_shape")) return rc;
    if (envs_per_wave) *envs_per_wave = h->epw;
    if (lanes_per_env) *lanes_per_env = h->quad ? 4 : 1;
    if (launches_per_step) *launches_per_step = runs_chain(h, 1) ? 1 : h->parts; /* chained: one launch over all tiles per tick */
    return POM_OK;
}

int pom_batch_issue_info(PomBatch* h, int32_t* issue_mode, int32_t* streams)
{
    if (int rc = check_call(h, "pom_batch_issue_info")) return rc;
    const bool chained = runs_chain(h, 1);
    if (issue_mode) *issue_mode = h->issue_mode == POM_ISSUE_CHAIN && !chained ? POM_ISSUE_THREADS : h->issue_mode;
    if (streams) *streams = !chained ? h->parts : h->chain_auto ? h->chain_last_use : h->chain_parts;
    return POM_OK;
}

} /* extern "C" */

#endif /* POM_API_HANDLE_H_ */
