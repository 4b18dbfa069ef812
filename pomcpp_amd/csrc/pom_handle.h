/*
 * pom_handle.h — the batch handle at work, core unit only: the error text and the definitions of what pom_host.h declares for every
 * unit (set_err, refuse, check_range, check_call, begin_call, ensure_agent_mem), the handle's streams forked and joined, and the
 * parameters a step launch takes from the handle (fill_params).  The handle itself (PomBatch): pom_host.h.  Who launches what:
 * pom_issue.h.
 */
#ifndef POM_HANDLE_H_
#define POM_HANDLE_H_

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>

#include "pom_host.h"
#include "pom_kernels.h"
#include "pom_chain.h"

static thread_local char g_err[256] = ""; /* the one error text of the library: every unit writes it through set_err and refuse */
void set_err(const char* what, hipError_t e)
{
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
}
int refuse(const char* who, const char* fmt, ...)
{
    const int at = snprintf(g_err, sizeof g_err, "%s: ", who);
    va_list ap;
    va_start(ap, fmt);
    if (at > 0 && at < (int)sizeof g_err) vsnprintf(g_err + at, sizeof g_err - (size_t)at, fmt, ap);
    va_end(ap);
    return POM_E_ARG;
}

static void drop_graphs(PomBatch* h);
static void stop_issuers(PomBatch* h);
enum { POM_KIND_SPLIT = 1, POM_KIND_CHAIN = 2 };
static int fork_parts(PomBatch* h, int kind = POM_KIND_SPLIT);
static int join_parts(PomBatch* h);
static int ensure_sub_streams(PomBatch* h, int parts);
static int chain_settle(PomBatch* h);
/* before anything but another chained call reads or changes the batch: the chained launches are joined and checked, tiles that
 * could not be played in the chain are caught up (chain_settle), then the sub-streams are joined into the caller's stream */
static int quiesce(PomBatch* h)
{
    if (int rc = chain_settle(h)) return rc;
    return join_parts(h);
}

int check_range(const PomBatch* h, const char* who, int64_t first, int64_t count)
{
    if (!h || first < 0 || count < 0 || first + count > h->n)
        return refuse(who, "range [%lld, %lld) outside batch", (long long)first, (long long)(first + count));
    return POM_OK;
}

/* the start of every call on a handle (pom_host.h) */
int check_call(const PomBatch* h, const char* who, const char* what)
{
    if (!h) return refuse(who, "the handle is NULL");
    return what ? refuse(who, "%s", what) : POM_OK;
}
int begin_call(PomBatch* h, const char* who, PomNeeds needs, const char* what)
{
    if (int rc = check_call(h, who, what)) return rc;
    HIPCHK(hipSetDevice(h->device));
    return needs == POM_SETTLED ? quiesce(h) : needs == POM_JOINED ? join_parts(h) : POM_OK;
}

static int ensure_sub_streams(PomBatch* h, int parts)
{
    if (parts <= 1) return POM_OK;
    if (!h->ev_fork) HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    for (int k = 0; k < parts; k++) {
        if (!h->sub[k]) HIPCHK(hipStreamCreateWithFlags(&h->sub[k], hipStreamNonBlocking));
        if (!h->ev_join[k]) HIPCHK(hipEventCreateWithFlags(&h->ev_join[k], hipEventDisableTiming));
    }
    return POM_OK;
}

/* the handle issues its several-tick calls as chained launches (pom_chain.h) where they can be had: what it was created for */
static bool chains(const PomBatch* h) { return h->issue_mode == POM_ISSUE_CHAIN && h->quad && h->chain_parts > 1; }
/* ... and this call can: one tick per launch, and the chain set up (or not yet tried) */
static bool runs_chain(const PomBatch* h, int ticks_per_launch)
{
    return chains(h) && ticks_per_launch == 1 && !(h->chain.tried && !h->chain.ok);
}

/* how many streams launches of a kind use: the sub-batch parts, or the streams chained launches rotate over (kind 0: what the
 * handle's several-tick calls will mostly be) */
static int streams_for(const PomBatch* h, int kind)
{
    return kind == POM_KIND_CHAIN || (kind == 0 && chains(h)) ? h->chain_parts : h->parts;
}

/* The part plan of a sub-batch step: part k of `parts` covers the step kernel's tiles [*b0, *b1) (false: none) and runs on the
 * caller's stream (part 0 of a split step, main_part) or on sub-stream k.  Chained launches take stream k of the `parts` streams
 * they rotate over the same way. */
static bool part_tiles(const PomBatch* h, int k, int parts, int64_t* b0, int64_t* b1)
{
    const int64_t tiles = h->n_pad / h->epw;
    *b0 = tiles * k / parts;
    *b1 = tiles * (k + 1) / parts;
    return *b1 > *b0;
}
static hipStream_t part_stream(const PomBatch* h, int k, int parts)
{
    return parts == 1 || k < h->main_part ? h->stream : h->sub[k];
}

/* caller's stream -> sub-streams: everything already queued on the caller's stream happens before the parts.  Streams are
 * created when a kind of launch first needs them (a process has few hardware queues: a handle should not hold streams it never
 * uses); pom_batch_create and pom_batch_fork create what the handle's usual launches need. */
static int fork_parts(PomBatch* h, int kind)
{
    /* sub-batch launches (every stream its own tiles) and chained launches (every launch all tiles, pom_chain.h) must not be
     * in flight together: going from one kind to the other joins the streams first */
    const int need = streams_for(h, kind);
    if (h->forked && ((h->last_kind && kind && h->last_kind != kind) || need > h->forked_n))
        if (int jr = join_parts(h)) return jr;
    if (kind) h->last_kind = kind; /* kind 0: only the fork (pom_batch_fork), no launches yet */
    if (need == 1 || h->forked) return POM_OK;
    if (int er = ensure_sub_streams(h, need)) return er;
    HIPCHK(hipEventRecord(h->ev_fork, h->stream));
    for (int k = h->main_part; k < need; k++) HIPCHK(hipStreamWaitEvent(h->sub[k], h->ev_fork, 0));
    h->forked = true;
    h->forked_n = need;
    return POM_OK;
}
/* sub-streams -> caller's stream: whatever is queued on the caller's stream next sees all parts finished */
static int join_parts(PomBatch* h)
{
    if (!h->forked) return POM_OK;
    for (int k = h->main_part; k < h->forked_n; k++) {
        HIPCHK(hipEventRecord(h->ev_join[k], h->sub[k]));
        HIPCHK(hipStreamWaitEvent(h->stream, h->ev_join[k], 0));
    }
    h->forked = false;
    h->forked_n = 0;
    h->last_kind = 0;
    return POM_OK;
}

int ensure_agent_mem(PomBatch* h)
{
    if (!h->agent_mem) {
        if (int jr = join_parts(h)) return jr; /* the next launch forks the sub-streams again, after this memset */
        HIPCHK(hipMalloc((void**)&h->agent_mem, (size_t)h->n_pad * 32));
        HIPCHK(hipMemsetAsync(h->agent_mem, 0, (size_t)h->n_pad * 32, h->stream));
    }
    return POM_OK;
}

static int fill_params(PomBatch* h, StepParams& p, const int32_t* moves_dev, uint64_t seed, int dist, int ticks,
                       const PomObserveOut* obs = nullptr)
{
    p.agent_mem = h->agent_mem;
    p.state = h->state;
    p.snap = h->snap;
    p.terminal = h->terminal;
    p.moves = moves_dev;
    p.wave_counters = h->wave_counters;
#if defined(POM_TRUNC)
    p.trunc = getenv("POM_TRUNC_AT") ? atoi(getenv("POM_TRUNC_AT")) : 990;
#endif
    p.n = h->n;
    p.n_pad = h->n_pad;
    p.env_offset = h->env_offset;
    p.seed = seed;
    p.tick0 = (uint32_t)h->tick;
    p.tick_base = h->tick_words + PomBatch::MAX_PARTS; /* the word that stays 0: outside a graph tick0 is the tick itself */
    p.dist = dist;
    p.ticks = ticks;
    p.mode = h->mode;
    p.auto_reset = h->auto_reset;
    p.max_steps = h->max_steps;
    p.episode = h->episode;
    p.board_seed = h->board_seed;
    p.fresh = h->fresh;
    p.block0 = p.block_end = 0;
    p.tile_seq = nullptr;
    p.chain_err = nullptr;
    p.chain_seq0 = 0;
    p.tape_len = 0;
    p.chain_wait_limit = 0;
    p.chain_rot = 0;
    p.obs_planes = obs ? obs->planes : nullptr;
    p.obs_agent_attrs = obs ? obs->agent_attrs : nullptr;
    p.obs_env_attrs = obs ? obs->env_attrs : nullptr;
    p.obs_dtype = obs ? obs->dtype : 0;
    p.obs_per_agent = obs ? obs->per_agent : 0;
    p.obs_viewer_attrs = obs && obs->view ? obs->viewer_attrs : nullptr;
    p.obs_view_radius = obs && obs->view ? obs->view_radius : 0;
#if defined(POM_DIAG)
    if (!h->diag) {
        HIPCHK(hipMalloc((void**)&h->diag, (size_t)h->n_waves * POM_PH_N * 8));
        HIPCHK(hipMemsetAsync(h->diag, 0, (size_t)h->n_waves * POM_PH_N * 8, h->stream));
    }
    p.diag = h->diag;
#endif
    return POM_OK;
}

#endif /* POM_HANDLE_H_ */
