/*
 * pom_handle.h — the batch handle and how a call on it starts: the error text and the one way to refuse (refuse), the handle
 * (PomBatch), its streams forked and joined, the start of every call on a handle (begin_call), and the parameters a step launch
 * takes from the handle (fill_params).  Who launches what: pom_issue.h.
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
#include <type_traits>

#include "pom_kernels.h"
#include "pom_chain.h"

static thread_local char g_err[256] = "";
static void set_err(const char* what, hipError_t e)
{
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
}
#define HIPCHK(call)                      \
    do {                                  \
        hipError_t e_ = (call);           \
        if (e_ != hipSuccess) {           \
            set_err(#call, e_);           \
            return POM_E_HIP;             \
        }                                 \
    } while (0)

/* The one way to refuse a call: pom_last_error() reads "<call>: <what>", the call returns POM_E_ARG.  Every POM_E_ARG of every entry
 * point comes from here, so the text always names the call that refused. */
__attribute__((format(printf, 2, 3))) static int refuse(const char* who, const char* fmt, ...)
{
    const int at = snprintf(g_err, sizeof g_err, "%s: ", who);
    va_list ap;
    va_start(ap, fmt);
    if (at > 0 && at < (int)sizeof g_err) vsnprintf(g_err + at, sizeof g_err - (size_t)at, fmt, ap);
    va_end(ap);
    return POM_E_ARG;
}

/* The head of every spec's check (pom_batch.h Pom*Spec): what is wrong with it, or nullptr.  SPEC_HEAD names the type for the text. */
template <class S>
static const char* spec_head(const S* s, const char* size_text)
{
    if (!s) return "the spec is NULL";
    if (s->struct_size != (int32_t)sizeof(S)) return size_text;
    if constexpr (std::is_array<decltype(S::reserved_)>::value) {
        for (const auto r : s->reserved_)
            if (r != 0) return "reserved_ must be 0";
    } else if (s->reserved_ != 0) return "reserved_ must be 0";
    return nullptr;
}
#define SPEC_HEAD(S, s) spec_head<S>(s, "struct_size is not sizeof(" #S ")")

struct PomBatch {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t n = 0, n_pad = 0, n_waves = 0, env_offset = 0; /* n_waves: counter slots, sized for the smallest EPW */
    int epw = 64;
    bool quad = false; /* EPW 16 with four lanes per env (pom_step_kernel's G = 4) */
    int mode = POM_MODE_ENV, auto_reset = 0, max_steps = 0;
    uint32_t* state = nullptr;
    uint32_t* snap = nullptr;       /* restart snapshot, array of structs */
    uint32_t* terminal = nullptr;   /* POM_RESET_AT_END: final record of each env's last finished episode, array of structs */
    int32_t* moves_dev = nullptr;   /* n_pad x 4 */
    uint32_t* agent_mem = nullptr;  /* SimpleAgent memory, [2][4 * n_pad], allocated on first use */
    uint32_t* episode = nullptr;    /* games started per env (fresh boards) */
    uint64_t board_seed = 0;
    int fresh = 0;
    int32_t* staging = nullptr;     /* staging_envs x 251 dwords (AoS), also status scratch */
    uint32_t* copy_scratch = nullptr; /* pom_batch_copy_envs: K1's image of state, agent memory, episode (and terminal), allocated on
                                         first use (pom_copy.h) */
    int64_t* copy_idx = nullptr;      /* ... and the host variant's indices on the device, n_pad int64 */
    int64_t staging_envs = 0;
    int64_t* wave_counters = nullptr;
    int64_t* totals_dev = nullptr;
    int* first_bad = nullptr;
    uint64_t tick = 0;
    /* A step is issued as `parts` kernels over contiguous tile ranges on internal streams: the launches are
     * independent (envs never interact), so one part's HBM load / store phases overlap the others' compute
     * instead of all wavefronts of the chip loading and storing in lock-step.  The caller's stream is forked
     * into the sub-streams lazily and joined again before anything else touches the batch. */
    enum { MAX_PARTS = 8, PROF_RING = 256 };
    int parts = 1;
    hipStream_t sub[MAX_PARTS] = {};
    hipEvent_t ev_fork = nullptr, ev_join[MAX_PARTS] = {};
    bool forked = false;
    int forked_n = 0; /* how many streams (indices below it) the fork covers */
    int main_part = 1; /* part 0 of a split step runs on the caller's stream itself, parts 1.. on sub-streams: one stream
                          fewer for the same overlap (3 parts: 21.2 -> 20.6 us per step at 65,536 envs); POM_MAIN_PART=0: all
                          parts on sub-streams */
    /* how the launches of a several-tick call are issued (launch_many; PomBatchOptions.issue_mode) */
    int issue_mode = POM_ISSUE_THREADS;
    struct PomIssuer* issuers[MAX_PARTS] = {}; /* POM_ISSUE_THREADS: one helper thread per sub-stream part, created on first use */
    bool issuers_failed = false;               /* a helper thread could not be started: the calling thread issues the rest */
    int last_kind = 0;                         /* what has been launched on the streams since they were forked: POM_KIND_SPLIT / _CHAIN */
    /* POM_ISSUE_GRAPH: multi-tick calls replay a captured chunk of launches (launch_many): POM_GRAPH_TICKS launches of every part as one HIP
     * graph per part.  tick_words[k] is the tick part k's replay starts at, read by the graph's kernels (StepParams.tick_base;
     * set by a one-lane kernel on the part's stream in front of each replay); tick_words[MAX_PARTS] stays 0 and is what every
     * launch outside a graph points at. */
    enum { MAX_GRAPHS = 4 };
    struct PomStepGraph* graphs[MAX_GRAPHS] = {};
    uint64_t graph_clock = 0;
    uint32_t* tick_words = nullptr;
    PomChain chain;          /* POM_ISSUE_CHAIN: the tiles' ticket words, set up on first use (pom_chain.h) */
    int chain_parts = 3;     /* ... and how many streams the chained launches may rotate over */
    bool chain_auto = true;  /* ... of which a call uses two if it is short and three if it is long (launch_many_chain) — unless the caller
                                asked for a number of streams */
    int chain_last_use = 2;  /* what the last chained call used (pom_batch_issue_info) */
    bool fuse_policy = true; /* pom_batch_step_simple: policy and tick in one kernel (quad shape); POM_FUSE=0 keeps them apart */
    /* optional per-launch timing (pom_batch_profile) */
    bool profiling = false;
    hipEvent_t prof_ev[2 * PROF_RING] = {};
    int prof_n = 0;
#if defined(POM_DIAG)
    long long* diag = nullptr;
    long long* diag_pol = nullptr;
#endif
};

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

static int check_range(const PomBatch* h, const char* who, int64_t first, int64_t count)
{
    if (!h || first < 0 || count < 0 || first + count > h->n)
        return refuse(who, "range [%lld, %lld) outside batch", (long long)first, (long long)(first + count));
    return POM_OK;
}

/* The start of every call on a handle.  Refuses a NULL handle, then `what` (what the caller found wrong with the other arguments, or
 * nullptr), both by the call's name and before any runtime call; selects the handle's device; and brings the handle to the state
 * the call needs: as it is (a call that only launches: launch_step settles for itself), the sub-streams joined into the caller's
 * stream, or settled (quiesce). */
enum PomNeeds { POM_AS_IS, POM_JOINED, POM_SETTLED };
static int check_call(const PomBatch* h, const char* who, const char* what = nullptr) /* (all of it for a call that only reads the handle) */
{
    if (!h) return refuse(who, "the handle is NULL");
    return what ? refuse(who, "%s", what) : POM_OK;
}
static int begin_call(PomBatch* h, const char* who, PomNeeds needs, const char* what = nullptr)
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

static int ensure_agent_mem(PomBatch* h)
{
    if (!h->agent_mem) {
        if (int jr = join_parts(h)) return jr; /* the next launch forks the sub-streams again, after this memset */
        HIPCHK(hipMalloc((void**)&h->agent_mem, (size_t)h->n_pad * 32));
        HIPCHK(hipMemsetAsync(h->agent_mem, 0, (size_t)h->n_pad * 32, h->stream));
    }
    return POM_OK;
}

struct PomObserveOut { /* pom_batch_step_device_observe / _range: where the fused kernel writes the observation */
    void* planes;
    int32_t* agent_attrs;
    int32_t* env_attrs;
    int32_t dtype, per_agent;
    /* the fogged views (pom_batch_step_device_observe_view / _range_view): view = 1 picks the VIEW kernels (launch_parts, launch_range),
     * which write viewer_attrs and ignore agent_attrs / per_agent; the other kernels ignore these */
    int32_t view, view_radius;
    int32_t* viewer_attrs;
};
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
