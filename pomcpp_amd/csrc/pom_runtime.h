/*
 * pom_runtime.h — host runtime of the batched stepper: the batch handle, its streams, and how a step becomes launches of
 * pom_step_kernel (pom_kernels.h).  The C-ABI functions of include/pom_batch.h (pom_batch.hip) are thin wrappers over this.
 */
#ifndef POM_RUNTIME_H_
#define POM_RUNTIME_H_

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <thread>

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

static int check_range(const PomBatch* h, int64_t first, int64_t count)
{
    if (!h || first < 0 || count < 0 || first + count > h->n) {
        snprintf(g_err, sizeof g_err, "range [%lld, %lld) outside batch", (long long)first, (long long)(first + count));
        return POM_E_ARG;
    }
    return POM_OK;
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

/* Which instantiation of pom_step_kernel a launch runs: the one table of them.  Quad shape (the default): one instantiation per
 * combination of fresh boards / fused policy / reset at the end for launches of ONE tick — plain, chained (pom_chain.h; the plain
 * one with the same flags is its twin, what chain_settle replays a tick with) and, for explicit moves, with the fused observation or the
 * fused fogged views —
 * and the plain replay kernel for launches of several ticks: the other several-tick combinations would need more than the 128 VGPRs
 * that keep four wavefronts on a SIMD (12-116 B of scratch each, round 2), so those modes always run one tick per launch
 * (max_ticks_per_launch).  The one-lane-per-env shapes: fresh boards or not.  Combinations without a kernel of their own are kept
 * away by max_ticks_per_launch, runs_chain and pom_batch_create. */
typedef void (*PomStepKernel)(StepParams);
static bool runs_fresh(const PomBatch* h) { return h->fresh && h->mode == POM_MODE_ENV && h->auto_reset; }
static bool runs_at_end(const PomBatch* h) { return h->auto_reset == POM_RESET_AT_END && h->mode == POM_MODE_ENV; }
static int max_ticks_per_launch(const PomBatch* h, bool policy)
{
    return (!h->quad || (!policy && !runs_fresh(h) && !runs_at_end(h))) ? INT_MAX : 1;
}
static PomStepKernel step_kernel(const PomBatch* h, bool policy, int ticks_per_launch, bool chained, bool observe, bool view = false)
{
    /* (listed in the order the kernels have always been emitted in: the order reaches the register allocation — 118 instead of
     * 119 VGPRs for the fresh-board kernel of 16 envs per wavefront, one lane each, when listed otherwise) */
    static const struct {
        PomStepKernel one_tick[8];    /* [fresh * 4 + policy * 2 + at_end] */
        PomStepKernel several_ticks;
        PomStepKernel one_lane[3][2]; /* [64 / 32 / 16 envs per wavefront][fresh ? 0 : 1] */
        PomStepKernel observe[4];     /* [fresh * 2 + at_end] (explicit moves: no policy) */
        PomStepKernel chained[8];     /* as one_tick */
        PomStepKernel view[4];        /* as observe: the fogged views (listed last: the kernels before it are emitted as they always were) */
    } k = {
        {pom_step_kernel<16, 4, false, false, false, true>, pom_step_kernel<16, 4, false, false, true, true>,
         pom_step_kernel<16, 4, false, true, false, true>, pom_step_kernel<16, 4, false, true, true, true>,
         pom_step_kernel<16, 4, true, false, false, true>, pom_step_kernel<16, 4, true, false, true, true>,
         pom_step_kernel<16, 4, true, true, false, true>, pom_step_kernel<16, 4, true, true, true, true>},
        pom_step_kernel<16, 4, false, false, false, false>,
        {{pom_step_kernel<64, 1, true>, pom_step_kernel<64, 1, false>},
         {pom_step_kernel<32, 1, true>, pom_step_kernel<32, 1, false>},
         {pom_step_kernel<16, 1, true>, pom_step_kernel<16, 1, false>}},
        {pom_step_kernel<16, 4, false, false, false, true, false, true>, pom_step_kernel<16, 4, false, false, true, true, false, true>,
         pom_step_kernel<16, 4, true, false, false, true, false, true>, pom_step_kernel<16, 4, true, false, true, true, false, true>},
        {pom_step_kernel<16, 4, false, false, false, true, true>, pom_step_kernel<16, 4, false, false, true, true, true>,
         pom_step_kernel<16, 4, false, true, false, true, true>, pom_step_kernel<16, 4, false, true, true, true, true>,
         pom_step_kernel<16, 4, true, false, false, true, true>, pom_step_kernel<16, 4, true, false, true, true, true>,
         pom_step_kernel<16, 4, true, true, false, true, true>, pom_step_kernel<16, 4, true, true, true, true, true>},
        {pom_step_kernel<16, 4, false, false, false, true, false, true, true>, pom_step_kernel<16, 4, false, false, true, true, false, true, true>,
         pom_step_kernel<16, 4, true, false, false, true, false, true, true>, pom_step_kernel<16, 4, true, false, true, true, false, true, true>}};
    const int fresh = runs_fresh(h) ? 1 : 0, at_end = runs_at_end(h) ? 1 : 0;
    if (!h->quad) return k.one_lane[h->epw == 64 ? 0 : h->epw == 32 ? 1 : 2][1 - fresh];
    if (observe) return (view ? k.view : k.observe)[2 * fresh + at_end];
    if (ticks_per_launch != 1) return k.several_ticks;
    return (chained ? k.chained : k.one_tick)[4 * fresh + (policy ? 2 : 0) + at_end];
}

/* A run: `count` launches of one kernel on one stream — a sub-batch part's, or those a chained call deals to one of its streams.
 * Launch j of the run is the call's launch i = first + j * stride, with the parameters `p` but for the tick, advanced by
 * i * tick_step (sub-batches: the ticks per launch; a chained launch keeps it, its tickets decide which tick it plays), and, where
 * rot_mod is set, chain_rot = (rot0 + i) * rot_mul % rot_mod (the rotation of launch_many_chain). */
struct PomRun {
    PomStepKernel kernel = nullptr;
    unsigned grid = 0;
    int part = 0; /* the stream's index (part_stream; its helper: issuer_for) */
    hipStream_t st = nullptr;
    StepParams p;
    int first = 0, stride = 1, count = 0;
    uint32_t tick_step = 0;
    uint32_t rot0 = 0, rot_mul = 0, rot_mod = 0;
};

/* launches [from, to) of a run, from whichever thread holds it; *queued counts what was queued.  timed: while profiling
 * (pom_batch_profile), start / stop events attached to the dispatch itself, i.e. the kernel's own duration as a profiler reports
 * it, not the stream's period (events recorded around a launch also time the gap) */
static hipError_t issue_run(PomBatch* h, const PomRun& r, int from, int to, bool timed, int* queued)
{
    for (int j = from; j < to; j++) {
        const uint32_t i = (uint32_t)(r.first + j * r.stride);
        StepParams q = r.p;
        q.tick0 += i * r.tick_step;
        if (r.rot_mod) q.chain_rot = (uint32_t)((uint64_t)(r.rot0 + i) * r.rot_mul % r.rot_mod);
        const bool prof = timed && h->profiling && h->prof_n < PomBatch::PROF_RING;
        hipEvent_t ev0 = prof ? h->prof_ev[2 * h->prof_n] : nullptr, ev1 = prof ? h->prof_ev[2 * h->prof_n + 1] : nullptr;
        void* args[1] = {&q};
        const hipError_t e = hipExtLaunchKernel(reinterpret_cast<const void*>(r.kernel), dim3(r.grid), dim3(64 * POM_WPB), args, 0, r.st, ev0, ev1, 0);
        if (e != hipSuccess) return e;
        if (prof) h->prof_n++;
        ++*queued;
    }
    return hipSuccess;
}

/* a helper thread: issues the launches of one sub-stream that issue_runs hands it */
struct PomIssuer {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    bool has_job = false, quit = false, busy = false;
    std::atomic<int> posted{0}; /* bumped with every job and by pom_batch_fork: a thread that has just worked (or was told that work
                                   is coming) polls this for up to a millisecond before it goes to sleep on the condition variable
                                   — a futex wake-up costs 10-30 us, a tenth of a 20-step burst */
    /* the job: launches 1 .. run.count - 1 of `run`, and how many of them were queued */
    PomRun run;
    int done = 0;
    hipError_t err = hipSuccess;
};

static void issuer_main(PomBatch* h, PomIssuer* w)
{
    (void)hipSetDevice(h->device);
    std::unique_lock<std::mutex> lk(w->mu);
    int seen = w->posted.load();
    for (;;) {
        if (!w->has_job && !w->quit) { /* poll briefly, then sleep */
            lk.unlock();
            const auto until = std::chrono::steady_clock::now() + std::chrono::milliseconds(1);
            while (w->posted.load(std::memory_order_acquire) == seen && std::chrono::steady_clock::now() < until) {
            }
            lk.lock();
        }
        if (!w->has_job && !w->quit && w->posted.load() != seen) { /* woken by pom_batch_fork: a job is on its way */
            seen = w->posted.load();
            continue;
        }
        w->cv.wait(lk, [w, seen] { return w->has_job || w->quit || w->posted.load() != seen; });
        seen = w->posted.load();
        if (w->quit) return;
        if (!w->has_job) continue;
        w->has_job = false;
        w->done = 0;
        w->err = issue_run(h, w->run, 1, w->run.count, false, &w->done);
        w->busy = false;
        w->cv.notify_all();
    }
}

static void stop_issuers(PomBatch* h)
{
    for (int k = 0; k < PomBatch::MAX_PARTS; k++) {
        PomIssuer* w = h->issuers[k];
        if (!w) continue;
        {
            std::lock_guard<std::mutex> g(w->mu);
            w->quit = true;
        }
        w->cv.notify_all();
        if (w->th.joinable()) w->th.join();
        delete w;
        h->issuers[k] = nullptr;
    }
}

/* the helper of sub-stream k, started on first use; nullptr if it cannot be had (the caller then issues that stream's launches) */
static PomIssuer* issuer_for(PomBatch* h, int k)
{
    if (h->issuers[k] || h->issuers_failed) return h->issuers[k];
    PomIssuer* w = new (std::nothrow) PomIssuer();
    if (w) {
        try {
            w->th = std::thread(issuer_main, h, w);
        } catch (...) { /* std::system_error: no thread to be had — nothing may cross the C boundary */
            delete w;
            w = nullptr;
        }
    }
    if (!w) h->issuers_failed = true;
    h->issuers[k] = w;
    return w;
}

/* Issues `n` runs, at most one per stream, listed in the order of their first launches; returns how many launches were queued,
 * *err the first failure (a thread issues nothing after its own first failure, nor hands out anything after one).
 * helpers = false: the calling thread issues everything in launch-number order, round-robin over the runs.
 * helpers = true: the first launch of EVERY run is issued right here, the caller's own stream first: a helper thread takes 10-25 us
 * to pick its job up (profiles/r02_region_trace.txt), and a part that starts a step late finishes a step late — alone on the
 * device.  The rest of each sub-stream's run goes to that stream's helper thread (issuer_for), which has one step's time to wake
 * up, while the calling thread issues the rest of its own stream's run (and of any run whose helper could not be started: the only
 * case in which the order of the launches differs from the helpers' one).  The call returns when everything is queued. */
static int issue_runs(PomBatch* h, const PomRun* runs, int n, bool helpers, hipError_t* err)
{
    int queued = 0;
    *err = hipSuccess;
    PomIssuer* started[PomBatch::MAX_PARTS] = {};
    int j0 = 0;
    if (helpers) {
        for (int r = 0; r < n && *err == hipSuccess; r++) *err = issue_run(h, runs[r], 0, runs[r].count > 0 ? 1 : 0, true, &queued);
        for (int r = 0; r < n && *err == hipSuccess; r++) {
            if (runs[r].st == h->stream || runs[r].count < 2) continue;
            PomIssuer* w = issuer_for(h, runs[r].part);
            if (!w) continue;
            {
                std::lock_guard<std::mutex> g(w->mu);
                w->run = runs[r];
                w->busy = true;
                w->has_job = true;
                w->posted.fetch_add(1, std::memory_order_release);
            }
            w->cv.notify_all();
            started[r] = w;
        }
        j0 = 1;
    }
    for (int j = j0, more = 1; more && *err == hipSuccess; j++) {
        more = 0;
        for (int r = 0; r < n && *err == hipSuccess; r++)
            if (!started[r] && j < runs[r].count) {
                *err = issue_run(h, runs[r], j, j + 1, true, &queued);
                more = 1;
            }
    }
    for (int r = 0; r < n; r++) { /* everything is queued when the call returns */
        PomIssuer* w = started[r];
        if (!w) continue;
        std::unique_lock<std::mutex> lk(w->mu);
        w->cv.wait(lk, [w] { return !w->busy; });
        queued += w->done;
        if (w->err != hipSuccess && *err == hipSuccess) *err = w->err;
    }
    return queued;
}

/* `launches` launches of every sub-batch part, p.ticks ticks each, from p.tick0 on; the caller advances the tick.  `one_launch`: the
 * whole batch in ONE launch on the caller's stream.  For steps that have to be joined with the caller's stream every tick (explicit
 * moves): forking into sub-streams and joining them again costs more than the overlap gains (65,536 envs, MI355X: 23.3 us per step
 * as one launch, 43.8 as two, 60.2 as three; profiles/r02a_explicit_streams.txt).  `threads`: with the helper threads (issue_runs) */
static int launch_parts(PomBatch* h, const StepParams& p, int launches, bool policy, bool one_launch, bool threads, bool view = false)
{
    const int parts = one_launch ? 1 : h->parts;
    if (int rc = one_launch ? join_parts(h) : fork_parts(h)) return rc;
    const PomStepKernel kernel = step_kernel(h, policy, p.ticks, false, p.obs_planes != nullptr, view);
    PomRun runs[PomBatch::MAX_PARTS];
    int n = 0;
    for (int k = 0; k < parts; k++) {
        int64_t b0, b1;
        if (!part_tiles(h, k, parts, &b0, &b1)) continue;
        PomRun& r = runs[n++];
        r.kernel = kernel;
        r.grid = (unsigned)((b1 - b0 + POM_WPB - 1) / POM_WPB);
        r.part = k;
        r.st = part_stream(h, k, parts);
        r.p = p;
        r.p.block0 = b0;
        r.p.block_end = b1;
        r.count = launches;
        r.tick_step = (uint32_t)p.ticks;
    }
    hipError_t err = hipSuccess;
    issue_runs(h, runs, n, threads, &err);
    if (err != hipSuccess) { /* some launches may be queued, others not: the handle's tick no longer describes its state */
        set_err("pom_step_kernel launch (the batch is in an undefined state: upload again or destroy it)", err);
        return POM_E_HIP;
    }
    return POM_OK;
}

static int launch_step(PomBatch* h, const int32_t* moves_dev, uint64_t seed, int dist, int ticks, bool policy = false, bool one_launch = false,
                       const PomObserveOut* obs = nullptr)
{
    StepParams p;
    if (int rc = chain_settle(h)) return rc; /* an ordinary launch after chained ones: every tile must stand on the tick the host thinks it does */
    if (int rc = fill_params(h, p, moves_dev, seed, dist, ticks, obs)) return rc;
    return launch_parts(h, p, 1, policy, one_launch, false, obs && obs->view);
}

#ifndef POM_GRAPH_TICKS
#define POM_GRAPH_TICKS 20
#endif

__global__ void pom_set_word_kernel(uint32_t* dst, uint32_t v) { *dst = v; }

struct PomStepGraph {
    hipGraph_t graph[PomBatch::MAX_PARTS] = {};
    hipGraphExec_t exec[PomBatch::MAX_PARTS] = {};
    StepParams key;      /* everything the nodes were built with (tick0 / tick_base / blocks zeroed) */
    int launches = 0, parts = 0, ticks_per_launch = 0;
    bool policy = false;
    uint64_t used = 0;
};

static void free_graph(PomStepGraph* g)
{
    if (!g) return;
    for (int k = 0; k < PomBatch::MAX_PARTS; k++) {
        if (g->exec[k]) (void)hipGraphExecDestroy(g->exec[k]);
        if (g->graph[k]) (void)hipGraphDestroy(g->graph[k]);
    }
    delete g;
}

static void drop_graphs(PomBatch* h)
{
    for (int k = 0; k < PomBatch::MAX_GRAPHS; k++) {
        free_graph(h->graphs[k]);
        h->graphs[k] = nullptr;
    }
}

/* the graphs of `launches` launches per part for these parameters: from the cache, or built now (nullptr + *rc on failure) */
static PomStepGraph* step_graph(PomBatch* h, const StepParams& p, int launches, int ticks_per_launch, bool policy, int* rc)
{
    *rc = POM_OK;
    for (int k = 0; k < PomBatch::MAX_GRAPHS; k++) {
        PomStepGraph* g = h->graphs[k];
        if (g && g->launches == launches && g->parts == h->parts && g->ticks_per_launch == ticks_per_launch && g->policy == policy &&
            memcmp(&g->key, &p, sizeof p) == 0) {
            g->used = ++h->graph_clock;
            return g;
        }
    }
    PomStepGraph* g = new (std::nothrow) PomStepGraph();
    if (!g) {
        *rc = POM_E_NOMEM;
        return nullptr;
    }
    memcpy(&g->key, &p, sizeof p);
    g->launches = launches;
    g->parts = h->parts;
    g->ticks_per_launch = ticks_per_launch;
    g->policy = policy;
    hipError_t err = hipSuccess;
    const PomStepKernel fn = step_kernel(h, policy, ticks_per_launch, false, false);
    for (int k = 0; k < h->parts && err == hipSuccess; k++) {
        int64_t b0, b1;
        if (!part_tiles(h, k, h->parts, &b0, &b1)) continue;
        err = hipGraphCreate(&g->graph[k], 0);
        hipGraphNode_t prev = nullptr;
        for (int i = 0; i < launches && err == hipSuccess; i++) {
            StepParams q = p;
            q.block0 = b0;
            q.block_end = b1;
            q.ticks = ticks_per_launch;
            q.tick0 = (uint32_t)(i * ticks_per_launch); /* relative to *tick_base */
            q.tick_base = h->tick_words + k;
            void* args[1] = {&q};
            hipKernelNodeParams np;
            memset(&np, 0, sizeof np);
            np.func = reinterpret_cast<void*>(fn);
            np.gridDim = dim3((unsigned)((b1 - b0 + POM_WPB - 1) / POM_WPB));
            np.blockDim = dim3(64 * POM_WPB);
            np.kernelParams = args;
            hipGraphNode_t node = nullptr;
            err = hipGraphAddKernelNode(&node, g->graph[k], prev ? &prev : nullptr, prev ? 1 : 0, &np);
            prev = node;
        }
        if (err == hipSuccess) err = hipGraphInstantiate(&g->exec[k], g->graph[k], nullptr, nullptr, 0);
    }
    if (err != hipSuccess) {
        set_err("building the step graph", err);
        free_graph(g);
        *rc = POM_E_HIP;
        return nullptr;
    }
    int slot = 0; /* a free slot, or the least recently used one */
    for (int k = 0; k < PomBatch::MAX_GRAPHS; k++) {
        if (!h->graphs[k]) {
            slot = k;
            break;
        }
        if (h->graphs[k]->used < h->graphs[slot]->used) slot = k;
    }
    free_graph(h->graphs[slot]);
    g->used = ++h->graph_clock;
    h->graphs[slot] = g;
    return g;
}

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
        if (!chain_setup(c, tiles, h->stream) && getenv("POM_CHAIN_VERBOSE"))
            fprintf(stderr, "pom: chained launches are not available on this device (allocation failed or the workgroup -> XCD probe did not find the "
                            "eight-XCD round-robin); launching sub-batches\n");
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

/* ---- several ticks in one call ---------------------------------------------------------------------------------------------
 * `launches` launches per part, ticks_per_launch ticks each; advances h->tick by what was queued.
 * The default up to 196,608 envs is POM_ISSUE_CHAIN (launch_many_chain, pom_chain.h): one launch over all tiles per tick,
 * consecutive launches on different streams, a ticket word per tile ordering the tile's ticks — 9.2 us per step at 65,536 envs
 * where sub-batches take 14.5.  What follows is how SUB-BATCH launches are issued: what a handle does where launches are not
 * chained (several ticks per launch, batches from 196,608 envs up, the one-lane-per-env shapes, a handle asked for another mode).
 * A step is then `parts` launches (one per sub-batch, on parallel streams) every ~16 us at 65,536 envs: the host has ~5 us per
 * launch, and a call of K ticks is judged by how soon all parts' first launches are out and whether the queues stay fed.
 * Three ways to issue them (PomBatchOptions.issue_mode; results cannot depend on the choice: the same kernels with the same
 * arguments go to the same streams in the same per-stream order).  Measured on MI355X, 65,536 envs, 3 parts, per step
 * (profiles/r03_issue_modes.txt):
 *                                   20-tick call from an idle device (the bench driver's shape)      500-tick call
 *   POM_ISSUE_THREADS               18.0 us, run to run the same                                      15.5 us
 *   POM_ISSUE_DIRECT                17.2 .. 26.4 us: one thread issues all 60 launches (2.8 us each   15.6 - 16.0 us
 *                                   on a quiet host, then it is ahead of the device; on a busy one it is not)
 *   POM_ISSUE_GRAPH                 21.4 .. 23.5 us: queued in 48 us, but the replayed nodes run with   16.1 - 16.2 us
 *                                   wider gaps than plain launches
 * THREADS: part k's launches of ALL the ticks of the call are issued by a helper thread of its own (issue_runs), the call returns
 * when everything is queued.  A helper that cannot be started is not an error: the calling thread issues its launches.
 * DIRECT: the calling thread issues everything, tick by tick; no library-owned threads.
 * GRAPH: part k's launches of POM_GRAPH_TICKS consecutive ticks are a HIP graph — a plain chain of kernel nodes, built once —
 * replayed on part k's stream with one hipGraphLaunch per part and chunk; no library-owned threads either.  The nodes'
 * arguments never change: a node carries its offset inside the chunk, and the tick the chunk starts at is a device word per
 * part (StepParams.tick_base) that a one-lane kernel sets on the part's stream in front of each replay.  (One graph holding
 * all parts as parallel branches was measured first: this runtime plays the branches one after the other — 18.5 us per step
 * in a 500-tick call.)  Ticks that do not fill a chunk are launched directly. */
static int launch_many(PomBatch* h, uint64_t seed, int dist, int launches, int ticks_per_launch, bool policy)
{
    static const int chunk = getenv("POM_GRAPH_TICKS") ? atoi(getenv("POM_GRAPH_TICKS")) : POM_GRAPH_TICKS;
    int done = 0;
    if (runs_chain(h, ticks_per_launch) && launches >= 1) {
        StepParams p;
        memset(&p, 0, sizeof p); /* consecutive calls' parameters are compared byte for byte */
        if (int rc = fill_params(h, p, nullptr, seed, dist, 1)) return rc;
        bool used = false;
        if (int rc = launch_many_chain(h, p, launches, policy, &used)) return rc;
        if (used) return POM_OK; /* (the tick was advanced by what was queued) */
    }
    if (int rc = chain_settle(h)) return rc;
    if (h->issue_mode == POM_ISSUE_GRAPH && chunk >= 2 && launches >= chunk && !h->profiling) {
        StepParams p;
        memset(&p, 0, sizeof p); /* the cache compares the bytes */
        if (int rc = fill_params(h, p, nullptr, seed, dist, ticks_per_launch)) return rc;
        p.tick0 = 0;
        p.tick_base = nullptr;
        int rc = POM_OK;
        PomStepGraph* g = step_graph(h, p, chunk, ticks_per_launch, policy, &rc);
        if (!g) return rc;
        if (int fr = fork_parts(h)) return fr;
        for (; launches - done >= chunk; done += chunk) {
            for (int k = 0; k < h->parts; k++) { /* the caller's own stream first: its part starts without a wait on the fork event */
                if (!g->exec[k]) continue;
                hipStream_t st = part_stream(h, k, h->parts);
                pom_set_word_kernel<<<dim3(1), dim3(1), 0, st>>>(h->tick_words + k, (uint32_t)h->tick);
                HIPCHK(hipGetLastError());
                HIPCHK(hipGraphLaunch(g->exec[k], st));
            }
            h->tick += (uint64_t)chunk * (uint64_t)ticks_per_launch;
        }
    }
    if (done == launches) return POM_OK;
    if (h->profiling) { /* per-launch events: launch_step attaches them */
        for (; done < launches; done++) {
            if (int rc = launch_step(h, nullptr, seed, dist, ticks_per_launch, policy)) return rc;
            h->tick += (uint64_t)ticks_per_launch;
        }
        return POM_OK;
    }
    StepParams p;
    if (int rc = fill_params(h, p, nullptr, seed, dist, ticks_per_launch)) return rc;
    /* (a handle of chained launches issues what cannot be chained — policy, fresh boards, several ticks per launch — with the helper threads) */
    const bool threads = (h->issue_mode == POM_ISSUE_THREADS || h->issue_mode == POM_ISSUE_CHAIN) && h->parts > 1 && launches - done >= 2;
    if (int rc = launch_parts(h, p, launches - done, policy, false, threads)) return rc;
    h->tick += (uint64_t)(launches - done) * (uint64_t)ticks_per_launch;
    return POM_OK;
}

static int launch_policy(PomBatch* h, uint64_t seed)
{
    if (int rc = chain_settle(h)) return rc;
    if (int rc = ensure_agent_mem(h)) return rc;
    PolicyParams p;
    p.state = h->state;
    p.snap = h->snap;
    p.agent_mem = h->agent_mem;
    p.moves = h->moves_dev;
    p.n = h->n;
    p.n_pad = h->n_pad;
    p.env_offset = h->env_offset;
    p.seed = seed;
    p.tick = (uint32_t)h->tick;
    p.mode = h->mode;
    p.auto_reset = h->auto_reset;
    p.episode = h->episode;
    p.board_seed = h->board_seed;
    p.fresh = h->fresh;
#if defined(POM_DIAG)
    if (!h->diag_pol) {
        HIPCHK(hipMalloc((void**)&h->diag_pol, (size_t)(h->n_pad / 16) * POM_PP_N * 8));
        HIPCHK(hipMemsetAsync(h->diag_pol, 0, (size_t)(h->n_pad / 16) * POM_PP_N * 8, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    p.diag = h->diag_pol;
#endif
    /* same split and the same streams as the tick, so that part k's policy -> tick -> policy chain pipelines */
    int rc = fork_parts(h);
    if (rc) return rc;
    for (int k = 0; k < h->parts; k++) {
        int64_t b0, b1;
        if (!part_tiles(h, k, h->parts, &b0, &b1)) continue;
        p.block0 = b0 * h->epw / 16; /* the policy kernel's tiles are 16 envs: the tick's part k, env for env */
        pom_policy_kernel<<<dim3((unsigned)((b1 - b0) * h->epw / 16)), dim3(64), 0, part_stream(h, k, h->parts)>>>(p);
        HIPCHK(hipGetLastError());
    }
    return POM_OK;
}

#endif /* POM_RUNTIME_H_ */
