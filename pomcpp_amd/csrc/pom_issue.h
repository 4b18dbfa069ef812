/*
 * pom_issue.h — how a step becomes launches: the table of pom_step_kernel's instantiations (step_kernel), a run of launches on one
 * stream and who issues it (the calling thread, the helper threads), the sub-batch parts of a step (launch_parts, launch_step), the
 * replayed graphs, and a call of several ticks (launch_many).  The handle: pom_handle.h; chained launches: pom_chain_host.h.
 */
#ifndef POM_ISSUE_H_
#define POM_ISSUE_H_

#include "pom_handle.h"

/* Which instantiation of pom_step_kernel a launch runs: the one table of them.  Quad shape (the default): one instantiation per
 * combination of fresh boards / fused policy / reset at the end for launches of ONE tick — plain, chained (pom_chain.h; the plain
 * one with the same flags is its twin, what chain_settle replays a tick with) and, for explicit moves, with the fused observation or the
 * fused fogged views —
 * and the plain replay kernel for launches of several ticks: the other several-tick combinations would need more than the 128 VGPRs
 * that keep four wavefronts on a SIMD (12-116 B of scratch each, round 2), so those modes always run one tick per launch
 * (max_ticks_per_launch).  The one-lane-per-env shapes: fresh boards or not.  Combinations without a kernel of their own are kept
 * away by max_ticks_per_launch, runs_chain and pom_batch_create. */
typedef void (*PomStepKernel)(StepParams);
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
        PomStepKernel view[4];        /* as observe: the fogged views */
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

static int launch_many_chain(PomBatch* h, const StepParams& p0, int launches, bool policy, bool* used); /* pom_chain_host.h */

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

#endif /* POM_ISSUE_H_ */
