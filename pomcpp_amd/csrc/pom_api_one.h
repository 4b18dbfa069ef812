/*
 * pom_api_one.h — pom_step / pom_env_step: the reference's Step on ONE State in host memory, through a pinned page per calling
 * thread and launches combined over the threads.  No handle.
 */
#ifndef POM_API_ONE_H_
#define POM_API_ONE_H_

#include "pom_handle.h"

/* pom_step / pom_env_step: a pinned, device-mapped page the kernel reads the State from and writes it back to
 * (pom_step_one_kernel), the host polling the kernel's last store.  The reference's Step is re-entrant over distinct States and
 * its performance test steps one env per std::thread (unit_test/bboard/performance_test.cpp:40-50,71-94): every calling thread
 * gets a slot of its own — a page and a sequence number — and posts its request there.  Launches are COMBINED: whichever
 * thread gets hold of the launch lock launches one kernel for every request pending at that moment (a workgroup per request),
 * the others find their page answered without having launched anything — the HIP runtime issues launches of one process one
 * after the other (~5 us each), so a launch per call would cap eight threads at three times one thread's rate.  Device 0.
 * POM_ONE_SLOTS slots; threads beyond that share (slot = thread number mod slots), which is what the per-slot mutex is for. */
struct PomOneShared {
    std::mutex init_mu, launch_mu;
    std::mutex slot_mu[POM_ONE_SLOTS];
    uint32_t seq[POM_ONE_SLOTS] = {};
    int32_t* io = nullptr;     /* host address of the pages */
    int32_t* io_dev = nullptr; /* the same pages as the device sees them */
    enum { STREAMS = 4 };
    hipStream_t stream[STREAMS] = {};
    unsigned turn = 0;
    std::atomic<uint64_t> pending{0};
    std::atomic<uint64_t> failed{0}; /* requests whose launch failed (answered by the launching thread) */
    std::atomic<bool> ready{false};
};
static PomOneShared g_one;
static std::atomic<unsigned> g_one_threads{0};

static int one_init(PomOneShared& o)
{
    std::lock_guard<std::mutex> g(o.init_mu);
    if (o.ready.load()) return POM_OK;
    HIPCHK(hipSetDevice(0));
    const size_t bytes = (size_t)POM_ONE_SLOTS * POM_ONE_PAGE_DWORDS * 4;
    if (!o.io) HIPCHK(hipHostMalloc((void**)&o.io, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer((void**)&o.io_dev, o.io, 0));
    for (int k = 0; k < PomOneShared::STREAMS; k++)
        if (!o.stream[k]) HIPCHK(hipStreamCreateWithFlags(&o.stream[k], hipStreamNonBlocking));
    memset(o.io, 0, bytes);
    o.ready.store(true);
    return POM_OK;
}

/* launch_mu held: one kernel for every request posted so far */
static void one_launch_pending(PomOneShared& o)
{
    const uint64_t mask = o.pending.exchange(0);
    if (!mask) return;
    StepOneParams p;
    p.io_base = o.io_dev;
    p.slots = mask;
    (void)hipSetDevice(0);
    pom_step_one_kernel<<<dim3((unsigned)__builtin_popcountll(mask)), dim3(64), 0, o.stream[o.turn++ % PomOneShared::STREAMS]>>>(p);
    if (hipGetLastError() != hipSuccess) o.failed.fetch_or(mask); /* their owners report it */
}

static int step_one(const char* who, void* state_1004, const int32_t moves[4], int32_t mode, int32_t max_steps, int32_t status4[4])
{
    if (!state_1004 || !moves) return refuse(who, "%s", !state_1004 ? "the State is NULL" : "moves is NULL");
    PomOneShared& o = g_one;
    if (!o.ready.load())
        if (int rc = one_init(o)) return rc;
    static thread_local int my_slot = -1;
    if (my_slot < 0) my_slot = (int)(g_one_threads.fetch_add(1) % POM_ONE_SLOTS);
    const uint64_t bit = 1ull << my_slot;
    std::lock_guard<std::mutex> lock(o.slot_mu[my_slot]);
    int32_t* io = o.io + (size_t)my_slot * POM_ONE_PAGE_DWORDS;
    const uint32_t seq = ++o.seq[my_slot] ? o.seq[my_slot] : ++o.seq[my_slot]; /* never 0: the page starts zeroed */
    memcpy(io, state_1004, POM_STATE_BYTES);
    memcpy(io + POM_ONE_MOVES, moves, 16);
    io[POM_ONE_MODE] = mode;
    io[POM_ONE_MAX_STEPS] = max_steps;
    io[POM_ONE_REQ] = (int32_t)seq;
    o.pending.fetch_or(bit, std::memory_order_release); /* posted: the page is complete */
    /* until the page is answered: launch what is pending whenever the launch lock is free (my own request, unless somebody
     * else's launch has taken it along), and watch the sequence word — the kernel's last store */
    volatile uint32_t* seq_word = reinterpret_cast<volatile uint32_t*>(io) + POM_ONE_SEQ;
    const auto until = std::chrono::steady_clock::now() + std::chrono::milliseconds(5);
    bool synced = false;
    for (;;) {
        if (*seq_word == seq) break;
        if (o.launch_mu.try_lock()) {
            one_launch_pending(o);
            o.launch_mu.unlock();
        }
        if (o.failed.load() & bit) {
            o.failed.fetch_and(~bit);
            snprintf(g_err, sizeof g_err, "pom_step: the kernel launch failed");
            return POM_E_HIP;
        }
        for (int spin = 0; spin < 64 && *seq_word != seq; spin++) __builtin_ia32_pause();
        if (*seq_word != seq && std::chrono::steady_clock::now() > until) {
            if (synced) {
                snprintf(g_err, sizeof g_err, "pom_step: the kernel finished without reporting");
                return POM_E_HIP;
            }
            /* not within milliseconds: wait the ordinary way — which is also where a device error surfaces */
            std::lock_guard<std::mutex> g(o.launch_mu);
            one_launch_pending(o);
            for (int k = 0; k < PomOneShared::STREAMS; k++) HIPCHK(hipStreamSynchronize(o.stream[k]));
            synced = true;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (io[POM_ONE_BAD]) {
        snprintf(g_err, sizeof g_err, "pom_step: the State holds a value outside the representable game states (it was left as it is)");
        return POM_E_UNREPRESENTABLE;
    }
    memcpy(state_1004, io + POM_ONE_OUT, POM_STATE_BYTES);
    if (status4) memcpy(status4, io + POM_ONE_STATUS, 16);
    return POM_OK;
}

extern "C" {

int pom_step(void* state_1004, const int32_t moves[4]) { return step_one("pom_step", state_1004, moves, POM_MODE_RAW, 0, nullptr); }

int pom_env_step(void* state_1004, const int32_t moves[4], int32_t max_steps, int32_t* done, int32_t* winner, int32_t* draw,
                 uint32_t* ubflags)
{
    int32_t st[4] = {0, -1, 0, 0};
    const int rc = step_one("pom_env_step", state_1004, moves, POM_MODE_ENV, max_steps, st);
    if (rc) return rc;
    if (done) *done = st[0];
    if (winner) *winner = st[1];
    if (draw) *draw = st[2];
    if (ubflags) *ubflags = (uint32_t)st[3];
    return POM_OK;
}

} /* extern "C" */

#endif /* POM_API_ONE_H_ */
