/*
 * pom_api_diag.h — the entry points that measure or test the library rather than play: the chained launches' statistics and their
 * self-test without the game (pom_chain_litmus), the diagnostic builds' readers (POM_DIAG, POM_CHAIN_DIAG), per-launch timing
 * (pom_batch_profile), and the stand-in policy of the closed-loop measurements (pom_bench_policy) with its kernel.
 */
#ifndef POM_API_DIAG_H_
#define POM_API_DIAG_H_

#include <vector>

#include "pom_chain_host.h"

extern "C" { /* (the kernel too: the profiles list it under its plain name) */

/* the stand-in policy of the closed-loop measurements (pom_batch.h): a workgroup takes 64 envs, reads their observations — 64 x 605
 * bytes, as dwords, coalesced; lane l sums w[k] * (2k + 1) over the group's dwords k = l, l + 256, ... — and every lane (env, agent) draws its move from its sum */
__global__ __launch_bounds__(256) void pom_bench_policy_kernel(const uint8_t* codes, int32_t* moves, int64_t first, int64_t count, uint32_t tick)
{
    const int64_t e0 = first + (int64_t)blockIdx.x * 64;
    const int64_t e = e0 + (threadIdx.x >> 2);
    uint32_t acc = 0;
    if (codes) {
        const int64_t envs = count - (int64_t)blockIdx.x * 64 < 64 ? count - (int64_t)blockIdx.x * 64 : 64;
        const uintptr_t lo = (uintptr_t)(codes + e0 * POM_OBS_CODE_PLANES * POM_CELLS), hi = lo + (uintptr_t)envs * POM_OBS_CODE_PLANES * POM_CELLS;
        const uint32_t* w = reinterpret_cast<const uint32_t*>((lo + 3) & ~(uintptr_t)3); /* whole dwords inside the range's bytes */
        const int64_t nw = (int64_t)((hi & ~(uintptr_t)3) - ((lo + 3) & ~(uintptr_t)3)) / 4;
        /* (a sum whose order does not matter: four loads in flight per lane) */
        uint32_t a1 = 0, a2 = 0, a3 = 0;
        int64_t k = threadIdx.x;
        for (; k + 768 < nw; k += 1024) {
            acc += w[k] * (uint32_t)(2 * k + 1);
            a1 += w[k + 256] * (uint32_t)(2 * (k + 256) + 1);
            a2 += w[k + 512] * (uint32_t)(2 * (k + 512) + 1);
            a3 += w[k + 768] * (uint32_t)(2 * (k + 768) + 1);
        }
        for (; k < nw; k += 256) acc += w[k] * (uint32_t)(2 * k + 1);
        acc += a1 + a2 + a3;
    }
    if (e < first + count) {
        uint32_t x = acc ^ ((uint32_t)e * 0x9E3779B1u) ^ ((threadIdx.x & 3u) * 0x85EBCA6Bu) ^ (tick * 0xC2B2AE35u);
        x ^= x >> 15;
        x *= 0x2C1B3C6Du;
        x ^= x >> 12;
        moves[e * 4 + (threadIdx.x & 3)] = (int32_t)((x >> 8) % 6u);
    }
}

int pom_batch_chain_stats(PomBatch* h, int64_t out[4])
{
    if (int rc = check_call(h, "pom_batch_chain_stats", !out ? "out is NULL" : nullptr)) return rc;
    out[0] = h->chain.stat_launches;
    out[1] = h->chain.stat_settles;
    out[2] = h->chain.stat_tiles_recovered;
    out[3] = h->chain.stat_ticks_replayed;
    return POM_OK;
}

/* self-test of the chained launches' hand-off, without the game (pom_kernels.h pom_chain_litmus_kernel): `launches` launches over
 * `tiles` records round-robin over `streams` streams; out[0] records found stale or torn, out[1] dwords that differed, out[2]
 * visits played, out[3] visits expected, out[4] tiles whose final record or word is not what `launches` clean visits leave,
 * out[5] the kernels' failure flags (POM_CHAIN_E_*; a give-up leaves its tile behind: counted in out[4]) */
int pom_chain_litmus(int32_t device, int64_t tiles, int32_t launches, int32_t streams, int64_t out[6])
{
    if (!out || tiles < 8 || tiles > (1 << 22) || launches < 1 || launches > (1 << 20) || streams < 1 || streams > PomBatch::MAX_PARTS)
        return refuse("pom_chain_litmus", "out must not be NULL, tiles 8..2^22, launches 1..2^20, streams 1..%d", (int)PomBatch::MAX_PARTS);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return POM_E_HIP;
    HIPCHK(hipSetDevice(device));
    PomChain c;
    hipStream_t st[PomBatch::MAX_PARTS] = {};
    uint32_t* data = nullptr;
    unsigned long long* res = nullptr;
    int rc = POM_OK;
    auto cleanup = [&] {
        for (int k = 0; k < streams; k++)
            if (st[k]) {
                (void)hipStreamSynchronize(st[k]);
                (void)hipStreamDestroy(st[k]);
            }
        chain_destroy(&c);
        (void)hipFree(data);
        (void)hipFree(res);
    };
    for (int k = 0; k < streams && rc == POM_OK; k++)
        if (hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking) != hipSuccess) rc = POM_E_HIP;
    if (rc == POM_OK && !chain_setup(&c, tiles, st[0])) {
        snprintf(g_err, sizeof g_err, "pom_chain_litmus: chained launches are not available on this device");
        rc = POM_E_HIP;
    }
    const size_t bytes = (size_t)tiles * POM_TILE_DWORDS * 4;
    if (rc == POM_OK && (hipMalloc((void**)&data, bytes) != hipSuccess || hipMalloc((void**)&res, 64) != hipSuccess)) rc = POM_E_NOMEM;
    if (rc != POM_OK) {
        cleanup();
        return rc;
    }
    try { /* (host vectors below: nothing may throw across the C boundary) */
    /* visit 0 expects 0 ^ tag: fill the records accordingly (on the host: this is a test) */
    {
        std::vector<uint32_t> init((size_t)tiles * POM_TILE_DWORDS);
        for (int64_t t = 0; t < tiles; t++)
            for (int k = 0; k < POM_TILE_DWORDS; k++) init[(size_t)t * POM_TILE_DWORDS + k] = (uint32_t)t * 2654435761u + (uint32_t)k;
        if (hipMemcpy(data, init.data(), bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemset(res, 0, 64) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            cleanup();
            return POM_E_HIP;
        }
    }
    LitmusParams p;
    p.data = data;
    p.tile_seq = c.tile_seq;
    p.err = c.aux;
    p.out = res;
    p.tiles = tiles;
    p.chain_seq0 = 0;
    p.wait_limit = c.wait_limit;
    const dim3 grid((unsigned)((tiles + 7) / 8 * 8));
    for (int k = 0; k < launches && rc == POM_OK; k++) {
        pom_chain_litmus_kernel<<<grid, dim3(64), 0, st[k % streams]>>>(p);
        if (hipGetLastError() != hipSuccess) rc = POM_E_HIP;
    }
    for (int k = 0; k < streams; k++)
        if (hipStreamSynchronize(st[k]) != hipSuccess) rc = POM_E_HIP;
    if (rc == POM_OK) {
        unsigned long long r3[3] = {0, 0, 0};
        uint32_t flags = 0;
        std::vector<uint32_t> fin((size_t)tiles * POM_TILE_DWORDS);
        std::vector<unsigned long long> words((size_t)tiles * POM_CHAIN_WORD_STRIDE);
        if (hipMemcpy(r3, res, 24, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&flags, c.aux, 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(fin.data(), data, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(words.data(), c.tile_seq, words.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) {
            rc = POM_E_HIP;
        } else {
            int64_t wrong = 0;
            for (int64_t t = 0; t < tiles; t++) {
                const unsigned long long w = words[(size_t)t * POM_CHAIN_WORD_STRIDE];
                bool ok = ((uint32_t)w & POM_CHAIN_COUNT_MASK) == (uint32_t)launches && (uint32_t)(w >> POM_CHAIN_TICKET_SHIFT) == (uint32_t)launches &&
                          !((uint32_t)w & POM_CHAIN_POISON);
                for (int k = 0; k < POM_TILE_DWORDS && ok; k++)
                    ok = fin[(size_t)t * POM_TILE_DWORDS + k] == ((uint32_t)launches ^ ((uint32_t)t * 2654435761u + (uint32_t)k));
                wrong += !ok;
            }
            out[0] = (int64_t)r3[0];
            out[1] = (int64_t)r3[1];
            out[2] = (int64_t)r3[2];
            out[3] = tiles * (int64_t)launches;
            out[4] = wrong;
            out[5] = (int64_t)flags;
        }
    }
    } catch (...) {
        rc = POM_E_NOMEM;
    }
    cleanup();
    return rc;
}

#if defined(POM_CHAIN_DIAG)
/* diagnostic build only: per tile 4 sums over the chained launches so far (cycles to the ticket, cycles polling, cycles in all, polls); cleared */
int pom_chain_diag_read(PomBatch* h, unsigned long long* out, int64_t tiles)
{
    const char* what = !h ? nullptr : !h->chain.tile_seq ? "the handle has no chained launches" : tiles != h->n_pad / h->epw ? "tiles is not the handle's" : nullptr;
    if (int rc = check_call(h, "pom_chain_diag_read", what)) return rc;
    if (int jr = join_parts(h)) return jr;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out, h->chain.tile_seq + tiles * POM_CHAIN_WORD_STRIDE, (size_t)tiles * 544, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->chain.tile_seq + tiles * POM_CHAIN_WORD_STRIDE, 0, (size_t)tiles * 544));
    HIPCHK(hipDeviceSynchronize());
    return POM_OK;
}
#endif
#if defined(POM_DIAG)
/* diagnostic build only: the step kernel with zero ticks = HBM -> LDS -> HBM round trip of every record */
int pom_diag_copy_only(PomBatch* h)
{
    if (int rc = check_call(h, "pom_diag_copy_only")) return rc;
    return launch_step(h, nullptr, 0, 0, 0);
}
/* the accumulators `acc` (rows x cols, a row per wavefront) as they are into `out`, then cleared */
static int diag_fetch(PomBatch* h, long long* acc, size_t rows, int cols, long long* out)
{
    hipError_t e = hipMemcpyAsync(out, acc, rows * cols * 8, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(acc, 0, rows * cols * 8, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) set_err("reading the diagnostic accumulators", e);
    return e == hipSuccess ? POM_OK : POM_E_HIP;
}
/* ... and summed over the rows into out[cols] */
static int diag_sums(PomBatch* h, long long* acc, size_t rows, int cols, long long* out)
{
    long long* tmp = new (std::nothrow) long long[rows * cols]; /* (nothing may throw across the C boundary) */
    if (!tmp) return POM_E_NOMEM;
    const int rc = diag_fetch(h, acc, rows, cols, tmp);
    for (int k = 0; k < cols && !rc; k++) {
        out[k] = 0;
        for (size_t w = 0; w < rows; w++) out[k] += tmp[w * cols + k];
    }
    delete[] tmp;
    return rc;
}
/* diagnostic build only: read and clear the per-phase cycle sums (summed over wavefronts) */
int pom_diag_read(PomBatch* h, long long out[POM_PH_N])
{
    if (int rc = check_call(h, "pom_diag_read", h && !h->diag ? "nothing has been launched yet" : nullptr)) return rc;
    return diag_sums(h, h->diag, (size_t)h->n_waves, POM_PH_N, out);
}
/* diagnostic build only: the per-wavefront accumulators as they are (n_waves x POM_PH_N), then cleared */
int pom_diag_read_raw(PomBatch* h, long long* out, long long max_waves)
{
    const char* what = !h ? nullptr : !h->diag ? "nothing has been launched yet" : max_waves < h->n_waves ? "max_waves is less than the handle's wavefronts" : nullptr;
    if (int rc = check_call(h, "pom_diag_read_raw", what)) return rc;
    if (int jr = join_parts(h)) return jr;
    return diag_fetch(h, h->diag, (size_t)h->n_waves, POM_PH_N, out);
}
/* diagnostic build only: the policy kernel's per-phase sums, read and cleared */
int pom_diag_policy_read(PomBatch* h, long long out[POM_PP_N])
{
    if (int rc = check_call(h, "pom_diag_policy_read", h && !h->diag_pol ? "the policy has not been launched yet" : nullptr)) return rc;
    if (int jr = join_parts(h)) return jr;
    return diag_sums(h, h->diag_pol, (size_t)(h->n_pad / 16), POM_PP_N, out);
}
#endif

int pom_batch_profile(PomBatch* h, int enable)
{
    if (int rc = begin_call(h, "pom_batch_profile", POM_AS_IS)) return rc;
    for (int k = 0; enable && k < 2 * PomBatch::PROF_RING; k++) /* all of them, or the call fails: a slot that exists is kept for the next try */
        if (!h->prof_ev[k]) HIPCHK(hipEventCreate(&h->prof_ev[k]));
    h->profiling = enable != 0;
    h->prof_n = 0;
    return POM_OK;
}

int pom_batch_profile_read(PomBatch* h, double* mean_ms, int64_t* launches)
{
    if (int rc = begin_call(h, "pom_batch_profile_read", POM_SETTLED)) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    double sum = 0;
    for (int k = 0; k < h->prof_n; k++) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, h->prof_ev[2 * k], h->prof_ev[2 * k + 1]));
        sum += ms;
    }
    if (mean_ms) *mean_ms = h->prof_n ? sum / h->prof_n : 0.0;
    if (launches) *launches = h->prof_n;
    h->prof_n = 0;
    return POM_OK;
}

int pom_bench_policy(const uint8_t* codes_dev, int32_t* moves_dev, int64_t first, int64_t count, uint32_t tick, void* stream)
{
    if (!moves_dev || first < 0 || count < 0) return refuse("pom_bench_policy", "moves_dev must not be NULL, first and count not negative");
    if (count == 0) return POM_OK;
    pom_bench_policy_kernel<<<dim3((unsigned)((count + 63) / 64)), dim3(256), 0, (hipStream_t)stream>>>(codes_dev, moves_dev, first, count, tick);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

} /* extern "C" */

#endif /* POM_API_DIAG_H_ */
