/*
 * pom_api_transfer.h — the entry points that move the batch's contents without playing a tick: States in (upload, generate) and out
 * (download, the terminal States), the snapshot, games copied by index (pom_copy.h), and what is read back beside the States —
 * status, last results, episodes, policy memory, counters, the device pointers.
 */
#ifndef POM_API_TRANSFER_H_
#define POM_API_TRANSFER_H_

#include "pom_chain_host.h"
#include "pom_copy.h"

/* The one loop over the staging buffer.  It holds h->staging_envs States (or, as scratch, a few int32 columns per env), so `count` envs
 * pass through it in chunks of that many: queue(offset of the chunk, its envs) puts the chunk's work on the handle's stream, then
 * the stream is synchronised — staging is reused by the next chunk, and what a chunk copied to the host can be read from then on. */
template <class Queue>
static int for_chunks(PomBatch* h, int64_t count, Queue queue)
{
    for (int64_t off = 0; off < count; off += h->staging_envs) {
        if (int rc = queue(off, count - off < h->staging_envs ? count - off : h->staging_envs)) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return POM_OK;
}
/* States out (the range checked by the caller): launch(first env, envs) fills the staging buffer with the States of the chunk */
template <class Launch>
static int download_chunks(PomBatch* h, const char* who, void* states, int64_t first, int64_t count, Launch launch)
{
    if (int rc = begin_call(h, who, POM_SETTLED, !states ? "states is NULL" : nullptr)) return rc;
    return for_chunks(h, count, [&](int64_t off, int64_t c) -> int {
        HIPCHK(hipMemsetAsync(h->staging, 0, (size_t)c * POM_STATE_BYTES, h->stream));
        launch(first + off, c);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync((char*)states + off * POM_STATE_BYTES, h->staging, (size_t)c * POM_STATE_BYTES, hipMemcpyDeviceToHost,
                              h->stream));
        return POM_OK;
    });
}
/* columns out (the same): launch(first env, envs) leaves `nout` arrays of `envs` int32 in the staging buffer (a few ints per env << 251) */
template <class Launch>
static int fetch_columns(PomBatch* h, const char* who, int64_t first, int64_t count, void* const* outs, int nout, Launch launch)
{
    if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
    return for_chunks(h, count, [&](int64_t off, int64_t c) -> int {
        launch(first + off, c);
        HIPCHK(hipGetLastError());
        for (int k = 0; k < nout; k++)
            if (outs[k])
                HIPCHK(hipMemcpyAsync((int32_t*)outs[k] + off, h->staging + (int64_t)k * c, (size_t)c * 4, hipMemcpyDeviceToHost, h->stream));
        return POM_OK;
    });
}

/* pom_batch_copy_envs / _device (pom_copy.h): K1 gathers every destination tile with its new columns, K2 writes the images back;
 * direct = K1 writes the batch's arrays itself (the host variant, where it has seen that no source is a destination) */
static int copy_envs(PomBatch* h, const int64_t* src_dev, int64_t first, int64_t count, int32_t flags, bool direct)
{
    if (count == 0) return POM_OK;
    CopyParams p;
    p.src = src_dev;
    p.first = first;
    p.count = count;
    p.n = h->n;
    p.n_pad = h->n_pad;
    p.tile0 = first / POM_TILE_ENVS;
    p.flags = flags;
    p.state = h->state;
    p.snap = h->snap;
    p.agent_mem = h->agent_mem;
    p.episode = h->episode;
    p.terminal = h->terminal;
    if (direct) {
        p.out_state = h->state;
        p.out_agent_mem = h->agent_mem;
        p.out_episode = h->episode;
        p.out_terminal = h->terminal;
    } else {
        const size_t np = (size_t)h->n_pad;
        if (!h->copy_scratch) { /* state image, agent memory [2][4 * n_pad], episode, terminal: laid out like the real arrays */
            const size_t words = np * (POM_REC_DWORDS + 9 + (h->terminal ? POM_REC_DWORDS : 0));
            hipError_t e = hipMalloc((void**)&h->copy_scratch, words * 4);
            if (e != hipSuccess) {
                h->copy_scratch = nullptr;
                set_err("pom_batch_copy_envs: scratch", e);
                return e == hipErrorOutOfMemory ? POM_E_NOMEM : POM_E_HIP;
            }
        }
        p.out_state = h->copy_scratch;
        p.out_agent_mem = h->copy_scratch + np * POM_REC_DWORDS;
        p.out_episode = p.out_agent_mem + np * 8;
        p.out_terminal = h->terminal ? p.out_episode + np : nullptr;
    }
    const unsigned tiles = (unsigned)((first + count - 1) / POM_TILE_ENVS - p.tile0 + 1);
    pom_copy_gather_kernel<<<dim3(tiles), dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    if (!direct) {
        pom_copy_scatter_kernel<true><<<dim3(tiles), dim3(64), 0, h->stream>>>(p);
        HIPCHK(hipGetLastError());
    } else if (flags & POM_COPY_SET_SNAPSHOT) {
        pom_copy_scatter_kernel<false><<<dim3(tiles), dim3(64), 0, h->stream>>>(p);
        HIPCHK(hipGetLastError());
    }
    return POM_OK;
}

static int copy_check(PomBatch* h, const char* who, const void* src, int64_t first, int64_t count, int32_t flags)
{
    if (int rc = check_range(h, who, first, count)) return rc;
    if ((flags & ~(POM_COPY_FROM_SNAPSHOT | POM_COPY_SET_SNAPSHOT)) != 0 || (!src && count > 0))
        return refuse(who, "unknown flags 0x%x or no index array", (unsigned)flags);
    return POM_OK;
}

extern "C" {

int pom_batch_upload(PomBatch* h, const void* states, int64_t first, int64_t count)
{
    static const char who[] = "pom_batch_upload";
    if (int rc = check_range(h, who, first, count)) return rc;
    if (int rc = begin_call(h, who, POM_SETTLED, !states ? "states is NULL" : nullptr)) return rc;
    const int big = INT_MAX;
    HIPCHK(hipMemcpyAsync(h->first_bad, &big, sizeof big, hipMemcpyHostToDevice, h->stream));
    /* the kernel leaves the first env of a chunk it could not pack: `fb` holds the answer for the chunk before, synchronised since */
    int fb = big;
    int64_t fb_first = 0, bad_env = -1;
    auto note_bad = [&]() -> int {
        if (fb == big || bad_env >= 0) return POM_OK;
        bad_env = fb_first + fb;
        HIPCHK(hipMemcpyAsync(h->first_bad, &big, sizeof big, hipMemcpyHostToDevice, h->stream));
        return POM_OK;
    };
    const int rc = for_chunks(h, count, [&](int64_t off, int64_t c) -> int {
        if (int br = note_bad()) return br;
        HIPCHK(hipMemcpyAsync(h->staging, (const char*)states + off * POM_STATE_BYTES, (size_t)c * POM_STATE_BYTES,
                              hipMemcpyHostToDevice, h->stream));
        pom_pack_kernel<<<dim3((unsigned)((c + 63) / 64)), dim3(64), 0, h->stream>>>(h->staging, first + off, c, h->state, h->snap,
                                                                                     h->n_pad, h->first_bad);
        HIPCHK(hipGetLastError());
        fb_first = first + off;
        HIPCHK(hipMemcpyAsync(&fb, h->first_bad, sizeof fb, hipMemcpyDeviceToHost, h->stream));
        return POM_OK;
    });
    if (rc) return rc;
    if (int br = note_bad()) return br;
    HIPCHK(hipMemsetAsync(h->episode + first, 0, (size_t)count * 4, h->stream)); /* an uploaded state is episode 0 of its env */
    if (h->terminal) HIPCHK(hipMemsetAsync(h->terminal + first * POM_REC_DWORDS, 0, (size_t)count * POM_REC_DWORDS * 4, h->stream));
    if (h->agent_mem) { /* uploaded envs start new games: fresh agents */
        HIPCHK(hipMemsetAsync(h->agent_mem + first * 4, 0, (size_t)count * 16, h->stream));
        HIPCHK(hipMemsetAsync(h->agent_mem + 4 * h->n_pad + first * 4, 0, (size_t)count * 16, h->stream));
    }
    if (bad_env >= 0) {
        snprintf(g_err, sizeof g_err, "pom_batch_upload: env %lld holds a value outside the representable game states "
                 "(it was replaced by a finished blank board)", (long long)bad_env);
        return POM_E_UNREPRESENTABLE;
    }
    return POM_OK;
}

int pom_batch_download(PomBatch* h, void* states, int64_t first, int64_t count)
{
    static const char who[] = "pom_batch_download";
    if (int rc = check_range(h, who, first, count)) return rc;
    return download_chunks(h, who, states, first, count, [h](int64_t e0, int64_t c) {
        pom_unpack_kernel<<<dim3((unsigned)((c + 63) / 64)), dim3(64), 0, h->stream>>>(h->state, e0, c, h->n_pad, h->staging);
    });
}

int pom_batch_download_terminal(PomBatch* h, void* states, int64_t first, int64_t count)
{
    static const char who[] = "pom_batch_download_terminal";
    if (int rc = check_range(h, who, first, count)) return rc;
    if (!h->terminal) return refuse(who, "the batch was not created with auto_reset = POM_RESET_AT_END");
    return download_chunks(h, who, states, first, count, [h](int64_t e0, int64_t c) {
        pom_unpack_aos_kernel<<<dim3((unsigned)((c + 63) / 64)), dim3(64), 0, h->stream>>>(h->terminal, e0, c, h->staging);
    });
}

int pom_batch_generate(PomBatch* h, uint64_t board_seed)
{
    if (int rc = begin_call(h, "pom_batch_generate", POM_SETTLED)) return rc;
    h->board_seed = board_seed;
    pom_generate_kernel<<<dim3((unsigned)((h->n + 15) / 16)), dim3(64), 0, h->stream>>>(h->state, h->snap, h->episode, h->n, h->n_pad,
                                                                                         h->env_offset, board_seed);
    HIPCHK(hipGetLastError());
    if (h->agent_mem) HIPCHK(hipMemsetAsync(h->agent_mem, 0, (size_t)h->n_pad * 32, h->stream)); /* new games: fresh agents */
    if (h->terminal) HIPCHK(hipMemsetAsync(h->terminal, 0, (size_t)h->n_pad * POM_REC_DWORDS * 4, h->stream));
    return POM_OK;
}

int pom_batch_snapshot(PomBatch* h)
{
    if (int rc = begin_call(h, "pom_batch_snapshot", POM_SETTLED)) return rc;
    pom_snapshot_kernel<<<dim3((unsigned)((h->n_pad + 255) / 256)), dim3(256), 0, h->stream>>>(h->state, h->snap, h->n_pad);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

int pom_batch_copy_envs(PomBatch* h, const int64_t* src_host, int64_t first, int64_t count, int32_t flags)
{
    static const char who[] = "pom_batch_copy_envs";
    if (int rc = copy_check(h, who, src_host, first, count, flags)) return rc;
    bool overlap = false;
    for (int64_t i = 0; i < count; i++) {
        const int64_t s = src_host[i];
        if (s >= h->n) return refuse(who, "src[%lld] = %lld is not an env of the batch (n = %lld)", (long long)i, (long long)s, (long long)h->n);
        overlap |= s >= first && s < first + count;
    }
    if (count == 0) return POM_OK;
    if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
    if (!h->copy_idx) {
        hipError_t e = hipMalloc((void**)&h->copy_idx, (size_t)h->n_pad * sizeof(int64_t));
        if (e != hipSuccess) {
            h->copy_idx = nullptr;
            set_err("pom_batch_copy_envs: index buffer", e);
            return e == hipErrorOutOfMemory ? POM_E_NOMEM : POM_E_HIP;
        }
    }
    HIPCHK(hipMemcpyAsync(h->copy_idx, src_host, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    return copy_envs(h, h->copy_idx, first, count, flags, !overlap);
}

int pom_batch_copy_envs_device(PomBatch* h, const int64_t* src_dev, int64_t first, int64_t count, int32_t flags)
{
    static const char who[] = "pom_batch_copy_envs_device";
    if (int rc = copy_check(h, who, src_dev, first, count, flags)) return rc;
    if (count == 0) return POM_OK;
    if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
    return copy_envs(h, src_dev, first, count, flags, false);
}

int pom_batch_status(PomBatch* h, int64_t first, int64_t count, int32_t* done, int32_t* winner, int32_t* draw, int32_t* alive,
                     int32_t* time_step, uint32_t* ubflags)
{
    static const char who[] = "pom_batch_status";
    if (int rc = check_range(h, who, first, count)) return rc;
    void* outs[6] = {done, winner, draw, alive, time_step, ubflags};
    return fetch_columns(h, who, first, count, outs, 6, [h](int64_t e0, int64_t c) {
        pom_status_kernel<<<dim3((unsigned)((c + 255) / 256)), dim3(256), 0, h->stream>>>(h->state, e0, c, h->n_pad, h->staging);
    });
}

int pom_batch_last_results(PomBatch* h, int64_t first, int64_t count, int32_t* finished, int32_t* winner, int32_t* draw,
                           int32_t* length, int32_t* alive)
{
    static const char who[] = "pom_batch_last_results";
    if (int rc = check_range(h, who, first, count)) return rc;
    if (!h->terminal) return refuse(who, "the batch was not created with auto_reset = POM_RESET_AT_END");
    void* outs[5] = {finished, winner, draw, length, alive};
    return fetch_columns(h, who, first, count, outs, 5, [h](int64_t e0, int64_t c) {
        pom_results_kernel<<<dim3((unsigned)((c + 255) / 256)), dim3(256), 0, h->stream>>>(h->state, h->terminal, e0, c, h->n_pad, h->staging);
    });
}

int pom_batch_episodes(PomBatch* h, int64_t first, int64_t count, uint32_t* out)
{
    static const char who[] = "pom_batch_episodes";
    if (int rc = check_range(h, who, first, count)) return rc;
    if (int rc = begin_call(h, who, POM_SETTLED, !out ? "out is NULL" : nullptr)) return rc;
    HIPCHK(hipMemcpyAsync(out, h->episode + first, (size_t)count * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return POM_OK;
}

int pom_batch_policy_memory(PomBatch* h, int64_t first, int64_t count, int32_t* out16)
{
    static const char who[] = "pom_batch_policy_memory";
    if (int rc = check_range(h, who, first, count)) return rc;
    if (int rc = begin_call(h, who, POM_SETTLED, !out16 ? "out16 is NULL" : nullptr)) return rc;
    if (!h->agent_mem) {
        memset(out16, 0, (size_t)count * 4 * 16 * sizeof(int32_t));
        return POM_OK;
    }
    uint32_t* tmp = new (std::nothrow) uint32_t[(size_t)count * 8];
    if (!tmp) return POM_E_NOMEM;
    hipError_t e1 = hipMemcpyAsync(tmp, h->agent_mem + first * 4, (size_t)count * 16, hipMemcpyDeviceToHost, h->stream);
    hipError_t e2 = hipMemcpyAsync(tmp + count * 4, h->agent_mem + 4 * h->n_pad + first * 4, (size_t)count * 16, hipMemcpyDeviceToHost, h->stream);
    hipError_t e3 = hipStreamSynchronize(h->stream);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
        delete[] tmp;
        set_err("policy memory download", e1 != hipSuccess ? e1 : e2 != hipSuccess ? e2 : e3);
        return POM_E_HIP;
    }
    for (int64_t k = 0; k < count * 4; k++) pom_policy_mem_unpack(tmp[k], tmp[count * 4 + k], out16 + 16 * k);
    delete[] tmp;
    return POM_OK;
}

int pom_batch_counters_device(PomBatch* h, void* dev_int64x4)
{
    if (int rc = begin_call(h, "pom_batch_counters_device", POM_JOINED, !dev_int64x4 ? "dev_int64x4 is NULL" : nullptr)) return rc;
    pom_reduce_counters_kernel<<<dim3(1), dim3(1024), 0, h->stream>>>(h->wave_counters, h->n_waves, (int64_t*)dev_int64x4);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

int pom_batch_counters(PomBatch* h, int64_t out[POM_CNT_N])
{
    /* (settled: a tile left behind by chained launches is caught up first: its steps count) */
    if (int rc = begin_call(h, "pom_batch_counters", POM_SETTLED, !out ? "out is NULL" : nullptr)) return rc;
    int rc = pom_batch_counters_device(h, h->totals_dev);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, h->totals_dev, POM_CNT_N * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return POM_OK;
}

int pom_batch_reset_counters(PomBatch* h)
{
    if (int rc = begin_call(h, "pom_batch_reset_counters", POM_SETTLED)) return rc;
    HIPCHK(hipMemsetAsync(h->wave_counters, 0, (size_t)h->n_waves * POM_CNT_N * 8, h->stream));
    return POM_OK;
}

int pom_batch_moves_device(PomBatch* h, int32_t** moves_dev)
{
    /* (joined: what the caller queues on the handle's stream next sees the policy's moves) */
    if (int rc = begin_call(h, "pom_batch_moves_device", POM_JOINED, !moves_dev ? "moves_dev is NULL" : nullptr)) return rc;
    *moves_dev = h->moves_dev;
    return POM_OK;
}

int pom_batch_device_view(PomBatch* h, void** base, int64_t* n_pad, int32_t* rec_dwords)
{
    if (int rc = begin_call(h, "pom_batch_device_view", POM_SETTLED)) return rc;
    if (base) *base = h->state;
    if (n_pad) *n_pad = h->n_pad;
    if (rec_dwords) *rec_dwords = POM_REC_DWORDS;
    return POM_OK;
}

} /* extern "C" */

#endif /* POM_API_TRANSFER_H_ */
