/*
 * pom_api_step.h — the entry points that play ticks: explicit moves from the host or the device (one tick, a tape of ticks), the
 * synthetic move streams (pom_batch_step_random), SimpleAgent's moves (the policy calls), and the closed-loop range call with its
 * optional observation.
 */
#ifndef POM_API_STEP_H_
#define POM_API_STEP_H_

#include "pom_chain_host.h"

/* closed-loop stepping: one tick for a range of whole tiles, one launch on the caller's stream, nothing forked or joined
 * (range_args: pom_host.h) */
int range_args(PomBatch* h, const char* who, int64_t first, int64_t count, const int32_t* moves_dev)
{
    if (int rc = check_range(h, who, first, count)) return rc;
    if (!moves_dev) return refuse(who, "moves_dev is NULL");
    if (!h->quad || (first & 15) || ((count & 15) && first + count != h->n))
        return refuse(who, "whole tiles of 16 envs (first %lld, count %lld), quad launch shape", (long long)first, (long long)count);
    return POM_OK;
}
static int launch_range(PomBatch* h, const char* who, int64_t first, int64_t count, const int32_t* moves_dev, void* stream, const PomObserveOut* obs)
{
    if (count == 0) return POM_OK;
    /* (settling is free, and no runtime call at all, once the handle is settled: what a graph capture needs) */
    if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
    StepParams p;
    if (int fr = fill_params(h, p, moves_dev, 0, 0, 1, obs)) return fr;
    p.block0 = first / 16;
    p.block_end = (first + count + 15) / 16;
    const void* kernel = reinterpret_cast<const void*>(step_kernel(h, false, 1, false, obs != nullptr, obs && obs->view));
    void* args[1] = {&p};
    HIPCHK(hipLaunchKernel(kernel, dim3((unsigned)((p.block_end - p.block0 + POM_WPB - 1) / POM_WPB)), dim3(64 * POM_WPB), args, 0,
                           stream ? (hipStream_t)stream : h->stream));
    return POM_OK;
}
/* the range call with a plain observation or none, under the name of the entry point that was called */
static int step_range(PomBatch* h, const char* who, int64_t first, int64_t count, const int32_t* moves_dev, void* stream, void* planes_dev,
                      int32_t dtype, int32_t per_agent, int32_t* agent_attrs_dev, int32_t* env_attrs_dev)
{
    if (int rc = range_args(h, who, first, count, moves_dev)) return rc;
    if (planes_dev)
        if (const char* what = observe_args(planes_dev, dtype, per_agent, agent_attrs_dev, env_attrs_dev)) return refuse(who, "%s", what);
    const PomObserveOut obs = {planes_dev, agent_attrs_dev, env_attrs_dev, dtype, per_agent ? 1 : 0, 0, 0, nullptr};
    return launch_range(h, who, first, count, moves_dev, stream, planes_dev ? &obs : nullptr);
}

extern "C" {

int pom_batch_step(PomBatch* h, const int32_t* moves_host)
{
    /* (settled: the previous step's parts still read moves_dev) */
    if (int rc = begin_call(h, "pom_batch_step", POM_SETTLED, !moves_host ? "moves_host is NULL" : nullptr)) return rc;
    HIPCHK(hipMemcpyAsync(h->moves_dev, moves_host, (size_t)h->n * 16, hipMemcpyHostToDevice, h->stream));
    return launch_step(h, h->moves_dev, 0, 0, 1, false, true);
}

int pom_batch_step_device(PomBatch* h, const int32_t* moves_dev)
{
    if (int rc = begin_call(h, "pom_batch_step_device", POM_AS_IS, !moves_dev ? "moves_dev is NULL" : nullptr)) return rc;
    /* the moves were produced on the caller's stream and may be overwritten there right after this call */
    return launch_step(h, moves_dev, 0, 0, 1, false, true);
}

int pom_batch_step_device_many(PomBatch* h, const int32_t* moves_dev, int32_t ticks)
{
    const char* what = !moves_dev ? "moves_dev is NULL" : ticks < 0 ? "ticks must be >= 0" : nullptr;
    if (int rc = check_call(h, "pom_batch_step_device_many", what)) return rc;
    if (ticks == 0) return POM_OK;
    HIPCHK(hipSetDevice(h->device));
    /* chained where the handle chains: one launch over all tiles per tick, the launches on different streams, a tile's visitor at
     * distance d from the call's first visit reads tick d of the tape (pom_chain.h).  Elsewhere, and for a single tick: plain
     * launches in a row on the caller's stream, as pom_batch_step_device. */
    if (ticks >= 2 && runs_chain(h, 1)) {
        StepParams p;
        memset(&p, 0, sizeof p);
        if (int rc = fill_params(h, p, moves_dev, 0, 0, 1)) return rc;
        bool used = false;
        const uint64_t tick_before = h->tick;
        const int rc = launch_many_chain(h, p, ticks, false, &used);
        h->tick = tick_before; /* explicit moves do not advance the tick that keys the synthetic stream (as pom_batch_step_device) */
        if (rc || used) return rc;
    }
    for (int32_t t = 0; t < ticks; t++)
        if (int rc = launch_step(h, moves_dev + (int64_t)t * h->n * 4, 0, 0, 1, false, true)) return rc;
    return POM_OK;
}

int pom_batch_step_random(PomBatch* h, uint64_t seed, int32_t dist, int32_t ticks, int32_t ticks_per_launch)
{
    const char* what = ticks < 0 ? "ticks must be >= 0"
                       : ticks_per_launch < 1 ? "ticks_per_launch must be >= 1"
                       : dist < POM_DIST_HARMLESS || dist > POM_DIST_STRESS ? "dist must be POM_DIST_HARMLESS, _RANDOM or _STRESS"
                                                                            : nullptr;
    if (int rc = begin_call(h, "pom_batch_step_random", POM_AS_IS, what)) return rc;
    /* ticks_per_launch is a request: results never depend on it, and the modes whose several-tick kernels would spill run one
     * tick per launch (max_ticks_per_launch) */
    const int32_t cap = max_ticks_per_launch(h, false);
    const int32_t tpl = ticks_per_launch < cap ? ticks_per_launch : cap;
    const int32_t whole = ticks / tpl;
    if (int rc = launch_many(h, seed, dist, whole, tpl, false)) return rc;
    const int32_t rest = ticks - whole * tpl;
    if (rest > 0) {
        if (int rc = launch_step(h, nullptr, seed, dist, rest)) return rc;
        h->tick += (uint64_t)rest;
    }
    return POM_OK;
}

int pom_batch_policy_simple(PomBatch* h, uint64_t seed, int32_t* moves_out_host)
{
    if (int rc = begin_call(h, "pom_batch_policy_simple", POM_AS_IS)) return rc;
    int rc = launch_policy(h, seed);
    if (rc) return rc;
    if (moves_out_host) {
        if (int jr = quiesce(h)) return jr;
        HIPCHK(hipMemcpyAsync(moves_out_host, h->moves_dev, (size_t)h->n * 16, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return POM_OK;
}

int pom_batch_step_policy(PomBatch* h)
{
    if (int rc = begin_call(h, "pom_batch_step_policy", POM_AS_IS)) return rc;
    int rc = launch_step(h, h->moves_dev, 0, 0, 1);
    if (rc) return rc;
    h->tick += 1;
    return POM_OK;
}

int pom_batch_step_simple(PomBatch* h, uint64_t seed, int32_t ticks)
{
    if (int rc = begin_call(h, "pom_batch_step_simple", POM_AS_IS, ticks < 0 ? "ticks must be >= 0" : nullptr)) return rc;
    if (h->quad && h->fuse_policy) { /* the fused kernel: policy and tick on one load of the record */
        if (int rc = ensure_agent_mem(h)) return rc;
        return launch_many(h, seed, 0, ticks, 1, true);
    }
    for (int32_t t = 0; t < ticks; t++) {
        int rc = launch_policy(h, seed);
        if (!rc) rc = launch_step(h, h->moves_dev, 0, 0, 1);
        if (rc) return rc;
        h->tick += 1;
    }
    return POM_OK;
}

int pom_batch_step_device_range(PomBatch* h, int64_t first, int64_t count, const int32_t* moves_dev, void* stream, void* planes_dev,
                                int32_t dtype, int32_t per_agent, int32_t* agent_attrs_dev, int32_t* env_attrs_dev)
{
    return step_range(h, "pom_batch_step_device_range", first, count, moves_dev, stream, planes_dev, dtype, per_agent, agent_attrs_dev, env_attrs_dev);
}

int pom_batch_step_device_range_view(PomBatch* h, int64_t first, int64_t count, const int32_t* moves_dev, void* stream, const PomViewSpec* spec)
{
    static const char who[] = "pom_batch_step_device_range_view";
    if (!spec) return step_range(h, who, first, count, moves_dev, stream, nullptr, 0, 0, nullptr, nullptr); /* NULL: no observation */
    if (int rc = range_args(h, who, first, count, moves_dev)) return rc;
    if (const char* what = view_args(spec)) return refuse(who, "%s", what);
    if (view_is_compact(spec)) return refuse(who, "%s", POM_COMPACT_VIEW_ELSEWHERE);
    const PomObserveOut obs = view_out(spec);
    return launch_range(h, who, first, count, moves_dev, stream, &obs);
}

} /* extern "C" */

#endif /* POM_API_STEP_H_ */
