/*
 * pom_api_memory.h — the entry point pom_batch_remember_view (pom_batch.h PomMemorySpec): the agents' fogged views merged into their
 * memory for a range of whole tiles.  Its kernel header is included right in front of it, after every other kernel of the library: the
 * order kernels are emitted in stays.
 */
#ifndef POM_API_MEMORY_H_
#define POM_API_MEMORY_H_

#include "pom_api_step.h"
#include "pom_view_memory.h"

static_assert(sizeof(PomMemorySpec) == POM_MEMORY_SPEC_SIZE, "pom_batch.h states the size");

extern "C" int pom_batch_remember_view(PomBatch* h, int64_t first, int64_t count, const PomMemorySpec* s, void* stream)
{
    static const char who[] = "pom_batch_remember_view";
    /* the spec's own fields first, then the handle and what depends on it */
    const char* what = !h ? "the handle is NULL" : SPEC_HEAD(PomMemorySpec, s);
    if (what) {}
    else if (s->reserved_ != 0) what = "reserved_ must be 0";
    else if (s->view_radius < 0 || s->view_radius > POM_VIEW_RADIUS_MAX) what = "view_radius must be 0..10";
    else if (s->agent_mask < 1 || s->agent_mask > 15) what = "agent_mask must be 1..15";
    else if (!s->memory_dev) what = "memory_dev is NULL";
    else if (!s->stamp_dev) what = "stamp_dev is NULL";
    else if (((uintptr_t)s->memory_dev & 3) || ((uintptr_t)s->stamp_dev & 7)) what = "memory_dev must be 4-byte, stamp_dev 8-byte aligned";
    else if (((uintptr_t)s->viewer_attrs_dev & 15) || ((uintptr_t)s->env_attrs_dev & 15)) what = "the attribute pointers must be 16-byte aligned";
    if (what) return refuse(who, "%s", what);
    /* (the range rules are range_args'; there are no moves here: its moves rule is given something that is not NULL) */
    if (int rc = range_args(h, who, first, count, reinterpret_cast<const int32_t*>(s))) return rc;
    if (count == 0) return POM_OK;
    /* (settling is free, and no runtime call at all, once the handle is settled: what a graph capture needs) */
    if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
    ViewMemoryParams p;
    p.state = h->state;
    p.episode = h->episode;
    p.memory = reinterpret_cast<uint32_t*>(s->memory_dev);
    p.stamp = s->stamp_dev;
    p.viewer_attrs = s->viewer_attrs_dev;
    p.env_attrs = s->env_attrs_dev;
    p.n = h->n;
    p.block0 = first / 16;
    p.view_radius = s->view_radius;
    p.agent_mask = s->agent_mask;
    /* tiles of the range, rounded up to a multiple of 8 as the rollouts' grid (rollout_begin): POM_MEM_SPLIT wavefronts per tile */
    p.tiles = (uint32_t)((first + count + 15) / 16 - p.block0);
    p.tiles8 = (p.tiles + 7) / 8 * 8;
    static_assert((((int64_t)1 << 30) / 16 + 8) * POM_MEM_SPLIT < (int64_t)INT_MAX, "the largest batch (create_plan) fits one grid");
    void* args[1] = {&p};
    HIPCHK(hipLaunchKernel(reinterpret_cast<const void*>(pom_view_memory_kernel), dim3(p.tiles8 * POM_MEM_SPLIT), dim3(64),
                           args, 0, stream ? (hipStream_t)stream : h->stream));
    return POM_OK;
}

#endif /* POM_API_MEMORY_H_ */
