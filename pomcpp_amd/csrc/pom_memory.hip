/*
 * pom_memory.hip — the view-memory unit of libpom_batch.so: pom_batch_remember_view (pom_batch.h PomMemorySpec), the agents' fogged
 * views merged into their memory for a range of whole tiles, and pom_batch_imagine (PomImagineSpec), playable games built from an
 * agent's view memory into slots of the handle — with their kernels.  What it shares with the other units: pom_host.h, pom_device.h.
 */
#include "pom_host.h"
#include "pom_view_memory.h"
#include "pom_imagine.h"

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

static_assert(sizeof(PomImagineSpec) == POM_IMAGINE_SPEC_SIZE, "pom_batch.h states the size");

extern "C" int pom_batch_imagine(PomBatch* h, const PomImagineSpec* s)
{
    static const char who[] = "pom_batch_imagine";
    /* the spec's own fields first, then the handle and what depends on it */
    const char* what = SPEC_HEAD(PomImagineSpec, s);
    if (what) {}
    else if (s->unknown != POM_IMAGINE_SAMPLE && s->unknown != POM_IMAGINE_PASSAGE) what = "unknown must be POM_IMAGINE_SAMPLE or POM_IMAGINE_PASSAGE";
    else if (s->rows <= 0 || (s->rows & 3)) what = "rows must be a positive multiple of 4";
    else if (s->count < 0) what = "count must be >= 0";
    else if (s->count > 0 && !s->view_dev) what = "view_dev is NULL";
    else if (s->count > 0 && !s->memory_dev) what = "memory_dev is NULL";
    else if (s->count > 0 && !s->viewer_attrs_dev) what = "viewer_attrs_dev is NULL";
    else if (s->count > 0 && (((uintptr_t)s->view_dev & 3) || ((uintptr_t)s->sample_dev & 3) || ((uintptr_t)s->memory_dev & 3) || ((uintptr_t)s->result_dev & 3)))
        what = "view_dev, sample_dev, memory_dev and result_dev must be 4-byte aligned";
    else if (s->count > 0 && (((uintptr_t)s->viewer_attrs_dev & 15) || ((uintptr_t)s->belief_attrs_dev & 15))) what = "the attribute pointers must be 16-byte aligned";
    else if (!h) what = "the handle is NULL";
    else if (s->first < 0 || s->first > h->n || s->count > h->n - s->first) what = "the range [first, first + count) lies outside the batch";
    else if (!h->quad) what = "needs the quad launch shape (envs_per_wave 16, lanes_per_env 4)";
    if (what) return refuse(who, "%s", what);
    if (s->count == 0) return POM_OK;
    /* settled, not only joined (as pom_batch_copy_envs_device); no runtime call at all once the handle is settled: what a capture needs */
    if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
    ImagineParams p;
    p.state = h->state;
    p.snap = h->snap;
    p.agent_mem = h->agent_mem;
    p.view = s->view_dev;
    p.sample = s->sample_dev;
    p.memory = reinterpret_cast<const uint32_t*>(s->memory_dev);
    p.viewer_attrs = s->viewer_attrs_dev;
    p.belief = s->belief_attrs_dev;
    p.result = s->result_dev;
    p.first = s->first;
    p.count = s->count;
    p.n_pad = h->n_pad;
    p.tile0 = s->first / POM_TILE_ENVS;
    p.seed = s->seed;
    p.rows = s->rows;
    p.unknown = s->unknown;
    void* args[1] = {&p};
    HIPCHK(hipLaunchKernel(reinterpret_cast<const void*>(pom_imagine_kernel), dim3((unsigned)((s->first + s->count - 1) / POM_TILE_ENVS - p.tile0 + 1)),
                           dim3(64), args, 0, s->stream ? (hipStream_t)s->stream : h->stream));
    return POM_OK;
}
