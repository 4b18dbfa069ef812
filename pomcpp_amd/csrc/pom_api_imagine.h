/*
 * pom_api_imagine.h — the entry point pom_batch_imagine (pom_batch.h PomImagineSpec): playable games built from an agent's view memory
 * into slots of the handle.  Its kernel header is included right in front of it, after every other kernel of the library: the order
 * kernels are emitted in stays.
 */
#ifndef POM_API_IMAGINE_H_
#define POM_API_IMAGINE_H_

#include "pom_api_memory.h"
#include "pom_imagine.h"

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

#endif /* POM_API_IMAGINE_H_ */
