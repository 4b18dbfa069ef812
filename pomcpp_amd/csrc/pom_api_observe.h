/*
 * pom_api_observe.h — the observation entry points: what the export kernels ask of their outputs (observe_args; view_args for the
 * fogged views of PomViewSpec), their arguments (observe_params), and the calls that export alone or fused with one tick of explicit
 * moves, plain and as views.  The range call takes the same outputs: pom_api_step.h.
 */
#ifndef POM_API_OBSERVE_H_
#define POM_API_OBSERVE_H_

#include "pom_chain_host.h"

/* the alignment the export kernels ask of their outputs: the planes on 4 elements (an env's four views start on that boundary), the
 * attribute arrays on 16 bytes */
static bool obs_misaligned(const void* planes_dev, int32_t dtype, const void* attrs_a, const void* attrs_b)
{
    const uintptr_t esz = dtype == POM_OBS_F16 ? 2 : dtype == POM_OBS_F32 ? 4 : 1;
    return ((uintptr_t)planes_dev & (4 * esz - 1)) || ((uintptr_t)attrs_a & 15) || ((uintptr_t)attrs_b & 15);
}

/* what every call with a plain observation asks of its outputs (pom_host.h) */
const char* observe_args(const void* planes_dev, int32_t dtype, int32_t per_agent, const int32_t* agent_attrs_dev, const int32_t* env_attrs_dev)
{
    if (!planes_dev) return "planes_dev is NULL";
    if (dtype < POM_OBS_U8 || dtype > POM_OBS_CODES) return "unknown dtype";
    if (dtype == POM_OBS_CODES && per_agent) return "POM_OBS_CODES names the agents by id (10..13), there is no per-agent view of it";
    if (obs_misaligned(planes_dev, dtype, agent_attrs_dev, env_attrs_dev) || (dtype == POM_OBS_U8 && !per_agent && ((uintptr_t)planes_dev & 15)))
        return "output pointers must be 16-byte aligned";
    return nullptr;
}

/* the export kernels' arguments for the whole batch (pom_host.h) */
ObserveParams observe_params(const PomBatch* h, void* planes_dev, int32_t dtype, int32_t per_agent, int32_t* agent_attrs_dev,
                             int32_t* env_attrs_dev, int32_t* viewer_attrs_dev, int32_t view_radius, int32_t view_compact)
{
    ObserveParams p;
    p.state = h->state;
    p.n = h->n;
    p.n_pad = h->n_pad;
    p.block0 = 0;
    p.planes = planes_dev;
    p.agent_attrs = agent_attrs_dev;
    p.env_attrs = env_attrs_dev;
    p.dtype = dtype;
    p.per_agent = per_agent ? 1 : 0;
    p.viewer_attrs = viewer_attrs_dev;
    p.view_radius = view_radius;
    p.view_compact = view_compact;
    return p;
}

/* ---- the fogged views (pom_batch.h PomViewSpec): the observation calls with the four agents' windows ---- */
static_assert(sizeof(PomViewSpec) == POM_VIEW_SPEC_SIZE, "pom_batch.h states the size");
static_assert(sizeof(PomCompactViewSpec) == POM_COMPACT_VIEW_SPEC_SIZE && offsetof(PomCompactViewSpec, view) == 0, "pom_batch.h states the size; a caller passes &spec.view");
const char* view_args(const PomViewSpec* s)
{
    if (s && s->struct_size == POM_COMPACT_VIEW_SPEC_SIZE) { /* the ABI grows by struct_size: the compact form's own fields first */
        const PomCompactViewSpec* c = reinterpret_cast<const PomCompactViewSpec*>(s);
        if (s->reserved_ != 0) return "reserved_ must be 0";
        if (c->reserved2_ != 0) return "reserved2_ must be 0";
        if (c->viewer_mask < 1 || c->viewer_mask > 15) return "viewer_mask must be 1..15";
        if (c->flags & ~(int32_t)POM_VIEW_CENTRED) return "unknown flags (POM_VIEW_CENTRED is the only one)";
        if (s->dtype != POM_OBS_CODES) return "the compact views are code planes: dtype must be POM_OBS_CODES";
    } else if (const char* head = SPEC_HEAD(PomViewSpec, s)) return head;
    if (s->dtype < POM_OBS_U8 || s->dtype > POM_OBS_CODES) return "unknown dtype";
    if (s->view_radius < 0 || s->view_radius > POM_VIEW_RADIUS_MAX) return "view_radius must be 0..10";
    if (!s->planes_dev) return "planes_dev is NULL";
    if (obs_misaligned(s->planes_dev, s->dtype, s->viewer_attrs_dev, s->env_attrs_dev)) /* the rule of per_agent = 1 (observe_args) */
        return "planes_dev must be aligned to 4 elements, the attribute pointers to 16 bytes";
    return nullptr;
}
PomObserveOut view_out(const PomViewSpec* s)
{
    const PomCompactViewSpec* c = reinterpret_cast<const PomCompactViewSpec*>(s);
    return PomObserveOut{s->planes_dev, nullptr, s->env_attrs_dev, s->dtype, 1, 1, s->view_radius, s->viewer_attrs_dev,
                         view_is_compact(s) ? obs_compact_word(c->viewer_mask, c->flags) : 0};
}

extern "C" {

int pom_batch_observe(PomBatch* h, void* planes_dev, int32_t dtype, int32_t per_agent, int32_t* agent_attrs_dev,
                      int32_t* env_attrs_dev)
{
    /* settled, not only joined: after chained launches a tile some visitor could not play is caught up first (chain_settle; free
     * while no chained launch has been issued since the last check) — the planes always describe the state a download returns */
    if (int rc = begin_call(h, "pom_batch_observe", POM_SETTLED, observe_args(planes_dev, dtype, per_agent, agent_attrs_dev, env_attrs_dev))) return rc;
    const ObserveParams p = observe_params(h, planes_dev, dtype, per_agent, agent_attrs_dev, env_attrs_dev);
    pom_observe_kernel<<<dim3((unsigned)((h->n + 15) / 16)), dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

int pom_batch_step_device_observe(PomBatch* h, const int32_t* moves_dev, void* planes_dev, int32_t dtype, int32_t per_agent,
                                  int32_t* agent_attrs_dev, int32_t* env_attrs_dev)
{
    const char* what = !moves_dev ? "moves_dev is NULL" : observe_args(planes_dev, dtype, per_agent, agent_attrs_dev, env_attrs_dev);
    if (int rc = begin_call(h, "pom_batch_step_device_observe", POM_AS_IS, what)) return rc;
    if (!h->quad) { /* the one-lane-per-env shapes have no fused twin: the two launches */
        if (int rc = pom_batch_step_device(h, moves_dev)) return rc;
        return pom_batch_observe(h, planes_dev, dtype, per_agent, agent_attrs_dev, env_attrs_dev);
    }
    const PomObserveOut obs = {planes_dev, agent_attrs_dev, env_attrs_dev, dtype, per_agent ? 1 : 0, 0, 0, nullptr};
    return launch_step(h, moves_dev, 0, 0, 1, false, true, &obs);
}

int pom_batch_observe_view(PomBatch* h, const PomViewSpec* spec)
{
    if (int rc = begin_call(h, "pom_batch_observe_view", POM_SETTLED, view_args(spec))) return rc; /* (settled: as pom_batch_observe) */
    const ObserveParams p = observe_params(h, spec->planes_dev, spec->dtype, 1, nullptr, spec->env_attrs_dev, spec->viewer_attrs_dev, spec->view_radius,
                                           view_out(spec).view_compact);
    if (view_is_compact(spec)) pom_observe_compact_kernel<<<dim3((unsigned)((h->n + 15) / 16)), dim3(64), 0, h->stream>>>(p);
    else pom_observe_view_kernel<<<dim3((unsigned)((h->n + 15) / 16)), dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

int pom_batch_step_device_observe_view(PomBatch* h, const int32_t* moves_dev, const PomViewSpec* spec)
{
    const char* what = !moves_dev ? "moves_dev is NULL" : view_args(spec);
    if (!what && view_is_compact(spec)) what = POM_COMPACT_VIEW_ELSEWHERE;
    if (int rc = begin_call(h, "pom_batch_step_device_observe_view", POM_AS_IS, what)) return rc;
    if (!h->quad) { /* the one-lane-per-env shapes have no fused twin: the two launches */
        if (int rc = pom_batch_step_device(h, moves_dev)) return rc;
        return pom_batch_observe_view(h, spec);
    }
    const PomObserveOut obs = view_out(spec);
    return launch_step(h, moves_dev, 0, 0, 1, false, true, &obs);
}

} /* extern "C" */

#endif /* POM_API_OBSERVE_H_ */
