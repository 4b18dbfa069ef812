/*
 * pom_mixed.hip — the mixed-step unit of libpom_batch.so: pom_batch_step_mixed (pom_batch.h PomMixedStepSpec), the closed-loop range
 * call with SimpleAgent for the agents of simple_mask, and its kernel.  What it shares with the other units: pom_host.h, pom_device.h.
 */
#include "pom_host.h"
#include "pom_step_mixed.h"

static_assert(sizeof(PomMixedStepSpec) == POM_MIXED_STEP_SPEC_SIZE, "pom_batch.h states the size");

/* Which instantiation of pom_step_mixed_kernel a launch runs: fresh boards x reset at the end (as step_kernel's table) x {no
 * observation, plain, fogged views} */
typedef void (*PomMixedKernel)(MixedStepParams);
static PomMixedKernel mixed_kernel(const PomBatch* h, bool observe, bool view)
{
    static const PomMixedKernel k[3][4] = { /* [none / plain / views][fresh * 2 + at_end] */
        {pom_step_mixed_kernel<false, false, false, false>, pom_step_mixed_kernel<false, true, false, false>,
         pom_step_mixed_kernel<true, false, false, false>, pom_step_mixed_kernel<true, true, false, false>},
        {pom_step_mixed_kernel<false, false, true, false>, pom_step_mixed_kernel<false, true, true, false>,
         pom_step_mixed_kernel<true, false, true, false>, pom_step_mixed_kernel<true, true, true, false>},
        {pom_step_mixed_kernel<false, false, true, true>, pom_step_mixed_kernel<false, true, true, true>,
         pom_step_mixed_kernel<true, false, true, true>, pom_step_mixed_kernel<true, true, true, true>}};
    return k[view ? 2 : observe ? 1 : 0][2 * (runs_fresh(h) ? 1 : 0) + (runs_at_end(h) ? 1 : 0)];
}

extern "C" int pom_batch_step_mixed(PomBatch* h, const PomMixedStepSpec* s)
{
    static const char who[] = "pom_batch_step_mixed";
    /* the spec's own fields first, then the handle and what depends on it */
    const char* what = !h ? "the handle is NULL" : SPEC_HEAD(PomMixedStepSpec, s);
    if (what) {}
    else if (s->flags != 0) what = "flags must be 0";
    else if (s->simple_mask < 0 || s->simple_mask > 15) what = "simple_mask must be 0..15";
    else if (s->tick < 0 || s->tick > (int64_t)UINT32_MAX) what = "tick must be 0..4294967295";
    else if (!s->moves_dev && s->simple_mask != 15) what = "moves_dev is NULL and simple_mask leaves agents to it";
    else if ((uintptr_t)s->moves_dev & 3) what = "moves_dev must be 4-byte aligned";
    else if (s->view && s->planes_dev) what = "view and planes_dev are two forms of one observation: pass one";
    else if (s->view && s->env_attrs_dev) what = "with view the env_attrs go to view->env_attrs_dev: env_attrs_dev must be NULL";
    if (what) return refuse(who, "%s", what);
    /* (the range rules are range_args'; its moves rule is stated above for this call: with all four agents in the mask there are none) */
    if (int rc = range_args(h, who, s->first, s->count, s->moves_dev ? s->moves_dev : reinterpret_cast<const int32_t*>(s))) return rc;
    PomObserveOut obs = {s->planes_dev, s->agent_attrs_dev, s->env_attrs_dev, s->dtype, s->per_agent ? 1 : 0, 0, 0, nullptr};
    if (s->view) {
        if (const char* va = view_args(s->view)) return refuse(who, "%s", va);
        obs = view_out(s->view);
    } else if (s->planes_dev) {
        if (const char* oa = observe_args(s->planes_dev, s->dtype, s->per_agent, s->agent_attrs_dev, s->env_attrs_dev)) return refuse(who, "%s", oa);
    }
    if (s->simple_mask && !h->agent_mem) {
        /* the one call that allocates: the agents' memory, cleared on the handle's stream — and waited for, because the launches that
         * use it go to the CALLER's streams, which nothing else orders behind the clear */
        if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
        if (int rc = ensure_agent_mem(h)) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    if (s->count == 0) return POM_OK;
    /* (settling is free, and no runtime call at all, once the handle is settled: what a graph capture needs) */
    if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
    MixedStepParams p;
    p.state = h->state;
    p.snap = h->snap;
    p.moves = s->moves_dev;
    p.agent_mem = h->agent_mem;
    p.episode = h->episode;
    p.terminal = h->terminal;
    p.wave_counters = h->wave_counters;
    p.n = h->n;
    p.n_pad = h->n_pad;
    p.env_offset = h->env_offset;
    p.block0 = s->first / 16;
    p.seed = s->seed;
    p.board_seed = h->board_seed;
    p.tick = (uint32_t)s->tick;
    p.simple_mask = s->simple_mask;
    p.mode = h->mode;
    p.auto_reset = h->auto_reset;
    p.max_steps = h->max_steps;
    const bool observe = s->view || s->planes_dev;
    p.obs_planes = observe ? obs.planes : nullptr;
    p.obs_agent_attrs = observe ? obs.agent_attrs : nullptr;
    p.obs_env_attrs = observe ? obs.env_attrs : nullptr;
    p.obs_viewer_attrs = s->view ? obs.viewer_attrs : nullptr;
    p.obs_dtype = observe ? obs.dtype : 0;
    p.obs_per_agent = observe ? obs.per_agent : 0;
    p.obs_view_radius = s->view ? obs.view_radius : 0;
    const void* kernel = reinterpret_cast<const void*>(mixed_kernel(h, observe, s->view != nullptr));
    void* args[1] = {&p};
    HIPCHK(hipLaunchKernel(kernel, dim3((unsigned)((s->first + s->count + 15) / 16 - p.block0)), dim3(64), args, 0,
                           s->stream ? (hipStream_t)s->stream : h->stream));
    return POM_OK;
}
