/*
 * pom_mixed_host.h — the host side that pom_batch_step_mixed (pom_mixed.hip) and pom_batch_step_events (pom_events.hip) share: what is
 * refused of a PomMixedStepSpec, and how a spec that passed becomes the kernel's parameters and its grid.  Stated once, for both: each
 * call brings its own name for the refusals and its own table of kernels.
 */
#ifndef POM_MIXED_HOST_H_
#define POM_MIXED_HOST_H_

#include "pom_host.h"
#include "pom_step_mixed.h"

static_assert(sizeof(PomMixedStepSpec) == POM_MIXED_STEP_SPEC_SIZE, "pom_batch.h states the size");

/* which of the kernel's sixteen instantiations a launch runs: [none / plain / views / compact views][fresh * 2 + at_end] (as
 * step_kernel's table); KC: the COMPACT kernel */
#define POM_MIXED_KERNEL_TABLE(K, KC)                                                                                                 \
    {{K<false, false, false, false>, K<false, true, false, false>, K<true, false, false, false>, K<true, true, false, false>},       \
     {K<false, false, true, false>, K<false, true, true, false>, K<true, false, true, false>, K<true, true, true, false>},           \
     {K<false, false, true, true>, K<false, true, true, true>, K<true, false, true, true>, K<true, true, true, true>},               \
     {KC<false, false>, KC<false, true>, KC<true, false>, KC<true, true>}}
inline int mixed_kernel_row(const PomMixedStepSpec* s) { return s->view ? (view_is_compact(s->view) ? 3 : 2) : s->planes_dev ? 1 : 0; }
inline int mixed_kernel_column(const PomBatch* h) { return 2 * (runs_fresh(h) ? 1 : 0) + (runs_at_end(h) ? 1 : 0); }

/* The checks: the spec's own fields first, then the handle and what depends on it.  POM_OK, with the observation's outputs in `obs`, or
 * the refusal by the name `who`; nothing of the handle has been touched */
static int mixed_step_args(PomBatch* h, const char* who, const PomMixedStepSpec* s, PomObserveOut& obs)
{
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
    obs = {s->planes_dev, s->agent_attrs_dev, s->env_attrs_dev, s->dtype, s->per_agent ? 1 : 0, 0, 0, nullptr};
    if (s->view) {
        if (const char* va = view_args(s->view)) return refuse(who, "%s", va);
        obs = view_out(s->view);
    } else if (s->planes_dev) {
        if (const char* oa = observe_args(s->planes_dev, s->dtype, s->per_agent, s->agent_attrs_dev, s->env_attrs_dev)) return refuse(who, "%s", oa);
    }
    return POM_OK;
}

/* A spec that passed mixed_step_args: the agents' memory if the mask needs it, the handle settled, and the launch's parameters.
 * `launch` is false when there is nothing to launch (count == 0) */
static int mixed_step_begin(PomBatch* h, const char* who, const PomMixedStepSpec* s, const PomObserveOut& obs, MixedStepParams& p, bool& launch)
{
    launch = false;
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
    p.obs_view_compact = s->view ? obs.view_compact : 0;
    launch = true;
    return POM_OK;
}
inline dim3 mixed_step_grid(const PomMixedStepSpec* s) { return dim3((unsigned)((s->first + s->count + 15) / 16 - s->first / 16)); }

#endif /* POM_MIXED_HOST_H_ */
