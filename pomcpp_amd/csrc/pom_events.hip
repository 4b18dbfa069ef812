/*
 * pom_events.hip — the step-events unit of libpom_batch.so: pom_batch_step_events (pom_batch.h PomStepEventsSpec), pom_batch_step_mixed
 * that also writes what the tick did, and the EVENTS instantiations of the mixed step's kernel (pom_step_mixed.h, pom_step_events.h).
 * The checks of the step's spec and the launch's parameters are pom_batch_step_mixed's own (pom_mixed_host.h).
 */
#include "pom_mixed_host.h"

static_assert(sizeof(PomStepEventsSpec) == POM_STEP_EVENTS_SPEC_SIZE, "pom_batch.h states the size");

typedef void (*PomEventsKernel)(MixedStepParams, StepEventsOut);

extern "C" int pom_batch_step_events(PomBatch* h, const PomMixedStepSpec* s, const PomStepEventsSpec* ev)
{
    static const char who[] = "pom_batch_step_events";
    static const PomEventsKernel k[4][4] = POM_MIXED_KERNEL_TABLE(pom_step_events_kernel, pom_step_events_compact_kernel);
    PomObserveOut obs;
    if (int rc = mixed_step_args(h, who, s, obs)) return rc;
    const char* what = !ev ? "the events spec is NULL" : SPEC_HEAD(PomStepEventsSpec, ev);
    if (what) {}
    else if (ev->flags != 0) what = "flags must be 0";
    else if (!ev->events_dev) what = "events_dev is NULL";
    else if ((uintptr_t)ev->events_dev & 3) what = "events_dev must be 4-byte aligned";
    else if ((uintptr_t)ev->outcome_dev & 3) what = "outcome_dev must be 4-byte aligned";
    if (what) return refuse(who, "%s", what);
    MixedStepParams p;
    bool launch;
    if (int rc = mixed_step_begin(h, who, s, obs, p, launch)) return rc;
    if (!launch) return POM_OK;
    StepEventsOut eo{ev->events_dev, ev->outcome_dev, ev->wood_dev};
    const void* kernel = reinterpret_cast<const void*>(k[mixed_kernel_row(s)][mixed_kernel_column(h)]);
    void* args[2] = {&p, &eo};
    HIPCHK(hipLaunchKernel(kernel, mixed_step_grid(s), dim3(64), args, 0, s->stream ? (hipStream_t)s->stream : h->stream));
    return POM_OK;
}
