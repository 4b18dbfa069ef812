/*
 * pom_mixed.hip — the mixed-step unit of libpom_batch.so: pom_batch_step_mixed (pom_batch.h PomMixedStepSpec), the closed-loop range
 * call with SimpleAgent for the agents of simple_mask, and its kernel.  What it shares with the other units: pom_host.h, pom_device.h;
 * with pom_events.hip: pom_mixed_host.h (the checks and the parameters) and the kernel's body (pom_step_mixed.h).
 */
#include "pom_mixed_host.h"

typedef void (*PomMixedKernel)(MixedStepParams);

extern "C" int pom_batch_step_mixed(PomBatch* h, const PomMixedStepSpec* s)
{
    static const char who[] = "pom_batch_step_mixed";
    static const PomMixedKernel k[4][4] = POM_MIXED_KERNEL_TABLE(pom_step_mixed_kernel, pom_step_mixed_compact_kernel);
    PomObserveOut obs;
    if (int rc = mixed_step_args(h, who, s, obs)) return rc;
    MixedStepParams p;
    bool launch;
    if (int rc = mixed_step_begin(h, who, s, obs, p, launch)) return rc;
    if (!launch) return POM_OK;
    const void* kernel = reinterpret_cast<const void*>(k[mixed_kernel_row(s)][mixed_kernel_column(h)]);
    void* args[1] = {&p};
    HIPCHK(hipLaunchKernel(kernel, mixed_step_grid(s), dim3(64), args, 0, s->stream ? (hipStream_t)s->stream : h->stream));
    return POM_OK;
}
