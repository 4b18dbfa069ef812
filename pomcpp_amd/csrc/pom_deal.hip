/*
 * pom_deal.hip — the deal unit of libpom_batch.so: pom_batch_deal (pom_batch.h PomDealSpec), Pommerman's standard start boards dealt on
 * the device, into the envs' records and restart snapshots or into the snapshots alone, and its kernel.  What it shares with the other
 * units: pom_host.h, pom_device.h.
 */
#include <cstddef>

#include "pom_host.h"
#include "pom_deal.h"

static_assert(sizeof(PomDealSpec) == POM_DEAL_SPEC_SIZE && sizeof(PomBoardLayout) == 20, "pom_batch.h states the size");
static_assert(offsetof(PomDealSpec, layout) == 40 && offsetof(PomDealSpec, games_dev) == 64 && offsetof(PomDealSpec, stream) == 88, "no implicit padding");

extern "C" int pom_batch_deal(PomBatch* h, const PomDealSpec* s)
{
    static const char who[] = "pom_batch_deal";
    /* the spec's own fields first, then the handle and what depends on it */
    const char* what = SPEC_HEAD(PomDealSpec, s);
    if (what) {}
    else if (s->reserved2_ != 0) what = "reserved2_ must be 0";
    else if (s->mode != POM_DEAL_START && s->mode != POM_DEAL_NEXT) what = "mode must be POM_DEAL_START or POM_DEAL_NEXT";
    else if (s->which < POM_DEAL_ALL || s->which > POM_DEAL_DONE) what = "which must be POM_DEAL_ALL, _MASK, _RESTARTED or _DONE";
    else if ((what = pom_deal_layout_bad(s->layout))) {}
    else if (s->count < 0) what = "count must be >= 0";
    else if (s->count > 0 && !s->games_dev) what = "games_dev is NULL";
    else if (s->count > 0 && s->which == POM_DEAL_MASK && !s->which_dev) what = "which_dev is NULL with POM_DEAL_MASK";
    else if (s->count > 0 && (((uintptr_t)s->games_dev & 3) || ((uintptr_t)s->which_dev & 3) || ((uintptr_t)s->result_dev & 3)))
        what = "games_dev, which_dev and result_dev must be 4-byte aligned";
    else if (!h) what = "the handle is NULL";
    else if (s->first < 0 || s->first > h->n || s->count > h->n - s->first) what = "the range [first, first + count) lies outside the batch";
    else if (s->which == POM_DEAL_RESTARTED && h->auto_reset != POM_RESET_AT_END) what = "POM_DEAL_RESTARTED needs a POM_RESET_AT_END handle";
    else if (!h->quad) what = "needs the quad launch shape (envs_per_wave 16, lanes_per_env 4)";
    if (what) return refuse(who, "%s", what);
    if (s->count == 0) return POM_OK;
    /* settled, not only joined (as pom_batch_imagine); no runtime call at all once the handle is settled: what a capture needs */
    if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
    DealParams p;
    p.state = h->state;
    p.snap = h->snap;
    p.agent_mem = h->agent_mem;
    p.games = s->games_dev;
    p.mask = s->which == POM_DEAL_MASK ? s->which_dev : nullptr;
    p.result = s->result_dev;
    p.first = s->first;
    p.count = s->count;
    p.n_pad = h->n_pad;
    p.tile0 = s->first / POM_TILE_ENVS;
    p.env_offset = h->env_offset;
    p.seed = s->seed;
    p.layout = s->layout;
    p.mode = s->mode;
    p.which = s->which;
    void* args[1] = {&p};
    HIPCHK(hipLaunchKernel(reinterpret_cast<const void*>(pom_deal_kernel), dim3((unsigned)((s->first + s->count - 1) / POM_TILE_ENVS - p.tile0 + 1)),
                           dim3(64), args, 0, s->stream ? (hipStream_t)s->stream : h->stream));
    return POM_OK;
}
