/*
 * pom_search.hip — the search unit of libpom_batch.so: the kernels and entry points of the calls that play ahead on scratch copies and
 * leave the batch as it is (forecast, the three rollouts, move safety, reach), and of the expansion that copies listed games into
 * slots and plays them one tick.  What it shares with the other units: pom_host.h (host side), pom_device.h (device side).
 */
#include "pom_host.h"
#include "pom_forecast.h"
#include "pom_rollout.h"
#include "pom_rollout_policy.h"
#include "pom_expand.h"
#include "pom_move_safety.h"
#include "pom_reach.h"

/* ---- the forecast (pom_batch.h PomForecastSpec): K ticks ahead on a scratch copy of every tile ---- */

static_assert(sizeof(PomForecastSpec) == POM_FORECAST_SPEC_SIZE, "pom_batch.h states the size");

extern "C" int pom_batch_forecast(PomBatch* h, const PomForecastSpec* s)
{
    const char* what = !h ? "the handle is NULL" : SPEC_HEAD(PomForecastSpec, s);
    if (what) {}
    else if (s->horizon < 1 || s->horizon > POM_FORECAST_MAX_TICKS) what = "horizon must be 1..32";
    else if (!s->flame_tick_dev) what = "flame_tick_dev is NULL";
    else if (((uintptr_t)s->flame_tick_dev & 15) || ((uintptr_t)s->agent_tick_dev & 15)) what = "flame_tick_dev and agent_tick_dev must be 16-byte aligned";
    else if (((uintptr_t)s->ubflags_dev & 3) || ((uintptr_t)s->moves_dev & 3)) what = "ubflags_dev and moves_dev must be 4-byte aligned";
    /* settled, not only joined (as pom_batch_observe): after chained launches a tile left behind is caught up first — the forecast
     * starts from the state a download returns */
    if (int rc = begin_call(h, "pom_batch_forecast", POM_SETTLED, what)) return rc;
    ForecastParams p;
    p.state = h->state;
    p.moves = s->moves_dev;
    p.flame_tick = s->flame_tick_dev;
    p.agent_tick = s->agent_tick_dev;
    p.ubflags = s->ubflags_dev;
    p.n = h->n;
    p.horizon = s->horizon;
    pom_forecast_kernel<<<dim3((unsigned)((h->n + 15) / 16)), dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

/* ---- the rollout (pom_batch.h PomRolloutSpec): R random playouts of every env on scratch copies of its tile; the policy rollout
 * (PomRolloutPolicySpec): the same with SimpleAgent for the agents of simple_mask and a per-agent first tick; and the policy rollout
 * for a list of jobs (PomRolloutJobsSpec) ---- */

static_assert(sizeof(PomRolloutSpec) == POM_ROLLOUT_SPEC_SIZE, "pom_batch.h states the size");
static_assert(sizeof(PomRolloutPolicySpec) == POM_ROLLOUT_POLICY_SPEC_SIZE, "pom_batch.h states the size");
static_assert(sizeof(PomRolloutJobsSpec) == POM_ROLLOUT_JOBS_SPEC_SIZE, "pom_batch.h states the size");

/* What the entry points share, up to the launch: the checks on the handle and on the fields all specs have (the callers have
 * checked what is their own), the device, the settling, and the grid — tiles of 16 envs (pom_batch_rollout_jobs: `items` = its jobs,
 * groups of 16 of them; the others pass -1: the batch's envs), and the same rounded up to a multiple of 8 (the grid is
 * samples * tiles8).  *tiles == 0 on return: nothing to launch (an error, an empty batch or an empty list: result_dev may then be NULL) */
static int rollout_begin(PomBatch* h, const char* who, int32_t horizon, int32_t samples, int32_t dist, const int32_t* moves_dev,
                         const uint32_t* result_dev, int64_t* tiles, int64_t* tiles8, int64_t items = -1)
{
    const char* what = nullptr;
    const int64_t count = items >= 0 ? items : h ? h->n : 0; /* (a count near 2^63 must not wrap) */
    const int64_t t = count / 16 + (count % 16 != 0), t8 = t > INT_MAX ? t : (t + 7) / 8 * 8;
    *tiles = *tiles8 = 0;
    if (!h) what = "the handle is NULL";
    else if (horizon < 1 || horizon > POM_ROLLOUT_MAX_TICKS) what = "horizon must be 1..1024";
    else if (samples < 1 || samples > POM_ROLLOUT_MAX_SAMPLES) what = "samples must be 1..256";
    else if (dist < POM_DIST_HARMLESS || dist > POM_DIST_STRESS) what = "dist must be POM_DIST_HARMLESS, _RANDOM or _STRESS";
    else if (!result_dev && items != 0) what = "result_dev is NULL";
    else if ((uintptr_t)result_dev & 15) what = "result_dev must be 16-byte aligned";
    else if ((uintptr_t)moves_dev & 3) what = "moves_dev must be 4-byte aligned";
    else if (t8 > (int64_t)INT_MAX || t8 * samples > (int64_t)INT_MAX)
        what = items >= 0 ? "samples x groups of 16 jobs exceed one grid: call with fewer samples or jobs"
                          : "samples x tiles of 16 envs exceed one grid: call with fewer samples";
    /* settled, not only joined (as pom_batch_forecast): after chained launches a tile left behind is caught up first — the playouts
     * start from the state a download returns */
    if (int rc = begin_call(h, who, POM_SETTLED, what)) return rc;
    *tiles = t;
    *tiles8 = t8;
    return POM_OK;
}

extern "C" int pom_batch_rollout(PomBatch* h, const PomRolloutSpec* s)
{
    static const char who[] = "pom_batch_rollout";
    if (const char* what = SPEC_HEAD(PomRolloutSpec, s)) return refuse(who, "%s", what);
    int64_t tiles, tiles8;
    const int rc = rollout_begin(h, who, s->horizon, s->samples, s->dist, s->moves_dev, s->result_dev, &tiles, &tiles8);
    if (rc || tiles == 0) return rc;
    RolloutParams p;
    p.state = h->state;
    p.moves = s->moves_dev;
    p.result = s->result_dev;
    p.n = h->n;
    p.env_offset = h->env_offset;
    p.seed = s->seed;
    p.horizon = s->horizon;
    p.dist = s->dist;
    p.max_steps = h->max_steps;
    p.tiles = (uint32_t)tiles;
    p.tiles8 = (uint32_t)tiles8;
    pom_rollout_kernel<<<dim3((unsigned)(tiles8 * s->samples)), dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

/* What pom_batch_rollout_policy and pom_batch_rollout_jobs share, one template over the spec type: the check of the head, the masks,
 * the flags and the moves rule (what is wrong, or nullptr) ... */
template <class S>
static const char* rollout_policy_spec(const S* s, const char* size_text)
{
    if (const char* head = spec_head(s, size_text)) return head;
    if (s->simple_mask < 0 || s->simple_mask > 15) return "simple_mask must be 0..15";
    if (s->first_mask < 0 || s->first_mask > 15) return "first_mask must be 0..15";
    if (s->flags & ~(int32_t)POM_ROLLOUT_FRESH_AGENTS) return "flags must be 0 or POM_ROLLOUT_FRESH_AGENTS";
    if (s->first_mask != 0 && !s->moves_dev) return "first_mask names agents but moves_dev is NULL";
    return nullptr;
}
/* ... and the kernel's arguments: `tiles` / `tiles8` as rollout_begin gave them */
template <class S>
static void rollout_policy_params(const PomBatch* h, const S* s, int64_t tiles, int64_t tiles8, RolloutPolicyParams& p)
{
    p.state = h->state;
    p.moves = s->first_mask ? s->moves_dev : nullptr; /* not read when no agent's first move is fixed */
    p.agent_mem = (s->flags & POM_ROLLOUT_FRESH_AGENTS) ? nullptr : h->agent_mem; /* a handle that never ran the policy has none: fresh agents */
    p.result = s->result_dev;
    p.n = h->n;
    p.n_pad = h->n_pad;
    p.env_offset = h->env_offset;
    p.seed = s->seed;
    p.horizon = s->horizon;
    p.dist = s->dist;
    p.max_steps = h->max_steps;
    p.simple_mask = s->simple_mask;
    p.first_mask = s->first_mask;
    p.tiles = (uint32_t)tiles;
    p.tiles8 = (uint32_t)tiles8;
}

extern "C" int pom_batch_rollout_policy(PomBatch* h, const PomRolloutPolicySpec* s)
{
    static const char who[] = "pom_batch_rollout_policy";
    if (const char* what = rollout_policy_spec(s, "struct_size is not sizeof(PomRolloutPolicySpec)")) return refuse(who, "%s", what);
    int64_t tiles, tiles8;
    const int rc = rollout_begin(h, who, s->horizon, s->samples, s->dist, s->moves_dev, s->result_dev, &tiles, &tiles8);
    if (rc || tiles == 0) return rc;
    RolloutPolicyParams p;
    rollout_policy_params(h, s, tiles, tiles8, p);
    const dim3 grid((unsigned)(tiles8 * s->samples));
    if (s->simple_mask) pom_rollout_policy_kernel<true><<<grid, dim3(64), 0, h->stream>>>(p);
    else pom_rollout_policy_kernel<false><<<grid, dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

extern "C" int pom_batch_rollout_jobs(PomBatch* h, const PomRolloutJobsSpec* s)
{
    static const char who[] = "pom_batch_rollout_jobs";
    const char* what = rollout_policy_spec(s, "struct_size is not sizeof(PomRolloutJobsSpec)");
    if (what) {}
    else if (s->jobs < 0) what = "jobs must be >= 0";
    else if (s->jobs > 0 && !s->src_dev) what = "src_dev is NULL";
    else if ((uintptr_t)s->src_dev & 7) what = "src_dev must be 8-byte aligned";
    if (what) return refuse(who, "%s", what);
    int64_t groups, groups8;
    const int rc = rollout_begin(h, who, s->horizon, s->samples, s->dist, s->moves_dev, s->result_dev, &groups, &groups8, s->jobs);
    if (rc || groups == 0) return rc; /* an empty list: the handle is settled, nothing is launched */
    RolloutJobsParams p;
    rollout_policy_params(h, s, groups, groups8, p);
    p.src = s->src_dev;
    p.jobs = s->jobs;
    const dim3 grid((unsigned)(groups8 * s->samples));
    if (s->simple_mask) pom_rollout_policy_kernel<true, true><<<grid, dim3(64), 0, h->stream>>>(p);
    else pom_rollout_policy_kernel<false, true><<<grid, dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

/* ---- the expansion (pom_batch.h PomExpandSpec): listed games copied into slots and ticked once, one launch ---- */

static_assert(sizeof(PomExpandSpec) == POM_EXPAND_SPEC_SIZE, "pom_batch.h states the size");

extern "C" int pom_batch_expand(PomBatch* h, const PomExpandSpec* s)
{
    static const char who[] = "pom_batch_expand";
    /* the spec's own fields first, then the handle and what depends on it */
    const char* what = SPEC_HEAD(PomExpandSpec, s);
    if (what) {}
    else if (s->flags != 0) what = "flags must be 0";
    else if (s->count < 0) what = "count must be >= 0";
    else if (s->count > 0 && !s->src_dev) what = "src_dev is NULL";
    else if (s->count > 0 && !s->moves_dev) what = "moves_dev is NULL";
    else if (s->count > 0 && ((uintptr_t)s->src_dev & 7)) what = "src_dev must be 8-byte aligned";
    else if (s->count > 0 && ((uintptr_t)s->moves_dev & 3)) what = "moves_dev must be 4-byte aligned";
    else if (s->count > 0 && ((uintptr_t)s->result_dev & 3)) what = "result_dev must be 4-byte aligned";
    else if (s->planes_dev && (s->dtype < POM_OBS_U8 || s->dtype > POM_OBS_CODES)) what = "dtype is no POM_OBS_*";
    else if (!h) what = "the handle is NULL";
    else if (s->first < 0 || s->first > h->n || s->count > h->n - s->first) what = "the range [first, first + count) lies outside the batch";
    else if (!h->quad) what = "needs the quad launch shape (envs_per_wave 16, lanes_per_env 4)";
    if (what) return refuse(who, "%s", what);
    if (s->planes_dev)
        if (const char* oa = observe_args(s->planes_dev, s->dtype, s->per_agent, s->agent_attrs_dev, s->env_attrs_dev)) return refuse(who, "%s", oa);
    if (s->count == 0) return POM_OK;
    /* settled, not only joined (as pom_batch_copy_envs_device): after chained launches a tile left behind is caught up first */
    if (int rc = begin_call(h, who, POM_SETTLED)) return rc;
    ExpandParams p;
    p.state = h->state;
    p.src = s->src_dev;
    p.moves = s->moves_dev;
    p.result = s->result_dev;
    p.first = s->first;
    p.count = s->count;
    p.n = h->n;
    p.n_pad = h->n_pad;
    p.tile0 = s->first / POM_TILE_ENVS;
    p.agent_mem = h->agent_mem;
    p.episode = h->episode;
    p.terminal = h->terminal;
    p.wave_counters = h->wave_counters;
    p.mode = h->mode;
    p.max_steps = h->max_steps;
    p.obs = observe_params(h, s->planes_dev, s->dtype, s->per_agent, s->agent_attrs_dev, s->env_attrs_dev);
    const dim3 grid((unsigned)((s->first + s->count - 1) / POM_TILE_ENVS - p.tile0 + 1));
    if (s->planes_dev) pom_expand_kernel<true><<<grid, dim3(64), 0, h->stream>>>(p);
    else pom_expand_kernel<false><<<grid, dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

/* ---- the move safety (pom_batch.h PomMoveSafetySpec): every asked agent's six candidate moves played K ticks ahead on scratch copies
 * of its tile, one launch ---- */

static_assert(sizeof(PomMoveSafetySpec) == POM_MOVE_SAFETY_SPEC_SIZE, "pom_batch.h states the size");

extern "C" int pom_batch_move_safety(PomBatch* h, const PomMoveSafetySpec* s)
{
    static const char who[] = "pom_batch_move_safety";
    const char* what = !h ? "the handle is NULL" : SPEC_HEAD(PomMoveSafetySpec, s);
    /* tiles of 16 envs, rounded up to a multiple of 8 as the rollouts' grid (rollout_begin); 6 variants per agent of the mask */
    const int64_t tiles = h ? (h->n + 15) / 16 : 0, tiles8 = (tiles + 7) / 8 * 8;
    const int variants = what ? 0 : 6 * __builtin_popcount((unsigned)s->agent_mask & 15u);
    if (what) {}
    else if (s->reserved2_ != 0) what = "reserved2_ must be 0";
    else if (s->horizon < 1 || s->horizon > POM_FORECAST_MAX_TICKS) what = "horizon must be 1..32";
    else if (s->agent_mask < 1 || s->agent_mask > 15) what = "agent_mask must be 1..15";
    else if (!s->death_tick_dev && !s->escape_tick_dev) what = "death_tick_dev and escape_tick_dev are both NULL";
    else if (((uintptr_t)s->death_tick_dev & 7) || ((uintptr_t)s->escape_tick_dev & 7)) what = "death_tick_dev and escape_tick_dev must be 8-byte aligned";
    else if ((uintptr_t)s->moves_dev & 3) what = "moves_dev must be 4-byte aligned";
    else if (tiles8 * variants > (int64_t)INT_MAX) what = "variants x tiles of 16 envs exceed one grid: call with fewer agents";
    /* settled, not only joined (as pom_batch_forecast): after chained launches a tile left behind is caught up first — the candidates
     * are played from the state a download returns */
    if (int rc = begin_call(h, who, POM_SETTLED, what)) return rc;
    MoveSafetyParams p;
    p.state = h->state;
    p.moves = s->moves_dev;
    p.death_tick = s->death_tick_dev;
    p.escape_tick = s->escape_tick_dev;
    p.n = h->n;
    p.horizon = s->horizon;
    p.agent_mask = s->agent_mask;
    p.tiles = (uint32_t)tiles;
    p.tiles8 = (uint32_t)tiles8;
    pom_move_safety_kernel<<<dim3((unsigned)(tiles8 * variants)), dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    return POM_OK;
}

/* ---- the reach (pom_batch.h PomReachSpec): every asked agent's FillRMap distances and first moves, one launch ---- */
static_assert(sizeof(PomReachSpec) == POM_REACH_SPEC_SIZE, "pom_batch.h states the size");

extern "C" int pom_batch_reach(PomBatch* h, const PomReachSpec* s)
{
    static const char who[] = "pom_batch_reach";
    const char* what = !h ? "the handle is NULL" : SPEC_HEAD(PomReachSpec, s);
    /* tiles of 16 envs, rounded up to a multiple of 8 as the rollouts' grid (rollout_begin); a variant per agent of the mask */
    const int64_t tiles = h ? (h->n + 15) / 16 : 0, tiles8 = (tiles + 7) / 8 * 8;
    if (what) {}
    else if (s->reserved2_ != 0) what = "reserved2_ must be 0";
    else if (s->agent_mask < 1 || s->agent_mask > 15) what = "agent_mask must be 1..15";
    else if (s->max_dist < 1 || s->max_dist > POM_REACH_MAX_DIST) what = "max_dist must be 1..120";
    else if (!s->dist_dev && !s->move_dev) what = "dist_dev and move_dev are both NULL";
    else if (((uintptr_t)s->dist_dev & 7) || ((uintptr_t)s->move_dev & 7)) what = "dist_dev and move_dev must be 8-byte aligned";
    static_assert((((int64_t)1 << 30) / 16 + 8) * 4 < (int64_t)INT_MAX, "four variants of the largest batch (create_plan) fit one grid");
    /* settled, not only joined (as pom_batch_forecast): after chained launches a tile left behind is caught up first — the maps are
     * those of the state a download returns */
    if (int rc = begin_call(h, who, POM_SETTLED, what)) return rc;
    ReachParams p;
    p.state = h->state;
    p.dist = s->dist_dev;
    p.move = s->move_dev;
    p.n = h->n;
    p.agent_mask = s->agent_mask;
    p.max_dist = s->max_dist;
    p.tiles = (uint32_t)tiles;
    p.tiles8 = (uint32_t)tiles8;
    const dim3 grid(p.tiles8 * (unsigned)__builtin_popcount((unsigned)s->agent_mask & 15u));
    if (p.move && p.dist) pom_reach_kernel<true, true><<<grid, dim3(64), 0, h->stream>>>(p);
    else if (p.move) pom_reach_kernel<true, false><<<grid, dim3(64), 0, h->stream>>>(p);
    else pom_reach_kernel<false, true><<<grid, dim3(64), 0, h->stream>>>(p);
    HIPCHK(hipGetLastError());
    return POM_OK;
}
