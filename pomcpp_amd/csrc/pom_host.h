/*
 * pom_host.h — the library's internal host interface: what the units of libpom_batch.so share on the host side.  The handle
 * (PomBatch, with the chained launches' state it holds), the one way to fail (HIPCHK, set_err) and to refuse (refuse, spec_head /
 * SPEC_HEAD), the start of every call on a handle (check_call, begin_call) and the argument rules several calls state (check_range,
 * range_args, observe_args, view_args) with the parameters they lead to (observe_params, view_out).  Every function declared here is
 * defined once, in the core unit (pom_batch.hip: pom_handle.h, pom_api_observe.h, pom_api_step.h), behind the one error text that
 * pom_last_error reads; POM_INTERNAL keeps them out of the library's exports.
 *
 * A unit is always built with the same defines as the core (__graft_entry__.build_hip): PomBatch and StepParams have members under
 * POM_DIAG / POM_TRUNC, and they are one type only then.
 */
#ifndef POM_HOST_H_
#define POM_HOST_H_

#include <type_traits>
#include <vector>

#include "pom_device.h"

#define POM_INTERNAL __attribute__((visibility("hidden")))

/* ---- failing and refusing ---- */
POM_INTERNAL void set_err(const char* what, hipError_t e); /* pom_last_error() reads "<what>: <the runtime's text>" */
#define HIPCHK(call)                      \
    do {                                  \
        hipError_t e_ = (call);           \
        if (e_ != hipSuccess) {           \
            set_err(#call, e_);           \
            return POM_E_HIP;             \
        }                                 \
    } while (0)

/* The one way to refuse a call: pom_last_error() reads "<call>: <what>", the call returns POM_E_ARG.  Every POM_E_ARG of every entry
 * point comes from here, so the text always names the call that refused. */
POM_INTERNAL __attribute__((format(printf, 2, 3))) int refuse(const char* who, const char* fmt, ...);

/* The head of every spec's check (pom_batch.h Pom*Spec): what is wrong with it, or nullptr.  SPEC_HEAD names the type for the text. */
template <class S>
static const char* spec_head(const S* s, const char* size_text)
{
    if (!s) return "the spec is NULL";
    if (s->struct_size != (int32_t)sizeof(S)) return size_text;
    if constexpr (std::is_array<decltype(S::reserved_)>::value) {
        for (const auto r : s->reserved_)
            if (r != 0) return "reserved_ must be 0";
    } else if (s->reserved_ != 0) return "reserved_ must be 0";
    return nullptr;
}
#define SPEC_HEAD(S, s) spec_head<S>(s, "struct_size is not sizeof(" #S ")")

/* ---- the chained launches' state in the handle (what it means and who sets it up: pom_chain.h) ---- */

/* one chained call (or several that continue the same play back to back): everything needed to play any of its ticks again */
struct PomChainCall {
    uint32_t visit0 = 0, launches = 0; /* the tiles' visits visit0 .. visit0 + launches - 1 */
    StepParams p;                      /* as launched: p.tick0 is the tick of visit p.chain_seq0 */
    bool policy = false;
};

struct PomChain {
    bool tried = false, ok = false;
    unsigned long long* tile_seq = nullptr; /* device, one word per tile (StepParams.tile_seq) */
    uint32_t* aux = nullptr;                /* device: [0] the kernels' POM_CHAIN_E_* flags, [1] number of poisoned tiles, then (tile, stored) pairs */
    uint32_t* aux_host = nullptr;           /* pinned: where chain_settle reads aux[0..1] */
    int64_t tiles = 0;
    uint32_t visits = 0;                    /* visits every tile has had since its word was last zeroed */
    uint32_t turn = 0;                      /* which stream the next launch goes to */
    bool unverified = false;                /* chained launches since the tiles' words were last checked (chain_settle) */
    uint64_t wait_limit = 0;                /* StepParams.chain_wait_limit */
    int64_t wave_slots = 0;                 /* wavefronts of the step kernel the device holds at once: 16 per CU (launch_many_chain's rotation) */
    StepParams last_key;                    /* what the chained launches possibly still in flight were launched with (tick0 = the */
    void (*last_kernel)(StepParams) = nullptr; /* offset between ticks and visits), and which instantiation */
    std::vector<PomChainCall> log;          /* the chained calls since the last settle */
    int64_t stat_launches = 0, stat_settles = 0, stat_tiles_recovered = 0, stat_ticks_replayed = 0; /* pom_batch_chain_stats */
};

/* ---- the handle ---- */
struct PomBatch {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int64_t n = 0, n_pad = 0, n_waves = 0, env_offset = 0; /* n_waves: counter slots, sized for the smallest EPW */
    int epw = 64;
    bool quad = false; /* EPW 16 with four lanes per env (pom_step_kernel's G = 4) */
    int mode = POM_MODE_ENV, auto_reset = 0, max_steps = 0;
    uint32_t* state = nullptr;
    uint32_t* snap = nullptr;       /* restart snapshot, array of structs */
    uint32_t* terminal = nullptr;   /* POM_RESET_AT_END: final record of each env's last finished episode, array of structs */
    int32_t* moves_dev = nullptr;   /* n_pad x 4 */
    uint32_t* agent_mem = nullptr;  /* SimpleAgent memory, [2][4 * n_pad], allocated on first use */
    uint32_t* episode = nullptr;    /* games started per env (fresh boards) */
    uint64_t board_seed = 0;
    int fresh = 0;
    int32_t* staging = nullptr;     /* staging_envs x 251 dwords (AoS), also status scratch */
    uint32_t* copy_scratch = nullptr; /* pom_batch_copy_envs: K1's image of state, agent memory, episode (and terminal), allocated on
                                         first use (pom_copy.h) */
    int64_t* copy_idx = nullptr;      /* ... and the host variant's indices on the device, n_pad int64 */
    int64_t staging_envs = 0;
    int64_t* wave_counters = nullptr;
    int64_t* totals_dev = nullptr;
    int* first_bad = nullptr;
    uint64_t tick = 0;
    /* A step is issued as `parts` kernels over contiguous tile ranges on internal streams: the launches are
     * independent (envs never interact), so one part's HBM load / store phases overlap the others' compute
     * instead of all wavefronts of the chip loading and storing in lock-step.  The caller's stream is forked
     * into the sub-streams lazily and joined again before anything else touches the batch. */
    enum { MAX_PARTS = 8, PROF_RING = 256 };
    int parts = 1;
    hipStream_t sub[MAX_PARTS] = {};
    hipEvent_t ev_fork = nullptr, ev_join[MAX_PARTS] = {};
    bool forked = false;
    int forked_n = 0; /* how many streams (indices below it) the fork covers */
    int main_part = 1; /* part 0 of a split step runs on the caller's stream itself, parts 1.. on sub-streams: one stream
                          fewer for the same overlap (3 parts: 21.2 -> 20.6 us per step at 65,536 envs); POM_MAIN_PART=0: all
                          parts on sub-streams */
    /* how the launches of a several-tick call are issued (launch_many; PomBatchOptions.issue_mode) */
    int issue_mode = POM_ISSUE_THREADS;
    struct PomIssuer* issuers[MAX_PARTS] = {}; /* POM_ISSUE_THREADS: one helper thread per sub-stream part, created on first use */
    bool issuers_failed = false;               /* a helper thread could not be started: the calling thread issues the rest */
    int last_kind = 0;                         /* what has been launched on the streams since they were forked: POM_KIND_SPLIT / _CHAIN */
    /* POM_ISSUE_GRAPH: multi-tick calls replay a captured chunk of launches (launch_many): POM_GRAPH_TICKS launches of every part as one HIP
     * graph per part.  tick_words[k] is the tick part k's replay starts at, read by the graph's kernels (StepParams.tick_base;
     * set by a one-lane kernel on the part's stream in front of each replay); tick_words[MAX_PARTS] stays 0 and is what every
     * launch outside a graph points at. */
    enum { MAX_GRAPHS = 4 };
    struct PomStepGraph* graphs[MAX_GRAPHS] = {};
    uint64_t graph_clock = 0;
    uint32_t* tick_words = nullptr;
    PomChain chain;          /* POM_ISSUE_CHAIN: the tiles' ticket words, set up on first use (pom_chain.h) */
    int chain_parts = 3;     /* ... and how many streams the chained launches may rotate over */
    bool chain_auto = true;  /* ... of which a call uses two if it is short and three if it is long (launch_many_chain) — unless the caller
                                asked for a number of streams */
    int chain_last_use = 2;  /* what the last chained call used (pom_batch_issue_info) */
    bool fuse_policy = true; /* pom_batch_step_simple: policy and tick in one kernel (quad shape); POM_FUSE=0 keeps them apart */
    /* optional per-launch timing (pom_batch_profile) */
    bool profiling = false;
    hipEvent_t prof_ev[2 * PROF_RING] = {};
    int prof_n = 0;
#if defined(POM_DIAG)
    long long* diag = nullptr;
    long long* diag_pol = nullptr;
#endif
};

/* which of the step kernels' modes a handle runs in (pom_issue.h step_kernel) */
inline bool runs_fresh(const PomBatch* h) { return h->fresh && h->mode == POM_MODE_ENV && h->auto_reset; }
inline bool runs_at_end(const PomBatch* h) { return h->auto_reset == POM_RESET_AT_END && h->mode == POM_MODE_ENV; }

/* ---- how a call on a handle starts ---- */

/* [first, first + count) lies in the batch, or the call is refused */
POM_INTERNAL int check_range(const PomBatch* h, const char* who, int64_t first, int64_t count);

/* The start of every call on a handle.  Refuses a NULL handle, then `what` (what the caller found wrong with the other arguments, or
 * nullptr), both by the call's name and before any runtime call; selects the handle's device; and brings the handle to the state
 * the call needs: as it is (a call that only launches: launch_step settles for itself), the sub-streams joined into the caller's
 * stream, or settled (quiesce). */
enum PomNeeds { POM_AS_IS, POM_JOINED, POM_SETTLED };
POM_INTERNAL int check_call(const PomBatch* h, const char* who, const char* what = nullptr); /* (all of it for a call that only reads the handle) */
POM_INTERNAL int begin_call(PomBatch* h, const char* who, PomNeeds needs, const char* what = nullptr);

/* the SimpleAgent memory, allocated and cleared on the handle's stream when a call first needs it */
POM_INTERNAL int ensure_agent_mem(PomBatch* h);

/* closed-loop stepping: a range of whole tiles of a quad-shape handle, and moves that are not NULL — or the call is refused */
POM_INTERNAL int range_args(PomBatch* h, const char* who, int64_t first, int64_t count, const int32_t* moves_dev);

/* ---- the observation's outputs ---- */

struct PomObserveOut { /* pom_batch_step_device_observe / _range: where the fused kernel writes the observation */
    void* planes;
    int32_t* agent_attrs;
    int32_t* env_attrs;
    int32_t dtype, per_agent;
    /* the fogged views (pom_batch_step_device_observe_view / _range_view): view = 1 picks the VIEW kernels (launch_parts, launch_range),
     * which write viewer_attrs and ignore agent_attrs / per_agent; the other kernels ignore these */
    int32_t view, view_radius;
    int32_t* viewer_attrs;
    /* the compact views (PomCompactViewSpec): pom_observe_compact.h's obs_compact_word, 0 for the four-view form.  Only
     * pom_batch_observe_view and the mixed step's units serve it */
    int32_t view_compact;
};

/* what every call with a plain observation asks of its outputs: what is wrong, or nullptr */
POM_INTERNAL const char* observe_args(const void* planes_dev, int32_t dtype, int32_t per_agent, const int32_t* agent_attrs_dev, const int32_t* env_attrs_dev);
/* the export kernels' arguments for the whole batch (viewer_attrs / view_radius: the fogged views only) */
POM_INTERNAL ObserveParams observe_params(const PomBatch* h, void* planes_dev, int32_t dtype, int32_t per_agent, int32_t* agent_attrs_dev,
                                          int32_t* env_attrs_dev, int32_t* viewer_attrs_dev = nullptr, int32_t view_radius = 0,
                                          int32_t view_compact = 0);
/* the fogged views (pom_batch.h PomViewSpec, or the PomCompactViewSpec it begins: both sizes pass): what is wrong with the spec, or
 * nullptr; and the outputs it names */
POM_INTERNAL const char* view_args(const PomViewSpec* s);
POM_INTERNAL PomObserveOut view_out(const PomViewSpec* s);
/* a spec that passed view_args is the longer one */
inline bool view_is_compact(const PomViewSpec* s) { return s->struct_size == POM_COMPACT_VIEW_SPEC_SIZE; }
/* what the calls that do not serve the compact form say */
#define POM_COMPACT_VIEW_ELSEWHERE \
    "a PomCompactViewSpec is served by pom_batch_observe_view, pom_batch_step_mixed and pom_batch_step_events, not by this call"

#endif /* POM_HOST_H_ */
