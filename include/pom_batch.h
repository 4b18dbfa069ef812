/*
 * pom_batch.h — C-ABI of the MI355X batched Pommerman stepper (libpom_batch.so).
 *
 * Drop-in boundary for ONE path of dist1ll/pomcpp: the simulation tick
 *     void bboard::Step(State* state, Move* moves);          include/bboard.hpp:668, src/bboard/step.cpp:9
 * and the bookkeeping Environment::Step wraps around it      src/bboard/environment.cpp:123-169
 * re-laid out over n concurrent boards on one GPU.  States cross the boundary
 * as the reference's own 1004-byte `bboard::State` (pom_state.h), moves as the
 * reference's `Move` ints (0 IDLE, 1 UP, 2 DOWN, 3 LEFT, 4 RIGHT, 5 BOMB),
 * four per env INCLUDING dead agents (their entries are read by FillDestPos /
 * FixSwitchMove, step_utility.cpp:138-170 — SURVEY.md Q9).
 *
 * Plain pointers and sizes only; no C++/torch types.  Every call returns a
 * PomError (the reference returns void and has UB on misuse; see pom_state.h
 * POM_UB_* for what the stepper does instead).  A handle is bound to one
 * device and one HIP stream; calls on one handle are not thread-safe, distinct
 * handles are independent.  Stepping is asynchronous on the handle's stream;
 * upload / download / status / counters synchronise it.
 *
 * There is deliberately no CPU fallback: without a HIP device every entry
 * point fails with POM_E_HIP.
 */
#ifndef POM_BATCH_H_
#define POM_BATCH_H_

#include <stdint.h>

#include "pom_rng.h"
#include "pom_state.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum PomError {
    POM_OK = 0,
    POM_E_ARG = 1,             /* null handle, range outside [0, n_envs), bad option; pom_last_error() names the refusing call: "<call>: <what>" */
    POM_E_HIP = 2,             /* HIP runtime error or no device; pom_last_error() has the text */
    POM_E_UNREPRESENTABLE = 3, /* an uploaded State holds a value no reachable game state has (pom_packed.h) */
    POM_E_NOMEM = 4
} PomError;

/* stepping semantics */
enum {
    POM_MODE_RAW = 0, /* bare bboard::Step: no timeStep++, finished envs keep stepping (what the reference's tests call) */
    POM_MODE_ENV = 1  /* Environment::Step: skip finished envs, Step, timeStep++, done / winner / draw */
};

typedef struct PomBatchOptions {
    int32_t struct_size;  /* = sizeof(PomBatchOptions), for ABI growth */
    int32_t device;       /* HIP device ordinal */
    void*   stream;       /* hipStream_t to run on, or NULL: the library creates one */
    int32_t mode;         /* POM_MODE_RAW / POM_MODE_ENV */
    int32_t auto_reset;   /* ENV mode, what happens to a finished env (POM_RESET_*):
                             0 nothing: it stays finished and is not stepped (Environment::Step, environment.cpp:125-128);
                             1 POM_RESET_AT_START: the NEXT tick first puts it back on its start state (snapshot, or the next
                               generated board) and steps that in the same tick — the caller never sees the start state, and a
                               move supplied for that tick was chosen looking at the finished game;
                             2 POM_RESET_AT_END: the tick that finishes the episode also puts the env on its next start state.
                               State, observation and status then show the new episode's first state (status bit "restarted"),
                               the next move is a move for it, and the finished episode's outcome and final State are kept
                               (pom_batch_last_results, pom_batch_download_terminal) until the env finishes again.  The
                               sequence of states stepped is the same in both modes.  In both modes a restart clears the
                               env's ubflags (pom_batch_status): they gather the flags of the current episode only. */
    int32_t max_steps;    /* ENV mode: env is done once timeStep reaches this (0 = no limit); StartGame's bound, environment.cpp:71 */
    int64_t env_offset;   /* global index of env 0, keys the synthetic move stream when a job is sharded over GPUs */
    int32_t envs_per_wave; /* 0 = default (16); else 16, 32 or 64 envs per wavefront (results are identical) */
    int32_t streams;       /* 0 = choose (chained launches: 2 in a short call, 3 from 50 launches up; sub-batches by batch size); else 1..8: the streams chained
                              launches rotate over, and the sub-batches per step — each on an internal stream — where launches
                              are not chained (results are identical; 1 = plain launches in a row on the handle's stream) */
    int32_t lanes_per_env; /* 0 = default (4: a quad of adjacent lanes runs each env's tick and splits its order-free parts,
                              needs envs_per_wave 16); 1 = one lane per env */
    int32_t fresh_boards;  /* with auto_reset: a finished env starts its next game on a newly generated board (pom_boardgen.h:
                              board_seed, env_offset + env, games played) instead of replaying its snapshot; drawn on the
                              device inside the tick, the host is not involved */
    uint64_t board_seed;   /* seed of those boards; pom_batch_generate replaces it */
    int32_t issue_mode;    /* how the launches of a several-tick call (pom_batch_step_random / _step_simple) are issued — POM_ISSUE_*;
                              results do not depend on it.  0 = POM_ISSUE_CHAIN up to 196,608 envs (default kernel shape),
                              POM_ISSUE_THREADS otherwise */
    int32_t reserved_;
} PomBatchOptions;

/* PomBatchOptions.issue_mode (environment POM_ISSUE = direct | threads | graph | chain overrides it).  Measured per step at 65,536
 * envs, 20-tick call from an idle device / 500-tick call: CHAIN 11.4 - 12.3 / 9.2 us (profiles/r03y_*); with the batch as
 * three sub-batches on parallel streams: THREADS 16.2 - 17.0 / 14.5 us, DIRECT and GRAPH behind that (measured earlier in the
 * round, 18.0 / 15.5 for THREADS then: DIRECT 17.2 .. 26.4 (host-dependent) / 15.6 - 16.0 us; GRAPH 21.4 .. 23.5 / 16.1 us;
 * pomcpp_amd/csrc/pom_issue.h, profiles/r03_issue_modes.txt) */
enum {
    POM_ISSUE_AUTO = 0,
    POM_ISSUE_DIRECT = 1,  /* the calling thread issues every launch; the library owns no thread */
    POM_ISSUE_THREADS = 2, /* one helper thread per internal sub-stream issues that stream's launches (created on first use, joined by
                              pom_batch_destroy; a helper that cannot be started falls back to DIRECT for its part) */
    POM_ISSUE_GRAPH = 3,   /* chunks of 20 ticks replayed as HIP graphs, one per sub-stream; no library-owned thread */
    POM_ISSUE_CHAIN = 4    /* chained launches (pomcpp_amd/csrc/pom_chain.h): every launch covers the WHOLE batch and plays one tick,
                              consecutive launches go to different internal HIP streams (two in a short call, three from 50 ticks
                              up), and a ticket word per 16-env tile orders that tile's ticks — a tile's next tick waits for the
                              same tile's previous tick only, not for the slowest wavefront of the launch before.  Asynchronous
                              like the other modes: the call returns when its launches are queued — by the calling thread and, in a
                              call of six launches or more, by the helper threads of the internal sub-streams (created on first
                              use, joined by pom_batch_destroy; environment POM_CHAIN_HELPERS=0: the calling thread alone); every
                              other call of this API joins the streams.  pom_batch_create probes the device once (workgroup -> XCD round-robin over
                              eight XCDs); where that does not hold, and for shapes without a chained twin (one lane per env,
                              several ticks per launch, one stream), launches are issued as with POM_ISSUE_THREADS.  A wavefront
                              that cannot play its tile (its predecessor did not show up within 2 s of wall-clock time) leaves
                              the tile alone; the next call that reads or changes the batch finds it and replays the tile's
                              missing ticks with ordinary launches (pom_batch_chain_stats counts such events: expected 0).
                              That check is ONE host synchronisation of the handle's stream: the first call after chained launches
                              that is not itself a chained call of the same kind — a step of another kind (pom_batch_step_device,
                              _step_device_observe, _step_device_range, _policy_simple, several ticks per launch), pom_batch_observe,
                              _snapshot, _generate, _reset_counters, _device_view, _set_streams, and every call that reads results
                              back — blocks the calling thread until the chained launches have finished.  pom_batch_flush,
                              _moves_device and _counters_device do NOT run it (they only join the streams): what they hand out may
                              lag by the ticks of a tile left behind until the next call that does */
};

enum { POM_RESET_OFF = 0, POM_RESET_AT_START = 1, POM_RESET_AT_END = 2 };

typedef struct PomBatch PomBatch;

/* counters accumulated since creation / pom_batch_reset_counters */
enum { POM_CNT_STEPS = 0, POM_CNT_EPISODES = 1, POM_CNT_RESETS = 2, POM_CNT_UB_TICKS = 3, POM_CNT_N = 4 };

const char* pom_last_error(void);
int pom_device_count(void);

int pom_batch_create(PomBatch** out, int64_t n_envs, const PomBatchOptions* opts);
int pom_batch_destroy(PomBatch* h);
int64_t pom_batch_size(const PomBatch* h);

/* host AoS (count x 1004 B) -> device; also becomes the envs' reset snapshot and clears their status */
int pom_batch_upload(PomBatch* h, const void* states, int64_t first, int64_t count);
/* device -> host AoS (count x 1004 B); agent padding bytes come back 0 */
int pom_batch_download(PomBatch* h, void* states, int64_t first, int64_t count);
/* make the current device state the reset snapshot */
int pom_batch_snapshot(PomBatch* h);
/* start boards without the host: every env gets the board (board_seed, env_offset + env, episode 0) of pom_boardgen.h — the
 * reference's InitState distribution (bboard.cpp:339-382: cells passage 5/7, rigid 1/7, wood 1/7, half the woods flagged,
 * agents in the corners) — as its state and its reset snapshot, generated on the device; the agents' memory starts afresh */
int pom_batch_generate(PomBatch* h, uint64_t board_seed);
/* games started so far by envs [first, first+count) (0 = still the first one), uint32 each */
int pom_batch_episodes(PomBatch* h, int64_t first, int64_t count, uint32_t* out);

/*
 * Copy and restore games by index on the device (tree search, Monte-Carlo rollouts, population methods): env first + i becomes a
 * copy of env src[i], for i in [0, count).  Indices are int64.  The host variant reads src_host now; the device variant reads
 * src_dev on the handle's stream, in stream order like the moves of pom_batch_step_device.
 *
 * Aliasing: the result is as if every source had been read before any destination was written.  Sources may lie inside
 * [first, first + count) and may repeat: an in-place resample src = before[perm_with_repeats] is the main case.
 *
 * Default (the source's CURRENT state): the destination takes over the source's record (board, timeStep, agents, bomb and flame
 * queues, status, ubflags), its SimpleAgent memory (if allocated), its episode counter (pom_batch_episodes) and, with
 * POM_RESET_AT_END, its terminal record and last results.  Afterwards nothing the API can read tells the destination from the
 * source but its env index — and that index keys the pom_rng.h move stream, the SimpleAgent's draw and fresh boards, so clones
 * of one root DIVERGE under pom_batch_step_random / _step_simple: what rollouts want.
 * POM_COPY_FROM_SNAPSHOT: the source is env src[i]'s restart snapshot instead of its current state; the destination gets fresh
 *   agent memory (as after pom_batch_upload), its episode counter and terminal record stay as they were.  src[i] = first + i
 *   puts a game back on its start.
 * POM_COPY_SET_SNAPSHOT: the copied record also becomes the destination's snapshot, status and ubflags cleared as
 *   pom_batch_snapshot does: a clone's restart point is its root.
 * Entries src[i] < 0 leave env first + i untouched (a masked copy or reset).  The device variant also leaves entries >= n
 * untouched; the host variant rejects them with POM_E_ARG before anything is changed.  A range outside [0, n) or unknown flags:
 * POM_E_ARG.  Counters (POM_CNT_*) and the handle's tick do not change.  Like pom_batch_upload the call first settles chained
 * launches; the copy itself is queued on the handle's stream and does not block.
 *
 * How it moves (pom_copy.h): one wavefront per destination tile gathers the tile with its new columns into a scratch image (state
 * columns are 124 bytes at byte c * 16 + e % 16 plus dwords 31..79 at dword d * 16 + e % 16 of the tile; snapshot and terminal
 * records are dense 80-dword records), then a second kernel writes the image back in whole tiles.  The scratch (320 B + 36 B per
 * env, + 320 B with POM_RESET_AT_END) is allocated on first use and freed by pom_batch_destroy.  The host variant skips the
 * scratch when no source lies in [first, first + count) (fan-out): the same bytes, one pass.
 */
enum { POM_COPY_FROM_SNAPSHOT = 1, POM_COPY_SET_SNAPSHOT = 2 };
int pom_batch_copy_envs(PomBatch* h, const int64_t* src_host, int64_t first, int64_t count, int32_t flags);
int pom_batch_copy_envs_device(PomBatch* h, const int64_t* src_dev, int64_t first, int64_t count, int32_t flags);

/* one tick with explicit moves: int32[n_envs][4], host or device memory */
int pom_batch_step(PomBatch* h, const int32_t* moves_host);
int pom_batch_step_device(PomBatch* h, const int32_t* moves_dev);
/* `ticks` ticks of bboard::Step(State*, Move[4]) with explicit moves from a TAPE in device memory, int32[ticks][n_envs][4] (tick t
 * of env e reads moves_dev[(t * n_envs + e) * 4 ..]; dead agents' entries included): what K calls of pom_batch_step_device with
 * moves_dev + t * n_envs * 4 do — same states, same counters — but issued as chained launches where the handle chains
 * (POM_ISSUE_CHAIN; ticks >= 2), i.e. at the speed of pom_batch_step_random instead of one joined launch per tick.  For replays,
 * open-loop rollouts and planners that fix K moves ahead; a policy that needs the state of tick t to choose the move of tick
 * t + 1 calls pom_batch_step_device per tick.  The tape is read asynchronously: it was written on the handle's stream (or before
 * the call) and must stay unchanged until the handle has been synchronised (pom_batch_sync, or any call that reads results
 * back).  Does not advance the tick of the synthetic move stream.  With POM_RESET_AT_END the caller sees only the last tick's
 * "finished" marks; winner / length of each env's most recent episode are kept as always. */
int pom_batch_step_device_many(PomBatch* h, const int32_t* moves_dev, int32_t ticks);
/* `ticks` ticks with the pom_rng.h move stream (seed, env_offset+env, tick); ticks_per_launch >= 1 keeps
 * the env tile resident in LDS for that many ticks per kernel launch (1 = state round-trips HBM each tick) */
int pom_batch_step_random(PomBatch* h, uint64_t seed, int32_t dist, int32_t ticks, int32_t ticks_per_launch);
/* SimpleAgent policy on the device (agents::SimpleAgent, include/agents.hpp:55-76, src/agents/simple_agent.cpp):
 * pom_batch_policy_simple asks all four agents of every env for a Move as Environment::Step does (environment.cpp:139-146:
 * live agents only, a dead agent's entry is IDLE) into the handle's move buffer and updates the agents' memory
 * (recentPositions, moveQueue); pom_batch_step_policy ticks with those moves; pom_batch_step_simple does both `ticks` times.
 * The one random draw an act() may make comes from the pom_rng.h stream keyed (seed, env_offset+env, tick), uniform 0..4.
 * An env that the next step will restart is read from its snapshot and gets fresh agents; pom_batch_upload resets the agents
 * of the uploaded envs.  moves_out_host (nullable): int32[n_envs][4], synchronises. */
int pom_batch_policy_simple(PomBatch* h, uint64_t seed, int32_t* moves_out_host);
int pom_batch_step_policy(PomBatch* h);
int pom_batch_step_simple(PomBatch* h, uint64_t seed, int32_t ticks);
/* the handle's move buffer in device memory, int32[n_envs][4]: what pom_batch_policy_simple fills and pom_batch_step_policy
 * consumes.  A device-side consumer may overwrite entries in between (on the handle's stream, see pom_batch_stream) — e.g. a
 * learned policy for agent 0 playing against three SimpleAgents — without a host round trip. */
int pom_batch_moves_device(PomBatch* h, int32_t** moves_dev);
/* agent memory of envs [first, first+count): 16 int32 per agent, 4 agents per env: recentPositions {x,y}x4, index, count,
 * moveQueue x4, index, count (the members of SimpleAgent that survive between act() calls) */
int pom_batch_policy_memory(PomBatch* h, int64_t first, int64_t count, int32_t* out16);
/* the tick counter that keys the synthetic stream (advanced by step_random / step_policy / step_simple) */
int pom_batch_set_tick(PomBatch* h, int64_t tick);

/* per-env results for [first, first+count): any output pointer may be NULL.
 * done/draw are 0/1, winner is -1 or the agent id (Environment::IsDone/IsDraw/GetWinner, environment.cpp:195-208) */
int pom_batch_status(PomBatch* h, int64_t first, int64_t count, int32_t* done, int32_t* winner, int32_t* draw,
                     int32_t* alive, int32_t* time_step, uint32_t* ubflags);

/* POM_RESET_AT_END: per env of [first, first+count), any output may be NULL: `finished` = 1 if the env's latest tick ended an
 * episode (the env now stands on its next start state); winner / draw / length (timeStep reached) / alive of the env's most
 * recently finished episode (-1 / 0 / 0 / 0 while it has not finished any); pom_batch_download_terminal gives that
 * episode's final State (all-zero while there is none).  POM_E_ARG in the other reset modes. */
int pom_batch_last_results(PomBatch* h, int64_t first, int64_t count, int32_t* finished, int32_t* winner, int32_t* draw,
                           int32_t* length, int32_t* alive);
int pom_batch_download_terminal(PomBatch* h, void* states, int64_t first, int64_t count);

int pom_batch_counters(PomBatch* h, int64_t out[POM_CNT_N]);
/* same totals left in device memory (int64[POM_CNT_N]) on the handle's stream, e.g. for an RCCL all-reduce; does not block
 * (and therefore does not run the check behind chained launches: a tile caught up later adds its steps later) */
int pom_batch_counters_device(PomBatch* h, void* dev_int64x4);
int pom_batch_reset_counters(PomBatch* h);
int pom_batch_sync(PomBatch* h);
/* order everything stepped so far before whatever is queued next on the handle's stream, without blocking the host
 * (steps run on internal sub-streams; every other call of this API does this implicitly) */
int pom_batch_flush(PomBatch* h);
/* the opposite, ahead of time: order the internal sub-streams behind what is queued on the handle's stream NOW, so that the
 * next step's launches need no cross-stream event first (a latency-sensitive caller does this before it starts its clock;
 * stepping does it by itself otherwise) */
int pom_batch_fork(PomBatch* h);
/* change the number of streams launches go to (1..8, see PomBatchOptions.streams); results do not depend on it,
 * the best value depends on how many hardware queues the process has free — a caller may try a few and keep the fastest */
int pom_batch_set_streams(PomBatch* h, int32_t streams);
/* per-launch timing with HIP events on the launch streams: enable, step (at most 256 launches are kept), read the mean */
int pom_batch_profile(PomBatch* h, int enable);
int pom_batch_profile_read(PomBatch* h, double* mean_ms, int64_t* launches);
/* how a step is issued: envs per wavefront, lanes per env and kernel launches (sub-batches) per step */
int pom_batch_launch_shape(PomBatch* h, int32_t* envs_per_wave, int32_t* lanes_per_env, int32_t* launches_per_step);
/* how the launches of a several-tick call are issued: the POM_ISSUE_* in force (AUTO resolved; POM_ISSUE_CHAIN only while chained
 * launches are available to the handle) and the number of streams they go to */
int pom_batch_issue_info(PomBatch* h, int32_t* issue_mode, int32_t* streams);

/* chained launches since creation: out[0] launches issued, out[1] checks run (one per join that followed chained launches),
 * out[2] tiles that a check found left behind by a wavefront that could not play them, out[3] ticks replayed for those tiles */
int pom_batch_chain_stats(PomBatch* h, int64_t out[4]);

/* Self-test of the hand-off chained launches rest on, without the game: `launches` launches over `tiles` 7-KB records on `streams`
 * streams; every visit checks that its record is exactly what the visit before it left (all 1,792 dwords) and rewrites it.
 * out[0] records a visit found stale or torn (must be 0), out[1] dwords that differed, out[2] visits played, out[3] visits
 * expected, out[4] tiles whose final record / ticket word is not what `launches` clean visits leave, out[5] POM_CHAIN_E_* flags
 * raised.  POM_E_HIP where the device does not offer chained launches. */
int pom_chain_litmus(int32_t device, int64_t tiles, int32_t launches, int32_t streams, int64_t out[6]);

/* the hipStream_t the handle's work is ordered on (the one given at creation, or the library's own), so that a caller can
 * order its own device work against steps and observations with events instead of pom_batch_sync */
int pom_batch_stream(PomBatch* h, void** stream);

/* zero-copy view for device-side consumers (policies, observation kernels): packed records in tiles of 16 envs,
 * dword d >= 31 (timeStep, agents, bomb and flame queues) of env e at base[(e / 16) * (16 * rec_dwords) + d * 16 + e % 16]; the
 * board (dwords 0..30 of the tile) is laid out by cell: cell c of env e is BYTE c * 16 + e % 16 of its tile, i.e. of
 * (uint8_t*)base + (e / 16) * 64 * rec_dwords; n_pad = envs the buffer holds (a multiple of 64); layout in
 * pomcpp_amd/csrc/pom_packed.h */
int pom_batch_device_view(PomBatch* h, void** base, int64_t* n_pad, int32_t* rec_dwords);

/*
 * Observation export: the current state of every env as dense planes for a training loop, written by one
 * kernel straight into caller-owned DEVICE memory (e.g. a torch tensor's data_ptr) on the handle's stream.  The reference has
 * no such function; the planes restate what its agents read off a State (Item codes and IS_* helpers bboard.hpp:54-109, Bomb
 * accessors :261-335, FLAME_ID :98-101, AgentInfo :228-245), one value per cell, row-major [y][x]:
 *    0 passage   1 rigid   2 wood (any flag)   3 Item::BOMB   4 flames   5 extra-bomb   6 incr-range   7 kick      (0 / 1)
 *    8..11       the cell shows agent 0..3 (per_agent: 8 = the viewer, 9..11 = agents id+1, id+2, id+3 mod 4)      (0 / 1)
 *    12 13 14    BMB_STRENGTH, BMB_TIME, BMB_DIR of the first live bomb in queue order on the cell (State::GetBomb order,
 *                bboard.cpp:277-287); also set under an agent, where the board shows no bomb
 *    15          timeLeft (clamped to 0..255) of the first live flame whose centre is the cell's FLAME_ID, on flame cells
 * planes:  [n][16][11][11] (per_agent = 0) or [n][4][16][11][11] (per_agent = 1: dead agents' views are written too), of
 *          uint8, IEEE half or float (all values are small integers, exact in each).
 * agent_attrs (nullable): int32 [n][4][8] = x, y, alive, ammo (maxBombCount - bombCount), bombCount, maxBombCount,
 *          bombStrength, canKick.   env_attrs (nullable): int32 [n][4] = timeStep, aliveAgents, status (1 done | 2 draw |
 *          4 timed out | 8 restarted: POM_RESET_AT_END put the env on this start state at the end of the last tick), winner
 *          (-1 = none) — the values pom_batch_status reports.
 *
 * POM_OBS_CODES — the compact form, uint8 [n][5][11][11], 605 bytes per env instead of 1,936 (the export is bound by the bytes it
 * writes): for training loops that expand the board themselves (an embedding look-up on the cell code).  The five arrays are the
 * ones a Pommerman observation carries:
 *    0  board: the small numbers of the reference's Item enum (bboard.hpp:54-71) — 0 passage, 1 rigid, 2 wood (any flag), 3 bomb,
 *       4 flames, 5 fog, 6 extra-bomb, 7 incr-range, 8 kick, 9 agent dummy, 10..13 agents 0..3; 255 for anything else
 *    1 2 3  bomb strength, life, direction (planes 12, 13, 14 above)        4  flame life (plane 15 above)
 * per_agent must be 0 (agents are named by id; agent_attrs says who is where).  The agents' own FOGGED views of either form:
 * PomViewSpec below.
 */
enum { POM_OBS_U8 = 0, POM_OBS_F16 = 1, POM_OBS_F32 = 2, POM_OBS_CODES = 3 };
enum { POM_OBS_PLANES = 16, POM_OBS_CODE_PLANES = 5, POM_OBS_AGENT_ATTRS = 8, POM_OBS_ENV_ATTRS = 4 };
int pom_batch_observe(PomBatch* h, void* planes_dev, int32_t dtype, int32_t per_agent, int32_t* agent_attrs_dev,
                      int32_t* env_attrs_dev);
/* pom_batch_step_device followed by pom_batch_observe in ONE launch: the kernel that plays the tick writes the observation of the
 * state it leaves behind while the tile is still in LDS (one read of the records and one launch per RL tick instead of two of
 * each; with POM_RESET_AT_END an env that has just finished shows its next start state, as pom_batch_observe would).  Same
 * outputs, bit for bit, as the two calls. */
int pom_batch_step_device_observe(PomBatch* h, const int32_t* moves_dev, void* planes_dev, int32_t dtype, int32_t per_agent,
                                  int32_t* agent_attrs_dev, int32_t* env_attrs_dev);

/* CLOSED-LOOP stepping: Step(State*, Move[4]) with THIS tick's moves from the caller every tick (the reference's real call shape:
 * Environment::Step collects act() of every agent and then steps, src/bboard/environment.cpp:139-149), without the whole chip
 * waiting for the caller's policy between two ticks.  One tick for the envs [first, first + count) only (whole tiles: first a
 * multiple of 16, count a multiple of 16 or reaching the batch's end), ONE launch on `stream` (NULL: the handle's stream), moves
 * from moves_dev = int32 [n][4] indexed by the env's number in the batch.  planes_dev != NULL: the observation of those envs
 * after the tick is written by the same launch (layout and arguments as pom_batch_observe, the arrays sized for the WHOLE batch;
 * only the range's part is written).  Nothing is forked or joined: the call is ordered by `stream` alone, so a caller that cuts
 * the batch into two or four ranges, each with a stream of its own carrying  policy(range) -> step(range) -> policy(range) ...,
 * has range A's policy running while range B steps — and the chains can be captured into a HIP graph (the call makes no
 * synchronising runtime call once the handle is settled: pom_batch_sync first).  The caller orders the streams behind whatever
 * put the batch into its present state.  The handle's tick (which keys pom_batch_step_random's move stream) does not advance.
 * Quad shape only (POM_E_ARG otherwise).  bench.py: other_configs.closed_loop_65536_envs. */
int pom_batch_step_device_range(PomBatch* h, int64_t first, int64_t count, const int32_t* moves_dev, void* stream, void* planes_dev,
                                int32_t dtype, int32_t per_agent, int32_t* agent_attrs_dev, int32_t* env_attrs_dev);
/*
 * PER-AGENT FOGGED VIEWS: the observation a Pommerman agent really gets — the board through a window around itself, fog elsewhere —
 * for all four agents of every env, written by the export's kernels (no second pass over the planes).  The three calls below are
 * pom_batch_observe, pom_batch_step_device_observe and pom_batch_step_device_range with a PomViewSpec in place of their output
 * arguments; the calls above keep their signatures and behaviour.
 * Viewer and window: view v of env e belongs to agent v, alive or dead (as per_agent = 1 writes dead agents' views too).  Its window is
 *          the set of cells with |x - x_v| <= view_radius and |y - y_v| <= view_radius, x_v, y_v the agent's position as agent_attrs
 *          reports it (a dead agent looks out from where it died), clipped by the board.  No other special cases.  view_radius 4 is
 *          Pommerman's 9x9 window; 10 fogs nothing.
 * planes:  POM_OBS_U8 / _F16 / _F32: [n][4][16][11][11].  Inside the window exactly what pom_batch_observe(per_agent = 1) writes for
 *          that view (planes 8..11 rotated: 8 = the viewer); outside it all 16 planes are 0 — planes 0..11 are one-hot on every real
 *          cell, so an all-zero cell is unambiguously fog.
 *          POM_OBS_CODES: uint8 [n][4][5][11][11].  Inside the window the five bytes pom_batch_observe(POM_OBS_CODES) writes (agents keep
 *          their absolute codes 10..13 in every view); outside it the board plane is 5 (Item::FOG) and planes 1..4 are 0.
 *          Alignment as for per_agent = 1: 4 x the element size (an env's four views are 2,420 / 7,744 elements: every env starts on
 *          that boundary).
 * viewer_attrs (nullable): int32 [n][4][12], rows of 48 bytes, the pointer 16-byte aligned — what a Pommerman observation carries
 *          beside the board, and nothing about the others that the board does not show:
 *          0..7 agent v's own row of agent_attrs (x, y, alive, ammo, bombCount, maxBombCount, bombStrength, canKick), 8 9 10 the alive
 *          flags of agents (v+1)%4, (v+2)%4, (v+3)%4, 11 timeStep.
 * env_attrs (nullable): as pom_batch_observe — done, winner and the rest are public.
 * POM_E_ARG (with a pom_last_error text): a null spec (pom_batch_step_device_range_view: NULL = no observation, the call is
 *          pom_batch_step_device_range without planes), struct_size != sizeof(PomViewSpec) (POM_VIEW_SPEC_SIZE), view_radius outside
 *          0..10, reserved_ != 0, an unknown dtype, a null or misaligned planes_dev, misaligned attribute pointers; nothing is written.
 * Ordering and settling: stream order, the settling of chained launches and the two launches of the one-lane-per-env shapes exactly as
 *          in the three calls above; with POM_RESET_AT_END an env that has just finished shows views of its next start state.  The fused
 *          and the range call equal the step followed by pom_batch_observe_view, bit for bit.
 */
enum { POM_OBS_VIEWER_ATTRS = 12, POM_VIEW_RADIUS_MAX = 10, POM_VIEW_SPEC_SIZE = 40 };
typedef struct PomViewSpec {
    int32_t struct_size;       /* = sizeof(PomViewSpec) */
    int32_t dtype;             /* POM_OBS_U8 / _F16 / _F32 / _CODES */
    int32_t view_radius;       /* 0..10, Chebyshev */
    int32_t reserved_;         /* must be 0 */
    void* planes_dev;          /* [n][4][16][11][11] of dtype, or uint8 [n][4][5][11][11] for POM_OBS_CODES */
    int32_t* viewer_attrs_dev; /* nullable: int32 [n][4][POM_OBS_VIEWER_ATTRS] */
    int32_t* env_attrs_dev;    /* nullable: as pom_batch_observe */
} PomViewSpec;
int pom_batch_observe_view(PomBatch* h, const PomViewSpec* spec);
int pom_batch_step_device_observe_view(PomBatch* h, const int32_t* moves_dev, const PomViewSpec* spec);
int pom_batch_step_device_range_view(PomBatch* h, int64_t first, int64_t count, const int32_t* moves_dev, void* stream,
                                     const PomViewSpec* spec);

/*
 * MIXED STEP: the closed-loop range call with SimpleAgent opponents — "my network plays some of the agents, agents::SimpleAgent the
 * rest, every agent sees its fogged view" as ONE launch per range and tick.  The three-call recipe (pom_batch_policy_simple, an
 * overwrite of the move buffer, pom_batch_step_policy, then an observation) is three launches on the whole batch, two reads of every
 * record and a Move[4] round trip through memory, and has no range form; this call is pom_batch_step_device_range(_view) with the
 * policy of pom_batch_step_simple inside it for the agents of simple_mask.
 * Semantics, per env e of [first, first + count) (whole tiles, as pom_batch_step_device_range), in this order:
 *   1 Restart at the start.  POM_RESET_AT_START and e finished: the env restarts from its snapshot, or on the next generated board
 *          (fresh_boards), and the SimpleAgent memory of ALL FOUR of its agents becomes zero — as pom_batch_step_simple does it.
 *   2 Finished envs.  POM_MODE_ENV, e finished and not restarted: nothing happens — no act, memory untouched, no tick.
 *   3 SimpleAgent moves.  Every LIVE agent a of simple_mask is asked exactly as pom_batch_policy_simple(seed) asks it at handle tick
 *          `tick`: SimpleAgent::act on the current state, its one draw (agent a's 16 bits of the pom_rng.h draw keyed (seed,
 *          env_offset + e, tick)) * 5 >> 16, its memory updated in place.  A dead agent of the mask gives IDLE.
 *   4 Explicit moves.  Every agent NOT in the mask gets moves_dev[e][a], dead agents' entries included (step_utility.cpp:138-170).  It
 *          is not asked, and its memory is not touched (pom_batch_rollout_policy's rule: an actor is in the mask and alive).
 *   5 The tick, its bookkeeping, counters, ubflags, terminal record and `finished` mark: exactly as pom_batch_step_device_range,
 *          POM_RESET_AT_END included — the finishing tick restarts the env, marks it restarted and wipes all four agents' memory.
 *   6 Observation: exactly as pom_batch_step_device_range (planes_dev) / _range_view (view) writes it for the range; the arrays are
 *          sized for the WHOLE batch and rows outside the range are not touched.
 * Ranges advance on their own, so the handle's tick cannot key the draw: `tick` is an argument, and the handle's tick does not
 * advance.  Nothing else changes either: the handle's move buffer (pom_batch_moves_device), envs outside the range, snapshots.
 * Equivalences:
 *   simple_mask == 0 is pom_batch_step_device_range(_view), bit for bit (which knows nothing of the agents' memory: nobody is asked
 *          here either, but where the memory exists step 1 and step 5 wipe that of the envs they restart).
 *   Any mask, first = 0, count = n equals, on a twin handle, pom_batch_set_tick(tick); pom_batch_policy_simple(seed); the entries of
 *          the move buffer of agents outside the mask overwritten with moves_dev; pom_batch_step_policy; pom_batch_observe(_view) —
 *          records, status, episodes, counters, terminal records and observation, and the memory of the mask's agents.  The memory
 *          of the agents outside the mask is what it was before the call, or zero where the env restarted in this call.  (One
 *          difference, with POM_RESET_AT_END: the sequence's tick has no policy in it and leaves the memory of an env that it
 *          restarts as it was; this call wipes it — step 5, as pom_batch_step_simple does.)
 *   simple_mask == 15, first = 0, count = n equals pom_batch_set_tick(tick); pom_batch_step_simple(seed, 1), bit for bit, memory included.
 * Ordering, settling, memory: as pom_batch_step_device_range — the handle is settled, nothing is forked or joined, ONE launch on
 *          `stream`, no synchronising runtime call once the handle is settled.  The one exception: the agents' memory is allocated
 *          and cleared by the first call with simple_mask != 0 on a handle that has none yet (no policy call before it), and that
 *          call synchronises the handle's stream once, so that the clear is ordered before any later launch on any stream.  A call
 *          with count == 0 is defined to do only that: make it once before capturing mixed steps into a graph.
 * POM_E_ARG (with a pom_last_error text naming pom_batch_step_mixed; nothing is launched): a null handle or spec, struct_size !=
 *          sizeof(PomMixedStepSpec) (POM_MIXED_STEP_SPEC_SIZE), simple_mask outside 0..15, tick outside 0..2^32-1, nonzero flags or
 *          reserved_, a null moves_dev with simple_mask != 15, moves_dev not 4-byte aligned, whatever pom_batch_step_device_range
 *          refuses of a range, pom_batch_observe of a plain observation and PomViewSpec of a view, `view` together with planes_dev,
 *          `view` together with a non-NULL env_attrs_dev, a launch shape other than the quad shape.
 * Not here: a host-pointer variant, several ticks per launch, a chained form, policies other than SimpleAgent, a mask per env, the
 *          one-lane-per-env shapes.
 */
enum { POM_MIXED_STEP_SPEC_SIZE = 104 }; /* 2 x int32, 2 x int64, pointer, uint64, int64, 3 pointers, 2 x int32, 2 pointers, 2 x int32: no implicit padding on an LP64 target */
typedef struct PomMixedStepSpec {
    int32_t struct_size;       /*   0  = sizeof(PomMixedStepSpec) */
    int32_t simple_mask;       /*   4  bit a: agent a plays SimpleAgent; 0..15 */
    int64_t first;             /*   8  whole tiles, as pom_batch_step_device_range */
    int64_t count;             /*  16 */
    const int32_t* moves_dev;  /*  24  int32 [n][4], indexed by the env's number in the batch; required unless simple_mask == 15 */
    uint64_t seed;             /*  32  seed of the SimpleAgent draw */
    int64_t tick;              /*  40  0 .. 2^32-1: keys this call's SimpleAgent draw */
    void* stream;              /*  48  NULL: the handle's stream */
    const PomViewSpec* view;   /*  56  nullable: the fogged views */
    void* planes_dev;          /*  64  nullable: the plain observation, as pom_batch_step_device_range */
    int32_t dtype;             /*  72  POM_OBS_* */
    int32_t per_agent;         /*  76 */
    int32_t* agent_attrs_dev;  /*  80  nullable */
    int32_t* env_attrs_dev;    /*  88  nullable; NULL if view is given (view->env_attrs_dev is the one used) */
    int32_t flags;             /*  96  must be 0 */
    int32_t reserved_;         /* 100  must be 0 */
} PomMixedStepSpec;
int pom_batch_step_mixed(PomBatch* h, const PomMixedStepSpec* spec);

/*
 * FORECAST: where will the fire be, and when — flames and deaths K ticks ahead, without touching the batch.  The reference's own
 * answer is strategy::IsInDanger (src/bboard/strategy.cpp:229-249), the smallest timer over the bombs whose cross covers a cell; its
 * comment says "TODO: add consideration for chained bomb explosions", and it knows nothing of walls, wood or moving bombs either.
 * Here the tick itself answers: one launch plays K ticks of bboard::Step (include/bboard.hpp:668, src/bboard/step.cpp:9-284) on a
 * scratch copy of every env that is never stored, so chains, blocked rays, wood turning into flames, kicked bombs in flight and
 * agents dying where they stand are all in it.  With moves_dev it answers "what happens if we do this": six calls, one per move
 * of an agent, are that agent's action-safety mask.
 * Semantics: for every env e < n, S_0 = a private copy of its current State and S_t = bboard::Step(S_{t-1}, m_t) for t = 1 .. K =
 *          horizon, with m_1 = moves_dev[e] (all four entries, dead agents' included, as pom_batch_step_device reads them:
 *          step_utility.cpp:138-170) or IDLE x 4 if moves_dev is NULL, and m_t = IDLE x 4 for t >= 2.  Bare Step as in
 *          POM_MODE_RAW whatever the handle's mode: no timeStep++ (environment.cpp:148-150), no done / max_steps logic
 *          (environment.cpp:125-128, 152-168), no restart; a finished env is forecast like any other.
 * flame_tick[e][y][x] (required; uint8 [n][11][11], row-major [y][x]): the smallest t in 1 .. K with IS_FLAME(S_t.board[y][x])
 *          (bboard.hpp:85), 0 if there is none.  A cell that burns now gets 1 only if it still burns after tick 1.
 * agent_tick[e][a] (nullable; int32 [n][4]): -1 if agent a is dead in S_0 (AgentInfo::dead, bboard.hpp:239); otherwise the smallest
 *          t with S_t.agents[a].dead; 0 if the agent is alive in S_K.
 * ubflags[e] (nullable; uint32 [n]): the OR of the POM_UB_* flags (pom_state.h) the K ticks raised, with the stepper's documented
 *          fallbacks as in a real tick.  The env's own flags (pom_batch_status) are neither included nor changed.
 * Nothing else changes: after the call nothing this API can read differs from before — records, snapshots and terminal records,
 *          status and the envs' own ubflags, POM_CNT_* (forecast ticks are not steps), episode counters, the handle's tick, agent
 *          memory, chain statistics.
 * Ordering: exactly as pom_batch_observe — chained launches are settled and the sub-streams joined first, then ONE launch on the
 *          handle's stream; moves_dev is read and the outputs are written in stream order.  Every launch shape of the handle gives
 *          the same outputs (the device buffers are 16-env tiles whatever the shape).
 * POM_E_ARG (with a pom_last_error text; nothing is written): a null handle or spec, struct_size != sizeof(PomForecastSpec)
 *          (POM_FORECAST_SPEC_SIZE), horizon outside 1 .. POM_FORECAST_MAX_TICKS, nonzero reserved_, a null flame_tick_dev,
 *          flame_tick_dev or agent_tick_dev not 16-byte aligned, ubflags_dev or moves_dev not 4-byte aligned.
 */
enum { POM_FORECAST_MAX_TICKS = 32, POM_FORECAST_SPEC_SIZE = 48 };
typedef struct PomForecastSpec {
    int32_t struct_size;        /* = sizeof(PomForecastSpec) */
    int32_t horizon;            /* K, 1..POM_FORECAST_MAX_TICKS */
    int32_t reserved_[2];       /* must be 0 */
    const int32_t* moves_dev;   /* nullable: int32 [n][4], the moves of forecast tick 1 (dead agents' entries included,
                                   as pom_batch_step_device reads them); NULL = IDLE.  Ticks 2..K are always all-IDLE */
    uint8_t* flame_tick_dev;    /* required: uint8 [n][11][11], row-major [y][x] */
    int32_t* agent_tick_dev;    /* nullable: int32 [n][4] */
    uint32_t* ubflags_dev;      /* nullable: uint32 [n] */
} PomForecastSpec;
int pom_batch_forecast(PomBatch* h, const PomForecastSpec* spec);

/*
 * ROLLOUT: how does the game end — R random playouts of every env to a finished game or a horizon of K ticks, without touching
 * the batch.  What Monte-Carlo leaf evaluation, a roll-out baseline for a value head and "which of my six moves survives most
 * often" need.  The reference plays a game out with Environment::StartGame (src/bboard/environment.cpp:68-88:
 * Step until IsDone or the step bound) over RandomAgents (src/agents/basic_agents.cpp:12-22); here ONE launch plays all R x n
 * playouts, each on a scratch copy of its env's 16-env tile that is never stored.
 * Semantics: for every env e < n and sample r < R = samples: S_0 = a private copy of the env's current State and status, and
 *          seed_r = pom_splitmix64(seed + r) (pom_rng.h).  For t = 1 .. K = horizon: stop if the game is finished
 *          (Environment::Step returns early, environment.cpp:125-128); otherwise m_t = moves_dev[e] if t == 1 and moves_dev is
 *          not NULL (all four entries, dead agents' included: step_utility.cpp:138-170), else
 *          m_t = pom_rng_moves(seed_r, env_offset + e, t - 1, dist); S_t = bboard::Step(S_{t-1}, m_t) (include/bboard.hpp:668,
 *          src/bboard/step.cpp:9-284).  After each tick the bookkeeping of Environment::Step (environment.cpp:148-168) whatever
 *          the handle's mode: timeStep++ on the private copy (:150); finished with a winner when aliveAgents == 1 (:152-163,
 *          the last alive index), finished as a draw when aliveAgents == 0 (:164-168), finished and timed out when the handle's
 *          max_steps > 0 and timeStep >= max_steps (StartGame's bound, environment.cpp:71).
 *          "Finished at S_0" is the record's own done bit (pom_batch_status), which is never set on a POM_MODE_RAW handle: such
 *          an env gets length 0 and its recorded outcome in every sample.  No restart is ever played and no fresh board drawn,
 *          whatever auto_reset says.
 * Equivalence: sample r without moves_dev is exactly what a POM_MODE_ENV handle with auto_reset = 0, the same max_steps and the
 *          same env_offset leaves in its statuses after pom_batch_upload(states), pom_batch_set_tick(0),
 *          pom_batch_step_random(seed_r, dist, K, 1); with moves_dev after pom_batch_step_device(moves), pom_batch_set_tick(1),
 *          pom_batch_step_random(seed_r, dist, K - 1, 1).
 * result[r][e] (required; uint32 [R][n], sample-major): POM_RO_ALIVE bit a = agent a is alive in the last state played
 *          (!AgentInfo::dead, bboard.hpp:239); POM_RO_DONE, POM_RO_DRAW (Environment::IsDone / IsDraw, environment.cpp:195-203),
 *          POM_RO_TIMEOUT; POM_RO_UB = some played tick raised a POM_UB_* flag (pom_state.h; the documented fallbacks apply as in
 *          a real tick; the env's own flags are neither read into this bit nor changed); bits POM_RO_WINNER_SHIFT .. + 2 =
 *          Environment::GetWinner() + 1 (environment.cpp:205-208), 0 for none; bits POM_RO_LENGTH_SHIFT .. 31 = ticks played.
 *          Every other bit is 0.
 * Nothing else changes: after the call nothing this API can read differs from before — records, snapshots and terminal records,
 *          status and the envs' ubflags, POM_CNT_* (rollout ticks are not steps), episode counters, the handle's tick, agent
 *          memory, chain statistics.
 * Ordering: exactly as pom_batch_forecast — chained launches are settled and the sub-streams joined first, then ONE launch on the
 *          handle's stream; moves_dev is read and result_dev written in stream order.  Every launch shape of the handle gives the
 *          same words.
 * POM_E_ARG (with a pom_last_error text; nothing is written): a null handle or spec, struct_size != sizeof(PomRolloutSpec)
 *          (POM_ROLLOUT_SPEC_SIZE), horizon outside 1 .. POM_ROLLOUT_MAX_TICKS, samples outside 1 .. POM_ROLLOUT_MAX_SAMPLES, dist
 *          no POM_DIST_*, nonzero reserved_, a null result_dev, result_dev not 16-byte aligned, moves_dev not 4-byte aligned; and a
 *          batch so large that samples x tiles does not fit one grid (more than 2^31 workgroups: call with fewer samples).
 * Not here: SimpleAgent playouts (pom_batch_rollout_policy below), reductions over the samples (torch does them on the words).
 *          Playouts of SOME envs, or several per env with different first moves: pom_batch_rollout_jobs below.
 */
enum { POM_ROLLOUT_MAX_TICKS = 1024, POM_ROLLOUT_MAX_SAMPLES = 256, POM_ROLLOUT_SPEC_SIZE = 48 };
enum { /* the result word */
    POM_RO_NONE = 0,           /* pom_batch_rollout_jobs: an entry of the list without a job (a played job's length is >= 1, or its DONE bit set) */
    POM_RO_ALIVE = 0xF,        /* bit a: agent a alive in the last state played */
    POM_RO_DONE = 0x10,
    POM_RO_DRAW = 0x20,
    POM_RO_TIMEOUT = 0x40,
    POM_RO_UB = 0x80,          /* a played tick raised a POM_UB_* flag */
    POM_RO_WINNER_SHIFT = 8,   /* 3 bits: winner + 1, 0 = nobody */
    POM_RO_WINNER_MASK = 0x700,
    POM_RO_LENGTH_SHIFT = 16   /* 16 bits: ticks played, 0 .. horizon */
};
typedef struct PomRolloutSpec {
    int32_t struct_size;       /* = sizeof(PomRolloutSpec) */
    int32_t horizon;           /* K, 1..POM_ROLLOUT_MAX_TICKS */
    int32_t samples;           /* R, 1..POM_ROLLOUT_MAX_SAMPLES */
    int32_t dist;              /* POM_DIST_HARMLESS / _RANDOM / _STRESS (pom_rng.h) */
    uint64_t seed;
    const int32_t* moves_dev;  /* nullable: int32 [n][4], the moves of tick 1 of EVERY sample (dead agents' entries included) */
    uint32_t* result_dev;      /* required: uint32 [R][n], sample-major, 16-byte aligned */
    int64_t reserved_;         /* must be 0 */
} PomRolloutSpec;
int pom_batch_rollout(PomBatch* h, const PomRolloutSpec* spec);

/*
 * ROLLOUT WITH A POLICY: the rollout above with agents::SimpleAgent (include/agents.hpp:55-76, src/agents/simple_agent.cpp) for the
 * agents of simple_mask, the pom_rng.h stream for the others, and a first tick that may be fixed agent by agent: "my move fixed, the
 * others play a sensible policy" — what a search's leaf evaluation and a roll-out baseline need; random agents
 * blow themselves up within a few dozen ticks and say little about the game the caller is in.  ONE launch plays all R x n playouts;
 * the agents' memory (two dwords per agent) is copied per sample into registers and never stored.
 * Semantics: for every env e < n and sample r < R = samples: seed_r = pom_splitmix64(seed + r); S_0 = a private copy of the env's
 *          current State and status; M_0 = a private copy of the env's four SimpleAgent memories as pom_batch_policy_memory reports
 *          them — all-zero (`new SimpleAgent()` with empty queues) if the handle never ran the policy or POM_ROLLOUT_FRESH_AGENTS is
 *          set.  For t = 1 .. K = horizon: stop if the game is finished (environment.cpp:125-128); otherwise
 *          1. every live agent a of simple_mask is asked for a move exactly as pom_batch_policy_simple(seed_r) asks it at handle tick
 *             t - 1: SimpleAgent::act on S_{t-1} (environment.cpp:139-146), its one draw = (agent a's 16 bits of
 *             pom_rng_draw(seed_r, env_offset + e, t - 1)) * 5 >> 16, its memory in M updated; a dead agent of the mask gives IDLE
 *             (environment.cpp:139-146);
 *          2. every agent not in simple_mask gets entry a of pom_rng_moves(seed_r, env_offset + e, t - 1, dist), dead agents too, as
 *             in pom_batch_rollout;
 *          3. at t == 1 every agent of first_mask gets moves_dev[e][a] instead (dead agents' entries are read as
 *             pom_batch_step_device reads them: step_utility.cpp:138-170).  A SimpleAgent overridden this way has still been asked
 *             and its memory has moved on: the "overwrite entries of the move buffer between pom_batch_policy_simple and
 *             pom_batch_step_policy" pattern of pom_batch_moves_device;
 *          4. S_t = bboard::Step(S_{t-1}, m_t) (include/bboard.hpp:668, src/bboard/step.cpp:9-284), then the bookkeeping of
 *             Environment::Step (environment.cpp:148-168: timeStep++, winner / draw; the handle's max_steps as StartGame's bound,
 *             environment.cpp:71) exactly as pom_batch_rollout does it, whatever the handle's mode.
 *          An env finished at S_0 (the record's own done bit) gets length 0 and its recorded outcome in every sample.
 * result[r][e]: pom_batch_rollout's word, bit for bit (POM_RO_*).
 * Equivalences: simple_mask == 0 with first_mask == 0 (no moves_dev needed), or with first_mask == 0xF and moves_dev, gives exactly
 *          pom_batch_rollout's words without / with moves_dev.  simple_mask == 0xF, first_mask == 0, POM_ROLLOUT_FRESH_AGENTS: sample r
 *          is what a POM_MODE_ENV handle with auto_reset = 0, the same max_steps and the same env_offset leaves in its statuses after
 *          pom_batch_upload(states), pom_batch_set_tick(0), pom_batch_step_simple(seed_r, K).  Without POM_ROLLOUT_FRESH_AGENTS sample r
 *          is what the handle itself would reach by pom_batch_set_tick(0), pom_batch_step_simple(seed_r, K) from where it stands
 *          (no restart is played: an env that finishes stays finished).
 * Nothing else changes: as pom_batch_rollout — records, snapshots and terminal records, status and ubflags, POM_CNT_*, episode
 *          counters, the handle's tick, agent memory, chain statistics are as before the call.
 * Ordering: exactly as pom_batch_rollout — chained launches are settled and the sub-streams joined first, then ONE launch on the
 *          handle's stream; moves_dev and the agents' memory are read and result_dev is written in stream order.
 * POM_E_ARG (with a pom_last_error text naming pom_batch_rollout_policy; nothing is written): everything pom_batch_rollout refuses
 *          (struct_size != sizeof(PomRolloutPolicySpec) = POM_ROLLOUT_POLICY_SPEC_SIZE), simple_mask or first_mask outside 0 .. 15,
 *          first_mask != 0 with a null moves_dev, flags other than 0 or POM_ROLLOUT_FRESH_AGENTS, nonzero reserved_.  A non-null
 *          moves_dev with first_mask == 0 is accepted and not read.
 */
enum { POM_ROLLOUT_FRESH_AGENTS = 1 };            /* flags */
enum { POM_ROLLOUT_POLICY_SPEC_SIZE = 56 };
typedef struct PomRolloutPolicySpec {
    int32_t struct_size;       /* = sizeof(PomRolloutPolicySpec) */
    int32_t horizon;           /* K, 1..POM_ROLLOUT_MAX_TICKS */
    int32_t samples;           /* R, 1..POM_ROLLOUT_MAX_SAMPLES */
    int32_t dist;              /* POM_DIST_*: the stream of the agents NOT in simple_mask */
    uint64_t seed;
    const int32_t* moves_dev;  /* nullable: int32 [n][4], tick-1 moves of the agents in first_mask */
    uint32_t* result_dev;      /* required: uint32 [R][n], sample-major, 16-byte aligned */
    int32_t simple_mask;       /* bit a: agent a plays SimpleAgent; else the pom_rng.h stream under dist */
    int32_t first_mask;        /* bit a: agent a's move of tick 1 is moves_dev[e][a] */
    int32_t flags;             /* 0 or POM_ROLLOUT_FRESH_AGENTS */
    int32_t reserved_;         /* must be 0 */
} PomRolloutPolicySpec;
int pom_batch_rollout_policy(PomBatch* h, const PomRolloutPolicySpec* spec);

/*
 * ROLLOUT OF A LIST OF JOBS: pom_batch_rollout_policy's playouts for a device-side list of (source env, moves of tick 1) instead of
 * one entry per env of the batch — what a search asks for: an agent's six-move table in ONE call (six jobs per env), the leaves
 * worth evaluating out of a large batch without playing the others and without a second handle.  ONE launch plays
 * all R x m playouts.
 * Semantics, by reduction: result[r][j] is, bit for bit, the word pom_batch_rollout_policy would write at result[r][src[j]] for the
 *          same horizon, samples, dist, seed, masks and flags, given a moves_dev whose row src[j] is moves[j].  That is: S_0 = a
 *          private copy of env src[j]'s current record and status; M_0 = a private copy of that env's SimpleAgent memory, or fresh
 *          agents, as pom_batch_rollout_policy defines it; seed_r = pom_splitmix64(seed + r); every draw is keyed by the SOURCE env,
 *          env_offset + src[j] — the job's number is never the key.  Hence:
 *          - jobs that share a source play under common random numbers: their words differ only through their first moves, the
 *            paired comparison a move table wants;
 *          - two jobs with the same source and the same moves give the same words.  More independent playouts come from `samples`.
 *          Sources may repeat and come in any order.  An entry with src[j] < 0 or src[j] >= n (indices in [n, n_pad) included) is
 *          "no job": its R words are written as POM_RO_NONE = 0, which no job produces (a game not finished at S_0 plays at least one
 *          tick: length >= 1; a finished one has POM_RO_DONE).  jobs == 0: POM_OK, nothing is written.
 * Nothing else changes, Ordering: exactly as pom_batch_rollout_policy — the handle is settled, then ONE launch on the handle's
 *          stream; src_dev, moves_dev and the agents' memory are read and result_dev is written in stream order.
 * POM_E_ARG (with a pom_last_error text naming pom_batch_rollout_jobs; nothing is written): everything pom_batch_rollout_policy
 *          refuses (struct_size != sizeof(PomRolloutJobsSpec) = POM_ROLLOUT_JOBS_SPEC_SIZE); jobs < 0; with jobs > 0 a null src_dev or
 *          result_dev, src_dev not 8-byte or result_dev not 16-byte aligned; first_mask != 0 with a null moves_dev; and a list so
 *          long that samples x groups of 16 jobs (rounded up to 8) does not fit one grid.
 * Not here: stream keys per job, a host-pointer variant, reductions over the samples, a source's snapshot as S_0.
 */
enum { POM_ROLLOUT_JOBS_SPEC_SIZE = 72 };
typedef struct PomRolloutJobsSpec {
    int32_t struct_size;       /*  0  = sizeof(PomRolloutJobsSpec) */
    int32_t horizon;           /*  4  K, 1..POM_ROLLOUT_MAX_TICKS */
    int32_t samples;           /*  8  R, 1..POM_ROLLOUT_MAX_SAMPLES */
    int32_t dist;              /* 12  POM_DIST_*: the stream of the agents not in simple_mask */
    uint64_t seed;             /* 16 */
    int64_t jobs;              /* 24  m >= 0 */
    const int64_t* src_dev;    /* 32  required if m > 0: int64 [m], job j plays env src[j]; 8-byte aligned */
    const int32_t* moves_dev;  /* 40  nullable: int32 [m][4], PER JOB: tick-1 moves of the agents in first_mask */
    uint32_t* result_dev;      /* 48  required if m > 0: uint32 [R][m], sample-major, 16-byte aligned */
    int32_t simple_mask;       /* 56 */
    int32_t first_mask;        /* 60 */
    int32_t flags;             /* 64  0 or POM_ROLLOUT_FRESH_AGENTS */
    int32_t reserved_;         /* 68  must be 0 */
} PomRolloutJobsSpec;
int pom_batch_rollout_jobs(PomBatch* h, const PomRolloutJobsSpec* spec);

/*
 * EXPAND: create the nodes of a search — for a device-side list, env first + j becomes the SUCCESSOR of env src[j] under moves[j]:
 * the copy of pom_batch_copy_envs (flags 0) and one tick, in ONE launch, for any range of destinations (not only whole 16-env
 * tiles), with one result word per child in pom_batch_rollout's format — which children are terminal is known without reading
 * pom_batch_status back — and, optionally, the observation of the new nodes for a value network.  With src[j] = first + j the same
 * call is a MASKED STEP: tick these envs only, with these moves.
 * Semantics: job j has destination d = first + j and source s = src[j].
 *   No job: env d is left bit for bit as it was and result[j] = POM_RO_NONE = 0 when s < 0; when s >= n (indices in [n, n_pad) and
 *          huge values included); and when s lies inside [first, first + count) and s != d.  The last is the only aliasing a one-pass
 *          kernel cannot serve — a slot that is being filled cannot be somebody's parent in the same call — and a search never has
 *          it: parents are not among the slots being filled.  Sources outside the range may repeat and come in any order.
 *   Otherwise env d first becomes what pom_batch_copy_envs with flags 0 makes of it: the source's current record with status and
 *          ubflags, its SimpleAgent memory (if allocated), its episode counter and, with POM_RESET_AT_END, its terminal record and
 *          last results; for s == d nothing is copied.  Then ONE tick is played on d with moves[j] (all four entries, dead agents'
 *          included: step_utility.cpp:138-170), as the handle's mode says: POM_MODE_RAW bare bboard::Step, no timeStep++;
 *          POM_MODE_ENV a finished source gives an unticked copy (environment.cpp:125-128), otherwise Step, timeStep++ and done /
 *          winner / draw / max_steps as in every tick (environment.cpp:148-168, :71).  The tick's POM_UB_* flags are ORed into the
 *          child's ubflags as in any tick.
 *   No restart is ever played and no fresh board drawn, whatever auto_reset and fresh_boards say: a child that finishes STAYS
 *          finished (with POM_RESET_AT_END it is not marked "restarted" and its terminal record stays its source's) — a search wants
 *          its terminal nodes.  What later ordinary steps do with such an env: with POM_RESET_AT_START the next tick restarts it
 *          (snapshot or next generated board) and steps that; with auto_reset 0 and with POM_RESET_AT_END it is skipped, tick after
 *          tick, until it is overwritten (pom_batch_copy_envs, pom_batch_upload, another expansion).
 * result[j] (nullable; uint32 [count]): the POM_RO_* word of the child as it now stands — POM_RO_ALIVE bits, POM_RO_DONE / _DRAW /
 *          _TIMEOUT, winner + 1 — POM_RO_UB if THIS tick raised a flag, and the length: 1 if a tick was played, 0 for the unticked copy
 *          of a finished source (which has POM_RO_DONE, so no job's word is 0).  With POM_MODE_RAW the status bits are whatever the
 *          record carries (0).
 * Counters: expansion ticks are steps of the batch.  POM_CNT_STEPS grows by the ticks played, POM_CNT_EPISODES by the children that
 *          finish in this tick, POM_CNT_UB_TICKS as usual; POM_CNT_RESETS, the handle's tick, the snapshots and the chain statistics
 *          do not change.
 * Observation: with planes_dev the launch also writes the observation of every env < n of the destination tiles first / 16 ..
 *          (first + count - 1) / 16 — arguments, layouts and alignment exactly as pom_batch_step_device_range, the arrays sized for
 *          the WHOLE batch.  Envs of a partly covered tile that are not destinations get the observation of their unchanged state.
 *          Fogged views are not part of this.
 * Ordering: as pom_batch_copy_envs_device — the handle is settled first, then ONE launch on the handle's stream; src_dev and
 *          moves_dev are read in stream order, the call does not block.
 * POM_E_ARG (with a pom_last_error text naming pom_batch_expand; nothing is written): a null handle or spec, struct_size !=
 *          sizeof(PomExpandSpec) (POM_EXPAND_SPEC_SIZE), nonzero flags or reserved_, count < 0, a range outside [0, n); with count > 0
 *          a null src_dev or moves_dev, src_dev not 8-byte, moves_dev or result_dev not 4-byte aligned; with planes_dev whatever
 *          pom_batch_observe refuses; a launch shape other than the quad shape.  count == 0: POM_OK, nothing is written.
 * Not here: a host-pointer list, fogged views, more than one tick per job, sources read from snapshots, a stream argument.
 */
enum { POM_EXPAND_SPEC_SIZE = 88 }; /* 2 x int32, 2 x int64, 4 pointers, 2 x int32, 2 pointers, int64: no implicit padding on an LP64 target */
typedef struct PomExpandSpec {
    int32_t struct_size;       /*  0  = sizeof(PomExpandSpec) */
    int32_t flags;             /*  4  must be 0 */
    int64_t first;             /*  8  destinations: env first + j, j in [0, count); any range inside [0, n) */
    int64_t count;             /* 16 */
    const int64_t* src_dev;    /* 24  required if count > 0: int64 [count], 8-byte aligned */
    const int32_t* moves_dev;  /* 32  required if count > 0: int32 [count][4], a row per JOB, dead agents' entries included */
    uint32_t* result_dev;      /* 40  nullable: uint32 [count], 4-byte aligned */
    void* planes_dev;          /* 48  nullable: the observation of the tiles touched, as pom_batch_step_device_range */
    int32_t dtype;             /* 56  POM_OBS_* */
    int32_t per_agent;         /* 60 */
    int32_t* agent_attrs_dev;  /* 64  nullable */
    int32_t* env_attrs_dev;    /* 72  nullable */
    int64_t reserved_;         /* 80  must be 0 */
} PomExpandSpec;
int pom_batch_expand(PomBatch* h, const PomExpandSpec* spec);

/*
 * MOVE SAFETY: an action mask — which of an agent's six moves does it survive, and from which is there somewhere to walk to?  All six
 * candidates of every asked agent of every env in ONE launch, without touching the batch.  The six-forecast recipe
 * gives the first answer at 6 launches per agent and a flame plane per call that a mask never reads; and its rule, "do m, then stand
 * still", calls BOMB fatal for every horizon >= 11 (the planted bomb goes off under the agent in tick 11), which is true of an agent
 * that stands still and useless for one that can walk.  Hence two answers per candidate: the exact one under that rule, and a stated
 * heuristic for "is there a way out".
 * Semantics: for every env e < n, agent a of agent_mask and candidate m in 0 .. 5 (IDLE, UP, DOWN, LEFT, RIGHT, BOMB): S_0 = a
 *          private copy of the env's current State; the moves of tick 1 are moves_dev[e] (IDLE x 4 if moves_dev is NULL) with entry a
 *          replaced by m — all four entries are read, dead agents' included, as pom_batch_step_device reads them
 *          (step_utility.cpp:138-170); S_1 = bboard::Step(S_0, those moves) and S_t = bboard::Step(S_{t-1}, IDLE x 4) for t = 2 .. K =
 *          horizon (include/bboard.hpp:668, src/bboard/step.cpp:9-284).  Bare Step as in POM_MODE_RAW whatever the handle's mode,
 *          exactly as pom_batch_forecast: no timeStep++, no done / max_steps logic, no restart; a finished env is played like any other.
 * death_tick[e][a][m] (nullable; int8 [n][4][6]), the exact answer: -1 if agent a is dead in S_0 (AgentInfo::dead, bboard.hpp:239);
 *          otherwise the smallest t with S_t.agents[a].dead; 0 if it is alive in S_K.  By definition the agent_tick[e][a] that
 *          pom_batch_forecast returns for the same horizon and those tick-1 moves.
 * escape_tick[e][a][m] (nullable; int8 [n][4][6]), "is there a way out", a heuristic defined exactly: Free_t = the cells whose
 *          S_t.board value is PASSAGE or IS_POWERUP (IS_WALKABLE, bboard.hpp:77-84), plus agent a's own cell while a is alive in S_t;
 *          flames, walls, wood, bombs and other agents are not free.  R_1 = {a's position in S_1} if a is alive in S_1, else {};
 *          R_t = (R_{t-1} and its four neighbours on the board) intersected with Free_t for t >= 2 — the cells a walker that makes at
 *          most one step per tick onto free cells can stand on after tick t.  The output is -1 if a is dead in S_0; otherwise the
 *          smallest t with R_t = {}; 0 if R_K is not empty: the agent can still be somewhere when the horizon ends.
 *          What the heuristic leaves out: a walker does not push the simulation — it picks nothing up, kicks nothing, collides with
 *          nobody, and the flames, bombs and other agents it walks among are those of the play in which the agent stood still.  It may
 *          step back onto a cell whose bomb it left (the cell is a bomb's only once the agent has gone; here the agent never goes).
 *          Consequences: death_tick == 0 implies escape_tick == 0 (the agent's own cell is free while it lives, so it is in every
 *          R_t); when both are > 0, escape_tick >= death_tick (R is empty only once the agent is dead).
 * Rows: the rows [e][a][*] of agents outside agent_mask are not written.  At least one of the two outputs is given.
 * Nothing else changes: after the call nothing this API can read differs from before — records, snapshots and terminal records,
 *          status and the envs' own ubflags, POM_CNT_* (these ticks are not steps), episode counters, the handle's tick, agent
 *          memory, chain statistics.
 * Ordering: exactly as pom_batch_forecast — chained launches are settled and the sub-streams joined first, then ONE launch on the
 *          handle's stream; moves_dev is read and the outputs are written in stream order.  Every launch shape of the handle gives
 *          the same bytes (the device buffers are 16-env tiles whatever the shape).
 * POM_E_ARG (with a pom_last_error text naming pom_batch_move_safety; nothing is written): a null handle or spec, struct_size !=
 *          sizeof(PomMoveSafetySpec) (POM_MOVE_SAFETY_SPEC_SIZE), horizon outside 1 .. POM_FORECAST_MAX_TICKS, agent_mask outside
 *          1 .. 15, nonzero reserved_ or reserved2_, both outputs null, an output not 8-byte aligned, moves_dev not 4-byte aligned; and
 *          a batch so large that variants (6 per agent of the mask) x tiles of 16 envs (rounded up to 8) does not fit one grid.
 * Not here: per-variant ubflags, flame planes (pom_batch_forecast has both), a job list, the others playing SimpleAgent
 *          (pom_batch_rollout_jobs has both), a walker that pushes the simulation.
 */
enum { POM_MOVE_SAFETY_SPEC_SIZE = 48 };
typedef struct PomMoveSafetySpec {
    int32_t struct_size;      /*  0  = sizeof(PomMoveSafetySpec) */
    int32_t horizon;          /*  4  K, 1..POM_FORECAST_MAX_TICKS */
    int32_t agent_mask;       /*  8  bit a: judge agent a's moves; 1..15 */
    int32_t reserved_;        /* 12  must be 0 */
    const int32_t* moves_dev; /* 16  nullable: int32 [n][4], the OTHERS' moves of tick 1 (row e, entry a is replaced by the candidate); NULL = IDLE */
    int8_t* death_tick_dev;   /* 24  nullable: int8 [n][4][6], 8-byte aligned */
    int8_t* escape_tick_dev;  /* 32  nullable: int8 [n][4][6], 8-byte aligned; at least one of the two outputs is given */
    int64_t reserved2_;       /* 40  must be 0 */
} PomMoveSafetySpec;
int pom_batch_move_safety(PomBatch* h, const PomMoveSafetySpec* spec);

/*
 * REACH: where can an agent walk, how far is it, and which way does it start?  The reference's reachability map — strategy::FillRMap
 * and, for every reached cell, MoveTowardsPosition (src/bboard/strategy.cpp:58-120, include/strategy.hpp:29-63) — of every asked agent
 * of every env in ONE launch, without touching the batch.  SimpleAgent runs the same search on the device for the one target its
 * decision is about (pom_batch_policy_simple); this call hands out the whole map: a distance plane for a network, "walk to the nearest
 * power-up" composed on top of pom_batch_forecast and pom_batch_move_safety, reward shaping.
 * Semantics: for every env e < n and agent a of agent_mask:
 *          agent a dead in the env's current State (AgentInfo::dead, bboard.hpp:239): both rows [e][a] are all zero.
 *          Otherwise let r be what FillRMap(state, r, a) leaves.
 *          dist[e][a][y][x] (nullable; uint8 [n][4][11][11]) = r.GetDistance(x, y) if that is <= max_dist, else 0.  0 is the source
 *          itself or a cell not reached.  All of the reference's rules hold: the search is breadth-first from the agent's cell, passage
 *          and power-ups are walked through (IS_WALKABLE, bboard.hpp:77-84), a cell showing any agent is reached but not walked
 *          through (strategy.cpp:49-52), bomb, flame, wood and rigid cells block, and the source is never re-entered and keeps 0
 *          (:82-89) — an agent standing on its own bomb starts like any other.
 *          move[e][a][y][x] (nullable; uint8 [n][4][11][11]) = the Move that MoveTowardsPosition(r, {x, y}) returns, for every cell
 *          with dist != 0: 1 UP, 2 DOWN, 3 LEFT, 4 RIGHT — the first step of the path the map's predecessors describe, which is the
 *          lexicographically smallest of the cell's shortest paths under FillRMap's neighbour order DOWN, UP, RIGHT, LEFT.  0 (IDLE)
 *          elsewhere: the reference spins forever when asked for the source or for a cell not reached, so 0 is unambiguous.
 *          With move_dev alone the rule is the same: cells farther than max_dist are 0.
 * Rows:    the rows [e][a] of agents outside agent_mask are not written.  At least one of the two outputs is given.
 * Nothing else changes: after the call nothing this API can read differs from before — records, snapshots and terminal records,
 *          status and the envs' ubflags, POM_CNT_*, episode counters, the handle's tick, agent memory, chain statistics.
 * Ordering: exactly as pom_batch_forecast — chained launches are settled and the sub-streams joined first, then ONE launch on the
 *          handle's stream; the outputs are written in stream order.  Every launch shape of the handle gives the same bytes (the
 *          device buffers are 16-env tiles whatever the shape).
 * POM_E_ARG (with a pom_last_error text naming pom_batch_reach; nothing is written): a null handle or spec, struct_size !=
 *          sizeof(PomReachSpec) (POM_REACH_SPEC_SIZE), agent_mask outside 1 .. 15, max_dist outside 1 .. POM_REACH_MAX_DIST, nonzero
 *          reserved_ or reserved2_, both outputs null, an output not 8-byte aligned.
 * Not here: a range or stream form, fogged reach (a viewer's window), a job list, IsInDanger / SafeDirections planes
 *          (pom_batch_forecast answers the danger question better), the raw predecessor index, a fused step + reach.
 */
enum { POM_REACH_MAX_DIST = 120 }; /* no cell of an 11 x 11 board is farther than 120 steps */
enum { POM_REACH_SPEC_SIZE = 40 }; /* 4 x int32, 2 pointers, int64: no implicit padding on an LP64 target */
typedef struct PomReachSpec {
    int32_t struct_size; /*  0  = sizeof(PomReachSpec) */
    int32_t agent_mask;  /*  4  bit a: agent a's map is computed; 1..15 */
    int32_t max_dist;    /*  8  1..POM_REACH_MAX_DIST: cells farther away are reported as not reached */
    int32_t reserved_;   /* 12  must be 0 */
    uint8_t* dist_dev;   /* 16  nullable: uint8 [n][4][11][11], 8-byte aligned */
    uint8_t* move_dev;   /* 24  nullable: uint8 [n][4][11][11], 8-byte aligned; at least one of the two outputs is given */
    int64_t reserved2_;  /* 32  must be 0 */
} PomReachSpec;
int pom_batch_reach(PomBatch* h, const PomReachSpec* spec);

/*
 * VIEW MEMORY: what each agent saw last, and how long ago.  The fogged views (PomViewSpec) are what an agent sees at one tick; every
 * agent, scripted or learned, merges them into a memory in its next line: keep what was seen, count remembered bombs and flames down,
 * stop believing in an enemy at a cell once it is visibly elsewhere or dead.  This call does that merge for the envs
 * [first, first + count) and the agents of agent_mask in ONE launch on `stream` (NULL: the handle's stream), in place of the view
 * export of a closed loop, not behind it: pom_batch_step_device_range / pom_batch_step_mixed without an observation, then this call on
 * the same stream.  A stated heuristic, as escape_tick is: the reference has no fog and no memory.
 * memory:  uint8 [n][4][6][11][11], caller-owned, sized for the WHOLE batch, 4-byte aligned (an env's four views are 2,904 bytes).  View v
 *          of env e belongs to agent v, alive or dead.  Planes 0..4 hold POM_OBS_CODES bytes (board code, bomb strength, bomb life, bomb
 *          direction, flame life), plane 5 is the AGE: 0 seen this tick, 1..254 ticks since the cell was last seen (saturating), 255 never
 *          seen in this game.  A WIPED view has board 5 (Item::FOG) in every cell, planes 1..4 = 0 and age 255.
 * stamp:   int32 [n][4][2], caller-owned, 8-byte aligned: (episode, timeStep) of the view's last update; episode -1 = no memory yet.
 * THE RULE, per env e of the range and agent v of the mask (other views and their stamp rows are not touched).  ep: the env's episode
 *          counter (pom_batch_episodes), t: its timeStep (env_attrs), (ep0, t0): the stamp.
 *          1 Wipe or age.  If ep0 != ep or t < t0 (a new game; a batch put back to an earlier state) the view is wiped.  Otherwise
 *            dt = min(t - t0, 255), and every cell OUTSIDE the viewer's window — PomViewSpec's: the agent's position as agent_attrs gives
 *            it, a dead agent looks out from where it died — goes through, in this order:
 *            1.1 a cell with age 255 stays as it is;
 *            1.2 a remembered bomb (life byte > 0): life = max(life - dt, 0); at 0 it is forgotten — planes 1..3 become 0, a board byte 3
 *                becomes 0, an agent code standing on it stays.  Remembered bombs do not move;
 *            1.3 a remembered flame (board 4): flame life = max(life - dt, 0); at 0 the board becomes 0;
 *            1.4 a stale agent (board 10 + a): cleared if agent a is dead by the public alive flags or a's present position lies inside
 *                v's window (v sees it elsewhere; the viewer itself is always such an agent) — to board 3 if the cell's bomb life after
 *                1.2 is above 0, else to 0;
 *            1.5 age = min(age + dt, 254).
 *            With dt = 0 none of 1.1 - 1.5 is applied.  Wood, power-ups and walls are kept as remembered.
 *          2 Copy the window.  Every cell INSIDE the window gets the five bytes pom_batch_observe(POM_OBS_CODES) writes for it now,
 *            verbatim, and age 0.
 *          3 Stamp := (ep, t).
 *          So: two calls at one tick equal one; a call every k-th tick ages by k; view_radius 10 gives the unfogged code planes, age 0.
 * What stamps do not catch: pom_batch_copy_envs / pom_batch_expand into a slot, or pom_batch_upload over it, at an equal or later
 *          timeStep of the same episode number — the caller sets those stamp rows to -1.  An env's four views are one call's business:
 *          two calls on the same env at the same time are not supported, whatever their masks.
 * viewer_attrs, env_attrs (nullable): exactly PomViewSpec's, written for the range.
 * Nothing else changes: records, snapshots and terminal records, status and ubflags, POM_CNT_*, episode counters, the handle's tick,
 *          agent memory, chain statistics.
 * Ordering: as pom_batch_step_device_range — whole tiles, quad shape, the handle is settled, nothing is forked or joined, ONE launch
 *          ordered by `stream` alone, no synchronising runtime call once the handle is settled (capturable behind a range step).
 * POM_E_ARG (with a pom_last_error text naming pom_batch_remember_view; nothing is written): a null spec, struct_size !=
 *          sizeof(PomMemorySpec) (POM_MEMORY_SPEC_SIZE), view_radius outside 0..10, agent_mask outside 1..15, nonzero reserved_, a null
 *          memory_dev or stamp_dev, memory_dev not 4-byte or stamp_dev not 8-byte aligned, attribute pointers not 16-byte aligned,
 *          whatever pom_batch_step_device_range refuses of a range or a handle.
 * Not here: the merge fused into the step kernels, other element types than the code bytes, remembered bombs that move.
 */
enum { POM_MEMORY_PLANES = 6, POM_MEMORY_AGE_NEVER = 255, POM_MEMORY_AGE_MAX = 254, POM_MEMORY_SPEC_SIZE = 48 };
typedef struct PomMemorySpec {
    int32_t struct_size;       /*  0  = sizeof(PomMemorySpec) */
    int32_t view_radius;       /*  4  0..POM_VIEW_RADIUS_MAX, Chebyshev */
    int32_t agent_mask;        /*  8  bit v: agent v's memory is updated; 1..15 */
    int32_t reserved_;         /* 12  must be 0 */
    uint8_t* memory_dev;       /* 16  uint8 [n][4][POM_MEMORY_PLANES][11][11] */
    int32_t* stamp_dev;        /* 24  int32 [n][4][2] */
    int32_t* viewer_attrs_dev; /* 32  nullable: int32 [n][4][POM_OBS_VIEWER_ATTRS] */
    int32_t* env_attrs_dev;    /* 40  nullable: as pom_batch_observe */
} PomMemorySpec;
int pom_batch_remember_view(PomBatch* h, int64_t first, int64_t count, const PomMemorySpec* spec, void* stream);

/* A stand-in for a learned policy in measurements and tests of the closed loop (NOT part of the stepper): one launch on `stream`
 * that writes Move[4] of the envs [first, first + count) into moves_dev (int32 [n][4]).  codes_dev != NULL: the POM_OBS_CODES
 * observation of the batch (uint8 [n][5][11][11]) — every byte of the range's observations is read and the moves depend on them;
 * NULL: the moves depend on (env, agent, tick) only.  The same function of its inputs on every call: tests recompute it. */
int pom_bench_policy(const uint8_t* codes_dev, int32_t* moves_dev, int64_t first, int64_t count, uint32_t tick, void* stream);

/* bboard::Step (include/bboard.hpp:668, src/bboard/step.cpp:9-284) for a single host State on the GPU (device 0): the literal
 * drop-in.  One launch per call: the kernel reads the State and Move[4] from a pinned page, plays the tick and writes the State
 * back; the call returns when that is done (about ten microseconds — the launch and the trip over PCIe, not the tick).
 * Re-entrant over distinct States like the reference's Step (performance_test.cpp:71-94 steps one env per std::thread): every
 * calling thread gets a pinned page and a stream of its own (up to 64 threads; more share), so threads stepping their own
 * States do not wait for each other.  Code that steps many States should still hand them to one PomBatch
 * (pom_batch_upload / pom_batch_step): a launch per State is latency, not throughput.
 * POM_E_UNREPRESENTABLE: the State holds a value the device record cannot hold, or one that ticks could push out of it (the upload
 * bounds of pom_packed.h: bombCount -108..107, maxBombCount <= 32646, bombStrength 0..134, aliveAgents >= -124); it is left as it is. */
int pom_step(void* state_1004, const int32_t moves[4]);

/* The same with Environment::Step's bookkeeping after the tick (src/bboard/environment.cpp:148-168): timeStep++, then
 * done / winner (-1 = none) / draw as pom_batch_status reports them, judged on this tick alone; max_steps > 0 also ends the
 * game at that timeStep.  The caller decides whether a game is stepped at all (the reference returns early from a finished
 * one, environment.cpp:125).  Outputs may be NULL.  ubflags: the POM_UB_* of this tick. */
int pom_env_step(void* state_1004, const int32_t moves[4], int32_t max_steps, int32_t* done, int32_t* winner, int32_t* draw,
                 uint32_t* ubflags);

#ifdef __cplusplus
}
#endif
#endif /* POM_BATCH_H_ */
