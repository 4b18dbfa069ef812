/*
 * pom_emul_probe.h — TEST-ONLY counters of the two host builds of the device tick (pom_emul.cpp, pom_emul_quad.cpp): what one
 * tick did to the resources that the envs of a wavefront share on the device.  Everything is counted at the store interface
 * (set_frame, claim, claims, claims_clear, set_cell, set_bomb); pom_step_body.h knows nothing of it.  tests/test_tile_mates.py
 * reads them to prove that its actors reach what they are written for.
 *
 *   frames      set_frame(d, v): the deepest d, a mask of every d written, the last value written to each d
 *   frame0_rem  the `rem` field of the value written to frame 0: 62 (REM_TOP) if the chain was started by TickBombs, a queue
 *               offset (< 20) if a blast inside loop B started it (which is one of the two ways `unforeseen_` is raised)
 *   claims      claim() calls; claims_clear() called = loop_b_todo ran; claims(c) is read once per queued bomb, in queue
 *               order (per lane: offsets sub, sub + G, ...): bit k of todo_claimed = "bomb k's cell is claimed twice", the part of
 *               loop_b_todo's result that depends on the counters
 *   hops        AgentBombChainReversion called from loop B (bomb_collision, the other way `unforeseen_` is raised): a chain starts
 *               with an agent item written right after a bomb word, every further agent item is one more hop (the second write
 *               of "bounced back onto a resting bomb" repeats the cell and is not counted)
 *   claims_cap  fault injection for the CPU tests only: claims() answers min(count, cap) — "the counter byte read 0 or 1" —,
 *   claims_add  plus claims_add — "somebody else's counts landed in this map too"
 */
#ifndef POM_EMUL_PROBE_H_
#define POM_EMUL_PROBE_H_

#include <cstdint>
#include <cstring>

#include "pom_packed.h"
#include "pom_step_body.h"

enum { POM_PROBE_WORDS = 8 + POM_STACK_DEPTH };

struct PomEmulProbe {
    int max_frame, n_claim, todo_ran, frame0_rem, hops_max;
    uint32_t frame_mask, todo_claimed;
    uint32_t frames[POM_STACK_DEPTH];
    int claims_cap = 0x7FFFFFFF, claims_add = 0;
    /* bookkeeping of the derivations */
    int reads[4], hops_cur, last_write, last_agent_cell, last_agent_val;
    enum { W_OTHER = 0, W_BOMB, W_AGENT };

    void reset()
    {
        max_frame = -1;
        frame0_rem = -1;
        n_claim = todo_ran = hops_max = hops_cur = 0;
        frame_mask = todo_claimed = 0;
        std::memset(frames, 0, sizeof frames);
        std::memset(reads, 0, sizeof reads);
        last_write = W_OTHER;
        last_agent_cell = last_agent_val = -1;
    }
    void on_frame(int d, int v)
    {
        if (d > max_frame) max_frame = d;
        frame_mask |= 1u << d;
        frames[d] = (uint32_t)v;
        if (d == 0) frame0_rem = (v >> 19) & 63;
        last_write = W_OTHER;
    }
    void on_claim() { __atomic_fetch_add(&n_claim, 1, __ATOMIC_RELAXED); }
    void on_clear() { todo_ran = 1; }
    int on_claims_read(int sub, int g, int count)
    {
        const int k = sub + g * reads[sub]++;
        const int v = (count < claims_cap ? count : claims_cap) + claims_add;
        if (v >= 2 && k < 32) __atomic_fetch_or(&todo_claimed, 1u << k, __ATOMIC_RELAXED);
        return v;
    }
    void on_bomb() { last_write = W_BOMB; }
    void on_cell(int c, int v)
    {
        const int agent = v >= POM_C_AGENT && v < POM_C_AGENT + 4;
        if (agent && todo_ran) {
            if (last_write == W_BOMB) hops_cur = 1;
            else if (!(last_write == W_AGENT && c == last_agent_cell && v == last_agent_val)) hops_cur++;
            if (hops_cur > hops_max) hops_max = hops_cur;
            last_agent_cell = c;
            last_agent_val = v;
        }
        last_write = agent ? W_AGENT : W_OTHER;
    }
    void get(int32_t* out) const
    {
        out[0] = max_frame; out[1] = (int32_t)frame_mask; out[2] = n_claim; out[3] = todo_ran; out[4] = (int32_t)todo_claimed;
        out[5] = frame0_rem; out[6] = hops_max; out[7] = 0;
        for (int d = 0; d < POM_STACK_DEPTH; d++) out[8 + d] = (int32_t)frames[d];
    }
};

extern PomEmulProbe g_pom_probe; /* pom_emul.cpp; one tick at a time (the tests are single-threaded) */

#endif
