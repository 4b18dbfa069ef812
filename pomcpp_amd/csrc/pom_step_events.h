/*
 * pom_step_events.h — what pom_batch_step_events adds to the mixed step's kernel (pom_step_mixed.h, EVENTS): the event word of one
 * agent, the wood scan of a tile's boards, and where the three arrays go.  The rule is pom_batch.h's (PomStepEventsSpec): a pure
 * function of S0 (the env's state when its tick begins), m (the moves handed to the tick) and S1 (what the tick and pom_env_epilogue
 * leave, before a restart at the end).  Lane m of a quad is agent m and keeps three registers of S0 through the tick: its two agent
 * words and, only when the wood count is asked for, the wood bits of its share of the tile's boards.
 */
#ifndef POM_STEP_EVENTS_H_
#define POM_STEP_EVENTS_H_

#include "pom_device.h"
#include "pom_result_word.h"

struct StepEventsOut {
    uint32_t* events;  /* uint32 [n][4]: word tile * 64 + lane, the index the moves are read at */
    uint32_t* outcome; /* nullable: uint32 [n] */
    uint8_t* wood;     /* nullable: uint8 [n] */
};

static_assert(POM_EV_WON == POM_EV_END << 1 && POM_EV_DRAW == POM_EV_END << 2 && POM_EV_TIMEOUT == POM_EV_END << 3, "the END group is four adjacent bits");

/* events[e][a] of an env that played a tick: a0 / a1 are agent a's two words (pom_packed.h) in S0 and S1, `move` is m[a] as
 * clamp_move leaves it, `status` is S1's status byte */
__device__ __forceinline__ uint32_t pom_event_word(int a0_s0, int a1_s0, int a0_s1, int a1_s1, int move, int member, bool restarted,
                                                   bool newly_done, uint32_t status, bool ub)
{
    const int alive0 = ag_dead(a0_s0) ^ 1, alive1 = ag_dead(a0_s1) ^ 1;
    /* PlantBombModifiedLife's one test (bboard.cpp:127), asked of the agents step.cpp:48-55 lets through */
    const int laid = alive0 & (int)(move == POM_MOVE_BOMB) & (int)(ag_bombcount(a0_s0) < ag_max_bombs(a1_s0));
    int exploded = ag_bombcount(a0_s0) + laid - ag_bombcount(a0_s1);
    exploded = exploded < 0 ? 0 : exploded > 15 ? 15 : exploded;
    uint32_t w = (uint32_t)move | POM_EV_PLAYED | (alive1 ? (uint32_t)POM_EV_ALIVE : 0u);
    w |= (alive0 & (alive1 ^ 1)) ? (uint32_t)POM_EV_DIED : 0u;
    w |= (alive0 & (int)(ag_pos(a0_s0) != ag_pos(a0_s1))) ? (uint32_t)POM_EV_MOVED : 0u;
    w |= laid ? (uint32_t)POM_EV_LAID : 0u;
    w |= ag_max_bombs(a1_s1) > ag_max_bombs(a1_s0) ? (uint32_t)POM_EV_GAIN_BOMB : 0u;
    w |= ag_strength(a1_s1) > ag_strength(a1_s0) ? (uint32_t)POM_EV_GAIN_RANGE : 0u;
    w |= (ag_kick(a0_s1) & (ag_kick(a0_s0) ^ 1)) ? (uint32_t)POM_EV_GAIN_KICK : 0u;
    w |= restarted ? (uint32_t)POM_EV_RESTARTED : 0u;
    w |= (uint32_t)exploded << POM_EV_EXPLODED_SHIFT;
    if (newly_done) {
        w |= POM_EV_END;
        w |= (int)((status >> POM_ST_WINNER_SHIFT) & 7u) == member + 1 ? (uint32_t)POM_EV_WON : 0u;
        w |= (status & POM_ST_DRAW) ? (uint32_t)POM_EV_DRAW : 0u;
        w |= (status & POM_ST_TIMEOUT) ? (uint32_t)POM_EV_TIMEOUT : 0u;
    }
    w |= ub ? (uint32_t)POM_EV_UB : 0u;
    return w;
}

/* The wood cells of the tile's sixteen boards, as bits.  The board is laid out by cell (pom_packed.h): cell c of column ec is byte
 * c * 16 + ec, so dword c * 4 + g holds cell c of the four envs 4g .. 4g + 3.  The sixteen lanes whose envs those are (a DPP row)
 * share their 124 dwords: lane li of the row takes cells li, 16 + li, .. 112 + li — 64 consecutive dwords per read over the
 * wavefront, no bank conflict — and tests four bytes at a time.  Byte j of the result: bit k = cell 16 k + li of env 4g + j is wood. */
__device__ __forceinline__ uint32_t pom_wood_bits(const uint32_t* tile, int lane)
{
    const int g = lane >> 4, li = lane & 15;
    uint32_t acc = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int c = k * 16 + li;
        const uint32_t x = tile[(k == 7 && c > 123 ? 123 : c) * 4 + g];
        /* a byte is wood when it is 6..10 (POM_C_WOOD + flag): bit 7 of low + 122 says >= 6, of low + 117 says >= 11, and no sum
         * carries into the next byte; a code with bit 7 set is a flame */
        const uint32_t low = x & 0x7F7F7F7Fu;
        uint32_t w = ((low + 0x7A7A7A7Au) ^ (low + 0x75757575u)) & ~x & 0x80808080u;
        if (k == 7) w = c > 120 ? 0u : w; /* (cells 121..123 are padding, and 124.. is not the board) */
        acc |= w >> (7 - k);
    }
    return acc;
}
static_assert(POM_C_WOOD == 6 && POM_C_AGENT == 11, "pom_wood_bits tests for 6..10");

/* wood[e]: the cells that were wood in `before` and are not in `after` (both pom_wood_bits), counted per env and summed over the row's
 * sixteen lanes; at most 121, so the saturation at 255 that the header states is never reached */
__device__ __forceinline__ uint32_t pom_wood_burnt(uint32_t before, uint32_t after, int ec)
{
    uint32_t b = before & ~after;
    b = b - ((b >> 1) & 0x55555555u);
    b = (b & 0x33333333u) + ((b >> 2) & 0x33333333u);
    b = (b + (b >> 4)) & 0x0F0F0F0Fu; /* a count of 0..8 per byte */
    b += (uint32_t)pom_dpp_x1((int)b);
    b += (uint32_t)pom_dpp_x2((int)b);
    b += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0x124, 0xF, 0xF, true); /* row_ror:4 */
    b += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0x128, 0xF, 0xF, true); /* row_ror:8 */
    return (b >> (8 * (ec & 3))) & 0xFFu;
}

#endif /* POM_STEP_EVENTS_H_ */
