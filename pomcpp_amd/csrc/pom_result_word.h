/*
 * pom_result_word.h — the POM_RO_* result word (pom_batch.h) of one env, for every kernel that reports one: the rollouts and expand
 * (pom_rollout.h, pom_expand.h) and the stepping call's outcome (pom_step_events.h).
 */
#ifndef POM_RESULT_WORD_H_
#define POM_RESULT_WORD_H_

#include "pom_device.h"

static_assert(POM_RO_DONE == (POM_ST_DONE << 4) && POM_RO_DRAW == (POM_ST_DRAW << 4) && POM_RO_TIMEOUT == (POM_ST_TIMEOUT << 1),
              "the status byte's bits move into the result word by shifts");

/* The result word (pom_batch.h POM_RO_*) of the env whose lane this is: who is alive, how the status byte says the game stands, whether
 * a played tick raised a flag, and the ticks played.  The owner lane of an env stores it. */
__device__ __forceinline__ uint32_t pom_rollout_word(const PomLane& L, uint32_t status, bool ub, uint32_t length)
{
    uint32_t alive = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) alive |= (uint32_t)(ag_dead(L.a0[i]) ^ 1) << i;
    return alive | ((status & (POM_ST_DONE | POM_ST_DRAW)) << 4) | ((status & POM_ST_TIMEOUT) << 1) | (ub ? (uint32_t)POM_RO_UB : 0u) |
           (((status >> POM_ST_WINNER_SHIFT) & 7u) << POM_RO_WINNER_SHIFT) | (length << POM_RO_LENGTH_SHIFT);
}

#endif /* POM_RESULT_WORD_H_ */
