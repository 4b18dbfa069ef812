/*
 * pom_chain_visit.h — the device side of the chained launches' hand-off (pom_chain.h is the host side and says what the scheme
 * relies on): a wavefront's visit of a tile — take a ticket, wait for the visit before it, hand the tile on.  Used by the CHAIN
 * instantiations of pom_step_kernel and by the hand-off litmus (pom_chain_litmus_kernel), both in pom_kernels.h.
 */
#ifndef POM_CHAIN_VISIT_H_
#define POM_CHAIN_VISIT_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pom_packed.h"

/* how long a wavefront waits for the visit before its own before it gives up (it must never hang the device): wall-clock time, so
 * that a holder descheduled for a while (several processes time-slicing one GPU, a debugger) is waited for; a give-up poisons the
 * tile and the host replays its ticks after the next join — slow, never wrong (pom_chain_host.h chain_settle) */
enum { POM_CHAIN_WAIT_LIMIT_US = 2000000 };
#ifndef POM_CHAIN_WORD_STRIDE
#define POM_CHAIN_WORD_STRIDE 16 /* 64-bit words between the ticket words of neighbouring tiles: a 128-byte line each (10.28 - 10.30 us
                                    per step against 10.41 - 10.48 with the words packed: atomics of neighbouring tiles do not queue on one line) */
#endif

struct PomChainVisit {
    int32_t dist = 0;            /* how many visits after the launch's chain_seq0 this one is: picks the tick (and the tape's tick) */
    unsigned long long done = 0; /* what the wavefront adds to the tile's word when its stores have arrived */
#if defined(POM_CHAIN_DIAG)
    long long t0 = 0, t1 = 0, t2 = 0, rt0 = 0;
    int polls = 0;
    uint32_t visit = 0;
#endif
};
/* which XCD this workgroup runs on (0..7; >= 8: not the machine this was written for) */
__device__ __forceinline__ uint32_t pom_chain_xcd()
{
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return x & 0xFu;
}
/* The address of an atomic that ONE lane issues (its caller stands behind `if (lane == 0)`).  The compiler cannot see that: it wraps
 * every atomic add on a wave-uniform address in its wave-reduction form — count the active lanes, a second exec bracket, a multiply; a
 * scalar loop over the active lanes where the value is not uniform; a multiply-add to hand every lane its own old value.  An address
 * that has been through a vector register counts as lane-varying and is left alone: the same vector atomic of the same order and scope,
 * issued by the one lane, without the scaffolding (profiles/queue_first_trip_ab.txt). */
template <bool ONE_LANE, class T>
__device__ __forceinline__ auto pom_one_lane_address(T* p)
{
    if constexpr (ONE_LANE) {
        /* (named a global address: behind the asm the compiler no longer sees where the pointer came from, and would issue a flat atomic) */
        auto g = (__attribute__((address_space(1))) T*)p;
        asm("" : "+v"(g));
        return g;
    } else {
        return p;
    }
}
/* Take a ticket for the tile's word and wait for the visit before it.  true: the tile is this wavefront's to play — its record, as
 * the previous visit stored it, may be loaded NOW (past the vector cache: sc1).  false: nothing may be touched (the tile is, or
 * has just been, poisoned; the flag word says why). */
template <bool ONE_LANE = false> /* the step kernels: the ticket as a plain one-lane atomic (pom_one_lane_address) */
__device__ __forceinline__ bool pom_chain_enter(unsigned long long* word, uint32_t chain_xcd, uint32_t chain_seq0, uint32_t tape_len, uint64_t wait_limit,
                                                uint32_t* err, int lane, PomChainVisit& v)
{
    const uint32_t xcd = chain_xcd + 1u;
#if defined(POM_CHAIN_DIAG)
    v.t0 = (long long)__builtin_readcyclecounter();
    v.rt0 = (long long)wall_clock64();
#endif
    /* take a ticket: the old value says which visit of the tile this is — and, mostly, that the visit before it is stored */
    unsigned long long w = 0;
    if (lane == 0) w = __hip_atomic_fetch_add(pom_one_lane_address<ONE_LANE>(word), 1ull << POM_CHAIN_TICKET_SHIFT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    w = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(w >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w);
    const uint32_t visit = (uint32_t)(w >> POM_CHAIN_TICKET_SHIFT);
    /* which tick: the call's first tick + how far this visit is from the call's first visit — a signed distance: launches of
     * two calls may be in flight together, and a wavefront of the later call can draw a ticket of the earlier one */
    v.dist = (int32_t)pom_chain_visit_distance(visit, chain_seq0);
#if defined(POM_CHAIN_DIAG)
    v.t1 = (long long)__builtin_readcyclecounter();
#endif
    /* stored visits == this visit's number: its turn.  Until then poll — for as long as the wall clock allows; a poisoned tile
     * (somebody before this visit could not play) is nobody's turn any more */
    int polls = 0;
    bool timed_out = false;
    if (!((uint32_t)w & POM_CHAIN_POISON) && (int32_t)pom_chain_visit_distance((uint32_t)w & POM_CHAIN_COUNT_MASK, visit) < 0) { /* wave-uniform */
        const uint64_t t_wait0 = wall_clock64();
        for (;;) {
            __builtin_amdgcn_s_sleep(1);
            w = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            w = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(w >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w);
            polls++;
            if (((uint32_t)w & POM_CHAIN_POISON) || (int32_t)pom_chain_visit_distance((uint32_t)w & POM_CHAIN_COUNT_MASK, visit) >= 0) break;
            if (wall_clock64() - t_wait0 >= wait_limit) {
                timed_out = true;
                break;
            }
        }
    }
    (void)polls;
    const uint32_t was_on = (uint32_t)(w >> 32) & 0xFu;
    const bool poisoned = ((uint32_t)w & POM_CHAIN_POISON) != 0;
    const bool wrong_xcd = was_on != 0u && was_on != xcd;
    const bool off_tape = tape_len != 0u && (uint32_t)v.dist >= tape_len;
    if (poisoned || timed_out || wrong_xcd || off_tape) {
        /* The visit before this one never arrived in time, or it was stored through another XCD's L2 (what this L2 holds of
         * the tile may be stale), or the ticket lies outside the move tape (launches of two tape calls in flight together:
         * the host joins between them, so never).  Nothing is stepped and NOTHING IS COUNTED: the tile is poisoned, every
         * later visitor leaves it alone, its stored count stays at the ticks it really played, and the host — which finds
         * the flag after the next join — replays the rest with ordinary launches (chain_settle, pom_chain_host.h). */
        if (lane == 0 && !poisoned) {
            __hip_atomic_fetch_or(word, (unsigned long long)POM_CHAIN_POISON, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_or(err, (uint32_t)(timed_out ? POM_CHAIN_E_TIMEOUT : wrong_xcd ? POM_CHAIN_E_XCD : POM_CHAIN_E_TAPE), __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
        }
        return false;
    }
#if defined(POM_CHAIN_DIAG)
    v.t2 = (long long)__builtin_readcyclecounter();
    v.polls = polls;
    v.visit = visit;
#endif
    v.done = 1ull + ((unsigned long long)(xcd - was_on) << 32);
    return true;
}
/* Hand the tile on: called after the record's stores have been ISSUED; waits until the L2 has acknowledged them, then counts the
 * visit as stored (which is what the next visitor polls for). */
template <bool ONE_LANE = false>
__device__ __forceinline__ void pom_chain_leave(unsigned long long* word, int lane, const PomChainVisit& v)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_fetch_add(pom_one_lane_address<ONE_LANE>(word), v.done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#endif /* POM_CHAIN_VISIT_H_ */
