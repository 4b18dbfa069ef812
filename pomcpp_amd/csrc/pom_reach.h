/*
 * pom_reach.h — pom_batch_reach's kernel (include/pom_batch.h PomReachSpec): the reference's reachability map of every asked agent of
 * every env — strategy::FillRMap's distances and, per reached cell, the Move that MoveTowardsPosition makes of its predecessors
 * (src/bboard/strategy.cpp:58-120) — in ONE launch, the batch untouched.
 *
 * The map is not searched cell by cell.  It is the policy's flood (pom_policy_body.h: 121-bit cell sets spread over a quad, one
 * 32-cell word per lane, pom_quad_neighbours) run forwards and level-synchronously from the agent's cell, with two things kept that
 * the policy throws away:
 *   - the level at which a cell joins is its distance.  The level is the same number in every lane of the wavefront (all floods start
 *     together), so it is not counted per cell: its seven bits are OR-ed, under the mask of the cells that joined, into seven bit planes
 *     (pom_reach_stamp), and the planes are turned into a byte per cell once, after the flood (pom_reach_cells4);
 *   - the first move.  FillRMap is a FIFO search that tries a cell's neighbours in the order DOWN, UP, RIGHT, LEFT (strategy.cpp:82-89),
 *     which gives every cell the lexicographically smallest of its shortest paths (the argument of pom_policy_body.h's header); its
 *     first step is the first of the source's neighbours ("gates"), in that order, that lies on SOME shortest path to the cell.  A
 *     labelled flood gives exactly that: four fronts, one per gate, and a cell that several fronts reach in the same level goes to the
 *     first of them (pom_reach_join4).  By induction over the level a cell's label is the smallest gate over all its shortest paths.
 * Cells that show an agent join (they get a distance and a move) but enter no front: the search does not continue through them
 * (strategy.cpp:49-52).  The source is never re-entered (:82-89) and keeps 0.
 *
 * The level functions are POM_HD templates over the quad abstraction Q of pom_policy_body.h, the flood's loop included
 * (pom_reach_flood; what differs between the device and the host is only "does any flood of the wavefront still grow"), so that the
 * same source is checked on the host against the compiled reference's maps (tests/emul/pom_reach_emul.cpp, tests/test_reach_host.py).
 *
 * Work split: the grid of pom_move_safety.h — one wavefront per (tile of 16 envs, asked agent), workgroup b = v * tiles8 + slot, all
 * variants of a tile on one XCD.  Quad q of the wavefront runs the flood of (env q of the tile, the variant's agent).
 * LDS: the tile's first 40 rows (board, timeStep, agents: 2,560 B), and two staging areas of 16 rows x 128 bytes for the outputs, from
 * which the rows leave in 64-byte runs of consecutive addresses.  No scratch memory.
 */
#ifndef POM_REACH_H_
#define POM_REACH_H_

#include "pom_policy_body.h"

enum { POM_REACH_PLANES = 7 }; /* POM_REACH_MAX_DIST = 120 < 2^7 */

/* ---- the level functions, for the device and for the host (tests/emul/pom_reach_emul.cpp) ---- */

/* Word m (cells 32m .. 32m+31) of the walkable set and of the agent set: pom_policy_prepare_fill's classification and gathering
 * (pom_policy_body.h), into registers.  P: uint32_t cells4(int k), the codes of cells 4k .. 4k+3, a byte each; k up to 31 must be
 * readable (what lies past cell 120 is masked here). */
template <class P>
POM_HD void pom_reach_sets_word(const P& p, int m, uint32_t& walk, uint32_t& agents)
{
    uint32_t w = 0, g = 0;
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        uint32_t w0, g0, w1, g1;
        pom_cells_walk_agent(p.cells4(8 * m + i), w0, g0);
        pom_cells_walk_agent(p.cells4(8 * m + i + 1), w1, g1);
        w |= pom_gather_flags(w1, pom_gather_flags(w0, 0u, 0), 1) << (4 * i);
        g |= pom_gather_flags(g1, pom_gather_flags(g0, 0u, 0), 1) << (4 * i);
    }
    const uint32_t keep = m == 3 ? 0x01FFFFFFu : ~0u; /* 121 = 96 + 25 */
    walk = w & keep;
    agents = g & keep;
}

/* the four neighbour sets of w one by one, in FillRMap's order: nb[0] DOWN (y + 1), nb[1] UP (y - 1), nb[2] RIGHT (x + 1, not across
 * the right edge), nb[3] LEFT (x - 1, not across the left edge) — the four terms of pom_quad_neighbours.  Bits past cell 120 are not
 * masked here: every use cuts to a set of cells. */
template <class Q>
POM_HD void pom_quad_neighbours4(const Q& q, typename Q::W w, typename Q::W (&nb)[4])
{
    const typename Q::W p = q.prev(w), n = q.next(w);
    nb[0] = (w << 11) | (p >> 21);
    nb[1] = (w >> 11) | (n << 21);
    nb[2] = ((w << 1) | (p >> 31)) & ~q.col0();
    nb[3] = ((w >> 1) | (n << 31)) & ~q.col10();
}

/* the cells that joined in level `level` get its bits: plane[i] holds bit i of every cell's distance */
template <class W>
POM_HD void pom_reach_stamp(W (&plane)[POM_REACH_PLANES], W joined, int level)
{
#pragma unroll
    for (int i = 0; i < POM_REACH_PLANES; i++)
        if ((level >> i) & 1) plane[i] = plane[i] | joined;
}

/* One level without labels.  enter: the cells a search may set foot on (walkable or showing an agent), walk: those it goes on from;
 * neither holds the source.  Returns the cells that joined. */
template <class Q>
POM_HD typename Q::W pom_reach_level(const Q& q, typename Q::W walk, typename Q::W enter, typename Q::W& front, typename Q::W& all)
{
    const typename Q::W joined = pom_quad_neighbours(q, front) & ~all & enter;
    all = all | joined;
    front = joined & walk;
    return joined;
}

/* A value the device compiler must take as it is.  Without it hipcc -Os --offload-arch=gfx950 (profiles/reach_kernel_resources.txt names the compiler) folds the four and-not steps of
 * pom_reach_join4 below — `open & ~(nb & open)` reaches instruction selection as `(nb & open) ^ open`, nested four deep — into
 * v_bitop3_b32 instructions whose truth tables are not the expressions': the third and fourth step (and `joined`) forget what the
 * first front took, read off the disassembly and seen on the GPU as DOWN gates that joined twice.  With an opaque `open` between the
 * steps every step is the two-input and-not it looks like.  Nothing on the host. */
template <class W>
POM_HD void pom_reach_opaque(W& w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(w));
#else
    (void)w;
#endif
}

/* One level of the labelled flood, from the neighbour sets nb[k] of the four fronts: a cell goes to the first front, in the order
 * DOWN, UP, RIGHT, LEFT, that reaches it.  lab[k]: all cells of label k so far.  Returns the cells that joined. */
template <class Q>
POM_HD typename Q::W pom_reach_join4(const Q&, const typename Q::W (&nb)[4], typename Q::W walk, typename Q::W enter,
                                     typename Q::W (&front)[4], typename Q::W (&lab)[4], typename Q::W& all)
{
    typename Q::W open = enter & ~all;
    const typename Q::W before = open;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const typename Q::W j = nb[k] & open;
        open = open & ~j;
        pom_reach_opaque(open);
        lab[k] = lab[k] | j;
        front[k] = j & walk;
    }
    const typename Q::W joined = before & ~open;
    all = all | joined;
    return joined;
}
template <class Q>
POM_HD typename Q::W pom_reach_level4(const Q& q, typename Q::W walk, typename Q::W enter, typename Q::W (&front)[4],
                                      typename Q::W (&lab)[4], typename Q::W& all)
{
    typename Q::W nb[4];
#pragma unroll
    for (int k = 0; k < 4; k++) nb[k] = pom_quad_neighbours(q, front[k]);
    return pom_reach_join4(q, nb, walk, enter, front, lab, all);
}

/* The whole flood from the cell set `src` ({the agent's cell}; {} for a dead agent: nothing is reached) for at most max_dist levels.
 * DIST: dist[i] = bit i of the distance of every reached cell.  MOVE: the labelled flood, mv[i] = bit i of the Move of every reached
 * cell; without it ONE front does.  more(w): does the flood — on the device any flood of the wavefront — still have a front. */
template <bool MOVE, bool DIST, class Q, class More>
POM_HD void pom_reach_flood(const Q& q, typename Q::W src, typename Q::W walk, typename Q::W agents, int max_dist,
                            typename Q::W (&dist)[POM_REACH_PLANES], typename Q::W (&mv)[3], const More& more)
{
    typedef typename Q::W W;
    const W none = src & ~src;
    walk = walk & ~src; /* FillRMap never re-enters its source */
    const W enter = (walk | agents) & ~src;
    W all = none;
#pragma unroll
    for (int i = 0; i < POM_REACH_PLANES; i++) dist[i] = none;
    mv[0] = mv[1] = mv[2] = none;
    if (MOVE) {
        W nb[4], front[4], lab[4] = {none, none, none, none};
        pom_quad_neighbours4(q, src, nb); /* the gates */
        W joined = pom_reach_join4(q, nb, walk, enter, front, lab, all);
        if (DIST) pom_reach_stamp(dist, joined, 1);
        POM_NOUNROLL
        for (int level = 2; level <= max_dist && more(front[0] | front[1] | front[2] | front[3]); level++) {
            joined = pom_reach_level4(q, walk, enter, front, lab, all);
            if (DIST) pom_reach_stamp(dist, joined, level);
        }
        static_assert(POM_MOVE_UP == 1 && POM_MOVE_DOWN == 2 && POM_MOVE_LEFT == 3 && POM_MOVE_RIGHT == 4, "the labels' Moves, bit by bit");
        mv[0] = lab[1] | lab[3];
        mv[1] = lab[0] | lab[3];
        mv[2] = lab[2];
    } else {
        W front = src;
        POM_NOUNROLL
        for (int level = 1; level <= max_dist && more(front); level++) pom_reach_stamp(dist, pom_reach_level(q, walk, enter, front, all), level);
    }
}

/* bit planes -> bytes: the values of cells 4j .. 4j+3 of a 32-cell word (j = 0..7), a byte each, from N planes of that word.  Four
 * bits b0..b3 times 0x00204081 put b_k at bit 8k (the four shifted copies occupy disjoint bits: no carry). */
template <int N>
POM_HD uint32_t pom_reach_cells4(const uint32_t (&plane)[N], int j)
{
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < N; i++) r |= ((((plane[i] >> (4 * j)) & 0xFu) * 0x00204081u) & 0x01010101u) << i;
    return r;
}

#if defined(__HIPCC__) /* ---- the kernel ---- */

#include "pom_device.h"
#include "pom_policy_wave.h"

struct ReachParams {
    const uint32_t* state;
    uint8_t* dist; /* nullable: uint8 [n][4][121] */
    uint8_t* move; /* nullable: uint8 [n][4][121]; one of the two is given */
    int64_t n;
    int32_t agent_mask; /* 1 .. 15 */
    int32_t max_dist;   /* 1 .. POM_REACH_MAX_DIST */
    uint32_t tiles, tiles8; /* tiles of 16 envs; the same rounded up to a multiple of 8: the grid is variants * tiles8 */
};

enum { POM_REACH_ROWS = POM_REC_AGENTS + 8, POM_REACH_STAGE_DWORDS = 16 * 32 }; /* the rows loaded; a staging area: 16 rows of 128 bytes */
static_assert(POM_REACH_MAX_DIST < (1 << POM_REACH_PLANES), "a distance fits the planes");
static_assert(POM_REACH_ROWS * 16 * 4 >= 64 * 31 + 48 + 16, "cells4(31) reads inside the rows loaded");

/* the board of the quad's env as pom_reach_sets_word reads it: cell c at byte c * 16 of the env's column (pom_packed.h) */
struct ReachCells {
    const uint8_t* b;
    __device__ uint32_t cells4(int k) const
    {
        const uint8_t* q = b + 64 * k;
        return (uint32_t)q[0] | ((uint32_t)q[16] << 8) | ((uint32_t)q[32] << 16) | ((uint32_t)q[48] << 24);
    }
};
/* the wavefront runs its 16 floods in lock-step for as many levels as the longest of them */
struct ReachWaveMore {
    __device__ bool operator()(uint32_t front) const { return __ballot(front != 0u) != 0; }
};

/* this lane's 32 cells of N planes as bytes into its quad's staging row: bytes 32 k .. 32 k + 31 of the row */
template <int N>
__device__ __forceinline__ void pom_reach_stage(uint32_t* row, int k, const uint32_t (&plane)[N])
{
    uint4* at = reinterpret_cast<uint4*>(row + 8 * k);
    at[0] = make_uint4(pom_reach_cells4(plane, 0), pom_reach_cells4(plane, 1), pom_reach_cells4(plane, 2), pom_reach_cells4(plane, 3));
    at[1] = make_uint4(pom_reach_cells4(plane, 4), pom_reach_cells4(plane, 5), pom_reach_cells4(plane, 6), pom_reach_cells4(plane, 7));
}
/* the 16 staged rows to out[e][agent][0..120], e = e0 + row: every instruction writes half a row, 64 (57) consecutive bytes */
__device__ __forceinline__ void pom_reach_store(uint8_t* out, const uint32_t* stage, int64_t e0, int64_t n, int agent, int lane)
{
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(stage);
#pragma unroll 4
    for (int i = 0; i < 32; i++) {
        const int row = i >> 1, byte = (i & 1) * 64 + lane; /* row: wave-uniform */
        if (e0 + row < n && byte < POM_CELLS) out[((e0 + row) * 4 + agent) * POM_CELLS + byte] = sb[row * 128 + byte];
    }
}

template <bool MOVE, bool DIST>
__global__ __launch_bounds__(64) void pom_reach_kernel(ReachParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POM_REACH_ROWS * 16];
    __shared__ __attribute__((aligned(16))) uint32_t stage[(MOVE && DIST ? 2 : 1) * POM_REACH_STAGE_DWORDS];
    const int lane = threadIdx.x;
    const uint32_t variant = blockIdx.x / p.tiles8, slot = blockIdx.x - variant * p.tiles8;
    if (slot >= p.tiles) return; /* a workgroup of the padding */
    const int64_t tile_id = pom_xcd_tile_order(slot, p.tiles);
    /* the HBM layout is 16-env tiles whatever the handle's launch shape; the buffers hold n_pad columns, so a last, short tile is
     * loaded whole */
    load_tile16_x4<POM_REACH_ROWS>(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    /* the variant: the variant-th agent of the mask — uniform: scalar code */
    int agent = 0;
    for (int a = 0, seen = 0; a < 4; a++) {
        if ((p.agent_mask >> a) & 1) {
            if (seen == (int)variant) agent = a;
            seen++;
        }
    }
    const int ec = lane >> 2, k = lane & 3;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the DMA rows have landed (one wavefront per workgroup: no barrier) */
    const int a0 = (int)tile[(POM_REC_AGENTS + 2 * agent) * 16 + ec];
    const PomQuadLanes Q(k);
    const ReachCells cells{reinterpret_cast<const uint8_t*>(tile) + ec};
    uint32_t walk, agents;
    pom_reach_sets_word(cells, k, walk, agents);
    /* a dead agent (AgentInfo::dead) reaches nothing: both rows are zero.  A live one's x and y are on the board (upload validates) */
    const uint32_t src = ag_dead(a0) ? 0u : Q.bit(ag_y(a0) * POM_N + ag_x(a0));
    uint32_t dist[POM_REACH_PLANES], mv[3];
    pom_reach_flood<MOVE, DIST>(Q, src, walk, agents, p.max_dist, dist, mv, ReachWaveMore());

    /* out: the planes as bytes into the staging rows, then row by row in runs of consecutive bytes */
    if (DIST) pom_reach_stage(stage + ec * 32, k, dist);
    if (MOVE) pom_reach_stage(stage + (DIST ? POM_REACH_STAGE_DWORDS : 0) + ec * 32, k, mv);
    obs_lds_order(); /* the lanes' staging writes are in LDS: no read below may be scheduled earlier */
    if (DIST) pom_reach_store(p.dist, stage, tile_id * 16, p.n, agent, lane);
    if (MOVE) pom_reach_store(p.move, stage + (DIST ? POM_REACH_STAGE_DWORDS : 0), tile_id * 16, p.n, agent, lane);
}

#endif /* __HIPCC__ */

#endif /* POM_REACH_H_ */
