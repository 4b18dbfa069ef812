/*
 * pom_deal.h — pom_batch_deal's kernel (include/pom_batch.h PomDealSpec, where THE RULE is stated): Pommerman's standard start board,
 * drawn on the device for any range of envs as a pure function of (seed, env, game number), into the env's record and restart snapshot
 * (POM_DEAL_START) or into the snapshot alone (POM_DEAL_NEXT), in ONE launch.
 *
 * The rule is written on 121-bit cell sets spread over a quad, one 32-cell word per lane, with the quad abstraction Q of
 * pom_policy_body.h (pom_quad_neighbours): on the device Q is PomQuadLanes (a word per lane, DPP exchanges), on the host
 * (tests/emul/pom_deal_emul.cpp, checked against tests/deal_oracle.py) four words at once.  Its pieces, all POM_HD:
 *   pom_deal_t        clause 5's number of pair k in attempt a: a pure function of (key, a, k), and 40 - k is static — so the lanes of
 *                     a quad compute ten of them each, all at once, and hand them round the quad in two packed registers a lane
 *                     (PomDealPacked: 8 DPP moves, no LDS);
 *   pom_deal_assign   clause 5's countdown over the 40 ready-made numbers, unrolled: the pairs' cells are compile-time constants, so
 *                     a pair's two bits are selects on constants and the rigid and wood sets come out of the countdown as sets;
 *   pom_deal_bad      clause 6: the flood from (1,1) by pom_quad_neighbours, then the count of walled-off passages;
 *   pom_deal_items    clause 7: pom_board_flags' countdown with a given count and a flag in 1..3, every lane of the quad over the whole
 *                     wood set (gathered with 4 DPP moves);
 *   pom_deal_dword    four cells' codes out of the sets;  pom_deal_row: clause 8, a fresh record's dwords 31..79 (pom_fresh_row) with the
 *                     agents one cell in from the corners.
 *
 * The kernel: one wavefront per tile, a quad of lanes per env, as pom_imagine_kernel.
 *   1  which envs of the tile are dealt (range, mask, the status byte of the record); a wavefront that deals none writes its zero
 *      result words and leaves;
 *   2  POM_DEAL_START: the tile into LDS as it stands (load_tile16_x4);
 *   3  the attempts: every quad retries on its own, the wavefront leaves the loop when a ballot shows no quad is left, or after 16;
 *   4  the items; the codes — lane k of the quad holds cells 32k .. 32k + 31, which are dwords 8k .. 8k + 7 of a dense record: the
 *      snapshot record is written from registers, a dword a store, and (START) the same bytes over the env's column of the tile;
 *   5  START: fresh agent memory, the whole tile out (store_tile16_x4) — every column that is not dealt leaves as it came.  NEXT stores
 *      no tile.
 * LDS: 5,120 B (the tile).  No scratch memory: nothing is indexed by a value that is not a compile-time constant after unrolling.
 */
#ifndef POM_DEAL_H_
#define POM_DEAL_H_

#include <stdint.h>

#include "pom_batch.h"
#include "pom_boardgen.h"
#include "pom_boardgen_body.h"
#include "pom_packed.h"
#include "pom_policy_body.h"

enum {
    POM_DEAL_PAIRS = 40,
    POM_DEAL_ATTEMPTS = 16,
    POM_DEAL_DRAW_STRIDE = 64,    /* draw 64 a + k: pair k of attempt a */
    POM_DEAL_DRAW_SELECT = 1024,  /* + c: is wood c chosen */
    POM_DEAL_DRAW_FLAG = 1280,    /* + c: what it hides */
    POM_DEAL_LANE_WOODS = 12,
    POM_DEAL_START_CELL = 1 * POM_BOARD_SIZE + 1, /* (1,1): where clause 6's flood starts */
    /* what a cell is before any draw (pom_deal_class) */
    POM_DEAL_PAIR = 0, POM_DEAL_FREE = 1, POM_DEAL_LANE = 2, POM_DEAL_AGENT = 4 /* + id */
};

/* ---- clauses 1 - 3: the geometry, at compile time ------------------------------------------------------------------------------- */
constexpr int pom_deal_line_class(int pos) /* position `pos` along one of the four lines y = 1, y = 9, x = 1, x = 9 */
{
    return pos == 2 || pos == 3 || pos == 7 || pos == 8 ? POM_DEAL_FREE : pos >= 4 && pos <= 6 ? POM_DEAL_LANE : POM_DEAL_PAIR;
}
constexpr int pom_deal_class(int c)
{
    const int y = c / POM_BOARD_SIZE, x = c % POM_BOARD_SIZE, lo = 1, hi = POM_BOARD_SIZE - 2;
    if (x == lo && y == lo) return POM_DEAL_AGENT + 0;
    if (x == hi && y == lo) return POM_DEAL_AGENT + 1;
    if (x == hi && y == hi) return POM_DEAL_AGENT + 2;
    if (x == lo && y == hi) return POM_DEAL_AGENT + 3;
    if ((y == lo || y == hi) && pom_deal_line_class(x) != POM_DEAL_PAIR) return pom_deal_line_class(x);
    if ((x == lo || x == hi) && pom_deal_line_class(y) != POM_DEAL_PAIR) return pom_deal_line_class(y);
    return x == y ? POM_DEAL_FREE : POM_DEAL_PAIR;
}
constexpr int pom_deal_transpose(int c) { return (c % POM_BOARD_SIZE) * POM_BOARD_SIZE + c / POM_BOARD_SIZE; }
constexpr bool pom_deal_is_upper(int c) { return pom_deal_class(c) == POM_DEAL_PAIR && c % POM_BOARD_SIZE > c / POM_BOARD_SIZE; }
/* the member with x > y of pair k (pairs are numbered by its ascending cell); k = POM_DEAL_PAIRS .. gives -1 */
constexpr int pom_deal_pair_upper(int k)
{
    for (int c = 0; c < POM_CELLS; c++)
        if (pom_deal_is_upper(c) && k-- == 0) return c;
    return -1;
}
constexpr int pom_deal_pair_count()
{
    int n = 0;
    for (int c = 0; c < POM_CELLS; c++) n += pom_deal_is_upper(c);
    return n;
}
static_assert(pom_deal_pair_count() == POM_DEAL_PAIRS && pom_deal_pair_upper(POM_DEAL_PAIRS - 1) >= 0 && pom_deal_pair_upper(POM_DEAL_PAIRS) < 0,
              "clause 3: the cells that clauses 1 and 2 leave form 40 mirror pairs");
/* word w (cells 32 w .. 32 w + 31) of the set of cells whose class is one of lo .. hi */
constexpr uint32_t pom_deal_class_word(int lo, int hi, int w)
{
    uint32_t m = 0;
    for (int b = 0; b < 32; b++)
        if (32 * w + b < POM_CELLS && pom_deal_class(32 * w + b) >= lo && pom_deal_class(32 * w + b) <= hi) m |= 1u << b;
    return m;
}

template <uint32_t V>
POM_HD uint32_t pom_deal_const() { return V; } /* (a value that must have been computed at compile time) */

/* ---- the layout (clause "Layout"): what pom_batch_deal refuses, or nullptr -------------------------------------------------------- */
POM_HD int pom_deal_lane_woods(const PomBoardLayout& l) { return (l.flags & POM_LAYOUT_NO_LANES) ? 0 : POM_DEAL_LANE_WOODS; }
POM_HD const char* pom_deal_layout_bad(const PomBoardLayout& l)
{
    const int L = pom_deal_lane_woods(l);
    if (l.flags & ~POM_LAYOUT_NO_LANES) return "layout.flags has unknown bits";
    if (l.num_rigid < 0 || (l.num_rigid & 1)) return "layout.num_rigid must be even and >= 0";
    if (l.num_wood < 0 || (l.num_wood & 1)) return "layout.num_wood must be even and >= 0";
    if (l.num_wood < L) return "layout.num_wood must be at least the 12 lane woods (or POM_LAYOUT_NO_LANES set)";
    if (l.num_rigid > 2 * POM_DEAL_PAIRS || l.num_rigid / 2 + (l.num_wood - L) / 2 > POM_DEAL_PAIRS) return "layout.num_rigid / 2 + (layout.num_wood - lane woods) / 2 must be <= 40 pairs";
    if (l.num_items < 0 || l.num_items > l.num_wood) return "layout.num_items must be 0..num_wood";
    if (l.max_inaccessible < 0 || l.max_inaccessible > POM_CELLS) return "layout.max_inaccessible must be 0..121";
    return nullptr;
}

/* ---- clauses 4 and 5 ----------------------------------------------------------------------------------------------------------- */
POM_HD uint32_t pom_deal_key(uint64_t seed, int64_t env, int32_t game) { return pom_board_key(seed, (uint32_t)env, (uint32_t)game); }
POM_HD int pom_deal_t(uint32_t key, int a, int k)
{
    return (int)pom_mulhi32(pom_board_draw(key, (uint32_t)(POM_DEAL_DRAW_STRIDE * a + k)), (uint32_t)(POM_DEAL_PAIRS - k));
}
/* where the countdown takes pair K's number from: the quad's packed registers — member m computed pairs m, m + 4, ..., m + 36, six bits each,
 * five to a word */
struct PomDealPacked {
    uint32_t w[4][2];
    template <int K>
    POM_HD int t() const { return (int)((w[K & 3][(K >> 2) / 5] >> (6 * ((K >> 2) % 5))) & 63u); }
};
POM_HD void pom_deal_pack(uint32_t key, int a, int member, uint32_t& p0, uint32_t& p1)
{
    p0 = p1 = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 5; i++) {
        p0 |= (uint32_t)pom_deal_t(key, a, member + 4 * i) << (6 * i);
        p1 |= (uint32_t)pom_deal_t(key, a, member + 4 * (i + 5)) << (6 * i);
    }
}
/* the countdown from pair K on; rigid and wood collect the cells of the pairs that become one */
template <int K, class Q, class T>
POM_HD void pom_deal_assign_from(const Q& q, const T& ts, int& need_r, int& need_w, typename Q::W& rigid, typename Q::W& wood)
{
    if constexpr (K < POM_DEAL_PAIRS) {
        constexpr int cu = pom_deal_pair_upper(K), cl = pom_deal_transpose(cu);
        const int t = ts.template t<K>();
        const typename Q::W bits = q.bit(cu) | q.bit(cl), none = bits & ~bits;
        const bool r = t < need_r, w = !r && t < need_r + need_w;
        rigid = rigid | (r ? bits : none);
        wood = wood | (w ? bits : none);
        need_r -= (int)r;
        need_w -= (int)w;
        pom_deal_assign_from<K + 1>(q, ts, need_r, need_w, rigid, wood);
    }
}
/* the sets of the constant classes, as the quad holds them (pom_deal_words: the Q's way from four words to its W) */
template <int LO, int HI, class Q>
POM_HD typename Q::W pom_deal_class_set(const Q& q)
{
    return pom_deal_words(q, pom_deal_const<pom_deal_class_word(LO, HI, 0)>(), pom_deal_const<pom_deal_class_word(LO, HI, 1)>(),
                          pom_deal_const<pom_deal_class_word(LO, HI, 2)>(), pom_deal_const<pom_deal_class_word(LO, HI, 3)>());
}
/* one attempt: the rigid set and the wood set, lanes included */
template <class Q, class T>
POM_HD void pom_deal_assign(const Q& q, const T& ts, const PomBoardLayout& l, typename Q::W& rigid, typename Q::W& wood)
{
    const int L = pom_deal_lane_woods(l);
    int need_r = l.num_rigid / 2, need_w = (l.num_wood - L) / 2;
    const typename Q::W lanes = pom_deal_class_set<POM_DEAL_LANE, POM_DEAL_LANE>(q);
    rigid = lanes & ~lanes;
    wood = L ? lanes : rigid;
    pom_deal_assign_from<0>(q, ts, need_r, need_w, rigid, wood);
}

/* ---- clause 6 ------------------------------------------------------------------------------------------------------------------ */
template <class Q>
POM_HD int pom_deal_bad(const Q& q, typename Q::W rigid, typename Q::W wood)
{
    const typename Q::W open = q.valid() & ~rigid;
    typename Q::W reach = q.bit(POM_DEAL_START_CELL);
    POM_NOUNROLL
    for (;;) {
        const typename Q::W grown = pom_quad_neighbours(q, reach) & open & ~reach;
        if (!q.any(grown)) break;
        reach = reach | grown;
    }
    const typename Q::W agents = pom_deal_class_set<POM_DEAL_AGENT, POM_DEAL_AGENT + 3>(q);
    return pom_deal_count(q, open & ~wood & ~agents & ~reach);
}

/* ---- clause 7: flag = f0 + 2 f1 of every wood ------------------------------------------------------------------------------------ */
template <class Q>
POM_HD void pom_deal_items(const Q& q, uint32_t key, typename Q::W wood, int num_items, typename Q::W& f0, typename Q::W& f1)
{
    uint32_t g[4];
    pom_deal_gather(q, wood, g);
    int left = __builtin_popcount(g[0]) + __builtin_popcount(g[1]) + __builtin_popcount(g[2]) + __builtin_popcount(g[3]), need = num_items;
    f0 = wood & ~wood;
    f1 = f0;
    const typename Q::W none = f0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int word = 0; word < 4; word++) {
        uint32_t w = g[word];
        POM_NOUNROLL
        while (w != 0 && need > 0) { /* need <= left always: once they are equal every remaining wood is chosen */
            const int c = 32 * word + __builtin_ctz(w);
            w &= w - 1;
            if ((int)pom_mulhi32(pom_board_draw(key, (uint32_t)(POM_DEAL_DRAW_SELECT + c)), (uint32_t)left) < need) {
                const uint32_t flag = 1u + pom_mulhi32(pom_board_draw(key, (uint32_t)(POM_DEAL_DRAW_FLAG + c)), 3u);
                const typename Q::W bit = q.bit(c);
                f0 = f0 | ((flag & 1u) ? bit : none);
                f1 = f1 | ((flag & 2u) ? bit : none);
                need--;
            }
            left--;
        }
    }
}

/* ---- the record ---------------------------------------------------------------------------------------------------------------- */
/* the codes of cells 32 word + 4 j .. + 3, a byte each — dword 8 word + j of a dense record: rigid, wood, f0, f1 are word `word` of
 * the sets.  The agents' cells hold neither (clause 1), and no bit lies past cell 120 */
POM_HD uint32_t pom_deal_dword(int word, int j, uint32_t rigid, uint32_t wood, uint32_t f0, uint32_t f1)
{
    constexpr int A = POM_DEAL_AGENT;
    /* the agents' cells; agents 1 and 3 have id bit 0, agents 2 and 3 id bit 1 */
    const uint32_t any4[4] = {pom_deal_const<pom_deal_class_word(A, A + 3, 0)>(), pom_deal_const<pom_deal_class_word(A, A + 3, 1)>(),
                              pom_deal_const<pom_deal_class_word(A, A + 3, 2)>(), pom_deal_const<pom_deal_class_word(A, A + 3, 3)>()};
    const uint32_t odd4[4] = {pom_deal_const<pom_deal_class_word(A + 1, A + 1, 0) | pom_deal_class_word(A + 3, A + 3, 0)>(),
                              pom_deal_const<pom_deal_class_word(A + 1, A + 1, 1) | pom_deal_class_word(A + 3, A + 3, 1)>(),
                              pom_deal_const<pom_deal_class_word(A + 1, A + 1, 2) | pom_deal_class_word(A + 3, A + 3, 2)>(),
                              pom_deal_const<pom_deal_class_word(A + 1, A + 1, 3) | pom_deal_class_word(A + 3, A + 3, 3)>()};
    const uint32_t high4[4] = {pom_deal_const<pom_deal_class_word(A + 2, A + 3, 0)>(), pom_deal_const<pom_deal_class_word(A + 2, A + 3, 1)>(),
                               pom_deal_const<pom_deal_class_word(A + 2, A + 3, 2)>(), pom_deal_const<pom_deal_class_word(A + 2, A + 3, 3)>()};
    const uint32_t any = pick4(word, any4), odd = pick4(word, odd4), high = pick4(word, high4);
    const uint32_t b0 = f0 | odd, b1 = f1 | high;
    uint32_t out = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        const int b = 4 * j + i;
        const uint32_t code = ((rigid >> b) & 1u) * POM_C_RIGID + ((wood >> b) & 1u) * POM_C_WOOD + ((any >> b) & 1u) * POM_C_AGENT + ((b0 >> b) & 1u) + 2u * ((b1 >> b) & 1u);
        out |= code << (8 * i);
    }
    return out;
}
/* clause 8: dword r >= POM_REC_TIMESTEP of the record — pom_fresh_row's, the agents one cell in from their corners */
POM_HD uint32_t pom_deal_row(int r)
{
    const uint32_t w = pom_fresh_row(r);
    if (r < POM_REC_AGENTS || r >= POM_REC_BOMBS || ((r - POM_REC_AGENTS) & 1)) return w;
    const int i = (r - POM_REC_AGENTS) >> 1;
    const uint32_t x = (i == 1 || i == 2) ? POM_BOARD_SIZE - 2 : 1, y = (i == 2 || i == 3) ? POM_BOARD_SIZE - 2 : 1;
    return (w & ~0xFFu) | x | (y << 4);
}
POM_HD uint32_t pom_deal_word(int attempts, int bad, int fallback)
{
    return (uint32_t)POM_DEAL_DEALT | (fallback ? (uint32_t)POM_DEAL_FALLBACK : 0u) | ((uint32_t)(attempts - 1) << POM_DEAL_ATTEMPTS_SHIFT) | ((uint32_t)bad << POM_DEAL_BAD_SHIFT);
}

#if defined(__HIPCC__) /* ---- the kernel ---- */

#include "pom_device.h"
#include "pom_policy_wave.h"

/* what the rule asks of a Q beyond pom_policy_body.h's list, for PomQuadLanes */
__device__ __forceinline__ uint32_t pom_deal_words(const PomQuadLanes& q, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t v[4] = {a, b, c, d};
    return pick4(q.k, v);
}
__device__ __forceinline__ int pom_deal_count(const PomQuadLanes&, uint32_t w)
{
    int v = __builtin_popcount(w);
    v += pom_dpp_x1(v);
    return v + pom_dpp_x2(v);
}
template <int J>
__device__ __forceinline__ uint32_t pom_deal_member(uint32_t v) /* the value held by member J of the quad */
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, J * 0x55, 0xF, 0xF, true);
}
__device__ __forceinline__ void pom_deal_gather(const PomQuadLanes&, uint32_t w, uint32_t (&g)[4])
{
    g[0] = pom_deal_member<0>(w);
    g[1] = pom_deal_member<1>(w);
    g[2] = pom_deal_member<2>(w);
    g[3] = pom_deal_member<3>(w);
}

struct DealParams {
    uint32_t* state;
    uint32_t* snap;          /* [n_pad][80], dense records */
    uint32_t* agent_mem;     /* [2][4 * n_pad] or nullptr */
    int32_t* games;          /* [n] */
    const int32_t* mask;     /* [n] or nullptr */
    uint32_t* result;        /* [n] or nullptr */
    int64_t first, count, n_pad, tile0, env_offset;
    uint64_t seed;
    PomBoardLayout layout;
    int32_t mode, which;
};

__global__ __launch_bounds__(64, 2) void pom_deal_kernel(DealParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POM_REC_DWORDS * 16];
    const int lane = threadIdx.x;
    const int64_t tile_id = p.tile0 + pom_xcd_tile_order(blockIdx.x, gridDim.x);
    const int ec = lane >> 2, member = lane & 3;
    const int64_t d = tile_id * 16 + ec;
    const bool in_range = d >= p.first && d - p.first < p.count;
    uint32_t* const tile_g = p.state + tile_id * POM_TILE_DWORDS;
    const bool start = p.mode == POM_DEAL_START;
    if (start) load_tile16_x4(tile_g, tile, lane);
    bool dealt = in_range;
    if (in_range && p.which == POM_DEAL_MASK) dealt = p.mask[d] != 0;
    if (in_range && p.which >= POM_DEAL_RESTARTED) { /* the status byte: M1 of agent 1 (pom_packed.h) */
        const uint32_t status = tile_g[(POM_REC_AGENTS + 3) * POM_TILE_ENVS + ec] >> 24;
        dealt = (status & (p.which == POM_DEAL_RESTARTED ? (uint32_t)POM_ST_RESTARTED : (uint32_t)POM_ST_DONE)) != 0;
    }
    /* the destination tile's DMA rows have landed (one wavefront per workgroup: no barrier) — before any column is written over, and
     * before a wavefront with nothing to deal may leave */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!__any(dealt)) {
        if (p.result && in_range && member == 0) p.result[d] = 0u;
        return;
    }
    const int32_t game = dealt ? p.games[d] : 0;
    const uint32_t key = pom_deal_key(p.seed, p.env_offset + d, game);
    const PomQuadLanes Q(member);

    /* clauses 5 and 6: every quad on its own */
    uint32_t rigid = 0, wood = 0;
    int attempts = 0, bad = 0;
    bool todo = dealt;
    POM_NOUNROLL
    for (int a = 0; a < POM_DEAL_ATTEMPTS; a++) {
        if (todo) {
            uint32_t p0, p1;
            pom_deal_pack(key, a, member, p0, p1);
            PomDealPacked ts;
            ts.w[0][0] = pom_deal_member<0>(p0);
            ts.w[0][1] = pom_deal_member<0>(p1);
            ts.w[1][0] = pom_deal_member<1>(p0);
            ts.w[1][1] = pom_deal_member<1>(p1);
            ts.w[2][0] = pom_deal_member<2>(p0);
            ts.w[2][1] = pom_deal_member<2>(p1);
            ts.w[3][0] = pom_deal_member<3>(p0);
            ts.w[3][1] = pom_deal_member<3>(p1);
            pom_deal_assign(Q, ts, p.layout, rigid, wood);
            bad = pom_deal_bad(Q, rigid, wood);
            attempts = a + 1;
            todo = bad > p.layout.max_inaccessible;
        }
        if (!__any(todo)) break;
    }
    uint32_t word = 0;
    if (dealt) {
        uint32_t f0, f1;
        pom_deal_items(Q, key, wood, p.layout.num_items, f0, f1);
        word = pom_deal_word(attempts, bad, todo);
        /* the record: lane `member` holds dwords 8 member .. 8 member + 7 of the board, the quad shares rows 31..79 */
        uint32_t* const rec = p.snap + d * POM_REC_DWORDS;
        uint8_t* const cells = reinterpret_cast<uint8_t*>(tile) + ec;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int dw = 8 * member + j;
            if (dw < POM_REC_BOARD_DWORDS) {
                const uint32_t w = pom_deal_dword(member, j, rigid, wood, f0, f1);
                rec[dw] = w;
                if (start) {
#pragma unroll
                    for (int i = 0; i < 4; i++) cells[(4 * dw + i) * POM_TILE_ENVS] = (uint8_t)(w >> (8 * i));
                }
            }
        }
        POM_NOUNROLL
        for (int r = POM_REC_TIMESTEP + member; r < POM_REC_DWORDS; r += 4) {
            const uint32_t w = pom_deal_row(r);
            rec[r] = w;
            if (start) tile[r * POM_TILE_ENVS + ec] = w;
        }
        if (start && p.agent_mem) { /* a new game: fresh agents */
            p.agent_mem[d * 4 + member] = 0;
            p.agent_mem[4 * p.n_pad + d * 4 + member] = 0;
        }
        if (member == 0) p.games[d] = (int32_t)((uint32_t)game + 1u);
    }
    if (start) {
        asm volatile("" ::: "memory"); /* the columns are written: the store below reads the tile row by row */
        store_tile16_x4(tile_g, tile, lane);
    }
    if (p.result && in_range && member == 0) p.result[d] = word;
}

#endif /* __HIPCC__ */

#endif /* POM_DEAL_H_ */
