/*
 * pom_packed.h — the device-resident record of one board ("env") and its
 * lossless conversion from / to the 1004-byte boundary State (pom_state.h,
 * i.e. bboard::State, /root/reference/include/bboard.hpp:356-506).
 *
 * HBM layout: an array of 16-env TILES, struct-of-arrays inside a tile — dword d >= 31 of env e lives at
 * buf[(e / 16) * 1280 + d * 16 + (e % 16)] (pom_rec_col, row stride POM_TILE_ENVS), and the board — the tile's first 31 rows,
 * 1,984 bytes — is laid out BY CELL: cell c of env e is byte c * 16 + (e % 16) of the tile (cells 121..123: zero), so that the
 * address of a cell in the wavefront's LDS copy of the tile is one shift-and-add of the cell number (round 5; with the cells of
 * an env packed four to a dword it was four instructions, and the tick does little else with its vector ALU than look at cells).  A tile is 5,120
 * contiguous bytes (40 lines of 128 B): the wavefront that owns it moves it with five 1-KB instructions (16 bytes per lane),
 * every cache line full in both directions, and touches ONE region of memory instead of 80 rows that
 * lie n_pad * 4 bytes apart (rounds 1-2: 4.35 G env-steps/s at 524,288 envs against 6.5 G at 262,144 —
 * beyond the memory-side cache the strided rows cost DRAM and TLB locality).
 *
 * POM_REC_DWORDS = 80 dwords (320 B) per env instead of 251 (rounds 1-4: 112, with 16-bit cells):
 *   [0..30]    board, 121 cells of 8 bits (a dense record — snapshot, terminal, host tests: cell c in byte c&3 of dword c>>2, the
 *              last three bytes 0; a tile: see above)
 *   [31]       timeStep
 *   [32..39]   agents: A0[i] = x:4 | y:4 | bombCount:8 (signed) @8 | canKick@16 | dead@17 | M0[i]:8 @24
 *                      A1[i] = maxBombCount:16 | bombStrength:8 @16 | M1[i]:8 @24
 *              The top bytes of the eight agent words carry what does not belong to an agent (two dwords saved: exactly five 1-KB
 *              moves per tile and direction):  M0 = aliveAgents (signed), bombs.index, bombs.count, flames.index
 *                                              M1 = flames.count, status, ubflags low byte, ubflags high byte
 *   [40..59]   bombs.queue raw (all 20 slots: stale slots are state)
 *   [60..79]   flames.queue: x:8 | y:8 | timeLeft:8 (signed) | strength:8
 *
 * Cell code (8 bit) for board value v (Item, bboard.hpp:54-71) — every value a game can reach from a valid start has one, and
 * the 256 codes are exactly used up:
 *   0 passage  1 rigid  2 Item::BOMB  3 / 4 / 5 extra-bomb / incr-range / kick  6..10 wood with flag 0..4  11..14 agent 0..3
 *   15 + id             a flame with FLAME_ID id = origin cell (0..120) and no power-up under it
 *   136 + 40 (f - 1) + 10 r + (d - 1)
 *                       a flame with power-up flag f = 1..3: the origin is NOT stored as a number but as where it lies from the
 *                       cell — d = 1..10 cells back along ray r (0: the cell is at +x of the origin, 1: -x, 2: +y, 3: -y).  A flagged
 *                       flame cell is a burnt wood, wood ends the ray that burns it, and SpawnFlame's rays run along the origin's
 *                       row and column (bboard.cpp:24-57, 198-263): in a reachable state the origin of such a cell always lies on
 *                       its row or column, at most 10 cells away.
 * So a cell is self-contained (no reference into the flame queue, whose slots are overwritten when it overflows), PopFlame's
 * "is this my flame" (bboard.cpp:148-180) is a compare on the code, and the record's board is 124 bytes instead of 244.
 * Values outside this set — fog, hand-written flame cells whose origin is not on their row / column, wood flags above 4, ... —
 * are rejected at upload (POM_E_UNREPRESENTABLE), never silently altered.
 */
#ifndef POM_PACKED_H_
#define POM_PACKED_H_

#include <stdint.h>

#include "pom_rng.h" /* POM_HD */
#include "pom_state.h"

enum {
    POM_REC_BOARD = 0,
    POM_REC_BOARD_DWORDS = 31,
    POM_REC_TIMESTEP = 31,
    POM_REC_AGENTS = 32,
    POM_REC_BOMBS = 40,
    POM_REC_FLAMES = 60,
    POM_REC_DWORDS = 80,
    POM_TILE_ENVS = 16,                              /* envs per tile of the device buffers = row stride of a column, in dwords */
    POM_TILE_DWORDS = POM_REC_DWORDS * POM_TILE_ENVS /* 1280 */
};
/* agent words */
enum { POM_AG_KICK = 1 << 16, POM_AG_DEAD = 1 << 17 };

/* The two "meta" words a record used to have, put together from / spread over the top bytes of its agent words:
 *   meta  = aliveAgents:8 | bombs.index:8 | bombs.count:8 | flames.index:8     (M0 of agents 0..3)
 *   meta2 = flames.count:8 | status:8 | ubflags:16                             (M1 of agents 0..3) */
POM_HD uint32_t pom_rec_meta(const uint32_t* rec, int64_t stride)
{
    return (rec[(POM_REC_AGENTS + 0) * stride] >> 24) | ((rec[(POM_REC_AGENTS + 2) * stride] >> 24) << 8) |
           ((rec[(POM_REC_AGENTS + 4) * stride] >> 24) << 16) | ((rec[(POM_REC_AGENTS + 6) * stride] >> 24) << 24);
}
POM_HD uint32_t pom_rec_meta2(const uint32_t* rec, int64_t stride)
{
    return (rec[(POM_REC_AGENTS + 1) * stride] >> 24) | ((rec[(POM_REC_AGENTS + 3) * stride] >> 24) << 8) |
           ((rec[(POM_REC_AGENTS + 5) * stride] >> 24) << 16) | ((rec[(POM_REC_AGENTS + 7) * stride] >> 24) << 24);
}
POM_HD void pom_rec_set_meta(uint32_t* rec, int64_t stride, uint32_t meta, uint32_t meta2)
{
    for (int i = 0; i < 4; i++) {
        uint32_t& a0 = rec[(POM_REC_AGENTS + 2 * i) * stride];
        uint32_t& a1 = rec[(POM_REC_AGENTS + 2 * i + 1) * stride];
        a0 = (a0 & 0x00FFFFFFu) | (((meta >> (8 * i)) & 0xFFu) << 24);
        a1 = (a1 & 0x00FFFFFFu) | (((meta2 >> (8 * i)) & 0xFFu) << 24);
    }
}

/* status byte of META2 */
enum {
    POM_ST_DONE = 1,     /* Environment::finished, environment.cpp:152-168 */
    POM_ST_DRAW = 2,     /* Environment::isDraw */
    POM_ST_WINNER_SHIFT = 2, /* 3 bits: agentWon + 1 (0 = nobody) */
    POM_ST_TIMEOUT = 32, /* timeStep reached max_steps (StartGame's loop bound, environment.cpp:71) */
    POM_ST_RESTARTED = 64 /* auto_reset at the end of the tick (POM_RESET_AT_END): the previous tick finished this env's episode and
                             put it on its next start state; the finished episode's record is in the terminal buffer */
};

enum {
    POM_C_PASSAGE = 0, POM_C_RIGID = 1, POM_C_BOMB = 2, POM_C_EXTRABOMB = 3, POM_C_INCRRANGE = 4, POM_C_KICK = 5,
    POM_C_WOOD = 6,    /* + flag 0..4 */
    POM_C_AGENT = 11,  /* + id */
    POM_C_FLAME = 15,  /* + origin cell */
    POM_C_FLAGGED = 136 /* + 40 (flag - 1) + 10 ray + (distance - 1) */
};

/* where env e's column starts in a device buffer (dword units); its dword d is at pom_rec_col(e) + d * POM_TILE_ENVS */
POM_HD int64_t pom_rec_col(int64_t e) { return (e >> 4) * POM_TILE_DWORDS + (e & 15); }

/* the code of a flame cell with power-up flag f (1..3) that lies d (1..10) cells along ray r (0 +x, 1 -x, 2 +y, 3 -y) from its origin */
POM_HD int pom_flagged_code(int f, int r, int d) { return POM_C_FLAGGED + 40 * (f - 1) + 10 * r + (d - 1); }

POM_HD int pom_cell_encode(int32_t v, int c /* the cell: y * 11 + x */) /* -1 if not representable */
{
    if (v == POM_PASSAGE) return POM_C_PASSAGE;
    if (v == POM_RIGID) return POM_C_RIGID;
    if (v == POM_BOMB) return POM_C_BOMB;
    if (v >= POM_EXTRABOMB && v <= POM_KICK) return POM_C_EXTRABOMB + (v - POM_EXTRABOMB);
    if (v >= POM_WOOD && v <= POM_WOOD + 4) return POM_C_WOOD + (v - POM_WOOD);
    if (v >= POM_AGENT0 && v < POM_AGENT0 + POM_AGENT_COUNT) return POM_C_AGENT + (v - POM_AGENT0);
    if (v >= POM_FLAMES && v < POM_FLAMES + (POM_CELLS << 3)) {
        const int id = (v - POM_FLAMES) >> 3, f = (v - POM_FLAMES) & 7;
        if (f == 0) return POM_C_FLAME + id;
        if (f > 3) return -1;
        const int cy = c / POM_BOARD_SIZE, cx = c - cy * POM_BOARD_SIZE, oy = id / POM_BOARD_SIZE, ox = id - oy * POM_BOARD_SIZE;
        if (oy == cy && ox != cx) return pom_flagged_code(f, cx > ox ? 0 : 1, cx > ox ? cx - ox : ox - cx);
        if (ox == cx && oy != cy) return pom_flagged_code(f, cy > oy ? 2 : 3, cy > oy ? cy - oy : oy - cy);
    }
    return -1;
}

POM_HD int32_t pom_cell_decode(int e, int c)
{
    if (e < POM_C_WOOD) return e <= POM_C_RIGID ? e : e == POM_C_BOMB ? POM_BOMB : POM_EXTRABOMB + (e - POM_C_EXTRABOMB);
    if (e < POM_C_AGENT) return POM_WOOD + (e - POM_C_WOOD);
    if (e < POM_C_FLAME) return POM_AGENT0 + (e - POM_C_AGENT);
    if (e < POM_C_FLAGGED) return POM_FLAMES + ((e - POM_C_FLAME) << 3);
    const int k = e - POM_C_FLAGGED, f = k / 40 + 1, r = (k % 40) / 10, d = k % 10 + 1;
    const int origin = c - d * (r == 0 ? 1 : r == 1 ? -1 : r == 2 ? POM_BOARD_SIZE : -POM_BOARD_SIZE);
    return POM_FLAMES + (origin << 3) + f;
}
/* FLAME_ID (bboard.hpp:98-101) of a flame code at cell c */
POM_HD int pom_flame_origin(int e, int c)
{
    if (e < POM_C_FLAGGED) return e - POM_C_FLAME;
    const int k = (e - POM_C_FLAGGED) % 40, r = k / 10, d = k % 10 + 1;
    return c - d * (r == 0 ? 1 : r == 1 ? -1 : r == 2 ? POM_BOARD_SIZE : -POM_BOARD_SIZE);
}

/* Where cell c of a record lives.  `rec` with stride 1: a dense record.  `rec` with stride POM_TILE_ENVS: the column of env
 * number `lane` (0..15) of a tile, i.e. rec = tile + lane — its board is the tile's byte c * 16 + lane. */
POM_HD int64_t pom_rec_cell_byte(int64_t stride, int lane, int c) { return stride == 1 ? (int64_t)c : (int64_t)c * POM_TILE_ENVS + lane - 4 * (int64_t)lane; }
POM_HD int pom_rec_cell(const uint32_t* rec, int64_t stride, int c, int lane = 0)
{
    return reinterpret_cast<const uint8_t*>(rec)[pom_rec_cell_byte(stride, lane, c)];
}
POM_HD void pom_rec_set_cell(uint32_t* rec, int64_t stride, int c, int code, int lane = 0)
{
    reinterpret_cast<uint8_t*>(rec)[pom_rec_cell_byte(stride, lane, c)] = (uint8_t)code;
}

/*
 * Moving one env's record between places, item by item (pom_batch_copy_envs, pom_copy.h).  A record is POM_COL_ITEMS items: the
 * 124 board bytes (cells 0..120 and the three zero bytes behind them), then dwords 31..79.  Item k of the column of env number
 * `lane` (0..15) of a tile (`tile` = the tile's first dword) is byte k * 16 + lane of the tile for k < 124, dword
 * (31 + k - 124) * 16 + lane otherwise; item k of a dense record (snapshot, terminal) is byte k for k < 124, dword 31 + k - 124
 * otherwise.  A wavefront moves a record with its lanes taking items lane, lane + 64, lane + 128; the host tests loop over k.
 */
enum { POM_COL_BOARD_ITEMS = 4 * POM_REC_BOARD_DWORDS, POM_COL_ITEMS = POM_COL_BOARD_ITEMS + POM_REC_DWORDS - POM_REC_TIMESTEP /* 173 */ };

/* tile column -> tile column */
POM_HD void pom_col_copy_item(uint32_t* dst_tile, int dst_lane, const uint32_t* src_tile, int src_lane, int k)
{
    if (k < POM_COL_BOARD_ITEMS)
        reinterpret_cast<uint8_t*>(dst_tile)[k * POM_TILE_ENVS + dst_lane] = reinterpret_cast<const uint8_t*>(src_tile)[k * POM_TILE_ENVS + src_lane];
    else {
        const int d = POM_REC_TIMESTEP + k - POM_COL_BOARD_ITEMS;
        dst_tile[d * POM_TILE_ENVS + dst_lane] = src_tile[d * POM_TILE_ENVS + src_lane];
    }
}
/* dense record -> tile column */
POM_HD void pom_rec_to_col_item(uint32_t* dst_tile, int dst_lane, const uint32_t* rec, int k)
{
    if (k < POM_COL_BOARD_ITEMS)
        reinterpret_cast<uint8_t*>(dst_tile)[k * POM_TILE_ENVS + dst_lane] = reinterpret_cast<const uint8_t*>(rec)[k];
    else {
        const int d = POM_REC_TIMESTEP + k - POM_COL_BOARD_ITEMS;
        dst_tile[d * POM_TILE_ENVS + dst_lane] = rec[d];
    }
}
/* tile column -> dense record; as_snapshot: status and ubflags come out clear (the top bytes of agent words 35, 37, 39 = bytes 1..3
 * of meta2), as pom_batch_snapshot leaves them */
POM_HD void pom_col_to_rec_item(uint32_t* rec, const uint32_t* src_tile, int src_lane, int k, bool as_snapshot)
{
    if (k < POM_COL_BOARD_ITEMS)
        reinterpret_cast<uint8_t*>(rec)[k] = reinterpret_cast<const uint8_t*>(src_tile)[k * POM_TILE_ENVS + src_lane];
    else {
        const int d = POM_REC_TIMESTEP + k - POM_COL_BOARD_ITEMS;
        const uint32_t v = src_tile[d * POM_TILE_ENVS + src_lane];
        const bool meta2_hi = d == POM_REC_AGENTS + 3 || d == POM_REC_AGENTS + 5 || d == POM_REC_AGENTS + 7;
        rec[d] = as_snapshot && meta2_hi ? v & 0x00FFFFFFu : v;
    }
}
/* whole records, for host code and tests */
POM_HD void pom_col_copy(uint32_t* dst_tile, int dst_lane, const uint32_t* src_tile, int src_lane)
{
    for (int k = 0; k < POM_COL_ITEMS; k++) pom_col_copy_item(dst_tile, dst_lane, src_tile, src_lane, k);
}
POM_HD void pom_rec_to_col(uint32_t* dst_tile, int dst_lane, const uint32_t* rec)
{
    for (int k = 0; k < POM_COL_ITEMS; k++) pom_rec_to_col_item(dst_tile, dst_lane, rec, k);
}
POM_HD void pom_col_to_rec(uint32_t* rec, const uint32_t* src_tile, int src_lane, bool as_snapshot)
{
    for (int k = 0; k < POM_COL_ITEMS; k++) pom_col_to_rec_item(rec, src_tile, src_lane, k, as_snapshot);
}

/*
 * Upload bounds of the narrow fields, chosen so that NO sequence of ticks can take a field out of its width (a state beyond them
 * is refused with POM_E_UNREPRESENTABLE; games start at bombCount 0, maxBombCount 1, bombStrength 1, aliveAgents 4):
 *   bombCount (8 bits, signed)  goes up by one per bomb its agent plants and down by one per bomb of its agent that explodes
 *        (bboard.cpp:95,116,144), and every planted bomb is queued: bombCount - (the agent's bombs in the queue) never changes.
 *        The queue holds 0..20 bombs, so bombCount stays within 20 of where it started.
 *   maxBombCount (16 bits, signed), bombStrength (8 bits)  grow by one per EXTRABOMB / INCRRANGE picked up and never shrink
 *        (step_utility.cpp:247-256).  A power-up comes from a cell (a power-up, a wood or a flagged flame of the start state) and
 *        picking it up uses it up; nothing puts a new one on the board.  So all agents together pick up at most 121.
 *        ag_strength_inc's hold at 255 (pom_step_body.h) is then a guard that no uploaded state reaches.
 *   aliveAgents (8 bits, signed)  goes down by one per agent that dies, and State::Kill kills an agent once (bboard.hpp:474-481).
 */
enum {
    POM_PACK_BOMBCOUNT_MIN = -128 + POM_MAX_BOMBS, POM_PACK_BOMBCOUNT_MAX = 127 - POM_MAX_BOMBS, /* -108 .. 107 */
    POM_PACK_MAXBOMBS_MAX = 32767 - POM_CELLS,                                                /* 32646 (and >= -32768) */
    POM_PACK_STRENGTH_MAX = 255 - POM_CELLS,                                                   /* 134 (and >= 0) */
    POM_PACK_ALIVE_MIN = -128 + POM_AGENT_COUNT                                                /* -124 (and <= 127) */
};
POM_HD int pom_pack_agent_bad(int32_t bomb_count, int32_t max_bombs, int32_t strength)
{
    return (bomb_count < POM_PACK_BOMBCOUNT_MIN) | (bomb_count > POM_PACK_BOMBCOUNT_MAX) | (max_bombs < -32768) |
           (max_bombs > POM_PACK_MAXBOMBS_MAX) | (strength < 0) | (strength > POM_PACK_STRENGTH_MAX);
}
POM_HD int pom_pack_alive_bad(int32_t alive) { return (alive < POM_PACK_ALIVE_MIN) | (alive > 127); }

POM_HD int32_t pom_sext8(uint32_t v) { return (int32_t)(int8_t)(v & 0xFF); }
POM_HD int32_t pom_sext16(uint32_t v) { return (int32_t)(int16_t)(v & 0xFFFF); }

/*
 * The State <-> record mapping, one function per kind of record item and direction: what a field's bits are and what upload
 * refuses is written here and nowhere else.  `st` is the State as 251 dwords (pom_state.h): board @0, timeStep @121,
 * aliveAgents @122, agents @123 (6 dwords each), bombs @147 (queue, index @167, count @168), flames @169 (4 dwords a slot,
 * index @249, count @250).  The pack functions return 1 if a field does not fit (the words they give are then not to be used).
 * A board cell is pom_cell_encode(st[c], c) / pom_cell_decode above.
 */
POM_HD uint32_t pom_pack_timestep(const int32_t* st) { return (uint32_t)st[121]; }
POM_HD void pom_unpack_timestep(uint32_t w, int32_t* st) { st[121] = (int32_t)w; }

/* Agent i's two words.  Their top bytes carry a scalar of the State each (M0 / M1 in the layout above), and the agent's
 * verdict covers the scalars it carries: aliveAgents and flames.count with agent 0, bombs.index, bombs.count, flames.index with
 * agents 1, 2, 3.  Status and ubflags (M1 of agents 1..3) start clear. */
POM_HD int pom_agent_m0_dword(int i) { return i == 0 ? 122 : i == 1 ? 167 : i == 2 ? 168 : 249; } /* the State dword in M0 of agent i */
POM_HD int pom_pack_agent(const int32_t* st, int i, uint32_t& a0, uint32_t& a1)
{
    const int32_t* a = st + 123 + 6 * i;
    const int32_t m0 = st[pom_agent_m0_dword(i)], fCnt = st[250];
    const uint32_t flags = (uint32_t)a[5], m1 = i == 0 ? (uint32_t)fCnt & 0xFFu : 0u;
    const int kick = (flags & 0xFF) != 0, dead = ((flags >> 8) & 0xFF) != 0;
    int bad = (a[0] < 0) | (a[0] >= POM_BOARD_SIZE) | (a[1] < 0) | (a[1] >= POM_BOARD_SIZE);
    bad |= pom_pack_agent_bad(a[2], a[3], a[4]);
    bad |= i == 0 ? pom_pack_alive_bad(m0) | (fCnt < 0) | (fCnt > 255)
                  : (m0 < 0) | (i == 2 ? m0 > POM_MAX_BOMBS : m0 >= POM_MAX_BOMBS); /* a count may be 20, an index not */
    a0 = ((uint32_t)a[0] & 0xF) | (((uint32_t)a[1] & 0xF) << 4) | (((uint32_t)a[2] & 0xFF) << 8) | (kick ? (uint32_t)POM_AG_KICK : 0u) |
         (dead ? (uint32_t)POM_AG_DEAD : 0u) | (((uint32_t)m0 & 0xFFu) << 24);
    a1 = ((uint32_t)a[3] & 0xFFFF) | (((uint32_t)a[4] & 0xFF) << 16) | (m1 << 24);
    return bad;
}
/* ... and back; the two padding bytes of the agent come out 0 */
POM_HD void pom_unpack_agent(uint32_t a0, uint32_t a1, int32_t* st, int i)
{
    int32_t* a = st + 123 + 6 * i;
    a[0] = (int32_t)(a0 & 0xF);
    a[1] = (int32_t)((a0 >> 4) & 0xF);
    a[2] = pom_sext8(a0 >> 8);
    a[3] = pom_sext16(a1);
    a[4] = (int32_t)((a1 >> 16) & 0xFF);
    a[5] = (int32_t)(((a0 & POM_AG_KICK) ? 1u : 0u) | ((a0 & POM_AG_DEAD) ? 0x100u : 0u));
    st[pom_agent_m0_dword(i)] = i == 0 ? pom_sext8(a0 >> 24) : (int32_t)(a0 >> 24);
    if (i == 0) st[250] = (int32_t)(a1 >> 24);
}

/* bombs.queue slot k, raw (all 20 slots: stale slots are state) */
POM_HD uint32_t pom_pack_bomb(const int32_t* st, int k) { return (uint32_t)st[147 + k]; }
POM_HD void pom_unpack_bomb(uint32_t w, int32_t* st, int k) { st[147 + k] = (int32_t)w; }
/* The device's own rule on top of the field widths: a LIVE bomb — slot k is one of the bombs.count slots from bombs.index on —
 * must sit on the board and belong to a real agent, because the tick indexes cells and agents with it (bomb word,
 * bboard.hpp:261-335: x:4 | y:4 | id:4 @8).  Upload to a batch and pom_step apply it; pom_pack_state alone does not (the host
 * model packs states that rely on that).  Only asked of a queue whose index and count pom_pack_agent accepts: another is
 * refused anyway. */
POM_HD int pom_pack_live_bomb_bad(const int32_t* st, int k)
{
    const int32_t b = st[147 + k], bIdx = st[167], bCnt = st[168];
    const int age = (int)((uint32_t)k - (uint32_t)bIdx) + (k < bIdx ? POM_MAX_BOMBS : 0); /* slot k is the age-th bomb of the queue */
    const int live = (bIdx >= 0) & (bIdx < POM_MAX_BOMBS) & (age < bCnt);
    return live & (((b & 0xF) >= POM_BOARD_SIZE) | (((b >> 4) & 0xF) >= POM_BOARD_SIZE) | (((b >> 8) & 0xF) >= POM_AGENT_COUNT));
}

/* flames.queue slot k, the stale slots too */
POM_HD int pom_pack_flame(const int32_t* st, int k, uint32_t& w)
{
    const int32_t* f = st + 169 + 4 * k;
    w = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | (((uint32_t)f[2] & 0xFF) << 16) | ((uint32_t)f[3] << 24);
    return (f[0] < 0) | (f[0] >= POM_BOARD_SIZE) | (f[1] < 0) | (f[1] >= POM_BOARD_SIZE) | (f[2] < -128) | (f[2] > 127) | (f[3] < 0) | (f[3] > 255);
}
POM_HD void pom_unpack_flame(uint32_t w, int32_t* st, int k)
{
    int32_t* o = st + 169 + 4 * k;
    o[0] = (int32_t)(w & 0xFF);
    o[1] = (int32_t)((w >> 8) & 0xFF);
    o[2] = pom_sext8(w >> 16);
    o[3] = (int32_t)(w >> 24);
}

/* the status byte and the flags of META2 as the C-ABI reports them */
struct PomStatus { int32_t done, winner /* -1: nobody */, draw, ubflags; };
POM_HD PomStatus pom_status_decode(uint32_t meta2)
{
    const uint32_t s8 = (meta2 >> 8) & 0xFF;
    return {(s8 & POM_ST_DONE) ? 1 : 0, (int32_t)((s8 >> POM_ST_WINNER_SHIFT) & 7) - 1, (s8 & POM_ST_DRAW) ? 1 : 0, (int32_t)(meta2 >> 16)};
}

/*
 * Pack one boundary State into a record.  `rec` is addressed with a stride so
 * the same code fills a column of a device tile (stride = POM_TILE_ENVS) and a dense
 * record in host-side tests (stride = 1).  Returns 0, or 1 if a field does not
 * fit the record (nothing is written in that case... the caller zero-fills).
 */
POM_HD int pom_pack_state(const int32_t* st, uint32_t* rec, int64_t stride, int lane = 0)
{
    int bad = 0;
    for (int c = 0; c < 4 * POM_REC_BOARD_DWORDS; c++) {
        const int e = c < POM_CELLS ? pom_cell_encode(st[c], c) : 0; /* (the three bytes behind the board: 0) */
        bad |= e < 0;
        pom_rec_set_cell(rec, stride, c, e & 0xFF, lane);
    }
    rec[POM_REC_TIMESTEP * stride] = pom_pack_timestep(st);
    for (int i = 0; i < POM_AGENT_COUNT; i++)
        bad |= pom_pack_agent(st, i, rec[(POM_REC_AGENTS + 2 * i) * stride], rec[(POM_REC_AGENTS + 2 * i + 1) * stride]);
    for (int k = 0; k < POM_MAX_BOMBS; k++) rec[(POM_REC_BOMBS + k) * stride] = pom_pack_bomb(st, k);
    for (int k = 0; k < POM_MAX_BOMBS; k++) bad |= pom_pack_flame(st, k, rec[(POM_REC_FLAMES + k) * stride]);
    return bad;
}

/* inverse of pom_pack_state */
POM_HD void pom_unpack_state(const uint32_t* rec, int64_t stride, int32_t* st, int lane = 0)
{
    for (int c = 0; c < POM_CELLS; c++) st[c] = pom_cell_decode(pom_rec_cell(rec, stride, c, lane), c);
    pom_unpack_timestep(rec[POM_REC_TIMESTEP * stride], st);
    for (int i = 0; i < POM_AGENT_COUNT; i++) pom_unpack_agent(rec[(POM_REC_AGENTS + 2 * i) * stride], rec[(POM_REC_AGENTS + 2 * i + 1) * stride], st, i);
    for (int k = 0; k < POM_MAX_BOMBS; k++) pom_unpack_bomb(rec[(POM_REC_BOMBS + k) * stride], st, k);
    for (int k = 0; k < POM_MAX_BOMBS; k++) pom_unpack_flame(rec[(POM_REC_FLAMES + k) * stride], st, k);
}

/*
 * The same two directions for ONE State handled by one wavefront (pom_step / pom_env_step, pom_step_one_kernel): the record
 * is column 0 of a zeroed tile, and lane 0..63 takes cells lane and lane + 64, lanes 0..3 an agent each, lanes 20..39 a bomb
 * slot, lanes 40..59 a flame slot, lane 61 timeStep.  Packing applies the live-bomb rule, as upload to a batch does.  A lane's
 * verdict covers its own items; the State is refused if any lane's is set.  The host tests call them for lane = 0..63.
 */
enum { POM_LANE_BOMBS = 20, POM_LANE_FLAMES = 40, POM_LANE_SCALARS = 61 };
POM_HD int pom_pack_lane(const int32_t* st, uint32_t* tile, int lane)
{
    int bad = 0;
    for (int c = lane; c < POM_CELLS; c += 64) { /* (the tile was zeroed: the three bytes past cell 120 stay 0) */
        const int e = pom_cell_encode(st[c], c);
        bad |= e < 0;
        pom_rec_set_cell(tile, POM_TILE_ENVS, c, e & 0xFF);
    }
    if (lane == POM_LANE_SCALARS) tile[POM_REC_TIMESTEP * POM_TILE_ENVS] = pom_pack_timestep(st);
    if (lane < POM_AGENT_COUNT)
        bad |= pom_pack_agent(st, lane, tile[(POM_REC_AGENTS + 2 * lane) * POM_TILE_ENVS], tile[(POM_REC_AGENTS + 2 * lane + 1) * POM_TILE_ENVS]);
    if (lane >= POM_LANE_BOMBS && lane < POM_LANE_BOMBS + POM_MAX_BOMBS) {
        const int k = lane - POM_LANE_BOMBS;
        tile[(POM_REC_BOMBS + k) * POM_TILE_ENVS] = pom_pack_bomb(st, k);
        bad |= pom_pack_live_bomb_bad(st, k);
    }
    if (lane >= POM_LANE_FLAMES && lane < POM_LANE_FLAMES + POM_MAX_BOMBS)
        bad |= pom_pack_flame(st, lane - POM_LANE_FLAMES, tile[(POM_REC_FLAMES + lane - POM_LANE_FLAMES) * POM_TILE_ENVS]);
    return bad;
}
POM_HD void pom_unpack_lane(const uint32_t* tile, int32_t* st, int lane)
{
    for (int c = lane; c < POM_CELLS; c += 64) st[c] = pom_cell_decode(pom_rec_cell(tile, POM_TILE_ENVS, c), c);
    if (lane == POM_LANE_SCALARS) pom_unpack_timestep(tile[POM_REC_TIMESTEP * POM_TILE_ENVS], st);
    if (lane < POM_AGENT_COUNT)
        pom_unpack_agent(tile[(POM_REC_AGENTS + 2 * lane) * POM_TILE_ENVS], tile[(POM_REC_AGENTS + 2 * lane + 1) * POM_TILE_ENVS], st, lane);
    if (lane >= POM_LANE_BOMBS && lane < POM_LANE_BOMBS + POM_MAX_BOMBS)
        pom_unpack_bomb(tile[(POM_REC_BOMBS + lane - POM_LANE_BOMBS) * POM_TILE_ENVS], st, lane - POM_LANE_BOMBS);
    if (lane >= POM_LANE_FLAMES && lane < POM_LANE_FLAMES + POM_MAX_BOMBS)
        pom_unpack_flame(tile[(POM_REC_FLAMES + lane - POM_LANE_FLAMES) * POM_TILE_ENVS], st, lane - POM_LANE_FLAMES);
}

/* Chained launches (pom_chain.h): the tile words count visits in 28-bit fields (tickets in bits 63..36, stored visits in 27..0) and
 * are zeroed before either reaches 2^27.  A visit's distance from the first visit of the call whose launch it rides in is SIGNED:
 * launches of two calls can be in flight together, and a wavefront of the later call may draw a ticket of the earlier one.
 * Bit 28 (POM_CHAIN_POISON): a visitor could not play its tick (it waited out its time limit for the visit before it, or found
 * the tile stored through another XCD's L2).  Nobody steps a poisoned tile: its stored count stays at the number of ticks it
 * really played, and the host replays the rest after the next join (pom_chain_host.h chain_settle). */
enum { POM_CHAIN_TICKET_SHIFT = 36, POM_CHAIN_COUNT_MASK = 0x0FFFFFFF, POM_CHAIN_POISON = 0x10000000 };
/* failure flags of chained launches (a device word, read back by chain_settle) */
enum { POM_CHAIN_E_TIMEOUT = 1, POM_CHAIN_E_XCD = 2, POM_CHAIN_E_UNEVEN = 4, POM_CHAIN_E_TAPE = 8 };
POM_HD uint32_t pom_chain_visit_distance(uint32_t visit, uint32_t first_visit_of_call)
{
    return (uint32_t)((int32_t)((visit - first_visit_of_call) << 4) >> 4);
}

#endif /* POM_PACKED_H_ */
