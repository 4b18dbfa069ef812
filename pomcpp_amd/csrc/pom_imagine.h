/*
 * pom_imagine.h — pom_batch_imagine's kernel (include/pom_batch.h PomImagineSpec, where THE RULE is stated): env first + j becomes a
 * playable game built from one agent's view memory and a seeded draw for what that agent never saw, in ONE launch.  The inverse of the
 * code-plane export plus a sampler.
 *
 * The rule is two functions, POM_HD so that the same source is checked on the host against the numpy checker (tests/emul/
 * pom_imagine_emul.cpp, tests/imagine_oracle.py).  Both work on the job's column of a tile in its by-cell layout — the record is built
 * where it will leave from, and the queues under construction live in their own rows of that column, so nothing needs an array of
 * registers or scratch memory:
 *   pom_imagine_cell    per cell, no cell depends on another: clauses 1 - 3 — what the cell is, the draw for an unknown cell and for a
 *                       wood's flag.  Bombs are written as Item::BOMB (also under an agent code: agents are put on last), flame pieces
 *                       as the mark POM_IMG_PIECE, which is no code a finished record holds.
 *   pom_imagine_finish  per job, in sequence: clauses 4 - 8 — the bomb queue by insertion into rows 40..59, the owners, the flames cut
 *                       out of the marked pieces in cell order and inserted into rows 60..79, the viewer, the others, the agent words.
 * The cell codes and the agent words come from pom_packed.h's encoders (pom_cell_encode, pom_pack_agent): the State <-> record mapping
 * stays written there.
 *
 * The kernel: one wavefront per DESTINATION tile, a quad of lanes per job, as pom_expand_kernel.
 *   1  the list's entries, then the destination tile into LDS as it stands (load_tile16_x4);
 *   2  the views: a view is 726 bytes and starts on an even byte, so it is read as the 182 aligned dwords that cover it, 64 consecutive
 *      dwords a round by the whole wavefront, eight jobs' rounds in flight at a time, into an LDS area of 183 dwords a job.  No byte is
 *      loaded from global memory;
 *   3  pom_imagine_cell: the quad's lanes take the cells member, member + 4, ... and write the codes over the job's column;
 *   4  pom_imagine_finish by the quad's first lane;
 *   5  a refused job (POM_IMAGINE_NO_ROOM) gets its column back from the batch, which still holds it;
 *   6  the built records as dense snapshot records, and fresh agent memory, by the quad;
 *   7  the whole tile out (store_tile16_x4) — every column that is no built destination leaves as it came — and the result words.
 * LDS: 5,120 B (tile) + 11,712 B (16 views).  No scratch memory.
 */
#ifndef POM_IMAGINE_H_
#define POM_IMAGINE_H_

#include <stdint.h>

#include "pom_batch.h"
#include "pom_boardgen.h"
#include "pom_packed.h"

enum {
    POM_IMG_CELLS = 121,
    POM_IMG_VIEW_BYTES = POM_MEMORY_PLANES * POM_IMG_CELLS, /* 726 */
    POM_IMG_VIEW_DWORDS = (POM_IMG_VIEW_BYTES + 2 + 3) / 4,  /* 182: a view starts on byte 0 or 2 of its first dword */
    POM_IMG_VIEW_STRIDE = POM_IMG_VIEW_DWORDS + 1,          /* an odd number of dwords between two jobs' views in LDS */
    POM_IMG_STRENGTH = 1 * POM_IMG_CELLS, POM_IMG_LIFE = 2 * POM_IMG_CELLS, POM_IMG_DIR = 3 * POM_IMG_CELLS, /* the planes of a view */
    POM_IMG_FLAME = 4 * POM_IMG_CELLS, POM_IMG_AGE = 5 * POM_IMG_CELLS,
    POM_IMG_PIECE = 255,                                    /* a flame piece not yet taken by a flame */
    POM_IMG_DRAW_FLAG = 128, POM_IMG_DRAW_AGENT = 256,      /* draw indices: the cell kinds are 0..120 */
};

POM_HD uint32_t pom_imagine_key(uint64_t seed, int32_t view, int32_t sample) { return pom_board_key(seed, (uint32_t)view, (uint32_t)sample); }
POM_HD int pom_imagine_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }
/* clause 1: is the cell known */
POM_HD int pom_imagine_known(int b, int age) { return (int)(age != POM_MEMORY_AGE_NEVER) & ((int)(b <= 4) | ((int)(b >= 6) & (int)(b <= 8)) | ((int)(b >= 10) & (int)(b <= 13))); }
/* clause 6: the cell a live viewer stands on, or -1 */
POM_HD int pom_imagine_viewer_cell(const int32_t* attrs)
{
    return attrs[2] != 0 ? pom_imagine_clamp(attrs[1], 0, POM_BOARD_SIZE - 1) * POM_BOARD_SIZE + pom_imagine_clamp(attrs[0], 0, POM_BOARD_SIZE - 1) : -1;
}

/* Clauses 1 - 3 for cell c: the code the cell gets before the queues are built; unknown = 1 if the cell is not known.  view: the 726
 * bytes; vc: pom_imagine_viewer_cell */
POM_HD int pom_imagine_cell(const uint8_t* view, int c, uint32_t key, int unknown_mode, int vc, int& unknown)
{
    const int b = view[c];
    const int known = pom_imagine_known(b, view[POM_IMG_AGE + c]);
    unknown = !known;
    int kind = b;
    if (!known) {
        const uint32_t t = unknown_mode == POM_IMAGINE_SAMPLE ? pom_mulhi32(pom_board_draw(key, (uint32_t)c), 7u) : 0u;
        kind = t == 1u ? 1 : t == 2u ? 2 : 0;
    }
    if (c == vc) return POM_C_PASSAGE; /* (the viewer is put there by pom_imagine_finish) */
    if (kind == 3 || kind >= 10) return view[POM_IMG_LIFE + c] > 0 ? pom_cell_encode(POM_BOMB, c) : (int)POM_C_PASSAGE;
    if (kind == 4) return view[POM_IMG_FLAME + c] > 0 ? (int)POM_IMG_PIECE : (int)POM_C_PASSAGE;
    if (kind == 2) {
        const uint32_t d = pom_board_draw(key, (uint32_t)(POM_IMG_DRAW_FLAG + c));
        return pom_cell_encode(POM_WOOD + ((d >> 31) ? 1 + (int32_t)((d >> 29) & 3u) : 0), c);
    }
    if (kind >= 6) return pom_cell_encode(POM_EXTRABOMB + (kind - 6), c);
    return kind == 1 ? pom_cell_encode(POM_RIGID, c) : (int)POM_C_PASSAGE;
}

/* a dropped flame's cells back to passage: the origin and its two arms carry the origin's code and nothing else does */
POM_HD void pom_imagine_clear_flame(uint8_t* cells, int o)
{
    const int code = pom_cell_encode(POM_FLAMES + (o << 3), o), x = o % POM_BOARD_SIZE;
    cells[o * POM_TILE_ENVS] = POM_C_PASSAGE;
    for (int i = 1; x + i < POM_BOARD_SIZE && cells[(o + i) * POM_TILE_ENVS] == code; i++) cells[(o + i) * POM_TILE_ENVS] = POM_C_PASSAGE;
    for (int cc = o + POM_BOARD_SIZE; cc < POM_IMG_CELLS && cells[cc * POM_TILE_ENVS] == code; cc += POM_BOARD_SIZE) cells[cc * POM_TILE_ENVS] = POM_C_PASSAGE;
}

/* Clauses 4 - 8 over the column `ec` of `tile` that pom_imagine_cell has filled: returns the result word.  POM_IMAGINE_NO_ROOM: the
 * column holds neither the old record nor a new one.  attrs: the viewer's 12; belief: its 4 x 3, or null; v: the viewer; unknown_cells:
 * the sum of pom_imagine_cell's `unknown` */
POM_HD uint32_t pom_imagine_finish(const uint8_t* view, uint32_t* tile, int ec, const int32_t* attrs, const int32_t* belief, int v, uint32_t key,
                                   int unknown_cells)
{
    uint8_t* const cells = reinterpret_cast<uint8_t*>(tile) + ec; /* cell c: cells[c * 16] */
    uint32_t* const bombs = tile + POM_REC_BOMBS * POM_TILE_ENVS + ec; /* slot k: bombs[k * 16] */
    uint32_t* const flames = tile + POM_REC_FLAMES * POM_TILE_ENVS + ec;
    const int bomb_code = pom_cell_encode(POM_BOMB, 0);
    uint32_t word = POM_IMAGINE_BUILT;
    const int alive_v = attrs[2] != 0, vc = pom_imagine_viewer_cell(attrs);
    uint32_t alive_mask = alive_v ? 1u << v : 0u;
    for (int k = 1; k < 4; k++) alive_mask |= attrs[7 + k] != 0 ? 1u << ((v + k) & 3) : 0u;
    const uint32_t others = alive_mask & ~(1u << v);

    /* clause 4: the bombs, inserted by (time, cell); the cells come in ascending order, so an equal time goes behind */
    int nb = 0;
    for (int c = 0; c < POM_IMG_CELLS; c++) {
        const int b = view[c], life = view[POM_IMG_LIFE + c];
        if (!pom_imagine_known(b, view[POM_IMG_AGE + c]) || !(b == 3 || b >= 10) || life == 0) continue;
        const int time = life > 15 ? 15 : life, st = view[POM_IMG_STRENGTH + c], dir = view[POM_IMG_DIR + c];
        const int y = c / POM_BOARD_SIZE, x = c - y * POM_BOARD_SIZE;
        const uint32_t w = (uint32_t)x | ((uint32_t)y << 4) | ((uint32_t)(st > 15 ? 15 : st) << 12) | ((uint32_t)time << 16) | ((uint32_t)(dir > 4 ? 0 : dir) << 20);
        int i = nb;
        while (i > 0 && (int)((bombs[(i - 1) * POM_TILE_ENVS] >> 16) & 15u) > time) i--;
        if (nb == POM_MAX_BOMBS) {
            word |= POM_IMAGINE_DROPPED_BOMBS;
            const uint32_t out = i == POM_MAX_BOMBS ? w : bombs[(POM_MAX_BOMBS - 1) * POM_TILE_ENVS];
            const int oc = (int)((out >> 4) & 15u) * POM_BOARD_SIZE + (int)(out & 15u);
            if (cells[oc * POM_TILE_ENVS] == bomb_code) cells[oc * POM_TILE_ENVS] = POM_C_PASSAGE;
            if (i == POM_MAX_BOMBS) continue;
            nb = POM_MAX_BOMBS - 1;
        }
        for (int k = nb; k > i; k--) bombs[k * POM_TILE_ENVS] = bombs[(k - 1) * POM_TILE_ENVS];
        bombs[i * POM_TILE_ENVS] = w;
        nb++;
    }
    /* the owners: the viewer's bombCount first, the rest round-robin over the other live agents; given: a byte per agent */
    uint32_t given = 0;
    {
        const int mine = pom_imagine_clamp(attrs[4], 0, nb);
        int cur = 3;
        for (int k = 0; k < nb; k++) {
            int owner = v;
            if (k >= mine && others) {
                do cur = (cur + 1) & 3; while (!((others >> cur) & 1u));
                owner = cur;
                given += 1u << (8 * owner);
            }
            bombs[k * POM_TILE_ENVS] |= (uint32_t)owner << 8;
        }
    }
    for (int k = nb; k < POM_MAX_BOMBS; k++) bombs[k * POM_TILE_ENVS] = 0;

    /* clause 5: the flames, cut out of the marked pieces in cell order and inserted by (timeLeft, origin) */
    int nf = 0;
    for (int c = 0; c < POM_IMG_CELLS; c++) {
        if (cells[c * POM_TILE_ENVS] != POM_IMG_PIECE) continue;
        const int fl = view[POM_IMG_FLAME + c], L = fl > 127 ? 127 : fl;
        const int y = c / POM_BOARD_SIZE, x = c - y * POM_BOARD_SIZE, code = pom_cell_encode(POM_FLAMES + (c << 3), c);
        int ax = 0, ay = 0;
        cells[c * POM_TILE_ENVS] = (uint8_t)code;
        for (int cc = c + 1; x + ax + 1 < POM_BOARD_SIZE && cells[cc * POM_TILE_ENVS] == POM_IMG_PIECE; cc++) {
            const int f2 = view[POM_IMG_FLAME + cc];
            if ((f2 > 127 ? 127 : f2) != L) break;
            cells[cc * POM_TILE_ENVS] = (uint8_t)code;
            ax++;
        }
        for (int cc = c + POM_BOARD_SIZE; cc < POM_IMG_CELLS && cells[cc * POM_TILE_ENVS] == POM_IMG_PIECE; cc += POM_BOARD_SIZE) {
            const int f2 = view[POM_IMG_FLAME + cc];
            if ((f2 > 127 ? 127 : f2) != L) break;
            cells[cc * POM_TILE_ENVS] = (uint8_t)code;
            ay++;
        }
        /* (pom_pack_flame's word: x | y << 8 | timeLeft << 16 | strength << 24) */
        const uint32_t w = (uint32_t)x | ((uint32_t)y << 8) | ((uint32_t)L << 16) | ((uint32_t)(ax > ay ? ax : ay) << 24);
        int i = nf;
        while (i > 0 && (int)((flames[(i - 1) * POM_TILE_ENVS] >> 16) & 255u) > L) i--;
        if (nf == POM_MAX_BOMBS) {
            word |= POM_IMAGINE_DROPPED_FLAMES;
            const uint32_t out = i == POM_MAX_BOMBS ? w : flames[(POM_MAX_BOMBS - 1) * POM_TILE_ENVS];
            pom_imagine_clear_flame(cells, (int)((out >> 8) & 255u) * POM_BOARD_SIZE + (int)(out & 255u));
            if (i == POM_MAX_BOMBS) continue;
            nf = POM_MAX_BOMBS - 1;
        }
        for (int k = nf; k > i; k--) flames[k * POM_TILE_ENVS] = flames[(k - 1) * POM_TILE_ENVS];
        flames[i * POM_TILE_ENVS] = w;
        nf++;
    }
    for (int k = nf; k < POM_MAX_BOMBS; k++) flames[k * POM_TILE_ENVS] = 0;

    /* clauses 6 and 7: the viewer, the remembered others, the drawn others; pos: a byte per agent, 255 = nowhere yet */
    uint32_t pos = 0xFFFFFFFFu, drawn = 0;
    if (alive_v) cells[vc * POM_TILE_ENVS] = (uint8_t)pom_cell_encode(POM_AGENT0 + v, vc);
    for (int c = 0; c < POM_IMG_CELLS; c++) {
        const int b = view[c];
        if (!pom_imagine_known(b, view[POM_IMG_AGE + c]) || b < 10 || c == vc) continue;
        const int a = b - 10;
        if (!((others >> a) & 1u) || ((pos >> (8 * a)) & 255u) != 255u) continue;
        pos = (pos & ~(255u << (8 * a))) | ((uint32_t)c << (8 * a));
        cells[c * POM_TILE_ENVS] = (uint8_t)pom_cell_encode(POM_AGENT0 + a, c);
    }
    for (int a = 0; a < POM_AGENT_COUNT; a++) {
        if (!((others >> a) & 1u) || ((pos >> (8 * a)) & 255u) != 255u) continue;
        int n1 = 0, n2 = 0;
        for (int c = 0; c < POM_IMG_CELLS; c++) {
            const int free_cell = cells[c * POM_TILE_ENVS] == POM_C_PASSAGE;
            n2 += free_cell;
            n1 += free_cell & (int)(view[POM_IMG_AGE + c] != 0);
        }
        if (n2 == 0) return POM_IMAGINE_NO_ROOM;
        const int unseen_only = n1 != 0;
        int k = (int)pom_mulhi32(pom_board_draw(key, (uint32_t)(POM_IMG_DRAW_AGENT + a)), (uint32_t)(unseen_only ? n1 : n2));
        int at = 0;
        for (int c = 0; c < POM_IMG_CELLS; c++) {
            if (cells[c * POM_TILE_ENVS] != POM_C_PASSAGE || (unseen_only && view[POM_IMG_AGE + c] == 0)) continue;
            if (k-- == 0) {
                at = c;
                break;
            }
        }
        pos = (pos & ~(255u << (8 * a))) | ((uint32_t)at << (8 * a));
        cells[at * POM_TILE_ENVS] = (uint8_t)pom_cell_encode(POM_AGENT0 + a, at);
        drawn |= 1u << a;
    }

    /* clause 8 and the agent words, through the State's fields and pom_packed.h's packer */
    int32_t st[POM_STATE_BYTES / 4];
    st[121] = attrs[11];
    st[122] = (int32_t)__builtin_popcount(alive_mask);
    st[167] = 0;
    st[168] = nb;
    st[249] = 0;
    st[250] = nf;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < POM_AGENT_COUNT; i++) {
        int32_t* a = st + 123 + 6 * i;
        const int me = i == v, alive = (int)((alive_mask >> i) & 1u), p = (int)((pos >> (8 * i)) & 255u), bc = (int)((given >> (8 * i)) & 255u);
        const int mx = belief ? pom_imagine_clamp(belief[3 * i], 0, POM_PACK_MAXBOMBS_MAX) : 1;
        a[0] = me ? pom_imagine_clamp(attrs[0], 0, POM_BOARD_SIZE - 1) : alive ? p % POM_BOARD_SIZE : 0;
        a[1] = me ? pom_imagine_clamp(attrs[1], 0, POM_BOARD_SIZE - 1) : alive ? p / POM_BOARD_SIZE : 0;
        a[2] = me ? pom_imagine_clamp(attrs[4], POM_PACK_BOMBCOUNT_MIN, POM_PACK_BOMBCOUNT_MAX) : bc;
        a[3] = me ? pom_imagine_clamp(attrs[5], -32768, POM_PACK_MAXBOMBS_MAX) : mx > bc ? mx : bc;
        a[4] = me ? pom_imagine_clamp(attrs[6], 0, POM_PACK_STRENGTH_MAX) : belief ? pom_imagine_clamp(belief[3 * i + 1], 0, POM_PACK_STRENGTH_MAX) : 1;
        a[5] = (int32_t)((me ? attrs[7] != 0 : belief ? belief[3 * i + 2] != 0 : 0) ? 1u : 0u) | (alive ? 0 : 0x100);
        pom_pack_agent(st, i, tile[(POM_REC_AGENTS + 2 * i) * POM_TILE_ENVS + ec], tile[(POM_REC_AGENTS + 2 * i + 1) * POM_TILE_ENVS + ec]);
    }
    tile[POM_REC_TIMESTEP * POM_TILE_ENVS + ec] = pom_pack_timestep(st);
    return word | ((uint32_t)unknown_cells << POM_IMAGINE_UNKNOWN_SHIFT) | (drawn << POM_IMAGINE_DRAWN_SHIFT);
}

#if defined(__HIPCC__) /* ---- the kernel ---- */

#include "pom_device.h"

struct ImagineParams {
    uint32_t* state;
    uint32_t* snap;              /* [n_pad][80], dense records */
    uint32_t* agent_mem;         /* [2][4 * n_pad] or nullptr */
    const int32_t* view;         /* [count] */
    const int32_t* sample;       /* [count] or nullptr */
    const uint32_t* memory;      /* uint8 [rows][726] as dwords */
    const int32_t* viewer_attrs; /* [rows][12] */
    const int32_t* belief;       /* [rows][12] or nullptr */
    uint32_t* result;            /* [count] or nullptr */
    int64_t first, count, n_pad, tile0;
    uint64_t seed;
    int32_t rows, unknown;
};

__global__ __launch_bounds__(64, 4) void pom_imagine_kernel(ImagineParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POM_REC_DWORDS * 16];
    __shared__ uint32_t views[16 * POM_IMG_VIEW_STRIDE];
    const int lane = threadIdx.x;
    const int64_t tile_id = p.tile0 + pom_xcd_tile_order(blockIdx.x, gridDim.x);
    const int ec = lane >> 2, member = lane & 3;
    const int64_t d = tile_id * 16 + ec, j = d - p.first;
    const bool in_range = j >= 0 && j < p.count;
    int view = in_range ? p.view[j] : -1;
    const bool job = view >= 0 && view < p.rows;
    view = job ? view : -1;
    const int sample = job ? (p.sample ? p.sample[j] : (int)j) : 0;
    load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    /* the views: eight jobs' 182 dwords in flight at a time (24 loads a lane), then into the area */
#pragma unroll
    for (int half = 0; half < 2; half++) {
        uint32_t r[8][3];
#pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            const int vj = __builtin_amdgcn_readlane(view, 4 * (8 * half + jj));
            if (vj >= 0) {
                const uint32_t* src = p.memory + (((int64_t)vj * POM_IMG_VIEW_BYTES) >> 2) + lane;
                r[jj][0] = src[0];
                r[jj][1] = src[64];
                r[jj][2] = lane + 128 < POM_IMG_VIEW_DWORDS ? src[128] : 0u;
            }
        }
#pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            const int vj = __builtin_amdgcn_readlane(view, 4 * (8 * half + jj));
            if (vj >= 0) {
                uint32_t* dst = views + (8 * half + jj) * POM_IMG_VIEW_STRIDE + lane;
                dst[0] = r[jj][0];
                dst[64] = r[jj][1];
                if (lane + 128 < POM_IMG_VIEW_DWORDS) dst[128] = r[jj][2];
            }
        }
    }
    /* the destination tile's DMA rows have landed (one wavefront per workgroup: no barrier) — before any column is written over */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    const uint8_t* const view_b = reinterpret_cast<const uint8_t*>(views + ec * POM_IMG_VIEW_STRIDE) + 2 * (view & 1); /* 726 * view mod 4 */
    const int32_t* const attrs = p.viewer_attrs + (int64_t)view * POM_OBS_VIEWER_ATTRS;
    const uint32_t key = pom_imagine_key(p.seed, view, sample);
    int unknown_cells = 0;
    if (job) {
        const int vc = pom_imagine_viewer_cell(attrs);
        uint8_t* const cells = reinterpret_cast<uint8_t*>(tile) + ec;
        POM_NOUNROLL
        for (int c = member; c < POM_IMG_CELLS; c += 4) {
            int u;
            cells[c * POM_TILE_ENVS] = (uint8_t)pom_imagine_cell(view_b, c, key, p.unknown, vc, u);
            unknown_cells += u;
        }
    }
    unknown_cells += __shfl_xor(unknown_cells, 1);
    unknown_cells += __shfl_xor(unknown_cells, 2);
    asm volatile("" ::: "memory"); /* the quad's other lanes wrote cells the first lane reads now */
    uint32_t word = 0;
    if (job && member == 0)
        word = pom_imagine_finish(view_b, tile, ec, attrs, p.belief ? p.belief + (int64_t)view * 12 : nullptr, view & 3, key, unknown_cells);
    word = (uint32_t)__shfl((int)word, lane & ~3);
    asm volatile("" ::: "memory");
    const bool built = job && (word & POM_IMAGINE_BUILT);
    if (job && !built) { /* refused: the column as the batch still holds it */
        const uint32_t* const src_tile = p.state + tile_id * POM_TILE_DWORDS;
        for (int k = member; k < POM_COL_ITEMS; k += 4) pom_col_copy_item(tile, ec, src_tile, ec, k);
    }
    asm volatile("" ::: "memory");
    if (built) {
        /* the restart snapshot: the dense record (cell c in byte c & 3 of dword c >> 2; status and ubflags are clear as built) */
        uint32_t* const rec = p.snap + d * POM_REC_DWORDS;
        const uint8_t* const cells = reinterpret_cast<const uint8_t*>(tile) + ec;
        POM_NOUNROLL
        for (int dw = member; dw < POM_REC_DWORDS; dw += 4) {
            uint32_t w;
            if (dw < POM_REC_BOARD_DWORDS)
                w = (uint32_t)cells[(4 * dw) * POM_TILE_ENVS] | ((uint32_t)cells[(4 * dw + 1) * POM_TILE_ENVS] << 8) |
                    ((uint32_t)cells[(4 * dw + 2) * POM_TILE_ENVS] << 16) | ((uint32_t)cells[(4 * dw + 3) * POM_TILE_ENVS] << 24);
            else w = tile[dw * POM_TILE_ENVS + ec];
            rec[dw] = w;
        }
        if (p.agent_mem) { /* a new game: fresh agents */
            p.agent_mem[d * 4 + member] = 0;
            p.agent_mem[4 * p.n_pad + d * 4 + member] = 0;
        }
    }
    if (__any(built)) store_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    if (p.result && in_range && member == 0) p.result[j] = word;
}

#endif /* __HIPCC__ */

#endif /* POM_IMAGINE_H_ */
