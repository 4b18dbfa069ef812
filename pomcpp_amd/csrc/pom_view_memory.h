/*
 * pom_view_memory.h — pom_batch_remember_view's kernel (include/pom_batch.h PomMemorySpec, where THE RULE is stated): every asked
 * agent's fogged view merged into what that agent remembers — uint8 [n][4][6][11][11], the five code planes and an age plane —
 * in ONE launch for a range of whole tiles, the batch untouched.
 *
 * The rule is per cell: a cell's new six bytes depend on its own old six, on the five bytes the export writes for it now, on whether
 * the viewer's window shows it, and on three things that are the same for the whole view (wipe, dt, which agents the viewer knows
 * to be elsewhere or dead).  pom_view_memory_cell below is that function and nothing else; it and the view's head
 * (pom_view_memory_head, pom_view_memory_gone) are POM_HD, so that the same source is checked on the host against the numpy checker
 * (tests/emul/pom_view_memory_emul.cpp, tests/test_view_memory_host.py).
 *
 * Work split: FOUR wavefronts per tile of 16 envs, one per pass of four envs that the export stages at a time (POM_MEM_SPLIT; with one
 * wavefront per tile, the export's split, 65,536 envs are one round of 4,096 wavefronts that each walk 16 envs one after the other:
 * 148 us against 123, profiles/view_memory_bench.txt).  The grid is the rollouts': the tiles rounded up to a multiple of 8, a tile's four
 * workgroups eight apart and so on one XCD, whose L2 serves the tile's record to three of them.  The whole tile comes into LDS with the
 * tick's loader (pom_observe_stage addresses it by env column); the five code planes of the wavefront's four envs are staged once by
 * pom_observe_stage<true>, as pom_observe_tile_codes_view stages them.  Then env by env:
 *   in    the env's four views are 4 x 726 B = 726 dwords, so every env starts on a dword: they are read as 12 rounds of 64 consecutive
 *         dwords into registers — one env AHEAD, while the env before is merged, so that the loads' latency is covered by the merge — and
 *         put into a 2,904-byte LDS area.  No byte is loaded from global memory: planes are 121 bytes, views 726, neither a multiple of 4.
 *   merge per view of the mask, two rounds of 64 lanes over the 121 cells: a lane reads its cell's six old bytes from the area and five
 *         staged bytes, applies pom_view_memory_cell and writes six bytes back in place (a cell depends on no other cell).
 *   out   the area leaves as the 726 dwords it came as, but for the dwords that lie wholly in views outside the mask, which are not
 *         written.  A dword that straddles two views (726 = 4 x 181 + 2) is written if either is in the mask, the other view's two
 *         bytes as they were read.
 * The stamps: lane -> (env lane / 4, view lane % 4), read as one 8-byte load per lane before the loop, written after it; the loop takes
 * a view's wipe and dt from that lane (v_readlane: the env and the view are wavefront-uniform).
 * LDS: 5,120 (tile) + 2,448 (code planes of four envs) + 2,912 (one env's views) = 10,480 B.  No scratch memory.
 */
#ifndef POM_VIEW_MEMORY_H_
#define POM_VIEW_MEMORY_H_

#include <stdint.h>

#include "pom_batch.h"
#include "pom_rng.h" /* POM_HD */

enum {
    POM_MEM_BOARD = 0, POM_MEM_STRENGTH = 1, POM_MEM_LIFE = 2, POM_MEM_DIR = 3, POM_MEM_FLAME = 4, POM_MEM_AGE = 5, /* the planes */
    POM_MEM_CELLS = 121,
    POM_MEM_VIEW_BYTES = POM_MEMORY_PLANES * POM_MEM_CELLS, /* 726 */
    POM_MEM_ENV_DWORDS = POM_MEM_VIEW_BYTES,                /* four views: 4 x 726 B = 726 dwords */
    POM_MEM_FOG = 5, POM_MEM_BOMB = 3, POM_MEM_FLAMES = 4, POM_MEM_AGENT0 = 10, /* board codes (POM_OBS_CODES) */
};

/* ---- THE RULE's pieces, for the device and for the host (tests/emul/pom_view_memory_emul.cpp) ---- */

/* Step 1's decision for one view: (ep, t) the env's episode counter and timeStep now, (ep0, t0) the view's stamp.  wipe: a new game,
 * no memory yet (ep0 = -1) or a batch put back to an earlier state; otherwise dt = min(t - t0, 255) */
POM_HD void pom_view_memory_head(uint32_t ep, int32_t t, int32_t ep0, int32_t t0, int& wipe, int& dt)
{
    wipe = (int)((uint32_t)ep0 != ep) | (int)(t < t0);
    const uint32_t d = (uint32_t)t - (uint32_t)t0; /* t >= t0 where it is used: the true difference */
    dt = wipe ? 0 : (int)(d > 255u ? 255u : d);
}

/* Is agent (x, y, dead) "gone" for a viewer with window w (obs_window's word: bits 0..10 the columns, 16..26 the rows it shows): dead
 * by the public flags, or seen where it stands now — a remembered sighting of it anywhere outside the window is stale.  x, y: 0..15 */
POM_HD uint32_t pom_view_memory_gone(uint32_t w, int x, int y, int dead) { return (uint32_t)(dead != 0) | (((w >> x) & (w >> (16 + y))) & 1u); }

/* One cell of one view.  m[0..5]: the remembered bytes (POM_MEM_*), in and out; now[0..4]: the bytes pom_batch_observe(POM_OBS_CODES)
 * writes for the cell at this tick; inside: the viewer's window shows the cell; gone: bit a = pom_view_memory_gone of agent a.
 * Written with selects, not branches: `inside` varies from lane to lane. */
POM_HD void pom_view_memory_cell(int (&m)[POM_MEMORY_PLANES], const int (&now)[POM_OBS_CODE_PLANES], int inside, int wipe, int dt, uint32_t gone)
{
    /* steps 1.1 - 1.5 on a cell outside the window of a view that is not wiped; a never-seen cell and dt = 0 change nothing */
    const int ages = (int)(dt != 0) & (int)(m[POM_MEM_AGE] != 255);
    int board = m[POM_MEM_BOARD];
    /* 1.2 a remembered bomb counts down; at 0 it is forgotten, an agent code standing on it stays */
    int life = m[POM_MEM_LIFE] - dt;
    life = life < 0 ? 0 : life;
    const int bomb_out = (int)(m[POM_MEM_LIFE] > 0) & (int)(life == 0);
    const int strength = bomb_out ? 0 : m[POM_MEM_STRENGTH], dir = bomb_out ? 0 : m[POM_MEM_DIR];
    board = (bomb_out & (int)(board == POM_MEM_BOMB)) ? 0 : board;
    /* 1.3 a remembered flame counts down; at 0 the cell is passage */
    const int is_flame = board == POM_MEM_FLAMES;
    int fl = m[POM_MEM_FLAME] - dt;
    fl = fl < 0 ? 0 : fl;
    const int flame = is_flame ? fl : m[POM_MEM_FLAME];
    board = (is_flame & (int)(fl == 0)) ? 0 : board;
    /* 1.4 a stale agent leaves the bomb it stood on, if that still ticks, or passage */
    const uint32_t a = (uint32_t)(board - POM_MEM_AGENT0);
    const int stale = (int)(a < 4u) & (int)((gone >> (a & 3u)) & 1u);
    board = stale ? (life > 0 ? POM_MEM_BOMB : 0) : board;
    /* 1.5 */
    int age = m[POM_MEM_AGE] + dt;
    age = age > 254 ? 254 : age;
    const int aged[POM_MEMORY_PLANES] = {board, strength, life, dir, flame, age};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < POM_MEMORY_PLANES; i++) {
        const int fogged = wipe ? (i == POM_MEM_BOARD ? POM_MEM_FOG : i == POM_MEM_AGE ? 255 : 0) : ages ? aged[i] : m[i];
        m[i] = inside ? (i == POM_MEM_AGE ? 0 : now[i < POM_OBS_CODE_PLANES ? i : 0]) : fogged; /* step 2: the window, verbatim, age 0 */
    }
}

#if defined(__HIPCC__) /* ---- the kernel ---- */

#include "pom_device.h"

struct ViewMemoryParams {
    const uint32_t* state;
    const uint32_t* episode; /* [n_pad]: what pom_batch_episodes reports */
    uint32_t* memory;        /* uint8 [n][4][6][121] as dwords: 726 per env */
    int32_t* stamp;          /* int32 [n][4][2] */
    int32_t* viewer_attrs;   /* nullable, as ObserveParams */
    int32_t* env_attrs;      /* nullable */
    int64_t n, block0;
    int32_t view_radius, agent_mask;
    uint32_t tiles, tiles8; /* tiles of the range; the same rounded up to a multiple of 8: the grid is POM_MEM_SPLIT * tiles8 */
};

enum { POM_MEM_ROUNDS = (POM_MEM_ENV_DWORDS + 63) / 64 }; /* 12 rounds of 64 dwords, the last one of 22 */
enum { POM_MEM_SPLIT = 16 / OBS_CODE_PASS_ENVS };         /* wavefronts per tile: one per staged pass of four envs */
static_assert(POM_MEM_CELLS == POM_CELLS && POM_MEMORY_PLANES == OBS_CODE_PLANES + 1, "the code planes and an age plane");
static_assert(4 * POM_MEM_VIEW_BYTES == 4 * POM_MEM_ENV_DWORDS, "an env's four views are a whole number of dwords");

__global__ __launch_bounds__(64) void pom_view_memory_kernel(ViewMemoryParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POM_REC_DWORDS * 16];
    __shared__ uint4 stage[obs_stage_vecs(1)];
    __shared__ __attribute__((aligned(16))) uint32_t area[POM_MEM_ENV_DWORDS + 2];
    const int lane = threadIdx.x;
    /* workgroup b runs on XCD b % 8: the POM_MEM_SPLIT wavefronts of a tile are eight workgroups apart, on one XCD — its L2 serves the
     * tile's record to the second, third and fourth of them */
    const uint32_t j = blockIdx.x >> 3, q = j % POM_MEM_SPLIT, slot = (j / POM_MEM_SPLIT) * 8u + (blockIdx.x & 7u);
    if (slot >= p.tiles) return; /* a workgroup of the padding */
    const int64_t tile_id = p.block0 + pom_xcd_tile_order(slot, p.tiles);
    const int64_t e0 = tile_id * 16;
    const int ec0 = (int)q * OBS_CODE_PASS_ENVS; /* this wavefront's envs: columns ec0 .. envs - 1 of the tile */
    const int envs = p.n - e0 < ec0 + OBS_CODE_PASS_ENVS ? (int)(p.n - e0) : ec0 + OBS_CODE_PASS_ENVS;
    if (ec0 >= envs) return; /* (the batch's last tile is short) */
    load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    /* this lane's view: (env lane / 4, view lane % 4) — its stamp and the env's episode counter */
    const int ec_l = lane >> 2, v_l = lane & 3;
    const bool in_pass = ec_l >= ec0 && ec_l < envs, mine = in_pass && ((p.agent_mask >> v_l) & 1);
    int2* const stamp_l = reinterpret_cast<int2*>(p.stamp) + (e0 + ec_l) * 4 + v_l;
    int2 st0 = make_int2(-1, 0);
    uint32_t ep_l = 0;
    if (mine) {
        st0 = *stamp_l;
        ep_l = p.episode[e0 + ec_l];
    }
    /* which of this lane's dwords of an env leave again: those with a byte in a view of the mask (bit i: round i) */
    uint32_t leaves = 0;
#pragma unroll
    for (int i = 0; i < POM_MEM_ROUNDS; i++) {
        const int b = 4 * (lane + 64 * i), va = b / POM_MEM_VIEW_BYTES, vb = (b + 3) / POM_MEM_VIEW_BYTES;
        if (lane + 64 * i < POM_MEM_ENV_DWORDS && (((p.agent_mask >> va) | (p.agent_mask >> vb)) & 1)) leaves |= 1u << i;
    }
    uint32_t next[POM_MEM_ROUNDS]; /* the env ahead */
    const uint32_t* in = p.memory + (e0 + ec0) * POM_MEM_ENV_DWORDS + lane;
#pragma unroll
    for (int i = 0; i < POM_MEM_ROUNDS; i++) next[i] = (i < POM_MEM_ROUNDS - 1 || lane + 64 * i < POM_MEM_ENV_DWORDS) ? in[64 * i] : 0u;
    /* (the builtin, not inline asm: pom_observe_alone says why) */
    __builtin_amdgcn_s_waitcnt(0x0F70);
    asm volatile("" ::: "memory");
    const int32_t t_l = (int32_t)tile[POM_REC_TIMESTEP * 16 + ec_l];
    int wipe_l, dt_l;
    pom_view_memory_head(ep_l, t_l, st0.x, st0.y, wipe_l, dt_l);
    const int head_l = dt_l | (wipe_l << 8);

    uint8_t* const area_b = reinterpret_cast<uint8_t*>(area);
    const uint8_t* const stage_b = reinterpret_cast<const uint8_t*>(stage);
    pom_observe_stage<true, 1>(tile, stage, (int)q, lane); /* the code planes of envs ec0 .. ec0 + 3 */
    POM_NOUNROLL
    for (int ec = ec0; ec < envs; ec++) {
#pragma unroll
        for (int i = 0; i < POM_MEM_ROUNDS; i++)
            if (i < POM_MEM_ROUNDS - 1 || lane + 64 * i < POM_MEM_ENV_DWORDS) area[lane + 64 * i] = next[i];
        if (ec + 1 < envs) {
            in += POM_MEM_ENV_DWORDS;
#pragma unroll
            for (int i = 0; i < POM_MEM_ROUNDS; i++)
                if (i < POM_MEM_ROUNDS - 1 || lane + 64 * i < POM_MEM_ENV_DWORDS) next[i] = in[64 * i];
        }
        obs_lds_order();
        /* where the four agents are and who is dead: agent_attrs' source (obs_attr_rows) */
        int a0[4];
#pragma unroll
        for (int a = 0; a < 4; a++) a0[a] = (int)tile[(POM_REC_AGENTS + 2 * a) * 16 + ec];
        const uint8_t* const now_b = stage_b + (ec & 3) * OBS_CODE_ENV_BYTES;
        for (int v = 0; v < 4; v++) {
            if (!((p.agent_mask >> v) & 1)) continue;
            const int head = __builtin_amdgcn_readlane(head_l, 4 * ec + v);
            const int wipe = head >> 8, dt = head & 0xFF;
            const uint32_t w = obs_window(tile, ec, v, p.view_radius);
            uint32_t gone = 0;
#pragma unroll
            for (int a = 0; a < 4; a++) gone |= pom_view_memory_gone(w, ag_x(a0[a]), ag_y(a0[a]), ag_dead(a0[a])) << a;
            uint8_t* const view_b = area_b + v * POM_MEM_VIEW_BYTES;
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int c = lane + 64 * i;
                if (i == 0 || c < POM_CELLS) {
                    const int y = (c * 745) >> 13, x = c - POM_N * y; /* c / 11 for c < 121 */
                    const int inside = (int)(((w >> x) & (w >> (16 + y))) & 1u);
                    int m[POM_MEMORY_PLANES], now[OBS_CODE_PLANES];
#pragma unroll
                    for (int k = 0; k < POM_MEMORY_PLANES; k++) m[k] = view_b[k * POM_CELLS + c];
#pragma unroll
                    for (int k = 0; k < OBS_CODE_PLANES; k++) now[k] = now_b[k * POM_CELLS + c];
                    pom_view_memory_cell(m, now, inside, wipe, dt, gone);
#pragma unroll
                    for (int k = 0; k < POM_MEMORY_PLANES; k++) view_b[k * POM_CELLS + c] = (uint8_t)m[k];
                }
            }
        }
        obs_lds_order();
        uint32_t* const out = p.memory + (e0 + ec) * POM_MEM_ENV_DWORDS + lane;
#pragma unroll
        for (int i = 0; i < POM_MEM_ROUNDS; i++)
            if ((leaves >> i) & 1u) out[64 * i] = area[lane + 64 * i];
        obs_lds_order();
    }
    /* step 3 */
    if (mine) *stamp_l = make_int2((int32_t)ep_l, t_l);
    /* viewer_attrs and env_attrs: the rows pom_observe_tile<VIEW> ends with, written a second time here — that tail moved into a function
     * of its own for both to call changes instructions in nine of the step kernels that inline it (compare_kernel_isa.py), and those
     * kernels are kept as measured */
    if (in_pass && p.viewer_attrs) {
        const uint32_t a0 = tile[(POM_REC_AGENTS + 2 * v_l) * 16 + ec_l], a1 = tile[(POM_REC_AGENTS + 2 * v_l + 1) * 16 + ec_l];
        int alive[3];
#pragma unroll
        for (int k = 1; k < 4; k++) alive[k - 1] = !ag_dead((int)tile[(POM_REC_AGENTS + 2 * ((v_l + k) & 3)) * 16 + ec_l]);
        int4* o = reinterpret_cast<int4*>(p.viewer_attrs + ((e0 + ec_l) * 4 + v_l) * POM_OBS_VIEWER_ATTRS);
        obs_attr_rows(o, a0, a1, ag_bombcount((int)a0), ag_max_bombs((int)a1));
        o[2] = make_int4(alive[0], alive[1], alive[2], t_l);
    }
    if (lane >= ec0 && lane < envs && p.env_attrs) {
        const uint32_t m = pom_rec_meta(tile + lane, 16), st = (pom_rec_meta2(tile + lane, 16) >> 8) & 0xFF;
        const int status = (int)((st & POM_ST_DONE) ? 1 : 0) | (int)((st & POM_ST_DRAW) ? 2 : 0) | (int)((st & POM_ST_TIMEOUT) ? 4 : 0) |
                           (int)((st & POM_ST_RESTARTED) ? 8 : 0);
        reinterpret_cast<int4*>(p.env_attrs)[e0 + lane] =
            make_int4((int)tile[POM_REC_TIMESTEP * 16 + lane], pom_sext8(m), status, (int)((st >> POM_ST_WINNER_SHIFT) & 7) - 1);
    }
}

#endif /* __HIPCC__ */

#endif /* POM_VIEW_MEMORY_H_ */
