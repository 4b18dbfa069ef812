/*
 * pom_copy.h — the kernels of pom_batch_copy_envs / _copy_envs_device (include/pom_batch.h): env first + i becomes a copy of env
 * src[i], as if every source had been read before any destination was written.
 *
 * One wavefront may own a destination tile that another wavefront reads a source column from, so the copy takes two passes:
 *   K1 pom_copy_gather_kernel   one wavefront per destination tile: the tile (5,120 B) into LDS, the source column of every env
 *                               with a valid source over its own column (from another tile of the state buffer or from the
 *                               source's snapshot record; pom_packed.h pom_col_copy_item / pom_rec_to_col_item), the whole tile
 *                               out to a scratch image; the agent memory, episode counter and terminal record of those envs
 *                               into scratch arrays laid out like the real ones.
 *   K2 pom_copy_scatter_kernel  one wavefront per destination tile: the scratch tile into the state buffer (16 B per lane, whole
 *                               cache lines), the other per-env arrays of the copied envs, and with POM_COPY_SET_SNAPSHOT their
 *                               snapshot records (read from the scratch tile, so a FROM_SNAPSHOT | SET_SNAPSHOT call reads `snap`
 *                               in K1 and writes it in K2).
 * No kernel reads and writes the same array, except the host variant's shortcut: where no source lies in the destination range,
 * K1 writes straight into the real arrays (`out` = the batch's own buffers).  Every byte it then stores into a column that is
 * not a destination is the byte it loaded from there, so a wavefront reading a source column out of that tile sees the same
 * bytes either way.
 *
 * An entry src[i] < 0 or >= n leaves env first + i as it is (its column is stored back as loaded).  Columns past n are never
 * destinations: they stay blank records.
 */
#ifndef POM_COPY_H_
#define POM_COPY_H_

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pom_batch.h"
#include "pom_packed.h"
#include "pom_tile.h" /* store_tile16_x4 */

struct CopyParams {
    const int64_t* src;        /* device int64[count] */
    int64_t first, count, n, n_pad;
    int64_t tile0;             /* first destination tile; workgroup b works on tile tile0 + b */
    int32_t flags;             /* POM_COPY_* */
    /* the batch's arrays */
    uint32_t* state;
    uint32_t* snap;
    uint32_t* agent_mem;       /* [2][4 * n_pad] or nullptr (no SimpleAgent memory allocated) */
    uint32_t* episode;         /* [n_pad] */
    uint32_t* terminal;        /* [n_pad][80] or nullptr (not POM_RESET_AT_END) */
    /* where K1 writes (the scratch image, laid out like the arrays above; or the arrays themselves) and K2 reads */
    uint32_t* out_state;
    uint32_t* out_agent_mem;
    uint32_t* out_episode;
    uint32_t* out_terminal;
};

/* the source of destination env e, or -1 (not a destination, or an entry that leaves it alone); wavefront-uniform */
__device__ __forceinline__ int64_t copy_source(const CopyParams& p, int64_t e)
{
    if (e < p.first || e >= p.first + p.count) return -1;
    const int64_t s = p.src[e - p.first];
    return s >= 0 && s < p.n ? s : -1;
}

__global__ __launch_bounds__(64) void pom_copy_gather_kernel(CopyParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[POM_TILE_DWORDS];
    const int lane = threadIdx.x;
    const int64_t t = p.tile0 + blockIdx.x;
    const bool from_snap = (p.flags & POM_COPY_FROM_SNAPSHOT) != 0;
    {   /* the destination tile as it stands: the columns without a valid source leave as they came */
        const uint4* g = reinterpret_cast<const uint4*>(p.state + t * POM_TILE_DWORDS);
        uint4* l = reinterpret_cast<uint4*>(tile);
#pragma unroll
        for (int k = lane; k < POM_TILE_DWORDS / 4; k += 64) l[k] = g[k];
    }
    __syncthreads();
    for (int ec = 0; ec < POM_TILE_ENVS; ec++) {
        const int64_t e = t * POM_TILE_ENVS + ec;
        const int64_t s = copy_source(p, e);
        if (s < 0) continue;
        if (from_snap) {
            const uint32_t* rec = p.snap + s * POM_REC_DWORDS;
            for (int k = lane; k < POM_COL_ITEMS; k += 64) pom_rec_to_col_item(tile, ec, rec, k);
        } else {
            const uint32_t* st = p.state + (s >> 4) * POM_TILE_DWORDS;
            for (int k = lane; k < POM_COL_ITEMS; k += 64) pom_col_copy_item(tile, ec, st, (int)(s & 15), k);
        }
        if (p.agent_mem && lane < 8) { /* 4 agents x the two words of each: fresh agents from a snapshot */
            const int64_t half = (int64_t)(lane >> 2) * 4 * p.n_pad, a = lane & 3;
            p.out_agent_mem[half + e * 4 + a] = from_snap ? 0u : p.agent_mem[half + s * 4 + a];
        }
        if (!from_snap) {
            if (lane == 0) p.out_episode[e] = p.episode[s];
            if (p.terminal)
                for (int k = lane; k < POM_REC_DWORDS; k += 64) p.out_terminal[e * POM_REC_DWORDS + k] = p.terminal[s * POM_REC_DWORDS + k];
        }
    }
    __syncthreads();
    store_tile16_x4(p.out_state + t * POM_TILE_DWORDS, tile, lane);
}

/* scatter = false: only the snapshots (the host variant's shortcut, where K1 wrote the real arrays) */
template <bool SCATTER>
__global__ __launch_bounds__(64) void pom_copy_scatter_kernel(CopyParams p)
{
    const int lane = threadIdx.x;
    const int64_t t = p.tile0 + blockIdx.x;
    const bool from_snap = (p.flags & POM_COPY_FROM_SNAPSHOT) != 0;
    if (SCATTER) {
        const uint4* g = reinterpret_cast<const uint4*>(p.out_state + t * POM_TILE_DWORDS);
        uint4* d = reinterpret_cast<uint4*>(p.state + t * POM_TILE_DWORDS);
#pragma unroll
        for (int k = lane; k < POM_TILE_DWORDS / 4; k += 64) d[k] = g[k];
    }
    for (int ec = 0; ec < POM_TILE_ENVS; ec++) {
        const int64_t e = t * POM_TILE_ENVS + ec;
        if (copy_source(p, e) < 0) continue;
        if (SCATTER) {
            if (p.agent_mem && lane < 8) {
                const int64_t i = (int64_t)(lane >> 2) * 4 * p.n_pad + e * 4 + (lane & 3);
                p.agent_mem[i] = p.out_agent_mem[i];
            }
            if (!from_snap) {
                if (lane == 0) p.episode[e] = p.out_episode[e];
                if (p.terminal)
                    for (int k = lane; k < POM_REC_DWORDS; k += 64) p.terminal[e * POM_REC_DWORDS + k] = p.out_terminal[e * POM_REC_DWORDS + k];
            }
        }
        if (p.flags & POM_COPY_SET_SNAPSHOT) {
            const uint32_t* st = p.out_state + t * POM_TILE_DWORDS;
            for (int k = lane; k < POM_COL_ITEMS; k += 64) pom_col_to_rec_item(p.snap + e * POM_REC_DWORDS, st, ec, k, true);
        }
    }
}

#endif /* POM_COPY_H_ */
