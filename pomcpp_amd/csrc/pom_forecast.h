/*
 * pom_forecast.h — pom_batch_forecast's kernel (include/pom_batch.h PomForecastSpec): where will the fire be, and when?
 *
 * A wavefront takes a tile of 16 envs into LDS exactly as the quad step kernel does (pom_tile.h: load_tile16_x4, lane_from_tile,
 * a quad of lanes per env), plays K ticks of the real tick (PomStepper::step_packed, pom_step_body.h) on that copy and never stores
 * it: after every tick it notes, per cell, the first tick that leaves the cell in flames, per agent the tick it died in, and the
 * tick's POM_UB_* flags.  Nothing of the batch is written — no record, no counter, no ticket word, no restart.
 *
 * LDS: the tick's LDS_ROWS rows (record, bomb destinations, frames / claim maps), and BEHIND them FC_STAGE_ROWS rows of staging —
 * a byte per cell and env in the board's own [cell][env] layout (byte c * 16 + el, pom_packed.h), 0 = not seen in flames yet.  The
 * staging lies behind LDS_ROWS and not over the tick's scratch rows as the policy's maps and the observation's staging area do in
 * pom_step_kernel: there the tick is over when the overlay is used, here it runs again between two scans, and a wavefront's
 * frames [row][16] and claim maps [env][124] (ROW_STACK, ROW_CLAIMS) reach over all of the scratch rows.
 */
#ifndef POM_FORECAST_H_
#define POM_FORECAST_H_

#include "pom_device.h"

struct ForecastParams {
    const uint32_t* state;
    const int32_t* moves; /* device int32[n][4] of forecast tick 1, or nullptr: IDLE */
    uint8_t* flame_tick;  /* uint8 [n][121] */
    int32_t* agent_tick;  /* nullable: int32 [n][4] */
    uint32_t* ubflags;    /* nullable: uint32 [n] */
    int64_t n;
    int32_t horizon;      /* 1 .. POM_FORECAST_MAX_TICKS */
};

enum {
    FC_BOARD_DWORDS = POM_CELLS * 4,       /* 484: the board by cell, a dword = one cell of four envs */
    FC_STAGE_ROW = LDS_ROWS,               /* behind everything the tick touches */
    FC_STAGE_ROWS = POM_REC_BOARD_DWORDS,  /* 31 rows = 1,984 B: 121 x 16 staging bytes (and the board's 48 bytes of padding) */
    FC_ROWS = FC_STAGE_ROW + FC_STAGE_ROWS,
    FC_OUT_BYTES = POM_CELLS * 16,         /* a tile's 16 x 121 output bytes: 121 stores of 16 bytes */
};
static_assert(FC_STAGE_ROW >= ROW_CLAIMS + 31 && FC_STAGE_ROW >= ROW_STACK + POM_STACK_DEPTH && FC_STAGE_ROW >= ROW_BDEST + 5,
              "the staging rows alias nothing the tick uses");
static_assert(FC_STAGE_ROWS * 64 >= FC_OUT_BYTES && POM_FORECAST_MAX_TICKS < 256, "a byte per cell and env holds the tick");
static_assert(FC_OUT_BYTES % 16 == 0 && FC_BOARD_DWORDS <= 8 * 64, "eight board dwords per lane; the tile's output is whole 16-byte stores");

__global__ __launch_bounds__(64, POM_QUAD_WAVES) void pom_forecast_kernel(ForecastParams p)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[FC_ROWS * 16];
    uint32_t* const stage_w = tile + FC_STAGE_ROW * 16;
    const int lane = threadIdx.x;
    const int64_t tile_id = pom_xcd_tile_order(blockIdx.x, gridDim.x);
    /* the HBM layout is 16-env tiles whatever the handle's launch shape (as pom_observe_kernel relies on); the buffers hold n_pad
     * columns, so a last, short tile is loaded whole */
    load_tile16_x4(p.state + tile_id * POM_TILE_DWORDS, tile, lane);
    /* the tick: lane -> (env lane / 4, member lane % 4) as in pom_step_kernel<16, 4> */
    const int ec = lane >> 2, member = lane & 3;
    const int64_t e = tile_id * 16 + ec;
    const bool valid = e < p.n; /* the lanes of an env past the batch's end step nothing and write nothing */
    /* tick 1's moves do not depend on the record: fetch them while it is on its way.  Lane m reads agent m's (dead agents' entries
     * included, as pom_batch_step_device reads them): 64 consecutive dwords per wavefront */
    int mine = POM_MOVE_IDLE;
    if (p.moves && valid) mine = p.moves[e * 4 + member];
#pragma unroll
    for (int i = 0; i < 2; i++)
        if (lane + 64 * i < FC_STAGE_ROWS * 4) reinterpret_cast<uint4*>(stage_w)[lane + 64 * i] = make_uint4(0, 0, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* the DMA rows have landed (one wavefront per workgroup: no barrier) */
    uint32_t* t = tile + ec;
    PomLane L;
    int time_step = 0;
    uint32_t status = 0;
    lane_from_tile(L, time_step, status, t, 16);
    pom_lane_diag_off(L);
    LdsEnv<16, 4> acc(tile, ec, member);
    PomStepper<LdsEnv<16, 4>> stepper(acc, L);
    L.ub = 0; /* the flags these K ticks raise; the env's own (the record's) are not the forecast's */
    /* lane m keeps agent m's answer (the quad's registers are identical: sel4 of any lane's copy): -1 dead before the first tick */
    int my_tick = ag_dead(sel4(member, L.a0)) ? -1 : 0;

    /* the moves, a nibble per agent, exchanged within the quad as the explicit-move path of pom_step_kernel does; ticks 2 .. K are
     * all-IDLE: the packed word of four IDLE moves is 0 */
    static_assert(POM_MOVE_IDLE == 0, "the packed all-IDLE word");
    uint32_t mvp = stepper.pack_moves_quad(mine);
    const int K = p.horizon;
    POM_NOUNROLL
    for (int tk = 1; tk <= K; tk++) {
        if (valid) {
            /* bare bboard::Step as in POM_MODE_RAW: no timeStep++, no done / max_steps logic, a finished env is played like any other */
            stepper.step_packed(mvp);
            mvp = 0u;
            my_tick = ((int)(my_tick == 0) & ag_dead(sel4(member, L.a0))) ? tk : my_tick;
        }
        obs_lds_order(); /* the lanes' board writes are in the tile: no read below may be scheduled earlier */
        /* the scan: a dword of the board = cell c of four envs.  The bytes that are flames (codes >= POM_C_FLAME = 15, pom_packed.h) and
         * whose staging byte is still 0 get this tick's number */
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int i = lane + 64 * j;
            if (j < FC_BOARD_DWORDS / 64 || i < FC_BOARD_DWORDS) {
                const uint32_t d = tile[i], s = stage_w[i];
                const uint32_t flame = (((d & 0x7F7F7F7Fu) + 0x71717171u) | d) & 0x80808080u;  /* bit 7 of the bytes >= 15 */
                const uint32_t seen = (((s & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | s) & 0x80808080u;   /* bit 7 of the bytes != 0 */
                const uint32_t fresh = (flame & ~seen) >> 7;                                      /* 1 in the bytes to set */
                stage_w[i] = s | (fresh * (uint32_t)tk);
            }
        }
        obs_lds_order(); /* ... and the next tick's accesses stay behind the scan */
    }

    /* out: the staging area transposed to [env][121] — the tile's 1,936 contiguous bytes as 16-byte stores (flame_tick is 16-byte
     * aligned and a tile's bytes are a multiple of 16), clipped at byte n * 121 for a last, short tile: its last bytes, where they
     * are no whole line, leave one by one */
    {
        const int64_t left = p.n - tile_id * 16;
        const int bytes = (int)(left < 16 ? left : 16) * POM_CELLS;
        const uint8_t* stage_b = reinterpret_cast<const uint8_t*>(stage_w);
        uint8_t* out_b = p.flame_tick + tile_id * FC_OUT_BYTES;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int v = lane + 64 * i; /* the 16-byte line */
            if (16 * v < bytes) {
                int el = (16 * v) / POM_CELLS, c = 16 * v - el * POM_CELLS; /* of the line's first byte */
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int b = 0; b < 16; b++) {
                    w[b >> 2] |= (uint32_t)stage_b[c * 16 + el] << (8 * (b & 3));
                    c++;
                    if (c == POM_CELLS) {
                        c = 0;
                        el++;
                    }
                }
                if (16 * v + 16 <= bytes) reinterpret_cast<uint4*>(out_b)[v] = make_uint4(w[0], w[1], w[2], w[3]);
                else {
                    for (int b = 0; 16 * v + b < bytes; b++) out_b[16 * v + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
                }
            }
        }
    }
    /* the agents' ticks: one int4 per env from the owner lane; the flags likewise */
    const int t0 = acc.gbcast<0>(my_tick), t1 = acc.gbcast<1>(my_tick), t2 = acc.gbcast<2>(my_tick), t3 = acc.gbcast<3>(my_tick);
    if (valid && member == 0) {
        if (p.agent_tick) reinterpret_cast<int4*>(p.agent_tick)[e] = make_int4(t0, t1, t2, t3);
        if (p.ubflags) p.ubflags[e] = L.ub;
    }
}

#endif /* POM_FORECAST_H_ */
