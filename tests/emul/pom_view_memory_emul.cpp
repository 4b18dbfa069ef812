/*
 * pom_view_memory_emul.cpp — TEST-ONLY host build of the rule functions of pom_batch_remember_view's kernel
 * (pomcpp_amd/csrc/pom_view_memory.h: pom_view_memory_head, pom_view_memory_gone, pom_view_memory_cell), to check them against the
 * numpy checker (tests/view_memory_oracle.py) without a GPU.  Never linked into the product.  The window is restated here from its
 * definition (the kernel takes obs_window's word, which is device code): |x - x_v| <= r and |y - y_v| <= r as two bit sets.
 */
#include <stddef.h>
#include <stdint.h>

#include "pom_view_memory.h"

extern "C" {

/* One call on n envs: memory uint8 [n][4][6][121] and stamp int32 [n][4][2] in place, from codes uint8 [n][5][121], agent_attrs
 * int32 [n][4][8] (x, y, alive first), time_step int32 [n] and episodes uint32 [n].  Views outside agent_mask are not touched. */
int pom_emul_remember(int n, int view_radius, int agent_mask, uint8_t* memory, int32_t* stamp, const uint8_t* codes, const int32_t* agent_attrs,
                      const int32_t* time_step, const uint32_t* episodes)
{
    for (int e = 0; e < n; e++) {
        const int32_t* at = agent_attrs + (size_t)e * 4 * 8;
        for (int v = 0; v < 4; v++) {
            if (!((agent_mask >> v) & 1)) continue;
            uint32_t cols = 0, rows = 0;
            for (int i = 0; i < 11; i++) {
                if (i >= at[8 * v] - view_radius && i <= at[8 * v] + view_radius) cols |= 1u << i;
                if (i >= at[8 * v + 1] - view_radius && i <= at[8 * v + 1] + view_radius) rows |= 1u << i;
            }
            const uint32_t w = cols | (rows << 16);
            uint32_t gone = 0;
            for (int a = 0; a < 4; a++) gone |= pom_view_memory_gone(w, at[8 * a] & 15, at[8 * a + 1] & 15, !at[8 * a + 2]) << a;
            int32_t* st = stamp + ((size_t)e * 4 + v) * 2;
            int wipe, dt;
            pom_view_memory_head(episodes[e], time_step[e], st[0], st[1], wipe, dt);
            uint8_t* view = memory + ((size_t)e * 4 + v) * POM_MEM_VIEW_BYTES;
            for (int c = 0; c < POM_MEM_CELLS; c++) {
                int m[POM_MEMORY_PLANES], now[POM_OBS_CODE_PLANES];
                for (int k = 0; k < POM_MEMORY_PLANES; k++) m[k] = view[k * POM_MEM_CELLS + c];
                for (int k = 0; k < POM_OBS_CODE_PLANES; k++) now[k] = codes[((size_t)e * POM_OBS_CODE_PLANES + k) * POM_MEM_CELLS + c];
                const int inside = (int)(((w >> (c % 11)) & (w >> (16 + c / 11))) & 1u);
                pom_view_memory_cell(m, now, inside, wipe, dt, gone);
                for (int k = 0; k < POM_MEMORY_PLANES; k++) view[k * POM_MEM_CELLS + c] = (uint8_t)m[k];
            }
            st[0] = (int32_t)episodes[e];
            st[1] = time_step[e];
        }
    }
    return 0;
}

}
