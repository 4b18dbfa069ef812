/*
 * pom_imagine_emul.cpp — TEST-ONLY host build of the rule functions of pom_batch_imagine's kernel (pomcpp_amd/csrc/pom_imagine.h:
 * pom_imagine_cell, pom_imagine_finish), to check them against the numpy checker (tests/imagine_oracle.py) without a GPU.  Never linked
 * into the product.  A job is built as the kernel builds it: over column j % 16 of a tile in its by-cell layout, the four members of the
 * quad taking the cells member, member + 4, ...; the column is then unpacked into a State by pom_packed.h.
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pom_imagine.h"

extern "C" {

/* `count` jobs: states int32 [count][251] (left as they are for a job that is not built), result uint32 [count]; memory uint8 [rows][726],
 * attrs int32 [rows][12], belief int32 [rows][12] or null, sample null: j. */
int pom_emul_imagine(int count, const int32_t* view, const int32_t* sample, int rows, const uint8_t* memory, const int32_t* attrs,
                     const int32_t* belief, uint64_t seed, int unknown, int32_t* states, uint32_t* result)
{
    for (int j = 0; j < count; j++) {
        uint32_t tile[POM_TILE_DWORDS];
        memset(tile, 0, sizeof tile);
        result[j] = 0;
        const int r = view[j], ec = j & 15;
        if (r < 0 || r >= rows) continue;
        const uint8_t* v = memory + (size_t)r * POM_IMG_VIEW_BYTES;
        const int32_t* at = attrs + (size_t)r * POM_OBS_VIEWER_ATTRS;
        const uint32_t key = pom_imagine_key(seed, r, sample ? sample[j] : j);
        const int vc = pom_imagine_viewer_cell(at);
        int unknown_cells = 0;
        for (int member = 0; member < 4; member++)
            for (int c = member; c < POM_IMG_CELLS; c += 4) {
                int u;
                reinterpret_cast<uint8_t*>(tile)[c * POM_TILE_ENVS + ec] = (uint8_t)pom_imagine_cell(v, c, key, unknown, vc, u);
                unknown_cells += u;
            }
        result[j] = pom_imagine_finish(v, tile, ec, at, belief ? belief + (size_t)r * 12 : nullptr, r & 3, key, unknown_cells);
        if (result[j] & POM_IMAGINE_BUILT) {
            int32_t* st = states + (size_t)j * (POM_STATE_BYTES / 4);
            memset(st, 0, POM_STATE_BYTES);
            pom_unpack_state(tile + ec, POM_TILE_ENVS, st, ec);
        }
    }
    return 0;
}

/* How many of `count` States upload would refuse (pom_pack_state, the live-bomb rule) or not give back bit for bit */
int pom_emul_imagine_refused(int count, const int32_t* states)
{
    int refused = 0;
    for (int j = 0; j < count; j++) {
        const int32_t* st = states + (size_t)j * (POM_STATE_BYTES / 4);
        uint32_t rec[POM_REC_DWORDS];
        int32_t back[POM_STATE_BYTES / 4];
        memset(back, 0, sizeof back);
        int bad = pom_pack_state(st, rec, 1);
        for (int k = 0; k < POM_MAX_BOMBS; k++) bad |= pom_pack_live_bomb_bad(st, k);
        if (!bad) pom_unpack_state(rec, 1, back);
        refused += bad || memcmp(back, st, POM_STATE_BYTES) != 0;
    }
    return refused;
}

}
