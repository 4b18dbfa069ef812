/*
 * pom_move_safety_emul.cpp — TEST-ONLY host build of the two set functions of pom_batch_move_safety's kernel
 * (pomcpp_amd/csrc/pom_move_safety.h: pom_free_word, pom_escape_grow), to check them against tests/move_safety_oracle.py's boolean
 * arrays without a GPU.  Never linked into the product.
 */
#include "pom_policy_emul.cpp" /* PomQuadHost: the four lanes of a quad at once, as the policy's level functions are fuzzed with */

#include "pom_move_safety.h"

struct BoardCodes {
    uint8_t cells[128];
    uint32_t cells4(int k) const { return (uint32_t)cells[4 * k] | ((uint32_t)cells[4 * k + 1] << 8) | ((uint32_t)cells[4 * k + 2] << 16) | ((uint32_t)cells[4 * k + 3] << 24); }
};

extern "C" {

/* one growth step of a 121-bit set on a 121-bit Free mask, four words each */
void pom_emul_escape_grow(const uint32_t reach[4], const uint32_t free_cells[4], uint32_t out[4])
{
    const PomQuadHost q;
    const QW r = pom_escape_grow(q, QW{{reach[0], reach[1], reach[2], reach[3]}}, QW{{free_cells[0], free_cells[1], free_cells[2], free_cells[3]}});
    for (int k = 0; k < 4; k++) out[k] = r.v[k];
}

/* Free of a State's board through pack -> cell codes -> pom_free_word, word by word as the quad's lanes build it; -1 if the state is
 * not representable */
int pom_emul_free_words(const void* state_1004, uint32_t out[4])
{
    uint32_t rec[POM_REC_DWORDS];
    if (pom_pack_state((const int32_t*)state_1004, rec, 1)) return -1;
    BoardCodes b;
    for (int c = 0; c < POM_CELLS; c++) b.cells[c] = (uint8_t)pom_rec_cell(rec, 1, c);
    for (int c = POM_CELLS; c < 128; c++) b.cells[c] = (uint8_t)(c & 1 ? POM_C_PASSAGE : POM_C_KICK); /* what follows the board in the tile is not cells, and may look free: the word must mask it */
    for (int m = 0; m < 4; m++) out[m] = pom_free_word(b, m);
    return 0;
}

}
