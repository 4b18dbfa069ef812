/*
 * pom_reach_emul.cpp — TEST-ONLY host build of the level functions of pom_batch_reach's kernel (pomcpp_amd/csrc/pom_reach.h:
 * pom_reach_sets_word, pom_reach_flood and what it is made of, pom_reach_cells4), to check them against the compiled reference's
 * maps (tests/golden/reach.npz) and the oracle's without a GPU.  Never linked into the product.
 */
#include "pom_policy_emul.cpp" /* PomQuadHost: the four lanes of a quad at once, as the policy's level functions are fuzzed with */

#include "pom_reach.h"

struct ReachBoardCodes {
    uint8_t cells[128];
    uint32_t cells4(int k) const { return (uint32_t)cells[4 * k] | ((uint32_t)cells[4 * k + 1] << 8) | ((uint32_t)cells[4 * k + 2] << 16) | ((uint32_t)cells[4 * k + 3] << 24); }
};
struct ReachHostMore {
    bool operator()(const QW& front) const { return PomQuadHost().any(front); }
};

template <bool MOVE, bool DIST>
static void reach_one(const QW& src, const QW& walk, const QW& agents, int max_dist, uint8_t* dist121, uint8_t* move121)
{
    const PomQuadHost q;
    QW dist[POM_REACH_PLANES], mv[3];
    pom_reach_flood<MOVE, DIST>(q, src, walk, agents, max_dist, dist, mv, ReachHostMore());
    /* the planes of every lane's word to bytes, as pom_reach_stage writes them: 128 bytes per row, the first 121 are cells */
    for (int k = 0; k < 4; k++) {
        uint32_t dw[POM_REACH_PLANES], mw[3];
        for (int i = 0; i < POM_REACH_PLANES; i++) dw[i] = dist[i].v[k];
        for (int i = 0; i < 3; i++) mw[i] = mv[i].v[k];
        for (int j = 0; j < 8; j++) {
            const uint32_t d4 = pom_reach_cells4(dw, j), m4 = pom_reach_cells4(mw, j);
            for (int b = 0; b < 4; b++) {
                const int c = 32 * k + 4 * j + b;
                if (c >= POM_CELLS) continue;
                if (DIST) dist121[c] = (uint8_t)(d4 >> (8 * b));
                if (MOVE) move121[c] = (uint8_t)(m4 >> (8 * b));
            }
        }
    }
}

extern "C" {

/* The rows [e][a] of pom_batch_reach for n States and the agents of agent_mask, through pack -> cell codes -> the kernel's sets and
 * flood: dist and move are uint8 [n][4][121], either may be NULL (the kernel's three instances: both, move alone with the labelled
 * flood, dist alone with one front).  Rows of agents outside the mask are not written.  Returns -1 if a State is not representable. */
int pom_emul_reach(const void* states_1004, int n, int agent_mask, int max_dist, uint8_t* dist, uint8_t* move)
{
    const PomQuadHost q;
    for (int e = 0; e < n; e++) {
        uint32_t rec[POM_REC_DWORDS];
        if (pom_pack_state((const int32_t*)((const char*)states_1004 + (size_t)e * 1004), rec, 1)) return -1;
        ReachBoardCodes b;
        for (int c = 0; c < POM_CELLS; c++) b.cells[c] = (uint8_t)pom_rec_cell(rec, 1, c);
        for (int c = POM_CELLS; c < 128; c++) b.cells[c] = (uint8_t)(c & 1 ? POM_C_PASSAGE : POM_C_AGENT); /* what follows the board in the tile is not cells: the words must mask it */
        QW walk, agents;
        for (int m = 0; m < 4; m++) pom_reach_sets_word(b, m, walk.v[m], agents.v[m]);
        for (int a = 0; a < 4; a++) {
            if (!((agent_mask >> a) & 1)) continue;
            const int a0 = (int)rec[POM_REC_AGENTS + 2 * a];
            const QW src = ag_dead(a0) ? QW{{0, 0, 0, 0}} : q.bit(ag_y(a0) * POM_N + ag_x(a0));
            uint8_t* d = dist ? dist + ((size_t)e * 4 + a) * POM_CELLS : nullptr;
            uint8_t* m = move ? move + ((size_t)e * 4 + a) * POM_CELLS : nullptr;
            if (d && m) reach_one<true, true>(src, walk, agents, max_dist, d, m);
            else if (m) reach_one<true, false>(src, walk, agents, max_dist, d, m);
            else if (d) reach_one<false, true>(src, walk, agents, max_dist, d, m);
        }
    }
    return 0;
}

}
