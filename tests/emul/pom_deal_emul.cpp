/*
 * pom_deal_emul.cpp — TEST-ONLY host build of the rule functions of pom_batch_deal's kernel (pomcpp_amd/csrc/pom_deal.h), to check them
 * against the literal checker (tests/deal_oracle.py) without a GPU.  Never linked into the product.  A board is dealt as the kernel deals
 * it — the attempts through the packed numbers of the quad's four members (PomDealPacked), the sets four words at once (PomQuadHost),
 * the record's dwords by pom_deal_dword and pom_deal_row — and the dense record is unpacked into a State by pom_packed.h.
 *
 * Built with -DPOM_DEAL_EMUL_MAIN it is a stand-alone program: it deals boards of four layouts and checks what no board may lack
 * (the counts, the symmetry, the fixed cells), for a run under the host sanitizers.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pom_policy_emul.cpp" /* PomQuadHost: the four lanes of a quad at once, as the policy's level functions are fuzzed with */

/* what the rule asks of a Q beyond pom_policy_body.h's list, for PomQuadHost */
static inline QW pom_deal_words(const PomQuadHost&, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return QW{{a, b, c, d}}; }
static inline int pom_deal_count(const PomQuadHost&, const QW& w)
{
    return __builtin_popcount(w.v[0]) + __builtin_popcount(w.v[1]) + __builtin_popcount(w.v[2]) + __builtin_popcount(w.v[3]);
}
static inline void pom_deal_gather(const PomQuadHost&, const QW& w, uint32_t (&g)[4])
{
    for (int k = 0; k < 4; k++) g[k] = w.v[k];
}

#include "pom_deal.h"

/* clause 5's numbers computed on the spot, pair by pair: the cross-check of the packed registers the kernel's countdown reads */
struct PomDealDirect {
    uint32_t key;
    int a;
    template <int K>
    int t() const { return pom_deal_t(key, a, K); }
};

/* one board: the dense record and the result word */
static uint32_t deal_one(uint64_t seed, int64_t env, int32_t game, const PomBoardLayout& l, uint32_t* rec)
{
    const PomQuadHost q;
    const uint32_t key = pom_deal_key(seed, env, game);
    QW rigid{{0, 0, 0, 0}}, wood{{0, 0, 0, 0}}, f0, f1;
    int attempts = 0, bad = 0, todo = 1;
    for (int a = 0; a < POM_DEAL_ATTEMPTS && todo; a++) {
        PomDealPacked ts;
        for (int member = 0; member < 4; member++) pom_deal_pack(key, a, member, ts.w[member][0], ts.w[member][1]);
        pom_deal_assign(q, ts, l, rigid, wood);
        QW r2, w2; /* the two ways to the numbers agree */
        pom_deal_assign(q, PomDealDirect{key, a}, l, r2, w2);
        if (memcmp(&r2, &rigid, sizeof r2) || memcmp(&w2, &wood, sizeof w2)) abort();
        bad = pom_deal_bad(q, rigid, wood);
        attempts = a + 1;
        todo = bad > l.max_inaccessible;
    }
    pom_deal_items(q, key, wood, l.num_items, f0, f1);
    for (int dw = 0; dw < POM_REC_BOARD_DWORDS; dw++) rec[dw] = pom_deal_dword(dw >> 3, dw & 7, rigid.v[dw >> 3], wood.v[dw >> 3], f0.v[dw >> 3], f1.v[dw >> 3]);
    for (int r = POM_REC_TIMESTEP; r < POM_REC_DWORDS; r++) rec[r] = pom_deal_row(r);
    return pom_deal_word(attempts, bad, todo);
}

extern "C" {

/* `count` boards: states int32 [count][251], words uint32 [count]; env, game int64 / int32 [count]; layout: the five int32.  Returns 1 if
 * the layout is refused (nothing is written) */
int pom_emul_deal(int count, uint64_t seed, const int64_t* env, const int32_t* game, const int32_t* layout, int32_t* states, uint32_t* words)
{
    PomBoardLayout l;
    memcpy(&l, layout, sizeof l);
    if (pom_deal_layout_bad(l)) return 1;
    for (int j = 0; j < count; j++) {
        uint32_t rec[POM_REC_DWORDS];
        words[j] = deal_one(seed, env[j], game[j], l, rec);
        int32_t* st = states + (size_t)j * (POM_STATE_BYTES / 4);
        memset(st, 0, POM_STATE_BYTES);
        pom_unpack_state(rec, 1, st);
    }
    return 0;
}

/* How many of `count` States upload would refuse (pom_pack_state, the live-bomb rule) or not give back bit for bit */
int pom_emul_deal_refused(int count, const int32_t* states)
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

const char* pom_emul_deal_layout_bad(const int32_t* layout)
{
    PomBoardLayout l;
    memcpy(&l, layout, sizeof l);
    return pom_deal_layout_bad(l);
}

}

#if defined(POM_DEAL_EMUL_MAIN)
int main(int argc, char** argv)
{
    const int boards = argc > 1 ? atoi(argv[1]) : 20000;
    const PomBoardLayout layouts[4] = {{36, 36, 20, 4, 0}, {0, 12, 0, 4, 0}, {20, 36, 36, 121, 0}, {56, 24, 10, 4, POM_LAYOUT_NO_LANES}};
    long fallbacks = 0, attempts = 0;
    for (int j = 0; j < boards; j++) {
        const PomBoardLayout& l = layouts[j & 3];
        uint32_t rec[POM_REC_DWORDS];
        int32_t st[POM_STATE_BYTES / 4];
        const uint32_t word = deal_one(0xDEA1u + (uint64_t)(j >> 12), j & 1 ? 1000000 + j : j, j % 7 == 0 ? 0x7FFFFFFF : j % 5, l, rec);
        memset(st, 0, sizeof st);
        pom_unpack_state(rec, 1, st);
        int rigid = 0, wood = 0, items = 0;
        for (int c = 0; c < POM_CELLS; c++) {
            const int32_t v = st[c], m = st[pom_deal_transpose(c)];
            rigid += v == POM_RIGID;
            wood += (v & ~7) == POM_WOOD;
            items += (v & ~7) == POM_WOOD && (v & 7) != 0;
            if ((v == POM_RIGID) != (m == POM_RIGID) || ((v & ~7) == POM_WOOD) != ((m & ~7) == POM_WOOD) || ((v & ~7) == POM_WOOD && (v & 7) > 3)) {
                fprintf(stderr, "board %d: cell %d breaks the symmetry or holds an unknown flag\n", j, c);
                return 1;
            }
            if (pom_deal_class(c) >= POM_DEAL_AGENT ? v != POM_AGENT0 + pom_deal_class(c) - POM_DEAL_AGENT : pom_deal_class(c) == POM_DEAL_FREE && v != POM_PASSAGE) {
                fprintf(stderr, "board %d: fixed cell %d holds %d\n", j, c, v);
                return 1;
            }
        }
        if (rigid != l.num_rigid || wood != l.num_wood || items != l.num_items || !(word & POM_DEAL_DEALT) ||
            (!(word & POM_DEAL_FALLBACK) && (int)(word >> POM_DEAL_BAD_SHIFT) > l.max_inaccessible)) {
            fprintf(stderr, "board %d: %d rigid, %d wood, %d items, word %08x\n", j, rigid, wood, items, word);
            return 1;
        }
        fallbacks += (word & POM_DEAL_FALLBACK) != 0;
        attempts += ((word >> POM_DEAL_ATTEMPTS_SHIFT) & 0xFF) + 1;
    }
    printf("pom_deal_emul: %d boards of 4 layouts ok, %ld attempts, %ld fallbacks\n", boards, attempts, fallbacks);
    return 0;
}
#endif
