/*
 * pom_compact_view_emul.cpp — TEST-ONLY host build of the compact views' byte mapping (pomcpp_amd/csrc/pom_observe_compact.h), to check
 * it against the index shuffle of tests/compact_view_oracle.py without a GPU.  Never linked into the product.  A batch leaves as the
 * kernel writes it (pom_observe.h pom_observe_tile_compact): pass by pass of four envs, the pass's unfogged code planes staged, its
 * whole dwords by obs_compact_dword, the one to three bytes a short last pass ends with by obs_compact_byte.
 *
 * Built with -DPOM_COMPACT_VIEW_EMUL_MAIN it is a stand-alone program: every mask, radius and form at batch sizes with every pass length
 * and every tail, between guard bytes, each byte also worked out the long way — for a run under the host sanitizers.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pom_observe_compact.h"

/* codes: uint8 [n][5][11][11], what pom_batch_observe(POM_OBS_CODES) writes; xy: uint8 [n][4], agent a's x | y << 4; out: uint8
 * [n][k][5][S][S].  Returns the bytes written */
extern "C" int64_t pom_emul_compact_views(int64_t n, int32_t viewer_mask, int32_t flags, int32_t radius, const uint8_t* codes, const uint8_t* xy,
                                          uint8_t* out)
{
    const int32_t word = obs_compact_word(viewer_mask, flags);
    const ObsCompact g = obs_compact_geom(word, radius);
    uint8_t stage[OBS_CV_PASS_ENVS * OBS_CV_ENV_BYTES];
    int64_t written = 0;
    for (int64_t e0 = 0; e0 < n; e0 += OBS_CV_PASS_ENVS) {
        const int64_t left = n - e0;
        const int m = left < (int64_t)OBS_CV_PASS_ENVS ? (int)left : (int)OBS_CV_PASS_ENVS;
        memset(stage, 0, sizeof stage);
        memcpy(stage, codes + e0 * OBS_CV_ENV_BYTES, (size_t)m * OBS_CV_ENV_BYTES);
        const uint8_t* xy0 = xy + e0 * 4;
        const auto pos = [xy0, m](int ei, int id) { return ei < m ? (int)xy0[ei * 4 + id] : 0; };
        uint8_t* out_b = out + e0 * (int64_t)g.row;
        const uint32_t bytes = (uint32_t)m * g.row;
        for (uint32_t i = 0; i < (bytes >> 2); i++) { /* (the kernel: 64 lanes, i = lane, lane + 64, ..) */
            const uint32_t w = obs_compact_dword(g, i, pos, stage);
            memcpy(out_b + 4 * (size_t)i, &w, 4);
        }
        for (uint32_t lane = 0; lane < (bytes & 3u); lane++) {
            const uint32_t b = (bytes & ~3u) + lane;
            out_b[b] = (uint8_t)obs_compact_byte(g, obs_compact_at(g, b), pos, stage);
        }
        written += bytes;
    }
    return written;
}

/* viewer id's row among the chosen ones, or -1 (viewer_attrs' index) */
extern "C" int32_t pom_emul_compact_rank(int32_t viewer_mask, int32_t flags, int32_t id) { return obs_compact_rank(obs_compact_word(viewer_mask, flags), id); }

#if defined(POM_COMPACT_VIEW_EMUL_MAIN)
int main(void)
{
    static const int sizes[] = {1, 2, 3, 4, 5, 17};
    enum { NMAX = 17, GUARD = 64 };
    static uint8_t codes[NMAX * OBS_CV_ENV_BYTES], xy[NMAX * 4];
    uint32_t s = 12345u;
    for (size_t i = 0; i < sizeof codes; i++) codes[i] = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
    for (size_t i = 0; i < sizeof xy; i++) {
        s = s * 1664525u + 1013904223u;
        xy[i] = (uint8_t)(((s >> 8) % 11u) | (((s >> 20) % 11u) << 4));
    }
    long checked = 0;
    for (int mask = 1; mask <= 15; mask++)
        for (int r = 0; r <= 10; r++)
            for (int centred = 0; centred < 2; centred++)
                for (int n : sizes) {
                    const int k = __builtin_popcount((unsigned)mask), S = centred ? 2 * r + 1 : 11;
                    const size_t size = (size_t)n * k * 5 * S * S;
                    uint8_t* buf = (uint8_t*)malloc(size + 2 * GUARD); /* exactly as long: the sanitizer sees one byte too many */
                    memset(buf, 0xAB, size + 2 * GUARD);
                    if (pom_emul_compact_views(n, mask, centred, r, codes, xy, buf + GUARD) != (int64_t)size) return 1;
                    for (int g = 0; g < GUARD; g++)
                        if (buf[g] != 0xAB || buf[GUARD + size + g] != 0xAB) return 2;
                    size_t at = 0;
                    for (int e = 0; e < n; e++)
                        for (int v = 0; v < 4; v++) {
                            if (!((mask >> v) & 1)) continue;
                            const int xv = xy[e * 4 + v] & 15, yv = xy[e * 4 + v] >> 4;
                            for (int p = 0; p < 5; p++)
                                for (int dy = 0; dy < S; dy++)
                                    for (int dx = 0; dx < S; dx++, at++) {
                                        const int x = centred ? xv - r + dx : dx, y = centred ? yv - r + dy : dy;
                                        const int shows = x >= 0 && x < 11 && y >= 0 && y < 11 && abs(x - xv) <= r && abs(y - yv) <= r;
                                        const int want = shows ? codes[e * OBS_CV_ENV_BYTES + p * 121 + y * 11 + x] : p == 0 ? 5 : 0;
                                        if (buf[GUARD + at] != want) {
                                            printf("mask %d r %d centred %d n %d: byte %zu is %d, not %d\n", mask, r, centred, n, at, buf[GUARD + at], want);
                                            return 3;
                                        }
                                    }
                        }
                    checked += (long)at;
                    free(buf);
                }
    printf("ok: %ld bytes\n", checked);
    return 0;
}
#endif
