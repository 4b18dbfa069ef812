/*
 * pom_observe_compact.h — the compact views' byte mapping (pom_batch.h PomCompactViewSpec), host and device: which staged byte, or
 * which constant, output byte b of a pass of four envs is.  The export's kernels (pom_observe.h pom_observe_tile_compact) store what
 * obs_compact_dword returns and nothing else; tests/emul/pom_compact_view_emul.cpp builds the same functions for the host.
 *
 * A pass is the four envs that pom_observe_stage<true, 1> stages (605 code bytes each: [5][11][11]); its output is the dense run
 * [4][k][5][S][S] of bytes, k the chosen viewers and S the side of a view (11, or 2 r + 1 centred).  Byte b of that run is
 *     b -> (ei env of the pass, j viewer index, pl plane, dy, dx)              obs_compact_at / obs_compact_next
 *       -> the cell (x, y) of the board it shows, or none                       obs_compact_source
 *       -> staged byte ei * 605 + pl * 121 + y * 11 + x, or fog (5 in plane 0, 0 in the others).
 * No runtime division on the way: b / S^2 and cell / S are a multiply-high by a constant of the launch (obs_cv_div), the small
 * quotients behind them multiply-shifts, and the three bytes that follow a dword's first one advance by carries.
 */
#ifndef POM_OBSERVE_COMPACT_H_
#define POM_OBSERVE_COMPACT_H_

#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "pom_batch.h"
#include "pom_rng.h" /* POM_HD */

enum { OBS_CV_N = 11, OBS_CV_CELLS = 121, OBS_CV_PLANES = 5, OBS_CV_ENV_BYTES = 605, OBS_CV_PASS_ENVS = 4, OBS_CV_FOG = 5 };

/* the one word the kernels get beside view_radius: 0 = the four-view form, else viewer_mask | flags << 4 (the mask is never 0) */
POM_HD int32_t obs_compact_word(int32_t viewer_mask, int32_t flags) { return viewer_mask | (flags << 4); }

/* floor(b / d) for b < 2^31 / 2 and d < 2^15 as mulhi(2 b + 1, ceil(2^31 / d)): (b + 1/2) / d has the same floor as b / d and lies
 * at least 1 / (2 d) below the next integer; the magic's excess adds less than (2 b + 1) / 2^32.  For the b < 35,280 and d <= 441
 * used here that is 1.7e-5 against 1.1e-3.  (d = 1 gives 2^31: exact.) */
POM_HD uint32_t obs_cv_magic(uint32_t d) { return (0x80000000u + d - 1u) / d; }
POM_HD uint32_t obs_cv_div(uint32_t b, uint32_t magic)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(2u * b + 1u, magic);
#else
    return (uint32_t)(((uint64_t)(2u * b + 1u) * magic) >> 32);
#endif
}

struct ObsCompact {
    int32_t k, S, r, centred;
    uint32_t S2, row;    /* bytes of a plane of a view; of an env's k views */
    uint32_t m_S2, m_S;  /* obs_cv_magic of S2 and S */
    uint32_t m_k;        /* t / k = (t * m_k) >> 8 for t < 16 */
    uint32_t ids;        /* the chosen viewers in rising order: viewer index j is agent (ids >> 2 j) & 3 */
};
POM_HD ObsCompact obs_compact_geom(int32_t word, int32_t r)
{
    ObsCompact g;
    g.centred = (word >> 4) & POM_VIEW_CENTRED;
    g.r = r;
    g.k = 0;
    g.ids = 0;
    for (int v = 0; v < 4; v++)
        if ((word >> v) & 1) g.ids |= (uint32_t)v << (2 * g.k++);
    g.S = g.centred ? 2 * r + 1 : OBS_CV_N;
    g.S2 = (uint32_t)(g.S * g.S);
    g.row = (uint32_t)g.k * OBS_CV_PLANES * g.S2;
    g.m_S2 = obs_cv_magic(g.S2);
    g.m_S = obs_cv_magic((uint32_t)g.S);
    g.m_k = 256u / (uint32_t)(g.k ? g.k : 1) + 1u;
    return g;
}
/* viewer `id`'s index among the chosen ones, or -1 */
POM_HD int obs_compact_rank(int32_t word, int id)
{
    const int below = word & ((1 << id) - 1);
    return ((word >> id) & 1) ? (below & 1) + ((below >> 1) & 1) + ((below >> 2) & 1) : -1;
}

struct ObsCompactAt {
    int ei, j, pl, dy, dx;
};
/* byte b < 4 * g.row of a pass's output */
POM_HD ObsCompactAt obs_compact_at(const ObsCompact& g, uint32_t b)
{
    ObsCompactAt a;
    const uint32_t gp = obs_cv_div(b, g.m_S2), cell = b - gp * g.S2; /* the plane among the pass's 4 k 5, the cell in it */
    const uint32_t dy = obs_cv_div(cell, g.m_S);
    const uint32_t t = (gp * 205u) >> 10; /* gp / 5 for gp < 80 */
    const uint32_t ei = (t * g.m_k) >> 8; /* t / k for t < 16 */
    a.dy = (int)dy;
    a.dx = (int)(cell - dy * (uint32_t)g.S);
    a.pl = (int)(gp - 5u * t);
    a.ei = (int)ei;
    a.j = (int)(t - ei * (uint32_t)g.k);
    return a;
}
/* the byte behind it */
POM_HD void obs_compact_next(const ObsCompact& g, ObsCompactAt& a)
{
    const int cx = a.dx + 1 == g.S;
    a.dx = cx ? 0 : a.dx + 1;
    const int cy = cx & (int)(a.dy + 1 == g.S);
    a.dy = cy ? 0 : a.dy + cx;
    const int cp = cy & (int)(a.pl + 1 == OBS_CV_PLANES);
    a.pl = cp ? 0 : a.pl + cy;
    const int cj = cp & (int)(a.j + 1 == g.k);
    a.j = cj ? 0 : a.j + cp;
    a.ei += cj;
}
/* Where the byte at `a` of a viewer standing at (xv, yv) comes from: the offset in the pass's staged bytes, or -1 for fog.  Centred,
 * the crop's corner lies at (xv - r, yv - r) and a cell shows if it is on the board (it is then inside the window); uncentred the
 * corner is the board's and a cell shows if the window holds it (it is then on the board).  One test serves both. */
POM_HD int obs_compact_source(const ObsCompact& g, const ObsCompactAt& a, int xv, int yv)
{
    const int x = a.dx + (g.centred ? xv - g.r : 0), y = a.dy + (g.centred ? yv - g.r : 0);
    const int shows = (int)((uint32_t)x < (uint32_t)OBS_CV_N) & (int)((uint32_t)y < (uint32_t)OBS_CV_N) &
                      (int)((uint32_t)(x - xv + g.r) <= (uint32_t)(2 * g.r)) & (int)((uint32_t)(y - yv + g.r) <= (uint32_t)(2 * g.r));
    return shows ? a.ei * OBS_CV_ENV_BYTES + a.pl * OBS_CV_CELLS + y * OBS_CV_N + x : -1;
}
/* pos(ei, id): agent id's position in env ei of the pass, x | y << 4 (the low byte of its first record word) */
template <class Pos>
POM_HD uint32_t obs_compact_byte(const ObsCompact& g, const ObsCompactAt& a, const Pos& pos, const uint8_t* stage_b)
{
    const int xy = pos(a.ei, (int)((g.ids >> (2 * a.j)) & 3u));
    const int src = obs_compact_source(g, a, xy & 15, (xy >> 4) & 15);
    const uint32_t staged = stage_b[src < 0 ? 0 : src];
    return src < 0 ? (a.pl == 0 ? (uint32_t)OBS_CV_FOG : 0u) : staged;
}
/* output dword i (bytes 4 i .. 4 i + 3) of a pass: the four bytes may belong to different (env, viewer, plane, row) */
template <class Pos>
POM_HD uint32_t obs_compact_dword(const ObsCompact& g, uint32_t i, const Pos& pos, const uint8_t* stage_b)
{
    ObsCompactAt a = obs_compact_at(g, 4u * i);
    uint32_t w = obs_compact_byte(g, a, pos, stage_b);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int s = 1; s < 4; s++) {
        obs_compact_next(g, a);
        w |= obs_compact_byte(g, a, pos, stage_b) << (8 * s);
    }
    return w;
}

#endif /* POM_OBSERVE_COMPACT_H_ */
