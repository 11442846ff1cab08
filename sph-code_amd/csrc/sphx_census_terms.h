// sphx_census_terms.h - the per-row terms of the census (sphx_census.hip) and the places of its LDS tile, as host and
// device code: tests/host/census_check.cpp replays a chunk's tile and walk on the host with the same functions.
//
// Quantity q of a row (mass m, type pt, velocity v, previous acceleration a, internal energy E, composition row f of s
// values, mu_specie mus):
//   0..3    m where pt == 0, == 1, == 2, != 2         drv:616's two sums and the masses by type
//   4       m                                          drv:636
//   5..7    m a_c                                      drv:465-468
//   8..10   m v_c
//   11      m ((vx^2 + vy^2) + vz^2)                   (the host halves the total)
//   12      E
//   13 + ty s + t   ((f[t] mus[t]) / rowsum) m where pt == ty, ty = 0, 1, 2     drv:656-658
// with rowsum = np.sum(f * mus) in NumPy's order (census_row_sum: phase_np_sum's order, sphx_phase_map.h).  A row outside
// a quantity's mask gives +0.0 BY SELECTION: its own values - a NaN mass, a zero row sum - never enter the quantity.
// drv:637 prints the gas quantity with the multiplication by the mass before the division; that form is not built.
#pragma once
#include <stddef.h>
#if defined(__clang__)
#pragma clang fp contract(off)       /* the terms are the reference's operations one by one */
#endif
#if defined(__HIPCC__)
#define SPHX_CEN_HD __host__ __device__
#else
#define SPHX_CEN_HD
#endif

#define SPHX_CEN_CHUNK 256       /* ids per chunk and lanes per workgroup (SPHX_TOT_CHUNK) */
#define SPHX_CEN_PITCH 257       /* doubles between two quantities' runs in the tile: the serial walks stay off one bank */
#define SPHX_CEN_TILE 29         /* quantities per tile: 29 x 257 x 8 B = 59 624 B of static LDS; s = 15 is two whole tiles */
#define SPHX_CEN_FIXED 13        /* quantities before the by-species ones */
enum { SPHX_CEN_M_GAS = 0, SPHX_CEN_M_STAR, SPHX_CEN_M_DUST, SPHX_CEN_M_NONDUST, SPHX_CEN_M_ALL, SPHX_CEN_MA, SPHX_CEN_MV = 8,
       SPHX_CEN_KIN2 = 11, SPHX_CEN_EINT = 12 };

SPHX_CEN_HD inline int sphx_cen_nq(int s) { return SPHX_CEN_FIXED + 3 * s; }
// place of row j (0 .. 255) of tile quantity tq (0 .. SPHX_CEN_TILE - 1)
SPHX_CEN_HD inline size_t sphx_cen_at(int tq, int j) { return (size_t)tq * SPHX_CEN_PITCH + (size_t)j; }
// tiles that cover nq quantities, and the quantities of tile t
SPHX_CEN_HD inline int sphx_cen_tiles(int nq) { return (nq + SPHX_CEN_TILE - 1) / SPHX_CEN_TILE; }
SPHX_CEN_HD inline int sphx_cen_tile_len(int nq, int t) {
    const int left = nq - t * SPHX_CEN_TILE;
    return left < SPHX_CEN_TILE ? left : SPHX_CEN_TILE;
}

// np.sum(f * mus) over a contiguous row of s < 128 values, NumPy's order: eight running sums over the whole blocks of
// eight, combined pairwise, then the rest one by one
SPHX_CEN_HD inline double sphx_cen_row_sum(int s, const double* f, const double* mus) {
    if (s < 8) {
        double res = 0.0;
        for (int t = 0; t < s; ++t) res += f[t] * mus[t];
        return res;
    }
    double r[8];
    for (int t = 0; t < 8; ++t) r[t] = f[t] * mus[t];
    int t = 8;
    for (; t < s - (s % 8); t += 8)
        for (int u = 0; u < 8; ++u) r[u] += f[t + u] * mus[t + u];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; t < s; ++t) res += f[t] * mus[t];
    return res;
}

struct SphxCenRow {
    double m, pt, vx, vy, vz, ax, ay, az, E;
    double rowsum;               // of the row's composition (unused where s == 0)
    const double* f;             // the composition row, or NULL
};

// term q of a row; s: species, mus: mu_specie
SPHX_CEN_HD inline double sphx_cen_term(const SphxCenRow& r, int q, int s, const double* mus) {
    switch (q) {
    case SPHX_CEN_M_GAS: return r.pt == 0.0 ? r.m : 0.0;
    case SPHX_CEN_M_STAR: return r.pt == 1.0 ? r.m : 0.0;
    case SPHX_CEN_M_DUST: return r.pt == 2.0 ? r.m : 0.0;
    case SPHX_CEN_M_NONDUST: return r.pt != 2.0 ? r.m : 0.0;
    case SPHX_CEN_M_ALL: return r.m;
    case SPHX_CEN_MA: return r.m * r.ax;
    case SPHX_CEN_MA + 1: return r.m * r.ay;
    case SPHX_CEN_MA + 2: return r.m * r.az;
    case SPHX_CEN_MV: return r.m * r.vx;
    case SPHX_CEN_MV + 1: return r.m * r.vy;
    case SPHX_CEN_MV + 2: return r.m * r.vz;
    case SPHX_CEN_KIN2: return r.m * ((r.vx * r.vx + r.vy * r.vy) + r.vz * r.vz);
    case SPHX_CEN_EINT: return r.E;
    default: break;
    }
    const int e = q - SPHX_CEN_FIXED, ty = e / s, t = e - ty * s;
    if (!r.f || r.pt != (double)ty) return 0.0;
    return ((r.f[t] * mus[t]) / r.rowsum) * r.m;
}
