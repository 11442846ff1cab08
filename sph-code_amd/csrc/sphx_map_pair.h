// sphx_map_pair.h - the arithmetic of the projected maps (sphx_map.hip), as host and device code: the pixel-centre
// expression, a particle's footprint, the range of pixels its bounding box holds, the pair term and what a pixel does
// with it.  tests/host/map_check.cpp replays the tile walk on the host with the same functions; include/sphx.h has the
// definitions.  Every operation is rounded on its own (no contraction): the tests restate them in NumPy, one by one.
#pragma once
#include <math.h>
#include <stddef.h>
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#define SPHX_MAP_HD __host__ __device__
#else
#define SPHX_MAP_HD
#endif

#define SPHX_MAP_TILE 16                     /* a tile is 16 x 16 pixels: one pixel per lane of a 256-lane workgroup */
#define SPHX_MAP_BATCH 256                   /* records of a tile's list staged through LDS at a time */
#define SPHX_MAP_C 1.4323944878270580        /* 9 / (2 pi) = (32/35) 315 / (64 pi) */
#define SPHX_MAP_MAXPIX (1ll << 28)          /* n_u n_v beyond this: SPHX_E_ARG */
enum { SPHX_MAP_GAS_COLUMN = 1, SPHX_MAP_DUST_COLUMN = 2, SPHX_MAP_GAS_T = 4, SPHX_MAP_DUST_T = 8, SPHX_MAP_COUNT = 16 };

// centre of pixel i of n along an axis of centre c and half-width w: c - w + (i + 1/2) 2 w / n, left to right
SPHX_MAP_HD inline double sphx_map_centre(double c, double w, int n, int i) {
    return c - w + ((double)i + 0.5) * 2.0 * w / (double)n;
}
// neither NaN nor inf
SPHX_MAP_HD inline bool sphx_map_finite(double v) { return v - v == 0.0; }

// What a particle lays on the image: its projected position, R^2, c = m (9 / 2 pi) R^-9, its temperature, gas or dust.
struct SphxMapRec { double xu, xv, R2, c, T, gas; };        // gas: 1.0 or 0.0 (six doubles: no padding to copy)
// R of a row: h(m) = (m / m_0)^(1/3) d for gas (type 0), sizes for dust (type 2); no other type has one (returns false)
SPHX_MAP_HD inline bool sphx_map_radius(double type, double m, double size, double d, double m0, double* R) {
    if (type == 0.0) { *R = cbrt(m / m0) * d; return true; }
    if (type == 2.0) { *R = size; return true; }
    return false;
}
// a row that never counts: a NaN or infinite coordinate, mass or radius, or R <= 0
SPHX_MAP_HD inline bool sphx_map_row_bad(double xu, double xv, double xw, double m, double R) {
    return !(sphx_map_finite(xu) && sphx_map_finite(xv) && sphx_map_finite(xw) && sphx_map_finite(m) && sphx_map_finite(R) && R > 0.0);
}
// R^-9 enters once per particle, here
SPHX_MAP_HD inline double sphx_map_coeff(double m, double R) {
    const double r2 = R * R, r4 = r2 * r2;
    return m * SPHX_MAP_C / (r4 * r4 * R);
}
// The pixels i of [0, n) with |u_i - x| <= R are lo .. hi (lo > hi: none).  u_i does not decrease with i and rounding
// keeps that order, so both ends are found by bisection on the pixel centres themselves: no estimate, no edge case.
SPHX_MAP_HD inline void sphx_map_span(double c, double w, int n, double x, double R, int* lo, int* hi) {
    int a = 0, b = n;                                    // first i with not (u_i - x < -R)
    while (a < b) {
        const int mid = a + (b - a) / 2;
        if (sphx_map_centre(c, w, n, mid) - x < -R) a = mid + 1; else b = mid;
    }
    *lo = a;
    b = n;                                               // first i >= lo with u_i - x > R
    while (a < b) {
        const int mid = a + (b - a) / 2;
        if (sphx_map_centre(c, w, n, mid) - x > R) b = mid; else a = mid + 1;
    }
    *hi = a - 1;
}
// s = R^2 - b^2 of a (particle, pixel) pair
SPHX_MAP_HD inline double sphx_map_s(const SphxMapRec& r, double u, double v) {
    const double du = u - r.xu, dv = v - r.xv;
    return r.R2 - (du * du + dv * dv);
}
// sigma = c s^3 sqrt(s), for s > 0
SPHX_MAP_HD inline double sphx_map_term(double c, double s) { return c * (s * s * s * sqrt(s)); }

// A pixel's sums.  want: the SPHX_MAP_* bits of the outputs asked for; a sum nobody reads is not formed.
struct SphxMapAcc { double gc, dc, gn, gd, dn, dd; int cnt; };
SPHX_MAP_HD inline void sphx_map_acc_zero(SphxMapAcc& a) { a.gc = a.dc = a.gn = a.gd = a.dn = a.dd = 0.0; a.cnt = 0; }
SPHX_MAP_HD inline void sphx_map_add(SphxMapAcc& a, const SphxMapRec& r, double u, double v, int want) {
    const double s = sphx_map_s(r, u, v);
    if (!(s > 0.0)) return;
    const double t = sphx_map_term(r.c, s);
    a.cnt += 1;
    // (each sum is replaced by a selected VALUE: a choice between two sums' addresses would put them in memory)
    const bool gas = r.gas != 0.0;
    const double tt = t * r.T;
    if (want & SPHX_MAP_GAS_COLUMN) a.gc = gas ? a.gc + t : a.gc;
    if (want & SPHX_MAP_DUST_COLUMN) a.dc = gas ? a.dc : a.dc + t;
    if (want & SPHX_MAP_GAS_T) {
        const bool in = gas && tt > 0.0;                 // temperature_arb's mask, nsc:1474-1480
        a.gn = in ? a.gn + tt : a.gn;
        a.gd = in ? a.gd + t : a.gd;
    }
    if (want & SPHX_MAP_DUST_T) {
        const bool in = !gas && t > 0.0;
        a.dn = in ? a.dn + tt : a.dn;
        a.dd = in ? a.dd + t : a.dd;
    }
}
// a ratio of the epilogue: 0 where nothing entered the denominator
SPHX_MAP_HD inline double sphx_map_ratio(double num, double den) { return den == 0.0 ? 0.0 : num / den; }
