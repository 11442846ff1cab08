// sphx_radphase_pair.h - the per-particle formulas of the radiative block of the reference's time loop,
// code_running.py:247-316 ("drv") with the composition chemistry of rad_heating, navier_stokes_cleaned.py:977-1012 ("nsc"),
// written once: the kernels of sphx_radphase.hip run them on a row staged in LDS, tests/host/radphase_check.cpp on the host.
//
// A row is one particle's composition, s contiguous doubles.  Every operation is rounded on its own, in the order the
// driver's NumPy expression has it (the including file switches contraction off); sums over the species run t = 0 .. s-1.
//   sphx_rp_ionise_row     nsc:976-1011 for one non-star particle: the three destroyed fractions that are ever read and
//                          the forward reactions, in place
//   sphx_rp_normalise_row  nsc:1012 (every particle): the row divided by its sum, the sum taken t = 0 .. s-1 as
//                          np.sum(.., axis=0) of the (S,N) array takes it
//   sphx_rp_tables         drv:258-260 / 283-285: mu, gamma, cross = sum f table / sum f
//   sphx_rp_coeff          drv:263-266 / 293-295: nan_to_num(x), then + 1 where >= 0, exp where < 0
//   sphx_rp_clamp          drv:270-273 / 308-311: E to [t_cmb, t_max] (gamma m k) / (mu m_h), T to [t_cmb, t_max]
//   sphx_rp_heat           drv:263-273 for one particle
//   sphx_rp_cool           drv:286-311 for one particle
#pragma once
#include <float.h>
#include <math.h>
// every operation below is rounded on its own, as the driver's NumPy rounds it: no fused multiply-add.  (The pragma has
// to stand before the functions it is to govern - in this header, not behind its #include; it holds to the end of the
// including file, which wants it anyway.)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#if defined(__HIPCC__)
#define SPHX_RP_HD __host__ __device__
#else
#define SPHX_RP_HD
#endif
#define SPHX_RP_PI 3.141592653589793           // np.pi

// np.nan_to_num of one value: NaN -> 0, +-inf -> +-DBL_MAX
SPHX_RP_HD inline double sphx_rp_nan_to_num(double v) {
    if (v != v) return 0.0;
    if (v > DBL_MAX) return DBL_MAX;
    if (v < -DBL_MAX) return -DBL_MAX;
    return v;
}

// nsc:976-1011.  f: the row (in: f_un, out: new_fun2 before nsc:1012).  mass, lf2: the particle's; ppj: photons per joule
// (the scalar nsc:976 multiplies lf2 by); fd3: frac_dest of species 0, 1, 2; mus, cs: mu_specie and cross_sections (s each).
// frac[3] (nullable): frac_destroyed_by_species of species 0, 1, 2.
SPHX_RP_HD inline void sphx_rp_ionise_row(int s, double* f, double mass, double lf2, double ppj, const double* fd3, const double* mus,
                                          const double* cs, double amu, double* frac) {
    const double n_photons = ppj * lf2;                                      // nsc:976
    double smu = 0.0, scs = 0.0;
    for (int t = 0; t < s; ++t) {
        const double a = f[t] * mus[t] * amu, b = cs[t] * f[t];
        smu = t ? smu + a : a; scs = t ? scs + b : b;
    }
    const double mols = mass / smu;                                          // nsc:977
    double fr[3];
    for (int t = 0; t < 3; ++t) {
        const double wi = f[t] * cs[t] / scs;                                // nsc:979
        const double ad = wi * fd3[t] * n_photons;                           // nsc:980
        const double at = f[t] * mols;                                       // nsc:981
        const double x0 = sphx_rp_nan_to_num(ad / at);                       // nsc:983
        const double x1 = exp(-x0) * 0.99;                                   // nsc:985
        double v = sphx_rp_nan_to_num(0.99 - x1);                            // nsc:986
        const double q = at / amu;
        if (q < 1e-10) v = 0.0;                                              // nsc:987
        if (q < 0.0) v = 0.99;                                               // nsc:988
        fr[t] = v;
        if (frac) frac[t] = v;
    }
    const double o0 = f[0], o1 = f[1], o2 = f[2];
    const double p0 = o0 * fr[0], p1 = o1 * fr[1], p2 = o2 * fr[2];
    double n2 = o2 + p0 * 2.;                                                // nsc:999
    f[3] = f[3] + p2;                                                        // nsc:1001
    f[4] = f[4] + p1;                                                        // nsc:1002
    f[5] = f[5] + (p2 + p1);                                                 // nsc:1003
    f[0] = o0 - p0;                                                          // nsc:1005
    f[1] = o1 - p1;                                                          // nsc:1006
    n2 = n2 - p2;                                                            // nsc:1007
    f[2] = n2;
}

// nsc:1012
SPHX_RP_HD inline void sphx_rp_normalise_row(int s, double* f) {
    double tot = f[0];
    for (int t = 1; t < s; ++t) tot += f[t];
    for (int t = 0; t < s; ++t) f[t] = f[t] / tot;
}

// drv:258-260 / 283-285
SPHX_RP_HD inline void sphx_rp_tables(int s, const double* f, const double* mus, const double* gam, const double* cs, double* mu,
                                      double* gamma, double* cross) {
    double a = 0.0, b = 0.0, c = 0.0, sf = 0.0;
    for (int t = 0; t < s; ++t) {
        const double v = f[t], ta = v * mus[t], tb = v * gam[t], tc = v * cs[t];
        a = t ? a + ta : ta; b = t ? b + tb : tb; c = t ? c + tc : tc; sf = t ? sf + v : v;
    }
    *mu = a / sf; *gamma = b / sf; *cross = c / sf;
}

// drv:263-266 / 293-295 on the quotient x
SPHX_RP_HD inline double sphx_rp_coeff(double x) {
    x = sphx_rp_nan_to_num(x);
    return x >= 0.0 ? x + 1. : exp(x);
}

struct SphxRpConst { double t_cmb, t_max, k, m_h, sb, cooling_timescale, dt; };
// what a particle's clamps did: bit 0 E raised, 1 E lowered, 2 T raised, 3 T lowered
enum { SPHX_RP_E_LO = 1, SPHX_RP_E_HI = 2, SPHX_RP_T_LO = 4, SPHX_RP_T_HI = 8 };

// drv:270-273 / 308-311; mu and gamma are the new ones
SPHX_RP_HD inline int sphx_rp_clamp(const SphxRpConst& c, double mass, double mu, double gamma, double* E, double* T) {
    int hit = 0;
    const double gmk = gamma * mass * c.k, mm = mu * c.m_h;
    const double lo = c.t_cmb * gmk / mm, hi = c.t_max * gmk / mm;
    if (*E < lo) { *E = lo; hit |= SPHX_RP_E_LO; }
    if (*E > hi) { *E = hi; hit |= SPHX_RP_E_HI; }
    if (*T < c.t_cmb) { *T = c.t_cmb; hit |= SPHX_RP_T_LO; }
    if (*T >= c.t_max) { *T = c.t_max; hit |= SPHX_RP_T_HI; }
    return hit;
}

// drv:263-273.  ptype: the particle's type; lf2: its deposited energy (read where ptype == 0); mu_before: the mu_array of
// drv:248, from before the heating (N_PART at drv:268 is that line's value); mu, gamma: drv:258-259's.
SPHX_RP_HD inline int sphx_rp_heat(const SphxRpConst& c, double ptype, double mass, double lf2, double mu_before, double mu, double gamma,
                                   double* E, double* T) {
    if (ptype == 0.0) {
        const double c0 = sphx_rp_coeff(lf2 / *E);                            // drv:263-266
        *E = *E * c0;                                                        // drv:267
        const double n_part = mass / (c.m_h * mu_before);                    // drv:248
        *T = *E / (n_part * gamma * c.k);                                    // drv:268
    }
    return sphx_rp_clamp(c, mass, mu, gamma, E, T);
}

// drv:286-311.  energy: rad_cooling's, per particle; lf2, mom: rad_heating's for this particle (read where ptype != 1);
// mu, gamma, cross: drv:283-285's.  vel: the particle's three components, in place.
SPHX_RP_HD inline int sphx_rp_cool(const SphxRpConst& c, double ptype, double mass, double size, double energy, double lf2,
                                   const double* mom, double mu, double gamma, double cross, double* E, double* T, double* vel) {
    const double n_part = mass / (c.m_h * mu);                               // drv:289
    if (ptype == 0.0) {
        double c1 = sphx_rp_coeff(-(energy * n_part) / *E);                   // drv:293-295
        c1 = c1 * exp(-c.dt / c.cooling_timescale * sqrt(*T / 1e4));         // drv:296
        *E = *E * c1;                                                        // drv:297
        *T = *E / (n_part * gamma * c.k);                                    // drv:298
    } else if (ptype == 2.0) {
        const double optical_depth = n_part * cross;                         // drv:286
        const double area = 4 * SPHX_RP_PI * (size * size);                  // drv:288
        const double w6 = 9. / area;                                         // drv:290
        const double optd = 1. - exp(-optical_depth * w6);                   // drv:291
        const double den = optd * 4 * SPHX_RP_PI * (size * size) * c.sb * 1e-5 * c.dt;
        *T = pow(lf2 / den + pow(c.t_cmb, 1. / 6.), 1. / 6.);                // drv:300
        *E = n_part * c.k * *T * gamma;                                      // drv:301
    }
    if (ptype != 1.0) { vel[0] += mom[0]; vel[1] += mom[1]; vel[2] += mom[2]; }      // drv:303
    return sphx_rp_clamp(c, mass, mu, gamma, E, T);
}
