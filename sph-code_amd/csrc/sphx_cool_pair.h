// sphx_cool_pair.h - rad_cooling's per-neighbour term (nsc:1044-1067), written once for the row pass and the transposed
// gather of sphx_cool.hip.
//
// A neighbour p enters through a 128-byte record of its OWN data: nothing below depends on the row but r^2, so the row
// pass (row j reading p) and the gather (p reading row j) form the same bits from the same r^2 - the masks of a pair
// agree between the two kernels by construction.
#pragma once
#include "sphx_weigh2.h"

struct alignas(128) CoolRec {
    double x, y, z;
    double h2;        // h(m)^2                                      nsc:675
    double cg;        // m*315*(m_0/m)^3 [type == 0]: the type mask of nsc:1044-1057 folded into Weigh2's factor
    double winv;      // 1 / Weigh2(x, x, m, d): the reference multiplies by [..]/Weigh2(x, x)   nsc:1048
    double mm;        // mu m_h (m_h, not amu)                       nsc:1044
    double f2, f3, f4, f5;                  // nan_to_num(f_un)[H, H+, He+, e-]
    double Hf, Hef, H2f;                    // recombination coefficients of nsc:1060-1062
    double eH, eHe;                         // energies per recombination of nsc:1066-1067
};
static_assert(sizeof(CoolRec) == 128, "one record, one 128-byte line");

// x [x > 0] of a nan_to_num'ed product (nsc:1044-1045): NaN and everything <= 0 give 0, +inf gives DBL_MAX
__device__ __forceinline__ double cool_pos(double v) { return v > 0.0 ? (v > DBL_MAX ? DBL_MAX : v) : 0.0; }

struct CoolPair {
    double relw;                            // rel_weights [rel_weights > 0]          nsc:1047-1048
    double ne, nHp, nHep, nH0;              // the four number densities, each [> 0]  nsc:1044-1057
};
// the five coefficients at temperature T (nsc:1038, 1060-1067); zero where T is not in (0, inf)
__device__ __forceinline__ void cool_coeffs(double T, double kB, CoolRec& r) {
#pragma clang fp contract(off)
    r.Hf = r.Hef = r.H2f = r.eH = r.eHe = 0.0;
    if (!(T > 0.0) || T > DBL_MAX) return;
    const double t4 = T / 10000.0, lt = log(t4);
    r.Hf = 4.13e-19 * pow(t4, -0.7131 - 0.0115 * lt);
    r.Hef = 2.72e-19 * pow(t4, -0.789);
    r.H2f = 7.3e-23 * 0.5 * sqrt(T / 100.0);
    r.eH = (0.684 - 0.0416 * lt + 0.54 * pow(t4, 0.37)) * kB * T;
    r.eHe = (0.684 - 0.0416 * log(t4 / 4.0)) * kB * T;
}
__device__ __forceinline__ CoolPair cool_pair(const CoolRec& p, double r2, double d9) {
#pragma clang fp contract(off)
    CoolPair o;
    const double W = weigh2_w(p.cg, p.h2 - r2, d9);                 // Weigh2 [type == 0]
    const double base = W / p.mm;
    o.ne = cool_pos(base * p.f5);
    o.nHp = cool_pos(base * p.f3);
    o.nHep = cool_pos(base * p.f4);
    o.nH0 = cool_pos(base * p.f2);
    o.relw = W > 0.0 ? (W > DBL_MAX ? DBL_MAX : W) * p.winv : 0.0;
    return o;
}
