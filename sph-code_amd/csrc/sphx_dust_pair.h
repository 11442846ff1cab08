// sphx_dust_pair.h - supernova_destruction's per-pair term (nsc:1232-1251), written once for the list kernel, the dust
// pass and the row pass of sphx_dust.hip.
//
// A dust entry i enters through a 128-byte record of its OWN data; beside it a pair needs the row's position, velocity
// and density.  The three kernels form r^2 and |dv|^2 by dust_r2 on the same operands in the same order, so a pair's
// masks, its efficiency and its lost atoms are the same bits wherever they are formed.
#pragma once
#include "sphx_weigh2.h"

struct alignas(128) DustRec {
    double x, y, z;
    double vx, vy, vz;
    double s2;        // sizes^2                                                      nsc:680
    double cw;        // m*315 [m > crit_mass]: the mass mask of nsc:1237 folded into Weigh2_dust's factor
    double den;       // 64 pi sizes^9
    double w0;        // Weigh2_dust(x, x): m*315*(sizes^2)^3 / den, unmasked          nsc:1234
    double N;         // m / (mu amu)                                                 nsc:1247
    double C;         // [m > crit_mass] as 0.0 / 1.0                                 nsc:1244
    double pad_[4];
};
static_assert(sizeof(DustRec) == 128, "one record, one 128-byte line");

// the 8 knots of the two efficiency curves and their 7 slopes, (y[t + 1] - y[t]) / (v[t + 1] - v[t]) formed on the host
struct DustKnots { double v[8], c[8], si[8], sc[7], ssi[7]; };

// (a_x - b_x)^2 + (a_y - b_y)^2 + (a_z - b_z)^2, left to right
__device__ __forceinline__ double dust_r2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return dx * dx + dy * dy + dz * dz;
}
// rho = wd [wd > 0] with the mass mask folded in; a NaN wd stays NaN (NaN x False)        nsc:1232, 1237
__device__ __forceinline__ double dust_rho(const DustRec& p, double r2) {
#pragma clang fp contract(off)
    const double q = p.s2 - r2;
    const double wd = p.cw * (q * q * q) / p.den;
    return wd * (wd > 0.0 ? 1.0 : 0.0);
}

struct DustPair {
    double ratio;     // nan_to_num(rho / w0)                                          nsc:1242
    double g;         // dens_j C_i / critical_density                                 nsc:1244
    double ec, esi;   // the two curves at v = |dv| / 1000                             nsc:1241-1242
};
// np.interp between the knots: 0 outside [v_0, v_7], the last knot inside, a NaN stays a NaN
__device__ __forceinline__ void dust_eff(const DustKnots& kn, double v, double& ec, double& esi) {
#pragma clang fp contract(off)
    if (v != v) { ec = esi = v; return; }
    if (v < kn.v[0] || v > kn.v[7]) { ec = esi = 0.0; return; }
    if (v == kn.v[7]) { ec = kn.c[7]; esi = kn.si[7]; return; }
    double v0 = kn.v[0], c0 = kn.c[0], s0 = kn.si[0], mc = kn.sc[0], ms = kn.ssi[0];
#pragma unroll
    for (int t = 1; t < 7; ++t)
        if (v >= kn.v[t]) { v0 = kn.v[t]; c0 = kn.c[t]; s0 = kn.si[t]; mc = kn.sc[t]; ms = kn.ssi[t]; }
    const double dv = v - v0;
    ec = mc * dv + c0;
    esi = ms * dv + s0;
}
__device__ __forceinline__ DustPair dust_pair(const DustRec& p, double r2, double dv2, double dens_j, double crit_density,
                                              const DustKnots& kn) {
#pragma clang fp contract(off)
    DustPair o;
    o.ratio = sphx_nan_to_num(dust_rho(p, r2) / p.w0);
    o.g = dens_j * p.C / crit_density;
    dust_eff(kn, sqrt(dv2) / 1000.0, o.ec, o.esi);
    return o;
}
// the fraction of species t destroyed, capped (a NaN stays a NaN), and whether the cap acted      nsc:1242-1245
__device__ __forceinline__ double dust_ff(const DustPair& pr, double eff, bool& capped) {
#pragma clang fp contract(off)
    const double ff = pr.g * (eff * pr.ratio);
    capped = ff >= 0.99;
    return capped ? 0.99 : ff;
}
// atoms of species t lost: (ff f_un[i,t]) N_i                                                   nsc:1251
__device__ __forceinline__ double dust_lost(double ff, double f, double N) {
#pragma clang fp contract(off)
    return ff * f * N;
}
