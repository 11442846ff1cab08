// sphx_chem_pair.h - the formulas of chemisputtering_2 (nsc:1265-1416), written once for the kernels of sphx_chem.hip.
//
// A list entry p enters through a 64-byte record of its OWN data (ChemRec): the gas weight of a pair depends on the row
// through r^2 alone.  Every operation is separately rounded, in the reference's order; NaN goes where NumPy sends it.
#pragma once
#include "sphx_weigh2.h"

#define CHEM_FIRST 6                    /* columns below are left alone: F_sput = 1, reuptake weight 0 (nsc:1326, 1343) */

struct alignas(64) ChemRec {
    double x, y, z;
    double h2;        // h(m)^2 = (m/m_0)^(2/3) d^2                  nsc:675
    double cg;        // m*315*(m_0/m)^3
    double mu;        // mu_array (the INPUT mu divides the weight; num_particles is divided by the recomputed one)
    double T;         // T, 2.73 for a star                           nsc:1282
    double type;      // particle_type
};
static_assert(sizeof(ChemRec) == 64, "one record, half a 128-byte line");

// the per-species tables on the device, s entries each
struct ChemTab {
    const double* mu;     // mu_specie
    const double* j0;     // -diff(mrn^-0.5) / diff(mrn^0.5) / (3 mineral_densities)       nsc:1305
    const double* b;      // 2 pi mu_specie amu                                             nsc:1306
    const double* sy;     // sputtering_yields
    double symax, kB, dt;
};

__device__ __forceinline__ double chem_r2(const ChemRec& p, double x, double y, double z) {
#pragma clang fp contract(off)
    const double dx = p.x - x, dy = p.y - y, dz = p.z - z;
    return dx * dx + dy * dy + dz * dz;
}
// w2g_num of a GAS entry: v (v > 0) with v = Weigh2 / mu - NaN stays NaN, as NumPy's product with a bool keeps it  nsc:1284, 1290
__device__ __forceinline__ double chem_weight(const ChemRec& p, double r2, double d9) {
#pragma clang fp contract(off)
    const double v = weigh2_w(p.cg, p.h2 - r2, d9) / p.mu;
    return v * (v > 0.0 ? 1.0 : 0.0);
}
// min(max(a exp(-4600 / T), lo), hi) with Python's min and max: a NaN first argument stays   nsc:1308-1309
__device__ __forceinline__ double chem_yield(double a, double T, double lo, double hi) {
#pragma clang fp contract(off)
    const double y = a * exp(-4600.0 / T);
    const double m = lo > y ? lo : y;
    return hi < m ? hi : m;
}
// F_sput of column s of a row (nsc:1303-1325): scd = the gas's SPH composition density there, scd3 and scd4 those of H+
// and He+, dc = the row's own dust density of the species
__device__ __forceinline__ double chem_fsput(const ChemTab& t, int s, double scd, double scd3, double scd4, double dc, double T) {
#pragma clang fp contract(off)
    const double J = t.j0[s] * sqrt(t.kB * T / t.b[s]);
    const double YH = chem_yield(0.5, T, 1e-7, 1e-3) * t.sy[s] / t.symax;
    const double YHe = chem_yield(5.0, T, 1e-6, 1e-2) * t.sy[s] / t.symax;
    double sput = (scd3 / t.mu[3] * YH + scd4 * YHe / t.mu[4]) * t.mu[s];
    if (sput > dc) sput = dc;                                            // "cannot sputter more mass than exists"
    const double Ku = scd + dc - sput;
    const double E = exp(Ku * J * t.dt);
    const double Lu = scd + dc * E - sput;
    double F = Ku / Lu;
    F = F * E;
    if (F != F) F = 1.0;                                                 // exp overflow: inf / inf -> 1
    if (F < 0.01) F = 0.01;
    return F;
}
// clamps 1 and 2 of a first-stage loss against the entry's count as it stands (nsc:1382-1384) -> the clamped loss
__device__ __forceinline__ double chem_clamp12(double cnt, double loss, unsigned& c1, unsigned& c2) {
#pragma clang fp contract(off)
    if (cnt - loss < 0.01 * cnt) { loss = 0.99 * cnt; ++c1; }
    if (cnt < 0.0) { loss = cnt; ++c2; }
    return loss;
}
// clamp 3 of the row's summed loss against its own count (nsc:1387)
__device__ __forceinline__ double chem_clamp3(double own, double tot, unsigned& c3) {
#pragma clang fp contract(off)
    if (tot + own < 0.01 * own) { tot = -0.99 * own; ++c3; }
    return tot;
}
