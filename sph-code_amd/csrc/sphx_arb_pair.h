// sphx_arb_pair.h - the arithmetic of ONE (query point, particle) pair of the arbitrary-point samplers (nsc:1422-1527:
// density_arb, dust_density_arb, temperature_arb, dust_temperature_arb, photoionization_arb), written once for the grid
// form (sphx_arb.hip: arb_grid_kernel, records staged through LDS) and the list form (arb_list_kernel, records gathered
// by the caller's ids), with the gate and the quotients both forms end on.  The two forms differ in where a record comes
// from and in which pairs they meet - never in an expression.
//
// Weights (nsc:673-681), in the library's form W = f (1 - q^2)^3 with q^2 = r^2 / h^2 and f = m C / h^3:
//   gas   Wg = m C h(m)^-9 (h(m)^2 - r^2)^3,  h(m) = (m / m_0)^(1/3) d;   dust  Wd = m C s^-9 (s^2 - r^2)^3, s = sizes.
// Neither is clipped: the cube keeps the sign and the reference's "> 0" masks do the clipping.
#pragma once
#include "sphx_internal.h"
// every operation separately rounded, as in sphx_pair.h: the masks "> 0" sit on the cancellation 1 - q^2
#pragma clang fp contract(off)

// What a particle contributes, whichever point asks (built once per call by arb_record_kernel).  12 doubles = 96 B.
struct ArbRec {
    double x, y, z;
    double sup;     // support radius max(h(m) [gas], s [dust]); < 0: listed among the wide particles instead (grid form)
    double fg;      // m C / h(m)^3 [type == 0]
    double ihg;     // 1 / h(m)^2
    double fd;      // m C / s^3 [type == 2]   (0 without sizes)
    double ihd;     // 1 / s^2
    double T;       // temperature             (0 without T)
    double pw;      // [type == 0] N_PART       (0 without n_part / value)
    double val;     // nan_to_num(photoionization), nsc:1523
    double pad;
};

// the sums of one query point: density_arb | temperature_arb's numerator, denominator | dust_density_arb (which is
// dust_temperature_arb's denominator: the same masked sum) | its numerator | photoionization_arb's numerator, denominator
struct ArbAcc {
    double dens, tn, td, dd, dtn, pn, pd;
    int cnt;        // members of the ball met (list form: not used)
};
__device__ __forceinline__ ArbAcc arb_acc_zero() { return ArbAcc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0}; }

// r2 = |x_k - x_0|^2.  R2: the ball's squared radius (grid form; a particle outside it is not on the list the reference
// would have been given) or +inf (list form: whatever is listed counts).  A NaN distance fails the test.
// clip: the grid form's reading of the two masks that a negative factor can turn round.  temperature_arb masks on the
// sign of Wg T and photoionization_arb on that of the ratio times N_PART: with T_k < 0 (N_PART_k < 0) a particle OUTSIDE
// its own support, where the unclipped weight is negative, passes them - anywhere in the ball.  The grid form never
// visits such a pair on purpose (its cost follows the supports), so there it must not count when it is met by chance:
// clip demands a positive weight as well.  For T >= 0 and N_PART >= 0 - every physical state - nothing changes; the
// list form (clip = false) keeps the reference's masks as they are.
template <bool clip>
__device__ __forceinline__ void arb_pair(ArbAcc& a, double r2, double R2, double fg, double ihg, double fd, double ihd,
                                         double T, double pw, double val) {
    if (!(r2 <= R2)) return;
    a.cnt += 1;
    const double tg = 1.0 - r2 * ihg;
    const double g3 = tg * tg * tg;
    const double Wg = fg * g3;                              // Weigh2 * [type == 0]                 nsc:1437
    if (Wg > 0.0) a.dens += Wg;                             // nsc:1439
    const double at = Wg * T;                               // nsc:1474
    if (at > 0.0 && (!clip || Wg > 0.0)) { a.tn += at; a.td += Wg; }     // the mask is the NUMERATOR's sign   nsc:1480
    const double td = 1.0 - r2 * ihd;
    const double Wd = fd * (td * td * td);                  // Weigh2_dust * [type == 2]            nsc:1455, 1501
    if (Wd > 0.0) { a.dd += Wd; a.dtn += Wd * T; }          // nsc:1457, 1504
    const double w = g3 * pw;                               // Weigh2(x, x_0) / Weigh2(x, x) [gas] N_PART   nsc:1521
    if (w > 0.0 && (!clip || g3 > 0.0)) { a.pn += w * val; a.pd += w; }  // nsc:1523
}

// the reference's gate (a row of at most one member returns 0 from every function, nsc:1432) and its quotients
struct ArbOut { double density, dust_density, temperature, dust_temperature, photoionization; };
__device__ __forceinline__ ArbOut arb_finish(const ArbAcc& a, bool gate) {
    ArbOut o{0.0, 0.0, 0.0, 0.0, 0.0};
    if (!gate) return o;
    o.density = a.dens;
    o.dust_density = a.dd;
    o.temperature = sphx_nan_to_num(a.tn / a.td);           // nsc:1480
    o.dust_temperature = sphx_nan_to_num(a.dtn / a.dd);     // nsc:1504
    o.photoionization = a.pn / a.pd;                        // no nan_to_num: 0/0 stays NaN         nsc:1523
    return o;
}
