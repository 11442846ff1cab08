// sphx_weigh2.h - Weigh2 of the loop forms (nsc:673-676), written once for sphx_loopforms.hip and sphx_cool.hip:
//   W = m*315*(m_0/m)^3*((m/m_0)^(2/3) d^2 - r^2)^3/(64 pi d^9)
// in three pieces, so that a kernel may keep the per-particle pieces in a record; weigh2() is their composition and its
// operations, in their order, are the reference's.  NumPy never fuses a multiply into an add: every function keeps its
// operations separately rounded, whatever the including file's setting.
#pragma once

#define PI64 201.06192982974676      /* 64 pi */

__device__ __forceinline__ double pow9(double d) {
#pragma clang fp contract(off)
    double d2 = d * d, d4 = d2 * d2;
    return d4 * d4 * d;
}
// h(m)^2 = (m/m_0)^(2/3) d^2
__device__ __forceinline__ double weigh2_h2(double m, double d, double m0) {
#pragma clang fp contract(off)
    return pow(m / m0, 2.0 / 3.0) * (d * d);
}
// m*315*(m_0/m)^3
__device__ __forceinline__ double weigh2_c(double m, double m0) {
#pragma clang fp contract(off)
    const double a = m0 / m;
    return m * 315.0 * (a * a * a);
}
// c q^3 / (64 pi d^9), q = h(m)^2 - r^2
__device__ __forceinline__ double weigh2_w(double c, double q, double d9) {
#pragma clang fp contract(off)
    return c * (q * q * q) / (PI64 * d9);
}
__device__ __forceinline__ double weigh2(double r2, double m, double d, double m0, double d9) {
#pragma clang fp contract(off)
    return weigh2_w(weigh2_c(m, m0), weigh2_h2(m, d, m0) - r2, d9);
}
