// sphx_pair.h - the arithmetic of ONE neighbour in hydro_update's sums (nsc:556-671, 719-742), written once for the
// gather kernels (sphx_sums.hip: one thread per particle) and the LDS kernels (sphx_blob.hip: LPP lanes per particle),
// with what both forms share around it: the 32-B record pieces, the fixed order of the partial sums, the crossing-time
// vote and its workgroup minimum.  The two forms differ in where a record comes from and in who holds which partial
// sum - never in an expression, which is why they agree bit for bit.
//
// Sqrt: the square root of the distances is a parameter of every term.  The gather kernels pass SqrtLib (the library's
// sqrt), the LDS kernels SqrtMid (sphx_blob.h: sqrt_mid, the same sequence without range checks); the bit-identity tests
// between the two forms are what proves sqrt_mid equal to sqrt() on the range - keep them apart.
// clip: the neighbour-side gradient is zero beyond h_j (nsc:689); a compile-time constant in the LDS kernels.
#pragma once
#include "sphx_internal.h"
// NumPy never fuses a multiply into an add: keep every operation separately rounded so that
// cancellations such as h_j^2 - r^2 at the kernel edge reproduce the reference bit for bit.
#pragma clang fp contract(off)

// 32-B pieces of a record, loaded as two 16-B vectors each
struct Q4 { double a, b, c, d; };
__device__ __forceinline__ Q4 gload4(const double* p) {
    const double2 lo = *reinterpret_cast<const double2*>(p);
    const double2 hi = *reinterpret_cast<const double2*>(p + 2);
    return Q4{lo.x, lo.y, hi.x, hi.y};
}

// (p0 + p1) [+ (p2 + p3)]: the order in which the partial sums over the list positions k mod SPHX_SUM_PARTS are added,
// in the gather kernels (here) and by the lane groups of the LDS kernels (sphx_blob.h: group_total)
__device__ __forceinline__ double parts_total(const double (&a)[SPHX_SUM_PARTS]) {
    if (SPHX_SUM_PARTS == 4) return (a[0] + a[1]) + (a[2] + a[3]);
    return a[0] + a[SPHX_SUM_PARTS - 1];
}
// ... of one member of the partial accumulators
template <class Acc>
__device__ __forceinline__ double parts_total(const Acc (&a)[SPHX_SUM_PARTS], double Acc::*f) {
    double v[SPHX_SUM_PARTS];
#pragma unroll
    for (int q = 0; q < SPHX_SUM_PARTS; ++q) v[q] = a[q].*f;
    return parts_total(v);
}

struct SqrtLib { __device__ __forceinline__ double operator()(double x) const { return sqrt(x); } };

// ---- the poly6 kernel of a pair ------------------------------------------------------------------------
// the ROUNDED distance, squared again (nsc:586; nsc:588 squares the rounded distance)
template <class Sqrt>
__device__ __forceinline__ double dist_sq(double rr) {
    const double r = Sqrt()(rr);
    return r * r;
}
// W = max(c1_j (h_j^2 - r^2)^3, 0)                                                       nsc:588-589
__device__ __forceinline__ double poly6_w(double c1, double qj) {
    const double W = c1 * (qj * qj * qj);
    return (W < 0.0) ? 0.0 : W;
}
// the gradients' coefficients of (dx, dy, dz): neighbour side c_b (h_j; nsc:591, not clipped - clip: nsc:689) and own
// side c_a (nsc:592), ci = -6 c1_i
struct GradPair { double cb, ca; };
__device__ __forceinline__ GradPair grad_pair(double r2, double qj, double c1_j, double hi2, double ci, bool clip) {
    const double qi = hi2 - r2;
    return GradPair{(clip && !(qj > 0.0)) ? 0.0 : -6.0 * c1_j * (qj * qj), ci * (qi * qi)};
}

// the species weight Nw_j W_ij alone (nsc:626); q0 = {x y z h2}
template <class Sqrt>
__device__ __forceinline__ double species_weight(const Q4& q0, double c1, double Nw, double xr, double yr, double zr) {
    const double dx = q0.a - xr, dy = q0.b - yr, dz = q0.c - zr;
    return Nw * poly6_w(c1, q0.d - dist_sq<Sqrt>(dx * dx + dy * dy + dz * dz));
}

// the metallicity expression of drv:663 on a particle's SPH-smoothed composition F[0 .. S): the mass in species >= 6 over
// the mass in all of them (0/0 -> NaN for a particle without gas neighbours)
template <int N>
__device__ __forceinline__ double species_metallicity(const AgbTable& agb, const double (&F)[N], int S) {
    double heavy = 0.0, all = 0.0;
#pragma unroll
    for (int t = 0; t < N; ++t) {
        if (t < S) {
            const double w = F[t] * agb.mu[t];
            all += w;
            if (t >= 6) heavy += w;
        }
    }
    return heavy / all;
}

// ---- pass 1: rho, rho_dust, n, grad P        nsc:586-615 ------------------------------------------------
struct DensAcc { double rho, rd, n, gx, gy, gz; };
// q0 = {x y z h2}, q1 = {c1 ms A Nw} of the neighbour; (xr, yr, zr) the reference point, hi2, ci = -6 c1_i, Ai the
// particle's own.  Returns the species weight Nw_j W_ij (nsc:626).
template <class Sqrt>
__device__ __forceinline__ double density_term(DensAcc& a, const Q4& q0, const Q4& q1, double xr, double yr, double zr,
                                               double hi2, double ci, double Ai, bool clip) {
    const double dx = q0.a - xr, dy = q0.b - yr, dz = q0.c - zr;
    const double r2 = dist_sq<Sqrt>(dx * dx + dy * dy + dz * dz);
    const double qj = q0.d - r2;
    const double c1 = q1.a, ms = q1.b, Aj = q1.c, Nw = q1.d;
    const double W = poly6_w(c1, qj);
    const GradPair g = grad_pair(r2, qj, c1, hi2, ci, clip);
    a.rho += fmax(ms, 0.0) * W;                           // nsc:605
    a.rd += fmax(-ms, 0.0) * W;                           // nsc:606
    const double nww = Nw * W;
    a.n += nww;                                           // nsc:607
    // nsc:615, the pair's common factor taken out of the three components: (A_j g_b + A_i g_a) / 2 = t (dx, dy, dz) with
    // t = (A_j c_b + A_i c_a) / 2 - 10 fp64 operations instead of 21, each a 4-cycle issue; a regrouping of
    // the reference's products (a few ulp per term against a bound of 1e-12 x sum|term|), the same in every variant
    const double tg = (Aj * g.cb + Ai * g.ca) * 0.5;
    a.gx += tg * dx;
    a.gy += tg * dy;
    a.gz += tg * dz;
    return nww;
}

// ---- pass 2: pi_ik                            nsc:643-649, 780 ------------------------------------------
// q0 = {x y z h2}, qv = {vx vy vz cs} of the neighbour, (r0, rv) of the reference point
struct PiPair { double pi, rel, dot, rr; };      // pi_ik, |dv|^2 (the crossing time's), dv . dx, |dx|^2
template <class Sqrt>
__device__ __forceinline__ PiPair pi_term(const Q4& q0, const Q4& qv, double rho_j, const Q4& r0, const Q4& rv,
                                          double rho_i, double cs_i) {
    const double dx = q0.a - r0.a, dy = q0.b - r0.b, dz = q0.c - r0.c;
    const double dvx = qv.a - rv.a, dvy = qv.b - rv.b, dvz = qv.c - rv.c;
    PiPair t;
    t.rr = dx * dx + dy * dy + dz * dz;
    t.dot = dvx * dx + dvy * dy + dvz * dz;
    double w = t.dot / Sqrt()(t.rr + 0.01 * q0.d);                    // nsc:643
    w = (w > 0.0) ? 0.0 : w;                                          // nsc:644
    const double rho_ab = (rho_j + rho_i) / 2.0;                      // nsc:646
    const double c_ab = 0.5 * (qv.d + cs_i);                          // nsc:647
    t.pi = -0.5 * (c_ab * 2.0 - 3.0 * w) * w / rho_ab;                // nsc:649
    t.rel = dvx * dvx + dvy * dvy + dvz * dvz;                        // nsc:780
    return t;
}

// t.rel alone, in pi_term's very expression: what a row whose sum is NaN already still wants of a neighbour (its
// crossing-time vote; sphx_settled.h).  qv, rv as above.
__device__ __forceinline__ double pi_rel(const Q4& qv, const Q4& rv) {
    const double dvx = qv.a - rv.a, dvy = qv.b - rv.b, dvz = qv.c - rv.c;
    return dvx * dvx + dvy * dvy + dvz * dvz;                         // nsc:780
}

// ---- pass 3: viscous acceleration + heat      nsc:651-653 -----------------------------------------------
struct ViscAcc { double x, y, z, h; };
// q0 = {x y z h2}, qv = {vx vy vz .}, Bj = m_j Pi_j [t_j==0], c1_j of the neighbour; hi2, ci = -6 c1_i, Bi the particle's own
template <class Sqrt>
__device__ __forceinline__ void visc_term(ViscAcc& a, const Q4& q0, const Q4& qv, double Bj, double c1_j, const Q4& r0,
                                          const Q4& rv, double hi2, double ci, double Bi, bool clip) {
    const double dx = q0.a - r0.a, dy = q0.b - r0.b, dz = q0.c - r0.c;
    const double r2 = dist_sq<Sqrt>(dx * dx + dy * dy + dz * dz);
    const GradPair g = grad_pair(r2, q0.d - r2, c1_j, hi2, ci, clip);
    const double tb = (Bj * g.cb + Bi * g.ca) / 2.0;                      // nsc:651, the common factor taken out (see pass 1)
    const double bx = tb * dx, by = tb * dy, bz = tb * dz;
    a.x += bx; a.y += by; a.z += bz;
    a.h += bx * (qv.a - rv.a) + by * (qv.b - rv.b) + bz * (qv.c - rv.c);   // nsc:653
}

// ---- passes 2 + 3 fused: the pairwise viscosity (visc_mode 1) -------------------------------------------
// pi_ik of nsc:649 stays inside the sum (the Monaghan form of the loop version, nsc:802-808):
//   B_ik = pi_ik (M_j c_b + M_i c_a) / 2 (dx, dy, dz),  M = m [t==0] C/h^9 (RecBC.Bw, sphx_prep),  c_b, c_a as pass 3
// The heat term is added as t_b * (dv . dx) with the very dot product whose sign made pi_ik > 0 (w < 0): every term is
// >= 0 by construction.  Mj = M_j; ci = -6 M_i.  Returns |dv|^2: this pass casts the crossing-time vote.
template <class Sqrt>
__device__ __forceinline__ double visc_pw_term(ViscAcc& a, const Q4& q0, const Q4& qv, double rho_j, double Mj,
                                               const Q4& r0, const Q4& rv, double rho_i, double cs_i, double hi2,
                                               double ci, bool clip) {
    const PiPair t = pi_term<Sqrt>(q0, qv, rho_j, r0, rv, rho_i, cs_i);
    const double dx = q0.a - r0.a, dy = q0.b - r0.b, dz = q0.c - r0.c;
    const double r2 = dist_sq<Sqrt>(t.rr);
    const GradPair g = grad_pair(r2, q0.d - r2, Mj, hi2, ci, clip);
    const double tb = t.pi * (g.cb + g.ca) / 2.0;
    a.x += tb * dx; a.y += tb * dy; a.z += tb * dz;
    a.h += tb * t.dot;                                                // nsc:653
    return t.rel;
}

// ---- dust -> gas drag                         nsc:678-681, 736-741 (net_impulse) -----------------------
// Loop-form semantics: smoothing length of the dust neighbour j (Weigh2_dust, nsc:678), deltas relative to the particle
// itself (r0, rv).  The force on the particle is added to (ox, oy, oz) and returned (zero where the kernel vanishes).
struct Vec3 { double x, y, z; };
__device__ __forceinline__ Vec3 drag_term(double& ox, double& oy, double& oz, const Q4& q0, const Q4& qv, const Q4& r0, const Q4& rv, int j,
                                          const double* __restrict__ m, const double* __restrict__ mgm,
                                          const double* __restrict__ mcs) {
    const double dx = q0.a - r0.a, dy = q0.b - r0.b, dz = q0.c - r0.c;
    const double ds2 = q0.d, ds = sqrt(ds2);
    const double q = ds2 - (dx * dx + dy * dy + dz * dz);
    const double ds4 = ds2 * ds2;
    const double wf = m[j] * 315.0 * (q * q * q) / (201.06192982974676 * (ds4 * ds4 * ds));   // nsc:678-681
    Vec3 f{0.0, 0.0, 0.0};
    if (wf > 0.0) {
        const double dvx = qv.a - rv.a, dvy = qv.b - rv.b, dvz = qv.c - rv.c;
        const double coef = wf / mgm[j] * mcs[j] * sqrt(dvx * dvx + dvy * dvy + dvz * dvz);
        f.x = coef * dvx; f.y = coef * dvy; f.z = coef * dvz;
        ox += f.x; oy += f.y; oz += f.z;
    }
    return f;
}

// ---- crossing time                            nsc:776-786 -------------------------------------------------
// a gas particle's vote h / sqrt(max |dv|^2), nan_to_num'ed, as the bits of a positive double (ordered as the values
// are); SPHX_CT_NONE where it casts none (a vote of zero: nsc:782 takes the positive ones)
__device__ __forceinline__ u64 ct_vote_bits(double h_i, double maxrel) {
    const double ct = sphx_nan_to_num(h_i / sqrt(maxrel));
    return (ct > 0.0) ? (u64)__double_as_longlong(ct) : SPHX_CT_NONE;
}
// minimum of the votes of a workgroup of T threads (every thread calls), then of all workgroups in *ct_bits
template <int T>
__device__ __forceinline__ void block_min_vote(u64 my_ct, u64* ct_bits) {
    __shared__ u64 sm[T / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 q = __shfl_xor(my_ct, o, 64);
        my_ct = q < my_ct ? q : my_ct;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = my_ct;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 r = sm[0];
        for (int w = 1; w < T / 64; ++w) r = sm[w] < r ? sm[w] : r;
        if (r != SPHX_CT_NONE) atomicMin(ct_bits, r);
    }
}
