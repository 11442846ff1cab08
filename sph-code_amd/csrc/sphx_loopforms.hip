// sphx_loopforms.hip - the per-particle loop forms the reference's time loop calls
// (nsc:673-816; drv:451-458): mass-derived smoothing length h(m) = (m/m_0)^(1/3) d with the
// driver-injected global d, clipped gradients, physical sign.  One thread per particle over
// the K-major neighbour list; deltas are relative to the particle itself.
#include "sphx_internal.h"
#include "sphx_pair.h"             // parts_total, the crossing-time vote and its workgroup minimum
// NumPy never fuses a multiply into an add: keep every operation separately rounded so that
// cancellations such as h_j^2 - r^2 at the kernel edge reproduce the reference bit for bit.
#pragma clang fp contract(off)
#include <float.h>
#include "sphx_weigh2.h"           // PI64, pow9, weigh2 (nsc:673-676)

// nsc:678-681
__device__ __forceinline__ double weigh2_dust(double r2, double m, double ds) {
    const double q = ds * ds - r2;
    return m * 315.0 * (q * q * q) / (PI64 * pow9(ds));
}
// nsc:683-690: scalar coefficient of (x - x_0); clipped, gas neighbours only
__device__ __forceinline__ double grad_coef(double r2, double m, double d, double m0, double d9, double tk) {
    const double a = m0 / m;
    const double q = pow(m / m0, 2.0 / 3.0) * (d * d) - r2;
    double c = -315.0 * 6.0 * (a * a * a) / (PI64 * d9) * (q * q) * ((tk == 0.0) ? 1.0 : 0.0);
    return (q > 0.0) ? c : 0.0;
}

struct LoopArgs {
    int n, npad, k;
    const int* nbr;
    const double *pos, *vel;                 // (n,3) AoS, as the reference passes them
    const double *m, *pt, *h, *mu, *gam, *E, *T, *rho, *mgm, *mcs;
    double d, m0, m_h, kB, amu;
    double *out1, *out3, *out3b;             // (n,), (n,3), (n,3)
    u64* ct_bits;
};

// mode 0 density (nsc:693), 1 dust_density (nsc:704), 2 num_dens (nsc:744)
template <int MODE>
__global__ __launch_bounds__(256) void loop_density_kernel(LoopArgs a) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const double xi = a.pos[3 * (size_t)i], yi = a.pos[3 * (size_t)i + 1], zi = a.pos[3 * (size_t)i + 2];
    const double d9 = pow9(a.d);
    double s = 0.0;
    for (int kk = 0; kk < a.k; ++kk) {
        int j = a.nbr[(size_t)kk * a.npad + i];
        if (j < 0) continue;
        const double dx = a.pos[3 * (size_t)j] - xi, dy = a.pos[3 * (size_t)j + 1] - yi,
                     dz = a.pos[3 * (size_t)j + 2] - zi;
        const double r2 = dx * dx + dy * dy + dz * dz;
        double v;
        if (MODE == 0) v = weigh2(r2, a.m[j], a.d, a.m0, d9) * ((a.pt[j] == 0.0) ? 1.0 : 0.0);
        else if (MODE == 1) v = weigh2_dust(r2, a.m[j], a.h[j]) * ((a.pt[j] == 2.0) ? 1.0 : 0.0);
        else v = weigh2(r2, a.m[j], a.d, a.m0, d9) / (a.mu[j] * a.m_h);
        if (v > 0.0) s += v;
    }
    a.out1[i] = s;
}

// nsc:755-774
__global__ __launch_bounds__(256) void loop_del_pressure_kernel(LoopArgs a) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double gx = 0.0, gy = 0.0, gz = 0.0;
    if (a.pt[i] == 0.0) {
        const double xi = a.pos[3 * (size_t)i], yi = a.pos[3 * (size_t)i + 1], zi = a.pos[3 * (size_t)i + 2];
        const double d9 = pow9(a.d), Ei = a.E[i];
        for (int kk = 0; kk < a.k; ++kk) {
            int j = a.nbr[(size_t)kk * a.npad + i];
            if (j < 0) continue;
            const double dx = a.pos[3 * (size_t)j] - xi, dy = a.pos[3 * (size_t)j + 1] - yi,
                         dz = a.pos[3 * (size_t)j + 2] - zi;
            const double r2 = dx * dx + dy * dy + dz * dz;
            const double c = grad_coef(r2, a.m[j], a.d, a.m0, d9, a.pt[j]);
            const double f = (a.E[j] + Ei) / a.gam[j];
            gx += 0.5 * sphx_nan_to_num(c * dx) * f;
            gy += 0.5 * sphx_nan_to_num(c * dy) * f;
            gz += 0.5 * sphx_nan_to_num(c * dz) * f;
        }
    }
    a.out3[3 * (size_t)i] = gx; a.out3[3 * (size_t)i + 1] = gy; a.out3[3 * (size_t)i + 2] = gz;
}

// nsc:788-816
__global__ __launch_bounds__(256) void loop_av_kernel(LoopArgs a) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double ax = 0.0, ay = 0.0, az = 0.0, heat = 0.0;
    if (a.pt[i] == 0.0) {
        const double xi = a.pos[3 * (size_t)i], yi = a.pos[3 * (size_t)i + 1], zi = a.pos[3 * (size_t)i + 2];
        const double vxi = a.vel[3 * (size_t)i], vyi = a.vel[3 * (size_t)i + 1], vzi = a.vel[3 * (size_t)i + 2];
        const double d9 = pow9(a.d), mi = a.m[i], rhoi = a.rho[i];
        const double csi = sphx_nan_to_num(sqrt(a.gam[i] * a.kB * a.T[i] / (a.mu[i] * a.amu)));
        for (int kk = 0; kk < a.k; ++kk) {
            int j = a.nbr[(size_t)kk * a.npad + i];
            if (j < 0 || a.pt[j] != 0.0) continue;            // sums run over gas neighbours only
            const double dx = a.pos[3 * (size_t)j] - xi, dy = a.pos[3 * (size_t)j + 1] - yi,
                         dz = a.pos[3 * (size_t)j + 2] - zi;
            const double dvx = a.vel[3 * (size_t)j] - vxi, dvy = a.vel[3 * (size_t)j + 1] - vyi,
                         dvz = a.vel[3 * (size_t)j + 2] - vzi;
            const double r2 = dx * dx + dy * dy + dz * dz;
            double w = (dvx * dx + dvy * dy + dvz * dz) / sqrt(r2);
            w = (w > 0.0) ? 0.0 : w;
            w = sphx_nan_to_num(w);                              // self pair: 0/0
            const double csj = sphx_nan_to_num(sqrt(a.gam[j] * a.kB * a.T[j] / (a.mu[j] * a.amu)));
            const double vsig = csj + csi - 3.0 * w;
            const double rho_ij = (a.rho[j] + rhoi) / 2.0;
            const double PI = -0.5 * vsig * w / rho_ij;
            const double c = grad_coef(r2, mi, a.d, a.m0, d9, a.pt[j]);     // h(m_i)  nsc:805
            const double gwx = sphx_nan_to_num(c * dx), gwy = sphx_nan_to_num(c * dy), gwz = sphx_nan_to_num(c * dz);
            const double mb = (a.m[j] + mi) / 2.0;
            ax += mb * PI * gwx; ay += mb * PI * gwy; az += mb * PI * gwz;
            heat += 0.5 * mb * PI * (dvx * gwx + dvy * gwy + dvz * gwz);
        }
    }
    a.out3[3 * (size_t)i] = ax; a.out3[3 * (size_t)i + 1] = ay; a.out3[3 * (size_t)i + 2] = az;
    a.out1[i] = heat;
}

// nsc:776-786
__global__ __launch_bounds__(256) void loop_ct_kernel(LoopArgs a) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    u64 mine = SPHX_CT_NONE;
    if (i < a.n && a.pt[i] == 0.0) {
        const double vxi = a.vel[3 * (size_t)i], vyi = a.vel[3 * (size_t)i + 1], vzi = a.vel[3 * (size_t)i + 2];
        double mx = 0.0;
        for (int kk = 0; kk < a.k; ++kk) {
            int j = a.nbr[(size_t)kk * a.npad + i];
            if (j < 0) continue;
            const double dvx = a.vel[3 * (size_t)j] - vxi, dvy = a.vel[3 * (size_t)j + 1] - vyi,
                         dvz = a.vel[3 * (size_t)j + 2] - vzi;
            mx = fmax(mx, dvx * dvx + dvy * dvy + dvz * dvz);
        }
        mine = ct_vote_bits(a.h[i], mx);
    }
    block_min_vote<256>(mine, a.ct_bits);
}

// nsc:719-742; the reaction as an ordered scatter (DragScatter, sphx_internal.h): np.add.at's order, the same bits every run
__global__ __launch_bounds__(256) void loop_impulse_kernel(LoopArgs a, DragScatter sc) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const double xi = a.pos[3 * (size_t)i], yi = a.pos[3 * (size_t)i + 1], zi = a.pos[3 * (size_t)i + 2];
    const double vxi = a.vel[3 * (size_t)i], vyi = a.vel[3 * (size_t)i + 1], vzi = a.vel[3 * (size_t)i + 2];
    double ox = 0.0, oy = 0.0, oz = 0.0;
    for (int kk = 0; kk < a.k; ++kk) {
        int j = a.nbr[(size_t)kk * a.npad + i];
        if (j < 0 || a.pt[j] != 2.0) continue;
        const double dx = a.pos[3 * (size_t)j] - xi, dy = a.pos[3 * (size_t)j + 1] - yi,
                     dz = a.pos[3 * (size_t)j + 2] - zi;
        const double wf = weigh2_dust(dx * dx + dy * dy + dz * dz, a.m[j], a.h[j]);
        double fx = 0.0, fy = 0.0, fz = 0.0;
        if (wf > 0.0) {
            const double dvx = a.vel[3 * (size_t)j] - vxi, dvy = a.vel[3 * (size_t)j + 1] - vyi,
                         dvz = a.vel[3 * (size_t)j + 2] - vzi;
            const double coef = wf / a.mgm[j] * a.mcs[j] * sqrt(dvx * dvx + dvy * dvy + dvz * dvz);
            fx = coef * dvx; fy = coef * dvy; fz = coef * dvz;
            ox += fx; oy += fy; oz += fz;
        }
        if (j != i) {
            const int slot = sc.start[j] + atomicSub(&sc.cnt[j], 1) - 1;
            sphx_drag_put(sc, slot, ((u64)(unsigned)i << 12) | (u64)kk, -fx, -fy, -fz);
        }
    }
    a.out3[3 * (size_t)i] = ox; a.out3[3 * (size_t)i + 1] = oy; a.out3[3 * (size_t)i + 2] = oz;
}

// ---- host side ---------------------------------------------------------------------------------
static int up(sphx_ctx* ctx, DevBuf& b, const void* host, size_t bytes) {
    SPHX_TRY(sphx_ensure(ctx, b, bytes));
    HIPCHK(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SPHX_OK;
}

static int loop_begin(sphx_ctx* ctx, int64_t n, int k, const int64_t* neighbor, LoopArgs* a) {
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "n=%lld out of range", (long long)n);
    if (k < 1 || k > 4096) return sphx_set_err(ctx, SPHX_E_ARG, "k=%d out of range", k);
    HIPCHK(hipSetDevice(ctx->device));
    ctx->map_perm = nullptr;
    ctx->qorder = nullptr;
    if (neighbor) {
        SPHX_TRY(up(ctx, ctx->idx64, neighbor, (size_t)n * k * sizeof(int64_t)));
        SPHX_TRY(sphx_transpose_nbr(ctx, n, k, ctx->idx64.as<int64_t>()));
        ctx->nbr_api_valid = true; ctx->nbr_api_n = n; ctx->nbr_api_k = k;
    } else if (!(ctx->nbr_api_valid && ctx->nbr_api_n == n && ctx->nbr_api_k == k)) {
        // NULL = "the list of the previous call" (320 MB of PCIe traffic per call at N = 1e6, K = 40)
        return sphx_set_err(ctx, SPHX_E_STATE, "neighbor == NULL but no (%lld, %d) list is held from a previous call",
                            (long long)n, k);
    }
    memset(a, 0, sizeof(*a));
    a->n = (int)n; a->npad = (int)sphx_pad64(n); a->k = k;
    a->nbr = ctx->nbr.as<int>();
    a->m0 = ctx->cst.m_0; a->m_h = ctx->cst.m_h; a->kB = ctx->cst.k_B; a->amu = ctx->cst.amu;
    return SPHX_OK;
}
#define UPF(buf, host, cnt, field)                                                           \
    do {                                                                                     \
        SPHX_TRY(up(ctx, ctx->buf, host, (size_t)(cnt) * sizeof(double)));                   \
        a.field = ctx->buf.as<double>();                                                     \
    } while (0)
#define LAUNCH1(kern)                                                                        \
    do {                                                                                     \
        hipLaunchKernelGGL(kern, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a); \
        HIPCHK(hipGetLastError());                                                           \
    } while (0)
static int down(sphx_ctx* ctx, void* host, const void* dev, size_t bytes) {
    HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPHX_OK;
}

extern "C" int sphx_density(sphx_ctx* ctx, int64_t n, int k, const double* points, const double* mass,
                            const double* particle_type, const int64_t* neighbor, double d, double* out) {
    if (!ctx) return SPHX_E_ARG;
    NEED(points); NEED(mass); NEED(particle_type); NEED(out);
    LoopArgs a;
    SPHX_TRY(loop_begin(ctx, n, k, neighbor, &a));
    UPF(in_a, points, 3 * n, pos); UPF(in_c, mass, n, m); UPF(in_h, particle_type, n, pt);
    a.d = d;
    SPHX_TRY(sphx_ensure(ctx, ctx->out_a, (size_t)n * sizeof(double)));
    a.out1 = ctx->out_a.as<double>();
    LAUNCH1(loop_density_kernel<0>);
    return down(ctx, out, a.out1, (size_t)n * sizeof(double));
}

int sphx_loop_density_dev(sphx_ctx* ctx, int64_t n, int k, const int* nbr, const double* points, const double* mass,
                          const double* ptype, double d, double m_0, double* out) {
    LoopArgs a;
    memset(&a, 0, sizeof(a));
    a.n = (int)n; a.npad = (int)sphx_pad64(n); a.k = k;
    a.nbr = nbr; a.pos = points; a.m = mass; a.pt = ptype;
    a.d = d; a.m0 = m_0;
    a.out1 = out;
    LAUNCH1(loop_density_kernel<0>);
    return SPHX_OK;
}

extern "C" int sphx_dust_density(sphx_ctx* ctx, int64_t n, int k, const double* points, const double* mass,
                                 const int64_t* neighbor, const double* particle_type,
                                 const double* sizes, double* out) {
    if (!ctx) return SPHX_E_ARG;
    NEED(points); NEED(mass); NEED(particle_type); NEED(sizes); NEED(out);
    LoopArgs a;
    SPHX_TRY(loop_begin(ctx, n, k, neighbor, &a));
    UPF(in_a, points, 3 * n, pos); UPF(in_c, mass, n, m); UPF(in_h, particle_type, n, pt);
    UPF(in_d, sizes, n, h);
    a.d = 1.0;
    SPHX_TRY(sphx_ensure(ctx, ctx->out_a, (size_t)n * sizeof(double)));
    a.out1 = ctx->out_a.as<double>();
    LAUNCH1(loop_density_kernel<1>);
    return down(ctx, out, a.out1, (size_t)n * sizeof(double));
}

extern "C" int sphx_num_dens(sphx_ctx* ctx, int64_t n, int k, const double* mass, const double* points,
                             const double* mu_array, const int64_t* neighbor, double d, double* out) {
    if (!ctx) return SPHX_E_ARG;
    NEED(points); NEED(mass); NEED(mu_array); NEED(out);
    LoopArgs a;
    SPHX_TRY(loop_begin(ctx, n, k, neighbor, &a));
    UPF(in_a, points, 3 * n, pos); UPF(in_c, mass, n, m); UPF(in_f, mu_array, n, mu);
    a.d = d;
    SPHX_TRY(sphx_ensure(ctx, ctx->out_a, (size_t)n * sizeof(double)));
    a.out1 = ctx->out_a.as<double>();
    LAUNCH1(loop_density_kernel<2>);
    return down(ctx, out, a.out1, (size_t)n * sizeof(double));
}

extern "C" int sphx_del_pressure(sphx_ctx* ctx, int64_t n, int k, const double* points, const double* mass,
                                 const double* particle_type, const int64_t* neighbor,
                                 const double* E_internal, const double* gamma_array, double d, double* out) {
    if (!ctx) return SPHX_E_ARG;
    NEED(points); NEED(mass); NEED(particle_type); NEED(E_internal); NEED(gamma_array); NEED(out);
    LoopArgs a;
    SPHX_TRY(loop_begin(ctx, n, k, neighbor, &a));
    UPF(in_a, points, 3 * n, pos); UPF(in_c, mass, n, m); UPF(in_h, particle_type, n, pt);
    UPF(in_e, E_internal, n, E); UPF(in_g, gamma_array, n, gam);
    a.d = d;
    SPHX_TRY(sphx_ensure(ctx, ctx->out_b, (size_t)n * 3 * sizeof(double)));
    a.out3 = ctx->out_b.as<double>();
    LAUNCH1(loop_del_pressure_kernel);
    return down(ctx, out, a.out3, (size_t)n * 3 * sizeof(double));
}

extern "C" int sphx_artificial_viscosity(sphx_ctx* ctx, int64_t n, int k, const int64_t* neighbor,
                                         const double* points, const double* particle_type,
                                         const double* sizes, const double* mass, const double* densities,
                                         const double* velocities, const double* T,
                                         const double* gamma_array, const double* mu_array, double d,
                                         double* visc_accel, double* visc_heat) {
    if (!ctx) return SPHX_E_ARG;
    (void)sizes;
    NEED(points); NEED(mass); NEED(particle_type); NEED(densities); NEED(velocities);
    NEED(T); NEED(gamma_array); NEED(mu_array); NEED(visc_accel); NEED(visc_heat);
    LoopArgs a;
    SPHX_TRY(loop_begin(ctx, n, k, neighbor, &a));
    UPF(in_a, points, 3 * n, pos); UPF(in_b, velocities, 3 * n, vel); UPF(in_c, mass, n, m);
    UPF(in_h, particle_type, n, pt); UPF(in_d, densities, n, rho); UPF(in_e, T, n, T);
    UPF(in_g, gamma_array, n, gam); UPF(in_f, mu_array, n, mu);
    a.d = d;
    SPHX_TRY(sphx_ensure(ctx, ctx->out_a, (size_t)n * sizeof(double)));
    SPHX_TRY(sphx_ensure(ctx, ctx->out_b, (size_t)n * 3 * sizeof(double)));
    a.out1 = ctx->out_a.as<double>(); a.out3 = ctx->out_b.as<double>();
    LAUNCH1(loop_av_kernel);
    SPHX_TRY(down(ctx, visc_accel, a.out3, (size_t)n * 3 * sizeof(double)));
    return down(ctx, visc_heat, a.out1, (size_t)n * sizeof(double));
}

extern "C" int sphx_crossing_time(sphx_ctx* ctx, int64_t n, int k, const int64_t* neighbor,
                                  const double* velocities, const double* sizes,
                                  const double* particle_type, double* out) {
    if (!ctx) return SPHX_E_ARG;
    NEED(velocities); NEED(sizes); NEED(particle_type); NEED(out);
    LoopArgs a;
    SPHX_TRY(loop_begin(ctx, n, k, neighbor, &a));
    UPF(in_b, velocities, 3 * n, vel); UPF(in_d, sizes, n, h); UPF(in_h, particle_type, n, pt);
    u64* ct_bits = ctx->scal.as<u64>() + SC_CT_BITS;
    ctx->ct_primed = false;
    SPHX_TRY(sphx_loop_ct_dev(ctx, n, k, a.nbr, a.vel, a.h, a.pt, ct_bits));
    u64 bits = 0;
    SPHX_TRY(down(ctx, &bits, ct_bits, sizeof(u64)));
    *out = sphx_loop_ct_value(ctx, bits);
    return SPHX_OK;
}
// ... on device inputs: velocities (n,3), sizes and ptype (n), a K-major list; the votes' minimum into *ct_bits (primed here)
int sphx_loop_ct_dev(sphx_ctx* ctx, int64_t n, int k, const int* nbr, const double* velocities, const double* sizes, const double* ptype,
                     u64* ct_bits) {
    LoopArgs a;
    memset(&a, 0, sizeof(a));
    a.n = (int)n; a.npad = (int)sphx_pad64(n); a.k = k;
    a.nbr = nbr; a.vel = velocities; a.h = sizes; a.pt = ptype;
    a.ct_bits = ct_bits;
    SPHX_TRY(sphx_prime_ct(ctx, ct_bits));
    LAUNCH1(loop_ct_kernel);
    return SPHX_OK;
}
// nsc:783-786 from the votes' minimum
double sphx_loop_ct_value(const sphx_ctx* ctx, u64 bits) {
    if (bits == SPHX_CT_NONE) return ctx->cst.dt_0 / 10.0;    // nsc:783-784
    double v;
    memcpy(&v, &bits, 8);
    return v + 0.0001;                                        // nsc:786
}

extern "C" int sphx_net_impulse(sphx_ctx* ctx, int64_t n, int k, const double* points, const double* mass,
                                const double* sizes, const double* velocities, const double* particle_type,
                                const int64_t* neighbor, const double* mean_grain_mass,
                                const double* mean_cross, double* accel_onto, double* accel_reaction) {
    if (!ctx) return SPHX_E_ARG;
    NEED(points); NEED(mass); NEED(sizes); NEED(velocities); NEED(particle_type);
    NEED(mean_grain_mass); NEED(mean_cross); NEED(accel_onto); NEED(accel_reaction);
    LoopArgs a;
    SPHX_TRY(loop_begin(ctx, n, k, neighbor, &a));
    UPF(in_a, points, 3 * n, pos); UPF(in_b, velocities, 3 * n, vel); UPF(in_c, mass, n, m);
    UPF(in_h, particle_type, n, pt); UPF(in_d, sizes, n, h); UPF(in_e, mean_grain_mass, n, mgm);
    UPF(in_f, mean_cross, n, mcs);
    SPHX_TRY(sphx_ensure(ctx, ctx->out_b, (size_t)n * 3 * sizeof(double)));
    SPHX_TRY(sphx_ensure(ctx, ctx->out_c, (size_t)n * 3 * sizeof(double)));
    a.out3 = ctx->out_b.as<double>(); a.out3b = ctx->out_c.as<double>();
    DragScatter sc;
    SPHX_TRY(sphx_drag_scatter_plan(ctx, n, k, a.nbr, a.pt, nullptr, &sc));
    hipLaunchKernelGGL(loop_impulse_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, a, sc);
    HIPCHK(hipGetLastError());
    SPHX_TRY(sphx_drag_scatter_reduce(ctx, n, sc, a.out3b));
    SPHX_TRY(down(ctx, accel_onto, a.out3, (size_t)n * 3 * sizeof(double)));
    return down(ctx, accel_reaction, a.out3b, (size_t)n * 3 * sizeof(double));
}

// ---- the loop forms on the device-resident, cell-sorted state of the step loop ------------------
// drv:451-458 as the reference's time loop evaluates them, on the step's own neighbour list:
//   rho = density, rho_dust = dust_density, n = num_dens, delp = del_pressure,
//   (av accel, av heat) = artificial_viscosity(..., densities = rho, ...), ct = crossing_time.
// Same expressions as the array-API kernels above (which the golden vectors pin), organised the way
// sphx_sums.hip / sphx_blob.hip organise hydro_update's sums: per-particle factors are worked out once
// per step into dense 64-B records (+ one 8-B side value), the six sums run as two passes, sums are
// kept as SPHX_SUM_PARTS partial sums over the list positions k mod SPHX_SUM_PARTS, and each pass
// exists in a gather form (one thread per particle) and an LDS form (blob image, four lanes per
// particle, sphx_blob.h) that agree bit for bit.
//   pass 1 record {x y z hq | w1 g1 +-mun E}, side gamma:  hq = (m/m_0)^(2/3) d^2, w1 = m 315 (m_0/m)^3,
//       g1 = -1890 (m_0/m)^3 / (64 pi d^9), mun = mu m_h carrying the gas flag in its sign
//   pass 2 record {x y z +-cs | vx vy vz rho}, side m:       cs >= 0 for gas, -(cs + 1) otherwise
// Dust neighbours (type 2, a few per cent at most) need m_j and sizes_j as well: fetched from global
// memory through the int32 list.
#include "sphx_blob.h"
struct RecP1 { double x, y, z, hq, w1, g1, muns, E; };
struct RecP2 { double x, y, z, css, vx, vy, vz, rho; };

struct LoopPrepArgs {
    int n;
    const double *x, *y, *z, *vx, *vy, *vz, *m, *pt, *mu, *gam, *E, *T;
    double d, m0, m_h, kB, amu;
    RecP1* p1; RecP2* p2;
};
__global__ __launch_bounds__(256) void loop_prep_kernel(LoopPrepArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const double m = a.m[i], d9 = pow9(a.d);
    const double aa = a.m0 / m;
    const bool gas = (a.pt[i] == 0.0);
    RecP1 r;
    r.x = a.x[i]; r.y = a.y[i]; r.z = a.z[i];
    r.hq = pow(m / a.m0, 2.0 / 3.0) * (a.d * a.d);              // nsc:675
    r.w1 = m * 315.0 * (aa * aa * aa);                           // nsc:676, up to (q*q*q) / (64 pi d^9)
    r.g1 = -315.0 * 6.0 * (aa * aa * aa) / (PI64 * d9);          // nsc:688, up to (q*q) and the type mask
    const double mun = a.mu[i] * a.m_h;                          // nsc:751
    r.muns = gas ? mun : -mun;
    r.E = a.E[i];
    a.p1[i] = r;
    RecP2 v;
    v.x = r.x; v.y = r.y; v.z = r.z;
    const double cs = sphx_nan_to_num(sqrt(a.gam[i] * a.kB * a.T[i] / (a.mu[i] * a.amu)));     // nsc:792
    v.css = gas ? cs : -(cs + 1.0);
    v.vx = a.vx[i]; v.vy = a.vy[i]; v.vz = a.vz[i];
    v.rho = 0.0;                                                 // pass 1 fills it in
    a.p2[i] = v;
}

// ---- terms of one neighbour (shared by the gather and the LDS kernels) -------------------------------
struct L1Acc { double rho, rd, n, gx, gy, gz; };
// q0 = {x y z hq}, q1 = {w1 g1 +-mun E}; (dm, dh) = mass and size of the neighbour if it is dust, else dm < 0
__device__ __forceinline__ void loop1_term(L1Acc& a, const Q4& q0, const Q4& q1, double gam_j, double dm, double dh,
                                           double xi, double yi, double zi, double Ei, bool gas_i, double d9) {
    const double dx = q0.a - xi, dy = q0.b - yi, dz = q0.c - zi;
    const double r2 = dx * dx + dy * dy + dz * dz;
    const double q = q0.d - r2;
    const double w = q1.a * (q * q * q) / (PI64 * d9);                           // Weigh2, nsc:673-676
    const bool gas_j = q1.c > 0.0;
    const double vr = w * (gas_j ? 1.0 : 0.0);
    if (vr > 0.0) a.rho += vr;                                                   // nsc:700
    const double vn = w / fabs(q1.c);
    if (vn > 0.0) a.n += vn;                                                     // nsc:751
    if (dm >= 0.0) {                                                             // Weigh2_dust, nsc:678-681
        const double vd = weigh2_dust(r2, dm, dh);
        if (vd > 0.0) a.rd += vd;                                                // nsc:715
    }
    if (gas_i) {                                                                 // nsc:755-774
        double c = q1.b * (q * q) * (gas_j ? 1.0 : 0.0);
        c = (q > 0.0) ? c : 0.0;
        const double f = (q1.d + Ei) / gam_j;
        a.gx += 0.5 * sphx_nan_to_num(c * dx) * f;
        a.gy += 0.5 * sphx_nan_to_num(c * dy) * f;
        a.gz += 0.5 * sphx_nan_to_num(c * dz) * f;
    }
}
struct L2Acc { double ax, ay, az, heat; };
// q0 = {x y z +-cs}, qv = {vx vy vz rho}; returns |dv|^2 (the crossing time takes every neighbour)
__device__ __forceinline__ double loop2_term(L2Acc& a, const Q4& q0, const Q4& qv, double m_j, const Q4& s0,
                                             const Q4& sv, double rho_i, double m_i, double hq_i, double g1_i) {
    const double dvx = qv.a - sv.a, dvy = qv.b - sv.b, dvz = qv.c - sv.c;
    const double rel = dvx * dvx + dvy * dvy + dvz * dvz;                         // nsc:780
    if (q0.d < 0.0) return rel;                                                   // sums over gas neighbours only
    const double dx = q0.a - s0.a, dy = q0.b - s0.b, dz = q0.c - s0.c;
    const double r2 = dx * dx + dy * dy + dz * dz;
    double w = (dvx * dx + dvy * dy + dvz * dz) / sqrt_mid(r2);                   // (sqrt's bits on this range: sphx_blob.h)
    w = (w > 0.0) ? 0.0 : w;
    w = sphx_nan_to_num(w);                                                          // self pair: 0/0
    const double vsig = q0.d + s0.d - 3.0 * w;
    const double rho_ij = (qv.d + rho_i) / 2.0;
    const double PI = -0.5 * vsig * w / rho_ij;
    const double q = hq_i - r2;                                                   // h(m_i), nsc:805
    double c = g1_i * (q * q) * 1.0;
    c = (q > 0.0) ? c : 0.0;
    const double gwx = sphx_nan_to_num(c * dx), gwy = sphx_nan_to_num(c * dy), gwz = sphx_nan_to_num(c * dz);
    const double mb = (m_j + m_i) / 2.0;
    a.ax += mb * PI * gwx; a.ay += mb * PI * gwy; a.az += mb * PI * gwz;
    a.heat += 0.5 * mb * PI * (dvx * gwx + dvy * gwy + dvz * gwz);
    return rel;
}

#define LNB 4
// ---- gather form ---------------------------------------------------------------------------------------
// pass 1: density (nsc:693), dust_density (nsc:704), num_dens (nsc:744), del_pressure (nsc:755)
__global__ __launch_bounds__(256) void loop_pass1_kernel(int n, int npad, int k, double d9,
                                                         const int* __restrict__ nbr,
                                                         const RecP1* __restrict__ p1,
                                                         const double* __restrict__ gam,
                                                         const double* __restrict__ pt, const double* __restrict__ m,
                                                         const double* __restrict__ h,
                                                         const int* __restrict__ qorder, double* rho, double* rhod,
                                                         double* nden, double* G, RecP2* p2) {
    const int p = xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;      // list column (blob order)
    if (p >= n) return;
    const int i = qorder ? qorder[p] : p;                                           // stored particle
    const double* sp = reinterpret_cast<const double*>(&p1[i]);
    const Q4 s0 = gload4(sp), s1 = gload4(sp + 4);
    const bool gas_i = s1.c > 0.0;
    L1Acc acc[SPHX_SUM_PARTS] = {};
    for (int kk0 = 0; kk0 < k; kk0 += LNB) {
        int jb[LNB];
        Q4 q0b[LNB], q1b[LNB];
        double gb[LNB];
#pragma unroll
        for (int u = 0; u < LNB; ++u) jb[u] = (kk0 + u < k) ? nbr[(size_t)(kk0 + u) * npad + p] : -1;
#pragma unroll
        for (int u = 0; u < LNB; ++u) {
            const int jj = jb[u] < 0 ? i : jb[u];
            const double* q = reinterpret_cast<const double*>(&p1[jj]);
            q0b[u] = gload4(q); q1b[u] = gload4(q + 4);
            gb[u] = gam[jj];
        }
#pragma unroll
        for (int u = 0; u < LNB; ++u) {
            if (jb[u] < 0) continue;
            double dm = -1.0, dh = 0.0;
            if (!(q1b[u].c > 0.0) && pt[jb[u]] == 2.0) { dm = m[jb[u]]; dh = h[jb[u]]; }
            loop1_term(acc[u & (SPHX_SUM_PARTS - 1)], q0b[u], q1b[u], gb[u], dm, dh, s0.a, s0.b, s0.c, s1.d, gas_i, d9);
        }
    }
    const double s_rho = parts_total(acc, &L1Acc::rho);
    rho[i] = s_rho; rhod[i] = parts_total(acc, &L1Acc::rd); nden[i] = parts_total(acc, &L1Acc::n);
    G[3 * (size_t)i] = parts_total(acc, &L1Acc::gx); G[3 * (size_t)i + 1] = parts_total(acc, &L1Acc::gy);
    G[3 * (size_t)i + 2] = parts_total(acc, &L1Acc::gz);
    p2[i].rho = s_rho;
}

// pass 2: artificial_viscosity (nsc:788-816) and crossing_time (nsc:776-786)
__global__ __launch_bounds__(256) void loop_pass2_kernel(int n, int npad, int k, const int* __restrict__ nbr,
                                                         const RecP1* __restrict__ p1,
                                                         const RecP2* __restrict__ p2,
                                                         const double* __restrict__ m, const double* __restrict__ h,
                                                         const int* __restrict__ qorder, double* va, double* vh,
                                                         u64* ct_bits) {
    const int p = xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
    u64 mine = SPHX_CT_NONE;
    if (p < n) {
        const int i = qorder ? qorder[p] : p;
        const double* sp = reinterpret_cast<const double*>(&p2[i]);
        const Q4 s0 = gload4(sp), sv = gload4(sp + 4);               // x y z +-cs | vx vy vz rho
        double ax = 0.0, ay = 0.0, az = 0.0, heat = 0.0;
        if (s0.d >= 0.0) {
            const double hq_i = p1[i].hq, g1_i = p1[i].g1, m_i = m[i];
            L2Acc acc[SPHX_SUM_PARTS] = {};
            double mx = 0.0;
            for (int kk0 = 0; kk0 < k; kk0 += LNB) {
                int jb[LNB];
                Q4 q0b[LNB], qvb[LNB];
                double mb[LNB];
#pragma unroll
                for (int u = 0; u < LNB; ++u) jb[u] = (kk0 + u < k) ? nbr[(size_t)(kk0 + u) * npad + p] : -1;
#pragma unroll
                for (int u = 0; u < LNB; ++u) {
                    const int jj = jb[u] < 0 ? i : jb[u];
                    const double* q = reinterpret_cast<const double*>(&p2[jj]);
                    q0b[u] = gload4(q); qvb[u] = gload4(q + 4);
                    mb[u] = m[jj];
                }
#pragma unroll
                for (int u = 0; u < LNB; ++u) {
                    if (jb[u] < 0) continue;
                    mx = fmax(mx, loop2_term(acc[u & (SPHX_SUM_PARTS - 1)], q0b[u], qvb[u], mb[u], s0, sv, sv.d, m_i, hq_i,
                                             g1_i));
                }
            }
            ax = parts_total(acc, &L2Acc::ax); ay = parts_total(acc, &L2Acc::ay); az = parts_total(acc, &L2Acc::az);
            heat = parts_total(acc, &L2Acc::heat);
            mine = ct_vote_bits(h[i], mx);
        }
        va[3 * (size_t)i] = ax; va[3 * (size_t)i + 1] = ay; va[3 * (size_t)i + 2] = az;
        vh[i] = heat;
    }
    block_min_vote<256>(mine, ct_bits);
}

// ---- LDS form (sphx_blob.h: blob image, LPP lanes per particle, persistent workgroups; blob_pass walks) --------
// Deltas are relative to the particle itself and every stored particle is computed (ghosts too: the callers pick).
struct Loop1Pass {
    typedef RecP1 Rec;
    typedef L1Acc Sums;
    static constexpr int NSIDE = 1, PER_SLOT = 72;          // side value: loop_dust_side_kernel's
    static constexpr bool CLIPS = false, VOTES = false, ROW_FROM_LIST = false;
    double d9;
    const RecP1* __restrict__ rec;
    const double* __restrict__ gside;
    double *rho, *rhod, *nden, *G;
    RecP2* p2;
    struct Row { Q4 s0, s1; bool gas_i; };
    struct Nb { Q8 q; double g; };
    __device__ __forceinline__ BlobSides sides() const { return {gside, 1}; }
    __device__ __forceinline__ Row load_row(int i) const {
        const Q8 s = gload8(&rec[i]);
        return Row{s.lo, s.hi, s.hi.c > 0.0};
    }
    __device__ __forceinline__ static void load_out(Row&, int, bool) {}
    __device__ __forceinline__ static bool wanted(const Row&) { return true; }
    __device__ __forceinline__ Nb staged(const double2* img, const double* side, int s, const int*) const {
        return Nb{lload8(img, s), side[s]};
    }
    __device__ __forceinline__ Nb global(int j) const { return Nb{gload8(&rec[j]), gside[j]}; }
    __device__ __forceinline__ static Nb none(const Row& r) { return Nb{Q8{r.s0, r.s1}, 1.0}; }
    template <bool CLIP>
    __device__ __forceinline__ double term(Sums& a, const Nb& f, const Row& r) const {
        double dm = -1.0, dh = 0.0;
        // not gas: a dust neighbour's mass travels in the side value, its size in the record's g1 (neither is
        // read for a neighbour that is not gas; loop_dust_side_kernel) - nothing is gathered here
        if (!(f.q.hi.c > 0.0) && f.g >= 0.0) { dm = f.g; dh = f.q.hi.b; }
        loop1_term(a, f.q.lo, f.q.hi, f.g, dm, dh, r.s0.a, r.s0.b, r.s0.c, r.s1.d, r.gas_i, d9);
        return 0.0;
    }
    __device__ __forceinline__ u64 finish(const Sums& a, double, const Row&, int i, int) const {
        rho[i] = a.rho; rhod[i] = a.rd; nden[i] = a.n;
        G[3 * (size_t)i] = a.gx; G[3 * (size_t)i + 1] = a.gy; G[3 * (size_t)i + 2] = a.gz;
        p2[i].rho = a.rho;
        return SPHX_CT_NONE;
    }
};
BLOB_KERNEL blob_loop1_kernel(BLOB_COMMON, double d9, const RecP1* __restrict__ p1, const double* __restrict__ side,
                              double* rho, double* rhod, double* nden, double* G, RecP2* p2, BlobSel sel) {
    blob_pass(Loop1Pass{d9, p1, side, rho, rhod, nden, G, p2}, n, npad, k, nblk, nbr, slot16, uniq, qorder, 0, nullptr, n,
              nullptr, sel);
}

struct Loop2Pass {
    typedef RecP2 Rec;
    typedef L2Acc Sums;
    static constexpr int NSIDE = 1, PER_SLOT = 72;          // side value: m_j
    static constexpr bool CLIPS = false, VOTES = true, ROW_FROM_LIST = false;
    const RecP1* __restrict__ p1;
    const RecP2* __restrict__ rec;
    const double* __restrict__ m;
    const double* __restrict__ h;
    double *va, *vh;
    struct Row { Q4 s0, sv; double hq_i, g1_i, m_i, h_i; };
    struct Nb { Q8 q; double m; };
    __device__ __forceinline__ BlobSides sides() const { return {m, 1}; }
    __device__ __forceinline__ Row load_row(int i) const {
        const Q8 s = gload8(&rec[i]);
        return Row{s.lo, s.hi, p1[i].hq, p1[i].g1, m[i], h[i]};
    }
    __device__ __forceinline__ static void load_out(Row&, int, bool) {}
    // a gas particle (others: zeros, no vote)
    __device__ __forceinline__ static bool wanted(const Row& r) { return r.s0.d >= 0.0; }
    __device__ __forceinline__ Nb staged(const double2* img, const double* side, int s, const int*) const {
        return Nb{lload8(img, s), side[s]};
    }
    __device__ __forceinline__ Nb global(int j) const { return Nb{gload8(&rec[j]), m[j]}; }
    __device__ __forceinline__ static Nb none(const Row& r) { return Nb{Q8{r.s0, r.sv}, r.m_i}; }
    template <bool CLIP>
    __device__ __forceinline__ double term(Sums& a, const Nb& f, const Row& r) const {
        return loop2_term(a, f.q.lo, f.q.hi, f.m, r.s0, r.sv, r.sv.d, r.m_i, r.hq_i, r.g1_i);
    }
    __device__ __forceinline__ u64 finish(const Sums& a, double mx, const Row& r, int i, int) const {
        va[3 * (size_t)i] = a.ax; va[3 * (size_t)i + 1] = a.ay; va[3 * (size_t)i + 2] = a.az;
        vh[i] = a.heat;
        return wanted(r) ? ct_vote_bits(r.h_i, mx) : SPHX_CT_NONE;
    }
};
BLOB_KERNEL blob_loop2_kernel(BLOB_COMMON, const RecP1* __restrict__ p1, const RecP2* __restrict__ p2,
                              const double* __restrict__ m, const double* __restrict__ h, double* va, double* vh,
                              u64* ct_bits, BlobSel sel) {
    blob_pass(Loop2Pass{p1, p2, m, h, va, vh}, n, npad, k, nblk, nbr, slot16, uniq, qorder, 0, nullptr, n, ct_bits, sel);
}

// The three launches of the loop-form sums on a set of SORTED state arrays `st` (the fused loop: the resident
// state; the device-pointer API: a gathered copy of the caller's owned + ghost arrays).
static int loop_prep_launch(sphx_ctx* ctx, int64_t n, double d, StateArrays& st) {
    const size_t nb = (size_t)n * sizeof(double);
    DevBuf* outs[] = {&ctx->rho, &ctx->rhod, &ctx->nden, &ctx->vh};
    for (DevBuf* b : outs) SPHX_TRY(sphx_ensure(ctx, *b, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->G, 3 * nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->va, 3 * nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->lrec_a, (size_t)n * sizeof(RecP1)));
    SPHX_TRY(sphx_ensure(ctx, ctx->lrec_v, (size_t)n * sizeof(RecP2)));
    LoopPrepArgs p;
    p.n = (int)n;
    p.x = st.x.as<double>(); p.y = st.y.as<double>(); p.z = st.z.as<double>();
    p.vx = st.vx.as<double>(); p.vy = st.vy.as<double>(); p.vz = st.vz.as<double>();
    p.m = st.m.as<double>(); p.pt = st.ptype.as<double>();
    p.mu = st.mu.as<double>(); p.gam = st.gam.as<double>(); p.E = st.E.as<double>(); p.T = st.T.as<double>();
    p.d = d; p.m0 = ctx->cst.m_0; p.m_h = ctx->cst.m_h; p.kB = ctx->cst.k_B; p.amu = ctx->cst.amu;
    p.p1 = ctx->lrec_a.as<RecP1>(); p.p2 = ctx->lrec_v.as<RecP2>();
    hipLaunchKernelGGL(loop_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}
// The LDS form's per-neighbour side value: gamma of a gas particle (del_pressure, nsc:755); for a dust particle its mass,
// with its size (this step's kNN radius, Weigh2_dust nsc:678) put where the record keeps g1 - a factor that the type
// mask zeroes for every neighbour that is not gas; -1 for a star.  (The gather form reads type, mass and size directly.)
__global__ __launch_bounds__(256) void loop_dust_side_kernel(int n, const double* __restrict__ pt, const double* __restrict__ m,
                                                             const double* __restrict__ h, const double* __restrict__ gam,
                                                             RecP1* p1, double* side) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double t = pt[i];
    if (t == 0.0) { side[i] = gam[i]; return; }
    if (t == 2.0) { side[i] = m[i]; p1[i].g1 = h[i]; }
    else side[i] = -1.0;
}
// pass 1: h = the neighbours' kNN radii (dust_density, nsc:704-717), sorted order
static int loop_pass1_launch(sphx_ctx* ctx, int64_t n, int k, double d, StateArrays& st, const double* h) {
    const double d2 = d * d, d4 = d2 * d2, d9 = d4 * d4 * d;               // pow9(d), as the kernels form it
    const int npad = (int)sphx_pad64(n);
    RecP1* p1 = ctx->lrec_a.as<RecP1>(); RecP2* p2 = ctx->lrec_v.as<RecP2>();
    if (ctx->qorder && ctx->blob_lists) {
        SPHX_TRY(sphx_ensure(ctx, ctx->loop_side, (size_t)n * sizeof(double)));
        hipLaunchKernelGGL(loop_dust_side_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n,
                           st.ptype.as<double>(), st.m.as<double>(), h, st.gam.as<double>(), p1, ctx->loop_side.as<double>());
        SPHX_TRY(blob_launch(ctx, blob_loop1_kernel, Loop1Pass::PER_SLOT, 0, n, k, d9, p1, ctx->loop_side.as<double>(),
                             ctx->rho.as<double>(), ctx->rhod.as<double>(), ctx->nden.as<double>(), ctx->G.as<double>(), p2,
                             sphx_blob_sel(ctx, 0)));
    } else {
        hipLaunchKernelGGL(loop_pass1_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n, npad, k, d9,
                           ctx->nbr.as<int>(), p1, st.gam.as<double>(), st.ptype.as<double>(), st.m.as<double>(),
                           h, ctx->qorder, ctx->rho.as<double>(), ctx->rhod.as<double>(),
                           ctx->nden.as<double>(), ctx->G.as<double>(), p2);
    }
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}
// pass 2: h = each particle's OWN kNN radius (crossing time, nsc:782); an entry of 0 casts no vote
static int loop_pass2_launch(sphx_ctx* ctx, int64_t n, int k, StateArrays& st, const double* h, u64* ct, int part = 0) {
    ctx->visc_rows_unfilled = false;      // (ctx->va, ctx->vh are rewritten here, as in sphx_pass_visc)
    const int npad = (int)sphx_pad64(n);
    RecP1* p1 = ctx->lrec_a.as<RecP1>(); RecP2* p2 = ctx->lrec_v.as<RecP2>();
    if (ctx->qorder && ctx->blob_lists) {
        SPHX_TRY(blob_launch(ctx, blob_loop2_kernel, Loop2Pass::PER_SLOT, 0, n, k, p1, p2, st.m.as<double>(), h,
                             ctx->va.as<double>(), ctx->vh.as<double>(), ct, sphx_blob_sel(ctx, part)));
    } else {
        hipLaunchKernelGGL(loop_pass2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n, npad, k,
                           ctx->nbr.as<int>(), p1, p2, st.m.as<double>(), h, ctx->qorder, ctx->va.as<double>(),
                           ctx->vh.as<double>(), ct);
    }
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

int sphx_loop_step_sums(sphx_ctx* ctx, int64_t n, int k, double d) {
    StateArrays& st = ctx->st;
    SPHX_TRY(loop_prep_launch(ctx, n, d, st));
    u64* ct = ctx->scal.as<u64>() + SC_CT_BITS;
    // SPHX_CT_NONE = "none yet"; the previous step's dt_kernel left it so
    if (!ctx->ct_primed) SPHX_TRY(sphx_prime_ct(ctx, ct));
    ctx->ct_primed = false;
    SPHX_TRY(loop_pass1_launch(ctx, n, k, d, st, st.hprev.as<double>()));
    SPHX_TRY(loop_pass2_launch(ctx, n, k, st, st.hprev.as<double>(), ct));
    return SPHX_OK;
}

// ---- the loop-form sums on caller-order device arrays (owned + ghosts): multigpu.py, forms = "loop" ----------
// The caller's arrays are gathered into sorted order (ctx->alt), the step's kernels run on them, and the owned
// particles' results are scattered back to caller order.  Ghost neighbours need, beside their state, E (del_pressure,
// nsc:755), their kNN radius (dust_density, nsc:704) and their density (artificial_viscosity, nsc:803): three halo phases.
struct DevGatherArgs {
    int n;
    const int* perm;                         // sorted -> caller
    const double *pos, *vel, *m, *T, *mu, *gam, *pt, *E;
    double *x, *y, *z, *vx, *vy, *vz, *sm, *sT, *smu, *sgam, *spt, *sE;
};
__global__ __launch_bounds__(256) void dev_gather_state_kernel(DevGatherArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.n) return;
    const size_t c = (size_t)a.perm[s];
    a.x[s] = a.pos[3 * c]; a.y[s] = a.pos[3 * c + 1]; a.z[s] = a.pos[3 * c + 2];
    a.vx[s] = a.vel[3 * c]; a.vy[s] = a.vel[3 * c + 1]; a.vz[s] = a.vel[3 * c + 2];
    a.sm[s] = a.m[c]; a.sT[s] = a.T[c]; a.smu[s] = a.mu[c]; a.sgam[s] = a.gam[c]; a.spt[s] = a.pt[c]; a.sE[s] = a.E[c];
}
// dst_sorted[s] = src_caller[perm[s]], or 0 for ghosts when owned_only
__global__ __launch_bounds__(256) void dev_to_sorted_kernel(int n, const int* perm, int n_active, int owned_only,
                                                            const double* src, double* dst) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int c = perm[s];
    dst[s] = (owned_only && c >= n_active) ? 0.0 : src[c];
}
__global__ __launch_bounds__(256) void dev_rho_to_records_kernel(int n, const int* perm, const double* rho, RecP2* p2) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) p2[s].rho = rho[perm[s]];
}
// caller[perm[s]] = sorted[s] for owned particles, w doubles per particle
__global__ __launch_bounds__(256) void dev_to_caller_kernel(int n, const int* perm, int n_active, int w,
                                                            const double* src, double* dst) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int c = perm[s];
    if (c >= n_active) return;
    for (int q = 0; q < w; ++q) dst[(size_t)c * w + q] = src[(size_t)s * w + q];
}

extern "C" int sphx_dev_loop_prep(sphx_ctx* ctx, const double* pos, const double* vel, const double* mass,
                                  const double* T, const double* mu, const double* gamma, const double* ptype,
                                  const double* E_internal, double d) {
    if (!ctx) return SPHX_E_ARG;
    NEED(pos); NEED(vel); NEED(mass); NEED(T); NEED(mu); NEED(gamma); NEED(ptype); NEED(E_internal);
    if (!ctx->map_perm) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_dev_loop_prep before sphx_dev_search");
    if (!(d > 0.0)) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_loop_prep: d must be positive");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->n;
    StateArrays& st = ctx->alt;
    DevBuf* bufs[] = {&st.x, &st.y, &st.z, &st.vx, &st.vy, &st.vz, &st.m, &st.T, &st.mu, &st.gam, &st.ptype, &st.E,
                      &st.hprev, &st.ax};
    for (DevBuf* b : bufs) SPHX_TRY(sphx_ensure(ctx, *b, (size_t)n * sizeof(double)));
    DevGatherArgs g;
    g.n = (int)n; g.perm = ctx->map_perm;
    g.pos = pos; g.vel = vel; g.m = mass; g.T = T; g.mu = mu; g.gam = gamma; g.pt = ptype; g.E = E_internal;
    g.x = st.x.as<double>(); g.y = st.y.as<double>(); g.z = st.z.as<double>();
    g.vx = st.vx.as<double>(); g.vy = st.vy.as<double>(); g.vz = st.vz.as<double>();
    g.sm = st.m.as<double>(); g.sT = st.T.as<double>(); g.smu = st.mu.as<double>(); g.sgam = st.gam.as<double>();
    g.spt = st.ptype.as<double>(); g.sE = st.E.as<double>();
    hipLaunchKernelGGL(dev_gather_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, g);
    HIPCHK(hipGetLastError());
    ctx->loop_d = d;
    return loop_prep_launch(ctx, n, d, st);
}

extern "C" int sphx_dev_loop_pass1(sphx_ctx* ctx, const double* h_complete, double* rho, double* rho_dust, double* nden,
                                   double* delp) {
    if (!ctx) return SPHX_E_ARG;
    NEED(h_complete);
    if (!ctx->map_perm || !(ctx->loop_d > 0.0)) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_dev_loop_pass1 before sphx_dev_loop_prep");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->n;
    const unsigned grid = (unsigned)((n + 255) / 256);
    StateArrays& st = ctx->alt;
    // the neighbours' radii (sorted) for pass 1; the owned particles' own radii (ghosts 0: no crossing-time vote) for pass 2
    hipLaunchKernelGGL(dev_to_sorted_kernel, dim3(grid), dim3(256), 0, ctx->stream, (int)n, ctx->map_perm, ctx->map_nactive, 0,
                       h_complete, st.hprev.as<double>());
    hipLaunchKernelGGL(dev_to_sorted_kernel, dim3(grid), dim3(256), 0, ctx->stream, (int)n, ctx->map_perm, ctx->map_nactive, 1,
                       h_complete, st.ax.as<double>());
    SPHX_TRY(loop_pass1_launch(ctx, n, ctx->k, ctx->loop_d, st, st.hprev.as<double>()));
    struct O { double* dst; const double* src; int w; } outs[] = {{rho, ctx->rho.as<double>(), 1}, {rho_dust, ctx->rhod.as<double>(), 1},
                                                                   {nden, ctx->nden.as<double>(), 1}, {delp, ctx->G.as<double>(), 3}};
    for (O& o : outs)
        if (o.dst)
            hipLaunchKernelGGL(dev_to_caller_kernel, dim3(grid), dim3(256), 0, ctx->stream, (int)n, ctx->map_perm,
                               ctx->map_nactive, o.w, o.src, o.dst);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

// Pass 2 while rho_j is still travelling: the blobs none of whose particles has a ghost neighbour (blob_dedup_kernel's
// classes) read only densities pass 1 itself left in the records.  Returns 1 when they were launched - the call of
// sphx_dev_loop_pass2 that follows then does the boundary blobs only - and 0 when there is no such list (nothing done).
extern "C" int sphx_dev_loop_pass2_interior(sphx_ctx* ctx) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->map_perm || !(ctx->loop_d > 0.0))
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_dev_loop_pass2_interior before sphx_dev_loop_pass1");
    ctx->loop2_interior_done = false;
    if (!(ctx->qorder && ctx->blob_lists && ctx->blob_split_valid)) return 0;
    HIPCHK(hipSetDevice(ctx->device));
    u64* ct = ctx->scal.as<u64>() + SC_CT_BITS;
    SPHX_TRY(sphx_prime_ct(ctx, ct));
    ctx->ct_primed = false;
    SPHX_TRY(loop_pass2_launch(ctx, ctx->n, ctx->k, ctx->alt, ctx->alt.ax.as<double>(), ct, 1));
    ctx->loop2_interior_done = true;
    return 1;
}

extern "C" int sphx_dev_loop_pass2(sphx_ctx* ctx, const double* rho_complete, double* visc_accel, double* visc_heat,
                                   double* ct_out) {
    if (!ctx) return SPHX_E_ARG;
    NEED(rho_complete);
    if (!ctx->map_perm || !(ctx->loop_d > 0.0)) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_dev_loop_pass2 before sphx_dev_loop_prep");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->n;
    const unsigned grid = (unsigned)((n + 255) / 256);
    StateArrays& st = ctx->alt;
    hipLaunchKernelGGL(dev_rho_to_records_kernel, dim3(grid), dim3(256), 0, ctx->stream, (int)n, ctx->map_perm, rho_complete,
                       ctx->lrec_v.as<RecP2>());
    u64* ct = ctx->scal.as<u64>() + SC_CT_BITS;
    const bool rest_only = ctx->loop2_interior_done;          // (the interior blobs ran, and voted their crossing times)
    ctx->loop2_interior_done = false;
    if (!rest_only) SPHX_TRY(sphx_prime_ct(ctx, ct));
    ctx->ct_primed = false;
    SPHX_TRY(loop_pass2_launch(ctx, n, ctx->k, st, st.ax.as<double>(), ct, rest_only ? 2 : 0));
    if (visc_accel)
        hipLaunchKernelGGL(dev_to_caller_kernel, dim3(grid), dim3(256), 0, ctx->stream, (int)n, ctx->map_perm, ctx->map_nactive,
                           3, ctx->va.as<double>(), visc_accel);
    if (visc_heat)
        hipLaunchKernelGGL(dev_to_caller_kernel, dim3(grid), dim3(256), 0, ctx->stream, (int)n, ctx->map_perm, ctx->map_nactive,
                           1, ctx->vh.as<double>(), visc_heat);
    HIPCHK(hipGetLastError());
    if (ct_out)   // the positive double whose bits are the minimum (+inf = none found)
        HIPCHK(hipMemcpyAsync(ct_out, ct, 8, hipMemcpyDeviceToDevice, ctx->stream));
    return SPHX_OK;
}
