// sphx_gravity.hip - self-gravity by direct summation with Plummer softening.
//
// The reference's gravity (nsc:252-415, grav_force_calculation_new) sums, for every particle, the
// monopoles  G m_c (c - x) / (|c - x|^2 + eps^2)^(3/2)  of a few kd-tree nodes, with eps = median of
// the smoothing lengths (nsc:358).  It cannot be run here (Python-2 idioms on SciPy's old pure-Python
// KDTree), and its node selection has no published definition to restate, so there is nothing to pin an
// approximation against.  What IS well defined is the sum it approximates: every particle taken as its
// own monopole with the same softening.  That exact sum is computed here - the known-answer test any
// tree code is validated against, and a usable solver up to a few 10^5 particles (O(N^2): 5 ms at
// 10^5, 0.5 s at 10^6 on MI355X).
//
// One thread per target, sources streamed through LDS in tiles of 256 {x,y,z,m} (32 B); the sum runs
// over sources in storage order (deterministic).  1 / r^3 is rsqrt-based: v_rsq_f64 plus two Newton
// steps (relative error < 1e-15).  No MFMA: the pair kernel is not a contraction (r^-3 of a difference).
#include "sphx_internal.h"
#include <rocprim/rocprim.hpp>
#include <string.h>

#define GRAV_TILE 256

// POT: the potential beside the acceleration (include/sphx.h: phi_i = -G sum_{j != i} m_j / s).  Every term's 1 / s is the
// `inv` its acceleration term forms; row i is left out of its own sum by STORAGE INDEX (at eps > 0 the self term would be
// m_i / eps, larger than the rest of the sum by D / eps: adding it and taking it off again leaves nothing of the sum).
// A lane adds its phi terms in the order of its acceleration terms.  POT = false is the kernel without any of it, and
// POT = true forms the same acceleration bits (acc may then be NULL: nothing stored).
template <bool POT>
__global__ __launch_bounds__(GRAV_TILE) void gravity_direct_kernel(int n, const double* __restrict__ x,
                                                                   const double* __restrict__ y,
                                                                   const double* __restrict__ z, int ps,
                                                                   const double* __restrict__ m,
                                                                   const double* eps_ptr, double eps_val, double G,
                                                                   const int* __restrict__ omap, double* acc,
                                                                   double* pot) {
    __shared__ double4 tile[GRAV_TILE];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const double eps = eps_ptr ? *eps_ptr : eps_val;
    const double e2 = eps * eps;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (i < n) { xi = x[(size_t)i * ps]; yi = y[(size_t)i * ps]; zi = z[(size_t)i * ps]; }
    double ax = 0.0, ay = 0.0, az = 0.0, ph = 0.0;
    for (int j0 = 0; j0 < n; j0 += GRAV_TILE) {
        const int j = j0 + threadIdx.x;
        double4 s = make_double4(0.0, 0.0, 0.0, 0.0);          // padding sources have no mass
        if (j < n) s = make_double4(x[(size_t)j * ps], y[(size_t)j * ps], z[(size_t)j * ps], m[j]);
        __syncthreads();
        tile[threadIdx.x] = s;
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < GRAV_TILE; ++t) {
            const double4 q = tile[t];
            const double dx = q.x - xi, dy = q.y - yi, dz = q.z - zi;
            const double r2 = dx * dx + dy * dy + dz * dz + e2;
            // r2^(-3/2); a coincident pair with eps = 0 (r2 == 0) contributes nothing
            double inv = 0.0;
            if (r2 > 0.0) {            // hardware seed (2^-26) + two Newton steps: < 1e-15, without the library
                const double hr = 0.5 * r2;                    // routine's scaling and class checks (r2 is mid-range)
                double yv = __builtin_amdgcn_rsq(r2);
                yv = yv * __builtin_fma(-hr * yv, yv, 1.5);
                inv = yv * __builtin_fma(-hr * yv, yv, 1.5);
            }
            const double w = q.w * (inv * inv * inv);
            ax += w * dx; ay += w * dy; az += w * dz;
            if (POT) ph = __builtin_fma(j0 + t == i ? 0.0 : q.w, inv, ph);
        }
    }
    if (i < n) {
        const int o = omap ? omap[i] : i;
        if (!POT || acc) { acc[3 * (size_t)o] = G * ax; acc[3 * (size_t)o + 1] = G * ay; acc[3 * (size_t)o + 2] = G * az; }
        if (POT) pot[o] = -G * ph;
    }
}

// median of h (n values) -> *out, NumPy's definition (mean of the two middle values for even n)
__global__ void median_pick_kernel(int n, const double* sorted, double* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0)
        *out = (n & 1) ? sorted[n / 2] : 0.5 * (sorted[n / 2 - 1] + sorted[n / 2]);
}

int sphx_median(sphx_ctx* ctx, int64_t n, const double* v, double* out_dev) {
    SPHX_TRY(sphx_ensure(ctx, ctx->grav_sort, (size_t)n * sizeof(double)));
    size_t tmp = 0;
    HIPCHK(rocprim::radix_sort_keys(nullptr, tmp, v, ctx->grav_sort.as<double>(), (size_t)n, 0, 64, ctx->stream));
    SPHX_TRY(sphx_ensure(ctx, ctx->grav_tmp, tmp));
    HIPCHK(rocprim::radix_sort_keys(ctx->grav_tmp.p, tmp, v, ctx->grav_sort.as<double>(), (size_t)n, 0, 64,
                                    ctx->stream));
    hipLaunchKernelGGL(median_pick_kernel, dim3(1), dim3(64), 0, ctx->stream, (int)n, ctx->grav_sort.as<double>(),
                       out_dev);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

// device arrays; eps from device memory (eps_dev) or by value
int sphx_gravity_launch(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z, int ps,
                        const double* m, const double* eps_dev, double eps, double G, const int* omap,
                        double* acc) {
    return sphx_gravity_pot_launch(ctx, n, x, y, z, ps, m, eps_dev, eps, G, omap, acc, nullptr);
}
int sphx_gravity_pot_launch(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z, int ps,
                            const double* m, const double* eps_dev, double eps, double G, const int* omap,
                            double* acc, double* pot) {
    const dim3 grid((unsigned)((n + GRAV_TILE - 1) / GRAV_TILE)), block(GRAV_TILE);
    if (pot)
        hipLaunchKernelGGL(gravity_direct_kernel<true>, grid, block, 0, ctx->stream, (int)n, x, y, z, ps, m, eps_dev, eps, G,
                           omap, acc, pot);
    else
        hipLaunchKernelGGL(gravity_direct_kernel<false>, grid, block, 0, ctx->stream, (int)n, x, y, z, ps, m, eps_dev, eps, G,
                           omap, acc, pot);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

// sphx_gravity_direct (pot == NULL) and sphx_gravity_direct_pot (accel nullable) on host arrays
static int grav_direct_host(sphx_ctx* ctx, const char* who, int64_t n, const double* mass, const double* points,
                            const double* sizes, double softening, double G, double* accel, double* pot) {
    if (!ctx) return SPHX_E_ARG;
    if (!mass || !points || !(pot || accel)) return sphx_set_err(ctx, SPHX_E_ARG, "%s: NULL argument", who);
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "n=%lld out of range", (long long)n);
    if (!sizes && !(softening >= 0.0)) return sphx_set_err(ctx, SPHX_E_ARG, "softening must be >= 0");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nb = (size_t)n * sizeof(double);
    SPHX_TRY(sphx_ensure(ctx, ctx->in_a, 3 * nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->in_b, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->out_b, 3 * nb));
    if (pot) {
        SPHX_TRY(sphx_ensure(ctx, ctx->gravpot_buf, nb));
        SPHX_TRY(ctx->gravpot_t.begin(ctx));
    }
    HIPCHK(hipMemcpyAsync(ctx->in_a.p, points, 3 * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->in_b.p, mass, nb, hipMemcpyHostToDevice, ctx->stream));
    const double* eps_dev = nullptr;
    if (sizes) {                                   // eps = median(sizes), nsc:358
        SPHX_TRY(sphx_ensure(ctx, ctx->in_c, nb));
        HIPCHK(hipMemcpyAsync(ctx->in_c.p, sizes, nb, hipMemcpyHostToDevice, ctx->stream));
        double* slot = ctx->scal.as<double>() + SC_GRAV_EPS;
        SPHX_TRY(sphx_median(ctx, n, ctx->in_c.as<double>(), slot));
        eps_dev = slot;
    }
    const double* p = ctx->in_a.as<double>();
    if (pot) { SPHX_TRY(ctx->gravpot_t.mark(ctx, 1)); SPHX_TRY(ctx->gravpot_t.mark(ctx, 2)); }
    SPHX_TRY(sphx_gravity_pot_launch(ctx, n, p, p + 1, p + 2, 3, ctx->in_b.as<double>(), eps_dev, softening, G, nullptr,
                                     accel ? ctx->out_b.as<double>() : nullptr, pot ? ctx->gravpot_buf.as<double>() : nullptr));
    if (pot) SPHX_TRY(ctx->gravpot_t.mark(ctx, 3));
    if (accel) HIPCHK(hipMemcpyAsync(accel, ctx->out_b.p, 3 * nb, hipMemcpyDeviceToHost, ctx->stream));
    if (pot) {
        HIPCHK(hipMemcpyAsync(pot, ctx->gravpot_buf.p, nb, hipMemcpyDeviceToHost, ctx->stream));
        SPHX_TRY(ctx->gravpot_t.mark(ctx, 4));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return pot ? ctx->gravpot_t.end(ctx) : SPHX_OK;
}
extern "C" int sphx_gravity_direct(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                                   const double* sizes, double softening, double G, double* accel) {
    if (ctx && !accel) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_gravity_direct: NULL argument");
    return grav_direct_host(ctx, "sphx_gravity_direct", n, mass, points, sizes, softening, G, accel, nullptr);
}
extern "C" int sphx_gravity_direct_pot(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                                       const double* sizes, double softening, double G, double* accel, double* pot) {
    if (ctx && !pot) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_gravity_direct_pot: NULL argument");
    return grav_direct_host(ctx, "sphx_gravity_direct_pot", n, mass, points, sizes, softening, G, accel, pot);
}

// =================================================================================================
// Tree form: monopoles of a cell pyramid over the search grid
// =================================================================================================
// The fine grid of the neighbour search (cells of 0.6 mean h, particles stored cell by cell) is the
// leaf level; level l has cells of 2^l fine cells a side with (mass, centre of mass).  A particle in
// level-l cell C takes, at each level l >= 1, the monopoles of the children of its parent's
// neighbours (+-ws parents) that are not themselves neighbours of C (+-ws cells) - the interaction
// list of a uniform-grid FMM, at most (2(2ws+1))^3 - (2ws+1)^3 cells (189 at ws = 1, 875 at ws = 2) -
// and sums directly over the particles of the level-1 cells within +-ws of its own.  Every source is
// counted exactly once; softening (eps) applies to monopoles and particles alike, as in the
// reference.  ws = 1: ~1.5e3 terms per particle, ~1 % rms force error; ws = 2: ~7e3 terms, ~0.2 %.
// One thread per particle in processing (blob) order, so the lanes of a wave walk the same cells
// and their loads of a cell record coalesce into one request.
// Centres of mass are held RELATIVE to a point inside the cloud (GravRef: the centre of the grid box), and the walks take cell - particle
// differences in that frame: a centre sum m x / M of absolute coordinates carries ulp(|x|), which for a cloud of size D at
// distance T from the origin is T / D times the round-off of the differences themselves (1e-7 of a row at T / D = 2^27).
// The near field differences two particles directly and needs no frame.
// (PYR_MAX, GravRef, Pyr: sphx_internal.h)

__global__ __launch_bounds__(256) void pyr_level1_kernel(GridParams g, Pyr py, const int* __restrict__ cell_start,
                                                         const double* __restrict__ x, const double* __restrict__ y,
                                                         const double* __restrict__ z, const double* __restrict__ m,
                                                         GravRef ref, double4* pyr, double4* quad) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int nx1 = py.nx[1], ny1 = py.ny[1], nz1 = py.nz[1];
    if (c >= nx1 * ny1 * nz1) return;
    const int X = c % nx1, Y = (c / nx1) % ny1, Z = c / (nx1 * ny1);
    const int fx0 = 2 * X, fx1 = min(2 * X + 2, g.nx);
    // first moments about the cell's first member (p0), so that an axis on which all members agree gives that value
    // back exactly (a line or a plane has no force across it, to the last bit)
    double sm = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, p0x = 0.0, p0y = 0.0, p0z = 0.0;
    bool have = false;
    for (int fz = 2 * Z; fz < min(2 * Z + 2, g.nz); ++fz)
        for (int fy = 2 * Y; fy < min(2 * Y + 2, g.ny); ++fy) {
            const int row = (fz * g.ny + fy) * g.nx;
            const int s = cell_start[row + fx0], e = cell_start[row + fx1];
            for (int j = s; j < e; ++j) {
                const double mj = m[j], rx = x[j] - ref.x, ry = y[j] - ref.y, rz = z[j] - ref.z;
                if (!have) { p0x = rx; p0y = ry; p0z = rz; have = true; }
                sm += mj; sx += mj * (rx - p0x); sy += mj * (ry - p0y); sz += mj * (rz - p0z);
            }
        }
    const bool massive = sm > 0.0;
    const double inv = massive ? 1.0 / sm : 0.0;
    const double cxm = massive ? p0x + sx * inv : 0.0, cym = massive ? p0y + sy * inv : 0.0,
                 czm = massive ? p0z + sz * inv : 0.0;
    pyr[py.off[1] + c] = make_double4(sm, cxm, cym, czm);
    if (quad) {
        // second moments about the centre of mass, S_ab = sum m d_a d_b (not made traceless: the
        // softened kernel is not harmonic, its expansion keeps the trace)
        double qxx = 0.0, qyy = 0.0, qzz = 0.0, qxy = 0.0, qxz = 0.0, qyz = 0.0;
        for (int fz = 2 * Z; fz < min(2 * Z + 2, g.nz); ++fz)
            for (int fy = 2 * Y; fy < min(2 * Y + 2, g.ny); ++fy) {
                const int row = (fz * g.ny + fy) * g.nx;
                const int s = cell_start[row + fx0], e = cell_start[row + fx1];
                for (int j = s; j < e; ++j) {
                    const double mj = m[j], dx = (x[j] - ref.x) - cxm, dy = (y[j] - ref.y) - cym, dz = (z[j] - ref.z) - czm;
                    qxx += mj * dx * dx; qyy += mj * dy * dy; qzz += mj * dz * dz;
                    qxy += mj * dx * dy; qxz += mj * dx * dz; qyz += mj * dy * dz;
                }
            }
        quad[2 * (py.off[1] + c)] = make_double4(qxx, qyy, qzz, qxy);
        quad[2 * (py.off[1] + c) + 1] = make_double4(qxz, qyz, 0.0, 0.0);
    }
}

__global__ __launch_bounds__(256) void pyr_up_kernel(Pyr py, int l, double4* pyr, double4* quad) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int nxl = py.nx[l], nyl = py.ny[l], nzl = py.nz[l];
    if (c >= nxl * nyl * nzl) return;
    const int X = c % nxl, Y = (c / nxl) % nyl, Z = c / (nxl * nyl);
    const int cx = py.nx[l - 1], cy = py.ny[l - 1], cz = py.nz[l - 1];
    const double4* ch = pyr + py.off[l - 1];
    double sm = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, p0x = 0.0, p0y = 0.0, p0z = 0.0;     // (p0: the first massive child)
    bool have = false;
    for (int k = 2 * Z; k < min(2 * Z + 2, cz); ++k)
        for (int j = 2 * Y; j < min(2 * Y + 2, cy); ++j)
            for (int i = 2 * X; i < min(2 * X + 2, cx); ++i) {
                const double4 q = ch[((size_t)k * cy + j) * cx + i];
                sm += q.x;                                      // (every child's mass, so that a NaN still travels up)
                if (!(q.x > 0.0)) continue;                     // a massless child has no centre to offer
                if (!have) { p0x = q.y; p0y = q.z; p0z = q.w; have = true; }
                sx += q.x * (q.y - p0x); sy += q.x * (q.z - p0y); sz += q.x * (q.w - p0z);
            }
    const double inv = sm > 0.0 ? 1.0 / sm : 0.0;
    const double cxm = p0x + sx * inv, cym = p0y + sy * inv, czm = p0z + sz * inv;          // (no massive child: 0)
    pyr[py.off[l] + c] = make_double4(sm, cxm, cym, czm);
    if (quad) {
        // S = sum over children of S_child + M_child s s^T, s = child's centre - this centre
        const double4* qh = quad + 2 * py.off[l - 1];
        double qxx = 0.0, qyy = 0.0, qzz = 0.0, qxy = 0.0, qxz = 0.0, qyz = 0.0;
        for (int k = 2 * Z; k < min(2 * Z + 2, cz); ++k)
            for (int j = 2 * Y; j < min(2 * Y + 2, cy); ++j)
                for (int i = 2 * X; i < min(2 * X + 2, cx); ++i) {
                    const size_t cc = ((size_t)k * cy + j) * cx + i;
                    const double4 q = ch[cc];
                    if (!(q.x > 0.0)) continue;
                    const double4 b = qh[2 * cc], e = qh[2 * cc + 1];
                    const double dx = q.y - cxm, dy = q.z - cym, dz = q.w - czm;
                    qxx += b.x + q.x * dx * dx; qyy += b.y + q.x * dy * dy; qzz += b.z + q.x * dz * dz;
                    qxy += b.w + q.x * dx * dy; qxz += e.x + q.x * dx * dz; qyz += e.y + q.x * dy * dz;
                }
        quad[2 * (py.off[l] + c)] = make_double4(qxx, qyy, qzz, qxy);
        quad[2 * (py.off[l] + c) + 1] = make_double4(qxz, qyz, 0.0, 0.0);
    }
}

// Monopole + second moments of a cell (M at c, S_ab = sum m d_a d_b about c) on a particle at x, r = c - x:
// the Taylor expansion of the SOFTENED kernel 1 / sqrt(r^2 + eps^2) to second order, s^2 = r^2 + eps^2,
//   a = (M / s^3 + 15/2 (r.S.r) / s^7 - 3/2 tr(S) / s^5) r - 3 (S.r) / s^5
// (for eps = 0 this is the usual traceless-quadrupole term).  f = 1 for a cell of the lane's list, else 0.
// s2 = 0 (no softening, and the cell's centre exactly on the particle: the wave kernel also runs, with f = 0, over the
// lane's own cell, and a lone particle's cell IS the particle) contributes nothing - as a coincident pair does in the
// direct sum; without the guard that term is 0 * inf.
// POT (every term below): the potential of the same record into *ph, as the positive sum the kernels store as -G ph -
//   a particle or monopole   qp / s                                         (qp: the mass the potential counts, 0 for the
//                                                                            lane's own row and for a masked record)
//   a cell of order 2        f [ M / s + 3/2 (r.S.r) / s^5 - 1/2 tr S / s^3 ]
// the second-order expansion of 1 / sqrt(|c + d - x|^2 + eps^2) in d summed over the cell, whose negative gradient in x is
// the acceleration term beside it.  1 / s is the `inv` the term has formed (no second rsqrt), so s2 = 0 gives nothing
// here too.  The fmas are written out: the wave kernel and the per-thread walk then round alike whatever the compiler
// contracts around them.  POT = false: the code without it.
template <bool POT = false>
__device__ __forceinline__ void grav_term_quad(double4 a4, double4 b4, double4 c4, double f, double xi, double yi,
                                               double zi, double e2, double& ax, double& ay, double& az,
                                               double* ph = nullptr) {
    const double dx = a4.y - xi, dy = a4.z - yi, dz = a4.w - zi;
    const double r2 = dx * dx + dy * dy + dz * dz + e2;
    const double y0 = r2 > 0.0 ? __builtin_amdgcn_rsq(r2) : 0.0;
    const double inv = y0 * __builtin_fma(-0.5 * r2 * y0, y0, 1.5);
    const double inv2 = inv * inv, inv3 = inv * inv2, inv5 = inv3 * inv2, inv7 = inv5 * inv2;
    const double srx = b4.x * dx + b4.w * dy + c4.x * dz;
    const double sry = b4.w * dx + b4.y * dy + c4.y * dz;
    const double srz = c4.x * dx + c4.y * dy + b4.z * dz;
    const double rsr = dx * srx + dy * sry + dz * srz;
    const double tr = b4.x + b4.y + b4.z;
    const double cr = f * (a4.x * inv3 + 7.5 * rsr * inv7 - 1.5 * tr * inv5), cq = f * 3.0 * inv5;
    ax += cr * dx - cq * srx; ay += cr * dy - cq * sry; az += cr * dz - cq * srz;
    if (POT) {
        const double pc = __builtin_fma(1.5 * rsr, inv5, __builtin_fma(-0.5 * tr, inv3, a4.x * inv));
        *ph = __builtin_fma(f, pc, *ph);
    }
}

// the same term where the softening guarantees r2 > 0 (no guard, no select)
template <bool POT = false>
__device__ __forceinline__ void grav_term_soft(double qx, double qy, double qz, double qm, double xi, double yi,
                                               double zi, double e2, double& ax, double& ay, double& az,
                                               double qp = 0.0, double* ph = nullptr) {
    const double dx = qx - xi, dy = qy - yi, dz = qz - zi;
    const double r2 = dx * dx + dy * dy + dz * dz + e2;
    const double y0 = __builtin_amdgcn_rsq(r2);
    const double inv = y0 * __builtin_fma(-0.5 * r2 * y0, y0, 1.5);
    const double w = qm * (inv * inv * inv);
    ax += w * dx; ay += w * dy; az += w * dz;
    if (POT) *ph = __builtin_fma(qp, inv, *ph);
}
template <bool POT = false>
__device__ __forceinline__ void grav_term(double qx, double qy, double qz, double qm, double xi, double yi, double zi,
                                          double e2, double& ax, double& ay, double& az, double qp = 0.0,
                                          double* ph = nullptr) {
    const double dx = qx - xi, dy = qy - yi, dz = qz - zi;
    const double r2 = dx * dx + dy * dy + dz * dz + e2;
    // 1/sqrt: the hardware seed (v_rsq_f64, ~2^-26) and one Newton step (~2^-51) instead of the library
    // routine's two steps, scaling and class checks - r2 sits mid-range (m^2), and a monopole sum that is
    // good to 1e-3 has no use for the last bit.  (The exact direct sum above keeps rsqrt().)
    double inv = 0.0;
    if (r2 > 0.0) {
        const double y0 = __builtin_amdgcn_rsq(r2);
        inv = y0 * __builtin_fma(-0.5 * r2 * y0, y0, 1.5);
    }
    const double w = qm * (inv * inv * inv);
    ax += w * dx; ay += w * dy; az += w * dz;
    if (POT) *ph = __builtin_fma(qp, inv, *ph);
}

// per-lane walks (each thread its own loops and loads): the per-thread kernel, and the wave kernel's
// fall-back where a wave's particles are not neighbours (blob order has a few long jumps)
// (POT: i is the lane's own row in x, y, z, m - left out of its potential by index)
template <bool POT>
__device__ __forceinline__ void near_walk_lane(const GridParams& g, int ws, int fx, int fy, int fz,
                                               const int* __restrict__ cell_start, const double* __restrict__ x,
                                               const double* __restrict__ y, const double* __restrict__ z,
                                               const double* __restrict__ m, double xi, double yi, double zi, double e2,
                                               double& ax, double& ay, double& az, int i, double* ph) {
    const int X = fx >> 1, Y = fy >> 1, Z = fz >> 1;
    const int x0 = max(2 * (X - ws), 0), x1 = min(2 * (X + ws) + 2, g.nx);
    const int y0 = max(2 * (Y - ws), 0), y1 = min(2 * (Y + ws) + 2, g.ny);
    const int z0 = max(2 * (Z - ws), 0), z1 = min(2 * (Z + ws) + 2, g.nz);
    for (int kz = z0; kz < z1; ++kz)
        for (int ky = y0; ky < y1; ++ky) {
            const int row = (kz * g.ny + ky) * g.nx;
            const int s = cell_start[row + x0], e = cell_start[row + x1];
            for (int j = s; j < e; ++j) {
                const double mj = m[j];
                grav_term<POT>(x[j], y[j], z[j], mj, xi, yi, zi, e2, ax, ay, az, POT ? (j == i ? 0.0 : mj) : 0.0, ph);
            }
        }
}
template <bool POT>
__device__ __forceinline__ void far_walk_lane(int ws, int X, int Y, int Z, int nxl, int nyl, int nzl,
                                              const double4* __restrict__ lev, const double4* __restrict__ qlev,
                                              double xi, double yi, double zi,
                                              double e2, double& ax, double& ay, double& az, double* ph) {
    const int PX = X >> 1, PY = Y >> 1, PZ = Z >> 1;
    const int x0 = max(2 * (PX - ws), 0), x1 = min(2 * (PX + ws) + 1, nxl - 1);
    const int y0 = max(2 * (PY - ws), 0), y1 = min(2 * (PY + ws) + 1, nyl - 1);
    const int z0 = max(2 * (PZ - ws), 0), z1 = min(2 * (PZ + ws) + 1, nzl - 1);
    for (int kz = z0; kz <= z1; ++kz) {
        const bool nz_ = abs(kz - Z) <= ws;
        for (int ky = y0; ky <= y1; ++ky) {
            const bool nyz = nz_ && abs(ky - Y) <= ws;
            const double4* rowp = lev + ((size_t)kz * nyl + ky) * nxl;
            for (int kx = x0; kx <= x1; ++kx) {
                if (nyz && abs(kx - X) <= ws) continue;          // a neighbour: resolved at a finer level
                const double4 q = rowp[kx];
                if (!(q.x > 0.0)) continue;
                if (qlev) {
                    const size_t cc = ((size_t)kz * nyl + ky) * nxl + kx;
                    grav_term_quad<POT>(q, qlev[2 * cc], qlev[2 * cc + 1], 1.0, xi, yi, zi, e2, ax, ay, az, ph);
                } else {
                    grav_term<POT>(q.y, q.z, q.w, q.x, xi, yi, zi, e2, ax, ay, az, q.x, ph);
                }
            }
        }
    }
}

template <bool POT>
__global__ __launch_bounds__(256) void gravity_tree_kernel(int n, GridParams g, Pyr py, int ws,
                                                           const int* __restrict__ cell_of_sorted,
                                                           const int* __restrict__ cell_start,
                                                           const double* __restrict__ x, const double* __restrict__ y,
                                                           const double* __restrict__ z, const double* __restrict__ m,
                                                           const double4* __restrict__ pyr,
                                                           const double4* __restrict__ quad, const double* eps_ptr,
                                                           double eps_val, double G, GravRef ref,
                                                           const int* __restrict__ qorder,
                                                           const int* __restrict__ omap, double* acc, double* pot) {
    const int p = xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int i = qorder ? qorder[p] : p;
    const double eps = eps_ptr ? *eps_ptr : eps_val;
    const double e2 = eps * eps;
    const double xi = x[i], yi = y[i], zi = z[i];
    const int c0 = cell_of_sorted[i];
    const int fx = c0 % g.nx, fy = (c0 / g.nx) % g.ny, fz = c0 / (g.nx * g.ny);
    double ax = 0.0, ay = 0.0, az = 0.0, ph = 0.0;
    near_walk_lane<POT>(g, ws, fx, fy, fz, cell_start, x, y, z, m, xi, yi, zi, e2, ax, ay, az, i, &ph);
    const double xr = xi - ref.x, yr = yi - ref.y, zr = zi - ref.z;          // the cells' frame
    for (int l = 1; l < py.nlev; ++l)
        far_walk_lane<POT>(ws, fx >> l, fy >> l, fz >> l, py.nx[l], py.ny[l], py.nz[l], pyr + py.off[l],
                           quad ? quad + 2 * py.off[l] : nullptr, xr, yr, zr, e2, ax, ay, az, &ph);
    const int o = omap ? omap[i] : i;
    if (!POT || acc) { acc[3 * (size_t)o] = G * ax; acc[3 * (size_t)o + 1] = G * ay; acc[3 * (size_t)o + 2] = G * az; }
    if (POT) pot[o] = -G * ph;
}

// ---- the same sum, one WAVE per 64 particles working through LDS -----------------------------------
// The 64 particles of a wave are neighbours (blob order), so their near regions and interaction lists
// overlap almost entirely.  At every level the wave takes the UNION box of its lanes' lists, stages it
// plane by plane into LDS with coalesced loads (each cell record / particle once per wave, not once per
// lane), and every lane runs over the staged records with broadcast LDS reads, a per-lane bit mask
// saying which of them belong to ITS list.  A lane adds its own terms in the same order as the
// per-thread kernel above (masked ones add +0): the result is bit-identical to it.
#define GT_CB 192                       // cell records / particles staged per wave
#ifndef GT_SLACK
#define GT_SLACK 1                      // cells a wave's union box may exceed one lane's box by, per axis
#endif
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return __builtin_amdgcn_readfirstlane(v);
}
// bits a..b (inclusive) of a 32-bit word, the range clipped to 0..31
__device__ __forceinline__ unsigned range_bits(int a, int b) {
    a = max(a, 0); b = min(b, 31);
    if (b < a) return 0u;
    const unsigned upto_b = (b == 31) ? 0xFFFFFFFFu : ((2u << b) - 1u);
    return upto_b & ~((1u << a) - 1u);
}
__device__ __forceinline__ void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// QUAD: cells carry quadrupoles too (three 32-B pieces per staged cell, half as many cells per stage)
// POT: the potential beside it.  A staged near-field record t of a batch is row j0 + t of the arrays, so the lane knows
// its own record by index; a masked record adds +0.0 to phi as it does to the acceleration.
template <bool QUAD, bool POT>
__global__ __launch_bounds__(256) void gravity_tree_wave_kernel(int n, GridParams g, Pyr py, int ws,
                                                                const int* __restrict__ cell_of_sorted,
                                                                const int* __restrict__ cell_start,
                                                                const double* __restrict__ x, const double* __restrict__ y,
                                                                const double* __restrict__ z, const double* __restrict__ m,
                                                                const double4* __restrict__ pyr,
                                                                const double4* __restrict__ quad, const double* eps_ptr,
                                                                double eps_val, double G, GravRef ref,
                                                                const int* __restrict__ qorder,
                                                                const int* __restrict__ omap, double* acc, double* pot) {
    constexpr int CB = QUAD ? GT_CB / 2 : GT_CB;      // cells staged at a time
    __shared__ double4 cbuf_all[4][QUAD ? 3 * (GT_CB / 2) : GT_CB];
    __shared__ int ibuf_all[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double4* cbuf = cbuf_all[wave];
    int* ibuf = ibuf_all[wave];
    const int p = xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
    const bool act = p < n;
    if (__builtin_amdgcn_ballot_w64(act) == 0ull) return;          // (a wave past the end)
    const int i = act ? (qorder ? qorder[p] : p) : 0;
    const double eps = eps_ptr ? *eps_ptr : eps_val;
    const double e2 = eps * eps;
    const bool soft = e2 > 1e-290;                                  // (wave-uniform)
    const double xi = x[i], yi = y[i], zi = z[i];
    int c0 = cell_of_sorted[i];
    c0 = act ? c0 : __builtin_amdgcn_readfirstlane(c0);             // idle lanes (last wave) shadow lane 0
    const int fx = c0 % g.nx, fy = (c0 / g.nx) % g.ny, fz = c0 / (g.nx * g.ny);
    double ax = 0.0, ay = 0.0, az = 0.0, ph = 0.0;
    // ---- near field: particles of the level-1 cells within +-ws of the lane's level-1 cell ---------
    {
        const int X = fx >> 1, Y = fy >> 1, Z = fz >> 1;
        const int lx0 = max(2 * (X - ws), 0), lx1 = min(2 * (X + ws) + 2, g.nx) - 1;      // fine cells, inclusive
        const int ly0 = max(2 * (Y - ws), 0), ly1 = min(2 * (Y + ws) + 2, g.ny) - 1;
        const int lz0 = max(2 * (Z - ws), 0), lz1 = min(2 * (Z + ws) + 2, g.nz) - 1;
        const int ux0 = wave_min_i(lx0), ux1 = wave_max_i(lx1);
        const int uy0 = wave_min_i(ly0), uy1 = wave_max_i(ly1);
        const int uz0 = wave_min_i(lz0), uz1 = wave_max_i(lz1);
        // the wave's particles are neighbours: its union box is little more than one lane's box
        const int own = 4 * ws + 2 + GT_SLACK;
        const bool compact = ux1 - ux0 < own && uy1 - uy0 < own && uz1 - uz0 < own;
        if (!compact) near_walk_lane<POT>(g, ws, fx, fy, fz, cell_start, x, y, z, m, xi, yi, zi, e2, ax, ay, az, i, &ph);
        for (int kz = uz0; compact && kz <= uz1; ++kz) {
            const bool zin = kz >= lz0 && kz <= lz1;
            for (int ky = uy0; ky <= uy1; ++ky) {
                const bool rowin = zin && ky >= ly0 && ky <= ly1;
                const int row = (kz * g.ny + ky) * g.nx;
                const int s = __builtin_amdgcn_readfirstlane(cell_start[row + ux0]);
                const int e = __builtin_amdgcn_readfirstlane(cell_start[row + ux1 + 1]);
                for (int j0 = s; j0 < e; j0 += 64) {
                    const int cnt = min(64, e - j0);
                    if (lane < cnt) {
                        const int j = j0 + lane;
                        cbuf[lane] = make_double4(x[j], y[j], z[j], m[j]);
                        ibuf[lane] = cell_of_sorted[j] - row;                   // the particle's fine x cell
                    }
                    lds_sync();
                    for (int t = 0; t < cnt; ++t) {
                        const double4 q = cbuf[t];
                        const int cx = ibuf[t];
                        const bool mine = rowin && cx >= lx0 && cx <= lx1;
                        grav_term<POT>(q.x, q.y, q.z, mine ? q.w : 0.0, xi, yi, zi, e2, ax, ay, az,
                                       POT ? ((mine && j0 + t != i) ? q.w : 0.0) : 0.0, &ph);
                    }
                    lds_sync();
                }
            }
        }
    }
    // ---- far field: interaction lists, level by level (in the cells' frame) ---------------------------
    const double xr = xi - ref.x, yr = yi - ref.y, zr = zi - ref.z;
    for (int l = 1; l < py.nlev; ++l) {
        const int X = fx >> l, Y = fy >> l, Z = fz >> l;
        const int PX = X >> 1, PY = Y >> 1, PZ = Z >> 1;
        const int nxl = py.nx[l], nyl = py.ny[l], nzl = py.nz[l];
        const int lx0 = max(2 * (PX - ws), 0), lx1 = min(2 * (PX + ws) + 1, nxl - 1);
        const int ly0 = max(2 * (PY - ws), 0), ly1 = min(2 * (PY + ws) + 1, nyl - 1);
        const int lz0 = max(2 * (PZ - ws), 0), lz1 = min(2 * (PZ + ws) + 1, nzl - 1);
        const double4* lev = pyr + py.off[l];
        const int ux0 = wave_min_i(lx0), ux1 = wave_max_i(lx1);
        const int uy0 = wave_min_i(ly0), uy1 = wave_max_i(ly1);
        const int uz0 = wave_min_i(lz0), uz1 = wave_max_i(lz1);
        const int W = ux1 - ux0 + 1;
        const int own = 4 * ws + 2 + GT_SLACK;
        if (W > 32 || W > own || uy1 - uy0 >= own || uz1 - uz0 >= own) {
            // a wave spread over more cells than neighbours would be: the per-lane walk
            far_walk_lane<POT>(ws, X, Y, Z, nxl, nyl, nzl, lev, QUAD ? quad + 2 * py.off[l] : nullptr, xr, yr, zr, e2,
                               ax, ay, az, &ph);
            continue;
        }
        const double4* qlev = QUAD ? quad + 2 * py.off[l] : nullptr;
        const unsigned xlist = range_bits(lx0 - ux0, lx1 - ux0);          // the lane's x range within the union row
        const unsigned xnear = range_bits(X - ws - ux0, X + ws - ux0);    // ... and its own neighbourhood in it
        const int rpc = CB / W;                                           // rows staged at a time
        for (int kz = uz0; kz <= uz1; ++kz) {
            const bool zin = kz >= lz0 && kz <= lz1;
            const bool znear = abs(kz - Z) <= ws;
            for (int kyc = uy0; kyc <= uy1; kyc += rpc) {
                const int nr = min(rpc, uy1 - kyc + 1);
                for (int r = 0; r < nr; ++r)
                    if (lane < W) {
                        const size_t cc = ((size_t)kz * nyl + (kyc + r)) * nxl + ux0 + lane;
                        cbuf[r * W + lane] = lev[cc];
                        if (QUAD) { cbuf[CB + r * W + lane] = qlev[2 * cc]; cbuf[2 * CB + r * W + lane] = qlev[2 * cc + 1]; }
                    }
                lds_sync();
                for (int r = 0; r < nr; ++r) {
                    const int ky = kyc + r;
                    const bool yin = zin && ky >= ly0 && ky <= ly1;
                    const bool near_row = znear && abs(ky - Y) <= ws;
                    const unsigned bits = yin ? (near_row ? (xlist & ~xnear) : xlist) : 0u;
                    const double4* rowq = cbuf + r * W;
                    if (QUAD) {
                        for (int t = 0; t < W; ++t) {
                            const double4 q = rowq[t];
                            if (!(q.x > 0.0)) continue;                           // (uniform: an empty cell)
                            grav_term_quad<POT>(q, rowq[CB + t], rowq[2 * CB + t], ((bits >> t) & 1u) ? 1.0 : 0.0, xr, yr, zr,
                                                e2, ax, ay, az, &ph);
                        }
                    } else if (soft) {
                        // r2 >= eps^2 > 0: no guard; two records in flight per trip
                        int t = 0;
                        for (; t + 1 < W; t += 2) {
                            const double4 q0 = rowq[t], q1 = rowq[t + 1];
                            grav_term_soft<POT>(q0.y, q0.z, q0.w, ((bits >> t) & 1u) ? q0.x : 0.0, xr, yr, zr, e2, ax, ay, az,
                                                POT ? (((bits >> t) & 1u) ? q0.x : 0.0) : 0.0, &ph);
                            grav_term_soft<POT>(q1.y, q1.z, q1.w, ((bits >> (t + 1)) & 1u) ? q1.x : 0.0, xr, yr, zr, e2, ax, ay, az,
                                                POT ? (((bits >> (t + 1)) & 1u) ? q1.x : 0.0) : 0.0, &ph);
                        }
                        if (t < W) {
                            const double4 q0 = rowq[t];
                            grav_term_soft<POT>(q0.y, q0.z, q0.w, ((bits >> t) & 1u) ? q0.x : 0.0, xr, yr, zr, e2, ax, ay, az,
                                                POT ? (((bits >> t) & 1u) ? q0.x : 0.0) : 0.0, &ph);
                        }
                    } else {
                        for (int t = 0; t < W; ++t) {
                            const double4 q = rowq[t];
                            if (!(q.x > 0.0)) continue;                           // (uniform: an empty cell)
                            grav_term<POT>(q.y, q.z, q.w, ((bits >> t) & 1u) ? q.x : 0.0, xr, yr, zr, e2, ax, ay, az,
                                           POT ? (((bits >> t) & 1u) ? q.x : 0.0) : 0.0, &ph);
                        }
                    }
                }
                lds_sync();
            }
        }
    }
    if (act) {
        const int o = omap ? omap[i] : i;
        if (!POT || acc) { acc[3 * (size_t)o] = G * ax; acc[3 * (size_t)o + 1] = G * ay; acc[3 * (size_t)o + 2] = G * az; }
        if (POT) pot[o] = -G * ph;
    }
}

__global__ __launch_bounds__(256) void gather1_kernel(int n, const int* perm, const double* in, double* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = in[perm[t]];
}

__global__ __launch_bounds__(256) void sorted_cells_kernel(int n, const int* cell_of, const int* perm, int* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = cell_of[perm[t]];
}

// The pyramid (and, at order 2, its second moments) of those particles, into ctx->grav_pyr / grav_quad; the fine cell
// of every sorted particle into ctx->grav_cell.  py and ref say how it is laid out and about which point.
// about: the frame to use (a decomposed run's ranks share one); nullptr: a point inside this cloud.
static int grav_pyramid(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z, const double* m,
                        Pyr& py, GravRef& ref, const GravRef* about = nullptr) {
    const GridParams g = ctx->grid;
    memset(&py, 0, sizeof(py));
    py.nx[0] = g.nx; py.ny[0] = g.ny; py.nz[0] = g.nz;
    long long tot = 0;
    int l = 0;
    do {
        ++l;
        py.nx[l] = (py.nx[l - 1] + 1) / 2; py.ny[l] = (py.ny[l - 1] + 1) / 2; py.nz[l] = (py.nz[l - 1] + 1) / 2;
        py.off[l] = tot;
        tot += (long long)py.nx[l] * py.ny[l] * py.nz[l];
    } while ((py.nx[l] > 1 || py.ny[l] > 1 || py.nz[l] > 1) && l < PYR_MAX);
    py.nlev = l;
    SPHX_TRY(sphx_ensure(ctx, ctx->grav_pyr, (size_t)tot * sizeof(double4)));
    SPHX_TRY(sphx_ensure(ctx, ctx->grav_cell, (size_t)n * sizeof(int)));
    double4* pyr = ctx->grav_pyr.as<double4>();
    double4* quad = nullptr;                            // order 2: two more 32-B pieces per cell
    if (ctx->grav_order >= 2) {
        SPHX_TRY(sphx_ensure(ctx, ctx->grav_quad, (size_t)tot * 2 * sizeof(double4)));
        quad = ctx->grav_quad.as<double4>();
    }
    // the frame: the centre of the grid box, brought inside the true bounding box axis by axis - the box of a thin slab is
    // padded to a cell's width, far more than the slab's thickness, whose round-off the cross-slab force needs
    const double bc[3] = {g.xmin + 0.5 * g.nx * g.cell, g.ymin + 0.5 * g.ny * g.cell, g.zmin + 0.5 * g.nz * g.cell};
    double rc[3];
    for (int c = 0; c < 3; ++c) rc[c] = fmin(fmax(bc[c], ctx->tbox_h[c]), ctx->tbox_h[3 + c]);
    ref.x = rc[0]; ref.y = rc[1]; ref.z = rc[2];
    if (about) ref = *about;
    const int n1 = py.nx[1] * py.ny[1] * py.nz[1];
    hipLaunchKernelGGL(pyr_level1_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, ctx->stream, g, py,
                       ctx->cell_start.as<int>(), x, y, z, m, ref, pyr, quad);
    for (int q = 2; q <= py.nlev; ++q) {
        const int nq = py.nx[q] * py.ny[q] * py.nz[q];
        hipLaunchKernelGGL(pyr_up_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, py, q, pyr, quad);
    }
    hipLaunchKernelGGL(sorted_cells_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n,
                       ctx->cell_of.as<int>(), ctx->perm.as<int>(), ctx->grav_cell.as<int>());
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

// the walk over a pyramid grav_pyramid built for these particles
static int grav_tree_walk(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z, const double* m,
                          const Pyr& py, const GravRef& ref, int ws, const double* eps_dev, double eps, double G,
                          const int* omap, double* acc, double* pot = nullptr) {
    const GridParams g = ctx->grid;
    const double4* pyr = ctx->grav_pyr.as<double4>();
    const double4* quad = ctx->grav_order >= 2 ? ctx->grav_quad.as<double4>() : nullptr;
    // (one argument list; pot == NULL: the kernels without the potential)
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n, g, py, ws,
                           ctx->grav_cell.as<int>(), ctx->cell_start.as<int>(), x, y, z, m, pyr, quad, eps_dev, eps, G, ref,
                           ctx->qorder, omap, acc, pot);
    };
    if (ctx->grav_per_thread) {       // SPHX_GRAV_KERNEL=0: the per-thread walk (the wave kernel's reference)
        if (pot) launch(gravity_tree_kernel<true>); else launch(gravity_tree_kernel<false>);
    } else if (quad) {
        if (pot) launch(gravity_tree_wave_kernel<true, true>); else launch(gravity_tree_wave_kernel<true, false>);
    } else {
        if (pot) launch(gravity_tree_wave_kernel<false, true>); else launch(gravity_tree_wave_kernel<false, false>);
    }
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

// Gravity of the particles x,y,z,m held in the cell-sorted order of the CURRENT grid (ctx->grid,
// cell_start, cell_of, perm as sphx_build_grid left them).  acc (n,3) is written at omap[i] (or i).
int sphx_gravity_tree_launch(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z,
                             const double* m, int ws, const double* eps_dev, double eps, double G, const int* omap,
                             double* acc) {
    Pyr py;
    GravRef ref;
    SPHX_TRY(grav_pyramid(ctx, n, x, y, z, m, py, ref));
    return grav_tree_walk(ctx, n, x, y, z, m, py, ref, ws, eps_dev, eps, G, omap, acc);
}

// The array call's route on the device, for a cloud in any order: x, y, z in ctx->in_b, in_c, in_d and the masses in
// ctx->in_h (n each; in_e .. in_g, in_i: sized by the caller) -> a fresh grid over them (k_cells), the cell-sorted copies,
// the pyramid and the walk; acc (n,3) and pot (n) in the caller's order.  pot == NULL: sphx_gravity_tree's launches.
// pot != NULL: the caller has begun ctx->gravpot_t; its stage 2 (grid and pyramid done) is marked here.
// sphx_state_gravity_potential comes through here with the state in id order: hence that call's bits.
static int grav_tree_side(sphx_ctx* ctx, int64_t n, int k_cells, int ws, const double* eps_dev, double eps, double G,
                          double* acc, double* pot) {
    double *x = ctx->in_b.as<double>(), *y = ctx->in_c.as<double>(), *z = ctx->in_d.as<double>();
    double *xs = ctx->in_e.as<double>(), *ys = ctx->in_f.as<double>(), *zs = ctx->in_g.as<double>();
    ctx->map_perm = nullptr;
    ctx->qorder = nullptr;
    ctx->clip_valid = false;
    SPHX_TRY(sphx_build_grid(ctx, n, k_cells, x, y, z, 0.0));
    SPHX_TRY(sphx_gather3(ctx, n, ctx->perm.as<int>(), x, y, z, xs, ys, zs));
    hipLaunchKernelGGL(gather1_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n,
                       ctx->perm.as<int>(), ctx->in_h.as<double>(), ctx->in_i.as<double>());
    Pyr py;
    GravRef ref;
    SPHX_TRY(grav_pyramid(ctx, n, xs, ys, zs, ctx->in_i.as<double>(), py, ref));
    if (pot) SPHX_TRY(ctx->gravpot_t.mark(ctx, 2));
    return grav_tree_walk(ctx, n, xs, ys, zs, ctx->in_i.as<double>(), py, ref, ws, eps_dev, eps, G, ctx->perm.as<int>(), acc, pot);
}
static int grav_tree_side_bufs(sphx_ctx* ctx, size_t nb) {
    DevBuf* bufs[] = {&ctx->in_b, &ctx->in_c, &ctx->in_d, &ctx->in_e, &ctx->in_f, &ctx->in_g, &ctx->in_h, &ctx->in_i};
    for (DevBuf* b : bufs) SPHX_TRY(sphx_ensure(ctx, *b, nb));
    return SPHX_OK;
}

// sphx_gravity_tree (pot == NULL) and sphx_gravity_tree_pot (accel nullable) on host arrays
static int grav_tree_host(sphx_ctx* ctx, const char* who, int64_t n, const double* mass, const double* points,
                          const double* sizes, double softening, double G, int ws, int k_cells, double* accel, double* pot) {
    if (!ctx) return SPHX_E_ARG;
    if (!mass || !points || !(pot || accel)) return sphx_set_err(ctx, SPHX_E_ARG, "%s: NULL argument", who);
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "n=%lld out of range", (long long)n);
    if (ws < 1 || ws > 4) return sphx_set_err(ctx, SPHX_E_ARG, "ws=%d not in 1..4", ws);
    if (!sizes && !(softening >= 0.0)) return sphx_set_err(ctx, SPHX_E_ARG, "softening must be >= 0");
    if (k_cells < 1) k_cells = 40;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nb = (size_t)n * sizeof(double);
    SPHX_TRY(grav_tree_side_bufs(ctx, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->in_a, 3 * nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->out_b, 3 * nb));
    if (pot) {
        SPHX_TRY(sphx_ensure(ctx, ctx->gravpot_buf, nb));
        SPHX_TRY(ctx->gravpot_t.begin(ctx));
    }
    HIPCHK(hipMemcpyAsync(ctx->in_a.p, points, 3 * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->in_h.p, mass, nb, hipMemcpyHostToDevice, ctx->stream));
    SPHX_TRY(sphx_aos_to_soa3(ctx, n, ctx->in_a.as<double>(), ctx->in_b.as<double>(), ctx->in_c.as<double>(),
                              ctx->in_d.as<double>()));
    const double* eps_dev = nullptr;
    if (sizes) {                                   // (in_a is free again: the positions are in in_b .. in_d)
        HIPCHK(hipMemcpyAsync(ctx->in_a.p, sizes, nb, hipMemcpyHostToDevice, ctx->stream));
        double* slot = ctx->scal.as<double>() + SC_GRAV_EPS;
        SPHX_TRY(sphx_median(ctx, n, ctx->in_a.as<double>(), slot));
        eps_dev = slot;
    }
    if (pot) SPHX_TRY(ctx->gravpot_t.mark(ctx, 1));
    SPHX_TRY(grav_tree_side(ctx, n, k_cells, ws, eps_dev, softening, G, accel ? ctx->out_b.as<double>() : nullptr,
                            pot ? ctx->gravpot_buf.as<double>() : nullptr));
    if (pot) SPHX_TRY(ctx->gravpot_t.mark(ctx, 3));
    if (accel) HIPCHK(hipMemcpyAsync(accel, ctx->out_b.p, 3 * nb, hipMemcpyDeviceToHost, ctx->stream));
    if (pot) {
        HIPCHK(hipMemcpyAsync(pot, ctx->gravpot_buf.p, nb, hipMemcpyDeviceToHost, ctx->stream));
        SPHX_TRY(ctx->gravpot_t.mark(ctx, 4));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return pot ? ctx->gravpot_t.end(ctx) : SPHX_OK;
}
extern "C" int sphx_gravity_tree(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                                 const double* sizes, double softening, double G, int ws, int k_cells,
                                 double* accel) {
    if (ctx && !accel) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_gravity_tree: NULL argument");
    return grav_tree_host(ctx, "sphx_gravity_tree", n, mass, points, sizes, softening, G, ws, k_cells, accel, nullptr);
}
extern "C" int sphx_gravity_tree_pot(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                                     const double* sizes, double softening, double G, int ws, double* accel, double* pot) {
    if (ctx && !pot) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_gravity_tree_pot: NULL argument");
    return grav_tree_host(ctx, "sphx_gravity_tree_pot", n, mass, points, sizes, softening, G, ws, 40, accel, pot);
}

// ---- potential and potential energy of the resident state (include/sphx.h: sphx_state_gravity_potential) ----
// The state goes into particle-id order first (the order sphx_state_download hands out), then through the array calls'
// own routes: phi by id is then the array call's bits on the downloaded state in every storage order, and the total is
// an ordered one over the ids.  Buffers of its own and the array calls' staging; the state itself is only read.
// the terms of the totals by id: pp (2, n) = {1/2 m phi, m}; tail[2] = eps, tail[3] = the count of non-finite phi (u64,
// an integer atomic per wave that saw one; zeroed by the caller)
__global__ __launch_bounds__(256) void gravpot_terms_kernel(int n, const double* __restrict__ m, const double* __restrict__ phi,
                                                            const double* __restrict__ eps_ptr, double* __restrict__ pp,
                                                            double* __restrict__ tail) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    double ph = 0.0;
    if (live) {
        const double mi = m[i];
        ph = phi[i];
        pp[i] = 0.5 * mi * ph;
        pp[(size_t)n + i] = mi;
    }
    const u64 bad = __ballot(live && !sphx_finite(ph));
    if ((threadIdx.x & (SPHX_WAVE - 1)) == 0 && bad) atomicAdd((u64*)(tail + 3), (u64)__popcll(bad));
    if (i == 0) tail[2] = *eps_ptr;
}

extern "C" int sphx_state_gravity_potential(sphx_ctx* ctx, double* pot_by_id, double out[4]) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_gravity_potential";
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no state uploaded", who);
    if (!ctx->gravity) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no gravity mode is set (sphx_state_set_gravity)", who);
    NEED(out);
    const int64_t n = ctx->n;
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld out of range", who, (long long)n);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)n, nb = nn * sizeof(double), nchunk = sphx_tot_chunks(n);
    if (ctx->gravity == 1) {
        for (DevBuf* b : {&ctx->in_b, &ctx->in_c, &ctx->in_d, &ctx->in_h}) SPHX_TRY(sphx_ensure(ctx, *b, nb));
    } else {
        SPHX_TRY(grav_tree_side_bufs(ctx, nb));
    }
    // ctx->gravpot_buf: phi by id (n) | pp (2, n) | part (2, nchunk) | tot: U, sum m, eps, bad (4)
    double *phi, *pp, *part, *tot;
    Carve cb;
    cb.take(phi, nn); cb.take(pp, 2 * nn); cb.take(part, 2 * nchunk); cb.take(tot, 4);
    SPHX_TRY(sphx_carve_into(ctx, ctx->gravpot_buf, cb));
    SPHX_TRY(ctx->gravpot_t.begin(ctx));
    const StateArrays& s = ctx->st;
    const int* id = s.id.as<int>();
    double *x = ctx->in_b.as<double>(), *y = ctx->in_c.as<double>(), *z = ctx->in_d.as<double>(), *m = ctx->in_h.as<double>();
    SPHX_TRY(sphx_scatter_rows_by_id(ctx, n, 1, id, s.x.as<double>(), x));
    SPHX_TRY(sphx_scatter_rows_by_id(ctx, n, 1, id, s.y.as<double>(), y));
    SPHX_TRY(sphx_scatter_rows_by_id(ctx, n, 1, id, s.z.as<double>(), z));
    SPHX_TRY(sphx_scatter_rows_by_id(ctx, n, 1, id, s.m.as<double>(), m));
    double* eps = ctx->scal.as<double>() + SC_GRAV_EPS;             // (the step forms its own before it reads the slot)
    SPHX_TRY(sphx_median(ctx, n, s.hprev.as<double>(), eps));
    SPHX_TRY(ctx->gravpot_t.mark(ctx, 1));
    int rc;
    if (ctx->gravity == 1) {
        SPHX_TRY(ctx->gravpot_t.mark(ctx, 2));
        rc = sphx_gravity_pot_launch(ctx, n, x, y, z, 1, m, eps, 0.0, ctx->grav_G, nullptr, nullptr, phi);
    } else {
        // a grid of its own between two steps, as sphx_state_sample builds one: the host side goes back as it was
        const GridHostState saved = sphx_grid_host_save(ctx);
        rc = grav_tree_side(ctx, n, 40, ctx->grav_ws, eps, 0.0, ctx->grav_G, nullptr, phi);
        sphx_grid_host_restore(ctx, saved);
    }
    SPHX_TRY(rc);
    HIPCHK(hipMemsetAsync(tot, 0, 4 * sizeof(double), st));
    hipLaunchKernelGGL(gravpot_terms_kernel, dim3(sphx_blocks(nn, 256)), dim3(256), 0, st, (int)n, m, phi, eps, pp, tot);
    HIPCHK(hipGetLastError());
    SPHX_TRY(sphx_ordered_totals(ctx, n, 2, pp, part, tot));
    SPHX_TRY(ctx->gravpot_t.mark(ctx, 3));
    u64* back = ctx->pinned->census;
    HIPCHK(hipMemcpyAsync(back, tot, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (pot_by_id) HIPCHK(hipMemcpyAsync(pot_by_id, phi, nb, hipMemcpyDeviceToHost, st));
    SPHX_TRY(ctx->gravpot_t.mark(ctx, 4));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(out, back, 3 * sizeof(double));
    out[3] = (double)back[3];
    return ctx->gravpot_t.end(ctx);
}

// =================================================================================================
// Gravity between parts: each part exports its mass to every other part as a flat list of records
// =================================================================================================
// A part (a rank of a decomposed run, a domain of an out-of-core one) holds the pyramid over its own particles.  What a
// peer q may see coarsely is decided cell by cell against Q_q, the bounding box of q's particles:
//   box(c)    the cell's box; on a face of the grid it reaches out to the part's true bounding box (the grid covers
//             mean +- 3 sigma and clamps outliers into its face cells), and ends with the grid where the cell overhangs it
//   accept(c) dist(box(c), Q_q) >= ws * longest edge of box(c)
// A child's box lies inside its parent's, so an accepted parent has accepted children only.  A cell is exported as one
// multipole record iff it is the FIRST accepted cell on the way down from the top cell (the walk from the top makes the
// choice unique whatever rounding does to the rule above); the particles of a level-1 cell with no accepted ancestor and
// not accepted itself travel as {x, y, z, m}.  Every massive particle is therefore in exactly one record, and every
// multipole a target in Q_q receives has ws cell edges of clearance - the guarantee of the single-domain interaction list.
// ws = 0: nothing is accepted, everything travels as particles (the exact form).
// Records are compacted by flag + exclusive scan + write (no atomics): peers in rank order, levels top-down, cells in
// index order; particles by level-1 cell, in storage order.  A cell record is three 32-B pieces {M, centre}, {Sxx Syy Szz
// Sxy}, {Sxz Syz 0 0} (zeros at order 1), its centre relative to a reference point all parts share.
#define GX_CELL_TILE 84                 // cell records staged at a time (3 pieces each: 252 of the tile's 256)
struct GxGeo {
    GridParams g;
    Pyr py;
    long long toff[PYR_MAX + 1];        // first position of level l in top-down order
    long long tot;                      // cells of all levels
    double shift[3];                    // the pyramid's frame - the shared frame
    double ws;                          // 0: never accept
};

// own: the exporter's TRUE bounding box {min xyz, max xyz}
__device__ __forceinline__ bool gx_accept(const GxGeo& e, int l, int X, int Y, int Z, const double* __restrict__ own,
                                          const double* __restrict__ Q) {
    const int idx[3] = {X, Y, Z}, nf[3] = {e.g.nx, e.g.ny, e.g.nz};
    const double org[3] = {e.g.xmin, e.g.ymin, e.g.zmin};
    double side = 0.0, d2 = 0.0;
    for (int c = 0; c < 3; ++c) {
        const long long f0 = (long long)idx[c] << l, f1 = (long long)(idx[c] + 1) << l;
        // (a face cell holds the outliers clamped into it: out to the true box, and no further than the grid inwards)
        const double lo = idx[c] == 0 ? fmin(org[c], own[c]) : org[c] + (double)f0 * e.g.cell;
        const double hi = f1 >= nf[c] ? fmax(org[c] + (double)nf[c] * e.g.cell, own[3 + c]) : org[c] + (double)f1 * e.g.cell;
        side = fmax(side, hi - lo);
        const double gap = fmax(0.0, fmax(Q[c] - hi, lo - Q[3 + c]));
        d2 += gap * gap;
    }
    return sqrt(d2) >= e.ws * side;
}

// position in top-down order -> (level, cell)
__device__ __forceinline__ void gx_locate(const GxGeo& e, long long pos, int& l, int& c) {
    l = e.py.nlev;
    while (l > 1 && pos >= e.toff[l - 1]) --l;
    c = (int)(pos - e.toff[l]);
}

// the level at which the way from the top cell down to cell (l; X, Y, Z) is first accepted; 0: nowhere
__device__ __forceinline__ int gx_first_accepted(const GxGeo& e, int l, int X, int Y, int Z, const double* __restrict__ own,
                                                 const double* __restrict__ Q) {
    if (!(e.ws > 0.0)) return 0;
    for (int L = e.py.nlev; L >= l; --L)
        if (gx_accept(e, L, X >> (L - l), Y >> (L - l), Z >> (L - l), own, Q)) return L;
    return 0;
}

// massive members of level-1 cell (X, Y, Z), visited in storage order
template <class F>
__device__ __forceinline__ void gx_members(const GridParams& g, int X, int Y, int Z, const int* __restrict__ cell_start,
                                           const double* __restrict__ m, F f) {
    const int fx0 = 2 * X, fx1 = min(2 * X + 2, g.nx);
    for (int fz = 2 * Z; fz < min(2 * Z + 2, g.nz); ++fz)
        for (int fy = 2 * Y; fy < min(2 * Y + 2, g.ny); ++fy) {
            const int row = (fz * g.ny + fy) * g.nx;
            const int s = cell_start[row + fx0], en = cell_start[row + fx1];
            for (int j = s; j < en; ++j)
                if (m[j] > 0.0) f(j);
        }
}

// one thread per (peer, cell): cflag = 1 where the cell travels as a record, pcnt = particles a level-1 cell sends
__global__ __launch_bounds__(256) void gx_flag_kernel(GxGeo e, int world, int self, const double* __restrict__ boxes,
                                                      const double4* __restrict__ pyr, const int* __restrict__ cell_start,
                                                      const double* __restrict__ m, int* cflag, int* pcnt) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long)world * e.tot) return;
    const int q = (int)(id / e.tot);
    int l, c;
    gx_locate(e, id - (long long)q * e.tot, l, c);
    const int nxl = e.py.nx[l], nyl = e.py.ny[l];
    const int X = c % nxl, Y = (c / nxl) % nyl, Z = c / (nxl * nyl);
    const double* Q = boxes + 6 * (size_t)q;
    const bool peer = q != self && Q[3] >= Q[0] && Q[4] >= Q[1] && Q[5] >= Q[2];      // (an empty part has hi < lo)
    const bool massive = pyr[e.py.off[l] + c].x > 0.0;
    int first = -1;
    if (peer && massive) first = gx_first_accepted(e, l, X, Y, Z, boxes + 6 * (size_t)self, Q);
    cflag[id] = first == l ? 1 : 0;
    if (l == 1) {
        int cnt = 0;
        if (first == 0) gx_members(e.g, X, Y, Z, cell_start, m, [&](int) { ++cnt; });
        pcnt[(size_t)q * e.toff[0] + c] = cnt;            // (toff[0]: cells of level 1)
    }
}

__global__ __launch_bounds__(256) void gx_write_kernel(GxGeo e, int world, const double4* __restrict__ pyr,
                                                       const double4* __restrict__ quad, const int* __restrict__ cell_start,
                                                       const double* __restrict__ x, const double* __restrict__ y,
                                                       const double* __restrict__ z, const double* __restrict__ m,
                                                       const int* __restrict__ cflag, const int* __restrict__ coff,
                                                       const int* __restrict__ pcnt, const int* __restrict__ poff,
                                                       double4* cells, long long cap_cells, double4* parts,
                                                       long long cap_parts) {
    const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long)world * e.tot) return;
    const int q = (int)(id / e.tot);
    int l, c;
    gx_locate(e, id - (long long)q * e.tot, l, c);
    if (cflag[id] && coff[id] < cap_cells) {
        const size_t cc = (size_t)(e.py.off[l] + c);
        double4 a = pyr[cc];
        a.y += e.shift[0]; a.z += e.shift[1]; a.w += e.shift[2];
        double4* rec = cells + 3 * (size_t)coff[id];
        rec[0] = a;
        rec[1] = quad ? quad[2 * cc] : make_double4(0.0, 0.0, 0.0, 0.0);
        rec[2] = quad ? quad[2 * cc + 1] : make_double4(0.0, 0.0, 0.0, 0.0);
    }
    if (l != 1) return;
    const size_t pc = (size_t)q * e.toff[0] + c;
    if (pcnt[pc] == 0) return;
    const int nxl = e.py.nx[1], nyl = e.py.ny[1];
    long long at = poff[pc];
    gx_members(e.g, c % nxl, (c / nxl) % nyl, c / (nxl * nyl), cell_start, m, [&](int j) {
        if (at < cap_parts) parts[at] = make_double4(x[j], y[j], z[j], m[j]);
        ++at;
    });
}

// counts (world,2): the records each peer is to get, from the scans' ends
__global__ void gx_counts_kernel(int world, long long tot, long long n1, const int* __restrict__ coff,
                                 const int* __restrict__ poff, int* counts) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= world) return;
    counts[2 * q] = coff[(size_t)(q + 1) * tot] - coff[(size_t)q * tot];
    counts[2 * q + 1] = poff[(size_t)(q + 1) * n1] - poff[(size_t)q * n1];
}

// The field of received records on the targets tidx[0..nt) (rows of the AoS array pts), ADDED to acc: one thread per
// target, the records staged through LDS in tiles and read by every lane at once (a broadcast), cells first, then
// particles, each in list order.  Cell centres and the targets are taken relative to ref, particles are differenced directly.
__global__ __launch_bounds__(GRAV_TILE) void gx_remote_kernel(int nt, const int* __restrict__ tidx,
                                                              const double* __restrict__ pts, GravRef ref,
                                                              const double4* __restrict__ cells, int ncells, int order,
                                                              const double4* __restrict__ parts, int nparts,
                                                              const double* eps_ptr, double eps_val, double G, double* acc) {
    __shared__ double4 tile[GRAV_TILE];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const double eps = eps_ptr ? *eps_ptr : eps_val;
    const double e2 = eps * eps;
    const int i = t < nt ? (tidx ? tidx[t] : t) : 0;
    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (t < nt) { xi = pts[3 * (size_t)i]; yi = pts[3 * (size_t)i + 1]; zi = pts[3 * (size_t)i + 2]; }
    const double xr = xi - ref.x, yr = yi - ref.y, zr = zi - ref.z;
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int c0 = 0; c0 < ncells; c0 += GX_CELL_TILE) {
        const int cnt = min(GX_CELL_TILE, ncells - c0);
        __syncthreads();
        if ((int)threadIdx.x < 3 * cnt) tile[threadIdx.x] = cells[3 * (size_t)c0 + threadIdx.x];
        __syncthreads();
        if (order >= 2) {
            for (int k = 0; k < cnt; ++k)
                grav_term_quad(tile[3 * k], tile[3 * k + 1], tile[3 * k + 2], 1.0, xr, yr, zr, e2, ax, ay, az);
        } else {
            for (int k = 0; k < cnt; ++k) {
                const double4 q = tile[3 * k];
                grav_term(q.y, q.z, q.w, q.x, xr, yr, zr, e2, ax, ay, az);
            }
        }
    }
    for (int j0 = 0; j0 < nparts; j0 += GRAV_TILE) {
        const int cnt = min(GRAV_TILE, nparts - j0);
        __syncthreads();
        if ((int)threadIdx.x < cnt) tile[threadIdx.x] = parts[(size_t)j0 + threadIdx.x];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const double4 q = tile[k];
            grav_term(q.x, q.y, q.z, q.w, xi, yi, zi, e2, ax, ay, az);
        }
    }
    if (t < nt) {
        acc[3 * (size_t)i] += G * ax; acc[3 * (size_t)i + 1] += G * ay; acc[3 * (size_t)i + 2] += G * az;
    }
}

// Flags and scans of the export of the part in hand (grid and pyramid current) to `world` peers; counts_dev (world,2).
// boxes_dev (world,6): every part's true bounding box, the exporter's own in row `self`.
static int gx_plan(sphx_ctx* ctx, GxGeo& e, const Pyr& py, const GravRef& ref, const GravRef& shared, int ws, int world,
                   int self, const double* boxes_dev, const double* m_sorted, int* counts_dev) {
    e.g = ctx->grid;
    e.py = py;
    long long at = 0;
    for (int l = py.nlev; l >= 1; --l) { e.toff[l] = at; at += (long long)py.nx[l] * py.ny[l] * py.nz[l]; }
    e.tot = at;
    e.toff[0] = (long long)py.nx[1] * py.ny[1] * py.nz[1];
    e.shift[0] = ref.x - shared.x; e.shift[1] = ref.y - shared.y; e.shift[2] = ref.z - shared.z;
    e.ws = (double)ws;
    const long long nflag = (long long)world * e.tot, npc = (long long)world * e.toff[0];
    if (nflag > 0x7FFFFF00ll)
        return sphx_set_err(ctx, SPHX_E_ARG, "gravity export: %d peers x %lld cells exceed the flag array", world, e.tot);
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_cflag, ((size_t)nflag + 1) * sizeof(int)));
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_coff, ((size_t)nflag + 1) * sizeof(int)));
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_pcnt, ((size_t)npc + 1) * sizeof(int)));
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_poff, ((size_t)npc + 1) * sizeof(int)));
    int *cflag = ctx->gx_cflag.as<int>(), *pcnt = ctx->gx_pcnt.as<int>();
    HIPCHK(hipMemsetAsync(cflag + nflag, 0, sizeof(int), ctx->stream));          // (the scans' closing zero)
    HIPCHK(hipMemsetAsync(pcnt + npc, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(gx_flag_kernel, dim3((unsigned)((nflag + 255) / 256)), dim3(256), 0, ctx->stream, e, world, self,
                       boxes_dev, ctx->grav_pyr.as<double4>(), ctx->cell_start.as<int>(), m_sorted, cflag, pcnt);
    HIPCHK(hipGetLastError());
    SPHX_TRY(sphx_excl_scan_int(ctx, cflag, ctx->gx_coff.as<int>(), (int)nflag));
    SPHX_TRY(sphx_excl_scan_int(ctx, pcnt, ctx->gx_poff.as<int>(), (int)npc));
    hipLaunchKernelGGL(gx_counts_kernel, dim3((unsigned)((world + 63) / 64)), dim3(64), 0, ctx->stream, world, e.tot,
                       e.toff[0], ctx->gx_coff.as<int>(), ctx->gx_poff.as<int>(), counts_dev);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

// ... and the records themselves, peers concatenated; nothing is written beyond the capacities
static int gx_write(sphx_ctx* ctx, const GxGeo& e, int world, const double* xs, const double* ys, const double* zs,
                    const double* m_sorted, double4* cells, long long cap_cells, double4* parts, long long cap_parts) {
    const long long nflag = (long long)world * e.tot;
    hipLaunchKernelGGL(gx_write_kernel, dim3((unsigned)((nflag + 255) / 256)), dim3(256), 0, ctx->stream, e, world,
                       ctx->grav_pyr.as<double4>(), ctx->grav_order >= 2 ? ctx->grav_quad.as<double4>() : nullptr,
                       ctx->cell_start.as<int>(), xs, ys, zs, m_sorted, ctx->gx_cflag.as<int>(), ctx->gx_coff.as<int>(),
                       ctx->gx_pcnt.as<int>(), ctx->gx_poff.as<int>(), cells, cap_cells, parts, cap_parts);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

__global__ __launch_bounds__(256) void gx_gather_part_kernel(int n, const int* __restrict__ ord,
                                                             const double* __restrict__ pts, const double* __restrict__ m,
                                                             double* x, double* y, double* z, double* mo) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const size_t i = (size_t)ord[t];
    x[t] = pts[3 * i]; y[t] = pts[3 * i + 1]; z[t] = pts[3 * i + 2]; mo[t] = m[i];
}
__global__ __launch_bounds__(256) void gx_compose_kernel(int n, const int* __restrict__ ord, const int* __restrict__ perm,
                                                         int* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = ord[perm[t]];
}

extern "C" int sphx_gravity_tree_parts(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                                       const double* sizes, double softening, double G, int ws, int k_cells, int nparts,
                                       const int32_t* part_of, double* accel, int64_t* counts) {
    if (!ctx) return SPHX_E_ARG;
    if (!mass || !points || !accel || !part_of)
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_gravity_tree_parts: NULL argument");
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "n=%lld out of range", (long long)n);
    if (ws < 0 || ws > 4) return sphx_set_err(ctx, SPHX_E_ARG, "ws=%d not in 0..4", ws);
    if (nparts < 1 || nparts > 1024) return sphx_set_err(ctx, SPHX_E_ARG, "nparts=%d not in 1..1024", nparts);
    if (!sizes && !(softening >= 0.0)) return sphx_set_err(ctx, SPHX_E_ARG, "softening must be >= 0");
    if (k_cells < 1) k_cells = 40;
    // ---- the parts on the host: members in caller order, bounding boxes, the shared reference point ----
    std::vector<int64_t> start((size_t)nparts + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (part_of[i] < 0 || part_of[i] >= nparts)
            return sphx_set_err(ctx, SPHX_E_ARG, "part_of[%lld]=%d not in 0..%d", (long long)i, (int)part_of[i], nparts - 1);
        ++start[(size_t)part_of[i] + 1];
    }
    for (int a = 0; a < nparts; ++a) start[a + 1] += start[a];
    std::vector<int> ord((size_t)n);
    std::vector<double> box((size_t)nparts * 6);
    for (int a = 0; a < nparts; ++a)
        for (int c = 0; c < 3; ++c) { box[6 * a + c] = INFINITY; box[6 * a + 3 + c] = -INFINITY; }
    {
        std::vector<int64_t> fill(start.begin(), start.end() - 1);
        for (int64_t i = 0; i < n; ++i) {
            const int a = part_of[i];
            ord[(size_t)fill[a]++] = (int)i;
            for (int c = 0; c < 3; ++c) {
                const double v = points[3 * i + c];
                if (v < box[6 * a + c]) box[6 * a + c] = v;
                if (v > box[6 * a + 3 + c]) box[6 * a + 3 + c] = v;
            }
        }
    }
    GravRef shared;
    {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int a = 0; a < nparts; ++a)
            for (int c = 0; c < 3; ++c) { lo[c] = fmin(lo[c], box[6 * a + c]); hi[c] = fmax(hi[c], box[6 * a + 3 + c]); }
        double mid[3];
        for (int c = 0; c < 3; ++c) mid[c] = (hi[c] >= lo[c]) ? lo[c] + 0.5 * (hi[c] - lo[c]) : 0.0;
        shared.x = mid[0]; shared.y = mid[1]; shared.z = mid[2];
    }
    if (counts) memset(counts, 0, (size_t)nparts * nparts * 2 * sizeof(int64_t));
    HIPCHK(hipSetDevice(ctx->device));
    ctx->map_perm = nullptr;
    ctx->qorder = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_pts, 3 * nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_m, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_ord, (size_t)n * sizeof(int)));
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_map, (size_t)n * sizeof(int)));
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_box, (size_t)nparts * 6 * sizeof(double)));
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_counts, (size_t)nparts * 2 * sizeof(int)));
    SPHX_TRY(sphx_ensure(ctx, ctx->out_b, 3 * nb));
    HIPCHK(hipMemcpyAsync(ctx->gx_pts.p, points, 3 * nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->gx_m.p, mass, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->gx_ord.p, ord.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->gx_box.p, box.data(), box.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const double* eps_dev = nullptr;
    if (sizes) {                                   // eps = median(sizes) over ALL particles, nsc:358
        SPHX_TRY(sphx_ensure(ctx, ctx->in_a, nb));
        HIPCHK(hipMemcpyAsync(ctx->in_a.p, sizes, nb, hipMemcpyHostToDevice, ctx->stream));
        double* slot = ctx->scal.as<double>() + SC_GRAV_EPS;
        SPHX_TRY(sphx_median(ctx, n, ctx->in_a.as<double>(), slot));
        eps_dev = slot;
    }
    int64_t nmax = 0;
    for (int a = 0; a < nparts; ++a) nmax = start[a + 1] - start[a] > nmax ? start[a + 1] - start[a] : nmax;
    DevBuf* bufs[] = {&ctx->in_b, &ctx->in_c, &ctx->in_d, &ctx->in_e, &ctx->in_f, &ctx->in_g, &ctx->in_h, &ctx->in_i};
    for (DevBuf* b : bufs) SPHX_TRY(sphx_ensure(ctx, *b, (size_t)nmax * sizeof(double)));
    double *x = ctx->in_b.as<double>(), *y = ctx->in_c.as<double>(), *z = ctx->in_d.as<double>();
    double *xs = ctx->in_e.as<double>(), *ys = ctx->in_f.as<double>(), *zs = ctx->in_g.as<double>();
    double *mp = ctx->in_h.as<double>(), *ms = ctx->in_i.as<double>();
    double* acc = ctx->out_b.as<double>();
    // ---- every part: its own field, then what it sends to each of the others ----
    std::vector<DevBuf> xc((size_t)nparts), xp((size_t)nparts);        // the parts' exports, kept until all are applied
    std::vector<int> cnt((size_t)nparts * nparts * 2, 0);
    int rc = SPHX_OK;
    auto part = [&](int a) -> int {
        const int64_t na = start[a + 1] - start[a];
        const int* ord_a = ctx->gx_ord.as<int>() + start[a];
        const unsigned gb = (unsigned)((na + 255) / 256);
        hipLaunchKernelGGL(gx_gather_part_kernel, dim3(gb), dim3(256), 0, ctx->stream, (int)na, ord_a,
                           ctx->gx_pts.as<double>(), ctx->gx_m.as<double>(), x, y, z, mp);
        HIPCHK(hipGetLastError());
        ctx->clip_valid = false;
        SPHX_TRY(sphx_build_grid(ctx, na, k_cells, x, y, z, 0.0));
        SPHX_TRY(sphx_gather3(ctx, na, ctx->perm.as<int>(), x, y, z, xs, ys, zs));
        hipLaunchKernelGGL(gather1_kernel, dim3(gb), dim3(256), 0, ctx->stream, (int)na, ctx->perm.as<int>(), mp, ms);
        hipLaunchKernelGGL(gx_compose_kernel, dim3(gb), dim3(256), 0, ctx->stream, (int)na, ord_a, ctx->perm.as<int>(),
                           ctx->gx_map.as<int>());
        HIPCHK(hipGetLastError());
        Pyr py;
        GravRef ref;
        SPHX_TRY(grav_pyramid(ctx, na, xs, ys, zs, ms, py, ref));
        if (ws > 0)
            SPHX_TRY(grav_tree_walk(ctx, na, xs, ys, zs, ms, py, ref, ws, eps_dev, softening, G, ctx->gx_map.as<int>(), acc));
        else
            SPHX_TRY(sphx_gravity_launch(ctx, na, xs, ys, zs, 1, ms, eps_dev, softening, G, ctx->gx_map.as<int>(), acc));
        if (nparts == 1) return SPHX_OK;
        GxGeo e;
        SPHX_TRY(gx_plan(ctx, e, py, ref, shared, ws, nparts, a, ctx->gx_box.as<double>(), ms, ctx->gx_counts.as<int>()));
        int* ca = cnt.data() + (size_t)a * nparts * 2;
        HIPCHK(hipMemcpyAsync(ca, ctx->gx_counts.p, (size_t)nparts * 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        long long tc = 0, tp = 0;
        for (int q = 0; q < nparts; ++q) { tc += ca[2 * q]; tp += ca[2 * q + 1]; }
        SPHX_TRY(sphx_ensure(ctx, xc[a], (size_t)(tc > 0 ? tc : 1) * 3 * sizeof(double4)));
        SPHX_TRY(sphx_ensure(ctx, xp[a], (size_t)(tp > 0 ? tp : 1) * sizeof(double4)));
        return gx_write(ctx, e, nparts, xs, ys, zs, ms, xc[a].as<double4>(), tc, xp[a].as<double4>(), tp);
    };
    for (int a = 0; a < nparts && rc == SPHX_OK; ++a)
        if (start[a + 1] > start[a]) rc = part(a);
    // ---- every part takes the others' records, sources in part order ----
    for (int b = 0; b < nparts && rc == SPHX_OK; ++b) {
        const int64_t nb_ = start[b + 1] - start[b];
        if (nb_ == 0) continue;
        for (int a = 0; a < nparts; ++a) {
            if (a == b || start[a + 1] == start[a]) continue;
            const int* ca = cnt.data() + (size_t)a * nparts * 2;
            long long oc = 0, op = 0;
            for (int q = 0; q < b; ++q) { oc += ca[2 * q]; op += ca[2 * q + 1]; }
            if (ca[2 * b] == 0 && ca[2 * b + 1] == 0) continue;
            hipLaunchKernelGGL(gx_remote_kernel, dim3((unsigned)((nb_ + GRAV_TILE - 1) / GRAV_TILE)), dim3(GRAV_TILE), 0,
                               ctx->stream, (int)nb_, ctx->gx_ord.as<int>() + start[b], ctx->gx_pts.as<double>(), shared,
                               xc[a].as<double4>() + 3 * oc, ca[2 * b], ctx->grav_order, xp[a].as<double4>() + op,
                               ca[2 * b + 1], eps_dev, softening, G, acc);
        }
        if (hipGetLastError() != hipSuccess) rc = sphx_set_err(ctx, SPHX_E_HIP, "sphx_gravity_tree_parts: remote launch failed");
    }
    if (rc == SPHX_OK && hipMemcpyAsync(accel, acc, 3 * nb, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = sphx_set_err(ctx, SPHX_E_HIP, "sphx_gravity_tree_parts: copy of the result failed");
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == SPHX_OK)
        rc = sphx_set_err(ctx, SPHX_E_HIP, "sphx_gravity_tree_parts: synchronise failed");
    for (int a = 0; a < nparts; ++a) { sphx_release(ctx, xc[a]); sphx_release(ctx, xp[a]); }
    if (rc == SPHX_OK && counts)
        for (size_t i = 0; i < cnt.size(); ++i) counts[i] = cnt[i];
    return rc;
}


// =================================================================================================
// The same between the ranks of a decomposed run (device pointers; multigpu.py drives the exchange)
// =================================================================================================
__global__ __launch_bounds__(256) void gx_dev_gather_kernel(int n, int n_owned, const int* __restrict__ perm,
                                                            const double* __restrict__ pos, const double* __restrict__ mass,
                                                            double* xs, double* ys, double* zs, double* ms) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int c = perm[s];
    xs[s] = pos[3 * (size_t)c]; ys[s] = pos[3 * (size_t)c + 1]; zs[s] = pos[3 * (size_t)c + 2];
    ms[s] = c < n_owned ? mass[c] : 0.0;                 // a ghost sits in the grid but belongs to its owner's pyramid
}

static int gx_dev_ready(sphx_ctx* ctx, const char* who) {
    if (!ctx->gx_built || !ctx->map_perm || ctx->n != ctx->gx_n)
        return sphx_set_err(ctx, SPHX_E_STATE, "%s before sphx_dev_gravity_build of the current search", who);
    return SPHX_OK;
}

extern "C" int sphx_dev_gravity_build(sphx_ctx* ctx, int64_t n_total, int64_t n_owned, const double* pos, const double* mass,
                                      const double ref[3]) {
    if (!ctx) return SPHX_E_ARG;
    NEED(pos); NEED(mass); NEED(ref);
    if (!ctx->map_perm || ctx->n != n_total || ctx->map_nactive != n_owned)
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_dev_gravity_build: no sphx_dev_search over %lld particles, %lld owned",
                            (long long)n_total, (long long)n_owned);
    if (!(isfinite(ref[0]) && isfinite(ref[1]) && isfinite(ref[2])))
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_gravity_build: reference point not finite");
    HIPCHK(hipSetDevice(ctx->device));
    ctx->gx_built = false;
    const size_t nb = (size_t)n_total * sizeof(double);
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_pts, 3 * nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->gx_m, nb));
    double* xs = ctx->gx_pts.as<double>();
    hipLaunchKernelGGL(gx_dev_gather_kernel, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, ctx->stream, (int)n_total,
                       (int)n_owned, ctx->map_perm, pos, mass, xs, xs + n_total, xs + 2 * n_total, ctx->gx_m.as<double>());
    HIPCHK(hipGetLastError());
    const GravRef about = {ref[0], ref[1], ref[2]};
    SPHX_TRY(grav_pyramid(ctx, n_total, xs, xs + n_total, xs + 2 * n_total, ctx->gx_m.as<double>(), ctx->gx_py, ctx->gx_ref,
                          &about));
    ctx->gx_built = true;
    ctx->gx_n = n_total;
    ctx->gx_nowned = n_owned;
    return SPHX_OK;
}

extern "C" int sphx_dev_gravity_local(sphx_ctx* ctx, int ws, double G, const double* eps_dev, double eps, double* accel) {
    if (!ctx) return SPHX_E_ARG;
    NEED(accel);
    if (ws < 0 || ws > 4) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_gravity_local: ws=%d not in 0..4", ws);
    if (!eps_dev && !(eps >= 0.0)) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_gravity_local: softening must be >= 0");
    SPHX_TRY(gx_dev_ready(ctx, "sphx_dev_gravity_local"));
    if (ws > 0 && ctx->use_verlet)
        return sphx_set_err(ctx, SPHX_E_STATE, "tree gravity is not combined with incremental search");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->gx_n;
    // the walk writes every particle of the grid, ghosts included, at its caller index: into a buffer of that length,
    // whose owned rows (the first n_owned) are the result
    SPHX_TRY(sphx_ensure(ctx, ctx->grav, 3 * (size_t)n * sizeof(double)));
    const double* xs = ctx->gx_pts.as<double>();
    if (ws > 0)
        SPHX_TRY(grav_tree_walk(ctx, n, xs, xs + n, xs + 2 * n, ctx->gx_m.as<double>(), ctx->gx_py, ctx->gx_ref, ws, eps_dev,
                                eps, G, ctx->map_perm, ctx->grav.as<double>()));
    else
        SPHX_TRY(sphx_gravity_launch(ctx, n, xs, xs + n, xs + 2 * n, 1, ctx->gx_m.as<double>(), eps_dev, eps, G, ctx->map_perm,
                                     ctx->grav.as<double>()));
    if (ctx->gx_nowned > 0)
        HIPCHK(hipMemcpyAsync(accel, ctx->grav.p, 3 * (size_t)ctx->gx_nowned * sizeof(double), hipMemcpyDeviceToDevice,
                              ctx->stream));
    return SPHX_OK;
}

extern "C" int sphx_dev_gravity_export(sphx_ctx* ctx, int world, int rank, const double* boxes, int ws, double* cells,
                                       int64_t cap_cells, double* parts, int64_t cap_parts, int32_t* counts) {
    if (!ctx) return SPHX_E_ARG;
    NEED(boxes); NEED(counts);
    if (world < 1 || world > 1024 || rank < 0 || rank >= world)
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_gravity_export: rank %d of %d", rank, world);
    if (ws < 0 || ws > 4) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_gravity_export: ws=%d not in 0..4", ws);
    if (cap_cells < 0 || cap_parts < 0 || (cap_cells > 0 && !cells) || (cap_parts > 0 && !parts))
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_gravity_export: capacity without a buffer");
    SPHX_TRY(gx_dev_ready(ctx, "sphx_dev_gravity_export"));
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->gx_n;
    const double* xs = ctx->gx_pts.as<double>();
    GxGeo e;
    const GravRef shared = ctx->gx_ref;                  // (the pyramid was built about the shared point: no shift)
    SPHX_TRY(gx_plan(ctx, e, ctx->gx_py, ctx->gx_ref, shared, ws, world, rank, boxes, ctx->gx_m.as<double>(), counts));
    return gx_write(ctx, e, world, xs, xs + n, xs + 2 * n, ctx->gx_m.as<double>(), (double4*)cells, cap_cells, (double4*)parts,
                    cap_parts);
}

extern "C" int sphx_dev_gravity_remote(sphx_ctx* ctx, int64_t n_owned, const double* pos, const double* cells, int64_t ncells,
                                       const double* parts, int64_t nparts, double G, const double* eps_dev, double eps,
                                       double* accel) {
    if (!ctx) return SPHX_E_ARG;
    NEED(pos); NEED(accel);
    if (ncells < 0 || nparts < 0 || ncells > 0x7FFFFFF0ll || nparts > 0x7FFFFFF0ll || (ncells > 0 && !cells) ||
        (nparts > 0 && !parts))
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_gravity_remote: %lld cells, %lld particles", (long long)ncells,
                            (long long)nparts);
    if (!eps_dev && !(eps >= 0.0)) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_gravity_remote: softening must be >= 0");
    SPHX_TRY(gx_dev_ready(ctx, "sphx_dev_gravity_remote"));
    if (n_owned != ctx->gx_nowned)
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dev_gravity_remote: n_owned=%lld, built for %lld", (long long)n_owned,
                            (long long)ctx->gx_nowned);
    HIPCHK(hipSetDevice(ctx->device));
    if (n_owned < 1 || (ncells == 0 && nparts == 0)) return SPHX_OK;
    hipLaunchKernelGGL(gx_remote_kernel, dim3((unsigned)((n_owned + GRAV_TILE - 1) / GRAV_TILE)), dim3(GRAV_TILE), 0,
                       ctx->stream, (int)n_owned, (const int*)nullptr, pos, ctx->gx_ref, (const double4*)cells, (int)ncells,
                       ctx->grav_order, (const double4*)parts, (int)nparts, eps_dev, eps, G, accel);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}
