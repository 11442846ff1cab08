// sphx_rad.hip - the radiative transfer of rad_heating (nsc:922-965): the columns between selected stars and sampled
// gas particles, spread over every non-star particle, and the energy and momentum they deposit.
//
// Both halves are dense triple products (rays x particles, sources x targets x non-star particles), independent of the
// cell grid and of the step's buffers.
//   columns   rays are dealt to lanes, RAD_RPL per lane (a, u, |u|^2 and the sums in registers); the particles are
//             staged tile by tile (RAD_TILE, SoA x y z h^2 w) into LDS, where every lane reads the same address - a
//             broadcast.  A handful of rays would leave the machine empty, so the particle range is split as well:
//             grid = ray tiles x particle chunks, each chunk's sums go to part[chunk][ray] and rad_column_sum adds
//             them in chunk order.  The chunking follows from (n, rays) alone and there is no floating-point atomic:
//             the same inputs give the same bits on every call.
//   deposit   one lane per non-star particle (compacted on the device, caller's order kept).  blocked / star_distance
//             of RAD_SRC_CHUNK sources x RAD_QT targets sits in LDS beside the targets; the target loop is innermost
//             and feeds RAD_SRC_CHUNK sums per weight (gd + 1)^-2.  Then exp, the distance factor and the two sums
//             over the sources, in source order.
// Vector stores from plain C++ only.
#include "sphx_wave.h"
#include "sphx_rad_pair.h"

#define RAD_TILE SPHX_RAD_TILE
#define RAD_WG 128                              // lanes of a column workgroup
#define RAD_RPL 2                               // rays per lane
#define RAD_SRC_CHUNK SPHX_RAD_SRC_CHUNK
#define RAD_QT 128                              // targets staged at a time by the deposit kernel
#define RAD_WG_TARGET 2048                      // column workgroups aimed at (8 per CU)
#define RAD_RED_BLOCKS 256
static_assert(RAD_WG * RAD_RPL == SPHX_RAD_WG_RAYS, "include/sphx.h documents the rays of a workgroup");

// ---- per particle: h^2, the column weight, the non-star flag; min(sizes) over the gas --------------------------------
struct RadPart {
    int n;
    const double *x, *y, *z;                    // SoA positions
    const double *m, *ptype, *sizes, *cross, *mu;      // ptype nullptr: columns alone
    double* h2;
    double* w;
    int* flag;                                  // [n + 1]: ptype != 1, flag[n] = 0
};
__global__ __launch_bounds__(256) void rad_prep_kernel(RadPart a, double amu) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > a.n) return;
    if (i == a.n) { if (a.flag) a.flag[i] = 0; return; }
    const double h = a.sizes[i];
    a.h2[i] = h * h;
    a.w[i] = SPHX_RAD_C2 * (1.0 / (h * h)) * a.cross[i] * a.m[i] / (a.mu[i] * amu);
    if (a.flag) a.flag[i] = (a.ptype[i] != 1.0) ? 1 : 0;
}
// {min sizes over ptype == 0, gas particles met, NaN sizes among them} -> part[block][3], then out[3]
__global__ __launch_bounds__(256) void rad_hmin_kernel(int n, const double* __restrict__ ptype, const double* __restrict__ sizes,
                                                       double* part) {
    __shared__ double sm[4][3];
    double mn = INFINITY, cn = 0.0, nn = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        if (ptype[i] != 0.0) continue;
        const double s = sizes[i];
        cn += 1.0;
        if (s != s) nn += 1.0;
        else if (s < mn) mn = s;
    }
    mn = wave_min_f64(mn); cn = wave_sum_f64(cn); nn = wave_sum_f64(nn);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[wv][0] = mn; sm[wv][1] = cn; sm[wv][2] = nn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = part + 3 * blockIdx.x;
        p[0] = fmin(fmin(sm[0][0], sm[1][0]), fmin(sm[2][0], sm[3][0]));
        p[1] = (sm[0][1] + sm[1][1]) + (sm[2][1] + sm[3][1]);
        p[2] = (sm[0][2] + sm[1][2]) + (sm[2][2] + sm[3][2]);
    }
}
__global__ __launch_bounds__(64) void rad_hmin_final(int nb, const double* part, double* out) {
    double mn = INFINITY, cn = 0.0, nn = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) { mn = fmin(mn, part[3 * b]); cn += part[3 * b + 1]; nn += part[3 * b + 2]; }
    mn = wave_min_f64(mn); cn = wave_sum_f64(cn); nn = wave_sum_f64(nn);
    if (threadIdx.x == 0) { out[0] = mn; out[1] = cn; out[2] = nn; }
}
// the non-star particles, caller's order kept: gidx[off[i]] = i
__global__ __launch_bounds__(256) void rad_compact_kernel(int n, const int* __restrict__ flag, const int* __restrict__ off,
                                                          int* __restrict__ gidx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && flag[i]) gidx[off[i]] = i;
}

// ---- columns ---------------------------------------------------------------------------------------------------------
struct RadColArgs {
    int n;                                      // particles
    const double *x, *y, *z, *h2, *w;
    int n_dst;
    long long R;                                // rays = n_src * n_dst, ray r = s * n_dst + q
    const double *src, *dst;                    // (n_src,3), (n_dst,3)
    int chunk_len;                              // particles per chunk (a multiple of RAD_TILE)
    double* part;                               // [chunks][R]
};
template <bool SEG>
__global__ __launch_bounds__(RAD_WG) void rad_column_kernel(RadColArgs a) {
    __shared__ double sx[RAD_TILE], sy[RAD_TILE], sz[RAD_TILE], sh[RAD_TILE], sw[RAD_TILE];
    const int tid = threadIdx.x;
    double ax[RAD_RPL], ay[RAD_RPL], az[RAD_RPL], ux[RAD_RPL], uy[RAD_RPL], uz[RAD_RPL], uu[RAD_RPL], acc[RAD_RPL];
    bool act[RAD_RPL];
    long long ray[RAD_RPL];
#pragma unroll
    for (int j = 0; j < RAD_RPL; ++j) {
        ray[j] = (long long)blockIdx.x * (RAD_WG * RAD_RPL) + j * RAD_WG + tid;
        act[j] = ray[j] < a.R;
        ax[j] = ay[j] = az[j] = ux[j] = uy[j] = uz[j] = uu[j] = acc[j] = 0.0;
        if (act[j]) {
            const long long s = ray[j] / a.n_dst, q = ray[j] - s * a.n_dst;
            ax[j] = a.src[3 * s]; ay[j] = a.src[3 * s + 1]; az[j] = a.src[3 * s + 2];
            ux[j] = a.dst[3 * q] - ax[j]; uy[j] = a.dst[3 * q + 1] - ay[j]; uz[j] = a.dst[3 * q + 2] - az[j];
            uu[j] = rad_dot(ux[j], uy[j], uz[j], ux[j], uy[j], uz[j]);
        }
    }
    // rays go to lanes in order, so within a wave a second ray implies a first one
    const bool any0 = __builtin_amdgcn_ballot_w64(act[0]) != 0, any1 = __builtin_amdgcn_ballot_w64(act[RAD_RPL - 1]) != 0;
    const long long p0 = (long long)blockIdx.y * a.chunk_len;
    const long long p1 = p0 + a.chunk_len < (long long)a.n ? p0 + a.chunk_len : (long long)a.n;
    for (long long base = p0; base < p1; base += RAD_TILE) {
        const int cnt = (int)(p1 - base < RAD_TILE ? p1 - base : RAD_TILE);
        __syncthreads();
        for (int i = tid; i < cnt; i += RAD_WG) {
            sx[i] = a.x[base + i]; sy[i] = a.y[base + i]; sz[i] = a.z[base + i]; sh[i] = a.h2[base + i]; sw[i] = a.w[base + i];
        }
        __syncthreads();
        if (any1) {
            for (int t = 0; t < cnt; ++t) {
                const double px = sx[t], py = sy[t], pz = sz[t], h2 = sh[t], w = sw[t];
#pragma unroll
                for (int j = 0; j < RAD_RPL; ++j)
                    acc[j] += rad_pair<SEG>(px, py, pz, h2, w, ax[j], ay[j], az[j], ux[j], uy[j], uz[j], uu[j]);
            }
        } else if (any0) {
            for (int t = 0; t < cnt; ++t)
                acc[0] += rad_pair<SEG>(sx[t], sy[t], sz[t], sh[t], sw[t], ax[0], ay[0], az[0], ux[0], uy[0], uz[0], uu[0]);
        }
    }
#pragma unroll
    for (int j = 0; j < RAD_RPL; ++j)
        if (act[j]) a.part[(long long)blockIdx.y * a.R + ray[j]] = acc[j];
}
// blocked = the chunks' sums in chunk order; star_distance = |u| by the reference's operations (nsc:931: squares added
// left to right, no contraction); bs = blocked / star_distance, what the deposit kernel reads
__global__ __launch_bounds__(256) void rad_column_sum(long long R, int chunks, const double* __restrict__ part, int n_dst,
                                                      const double* __restrict__ src, const double* __restrict__ dst,
                                                      double* __restrict__ blocked, double* __restrict__ sd, double* __restrict__ bs) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    double sum = 0.0;
    for (int c = 0; c < chunks; ++c) sum += part[(long long)c * R + r];
    const long long s = r / n_dst, q = r - s * n_dst;
    const double ux = dst[3 * q] - src[3 * s], uy = dst[3 * q + 1] - src[3 * s + 1], uz = dst[3 * q + 2] - src[3 * s + 2];
    const double dist = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy)), __dmul_rn(uz, uz)));
    blocked[r] = sum;
    sd[r] = dist;
    bs[r] = sum / dist;
}

// ---- spread and deposit ------------------------------------------------------------------------------------------------
struct RadDepArgs {
    int ng;                                     // non-star particles
    const int* gidx;                            // their particle indices, caller's order
    const double *x, *y, *z, *w, *m, *sizes;
    int n_src, n_dst;
    const double *src, *dst, *lum;              // (n_src,3), (n_dst,3), luminosities (n_src)
    const double* bs;                           // (n_src,n_dst) blocked / star_distance
    double hmin2;                               // min(sizes over ptype == 0)^2
    double dt, solar_luminosity, c;
    double *lf2, *mom, *ext, *lumf;             // (ng), (ng,3), (ng), (n_src,ng); any may be nullptr
};
__global__ __launch_bounds__(256) void rad_deposit_kernel(RadDepArgs a) {
    __shared__ double sbs[RAD_SRC_CHUNK][RAD_QT];
    __shared__ double sqx[RAD_QT], sqy[RAD_QT], sqz[RAD_QT];
    const int tid = threadIdx.x;
    const int g = blockIdx.x * 256 + tid;
    const bool act = g < a.ng;
    const int p = act ? a.gidx[g] : 0;
    double xg = 0.0, yg = 0.0, zg = 0.0, extg = 0.0, mg = 1.0, aint = 0.0;
    if (act) {
        xg = a.x[p]; yg = a.y[p]; zg = a.z[p]; extg = a.w[p]; mg = a.m[p];
        const double h = a.sizes[p];
        aint = 3.141592653589793 * (h * h);                                                  // nsc:958
    }
    double lf = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
    for (int s0 = 0; s0 < a.n_src; s0 += RAD_SRC_CHUNK) {
        const int ns = a.n_src - s0 < RAD_SRC_CHUNK ? a.n_src - s0 : RAD_SRC_CHUNK;
        double A[RAD_SRC_CHUNK];
#pragma unroll
        for (int si = 0; si < RAD_SRC_CHUNK; ++si) A[si] = 0.0;
        double B = 0.0;
        for (int q0 = 0; q0 < a.n_dst; q0 += RAD_QT) {
            const int nq = a.n_dst - q0 < RAD_QT ? a.n_dst - q0 : RAD_QT;
            __syncthreads();
            for (int i = tid; i < RAD_SRC_CHUNK * RAD_QT; i += 256) {
                const int si = i / RAD_QT, qi = i - si * RAD_QT;
                sbs[si][qi] = (si < ns && qi < nq) ? a.bs[(long long)(s0 + si) * a.n_dst + q0 + qi] : 0.0;
            }
            for (int i = tid; i < nq; i += 256) {
                sqx[i] = a.dst[3 * (long long)(q0 + i)]; sqy[i] = a.dst[3 * (long long)(q0 + i) + 1]; sqz[i] = a.dst[3 * (long long)(q0 + i) + 2];
            }
            __syncthreads();
            for (int qi = 0; qi < nq; ++qi) {
                const double dx = xg - sqx[qi], dy = yg - sqy[qi], dz = zg - sqz[qi];
                const double g1 = sqrt(dx * dx + dy * dy + dz * dz) + 1.0;                    // nsc:941, 949: one metre
                const double wq = 1.0 / (g1 * g1);
                B += wq;
#pragma unroll
                for (int si = 0; si < RAD_SRC_CHUNK; ++si) A[si] += wq * sbs[si][qi];
            }
        }
        if (!act) continue;
#pragma unroll
        for (int si = 0; si < RAD_SRC_CHUNK; ++si) {
            if (si >= ns) continue;                    // (a guard, not a bound: A stays in registers)
            const int s = s0 + si;
            const double rx = xg - a.src[3 * (long long)s], ry = yg - a.src[3 * (long long)s + 1], rz = zg - a.src[3 * (long long)s + 2];
            const double sd2 = sqrt(rx * rx + ry * ry + rz * rz);                            // nsc:944
            const double lumf = sphx_nan_to_num(sd2 * A[si] / B);                            // nsc:949
            if (a.lumf) a.lumf[(long long)s * a.ng + g] = lumf;
            const double sdn = sphx_nan_to_num(sd2);
            const double df = (sdn * sdn + a.hmin2) * 4.0 * 3.141592653589793;               // nsc:957
            const double ell = sphx_nan_to_num(exp(-lumf) / df * a.lum[s] * aint * extg);    // nsc:956, 960-961
            lf += ell;                                                                       // nsc:963
            mx += rx / sd2 * ell; my += ry / sd2 * ell; mz += rz / sd2 * ell;                // nsc:945, 965
        }
    }
    if (!act) return;
    if (a.lf2) a.lf2[g] = lf * a.dt * a.solar_luminosity;
    if (a.mom) {
        a.mom[3 * (long long)g] = mx / mg * a.dt / a.c; a.mom[3 * (long long)g + 1] = my / mg * a.dt / a.c;
        a.mom[3 * (long long)g + 2] = mz / mg * a.dt / a.c;
    }
    if (a.ext) a.ext[g] = extg;                                                              // nsc:954
}

// =====================================================================================================================
// host side
// =====================================================================================================================
static int rad_check(sphx_ctx* ctx, const char* who, int64_t n, int64_t n_src, const void* src, int64_t n_dst, const void* dst,
                     int mode) {
    if (n < 0 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld out of range", who, (long long)n);
    if (n_src < 0 || n_dst < 0 || n_src > (1ll << 24) || n_dst > (1ll << 24) || n_src * n_dst > (1ll << 28))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n_src=%lld, n_dst=%lld out of range", who, (long long)n_src, (long long)n_dst);
    if (n_src > 0 && !src) return sphx_set_err(ctx, SPHX_E_ARG, "%s: argument src is NULL", who);
    if (n_dst > 0 && !dst) return sphx_set_err(ctx, SPHX_E_ARG, "%s: argument dst is NULL", who);
    if (mode != SPHX_RAD_LINE && mode != SPHX_RAD_SEGMENT) return sphx_set_err(ctx, SPHX_E_ARG, "%s: unknown mode %d", who, mode);
    return SPHX_OK;
}

struct RadHostOut { double *lf2, *momentum, *extinction, *blocked, *star_distance, *lum_factor; };

// Device layout of ctx->rad_in (doubles): [0,3n) points AoS (host path) | m | ptype | sizes | cross | mu  (n each)
//                  ctx->rad_soa:          x | y | z | h2 | w (n each)
// The particles' attributes are on the device (RadPart's inputs filled); sources, luminosities and targets come from the host.
// rays_on_device: src and dst are device pointers (the resident radiative phase gathers them by id); t: the stage timer to
// mark, or NULL; dev (nullable): where the deposit's results lie on the device afterwards
static int rad_run(sphx_ctx* ctx, const char* who, RadPart pa, int64_t n_src, const double* src, const double* lum,
                   int64_t n_dst, const double* dst, double dt, int mode, bool transfer, const RadHostOut& ho,
                   bool rays_on_device, StageTimer* t, RadDevOut* dev) {
    const hipMemcpyKind ray_copy = rays_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const int64_t n = pa.n;
    const int64_t R = n_src * n_dst;
    // rays, their outputs, the sources' luminosities: src | dst | lum | blocked | sd | bs
    double *d_src, *d_dst, *d_lum, *d_blocked, *d_sd, *d_bs;
    Carve cr;
    cr.take(d_src, 3 * (size_t)n_src); cr.take(d_dst, 3 * (size_t)n_dst); cr.take(d_lum, (size_t)n_src);
    cr.take(d_blocked, (size_t)R); cr.take(d_sd, (size_t)R); cr.take(d_bs, (size_t)R);
    cr.slack(8 * sizeof(double));
    SPHX_TRY(sphx_carve_into(ctx, ctx->rad_ray, cr));
    if (n_src > 0) HIPCHK(hipMemcpyAsync(d_src, src, (size_t)n_src * 3 * sizeof(double), ray_copy, ctx->stream));
    if (n_dst > 0) HIPCHK(hipMemcpyAsync(d_dst, dst, (size_t)n_dst * 3 * sizeof(double), ray_copy, ctx->stream));
    if (transfer && n_src > 0) HIPCHK(hipMemcpyAsync(d_lum, lum, (size_t)n_src * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    // per particle: flag | off | gidx (n + 1 entries each and four of head-room, on 16-byte boundaries) | the reductions
    int *flag, *off, *gidx;
    double* red;
    Carve cg;
    cg.take(flag, (size_t)n + 5, 16); cg.take(off, (size_t)n + 5, 16); cg.take(gidx, (size_t)n + 5, 16);
    cg.take(red, 16 + 3 * RAD_RED_BLOCKS, 16);
    SPHX_TRY(sphx_carve_into(ctx, ctx->rad_gas, cg));
    pa.flag = transfer ? flag : nullptr;
    hipLaunchKernelGGL(rad_prep_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, ctx->stream, pa, ctx->cst.amu);
    HIPCHK(hipGetLastError());
    int64_t ng = 0;
    double hmin = 0.0;
    if (transfer) {
        int rb = (int)((n + 255) / 256);
        if (rb > RAD_RED_BLOCKS) rb = RAD_RED_BLOCKS;
        if (rb < 1) rb = 1;
        hipLaunchKernelGGL(rad_hmin_kernel, dim3(rb), dim3(256), 0, ctx->stream, (int)n, pa.ptype, pa.sizes, red + 16);
        hipLaunchKernelGGL(rad_hmin_final, dim3(1), dim3(64), 0, ctx->stream, rb, red + 16, red);
        HIPCHK(hipGetLastError());
        SPHX_TRY(sphx_excl_scan_int(ctx, flag, off, (int)n));          // (flag[n] = 0; both start on 16-byte boundaries)
        hipLaunchKernelGGL(rad_compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n, flag, off, gidx);
        HIPCHK(hipGetLastError());
        PinnedSide& pin = ctx->pinned->side;
        HIPCHK(hipMemcpyAsync(pin.red, red, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(&pin.count, off + n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        const double* rd = pin.red;
        ng = pin.count;
        if (!(rd[1] > 0.0))                                // the reference raises on the empty min (nsc:957)
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: no particle with ptypes == 0 (the distance factor needs min(sizes) over them)", who);
        hmin = rd[2] > 0.0 ? NAN : rd[0];                  // (np.min hands a NaN on)
    }
    if (t) SPHX_TRY(t->mark(ctx, 1));
    // columns
    if (R > 0) {
        const int64_t ray_tiles = (R + RAD_WG * RAD_RPL - 1) / (RAD_WG * RAD_RPL);
        const int64_t tiles = (n + RAD_TILE - 1) / RAD_TILE;
        int64_t chunks = (RAD_WG_TARGET + ray_tiles - 1) / ray_tiles;
        if (chunks > tiles) chunks = tiles;
        if (chunks > 65535) chunks = 65535;
        if (chunks < 1) chunks = 1;
        const int64_t chunk_len = ((tiles + chunks - 1) / chunks) * RAD_TILE;
        chunks = n > 0 ? (n + chunk_len - 1) / chunk_len : 1;
        SPHX_TRY(sphx_ensure(ctx, ctx->rad_part, (size_t)chunks * (size_t)R * sizeof(double)));
        RadColArgs ca;
        ca.n = (int)n; ca.x = pa.x; ca.y = pa.y; ca.z = pa.z; ca.h2 = pa.h2; ca.w = pa.w;
        ca.n_dst = (int)n_dst; ca.R = R; ca.src = d_src; ca.dst = d_dst;
        ca.chunk_len = (int)(chunk_len > 0 ? chunk_len : RAD_TILE);
        ca.part = ctx->rad_part.as<double>();
        const dim3 grid((unsigned)ray_tiles, (unsigned)chunks);
        if (mode == SPHX_RAD_SEGMENT) hipLaunchKernelGGL(rad_column_kernel<true>, grid, dim3(RAD_WG), 0, ctx->stream, ca);
        else hipLaunchKernelGGL(rad_column_kernel<false>, grid, dim3(RAD_WG), 0, ctx->stream, ca);
        hipLaunchKernelGGL(rad_column_sum, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, ctx->stream, (long long)R, (int)chunks,
                           ca.part, (int)n_dst, d_src, d_dst, d_blocked, d_sd, d_bs);
        HIPCHK(hipGetLastError());
    }
    if (t) SPHX_TRY(t->mark(ctx, 2));
    // spread and deposit: lf2 | ext | momentum (3) | lum_factor (n_src)
    double *o_lf2 = nullptr, *o_ext = nullptr, *o_mom = nullptr, *o_lumf = nullptr;
    if (transfer && ng > 0) {
        const bool want_lumf = ho.lum_factor != nullptr;
        Carve co;
        co.take(o_lf2, (size_t)ng); co.take(o_ext, (size_t)ng); co.take(o_mom, 3 * (size_t)ng);
        if (want_lumf) co.take(o_lumf, (size_t)n_src * (size_t)ng);
        SPHX_TRY(sphx_carve_into(ctx, ctx->rad_out, co));
        RadDepArgs da;
        da.ng = (int)ng; da.gidx = gidx;
        da.x = pa.x; da.y = pa.y; da.z = pa.z; da.w = pa.w; da.m = pa.m; da.sizes = pa.sizes;
        da.n_src = (int)n_src; da.n_dst = (int)n_dst; da.src = d_src; da.dst = d_dst; da.lum = d_lum; da.bs = d_bs;
        da.hmin2 = hmin * hmin; da.dt = dt; da.solar_luminosity = ctx->cst.solar_luminosity; da.c = ctx->cst.c;
        da.lf2 = o_lf2; da.mom = o_mom; da.ext = o_ext; da.lumf = o_lumf;
        hipLaunchKernelGGL(rad_deposit_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, ctx->stream, da);
        HIPCHK(hipGetLastError());
    }
    if (t) SPHX_TRY(t->mark(ctx, 3));
    const CopyF64 ps[] = {{ho.blocked, d_blocked, (size_t)R}, {ho.star_distance, d_sd, (size_t)R}, {ho.lf2, o_lf2, (size_t)ng},
                          {ho.extinction, o_ext, (size_t)ng}, {ho.momentum, o_mom, 3 * (size_t)ng},
                          {ho.lum_factor, o_lumf, (size_t)n_src * (size_t)ng}};
    SPHX_TRY(sphx_download_f64(ctx, ps, 6));
    if (t) SPHX_TRY(t->mark(ctx, 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (dev) { dev->lf2 = o_lf2; dev->ext = o_ext; dev->mom = o_mom; dev->ng = ng; }
    return t ? t->end(ctx) : SPHX_OK;
}

// the two buffers of the particles' attributes, nn doubles an array
struct RadIn { double *points, *m, *ptype, *sizes, *cross, *mu; };
struct RadSoa { double *x, *y, *z, *h2, *w; };
static int rad_in_carve(sphx_ctx* ctx, size_t nn, RadIn* in) {
    Carve c;
    c.take(in->points, 3 * nn); c.take(in->m, nn); c.take(in->ptype, nn); c.take(in->sizes, nn); c.take(in->cross, nn); c.take(in->mu, nn);
    return sphx_carve_into(ctx, ctx->rad_in, c);
}
static int rad_soa_carve(sphx_ctx* ctx, size_t nn, RadSoa* soa) {
    Carve c;
    c.take(soa->x, nn); c.take(soa->y, nn); c.take(soa->z, nn); c.take(soa->h2, nn); c.take(soa->w, nn);
    return sphx_carve_into(ctx, ctx->rad_soa, c);
}
static RadPart rad_part(int64_t n, const RadIn& in, const RadSoa& soa) {
    RadPart pa;
    pa.n = (int)n;
    pa.x = soa.x; pa.y = soa.y; pa.z = soa.z; pa.h2 = soa.h2; pa.w = soa.w;
    pa.m = in.m; pa.ptype = in.ptype; pa.sizes = in.sizes; pa.cross = in.cross; pa.mu = in.mu;
    pa.flag = nullptr;
    return pa;
}

// host arrays -> ctx->rad_in / rad_soa; fills pa's inputs and outputs (ptype may be NULL)
static int rad_stage_host(sphx_ctx* ctx, int64_t n, const double* points, const double* ptype, const double* mass,
                          const double* sizes, const double* cross, const double* mu, RadPart* pa) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    RadIn in;
    RadSoa soa;
    SPHX_TRY(rad_in_carve(ctx, nn, &in));
    SPHX_TRY(rad_soa_carve(ctx, nn, &soa));
    const size_t nd = (size_t)n;
    const CopyF64 us[] = {{points, in.points, 3 * nd}, {mass, in.m, nd}, {ptype, in.ptype, nd}, {sizes, in.sizes, nd},
                          {cross, in.cross, nd}, {mu, in.mu, nd}};
    if (n > 0) {
        SPHX_TRY(sphx_upload_f64(ctx, us, 6));
        SPHX_TRY(sphx_aos_to_soa3(ctx, n, in.points, soa.x, soa.y, soa.z));
    }
    *pa = rad_part(n, in, soa);
    if (!ptype) pa->ptype = nullptr;
    return SPHX_OK;
}

extern "C" int sphx_rad_columns(sphx_ctx* ctx, int64_t n, const double* points, const double* sizes, const double* mass,
                                const double* mu, const double* cross, int64_t n_src, const double* src, int64_t n_dst,
                                const double* dst, int mode, double* blocked, double* star_distance) {
    if (!ctx) return SPHX_E_ARG;
    SPHX_TRY(rad_check(ctx, "sphx_rad_columns", n, n_src, src, n_dst, dst, mode));
    if (n > 0) { NEED(points); NEED(sizes); NEED(mass); NEED(mu); NEED(cross); }
    if (n_src * n_dst == 0) return SPHX_OK;
    NEED(blocked);
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->rad_t.begin(ctx));
    RadPart pa;
    SPHX_TRY(rad_stage_host(ctx, n, points, nullptr, mass, sizes, cross, mu, &pa));
    const RadHostOut ho{nullptr, nullptr, nullptr, blocked, star_distance, nullptr};
    return rad_run(ctx, "sphx_rad_columns", pa, n_src, src, nullptr, n_dst, dst, 0.0, mode, false, ho, false, &ctx->rad_t, nullptr);
}

extern "C" int sphx_rad_transfer(sphx_ctx* ctx, int64_t n, const double* points, const double* ptypes, const double* mass,
                                 const double* sizes, const double* cross, const double* mu, int64_t n_src, const double* src,
                                 const double* luminosities, int64_t n_dst, const double* dst, double dt, int mode, double* lf2,
                                 double* momentum, double* extinction, double* blocked, double* star_distance,
                                 double* lum_factor) {
    if (!ctx) return SPHX_E_ARG;
    SPHX_TRY(rad_check(ctx, "sphx_rad_transfer", n, n_src, src, n_dst, dst, mode));
    if (n_src > 0) NEED(luminosities);
    if (n < 1) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_rad_transfer: no particle with ptypes == 0 (n = 0)");
    NEED(points); NEED(ptypes); NEED(mass); NEED(sizes); NEED(cross); NEED(mu);
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->rad_t.begin(ctx));
    RadPart pa;
    SPHX_TRY(rad_stage_host(ctx, n, points, ptypes, mass, sizes, cross, mu, &pa));
    const RadHostOut ho{lf2, momentum, extinction, blocked, star_distance, lum_factor};
    return rad_run(ctx, "sphx_rad_transfer", pa, n_src, src, luminosities, n_dst, dst, dt, mode, true, ho, false, &ctx->rad_t, nullptr);
}

// The same on the step loop's resident state.  Everything is read into buffers of this file's own, in the caller's
// particle order (the order the sums then run in: the bits are those of sphx_rad_transfer on the downloaded state);
// nothing the step owns is written, and the one host-side field of the context that changes is the epoch counter of the
// single-launch scan (lbs_epoch, which every scan bumps - as sphx_state_sample always has), so the loop goes on undisturbed.
extern "C" int sphx_state_rad_transfer(sphx_ctx* ctx, const double* cross, int64_t n_src, const double* src,
                                       const double* luminosities, int64_t n_dst, const double* dst, double dt, int mode,
                                       double* lf2, double* momentum, double* extinction, double* blocked,
                                       double* star_distance, double* lum_factor) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_rad_transfer: no state uploaded");
    if (ctx->step_count < 1)
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_rad_transfer before the first sphx_step: sizes do not exist yet");
    const int64_t n = ctx->n;
    SPHX_TRY(rad_check(ctx, "sphx_state_rad_transfer", n, n_src, src, n_dst, dst, mode));
    NEED(cross);
    if (n_src > 0) NEED(luminosities);
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->rad_t.begin(ctx));
    const size_t nn = (size_t)n;
    RadIn in;
    RadSoa soa;
    SPHX_TRY(rad_in_carve(ctx, nn, &in));
    SPHX_TRY(rad_soa_carve(ctx, nn, &soa));
    HIPCHK(hipMemcpyAsync(in.cross, cross, nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const StateArrays& s = ctx->st;
    // the resident state (storage order) into the caller's order: the SoA positions, m, ptype, hprev, mu (slot by slot: no
    // list is read here, so no processing order and no col)
    PhaseGather ga = {};
    ga.n = (int)n; ga.id = s.id.as<int>();
    ga.x = s.x.as<double>(); ga.y = s.y.as<double>(); ga.z = s.z.as<double>();
    ga.m = s.m.as<double>(); ga.pt = s.ptype.as<double>(); ga.h = sphx_phase_sizes(ctx); ga.mu = s.mu.as<double>();
    ga.sx = soa.x; ga.sy = soa.y; ga.sz = soa.z; ga.om = in.m; ga.opt = in.ptype; ga.oh = in.sizes; ga.omu = in.mu;
    SPHX_TRY(sphx_phase_gather(ctx, ga));
    const RadPart pa = rad_part(n, in, soa);
    const RadHostOut ho{lf2, momentum, extinction, blocked, star_distance, lum_factor};
    return rad_run(ctx, "sphx_state_rad_transfer", pa, n_src, src, luminosities, n_dst, dst, dt, mode, true, ho, false, &ctx->rad_t, nullptr);
}

// nsc:922-965 on particle attributes that are on the device already, in the caller's particle order (the resident
// radiative phase, sphx_phase.hip): x, y, z SoA; src and dst device pointers; lum on the host.  No timer of this family
// is touched.  The same kernels on the same values as sphx_rad_transfer: the same bits.
int sphx_rad_run_dev(sphx_ctx* ctx, const char* who, int64_t n, const double* x, const double* y, const double* z, const double* m,
                     const double* ptype, const double* sizes, const double* cross, const double* mu, int64_t n_src,
                     const double* src_dev, const double* lum_host, int64_t n_dst, const double* dst_dev, double dt, int mode,
                     RadDevOut* out) {
    SPHX_TRY(rad_check(ctx, who, n, n_src, src_dev, n_dst, dst_dev, mode));
    RadSoa soa;                                      // (h2 and w alone: the positions are the caller's)
    SPHX_TRY(rad_soa_carve(ctx, (size_t)n, &soa));
    RadPart pa;
    pa.n = (int)n;
    pa.x = x; pa.y = y; pa.z = z; pa.h2 = soa.h2; pa.w = soa.w;
    pa.m = m; pa.ptype = ptype; pa.sizes = sizes; pa.cross = cross; pa.mu = mu;
    pa.flag = nullptr;
    const RadHostOut ho{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return rad_run(ctx, who, pa, n_src, src_dev, lum_host, n_dst, dst_dev, dt, mode, true, ho, true, nullptr, out);
}
