// sphx_sn.hip - supernova_impulse (nsc:1192-1204) as an array call: per exploding star the nearest gas rows whose running
// mass stays below mass_displaced, and their radial kick.  include/sphx.h has the definition; here the route to it:
//   keys      the squared distance of every row to the star as a 64-bit key (the bits of a non-negative double order as
//             unsigned integers; NaN is the largest key)
//   bound     a key that no selected row exceeds, from histograms over eight key bits a level: per bin the gas rows and
//             their mass in integer fixed point (integer atomics: the same bound on every run), refined inside the bin
//             where the mass crosses mass_displaced until the rows under the bound fit one LDS sort
//   compact   the gas rows under the bound as (key, id), in whatever order the atomics give
//   sort      by (key, id) - a total order, which removes that order and IS the tie rule - in one workgroup's LDS where
//             they fit, by a bitonic network in global memory otherwise
//   walk      one wave adds the masses left to right and stops at the first running sum that is not < mass_displaced;
//             it tells whether it stopped before the candidates ran out: if not, and rows were left out, the bound is
//             widened to "every gas row" and the star is done again (only masses that are not positive and
//             finite can cause it)
//   kick      true_mass by sphx_ordered_totals over the selection in sorted order, vel, d_vels, the velocities
// No floating-point atomic anywhere.
#include "sphx_internal.h"
#include "sphx_phase_map.h"
#include <limits.h>
#pragma clang fp contract(off)

#define SN_WG 256
#define SN_SORT_WG 1024
#define SN_BINS 256
static_assert(SN_BINS == SN_WG, "sn_hist_kernel: a lane per bin");
#define SN_W1 4294967296.0                 // the fixed-point weight of mass_displaced: 2^32 (n < 2^31 rows cannot overflow 64 bits)
#define SN_TARGET ((1ull << 32) + (1ull << 12))
static_assert(SPHX_SN_LDS_CAP == 4096, "sn_sort_lds_kernel's arrays");
// device scalars (u64) behind the two histograms
enum { SNS_CURSOR = 0, SNS_BAD_MASS = 1, SNS_ZERO = 2, SNS_NSEL = 3, SNS_CROSSED = 4, SNS_CT = 5, SNS_N = 8 };   // (SNS_CT: the event's crossing time)

__device__ __forceinline__ bool sn_is_gas(double t) { return t == 0.0; }
__device__ __forceinline__ bool sn_good_mass(double m) { return m > 0.0 && sphx_finite(m); }
// the weight of a row's mass, rounded DOWN (so the weights never claim more mass than there is); NaN stops the walk
// where it stands (NaN < M is false), so it weighs as much as mass_displaced itself
__device__ __forceinline__ u64 sn_weight(double m, double M) {
    if (m != m) return (u64)SN_W1;
    if (!(m > 0.0)) return 0ull;
    const double t = m / M * SN_W1;
    return t >= SN_W1 ? (u64)SN_W1 : (u64)t;
}

// nsc:1194: s = (dx^2 + dy^2) + dz^2, NumPy's order over the three columns
__device__ __forceinline__ double sn_dist2(const double* __restrict__ pos, int i, double sx, double sy, double sz, double& dx,
                                           double& dy, double& dz) {
    dx = pos[3 * (size_t)i] - sx; dy = pos[3 * (size_t)i + 1] - sy; dz = pos[3 * (size_t)i + 2] - sz;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(SN_WG) void sn_key_kernel(int n, const double* __restrict__ pos, int ku, u64* __restrict__ key) {
    const int i = blockIdx.x * SN_WG + threadIdx.x;
    if (i >= n) return;
    double dx, dy, dz;
    const double s = sn_dist2(pos, i, pos[3 * (size_t)ku], pos[3 * (size_t)ku + 1], pos[3 * (size_t)ku + 2], dx, dy, dz);
    key[i] = s != s ? ~0ull : (u64)__double_as_longlong(s);
}

// the gas rows whose key agrees with `prefix` under `mask`, by the eight bits at `shift`: hist[bin] mass, hist[SN_BINS + bin] rows
__global__ __launch_bounds__(SN_WG) void sn_hist_kernel(int n, const u64* __restrict__ key, const double* __restrict__ ptype,
                                                        const double* __restrict__ mass, double M, u64 prefix, u64 mask, int shift,
                                                        u64* __restrict__ hist) {
    __shared__ u64 hw[SN_BINS];
    __shared__ unsigned hc[SN_BINS];
    hw[threadIdx.x] = 0ull; hc[threadIdx.x] = 0u;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * SN_WG + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * SN_WG) {
        const u64 kk = key[i];
        if (!sn_is_gas(ptype[i]) || (kk & mask) != prefix) continue;
        const int bin = (int)((kk >> shift) & (SN_BINS - 1));
        const u64 w = sn_weight(mass[i], M);
        if (w) atomicAdd(&hw[bin], w);
        atomicAdd(&hc[bin], 1u);
    }
    __syncthreads();
    if (hc[threadIdx.x]) {
        if (hw[threadIdx.x]) atomicAdd(&hist[threadIdx.x], hw[threadIdx.x]);
        atomicAdd(&hist[SN_BINS + threadIdx.x], (u64)hc[threadIdx.x]);
    }
}

// the gas rows with key <= bound into (ckey, cid), P slots of which the rest holds the sentinel (largest key, largest id)
__global__ __launch_bounds__(SN_WG) void sn_pad_kernel(int P, u64* __restrict__ ckey, int* __restrict__ cid) {
    const int i = blockIdx.x * SN_WG + threadIdx.x;
    if (i < P) { ckey[i] = ~0ull; cid[i] = INT_MAX; }
}
__global__ __launch_bounds__(SN_WG) void sn_compact_kernel(int n, const u64* __restrict__ key, const double* __restrict__ ptype,
                                                           const double* __restrict__ mass, u64 bound, int P, u64* __restrict__ ckey,
                                                           int* __restrict__ cid, u64* __restrict__ scal) {
    const int i = blockIdx.x * SN_WG + threadIdx.x;
    if (i >= n) return;
    const u64 kk = key[i];
    if (!sn_is_gas(ptype[i]) || kk > bound) return;
    const u64 slot = atomicAdd(&scal[SNS_CURSOR], 1ull);
    if (slot < (u64)P) { ckey[slot] = kk; cid[slot] = i; }
    if (!sn_good_mass(mass[i])) atomicAdd(&scal[SNS_BAD_MASS], 1ull);
}

// one compare-exchange of the bitonic network on (key, id), by the lower lane of the pair
__device__ __forceinline__ void sn_cmpx(u64* key, int* id, int i, int j, int k) {
    const int l = i ^ j;
    if (l <= i) return;
    const u64 ka = key[i], kb = key[l];
    const int ia = id[i], ib = id[l];
    const bool gt = ka > kb || (ka == kb && ia > ib);
    if (gt == ((i & k) == 0)) { key[i] = kb; key[l] = ka; id[i] = ib; id[l] = ia; }
}
// P <= SPHX_SN_LDS_CAP, a power of two: the whole network in one workgroup's LDS
__global__ __launch_bounds__(SN_SORT_WG) void sn_sort_lds_kernel(int P, u64* __restrict__ ckey, int* __restrict__ cid) {
    __shared__ u64 sk[SPHX_SN_LDS_CAP];
    __shared__ int si[SPHX_SN_LDS_CAP];
    for (int i = threadIdx.x; i < P; i += SN_SORT_WG) { sk[i] = ckey[i]; si[i] = cid[i]; }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += SN_SORT_WG) sn_cmpx(sk, si, i, j, k);
            __syncthreads();
        }
    for (int i = threadIdx.x; i < P; i += SN_SORT_WG) { ckey[i] = sk[i]; cid[i] = si[i]; }
}
// ... and one step (j, k) of it in global memory
__global__ __launch_bounds__(SN_WG) void sn_sort_step_kernel(int P, int j, int k, u64* __restrict__ ckey, int* __restrict__ cid) {
    const int i = blockIdx.x * SN_WG + threadIdx.x;
    if (i < P) sn_cmpx(ckey, cid, i, j, k);
}

// lane j's value to every lane, j the same in all of them (two register reads; a shuffle would go through the LDS)
__device__ __forceinline__ double sn_lane_value(double v, int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}
// One wave: the running sum of nsc:1197's np.cumsum, left to right over the c sorted candidates, every lane the same
// chain, lane j keeping the sum up to row j of the 64 in hand, a ballot finding the first that is not < M; selected while
// running < M.  scal[SNS_NSEL]: the rows selected; scal[SNS_CROSSED]: 1 when a row stopped it.
__global__ __launch_bounds__(SPHX_WAVE) void sn_walk_kernel(int c, const double* __restrict__ cm, double M, u64* __restrict__ scal) {
    const int lane = threadIdx.x;
    double running = 0.0;
    int nsel = 0, crossed = 0;
    double next = lane < c ? cm[lane] : 0.0;
    for (int base = 0; base < c && !crossed; base += SPHX_WAVE) {
        const int cnt = min(SPHX_WAVE, c - base), ahead = base + SPHX_WAVE + lane;
        const double m = next;
        next = ahead < c ? cm[ahead] : 0.0;                  // (the next 64 masses are on their way during the chain)
        double mine = 0.0;                                   // the running sum up to and with this lane's row
#pragma unroll
        for (int j = 0; j < SPHX_WAVE; ++j) {                // (no branch in the chain; the lanes past cnt hold 0)
            running += sn_lane_value(m, j);
            mine = lane == j ? running : mine;
        }
        const u64 stops = __ballot(lane < cnt && !(mine < M));
        crossed = stops != 0ull;
        nsel = base + (crossed ? __ffsll((long long)stops) - 1 : cnt);
    }
    if (lane == 0) { scal[SNS_NSEL] = (u64)nsel; scal[SNS_CROSSED] = (u64)crossed; }
}

// the sorted candidates' masses side by side: what the walk adds up and, its first n_sel entries, what true_mass sums
__global__ __launch_bounds__(SN_WG) void sn_candmass_kernel(int n, int c, const int* __restrict__ cid, const double* __restrict__ mass,
                                                            double* __restrict__ cm) {
    const int j = blockIdx.x * SN_WG + threadIdx.x;
    if (j >= c) return;
    const int id = cid[j];
    cm[j] = id < n ? mass[id] : 0.0;                         // (a sentinel among the c rows: the caller refuses, sn_select)
}
// nsc:1200: vel = (2 supernova_energy 0.736 / true_mass)^0.5, kick_energy = supernova_energy 0.736 (2 x is exact, so the
// reference's (2 E) 0.736 and 2 (E 0.736) are the same double)
__global__ void sn_vel_kernel(const double* __restrict__ tot, double kick_energy, double* __restrict__ true_mass, double* __restrict__ vel) {
    const double tm = tot[0];
    *true_mass = tm;
    *vel = sqrt(2.0 * kick_energy / tm);
}
// nsc:1201: d_vels = (dx / sqrt(s)) vel per component; drv:351-352: velocities[selected] += d_vels
__global__ __launch_bounds__(SN_WG) void sn_kick_kernel(int nsel, const int* __restrict__ cid, const double* __restrict__ pos, int ku,
                                                        const double* __restrict__ vel_dev, long long* __restrict__ sel_ids,
                                                        double* __restrict__ d_vels, double* __restrict__ velocities,
                                                        u64* __restrict__ scal) {
    const int j = blockIdx.x * SN_WG + threadIdx.x;
    if (j >= nsel) return;
    const int i = cid[j];
    double dx, dy, dz;
    const double s = sn_dist2(pos, i, pos[3 * (size_t)ku], pos[3 * (size_t)ku + 1], pos[3 * (size_t)ku + 2], dx, dy, dz);
    const double r = sqrt(s), vel = *vel_dev;
    const double kx = dx / r * vel, ky = dy / r * vel, kz = dz / r * vel;
    sel_ids[j] = i;
    d_vels[3 * (size_t)j] = kx; d_vels[3 * (size_t)j + 1] = ky; d_vels[3 * (size_t)j + 2] = kz;
    if (velocities) {
        velocities[3 * (size_t)i] += kx; velocities[3 * (size_t)i + 1] += ky; velocities[3 * (size_t)i + 2] += kz;
    }
    if (s == 0.0) atomicAdd(&scal[SNS_ZERO], 1ull);
}

// =====================================================================================================================
// host side
// =====================================================================================================================
static int sn_pow2(int64_t c) {
    int64_t p = 64;
    while (p < c) p <<= 1;
    return (int)p;
}
static int sn_mark(sphx_ctx* ctx, int i) {
    HIPCHK(hipEventRecord(ctx->sn_ev[i], ctx->stream));
    return SPHX_OK;
}

// The gas rows with key <= bound, sorted by (key, id), and the walk over them: c candidates, nsel selected, crossed.
static int sn_select(sphx_ctx* ctx, const char* who, int64_t n, const double* mass, const double* ptype, double M, u64 bound, int64_t c, u64* key, u64* scal,
                     int64_t* nsel, bool* crossed, double** cm_out, int** cid_out) {
    hipStream_t st = ctx->stream;
    const int P = sn_pow2(c);
    u64* ckey;
    double* cm;
    int* cid;
    Carve cc;
    cc.take(ckey, (size_t)P); cc.take(cm, (size_t)P); cc.take(cid, (size_t)P);      // keys | masses | ids
    SPHX_TRY(sphx_carve_into(ctx, ctx->sn_cand, cc));
    HIPCHK(hipMemsetAsync(scal + SNS_CURSOR, 0, sizeof(u64), st));
    hipLaunchKernelGGL(sn_pad_kernel, dim3(sphx_blocks((size_t)P, SN_WG)), dim3(SN_WG), 0, st, P, ckey, cid);
    hipLaunchKernelGGL(sn_compact_kernel, dim3(sphx_blocks((size_t)n, SN_WG)), dim3(SN_WG), 0, st, (int)n, key, ptype, mass, bound, P, ckey, cid,
                       scal);
    HIPCHK(hipGetLastError());
    SPHX_TRY(sn_mark(ctx, 3));
    if (P <= SPHX_SN_LDS_CAP) {
        hipLaunchKernelGGL(sn_sort_lds_kernel, dim3(1), dim3(SN_SORT_WG), 0, st, P, ckey, cid);
        ++ctx->sn_counts[SPHX_SN_LDS_SORTS];
    } else {
        for (int k = 2; k <= P && k > 0; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1)
                hipLaunchKernelGGL(sn_sort_step_kernel, dim3(sphx_blocks((size_t)P, SN_WG)), dim3(SN_WG), 0, st, P, j, k, ckey, cid);
        ++ctx->sn_counts[SPHX_SN_GLOBAL_SORTS];
    }
    HIPCHK(hipGetLastError());
    SPHX_TRY(sn_mark(ctx, 4));
    if (c > 0) hipLaunchKernelGGL(sn_candmass_kernel, dim3(sphx_blocks((size_t)c, SN_WG)), dim3(SN_WG), 0, st, (int)n, (int)c, cid, mass, cm);
    hipLaunchKernelGGL(sn_walk_kernel, dim3(1), dim3(SPHX_WAVE), 0, st, (int)c, cm, M, scal);
    HIPCHK(hipGetLastError());
    u64 back[SNS_N];
    HIPCHK(hipMemcpyAsync(back, scal, sizeof(back), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if ((int64_t)back[SNS_CURSOR] != c)
        return sphx_set_err(ctx, SPHX_E_HIP, "%s: %llu rows under the bound, the histograms counted %lld", who,
                            (unsigned long long)back[SNS_CURSOR], (long long)c);
    ctx->sn_counts[SPHX_SN_CANDIDATES] += c;
    *nsel = (int64_t)back[SNS_NSEL]; *crossed = back[SNS_CROSSED] != 0;
    *cm_out = cm; *cid_out = cid;
    return SPHX_OK;
}

// The bound of one star from the histograms: *bound, the c rows under it, the n_gas gas rows there are.
static int sn_bound(sphx_ctx* ctx, int64_t n, const double* mass, const double* ptype, double M, const u64* key, u64* hist, u64* bound,
                    int64_t* c, int64_t* n_gas) {
    hipStream_t st = ctx->stream;
    const unsigned hblk = sphx_blocks((size_t)n, SN_WG) < 1024u ? sphx_blocks((size_t)n, SN_WG) : 1024u;
    u64 prefix = 0ull, mask = 0ull, w_below = 0ull, c_below = 0ull;
    u64 h[2 * SN_BINS];
    for (int shift = 56; shift >= 0; shift -= 8) {
        HIPCHK(hipMemsetAsync(hist, 0, sizeof(h), st));
        hipLaunchKernelGGL(sn_hist_kernel, dim3(hblk), dim3(SN_WG), 0, st, (int)n, key, ptype, mass, M, prefix, mask, shift, hist);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h, hist, sizeof(h), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        u64 w = w_below, cc = c_below;
        int b = 0;
        for (; b < SN_BINS; ++b) {
            w += h[b]; cc += h[SN_BINS + b];
            if (w >= SN_TARGET) break;
        }
        if (shift == 56) {
            u64 all = 0ull;
            for (int t = 0; t < SN_BINS; ++t) all += h[SN_BINS + t];
            *n_gas = (int64_t)all;
        }
        if (b == SN_BINS) {           // the weights never reach the target (only possible at the first level): every gas row
            *bound = ~0ull; *c = (int64_t)cc;
            return SPHX_OK;
        }
        const u64 low = shift ? ((1ull << shift) - 1ull) : 0ull;
        *bound = prefix | ((u64)b << shift) | low;
        *c = (int64_t)cc;
        // fine enough: the rows fit one LDS sort - or cannot (the bins below hold too many) and this bin adds no more than
        // one LDS sort's worth to them
        const u64 below = cc - h[SN_BINS + b];
        if (cc <= (u64)SPHX_SN_LDS_CAP || (below >= (u64)SPHX_SN_LDS_CAP && h[SN_BINS + b] <= (u64)SPHX_SN_LDS_CAP) || shift == 0)
            return SPHX_OK;
        w_below = w - h[b]; c_below = below;
        prefix |= (u64)b << shift; mask |= (u64)(SN_BINS - 1) << shift;
    }
    return SPHX_OK;
}

// ctx->sn_work: keys (n) | histograms (2 SN_BINS) | scalars (SNS_N) | chunk sums | total
struct SnWork { u64 *key, *hist, *scal; double *part, *tot; };
static int sn_work_carve(sphx_ctx* ctx, int64_t n, SnWork* w) {
    Carve c;
    c.take(w->key, (size_t)n); c.take(w->hist, 2 * SN_BINS); c.take(w->scal, SNS_N); c.take(w->part, sphx_tot_chunks(n)); c.take(w->tot, 1);
    c.slack(7 * sizeof(double));
    return sphx_carve_into(ctx, ctx->sn_work, c);
}
// ctx->sn_in: points (n,3) | velocities (n,3) | masses | ptypes (n each); gathered from the state: | sizes | mu (n each)
struct SnIn { double *pos, *vel, *m, *pt, *h, *mu; };
static int sn_in_carve(sphx_ctx* ctx, size_t nn, bool gathered, SnIn* in) {
    Carve c;
    c.take(in->pos, 3 * nn); c.take(in->vel, 3 * nn); c.take(in->m, nn); c.take(in->pt, nn);
    if (gathered) { c.take(in->h, nn); c.take(in->mu, nn); }
    return sphx_carve_into(ctx, ctx->sn_in, c);
}

int sphx_sn_check(sphx_ctx* ctx, const char* who, int64_t n, int64_t n_sn, const int64_t* supernova_pos, double mass_displaced, int64_t cap) {
    if (n < 1 || n > 0x7FFFFFF0ll || n_sn < 0 || cap < 0 || cap > 0x7FFFFFF0ll)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld, n_sn=%lld, cap=%lld (need 1 <= n < 2^31, n_sn >= 0, 0 <= cap < 2^31)", who, (long long)n,
                            (long long)n_sn, (long long)cap);
    if (!(mass_displaced > 0.0) || !sphx_finite(mass_displaced))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: mass_displaced=%g must be positive and finite", who, mass_displaced);
    for (int64_t s = 0; s < n_sn; ++s)
        if (supernova_pos[s] < 0 || supernova_pos[s] >= n)
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: supernova_pos[%lld]=%lld outside [0, %lld)", who, (long long)s, (long long)supernova_pos[s],
                                (long long)n);
    return SPHX_OK;
}

// The stars one after the other on device inputs: pos (n,3), mass, ptype (n), velocities (n,3) or NULL (kicked in place).
// The outputs stay on the device (res), cap rows of them; res->total rows are needed: with total > cap nothing was kicked
// from the first star that did not fit on, and the caller refuses.  Checked by the caller: sphx_sn_check.
int sphx_sn_run(sphx_ctx* ctx, const char* who, int64_t n, const double* pos, const double* mass, const double* ptype, int64_t n_sn,
                const int64_t* supernova_pos, double mass_displaced, double kick_energy, double* velocities, int64_t cap, SnRes* res) {
    hipStream_t st = ctx->stream;
    for (int i = 0; i <= SPHX_SN_STAGES; ++i)
        if (!ctx->sn_ev[i]) HIPCHK(hipEventCreate(&ctx->sn_ev[i]));
    for (int i = 0; i < SPHX_SN_STAGES; ++i) ctx->sn_ms[i] = 0.0;
    for (int i = 0; i < SPHX_SN_NCOUNT; ++i) ctx->sn_counts[i] = 0;
    const size_t nn = (size_t)n, ns = (size_t)(n_sn > 0 ? n_sn : 1), cp = (size_t)(cap > 0 ? cap : 1);
    SnWork w;
    SPHX_TRY(sn_work_carve(ctx, n, &w));
    u64 *key = w.key, *hist = w.hist, *scal = w.scal;
    double *part = w.part, *tot = w.tot;
    // outputs: d_vels (cap,3) | true_mass (n_sn) | vel (n_sn) | sel_ids (cap) int64
    Carve co;
    co.take(res->d_vels, 3 * cp); co.take(res->true_mass, ns); co.take(res->vel, ns); co.take(res->sel_ids, cp);
    SPHX_TRY(sphx_carve_into(ctx, ctx->sn_out, co));
    res->sel_count.assign((size_t)n_sn, 0);
    res->total = 0;
    HIPCHK(hipMemsetAsync(scal, 0, SNS_N * sizeof(u64), st));
    for (int64_t s = 0; s < n_sn; ++s) {
        const int ku = (int)supernova_pos[s];
        SPHX_TRY(sn_mark(ctx, 0));
        hipLaunchKernelGGL(sn_key_kernel, dim3(sphx_blocks(nn, SN_WG)), dim3(SN_WG), 0, st, (int)n, pos, ku, key);
        HIPCHK(hipGetLastError());
        SPHX_TRY(sn_mark(ctx, 1));
        u64 bound; int64_t c, n_gas, nsel; bool crossed;
        SPHX_TRY(sn_bound(ctx, n, mass, ptype, mass_displaced, key, hist, &bound, &c, &n_gas));
        SPHX_TRY(sn_mark(ctx, 2));
        double* cm; int* cid;
        SPHX_TRY(sn_select(ctx, who, n, mass, ptype, mass_displaced, bound, c, key, scal, &nsel, &crossed, &cm, &cid));
        if (!crossed && c < n_gas) {              // the walk ran out of candidates and rows were left out: every gas row
            ++ctx->sn_counts[SPHX_SN_WIDENINGS];
            SPHX_TRY(sn_select(ctx, who, n, mass, ptype, mass_displaced, ~0ull, n_gas, key, scal, &nsel, &crossed, &cm, &cid));
        }
        SPHX_TRY(sn_mark(ctx, 5));
        res->sel_count[(size_t)s] = nsel;
        const int64_t off = res->total;
        res->total += nsel;
        if (res->total <= cap) {
            if (nsel > 0) {
                SPHX_TRY(sphx_ordered_totals(ctx, nsel, 1, cm, part, tot));
            } else {
                HIPCHK(hipMemsetAsync(tot, 0, sizeof(double), st));     // the empty sum: vel = inf
            }
            hipLaunchKernelGGL(sn_vel_kernel, dim3(1), dim3(1), 0, st, tot, kick_energy, res->true_mass + s, res->vel + s);
            if (nsel > 0)
                hipLaunchKernelGGL(sn_kick_kernel, dim3(sphx_blocks((size_t)nsel, SN_WG)), dim3(SN_WG), 0, st, (int)nsel, cid, pos, ku,
                                   res->vel + s, res->sel_ids + off, res->d_vels + 3 * off, velocities, scal);
            HIPCHK(hipGetLastError());
        }
        SPHX_TRY(sn_mark(ctx, 6));
        HIPCHK(hipEventSynchronize(ctx->sn_ev[6]));     // (the candidates' buffer is the next star's too)
        for (int i = 0; i < SPHX_SN_STAGES; ++i) {
            float t = 0.f;
            HIPCHK(hipEventElapsedTime(&t, ctx->sn_ev[i], ctx->sn_ev[i + 1]));
            ctx->sn_ms[i] += t;
        }
    }
    u64 back[SNS_N];
    HIPCHK(hipMemcpyAsync(back, scal, sizeof(back), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ctx->sn_counts[SPHX_SN_ZERO_DISTANCE] = (int64_t)back[SNS_ZERO];
    ctx->sn_counts[SPHX_SN_BAD_MASS] = (int64_t)back[SNS_BAD_MASS];
    return SPHX_OK;
}

extern "C" int sphx_supernova_impulse(sphx_ctx* ctx, int64_t n, const double* points, const double* masses, const double* ptypes,
                                      int64_t n_sn, const int64_t* supernova_pos, double mass_displaced, double kick_energy,
                                      double* velocities_inout, int64_t cap, int64_t* sel_count, int64_t* sel_ids, double* d_vels,
                                      double* true_mass, double* vel, int64_t* counts) {
    if (!ctx) return SPHX_E_ARG;
    NEED(points); NEED(masses); NEED(ptypes); NEED(sel_count); NEED(true_mass); NEED(vel);
    if (n_sn > 0) NEED(supernova_pos);
    if (cap > 0) { NEED(sel_ids); NEED(d_vels); }
    SPHX_TRY(sphx_sn_check(ctx, "sphx_supernova_impulse", n, n_sn, supernova_pos, mass_displaced, cap));
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nn = (size_t)n;
    SnIn in;
    SPHX_TRY(sn_in_carve(ctx, nn, false, &in));
    double *d_pos = in.pos, *d_v = in.vel, *d_m = in.m, *d_pt = in.pt;
    const CopyF64 us[] = {{points, d_pos, 3 * nn}, {velocities_inout, d_v, 3 * nn}, {masses, d_m, nn}, {ptypes, d_pt, nn}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 4));
    SnRes res;
    SPHX_TRY(sphx_sn_run(ctx, "sphx_supernova_impulse", n, d_pos, d_m, d_pt, n_sn, supernova_pos, mass_displaced, kick_energy,
                         velocities_inout ? d_v : nullptr, cap, &res));
    if (res.total > cap)
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_supernova_impulse: cap=%lld, the selections hold %lld rows", (long long)cap,
                            (long long)res.total);
    const CopyF64 ds[] = {{velocities_inout, d_v, 3 * nn}, {d_vels, res.d_vels, 3 * (size_t)res.total}, {true_mass, res.true_mass, (size_t)n_sn},
                          {vel, res.vel, (size_t)n_sn}, {sel_ids, res.sel_ids, (size_t)res.total}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 5));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int64_t s = 0; s < n_sn; ++s) sel_count[s] = res.sel_count[(size_t)s];
    if (counts)
        for (int i = 0; i < SPHX_SN_NCOUNT; ++i) counts[i] = ctx->sn_counts[i];
    return SPHX_OK;
}

// ---- the event on the resident state (drv:350-358), N unchanged ----
// The state is GATHERED into the caller's particle order as the phases gather it (sphx_phase_gather: positions, kicked
// velocities, masses, types, the step's radii), the step's own list translated to caller ids (sphx_phase_translate);
// sphx_sn_run works on that copy, the crossing time is formed on it, and only then the velocities go back through
// st.id: a refused call has written nothing of the state.
extern "C" int sphx_state_supernova_impulse(sphx_ctx* ctx, int64_t n_sn, const int64_t* ids, double mass_displaced, double kick_energy,
                                            double dt_0, int64_t cap, int64_t* sel_count, int64_t* sel_ids, double* d_vels,
                                            double* true_mass, double* vel, int64_t* counts, double* ct, double* dt_event) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_supernova_impulse";
    SPHX_TRY(sphx_phase_need_list(ctx, who));
    NEED(sel_count); NEED(true_mass); NEED(vel); NEED(ct); NEED(dt_event);
    if (n_sn > 0) NEED(ids);
    if (cap > 0) { NEED(sel_ids); NEED(d_vels); }
    const int64_t n = ctx->n;
    const int k = ctx->k;
    SPHX_TRY(sphx_sn_check(ctx, who, n, n_sn, ids, mass_displaced, cap));
    HIPCHK(hipSetDevice(ctx->device));
    // gathered (mu is not read)
    SnIn in;
    SPHX_TRY(sn_in_carve(ctx, (size_t)n, true, &in));
    double *d_pos = in.pos, *d_v = in.vel, *d_m = in.m, *d_pt = in.pt, *d_h = in.h, *d_mu = in.mu;
    PhaseInts pi;
    SPHX_TRY(sphx_phase_ints(ctx, n, k, &pi));
    int *col = pi.col, *list = pi.list;
    const StateArrays& st = ctx->st;
    PhaseGather ga;
    ga.n = (int)n; ga.qorder = ctx->step_qorder; ga.id = st.id.as<int>();
    ga.x = st.x.as<double>(); ga.y = st.y.as<double>(); ga.z = st.z.as<double>();
    ga.vx = st.vx.as<double>(); ga.vy = st.vy.as<double>(); ga.vz = st.vz.as<double>();
    ga.m = st.m.as<double>(); ga.mu = st.mu.as<double>(); ga.h = sphx_phase_sizes(ctx); ga.pt = st.ptype.as<double>();
    ga.T = nullptr; ga.E = nullptr;
    ga.col = col; ga.pos = d_pos; ga.sx = ga.sy = ga.sz = nullptr; ga.vel = d_v; ga.om = d_m; ga.omu = d_mu; ga.oh = d_h; ga.opt = d_pt;
    ga.oT = nullptr; ga.oE = nullptr;
    SPHX_TRY(sphx_phase_gather(ctx, ga));
    SPHX_TRY(sphx_phase_translate(ctx, col, true, list));
    SnRes res;
    SPHX_TRY(sphx_sn_run(ctx, who, n, d_pos, d_m, d_pt, n_sn, ids, mass_displaced, kick_energy, d_v, cap, &res));
    if (res.total > cap)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: cap=%lld, the selections hold %lld rows", who, (long long)cap, (long long)res.total);
    // drv:357: crossing_time on the step's list, the KICKED velocities, the step's radii
    SnWork w;
    SPHX_TRY(sn_work_carve(ctx, n, &w));            // (as sphx_sn_run has just carved it)
    u64* ct_bits = w.scal + SNS_CT;
    SPHX_TRY(sphx_loop_ct_dev(ctx, n, k, list, d_v, d_h, d_pt, ct_bits));
    const PhaseBack ba{(int)n, st.id.as<int>(), d_v, st.vx.as<double>(), st.vy.as<double>(), st.vz.as<double>(), 0,
                       {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}};
    SPHX_TRY(sphx_phase_back(ctx, ba));
    u64 bits = 0;
    HIPCHK(hipMemcpyAsync(&bits, ct_bits, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    const CopyF64 ds[] = {{d_vels, res.d_vels, 3 * (size_t)res.total}, {true_mass, res.true_mass, (size_t)n_sn}, {vel, res.vel, (size_t)n_sn},
                          {sel_ids, res.sel_ids, (size_t)res.total}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int64_t s = 0; s < n_sn; ++s) sel_count[s] = res.sel_count[(size_t)s];
    if (counts)
        for (int i = 0; i < SPHX_SN_NCOUNT; ++i) counts[i] = ctx->sn_counts[i];
    *ct = sphx_loop_ct_value(ctx, bits);
    const double short_dt = dt_0 / 100.;
    *dt_event = *ct < short_dt ? *ct : short_dt;              // drv:358: min(dt_0/100., ct), Python's: the first unless the second is smaller
    return SPHX_OK;
}

extern "C" int sphx_sn_last_timing(sphx_ctx* ctx, double ms[SPHX_SN_STAGES]) {
    if (!ctx || !ms) return SPHX_E_ARG;
    for (int i = 0; i < SPHX_SN_STAGES; ++i) ms[i] = ctx->sn_ms[i];
    return SPHX_OK;
}
