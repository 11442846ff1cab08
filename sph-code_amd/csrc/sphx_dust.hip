// sphx_dust.hip - supernova_destruction (nsc:1211-1263): shock sputtering of dust by the gas rows that hold it, on the
// neighbour list `neighbors` returned.
//
// The reference loops over the gas rows j in ascending order; each row forms, for every dust entry i and species t, the
// atoms lost, accepts them only while acc[i,t] + lost < 1 - which reads what EARLIER rows took from i - adds the
// accepted ones to acc[i,:] and their sum over the row to reup[j,:].  The pair term depends on j's and i's data alone;
// only the guard depends on the order.  Here:
//   prep      one lane per particle: a 128-byte record of what a pair needs from either side (DustRec, sphx_dust_pair.h).
//   list      one lane per list entry: the (n,k) int64 list becomes the K-major int32 list the row pass reads coalesced
//             (an entry outside [0, n) becomes -1), the (gas row, dust entry) pairs are counted per dust particle, and the
//             row's flag collects "has a dust entry", "some rho > 0", "some rho is NaN" (integer atomics): the row
//             contributes when sum_k rho > 0 (nsc:1239), i.e. when the flag is 3.
//   reverse   for each dust particle i the pairs that hold it - count (above), then scan, fill (dust_fill_kernel) and the
//             sort of each slice by sphx_rev_build (sphx_side.hip, which rad_cooling and chemisputtering_2 use as well).
//             An entry is the 4-byte key j K + k: ascending keys are ascending rows, and the key names the slot.
//   dust      one lane per particle i: walks its slice in ascending key with acc[t] in registers for the selected
//             species, applies the guard, leaves one word of accept bits per pair in an (K, npad) array, counts the
//             regimes (integer atomics, one per wave and counter), writes frac_destruction[i,:].
//   rows      one lane per row j: recomputes its K pairs in list order on the same operands, multiplies by the stored
//             accept bits, sums, writes frac_reuptake[j,:].
// No floating-point atomic anywhere: the same inputs give the same bits on every call.  Vector stores from plain C++
// only.  Every operation separately rounded, as NumPy's are.
#include "sphx_internal.h"
#include "sphx_dust_pair.h"
#pragma clang fp contract(off)

#define DUST_WG SPHX_DUST_WG
#define DUST_NCOUNT 5

struct DustPrep {
    int n;
    const double *pos, *vel, *m, *mu, *sizes;           // (n,3) x 2, (n,) x 3
    double crit_mass, amu;
    DustRec* rec;
};
__global__ __launch_bounds__(DUST_WG) void dust_prep_kernel(DustPrep a) {
    const int i = blockIdx.x * DUST_WG + threadIdx.x;
    if (i >= a.n) return;
    DustRec r;
    r.x = a.pos[3 * (size_t)i]; r.y = a.pos[3 * (size_t)i + 1]; r.z = a.pos[3 * (size_t)i + 2];
    r.vx = a.vel[3 * (size_t)i]; r.vy = a.vel[3 * (size_t)i + 1]; r.vz = a.vel[3 * (size_t)i + 2];
    const double m = a.m[i], s = a.sizes[i];
    const bool big = m > a.crit_mass;
    r.s2 = s * s;
    r.den = PI64 * pow9(s);
    r.cw = big ? m * 315.0 : 0.0;
    const double q = r.s2 - 0.0;
    r.w0 = m * 315.0 * (q * q * q) / r.den;
    r.N = m / (a.mu[i] * a.amu);
    r.C = big ? 1.0 : 0.0;
    r.pad_[0] = r.pad_[1] = r.pad_[2] = r.pad_[3] = 0.0;
    a.rec[i] = r;
}

// the pairs that exist: a gas row's dust entry (nsc:1220-1222, 1237)
__device__ __forceinline__ bool dust_is_pair(const double* __restrict__ ptype, int j, int p) {
    return p >= 0 && ptype[j] == 0.0 && ptype[p] == 2.0;
}

// entry e of the list.  FROM64: e = (j, kk) of the (n,k) int64 list nb, whose K-major int32 form is written to nbr_out;
// else e = (kk, j) of a K-major int32 list that exists already (nbr_in; sphx_state_dust_phase's)
template <bool FROM64>
__global__ __launch_bounds__(DUST_WG) void dust_list_kernel(int n, int npad, int k, const long long* __restrict__ nb,
                                                            const int* __restrict__ nbr_in, const double* __restrict__ ptype,
                                                            const DustRec* __restrict__ rec, int* __restrict__ nbr_out, int* cnt,
                                                            int* flag) {
    const long long e = (long long)blockIdx.x * DUST_WG + threadIdx.x;
    int j, p;
    if (FROM64) {
        if (e >= (long long)n * k) return;
        j = (int)(e / k);
        const int kk = (int)(e - (long long)j * k);
        p = sphx_list_entry64(nb[e], n);
        nbr_out[(size_t)kk * npad + j] = p;
    } else {
        if (e >= (long long)npad * k) return;
        j = (int)(e % npad);
        if (j >= n) return;
        p = nbr_in[e];
    }
    if (dust_is_pair(ptype, j, p)) {
        atomicAdd(&cnt[p], 1);
        const DustRec r = rec[p];
        const double rho = dust_rho(r, dust_r2(r.x, r.y, r.z, rec[j].x, rec[j].y, rec[j].z));
        atomicOr(&flag[j], 1 | (rho > 0.0 ? 2 : 0) | (rho != rho ? 4 : 0));
    }
}
// slice of i: the keys j k + kk of the pairs that hold it, in the order the atomics hand out (sorted afterwards)
__global__ __launch_bounds__(DUST_WG) void dust_fill_kernel(int n, int npad, int k, const int* __restrict__ nbr,
                                                            const double* __restrict__ ptype, const int* __restrict__ start,
                                                            int* cur, int* __restrict__ rev) {
    const long long e = (long long)blockIdx.x * DUST_WG + threadIdx.x;
    if (e >= (long long)npad * k) return;
    const int kk = (int)(e / npad), j = (int)(e - (long long)kk * npad);
    if (j >= n) return;
    const int p = nbr[e];
    if (dust_is_pair(ptype, j, p)) rev[start[p] + atomicAdd(&cur[p], 1)] = j * k + kk;
}

struct DustWalk {
    int n, npad, k, s;
    unsigned sel, si;                                   // bit t: species t has a curve; that curve is the silicon one
    int fraction;                                       // guard: limit = N_i instead of 1
    const int *start, *rev, *nbr, *flag;
    const DustRec* rec;
    const double *dens, *fun, *ptype;                   // (n,), (n,s), (n,)
    double crit_density;
    const DustKnots* kn;                                // on the device
    unsigned* msk;                                      // (k, npad): accept bits of pair (j, kk) at kk npad + j
    unsigned long long* counts;                         // DUST_NCOUNT
    double *destr, *reup;                               // (n,s) each
};

// one atomic per wave and counter (every lane of the wave calls this)
__device__ __forceinline__ void dust_count(unsigned long long* slot, unsigned v) {
    for (int off = warpSize / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && v) atomicAdd(slot, (unsigned long long)v);
}

__global__ __launch_bounds__(DUST_WG) void dust_pass_kernel(DustWalk a) {
    const int i = blockIdx.x * DUST_WG + threadIdx.x;
    unsigned c_pos = 0, c_acc = 0, c_rej = 0, c_rej_small = 0, c_cap = 0;
    if (i < a.n) {
        const DustRec me = a.rec[i];
        const double limit = a.fraction ? me.N : 1.0;
        double acc[SPHX_MAX_SPECIES], f[SPHX_MAX_SPECIES];
#pragma unroll
        for (int t = 0; t < SPHX_MAX_SPECIES; ++t) {
            acc[t] = 0.0;
            f[t] = (t < a.s && ((a.sel >> t) & 1u)) ? a.fun[(size_t)i * a.s + t] : 0.0;
        }
        const int t1 = a.start[i + 1];
        for (int u = a.start[i]; u < t1; ++u) {                          // ascending (j, kk): the reference's loop order
            const int key = a.rev[u];
            const int j = key / a.k, kk = key - j * a.k;
            unsigned word = 0;
            if (a.flag[j] == 3) {
                const DustRec* rj = a.rec + j;
                const double r2 = dust_r2(me.x, me.y, me.z, rj->x, rj->y, rj->z);
                const double dv2 = dust_r2(me.vx, me.vy, me.vz, rj->vx, rj->vy, rj->vz);
                const DustPair pr = dust_pair(me, r2, dv2, a.dens[j], a.crit_density, *a.kn);
#pragma unroll
                for (int t = 0; t < SPHX_MAX_SPECIES; ++t) {
                    if (!((a.sel >> t) & 1u)) continue;
                    bool capped;
                    const double ff = dust_ff(pr, ((a.si >> t) & 1u) ? pr.esi : pr.ec, capped);
                    double lost = dust_lost(ff, f[t], me.N);
                    const bool accept = acc[t] + lost < limit;           // nsc:1252
                    c_cap += capped;
                    if (lost > 0.0) {
                        ++c_pos;
                        if (accept) ++c_acc;
                        else { ++c_rej; c_rej_small += lost < limit; }
                    }
                    lost = lost * (accept ? 1.0 : 0.0);                  // NaN x False = NaN
                    acc[t] += lost;                                      // nsc:1257
                    word |= accept ? (1u << t) : 0u;
                }
            }
            a.msk[(size_t)kk * a.npad + j] = word;
        }
        double* out = a.destr + (size_t)i * a.s;
#pragma unroll
        for (int t = 0; t < SPHX_MAX_SPECIES; ++t)
            if (t < a.s) out[t] = sphx_nan_to_num(acc[t] / me.N);        // nsc:1260
    }
    dust_count(a.counts + 0, c_pos); dust_count(a.counts + 1, c_acc); dust_count(a.counts + 2, c_rej);
    dust_count(a.counts + 3, c_rej_small); dust_count(a.counts + 4, c_cap);
}

__global__ __launch_bounds__(DUST_WG) void dust_row_kernel(DustWalk a) {
    const int j = blockIdx.x * DUST_WG + threadIdx.x;
    if (j >= a.n) return;
    double sum[SPHX_MAX_SPECIES];
#pragma unroll
    for (int t = 0; t < SPHX_MAX_SPECIES; ++t) sum[t] = 0.0;
    const DustRec* me = a.rec + j;
    if (a.flag[j] == 3) {
        const double xj = me->x, yj = me->y, zj = me->z, vxj = me->vx, vyj = me->vy, vzj = me->vz, dens = a.dens[j];
        for (int kk = 0; kk < a.k; ++kk) {                               // list order: np.sum(dust_lost, axis=0), nsc:1253
            const int p = a.nbr[(size_t)kk * a.npad + j];
            if (!dust_is_pair(a.ptype, j, p)) continue;
            const DustRec r = a.rec[p];
            const DustPair pr = dust_pair(r, dust_r2(r.x, r.y, r.z, xj, yj, zj), dust_r2(r.vx, r.vy, r.vz, vxj, vyj, vzj), dens,
                                          a.crit_density, *a.kn);
            const unsigned word = a.msk[(size_t)kk * a.npad + j];
            const double* f = a.fun + (size_t)p * a.s;
#pragma unroll
            for (int t = 0; t < SPHX_MAX_SPECIES; ++t) {
                if (!((a.sel >> t) & 1u)) continue;
                bool capped;
                const double ff = dust_ff(pr, ((a.si >> t) & 1u) ? pr.esi : pr.ec, capped);
                sum[t] += dust_lost(ff, f[t], r.N) * (((word >> t) & 1u) ? 1.0 : 0.0);
            }
        }
    }
    const double N = me->N;
    double* out = a.reup + (size_t)j * a.s;
#pragma unroll
    for (int t = 0; t < SPHX_MAX_SPECIES; ++t)
        if (t < a.s) out[t] = sphx_nan_to_num(sum[t] / N);               // nsc:1261
}

// =====================================================================================================================
// host side: three parts (as sphx_rad.hip's rad_stage_host / rad_run) - the parameters checked and the host inputs staged
// (sphx_dust_params, dust_stage_host), the run on device inputs (sphx_dust_run: sphx_state_dust_phase calls it on the
// gathered resident state and leaves the outputs where they are), the outputs brought back.
// =====================================================================================================================
static_assert(sizeof(DustKnots) <= 40 * sizeof(double), "sphx_ctx::dust_kn holds the knots");

int sphx_dust_check_shape(sphx_ctx* ctx, const char* who, int64_t n, int k, int s) {
    if (n < 1 || k < 1 || k > 64 || s < 1 || s > SPHX_MAX_SPECIES)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld, k=%d, s=%d (need n >= 1, 1 <= k <= 64, 1 <= s <= %d)", who, (long long)n, k, s,
                            SPHX_MAX_SPECIES);
    if (n > 0x7FFFFFF0ll || sphx_pad64(n) * (int64_t)k > 0x7FFFFFF0ll)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld x k=%d out of range", who, (long long)n, k);
    return SPHX_OK;
}
int sphx_dust_check_scalars(sphx_ctx* ctx, const char* who, double crit_mass, double critical_density, int guard_mode) {
    if (!sphx_finite(crit_mass) || !sphx_finite(critical_density))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: crit_mass=%g, critical_density=%g must be finite", who, crit_mass, critical_density);
    if (guard_mode != SPHX_DUST_GUARD_COUNT && guard_mode != SPHX_DUST_GUARD_FRACTION)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: unknown guard mode %d", who, guard_mode);
    return SPHX_OK;
}
// the selector's bits into par; the knots and their slopes into ctx->dust_kn (held by the context: the upload reads it)
int sphx_dust_params(sphx_ctx* ctx, const char* who, int s, double crit_mass, double critical_density, const int32_t* species_curve,
                     const double knots_v[8], const double knots_c[8], const double knots_si[8], int guard_mode, DustPar* par) {
    DustKnots& kn = *reinterpret_cast<DustKnots*>(ctx->dust_kn);
    par->crit_mass = crit_mass; par->crit_density = critical_density;
    par->fraction = guard_mode == SPHX_DUST_GUARD_FRACTION;
    par->sel = par->si = 0;
    for (int t = 0; t < s; ++t) {
        if (species_curve[t] < 0 || species_curve[t] > 2)
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: species_curve[%d]=%d (need 0, 1 or 2)", who, t, (int)species_curve[t]);
        if (species_curve[t]) par->sel |= 1u << t;
        if (species_curve[t] == 2) par->si |= 1u << t;
    }
    for (int t = 0; t < 8; ++t) {
        if (!sphx_finite(knots_v[t]) || !sphx_finite(knots_c[t]) || !sphx_finite(knots_si[t]) || (t && !(knots_v[t] > knots_v[t - 1])))
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: knot %d must be finite and knots_v increasing", who, t);
        kn.v[t] = knots_v[t]; kn.c[t] = knots_c[t]; kn.si[t] = knots_si[t];
    }
    for (int t = 0; t < 7; ++t) {
        kn.sc[t] = (knots_c[t + 1] - knots_c[t]) / (knots_v[t + 1] - knots_v[t]);
        kn.ssi[t] = (knots_si[t + 1] - knots_si[t]) / (knots_v[t + 1] - knots_v[t]);
    }
    return SPHX_OK;
}

// inputs in ctx->dust_in: points, velocities (3n each) | mass | mu | sizes | densities | ptype (n each) | f_un (n s)
int sphx_dust_inputs(sphx_ctx* ctx, int64_t n, int s, DustDev* in) {
    const size_t nn = (size_t)n;
    Carve c;
    c.take(in->pos, 3 * nn); c.take(in->vel, 3 * nn); c.take(in->m, nn); c.take(in->mu, nn); c.take(in->sizes, nn); c.take(in->dens, nn);
    c.take(in->ptype, nn); c.take(in->fun, nn * (size_t)s);
    return sphx_carve_into(ctx, ctx->dust_in, c);
}

static int dust_stage_host(sphx_ctx* ctx, int64_t n, int k, int s, const double* points, const double* velocities,
                           const int64_t* neighbor, const double* mass, const double* f_un, const double* mu, const double* sizes,
                           const double* densities, const double* ptype, DustDev* in) {
    const size_t nn = (size_t)n, ns = nn * (size_t)s, nk = nn * (size_t)k;
    SPHX_TRY(sphx_dust_inputs(ctx, n, s, in));
    SPHX_TRY(sphx_ensure(ctx, ctx->dust_nb, nk * sizeof(int64_t)));
    const CopyF64 us[] = {{points, in->pos, 3 * nn}, {velocities, in->vel, 3 * nn}, {mass, in->m, nn}, {mu, in->mu, nn}, {sizes, in->sizes, nn},
                          {densities, in->dens, nn}, {ptype, in->ptype, nn}, {f_un, in->fun, ns}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 8));
    HIPCHK(hipMemcpyAsync(ctx->dust_nb.p, neighbor, nk * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    return SPHX_OK;
}

// The middle part: everything between the inputs on the device and frac_destruction / frac_reuptake / the five counters
// on the device (res).  nbr: a K-major int32 list that exists already, or NULL: the (n,k) int64 list in ctx->dust_nb, whose
// K-major form is made on the way.  t: the caller's stage timer, marks 1 .. 3 (NULL: none).
int sphx_dust_run(sphx_ctx* ctx, const char* who, int64_t n, int k, int s, const DustDev& in, const int* nbr_given, const DustPar& par,
                  StageTimer* t, DustRes* res) {
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)n, npad = (size_t)sphx_pad64(n), ns = nn * (size_t)s, nk = nn * (size_t)k;
    const DustKnots& kn = *reinterpret_cast<const DustKnots*>(ctx->dust_kn);
    const double *d_pt = in.ptype;
    // ---- records; the K-major list, the rows' flags, the counts ----
    SPHX_TRY(sphx_ensure(ctx, ctx->dust_rec, nn * sizeof(DustRec)));
    // ints: nbr (k npad) | cnt (n + 1) | cur (n + 1) | flag (n + 1) | start (n + 1) | msk (k npad), each part on a 16-byte boundary
    int *own, *cnt, *cur, *flag, *start;
    unsigned* msk;
    Carve ci;
    ci.take(own, (size_t)k * npad);
    ci.take(cnt, nn + 1, 16); ci.take(cur, nn + 1, 16); ci.take(flag, nn + 1, 16); ci.take(start, nn + 1, 16);
    ci.take(msk, (size_t)k * npad, 16);
    SPHX_TRY(sphx_carve_into(ctx, ctx->dust_int, ci));
    const int* nbr = nbr_given ? nbr_given : own;
    HIPCHK(hipMemsetAsync(cnt, 0, (size_t)(start - cnt) * sizeof(int), st));
    // outputs: counters (8 u64) | the knots (40 doubles) | frac_destruction (n s) | frac_reuptake (n s)
    DustWalk wa;
    double* knots;
    Carve co;
    co.take(wa.counts, 8); co.take(knots, 40); co.take(wa.destr, ns); co.take(wa.reup, ns);
    SPHX_TRY(sphx_carve_into(ctx, ctx->dust_out, co));
    HIPCHK(hipMemsetAsync(wa.counts, 0, 8 * sizeof(double), st));
    HIPCHK(hipMemcpyAsync(knots, &kn, sizeof(DustKnots), hipMemcpyHostToDevice, st));
    DustPrep pa;
    pa.n = (int)n; pa.pos = in.pos; pa.vel = in.vel; pa.m = in.m; pa.mu = in.mu; pa.sizes = in.sizes;
    pa.crit_mass = par.crit_mass; pa.amu = par.amu;
    pa.rec = ctx->dust_rec.as<DustRec>();
    const unsigned nblk = sphx_blocks(nn, DUST_WG), eblk = sphx_blocks((size_t)k * npad, DUST_WG);
    hipLaunchKernelGGL(dust_prep_kernel, dim3(nblk), dim3(DUST_WG), 0, st, pa);
    if (nbr_given)
        hipLaunchKernelGGL(dust_list_kernel<false>, dim3(eblk), dim3(DUST_WG), 0, st, (int)n, (int)npad, k, (const long long*)nullptr, nbr,
                           d_pt, pa.rec, (int*)nullptr, cnt, flag);
    else
        hipLaunchKernelGGL(dust_list_kernel<true>, dim3(sphx_blocks(nk, DUST_WG)), dim3(DUST_WG), 0, st, (int)n, (int)npad, k,
                           (const long long*)ctx->dust_nb.p, (const int*)nullptr, d_pt, pa.rec, own, cnt, flag);
    HIPCHK(hipGetLastError());
    if (t) SPHX_TRY(t->mark(ctx, 1));
    // ---- the reverse list: keys j k + kk (cnt[n] = 0: the memset above; cnt and start lie on 16-byte boundaries) ----
    RevList rl;
    SPHX_TRY(sphx_rev_build(ctx, who, n, cnt, start, nk, (unsigned long long)nk, [&](const int* start_, int* rev_raw) {
        hipLaunchKernelGGL(dust_fill_kernel, dim3(eblk), dim3(DUST_WG), 0, st, (int)n, (int)npad, k, nbr, d_pt, start_, cur, rev_raw);
    }, &rl));
    if (t) SPHX_TRY(t->mark(ctx, 2));
    // ---- the dust pass, then the row pass ----
    wa.sel = par.sel; wa.si = par.si;
    wa.n = (int)n; wa.npad = (int)npad; wa.k = k; wa.s = s;
    wa.fraction = par.fraction;
    wa.start = start; wa.rev = rl.rev; wa.nbr = nbr; wa.flag = flag; wa.rec = pa.rec;
    wa.dens = in.dens; wa.fun = in.fun; wa.ptype = d_pt;
    wa.crit_density = par.crit_density;
    wa.msk = msk;
    wa.kn = reinterpret_cast<const DustKnots*>(knots);
    hipLaunchKernelGGL(dust_pass_kernel, dim3(nblk), dim3(DUST_WG), 0, st, wa);
    HIPCHK(hipGetLastError());
    if (t) SPHX_TRY(t->mark(ctx, 3));
    hipLaunchKernelGGL(dust_row_kernel, dim3(nblk), dim3(DUST_WG), 0, st, wa);
    HIPCHK(hipGetLastError());
    res->destr = wa.destr; res->reup = wa.reup; res->counters = wa.counts;
    return SPHX_OK;
}

extern "C" int sphx_supernova_destruction(sphx_ctx* ctx, int64_t n, int k, int s, const double* points, const double* velocities,
                                          const int64_t* neighbor, const double* mass, const double* f_un, const double* mu,
                                          const double* sizes, const double* densities, const double* ptype, double crit_mass,
                                          double critical_density, const int32_t* species_curve, const double knots_v[8],
                                          const double knots_c[8], const double knots_si[8], int guard_mode,
                                          double* frac_destruction, double* frac_reuptake, int64_t* counts) {
    if (!ctx) return SPHX_E_ARG;
    SPHX_TRY(sphx_dust_check_shape(ctx, "sphx_supernova_destruction", n, k, s));
    SPHX_TRY(sphx_dust_check_scalars(ctx, "sphx_supernova_destruction", crit_mass, critical_density, guard_mode));
    NEED(points); NEED(velocities); NEED(neighbor); NEED(mass); NEED(f_un); NEED(mu); NEED(sizes); NEED(densities); NEED(ptype);
    NEED(species_curve); NEED(knots_v); NEED(knots_c); NEED(knots_si); NEED(frac_destruction); NEED(frac_reuptake);
    DustPar par;
    SPHX_TRY(sphx_dust_params(ctx, "sphx_supernova_destruction", s, crit_mass, critical_density, species_curve, knots_v, knots_c, knots_si,
                              guard_mode, &par));
    par.amu = ctx->cst.amu;
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->dust_t.begin(ctx));
    DustDev in;
    SPHX_TRY(dust_stage_host(ctx, n, k, s, points, velocities, neighbor, mass, f_un, mu, sizes, densities, ptype, &in));
    DustRes res;
    SPHX_TRY(sphx_dust_run(ctx, "sphx_supernova_destruction", n, k, s, in, nullptr, par, &ctx->dust_t, &res));
    const size_t ns = (size_t)n * (size_t)s;
    const CopyF64 ds[] = {{frac_destruction, res.destr, ns}, {frac_reuptake, res.reup, ns}, {counts, res.counters, DUST_NCOUNT}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 3));
    SPHX_TRY(ctx->dust_t.mark(ctx, 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ctx->dust_t.end(ctx);
}
