// sphx_cool.hip - rad_cooling (nsc:1019-1176): recombination and its cooling by the linearised Draine model, on the
// neighbour list `neighbors` returned.
//
// The reference loops over the gas rows j; each row forms seven sums over its K neighbours, six row scalars from them,
// and scatter-adds seven values into its neighbours' rows.  Here:
//   prep      one lane per particle: a 128-byte record of everything a pair needs from the neighbour (CoolRec,
//             sphx_cool_pair.h) - the five temperature coefficients are formed N times, not N K times.
//   list      one lane per list entry: the (n,k) int64 list becomes the K-major int32 list the row pass reads
//             coalesced (an entry outside [0, n) becomes -1 and contributes nothing), the rows that contribute are
//             flagged (a gas row with a gas neighbour, nsc:1028-1030) and the gas-gas pairs are counted per neighbour.
//   rows      one lane per row: the sums over K in list order, the six row scalars -> table (n,6).
//   reverse   the scatter is turned round: for each particle p the rows j that hold it - count (above), then scan, fill
//             (cool_fill_kernel) and the sort of each slice by sphx_rev_build (sphx_side.hip), so that p adds its
//             contributions in ascending j, the order the reference's loop adds them in.  An entry is a 4-byte row
//             index.  The same inputs give the same bits on every call.  No floating-point atomic anywhere.
//   gather    one lane per particle p: walks its slice (of any length: a hub particle sits in many rows), recomputes
//             the pair's weight and masks from its own record and x_j - cool_pair on the same r^2 the row pass used -
//             reads row j's six scalars, and then runs the elementwise epilogue (nsc:1112-1176) on what it holds.
// Vector stores from plain C++ only.  Every operation separately rounded, as NumPy's are.
#include "sphx_internal.h"
#include "sphx_cool_pair.h"
#pragma clang fp contract(off)

#define COOL_WG SPHX_COOL_WG

// np.minimum(x, 0.9999): a NaN stays a NaN (nsc:1089, 1094 in their repaired reading)
__device__ __forceinline__ double cool_cap(double x) { return x < 0.9999 ? x : (x != x ? x : 0.9999); }

struct CoolPrep {
    int n, s;
    const double *pos, *ptype, *m, *mu, *T, *fun;      // (n,3), (n,) x 4, (n,s)
    double d, m0, m_h, kB;
    CoolRec* rec;
};
__global__ __launch_bounds__(COOL_WG) void cool_prep_kernel(CoolPrep a) {
    const int i = blockIdx.x * COOL_WG + threadIdx.x;
    if (i >= a.n) return;
    CoolRec r;
    r.x = a.pos[3 * (size_t)i]; r.y = a.pos[3 * (size_t)i + 1]; r.z = a.pos[3 * (size_t)i + 2];
    const double m = a.m[i], d9 = pow9(a.d);
    const bool gas = a.ptype[i] == 0.0;
    const double c = weigh2_c(m, a.m0);
    r.h2 = weigh2_h2(m, a.d, a.m0);
    r.cg = gas ? c : 0.0;
    r.winv = 1.0 / weigh2_w(c, r.h2 - 0.0, d9);
    r.mm = a.mu[i] * a.m_h;
    const double* f = a.fun + (size_t)i * a.s;
    r.f2 = sphx_nan_to_num(f[2]); r.f3 = sphx_nan_to_num(f[3]); r.f4 = sphx_nan_to_num(f[4]); r.f5 = sphx_nan_to_num(f[5]);
    cool_coeffs(gas ? a.T[i] : 0.0, a.kB, r);
    a.rec[i] = r;
}

// entry e = (j, kk) of the list.  KMAJOR false: the caller's (n,k) int64 list, turned into the K-major int32 list nbr;
// KMAJOR true: nbr is given (K-major, rows of npad columns, caller ids, -1 = missing: what phase_list_kernel makes of the
// step's own list) and is only read.  Either way the reverse list's counts and the rows' flags.
template <bool KMAJOR>
__global__ __launch_bounds__(COOL_WG) void cool_list_kernel(int n, int npad, int k, const long long* __restrict__ nb,
                                                            const double* __restrict__ ptype, int* nbr, int* cnt, int* flag) {
    const long long e = (long long)blockIdx.x * COOL_WG + threadIdx.x;
    if (e >= (long long)n * k) return;
    const int j = (int)(e / k), kk = (int)(e - (long long)j * k);
    int p;
    if (KMAJOR) {
        const int q = nbr[(size_t)kk * npad + j];
        p = (q >= 0 && q < n) ? q : -1;
    } else {
        p = sphx_list_entry64(nb[e], n);
        nbr[(size_t)kk * npad + j] = p;
    }
    if (p >= 0 && ptype[j] == 0.0 && ptype[p] == 0.0) {
        atomicAdd(&cnt[p], 1);
        flag[j] = 1;
    }
}
// slice of p: the rows that hold it, in the order the atomics hand out (sorted afterwards)
__global__ __launch_bounds__(COOL_WG) void cool_fill_kernel(int n, int npad, int k, const int* __restrict__ nbr,
                                                            const double* __restrict__ ptype, const int* __restrict__ start,
                                                            int* cur, int* __restrict__ rev) {
    const long long e = (long long)blockIdx.x * COOL_WG + threadIdx.x;
    if (e >= (long long)npad * k) return;
    const int kk = (int)(e / npad), j = (int)(e - (long long)kk * npad);
    if (j >= n) return;
    const int p = nbr[e];
    if (p >= 0 && ptype[j] == 0.0 && ptype[p] == 0.0) rev[start[p] + atomicAdd(&cur[p], 1)] = j;
}

struct CoolRows {
    int n, npad, k;
    const int* nbr;
    const int* flag;
    const CoolRec* rec;
    double dt, d;
    double* tab;                                        // (n,6): f_Hn, f_H, f_He, f_e, E_H, E_He
};
__global__ __launch_bounds__(COOL_WG) void cool_row_kernel(CoolRows a) {
    const int j = blockIdx.x * COOL_WG + threadIdx.x;
    if (j >= a.n) return;
    double* t = a.tab + 6 * (size_t)j;
    if (!a.flag[j]) {
        t[0] = t[1] = t[2] = t[3] = t[4] = t[5] = 0.0;
        return;
    }
    const double xj = a.rec[j].x, yj = a.rec[j].y, zj = a.rec[j].z, d9 = pow9(a.d);
    double num_e = 0.0, A = 0.0, B = 0.0, SH = 0.0, SHe = 0.0, nHp = 0.0, nHep = 0.0, Cn = 0.0;
    for (int kk = 0; kk < a.k; ++kk) {
        const int p = a.nbr[(size_t)kk * a.npad + j];
        if (p < 0) continue;
        const CoolRec r = a.rec[p];
        const double dx = r.x - xj, dy = r.y - yj, dz = r.z - zj;
        const CoolPair pr = cool_pair(r, dx * dx + dy * dy + dz * dz, d9);
        if (pr.ne > 0.0) {                                               // the [n_e > 0] selections of nsc:1075-1097
            const double th = r.Hf * pr.ne, the = r.Hef * pr.ne;
            num_e += pr.ne; A += th; B += the;
            SH += th * r.eH; SHe += the * r.eHe;
        }
        nHp += pr.nHp; nHep += pr.nHep;                                  // (zero where not positive)
        if (pr.nH0 > 0.0) Cn += r.H2f * pr.nH0;
    }
    const double fe = cool_cap((A * nHp + B * nHep) / num_e * a.dt);     // nsc:1088-1089; num_e = 0: NaN
    const double sH = sphx_nan_to_num(A / (A + B)), sHe = sphx_nan_to_num(B / (A + B));     // nsc:1091-1092
    t[0] = sphx_nan_to_num(cool_cap(Cn * a.dt));                         // nsc:1094, 1105
    t[1] = sphx_nan_to_num(fe * sH);                                     // nsc:1091, 1106
    t[2] = sphx_nan_to_num(fe * sHe);
    t[3] = sphx_nan_to_num(fe);
    t[4] = SH * sH * a.dt;                                               // nsc:1096-1097
    t[5] = SHe * sHe * a.dt;
}

struct CoolGather {
    int n, s;
    const int *start, *rev;
    const CoolRec* rec;
    const double* tab;
    const double* fun;                                  // (n,s)
    double d;
    double *final_comp, *energy, *rec_array;            // (n,s), (n,), (s,n)
};
__global__ __launch_bounds__(COOL_WG) void cool_gather_kernel(CoolGather a) {
    const int p = blockIdx.x * COOL_WG + threadIdx.x;
    if (p >= a.n) return;
    const CoolRec me = a.rec[p];
    const double d9 = pow9(a.d);
    double e3 = 0.0, e4 = 0.0, r2 = 0.0, r3 = 0.0, r4 = 0.0, r5 = 0.0, rel = 0.0;
    const int t1 = a.start[p + 1];
    for (int t = a.start[p]; t < t1; ++t) {                              // ascending j: the reference's loop order
        const int j = a.rev[t];
        const double dx = me.x - a.rec[j].x, dy = me.y - a.rec[j].y, dz = me.z - a.rec[j].z;
        const CoolPair pr = cool_pair(me, dx * dx + dy * dy + dz * dz, d9);
        const double* row = a.tab + 6 * (size_t)j;
        const double w = pr.relw;
        e3 += sphx_nan_to_num(row[4] * w);                               // nsc:1102-1103
        e4 += sphx_nan_to_num(row[5] * w);
        if (pr.nH0 > 0.0) r2 += row[0] * w;                              // nsc:1105-1108
        if (pr.ne > 0.0) { r3 += row[1] * w; r4 += row[2] * w; r5 += row[3] * w; }
        rel += w;                                                        // nsc:1110
    }
    // ---- epilogue, nsc:1112-1176 ----
    const double den = rel + 1e-90;
    r2 = sphx_nan_to_num(r2 / den); r3 = sphx_nan_to_num(r3 / den); r4 = sphx_nan_to_num(r4 / den); r5 = sphx_nan_to_num(r5 / den);
    e3 = e3 / den; e4 = e4 / den;
    const double* fin = a.fun + (size_t)p * a.s;
    double f0 = sphx_nan_to_num(fin[0]), f1 = sphx_nan_to_num(fin[1]);
    double f2 = me.f2, f3 = me.f3, f4 = me.f4, f5 = me.f5;
    const double Hp = f5 * r3, Hep = f5 * r4, el = f5 * r5;              // nsc:1118-1120
    const double qa = sphx_nan_to_num(Hp / f3), qb = sphx_nan_to_num(Hep / f4);
    const double mf2 = qa > qb ? qa : qb;                                // nsc:1122: the third argument is `out`
    double mult = mf2;
    if (mf2 > 0.9999) mult = 0.9999 / mf2;                               // nsc:1124-1126; mf2 == 0.9999 keeps its value
    if (mf2 < 0.9999) mult = 1.0;
    if (f5 < 1e-10) mult = 0.0;
    a.energy[p] = e3 * f3 + e4 * f4;                                     // nsc:1138
    f1 += Hep * mult; f2 += Hp * mult;                                   // nsc:1148-1153
    f3 -= Hp * mult; f4 -= Hep * mult; f5 -= el * mult;
    r2 = r2 < 0.9999 ? r2 : 0.9999;                                      // nsc:1155 (r2 is no NaN here)
    const double H2 = f2 * r2;
    f0 += H2 / 2.0; f2 -= H2;                                            // nsc:1158-1159
    double sum = ((((f0 + f1) + f2) + f3) + f4) + f5;                    // nsc:1174: over all S species, in their order
    for (int c = 6; c < a.s; ++c) sum += sphx_nan_to_num(fin[c]);
    double* fo = a.final_comp + (size_t)p * a.s;
    fo[0] = f0 / sum; fo[1] = f1 / sum; fo[2] = f2 / sum; fo[3] = f3 / sum; fo[4] = f4 / sum; fo[5] = f5 / sum;
    for (int c = 6; c < a.s; ++c) fo[c] = sphx_nan_to_num(fin[c]) / sum;
    const size_t n = (size_t)a.n;
    a.rec_array[p] = 0.0; a.rec_array[n + p] = 0.0;
    a.rec_array[2 * n + p] = r2; a.rec_array[3 * n + p] = r3; a.rec_array[4 * n + p] = r4; a.rec_array[5 * n + p] = r5;
    for (int c = 6; c < a.s; ++c) a.rec_array[(size_t)c * n + p] = 0.0;
}

// =====================================================================================================================
// host side
// =====================================================================================================================
// nsc:1019-1176 on inputs that are on the device, in the caller's particle order.  The list: nb64, the (n,k) int64 list
// on the device, or kmajor, the K-major int32 list in caller ids (nb64 NULL).  t: the stage timer whose stages 1 .. 3 are
// marked, or NULL.  Results on the device (ctx->cool_out, ctx->cool_tab).
int sphx_cool_run(sphx_ctx* ctx, const char* who, int64_t n, int k, int s, const CoolDev& in, const long long* nb64, const int* kmajor,
                  double dt, double d, StageTimer* t, CoolRes* res) {
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)n, npad = (size_t)sphx_pad64(n), ns = nn * (size_t)s, nk = nn * (size_t)k;
    // ---- records; the K-major list, the rows' flags, the counts ----
    SPHX_TRY(sphx_ensure(ctx, ctx->cool_rec, nn * sizeof(CoolRec)));
    // ints: nbr (k npad) | cnt (n + 1) | cur (n + 1) | flag (n + 1) | start (n + 1), each part on a 16-byte boundary
    int *own, *cnt, *cur, *flag, *start;
    Carve ci;
    ci.take(own, (size_t)k * npad);
    ci.take(cnt, nn + 1, 16); ci.take(cur, nn + 1, 16); ci.take(flag, nn + 1, 16); ci.take(start, nn + 1, 16);
    ci.pad(16);
    SPHX_TRY(sphx_carve_into(ctx, ctx->cool_int, ci));
    int* nbr = nb64 ? own : const_cast<int*>(kmajor);
    HIPCHK(hipMemsetAsync(cnt, 0, (size_t)(start - cnt) * sizeof(int), st));
    CoolPrep pa;
    pa.n = (int)n; pa.s = s; pa.pos = in.pos; pa.ptype = in.pt; pa.m = in.m; pa.mu = in.mu; pa.T = in.T; pa.fun = in.fun;
    pa.d = d; pa.m0 = ctx->cst.m_0; pa.m_h = ctx->cst.m_h; pa.kB = ctx->cst.k_B;
    pa.rec = ctx->cool_rec.as<CoolRec>();
    const unsigned nblk = sphx_blocks(nn, COOL_WG);
    const dim3 lgrid(sphx_blocks(nk, COOL_WG));
    hipLaunchKernelGGL(cool_prep_kernel, dim3(nblk), dim3(COOL_WG), 0, st, pa);
    if (nb64) hipLaunchKernelGGL(cool_list_kernel<false>, lgrid, dim3(COOL_WG), 0, st, (int)n, (int)npad, k, nb64, in.pt, nbr, cnt, flag);
    else hipLaunchKernelGGL(cool_list_kernel<true>, lgrid, dim3(COOL_WG), 0, st, (int)n, (int)npad, k, nb64, in.pt, nbr, cnt, flag);
    HIPCHK(hipGetLastError());
    if (t) SPHX_TRY(t->mark(ctx, 1));
    // ---- rows ----
    SPHX_TRY(sphx_ensure(ctx, ctx->cool_tab, 6 * nn * sizeof(double)));
    CoolRows ra;
    ra.n = (int)n; ra.npad = (int)npad; ra.k = k; ra.nbr = nbr; ra.flag = flag; ra.rec = pa.rec; ra.dt = dt; ra.d = d;
    ra.tab = ctx->cool_tab.as<double>();
    hipLaunchKernelGGL(cool_row_kernel, dim3(nblk), dim3(COOL_WG), 0, st, ra);
    HIPCHK(hipGetLastError());
    if (t) SPHX_TRY(t->mark(ctx, 2));
    // ---- the reverse list: keys are rows (cnt[n] = 0: the memset above; cnt and start lie on 16-byte boundaries) ----
    RevList rl;
    SPHX_TRY(sphx_rev_build(ctx, who, n, cnt, start, nk, (unsigned long long)n, [&](const int* start_, int* rev_raw) {
        hipLaunchKernelGGL(cool_fill_kernel, dim3(sphx_blocks((size_t)k * npad, COOL_WG)), dim3(COOL_WG), 0, st, (int)n, (int)npad, k, nbr,
                           in.pt, start_, cur, rev_raw);
    }, &rl));
    // ---- gather and epilogue: final_comp (n s) | energy (n) | rec_array (s n) ----
    CoolGather ga;
    ga.n = (int)n; ga.s = s; ga.start = start; ga.rev = rl.rev; ga.rec = pa.rec; ga.tab = ra.tab; ga.fun = in.fun; ga.d = d;
    Carve co;
    co.take(ga.final_comp, ns); co.take(ga.energy, nn); co.take(ga.rec_array, ns);
    SPHX_TRY(sphx_carve_into(ctx, ctx->cool_out, co));
    hipLaunchKernelGGL(cool_gather_kernel, dim3(nblk), dim3(COOL_WG), 0, st, ga);
    HIPCHK(hipGetLastError());
    if (t) SPHX_TRY(t->mark(ctx, 3));
    res->final_comp = ga.final_comp; res->energy = ga.energy; res->rec_array = ga.rec_array; res->tab = ra.tab;
    return SPHX_OK;
}
int sphx_cool_check(sphx_ctx* ctx, const char* who, int64_t n, int k, int s, double dt, double d) {
    if (n < 1 || k < 1 || s < 6)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld, k=%d, s=%d (need n >= 1, k >= 1, s >= 6)", who, (long long)n, k, s);
    if (n > 0x7FFFFFF0ll || sphx_pad64(n) * (int64_t)k > 0x7FFFFFF0ll || n * (int64_t)s > (1ll << 40))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld x k=%d (or x s=%d) out of range", who, (long long)n, k, s);
    if (!sphx_finite(dt) || !sphx_finite(d))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: dt=%g, d=%g must be finite", who, dt, d);
    return SPHX_OK;
}

extern "C" int sphx_rad_cooling(sphx_ctx* ctx, int64_t n, int k, int s, const double* points, const double* ptype,
                                const double* mass, const double* f_un, const int64_t* neighbor, const double* mu,
                                const double* T, double dt, double d, double* final_comp, double* energy, double* rec_array,
                                double* row_table) {
    if (!ctx) return SPHX_E_ARG;
    SPHX_TRY(sphx_cool_check(ctx, "sphx_rad_cooling", n, k, s, dt, d));
    NEED(points); NEED(ptype); NEED(mass); NEED(f_un); NEED(neighbor); NEED(mu); NEED(T);
    NEED(final_comp); NEED(energy); NEED(rec_array);
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->cool_t.begin(ctx));
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)n, ns = nn * (size_t)s, nk = nn * (size_t)k;
    // ---- inputs: points (3n) | ptype | mass | mu | T (n each) | f_un (n s); the list as given ----
    double *d_pos, *d_pt, *d_m, *d_mu, *d_T, *d_fun;
    Carve c;
    c.take(d_pos, 3 * nn); c.take(d_pt, nn); c.take(d_m, nn); c.take(d_mu, nn); c.take(d_T, nn); c.take(d_fun, ns);
    SPHX_TRY(sphx_carve_into(ctx, ctx->cool_in, c));
    SPHX_TRY(sphx_ensure(ctx, ctx->cool_nb, nk * sizeof(int64_t)));
    const CopyF64 us[] = {{points, d_pos, 3 * nn}, {ptype, d_pt, nn}, {mass, d_m, nn}, {mu, d_mu, nn}, {T, d_T, nn}, {f_un, d_fun, ns}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 6));
    HIPCHK(hipMemcpyAsync(ctx->cool_nb.p, neighbor, nk * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const CoolDev din{d_pos, d_pt, d_m, d_mu, d_T, d_fun};
    CoolRes r;
    SPHX_TRY(sphx_cool_run(ctx, "sphx_rad_cooling", n, k, s, din, (const long long*)ctx->cool_nb.p, nullptr, dt, d, &ctx->cool_t, &r));
    const CopyF64 ds[] = {{final_comp, r.final_comp, ns}, {energy, r.energy, nn}, {rec_array, r.rec_array, ns}, {row_table, r.tab, 6 * nn}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 4));
    SPHX_TRY(ctx->cool_t.mark(ctx, 4));
    HIPCHK(hipStreamSynchronize(st));
    return ctx->cool_t.end(ctx);
}
