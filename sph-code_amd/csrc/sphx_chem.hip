// sphx_chem.hip - chemisputtering_2 (nsc:1265-1416): thermal / chemical sputtering of the dust rows and reuptake by the gas
// entries of their lists, on the neighbour list `neighbors` returned.
//
// The reference loops over the dust rows j in ascending order and rewrites the shared counts num_particles between rows.
// Almost all of a row reads the INPUTS alone (the gas weights, the composition density, the temperature, F_sput, the
// reuptake weights, new0 = (F_sput - 1) num0[j]); what depends on the order is three clamps against counts as the earlier
// rows left them.  That is a DAG over the rows, and it is solved by rounds: in a round every row clamps
// against counts formed from num0 and the PREVIOUS round's clamped sums of the earlier rows; a row whose earlier sharers
// hold their sequential value gets its sequential value, so a round that changes no bit has reached the sequential
// result.  No lane waits on another workgroup; a round is two launches and one counter.
//   prep      one lane per particle: num0 = f_un mass / sum(f_un mu_specie), the 64-byte record (ChemRec), the dust flag.
//   list      one lane per list entry: the (n,k) int64 list becomes the K-major int32 list (an entry outside [0, n): -1).
//   (scan of the dust flags: the dust rows get ordinals; everything per dust row is stored by ordinal, padded to 64)
//   row A     one lane per dust row: the gas weights of its entries, their sums, whether it contributes, the
//             temperature, the reuptake weight wk of every entry (three normalisations over the stored column).
//   row B     one lane per (dust row, column >= 6): the composition density, F_sput, new0.
//   reverse   for each gas particle the (contributing row, entry) pairs that hold it: count, then scan, fill
//             (chem_fill_kernel) and the sort of each slice by sphx_rev_build (sphx_side.hip, which rad_cooling and
//             supernova_destruction use as well).  An entry is the 4-byte key ordinal K + k: ascending keys are
//             ascending rows.  `pos` maps a row's entry back to its place in the reverse list.
//   gas pass  one lane per (gas particle, column >= 6): walks the slice in ascending row with the running count in a
//             register, applies clamps 1 and 2 to new0 wk, stores the clamped first-stage loss per (pair, column), then
//             subtracts the previous round's nan_to_num(sumc wk).
//   dust pass one lane per (dust row, column >= 6): sums its entries' first-stage losses in list order (a non-gas entry
//             has loss 0 and only clamps 1 and 2 on its count act - an earlier dust row's count includes what the
//             previous round gave it), applies clamp 3, spreads by wk, compares the bits with the previous round's.
//   closing   per column the sums of the positive and of the negative counts (chunks of 256 rows, then a tree over the
//             chunks: the same order on every call), then the zeroing and rescale, mass_new, f_un_new.
// A lane per (row, column) rather than a lane per row with the columns in registers: the columns of a row are
// independent in both passes, the stores of a pair's columns coalesce, and no kernel indexes a register array.
// No floating-point atomic anywhere: the same inputs give the same bits on every call.  Vector stores from plain C++
// only.  Every operation separately rounded, as NumPy's are; double where the reference has longdouble.
#include "sphx_internal.h"
#include "sphx_chem_pair.h"
#include <cstring>
#pragma clang fp contract(off)

#define CHEM_WG SPHX_CHEM_WG
#define CHEM_CHUNK 256                  // rows of a first-level partial sum of the closing correction
enum { CH_CHANGED = 0, CH_C1, CH_C2, CH_C3, CH_ROWS, CH_CORR, CH_NCOUNT = 8 };
// The counters: CH_NCOUNT totals, then CH_SLOTS copies of them a 128-byte line apart.  A wave adds to the copy of its
// workgroup - millions of clamp events a round on ONE address serialise in the L2: measured at 10^6 particles, 3.6 ms a
// round against 0.7 ms this way; chem_fold_kernel sums the copies into the totals and clears them.
#define CH_SLOTS 32
#define CH_STRIDE 16
#define CH_HEADER ((CH_SLOTS + 1) * CH_STRIDE)

// one atomic per wave and counter (every lane of the wave calls this)
__device__ __forceinline__ void chem_count(unsigned long long* counts, int which, unsigned v) {
    for (int off = warpSize / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & (warpSize - 1)) == 0 && v)
        atomicAdd(counts + (1 + (blockIdx.x & (CH_SLOTS - 1))) * CH_STRIDE + which, (unsigned long long)v);
}
// lane t < nfold: totals[first + t] = the sum of its copies, which are cleared
__global__ void chem_fold_kernel(unsigned long long* counts, int first, int nfold) {
    const int t = first + threadIdx.x;
    if ((int)threadIdx.x >= nfold) return;
    unsigned long long sum = 0;
    for (int c = 1; c <= CH_SLOTS; ++c) {
        sum += counts[c * CH_STRIDE + t];
        counts[c * CH_STRIDE + t] = 0;
    }
    counts[t] = sum;
}

struct ChemPrep {
    int n, s;
    const double *pos, *m, *mu, *T, *ptype, *fun, *mus;
    double d, m0;
    ChemRec* rec;
    double *num0, *numfin;
    int* isd;
};
__global__ __launch_bounds__(CHEM_WG) void chem_prep_kernel(ChemPrep a) {
    const int i = blockIdx.x * CHEM_WG + threadIdx.x;
    if (i >= a.n) return;
    const double m = a.m[i], type = a.ptype[i];
    ChemRec r;
    r.x = a.pos[3 * (size_t)i]; r.y = a.pos[3 * (size_t)i + 1]; r.z = a.pos[3 * (size_t)i + 2];
    r.h2 = weigh2_h2(m, a.d, a.m0);
    r.cg = weigh2_c(m, a.m0);
    r.mu = a.mu[i];
    r.T = type == 1.0 ? 2.73 : a.T[i];
    r.type = type;
    a.rec[i] = r;
    a.isd[i] = type == 2.0;
    const double* f = a.fun + (size_t)i * a.s;
    double mubase = 0.0;
    for (int t = 0; t < a.s; ++t) mubase += f[t] * a.mus[t];                 // nsc:1266
    for (int t = 0; t < a.s; ++t) {
        const double v = f[t] * m / mubase;                                  // nsc:1267
        a.num0[(size_t)i * a.s + t] = v;
        a.numfin[(size_t)i * a.s + t] = v;
    }
}

// entry e = (j, kk) of the (n,k) list
__global__ __launch_bounds__(CHEM_WG) void chem_list_kernel(int n, int npad, int k, const long long* __restrict__ nb, int* __restrict__ nbr) {
    const long long e = (long long)blockIdx.x * CHEM_WG + threadIdx.x;
    if (e >= (long long)n * k) return;
    const int j = (int)(e / k), kk = (int)(e - (long long)j * k);
    nbr[(size_t)kk * npad + j] = sphx_list_entry64(nb[e], n);
}

// what the kernels after the scan of the dust flags share
struct ChemRows {
    int n, npad, k, s, ns, nd, ndpad;
    const int *nbr, *isd, *ord;         // K-major list; dust flag; ordinal of a dust particle (exclusive scan of isd)
    int *dustid, *contrib;              // (ndpad): the particle of an ordinal; whether the row contributes
    const ChemRec* rec;
    const double *fun, *num0, *sizes, *m;
    ChemTab tab;
    double d9;
    double *wg, *wk;                    // (k, ndpad): gas weight, reuptake weight of entry kk of ordinal a at kk ndpad + a
    double *tsph, *scd3, *scd4, *selfw; // (ndpad)
    double *new0;                       // (ndpad, ns)
    double *sumc0, *new20;              // round 0's "previous" sums: the unclamped new0
    unsigned long long* counts;
};

__global__ __launch_bounds__(CHEM_WG) void chem_row_a_kernel(ChemRows a) {
    const int j = blockIdx.x * CHEM_WG + threadIdx.x;
    unsigned contributes = 0;
    if (j < a.n && a.isd[j]) {
        const int dj = a.ord[j];
        a.dustid[dj] = j;
        const ChemRec me = a.rec[j];
        const double mu5 = a.tab.mu[5];
        double sw = 0.0, swT = 0.0, s3 = 0.0, s4 = 0.0, A = 0.0;
        unsigned long long rp = 0;                                           // reuptake points: gas and w > 0   nsc:1336
        bool anygas = false;
        for (int kk = 0; kk < a.k; ++kk) {
            const int p = a.nbr[(size_t)kk * a.npad + j];
            double w = 0.0, rw0 = 0.0;
            if (p >= 0) {
                const ChemRec r = a.rec[p];
                if (r.type == 0.0) {
                    anygas = true;
                    w = chem_weight(r, chem_r2(r, me.x, me.y, me.z), a.d9);
                    const double* f = a.fun + (size_t)p * a.s;
                    sw += w; swT += w * r.T;                                 // nsc:1298, 1302
                    s3 += w * f[3]; s4 += w * f[4];
                    if (w > 0.0) {
                        rp |= 1ull << kk;
                        rw0 = w * f[5] * mu5;                                // the He++ column                nsc:1338
                        A += rw0;
                    }
                }
            }
            a.wg[(size_t)kk * a.ndpad + dj] = w;
            a.wk[(size_t)kk * a.ndpad + dj] = rw0;
        }
        contributes = anygas && sw > 0.0;                                    // nsc:1274, 1298
        a.contrib[dj] = (int)contributes;
        if (contributes) {
            a.tsph[dj] = swT / sw;
            a.scd3[dj] = s3 * a.tab.mu[3];
            a.scd4[dj] = s4 * a.tab.mu[4];
            const double sz = a.sizes[j], q = sz * sz - 0.0;
            a.selfw[dj] = a.m[j] * 315.0 * (q * q * q) / (PI64 * pow9(sz)); // Weigh2_dust(x, x, ...)          nsc:1296
            // the weight is normalised, normalised again, its NaNs filled, and normalised once more        nsc:1345-1363
            double B = 0.0, tot = 0.0, C = 0.0;
            for (int kk = 0; kk < a.k; ++kk)
                if ((rp >> kk) & 1ull) B += a.wk[(size_t)kk * a.ndpad + dj] / A;
            for (int kk = 0; kk < a.k; ++kk)
                if ((rp >> kk) & 1ull) tot += sphx_nan_to_num(a.wk[(size_t)kk * a.ndpad + dj] / A / B);
            tot = tot * (double)a.ns;                                        // the same number in every column >= 6
            const double fill = tot < 1e-15 ? 1.0 / (double)__popcll(rp) : 0.0;
            for (int kk = 0; kk < a.k; ++kk)
                if ((rp >> kk) & 1ull) {
                    const double v = a.wk[(size_t)kk * a.ndpad + dj] / A / B;
                    C += v != v ? fill : v;
                }
            for (int kk = 0; kk < a.k; ++kk)
                if ((rp >> kk) & 1ull) {
                    double v = a.wk[(size_t)kk * a.ndpad + dj] / A / B;
                    if (v != v) v = fill;
                    a.wk[(size_t)kk * a.ndpad + dj] = sphx_nan_to_num(v / C);
                }
        }
    }
    chem_count(a.counts, CH_ROWS, contributes);
}

// lane t = (ordinal, column CHEM_FIRST + si)
__global__ __launch_bounds__(CHEM_WG) void chem_row_b_kernel(ChemRows a) {
    const long long t = (long long)blockIdx.x * CHEM_WG + threadIdx.x;
    if (t >= (long long)a.nd * a.ns) return;
    const int dj = (int)(t / a.ns), si = (int)(t - (long long)dj * a.ns), s = CHEM_FIRST + si;
    double v = 0.0;
    if (a.contrib[dj]) {
        const int j = a.dustid[dj];
        double acc = 0.0;
        for (int kk = 0; kk < a.k; ++kk) {                                   // list order                       nsc:1300
            const double w = a.wg[(size_t)kk * a.ndpad + dj];
            if (w == 0.0) continue;                                          // (adds nothing; a non-gas or missing entry)
            acc += w * a.fun[(size_t)a.nbr[(size_t)kk * a.npad + j] * a.s + s];
        }
        const double mus = a.tab.mu[s];
        const double dc = a.selfw[dj] * a.fun[(size_t)j * a.s + s] * mus;    // nsc:1303
        const double F = chem_fsput(a.tab, s, acc * mus, a.scd3[dj], a.scd4[dj], dc, a.tsph[dj]);
        v = (F - 1.0) * a.num0[(size_t)j * a.s + s];                         // nsc:1374
    }
    a.new0[t] = v; a.sumc0[t] = v; a.new20[t] = v;
}

// the pairs that exist: a contributing row's gas entry
__device__ __forceinline__ int chem_pair_of(const ChemRows& a, long long e, int& dj, int& kk) {
    kk = (int)(e / a.ndpad); dj = (int)(e - (long long)kk * a.ndpad);
    if (dj >= a.nd || !a.contrib[dj]) return -1;
    const int p = a.nbr[(size_t)kk * a.npad + a.dustid[dj]];
    return (p >= 0 && a.rec[p].type == 0.0) ? p : -1;
}
__global__ __launch_bounds__(CHEM_WG) void chem_count_kernel(ChemRows a, int* cnt) {
    const long long e = (long long)blockIdx.x * CHEM_WG + threadIdx.x;
    if (e >= (long long)a.k * a.ndpad) return;
    int dj, kk;
    const int p = chem_pair_of(a, e, dj, kk);
    if (p >= 0) atomicAdd(&cnt[p], 1);
}
// slice of gas particle p: the keys ordinal k + kk of the pairs that hold it, in the order the atomics hand out (sorted afterwards)
__global__ __launch_bounds__(CHEM_WG) void chem_fill_kernel(ChemRows a, const int* __restrict__ start, int* cur, int* __restrict__ rev) {
    const long long e = (long long)blockIdx.x * CHEM_WG + threadIdx.x;
    if (e >= (long long)a.k * a.ndpad) return;
    int dj, kk;
    const int p = chem_pair_of(a, e, dj, kk);
    if (p >= 0) rev[start[p] + atomicAdd(&cur[p], 1)] = dj * a.k + kk;
}
__global__ __launch_bounds__(CHEM_WG) void chem_pos_kernel(int M, int k, int ndpad, const int* __restrict__ rev, int* __restrict__ pos) {
    const int u = blockIdx.x * CHEM_WG + threadIdx.x;
    if (u >= M) return;
    const int key = rev[u], dj = key / k, kk = key - dj * k;
    pos[(size_t)kk * ndpad + dj] = u;
}

struct ChemRound {
    int n, npad, k, s, ns, nd, ndpad;
    const int *nbr, *ord, *dustid, *contrib, *start, *rev, *pos;
    const ChemRec* rec;
    const double *num0, *wk, *new0;
    const double *sumc_prev, *new2_prev;     // (ndpad, ns)
    double *sumc, *new2;
    double* first;                           // (M, ns): the clamped first-stage loss of pair u, column si at u ns + si
    double* numfin;                          // (n, s)
    unsigned long long* counts;
};

// lane t = (particle g, column CHEM_FIRST + si)
__global__ __launch_bounds__(CHEM_WG) void chem_gas_kernel(ChemRound a) {
    const long long t = (long long)blockIdx.x * CHEM_WG + threadIdx.x;
    unsigned c1 = 0, c2 = 0;
    if (t < (long long)a.n * a.ns) {
        const int g = (int)(t / a.ns), si = (int)(t - (long long)g * a.ns);
        const int u0 = a.start[g], u1 = a.start[g + 1];
        if (u1 > u0) {
            const size_t at = (size_t)g * a.s + CHEM_FIRST + si;
            double cnt = a.num0[at];
            for (int u = u0; u < u1; ++u) {                                  // ascending (row, kk): the reference's loop order
                const int key = a.rev[u];
                const int dj = key / a.k, kk = key - dj * a.k;
                const double w = a.wk[(size_t)kk * a.ndpad + dj];
                const size_t row = (size_t)dj * a.ns + si;
                a.first[(size_t)u * a.ns + si] = chem_clamp12(cnt, a.new0[row] * w, c1, c2);   // nsc:1377-1384
                cnt = cnt + sphx_nan_to_num(-(a.sumc_prev[row] * w));        // nsc:1388, 1393
            }
            a.numfin[at] = cnt;
        }
    }
    chem_count(a.counts, CH_C1, c1); chem_count(a.counts, CH_C2, c2);
}

// lane t = (ordinal, column CHEM_FIRST + si)
__global__ __launch_bounds__(CHEM_WG) void chem_dust_kernel(ChemRound a) {
    const long long t = (long long)blockIdx.x * CHEM_WG + threadIdx.x;
    unsigned c1 = 0, c2 = 0, c3 = 0, changed = 0;
    if (t < (long long)a.nd * a.ns) {
        const int dj = (int)(t / a.ns), si = (int)(t - (long long)dj * a.ns), s = CHEM_FIRST + si;
        if (a.contrib[dj]) {
            const int j = a.dustid[dj];
            double tot = 0.0;
            for (int kk = 0; kk < a.k; ++kk) {                               // list order: np.sum(ploss, axis=0)  nsc:1386
                const int p = a.nbr[(size_t)kk * a.npad + j];
                if (p < 0) continue;
                const double type = a.rec[p].type;
                if (type == 0.0) {
                    tot += a.first[(size_t)a.pos[(size_t)kk * a.ndpad + dj] * a.ns + si];
                } else {                                                     // loss 0: only a negative count acts
                    double cnt = a.num0[(size_t)p * a.s + s];
                    if (type == 2.0 && p < j) {
                        const int dp = a.ord[p];
                        if (a.contrib[dp]) cnt = cnt + a.new2_prev[(size_t)dp * a.ns + si];   // nsc:1395
                    }
                    tot += chem_clamp12(cnt, 0.0, c1, c2);
                }
            }
            const double own = a.num0[(size_t)j * a.s + s];
            tot = chem_clamp3(own, tot, c3);
            double got = 0.0;
            for (int kk = 0; kk < a.k; ++kk) {                               // nsc:1388-1389
                const double w = a.wk[(size_t)kk * a.ndpad + dj];
                if (w == 0.0) continue;                                      // (0 or NaN: nan_to_num gives 0)
                got += sphx_nan_to_num(tot * w);
            }
            changed = __double_as_longlong(tot) != __double_as_longlong(a.sumc_prev[t]) ||
                      __double_as_longlong(got) != __double_as_longlong(a.new2_prev[t]);
            a.sumc[t] = tot; a.new2[t] = got;
            a.numfin[(size_t)j * a.s + s] = own + got;                       // nsc:1395
        } else {
            a.sumc[t] = a.sumc_prev[t]; a.new2[t] = a.new2_prev[t];
        }
    }
    chem_count(a.counts, CH_C1, c1); chem_count(a.counts, CH_C2, c2); chem_count(a.counts, CH_C3, c3);
    chem_count(a.counts, CH_CHANGED, changed);
}

// ---- the closing correction (nsc:1400-1409) ----
// lane t = (chunk c of CHEM_CHUNK rows, column s): the sums of the positive and of the negative counts, in row order
__global__ __launch_bounds__(CHEM_WG) void chem_colsum_kernel(int n, int s, int nchunk, const double* __restrict__ num, double* __restrict__ part) {
    const long long t = (long long)blockIdx.x * CHEM_WG + threadIdx.x;
    if (t >= (long long)nchunk * s) return;
    const int c = (int)(t / s), col = (int)(t - (long long)c * s);
    const int i1 = min(n, (c + 1) * CHEM_CHUNK);
    double pos = 0.0, neg = 0.0;
    for (int i = c * CHEM_CHUNK; i < i1; ++i) {
        const double v = num[(size_t)i * s + col];
        if (v > 0.0) pos += v;
        if (v < 0.0) neg += v;
    }
    part[2 * t] = pos; part[2 * t + 1] = neg;
}
// one workgroup per column: lane l adds the chunks l, l + CHEM_WG, ... in order, then a tree over the lanes
__global__ __launch_bounds__(CHEM_WG) void chem_colfac_kernel(int s, int nchunk, const double* __restrict__ part, double* __restrict__ fac,
                                                              unsigned long long* counts) {
    __shared__ double sp[CHEM_WG], sn[CHEM_WG];
    const int col = blockIdx.x, l = threadIdx.x;
    double pos = 0.0, neg = 0.0;
    for (int c = l; c < nchunk; c += CHEM_WG) {
        pos += part[2 * ((size_t)c * s + col)];
        neg += part[2 * ((size_t)c * s + col) + 1];
    }
    sp[l] = pos; sn[l] = neg;
    __syncthreads();
    for (int h = CHEM_WG / 2; h > 0; h >>= 1) {
        if (l < h) { sp[l] += sp[l + h]; sn[l] += sn[l + h]; }
        __syncthreads();
    }
    if (l == 0) {
        const bool fix = sn[0] < 0.0;                                        // nsc:1404
        fac[2 * col] = fix ? 1.0 : 0.0;
        fac[2 * col + 1] = 1.0 + sn[0] / sp[0];                              // nsc:1406
        if (fix) atomicAdd(counts + CH_CORR, 1ull);
    }
}
__device__ __forceinline__ double chem_fixed(double v, const double* __restrict__ fac, int t) {
    if (fac[2 * t] != 0.0) {
        if (v < 0.0) v = 0.0;
        if (v > 0.0) v = v * fac[2 * t + 1];
    }
    return v;
}
__global__ __launch_bounds__(CHEM_WG) void chem_final_kernel(int n, int s, const double* __restrict__ num, const double* __restrict__ fac,
                                                             const double* __restrict__ mus, double* __restrict__ mass_new,
                                                             double* __restrict__ fun_new) {
    const int i = blockIdx.x * CHEM_WG + threadIdx.x;
    if (i >= n) return;
    const double* v = num + (size_t)i * s;
    double mass = 0.0, tot = 0.0;
    for (int t = 0; t < s; ++t) {
        const double c = chem_fixed(v[t], fac, t);
        mass += c * mus[t];                                                  // nsc:1408
        tot += c;
    }
    mass_new[i] = mass;
    for (int t = 0; t < s; ++t) fun_new[(size_t)i * s + t] = chem_fixed(v[t], fac, t) / tot;   // nsc:1409
}

// =====================================================================================================================
// host side: three parts (as sphx_rad.hip's rad_stage_host / rad_run) - the tables and the host inputs staged
// (sphx_chem_tables, chem_stage_host), the run on device inputs (sphx_chem_run: sphx_state_dust_phase calls it on the
// gathered resident state and leaves the outputs where they are), the outputs brought back.
// =====================================================================================================================

// the range checks every caller shares: the shape, then (behind the callers' NULL checks) the scalars
int sphx_chem_check_shape(sphx_ctx* ctx, const char* who, int64_t n, int k, int s) {
    if (n < 1 || k < 1 || k > 64 || s < CHEM_FIRST + 1 || s > SPHX_MAX_SPECIES)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld, k=%d, s=%d (need n >= 1, 1 <= k <= 64, %d <= s <= %d)", who, (long long)n, k, s,
                            CHEM_FIRST + 1, SPHX_MAX_SPECIES);
    if (n > 0x7FFFFFF0ll || sphx_pad64(n) * (int64_t)k > 0x7FFFFFF0ll)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld x k=%d out of range", who, (long long)n, k);
    return SPHX_OK;
}
int sphx_chem_check_scalars(sphx_ctx* ctx, const char* who, double d, double dt, const double mrn[2], double k_B, double amu,
                            double m_0) {
    if (!sphx_finite(d) || !sphx_finite(dt) || !sphx_finite(k_B) || !sphx_finite(amu) || !sphx_finite(m_0) || !sphx_finite(mrn[0]) ||
        !sphx_finite(mrn[1]))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: d=%g, dt=%g, k_B=%g, amu=%g, m_0=%g, mrn=(%g, %g) must be finite", who, d, dt, k_B, amu,
                            m_0, mrn[0], mrn[1]);
    return SPHX_OK;
}

// the tables mu_specie | j0 | b | sputtering_yields, s entries each, into ctx->chem_tab (held by the context: the upload reads it)
int sphx_chem_tables(sphx_ctx* ctx, const char* who, int s, const double* mu_specie, const double* mineral_densities,
                     const double* sputtering_yields, const double mrn[2], double amu, double* symax_out) {
    double* tab = ctx->chem_tab;
    const double c0 = -(pow(mrn[1], -0.5) - pow(mrn[0], -0.5)) / (pow(mrn[1], 0.5) - pow(mrn[0], 0.5));   // nsc:1305
    double symax = sputtering_yields[0];
    for (int t = 0; t < s; ++t) {
        if (!sphx_finite(mu_specie[t]) || !sphx_finite(mineral_densities[t]) || !sphx_finite(sputtering_yields[t]))
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: table entry %d must be finite", who, t);
        tab[t] = mu_specie[t];
        tab[s + t] = c0 / (3.0 * mineral_densities[t]);
        tab[2 * s + t] = 2.0 * 3.141592653589793 * mu_specie[t] * amu;      // nsc:1306
        tab[3 * s + t] = sputtering_yields[t];
        if (sputtering_yields[t] > symax) symax = sputtering_yields[t];
    }
    *symax_out = symax;
    return SPHX_OK;
}

// ints per particle: nbr (k npad, the K-major list's place) | isd | ord | cnt | cur | start (n + 1 each, on 16-byte boundaries)
int sphx_chem_ints(sphx_ctx* ctx, int64_t n, int k, ChemInts* out) {
    const size_t nn = (size_t)n, npad = (size_t)sphx_pad64(n);
    Carve c;
    c.take(out->nbr, (size_t)k * npad);
    c.take(out->isd, nn + 1, 16); c.take(out->ord, nn + 1, 16); c.take(out->cnt, nn + 1, 16); c.take(out->cur, nn + 1, 16);
    c.take(out->start, nn + 1, 16);
    c.pad(16);
    c.take(out->end, 0);
    return sphx_carve_into(ctx, ctx->chem_int, c);
}

// inputs in ctx->chem_in: points (3n) | mass | mu | sizes | T | ptype (n each) | f_un (n s) | the tables (4 s)
int sphx_chem_inputs(sphx_ctx* ctx, int64_t n, int s, ChemDev* in) {
    const size_t nn = (size_t)n;
    Carve c;
    c.take(in->pos, 3 * nn); c.take(in->m, nn); c.take(in->mu, nn); c.take(in->sizes, nn); c.take(in->T, nn); c.take(in->ptype, nn);
    c.take(in->fun, nn * (size_t)s); c.take(in->tab, 4 * (size_t)s);
    return sphx_carve_into(ctx, ctx->chem_in, c);
}

// the host arrays and the (n,k) int64 list onto the device; the list into its K-major int32 form
static int chem_stage_host(sphx_ctx* ctx, int64_t n, int k, int s, const double* points, const int64_t* neighbor, const double* mass,
                           const double* f_un, const double* mu, const double* sizes, const double* T, const double* ptype,
                           ChemDev* in, int** nbr_out) {
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)n, npad = (size_t)sphx_pad64(n), ns_ = nn * (size_t)s, nk = nn * (size_t)k;
    SPHX_TRY(sphx_chem_inputs(ctx, n, s, in));
    SPHX_TRY(sphx_ensure(ctx, ctx->chem_nb, nk * sizeof(int64_t)));
    const CopyF64 us[] = {{points, in->pos, 3 * nn}, {mass, in->m, nn}, {mu, in->mu, nn}, {sizes, in->sizes, nn}, {T, in->T, nn},
                          {ptype, in->ptype, nn}, {f_un, in->fun, ns_}, {ctx->chem_tab, in->tab, 4 * (size_t)s}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 8));
    HIPCHK(hipMemcpyAsync(ctx->chem_nb.p, neighbor, nk * sizeof(int64_t), hipMemcpyHostToDevice, st));
    ChemInts ci;
    SPHX_TRY(sphx_chem_ints(ctx, n, k, &ci));
    hipLaunchKernelGGL(chem_list_kernel, dim3(sphx_blocks(nk, CHEM_WG)), dim3(CHEM_WG), 0, st, (int)n, (int)npad, k,
                       (const long long*)ctx->chem_nb.p, ci.nbr);
    HIPCHK(hipGetLastError());
    *nbr_out = ci.nbr;
    return SPHX_OK;
}

// The middle part: everything between the inputs on the device (in; the K-major list nbr, which may lie anywhere) and
// mass_new / f_un_new on the device (res).  t: the caller's stage timer, marks 1 .. 4 (NULL: none).  The counters 4 .. 7
// are on their way into ctx->pinned->side.red when this returns: sphx_chem_counts after the caller's next synchronise.
int sphx_chem_run(sphx_ctx* ctx, const char* who, int64_t n, int k, int s, const ChemDev& in, const int* nbr, const ChemPar& par,
                  StageTimer* t, ChemRes* res) {
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)n, npad = (size_t)sphx_pad64(n), ns_ = nn * (size_t)s;
    const int ns = s - CHEM_FIRST;
    const double *d_pos = in.pos, *d_m = in.m, *d_mu = in.mu, *d_sz = in.sizes, *d_T = in.T, *d_pt = in.ptype, *d_fun = in.fun,
                 *d_tab = in.tab;
    const double d = par.d;
    // ---- records, num0, the dust rows' ordinals ----
    SPHX_TRY(sphx_ensure(ctx, ctx->chem_rec, nn * sizeof(ChemRec)));
    const size_t nchunk = (nn + CHEM_CHUNK - 1) / CHEM_CHUNK;
    // per particle: counters (CH_HEADER u64) | num0 (n s) | numfin (n s) | mass_new (n) | f_un_new (n s) | partial sums (2 nchunk s) | factors (2 s)
    unsigned long long* d_cnt;
    double *num0, *numfin, *d_mass, *d_fnew, *part, *fac;
    Carve co;
    co.take(d_cnt, CH_HEADER); co.take(num0, ns_); co.take(numfin, ns_); co.take(d_mass, nn); co.take(d_fnew, ns_);
    co.take(part, 2 * nchunk * (size_t)s); co.take(fac, 2 * (size_t)s);
    SPHX_TRY(sphx_carve_into(ctx, ctx->chem_out, co));
    HIPCHK(hipMemsetAsync(d_cnt, 0, CH_HEADER * sizeof(double), st));
    // ints (sphx_chem_ints): isd | ord | cnt | cur | start behind the list's place
    ChemInts ci;
    SPHX_TRY(sphx_chem_ints(ctx, n, k, &ci));
    int *isd = ci.isd, *ord = ci.ord, *cnt = ci.cnt, *cur = ci.cur, *start = ci.start;
    HIPCHK(hipMemsetAsync(isd, 0, (size_t)(ci.end - isd) * sizeof(int), st));
    ChemPrep pa;
    pa.n = (int)n; pa.s = s; pa.pos = d_pos; pa.m = d_m; pa.mu = d_mu; pa.T = d_T; pa.ptype = d_pt; pa.fun = d_fun; pa.mus = d_tab;
    pa.d = d; pa.m0 = par.m_0; pa.rec = ctx->chem_rec.as<ChemRec>(); pa.num0 = num0; pa.numfin = numfin; pa.isd = isd;
    const unsigned nblk = sphx_blocks(nn, CHEM_WG);
    hipLaunchKernelGGL(chem_prep_kernel, dim3(nblk), dim3(CHEM_WG), 0, st, pa);
    HIPCHK(hipGetLastError());
    SPHX_TRY(sphx_excl_scan_int(ctx, isd, ord, (int)n));                 // (isd[n] = 0: the memset above; both start on 16-byte boundaries)
    HIPCHK(hipMemcpyAsync(&ctx->pinned->side.count, ord + n, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const size_t nd = (size_t)ctx->pinned->side.count;
    if (nd > nn) return sphx_set_err(ctx, SPHX_E_HIP, "%s: %zu dust rows of %zu particles", who, nd, nn);
    if (t) SPHX_TRY(t->mark(ctx, 1));
    unsigned long long* hc = res->hc;
    for (int q = 0; q < CH_NCOUNT; ++q) hc[q] = 0;
    size_t M = 0;
    int64_t rounds = 0;
    if (nd > 0) {
        // ---- the row passes ----
        const size_t ndpad = (size_t)sphx_pad64((int64_t)nd), row = ndpad * (size_t)ns;
        // per dust row: wg, wk (k ndpad each) | tsph, scd3, scd4, selfw (ndpad each) | new0, sumc x 2, new2 x 2 (ndpad ns each)
        ChemRows ra;
        double *sumc[2], *new2[2];
        Carve cr;
        cr.take(ra.wg, (size_t)k * ndpad); cr.take(ra.wk, (size_t)k * ndpad);
        cr.take(ra.tsph, ndpad); cr.take(ra.scd3, ndpad); cr.take(ra.scd4, ndpad); cr.take(ra.selfw, ndpad);
        cr.take(ra.new0, row); cr.take(sumc[0], row); cr.take(sumc[1], row); cr.take(new2[0], row); cr.take(new2[1], row);
        SPHX_TRY(sphx_carve_into(ctx, ctx->chem_row, cr));
        // ints per dust row: dustid, contrib (ndpad each) | pos (k ndpad)
        int* pos;
        Carve cri;
        cri.take(ra.dustid, ndpad); cri.take(ra.contrib, ndpad); cri.take(pos, (size_t)k * ndpad);
        SPHX_TRY(sphx_carve_into(ctx, ctx->chem_rowi, cri));
        ra.n = (int)n; ra.npad = (int)npad; ra.k = k; ra.s = s; ra.ns = ns; ra.nd = (int)nd; ra.ndpad = (int)ndpad;
        ra.nbr = nbr; ra.isd = isd; ra.ord = ord;
        HIPCHK(hipMemsetAsync(ra.dustid, 0, (size_t)(pos - ra.dustid) * sizeof(int), st));
        ra.rec = pa.rec; ra.fun = d_fun; ra.num0 = num0; ra.sizes = d_sz; ra.m = d_m;
        ra.tab.mu = d_tab; ra.tab.j0 = d_tab + s; ra.tab.b = d_tab + 2 * s; ra.tab.sy = d_tab + 3 * s;
        ra.tab.symax = par.symax; ra.tab.kB = par.k_B; ra.tab.dt = par.dt;
        const double d2 = d * d, d4 = d2 * d2;
        ra.d9 = d4 * d4 * d;
        ra.sumc0 = sumc[0]; ra.new20 = new2[0];
        ra.counts = d_cnt;
        const unsigned rblk = sphx_blocks(nd * (size_t)ns, CHEM_WG);
        hipLaunchKernelGGL(chem_row_a_kernel, dim3(nblk), dim3(CHEM_WG), 0, st, ra);
        hipLaunchKernelGGL(chem_row_b_kernel, dim3(rblk), dim3(CHEM_WG), 0, st, ra);
        hipLaunchKernelGGL(chem_fold_kernel, dim3(1), dim3(64), 0, st, d_cnt, (int)CH_ROWS, 1);
        HIPCHK(hipGetLastError());
        if (t) SPHX_TRY(t->mark(ctx, 2));
        // ---- the reverse list: count; scan, fill and sort of keys ordinal k + kk (sphx_rev_build); positions ----
        const unsigned eblk = sphx_blocks((size_t)k * ndpad, CHEM_WG);
        hipLaunchKernelGGL(chem_count_kernel, dim3(eblk), dim3(CHEM_WG), 0, st, ra, cnt);
        HIPCHK(hipGetLastError());
        // (the row counter rides on the builder's synchronise)
        HIPCHK(hipMemcpyAsync(ctx->pinned->side.red, d_cnt + CH_ROWS - CH_ROWS % 4, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
        RevList rl;
        SPHX_TRY(sphx_rev_build(ctx, who, n, cnt, start, (size_t)k * nd, (unsigned long long)nd * (unsigned long long)k,
                                [&](const int* start_, int* rev_raw) {
                                    hipLaunchKernelGGL(chem_fill_kernel, dim3(eblk), dim3(CHEM_WG), 0, st, ra, start_, cur, rev_raw);
                                }, &rl));
        M = rl.M;
        std::memcpy(hc + CH_ROWS - CH_ROWS % 4, ctx->pinned->side.red, 4 * sizeof(double));
        if (M > 0) {
            SPHX_TRY(sphx_ensure(ctx, ctx->chem_first, M * (size_t)ns * sizeof(double)));
            const int* rev = rl.rev;
            hipLaunchKernelGGL(chem_pos_kernel, dim3(sphx_blocks(M, CHEM_WG)), dim3(CHEM_WG), 0, st, (int)M, k, (int)ndpad, rev, pos);
            HIPCHK(hipGetLastError());
            if (t) SPHX_TRY(t->mark(ctx, 3));
            // ---- the rounds: until one changes no bit; (contributing rows + 1) always suffice ----
            ChemRound wa;
            wa.n = (int)n; wa.npad = (int)npad; wa.k = k; wa.s = s; wa.ns = ns; wa.nd = (int)nd; wa.ndpad = (int)ndpad;
            wa.nbr = nbr; wa.ord = ord; wa.dustid = ra.dustid; wa.contrib = ra.contrib; wa.start = start; wa.rev = rev; wa.pos = pos;
            wa.rec = pa.rec; wa.num0 = num0; wa.wk = ra.wk; wa.new0 = ra.new0;
            wa.first = ctx->chem_first.as<double>(); wa.numfin = numfin; wa.counts = d_cnt;
            const unsigned gblk = sphx_blocks(nn * (size_t)ns, CHEM_WG);
            const int64_t limit = (int64_t)hc[CH_ROWS] + 1;
            for (;;) {
                const int a = (int)(rounds & 1);
                wa.sumc_prev = sumc[a]; wa.new2_prev = new2[a]; wa.sumc = sumc[a ^ 1]; wa.new2 = new2[a ^ 1];
                hipLaunchKernelGGL(chem_gas_kernel, dim3(gblk), dim3(CHEM_WG), 0, st, wa);
                hipLaunchKernelGGL(chem_dust_kernel, dim3(rblk), dim3(CHEM_WG), 0, st, wa);
                hipLaunchKernelGGL(chem_fold_kernel, dim3(1), dim3(64), 0, st, d_cnt, (int)CH_CHANGED, 4);
                HIPCHK(hipGetLastError());
                HIPCHK(hipMemcpyAsync(ctx->pinned->side.red, d_cnt, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                std::memcpy(hc, ctx->pinned->side.red, 4 * sizeof(double));
                ++rounds;
                if (hc[CH_CHANGED] == 0 || rounds >= limit) break;
            }
        } else {
            if (t) SPHX_TRY(t->mark(ctx, 3));
        }
    } else {
        if (t) SPHX_TRY(t->mark(ctx, 2));
        if (t) SPHX_TRY(t->mark(ctx, 3));
    }
    if (t) SPHX_TRY(t->mark(ctx, 4));
    // ---- the closing correction, the outputs ----
    hipLaunchKernelGGL(chem_colsum_kernel, dim3(sphx_blocks(nchunk * (size_t)s, CHEM_WG)), dim3(CHEM_WG), 0, st, (int)n, s,
                       (int)nchunk, numfin, part);
    hipLaunchKernelGGL(chem_colfac_kernel, dim3((unsigned)s), dim3(CHEM_WG), 0, st, s, (int)nchunk, part, fac, d_cnt);
    hipLaunchKernelGGL(chem_final_kernel, dim3(nblk), dim3(CHEM_WG), 0, st, (int)n, s, numfin, fac, d_tab, d_mass, d_fnew);
    HIPCHK(hipGetLastError());
    res->mass_new = d_mass; res->fun_new = d_fnew; res->M = M; res->rounds = rounds;
    res->counters = d_cnt;
    return SPHX_OK;
}

// counts[7] as sphx_chemisputtering_2 defines them; after the synchronise behind the copy of res.counters + 4 into
// ctx->pinned->side.red
void sphx_chem_counts(sphx_ctx* ctx, ChemRes* res, int64_t* counts) {
    unsigned long long* hc = res->hc;
    std::memcpy(hc + 4, ctx->pinned->side.red, 4 * sizeof(double));
    if (counts) {
        counts[0] = (int64_t)hc[CH_ROWS]; counts[1] = (int64_t)res->M; counts[2] = (int64_t)hc[CH_C1]; counts[3] = (int64_t)hc[CH_C2];
        counts[4] = (int64_t)hc[CH_C3]; counts[5] = (int64_t)hc[CH_CORR]; counts[6] = res->rounds;
    }
}

extern "C" int sphx_chemisputtering_2(sphx_ctx* ctx, int64_t n, int k, int s, const double* points, const int64_t* neighbor,
                                      const double* mass, const double* f_un, const double* mu, const double* sizes, const double* T,
                                      const double* ptype, double d, double dt, const double* mu_specie, const double* mineral_densities,
                                      const double* sputtering_yields, const double mrn[2], double k_B, double amu, double m_0,
                                      double* mass_new, double* f_un_new, int64_t* counts) {
    if (!ctx) return SPHX_E_ARG;
    SPHX_TRY(sphx_chem_check_shape(ctx, "sphx_chemisputtering_2", n, k, s));
    NEED(points); NEED(neighbor); NEED(mass); NEED(f_un); NEED(mu); NEED(sizes); NEED(T); NEED(ptype);
    NEED(mu_specie); NEED(mineral_densities); NEED(sputtering_yields); NEED(mrn); NEED(mass_new); NEED(f_un_new);
    SPHX_TRY(sphx_chem_check_scalars(ctx, "sphx_chemisputtering_2", d, dt, mrn, k_B, amu, m_0));
    ChemPar par;
    par.d = d; par.dt = dt; par.k_B = k_B; par.m_0 = m_0;
    SPHX_TRY(sphx_chem_tables(ctx, "sphx_chemisputtering_2", s, mu_specie, mineral_densities, sputtering_yields, mrn, amu, &par.symax));
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->chem_t.begin(ctx));
    ChemDev in;
    int* nbr;
    SPHX_TRY(chem_stage_host(ctx, n, k, s, points, neighbor, mass, f_un, mu, sizes, T, ptype, &in, &nbr));
    ChemRes res;
    SPHX_TRY(sphx_chem_run(ctx, "sphx_chemisputtering_2", n, k, s, in, nbr, par, &ctx->chem_t, &res));
    const CopyF64 ds[] = {{mass_new, res.mass_new, (size_t)n}, {f_un_new, res.fun_new, (size_t)n * (size_t)s}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 2));
    HIPCHK(hipMemcpyAsync(ctx->pinned->side.red, res.counters + 4, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SPHX_TRY(ctx->chem_t.mark(ctx, 5));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    sphx_chem_counts(ctx, &res, counts);
    return ctx->chem_t.end(ctx);
}
