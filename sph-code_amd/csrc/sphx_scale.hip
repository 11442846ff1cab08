// sphx_scale.hip - the closing block of the reference's time loop, code_running.py:493-540: the global length scale d
// from the 90th percentile of |x|^2 over the slow rows (sphx_length_scale), the gas rows' sizes adapted to the change of
// their density and capped at d, the dust rows set to d / raise_factor^(1/3) (sphx_adapt_sizes), and both on the resident
// state (sphx_state_length_scale).  include/sphx.h has the definition; here the route to it:
//   keys      |x|^2 of every slow row as a 64-bit key (the bits of a non-negative double order as unsigned integers; a
//             NaN is SCALE_KEY_NAN, above +inf; a row that is not slow is SCALE_KEY_OUT, the only keys with bit 63 set,
//             and no later kernel counts it).  NaN keys are counted by ballot, one integer atomic per wave.
//   select    the key of rank lo by a radix histogram, EIGHT BITS A LEVEL, ALWAYS EIGHT LEVELS (no early stop: sixteen
//             small launches, no branch on the host): scale_hist_kernel counts the rows under the prefix found so far by
//             the next eight bits (LDS per workgroup, then one global add per non-empty bin - integer atomics only, the
//             same bins on every run and for every grid), scale_choose_kernel - ONE workgroup - scans the 256 bins, picks
//             the bin that holds the rank, and writes prefix, mask and the remaining rank to device scalars that the next
//             level's kernel reads.  The kernel boundary on the stream is the only synchronisation: no flag, no fence, no
//             host wait between levels.  The first level's total is M, from which lo and hi are formed in double as
//             NumPy forms them.  The last level's bin is ONE key: where rank hi falls among its duplicates b = a;
//             otherwise scale_next_kernel takes the smallest slow key above a with an integer atomicMin (LDS, then one
//             per workgroup).  ONE read-back of the scalars (M, n_nan, lo, hi, a, b) ends the selection.
//   finish    the lerp and the two pow calls in host C, in NumPy's order (sphx_length_scale_finish; needs no device)
//   counts    exp_neighbor_count by integer global atomics straight from the list, num_nontrivial per row
//   adapt     one elementwise kernel; d and d / raise_factor^(1/3) arrive as scalars
// On the resident state nothing is gathered into upload order: the keys do not depend on the row order, the counts and the
// kernel work in storage slots (the step's own K-major list, st.hprev, ctx->rho), densities_0 is reached through st.id.
// No floating-point atomic anywhere.  Vector stores from plain C++ only.  Every operation separately rounded.
#include "sphx_internal.h"
#include "sphx_phase_map.h"
#include <cstring>
#pragma clang fp contract(off)

#define SCALE_WG 256
#define SCALE_BINS 256
static_assert(SCALE_BINS == SCALE_WG, "scale_hist_kernel, scale_choose_kernel: a lane per bin");
#define SCALE_KEY_NAN 0x7FFFFFFFFFFFFFFFull
#define SCALE_KEY_OUT 0xFFFFFFFFFFFFFFFFull
#define SCALE_MAX_BLOCKS 1024u
// device scalars (u64) behind the histogram
enum { SS_PREFIX = 0, SS_MASK, SS_RANK, SS_M, SS_NNAN, SS_LO, SS_HI, SS_A, SS_B, SS_NEED, SS_BONUS, SS_CAPPED, SS_FIXED, SS_MISSING, SS_N = 16 };
static_assert(SS_N <= SC_NSLOTS, "the scalars fit the pinned scalar block");
static_assert(SS_BONUS + SPHX_SCALE_NCOUNT == SS_MISSING + 1, "the four counts lie side by side");

// flag's rows of a wave onto one counter: one integer atomic per wave that has any
__device__ __forceinline__ void scale_count(bool flag, u64* counter) {
    const u64 b = __ballot(flag);
    if (b && (threadIdx.x & (SPHX_WAVE - 1)) == (unsigned)(__ffsll((long long)b) - 1)) atomicAdd(counter, (u64)__popcll(b));
}

// drv:493, 515: the positions and velocities as three pointers and an element stride (3: (n,3) rows; 1: the state's columns)
struct ScaleKeys { int n; const double *x, *y, *z; int ps; const double *vx, *vy, *vz; int vs; double v_max2; };
__global__ __launch_bounds__(SCALE_WG) void scale_key_kernel(ScaleKeys a, u64* __restrict__ key, u64* __restrict__ scal) {
    const int i = blockIdx.x * SCALE_WG + threadIdx.x;
    bool is_nan = false;
    if (i < a.n) {
        const size_t p = (size_t)i * a.ps, q = (size_t)i * a.vs;
        const double vx = a.vx[q], vy = a.vy[q], vz = a.vz[q];
        const double vc = (vx * vx + vy * vy) + vz * vz;                     // drv:493 (NumPy's order over three columns)
        u64 kk = SCALE_KEY_OUT;
        if (vc < a.v_max2) {                                                 // (a NaN speed is not slow)
            const double x = a.x[p], y = a.y[p], z = a.z[p];
            const double s = (x * x + y * y) + z * z;                        // drv:515
            is_nan = s != s;
            kk = is_nan ? SCALE_KEY_NAN : (u64)__double_as_longlong(s);
        }
        key[i] = kk;
    }
    scale_count(is_nan, scal + SS_NNAN);
}

// the slow rows whose key agrees with the prefix under the mask (both device scalars), by the eight bits at `shift`
__global__ __launch_bounds__(SCALE_WG) void scale_hist_kernel(int n, const u64* __restrict__ key, const u64* __restrict__ scal, int shift,
                                                              u64* __restrict__ hist) {
    __shared__ unsigned hc[SCALE_BINS];
    hc[threadIdx.x] = 0u;
    __syncthreads();
    const u64 prefix = scal[SS_PREFIX], mask = scal[SS_MASK];
    for (size_t i = (size_t)blockIdx.x * SCALE_WG + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * SCALE_WG) {
        const u64 kk = key[i];
        if ((kk >> 63) || (kk & mask) != prefix) continue;
        atomicAdd(&hc[(int)((kk >> shift) & (SCALE_BINS - 1))], 1u);
    }
    __syncthreads();
    if (hc[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (u64)hc[threadIdx.x]);
}

// One workgroup, a lane per bin: the bin that holds the remaining rank; prefix, mask and the rank inside the bin for the
// next level; the bins zeroed for it.  First level (shift 56): M, lo and hi.  Last level (shift 0): a, and b where it is a.
__global__ __launch_bounds__(SCALE_WG) void scale_choose_kernel(int shift, double qf, u64* __restrict__ hist, u64* __restrict__ scal) {
    __shared__ u64 inc[SCALE_BINS];
    const int t = threadIdx.x;
    const u64 mine = hist[t];
    inc[t] = mine;
    hist[t] = 0ull;
    __syncthreads();
    for (int off = 1; off < SCALE_BINS; off <<= 1) {                         // inclusive sums over the bins
        const u64 add = t >= off ? inc[t - off] : 0ull;
        __syncthreads();
        inc[t] += add;
        __syncthreads();
    }
    u64 rank = scal[SS_RANK], span = scal[SS_HI] - scal[SS_LO];
    const u64 prefix0 = scal[SS_PREFIX], mask0 = scal[SS_MASK];
    __syncthreads();                                                         // (every lane has read the scalars: now they are written)
    if (shift == 56) {
        const u64 M = inc[SCALE_BINS - 1];
        u64 lo = 0ull, hi = 0ull;
        if (M > 0ull) {                                                      // np.percentile, method linear (include/sphx.h)
            const double last = (double)(M - 1ull), vi = last * qf;
            if (vi >= last) lo = hi = M - 1ull;
            else { lo = (u64)floor(vi); hi = lo + 1ull; }
        }
        rank = lo; span = hi - lo;
        if (t == 0) { scal[SS_M] = M; scal[SS_LO] = lo; scal[SS_HI] = hi; }
    }
    const u64 below = inc[t] - mine;
    if (mine > 0ull && below <= rank && rank < inc[t]) {                     // (one lane, or none when M = 0)
        const u64 prefix = prefix0 | ((u64)t << shift);
        scal[SS_PREFIX] = prefix;
        scal[SS_MASK] = mask0 | ((u64)(SCALE_BINS - 1) << shift);
        scal[SS_RANK] = rank - below;
        if (shift == 0) {
            const bool same = rank - below + span < mine;                    // rank hi among a's duplicates
            scal[SS_A] = prefix;
            scal[SS_B] = same ? prefix : SCALE_KEY_OUT;
            scal[SS_NEED] = same ? 0ull : 1ull;
        }
    }
}

// where b is not a: the smallest slow key above a
__global__ __launch_bounds__(SCALE_WG) void scale_next_kernel(int n, const u64* __restrict__ key, u64* __restrict__ scal) {
    if (scal[SS_NEED] == 0ull) return;
    __shared__ u64 best;
    if (threadIdx.x == 0) best = SCALE_KEY_OUT;
    __syncthreads();
    const u64 a = scal[SS_A];
    u64 m = SCALE_KEY_OUT;
    for (size_t i = (size_t)blockIdx.x * SCALE_WG + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * SCALE_WG) {
        const u64 kk = key[i];
        if (!(kk >> 63) && kk > a && kk < m) m = kk;
    }
    if (m != SCALE_KEY_OUT) atomicMin(&best, m);
    __syncthreads();
    if (threadIdx.x == 0 && best != SCALE_KEY_OUT) atomicMin(&scal[SS_B], best);
}

// drv:527-530, nsc:545 from an (n,k) int64 list, a lane per entry
__global__ __launch_bounds__(SCALE_WG) void scale_count_rows_kernel(int n, int k, const long long* __restrict__ nb, unsigned* __restrict__ rev,
                                                                    unsigned* __restrict__ nontriv, u64* __restrict__ scal) {
    const long long e = (long long)blockIdx.x * SCALE_WG + threadIdx.x;
    bool missing = false;
    if (e < (long long)n * k) {
        const int q = sphx_list_entry64(nb[e], n);
        missing = q < 0;
        if (!missing) { atomicAdd(&rev[q], 1u); atomicAdd(&nontriv[(int)(e / k)], 1u); }
    }
    scale_count(missing, scal + SS_MISSING);
}
// ... and from the step's own list (int32, K-major, storage slots, sphx_phase_map.h), a lane per column
__global__ __launch_bounds__(SCALE_WG) void scale_count_cols_kernel(int n, int npad, int k, const int* __restrict__ nbr, const int* __restrict__ qorder,
                                                                    unsigned* __restrict__ rev, unsigned* __restrict__ nontriv,
                                                                    u64* __restrict__ scal) {
    const int p = blockIdx.x * SCALE_WG + threadIdx.x;
    unsigned mine = 0u, gone = 0u;
    if (p < n) {
        for (int kk = 0; kk < k; ++kk) {
            const int q = nbr[sphx_phase_at(kk, npad, p)];
            if (q >= 0 && q < n) { atomicAdd(&rev[q], 1u); ++mine; }
            else ++gone;
        }
        nontriv[sphx_phase_slot(qorder, p)] = mine;
    }
    if (gone) atomicAdd(&scal[SS_MISSING], (u64)gone);
}

// drv:532-538, a lane per row j.  id (nullable: identity): densities_0 is read, and the caller-order outputs are written,
// at id[j]; the slot-order sizes at j.
struct ScaleAdapt {
    int n;
    const int* id;
    const unsigned *rev, *nontriv;
    const double *dens, *d0;              // d0 NULL: new_smoothing = 1. (drv:534-535)
    const double *sizes, *ptype;
    double d, d_dust;
    double *sizes_slot, *sizes_out, *smooth_out, *d0_next;     // each nullable
    long long *rev_out, *nontriv_out;                          // each nullable
};
__global__ __launch_bounds__(SCALE_WG) void scale_adapt_kernel(ScaleAdapt a, u64* __restrict__ scal) {
    const int j = blockIdx.x * SCALE_WG + threadIdx.x;
    bool bonus = false, capped = false, fixed = false;
    if (j < a.n) {
        const size_t i = a.id ? (size_t)a.id[j] : (size_t)j;
        const long long cnt = (long long)a.rev[j], nt = (long long)a.nontriv[j];
        const double s = a.sizes[j], t = a.ptype[j];
        double ns = 1.;                                                      // drv:535
        if (a.d0) {                                                          // drv:533
            const double rho = a.dens[j], rho0 = a.d0[i];
            const double x = -(rho - rho0) / (3.0 * rho);
            const double y = sphx_nan_to_num(x);
            fixed = !(y == x);
            bonus = cnt + nt - 1 < 2;
            ns = (exp(y) * 2.0) / 2. + (bonus ? 0.1 : 0.0);
        }
        double out = s;
        if (t == 0.0) {
            out = ns * s;                                                    // drv:536
            if (out > a.d) { out = a.d; capped = true; }                     // drv:537
        }
        if (t == 2.0) out = a.d_dust;                                        // drv:538
        if (a.sizes_slot) a.sizes_slot[j] = out;
        if (a.sizes_out) a.sizes_out[i] = out;
        if (a.smooth_out) a.smooth_out[i] = ns;
        if (a.rev_out) a.rev_out[i] = cnt;
        if (a.nontriv_out) a.nontriv_out[i] = nt;
        if (a.d0_next) a.d0_next[i] = a.dens[j];                             // drv:540
    }
    scale_count(bonus, scal + SS_BONUS);
    scale_count(capped, scal + SS_CAPPED);
    scale_count(fixed, scal + SS_FIXED);
}

// =====================================================================================================================
// host side
// =====================================================================================================================
static double scale_key_value(u64 kk) {
    if (kk >= SCALE_KEY_NAN) return NAN;
    double v;
    std::memcpy(&v, &kk, sizeof(v));
    return v;
}

extern "C" int sphx_length_scale_finish(int64_t n_slow, int64_t n_nan, double qf, double a, double b, double n_int, double fill,
                                        double* max_dist, double* d) {
    if (n_slow < 1 || !max_dist || !d || !(qf >= 0.0 && qf <= 1.0)) return SPHX_E_ARG;
    const double vi = (double)(n_slow - 1) * qf;
    const double lo = vi >= (double)(n_slow - 1) ? (double)(n_slow - 1) : floor(vi);
    const double g = vi - lo;
    const double diff = b - a;
    double r = a + diff * g;                                                 // _lerp
    if (g >= 0.5) r = b - diff * (1 - g);
    if (n_nan > 0) r = NAN;                                                  // (a NaN among the values: NumPy's result)
    *max_dist = r;                                                           // drv:518
    const double V_new = pow(r, 3. / 2.);                                    // drv:520
    *d = pow(V_new / (double)n_slow / fill * n_int, 1. / 3.);                // drv:521
    return SPHX_OK;
}

struct ScaleWork { u64 *key, *hist, *scal; };
static int scale_work(sphx_ctx* ctx, int64_t n, ScaleWork* w) {
    Carve c;
    c.take(w->key, (size_t)n); c.take(w->hist, SCALE_BINS); c.take(w->scal, SS_N);
    return sphx_carve_into(ctx, ctx->scale_work, c);
}
static unsigned scale_blocks(size_t lanes) { return sphx_blocks(lanes, SCALE_WG); }
static unsigned scale_grid(int64_t n) {
    const unsigned b = scale_blocks((size_t)n);
    return b < SCALE_MAX_BLOCKS ? b : SCALE_MAX_BLOCKS;
}

struct ScaleSel { int64_t n_slow, n_nan, lo, hi; double a, b, max_dist, d; };
// keys and selection on device inputs, timer marks 1 and 2; the one read-back; the finish.  Refuses M = 0.
static int scale_select(sphx_ctx* ctx, const char* who, ScaleKeys ka, double qf, double n_int, double fill, const ScaleWork& w, ScaleSel* out) {
    hipStream_t st = ctx->stream;
    const int n = ka.n;
    HIPCHK(hipMemsetAsync(w.hist, 0, (SCALE_BINS + SS_N) * sizeof(u64), st));
    hipLaunchKernelGGL(scale_key_kernel, dim3(scale_blocks((size_t)n)), dim3(SCALE_WG), 0, st, ka, w.key, w.scal);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->scale_t.mark(ctx, 1));
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(scale_hist_kernel, dim3(scale_grid(n)), dim3(SCALE_WG), 0, st, n, w.key, w.scal, shift, w.hist);
        hipLaunchKernelGGL(scale_choose_kernel, dim3(1), dim3(SCALE_WG), 0, st, shift, qf, w.hist, w.scal);
    }
    hipLaunchKernelGGL(scale_next_kernel, dim3(scale_grid(n)), dim3(SCALE_WG), 0, st, n, w.key, w.scal);
    HIPCHK(hipGetLastError());
    u64* back = ctx->pinned->scal;
    HIPCHK(hipMemcpyAsync(back, w.scal, SS_N * sizeof(u64), hipMemcpyDeviceToHost, st));
    SPHX_TRY(ctx->scale_t.mark(ctx, 2));
    HIPCHK(hipStreamSynchronize(st));
    out->n_slow = (int64_t)back[SS_M]; out->n_nan = (int64_t)back[SS_NNAN];
    if (out->n_slow < 1)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: no row is slower than v_max (np.percentile of an empty selection raises)", who);
    out->lo = (int64_t)back[SS_LO]; out->hi = (int64_t)back[SS_HI];
    out->a = scale_key_value(back[SS_A]); out->b = scale_key_value(back[SS_B]);
    if (back[SS_B] == SCALE_KEY_OUT)
        return sphx_set_err(ctx, SPHX_E_HIP, "%s: no key of rank %lld among %lld slow rows", who, (long long)out->hi, (long long)out->n_slow);
    return sphx_length_scale_finish(out->n_slow, out->n_nan, qf, out->a, out->b, n_int, fill, &out->max_dist, &out->d);
}
static int scale_check(sphx_ctx* ctx, const char* who, int64_t n, double v_max2, double qf, double n_int, double fill) {
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld (need 1 <= n < 2^31 - 16)", who, (long long)n);
    if (!(qf >= 0.0 && qf <= 1.0)) return sphx_set_err(ctx, SPHX_E_ARG, "%s: qf=%g outside [0, 1]", who, qf);
    if (v_max2 != v_max2 || n_int != n_int || fill != fill) return sphx_set_err(ctx, SPHX_E_ARG, "%s: v_max2, n_int or fill is NaN", who);
    return SPHX_OK;
}
static void scale_sel_out(const ScaleSel& s, int64_t* n_slow, int64_t* n_nan, int64_t* lo, double* a, double* b, double* max_dist, double* d) {
    if (n_slow) *n_slow = s.n_slow;
    if (n_nan) *n_nan = s.n_nan;
    if (lo) *lo = s.lo;
    if (a) *a = s.a;
    if (b) *b = s.b;
    if (max_dist) *max_dist = s.max_dist;
    if (d) *d = s.d;
}

extern "C" int sphx_length_scale(sphx_ctx* ctx, int64_t n, const double* points, const double* velocities, double v_max2, double qf,
                                 double n_int, double fill, int64_t* n_slow, int64_t* n_nan, int64_t* lo, double* a, double* b,
                                 double* max_dist, double* d) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_length_scale";
    NEED(points); NEED(velocities); NEED(d);
    SPHX_TRY(scale_check(ctx, who, n, v_max2, qf, n_int, fill));
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nn = (size_t)n;
    ScaleWork w;
    SPHX_TRY(scale_work(ctx, n, &w));
    double *p, *v;
    Carve c;
    c.take(p, 3 * nn); c.take(v, 3 * nn);
    SPHX_TRY(sphx_carve_into(ctx, ctx->scale_in, c));
    SPHX_TRY(ctx->scale_t.begin(ctx));
    const CopyF64 us[] = {{points, p, 3 * nn}, {velocities, v, 3 * nn}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 2));
    const ScaleKeys ka{(int)n, p, p + 1, p + 2, 3, v, v + 1, v + 2, 3, v_max2};
    ScaleSel sel;
    SPHX_TRY(scale_select(ctx, who, ka, qf, n_int, fill, w, &sel));
    for (int i = 3; i <= 5; ++i) SPHX_TRY(ctx->scale_t.mark(ctx, i));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    scale_sel_out(sel, n_slow, n_nan, lo, a, b, max_dist, d);
    return ctx->scale_t.end(ctx);
}

// ctx->scale_int: rev (n) | nontriv (n), u32; ctx->scale_out: sizes (n) | new_smoothing (n) | rev64 (n) | nontriv64 (n)
struct ScaleBufs { unsigned *rev, *nontriv; double *sizes, *smooth; long long *rev64, *nontriv64; };
static int scale_bufs(sphx_ctx* ctx, int64_t n, ScaleBufs* o) {
    const size_t nn = (size_t)n;
    Carve ci, co;
    ci.take(o->rev, nn); ci.take(o->nontriv, nn);
    SPHX_TRY(sphx_carve_into(ctx, ctx->scale_int, ci));
    co.take(o->sizes, nn); co.take(o->smooth, nn); co.take(o->rev64, nn); co.take(o->nontriv64, nn);
    SPHX_TRY(sphx_carve_into(ctx, ctx->scale_out, co));
    HIPCHK(hipMemsetAsync(o->rev, 0, 2 * nn * sizeof(unsigned), ctx->stream));
    return SPHX_OK;
}
static int scale_adapt_run(sphx_ctx* ctx, const ScaleAdapt& a, u64* scal) {
    hipLaunchKernelGGL(scale_adapt_kernel, dim3(scale_blocks((size_t)a.n)), dim3(SCALE_WG), 0, ctx->stream, a, scal);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

extern "C" int sphx_adapt_sizes(sphx_ctx* ctx, int64_t n, int k, const int64_t* neighbor, const double* densities, const double* densities_0,
                                const double* sizes, const double* ptype, double d, double d_dust, double* sizes_out,
                                int64_t* rev_count_out, int64_t* nontrivial_out, double* new_smoothing_out, int64_t* counts) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_adapt_sizes";
    NEED(neighbor); NEED(densities); NEED(sizes); NEED(ptype); NEED(sizes_out);
    if (n < 1 || n > 0x7FFFFFF0ll || k < 1 || k > SPHX_MAX_K)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld, k=%d (need 1 <= n < 2^31 - 16, 1 <= k <= %d)", who, (long long)n, k, SPHX_MAX_K);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)n, nk = nn * (size_t)k;
    ScaleWork w;
    SPHX_TRY(scale_work(ctx, n, &w));
    ScaleBufs o;
    SPHX_TRY(scale_bufs(ctx, n, &o));
    // inputs: densities | densities_0 | sizes | ptype (n each) | the list (n k int64)
    double *d_rho, *d_rho0, *d_sz, *d_pt;
    long long* nb;
    Carve c;
    c.take(d_rho, nn); c.take(d_rho0, nn); c.take(d_sz, nn); c.take(d_pt, nn); c.take(nb, nk);
    SPHX_TRY(sphx_carve_into(ctx, ctx->scale_in, c));
    SPHX_TRY(ctx->scale_t.begin(ctx));
    HIPCHK(hipMemsetAsync(w.scal, 0, SS_N * sizeof(u64), st));
    const CopyF64 us[] = {{densities, d_rho, nn}, {densities_0, d_rho0, nn}, {sizes, d_sz, nn}, {ptype, d_pt, nn}, {neighbor, nb, nk}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 5));
    SPHX_TRY(ctx->scale_t.mark(ctx, 1));
    SPHX_TRY(ctx->scale_t.mark(ctx, 2));
    hipLaunchKernelGGL(scale_count_rows_kernel, dim3(scale_blocks(nk)), dim3(SCALE_WG), 0, st, (int)n, k, nb, o.rev, o.nontriv, w.scal);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->scale_t.mark(ctx, 3));
    const ScaleAdapt a{(int)n, nullptr, o.rev, o.nontriv, d_rho, densities_0 ? d_rho0 : nullptr, d_sz, d_pt, d, d_dust,
                       nullptr, o.sizes, o.smooth, nullptr, o.rev64, o.nontriv64};
    SPHX_TRY(scale_adapt_run(ctx, a, w.scal));
    SPHX_TRY(ctx->scale_t.mark(ctx, 4));
    u64* back = ctx->pinned->scal;
    HIPCHK(hipMemcpyAsync(back, w.scal, SS_N * sizeof(u64), hipMemcpyDeviceToHost, st));
    const CopyF64 ds[] = {{sizes_out, o.sizes, nn}, {new_smoothing_out, o.smooth, nn}, {rev_count_out, o.rev64, nn}, {nontrivial_out, o.nontriv64, nn}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 4));
    SPHX_TRY(ctx->scale_t.mark(ctx, 5));
    HIPCHK(hipStreamSynchronize(st));
    if (counts)
        for (int i = 0; i < SPHX_SCALE_NCOUNT; ++i) counts[i] = (int64_t)back[SS_BONUS + i];
    return ctx->scale_t.end(ctx);
}

extern "C" int sphx_state_length_scale(sphx_ctx* ctx, double v_max2, double qf, double n_int, double fill, double raise_factor, int apply,
                                       int64_t* n_slow, int64_t* n_nan, int64_t* lo, double* a, double* b, double* max_dist, double* d,
                                       double* d_dust, int64_t* counts, double* sizes_out, int64_t* rev_count_out) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_length_scale";
    SPHX_TRY(sphx_phase_need_list(ctx, who));
    NEED(d); NEED(d_dust);
    const int64_t n = ctx->n;
    const int k = ctx->k;
    SPHX_TRY(scale_check(ctx, who, n, v_max2, qf, n_int, fill));
    if (raise_factor != raise_factor) return sphx_set_err(ctx, SPHX_E_ARG, "%s: raise_factor is NaN", who);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const size_t nn = (size_t)n;
    const StateArrays& st = ctx->st;
    ScaleWork w;
    SPHX_TRY(scale_work(ctx, n, &w));
    SPHX_TRY(ctx->scale_t.begin(ctx));
    // ---- drv:493-521, on the state's columns as they lie ----
    const ScaleKeys ka{(int)n, st.x.as<double>(), st.y.as<double>(), st.z.as<double>(), 1, st.vx.as<double>(), st.vy.as<double>(),
                       st.vz.as<double>(), 1, v_max2};
    ScaleSel sel;
    SPHX_TRY(scale_select(ctx, who, ka, qf, n_int, fill, w, &sel));
    const double dd = sel.d / pow(raise_factor, 1. / 3.);                    // drv:538
    if (apply && sel.d != sel.d)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: d is NaN (%lld NaN positions among the slow rows, max_dist=%g): not applied", who,
                            (long long)sel.n_nan, sel.max_dist);
    if (apply && ctx->loop_forms && !(sel.d > 0.0))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: d=%g: the loop forms need d > 0, not applied", who, sel.d);
    // ---- drv:527-540, in storage slots ----
    ScaleBufs o;
    SPHX_TRY(scale_bufs(ctx, n, &o));
    if (apply) {
        SPHX_TRY(sphx_ensure(ctx, ctx->scale_sizes, nn * sizeof(double)));
        if (!ctx->scale_d0_valid) SPHX_TRY(sphx_ensure(ctx, ctx->scale_d0, nn * sizeof(double)));
    }
    hipLaunchKernelGGL(scale_count_cols_kernel, dim3(scale_blocks(nn)), dim3(SCALE_WG), 0, stream, (int)n, (int)sphx_pad64(n), k,
                       ctx->nbr.as<int>(), ctx->step_qorder, o.rev, o.nontriv, w.scal);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->scale_t.mark(ctx, 3));
    const bool have_rho = !ctx->sums_stale && ctx->rho.p;                    // (behind an insertion the sums have the old row count)
    const bool have_d0 = ctx->scale_d0_valid && have_rho;
    const ScaleAdapt ad{(int)n, st.id.as<int>(), o.rev, o.nontriv, have_rho ? ctx->rho.as<double>() : nullptr,
                        have_d0 ? ctx->scale_d0.as<double>() : nullptr, st.hprev.as<double>(), st.ptype.as<double>(), sel.d, dd,
                        apply ? ctx->scale_sizes.as<double>() : nullptr, o.sizes, nullptr,
                        apply && have_rho ? ctx->scale_d0.as<double>() : nullptr, o.rev64, nullptr};
    SPHX_TRY(scale_adapt_run(ctx, ad, w.scal));
    SPHX_TRY(ctx->scale_t.mark(ctx, 4));
    u64* back = ctx->pinned->scal;
    HIPCHK(hipMemcpyAsync(back, w.scal, SS_N * sizeof(u64), hipMemcpyDeviceToHost, stream));
    const CopyF64 ds[] = {{sizes_out, o.sizes, nn}, {rev_count_out, o.rev64, nn}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 2));
    SPHX_TRY(ctx->scale_t.mark(ctx, 5));
    HIPCHK(hipStreamSynchronize(stream));
    if (apply) {
        ctx->scale_sizes_valid = true;
        ctx->scale_d0_valid = have_rho;
        if (ctx->loop_forms) ctx->loop_d = sel.d;                            // nsc.d = d, drv:523
    }
    scale_sel_out(sel, n_slow, n_nan, lo, a, b, max_dist, d);
    *d_dust = dd;
    if (counts)
        for (int i = 0; i < SPHX_SCALE_NCOUNT; ++i) counts[i] = (int64_t)back[SS_BONUS + i];
    return ctx->scale_t.end(ctx);
}

extern "C" int sphx_state_download_sizes(sphx_ctx* ctx, double* sizes) {
    if (!ctx) return SPHX_E_ARG;
    NEED(sizes);
    if (!ctx->has_state || !ctx->scale_sizes_valid)
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_download_sizes: no adapted sizes stand (sphx_state_length_scale with apply, since the last step)");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nb = (size_t)ctx->n * sizeof(double);
    SPHX_TRY(sphx_ensure(ctx, ctx->out_a, nb));
    SPHX_TRY(sphx_scatter_rows_by_id(ctx, ctx->n, 1, ctx->st.id.as<int>(), ctx->scale_sizes.as<double>(), ctx->out_a.as<double>()));
    HIPCHK(hipMemcpyAsync(sizes, ctx->out_a.p, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPHX_OK;
}

extern "C" int sphx_scale_last_timing(sphx_ctx* ctx, double ms[5]) {
    return last_timing(ctx, &sphx_ctx::scale_t, ms);
}
