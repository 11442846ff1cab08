// sphx_census.hip - what decides the physics of a pass of the driver's loop and what the run is for, formed where the
// state lives: the census (the sums, counts and the maximum of drv:341, 465-468, 616-617, 636, 656-658 and of
// Simulation.diagnostics), the ordered selections (drv:620's dust temperatures, the star rows of the schedule drv:244,
// the AGB rows of drv:660-664) and the stellar clock (star_ages by particle id, drv:604, drv:371).  include/sphx.h has the
// definitions; here the route:
//   census_kernel     one workgroup of 256 lanes per chunk of 256 consecutive PARTICLE IDS; lane j owns id c 256 + j,
//                     reaches its storage slot through the slot map (the inverse of st.id; the array calls: identity),
//                     loads its row's scalars and its contiguous composition row, forms its terms (sphx_census_terms.h)
//                     and lays them in LDS as [quantity][257], a tile of 29 quantities at a time; lane q of the tile then
//                     sums its quantity's rows left to right and stores part[q][c].  No term is materialised in memory.
//                     The counts are integer atomics (one per wave and count), the largest stellar mass a tree over
//                     the lanes that hands a NaN on.
//   the totals        sphx_ordered_totals_of_parts (sphx_side.hip): sphx_ordered_totals' own second stage - lane l of 256
//                     adds the chunks l, l + 256, ... in order, then the binary tree.  So a total is the same bits on
//                     every call and in every storage order, and the tests restate it in NumPy.
//   the selections    lane per id -> flag -> sphx_excl_scan_int -> the host checks the total against the caller's capacity
//                     -> scatter of the named columns: ascending particle id by construction.
// The census only reads the state, in buffers of its own (ctx->census_*).  Plain C++, vector stores, no fp atomics.
#include "sphx_internal.h"
#include "sphx_census_terms.h"
#pragma clang fp contract(off)

#define CEN_WG SPHX_CEN_CHUNK
static_assert(SPHX_CEN_CHUNK == SPHX_TOT_CHUNK, "the census' chunks are the ordered totals' chunks");
static_assert(SPHX_CEN_TILE * SPHX_CEN_PITCH * sizeof(double) + CEN_WG * sizeof(double) <= 65536, "the tile and the maxima fit static LDS");
static_assert(SPHX_CEN_FIXED + 3 * SPHX_MAX_SPECIES + 1 + 4 + 2 == SPHX_CENSUS_PIN, "the read-back's place in PinnedLayout");

// the larger of two values, a NaN handed on
__device__ __forceinline__ double cen_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// slot[id[j]] = j: where the particle with an id lies in the state
__global__ __launch_bounds__(CEN_WG) void census_slot_kernel(int n, const int* __restrict__ id, int* __restrict__ slot) {
    const int j = blockIdx.x * CEN_WG + threadIdx.x;
    if (j >= n) return;
    const int i = id[j];
    if ((unsigned)i < (unsigned)n) slot[i] = j;
}

struct CensusArgs {
    int n, s, fs, nq, nchunk;        // fs: doubles between two composition rows
    const int* slot;                 // storage slot of an id (NULL: the id)
    const double *m, *pt, *vx, *vy, *vz, *ax, *ay, *az, *E;      // by slot; vs / as: their strides; vx, ax, E may be NULL
    int vs, as;
    const double *fun, *mus;         // composition rows BY ID and mu_specie, or NULL
    double *part, *pmax;             // (nq, nchunk), (nchunk)
    u64* cnt;                        // types 0, 1, 2 and != 2
};
__global__ __launch_bounds__(CEN_WG) void census_kernel(CensusArgs a) {
    __shared__ double tile[SPHX_CEN_TILE * SPHX_CEN_PITCH];
    __shared__ double smax[CEN_WG];
    const int c = blockIdx.x, j = threadIdx.x;
    const long long i = (long long)c * SPHX_CEN_CHUNK + j;
    const bool live = i < a.n;
    const int rows = min(SPHX_CEN_CHUNK, a.n - c * SPHX_CEN_CHUNK);
    SphxCenRow r;
    r.m = 0.0; r.pt = -1.0; r.vx = r.vy = r.vz = 0.0; r.ax = r.ay = r.az = 0.0; r.E = 0.0; r.rowsum = 0.0; r.f = nullptr;
    if (live) {
        const size_t p = a.slot ? (size_t)a.slot[i] : (size_t)i;
        r.m = a.m[p]; r.pt = a.pt[p];
        if (a.vx) { r.vx = a.vx[p * a.vs]; r.vy = a.vy[p * a.vs]; r.vz = a.vz[p * a.vs]; }
        if (a.ax) { r.ax = a.ax[p * a.as]; r.ay = a.ay[p * a.as]; r.az = a.az[p * a.as]; }
        if (a.E) r.E = a.E[p];
        if (a.fun) {
            r.f = a.fun + (size_t)i * a.fs;
            r.rowsum = sphx_cen_row_sum(a.s, r.f, a.mus);
        }
    }
    // the counts: a ballot per type, one integer atomic per wave that saw any
    {
        const u64 b0 = __ballot(live && r.pt == 0.0), b1 = __ballot(live && r.pt == 1.0), b2 = __ballot(live && r.pt == 2.0),
                  b3 = __ballot(live && r.pt != 2.0);
        if ((j & (SPHX_WAVE - 1)) == 0) {
            if (b0) atomicAdd(a.cnt + 0, (u64)__popcll(b0));
            if (b1) atomicAdd(a.cnt + 1, (u64)__popcll(b1));
            if (b2) atomicAdd(a.cnt + 2, (u64)__popcll(b2));
            if (b3) atomicAdd(a.cnt + 3, (u64)__popcll(b3));
        }
    }
    // the largest stellar mass of the chunk
    smax[j] = (live && r.pt == 1.0) ? r.m : -INFINITY;
    __syncthreads();
    for (int h = CEN_WG / 2; h > 0; h >>= 1) {
        if (j < h) smax[j] = cen_max(smax[j], smax[j + h]);
        __syncthreads();
    }
    if (j == 0) a.pmax[c] = smax[0];
    // the sums, a tile of quantities at a time
    const int ntile = sphx_cen_tiles(a.nq);
    for (int t = 0; t < ntile; ++t) {
        const int len = sphx_cen_tile_len(a.nq, t), q0 = t * SPHX_CEN_TILE;
        for (int tq = 0; tq < len; ++tq) tile[sphx_cen_at(tq, j)] = live ? sphx_cen_term(r, q0 + tq, a.s, a.mus) : 0.0;
        __syncthreads();
        if (j < len) {
            double sum = 0.0;
            for (int row = 0; row < rows; ++row) sum += tile[sphx_cen_at(j, row)];
            a.part[(size_t)(q0 + j) * a.nchunk + c] = sum;
        }
        __syncthreads();
    }
}
// one workgroup: the largest of the chunks' maxima
__global__ __launch_bounds__(CEN_WG) void census_max_kernel(int nchunk, const double* __restrict__ pmax, double* __restrict__ out) {
    __shared__ double sm[CEN_WG];
    const int l = threadIdx.x;
    double v = -INFINITY;
    for (int c = l; c < nchunk; c += CEN_WG) v = cen_max(v, pmax[c]);
    sm[l] = v;
    __syncthreads();
    for (int h = CEN_WG / 2; h > 0; h >>= 1) {
        if (l < h) sm[l] = cen_max(sm[l], sm[l + h]);
        __syncthreads();
    }
    if (l == 0) out[0] = sm[0];
}

// ---- the selections ----
struct SelectArgs {
    int n, s, fs, type, window;
    const int* slot;
    const double *m, *pt, *T;        // by slot; T may be NULL
    const double *age, *fun;         // by id; either may be NULL
    double unit, lo, hi;             // window: lo < m / unit < hi (drv:660)
    int* flag;                       // (n + 1), flag[n] = 0
    const int* start;                // its exclusive scan
    long long* oid;
    double *om, *oT, *oage, *of;     // of (count, s) or NULL
};
__global__ __launch_bounds__(CEN_WG) void census_flag_kernel(SelectArgs a) {
    const long long i = (long long)blockIdx.x * CEN_WG + threadIdx.x;
    if (i > a.n) return;
    int f = 0;
    if (i < a.n) {
        const size_t p = a.slot ? (size_t)a.slot[i] : (size_t)i;
        f = a.pt[p] == (double)a.type;
        if (f && a.window) {
            const double u = a.m[p] / a.unit;
            f = (u > a.lo) && (u < a.hi);
        }
    }
    a.flag[i] = f;
}
__global__ __launch_bounds__(CEN_WG) void census_pick_kernel(SelectArgs a) {
    const long long i = (long long)blockIdx.x * CEN_WG + threadIdx.x;
    if (i >= a.n || !a.flag[i]) return;
    const size_t p = a.slot ? (size_t)a.slot[i] : (size_t)i, o = (size_t)a.start[i];
    a.oid[o] = i;
    a.om[o] = a.m[p];
    a.oT[o] = a.T ? a.T[p] : 0.0;
    a.oage[o] = a.age ? a.age[i] : 0.0;
    if (a.of) {
        const double* f = a.fun + (size_t)i * a.fs;
        for (int t = 0; t < a.s; ++t) a.of[o * a.s + t] = f[t];
    }
}

// ---- the stellar clock ----
// drv:604, one lane per storage slot (id NULL: slot = id)
__global__ __launch_bounds__(CEN_WG) void census_advance_kernel(int n, const int* __restrict__ id, const double* __restrict__ pt,
                                                                 double dt, double* __restrict__ ages) {
    const int j = blockIdx.x * CEN_WG + threadIdx.x;
    if (j >= n) return;
    const int i = id ? id[j] : j;
    if ((unsigned)i >= (unsigned)n) return;
    if (pt[j] == 1.0 && ages[i] > -2.0) ages[i] += dt;
}
__global__ __launch_bounds__(CEN_WG) void census_fill_kernel(long long first, long long end, double v, double* __restrict__ out) {
    const long long i = first + (long long)blockIdx.x * CEN_WG + threadIdx.x;
    if (i < end) out[i] = v;
}

// =====================================================================================================================
// host side
// =====================================================================================================================
static int cen_check_n(sphx_ctx* ctx, const char* who, int64_t n) {
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld (need 1 <= n < 2^31 - 16)", who, (long long)n);
    return SPHX_OK;
}
// ctx->census_int: slot | flag | start (n + 1 each; the scan wants 16-byte boundaries)
struct CenInts { int *slot, *flag, *start; };
static int cen_ints(sphx_ctx* ctx, int64_t n, CenInts* o) {
    Carve c;
    c.take(o->slot, (size_t)n + 1, 16); c.take(o->flag, (size_t)n + 1, 16); c.take(o->start, (size_t)n + 1, 16);
    c.pad(16);
    return sphx_carve_into(ctx, ctx->census_int, c);
}
// the slot map of the resident state into ctx->census_int
static int cen_slot_map(sphx_ctx* ctx, const int** slot) {
    CenInts ci;
    SPHX_TRY(cen_ints(ctx, ctx->n, &ci));
    SPHX_TRY(sphx_slot_map(ctx, ci.slot));
    *slot = ci.slot;
    return SPHX_OK;
}
int sphx_slot_map(sphx_ctx* ctx, int* slot) {
    const size_t nn = (size_t)ctx->n;
    HIPCHK(hipMemsetAsync(slot, 0, nn * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(census_slot_kernel, dim3(sphx_blocks(nn, CEN_WG)), dim3(CEN_WG), 0, ctx->stream, (int)ctx->n, ctx->st.id.as<int>(), slot);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

// chunk sums, totals, maximum and counts of `a` (part, pmax, cnt are set here), timer marks 2 .. 4, the results out
static int cen_run(sphx_ctx* ctx, CensusArgs a, double* totals, int64_t* counts, double* max_star_mass) {
    hipStream_t st = ctx->stream;
    const size_t nchunk = sphx_tot_chunks(a.n), nq = (size_t)a.nq;
    // ctx->census_buf: tot (nq) | max (1) | counts (4 u64) | pmax (nchunk) | part (nq, nchunk)
    double *tot, *gmax;
    Carve c;
    c.take(tot, nq); c.take(gmax, 1); c.take(a.cnt, 4); c.take(a.pmax, nchunk); c.take(a.part, nq * nchunk);
    SPHX_TRY(sphx_carve_into(ctx, ctx->census_buf, c));
    a.nchunk = (int)nchunk;
    HIPCHK(hipMemsetAsync(a.cnt, 0, 4 * sizeof(u64), st));
    hipLaunchKernelGGL(census_kernel, dim3((unsigned)nchunk), dim3(CEN_WG), 0, st, a);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->census_t.mark(ctx, 2));
    SPHX_TRY(sphx_ordered_totals_of_parts(ctx, nchunk, a.nq, a.part, tot));
    hipLaunchKernelGGL(census_max_kernel, dim3(1), dim3(CEN_WG), 0, st, (int)nchunk, a.pmax, gmax);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->census_t.mark(ctx, 3));
    u64* back = ctx->pinned->census;
    HIPCHK(hipMemcpyAsync(back, tot, (nq + 5) * sizeof(double), hipMemcpyDeviceToHost, st));
    SPHX_TRY(ctx->census_t.mark(ctx, 4));
    HIPCHK(hipStreamSynchronize(st));
    memcpy(totals, back, nq * sizeof(double));
    if (max_star_mass) memcpy(max_star_mass, back + nq, sizeof(double));
    if (counts)
        for (int q = 0; q < 4; ++q) counts[q] = (int64_t)back[nq + 1 + q];
    return ctx->census_t.end(ctx);
}
static int cen_check_mus(sphx_ctx* ctx, const char* who, int s, const double* mu_specie) {
    if (s < 1 || s > SPHX_MAX_SPECIES) return sphx_set_err(ctx, SPHX_E_ARG, "%s: s=%d (need 1 <= s <= %d)", who, s, SPHX_MAX_SPECIES);
    for (int t = 0; t < s; ++t) ctx->census_tab[t] = mu_specie[t];
    return SPHX_OK;
}

extern "C" int sphx_census(sphx_ctx* ctx, int64_t n, int s, const double* mass, const double* ptype, const double* f_un,
                           const double* mu_specie, const double* velocities, const double* total_accel, const double* E_internal,
                           double* totals, int64_t counts[4], double* max_star_mass) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_census";
    NEED(mass); NEED(ptype); NEED(totals);
    SPHX_TRY(cen_check_n(ctx, who, n));
    if (f_un) { NEED(mu_specie); SPHX_TRY(cen_check_mus(ctx, who, s, mu_specie)); }
    else s = 0;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, S = (size_t)s;
    // ctx->census_in: mass | ptype | E (n each) | velocities | total_accel (n,3) | f_un (n,s) | mu_specie (s)
    double *d_m, *d_pt, *d_E, *d_v, *d_a, *d_f, *d_mus;
    Carve c;
    c.take(d_m, nn); c.take(d_pt, nn); c.take(d_E, nn); c.take(d_v, 3 * nn); c.take(d_a, 3 * nn); c.take(d_f, nn * S); c.take(d_mus, S);
    c.slack(sizeof(double));
    SPHX_TRY(sphx_carve_into(ctx, ctx->census_in, c));
    SPHX_TRY(ctx->census_t.begin(ctx));
    const CopyF64 us[] = {{mass, d_m, nn}, {ptype, d_pt, nn}, {E_internal, d_E, nn}, {velocities, d_v, 3 * nn}, {total_accel, d_a, 3 * nn},
                          {f_un, d_f, nn * S}, {f_un ? ctx->census_tab : nullptr, d_mus, S}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 7));
    SPHX_TRY(ctx->census_t.mark(ctx, 1));
    CensusArgs a;
    a.n = (int)n; a.s = s; a.fs = s; a.nq = sphx_cen_nq(s); a.slot = nullptr;
    a.m = d_m; a.pt = d_pt; a.E = E_internal ? d_E : nullptr;
    a.vx = velocities ? d_v : nullptr; a.vy = d_v + 1; a.vz = d_v + 2; a.vs = 3;
    a.ax = total_accel ? d_a : nullptr; a.ay = d_a + 1; a.az = d_a + 2; a.as = 3;
    a.fun = f_un ? d_f : nullptr; a.mus = d_mus;
    return cen_run(ctx, a, totals, counts, max_star_mass);
}

extern "C" int sphx_state_census(sphx_ctx* ctx, const double* mu_specie, double* totals, int64_t counts[4], double* max_star_mass) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_census";
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no state uploaded", who);
    NEED(totals);
    const bool species = mu_specie != nullptr;
    if (species && (ctx->s < 1 || !ctx->fun_id.p))
        return sphx_set_err(ctx, SPHX_E_STATE, "%s: the state carries no composition (f_un): no sums by species", who);
    SPHX_TRY(cen_check_n(ctx, who, ctx->n));
    const int s = species ? ctx->s : 0;
    if (species) SPHX_TRY(cen_check_mus(ctx, who, s, mu_specie));
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->census_t.begin(ctx));
    const int* slot = nullptr;
    SPHX_TRY(cen_slot_map(ctx, &slot));
    SPHX_TRY(sphx_ensure(ctx, ctx->census_in, (SPHX_MAX_SPECIES + 1) * sizeof(double)));
    double* d_mus = ctx->census_in.as<double>();
    if (species) HIPCHK(hipMemcpyAsync(d_mus, ctx->census_tab, (size_t)s * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SPHX_TRY(ctx->census_t.mark(ctx, 1));
    const StateArrays& st = ctx->st;
    CensusArgs a;
    a.n = (int)ctx->n; a.s = s; a.fs = ctx->sp; a.nq = sphx_cen_nq(s); a.slot = slot;
    a.m = st.m.as<double>(); a.pt = st.ptype.as<double>(); a.E = st.E.as<double>();
    a.vx = st.vx.as<double>(); a.vy = st.vy.as<double>(); a.vz = st.vz.as<double>(); a.vs = 1;
    a.ax = st.ax.as<double>(); a.ay = st.ay.as<double>(); a.az = st.az.as<double>(); a.as = 1;
    a.fun = species ? ctx->fun_id.as<double>() : nullptr; a.mus = d_mus;
    return cen_run(ctx, a, totals, counts, max_star_mass);
}

extern "C" int sphx_census_last_timing(sphx_ctx* ctx, double ms[4]) {
    return last_timing(ctx, &sphx_ctx::census_t, ms);
}

// flags, scan, the count on the host, the capacity check, the scatter, the rows out.  a: everything but flag, start and
// the outputs.  ids == NULL: the count alone.
static int cen_select(sphx_ctx* ctx, const char* who, SelectArgs a, int64_t cap, int64_t* count, int64_t* ids, double* mass_out,
                      double* T_out, double* age_out, double* f_out) {
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)a.n, S = (size_t)a.s;
    CenInts ci;                                      // (a.slot, where set, lies in the first part)
    SPHX_TRY(cen_ints(ctx, a.n, &ci));
    int *flag = ci.flag, *start = ci.start;
    a.flag = flag; a.start = start;
    hipLaunchKernelGGL(census_flag_kernel, dim3(sphx_blocks(nn + 1, CEN_WG)), dim3(CEN_WG), 0, st, a);
    HIPCHK(hipGetLastError());
    SPHX_TRY(sphx_excl_scan_int(ctx, flag, start, a.n));
    u64* back = ctx->pinned->census;
    HIPCHK(hipMemcpyAsync(back, start + nn, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t cnt = (int64_t)*(const int*)back;
    *count = cnt;
    if (!ids || cnt == 0) return SPHX_OK;
    if (cnt < 0 || cnt > (int64_t)a.n) return sphx_set_err(ctx, SPHX_E_HIP, "%s: the scan counts %lld rows of %d", who, (long long)cnt, a.n);
    if (cnt > cap)                                   // (before anything is copied, as sphx_state_insert_rows checks its capacities)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: the selection holds %lld rows, the outputs %lld", who, (long long)cnt, (long long)cap);
    const size_t nc = (size_t)cnt;
    const bool want_f = f_out != nullptr;
    // ctx->census_buf: ids (count int64) | mass | T | age (count) | f (count, s)
    Carve c;
    c.take(a.oid, nc); c.take(a.om, nc); c.take(a.oT, nc); c.take(a.oage, nc);
    a.of = nullptr;
    if (want_f) c.take(a.of, nc * S);
    SPHX_TRY(sphx_carve_into(ctx, ctx->census_buf, c));
    hipLaunchKernelGGL(census_pick_kernel, dim3(sphx_blocks(nn, CEN_WG)), dim3(CEN_WG), 0, st, a);
    HIPCHK(hipGetLastError());
    const CopyF64 ds[] = {{ids, a.oid, nc}, {mass_out, a.om, nc}, {T_out, a.oT, nc}, {age_out, a.oage, nc}, {f_out, a.of, nc * S}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 5));
    HIPCHK(hipStreamSynchronize(st));
    return SPHX_OK;
}
static int cen_check_select(sphx_ctx* ctx, const char* who, int type, int window, double unit, double lo, double hi, int64_t cap,
                            const int64_t* count) {
    NEED(count);
    if (type < 0 || type > 2) return sphx_set_err(ctx, SPHX_E_ARG, "%s: type=%d (0 gas, 1 star, 2 dust)", who, type);
    if (cap < 0) return sphx_set_err(ctx, SPHX_E_ARG, "%s: cap=%lld", who, (long long)cap);
    if (window && (unit != unit || lo != lo || hi != hi)) return sphx_set_err(ctx, SPHX_E_ARG, "%s: the mass window holds a NaN", who);
    return SPHX_OK;
}

extern "C" int sphx_census_select(sphx_ctx* ctx, int64_t n, int s, const double* mass, const double* ptype, const double* T,
                                  const double* star_ages, const double* f_un, int type, int window, double unit, double lo, double hi,
                                  int64_t cap, int64_t* count, int64_t* ids, double* mass_out, double* T_out, double* age_out,
                                  double* f_out) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_census_select";
    NEED(mass); NEED(ptype);
    SPHX_TRY(cen_check_n(ctx, who, n));
    SPHX_TRY(cen_check_select(ctx, who, type, window, unit, lo, hi, cap, count));
    if (f_out && (!f_un || s < 1 || s > SPHX_MAX_SPECIES)) return sphx_set_err(ctx, SPHX_E_ARG, "%s: f_out needs f_un (n,s), 1 <= s <= %d", who, SPHX_MAX_SPECIES);
    if (!f_un) s = 0;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, S = (size_t)s;
    double *d_m, *d_pt, *d_T, *d_age, *d_f;
    Carve c;
    c.take(d_m, nn); c.take(d_pt, nn); c.take(d_T, nn); c.take(d_age, nn); c.take(d_f, nn * S);
    c.slack(sizeof(double));
    SPHX_TRY(sphx_carve_into(ctx, ctx->census_in, c));
    const CopyF64 us[] = {{mass, d_m, nn}, {ptype, d_pt, nn}, {T, d_T, nn}, {star_ages, d_age, nn}, {f_un, d_f, nn * S}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 5));
    SelectArgs a;
    a.n = (int)n; a.s = s; a.fs = s; a.type = type; a.window = window; a.slot = nullptr;
    a.m = d_m; a.pt = d_pt; a.T = T ? d_T : nullptr; a.age = star_ages ? d_age : nullptr; a.fun = f_un ? d_f : nullptr;
    a.unit = unit; a.lo = lo; a.hi = hi;
    return cen_select(ctx, who, a, cap, count, ids, mass_out, T_out, age_out, f_out);
}

extern "C" int sphx_state_census_select(sphx_ctx* ctx, int type, int window, double unit, double lo, double hi, int64_t cap,
                                        int64_t* count, int64_t* ids, double* mass_out, double* T_out, double* age_out, double* f_out) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_census_select";
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no state uploaded", who);
    SPHX_TRY(cen_check_n(ctx, who, ctx->n));
    SPHX_TRY(cen_check_select(ctx, who, type, window, unit, lo, hi, cap, count));
    if (age_out && !ctx->star_ages_valid) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no star_ages are set (sphx_state_set_star_ages)", who);
    if (f_out && (ctx->s < 1 || !ctx->fun_id.p)) return sphx_set_err(ctx, SPHX_E_STATE, "%s: the state carries no composition (f_un)", who);
    HIPCHK(hipSetDevice(ctx->device));
    const int* slot = nullptr;
    SPHX_TRY(cen_slot_map(ctx, &slot));
    const StateArrays& st = ctx->st;
    SelectArgs a;
    a.n = (int)ctx->n; a.s = f_out ? ctx->s : 0; a.fs = ctx->sp; a.type = type; a.window = window; a.slot = slot;
    a.m = st.m.as<double>(); a.pt = st.ptype.as<double>(); a.T = st.T.as<double>();
    a.age = ctx->star_ages_valid ? ctx->star_ages.as<double>() : nullptr;
    a.fun = f_out ? ctx->fun_id.as<double>() : nullptr;
    a.unit = unit; a.lo = lo; a.hi = hi;
    return cen_select(ctx, who, a, cap, count, ids, mass_out, T_out, age_out, f_out);
}

// ---- the stellar clock ----
extern "C" int sphx_state_set_star_ages(sphx_ctx* ctx, const double* star_ages) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_set_star_ages: no state uploaded");
    HIPCHK(hipSetDevice(ctx->device));
    if (!star_ages) { ctx->star_ages_valid = false; return SPHX_OK; }
    const size_t nb = (size_t)ctx->n * sizeof(double);
    SPHX_TRY(sphx_ensure(ctx, ctx->star_ages, nb));
    HIPCHK(hipMemcpyAsync(ctx->star_ages.p, star_ages, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->star_ages_valid = true;
    return SPHX_OK;
}
static int cen_need_ages(sphx_ctx* ctx, const char* who) {
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no state uploaded", who);
    if (!ctx->star_ages_valid) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no star_ages are set (sphx_state_set_star_ages)", who);
    return SPHX_OK;
}
extern "C" int sphx_state_download_star_ages(sphx_ctx* ctx, double* star_ages) {
    if (!ctx) return SPHX_E_ARG;
    NEED(star_ages);
    SPHX_TRY(cen_need_ages(ctx, "sphx_state_download_star_ages"));
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(star_ages, ctx->star_ages.p, (size_t)ctx->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPHX_OK;
}
extern "C" int sphx_state_advance_star_ages(sphx_ctx* ctx, double dt) {
    if (!ctx) return SPHX_E_ARG;
    SPHX_TRY(cen_need_ages(ctx, "sphx_state_advance_star_ages"));
    HIPCHK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(census_advance_kernel, dim3(sphx_blocks((size_t)ctx->n, CEN_WG)), dim3(CEN_WG), 0, ctx->stream, (int)ctx->n,
                       ctx->st.id.as<int>(), ctx->st.ptype.as<double>(), dt, ctx->star_ages.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPHX_OK;
}
extern "C" int sphx_advance_star_ages(sphx_ctx* ctx, int64_t n, double* star_ages, const double* ptype, double dt) {
    if (!ctx) return SPHX_E_ARG;
    NEED(star_ages); NEED(ptype);
    SPHX_TRY(cen_check_n(ctx, "sphx_advance_star_ages", n));
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nn = (size_t)n;
    double *p, *d_pt;
    Carve c;
    c.take(p, nn); c.take(d_pt, nn);
    SPHX_TRY(sphx_carve_into(ctx, ctx->census_in, c));
    const CopyF64 us[] = {{star_ages, p, nn}, {ptype, d_pt, nn}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 2));
    hipLaunchKernelGGL(census_advance_kernel, dim3(sphx_blocks(nn, CEN_WG)), dim3(CEN_WG), 0, ctx->stream, (int)n, (const int*)nullptr, d_pt, dt, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(star_ages, p, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPHX_OK;
}
// drv:371 inside sphx_state_insert_rows; a state without ages: nothing happens
int sphx_star_ages_grow(sphx_ctx* ctx, int64_t n_old, int64_t n_new, std::vector<void*>& retired) {
    if (!ctx->star_ages_valid) return SPHX_OK;
    int grown = 0;
    return sphx_ensure_keep(ctx, ctx->star_ages, (size_t)n_new * sizeof(double), (size_t)n_old * sizeof(double), retired, &grown);
}
int sphx_star_ages_fill(sphx_ctx* ctx, int64_t n_old, int64_t n_new) {
    if (!ctx->star_ages_valid || n_new <= n_old) return SPHX_OK;
    if (!ctx->star_ages.p || ctx->star_ages.cap < (size_t)n_new * sizeof(double))
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_insert_rows: the star_ages buffer does not hold %lld rows", (long long)n_new);
    hipLaunchKernelGGL(census_fill_kernel, dim3(sphx_blocks((size_t)(n_new - n_old), CEN_WG)), dim3(CEN_WG), 0, ctx->stream,
                       (long long)n_old, (long long)n_new, -2.0, ctx->star_ages.as<double>());
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}
