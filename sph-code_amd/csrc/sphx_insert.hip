// sphx_insert.hip - the insertion of a supernova's new particles into the resident state, code_running.py:361-396
// (drv:361-396): the block of the time loop that changes N.  include/sphx.h has the definitions; here the route:
//   sphx_state_download_rows   the few rows an event needs on the host (the exploding stars): one kernel over the state,
//                              every storage slot looking its caller id up in the SORTED list of the ids asked for (a
//                              binary search per thread, no N-sized inverse table), the slot that finds itself writing the
//                              row out
//   sphx_state_insert_rows     a. every per-particle buffer of the state grown with its contents kept (sphx_ensure_keep:
//                                 nothing inside the head-room), and the host's check that each now holds N + m rows
//                                 BEFORE any kernel is launched
//                              b. ONE kernel over N + m rows (insert_kernel): the clamp of T and mu, gamma formed again on
//                                 the old rows (drv:382, 393-394), m, E and the composition of the star rows rewritten
//                                 (drv:364-366) - found by the same binary search - and every field of the new rows
//                                 (drv:363, 367-372, 379-381)
//                              c. the driver's re-search drv:386 on the grown state (sphx_step_research, sphx_api.hip)
//                              d. the one-shot "no previous acceleration" of the next step (drv:484-485)
// mu, gamma and the drag coefficients are row sums in NumPy's order: phase_np_sum (sphx_phase_map.h), the one the dust
// and the radiative bookkeeping use.  Plain C++, vector stores; the only atomic is an integer count of the clamped rows.
#include "sphx_internal.h"
#include "sphx_phase_map.h"
#include <algorithm>
#include <numeric>
#pragma clang fp contract(off)

#define INS_WG 256

// the place of id in the ascending list ids[0 .. n), or -1
__device__ __forceinline__ int ins_find(const int* __restrict__ ids, int n, int id) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && ids[lo] == id) ? lo : -1;
}

// ---- the rows with the caller ids `ids` (ascending, nr of them) into row order[r] of the outputs ----
struct RowsArgs {
    int n, nr, s, sp;
    const int *id, *ids, *order;
    const double *x, *y, *z, *vx, *vy, *vz, *m, *E, *fun;
    double *pos, *vel, *om, *oE, *of;            // (nr,3) x 2, (nr) x 2, (nr,s) or NULL
};
__global__ __launch_bounds__(INS_WG) void ins_rows_kernel(RowsArgs a) {
    const int j = blockIdx.x * INS_WG + threadIdx.x;
    if (j >= a.n) return;
    const int id = a.id[j];
    const int r = ins_find(a.ids, a.nr, id);
    if (r < 0) return;
    const size_t o = (size_t)a.order[r];
    a.pos[3 * o] = a.x[j]; a.pos[3 * o + 1] = a.y[j]; a.pos[3 * o + 2] = a.z[j];
    a.vel[3 * o] = a.vx[j]; a.vel[3 * o + 1] = a.vy[j]; a.vel[3 * o + 2] = a.vz[j];
    a.om[o] = a.m[j]; a.oE[o] = a.E[j];
    if (a.of) {
        const double* f = a.fun + (size_t)id * a.sp;
        for (int t = 0; t < a.s; ++t) a.of[o * a.s + t] = f[t];
    }
}

// ---- drv:363-382, 393-394 on the device, one lane per row of the grown state ----
struct InsertArgs {
    int n_old, n_app, n_rew, s, sp;
    double *x, *y, *z, *vx, *vy, *vz, *ax, *ay, *az, *m, *T, *mu, *gam, *E, *hprev, *ptype;
    int* id;
    double* fun;                                 // the composition rows by caller id, sp doubles apart (NULL: the state has none)
    double *mgm, *mcs;                           // NULL: drag off
    const int* rew_ids;                          // ascending
    const double *rew_m, *rew_E, *rew_f;         // in the order of rew_ids
    const double *app_pos, *app_vel, *app_m, *app_pt, *app_E, *app_f;
    const double *mus, *gas, *gm, *se;           // mu_specie, gamma_specie, grain_mass, sigma_effective (s each)
    double t_cmb;
    u64* moved;                                  // rows whose T the clamp moved
};
__global__ __launch_bounds__(INS_WG) void insert_kernel(InsertArgs a) {
    const int t = blockIdx.x * INS_WG + threadIdx.x;
    const bool live = t < a.n_old + a.n_app;
    bool moved = false;
    if (live) {
        const double* f = nullptr;               // the row's composition as it stands after the event
        bool fresh_f = false;                    // ... which this lane has to store
        size_t row;
        if (t < a.n_old) {
            const int id = a.id[t];
            row = (size_t)id;
            const double T = a.T[t];
            if (T < a.t_cmb) { a.T[t] = a.t_cmb; moved = true; }               // drv:382 (a NaN stays)
            const int r = ins_find(a.rew_ids, a.n_rew, id);
            if (r >= 0) {                                                       // drv:364-366
                a.m[t] = a.rew_m[r]; a.E[t] = a.rew_E[r];
                f = a.rew_f + (size_t)r * a.s;
                fresh_f = true;
            } else if (a.fun) {
                f = a.fun + row * a.sp;
            }
        } else {
            const size_t j = (size_t)(t - a.n_old);
            row = (size_t)t;
            a.x[t] = a.app_pos[3 * j]; a.y[t] = a.app_pos[3 * j + 1]; a.z[t] = a.app_pos[3 * j + 2];      // drv:372
            a.vx[t] = a.app_vel[3 * j]; a.vy[t] = a.app_vel[3 * j + 1]; a.vz[t] = a.app_vel[3 * j + 2];  // drv:370
            a.ax[t] = 0.0; a.ay[t] = 0.0; a.az[t] = 0.0;
            a.m[t] = a.app_m[j]; a.E[t] = a.app_E[j]; a.ptype[t] = a.app_pt[j];                         // drv:363, 367-368
            a.hprev[t] = 0.0;
            a.id[t] = t;
            moved = 0.0 < a.t_cmb;
            a.T[t] = moved ? a.t_cmb : 0.0;                                                              // drv:379-382
            f = a.app_f + j * a.s;
            fresh_f = true;
        }
        if (f) {                                                                                         // drv:393-394
            const double sf = phase_np_sum(a.s, [&](int q) { return f[q]; });
            a.mu[t] = phase_np_sum(a.s, [&](int q) { return f[q] * a.mus[q]; }) / sf;
            a.gam[t] = phase_np_sum(a.s, [&](int q) { return f[q] * a.gas[q]; }) / sf;
        }
        if (fresh_f && a.mgm) {                                                 // nsc:720-726, as Simulation forms them
            a.mgm[t] = phase_np_sum(a.s, [&](int q) { return a.gm[q] * f[q]; });
            a.mcs[t] = phase_np_sum(a.s, [&](int q) { return a.se[q] * f[q]; });
        }
        if (fresh_f && a.fun) {                                                 // drv:365, 369 (after the sums: f may be this row)
            double* dst = a.fun + row * a.sp;
            for (int q = 0; q < a.s; ++q) dst[q] = f[q];
            for (int q = a.s; q < a.sp; ++q) dst[q] = 0.0;
        }
    }
    const u64 b = __ballot(moved);
    if (b && (threadIdx.x & (SPHX_WAVE - 1)) == 0) atomicAdd(a.moved, (u64)__popcll(b));
}

// =====================================================================================================================
// host side
// =====================================================================================================================
// ids (each in [0, n), none twice) ascending into `sorted`, order[r] = where sorted[r] stood
static int ins_sort_ids(sphx_ctx* ctx, const char* who, int64_t n, int64_t nr, const int64_t* ids, std::vector<int>& sorted,
                        std::vector<int>& order) {
    for (int64_t r = 0; r < nr; ++r)
        if (ids[r] < 0 || ids[r] >= n)
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: ids[%lld]=%lld outside [0, %lld)", who, (long long)r, (long long)ids[r], (long long)n);
    order.resize((size_t)nr);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int p, int q) { return ids[p] < ids[q]; });
    sorted.resize((size_t)nr);
    for (int64_t r = 0; r < nr; ++r) sorted[(size_t)r] = (int)ids[order[(size_t)r]];
    for (int64_t r = 1; r < nr; ++r)
        if (sorted[(size_t)r] == sorted[(size_t)r - 1])
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: id %d is given twice", who, sorted[(size_t)r]);
    return SPHX_OK;
}

extern "C" int sphx_state_download_rows(sphx_ctx* ctx, int64_t n_rows, const int64_t* ids, double* pos, double* vel, double* mass,
                                        double* E_internal, double* f_un) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_download_rows";
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no state uploaded", who);
    if (n_rows < 0 || n_rows > ctx->n) return sphx_set_err(ctx, SPHX_E_ARG, "%s: n_rows=%lld", who, (long long)n_rows);
    if (n_rows == 0) return SPHX_OK;
    NEED(ids); NEED(pos); NEED(vel); NEED(mass); NEED(E_internal);
    if (f_un && (ctx->s < 1 || !ctx->fun_id.p)) return sphx_set_err(ctx, SPHX_E_STATE, "%s: the state carries no composition (f_un)", who);
    std::vector<int> sorted, order;
    SPHX_TRY(ins_sort_ids(ctx, who, ctx->n, n_rows, ids, sorted, order));
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nr = (size_t)n_rows, s = (size_t)ctx->s;
    // ins_rows: pos | vel (nr,3) | m | E (nr) | f (nr,s) | sorted ids | order (ints)
    RowsArgs a;
    double* d_f;
    int *d_ids, *d_order;
    Carve c;
    c.take(a.pos, 3 * nr); c.take(a.vel, 3 * nr); c.take(a.om, nr); c.take(a.oE, nr); c.take(d_f, nr * s);
    c.take(d_ids, nr); c.take(d_order, nr);
    SPHX_TRY(sphx_carve_into(ctx, ctx->ins_rows, c));
    HIPCHK(hipMemcpyAsync(d_ids, sorted.data(), nr * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_order, order.data(), nr * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const StateArrays& st = ctx->st;
    a.n = (int)ctx->n; a.nr = (int)n_rows; a.s = ctx->s; a.sp = ctx->sp;
    a.id = st.id.as<int>(); a.ids = d_ids; a.order = d_order;
    a.x = st.x.as<double>(); a.y = st.y.as<double>(); a.z = st.z.as<double>();
    a.vx = st.vx.as<double>(); a.vy = st.vy.as<double>(); a.vz = st.vz.as<double>();
    a.m = st.m.as<double>(); a.E = st.E.as<double>(); a.fun = ctx->fun_id.as<double>();
    a.of = f_un ? d_f : nullptr;
    hipLaunchKernelGGL(ins_rows_kernel, dim3(sphx_blocks((size_t)ctx->n, INS_WG)), dim3(INS_WG), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    const CopyF64 ds[] = {{pos, a.pos, 3 * nr}, {vel, a.vel, 3 * nr}, {mass, a.om, nr}, {E_internal, a.oE, nr}, {f_un, a.of, nr * s}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 5));
    HIPCHK(hipStreamSynchronize(ctx->stream));       // (sorted and order are read by then)
    return SPHX_OK;
}

extern "C" int sphx_state_insert_rows(sphx_ctx* ctx, int s, int64_t n_rew, const int64_t* rew_ids, const double* rew_mass,
                                      const double* rew_E, const double* rew_f_un, int64_t n_app, const double* app_pos,
                                      const double* app_vel, const double* app_mass, const double* app_ptype, const double* app_E,
                                      const double* app_f_un, double t_cmb, const double* mu_specie, const double* gamma_specie,
                                      const double* grain_mass, const double* sigma_effective, int k, double dist) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_insert_rows";
    // ---- every refusal comes first: a refused call has written nothing ----
    SPHX_TRY(sphx_phase_need_list(ctx, who));
    const int64_t n = ctx->n;
    if (n_rew < 0 || n_app < 0) return sphx_set_err(ctx, SPHX_E_ARG, "%s: n_rew=%lld, n_app=%lld", who, (long long)n_rew, (long long)n_app);
    if (s < 1 || s > SPHX_MAX_SPECIES || (ctx->s > 0 && s != ctx->s))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: s=%d, the state carries %d species (need 1 <= s <= %d)", who, s, ctx->s, SPHX_MAX_SPECIES);
    if (k < 1 || k > SPHX_MAX_K) return sphx_set_err(ctx, SPHX_E_ARG, "%s: N_NEIGH=%d not in 1..%d", who, k, SPHX_MAX_K);
    if (n + n_app > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "%s: N + m = %lld is over the limit", who, (long long)(n + n_app));
    NEED(mu_specie); NEED(gamma_specie);
    if (n_rew > 0) { NEED(rew_ids); NEED(rew_mass); NEED(rew_E); NEED(rew_f_un); }
    if (n_app > 0) { NEED(app_pos); NEED(app_vel); NEED(app_mass); NEED(app_ptype); NEED(app_E); NEED(app_f_un); }
    if (t_cmb != t_cmb) return sphx_set_err(ctx, SPHX_E_ARG, "%s: t_cmb is NaN", who);
    SPHX_TRY(sphx_phase_check_tables(ctx, who, s, gamma_specie, grain_mass, sigma_effective));
    for (int q = 0; q < s; ++q)
        if (!sphx_finite(mu_specie[q])) return sphx_set_err(ctx, SPHX_E_ARG, "%s: table entry %d must be finite", who, q);
    for (int64_t e = 0; e < 3 * n_app; ++e)
        if (!sphx_finite(app_pos[e]))
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: the position of new row %lld is not finite", who, (long long)(e / 3));
    std::vector<int> sorted, order;
    SPHX_TRY(ins_sort_ids(ctx, who, n, n_rew, rew_ids, sorted, order));
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    // (the step's side stream may still read the radii for its sum of h: nothing of the state is freed under it)
    if (ctx->side_stream) HIPCHK(hipStreamSynchronize(ctx->side_stream));
    SPHX_TRY(ctx->ins_t.begin(ctx));
    const size_t nr = (size_t)n_rew, na = (size_t)n_app, S = (size_t)s;
    const bool drag = ctx->drag;
    // ---- the inputs in one staging block; doubles: rew_m | rew_E (nr) | rew_f (nr S) | app_pos | app_vel (na 3) | app_m |
    //      app_pt | app_E (na) | app_f (na S) | mus | gamma | gm | se (S); then the clamp count (u64) and the sorted ids.
    //      The one layout is bound twice: to the host's copy, which is filled here, then to the device's ----
    struct Stage { double *rew_m, *rew_E, *rew_f, *app_pos, *app_vel, *app_m, *app_pt, *app_E, *app_f, *tab; u64* moved; double* end; int* ids; };
    Stage dv;
    Carve c;
    c.take(dv.rew_m, nr); c.take(dv.rew_E, nr); c.take(dv.rew_f, nr * S); c.take(dv.app_pos, 3 * na); c.take(dv.app_vel, 3 * na);
    c.take(dv.app_m, na); c.take(dv.app_pt, na); c.take(dv.app_E, na); c.take(dv.app_f, na * S); c.take(dv.tab, 4 * S);
    c.take(dv.moved, 1); c.take(dv.end, 0); c.take(dv.ids, nr + 1);
    std::vector<double>& h = ctx->ins_host;          // (held by the context: the upload reads it)
    h.assign(c.bytes() / sizeof(double) + 1, 0.0);
    c.bind(h.data());
    const Stage hs = dv;
    double *h_rm = hs.rew_m, *h_rE = hs.rew_E, *h_rf = hs.rew_f, *h_ap = hs.app_pos, *h_av = hs.app_vel, *h_am = hs.app_m,
           *h_apt = hs.app_pt, *h_aE = hs.app_E, *h_af = hs.app_f, *h_tab = hs.tab;
    for (size_t r = 0; r < nr; ++r) {
        const size_t o = (size_t)order[r];
        h_rm[r] = rew_mass[o]; h_rE[r] = rew_E[o];
        memcpy(h_rf + r * S, rew_f_un + o * S, S * sizeof(double));
    }
    if (na) {
        memcpy(h_ap, app_pos, 3 * na * sizeof(double)); memcpy(h_av, app_vel, 3 * na * sizeof(double));
        memcpy(h_am, app_mass, na * sizeof(double)); memcpy(h_apt, app_ptype, na * sizeof(double));
        memcpy(h_aE, app_E, na * sizeof(double)); memcpy(h_af, app_f_un, na * S * sizeof(double));
    }
    for (size_t q = 0; q < S; ++q) {
        h_tab[q] = mu_specie[q]; h_tab[S + q] = gamma_specie[q];
        h_tab[2 * S + q] = drag ? grain_mass[q] : 0.0; h_tab[3 * S + q] = drag ? sigma_effective[q] : 0.0;
    }
    ctx->ins_ids = sorted;
    SPHX_TRY(sphx_carve_into(ctx, ctx->ins_in, c));
    HIPCHK(hipMemcpyAsync(dv.rew_m, h.data(), (size_t)(dv.end - dv.rew_m) * sizeof(double), hipMemcpyHostToDevice, stream));   // (the count's slot: zero)
    if (nr) HIPCHK(hipMemcpyAsync(dv.ids, ctx->ins_ids.data(), nr * sizeof(int), hipMemcpyHostToDevice, stream));
    SPHX_TRY(ctx->ins_t.mark(ctx, 1));
    // ---- a. grow, contents kept ----
    const int64_t n_new = n + n_app;
    StateArrays& st = ctx->st;
    DevBuf* f64s[] = {&st.x, &st.y, &st.z, &st.vx, &st.vy, &st.vz, &st.ax, &st.ay, &st.az, &st.m, &st.T, &st.mu, &st.gam, &st.E, &st.hprev,
                      &st.ptype, &st.mgm, &st.mcs};
    const int nf = drag ? 18 : 16;
    const bool has_fun = ctx->s > 0 && ctx->fun_id.p;
    std::vector<void*> retired;
    int grown = 0;
    int rc = SPHX_OK;
    for (int q = 0; q < nf && rc == SPHX_OK; ++q)
        rc = sphx_ensure_keep(ctx, *f64s[q], (size_t)n_new * sizeof(double), (size_t)n * sizeof(double), retired, &grown);
    if (rc == SPHX_OK) rc = sphx_ensure_keep(ctx, st.id, (size_t)n_new * sizeof(int), (size_t)n * sizeof(int), retired, &grown);
    if (rc == SPHX_OK && has_fun)
        rc = sphx_ensure_keep(ctx, ctx->fun_id, (size_t)n_new * ctx->sp * sizeof(double), (size_t)n * ctx->sp * sizeof(double), retired, &grown);
    if (rc == SPHX_OK) rc = sphx_star_ages_grow(ctx, n, n_new, retired);       // (the stellar clock, where it is set: sphx_census.hip)
    {
        const int rf = sphx_free_retired(ctx, retired);
        if (rc == SPHX_OK) rc = rf;
    }
    if (rc != SPHX_OK) return rc;                    // (every buffer still holds its N rows: the state stands)
    // the host's check, before the first kernel: every buffer the kernel writes holds N + m rows
    for (int q = 0; q < nf; ++q)
        if (!f64s[q]->p || f64s[q]->cap < (size_t)n_new * sizeof(double))
            return sphx_set_err(ctx, SPHX_E_STATE, "%s: state buffer %d holds %zu bytes, %lld rows need %zu", who, q, f64s[q]->cap,
                                (long long)n_new, (size_t)n_new * sizeof(double));
    if (!st.id.p || st.id.cap < (size_t)n_new * sizeof(int) || (has_fun && ctx->fun_id.cap < (size_t)n_new * ctx->sp * sizeof(double)))
        return sphx_set_err(ctx, SPHX_E_STATE, "%s: the id or composition buffer does not hold %lld rows", who, (long long)n_new);
    SPHX_TRY(ctx->ins_t.mark(ctx, 2));
    SPHX_TRY(sphx_star_ages_fill(ctx, n, n_new));                              // drv:371: -2 for every appended row
    // ---- b. one kernel over N + m rows ----
    InsertArgs a;
    a.n_old = (int)n; a.n_app = (int)n_app; a.n_rew = (int)n_rew; a.s = s; a.sp = has_fun ? ctx->sp : 0;
    a.x = st.x.as<double>(); a.y = st.y.as<double>(); a.z = st.z.as<double>();
    a.vx = st.vx.as<double>(); a.vy = st.vy.as<double>(); a.vz = st.vz.as<double>();
    a.ax = st.ax.as<double>(); a.ay = st.ay.as<double>(); a.az = st.az.as<double>();
    a.m = st.m.as<double>(); a.T = st.T.as<double>(); a.mu = st.mu.as<double>(); a.gam = st.gam.as<double>(); a.E = st.E.as<double>();
    a.hprev = st.hprev.as<double>(); a.ptype = st.ptype.as<double>(); a.id = st.id.as<int>();
    a.fun = has_fun ? ctx->fun_id.as<double>() : nullptr;
    a.mgm = drag ? st.mgm.as<double>() : nullptr; a.mcs = drag ? st.mcs.as<double>() : nullptr;
    a.rew_ids = dv.ids;
    a.rew_m = dv.rew_m; a.rew_E = dv.rew_E; a.rew_f = dv.rew_f;
    a.app_pos = dv.app_pos; a.app_vel = dv.app_vel; a.app_m = dv.app_m; a.app_pt = dv.app_pt; a.app_E = dv.app_E; a.app_f = dv.app_f;
    a.mus = dv.tab; a.gas = dv.tab + S; a.gm = dv.tab + 2 * S; a.se = dv.tab + 3 * S;
    a.t_cmb = t_cmb;
    a.moved = dv.moved;
    hipLaunchKernelGGL(insert_kernel, dim3(sphx_blocks((size_t)n_new, INS_WG)), dim3(INS_WG), 0, stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&ctx->pinned->scal[0], dv.moved, sizeof(u64), hipMemcpyDeviceToHost, stream));
    SPHX_TRY(ctx->ins_t.mark(ctx, 3));
    // ---- e. what no longer fits N + m ----
    ctx->n = n_new;
    ctx->npad = sphx_pad64(n_new);
    ctx->tprev_valid = false;
    ctx->nbr_api_valid = false;
    ctx->list_valid = false;
    ctx->sums_stale = true;
    // ---- c. drv:386 ----
    SPHX_TRY(sphx_step_research(ctx, k, dist));
    SPHX_TRY(ctx->ins_t.mark(ctx, 4));
    // ---- d. ----
    ctx->no_old_once = true;
    HIPCHK(hipStreamSynchronize(stream));
    ctx->ins_info[0] = grown; ctx->ins_info[1] = n_app; ctx->ins_info[2] = n_rew; ctx->ins_info[3] = (int64_t)ctx->pinned->scal[0];
    return ctx->ins_t.end(ctx);
}

extern "C" int sphx_insert_last_info(sphx_ctx* ctx, int64_t info[4]) {
    if (!ctx || !info) return SPHX_E_ARG;
    for (int i = 0; i < 4; ++i) info[i] = ctx->ins_info[i];
    return SPHX_OK;
}
