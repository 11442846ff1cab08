// sphx_api.hip - the C ABI of include/sphx.h: context, host-pointer entry points that mirror
// the reference's Python callables, and the device-resident step loop.
#include "sphx_internal.h"
#include <stdarg.h>
#include <stdlib.h>
#include <new>

int sphx_set_err(sphx_ctx* ctx, int code, const char* fmt, ...) {
    if (ctx) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

void sphx_release(sphx_ctx* ctx, DevBuf& b) {
    for (size_t q = 0; q < ctx->allocs.size(); ++q)
        if (ctx->allocs[q] == b.p) { ctx->allocs[q] = ctx->allocs.back(); ctx->allocs.pop_back(); break; }
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

int sphx_ensure(sphx_ctx* ctx, DevBuf& b, size_t bytes, hipStream_t in_use_on) {
    if (bytes == 0) bytes = 8;
    if (b.cap >= bytes) return SPHX_OK;
    if (b.p) {
        // buffers may still be referenced by queued work
        HIPCHK(hipStreamSynchronize(in_use_on));
        sphx_release(ctx, b);
    }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return sphx_set_err(ctx, SPHX_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    b.cap = want;
    ctx->allocs.push_back(b.p);
    return SPHX_OK;
}

// The keeping variant (sphx_insert.hip: the state grows and its rows stay): the new allocation is made first, the first
// `keep` bytes are copied device to device on the context's stream, and the outgrown allocation is handed to `retired` -
// the caller frees those (sphx_free_retired) once the stream has passed the copies.  Inside the head-room nothing happens.
int sphx_ensure_keep(sphx_ctx* ctx, DevBuf& b, size_t bytes, size_t keep, std::vector<void*>& retired, int* grown) {
    if (bytes == 0) bytes = 8;
    if (b.cap >= bytes) return SPHX_OK;
    const size_t want = bytes + bytes / 8 + 256;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) return sphx_set_err(ctx, SPHX_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    if (b.p && keep > 0) {
        if (keep > b.cap) keep = b.cap;
        e = hipMemcpyAsync(p, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return sphx_set_err(ctx, SPHX_E_HIP, "sphx_ensure_keep: copy failed: %s", hipGetErrorString(e));
        }
    }
    if (b.p) {
        for (size_t q = 0; q < ctx->allocs.size(); ++q)
            if (ctx->allocs[q] == b.p) { ctx->allocs[q] = ctx->allocs.back(); ctx->allocs.pop_back(); break; }
        retired.push_back(b.p);
    }
    b.p = p;
    b.cap = want;
    ctx->allocs.push_back(p);
    if (grown) ++*grown;
    return SPHX_OK;
}
int sphx_free_retired(sphx_ctx* ctx, std::vector<void*>& retired) {
    if (retired.empty()) return SPHX_OK;
    hipError_t e = hipStreamSynchronize(ctx->stream);          // the copies out of them are done
    for (void* p : retired) (void)hipFree(p);
    retired.clear();
    if (e != hipSuccess) return sphx_set_err(ctx, SPHX_E_HIP, "sphx_free_retired: %s", hipGetErrorString(e));
    return SPHX_OK;
}

static void default_constants(sphx_constants* c) {
    c->k_B = 1.380649e-23;
    c->amu = 1.66053906892e-27;
    c->m_h = 1.0008 * c->amu;
    c->m_0 = 31.622776601683793 * 1.989e30;          // 10**1.5 * solar_mass, nsc:36
    c->dt_0 = 60. * 60. * 24. * 365. * 250000.;
    c->max_age = 3e7 * 60. * 60. * 24. * 365.;
    c->pos_clamp = 1e11 * 149597870700.0;
    c->solar_luminosity = 3.846e26;
    c->c = 299792458.0;
}

extern "C" int sphx_version(void) { return 100; }

// How this library was built, and what a context read from the environment when it was created (bench.py puts both into
// its line).  "experiments=0": no result-changing or extra-launch switches exist in the library.
extern "C" const char* sphx_build_info(void) { return "gfx950 experiments=0"; }
extern "C" const char* sphx_tunables(const sphx_ctx* ctx) { return ctx ? ctx->tunables : ""; }

extern "C" int sphx_host_alloc(void** out, size_t bytes) {
    if (!out) return SPHX_E_ARG;
    *out = nullptr;
    if (bytes == 0) bytes = 8;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return SPHX_E_NOMEM;
    }
    return SPHX_OK;
}
extern "C" int sphx_host_free(void* p) {
    if (p && hipHostFree(p) != hipSuccess) return SPHX_E_HIP;
    return SPHX_OK;
}

// The step's main stream and its side stream (state permutation's second half, record build, h sums, read-backs).
// The main stream at the device's highest priority, the side stream at its lowest: what the step waits for is dispatched
// first (step 1.257 -> 1.242 ms, four runs each, against both at the default priority).
static hipError_t sphx_stream_create(hipStream_t* st, int side) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, side ? least : greatest);
}

extern "C" int sphx_create(sphx_ctx** out, int device) {
    if (!out) return SPHX_E_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) {
        fprintf(stderr, "sphx_create: no usable HIP device %d (found %d). libsphx has no CPU path.\n",
                device, count);
        return SPHX_E_HIP;
    }
    sphx_ctx* ctx = new (std::nothrow) sphx_ctx();
    if (!ctx) return SPHX_E_NOMEM;
    ctx->device = device;
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    memset(&ctx->grid, 0, sizeof(ctx->grid));
    default_constants(&ctx->cst);
    // Tunables: read from the environment ONCE, here, and recorded (sphx_tunables): a bench line can show the
    // configuration it ran.  None of them changes a result.  The switches between two forms of a kernel or a pass
    // (SPHX_KNN_GROUP, SPHX_BLOB, SPHX_LDS, SPHX_SPECIES_FUSED ...) are pinned bit for bit to the default by the tests;
    // the rest are numeric tuning knobs that steer performance only.
    auto env = [&](const char* name) -> const char* {
        const char* e = getenv(name);
        if (e) {
            const size_t used = strlen(ctx->tunables);
            snprintf(ctx->tunables + used, sizeof(ctx->tunables) - used, "%s%s=%s", used ? " " : "", name, e);
        }
        return e;
    };
    if (const char* e = env("SPHX_RSCALE")) { double v = atof(e); if (v >= 1.0) ctx->rscale = v; }
    if (const char* e = env("SPHX_CELL")) { double v = atof(e); if (v > 0.0) ctx->cell_factor = v; }
    if (const char* e = env("SPHX_RSCALE_BUILD")) { double v = atof(e); if (v >= 1.0) ctx->rscale_build = v; }
    if (const char* e = env("SPHX_VERLET")) ctx->use_verlet = atoi(e) != 0;
    if (const char* e = env("SPHX_BLOB")) ctx->use_blob = atoi(e) != 0;
    if (const char* e = env("SPHX_BLOB_CURVE")) ctx->blob_curve = atoi(e);
    if (const char* e = env("SPHX_KNN_GROUP")) ctx->use_group = atoi(e) != 0;
    if (const char* e = env("SPHX_HCLIP")) { double v = atof(e); if (v > 1.0) ctx->h_clip_factor = v; }
    if (const char* e = env("SPHX_TIMING_DETAIL")) ctx->timing_detail = atoi(e) != 0;
    if (const char* e = env("SPHX_MAX_CELLS")) { long long v = atoll(e); if (v > 0) ctx->max_cells = v; }
    if (const char* e = env("SPHX_CELL_FEEDBACK")) ctx->cell_feedback = atoi(e) != 0;
    if (const char* e = env("SPHX_CELL_FB_HI")) ctx->cell_fb_hi = atof(e);
    if (const char* e = env("SPHX_CELL_FB_LO")) ctx->cell_fb_lo = atof(e);
    if (const char* e = env("SPHX_DRAG_LDS")) ctx->drag_lds = atoi(e) != 0;
    if (const char* e = env("SPHX_BLOB_SPLIT")) ctx->blob_split_on = atoi(e) != 0;
    if (const char* e = env("SPHX_SPECIES_FUSED")) ctx->species_fused = atoi(e) != 0;
    if (const char* e = env("SPHX_SPECIES_LDS")) ctx->species_lds = atoi(e) != 0;
    if (const char* e = env("SPHX_HINT_DISTRUST")) ctx->distrust_mode = atoi(e);     // 0 never, 1 always, 2 auto
    if (const char* e = env("SPHX_OUTLIER_LEVELS")) ctx->olev_mode = atoi(e);     // 0 off, 1 always, 2 when far queries were met
    if (const char* e = env("SPHX_BOX_SIGMAS")) { double v = atof(e); if (v >= 1.0) ctx->box_sigmas = v; }
    if (const char* e = env("SPHX_GRAV_KERNEL")) ctx->grav_per_thread = atoi(e) == 0;
    if (const char* e = env("SPHX_GRAV_ORDER")) { int v = atoi(e); if (v == 1 || v == 2) ctx->grav_order = v; }
    if (const char* e = env("SPHX_GRAV_WS")) { int v = atoi(e); if (v >= 1 && v <= 4) ctx->grav_ws = v; }
    if (const char* e = env("SPHX_LDS")) ctx->use_lds = atoi(e) != 0;
    if (const char* e = env("SPHX_BLOB_SLOTS")) ctx->blob_slots = atoi(e);
    if (const char* e = env("SPHX_BLOB_WGS")) {      // workgroups per CU of the LDS passes' persistent grid
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
        if (atoi(e) > 0) ctx->blob_grid = ((cus * atoi(e) + 7) / 8) * 8;
    }
    bool ok = hipSetDevice(device) == hipSuccess &&
              sphx_stream_create(&ctx->stream, 0) == hipSuccess &&
              hipHostMalloc((void**)&ctx->pinned, sizeof(PinnedLayout), hipHostMallocDefault) == hipSuccess;
    ctx->own_stream = ctx->stream;
    for (int i = 0; ok && i < 10; ++i) ok = hipEventCreate(&ctx->ev[i]) == hipSuccess;
    for (int r = 0; ok && r < 3; ++r)
        for (int i = 0; ok && i < 10; ++i) ok = hipEventCreate(&ctx->evring[r][i]) == hipSuccess;
    for (int r = 0; ok && r < 2; ++r)
        ok = hipEventCreateWithFlags(&ctx->lag_bev[r], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&ctx->lag_hev[r], hipEventDisableTiming) == hipSuccess;
    if (ok) ok = sphx_stream_create(&ctx->side_stream, 1) == hipSuccess &&
                 hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&ctx->ev_perm, hipEventDisableTiming) == hipSuccess;
    if (ok) ok = sphx_ensure(ctx, ctx->scal, SC_NSLOTS * 8) == SPHX_OK &&
                 hipMemsetAsync(ctx->scal.p, 0, SC_NSLOTS * 8, ctx->stream) == hipSuccess &&
                 sphx_ensure(ctx, ctx->badc, (size_t)BADC_BUCKETS * BADC_STRIDE * sizeof(u64)) == SPHX_OK &&
                 hipMemsetAsync(ctx->badc.p, 0, (size_t)BADC_BUCKETS * BADC_STRIDE * sizeof(u64), ctx->stream) == hipSuccess;
    if (!ok) {
        fprintf(stderr, "sphx_create: HIP initialisation failed on device %d\n", device);
        delete ctx;
        return SPHX_E_HIP;
    }
    *out = ctx;
    return SPHX_OK;
}

extern "C" void sphx_destroy(sphx_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (void* p : ctx->allocs) (void)hipFree(p);
    for (int i = 0; i < 10; ++i)
        if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    for (int i = 0; i <= SPHX_SN_STAGES; ++i)
        if (ctx->sn_ev[i]) (void)hipEventDestroy(ctx->sn_ev[i]);
    for (int r = 0; r < 3; ++r)
        for (int i = 0; i < 10; ++i)
            if (ctx->evring[r][i]) (void)hipEventDestroy(ctx->evring[r][i]);
    for (int r = 0; r < 2; ++r) {
        if (ctx->lag_bev[r]) (void)hipEventDestroy(ctx->lag_bev[r]);
        if (ctx->lag_hev[r]) (void)hipEventDestroy(ctx->lag_hev[r]);
    }
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->olev_ev) (void)hipEventDestroy(ctx->olev_ev);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_perm) (void)hipEventDestroy(ctx->ev_perm);
    if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" const char* sphx_last_error(const sphx_ctx* ctx) { return ctx ? ctx->err : "null context"; }

extern "C" int sphx_set_constants(sphx_ctx* ctx, const sphx_constants* c) {
    if (!ctx || !c) return SPHX_E_ARG;
    ctx->cst = *c;
    return SPHX_OK;
}
extern "C" int sphx_set_tuning(sphx_ctx* ctx, double rscale, double cell_factor) {
    if (!ctx) return SPHX_E_ARG;
    if (rscale > 0.0) {
        if (rscale < 1.0) return sphx_set_err(ctx, SPHX_E_ARG, "rscale %g < 1", rscale);
        ctx->rscale = rscale;
    }
    if (cell_factor > 0.0) ctx->cell_factor = cell_factor;
    return SPHX_OK;
}
extern "C" int sphx_set_incremental(sphx_ctx* ctx, int verlet, double rscale_build) {
    if (!ctx) return SPHX_E_ARG;
    ctx->use_verlet = verlet != 0;
    if (!ctx->use_verlet) ctx->list_valid = false;
    if (rscale_build > 0.0) {
        if (rscale_build < 1.0) return sphx_set_err(ctx, SPHX_E_ARG, "rscale_build %g < 1", rscale_build);
        ctx->rscale_build = rscale_build;
    }
    return SPHX_OK;
}
extern "C" int sphx_get_constants(const sphx_ctx* ctx, sphx_constants* c) {
    if (!ctx || !c) return SPHX_E_ARG;
    *c = ctx->cst;
    return SPHX_OK;
}

// ---- staging helpers ------------------------------------------------------------------------
static int upload(sphx_ctx* ctx, DevBuf& b, const void* host, size_t bytes) {
    SPHX_TRY(sphx_ensure(ctx, b, bytes));
    HIPCHK(hipMemcpyAsync(b.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return SPHX_OK;
}
static int download(sphx_ctx* ctx, void* host, const void* dev, size_t bytes) {
    if (!host) return SPHX_OK;
    HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return SPHX_OK;
}
int sphx_upload_f64(sphx_ctx* ctx, const CopyF64* t, int nt) {
    for (int i = 0; i < nt; ++i)
        if (t[i].host)
            HIPCHK(hipMemcpyAsync(const_cast<void*>(t[i].dev), t[i].host, t[i].count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return SPHX_OK;
}
int sphx_download_f64(sphx_ctx* ctx, const CopyF64* t, int nt) {
    for (int i = 0; i < nt; ++i)
        if (t[i].host && t[i].dev && t[i].count > 0)
            HIPCHK(hipMemcpyAsync(const_cast<void*>(t[i].host), t[i].dev, t[i].count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    return SPHX_OK;
}

// ---- the side calls' stage timer ----------------------------------------------------------------
int StageTimer::begin(sphx_ctx* ctx) {
    for (int i = 0; i <= stages; ++i)
        if (!ev[i]) HIPCHK(hipEventCreate(&ev[i]));
    for (int i = 0; i < stages; ++i) ms[i] = 0.0;
    return mark(ctx, 0);
}
int StageTimer::mark(sphx_ctx* ctx, int i) {
    HIPCHK(hipEventRecord(ev[i], ctx->stream));
    return SPHX_OK;
}
int StageTimer::end(sphx_ctx* ctx) {
    for (int i = 0; i < stages; ++i) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
        ms[i] = t;
    }
    return SPHX_OK;
}
extern "C" int sphx_arb_last_timing(sphx_ctx* ctx, double ms[4]) { return last_timing(ctx, &sphx_ctx::arb_t, ms); }
extern "C" int sphx_rad_last_timing(sphx_ctx* ctx, double ms[4]) { return last_timing(ctx, &sphx_ctx::rad_t, ms); }
extern "C" int sphx_cool_last_timing(sphx_ctx* ctx, double ms[4]) { return last_timing(ctx, &sphx_ctx::cool_t, ms); }
extern "C" int sphx_dust_last_timing(sphx_ctx* ctx, double ms[4]) { return last_timing(ctx, &sphx_ctx::dust_t, ms); }
extern "C" int sphx_chem_last_timing(sphx_ctx* ctx, double ms[5]) { return last_timing(ctx, &sphx_ctx::chem_t, ms); }
extern "C" int sphx_phase_last_timing(sphx_ctx* ctx, double ms[5]) { return last_timing(ctx, &sphx_ctx::phase_t, ms); }
extern "C" int sphx_state_radphase_last_timing(sphx_ctx* ctx, double ms[5]) { return last_timing(ctx, &sphx_ctx::radstate_t, ms); }
extern "C" int sphx_radphase_last_timing(sphx_ctx* ctx, double ms[4]) { return last_timing(ctx, &sphx_ctx::radphase_t, ms); }
extern "C" int sphx_insert_last_timing(sphx_ctx* ctx, double ms[4]) { return last_timing(ctx, &sphx_ctx::ins_t, ms); }
extern "C" int sphx_gravpot_last_timing(sphx_ctx* ctx, double ms[4]) { return last_timing(ctx, &sphx_ctx::gravpot_t, ms); }

// =============================================================================================
// nsc.neighbors                                                                nsc:541-552
// =============================================================================================
extern "C" int sphx_neighbors(sphx_ctx* ctx, int64_t n, int k, const double* points, double dist,
                              double eps, int64_t* idx, double* dist_out, int64_t* nontriv,
                              double* h) {
    (void)eps;
    if (!ctx) return SPHX_E_ARG;
    NEED(points);
    if (n < 1) return sphx_set_err(ctx, SPHX_E_ARG, "n=%lld < 1", (long long)n);
    if (k < 1 || k > SPHX_MAX_K) return sphx_set_err(ctx, SPHX_E_ARG, "N_NEIGH=%d not in 1..%d", k, SPHX_MAX_K);
    HIPCHK(hipSetDevice(ctx->device));
    ctx->map_perm = nullptr;
    ctx->qorder = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    SPHX_TRY(upload(ctx, ctx->in_a, points, 3 * nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->in_b, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->in_c, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->in_d, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->in_e, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->in_f, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->in_g, nb));
    double *x = ctx->in_b.as<double>(), *y = ctx->in_c.as<double>(), *z = ctx->in_d.as<double>();
    double *xs = ctx->in_e.as<double>(), *ys = ctx->in_f.as<double>(), *zs = ctx->in_g.as<double>();
    SPHX_TRY(sphx_aos_to_soa3(ctx, n, ctx->in_a.as<double>(), x, y, z));
    ctx->clip_valid = false;                 // a fresh point set: no history for the robust box
    SPHX_TRY(sphx_build_grid(ctx, n, k, x, y, z, 0.0));
    SPHX_TRY(sphx_gather3(ctx, n, ctx->perm.as<int>(), x, y, z, xs, ys, zs));
    SPHX_TRY(sphx_ensure(ctx, ctx->idx64, (size_t)n * k * sizeof(int64_t)));
    SPHX_TRY(sphx_ensure(ctx, ctx->dist_out, (size_t)n * k * sizeof(double)));
    SPHX_TRY(sphx_ensure(ctx, ctx->nontriv, (size_t)n * sizeof(int64_t)));
    SPHX_TRY(sphx_ensure(ctx, ctx->h_api, nb));
    KnnOut o;
    o.nbr = nullptr; o.h_sorted = nullptr;
    o.idx64 = ctx->idx64.as<int64_t>(); o.dist = ctx->dist_out.as<double>();
    o.nontriv = ctx->nontriv.as<int64_t>(); o.h_by_id = ctx->h_api.as<double>();
    KnnIn in;
    in.xs = xs; in.ys = ys; in.zs = zs;
    in.id = ctx->perm.as<int>();             // sorted -> original index is the permutation itself
    in.rbound = dist;
    SPHX_TRY(sphx_knn(ctx, n, k, in, o));
    SPHX_TRY(download(ctx, idx, o.idx64, (size_t)n * k * sizeof(int64_t)));
    SPHX_TRY(download(ctx, dist_out, o.dist, (size_t)n * k * sizeof(double)));
    SPHX_TRY(download(ctx, nontriv, o.nontriv, (size_t)n * sizeof(int64_t)));
    SPHX_TRY(download(ctx, h, o.h_by_id, nb));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPHX_OK;
}

// =============================================================================================
// nsc.hydro_update                                                             nsc:556-671
// =============================================================================================
extern "C" int sphx_hydro_update(sphx_ctx* ctx, int64_t n, int k, int s, const int64_t* neighbor,
                                 const double* points, const double* mass, const double* sizes,
                                 const double* f_un, const double* particle_type, const double* T,
                                 const double* mu_array, const double* gamma_array,
                                 const double* velocities, int visc_mode, double* hydro_accel,
                                 double* visc_accel, double* visc_heat, double* rho, double* nden,
                                 double* f_un_nb, double* rho_dust) {
    if (!ctx) return SPHX_E_ARG;
    NEED(points); NEED(mass); NEED(sizes); NEED(particle_type); NEED(T);
    NEED(mu_array); NEED(gamma_array); NEED(velocities);
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "n=%lld out of range", (long long)n);
    if (k < 1 || k > 4096) return sphx_set_err(ctx, SPHX_E_ARG, "k=%d out of range", k);
    if (visc_mode != 0 && visc_mode != 1)
        return sphx_set_err(ctx, SPHX_E_ARG, "visc_mode %d unknown (0 = ref_axis0, 1 = pairwise)", visc_mode);
    if (f_un_nb && (!f_un || s < 1 || s > SPHX_MAX_SPECIES))
        return sphx_set_err(ctx, SPHX_E_ARG, "species output needs f_un and 1 <= s <= %d", SPHX_MAX_SPECIES);
    HIPCHK(hipSetDevice(ctx->device));
    ctx->map_perm = nullptr;
    ctx->qorder = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    if (!neighbor && !(ctx->nbr_api_valid && ctx->nbr_api_n == n && ctx->nbr_api_k == k))
        return sphx_set_err(ctx, SPHX_E_STATE, "neighbor == NULL but no (%lld, %d) list is held from a previous call",
                            (long long)n, k);
    if (neighbor) SPHX_TRY(upload(ctx, ctx->idx64, neighbor, (size_t)n * k * sizeof(int64_t)));
    SPHX_TRY(upload(ctx, ctx->in_a, points, 3 * nb));
    SPHX_TRY(upload(ctx, ctx->in_b, velocities, 3 * nb));
    SPHX_TRY(upload(ctx, ctx->in_c, mass, nb));
    SPHX_TRY(upload(ctx, ctx->in_d, sizes, nb));
    SPHX_TRY(upload(ctx, ctx->in_e, T, nb));
    SPHX_TRY(upload(ctx, ctx->in_f, mu_array, nb));
    SPHX_TRY(upload(ctx, ctx->in_g, gamma_array, nb));
    SPHX_TRY(upload(ctx, ctx->in_h, particle_type, nb));
    if (neighbor) {
        SPHX_TRY(sphx_transpose_nbr(ctx, n, k, ctx->idx64.as<int64_t>()));
        ctx->nbr_api_valid = true; ctx->nbr_api_n = n; ctx->nbr_api_k = k;
    }
    PrepIn pin;
    pin.pos_aos(ctx->in_a.as<double>()); pin.vel_aos(ctx->in_b.as<double>());
    pin.m = ctx->in_c.as<double>(); pin.h = ctx->in_d.as<double>(); pin.T = ctx->in_e.as<double>();
    pin.mu = ctx->in_f.as<double>(); pin.gam = ctx->in_g.as<double>(); pin.ptype = ctx->in_h.as<double>();
    // (pairwise: the call's own argument; the context's step mode plays no part)
    SPHX_TRY(sphx_prep(ctx, n, pin, visc_mode == 1, ctx->stream));
    SPHX_TRY(sphx_pass_density(ctx, n, k));
    if (visc_mode == 1) {
        SPHX_TRY(sphx_pass_visc_pw(ctx, n, k, ctx->in_c.as<double>()));
    } else {
        SPHX_TRY(sphx_pass_pi(ctx, n, k, ctx->in_d.as<double>(), ctx->in_h.as<double>()));
        SPHX_TRY(sphx_pass_visc(ctx, n, k, ctx->in_c.as<double>()));
    }
    if (f_un_nb) {
        SPHX_TRY(upload(ctx, ctx->in_i, f_un, (size_t)n * s * sizeof(double)));
        SPHX_TRY(sphx_ensure(ctx, ctx->F, (size_t)n * s * sizeof(double)));
        SPHX_TRY(sphx_pass_species(ctx, n, k, s, ctx->in_i.as<double>(), ctx->F.as<double>()));
        SPHX_TRY(download(ctx, f_un_nb, ctx->F.p, (size_t)n * s * sizeof(double)));
    }
    SPHX_TRY(download(ctx, hydro_accel, ctx->ha.p, 3 * nb));
    SPHX_TRY(download(ctx, visc_accel, ctx->va.p, 3 * nb));
    SPHX_TRY(download(ctx, visc_heat, ctx->vh.p, nb));
    SPHX_TRY(download(ctx, rho, ctx->rho.p, nb));
    SPHX_TRY(download(ctx, nden, ctx->nden.p, nb));
    SPHX_TRY(download(ctx, rho_dust, ctx->rhod.p, nb));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPHX_OK;
}

// =============================================================================================
// device-resident state + step                                       drv:217-238, 437-491
// =============================================================================================
extern "C" int sphx_state_upload(sphx_ctx* ctx, int64_t n, int s, const double* pos, const double* vel,
                                 const double* mass, const double* ptype, const double* f_un,
                                 const double* T, const double* mu, const double* gamma,
                                 const double* E_internal, const double* accel_old) {
    if (!ctx) return SPHX_E_ARG;
    NEED(pos); NEED(vel); NEED(mass); NEED(ptype); NEED(T); NEED(mu); NEED(gamma); NEED(E_internal);
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "n=%lld out of range", (long long)n);
    if (f_un && (s < 1 || s > SPHX_MAX_SPECIES)) return sphx_set_err(ctx, SPHX_E_ARG, "s=%d out of range", s);
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nb = (size_t)n * sizeof(double);
    StateArrays& st = ctx->st;
    DevBuf* scal[] = {&st.x, &st.y, &st.z, &st.vx, &st.vy, &st.vz, &st.ax, &st.ay, &st.az,
                      &st.m, &st.T, &st.mu, &st.gam, &st.E, &st.hprev, &st.ptype};
    for (DevBuf* b : scal) SPHX_TRY(sphx_ensure(ctx, *b, nb));
    SPHX_TRY(sphx_ensure(ctx, st.id, (size_t)n * sizeof(int)));
    SPHX_TRY(upload(ctx, ctx->in_a, pos, 3 * nb));
    SPHX_TRY(sphx_aos_to_soa3(ctx, n, ctx->in_a.as<double>(), st.x.as<double>(), st.y.as<double>(), st.z.as<double>()));
    SPHX_TRY(upload(ctx, ctx->in_b, vel, 3 * nb));
    SPHX_TRY(sphx_aos_to_soa3(ctx, n, ctx->in_b.as<double>(), st.vx.as<double>(), st.vy.as<double>(), st.vz.as<double>()));
    if (accel_old) {
        SPHX_TRY(upload(ctx, ctx->in_c, accel_old, 3 * nb));
        SPHX_TRY(sphx_aos_to_soa3(ctx, n, ctx->in_c.as<double>(), st.ax.as<double>(), st.ay.as<double>(), st.az.as<double>()));
    } else {
        HIPCHK(hipMemsetAsync(st.ax.p, 0, nb, ctx->stream));
        HIPCHK(hipMemsetAsync(st.ay.p, 0, nb, ctx->stream));
        HIPCHK(hipMemsetAsync(st.az.p, 0, nb, ctx->stream));
    }
    HIPCHK(hipMemcpyAsync(st.m.p, mass, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(st.T.p, T, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(st.mu.p, mu, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(st.gam.p, gamma, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(st.E.p, E_internal, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(st.ptype.p, ptype, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(st.hprev.p, 0, nb, ctx->stream));
    SPHX_TRY(sphx_iota(ctx, n, st.id.as<int>()));
    ctx->s = 0;
    if (f_un) {
        // rows padded to whole 128-B lines (16 doubles for the reference's 15 species): one aligned line per neighbour
        // in the species pass; kept in upload order (ctx->fun_id): the pass reaches a row through the particle's id
        const int sp = (s + 15) & ~15;
        SPHX_TRY(upload(ctx, ctx->in_d, f_un, (size_t)n * s * sizeof(double)));
        SPHX_TRY(sphx_ensure(ctx, ctx->fun_id, (size_t)n * sp * sizeof(double)));
        HIPCHK(hipMemsetAsync(ctx->fun_id.p, 0, (size_t)n * sp * sizeof(double), ctx->stream));
        HIPCHK(hipMemcpy2DAsync(ctx->fun_id.p, (size_t)sp * sizeof(double), ctx->in_d.p, (size_t)s * sizeof(double),
                                (size_t)s * sizeof(double), (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->s = s;
        ctx->sp = sp;
    }
    HIPCHK(hipMemsetAsync(ctx->scal.p, 0, SC_NSLOTS * 8, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->badc.p, 0, (size_t)BADC_BUCKETS * BADC_STRIDE * sizeof(u64), ctx->stream));
    ctx->ct_primed = false;       // SC_CT_BITS was just zeroed: the next pass 2 must prime it again
    ctx->nbr_api_valid = false;
    sphx_step_list_drop(ctx);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->n = n;
    ctx->npad = sphx_pad64(n);
    ctx->has_state = true;
    ctx->drag = false;
    ctx->agb_on = false;
    ctx->gravity = 0;
    ctx->loop_forms = 0;
    ctx->list_valid = false;
    ctx->clip_valid = false;
    ctx->h_clip = 0.0;
    ctx->lag_bvalid[0] = ctx->lag_bvalid[1] = ctx->lag_hvalid[0] = ctx->lag_hvalid[1] = false;
    ctx->step_count = 0;
    ctx->tprev_valid = false;
    ctx->dt_last = 0.0;
    ctx->no_old_once = false;
    ctx->sums_stale = false;
    ctx->visc_rows_unfilled = false;
    ctx->scale_sizes_valid = false; ctx->scale_d0_valid = false;       // (sphx_scale.hip)
    ctx->star_ages_valid = false;                                      // (sphx_census.hip)
    return SPHX_OK;
}

extern "C" int sphx_state_set_drag(sphx_ctx* ctx, const double* mean_grain_mass, const double* mean_cross) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state || ctx->step_count != 0)
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_set_drag must follow sphx_state_upload directly");
    HIPCHK(hipSetDevice(ctx->device));
    if (!mean_grain_mass || !mean_cross) { ctx->drag = false; return SPHX_OK; }
    const size_t nb = (size_t)ctx->n * sizeof(double);
    SPHX_TRY(sphx_ensure(ctx, ctx->st.mgm, nb));
    SPHX_TRY(sphx_ensure(ctx, ctx->st.mcs, nb));
    HIPCHK(hipMemcpyAsync(ctx->st.mgm.p, mean_grain_mass, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->st.mcs.p, mean_cross, nb, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->drag = true;
    return SPHX_OK;
}

extern "C" int sphx_state_set_loop_forms(sphx_ctx* ctx, int on, double d) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_set_loop_forms before sphx_state_upload");
    if (on && !(d > 0.0)) return sphx_set_err(ctx, SPHX_E_ARG, "the loop forms need the driver's global d > 0 (drv:68)");
    if (on && ctx->use_verlet) return sphx_set_err(ctx, SPHX_E_STATE, "loop-form steps are not combined with incremental search");
    if (on && ctx->visc_mode != 0)
        return sphx_set_err(ctx, SPHX_E_ARG, "loop-form steps have their own (pairwise) viscosity: visc_mode must be 0");
    ctx->loop_forms = on ? 1 : 0;
    ctx->loop_d = d;
    return SPHX_OK;
}

extern "C" int sphx_set_gravity_order(sphx_ctx* ctx, int order) {
    if (!ctx) return SPHX_E_ARG;
    if (order != 1 && order != 2) return sphx_set_err(ctx, SPHX_E_ARG, "gravity order %d not 1 (monopole) or 2 (quadrupole)", order);
    ctx->grav_order = order;
    return SPHX_OK;
}

extern "C" int sphx_set_clip_grad(sphx_ctx* ctx, int on) {
    if (!ctx) return SPHX_E_ARG;
    ctx->clip_grad = on ? 1 : 0;
    return SPHX_OK;
}

extern "C" int sphx_set_visc_mode(sphx_ctx* ctx, int mode) {
    if (!ctx) return SPHX_E_ARG;
    if (mode != 0 && mode != 1)
        return sphx_set_err(ctx, SPHX_E_ARG, "visc_mode %d unknown (0 = ref_axis0, 1 = pairwise)", mode);
    if (mode != 0 && ctx->loop_forms)
        return sphx_set_err(ctx, SPHX_E_ARG, "loop-form steps have their own (pairwise) viscosity: visc_mode must be 0");
    ctx->visc_mode = mode;
    return SPHX_OK;
}

extern "C" int sphx_state_set_gravity(sphx_ctx* ctx, int mode, double G) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_set_gravity before sphx_state_upload");
    if (mode < 0 || mode > 2) return sphx_set_err(ctx, SPHX_E_ARG, "gravity mode %d not in {0, 1, 2}", mode);
    if (mode == 2 && ctx->use_verlet)
        return sphx_set_err(ctx, SPHX_E_STATE, "tree gravity needs the cell grid of every step: not with incremental search");
    ctx->gravity = mode;
    ctx->grav_G = G;
    return SPHX_OK;
}

// ---- one step of the fused loop, in three phases: grid + search, sums, gravity + update ----
static PrepIn prep_in_of_state(const StateArrays& s) {
    PrepIn in;
    in.x = s.x.as<double>(); in.y = s.y.as<double>(); in.z = s.z.as<double>(); in.ps = 1;
    in.vx = s.vx.as<double>(); in.vy = s.vy.as<double>(); in.vz = s.vz.as<double>(); in.vs = 1;
    in.m = s.m.as<double>(); in.h = s.hprev.as<double>(); in.T = s.T.as<double>();
    in.mu = s.mu.as<double>(); in.gam = s.gam.as<double>(); in.ptype = s.ptype.as<double>();
    return in;
}

// cell size of the next grid from the previous step's mean h (read back together with the search's counters); 0: none yet
static int step_cell_hint(sphx_ctx* ctx, int64_t n, double* cell_hint) {
    *cell_hint = 0.0;
    if (ctx->step_count == 0) return SPHX_OK;
    const double* hs;                                                  // [0] sum ... [3] count
    if (ctx->lag_hvalid[ctx->lag_hslot]) {
        // copied out right after the previous step's search: no wait on that step's tail
        HIPCHK(hipEventSynchronize(ctx->lag_halias[ctx->lag_hslot] ? ctx->lag_halias[ctx->lag_hslot]
                                                                     : ctx->lag_hev[ctx->lag_hslot]));
        hs = ctx->pinned->lag[ctx->lag_hslot].hs;
        // the same copy carries the previous search's counters
        const u64* sv = (const u64*)hs;           // slots SC_HSUM ..: [5] SC_NFAILQ [6] SC_SHORT [7] SC_FARQ [8] SC_BADHINT
        for (int q = 0; q < 10; ++q) ctx->knn_lag[q] = sv[(SC_NFAILQ - SC_HSUM) + q];      // .. SC_KGDBG + 2
        ctx->knn_lag_valid = true;
    } else {
        HIPCHK(hipMemcpyAsync(ctx->pinned->hsum, ctx->scal.as<double>() + SC_HSUM, sizeof(ctx->pinned->hsum),
                              hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        hs = ctx->pinned->hsum;
    }
    const double hmean = hs[3] > 0.0 ? hs[0] / hs[3] : 0.0;
    if (hmean > 0.0 && isfinite(hmean)) {
        // SPHX_CELL_FEEDBACK: when a sizeable share of the particles lives in cells of >= DENSE_CELL members (a core
        // much denser than the mean radius suggests: the 27 cells around a group overflow its tile and the search hands
        // the group's queries on), the cells shrink, 3 % a step; they relax again, 1 % a step, once that share is small.
        // (A property of the positions alone: every variant of the search sees the same grid.)
        *cell_hint = ctx->cell_factor * sphx_cell_feedback(ctx, n) * hmean;
        ctx->h_clip = ctx->h_clip_factor * hmean;
    }
    return SPHX_OK;
}

// Phase 1: the neighbour list of this step in ctx->nbr and the radii in st.hprev - refreshed from the Verlet lists, or by
// grid build, blob order, permutation of the state and search.  Records ev[1] in front of the search.
// fresh: the search of a state that has just grown (sphx_state_insert_rows, drv:386) - no radius is handed to it, as none
// is to the first step's.
static int step_search(sphx_ctx* ctx, int k, double dist, hipEvent_t* ev, bool fresh = false) {
    const int64_t n = ctx->n;
    // drv:233-238: applied by the grid build's first pass over the particles (sphx_grid.hip); the Verlet path looks at
    // the positions before any grid is built, so it clamps here
    if (ctx->use_verlet) SPHX_TRY(sphx_clamp(ctx, n, ctx->st));
    SPHX_TRY(sphx_ensure(ctx, ctx->nbr, (size_t)k * ctx->npad * sizeof(int)));
    // ---- incremental exact kNN from the Verlet lists (sphx_refresh.hip) ---------------------
    if (ctx->use_verlet && ctx->list_valid && ctx->list_n == n && ctx->list_k == k) {
        StateArrays& r = ctx->st;
        HIPCHK(hipEventRecord(ev[1], ctx->stream));
        int64_t nfail = 0;
        SPHX_TRY(sphx_knn_refresh(ctx, n, k, r.x.as<double>(), r.y.as<double>(), r.z.as<double>(),
                                  ctx->nbr.as<int>(), r.hprev.as<double>(), &nfail));
        if (nfail == 0) {
            ctx->stats.refresh_steps++;
            return SPHX_OK;
        }
        ctx->list_valid = false;         // some result could not be proven exact: rebuild
    }
    double cell_hint = 0.0;
    SPHX_TRY(step_cell_hint(ctx, n, &cell_hint));
    {
        StateArrays& r = ctx->st;       // the box statistics are the previous step's when there are any
        const bool blob = ctx->use_blob && !ctx->use_verlet;
        GridBuildOpts g;
        g.lagged = true;
        g.alias_ev = ev[1];               // (recorded below, behind the state's permutation)
        g.sort_cells_later = blob;        // the blob-order pass over the cells sorts their members too
        // ... or no pass over the cells at all: the scatter counts them along the curve, the gather below orders their
        // members, and the host's cues are counted on the side stream (sphx_permute_state, split)
        g.count_curve = blob && ctx->side_stream && ctx->ev_perm;
        if (!ctx->use_verlet) { g.clamp_vel[0] = r.vx.as<double>(); g.clamp_vel[1] = r.vy.as<double>(); g.clamp_vel[2] = r.vz.as<double>(); }
        SPHX_TRY(sphx_build_grid(ctx, n, k, r.x.as<double>(), r.y.as<double>(), r.z.as<double>(), cell_hint, g));
        // (the blob order needs cell_of / perm / cell_start only: before the state is permuted, so that the
        //  deferred member sort has run when perm is used; its last scatter: in sphx_permute_state's kernel, right below)
        if (blob) SPHX_TRY(sphx_build_blob_order(ctx, n, /*defer_scatter=*/true));
    }
    const bool split = ctx->side_stream && !ctx->use_verlet;
    SPHX_TRY(sphx_permute_state(ctx, n, split, ev[1]));      // (records ev[1] behind the search's part)
    StateArrays& r = ctx->st;
    KnnIn in;
    in.xs = r.x.as<double>(); in.ys = r.y.as<double>(); in.zs = r.z.as<double>();
    in.id = r.id.as<int>(); in.inv = ctx->inv.as<int>();
    in.rsearch = fresh ? nullptr : r.hprev.as<double>();
    in.hinted = !fresh && ctx->step_count > 0 && !ctx->use_verlet;     // hprev holds the previous step's radii
    in.lag_external = true;              // (step_cell_hint has handed the previous search's counters over)
    in.rscale = ctx->rscale;
    in.rbound = dist;
    KnnOut o;
    o.nbr = ctx->nbr.as<int>();
    o.h_sorted = r.hprev.as<double>();   // read as the search-radius hint, then overwritten
    o.idx64 = nullptr; o.dist = nullptr; o.nontriv = nullptr; o.h_by_id = nullptr;
    if (ctx->use_verlet) {
        SPHX_TRY(sphx_ensure(ctx, ctx->list64, (size_t)n * 64 * sizeof(int)));
        SPHX_TRY(sphx_ensure(ctx, ctx->dref, (size_t)n * sizeof(double)));
        o.list64 = ctx->list64.as<int>();
        o.dref = ctx->dref.as<double>();
        in.rscale = ctx->rscale_build;   // wider: the list must hold 64 entries to earn its margin
    }
    SPHX_TRY(sphx_knn(ctx, n, k, in, o));
    if (split) HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_perm, 0));    // the rest of the state is in place
    if (ctx->use_verlet) {
        SPHX_TRY(sphx_save_list_positions(ctx, n, r.x.as<double>(), r.y.as<double>(), r.z.as<double>()));
        ctx->list_valid = true;
        ctx->list_n = n;
        ctx->list_k = k;
    }
    ctx->stats.rebuild_steps++;
    return SPHX_OK;
}

// the sum of h on `stream` and its copy to the host: the next step's cell size, read there when the next grid is sized;
// the search's counters travel in the same copy (SC_HSUM .. SC_BADHINT are consecutive slots)
static int step_h_sums_out(sphx_ctx* ctx, int64_t n, const double* h, hipStream_t stream) {
    SPHX_TRY(sphx_hsum(ctx, n, h, stream));
    const int hsl = ctx->lag_hslot ^ 1;
    HIPCHK(hipMemcpyAsync(ctx->pinned->lag[hsl].hs, ctx->scal.as<double>() + SC_HSUM,
                          (SC_KGDBG + 2 - SC_HSUM + 1) * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipEventRecord(ctx->lag_hev[hsl], stream));
    ctx->lag_halias[hsl] = nullptr;
    ctx->lag_hvalid[hsl] = true;
    ctx->lag_hslot = hsl;
    return SPHX_OK;
}

// Phase 2: the sums of hydro_update (or the loop forms) on the list of phase 1.  search_end: the event recorded behind the search.
// *rows_by_byte: pass 2 left every row's class in ctx->row_settled and stored no NaNs for the settled rows - the update
// that follows has to take its rows by those bytes (sphx_update_rows.h)
static int step_sums(sphx_ctx* ctx, int k, hipEvent_t* ev, hipEvent_t search_end, bool detail, bool* rows_by_byte) {
    const int64_t n = ctx->n;
    *rows_by_byte = false;
    StateArrays& s = ctx->st;
    const bool pairwise = ctx->visc_mode == 1 && !ctx->loop_forms;     // (what sphx_prep builds RecBC.Bw for)
    // the record build (bandwidth-bound) does not depend on the list dedup (latency-bound): side by side on the side
    // stream - and behind it there the sum of h and its copy to the host (the passes wait for the records, not for
    // those; nobody but the next step's host code reads the sums)
    const bool fork = ctx->qorder && ctx->use_lds && !ctx->loop_forms && ctx->side_stream;
    if (fork) HIPCHK(hipStreamWaitEvent(ctx->side_stream, search_end, 0));       // (the search's end event doubles as the fork)
    else SPHX_TRY(step_h_sums_out(ctx, n, s.hprev.as<double>(), ctx->stream));
    if (ctx->qorder && ctx->use_lds) SPHX_TRY(sphx_blob_translate(ctx, n, k));
    const bool species = ctx->s > 0 && ctx->fun_id.p;      // nsc:624-627 on the step's list: the state carries f_un
    if (ctx->loop_forms) {
        // the reference's time loop (drv:451-458): loop forms on this step's neighbour list
        if (ctx->drag || species)          // (the species pass reads hydro_update's records, RecA)
            SPHX_TRY(sphx_prep(ctx, n, prep_in_of_state(s), pairwise, ctx->stream));
        if (detail) HIPCHK(hipEventRecord(ev[3], ctx->stream));
        SPHX_TRY(sphx_loop_step_sums(ctx, n, k, ctx->loop_d));
        if (detail) HIPCHK(hipEventRecord(ev[9], ctx->stream));
        if (species) SPHX_TRY(sphx_step_species(ctx, n, k));       // (+ metallicity, AGB yields)
        if (detail) HIPCHK(hipEventRecord(ev[4], ctx->stream));
        if (detail) HIPCHK(hipEventRecord(ev[5], ctx->stream));
    } else {
        // (forked: the side stream is behind the search's end event, and so behind everything that read the previous
        //  records - also what sphx_prep waits for before it frees an outgrown record buffer)
        SPHX_TRY(sphx_prep(ctx, n, prep_in_of_state(s), pairwise, fork ? ctx->side_stream : ctx->stream));
        if (fork) {
            HIPCHK(hipEventRecord(ctx->ev_join, ctx->side_stream));
            HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
            SPHX_TRY(step_h_sums_out(ctx, n, s.hprev.as<double>(), ctx->side_stream));
        }
        if (detail) HIPCHK(hipEventRecord(ev[3], ctx->stream));
        // Pass 1, lean: nothing in the step reads G (hydro_accel = G / rho is what the update takes).  The species pass
        // (+ metallicity and AGB yields when a table is set) inside pass 1's kernel where both run out of LDS (their
        // first sweeps are the same), else behind it
        const bool sp_fused = species && ctx->species_fused && ctx->species_lds && ctx->use_lds && ctx->qorder && ctx->blob_lists &&
                              !ctx->map_perm && ctx->sp == 16 && ctx->s <= 16 && k <= SPHX_MAX_K;
        if (sp_fused) {
            const int S = ctx->s;
            SPHX_TRY(sphx_ensure(ctx, ctx->rho, (size_t)n * sizeof(double)));
            SPHX_TRY(sphx_ensure(ctx, ctx->rhod, (size_t)n * sizeof(double)));
            SPHX_TRY(sphx_ensure(ctx, ctx->nden, (size_t)n * sizeof(double)));
            SPHX_TRY(sphx_ensure(ctx, ctx->G, (size_t)n * 3 * sizeof(double)));
            SPHX_TRY(sphx_ensure(ctx, ctx->ha, (size_t)n * 3 * sizeof(double)));
            SPHX_TRY(sphx_ensure(ctx, ctx->F, (size_t)n * S * sizeof(double)));
            if (ctx->agb_on) {
                SPHX_TRY(sphx_ensure(ctx, ctx->Zmet, (size_t)n * sizeof(double)));
                SPHX_TRY(sphx_ensure(ctx, ctx->agb_dust, (size_t)n * S * sizeof(double)));
            }
            SPHX_TRY(sphx_blob_density_species(ctx, n, k, /*lean=*/true, S, ctx->fun_id.as<double>(), s.id.as<int>(),
                                               s.m.as<double>(), ctx->F.as<double>(), ctx->Zmet.as<double>(),
                                               ctx->agb_dust.as<double>(), (ctx->agb_on && ctx->Zmet.p && ctx->agb_dust.p) ? 1 : 0));
        } else {
            SPHX_TRY(sphx_pass_density(ctx, n, k, /*lean=*/true));
        }
        if (detail) HIPCHK(hipEventRecord(ev[9], ctx->stream));
        if (species && !sp_fused) SPHX_TRY(sphx_step_species(ctx, n, k));
        if (detail) HIPCHK(hipEventRecord(ev[4], ctx->stream));
        if (ctx->visc_mode == 1) {                 // passes 2 + 3 in one (pairwise viscosity): ms_pi stays 0
            SPHX_TRY(sphx_pass_visc_pw(ctx, n, k, s.m.as<double>()));
        } else {
            // the LDS passes on all blobs of one GPU: pass 2 settles pass 3's NaN rows and marks the blobs with others (sphx_blob.hip)
            const bool hand_visc = sphx_blob_can_hand_visc(ctx, n);
            // ... and where nothing but pass 3 stands between pass 2 and the update (neither drag nor gravity), a settled
            // row's four NaNs are neither stored nor loaded: pass 2 leaves each row's class in a byte, and the update
            // takes a settled row's viscous sums as the constant they are (sphx_update_rows.h)
            const bool by_byte = hand_visc && !ctx->drag && !ctx->gravity;
            *rows_by_byte = by_byte;
            if (hand_visc) {                       // (pass 2 writes them: sized here, not in front of pass 3)
                SPHX_TRY(sphx_ensure(ctx, ctx->va, (size_t)n * 3 * sizeof(double)));
                SPHX_TRY(sphx_ensure(ctx, ctx->vh, (size_t)n * sizeof(double)));
                SPHX_TRY(sphx_blob_size_marks(ctx, n, by_byte));
            }
            SPHX_TRY(sphx_pass_pi(ctx, n, k, s.hprev.as<double>(), s.ptype.as<double>(), hand_visc, by_byte));
            if (detail) HIPCHK(hipEventRecord(ev[5], ctx->stream));
            SPHX_TRY(sphx_pass_visc(ctx, n, k, s.m.as<double>(), hand_visc));
        }
    }
    if (ctx->drag)
        SPHX_TRY(sphx_pass_drag(ctx, n, k, s.m.as<double>(), s.ptype.as<double>(), s.mgm.as<double>(), s.mcs.as<double>()));
    return SPHX_OK;
}

// call_first / call_last: the first / last step of this sphx_step call (they carry the call's start and end events)
// no_old: drv:484-485, the step behind an insertion (the previous acceleration has another shape: dv = a dt)
static int one_step(sphx_ctx* ctx, int k, double dist, int first, double fixed_dt, bool call_first, bool call_last, int no_old) {
    const int64_t n = ctx->n;
    const int ring = (int)(ctx->step_count % 3);
    hipEvent_t* ev = ctx->evring[ring];
    // Timing events: around the step and around the search always (the bench's roofline needs the search's launch time);
    // one per pass only on request (sphx_set_timing_detail / SPHX_TIMING_DETAIL=1) - an event record between two
    // dependent kernels costs the stream ~10 us, six of them 4 % of a 1.5 ms step.
    const bool detail = ctx->timing_detail;
    ctx->ev_detail[ring] = detail;
    // (the step's own start and end events likewise: without them the call's first and last step bracket the call,
    //  whose time is then shared out over its steps)
    const bool rec0 = detail || call_first, rec7 = detail || call_last;
    ctx->ev_has07[ring] = (rec0 ? 1 : 0) | (rec7 ? 2 : 0) | (ctx->visc_mode == 1 && !ctx->loop_forms ? 4 : 0);
    ctx->map_perm = nullptr;
    ctx->qorder = nullptr;
    ctx->blob_lists = false;
    ctx->blob_split_valid = false;
    ctx->pass_part = 0;
    ctx->nbr_api_valid = false;   // the step overwrites the K-major list (search or Verlet refresh)
    sphx_step_list_drop(ctx);
    if (rec0) HIPCHK(hipEventRecord(ev[0], ctx->stream));
    SPHX_TRY(step_search(ctx, k, dist, ev));
    HIPCHK(hipEventRecord(ev[2], ctx->stream));
    bool rows_by_byte = false;
    SPHX_TRY(step_sums(ctx, k, ev, ev[2], detail, &rows_by_byte));
    if (detail) HIPCHK(hipEventRecord(ev[6], ctx->stream));
    StateArrays& s = ctx->st;
    if (ctx->gravity) {                          // drv:448-449; softening = median(h), nsc:358
        SPHX_TRY(sphx_ensure(ctx, ctx->grav, (size_t)n * 3 * sizeof(double)));
        double* eps = ctx->scal.as<double>() + SC_GRAV_EPS;
        SPHX_TRY(sphx_median(ctx, n, s.hprev.as<double>(), eps));
        if (ctx->gravity == 1)
            SPHX_TRY(sphx_gravity_launch(ctx, n, s.x.as<double>(), s.y.as<double>(), s.z.as<double>(), 1,
                                         s.m.as<double>(), eps, 0.0, ctx->grav_G, nullptr, ctx->grav.as<double>()));
        else
            SPHX_TRY(sphx_gravity_tree_launch(ctx, n, s.x.as<double>(), s.y.as<double>(), s.z.as<double>(),
                                              s.m.as<double>(), ctx->grav_ws, eps, 0.0, ctx->grav_G, nullptr,
                                              ctx->grav.as<double>()));
    }
    if (detail) HIPCHK(hipEventRecord(ev[8], ctx->stream));
    // (dt by drv:222-229 inside the update kernel; the crossing-time vote is reset by the next step's first kernel, or
    //  primed by its pass 2 when that grid build is not the fused one)
    SPHX_TRY(sphx_integrate(ctx, n, 1, first, fixed_dt, no_old, rows_by_byte));
    if (rows_by_byte) ctx->stats.update_split_steps++;
    ctx->visc_rows_unfilled = rows_by_byte;            // (sphx_state_download fills ctx->va, ctx->vh in before it reads)
    ctx->sums_stale = false;
    if (rec7) HIPCHK(hipEventRecord(ev[7], ctx->stream));
    ctx->step_count++;
    return SPHX_OK;
}

// drv:386: the search behind an insertion, on the grown state (ctx->n rows), as the first step's search runs - and what
// sphx_step leaves behind its last search: the list marked the step's own (the phases read it next, as the driver's
// drv:399-435 read the list of :386), and the sum of h with the search's counters copied out, so that the next step
// sizes its cells and its list-mode grid from THIS search over ctx->n rows, not from the one before the insertion.
int sphx_step_research(sphx_ctx* ctx, int k, double dist) {
    if (!(dist > 0.0) || !isfinite(dist)) dist = 0.0;
    ctx->k = k;
    ctx->map_perm = nullptr;
    ctx->qorder = nullptr;
    ctx->blob_lists = false;
    ctx->blob_split_valid = false;
    ctx->pass_part = 0;
    ctx->nbr_api_valid = false;
    sphx_step_list_drop(ctx);
    ctx->scale_sizes_valid = false; ctx->scale_d0_valid = false;       // drv:532 behind drv:368: the lengths differ
    SPHX_TRY(step_search(ctx, k, dist, ctx->ev, /*fresh=*/true));
    HIPCHK(hipEventRecord(ctx->ev[2], ctx->stream));
    SPHX_TRY(step_h_sums_out(ctx, ctx->n, ctx->st.hprev.as<double>(), ctx->stream));
    ctx->step_list_valid = true; ctx->step_qorder = ctx->qorder; ctx->step_list_n = ctx->n; ctx->step_list_k = k;
    return SPHX_OK;
}

static int collect_stats(sphx_ctx* ctx, int ring) {
    if (!(ctx->ev_pending & (1u << ring))) return SPHX_OK;
    ctx->ev_pending &= ~(1u << ring);
    hipEvent_t* ev = ctx->evring[ring];
    const int has = ctx->ev_has07[ring];
    HIPCHK(hipEventSynchronize((has & 2) ? ev[7] : ev[2]));
    sphx_stats& st = ctx->stats;
    float ms[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    HIPCHK(hipEventElapsedTime(&ms[1], ev[1], ev[2]));
    st.ms_search += ms[1];
    st.steps += 1;
    st.search_steps += 1;
    st.n = ctx->n;
    if (!ctx->ev_detail[ring]) return SPHX_OK;    // (only the search's events were recorded for this step; ms_total: per call)
    float tot;
    HIPCHK(hipEventElapsedTime(&tot, ev[0], ev[7]));
    HIPCHK(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
    st.ms_grid += ms[0]; st.ms_total += tot;
    for (int i = 2; i < 6; ++i) {
        if ((has & 4) && i >= 4) break;             // pairwise viscosity: one pass between ev[4] and ev[6], no ev[5]
        HIPCHK(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    }
    if (has & 4) HIPCHK(hipEventElapsedTime(&ms[5], ev[4], ev[6]));
    st.ms_prep += ms[2];
    float mg = 0.f, mi = 0.f;
    HIPCHK(hipEventElapsedTime(&mg, ev[6], ev[8]));
    HIPCHK(hipEventElapsedTime(&mi, ev[8], ev[7]));
    ms[6] = mi;
    st.ms_gravity += mg;
    {                                             // (ev[9] is recorded between the sums before it and the species pass)
        float md = 0.f, msp = 0.f;
        HIPCHK(hipEventElapsedTime(&md, ev[3], ev[9]));
        HIPCHK(hipEventElapsedTime(&msp, ev[9], ev[4]));
        ms[3] = md;
        st.ms_species += msp;
    }
    st.ms_density += ms[3]; st.ms_pi += ms[4]; st.ms_visc += ms[5]; st.ms_integrate += ms[6];
    st.detail_steps += 1;
    return SPHX_OK;
}

extern "C" int sphx_step(sphx_ctx* ctx, int nsteps, int k, double dist, int first, double fixed_dt) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_step before sphx_state_upload");
    if (k < 1 || k > SPHX_MAX_K) return sphx_set_err(ctx, SPHX_E_ARG, "N_NEIGH=%d not in 1..%d", k, SPHX_MAX_K);
    if (nsteps < 1) return sphx_set_err(ctx, SPHX_E_ARG, "nsteps=%d < 1", nsteps);
    HIPCHK(hipSetDevice(ctx->device));
    if (!(dist > 0.0) || !isfinite(dist)) dist = 0.0;
    ctx->k = k;
    ctx->scale_sizes_valid = false;                        // drv:437: the search replaces the adapted sizes
    const bool per_call = !ctx->timing_detail;             // (else every step times itself)
    // the call's wall time on the stream, over all its steps
    if (per_call) HIPCHK(hipEventRecord(ctx->ev[8], ctx->stream));
    for (int it = 0; it < nsteps; ++it) {
        // each step sizes the grid and takes the search's decisions from the lagged read-backs
        const int ring = (int)(ctx->step_count % 3);
        SPHX_TRY(collect_stats(ctx, ring));            // (the step launched three steps ago, if still uncollected)
        const int no_old = ctx->no_old_once ? 1 : 0;       // (one shot: set by sphx_state_insert_rows)
        ctx->no_old_once = false;
        SPHX_TRY(one_step(ctx, k, dist, first && it == 0, fixed_dt, false, false, no_old));
        ctx->ev_pending |= 1u << ring;
        SPHX_TRY(collect_stats(ctx, (ring + 1) % 3));  // two steps ago: finished long since, no wait
    }
    // the list, its column order and the ids are this step's until something rewrites them (sphx_phase.hip reads them)
    ctx->step_list_valid = true; ctx->step_qorder = ctx->qorder; ctx->step_list_n = ctx->n; ctx->step_list_k = k;
    if (per_call) HIPCHK(hipEventRecord(ctx->ev[9], ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->pinned->scal, ctx->scal.p, SC_NSLOTS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < 3; ++r) SPHX_TRY(collect_stats(ctx, (int)((ctx->step_count + r) % 3)));   // oldest first
    if (per_call) {                                        // the call's wall time on the stream, over all its steps
        float tot = 0.f;
        HIPCHK(hipEventElapsedTime(&tot, ctx->ev[8], ctx->ev[9]));
        ctx->stats.ms_total += tot;
    }
    const u64* sc = ctx->pinned->scal;
    memcpy(&ctx->dt_last, &sc[SC_DT], sizeof(double));
    ctx->stats.candidates = (int64_t)sc[SC_CAND];
    ctx->stats.retries = (int64_t)sc[SC_RETRY];
    ctx->stats.fallback_queries = (int64_t)(u32)sc[SC_NFAILQ];
    ctx->stats.short_rows = (int64_t)sc[SC_SHORT];
    SPHX_TRY(sphx_badc_read(ctx));
    return SPHX_OK;
}

extern "C" int sphx_state_download(sphx_ctx* ctx, double* pos, double* vel, double* accel,
                                   double* E_internal, double* T, double* sizes, double* rho,
                                   double* nden, double* visc_heat, double* dt_last) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "no state uploaded");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->n;
    const size_t nb = (size_t)n * sizeof(double);
    StateArrays& s = ctx->st;
    const int* id = s.id.as<int>();
    SPHX_TRY(sphx_ensure(ctx, ctx->out_a, 3 * nb));
    double* stage = ctx->out_a.as<double>();
    struct V3 { double* host; DevBuf *a, *b, *c; };
    V3 v3[] = {{pos, &s.x, &s.y, &s.z}, {vel, &s.vx, &s.vy, &s.vz}, {accel, &s.ax, &s.ay, &s.az}};
    for (V3& v : v3) {
        if (!v.host) continue;
        SPHX_TRY(sphx_soa3_to_aos_by_id(ctx, n, id, v.a->as<double>(), v.b->as<double>(), v.c->as<double>(), stage));
        SPHX_TRY(download(ctx, v.host, stage, 3 * nb));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    struct V1 { double* host; const double* dev; };
    const bool stepped = ctx->step_count > 0 && !ctx->sums_stale;     // (an insertion since: "not stepped yet" for them)
    // (an update by bytes read no viscous sums for its settled rows, and pass 2 stored none: their NaNs now, once)
    if (stepped && visc_heat) SPHX_TRY(sphx_settled_visc_fill(ctx, n));
    V1 v1[] = {{E_internal, s.E.as<double>()}, {T, s.T.as<double>()}, {sizes, s.hprev.as<double>()},
               {rho, stepped ? ctx->rho.as<double>() : nullptr},
               {nden, stepped ? ctx->nden.as<double>() : nullptr},
               {visc_heat, stepped ? ctx->vh.as<double>() : nullptr}};
    for (V1& v : v1) {
        if (!v.host) continue;
        if (!v.dev) { memset(v.host, 0, nb); continue; }
        SPHX_TRY(sphx_scatter_rows_by_id(ctx, n, 1, id, v.dev, stage));
        SPHX_TRY(download(ctx, v.host, stage, nb));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (dt_last) *dt_last = ctx->dt_last;
    return SPHX_OK;
}

// The AGB dust-yield table (config_helper.py:138-178: 11 degree-1 splines over (metallicity, mass)) into the context
int sphx_agb_table_set(sphx_ctx* ctx, int S, int nspl, const int32_t* ntx, const int32_t* nty, const double* tx, const double* ty,
                       const double* coeffs, const int32_t* mapto, double divisor, const double* mu_specie, double solar_mass) {
    ctx->agb_on = false;
    if (nspl == 0) return SPHX_OK;
    if (S < 7 || S > AGB_MAX_SPEC) return sphx_set_err(ctx, SPHX_E_ARG, "AGB table: %d species (7..%d)", S, AGB_MAX_SPEC);
    if (!ntx || !nty || !tx || !ty || !coeffs || !mapto || !mu_specie)
        return sphx_set_err(ctx, SPHX_E_ARG, "AGB table: NULL argument");
    if (nspl < 1 || nspl > AGB_MAX_SPL) return sphx_set_err(ctx, SPHX_E_ARG, "AGB table: %d splines", nspl);
    if (!(divisor != 0.0)) return sphx_set_err(ctx, SPHX_E_ARG, "AGB table: divisor is 0");
    HIPCHK(hipSetDevice(ctx->device));
    AgbTable& t = ctx->agb;
    t.nspl = nspl; t.nspec = S;
    size_t ntx_tot = 0, nty_tot = 0, nc_tot = 0;
    for (int o = 0; o < nspl; ++o) {
        if (ntx[o] < 4 || nty[o] < 4) return sphx_set_err(ctx, SPHX_E_ARG, "AGB table: spline %d has fewer than 4 knots", o);
        if (mapto[o] < 0 || mapto[o] >= S) return sphx_set_err(ctx, SPHX_E_ARG, "AGB table: mapto[%d]=%d out of range", o, mapto[o]);
        ntx_tot += ntx[o]; nty_tot += nty[o]; nc_tot += (size_t)(ntx[o] - 2) * (nty[o] - 2);
    }
    size_t ox = 0, oy = ntx_tot, oc = ntx_tot + nty_tot;
    for (int o = 0; o < nspl; ++o) {
        t.tx_off[o] = (int)ox; t.ty_off[o] = (int)oy; t.c_off[o] = (int)oc;
        t.ntx[o] = ntx[o]; t.nty[o] = nty[o]; t.mapto[o] = mapto[o];
        ox += ntx[o]; oy += nty[o]; oc += (size_t)(ntx[o] - 2) * (nty[o] - 2);
    }
    for (int s = 0; s < S; ++s) t.mu[s] = mu_specie[s];
    t.divisor = divisor; t.solar = solar_mass;
    SPHX_TRY(sphx_ensure(ctx, ctx->agb_knots, (ntx_tot + nty_tot + nc_tot + 6 * (size_t)nspl) * sizeof(double)));
    double* kd = ctx->agb_knots.as<double>();
    {   // the per-spline integers once more, in device memory (AgbTable::meta_off)
        double meta[6 * AGB_MAX_SPL];
        t.covered = 0u;
        for (int o = 0; o < nspl; ++o) {
            bool later = false;
            for (int o2 = o + 1; o2 < nspl; ++o2) later = later || mapto[o2] == mapto[o];
            meta[6 * o + 0] = t.tx_off[o]; meta[6 * o + 1] = t.ty_off[o]; meta[6 * o + 2] = t.c_off[o];
            meta[6 * o + 3] = t.ntx[o]; meta[6 * o + 4] = t.nty[o]; meta[6 * o + 5] = later ? -1.0 : (double)mapto[o];
            t.covered |= 1u << mapto[o];
        }
        t.meta_off = (int)(ntx_tot + nty_tot + nc_tot);
        HIPCHK(hipMemcpyAsync(kd + t.meta_off, meta, 6 * (size_t)nspl * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));       // (meta is a stack array)
    }
    HIPCHK(hipMemcpyAsync(kd, tx, ntx_tot * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(kd + ntx_tot, ty, nty_tot * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(kd + ntx_tot + nty_tot, coeffs, nc_tot * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    t.knots = kd;
    ctx->agb_on = true;
    return SPHX_OK;
}

// ... for the step's species pass: with it every step also leaves Z_i (drv:663 on the smoothed composition) and the
// yields of config_helper.py:183-189 at (Z_i, m_i).  nspl == 0 switches it off.  Call after sphx_state_upload with f_un.
extern "C" int sphx_state_set_agb(sphx_ctx* ctx, int nspl, const int32_t* ntx, const int32_t* nty, const double* tx,
                                  const double* ty, const double* coeffs, const int32_t* mapto, double divisor,
                                  const double* mu_specie, double solar_mass) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_set_agb before sphx_state_upload");
    ctx->agb_on = false;
    if (nspl == 0) return SPHX_OK;
    if (ctx->s < 7 || !ctx->fun_id.p)
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_set_agb: the state carries no composition (f_un) of >= 7 species");
    return sphx_agb_table_set(ctx, ctx->s, nspl, ntx, nty, tx, ty, coeffs, mapto, divisor, mu_specie, solar_mass);
}

// F (S,n) species number densities of the last step (nsc:624-627), Z (n,), agb_dust (n,S) - caller order; any may be NULL
__global__ __launch_bounds__(256) void scatter_species_major(int n, int S, const int* id, const double* in, double* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const size_t o = (size_t)id[t];
    for (int s = 0; s < S; ++s) out[(size_t)s * n + o] = in[(size_t)s * n + t];
}
extern "C" int sphx_state_download_species(sphx_ctx* ctx, double* F, double* Z, double* agb_dust) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state || ctx->s < 1 || !ctx->fun_id.p || ctx->step_count < 1 || ctx->sums_stale)
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_download_species: no species pass has run (state without f_un, "
                                                 "or no step yet)");
    if ((Z || agb_dust) && !ctx->agb_on) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_download_species: no AGB table set");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->n;
    const int S = ctx->s;
    const int* id = ctx->st.id.as<int>();
    SPHX_TRY(sphx_ensure(ctx, ctx->out_a, (size_t)n * S * sizeof(double)));
    double* stage = ctx->out_a.as<double>();
    if (F) {
        hipLaunchKernelGGL(scatter_species_major, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n, S, id,
                           ctx->F.as<double>(), stage);
        SPHX_TRY(download(ctx, F, stage, (size_t)n * S * sizeof(double)));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (Z) {
        SPHX_TRY(sphx_scatter_rows_by_id(ctx, n, 1, id, ctx->Zmet.as<double>(), stage));
        SPHX_TRY(download(ctx, Z, stage, (size_t)n * sizeof(double)));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    if (agb_dust) {
        SPHX_TRY(sphx_scatter_rows_by_id(ctx, n, S, id, ctx->agb_dust.as<double>(), stage));
        SPHX_TRY(download(ctx, agb_dust, stage, (size_t)n * S * sizeof(double)));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return SPHX_OK;
}

int sphx_badc_read(sphx_ctx* ctx) {
    u64* hb = ctx->pinned->badc;
    HIPCHK(hipMemcpyAsync(hb, ctx->badc.p, (size_t)BADC_BUCKETS * BADC_STRIDE * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    u64 tot[4] = {0, 0, 0, 0};
    for (int b = 0; b < BADC_BUCKETS; ++b)
        for (int q = 0; q < 4; ++q) tot[q] += hb[b * BADC_STRIDE + q];
    ctx->stats.bad_accel = (int64_t)tot[BAD_ACCEL]; ctx->stats.bad_energy = (int64_t)tot[BAD_ENERGY];
    ctx->stats.bad_state = (int64_t)tot[BAD_STATE]; ctx->stats.bad_h = (int64_t)tot[BAD_H];
    return SPHX_OK;
}

extern "C" int sphx_get_stats(sphx_ctx* ctx, sphx_stats* out) {
    if (!ctx || !out) return SPHX_E_ARG;
    SPHX_TRY(sphx_dev_collect(ctx));
    if (ctx->map_perm) {               // the device-pointer API has no sphx_step to read the failure counters back: here
        HIPCHK(hipSetDevice(ctx->device));
        SPHX_TRY(sphx_badc_read(ctx));
    }
    // the last hinted search's tie list: entries reserved (read behind the stream: the word stands until the next grid
    // build) and room
    ctx->stats.tie_entries = 0;
    ctx->stats.tie_capacity = ctx->tie_cap_last;
    if (ctx->tie_count_dev) {
        int cnt = 0;
        u64 nfail = 0;
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipMemcpyAsync(&cnt, ctx->tie_count_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(&nfail, ctx->scal.as<u64>() + SC_NFAILQ, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        ctx->stats.tie_entries = (int64_t)(u32)cnt;
        // (sphx_step reads this slot itself; the device-pointer API has no other place that does)
        if (ctx->map_perm) ctx->stats.fallback_queries = (int64_t)(u32)nfail;
    }
    // the sums the LDS passes found NaN before they were finished (sphx_blob.h: blob_pass)
    if (ctx->scal.p) {
        u64 cnt[3] = {0, 0, 0};
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipMemcpyAsync(cnt, ctx->scal.as<u64>() + SC_SETTLED, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        ctx->stats.visc_blobs_settled = (int64_t)cnt[0];
        ctx->stats.pi_waves_settled = (int64_t)cnt[1];
        ctx->stats.visc_launches_skipped = (int64_t)cnt[2];
    }
    *out = ctx->stats;
    // the grid build's single-launch scan bounds its waits; a wait that ran out raised a flag (and left wrong numbers)
    for (int w = 0; w < 2; ++w) {
        if (!ctx->lbs_state[w].p) continue;
        int flag = 0;
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipMemcpy(&flag, ctx->lbs_state[w].as<int>() + 2, sizeof(int), hipMemcpyDeviceToHost));
        if (flag) return sphx_set_err(ctx, SPHX_E_STATE, "lookback_scan_kernel: a tile's sum never arrived (results since then are wrong)");
    }
    return SPHX_OK;
}
extern "C" int sphx_set_timing_detail(sphx_ctx* ctx, int on) {
    if (!ctx) return SPHX_E_ARG;
    ctx->timing_detail = on != 0;
    return SPHX_OK;
}

extern "C" int sphx_reset_stats(sphx_ctx* ctx) {
    if (!ctx) return SPHX_E_ARG;
    SPHX_TRY(sphx_dev_collect(ctx));
    memset(&ctx->stats, 0, sizeof(ctx->stats));
    HIPCHK(hipMemsetAsync(ctx->scal.as<u64>() + SC_CAND, 0, 2 * sizeof(u64), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->scal.as<u64>() + SC_SHORT, 0, sizeof(u64), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->scal.as<u64>() + SC_SETTLED, 0, 3 * sizeof(u64), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->badc.p, 0, (size_t)BADC_BUCKETS * BADC_STRIDE * sizeof(u64), ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPHX_OK;
}
