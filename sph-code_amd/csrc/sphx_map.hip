// sphx_map.hip - the state projected along a coordinate axis onto a pixel grid: column density of gas and of dust, their
// column-weighted temperatures and the number of particles over each pixel (include/sphx.h has the definitions,
// sphx_map_pair.h the arithmetic).  The line integral of the poly6 weight is closed-form per (particle, pixel) pair, so
// the work is pair evaluation over a 2-D binning:
//   map_foot_kernel    one lane per PARTICLE ID (through the slot map on the resident state; the array call: identity):
//                      its record (x_u, x_v, R^2, c = m (9 / 2 pi) R^-9, T, gas or dust), the inclusive range of 16 x 16
//                      tiles whose pixel CENTRES its bounding box holds (bisection on the centres themselves), its pair
//                      count into a 64-bit total, the rows that never count into `skipped`
//   map_count_kernel   counts per tile by integer atomics; sphx_excl_scan_int; the 64-bit total, the scan's total and the
//                      skipped rows come to the host - the call's one wait - and are checked before anything is sized
//   the tile lists     sphx_rev_fill_sort (sphx_side.hip): map_fill_kernel in whatever order the atomics give, then the
//                      segmented sort that removes it - each tile lists its particles in ascending id
//   map_tile_kernel    one workgroup of 256 lanes per tile, one pixel per lane, the sums in registers; the list goes
//                      through LDS 256 records at a time and every lane reads the same record (a broadcast); s > 0 decides;
//                      the ratios in the same kernel.  A lane beyond the image edge computes and does not store.
// Every sum of a pixel runs in ascending particle id: the same bits on every call and in every storage order.  The state is
// only read, in buffers of its own (ctx->map_*).  Plain C++, vector stores, integer atomics only.
#include "sphx_internal.h"
#include "sphx_map_pair.h"
#include "sphx_revlist.h"
#pragma clang fp contract(off)

#define MAP_WG 256
static_assert(SPHX_MAP_TILE * SPHX_MAP_TILE == MAP_WG && SPHX_MAP_BATCH == MAP_WG, "a lane per pixel of a tile, a lane per staged record");
static_assert(sizeof(SphxMapRec) == 48, "a footprint record is 48 bytes");

struct MapFootArgs {
    int n;
    const int* slot;                         // storage slot of an id (NULL: the id)
    const double *xu, *xv, *xw;              // by slot, stride ps
    int ps;
    const double *m, *pt, *T, *sizes;        // by slot
    double d, m0;
    double cu, cv, wu, wv;
    int nu, nv, ntx, nty;
    int depth; double lo, hi;
    SphxMapRec* rec;                         // by id
    int4* range;                             // by id: tiles x .. y along u, z .. w along v (x > y: none)
    u64* scal;                               // [0] pairs (particle, tile), [1] skipped rows
};
__global__ __launch_bounds__(MAP_WG) void map_foot_kernel(MapFootArgs a) {
    const long long i = (long long)blockIdx.x * MAP_WG + threadIdx.x;
    const bool live = i < a.n;
    int4 rg = make_int4(1, 0, 1, 0);
    bool bad = false;
    u64 pairs = 0;
    if (live) {
        const size_t p = a.slot ? (size_t)a.slot[i] : (size_t)i;
        const double ty = a.pt[p], m = a.m[p];
        double R = 0.0;
        if (sphx_map_radius(ty, m, a.sizes[p], a.d, a.m0, &R)) {
            const double xu = a.xu[p * a.ps], xv = a.xv[p * a.ps], xw = a.xw[p * a.ps];
            bad = sphx_map_row_bad(xu, xv, xw, m, R);
            if (!bad && (!a.depth || (xw >= a.lo && xw < a.hi))) {
                SphxMapRec r;
                r.xu = xu; r.xv = xv; r.R2 = R * R; r.c = sphx_map_coeff(m, R); r.T = a.T[p]; r.gas = ty == 0.0 ? 1.0 : 0.0;
                a.rec[i] = r;
                int ilo, ihi, jlo, jhi;
                sphx_map_span(a.cu, a.wu, a.nu, xu, R, &ilo, &ihi);
                sphx_map_span(a.cv, a.wv, a.nv, xv, R, &jlo, &jhi);
                if (ilo <= ihi && jlo <= jhi) {
                    rg = make_int4(ilo / SPHX_MAP_TILE, ihi / SPHX_MAP_TILE, jlo / SPHX_MAP_TILE, jhi / SPHX_MAP_TILE);
                    pairs = (u64)(rg.y - rg.x + 1) * (u64)(rg.w - rg.z + 1);
                }
            }
        }
        a.range[i] = rg;
    }
    for (int off = SPHX_WAVE / 2; off > 0; off >>= 1) pairs += __shfl_down(pairs, off);
    const u64 nb = __ballot(bad);
    if ((threadIdx.x & (SPHX_WAVE - 1)) == 0) {
        if (pairs) atomicAdd(a.scal + 0, pairs);
        if (nb) atomicAdd(a.scal + 1, (u64)__popcll(nb));
    }
}
// cnt[tile] += 1 for every tile of every particle's range
__global__ __launch_bounds__(MAP_WG) void map_count_kernel(int n, int ntx, const int4* __restrict__ range, int* __restrict__ cnt) {
    const long long i = (long long)blockIdx.x * MAP_WG + threadIdx.x;
    if (i >= n) return;
    const int4 rg = range[i];
    for (int ty = rg.z; ty <= rg.w; ++ty)
        for (int tx = rg.x; tx <= rg.y; ++tx) atomicAdd(cnt + (size_t)ty * ntx + tx, 1);
}
// the id into every tile's slice, at the place the tile's cursor hands out
__global__ __launch_bounds__(MAP_WG) void map_fill_kernel(int n, int ntx, const int4* __restrict__ range, const int* __restrict__ start,
                                                          int* __restrict__ cur, int* __restrict__ rev_raw) {
    const long long i = (long long)blockIdx.x * MAP_WG + threadIdx.x;
    if (i >= n) return;
    const int4 rg = range[i];
    for (int ty = rg.z; ty <= rg.w; ++ty)
        for (int tx = rg.x; tx <= rg.y; ++tx) {
            const size_t t = (size_t)ty * ntx + tx;
            const int at = atomicAdd(cur + t, 1);
            if (at < start[t + 1] - start[t]) rev_raw[(size_t)start[t] + at] = (int)i;
        }
}

struct MapTileArgs {
    double cu, cv, wu, wv;
    int nu, nv, ntx, want, n;
    const int *start, *rev;
    const SphxMapRec* rec;
    double *gc, *dc, *gt, *dt;               // (nv, nu), any may be NULL
    long long* count;
};
__global__ __launch_bounds__(MAP_WG) void map_tile_kernel(MapTileArgs a) {
    __shared__ SphxMapRec sh[SPHX_MAP_BATCH];
    const int tile = blockIdx.x, l = threadIdx.x;
    const int tx = tile % a.ntx, ty = tile / a.ntx;
    const int i = tx * SPHX_MAP_TILE + (l & (SPHX_MAP_TILE - 1)), j = ty * SPHX_MAP_TILE + l / SPHX_MAP_TILE;
    const double u = sphx_map_centre(a.cu, a.wu, a.nu, i), v = sphx_map_centre(a.cv, a.wv, a.nv, j);
    SphxMapAcc acc;
    sphx_map_acc_zero(acc);
    const int b0 = a.start[tile], b1 = a.start[tile + 1];
    for (int base = b0; base < b1; base += SPHX_MAP_BATCH) {
        const int len = min(SPHX_MAP_BATCH, b1 - base);
        __syncthreads();                     // the batch before has been read by every lane
        if (l < len) {
            const int id = a.rev[base + l];
            SphxMapRec r;
            r.xu = r.xv = r.c = r.T = r.gas = 0.0; r.R2 = -1.0;       // (an id outside the state: a record no pixel passes)
            if ((unsigned)id < (unsigned)a.n) r = a.rec[id];
            sh[l] = r;
        }
        __syncthreads();
        for (int r = 0; r < len; ++r) sphx_map_add(acc, sh[r], u, v, a.want);
    }
    if (i >= a.nu || j >= a.nv) return;
    const size_t o = (size_t)j * a.nu + i;
    if (a.gc) a.gc[o] = acc.gc;
    if (a.dc) a.dc[o] = acc.dc;
    if (a.gt) a.gt[o] = sphx_map_ratio(acc.gn, acc.gd);
    if (a.dt) a.dt[o] = sphx_map_ratio(acc.dn, acc.dd);
    if (a.count) a.count[o] = acc.cnt;
}

// =====================================================================================================================
// host side
// =====================================================================================================================
struct MapGeom { int au, av; double cu, cv, wu, wv; int nu, nv; int depth; double lo, hi; };
struct MapHostOut { double *gc, *dc, *gt, *dt; int64_t *count, *skipped, *pairs; };

static int map_check(sphx_ctx* ctx, const char* who, int64_t n, const int axes[2], const double center[2], const double half_width[2],
                     const int npix[2], const double* depth, MapGeom* g) {
    NEED(axes); NEED(center); NEED(half_width); NEED(npix);
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld (need 1 <= n < 2^31 - 16)", who, (long long)n);
    if (axes[0] < 0 || axes[0] > 2 || axes[1] < 0 || axes[1] > 2 || axes[0] == axes[1])
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: axes=(%d, %d) (two different indices of 0, 1, 2)", who, axes[0], axes[1]);
    for (int q = 0; q < 2; ++q) {
        if (!(half_width[q] > 0.0) || !sphx_map_finite(half_width[q]))
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: half_width[%d]=%g (need positive and finite)", who, q, half_width[q]);
        if (!sphx_map_finite(center[q])) return sphx_set_err(ctx, SPHX_E_ARG, "%s: center[%d]=%g is not finite", who, q, center[q]);
        if (npix[q] < 1) return sphx_set_err(ctx, SPHX_E_ARG, "%s: npix[%d]=%d < 1", who, q, npix[q]);
    }
    if ((long long)npix[0] * (long long)npix[1] > SPHX_MAP_MAXPIX)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: %d x %d pixels (at most 2^28)", who, npix[0], npix[1]);
    if (depth && !(depth[0] < depth[1])) return sphx_set_err(ctx, SPHX_E_ARG, "%s: depth=(%g, %g) (need lo < hi)", who, depth[0], depth[1]);
    g->au = axes[0]; g->av = axes[1];
    g->cu = center[0]; g->cv = center[1]; g->wu = half_width[0]; g->wv = half_width[1];
    g->nu = npix[0]; g->nv = npix[1];
    g->depth = depth != nullptr; g->lo = depth ? depth[0] : 0.0; g->hi = depth ? depth[1] : 0.0;
    return SPHX_OK;
}

// f: everything of the footprints' arguments but the geometry and the outputs.  The timer has begun.
// resident: the ids reach their rows through the slot map, built here.
static int map_run(sphx_ctx* ctx, const char* who, MapFootArgs f, const MapGeom& g, const MapHostOut& ho, bool resident) {
    hipStream_t st = ctx->stream;
    const size_t nn = (size_t)f.n, npix = (size_t)g.nu * (size_t)g.nv;
    const int ntx = (g.nu + SPHX_MAP_TILE - 1) / SPHX_MAP_TILE, nty = (g.nv + SPHX_MAP_TILE - 1) / SPHX_MAP_TILE;
    const size_t nt = (size_t)ntx * (size_t)nty;
    f.cu = g.cu; f.cv = g.cv; f.wu = g.wu; f.wv = g.wv; f.nu = g.nu; f.nv = g.nv; f.ntx = ntx; f.nty = nty;
    f.depth = g.depth; f.lo = g.lo; f.hi = g.hi;
    // ctx->map_rec: records (n) | tile ranges (n)
    {
        Carve c;
        c.take(f.rec, nn, 16); c.take(f.range, nn, 16);
        SPHX_TRY(sphx_carve_into(ctx, ctx->map_rec, c));
    }
    // ctx->map_int: slot (n, the resident call) | cnt | start (tiles + 1) | cur (tiles)
    int *slot, *cnt, *start, *cur;
    {
        Carve c;
        c.take(slot, resident ? nn : 0, 16); c.take(cnt, nt + 1, 16); c.take(start, nt + 1, 16); c.take(cur, nt, 16);
        c.pad(16);
        SPHX_TRY(sphx_carve_into(ctx, ctx->map_int, c));
    }
    f.slot = nullptr;
    if (resident) {
        SPHX_TRY(sphx_slot_map(ctx, slot));
        f.slot = slot;
    }
    // ctx->map_out: pairs, skipped (u64) | the images asked for | count
    const int want = (ho.gc ? SPHX_MAP_GAS_COLUMN : 0) | (ho.dc ? SPHX_MAP_DUST_COLUMN : 0) | (ho.gt ? SPHX_MAP_GAS_T : 0) |
                     (ho.dt ? SPHX_MAP_DUST_T : 0) | (ho.count ? SPHX_MAP_COUNT : 0);
    MapTileArgs t;
    {
        Carve c;
        c.take(f.scal, 2);
        c.take(t.gc, ho.gc ? npix : 0); c.take(t.dc, ho.dc ? npix : 0); c.take(t.gt, ho.gt ? npix : 0); c.take(t.dt, ho.dt ? npix : 0);
        c.take(t.count, ho.count ? npix : 0);
        SPHX_TRY(sphx_carve_into(ctx, ctx->map_out, c));
    }
    if (!ho.gc) t.gc = nullptr;
    if (!ho.dc) t.dc = nullptr;
    if (!ho.gt) t.gt = nullptr;
    if (!ho.dt) t.dt = nullptr;
    if (!ho.count) t.count = nullptr;
    HIPCHK(hipMemsetAsync(f.scal, 0, 2 * sizeof(u64), st));
    HIPCHK(hipMemsetAsync(cnt, 0, (nt + 1) * sizeof(int), st));
    HIPCHK(hipMemsetAsync(cur, 0, nt * sizeof(int), st));
    hipLaunchKernelGGL(map_foot_kernel, dim3(sphx_blocks(nn, MAP_WG)), dim3(MAP_WG), 0, st, f);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->map_t.mark(ctx, 1));
    hipLaunchKernelGGL(map_count_kernel, dim3(sphx_blocks(nn, MAP_WG)), dim3(MAP_WG), 0, st, f.n, ntx, f.range, cnt);
    HIPCHK(hipGetLastError());
    SPHX_TRY(sphx_excl_scan_int(ctx, cnt, start, (int)nt));
    u64* back = ctx->pinned->map;
    back[2] = 0;
    HIPCHK(hipMemcpyAsync(back, f.scal, 2 * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(back + 2, start + nt, sizeof(int), hipMemcpyDeviceToHost, st));
    SPHX_TRY(ctx->map_t.mark(ctx, 2));
    HIPCHK(hipStreamSynchronize(st));                // the call's one wait: the pair count before anything is sized
    const u64 pairs = back[0], skipped = back[1];
    if (pairs > 0x7FFFFFFFull)
        return sphx_set_err(ctx, SPHX_E_NOMEM, "%s: %llu (particle, tile) pairs, more than the 2^31 - 1 a list holds: widen the window or use fewer pixels",
                            who, (unsigned long long)pairs);
    if ((u64)(unsigned)*(const int*)(back + 2) != pairs)
        return sphx_set_err(ctx, SPHX_E_HIP, "%s: the scan counts %d pairs, the footprints %llu", who, *(const int*)(back + 2), (unsigned long long)pairs);
    RevList rl;
    const int4* range = f.range;
    const int n = f.n;
    SPHX_TRY(sphx_rev_fill_sort(ctx, (int64_t)nt, start, (size_t)pairs, (unsigned long long)nn,
                                [&](const int* start_, int* rev_raw) {
                                    hipLaunchKernelGGL(map_fill_kernel, dim3(sphx_blocks(nn, MAP_WG)), dim3(MAP_WG), 0, st, n, ntx, range, start_, cur, rev_raw);
                                },
                                ctx->map_rev, ctx->map_tmp, &rl));
    SPHX_TRY(ctx->map_t.mark(ctx, 3));
    t.cu = g.cu; t.cv = g.cv; t.wu = g.wu; t.wv = g.wv; t.nu = g.nu; t.nv = g.nv; t.ntx = ntx; t.want = want; t.n = n;
    t.start = start; t.rev = rl.rev; t.rec = f.rec;
    hipLaunchKernelGGL(map_tile_kernel, dim3((unsigned)nt), dim3(MAP_WG), 0, st, t);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->map_t.mark(ctx, 4));
    const CopyF64 ds[] = {{ho.gc, t.gc, npix}, {ho.dc, t.dc, npix}, {ho.gt, t.gt, npix}, {ho.dt, t.dt, npix}, {ho.count, t.count, npix}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 5));
    SPHX_TRY(ctx->map_t.mark(ctx, 5));
    HIPCHK(hipStreamSynchronize(st));
    if (ho.skipped) *ho.skipped = (int64_t)skipped;
    if (ho.pairs) *ho.pairs = (int64_t)pairs;
    return ctx->map_t.end(ctx);
}

extern "C" int sphx_project_maps(sphx_ctx* ctx, int64_t n, const double* points, const double* mass, const double* particle_type,
                                 const double* sizes, const double* T, double d, const int axes[2], const double center[2],
                                 const double half_width[2], const int npix[2], const double* depth, double* gas_column,
                                 double* dust_column, double* gas_temperature, double* dust_temperature, int64_t* count,
                                 int64_t* skipped, int64_t* pairs) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_project_maps";
    NEED(points); NEED(mass); NEED(particle_type); NEED(sizes); NEED(T);
    MapGeom g;
    SPHX_TRY(map_check(ctx, who, n, axes, center, half_width, npix, depth, &g));
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nn = (size_t)n;
    // ctx->map_in: points (n,3) | mass | particle_type | sizes | T (n each)
    double *d_p, *d_m, *d_pt, *d_s, *d_T;
    Carve c;
    c.take(d_p, 3 * nn); c.take(d_m, nn); c.take(d_pt, nn); c.take(d_s, nn); c.take(d_T, nn);
    SPHX_TRY(sphx_carve_into(ctx, ctx->map_in, c));
    SPHX_TRY(ctx->map_t.begin(ctx));
    const CopyF64 us[] = {{points, d_p, 3 * nn}, {mass, d_m, nn}, {particle_type, d_pt, nn}, {sizes, d_s, nn}, {T, d_T, nn}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 5));
    MapFootArgs f;
    f.n = (int)n;
    f.xu = d_p + g.au; f.xv = d_p + g.av; f.xw = d_p + (3 - g.au - g.av); f.ps = 3;
    f.m = d_m; f.pt = d_pt; f.T = d_T; f.sizes = d_s;
    f.d = d; f.m0 = ctx->cst.m_0;
    const MapHostOut ho{gas_column, dust_column, gas_temperature, dust_temperature, count, skipped, pairs};
    return map_run(ctx, who, f, g, ho, false);
}

extern "C" int sphx_state_project(sphx_ctx* ctx, double d, const int axes[2], const double center[2], const double half_width[2],
                                  const int npix[2], const double* depth, double* gas_column, double* dust_column,
                                  double* gas_temperature, double* dust_temperature, int64_t* count, int64_t* skipped, int64_t* pairs) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_project";
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no state uploaded", who);
    if (ctx->step_count < 1) return sphx_set_err(ctx, SPHX_E_STATE, "%s before the first sphx_step: sizes do not exist yet", who);
    MapGeom g;
    SPHX_TRY(map_check(ctx, who, ctx->n, axes, center, half_width, npix, depth, &g));
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->map_t.begin(ctx));
    const StateArrays& s = ctx->st;
    const double* pos[3] = {s.x.as<double>(), s.y.as<double>(), s.z.as<double>()};
    MapFootArgs f;
    f.n = (int)ctx->n;
    f.xu = pos[g.au]; f.xv = pos[g.av]; f.xw = pos[3 - g.au - g.av]; f.ps = 1;
    f.m = s.m.as<double>(); f.pt = s.ptype.as<double>(); f.T = s.T.as<double>(); f.sizes = s.hprev.as<double>();
    f.d = d; f.m0 = ctx->cst.m_0;
    const MapHostOut ho{gas_column, dust_column, gas_temperature, dust_temperature, count, skipped, pairs};
    return map_run(ctx, who, f, g, ho, true);
}

extern "C" int sphx_map_last_timing(sphx_ctx* ctx, double ms[5]) { return last_timing(ctx, &sphx_ctx::map_t, ms); }
