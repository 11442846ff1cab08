// sphx_arb.hip - SPH fields sampled at arbitrary points (nsc:1422-1527: neighbors_arb, density_arb, dust_density_arb,
// temperature_arb, dust_temperature_arb, photoionization_arb).
//
// Grid form.  The particles are binned by sphx_build_grid (cell edge = the mean support), turned into ArbRec records
// in cell-sorted order, and the query points are sorted by the same cell key.  A workgroup of one wave takes 64
// consecutive sorted query points, one per lane, and walks the cell rows its points' bounding box can reach:
//   - a particle whose support exceeds ARB_WIDE cells is "wide": it is kept out of the cells' reach and listed apart
//     (in sorted order), so the rows a wave walks follow the typical support and never the largest one;
//   - a row's cells are culled by their largest member support (arb_cell_max), the members of the cells left by their
//     own, against the wave's box; what survives is staged through LDS, 64 records at a time, and every lane adds
//     the pair terms of its own point.
// A point's terms are added in an order fixed by the inputs alone - cells in index order, members in a cell's sorted
// order, then the wide particles in sorted order - and culling only ever drops terms that add nothing, so the result
// does not depend on which other points share the wave: two runs, or the same points in another order, give the
// same bits.  Vector stores only; the one atomic is the integer counter of pair evaluations (one add per wave).
//
// Gate (nsc:1432: a ball of at most one particle returns 0) needs min(count within R, 2).  The sums count the ball
// members they meet; arb_gate_kernel settles the points still below 2 (or every point, when the caller wants full
// counts) exactly: per cell row, the cells wholly inside the ball are counted from cell_start alone, the others
// member by member.  R may be the whole cloud; the sums never depend on it.
//
// List form: one lane per CSR row, in list order (arb_list_kernel) - what pins the arithmetic to the reference.
#include "sphx_wave.h"
#include "sphx_arb_pair.h"
#include <rocprim/rocprim.hpp>

#define ARB_WIDE 2.0              // supports beyond this many cells go to the wide list
#define ARB_SLACK 2e-9            // relative slack of every culling test (positions in cell units carry ~1e-13)
#define ARB_NACC 7

// ---- particle side -----------------------------------------------------------------------------------------------
struct ArbPartIn {
    const double *x, *y, *z;      // SoA positions, source order
    const double *m, *ptype, *sizes, *T, *npart, *value;     // sizes, T, npart, value nullable
    const int* aux_id;            // nullable: npart / value are indexed by aux_id[i] (the state's particle ids)
    double d, m0;
};
__device__ __forceinline__ double arb_h_gas(double m, double m0, double d) { return cbrt(m / m0) * d; }
__device__ __forceinline__ ArbRec arb_make_rec(const ArbPartIn& in, int i, double px, double py, double pz) {
    ArbRec r;
    r.x = px; r.y = py; r.z = pz;
    const double m = in.m[i], t = in.ptype[i];
    const double h = arb_h_gas(m, in.m0, in.d);
    const double s = in.sizes ? in.sizes[i] : 0.0;
    r.fg = (t == 0.0) ? m * SPHX_W6_C / (h * h * h) : 0.0;
    r.ihg = 1.0 / (h * h);
    r.fd = (in.sizes && t == 2.0) ? m * SPHX_W6_C / (s * s * s) : 0.0;
    r.ihd = in.sizes ? 1.0 / (s * s) : 0.0;
    r.T = in.T ? in.T[i] : 0.0;
    const int a = in.aux_id ? in.aux_id[i] : i;
    const bool ph = in.npart && in.value;
    r.pw = (ph && t == 0.0) ? in.npart[a] : 0.0;
    r.val = ph ? sphx_nan_to_num(in.value[a]) : 0.0;
    double sup = 0.0;
    if (t == 0.0 && h > sup) sup = h;
    if (in.sizes && t == 2.0 && s > sup) sup = s;
    r.sup = (sup <= DBL_MAX) ? sup : DBL_MAX;
    r.pad = 0.0;
    return r;
}
__device__ __forceinline__ void arb_store_rec(ArbRec* dst, const ArbRec& r) {
    double2* q = reinterpret_cast<double2*>(dst);
    q[0] = make_double2(r.x, r.y);   q[1] = make_double2(r.z, r.sup);
    q[2] = make_double2(r.fg, r.ihg); q[3] = make_double2(r.fd, r.ihd);
    q[4] = make_double2(r.T, r.pw);  q[5] = make_double2(r.val, r.pad);
}

// {max sizes, max support, sum of supports, particles with a support} -> part[block][4], then out[4]
#define ARB_RED_BLOCKS 256
__global__ __launch_bounds__(256) void arb_reduce_kernel(int n, ArbPartIn in, double* part) {
    __shared__ double sm[4][4];
    double mxs = 0.0, mxu = 0.0, su = 0.0, cn = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const double m = in.m[i], t = in.ptype[i];
        const double s = in.sizes ? in.sizes[i] : 0.0;
        if (s <= DBL_MAX) mxs = fmax(mxs, s);
        double sup = 0.0;
        const double h = arb_h_gas(m, in.m0, in.d);
        if (t == 0.0 && h > sup) sup = h;
        if (in.sizes && t == 2.0 && s > sup) sup = s;
        if (sup > 0.0 && sup <= DBL_MAX) { mxu = fmax(mxu, sup); su += sup; cn += 1.0; }
    }
    mxs = wave_max_f64(mxs); mxu = wave_max_f64(mxu); su = wave_sum_f64(su); cn = wave_sum_f64(cn);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[w][0] = mxs; sm[w][1] = mxu; sm[w][2] = su; sm[w][3] = cn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = part + 4 * blockIdx.x;
        p[0] = fmax(fmax(sm[0][0], sm[1][0]), fmax(sm[2][0], sm[3][0]));
        p[1] = fmax(fmax(sm[0][1], sm[1][1]), fmax(sm[2][1], sm[3][1]));
        p[2] = (sm[0][2] + sm[1][2]) + (sm[2][2] + sm[3][2]);
        p[3] = (sm[0][3] + sm[1][3]) + (sm[2][3] + sm[3][3]);
    }
}
__global__ __launch_bounds__(64) void arb_reduce_final(int nb, const double* part, double* out) {
    double mxs = 0.0, mxu = 0.0, su = 0.0, cn = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) {
        mxs = fmax(mxs, part[4 * b]); mxu = fmax(mxu, part[4 * b + 1]); su += part[4 * b + 2]; cn += part[4 * b + 3];
    }
    mxs = wave_max_f64(mxs); mxu = wave_max_f64(mxu); su = wave_sum_f64(su); cn = wave_sum_f64(cn);
    if (threadIdx.x == 0) { out[0] = mxs; out[1] = mxu; out[2] = su; out[3] = cn; }
}

// records in sorted order (perm: sorted -> source; nullptr: identity = the list form's caller order); sp: the positions
// in sorted order, SoA with stride n (nullptr: in.x / y / z by source index); wide != nullptr: wide[j] = 1 and sup = -1
// for a particle whose support exceeds wcut
__global__ __launch_bounds__(256) void arb_record_kernel(int n, ArbPartIn in, const int* __restrict__ perm,
                                                         const double* __restrict__ sp, double wcut,
                                                         ArbRec* __restrict__ rec, int* __restrict__ wide) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > n) return;
    if (j == n) { if (wide) wide[n] = 0; return; }
    const int src = perm ? perm[j] : j;
    ArbRec r = sp ? arb_make_rec(in, src, sp[j], sp[(size_t)n + j], sp[2 * (size_t)n + j])
                  : arb_make_rec(in, src, in.x[src], in.y[src], in.z[src]);
    if (wide) {
        const int w = r.sup > wcut ? 1 : 0;
        wide[j] = w;
        if (w) r.sup = -1.0;
    }
    arb_store_rec(rec + j, r);
}
// the wide particles' records, in sorted order, with their supports back in place
__global__ __launch_bounds__(256) void arb_wide_kernel(int n, ArbPartIn in, const int* __restrict__ perm,
                                                       const double* __restrict__ sp, const int* __restrict__ wide,
                                                       const int* __restrict__ woff, ArbRec* __restrict__ wrec) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !wide[j]) return;
    arb_store_rec(wrec + woff[j], arb_make_rec(in, perm[j], sp[j], sp[(size_t)n + j], sp[2 * (size_t)n + j]));
}
// largest support among a cell's members that are not wide; -1 for a cell without any
__global__ __launch_bounds__(256) void arb_cell_max(int ncells, const int* __restrict__ cell_start,
                                                    const ArbRec* __restrict__ rec, double* __restrict__ cmax) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncells) return;
    double mx = -1.0;
    for (int j = cell_start[c]; j < cell_start[c + 1]; ++j) mx = fmax(mx, rec[j].sup);
    cmax[c] = mx;
}

// ---- query side ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int arb_cell_coord(double v, double vmin, double inv_cell, int nmax1) {
    double t = (v - vmin) * inv_cell;                  // sphx_grid.hip: cell_coord_g, the same monotone map
    t = fmin(fmax(t, 0.0), (double)nmax1);
    return (int)t;
}
__global__ __launch_bounds__(256) void arb_query_key(int m, const double* __restrict__ q, GridParams g, int* key, int* idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int cx = arb_cell_coord(q[3 * (size_t)i], g.xmin, g.inv_cell, g.nx - 1);
    const int cy = arb_cell_coord(q[3 * (size_t)i + 1], g.ymin, g.inv_cell, g.ny - 1);
    const int cz = arb_cell_coord(q[3 * (size_t)i + 2], g.zmin, g.inv_cell, g.nz - 1);
    key[i] = (cz * g.ny + cy) * g.nx + cx;
    idx[i] = i;
}

struct ArbGridArgs {
    int m;                         // query points
    const double* q;               // (m,3) caller order
    const int* qidx;               // sorted -> caller index
    GridParams g;
    const int* cell_start;
    const double* cmax;
    const double* sp;              // the particles' positions in sorted order, SoA with stride n
    int n;
    const ArbRec* rec;             // n records, sorted order (nullptr in a count-only call: the sums are not formed)
    const ArbRec* wrec;            // the wide particles'
    int nwide;
    double R, R2;                  // the ball
    double wcut;                   // ARB_WIDE cells
    double tb[6];                  // true bounding box of the particles {min xyz, max xyz}
    double* acc;                   // [ARB_NACC][mpad] sums, sorted query order
    int* cnt;                      // [mpad] ball members met
    u64* candidates;
};
// a finite point no farther than R from the particles' bounding box (anything else has an empty ball)
__device__ __forceinline__ bool arb_query_live(const double (&tb)[6], double R, double x, double y, double z) {
    if (!(fabs(x) <= DBL_MAX && fabs(y) <= DBL_MAX && fabs(z) <= DBL_MAX)) return false;
    const double gx = fmax(fmax(tb[0] - x, x - tb[3]), 0.0), gy = fmax(fmax(tb[1] - y, y - tb[4]), 0.0),
                 gz = fmax(fmax(tb[2] - z, z - tb[5]), 0.0);
    return (gx * gx + gy * gy + gz * gz) * (1.0 - ARB_SLACK) <= R * R;
}
// gap between [lo, hi] (cell units) and cell c of an axis of nc cells; the boundary cells are half-infinite (they hold
// whatever was clamped into them)
__device__ __forceinline__ double arb_cell_gap(int c, int nc, double lo, double hi) {
    double g = 0.0;
    if (c > 0) g = fmax(g, (double)c - hi);
    if (c < nc - 1) g = fmax(g, lo - (double)(c + 1));
    return g;
}

struct ArbStage { double x[64], y[64], z[64], fg[64], ihg[64], fd[64], ihd[64], T[64], pw[64], val[64]; };

__global__ __launch_bounds__(64) void arb_grid_kernel(ArbGridArgs a) {
    __shared__ ArbStage st;
    const int lane = threadIdx.x;
    const int qi = blockIdx.x * 64 + lane;
    const int mpad = (a.m + 63) & ~63;
    double qx = 0.0, qy = 0.0, qz = 0.0;
    bool act = false;
    if (qi < a.m) {
        const int src = a.qidx[qi];
        qx = a.q[3 * (size_t)src]; qy = a.q[3 * (size_t)src + 1]; qz = a.q[3 * (size_t)src + 2];
        act = arb_query_live(a.tb, a.R, qx, qy, qz);
    }
    ArbAcc acc = arb_acc_zero();
    const u64 live = __builtin_amdgcn_ballot_w64(act);
    if (live) {
        const GridParams g = a.g;
        // the wave's box, in space and in cell units
        const double lox = wave_min_f64(act ? qx : INFINITY), hix = wave_max_f64(act ? qx : -INFINITY);
        const double loy = wave_min_f64(act ? qy : INFINITY), hiy = wave_max_f64(act ? qy : -INFINITY);
        const double loz = wave_min_f64(act ? qz : INFINITY), hiz = wave_max_f64(act ? qz : -INFINITY);
        const double tlx = (lox - g.xmin) * g.inv_cell, thx = (hix - g.xmin) * g.inv_cell;
        const double tly = (loy - g.ymin) * g.inv_cell, thy = (hiy - g.ymin) * g.inv_cell;
        const double tlz = (loz - g.zmin) * g.inv_cell, thz = (hiz - g.zmin) * g.inv_cell;
        const double wc = a.wcut * (1.0 + ARB_SLACK);
        const int x0 = arb_cell_coord(lox - wc, g.xmin, g.inv_cell, g.nx - 1), x1 = arb_cell_coord(hix + wc, g.xmin, g.inv_cell, g.nx - 1);
        const int y0 = arb_cell_coord(loy - wc, g.ymin, g.inv_cell, g.ny - 1), y1 = arb_cell_coord(hiy + wc, g.ymin, g.inv_cell, g.ny - 1);
        const int z0 = arb_cell_coord(loz - wc, g.zmin, g.inv_cell, g.nz - 1), z1 = arb_cell_coord(hiz + wc, g.zmin, g.inv_cell, g.nz - 1);
        const double cell2 = g.cell * g.cell * (1.0 - ARB_SLACK);
        int staged = 0;
        u64 npairs = 0;
        const int nlive = __popcll(live);

        // every lane adds the staged records' terms to its own point
        auto process = [&]() {
            __syncthreads();
            if (act) {
                for (int t = 0; t < staged; ++t) {
                    const double dx = st.x[t] - qx, dy = st.y[t] - qy, dz = st.z[t] - qz;
                    arb_pair<true>(acc, dx * dx + dy * dy + dz * dz, a.R2, st.fg[t], st.ihg[t], st.fd[t], st.ihd[t], st.T[t],
                             st.pw[t], st.val[t]);
                }
            }
            npairs += (u64)staged * (u64)nlive;
            __syncthreads();
            staged = 0;
        };
        // records [s, e) of `recs`: the ones whose support reaches the wave's box are staged, in order
        auto feed = [&](const ArbRec* recs, int s, int e) {
            for (int base = s; base < e; base += 64) {
                const int j = base + lane;
                bool keep = false;
                double px = 0.0, py = 0.0, pz = 0.0;
                if (j < e) {
                    const double2 p0 = *reinterpret_cast<const double2*>(&recs[j].x);
                    const double2 p1 = *reinterpret_cast<const double2*>(&recs[j].z);
                    px = p0.x; py = p0.y; pz = p1.x;
                    const double sup = p1.y;
                    if (sup >= 0.0) {
                        const double gx = fmax(fmax(lox - px, px - hix), 0.0), gy = fmax(fmax(loy - py, py - hiy), 0.0),
                                     gz = fmax(fmax(loz - pz, pz - hiz), 0.0);
                        keep = (gx * gx + gy * gy + gz * gz) * (1.0 - ARB_SLACK) <= sup * sup;
                    }
                }
                const u64 b = __builtin_amdgcn_ballot_w64(keep);
                const int pc = __popcll(b);
                if (!pc) continue;
                if (staged + pc > 64) process();
                if (keep) {
                    const int pos = staged + __popcll(b & ((1ull << lane) - 1ull));
                    const double2 p2 = *reinterpret_cast<const double2*>(&recs[j].fg);
                    const double2 p3 = *reinterpret_cast<const double2*>(&recs[j].fd);
                    const double2 p4 = *reinterpret_cast<const double2*>(&recs[j].T);
                    st.x[pos] = px; st.y[pos] = py; st.z[pos] = pz;
                    st.fg[pos] = p2.x; st.ihg[pos] = p2.y; st.fd[pos] = p3.x; st.ihd[pos] = p3.y;
                    st.T[pos] = p4.x; st.pw[pos] = p4.y; st.val[pos] = recs[j].val;
                }
                staged += pc;
            }
        };

        for (int cz = z0; cz <= z1; ++cz) {
            const double gz = arb_cell_gap(cz, g.nz, tlz, thz);
            for (int cy = y0; cy <= y1; ++cy) {
                const double gy = arb_cell_gap(cy, g.ny, tly, thy);
                const double gyz = gy * gy + gz * gz;
                const int row = (cz * g.ny + cy) * g.nx;
                int first = -1, last = -1;
                for (int cb = x0; cb <= x1; cb += 64) {
                    const int cx = cb + lane;
                    bool keep = false;
                    if (cx <= x1) {
                        const double cm = a.cmax[row + cx];
                        if (cm >= 0.0) {
                            const double gx = arb_cell_gap(cx, g.nx, tlx, thx);
                            keep = (gx * gx + gyz) * cell2 <= cm * cm;
                        }
                    }
                    const u64 b = __builtin_amdgcn_ballot_w64(keep);
                    if (b) {
                        if (first < 0) first = cb + __builtin_ctzll(b);
                        last = cb + 63 - __builtin_clzll(b);
                    }
                }
                if (first < 0) continue;
                feed(a.rec, a.cell_start[row + first], a.cell_start[row + last + 1]);
            }
        }
        feed(a.wrec, 0, a.nwide);
        if (staged) process();
        if (lane == 0 && npairs) atomicAdd(a.candidates, npairs);
    }
    if (qi < a.m) {
        a.acc[0 * (size_t)mpad + qi] = acc.dens; a.acc[1 * (size_t)mpad + qi] = acc.tn; a.acc[2 * (size_t)mpad + qi] = acc.td;
        a.acc[3 * (size_t)mpad + qi] = acc.dd;   a.acc[4 * (size_t)mpad + qi] = acc.dtn; a.acc[5 * (size_t)mpad + qi] = acc.pn;
        a.acc[6 * (size_t)mpad + qi] = acc.pd;
        a.cnt[qi] = acc.cnt;
    }
}

// the outputs of sphx_arb_fields*, device side: (m,) each, caller order; nullptr: not wanted
struct ArbOutPtrs { double *density, *dust_density, *temperature, *dust_temperature, *photoionization; long long* count; };
__device__ __forceinline__ void arb_write_out(const ArbOutPtrs& o, int dst, const ArbAcc& acc, long long count) {
    const ArbOut r = arb_finish(acc, count > 1);
    if (o.density) o.density[dst] = r.density;
    if (o.dust_density) o.dust_density[dst] = r.dust_density;
    if (o.temperature) o.temperature[dst] = r.temperature;
    if (o.dust_temperature) o.dust_temperature[dst] = r.dust_temperature;
    if (o.photoionization) o.photoionization[dst] = r.photoionization;
    if (o.count) o.count[dst] = count;
}

// Settles the ball count of every point the sums left below 2 (full: of every point, exactly), applies the gate and
// writes the outputs in caller order.  One lane per sorted query point.
__global__ __launch_bounds__(64) void arb_gate_kernel(ArbGridArgs a, int full, ArbOutPtrs out) {
    const int qi = blockIdx.x * 64 + threadIdx.x;
    if (qi >= a.m) return;
    const int mpad = (a.m + 63) & ~63;
    const int src = a.qidx[qi];
    const double qx = a.q[3 * (size_t)src], qy = a.q[3 * (size_t)src + 1], qz = a.q[3 * (size_t)src + 2];
    long long c = a.cnt[qi];
    if ((full || c < 2) && arb_query_live(a.tb, a.R, qx, qy, qz)) {
        const GridParams g = a.g;
        c = 0;
        const double Rp = a.R * (1.0 + ARB_SLACK);
        const int x0 = arb_cell_coord(qx - Rp, g.xmin, g.inv_cell, g.nx - 1), x1 = arb_cell_coord(qx + Rp, g.xmin, g.inv_cell, g.nx - 1);
        const int y0 = arb_cell_coord(qy - Rp, g.ymin, g.inv_cell, g.ny - 1), y1 = arb_cell_coord(qy + Rp, g.ymin, g.inv_cell, g.ny - 1);
        const int z0 = arb_cell_coord(qz - Rp, g.zmin, g.inv_cell, g.nz - 1), z1 = arb_cell_coord(qz + Rp, g.zmin, g.inv_cell, g.nz - 1);
        const double tx = (qx - g.xmin) * g.inv_cell, ty = (qy - g.ymin) * g.inv_cell, tz = (qz - g.zmin) * g.inv_cell;
        const double Rc = a.R * g.inv_cell;                   // the radius in cell units
        const double Rin2 = Rc * Rc * (1.0 - ARB_SLACK), Rout2 = Rc * Rc * (1.0 + ARB_SLACK);
        auto members = [&](int s, int e) {
            for (int j = s; j < e; ++j) {
                const double dx = a.sp[j] - qx, dy = a.sp[(size_t)a.n + j] - qy, dz = a.sp[2 * (size_t)a.n + j] - qz;
                if (dx * dx + dy * dy + dz * dz <= a.R2) ++c;
                if (!full && c >= 2) return;
            }
        };
        for (int cz = z0; cz <= z1 && (full || c < 2); ++cz) {
            const double gz = arb_cell_gap(cz, g.nz, tz, tz);
            const bool zin = cz > 0 && cz < g.nz - 1;
            const double fz = fmax(fabs(tz - (double)cz), fabs((double)(cz + 1) - tz));
            for (int cy = y0; cy <= y1 && (full || c < 2); ++cy) {
                const double gy = arb_cell_gap(cy, g.ny, ty, ty);
                if (gy * gy + gz * gz > Rout2) continue;
                const int row = (cz * g.ny + cy) * g.nx;
                const bool yin = cy > 0 && cy < g.ny - 1;
                const double fy = fmax(fabs(ty - (double)cy), fabs((double)(cy + 1) - ty));
                // the cells of this row wholly inside the ball: an interval [ia, ib] of interior cells
                int ia = 1, ib = 0;
                const double rem = Rin2 - fy * fy - fz * fz;
                if (zin && yin && rem > 0.0) {
                    const double rr = sqrt(rem);
                    const double lo = ceil(tx - rr), hi = floor(tx + rr) - 1.0;
                    const int i0 = x0 > 1 ? x0 : 1, i1 = x1 < g.nx - 2 ? x1 : g.nx - 2;
                    ia = lo > (double)i0 ? (lo > (double)i1 ? i1 + 1 : (int)lo) : i0;
                    ib = hi < (double)i1 ? (hi < (double)i0 ? i0 - 1 : (int)hi) : i1;
                }
                if (ia <= ib) {
                    c += a.cell_start[row + ib + 1] - a.cell_start[row + ia];
                    if (full || c < 2) members(a.cell_start[row + x0], a.cell_start[row + ia]);
                    if (full || c < 2) members(a.cell_start[row + ib + 1], a.cell_start[row + x1 + 1]);
                } else {
                    members(a.cell_start[row + x0], a.cell_start[row + x1 + 1]);
                }
            }
        }
    }
    ArbAcc acc;
    acc.dens = a.acc[0 * (size_t)mpad + qi]; acc.tn = a.acc[1 * (size_t)mpad + qi]; acc.td = a.acc[2 * (size_t)mpad + qi];
    acc.dd = a.acc[3 * (size_t)mpad + qi];   acc.dtn = a.acc[4 * (size_t)mpad + qi]; acc.pn = a.acc[5 * (size_t)mpad + qi];
    acc.pd = a.acc[6 * (size_t)mpad + qi];
    acc.cnt = 0;
    arb_write_out(out, src, acc, c);
}

// ---- list form: one lane per row, in list order ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void arb_list_kernel(int m, int n, const double* __restrict__ q,
                                                      const long long* __restrict__ row_start,
                                                      const long long* __restrict__ members, const ArbRec* __restrict__ rec,
                                                      ArbOutPtrs out, u64* candidates) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    u64 np = 0;
    if (i < m) {
        const double qx = q[3 * (size_t)i], qy = q[3 * (size_t)i + 1], qz = q[3 * (size_t)i + 2];
        ArbAcc acc = arb_acc_zero();
        const long long s = row_start[i], e = row_start[i + 1];
        for (long long p = s; p < e; ++p) {
            const long long id = members[p];
            if (id < 0 || id >= (long long)n) continue;
            const ArbRec* r = rec + id;
            const double2 p0 = *reinterpret_cast<const double2*>(&r->x), p1 = *reinterpret_cast<const double2*>(&r->z);
            const double2 p2 = *reinterpret_cast<const double2*>(&r->fg), p3 = *reinterpret_cast<const double2*>(&r->fd);
            const double2 p4 = *reinterpret_cast<const double2*>(&r->T);
            const double dx = p0.x - qx, dy = p0.y - qy, dz = p1.x - qz;
            arb_pair<false>(acc, dx * dx + dy * dy + dz * dz, INFINITY, p2.x, p2.y, p3.x, p3.y, p4.x, p4.y, r->val);
            ++np;
        }
        arb_write_out(out, i, acc, e - s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) np += __shfl_xor(np, o, 64);
    if (threadIdx.x == 0 && np) atomicAdd(candidates, np);
}

// =====================================================================================================================
// host side
// =====================================================================================================================
struct ArbHostOut { double *density, *dust_density, *temperature, *dust_temperature, *photoionization; int64_t* count; };

// device output block [6][m] in ctx->arb_out, pointers only for what the caller wants and the inputs allow
static int arb_out_ptrs(sphx_ctx* ctx, int64_t m, const ArbHostOut& h, bool has_sizes, bool has_T, bool has_ph, ArbOutPtrs* o) {
    const size_t mm = (size_t)(m > 0 ? m : 1);
    Carve c;
    c.take(o->density, mm); c.take(o->dust_density, mm); c.take(o->temperature, mm); c.take(o->dust_temperature, mm);
    c.take(o->photoionization, mm); c.take(o->count, mm);
    SPHX_TRY(sphx_carve_into(ctx, ctx->arb_out, c));
    if (!h.density) o->density = nullptr;
    if (!(h.dust_density && has_sizes)) o->dust_density = nullptr;
    if (!(h.temperature && has_T)) o->temperature = nullptr;
    if (!(h.dust_temperature && has_sizes && has_T)) o->dust_temperature = nullptr;
    if (!(h.photoionization && has_ph)) o->photoionization = nullptr;
    if (!h.count) o->count = nullptr;
    return SPHX_OK;
}
static int arb_out_download(sphx_ctx* ctx, int64_t m, const ArbHostOut& h, const ArbOutPtrs& o, const u64* cand_dev, int64_t* candidates) {
    const size_t md = (size_t)m;                           // (count: int64, the width of a double)
    const CopyF64 ps[] = {{h.density, o.density, md}, {h.dust_density, o.dust_density, md}, {h.temperature, o.temperature, md},
                          {h.dust_temperature, o.dust_temperature, md}, {h.photoionization, o.photoionization, md},
                          {h.count, o.count, md}};
    SPHX_TRY(sphx_download_f64(ctx, ps, 6));
    u64* cand = &ctx->pinned->side.cand;
    HIPCHK(hipMemcpyAsync(cand, cand_dev, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    SPHX_TRY(ctx->arb_t.mark(ctx, 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (candidates) *candidates = (int64_t)*cand;
    return ctx->arb_t.end(ctx);
}
// ctx->arb_red: the reduction's result (4 of 8 doubles) | the candidates counter | from the next 128-byte line, block partials
struct ArbRed { double* res; u64* cand; double* part; };
static int arb_red_prepare(sphx_ctx* ctx, ArbRed* r) {
    Carve c;
    c.take(r->res, 8); c.take(r->cand, 1); c.take(r->part, 4 * ARB_RED_BLOCKS, 128);
    SPHX_TRY(sphx_carve_into(ctx, ctx->arb_red, c));
    HIPCHK(hipMemsetAsync(r->res, 0, (size_t)(r->part - r->res) * sizeof(double), ctx->stream));
    return SPHX_OK;
}

static bool arb_ball_hit(const sphx_ctx* ctx, int64_t ball_id, int64_t n, int64_t m) {
    return ball_id != 0 && ctx->arb_ball_id == ball_id && ctx->arb_ball_n == n && ctx->arb_ball_m == m;
}

// The grid form on particles whose attributes are on the device already (any order); the query points come from the
// host.  hit: the geometry of this ball - sorted positions, cell list, query points and their sorted order - is the one the
// context holds (arb_ball_hit): in.x / y / z and arb_points are not read.  Without any field output only the counts
// are formed (no records, no sums).
static int arb_run_grid(sphx_ctx* ctx, int64_t n, const ArbPartIn& in, int64_t m, const double* arb_points, double radius,
                        const ArbHostOut& hout, int64_t* candidates, int64_t ball_id, bool hit) {
    ArbRed red;
    SPHX_TRY(arb_red_prepare(ctx, &red));
    const bool has_ph = in.npart && in.value;
    ArbOutPtrs o;
    SPHX_TRY(arb_out_ptrs(ctx, m, hout, in.sizes != nullptr, in.T != nullptr, has_ph, &o));
    if (m == 0) { if (candidates) *candidates = 0; return SPHX_OK; }
    const bool sums = o.density || o.dust_density || o.temperature || o.dust_temperature || o.photoionization;
    const int64_t mpad = sphx_pad64(m);
    if (!hit) {
        ctx->arb_ball_id = 0;                              // (the held geometry is being replaced)
        SPHX_TRY(sphx_ensure(ctx, ctx->arb_q, (size_t)m * 3 * sizeof(double)));
        HIPCHK(hipMemcpyAsync(ctx->arb_q.p, arb_points, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    // the query points' keys and order, and their sorted copies (a hit: the buffer stands, with the sorted order in it)
    int *key, *idx, *key2, *idx2;
    Carve ck;
    ck.take(key, (size_t)mpad); ck.take(idx, (size_t)mpad); ck.take(key2, (size_t)mpad); ck.take(idx2, (size_t)mpad);
    SPHX_TRY(sphx_carve_into(ctx, ctx->arb_key, ck));
    // the points' sums, then their counts
    ArbGridArgs a;
    Carve ca;
    ca.take(a.acc, ARB_NACC * (size_t)mpad); ca.take(a.cnt, (size_t)mpad);
    SPHX_TRY(sphx_carve_into(ctx, ctx->arb_acc, ca));
    SPHX_TRY(ctx->arb_t.mark(ctx, 1));
    // supports: the ball's radius and, for a new geometry, the cell size
    double R = radius, cell_hint = 0.0;
    if (!hit || !(radius > 0.0)) {
        int rb = (int)((n + 255) / 256);
        if (rb > ARB_RED_BLOCKS) rb = ARB_RED_BLOCKS;
        hipLaunchKernelGGL(arb_reduce_kernel, dim3(rb), dim3(256), 0, ctx->stream, (int)n, in, red.part);
        hipLaunchKernelGGL(arb_reduce_final, dim3(1), dim3(64), 0, ctx->stream, rb, red.part, red.res);
        HIPCHK(hipGetLastError());
        const double* rd = ctx->pinned->side.red;
        HIPCHK(hipMemcpyAsync(ctx->pinned->side.red, red.res, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (!(radius > 0.0)) R = rd[0];
        cell_hint = rd[3] > 0.0 ? rd[2] / rd[3] : 0.0;     // the mean support
    }
    if (!(R > 0.0) || !(R <= DBL_MAX))
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_arb_fields: no ball radius (radius <= 0 and no positive finite sizes)");
    if (!hit) {
        ctx->map_perm = nullptr;
        ctx->qorder = nullptr;
        ctx->clip_valid = false;
        SPHX_TRY(sphx_build_grid(ctx, n, 40, in.x, in.y, in.z, cell_hint));
        const GridParams g = ctx->grid;
        // the geometry into buffers of this file's own: the grid's are every entry point's scratch
        SPHX_TRY(sphx_ensure(ctx, ctx->arb_pos, (size_t)n * 3 * sizeof(double)));
        SPHX_TRY(sphx_ensure(ctx, ctx->arb_cs, ((size_t)g.ncells + 2) * sizeof(int)));
        SPHX_TRY(sphx_ensure(ctx, ctx->arb_perm, (size_t)n * sizeof(int)));
        HIPCHK(hipMemcpyAsync(ctx->arb_cs.p, ctx->cell_start.p, ((size_t)g.ncells + 1) * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->arb_perm.p, ctx->perm.p, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        double* sp0 = ctx->arb_pos.as<double>();
        SPHX_TRY(sphx_gather3(ctx, n, ctx->arb_perm.as<int>(), in.x, in.y, in.z, sp0, sp0 + n, sp0 + 2 * n));
        ctx->arb_g = g;
        for (int c = 0; c < 6; ++c) ctx->arb_tb[c] = ctx->tbox_h[c];
        // query points: key, stable sort by cell (equal keys keep the caller's order)
        hipLaunchKernelGGL(arb_query_key, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, (int)m,
                           ctx->arb_q.as<double>(), g, key, idx);
        HIPCHK(hipGetLastError());
        int bits = 1;
        while (bits < 31 && (1ll << bits) < (long long)g.ncells) ++bits;
        size_t tmp_bytes = 0;
        HIPCHK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key, key2, idx, idx2, (size_t)m, 0, bits, ctx->stream));
        SPHX_TRY(sphx_ensure(ctx, ctx->arb_tmp, tmp_bytes + 64));
        HIPCHK(rocprim::radix_sort_pairs(ctx->arb_tmp.p, tmp_bytes, key, key2, idx, idx2, (size_t)m, 0, bits, ctx->stream));
        if (ball_id) { ctx->arb_ball_id = ball_id; ctx->arb_ball_n = n; ctx->arb_ball_m = m; }
    }
    const GridParams g = ctx->arb_g;
    const int* perm = ctx->arb_perm.as<int>();
    const int* cell_start = ctx->arb_cs.as<int>();
    const double* sp = ctx->arb_pos.as<double>();
    const double wcut = ARB_WIDE * g.cell;
    int nwide = 0;
    ArbRec* rec = nullptr;
    if (sums) {                                            // records, wide list, per-cell maxima
        SPHX_TRY(sphx_ensure(ctx, ctx->arb_rec, (size_t)n * sizeof(ArbRec)));
        // the wide flags (n + 1 and four of head-room) | their scan, 16-byte aligned: the single-launch scan wants it
        // (the room as it has been: 2 (n + 8) ints and 64 bytes)
        int *wide, *woff;
        Carve cf;
        cf.take(wide, (size_t)n + 5, 16); cf.take(woff, (size_t)n + 11, 16);
        cf.slack(64);
        SPHX_TRY(sphx_carve_into(ctx, ctx->arb_flag, cf));
        SPHX_TRY(sphx_ensure(ctx, ctx->arb_cmax, (size_t)g.ncells * sizeof(double)));
        rec = ctx->arb_rec.as<ArbRec>();
        hipLaunchKernelGGL(arb_record_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, ctx->stream, (int)n, in, perm, sp,
                           wcut, rec, wide);
        HIPCHK(hipGetLastError());
        SPHX_TRY(sphx_excl_scan_int(ctx, wide, woff, (int)n));
        HIPCHK(hipMemcpyAsync(&ctx->pinned->side.count, woff + n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        hipLaunchKernelGGL(arb_cell_max, dim3((unsigned)((g.ncells + 255) / 256)), dim3(256), 0, ctx->stream, g.ncells,
                           cell_start, rec, ctx->arb_cmax.as<double>());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        nwide = ctx->pinned->side.count;
        SPHX_TRY(sphx_ensure(ctx, ctx->arb_wrec, (size_t)(nwide > 0 ? nwide : 1) * sizeof(ArbRec)));
        if (nwide > 0)
            hipLaunchKernelGGL(arb_wide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (int)n, in, perm, sp,
                               wide, woff, ctx->arb_wrec.as<ArbRec>());
    }
    SPHX_TRY(ctx->arb_t.mark(ctx, 2));
    a.m = (int)m;
    a.q = ctx->arb_q.as<double>();
    a.qidx = idx2;
    a.g = g;
    a.cell_start = cell_start;
    a.cmax = ctx->arb_cmax.as<double>();
    a.sp = sp;
    a.n = (int)n;
    a.rec = rec;
    a.wrec = ctx->arb_wrec.as<ArbRec>();
    a.nwide = nwide;
    a.R = R; a.R2 = R * R;
    a.wcut = wcut;
    for (int c = 0; c < 6; ++c) a.tb[c] = ctx->arb_tb[c];
    a.candidates = red.cand;
    const unsigned nb = (unsigned)(mpad / 64);
    if (sums) hipLaunchKernelGGL(arb_grid_kernel, dim3(nb), dim3(64), 0, ctx->stream, a);
    else HIPCHK(hipMemsetAsync(a.acc, 0, ca.bytes(), ctx->stream));
    hipLaunchKernelGGL(arb_gate_kernel, dim3(nb), dim3(64), 0, ctx->stream, a, hout.count ? 1 : 0, o);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->arb_t.mark(ctx, 3));
    return arb_out_download(ctx, m, hout, o, red.cand, candidates);
}

static int arb_check_common(sphx_ctx* ctx, const char* who, int64_t n, int64_t m, const void* arb_points) {
    if (n < 1 || n > 0x7FFFFFF0ll) return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld out of range", who, (long long)n);
    if (m < 0 || m > 0x7FFFFF00ll / 3) return sphx_set_err(ctx, SPHX_E_ARG, "%s: m=%lld out of range", who, (long long)m);
    if (m > 0 && !arb_points) return sphx_set_err(ctx, SPHX_E_ARG, "%s: argument arb_points is NULL", who);
    return SPHX_OK;
}

// host arrays -> device staging (in_a .. in_j), SoA positions; fills `in`
static int arb_stage_particles(sphx_ctx* ctx, int64_t n, const double* points, const double* mass, const double* ptype,
                               const double* sizes, const double* T, const double* n_part, const double* value, double d,
                               ArbPartIn* in) {
    const size_t nb = (size_t)n * sizeof(double);
    SPHX_TRY(sphx_ensure(ctx, ctx->in_a, 3 * nb));
    DevBuf* bufs[] = {&ctx->in_b, &ctx->in_c, &ctx->in_d, &ctx->in_e, &ctx->in_f, &ctx->in_g, &ctx->in_h, &ctx->in_i, &ctx->in_j};
    for (DevBuf* b : bufs) SPHX_TRY(sphx_ensure(ctx, *b, nb));
    double *x = nullptr, *y = nullptr, *z = nullptr;
    if (points) {                                          // (NULL: the positions are on the device already - a held ball)
        HIPCHK(hipMemcpyAsync(ctx->in_a.p, points, 3 * nb, hipMemcpyHostToDevice, ctx->stream));
        x = ctx->in_b.as<double>(); y = ctx->in_c.as<double>(); z = ctx->in_d.as<double>();
        SPHX_TRY(sphx_aos_to_soa3(ctx, n, ctx->in_a.as<double>(), x, y, z));
    }
    in->x = x; in->y = y; in->z = z;
    const size_t nd = (size_t)n;
    const CopyF64 us[] = {{mass, ctx->in_e.p, nd}, {ptype, ctx->in_f.p, nd}, {sizes, ctx->in_g.p, nd},
                          {T, ctx->in_h.p, nd}, {n_part, ctx->in_i.p, nd}, {value, ctx->in_j.p, nd}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 6));
    auto given = [](const double* host, const DevBuf& b) { return host ? b.as<double>() : nullptr; };
    in->m = given(mass, ctx->in_e); in->ptype = given(ptype, ctx->in_f); in->sizes = given(sizes, ctx->in_g);
    in->T = given(T, ctx->in_h); in->npart = given(n_part, ctx->in_i); in->value = given(value, ctx->in_j);
    in->aux_id = nullptr;
    in->d = d;
    in->m0 = ctx->cst.m_0;
    return SPHX_OK;
}

extern "C" int sphx_arb_fields(sphx_ctx* ctx, int64_t n, const double* points, const double* mass,
                               const double* particle_type, const double* sizes, const double* T, const double* n_part,
                               const double* value, double d, int64_t m, const double* arb_points, double radius,
                               double* density, double* dust_density, double* temperature, double* dust_temperature,
                               double* photoionization, int64_t* count, int64_t* candidates, int64_t ball_id) {
    if (!ctx) return SPHX_E_ARG;
    NEED(points); NEED(mass); NEED(particle_type);
    SPHX_TRY(arb_check_common(ctx, "sphx_arb_fields", n, m, arb_points));
    if (!sizes && !(radius > 0.0))
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_arb_fields: radius <= 0 means max(sizes), but sizes is NULL");
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->arb_t.begin(ctx));
    const bool hit = arb_ball_hit(ctx, ball_id, n, m);
    ArbPartIn in;
    SPHX_TRY(arb_stage_particles(ctx, n, hit ? nullptr : points, mass, particle_type, sizes, T, n_part, value, d, &in));
    const ArbHostOut hout{density, dust_density, temperature, dust_temperature, photoionization, count};
    return arb_run_grid(ctx, n, in, m, arb_points, radius, hout, candidates, ball_id, hit);
}

extern "C" int sphx_arb_fields_list(sphx_ctx* ctx, int64_t n, const double* points, const double* mass,
                                    const double* particle_type, const double* sizes, const double* T,
                                    const double* n_part, const double* value, double d, int64_t m,
                                    const double* arb_points, const int64_t* row_start, const int64_t* members,
                                    double* density, double* dust_density, double* temperature,
                                    double* dust_temperature, double* photoionization, int64_t* count,
                                    int64_t* candidates) {
    if (!ctx) return SPHX_E_ARG;
    NEED(points); NEED(mass); NEED(particle_type); NEED(row_start);
    SPHX_TRY(arb_check_common(ctx, "sphx_arb_fields_list", n, m, arb_points));
    if (row_start[0] < 0) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_arb_fields_list: row_start[0] < 0");
    for (int64_t i = 0; i < m; ++i)
        if (row_start[i + 1] < row_start[i])
            return sphx_set_err(ctx, SPHX_E_ARG, "sphx_arb_fields_list: row_start decreases at row %lld", (long long)i);
    const int64_t nnz = row_start[m];
    if (nnz > row_start[0] && !members) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_arb_fields_list: argument members is NULL");
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->arb_t.begin(ctx));
    ctx->arb_ball_id = 0;                                  // (the query buffers of a held ball are overwritten below)
    ArbPartIn in;
    SPHX_TRY(arb_stage_particles(ctx, n, points, mass, particle_type, sizes, T, n_part, value, d, &in));
    ArbRed red;
    SPHX_TRY(arb_red_prepare(ctx, &red));
    const ArbHostOut hout{density, dust_density, temperature, dust_temperature, photoionization, count};
    ArbOutPtrs o;
    SPHX_TRY(arb_out_ptrs(ctx, m, hout, sizes != nullptr, T != nullptr, n_part && value, &o));
    if (m == 0) { if (candidates) *candidates = 0; return SPHX_OK; }
    SPHX_TRY(sphx_ensure(ctx, ctx->arb_rec, (size_t)n * sizeof(ArbRec)));
    SPHX_TRY(sphx_ensure(ctx, ctx->arb_q, (size_t)m * 3 * sizeof(double)));
    SPHX_TRY(sphx_ensure(ctx, ctx->arb_key, ((size_t)m + 1) * sizeof(int64_t)));
    SPHX_TRY(sphx_ensure(ctx, ctx->arb_tmp, (size_t)(nnz > 0 ? nnz : 1) * sizeof(int64_t)));
    HIPCHK(hipMemcpyAsync(ctx->arb_q.p, arb_points, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->arb_key.p, row_start, ((size_t)m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    if (nnz > 0) HIPCHK(hipMemcpyAsync(ctx->arb_tmp.p, members, (size_t)nnz * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    SPHX_TRY(ctx->arb_t.mark(ctx, 1));
    hipLaunchKernelGGL(arb_record_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, ctx->stream, (int)n, in,
                       (const int*)nullptr, (const double*)nullptr, 0.0, ctx->arb_rec.as<ArbRec>(), (int*)nullptr);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->arb_t.mark(ctx, 2));
    hipLaunchKernelGGL(arb_list_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, ctx->stream, (int)m, (int)n,
                       ctx->arb_q.as<double>(), ctx->arb_key.as<long long>(), ctx->arb_tmp.as<long long>(),
                       ctx->arb_rec.as<ArbRec>(), o, red.cand);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->arb_t.mark(ctx, 3));
    return arb_out_download(ctx, m, hout, o, red.cand, candidates);
}

// The grid form on the step loop's resident state.  The grid build works in buffers the step rebuilds from scratch
// every step; what it leaves on the host side of the context (the grid, the statistics window of the robust box, the
// cell statistics) is put back, so the next sphx_step sizes its grid as if this call had not happened.
extern "C" int sphx_state_sample(sphx_ctx* ctx, double d, const double* n_part, const double* value, int64_t m,
                                 const double* arb_points, double radius, double* density, double* dust_density,
                                 double* temperature, double* dust_temperature, double* photoionization, int64_t* count,
                                 int64_t* candidates) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_sample: no state uploaded");
    if (ctx->step_count < 1)
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_sample before the first sphx_step: sizes do not exist yet");
    const int64_t n = ctx->n;
    SPHX_TRY(arb_check_common(ctx, "sphx_state_sample", n, m, arb_points));
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->arb_t.begin(ctx));
    const size_t nb = (size_t)n * sizeof(double);
    StateArrays& s = ctx->st;
    ArbPartIn in;
    in.x = s.x.as<double>(); in.y = s.y.as<double>(); in.z = s.z.as<double>();
    in.m = s.m.as<double>(); in.ptype = s.ptype.as<double>(); in.sizes = s.hprev.as<double>(); in.T = s.T.as<double>();
    in.npart = in.value = nullptr;
    in.aux_id = s.id.as<int>();
    if (n_part && value) {
        SPHX_TRY(sphx_ensure(ctx, ctx->in_i, nb));
        SPHX_TRY(sphx_ensure(ctx, ctx->in_j, nb));
        HIPCHK(hipMemcpyAsync(ctx->in_i.p, n_part, nb, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->in_j.p, value, nb, hipMemcpyHostToDevice, ctx->stream));
        in.npart = ctx->in_i.as<double>(); in.value = ctx->in_j.as<double>();
    }
    in.d = d;
    in.m0 = ctx->cst.m_0;
    const ArbHostOut hout{density, dust_density, temperature, dust_temperature, photoionization, count};
    const GridHostState saved = sphx_grid_host_save(ctx);
    const int rc = arb_run_grid(ctx, n, in, m, arb_points, radius, hout, candidates, 0, false);
    sphx_grid_host_restore(ctx, saved);
    return rc;
}
