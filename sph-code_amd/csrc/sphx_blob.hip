// sphx_blob.hip - the sum passes of the step loop with the neighbour records staged in LDS.
//
// In blob order (sphx_grid.hip: sphx_build_blob_order) the BLOB_P particles of a workgroup form a
// compact blob and share most of their neighbours: 128 particles x 40 references name only ~600
// distinct particles.  blob_dedup_kernel finds that distinct set once per step with an open-
// addressing hash table in LDS whose entry number IS the slot number: it rewrites the workgroup's
// part of the neighbour list as 16-bit slot numbers and stores the table (slot -> particle, -1 =
// empty).  Each pass then fetches every distinct record ONCE per workgroup into an LDS image
// (~5 gathers per particle instead of 40) and runs its neighbour loop out of LDS.
//
// LPP = 4 lanes serve one particle: lane 4t+q sums the list positions k = q mod 4, and the four
// partial sums are added at the end as (p0 + p1) + (p2 + p3) by two DPP exchanges - the same fixed
// order the gather kernels of sphx_sums.hip use, so the results are bit-identical to theirs.  512
// threads per workgroup, two workgroups per CU (LDS-bound): four waves per SIMD hide LDS latency
// (two lanes per particle, i.e. two waves per SIMD, measured 10 % slower), and one workgroup stages
// while the other computes.
//
// LDS image: BLOB_S slots; a record is kept as 16-byte chunks, chunk c of slot s at
// (c * BLOB_S + s) * 16, so one ds_read_b128 of 16 lanes meets 16 bank-quads selected by s mod 16.
// The workgroup's slot lists (K x BLOB_P x 2 B) sit next to it: the neighbour loop touches only LDS.
// A reference that found no free entry within BLOB_PROBES probes (blobs with more than ~900
// distinct neighbours; the most seen at BLOB_P = 128 is ~800) keeps the 0xFFFE marker and is
// fetched from global memory through the int32 list.
//
// What is computed for a neighbour is not written here: a pass hands its operands to the term functions of sphx_pair.h,
// which the gather kernels call too.  How a pass walks its blobs and slot lists is not written here either: blob_pass
// (sphx_blob.h) does, for the pass descriptions below and those of sphx_loopforms.hip.
#include "sphx_blob.h"
#include "sphx_wave.h"
#pragma clang fp contract(off)            // (as sphx_pair.h: NumPy never fuses a multiply into an add)
#include <float.h>
#include <stdlib.h>
#include <stdio.h>
#ifndef BLOB_PI_SATURATES
#define BLOB_PI_SATURATES 1          // pass 2 stops summing Pi in a wave whose rows' sums are all NaN (0: sums on)
#endif

// ---- once per step: distinct neighbours of each workgroup ------------------------------------
// Phase 1: every reference is inserted into a sparse open-addressing table of particle indices
// (DD_TAB entries for <= ~900 distinct keys: 1.2 probes on average, where a table as small as the
// image needed 3-4 and its slowest lane 15) and remembers the entry it landed in (LDS tile, 16 bit).
// Phase 2: the occupied entries are numbered in table order by a workgroup prefix sum - the image
// slots, dense from 0 - and written out as the slot -> particle table.  Phase 3: the tile is
// translated entry -> slot in place and leaves as whole 256-B rows.  (The slot numbering depends on
// which lane won an entry; no sum depends on it.)
#define DD_TAB 2048
#define DD_PROBES 64
__device__ __forceinline__ unsigned dd_hash(int j) { return ((unsigned)j * 2654435761u) >> 21; }

// bclass (device API, decomposed runs; nullptr otherwise): what the workgroup's particles need from other ranks -
// 0 "interior": some of its particles are owned and every neighbour of theirs is owned too, so its sums can run before
// the ghosts' values of the step have arrived; 1 "boundary"; 2: all of its particles are ghosts (nothing to compute).
__global__ __launch_bounds__(BLOB_T) void blob_dedup_kernel(int n, int npad, int k, int slots,
                                                            const int* __restrict__ nbr, u16* slot16,
                                                            int* uniq, const int* __restrict__ qorder,
                                                            const int* __restrict__ omap, int n_active,
                                                            unsigned char* bclass) {
    __builtin_amdgcn_s_setprio(DEDUP_PRIO);      // ahead of the record build that streams beside it on the other stream: this kernel is the one the passes wait for (step -13 us)
    extern __shared__ u16 dd_tile[];              // [k][BLOB_P] entry / slot numbers
    __shared__ int key[DD_TAB];
    __shared__ u16 slot_of[DD_TAB];
    __shared__ int wave_tot[BLOB_T / 64];
    const int b = xcd_block(blockIdx.x, gridDim.x);
    const int t = threadIdx.x >> 1, half = threadIdx.x & 1;
    const int p = b * BLOB_P + t;
    for (int q = threadIdx.x; q < DD_TAB; q += BLOB_T) key[q] = -1;
    __syncthreads();
    {
        const int nm = (k + 1) >> 1;
        const bool live = p < n;
        int jn[DD_BATCH];                         // the next batch is in flight while this one is hashed
#pragma unroll
        for (int u = 0; u < DD_BATCH; ++u) {
            const int kk = 2 * u + half;
            jn[u] = (kk < k && live) ? nbr[(size_t)kk * npad + p] : -1;
        }
        for (int m0 = 0; m0 < nm; m0 += DD_BATCH) {
            int jb[DD_BATCH];
#pragma unroll
            for (int u = 0; u < DD_BATCH; ++u) {
                jb[u] = jn[u];
                const int kk = 2 * (m0 + DD_BATCH + u) + half;
                jn[u] = (kk < k && live) ? nbr[(size_t)kk * npad + p] : -1;
            }
            // first probe of the whole batch side by side (the table is sparse: 1.2 probes on average, so nearly every
            // reference is settled here with its LDS round trips overlapped instead of chained), then the stragglers
            unsigned hb[DD_BATCH];
            int eb[DD_BATCH];
#pragma unroll
            for (int u = 0; u < DD_BATCH; ++u) {
                hb[u] = dd_hash(jb[u] < 0 ? 0 : jb[u]);
                eb[u] = key[hb[u]];
            }
#pragma unroll
            for (int u = 0; u < DD_BATCH; ++u)
                if (jb[u] >= 0 && eb[u] == -1) {
                    const int old = atomicCAS(&key[hb[u]], -1, jb[u]);
                    eb[u] = (old == -1) ? jb[u] : old;
                }
#pragma unroll
            for (int u = 0; u < DD_BATCH; ++u) {
                const int kk = 2 * (m0 + u) + half;
                if (kk >= k) continue;
                const int j = jb[u];
                unsigned s = SLOT_NONE;
                if (j >= 0) {
                    unsigned h = hb[u];
                    s = SLOT_OVER;
                    if (eb[u] == j) {
                        s = h;
                    } else {
                        for (int probe = 1; probe < DD_PROBES; ++probe) {
                            h = (h + 1) & (DD_TAB - 1);
                            int e = key[h];
                            if (e == -1) {
                                e = atomicCAS(&key[h], -1, j);
                                if (e == -1) e = j;
                            }
                            if (e == j) { s = h; break; }
                        }
                    }
                }
                dd_tile[kk * BLOB_P + t] = (u16)s;
            }
        }
    }
    __syncthreads();
    // number the occupied entries: DD_TAB / BLOB_T consecutive entries per thread
    constexpr int EPT = DD_TAB / BLOB_T;
    const int e0 = threadIdx.x * EPT;
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < EPT; ++q) cnt += key[e0 + q] != -1;
    const int incl = wave_scan_incl(cnt);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    int base = incl - cnt, total = 0;
#pragma unroll
    for (int w = 0; w < BLOB_T / 64; ++w) {
        const int tw = wave_tot[w];
        if (w < wv) base += tw;
        total += tw;
    }
    int* uq = uniq + (size_t)b * BLOB_S;
    int needs_ghost = 0;
#pragma unroll
    for (int q = 0; q < EPT; ++q) {
        const int j = key[e0 + q];
        if (j != -1) {
            slot_of[e0 + q] = (u16)(base < slots ? base : SLOT_OVER);
            if (base < slots) uq[base] = j;
            ++base;
            if (bclass && omap[j] >= n_active) needs_ghost = 1;
        }
    }
    for (int q = (total < slots ? total : slots) + threadIdx.x; q < BLOB_S; q += BLOB_T) uq[q] = -1;
    __syncthreads();
    // entry -> slot, then out in 16-B pieces of whole rows
    const int pieces = k * (BLOB_P / 8);
    for (int q = threadIdx.x; q < pieces; q += BLOB_T) {
        u16* src = dd_tile + q * 8;
        const int kk = q / (BLOB_P / 8), c = q % (BLOB_P / 8);
        unsigned v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const unsigned e = src[u];
            v[u] = e < DD_TAB ? (unsigned)slot_of[e] : e;
            if (v[u] == SLOT_OVER) needs_ghost = 1;      // (an unstaged neighbour is not looked up here: taken as foreign)
        }
        if ((size_t)b * BLOB_P + c * 8 < (size_t)npad)
            *reinterpret_cast<uint4*>(slot16 + (size_t)kk * npad + (size_t)b * BLOB_P + c * 8) =
                make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
    }
    if (bclass) {                                          // (uniform: a kernel argument)
        const int owned_q = (half == 0 && p < n && omap[qorder[p]] < n_active) ? 1 : 0;
        const int any_owned = __syncthreads_or(owned_q);
        const int any_ghost = __syncthreads_or(needs_ghost);
        if (threadIdx.x == 0) bclass[b] = (unsigned char)(!any_owned ? 2 : (any_ghost ? 1 : 0));
    }
}

// interior blobs, then boundary blobs, each in blob order: list[0 .. cnt[0]) and list[cnt[0] .. cnt[0] + cnt[1]).
// One workgroup (a few thousand blobs per 10^6 particles); each thread takes a run of consecutive blobs.
#define SPLIT_T 1024
__global__ __launch_bounds__(SPLIT_T) void blob_split_kernel(int nblk, const unsigned char* __restrict__ bclass, int* list,
                                                             int* cnt) {
    __shared__ int wsum[2][SPLIT_T / 64];
    const int per = (nblk + SPLIT_T - 1) / SPLIT_T;
    const int b0 = threadIdx.x * per, b1 = (b0 + per < nblk) ? b0 + per : nblk;
    int c0 = 0, c1 = 0;
    for (int b = b0; b < b1; ++b) { const int c = bclass[b]; c0 += c == 0; c1 += c == 1; }
    const int i0 = wave_scan_incl(c0), i1 = wave_scan_incl(c1);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 63) { wsum[0][wv] = i0; wsum[1][wv] = i1; }
    __syncthreads();
    int o0 = i0 - c0, o1 = i1 - c1, t0 = 0, t1 = 0;
    for (int w = 0; w < SPLIT_T / 64; ++w) {
        if (w < wv) { o0 += wsum[0][w]; o1 += wsum[1][w]; }
        t0 += wsum[0][w]; t1 += wsum[1][w];
    }
    for (int b = b0; b < b1; ++b) {
        const int c = bclass[b];
        if (c == 0) list[o0++] = b;
        else if (c == 1) list[t0 + o1++] = b;
    }
    if (threadIdx.x == 0) { cnt[0] = t0; cnt[1] = t1; cnt[2] = nblk - t0 - t1; }
}

int sphx_blob_translate(sphx_ctx* ctx, int64_t n, int k) {
    const int64_t npad = sphx_pad64(n);
    const int nblk = (int)((npad + BLOB_P - 1) / BLOB_P);
    SPHX_TRY(sphx_ensure(ctx, ctx->slot16, (size_t)k * npad * sizeof(u16) + 512));   // tiles are read in whole rows
    SPHX_TRY(sphx_ensure(ctx, ctx->uniq, (size_t)nblk * BLOB_S * sizeof(int)));
    int slots = ctx->blob_slots;
    if (slots < 1) slots = 1;
    if (slots > BLOB_S) slots = BLOB_S;
    // decomposed runs (device API): blobs sorted into interior / boundary, so that the interior ones can run under a halo phase
    const bool split = ctx->map_perm != nullptr && ctx->blob_split_on;
    unsigned char* bclass = nullptr;
    ctx->blob_split_valid = false;
    if (split) {
        SPHX_TRY(sphx_ensure(ctx, ctx->blob_class, (size_t)nblk));
        SPHX_TRY(sphx_ensure(ctx, ctx->blob_split, ((size_t)nblk + 4) * sizeof(int)));
        bclass = ctx->blob_class.as<unsigned char>();
    }
    hipLaunchKernelGGL(blob_dedup_kernel, dim3(nblk), dim3(BLOB_T), (size_t)k * BLOB_P * sizeof(u16), ctx->stream, (int)n, (int)npad, k, slots,
                       ctx->nbr.as<int>(), ctx->slot16.as<u16>(), ctx->uniq.as<int>(), ctx->qorder, ctx->map_perm,
                       ctx->map_nactive, bclass);
    if (split) {
        int* list = ctx->blob_split.as<int>();
        hipLaunchKernelGGL(blob_split_kernel, dim3(1), dim3(SPLIT_T), 0, ctx->stream, nblk, bclass, list, list + (size_t)nblk);
        ctx->blob_split_valid = true;
        ctx->blob_split_nblk = nblk;
    }
    HIPCHK(hipGetLastError());
    ctx->blob_lists = true;
    return SPHX_OK;
}

// ---- the four sum passes of hydro_update: what each stages, loads, computes per pair and writes.  How a pass walks
// its blobs and slot lists is blob_pass (sphx_blob.h). ---------------------------------------------------------------

// ---- pass 1: rho, rho_dust, n, grad P        nsc:588-619 --------------------------------------
struct DensityPass {
    typedef RecA Rec;
    typedef DensAcc Sums;
    static constexpr int NSIDE = 0, PER_SLOT = 64;
    static constexpr bool CLIPS = true, VOTES = false, ROW_FROM_LIST = true;
    const RecA* __restrict__ rec;
    double *rho_s, *rho, *rhod, *nden, *G, *ha;
    struct Row { double xr, yr, zr, hi2, ci, Ai; };
    typedef Q8 Nb;                                          // x y z h2 | c1 ms A Nw
    __device__ __forceinline__ BlobSides sides() const { return {}; }
    __device__ __forceinline__ Row load_row(int i) const {
        const Q8 s = gload8(&rec[i]);
        return Row{s.lo.a, s.lo.b, s.lo.c, s.lo.d, -6.0 * s.hi.a, s.hi.c};
    }
    __device__ __forceinline__ static void load_out(Row&, int, bool) {}
    __device__ __forceinline__ static void row_point(Row& r, const Nb& f) { r.xr = f.lo.a; r.yr = f.lo.b; r.zr = f.lo.c; }
    __device__ __forceinline__ static bool wanted(const Row&) { return true; }
    __device__ __forceinline__ Nb staged(const double2* img, const double*, int s, const int*) const {
        return lload8(img, s);
    }
    __device__ __forceinline__ Nb global(int j) const { return gload8(&rec[j]); }
    __device__ __forceinline__ static Nb none(const Row& r) { return Nb{Q4{r.xr, r.yr, r.zr, 0.0}, Q4{0.0, 0.0, 0.0, 0.0}}; }
    // returns the species weight Nw_j W_ij (nsc:626), for the kernel that goes on to the composition sweeps
    template <bool CLIP>
    __device__ __forceinline__ double term(Sums& a, const Nb& f, const Row& r) const {
        return density_term<SqrtMid>(a, f.lo, f.hi, r.xr, r.yr, r.zr, r.hi2, r.ci, r.Ai, CLIP);
    }
    __device__ __forceinline__ u64 finish(const Sums& a, double, const Row&, int i, int o) const {
        rho[o] = a.rho; rhod[o] = a.rd; nden[o] = a.n;
        rho_s[i] = a.rho;                                     // storage order: staged by pass 2
        if (G) { G[3 * (size_t)o + 0] = -a.gx; G[3 * (size_t)o + 1] = -a.gy; G[3 * (size_t)o + 2] = -a.gz; }
        ha[3 * (size_t)o + 0] = -a.gx / a.rho;                // nsc:619
        ha[3 * (size_t)o + 1] = -a.gy / a.rho;
        ha[3 * (size_t)o + 2] = -a.gz / a.rho;
        return SPHX_CT_NONE;
    }
};
BLOB_KERNEL blob_density_kernel(BLOB_COMMON, int clip, const int* __restrict__ omap, int n_active,
                                const RecA* __restrict__ rec, double* rho_s, double* rho, double* rhod, double* nden,
                                double* G, double* ha, BlobSel sel) {
    blob_pass(DensityPass{rec, rho_s, rho, rhod, nden, G, ha}, n, npad, k, nblk, nbr, slot16, uniq, qorder, clip, omap,
              n_active, nullptr, sel);
}

// what pass 3 writes for a settled row (sphx_settled.h): by ViscPass::settle, or by pass 2 where it hands its rows on
__device__ __forceinline__ void visc_settle_store(double* va, double* vh, int o) {
    const double q = __builtin_nan("");
    va[3 * (size_t)o + 0] = q; va[3 * (size_t)o + 1] = q; va[3 * (size_t)o + 2] = q;
    vh[o] = q;
}

// ---- pass 2: Pi_i, crossing time             nsc:639-649, nsc:776-786 --------------------------
// Handing on (marks != nullptr; the fused single-GPU step): m Pi_i, which pass 3's vote on "settled" turns on, is in a
// register at finish.  A settled row gets pass 3's NaNs here; a blob that holds a row that is not is marked, and pass 3
// walks the marked blobs alone (blob_visc_kernel).  Where the step's update takes its rows by class (row_settled != nullptr;
// sphx_update_rows.h) the row's class goes out as one byte in place of the four NaNs - for every row that writes, in
// every launch, so that nothing has to be reset: the update of a settled row reads none of pass 3's outputs.
struct PiPass {
    typedef RecB Rec;
    struct Sums { double pi; };
    static constexpr int NSIDE = 1, PER_SLOT = 72;          // side value: rho_j
    static constexpr bool CLIPS = false, VOTES = true, ROW_FROM_LIST = true;
    static constexpr bool SATURATES = BLOB_PI_SATURATES != 0;
    static constexpr bool HANDS_ON = true;
    const RecB* __restrict__ rec;
    const double* __restrict__ rho_s;
    const RecSelf* __restrict__ selfr;
    RecBC* bc;
    double *Pi, *BwOut;
    double *va, *vh;                                        // pass 3's outputs and, per blob, whether it has rows left to sum
    unsigned char* marks;                                   // (nullptr: nothing is handed on)
    unsigned char* row_settled;                             // (nullptr: the settled rows get their NaNs)
    __device__ __forceinline__ bool hands_on() const { return marks != nullptr; }
    __device__ __forceinline__ void hand_on(int b, bool any_live) const { marks[b] = any_live ? 1 : 0; }
    struct Row { Q4 r0, rv; double rho_i, cs_i, ms_i, h_i; };
    struct Nb { Q8 q; double rho; };
    __device__ __forceinline__ BlobSides sides() const { return {rho_s, 1}; }
    __device__ __forceinline__ Row load_row(int i) const {
        const RecSelf sf = selfr[i];
        const Q8 s = gload8(&rec[i]);
        return Row{s.lo, s.hi, rho_s[i], sf.csi, sf.mg, sf.h};
    }
    __device__ __forceinline__ static void load_out(Row&, int, bool) {}
    __device__ __forceinline__ static void row_point(Row& r, const Nb& f) { r.r0 = f.q.lo; r.rv = f.q.hi; }
    __device__ __forceinline__ static bool wanted(const Row&) { return true; }
    __device__ __forceinline__ Nb staged(const double2* img, const double* side, int s, const int*) const {
        return Nb{lload8(img, s), side[s]};
    }
    __device__ __forceinline__ Nb global(int j) const { return Nb{gload8(&rec[j]), rho_s[j]}; }
    __device__ __forceinline__ static Nb none(const Row& r) { return Nb{Q8{r.r0, r.rv}, r.rho_i}; }
    template <bool CLIP>
    __device__ __forceinline__ double term(Sums& a, const Nb& f, const Row& r) const {
        const PiPair t = pi_term<SqrtMid>(f.q.lo, f.q.hi, f.rho, r.r0, r.rv, r.rho_i, r.cs_i);
        a.pi += t.pi;
        return t.rel;
    }
    // a NaN partial sum stays NaN: from then on only the neighbour's velocity chunks {vx vy | vz cs} are read, for the vote
    typedef Q4 Vel;
    __device__ __forceinline__ static bool saturated(const Sums& a) { return sphx_is_nan(a.pi); }
    __device__ __forceinline__ static Vel short_staged(const double2* img, int s) { return lload4(img, s, 1); }
    __device__ __forceinline__ Vel short_global(int j) const { return gload4(reinterpret_cast<const double*>(&rec[j]) + 4); }
    __device__ __forceinline__ static Vel short_none(const Row& r) { return r.rv; }
    __device__ __forceinline__ static double term_short(const Vel& qv, const Row& r) { return pi_rel(qv, r.rv); }
    __device__ __forceinline__ u64 finish(const Sums& a, double maxrel, const Row& r, int i, int o, bool has_first,
                                          bool& live) const {
        Pi[o] = a.pi;
        const double bw = fmax(r.ms_i, 0.0) * a.pi;                         // m Pi [t==0]  nsc:651
        bc[i].Bw = bw;
        if (BwOut) BwOut[o] = bw;
        if (marks) {                                                        // (uniform: an argument; the row writes)
            live = !sphx_row_settled(bw, has_first, true);
            if (row_settled) row_settled[o] = live ? 0 : 1;                 // (uniform as well)
            else if (!live) visc_settle_store(va, vh, o);
        }
        return (r.ms_i > 0.0) ? ct_vote_bits(r.h_i, maxrel) : SPHX_CT_NONE; // gas only     nsc:782
    }
};
BLOB_KERNEL blob_pi_kernel(BLOB_COMMON, const int* __restrict__ omap, int n_active, const RecB* __restrict__ recb,
                           const double* __restrict__ rho_s, const RecSelf* __restrict__ selfr, RecBC* bc, double* Pi,
                           double* BwOut, u64* ct_bits, BlobSel sel, u64* counts, double* va, double* vh,
                           unsigned char* marks, unsigned char* row_settled) {
    blob_pass(PiPass{recb, rho_s, selfr, bc, Pi, BwOut, va, vh, marks, row_settled}, n, npad, k, nblk, nbr, slot16, uniq, qorder, 0, omap,
              n_active, ct_bits, sel, counts);
}

// ---- pass 3: viscous acceleration + heat      nsc:651-654 --------------------------------------
struct ViscPass {
    typedef RecB Rec;
    typedef ViscAcc Sums;
    static constexpr int NSIDE = 2, PER_SLOT = 72;          // image {x y | z h2 | vx vy | vz Bw}, side value: c1
    static constexpr bool CLIPS = true, VOTES = false, ROW_FROM_LIST = true;
    static constexpr bool SETTLES = true;
    const RecB* __restrict__ rec;
    const RecBC* __restrict__ bc;
    const double* __restrict__ m;
    double *va, *vh;
    bool handed;                                             // pass 2 has written the settled rows (PiPass, handing on)
    struct Row { Q4 r0, rv; double hi2, ci, Bi, mi; };
    struct Nb { Q8 q; double c1; };                          // q.hi.d = Bw_j
    __device__ __forceinline__ BlobSides sides() const {
        const double* bcd = reinterpret_cast<const double*>(bc);
        return {bcd, 2, bcd + 1, 2};
    }
    __device__ __forceinline__ Row load_row(int i) const {
        const double2 bci = *reinterpret_cast<const double2*>(&bc[i]);      // Bw, c1
        const Q8 s = gload8(&rec[i]);
        return Row{s.lo, s.hi, s.lo.d, -6.0 * bci.y, bci.x, 0.0};
    }
    // m in output order
    __device__ __forceinline__ void load_out(Row& r, int o, bool on) const { r.mi = on ? m[o] : 0.0; }
    __device__ __forceinline__ static void row_point(Row& r, const Nb& f) { r.r0 = f.q.lo; r.rv = f.q.hi; }
    __device__ __forceinline__ static bool wanted(const Row&) { return true; }
    __device__ __forceinline__ Nb staged(const double2* img, const double* side, int s, const int*) const {
        return Nb{lload8(img, s), side[s]};
    }
    __device__ __forceinline__ Nb global(int j) const {
        Nb f{gload8(&rec[j]), 0.0};
        const double2 tt = *reinterpret_cast<const double2*>(&bc[j]);
        f.q.hi.d = tt.x; f.c1 = tt.y;
        return f;
    }
    __device__ __forceinline__ static Nb none(const Row& r) { return Nb{Q8{r.r0, r.rv}, 0.0}; }
    template <bool CLIP>
    __device__ __forceinline__ double term(Sums& a, const Nb& f, const Row& r) const {
        visc_term<SqrtMid>(a, f.q.lo, f.q.hi, f.q.hi.d, f.c1, r.r0, r.rv, r.hi2, r.ci, r.Bi, CLIP);
        return 0.0;
    }
    __device__ __forceinline__ u64 finish(const Sums& a, double, const Row& r, int, int o) const {
        va[3 * (size_t)o + 0] = -a.x; va[3 * (size_t)o + 1] = -a.y; va[3 * (size_t)o + 2] = -a.z;
        vh[o] = a.h * r.mi / 2.0;                                           // nsc:654
        return SPHX_CT_NONE;
    }
    // every term holds Bw_i c_a: with a NaN Bw_i (Pi_i NaN: PiPass::finish, dust rows too) the four sums are NaN
    __device__ __forceinline__ double own(int i) const { return bc[i].Bw; }
    __device__ __forceinline__ void settle(int o) const {
        if (!handed) visc_settle_store(va, vh, o);
    }
};
// The blobs of a launch of pass 3 that pass 2 has marked (one byte per blob: it holds a row that is not settled; the rows
// that are, pass 2 has written), dealt out over the workgroups without a global list, an atomic or anything to reset:
// every workgroup counts the marks (16 per thread and round, VISC_ROUND blobs per round), then numbers the marked blobs
// in blob order - one prefix sum over the workgroup per round - and keeps in blob_own_list() those that fall to it.
// Number r of `total` goes where blob r of as many goes (xcd_block: neighbouring blobs on one XCD).  Returns
//   VISC_NONE   nothing is marked: nothing to stage, walk or write
//   -1          every blob is marked: the walk as without marks (a healthy state pays the count alone)
//   own_n >= 0  entries of blob_own_list() to walk (at most BLOB_OWN_MAX: sphx_blob_can_hand_visc)
// and the number of marked blobs in `total`.  Every thread of the workgroup calls (barriers inside); the results are
// uniform over the grid: every workgroup reads the same marks.
#define VISC_NONE (-2)
#define VISC_ROUND (16 * PASS_T)
__device__ __forceinline__ int visc_own_blobs(const unsigned char* __restrict__ marks, int nblk, int& total) {
    __shared__ int wave_tot[PASS_T / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    auto marked = [&](int b0, unsigned (&w)[4]) -> int {         // this thread's 16 marks from blob b0 on, and how many are set
        w[0] = w[1] = w[2] = w[3] = 0u;
        if (b0 >= nblk) return 0;
        const uint4 mk = *reinterpret_cast<const uint4*>(marks + b0);              // (the buffer ends on a whole piece)
        w[0] = mk.x; w[1] = mk.y; w[2] = mk.z; w[3] = mk.w;
        int cnt = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (b0 + q >= nblk) w[q >> 2] &= ~(0xFFu << (8 * (q & 3)));             // (beyond the last blob: not written)
            cnt += ((w[q >> 2] >> (8 * (q & 3))) & 0xFFu) ? 1 : 0;
        }
        return cnt;
    };
    unsigned w[4];
    int mine = 0;
    for (int base = 0; base < nblk; base += VISC_ROUND) mine += marked(base + 16 * (int)threadIdx.x, w);
    mine = wave_scan_incl(mine);
    if (lane == 63) wave_tot[wv] = mine;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int q = 0; q < PASS_T / 64; ++q) total += wave_tot[q];
    if (total == 0) return VISC_NONE;
    if (total == nblk) return -1;
    int before = 0;                                              // marked blobs in the rounds before this one
    for (int base = 0; base < nblk; base += VISC_ROUND) {
        __syncthreads();                                         // (wave_tot is read above, and in the round before)
        const int b0 = base + 16 * (int)threadIdx.x;
        const int cnt = marked(b0, w);
        const int incl = wave_scan_incl(cnt);
        if (lane == 63) wave_tot[wv] = incl;
        __syncthreads();
        int r = before + incl - cnt;                             // the number of this thread's first marked blob
#pragma unroll
        for (int q = 0; q < PASS_T / 64; ++q) {
            const int tw = wave_tot[q];
            if (q < wv) r += tw;
            before += tw;
        }
        if (cnt) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                if ((w[q >> 2] >> (8 * (q & 3))) & 0xFFu) {
                    const int bi = xcd_block_inv(r, total);      // the workgroup-strided index that lands on number r
                    if (bi % (int)gridDim.x == (int)blockIdx.x) blob_own_list()[bi / (int)gridDim.x] = b0 + q;
                    ++r;
                }
            }
        }
    }
    __syncthreads();
    return ((int)blockIdx.x < total) ? (total - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
}

// marks (nullptr: every blob of `sel`, as without): the fused step's hand-over from pass 2 (PiPass) - the launch walks
// the marked blobs alone, counts the others as settled, and `settle` stores nothing.
BLOB_KERNEL blob_visc_kernel(BLOB_COMMON, int clip, const int* __restrict__ omap, int n_active,
                             const RecB* __restrict__ recb, const RecBC* __restrict__ bc, const double* __restrict__ m,
                             double* va, double* vh, BlobSel sel, u64* counts,
                             const unsigned char* __restrict__ marks) {
    int own_n = -1;
    if (marks) {
        int total;
        own_n = visc_own_blobs(marks, nblk, total);
        if (counts && blockIdx.x == 0 && threadIdx.x == 0) {
            atomicAdd(counts + BLOB_CNT_BLOBS_SETTLED, (u64)(nblk - total));
            if (own_n == VISC_NONE) atomicAdd(counts + BLOB_CNT_LAUNCHES_SKIPPED, (u64)1);
        }
        if (own_n == VISC_NONE) return;                          // (uniform over the grid)
    }
    blob_pass(ViscPass{recb, bc, m, va, vh, marks != nullptr}, n, npad, k, nblk, nbr, slot16, uniq, qorder, clip, omap, n_active,
              nullptr, sel, counts, own_n);
}

// ---- passes 2 + 3 fused: the pairwise viscosity (visc_mode 1; sphx_sums.hip pass_visc_pw_kernel) ------------------
// LDS image: RecB {x y | z h2 | vx vy | vz cs} + rho_j, 72 B per slot as pass 2's (79 360 B at K = 40: two workgroups per
// CU).  M_j = m_j [t_j==0] c1_j (RecBC[j].Bw) stays out of it and is fetched by an 8-B gather through the int32 list (the
// list entry a coalesced load, the record a dependent one).  Staging M_j as well - 80 B per slot, 87 040 B, one workgroup
// per CU - measured slower: 0.345 against 0.306 ms at 10^6.
struct ViscPwPass {
    typedef RecB Rec;
    typedef ViscAcc Sums;
    static constexpr int NSIDE = 1, PER_SLOT = 72;          // side value: rho_j
    static constexpr bool CLIPS = true, VOTES = true, ROW_FROM_LIST = true;
    const RecB* __restrict__ rec;
    const double* __restrict__ rho_s;
    const RecBC* __restrict__ bc;
    const RecSelf* __restrict__ selfr;
    const double* __restrict__ m;
    double *va, *vh;
    struct Row { Q4 r0, rv; double rho_i, cs_i, h_i, mg, hi2, ci, mi; };
    struct Nb { Q8 q; double rho, mc; };
    __device__ __forceinline__ BlobSides sides() const { return {rho_s, 1}; }
    __device__ __forceinline__ Row load_row(int i) const {
        const RecSelf sf = selfr[i];
        const double rho_i = rho_s[i], mci = bc[i].Bw;
        const Q8 s = gload8(&rec[i]);
        return Row{s.lo, s.hi, rho_i, sf.csi, sf.h, sf.mg, s.lo.d, -6.0 * mci, 0.0};
    }
    // m in output order
    __device__ __forceinline__ void load_out(Row& r, int o, bool on) const { r.mi = on ? m[o] : 0.0; }
    __device__ __forceinline__ static void row_point(Row& r, const Nb& f) { r.r0 = f.q.lo; r.rv = f.q.hi; }
    __device__ __forceinline__ static bool wanted(const Row&) { return true; }
    __device__ __forceinline__ Nb staged(const double2* img, const double* side, int s, const int* jp) const {
        return Nb{lload8(img, s), side[s], bc[*jp].Bw};
    }
    __device__ __forceinline__ Nb global(int j) const { return Nb{gload8(&rec[j]), rho_s[j], bc[j].Bw}; }
    __device__ __forceinline__ static Nb none(const Row& r) { return Nb{Q8{r.r0, r.rv}, r.rho_i, 0.0}; }
    template <bool CLIP>
    __device__ __forceinline__ double term(Sums& a, const Nb& f, const Row& r) const {
        return visc_pw_term<SqrtMid>(a, f.q.lo, f.q.hi, f.rho, f.mc, r.r0, r.rv, r.rho_i, r.cs_i, r.hi2, r.ci, CLIP);
    }
    __device__ __forceinline__ u64 finish(const Sums& a, double maxrel, const Row& r, int, int o) const {
        va[3 * (size_t)o + 0] = -a.x; va[3 * (size_t)o + 1] = -a.y; va[3 * (size_t)o + 2] = -a.z;
        vh[o] = a.h * r.mi / 2.0;                                           // nsc:654
        return (r.mg > 0.0) ? ct_vote_bits(r.h_i, maxrel) : SPHX_CT_NONE;   // gas only     nsc:782
    }
};
BLOB_KERNEL blob_visc_pw_kernel(BLOB_COMMON, int clip, const int* __restrict__ omap, int n_active,
                                const RecB* __restrict__ recb, const double* __restrict__ rho_s,
                                const RecBC* __restrict__ bc, const RecSelf* __restrict__ selfr,
                                const double* __restrict__ m, double* va, double* vh, u64* ct_bits, BlobSel sel) {
    blob_pass(ViscPwPass{recb, rho_s, bc, selfr, m, va, vh}, n, npad, k, nblk, nbr, slot16, uniq, qorder, clip, omap, n_active,
              ct_bits, sel);
}

// ---- sweeps (2), (3) of the species pass (blob_species_kernel) and its epilogue -------------------------------------
// w: the weights Nw_j W_ij of this lane's list positions, in registers (every index a compile-time constant).  The image
// is refilled with the lower, then the upper 64 bytes of the distinct neighbours' composition rows; the lane accumulates
// weight x row, the group's totals are F[s, i]; then Z_i (drv:663) and the AGB yields at (Z_i, m_i).  Every thread of the
// workgroup calls (barriers inside); the caller synchronises before the image is written again.
template <int SPEC_MAXM>
__device__ __forceinline__ void species_sweeps(const double (&w)[SPEC_MAXM], double2* img, const u16* tile,
                                               const int* __restrict__ uq, const int* __restrict__ nbr, int n, int npad,
                                               int nm, int p, int i, int t, int half, bool live, int S,
                                               const double* __restrict__ fun, const int* __restrict__ row_of,
                                               const double* __restrict__ m, const AgbTable& agb, int agb_on, double* F,
                                               double* Zout, double* agb_out) {
    double tot[16];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        __syncthreads();                                   // everybody is done with the previous image
        // this half of the distinct neighbours' composition rows into the image
        {
            int ju[NSTAGE];
#pragma unroll
            for (int r = 0; r < NSTAGE; ++r) {
                const int s = threadIdx.x + r * PASS_T;
                ju[r] = (s < BLOB_S) ? uq[s] : -1;
            }
            double2 c[NSTAGE][4];
#pragma unroll
            for (int r = 0; r < NSTAGE; ++r) {
                const int jr = ju[r] < 0 ? 0 : ju[r];
                const double2* g = reinterpret_cast<const double2*>(fun + (size_t)(row_of ? row_of[jr] : jr) * 16) + 4 * hh;
                c[r][0] = g[0]; c[r][1] = g[1]; c[r][2] = g[2]; c[r][3] = g[3];
            }
#pragma unroll
            for (int r = 0; r < NSTAGE; ++r) {
                const int s = threadIdx.x + r * PASS_T;
                if (ju[r] >= 0) {
                    img[0 * BLOB_S + s] = c[r][0]; img[1 * BLOB_S + s] = c[r][1];
                    img[2 * BLOB_S + s] = c[r][2]; img[3 * BLOB_S + s] = c[r][3];
                }
            }
        }
        __syncthreads();
        double acc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = 0.0;
#pragma unroll
        for (int mm = 0; mm < SPEC_MAXM; ++mm) {
            if (mm < nm) {
                const unsigned sl = tile[(LPP * mm + half) * BLOB_P + t];
                if (sl != SLOT_NONE && live) {
                    Q4 f0, f1;
                    if (sl < SLOT_OVER) { f0 = lload4(img, (int)sl, 0); f1 = lload4(img, (int)sl, 1); }
                    else {
                        const int jo = nbr[(size_t)(LPP * mm + half) * npad + p];
                        const double* q = fun + (size_t)(row_of ? row_of[jo] : jo) * 16 + 8 * hh;
                        f0 = gload4(q); f1 = gload4(q + 4);
                    }
                    const double wm = w[mm];
                    acc[0] += wm * f0.a; acc[1] += wm * f0.b; acc[2] += wm * f0.c; acc[3] += wm * f0.d;
                    acc[4] += wm * f1.a; acc[5] += wm * f1.b; acc[6] += wm * f1.c; acc[7] += wm * f1.d;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) tot[8 * hh + q] = group_total(acc[q]);
    }
    if (live && !half) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (q < S) F[(size_t)q * n + i] = tot[q];
    }
    if (live && agb_on) {
        // every lane of the group holds the totals: the metallicity in all four, the splines dealt over them
        const double Z = species_metallicity(agb, tot, S);
        if (!half) Zout[i] = Z;
        const double Mi = m[i];
        double* row = agb_out + (size_t)i * S;
        for (int q = half; q < S; q += LPP)
            if (!((agb.covered >> q) & 1u)) row[q] = 0.0;  // species no spline writes
        for (int o = half; o < agb.nspl; o += LPP) {
            double val;
            const int target = agb_one_spline(agb, o, Mi, Z, val);
            if (target >= 0) row[target] = val;
        }
    }
}

// ---- pass 1 + species pass in one kernel (the step loop with a composition, hydro_update's sums) -----------------------
// The species pass's first sweep repeats pass 1's staging and its W_ij: here pass 1 keeps every lane's weights Nw_j W_ij
// in registers and the two composition sweeps of blob_species_kernel follow on the same slot lists - one staging and one
// set of kernel evaluations fewer per blob (with-species step 1.65 -> see DESIGN 6.1).  Same expressions in the same
// order as the two kernels run one after the other: bit-identical outputs.
template <int SPEC_MAXM>
__global__ __launch_bounds__(PASS_T, PASS_MINW) void blob_density_species_kernel(int n, int npad, int k, int nblk,
        const int* __restrict__ nbr, const u16* __restrict__ slot16, const int* __restrict__ uniq,
        const int* __restrict__ qorder, int clip, const RecA* __restrict__ rec, double* rho_s, double* rho, double* rhod,
        double* nden, double* G, double* ha,
        int S, const double* __restrict__ fun, const int* __restrict__ row_of, const double* __restrict__ m, AgbTable agb,
        int agb_on, double* F, double* Zout, double* agb_out) {
    const DensityPass ps{rec, rho_s, rho, rhod, nden, G, ha};      // pass 1 itself: its row, batches and epilogue
    double2* img = BlobLds<0>::img();
    u16* tile = BlobLds<0>::tile();
    const int t = threadIdx.x / LPP, half = threadIdx.x & (LPP - 1);
    const int nm = KPAD(k) / LPP;
    for (int bi = blockIdx.x; bi < nblk; bi += gridDim.x) {
        const int b = xcd_block(bi, nblk);
        const int p = b * BLOB_P + t;
        const bool live = p < n;
        const int i = live ? qorder[p] : 0;
        const int* uq = uniq + (size_t)b * BLOB_S;
        stage<0>(img, nullptr, tile, rec, nullptr, 0, nullptr, 0, uq, slot16, npad, k, b);
        DensityPass::Row row = ps.load_row(i);
        __syncthreads();
        double w[SPEC_MAXM];
#pragma unroll
        for (int mm = 0; mm < SPEC_MAXM; ++mm) w[mm] = 0.0;
        if (live) {
            blob_row_point(ps, row, nbr, p, t);
            DensAcc a{};
            // (unrolled at compile time, unlike blob_pass's loop: the weights' register indices must be constants)
#pragma unroll
            for (int m0 = 0; m0 < SPEC_MAXM; m0 += NB) {
                if (m0 < nm) {
                    unsigned cur[NB];
                    load_slots(cur, tile, m0, half, t);
                    double wo[NB];
                    blob_batch_any(ps, clip, a, wo, cur, nbr + ((size_t)(LPP * m0 + half) * npad + p),
                                   LPP * (size_t)npad, row);
#pragma unroll
                    for (int u = 0; u < NB; ++u) if (m0 + u < SPEC_MAXM) w[m0 + u] = wo[u];
                }
            }
            group_total_fields(a);
            if (!half) ps.finish(a, 0.0, row, i, i);
        }
        // ---- the composition sweeps of the species pass, on the weights in hand
        species_sweeps(w, img, tile, uq, nbr, n, npad, nm, p, i, t, half, live, S, fun, row_of, m, agb, agb_on, F, Zout, agb_out);
        __syncthreads();                                       // the image is rewritten by the next blob
    }
}


// ---- species pass (nsc:624-627) out of LDS, + metallicity and AGB yields ---------------------------
// F[s,i] = sum_k Nw_j W_ij f_un[j,s] needs, per neighbour, the 64-B record (for W) AND the 128-B composition row: 184 KB
// for a blob's 960 slots, more than a CU has.  So the blob is walked three times over the same slot lists: (1) the
// records are staged and every lane turns its list positions into weights Nw_j W_ij kept in REGISTERS (K/4 doubles);
// (2), (3) the image is refilled with the lower / upper 64 bytes of the distinct neighbours' composition rows and the
// lane accumulates weight x row.  Each distinct row is fetched once per blob (~5 per particle) instead of once per
// reference (40 per particle: the gather form, sphx_sums.hip, bound by exactly that: 1.77 ms at 1e6 particles).
// Sums: the lane's positions k = q mod 4 in ascending k, then (p0 + p1) + (p2 + p3) as in the other LDS passes.
// SPEC_MAXM: list positions per lane the registers are sized for (K <= 40: 10; else 16)
template <int SPEC_MAXM>
__global__ __launch_bounds__(PASS_T, PASS_MINW) void blob_species_kernel(int n, int npad, int k, int nblk,
                                                              const int* __restrict__ nbr,
                                                              const u16* __restrict__ slot16,
                                                              const int* __restrict__ uniq,
                                                              const int* __restrict__ qorder, int S,
                                                              const RecA* __restrict__ rec,
                                                              const double* __restrict__ fun,       // rows of 16 doubles
                                                              const int* __restrict__ row_of,       // (nullable) row of particle j
                                                              const double* __restrict__ m, AgbTable agb, int agb_on,
                                                              double* F, double* Zout, double* agb_out) {
    extern __shared__ double2 img[];                       // 4 * BLOB_S chunks, then the slot tile
    u16* tile = reinterpret_cast<u16*>(img + 4 * BLOB_S);
    const int t = threadIdx.x / LPP, half = threadIdx.x & (LPP - 1);
    const int nm = KPAD(k) / LPP;
    for (int bi = blockIdx.x; bi < nblk; bi += gridDim.x) {
        const int b = xcd_block(bi, nblk);
        const int p = b * BLOB_P + t;
        const bool live = p < n;
        const int i = live ? qorder[p] : 0;
        const int* uq = uniq + (size_t)b * BLOB_S;
        stage<0>(img, nullptr, tile, rec, nullptr, 0, nullptr, 0, uq, slot16, npad, k, b);
        __syncthreads();
        // ---- (1) weights of this lane's list positions
        double w[SPEC_MAXM];
        {
            double xr, yr, zr;
            {
                const int j0 = live ? nbr[p] : 0;                   // deltas are relative to the first neighbour (nsc:580-581)
                const unsigned sl0 = tile[t];
                if (sl0 < SLOT_OVER) { const Q4 r = lload4(img, (int)sl0, 0); xr = r.a; yr = r.b; zr = r.c; }
                else { const int jj = j0 < 0 ? i : j0; xr = rec[jj].x; yr = rec[jj].y; zr = rec[jj].z; }
            }
#pragma unroll
            for (int mm = 0; mm < SPEC_MAXM; ++mm) {
                w[mm] = 0.0;
                if (mm < nm) {
                    const unsigned sl = tile[(LPP * mm + half) * BLOB_P + t];
                    if (sl != SLOT_NONE && live) {
                        Q4 q0, q1;
                        if (sl < SLOT_OVER) { q0 = lload4(img, (int)sl, 0); q1 = lload4(img, (int)sl, 1); }
                        else {
                            const double* q = reinterpret_cast<const double*>(&rec[nbr[(size_t)(LPP * mm + half) * npad + p]]);
                            q0 = gload4(q); q1 = gload4(q + 4);
                        }
                        w[mm] = species_weight<SqrtMid>(q0, q1.a, q1.d, xr, yr, zr);
                    }
                }
            }
        }
        // ---- (2), (3)
        species_sweeps(w, img, tile, uq, nbr, n, npad, nm, p, i, t, half, live, S, fun, row_of, m, agb, agb_on, F, Zout, agb_out);
        __syncthreads();                                       // the image is rewritten by the next blob
    }
}

// ---- gas-dust drag out of LDS                 nsc:719-742 (net_impulse; gather form: sphx_sums.hip) ---------------------
// Only dust neighbours count (a tenth of the references in the two-phase cloud), and every one of them costs the
// gather form a chain of gathers (type, record, m, grain mass, cross-section) and an atomic with return for its place
// in the receiver's slice of the ordered scatter.  Here the blob's distinct neighbours carry a dust flag in LDS, the
// references to each are counted in LDS, and the blob reserves its share of a receiver's slice with ONE global atomic
// per distinct dust neighbour (ranks inside the share come from an LDS counter; the order within a slice is free: the
// reduction sorts by key).  FILL = false: the counting pass of the scatter plan (sphx_drag_scatter_plan).
#define DRAG_XLDS (BLOB_S * (2 * sizeof(int) + 1))          // count, base, dust flag per image slot
template <bool FILL>
__global__ __launch_bounds__(PASS_T, PASS_MINW) void blob_drag_kernel(int n, int npad, int k, int nblk,
                                                           const int* __restrict__ nbr,
                                                           const u16* __restrict__ slot16,
                                                           const int* __restrict__ uniq,
                                                           const int* __restrict__ qorder,
                                                           const RecB* __restrict__ recb,
                                                           const double* __restrict__ m,
                                                           const double* __restrict__ ptype,
                                                           const double* __restrict__ mgm,
                                                           const double* __restrict__ mcs,
                                                           const int* __restrict__ id, double* onto, DragScatter sc) {
    extern __shared__ double2 img[];                       // FILL: 4 * BLOB_S chunks; then the slot tile, counts, bases, flags
    u16* tile = reinterpret_cast<u16*>(img + (FILL ? 4 * BLOB_S : 0));
    int* cntL = reinterpret_cast<int*>(tile + KPAD(k) * BLOB_P);
    int* baseL = cntL + BLOB_S;
    unsigned char* dust = reinterpret_cast<unsigned char*>(baseL + BLOB_S);
    const int t = threadIdx.x / LPP, part = threadIdx.x & (LPP - 1);
    const int nm = KPAD(k) / LPP;
    for (int bi = blockIdx.x; bi < nblk; bi += gridDim.x) {
        const int b = xcd_block(bi, nblk);
        const int p = b * BLOB_P + t;
        const bool live = p < n;
        const int i = live ? qorder[p] : 0;
        const int* uq = uniq + (size_t)b * BLOB_S;
        if (FILL) {
            stage<0>(img, nullptr, tile, recb, nullptr, 0, nullptr, 0, uq, slot16, npad, k, b);
        } else {
            const int pieces = KPAD(k) * (BLOB_P / 8);
            for (int q = threadIdx.x; q < pieces; q += PASS_T) {
                const int kk = q / (BLOB_P / 8), c = q % (BLOB_P / 8);
                uint4 v = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
                if (kk < k) v = *reinterpret_cast<const uint4*>(slot16 + (size_t)kk * npad + (size_t)b * BLOB_P + c * 8);
                *reinterpret_cast<uint4*>(tile + kk * BLOB_P + c * 8) = v;
            }
        }
        for (int s = threadIdx.x; s < BLOB_S; s += PASS_T) {
            const int j = uq[s];
            dust[s] = (j >= 0 && ptype[j] == 2.0) ? 1 : 0;                       // nsc:736
            cntL[s] = 0;
        }
        __syncthreads();
        // references per distinct dust neighbour (a particle's reference to itself casts no reaction: nsc:741)
        if (live) {
            for (int m0 = 0; m0 < nm; ++m0) {
                const int kk = LPP * m0 + part;
                const unsigned sl = tile[kk * BLOB_P + t];
                if (sl < SLOT_OVER) {
                    if (dust[sl] && uq[sl] != i) atomicAdd(&cntL[sl], 1);
                } else if (sl == SLOT_OVER && !FILL) {
                    const int j = nbr[(size_t)kk * npad + p];
                    if (j != i && ptype[j] == 2.0) atomicAdd(&sc.cnt[j], 1);
                }
            }
        }
        __syncthreads();
        if (!FILL) {
            for (int s = threadIdx.x; s < BLOB_S; s += PASS_T)
                if (cntL[s]) atomicAdd(&sc.cnt[uq[s]], cntL[s]);
            __syncthreads();
            continue;
        }
        // the blob's share of every receiver's slice (handed out from the slice's end, as the gather form does)
        for (int s = threadIdx.x; s < BLOB_S; s += PASS_T) {
            const int c = cntL[s];
            if (c) {
                const int j = uq[s];
                baseL[s] = sc.start[j] + atomicSub(&sc.cnt[j], c) - c;
                cntL[s] = 0;
            }
        }
        const double* rq = reinterpret_cast<const double*>(&recb[i]);
        const Q4 r0 = gload4(rq), rv = gload4(rq + 4);
        __syncthreads();
        double ox = 0.0, oy = 0.0, oz = 0.0;
        if (live) {
            // which of the lane's list positions name a dust neighbour: one in ten.  Walking all of them, nearly every step
            // finds SOME lane of the wave at a dust neighbour and the other sixty waiting for its gathers; walking only the
            // marked ones, the wave is through after as many steps as its busiest lane has dust neighbours (3-4, not 10)
            unsigned dm = 0;
            for (int m0 = 0; m0 < nm; ++m0) {
                const int kk = LPP * m0 + part;
                const unsigned sl = tile[kk * BLOB_P + t];
                bool d = false;
                if (sl < SLOT_OVER) d = dust[sl] != 0;
                else if (sl == SLOT_OVER) d = ptype[nbr[(size_t)kk * npad + p]] == 2.0;
                dm |= (d ? 1u : 0u) << m0;
            }
            while (dm) {                                   // (ascending list position: the order of the partial sum)
                const int m0 = __builtin_ctz(dm);
                dm &= dm - 1;
                const int kk = LPP * m0 + part;
                const unsigned sl = tile[kk * BLOB_P + t];
                int j;
                Q4 q0, qv;
                if (sl < SLOT_OVER) {
                    j = uq[sl];
                    q0 = lload4(img, (int)sl, 0); qv = lload4(img, (int)sl, 1);
                } else {
                    j = nbr[(size_t)kk * npad + p];
                    const double* qb = reinterpret_cast<const double*>(&recb[j]);
                    q0 = gload4(qb); qv = gload4(qb + 4);
                }
                const Vec3 f = drag_term(ox, oy, oz, q0, qv, r0, rv, j, m, mgm, mcs);
                if (j != i) {                                              // nsc:741
                    const int slot = (sl < SLOT_OVER) ? baseL[sl] + atomicAdd(&cntL[sl], 1)
                                                      : sc.start[j] + atomicSub(&sc.cnt[j], 1) - 1;
                    sphx_drag_put(sc, slot, ((u64)(unsigned)id[i] << 8) | (u64)kk, -f.x, -f.y, -f.z);
                }
            }
        }
        const double tx = group_total(ox), ty = group_total(oy), tz = group_total(oz);
        if (live && part == 0) { onto[3 * (size_t)i] = tx; onto[3 * (size_t)i + 1] = ty; onto[3 * (size_t)i + 2] = tz; }
        __syncthreads();
    }
}

// ---- launchers (buffers are sized by the callers in sphx_sums.hip) -----------------------------
BlobSel sphx_blob_sel(sphx_ctx* ctx, int part) {
    if (!ctx->blob_split_valid) return BlobSel{nullptr, nullptr, 0};
    const int* list = ctx->blob_split.as<int>();
    return BlobSel{list, list + (size_t)ctx->blob_split_nblk, part == 0 ? 3 : part};
}

// persistent grid: two workgroups per CU (what the LDS image allows), a multiple of the 8 XCDs
int sphx_blob_grid(sphx_ctx* ctx, int nblk) {
    if (ctx->blob_grid <= 0) {
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
        ctx->blob_grid = ((cus * 2 + 7) / 8) * 8;
    }
    return nblk < ctx->blob_grid ? nblk : ctx->blob_grid;
}

int sphx_lds_opt_in(sphx_ctx* ctx, const void* kernel, size_t bytes) {
    for (int q = 0; q < ctx->n_lds_raised; ++q)
        if (ctx->lds_raised[q] == kernel) return SPHX_OK;
    if (ctx->n_lds_raised == SPHX_LDS_KERNELS)
        return sphx_set_err(ctx, SPHX_E_HIP, "sphx_lds_opt_in: more than %d kernels", SPHX_LDS_KERNELS);
    HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    ctx->lds_raised[ctx->n_lds_raised++] = kernel;
    return SPHX_OK;
}

// callers' particles that are computed (device API: the owned ones; ghosts, o >= n_active, are candidates only)
static int blob_n_active(const sphx_ctx* ctx, int64_t n) { return ctx->map_perm ? ctx->map_nactive : (int)n; }

int sphx_blob_density(sphx_ctx* ctx, int64_t n, int k, bool lean) {
    return blob_launch(ctx, blob_density_kernel, DensityPass::PER_SLOT, 0, n, k, ctx->clip_grad, ctx->map_perm,
                       blob_n_active(ctx, n), ctx->rec1.as<RecA>(), ctx->rho_s.as<double>(), ctx->rho.as<double>(),
                       ctx->rhod.as<double>(), ctx->nden.as<double>(), lean ? nullptr : ctx->G.as<double>(), ctx->ha.as<double>(),
                       sphx_blob_sel(ctx, ctx->pass_part));
}

// Whether the passes 2 and 3 of this step can hand over (sphx_pass_pi): all blobs of one GPU, and no workgroup of pass 3
// with more blobs than its list holds (BLOB_OWN_MAX x 512 blobs = 4 x 10^6 particles).  The caller sizes ctx->va, ctx->vh
// and the marks (sphx_blob_size_marks).
bool sphx_blob_can_hand_visc(sphx_ctx* ctx, int64_t n) {
    if (!ctx->qorder || !ctx->blob_lists || ctx->map_perm || ctx->blob_split_valid) return false;
    const int nblk = (int)((sphx_pad64(n) + BLOB_P - 1) / BLOB_P);
    return nblk <= BLOB_OWN_MAX * sphx_blob_grid(ctx, nblk);
}
int sphx_blob_size_marks(sphx_ctx* ctx, int64_t n, bool row_bytes) {            // one byte per blob, read in 16-B pieces
    const size_t nblk = (size_t)((sphx_pad64(n) + BLOB_P - 1) / BLOB_P);
    if (row_bytes) SPHX_TRY(sphx_ensure(ctx, ctx->row_settled, (size_t)n));       // ... and one per row (the update by bytes)
    return sphx_ensure(ctx, ctx->visc_live, (nblk + 15) / 16 * 16);
}

// hand_on: pass 2 settles pass 3's rows and marks the blobs with others (ctx->va, ctx->vh, ctx->visc_live are sized)
// row_bytes (with hand_on): the rows' classes into ctx->row_settled instead of the settled rows' NaNs
int sphx_blob_pi(sphx_ctx* ctx, int64_t n, int k, u64* ct_bits, bool hand_on, bool row_bytes) {
    return blob_launch(ctx, blob_pi_kernel, PiPass::PER_SLOT, 0, n, k, ctx->map_perm, blob_n_active(ctx, n), ctx->recv.as<RecB>(),
                       ctx->rho_s.as<double>(), ctx->self_s.as<RecSelf>(), ctx->bc_s.as<RecBC>(), ctx->Pi.as<double>(),
                       ctx->map_perm ? ctx->Bw.as<double>() : nullptr, ct_bits, sphx_blob_sel(ctx, ctx->pass_part),
                       ctx->scal.as<u64>() + SC_SETTLED, hand_on ? ctx->va.as<double>() : nullptr,
                       hand_on ? ctx->vh.as<double>() : nullptr, hand_on ? ctx->visc_live.as<unsigned char>() : nullptr,
                       hand_on && row_bytes ? ctx->row_settled.as<unsigned char>() : nullptr);
}

// handed: the pass 2 before it ran with hand_on
int sphx_blob_visc(sphx_ctx* ctx, int64_t n, int k, const double* m, bool handed) {
    return blob_launch(ctx, blob_visc_kernel, ViscPass::PER_SLOT, 0, n, k, ctx->clip_grad, ctx->map_perm, blob_n_active(ctx, n),
                       ctx->recv.as<RecB>(), ctx->bc_s.as<RecBC>(), m, ctx->va.as<double>(), ctx->vh.as<double>(),
                       sphx_blob_sel(ctx, ctx->pass_part), ctx->scal.as<u64>() + SC_SETTLED,
                       handed ? ctx->visc_live.as<const unsigned char>() : nullptr);
}

int sphx_blob_visc_pw(sphx_ctx* ctx, int64_t n, int k, const double* m, u64* ct_bits) {
    return blob_launch(ctx, blob_visc_pw_kernel, ViscPwPass::PER_SLOT, 0, n, k, ctx->clip_grad, ctx->map_perm,
                       blob_n_active(ctx, n), ctx->recv.as<RecB>(), ctx->rho_s.as<double>(), ctx->bc_s.as<RecBC>(),
                       ctx->self_s.as<RecSelf>(), m, ctx->va.as<double>(), ctx->vh.as<double>(), ct_bits, sphx_blob_sel(ctx, ctx->pass_part));
}

// (the weights' registers are sized for K <= 40, else for SPHX_MAX_K: SPEC_MAXM)
int sphx_blob_density_species(sphx_ctx* ctx, int64_t n, int k, bool lean, int S, const double* fun, const int* row_of,
                              const double* m_sorted, double* F, double* Z, double* agb, int agb_on) {
    const auto kern = (KPAD(k) / LPP <= 10) ? blob_density_species_kernel<10> : blob_density_species_kernel<16>;
    return blob_launch(ctx, kern, 64, 0, n, k, ctx->clip_grad, ctx->rec1.as<RecA>(), ctx->rho_s.as<double>(), ctx->rho.as<double>(),
                       ctx->rhod.as<double>(), ctx->nden.as<double>(), lean ? nullptr : ctx->G.as<double>(),
                       ctx->ha.as<double>(), S, fun, row_of, m_sorted, ctx->agb, agb_on, F, Z, agb);
}

int sphx_blob_species(sphx_ctx* ctx, int64_t n, int k, int S, const double* fun, const int* row_of, const double* m_sorted, double* F,
                      double* Z, double* agb, int agb_on) {
    const auto kern = (KPAD(k) / LPP <= 10) ? blob_species_kernel<10> : blob_species_kernel<16>;
    return blob_launch(ctx, kern, 64, 0, n, k, S, ctx->rec1.as<RecA>(), fun, row_of, m_sorted, ctx->agb, agb_on, F, Z, agb);
}

// counting pass of the scatter plan (true) / the pass itself (false -> fill) on the blob lists
int sphx_blob_drag(sphx_ctx* ctx, int64_t n, int k, bool count_only, const double* m, const double* ptype, const double* mgm,
                   const double* mcs, const int* id, double* onto, const DragScatter& sc) {
    if (count_only)
        return blob_launch(ctx, blob_drag_kernel<false>, 0, DRAG_XLDS, n, k, nullptr, m, ptype, mgm, mcs, id, onto, sc);
    return blob_launch(ctx, blob_drag_kernel<true>, 64, DRAG_XLDS, n, k, ctx->recv.as<RecB>(), m, ptype, mgm, mcs, id, onto, sc);
}
