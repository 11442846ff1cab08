// sphx_blob.h - shared pieces of the LDS-staged sum passes (sphx_blob.hip: hydro_update's sums;
// sphx_loopforms.hip: the loop forms of the step's loop-form mode): blob geometry, the LDS image
// layout, staging, slot-list access, the lanes-per-particle reductions, the walk of a pass over its
// blobs and slot lists (blob_pass: written once, for every pass description) and the launcher.
#pragma once
#include "sphx_internal.h"
#include "sphx_pair.h"          // Q4, gload4; the pair terms the LDS kernels share with the gather kernels
#include "sphx_settled.h"       // when a row's sum is NaN without (further) summing

#ifndef BLOB_P
#define BLOB_P 128                  // particles per workgroup
#endif
#define BLOB_T (2 * BLOB_P)          // threads of the dedup kernel (two per particle)
#define LPP SPHX_SUM_PARTS           // lanes per particle in the passes = partial sums per total
#define PASS_T (BLOB_P * LPP)       // threads per workgroup of the passes
#ifndef BLOB_S
#define BLOB_S 960                  // hash-table entries = image slots
#endif
#ifndef DEDUP_PRIO
#define DEDUP_PRIO 2                 // wave priority of the list dedup
#endif
#ifndef BLOB_STAGE_PRIO
#define BLOB_STAGE_PRIO 1            // wave priority while a workgroup stages its image (0: as every other wave)
#endif
#ifndef PASS_MINW
#define PASS_MINW 4                  // waves per SIMD the pass kernels are compiled for
#endif
#define BLOB_PROBES 96
#define SLOT_NONE 0xFFFFu           // no neighbour (list shorter than K)
#define SLOT_OVER 0xFFFEu           // neighbour not staged: read it from global memory
#define DD_BATCH 8                  // list entries fetched together per lane by the dedup kernel

typedef unsigned short u16;

// ---- helpers -----------------------------------------------------------------------------------
// chunks 2c, 2c+1 of slot s
__device__ __forceinline__ Q4 lload4(const double2* img, int s, int c2) {
    const double2 lo = img[(2 * c2) * BLOB_S + s];
    const double2 hi = img[(2 * c2 + 1) * BLOB_S + s];
    return Q4{lo.x, lo.y, hi.x, hi.y};
}
// a whole 64-B record: from slot s of the image / from global memory
struct Q8 { Q4 lo, hi; };
__device__ __forceinline__ Q8 lload8(const double2* img, int s) { return Q8{lload4(img, s, 0), lload4(img, s, 1)}; }
template <class Rec>
__device__ __forceinline__ Q8 gload8(const Rec* r) {
    const double* q = reinterpret_cast<const double*>(r);
    return Q8{gload4(q), gload4(q + 4)};
}
// sqrt for the distances of the neighbour loops: the library's correctly rounded sequence (v_rsq_f64
// seed, two coupled Newton steps on g ~ sqrt(x), h ~ 1/(2 sqrt(x)), residual corrections) without its
// exponent rescaling and class checks - squared distances here are 0 or sit mid-range (1e20..1e45 m^2).
// Measured: library sqrt = 18 fp64-multiply issue slots, this = 11 (a pass spends ~80 per neighbour).
// Bit-identical to sqrt() on that range (test_step_loop_variants_are_bit_identical compares against
// the gather kernels, which call sqrt()).
__device__ __forceinline__ double sqrt_mid(double x) {
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y;
    double h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    const double d0 = __builtin_fma(-g, g, x);
    g = __builtin_fma(d0, h, g);
    const double d1 = __builtin_fma(-g, g, x);
    g = __builtin_fma(d1, h, g);
    return x > 0.0 ? g : 0.0;
}
struct SqrtMid { __device__ __forceinline__ double operator()(double x) const { return sqrt_mid(x); } };   // the terms of sphx_pair.h

// the value held by the other lane of the pair (lane ^ 1), moved inside the VALU
__device__ __forceinline__ double pair_swap(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0xB1, 0xF, 0xF, true);          // quad_perm [1,0,3,2]
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0xB1, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double pair_swap2(double v) {                                   // lane ^ 2
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x4E, 0xF, 0xF, true);          // quad_perm [2,3,0,1]
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x4E, 0xF, 0xF, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// total of the particle's LPP partial sums, in the fixed order (p0 + p1) [+ (p2 + p3)] that the gather
// kernels use as well (valid in every lane of the group)
__device__ __forceinline__ double group_total(double acc) {
    acc = acc + pair_swap(acc);
    if (LPP == 4) acc = acc + pair_swap2(acc);
    return acc;
}
__device__ __forceinline__ double group_max(double v) {
    v = fmax(v, pair_swap(v));
    if (LPP == 4) v = fmax(v, pair_swap2(v));
    return v;
}
// group_total of every double of a struct of sums
template <class S>
__device__ __forceinline__ void group_total_fields(S& s) {
    constexpr int NF = sizeof(S) / sizeof(double);
    static_assert(sizeof(S) == NF * sizeof(double), "a struct of doubles");
    double f[NF];
    __builtin_memcpy(f, &s, sizeof(S));
#pragma unroll
    for (int q = 0; q < NF; ++q) f[q] = group_total(f[q]);
    __builtin_memcpy(&s, f, sizeof(S));
}

#define NSTAGE ((BLOB_S + PASS_T - 1) / PASS_T)
#define NB (8 / LPP) // neighbours in flight per lane (one batch = 8 list positions)
#define KPAD(k) ((((k) + 7) / 8) * 8)      // slot tile rows: whole batches
#define IMG_BYTES(per_slot, k) ((size_t)BLOB_S * (per_slot) + (size_t)KPAD(k) * BLOB_P * sizeof(u16))

// Fill the workgroup's LDS: slot lists (16-B pieces; rows k..KPAD(k) read as "no neighbour") and the
// records of the occupied table entries.  NSIDE 1: one 8-B side value per slot.  NSIDE 2 (pass 3):
// g0 replaces the record's last double (cs, unused there) and g1 is the side value.  All global
// loads are issued before the first use.  (One lane per record: four lanes per record - 16 whole records per load
// instruction instead of 64 quarter records, a quarter of the distinct lines per instruction - measured SLOWER, passes
// +10 % (162 / 181 / 149 -> 180 / 200 / 163 us): eight rounds of loads per thread instead of two, 4-way conflicts on the
// image stores; round 3.)
template <int NSIDE, class Rec>
__device__ __forceinline__ void stage(double2* img, double* side, u16* tile, const Rec* __restrict__ rec,
                                      const double* __restrict__ g0, int g0_stride,
                                      const double* __restrict__ g1, int g1_stride,
                                      const int* __restrict__ uq, const u16* __restrict__ slot16, int npad,
                                      int k, int b) {
    // the few instructions of a staging go ahead of the other resident workgroup's arithmetic: its loads are out a little
    // earlier (passes -4 % at 1e6: 0.160 / 0.199 / 0.150 -> 0.153 / 0.195 / 0.145 ms; priority 3 the same; raised again while
    // a batch's LDS reads are issued: nothing more)
    __builtin_amdgcn_s_setprio(BLOB_STAGE_PRIO);
    int ju[NSTAGE];
#pragma unroll
    for (int r = 0; r < NSTAGE; ++r) {
        const int s = threadIdx.x + r * PASS_T;
        ju[r] = (s < BLOB_S) ? uq[s] : -1;
    }
    const int pieces = KPAD(k) * (BLOB_P / 8);
    for (int q = threadIdx.x; q < pieces; q += PASS_T) {
        const int kk = q / (BLOB_P / 8), c = q % (BLOB_P / 8);
        uint4 v = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
        if (kk < k) v = *reinterpret_cast<const uint4*>(slot16 + (size_t)kk * npad + (size_t)b * BLOB_P + c * 8);
        *reinterpret_cast<uint4*>(tile + kk * BLOB_P + c * 8) = v;
    }
    double2 c[NSTAGE][4];
    double e0[NSTAGE], e1[NSTAGE];
#pragma unroll
    for (int r = 0; r < NSTAGE; ++r) {
        const int j = ju[r] < 0 ? 0 : ju[r];
        const double2* g = reinterpret_cast<const double2*>(&rec[j]);       // empty entry: particle 0, not stored
        c[r][0] = g[0]; c[r][1] = g[1]; c[r][2] = g[2]; c[r][3] = g[3];
        e0[r] = (NSIDE > 0) ? g0[(size_t)j * g0_stride] : 0.0;
        e1[r] = (NSIDE > 1) ? g1[(size_t)j * g1_stride] : 0.0;
    }
#pragma unroll
    for (int r = 0; r < NSTAGE; ++r) {
        const int s = threadIdx.x + r * PASS_T;
        if (ju[r] >= 0) {
            if (NSIDE == 2) c[r][3].y = e0[r];
            img[0 * BLOB_S + s] = c[r][0]; img[1 * BLOB_S + s] = c[r][1];
            img[2 * BLOB_S + s] = c[r][2]; img[3 * BLOB_S + s] = c[r][3];
            if (NSIDE == 1) side[s] = e0[r];
            if (NSIDE == 2) side[s] = e1[r];
        }
    }
    __builtin_amdgcn_s_setprio(0);
}

// the lane's slot numbers for batch m0 (tile rows beyond k hold SLOT_NONE)
__device__ __forceinline__ void load_slots(unsigned (&sl)[NB], const u16* tile, int m0, int half, int t) {
#pragma unroll
    for (int u = 0; u < NB; ++u) sl[u] = tile[(LPP * (m0 + u) + half) * BLOB_P + t];
}
__device__ __forceinline__ bool all_staged(const unsigned (&sl)[NB]) {
    unsigned worst = sl[0];
#pragma unroll
    for (int u = 1; u < NB; ++u) worst = worst > sl[u] ? worst : sl[u];
    return __ballot(worst >= SLOT_OVER) == 0ull;
}


// The blobs a launch works through: all nblk of them, or one of blob_split_kernel's lists (decomposed runs: the
// interior blobs while a halo phase is in flight, the boundary blobs after it) - its length read from device memory.
// list: interior blobs, then boundary blobs (each in blob order); cnt = {interior, boundary, idle}.
// mode 1: the interior ones, 2: the boundary ones, 3: both (every blob with something to compute).
struct BlobSel { const int* list; const int* cnt; int mode; };
__device__ __forceinline__ int blob_sel_count(const BlobSel& s, int nblk) {
    if (!s.list) return nblk;
    return (s.mode == 1) ? s.cnt[0] : (s.mode == 2) ? s.cnt[1] : s.cnt[0] + s.cnt[1];
}
__device__ __forceinline__ int blob_sel_at(const BlobSel& s, int bi, int count) {
    const int q = xcd_block(bi, count);
    return s.list ? s.list[q + (s.mode == 2 ? s.cnt[0] : 0)] : q;
}
// part: 0 all blobs (with a valid split: all but the idle ones), 1 the interior ones, 2 the boundary ones
BlobSel sphx_blob_sel(sphx_ctx* ctx, int part);

int sphx_blob_grid(sphx_ctx* ctx, int nblk);       // persistent grid of the LDS passes (2 workgroups per CU)
// allow `kernel` up to `bytes` of dynamic LDS on the context's device (once per kernel: sphx_ctx::lds_raised)
int sphx_lds_opt_in(sphx_ctx* ctx, const void* kernel, size_t bytes);

// the launch bounds of a pass kernel and the arguments every LDS kernel begins with
#define BLOB_KERNEL __global__ __launch_bounds__(PASS_T, PASS_MINW) void
#define BLOB_COMMON int n, int npad, int k, int nblk, const int* __restrict__ nbr, const u16* __restrict__ slot16, \
                    const int* __restrict__ uniq, const int* __restrict__ qorder
// One launch on the persistent grid: blob_launch fills in BLOB_COMMON, `rest` are the arguments behind it.
// Dynamic LDS: per_slot bytes of image per slot (0: no image) and the slot tile, + extra.
template <class Kern, class... Rest>
static int blob_launch(sphx_ctx* ctx, Kern kern, int per_slot, size_t extra, int64_t n, int k, Rest... rest) {
    const int64_t npad = sphx_pad64(n);
    const int nblk = (int)((npad + BLOB_P - 1) / BLOB_P);
    SPHX_TRY(sphx_lds_opt_in(ctx, reinterpret_cast<const void*>(kern), IMG_BYTES(per_slot, SPHX_MAX_K) + extra));
    hipLaunchKernelGGL(kern, dim3(sphx_blob_grid(ctx, nblk)), dim3(PASS_T), IMG_BYTES(per_slot, k) + extra, ctx->stream, (int)n,
                       (int)npad, k, nblk, ctx->nbr.as<int>(), ctx->slot16.as<u16>(), ctx->uniq.as<int>(), ctx->qorder, rest...);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

// ---- the walk of an LDS sum pass ------------------------------------------------------------------------------------
// How a pass goes through its blobs and its slot lists is written here once (blob_pass); a kernel is its __global__
// signature, a pass description P and one call.  P says what differs between the passes and nothing of the walk:
//   Rec, NSIDE, PER_SLOT, rec, sides()   what is staged: the 64-B records, the side values per slot (stage<>), and the
//                                        image bytes per slot the launcher is given
//   Row, load_row(i), load_out(row, o, on)
//                                        the row particle's own loads, issued ahead of the barrier behind the staging:
//                                        by stored particle i, then what is indexed by the output index o
//   ROW_FROM_LIST, row_point(row, nb)    deltas are relative to the first list position (hydro_update, nsc:580-581)
//                                        or to the particle itself (loop forms)
//   wanted(row)                          whether the row particle sums at all
//   Nb, staged(img, side, s, jp), global(j), none(row)
//                                        one list position's operands: out of image slot s (jp: where the int32 list
//                                        names it, for what is not staged), from global memory, or the stand-in of a
//                                        position the list does not have
//   Sums, term<CLIP>(sums, nb, row)      the pair's term (sphx_pair.h, or the loop forms'); its return value is the
//                                        candidate of the crossing-time maximum (VOTES) or the species weight
//   CLIPS                                whether the term distinguishes clipped gradients (4-way dispatch, else 2-way)
//   finish(sums, max, row, i, o), VOTES  what the first lane of a particle writes; returns its crossing-time vote
// and, optional (a description without them walks as before, instruction for instruction; sphx_settled.h):
//   SETTLES, own(i), settle(o)           a row whose own value own(i) is NaN - and that writes, and has a first list
//                                        position - sums to NaN whatever its neighbours hold: settle(o) writes that.  A
//                                        blob of such rows is neither staged nor walked, a wave of them is not walked.
//   SATURATES, saturated(sums), Vel, short_staged(img, s), short_global(j), short_none(row), term_short(vel, row)
//                                        sums that stay NaN once they are: when every row of a wave has one, the wave's
//                                        remaining batches fetch and compute only what term()'s return value needs
//   HANDS_ON, hands_on(), finish(sums, max, row, i, o, has_first, live), hand_on(b, any_live)
//                                        a pass that knows at finish how the NEXT pass's vote on the row will go: finish is
//                                        told whether the row has a first list position and settles the row for that pass,
//                                        or says that it is `live`; behind the barrier that closes blob b, hand_on is told
//                                        whether any of its rows is (one thread; hands_on() false: neither is asked for)
template <class P, class = void> struct BlobSettles { static constexpr bool value = false; };
template <class P> struct BlobSettles<P, decltype((void)P::SETTLES)> { static constexpr bool value = P::SETTLES; };
template <class P, class = void> struct BlobSaturates { static constexpr bool value = false; };
template <class P> struct BlobSaturates<P, decltype((void)P::SATURATES)> { static constexpr bool value = P::SATURATES; };
template <class P, class = void> struct BlobHandsOn { static constexpr bool value = false; };
template <class P> struct BlobHandsOn<P, decltype((void)P::HANDS_ON)> { static constexpr bool value = P::HANDS_ON; };
// the counters of the two shortcuts behind a launch's pointer (nullptr: not counted)
// (LAUNCHES_SKIPPED: launches of pass 3 that found no live row left by pass 2 and returned; their blobs count as settled)
enum { BLOB_CNT_BLOBS_SETTLED = 0, BLOB_CNT_WAVES_SATURATED = 1, BLOB_CNT_LAUNCHES_SKIPPED = 2 };
struct BlobSides { const double* g0 = nullptr; int s0 = 0; const double* g1 = nullptr; int s1 = 0; };   // stage<>'s g0, g1

// dynamic LDS of a pass: 4 * BLOB_S chunks of image, BLOB_S side values (NSIDE > 0), the slot tile.  (Accessors, not
// pointers handed on in a struct: the compiler has to see the LDS address space at every use, or it merges an image read
// with the global-memory read of the other branch into one flat load.)
template <int NSIDE>
struct BlobLds {
    // (`img`: the one dynamic-LDS symbol of every kernel of the library, blob_species_kernel's and blob_drag_kernel's too -
    // with a second one in the module the species kernels came out with flat loads as well)
    static __device__ __forceinline__ double2* img() { extern __shared__ double2 img[]; return img; }
    static __device__ __forceinline__ double* side() { return reinterpret_cast<double*>(img() + 4 * BLOB_S); }
    static __device__ __forceinline__ u16* tile() { return reinterpret_cast<u16*>(side() + (NSIDE ? BLOB_S : 0)); }
};

// A batch of NB list positions of this lane.  FAST: every lane of the wave has a staged neighbour at
// each of them (the usual case): straight-line LDS reads and arithmetic, nothing to branch on.
// Otherwise a position may be empty (skipped) or unstaged (fetched through the int32 list).
// out: what the term returned (0 where the list has no neighbour).
template <bool FAST, bool CLIP, class P>
__device__ __forceinline__ void blob_batch(const P& ps, typename P::Sums& a, double (&out)[NB], const unsigned (&sl)[NB],
                                           const int* __restrict__ jp, size_t colstep, const typename P::Row& row) {
    typedef BlobLds<P::NSIDE> L;
    typename P::Nb f[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (FAST || sl[u] < SLOT_OVER) f[u] = ps.staged(L::img(), L::side(), (int)sl[u], jp + u * colstep);
        else if (sl[u] == SLOT_OVER) f[u] = ps.global(jp[u * colstep]);
        else f[u] = P::none(row);
    }
    if (FAST) __builtin_amdgcn_sched_barrier(0);       // all of the batch's LDS reads are issued before its arithmetic
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        out[u] = 0.0;
        if (!FAST && sl[u] == SLOT_NONE) continue;
        out[u] = ps.template term<CLIP>(a, f[u], row);
    }
}
// the batch in the form its slots and the runtime `clip` ask for
template <class P>
__device__ __forceinline__ void blob_batch_any(const P& ps, int clip, typename P::Sums& a, double (&out)[NB],
                                               const unsigned (&sl)[NB], const int* __restrict__ jp, size_t colstep,
                                               const typename P::Row& row) {
    const bool fast = all_staged(sl);
    if constexpr (P::CLIPS) {
        if (fast && !clip) blob_batch<true, false>(ps, a, out, sl, jp, colstep, row);
        else if (fast) blob_batch<true, true>(ps, a, out, sl, jp, colstep, row);
        else if (!clip) blob_batch<false, false>(ps, a, out, sl, jp, colstep, row);
        else blob_batch<false, true>(ps, a, out, sl, jp, colstep, row);
    } else {
        if (fast) blob_batch<true, false>(ps, a, out, sl, jp, colstep, row);
        else blob_batch<false, false>(ps, a, out, sl, jp, colstep, row);
    }
}
// A batch of a saturated wave (P::SATURATES): the operands and the arithmetic of term()'s return value alone.
template <bool FAST, class P>
__device__ __forceinline__ void blob_batch_short(const P& ps, double (&out)[NB], const unsigned (&sl)[NB],
                                                 const int* __restrict__ jp, size_t colstep, const typename P::Row& row) {
    typedef BlobLds<P::NSIDE> L;
    typename P::Vel f[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (FAST || sl[u] < SLOT_OVER) f[u] = P::short_staged(L::img(), (int)sl[u]);
        else if (sl[u] == SLOT_OVER) f[u] = ps.short_global(jp[u * colstep]);
        else f[u] = P::short_none(row);
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        out[u] = 0.0;
        if (!FAST && sl[u] == SLOT_NONE) continue;
        out[u] = P::term_short(f[u], row);
    }
}
// what the vote on "settled" needs of a row (P::SETTLES), fetched a blob ahead of the vote: its particle's own value,
// its output index and its first list position
struct RowAhead { int i, o; unsigned first; double own; };
template <class P>
__device__ __forceinline__ RowAhead blob_row_ahead(const P& ps, int i, int p, int n, const u16* __restrict__ slot16,
                                                   const int* __restrict__ omap) {
    RowAhead r;
    r.i = i;                                               // (p >= n: particle 0, a valid address; it writes nothing)
    r.o = (p < n) ? (omap ? omap[i] : i) : 0x7FFFFFFF;
    r.first = (p < n) ? slot16[p] : SLOT_NONE;
    r.own = ps.own(i);
    return r;
}
// Whether `mine` holds in every thread of the workgroup, decided AT a barrier the caller needs anyway (every thread
// calls, in uniform control flow): each wave leaves its verdict in LDS ahead of the barrier and reads all of them behind
// it.  Two sets of words by the parity of `round`, which the caller counts up: a wave that is through may vote again
// (other set) while a slower one still reads; the set after that lies behind the next barrier.  (__syncthreads_and
// is three barriers and an LDS atomic: measured slower on a pass whose blobs take 9 us each)
template <int T>
__device__ __forceinline__ bool block_all_at_barrier(bool mine, unsigned round) {
    __shared__ int verdict[2][T / 64];
    static_assert(T / 64 == 8, "eight waves: read as two 16-B pieces");
    int* v = verdict[round & 1];
    const int wave_all = __ballot(!mine) == 0ull;
    if ((threadIdx.x & 63) == 0) v[threadIdx.x >> 6] = wave_all;
    __syncthreads();
    const int4 lo = *reinterpret_cast<const int4*>(v), hi = *reinterpret_cast<const int4*>(v + 4);
    const int all = (lo.x & lo.y) & (lo.z & lo.w) & (hi.x & hi.y) & (hi.z & hi.w);
    return __builtin_amdgcn_readfirstlane(all) != 0;
}
// sum of a count over the workgroup's waves (every thread calls; `v` is uniform in a wave), added to *dst by one thread
template <int T>
__device__ __forceinline__ void block_add_count(unsigned v, u64* dst) {
    __shared__ unsigned sm[T / 64];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned r = 0;
        for (int w = 0; w < T / 64; ++w) r += sm[w];
        if (r) atomicAdd(dst, (u64)r);
    }
}
// the blobs a workgroup takes where it is not dealt them by its number (blob_pass, own_n >= 0): filled by the kernel
#define BLOB_OWN_MAX 64
__device__ __forceinline__ int* blob_own_list() {
    __shared__ int own[BLOB_OWN_MAX];
    return own;
}
// HANDS_ON: whether a row of the blob in hand is live for the next pass (raised at finish, read and lowered by thread 0
// behind the barrier that closes the blob)
__device__ __forceinline__ int* blob_live_flag() {
    __shared__ int flag;
    return &flag;
}
// the row point out of the first list position (column p of the list, particle t of the blob): image, global memory,
// or - no first neighbour - what load_row left.  (The pass's whole fetch is called and row_point keeps what it wants:
// the loads of the rest - a side value, ViscPwPass's bc[*jp] - are plain loads of valid addresses that the compiler
// drops as dead; made volatile or atomic they would be executed.)
template <class P>
__device__ __forceinline__ void blob_row_point(const P& ps, typename P::Row& row, const int* __restrict__ nbr, int p,
                                               int t) {
    typedef BlobLds<P::NSIDE> L;
    const unsigned sl0 = L::tile()[t];
    if (sl0 < SLOT_OVER) P::row_point(row, ps.staged(L::img(), L::side(), (int)sl0, nbr + p));
    else if (sl0 == SLOT_OVER) P::row_point(row, ps.global(nbr[p]));
}

// The pass.  A change to the walk - workgroups per CU, prefetch depth, how blobs are handed out - is made here.
// clip: ignored unless P::CLIPS.  omap, n_active: outputs go to the caller's index o (device API: ghosts, o >= n_active,
// are candidates only); omap == nullptr: o = the stored particle.  ct_bits: where P::VOTES passes vote.
// counts: the shortcuts taken (BLOB_CNT_*; nullptr: not counted) - one atomic per workgroup, at its end.
// own_n (-1: the blobs of `sel`, dealt out by workgroup number): THIS workgroup takes the blobs blob_own_list()[0 .. own_n).
template <class P>
__device__ __forceinline__ void blob_pass(const P& ps, int n, int npad, int k, int nblk, const int* __restrict__ nbr,
                                          const u16* __restrict__ slot16, const int* __restrict__ uniq,
                                          const int* __restrict__ qorder, int clip, const int* __restrict__ omap,
                                          int n_active, u64* ct_bits, const BlobSel& sel, u64* counts = nullptr,
                                          int own_n = -1) {
    static_assert(P::PER_SLOT == 64 + (P::NSIDE ? 8 : 0), "image bytes per slot: the record and one side value");
    constexpr bool SETTLES = BlobSettles<P>::value, SATURATES = BlobSaturates<P>::value, HANDS_ON = BlobHandsOn<P>::value;
    static_assert(!SATURATES || LPP == 4, "sphx_wave_saturated: a row's lanes are one nibble of the wave's mask");
    typedef BlobLds<P::NSIDE> L;
    const BlobSides sd = ps.sides();
    const int t = threadIdx.x / LPP, half = threadIdx.x & (LPP - 1);     // half: which partial sum
    u64 my_ct = SPHX_CT_NONE;
    unsigned blobs_settled = 0, waves_saturated = 0;         // shortcuts taken (the first: uniform in the workgroup)
    // persistent workgroups (two per CU): blob after blob, no dispatch gap between them
    if constexpr (HANDS_ON) {
        if (threadIdx.x == 0) *blob_live_flag() = 0;         // (raised only behind the first staging's barrier)
    }
    const int stride = gridDim.x;
    const bool own = own_n >= 0;
    const int nsel = own ? (own_n ? (int)blockIdx.x + (own_n - 1) * stride + 1 : 0) : blob_sel_count(sel, nblk);
    auto blob_at = [&](int bq) -> int {
        return own ? blob_own_list()[(bq - (int)blockIdx.x) / stride] : blob_sel_at(sel, bq, nsel);
    };
    // SETTLES: the vote's operands hang on the chain qorder[p] -> own(i).  They are fetched a blob ahead, and the
    // particle two blobs ahead, and a blob's vote rides on the barrier that ends the blob before it
    // (block_all_at_barrier): a blob that runs meets no wait and no barrier it did not have.  Where blob after blob
    // is settled, the workgroup goes at one round trip and one barrier per blob.
    auto particle_of = [&](int bq) -> int {
        const int pq = blob_at(bq) * BLOB_P + t;
        return (pq < n) ? qorder[pq] : 0;
    };
    auto nothing_left = [&](const RowAhead& r) -> bool {     // a row that writes nothing counts as settled for the vote
        return !(r.o < n_active) || sphx_row_settled(r.own, r.first != SLOT_NONE, true);
    };
    RowAhead cur{0, 0x7FFFFFFF, SLOT_NONE, 0.0};
    int i_next = 0;
    bool blob_settled = false;                               // the vote on the blob about to begin
    unsigned round = 0;
    if constexpr (SETTLES) {
        if ((int)blockIdx.x < nsel)
            cur = blob_row_ahead(ps, particle_of(blockIdx.x), blob_at(blockIdx.x) * BLOB_P + t, n, slot16, omap);
        if ((int)blockIdx.x + stride < nsel) i_next = particle_of(blockIdx.x + stride);
        blob_settled = block_all_at_barrier<PASS_T>(nothing_left(cur), round++);
    }
    for (int bi = blockIdx.x; bi < nsel; bi += stride) {
        const int b = blob_at(bi);
        const int p = b * BLOB_P + t;
        int i, o;
        bool settled = false;
        // the next blob's row operands and the particle of the one after it
        auto fetch_ahead = [&]() {
            if constexpr (SETTLES) {
                if (bi + stride < nsel) {                   // (the last blob votes on itself once more: nobody asks)
                    cur = blob_row_ahead(ps, i_next, blob_at(bi + stride) * BLOB_P + t, n, slot16, omap);
                    if (bi + 2 * stride < nsel) i_next = particle_of(bi + 2 * stride);
                }
            }
        };
        if constexpr (SETTLES) {
            i = cur.i; o = cur.o;
            settled = sphx_row_settled(cur.own, cur.first != SLOT_NONE, o < n_active);
            if (blob_settled) {                            // no image, no walk: the sums are NaN (sphx_settled.h)
                fetch_ahead();
                if (settled && !half) ps.settle(o);
                ++blobs_settled;
                blob_settled = block_all_at_barrier<PASS_T>(nothing_left(cur), round++);
                continue;
            }
        } else {
            i = (p < n) ? qorder[p] : 0;
        }
        stage<P::NSIDE>(L::img(), L::side(), L::tile(), ps.rec, sd.g0, sd.s0, sd.g1, sd.s1, uniq + (size_t)b * BLOB_S,
                        slot16, npad, k, b);
        typename P::Row row = ps.load_row(i);                // (issued ahead of the wait for omap[i], not behind it)
        if constexpr (!SETTLES) o = (p < n) ? (omap ? omap[i] : i) : 0x7FFFFFFF;
        ps.load_out(row, o, o < n_active);
        // (behind the staging's loads, not in front of them: loads return in order, and a gather issued first would
        //  hold back the slot table that the records' addresses wait for)
        if constexpr (SETTLES) fetch_ahead();
        __syncthreads();
        if (o < n_active) {
            if (SETTLES && __ballot(!settled) == 0ull) {    // a wave of settled rows in a blob that runs
                if constexpr (SETTLES) { if (!half) ps.settle(o); }
            } else {
                if constexpr (P::ROW_FROM_LIST) blob_row_point(ps, row, nbr, p, t);
                typename P::Sums a{};
                double mx = 0.0;
                if (P::wanted(row)) {
                    const int nm = KPAD(k) / LPP;
                    unsigned sl[NB];
                    load_slots(sl, L::tile(), 0, half, t);
                    bool short_form = false;         // SATURATES: every row of this wave has a NaN sum already
                    bool short_used = false;
                    for (int m0 = 0; m0 < nm; m0 += NB) {
                        unsigned cur_sl[NB];
#pragma unroll
                        for (int u = 0; u < NB; ++u) cur_sl[u] = sl[u];
                        // next batch's slots, behind this one's reads
                        if (m0 + NB < nm) load_slots(sl, L::tile(), m0 + NB, half, t);
                        double out[NB];
                        const int* jp = nbr + ((size_t)(LPP * m0 + half) * npad + p);
                        if constexpr (SATURATES) {
                            if (__builtin_expect(short_form, false)) {     // (laid out behind the full batch)
                                short_used = true;
                                if (all_staged(cur_sl)) blob_batch_short<true>(ps, out, cur_sl, jp, LPP * (size_t)npad, row);
                                else blob_batch_short<false>(ps, out, cur_sl, jp, LPP * (size_t)npad, row);
                            } else {
                                blob_batch_any(ps, clip, a, out, cur_sl, jp, LPP * (size_t)npad, row);
                                // (only the lanes of rows that sum are here: __ballot(true) is the wave's live rows)
                                short_form = sphx_wave_saturated(__ballot(P::saturated(a)), __ballot(true));
                            }
                        } else {
                            blob_batch_any(ps, clip, a, out, cur_sl, jp, LPP * (size_t)npad, row);
                        }
                        if (P::VOTES) {
#pragma unroll
                            for (int u = 0; u < NB; ++u) mx = fmax(mx, out[u]);
                        }
                    }
                    if (SATURATES && short_used) ++waves_saturated;
                }
                group_total_fields(a);
                if (P::VOTES) mx = group_max(mx);
                if (!half) {
                    u64 cb;
                    if constexpr (HANDS_ON) {
                        bool live = false;
                        cb = ps.finish(a, mx, row, i, o, L::tile()[t] != SLOT_NONE, live);
                        if (live) *blob_live_flag() = 1;       // (every live row the same word, the same value)
                    } else {
                        cb = ps.finish(a, mx, row, i, o);
                    }
                    my_ct = cb < my_ct ? cb : my_ct;
                }
            }
        }
        // the image is rewritten by the next blob
        if constexpr (SETTLES) blob_settled = block_all_at_barrier<PASS_T>(nothing_left(cur), round++);
        else __syncthreads();
        if constexpr (HANDS_ON) {
            // (the next blob's rows raise the flag behind the barrier that follows its staging: this thread is through here)
            if (ps.hands_on() && threadIdx.x == 0) { ps.hand_on(b, *blob_live_flag() != 0); *blob_live_flag() = 0; }
        }
    }
    if (P::VOTES) block_min_vote<PASS_T>(my_ct, ct_bits);
    if constexpr (SETTLES) {
        if (counts && threadIdx.x == 0 && blobs_settled) atomicAdd(counts + BLOB_CNT_BLOBS_SETTLED, (u64)blobs_settled);
    }
    if constexpr (SATURATES) {
        if (counts) block_add_count<PASS_T>(waves_saturated, counts + BLOB_CNT_WAVES_SATURATED);      // (uniform: an argument)
    }
}
