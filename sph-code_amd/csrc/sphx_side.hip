// sphx_side.hip - what the side stages beside the step share on the device: the reverse list of rad_cooling,
// supernova_destruction and chemisputtering_2 (sphx_rev_build), and the ordered totals of the two resident phases'
// bookkeeping (sphx_ordered_totals).  The one translation unit of these stages that includes rocprim.
#include "sphx_internal.h"
#include "sphx_revlist.h"
#include <rocprim/rocprim.hpp>
#pragma clang fp contract(off)

// ---- the reverse list ----
// A stage's scatter turned round: for each of the n segments (the particles that receive) the entries that hold it.  The
// stage has counted them (cnt, with cnt[n] = 0; cnt and start on 16-byte boundaries); here the exclusive scan into start,
// the total M brought to the host (one synchronise), the stage's own fill kernel - whose order is whatever the atomics
// give - and the sort of every slice, which removes that order: the same inputs give the same list on every call.
// pairs: what M cannot exceed.  key_end: the entries are keys in [0, key_end).  fill(start, rev_raw) launches the fill.
// M == 0: nothing is filled or sorted.  The list is in ctx->side_rev (sphx_revlist.h has the layout) until the next call.
int sphx_rev_build(sphx_ctx* ctx, const char* who, int64_t n, const int* cnt, int* start, size_t pairs, unsigned long long key_end,
                   const std::function<void(const int* start, int* rev_raw)>& fill, RevList* out) {
    hipStream_t st = ctx->stream;
    SPHX_TRY(sphx_excl_scan_int(ctx, cnt, start, (int)n));
    HIPCHK(hipMemcpyAsync(&ctx->pinned->side.count, start + n, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const size_t M = (size_t)ctx->pinned->side.count;
    if (M > pairs) return sphx_set_err(ctx, SPHX_E_HIP, "%s: reverse list of %zu entries from %zu pairs", who, M, pairs);
    return sphx_rev_fill_sort(ctx, n, start, M, key_end, fill, ctx->side_rev, ctx->side_tmp, out);
}
// The fill and the segmented sort alone, into the caller's buffers (the projected maps, sphx_map.hip: segments are tiles,
// entries particle ids, and the total has been checked on the host against a 64-bit count before anything is sized).
int sphx_rev_fill_sort(sphx_ctx* ctx, int64_t n, const int* start, size_t M, unsigned long long key_end,
                       const std::function<void(const int* start, int* rev_raw)>& fill, DevBuf& rev_buf, DevBuf& tmp_buf, RevList* out) {
    hipStream_t st = ctx->stream;
    SPHX_TRY(sphx_ensure(ctx, rev_buf, sphx_rev_ints(M) * sizeof(int)));
    int* rev_raw = rev_buf.as<int>();
    int* rev = rev_raw + sphx_rev_sorted_at(M);
    if (M > 0) {
        fill(start, rev_raw);
        HIPCHK(hipGetLastError());
        const unsigned bits = sphx_rev_bits(key_end);
        size_t sort_bytes = 0;
        HIPCHK(rocprim::segmented_radix_sort_keys(nullptr, sort_bytes, rev_raw, rev, (unsigned)M, (unsigned)n, start, start + 1, 0u, bits, st));
        SPHX_TRY(sphx_ensure(ctx, tmp_buf, sort_bytes + 64));
        HIPCHK(rocprim::segmented_radix_sort_keys(tmp_buf.p, sort_bytes, rev_raw, rev, (unsigned)M, (unsigned)n, start, start + 1, 0u, bits, st));
    }
    out->M = M; out->rev = rev;
    return SPHX_OK;
}

// ---- the ordered totals ----
// Sums over the particles of nq per-particle terms pp (nq, n): per chunk of SPHX_TOT_CHUNK rows in index order, then the
// chunks by one workgroup per quantity in a fixed order (chem_colsum_kernel's scheme): the same bits on every call.
#define TOT_WG 256
static_assert(SPHX_TOT_CHUNK == 256, "a chunk is 256 rows");
// lane t = (quantity q, chunk c): the chunk's sum in index order
__global__ __launch_bounds__(TOT_WG) void sphx_chunksum_kernel(int n, int nq, int nchunk, const double* __restrict__ pp, double* __restrict__ part) {
    const int t = blockIdx.x * TOT_WG + threadIdx.x;
    if (t >= nq * nchunk) return;
    const int q = t / nchunk, c = t - q * nchunk;
    const int i1 = min(n, (c + 1) * SPHX_TOT_CHUNK);
    double sum = 0.0;
    for (int i = c * SPHX_TOT_CHUNK; i < i1; ++i) sum += pp[(size_t)q * n + i];
    part[t] = sum;
}
// one workgroup per quantity: lane l adds the chunks l, l + TOT_WG, ... in order, then a tree over the lanes
__global__ __launch_bounds__(TOT_WG) void sphx_total_kernel(int nchunk, const double* __restrict__ part, double* __restrict__ tot) {
    __shared__ double sm[TOT_WG];
    const int q = blockIdx.x, l = threadIdx.x;
    double sum = 0.0;
    for (int c = l; c < nchunk; c += TOT_WG) sum += part[(size_t)q * nchunk + c];
    sm[l] = sum;
    __syncthreads();
    for (int h = TOT_WG / 2; h > 0; h >>= 1) {
        if (l < h) sm[l] += sm[l + h];
        __syncthreads();
    }
    if (l == 0) tot[q] = sm[0];
}
// the second stage on ready chunk sums (the census forms its own, sphx_census.hip)
int sphx_ordered_totals_of_parts(sphx_ctx* ctx, size_t nchunk, int nq, const double* part, double* tot) {
    hipLaunchKernelGGL(sphx_total_kernel, dim3((unsigned)nq), dim3(TOT_WG), 0, ctx->stream, (int)nchunk, part, tot);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}
// part: nq sphx_tot_chunks(n) doubles, tot: nq.  The totals' copy into ctx->pinned->scal is queued: the caller reads it
// after its next synchronise (nq <= SC_NSLOTS: the callers assert it at their enums).
int sphx_ordered_totals(sphx_ctx* ctx, int64_t n, int nq, const double* pp, double* part, double* tot) {
    hipStream_t st = ctx->stream;
    const size_t nchunk = sphx_tot_chunks(n);
    hipLaunchKernelGGL(sphx_chunksum_kernel, dim3(sphx_blocks((size_t)nq * nchunk, TOT_WG)), dim3(TOT_WG), 0, st, (int)n, nq, (int)nchunk, pp, part);
    SPHX_TRY(sphx_ordered_totals_of_parts(ctx, nchunk, nq, part, tot));
    HIPCHK(hipMemcpyAsync(ctx->pinned->scal, tot, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, st));
    return SPHX_OK;
}
