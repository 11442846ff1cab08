// sphx_phase_map.h - the slot arithmetic that turns the step's own neighbour list into a list in caller ids
// (sphx_phase.hip: sphx_state_dust_phase, sphx_state_download_neighbors).
//
// The step's list (ctx->nbr) is int32, K-major with rows of npad columns.  Column p belongs to the particle in storage
// slot qorder[p] (qorder == NULL: slot p), an entry is a storage slot or -1, and the particle in slot j has the caller id
// id[j].  The caller-order list has the same layout with column i for caller id i and entries that are caller ids:
//   col[id[slot(p)]] = p                                  one lane per column p       (sphx_phase_col_lane)
//   out[kk][i] = id[nbr[kk][col[i]]], or -1               one lane per (kk, i)        (sphx_phase_entry)
// The second pass stores coalesced; its loads go through col.  The columns i in [n, npad) are written -1.
// The (n,k) int64 list of sphx_state_download_neighbors holds n for a missing entry (sphx_phase_entry64).
// The rule is host code as well: tests/host/phase_map_check.cpp replays both passes over random orders and lists.
#pragma once
#include <stddef.h>
#if defined(__HIPCC__)
#define SPHX_PHASE_HD __host__ __device__
#else
#define SPHX_PHASE_HD
#endif
// place of column c of list position kk
SPHX_PHASE_HD inline size_t sphx_phase_at(int kk, int npad, int c) { return (size_t)kk * (size_t)npad + (size_t)c; }
// lane p < n of the first pass: the storage slot of column p, and col[] of its caller id
SPHX_PHASE_HD inline int sphx_phase_slot(const int* qorder, int p) { return qorder ? qorder[p] : p; }
SPHX_PHASE_HD inline void sphx_phase_col_lane(const int* qorder, const int* id, int p, int* col) { col[id[sphx_phase_slot(qorder, p)]] = p; }
// lane e < k npad of the second pass: list position kk = e / npad, caller id i = e % npad
SPHX_PHASE_HD inline int sphx_phase_entry(const int* nbr, const int* id, const int* col, int n, int npad, int kk, int i) {
    if (i >= n) return -1;
    const int q = nbr[sphx_phase_at(kk, npad, col[i])];
    return (q >= 0 && q < n) ? id[q] : -1;
}
// entry (i, kk) of the (n,k) int64 list from the caller-order K-major list
SPHX_PHASE_HD inline long long sphx_phase_entry64(const int* out, int n, int npad, int k, long long e) {
    const int i = (int)(e / k), kk = (int)(e - (long long)i * k);
    const int v = out[sphx_phase_at(kk, npad, i)];
    return v >= 0 ? (long long)v : (long long)n;
}

#if defined(__HIPCC__)
// np.sum over a contiguous row of s < 128 values term(0) .. term(s - 1), in NumPy's order (eight running sums over the
// whole blocks of eight, combined pairwise, then the rest one by one): what Simulation forms mean_grain_mass and
// mean_cross with
template <class Term>
__device__ __forceinline__ double phase_np_sum(int s, Term term) {
    if (s < 8) {
        double res = 0.0;
        for (int t = 0; t < s; ++t) res += term(t);
        return res;
    }
    double r0 = term(0), r1 = term(1), r2 = term(2), r3 = term(3), r4 = term(4), r5 = term(5), r6 = term(6), r7 = term(7);
    int t = 8;
    for (; t < s - (s % 8); t += 8) {
        r0 += term(t); r1 += term(t + 1); r2 += term(t + 2); r3 += term(t + 3);
        r4 += term(t + 4); r5 += term(t + 5); r6 += term(t + 6); r7 += term(t + 7);
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; t < s; ++t) res += term(t);
    return res;
}
#endif
