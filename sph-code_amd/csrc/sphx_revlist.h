// sphx_revlist.h - the two size rules of the side stages' reverse list (sphx_rev_build, sphx_side.hip).
//
// The list lives in one buffer of ints, the entries as the fill kernel left them in front and the sorted ones behind:
//   [0, M)                                  as filled, in the order the atomics handed out
//   [sphx_rev_sorted_at(M), ... + M)        each slice sorted ascending: what the stage reads
// The sorted half starts a multiple of four ints (16 bytes) behind the raw one, at least M; both fit sphx_rev_ints(M).
// An entry is a key in [0, key_end); the segmented radix sort looks at the low sphx_rev_bits(key_end) bits alone.
// The rules are host code as well: tests/host/revlist_check.cpp checks them by brute force.
#pragma once
#include <stddef.h>
#if defined(__HIPCC__)
#define SPHX_REV_HD __host__ __device__
#else
#define SPHX_REV_HD
#endif
// the least b in [1, 32] with 2^b >= key_end
SPHX_REV_HD inline unsigned sphx_rev_bits(unsigned long long key_end) {
    unsigned bits = 1;
    while (bits < 32 && (1ull << bits) < key_end) ++bits;
    return bits;
}
SPHX_REV_HD inline size_t sphx_rev_sorted_at(size_t M) { return (M + 3) & ~size_t(3); }
SPHX_REV_HD inline size_t sphx_rev_ints(size_t M) { return 2 * (M + 4); }
