// sphx_settled.h - when a row's sum is known to be NaN without (further) summing (blob_pass, sphx_blob.h).
//
// hydro_update's sums carry NaN like any other value: a particle with T < 0 has a NaN sound speed, every Pi that meets
// it is NaN, and every viscous force that meets such a Pi is NaN; the integrator's nan_to_num turns all of
// them into 0.  Two facts of IEEE arithmetic let a pass stop early and still write what the full sum writes - a NaN:
//   pass 3: every term of a row holds Bw_i x c_a (visc_term, sphx_pair.h), and NaN x anything is NaN, 0 and inf
//           included: a row whose own Bw_i is NaN and that has one term at all is settled before its loop.
//   pass 2: x + NaN is NaN, so a partial sum that is NaN stays NaN, and the row's total (p0 + p1) + (p2 + p3) is NaN as
//           soon as one of its partials is: the row is saturated, and only |dv|^2 of the crossing time is still wanted.
// NaN only: x != x.  An infinite value is neither (inf x 0 is NaN, inf x 1 is not: it has to be summed).
// The rules are host code as well: tests/host/settled_check.cpp replays them over every class of double.
#pragma once
#if defined(__HIPCC__)
#define SPHX_SETTLED_HD __host__ __device__
#else
#define SPHX_SETTLED_HD
#endif
// (the comparison, not isnan(): no header, and the same instruction on both sides)
SPHX_SETTLED_HD inline bool sphx_is_nan(double x) { return x != x; }
// pass 3: a row that writes (output index below n_active) and has a first list position - hence at least one term
SPHX_SETTLED_HD inline bool sphx_row_settled(double own_bw, bool has_first, bool writes) {
    return writes && has_first && sphx_is_nan(own_bw);
}
// pass 2: a row is saturated as soon as one of the partial sums of its four lanes is NaN
SPHX_SETTLED_HD inline bool sphx_quad_saturated(bool s0, bool s1, bool s2, bool s3) { return (s0 || s1) || (s2 || s3); }
// ... and a wave goes on in the short form when every live row of it is.  The rule on the wave's lane masks (a row's
// four lanes are one aligned nibble): nan = the lanes whose partial sum is NaN, live = the lanes that sum at all (whole
// rows).  Scalar arithmetic on two 64-bit masks: nothing in the vector unit beside the comparison that gives `nan`.
SPHX_SETTLED_HD inline bool sphx_wave_saturated(unsigned long long nan, unsigned long long live) {
    unsigned long long any = nan | (nan >> 1);               // bit 0 of a nibble: lanes 0 | 1, bit 2: lanes 2 | 3
    any |= any >> 2;                                         // bit 0: any of the four
    const unsigned long long first = 0x1111111111111111ull;  // the first lane of every row
    return (live & first & ~any) == 0ull;
}
