// sphx_update_rows.h - the two classes of rows of the leapfrog/energy update (integrate_kernel, sphx_integrate.hip).
//
// Where pass 2 hands its rows on (sphx_blob.hip: PiPass::finish) and nothing but pass 3 stands between it and the update,
// it leaves one byte per row: not 0 - pass 3's result for the row is settled (sphx_settled.h: NaN in all four values,
// which the update's nan_to_num turns into 0), 0 - pass 3 sums the row.  Nobody stores a settled row's NaNs, and the update
// does not load them: it puts the value through the same expressions as a constant.  The rules below are host code as
// well: tests/host/update_rows_check.cpp replays them on random byte arrays.
#pragma once
#if defined(__HIPCC__)
#define SPHX_ROWS_HD __host__ __device__
#else
#define SPHX_ROWS_HD
#endif
// whether the row's va / vh come out of memory (else: NaN, what a settled row holds).  by_byte false: the launch has no
// bytes (every other path), every row loads
SPHX_ROWS_HD inline bool sphx_update_loads_visc(bool by_byte, unsigned char settled_byte) {
    return !by_byte || settled_byte == 0;
}
// who leaves the step's dt in *dt_out: thread 0, whatever class its row is of
SPHX_ROWS_HD inline bool sphx_update_writes_dt(int i) { return i == 0; }
