// sphx_runs.h - runs of equal cell id among the consecutive lanes of a wave (grid_count_fused, sphx_grid.hip).
//
// The state arrives in the previous step's cell order, so the particles of one cell sit in consecutive threads.  A run is
// a maximal stretch of consecutive active lanes with the same cell id; its first lane, the head, adds the run's length
// to the cell's count with ONE atomic, and every lane of the run takes the returned base plus its distance from the head
// as its arrival number.  A run never crosses a wave, and equal cells that are not adjacent in lane order (A B A B) are
// runs of their own.
//   heads:    wave mask of the lanes that begin a run (lane 0 always does); only active lanes vote
//   n_active: the active lanes are lanes 0 .. n_active - 1 (a grid-stride loop's last trip: a prefix of the wave)
// The rule is host code as well: tests/host/grid_runs_check.cpp replays it over random and adversarial waves.
#pragma once
#if defined(__HIPCC__)
#define SPHX_RUN_HD __host__ __device__
#else
#define SPHX_RUN_HD
#endif
struct SphxRun { int head; int len; };                 // the lane that begins this lane's run; the run's length
SPHX_RUN_HD inline SphxRun sphx_run_of_lane(unsigned long long heads, int n_active, int lane) {
    // (heads shifted by the lane number, not masked: a mask per lane is four more registers held across the kernel's loop)
    const unsigned long long below = heads << (63 - lane), above = (heads >> lane) >> 1;
    SphxRun r;
    r.head = below ? lane - __builtin_clzll(below) : 0;                // the nearest head at or below this lane
    const int next = above ? lane + 1 + __builtin_ctzll(above) : n_active;   // the next run's head, or the end of the active lanes
    r.len = next - r.head;
    return r;
}
