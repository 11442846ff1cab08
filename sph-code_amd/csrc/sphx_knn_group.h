// sphx_knn_group.h - arguments of the lane-per-query grouped search (sphx_knn_group.hip)
#pragma once

// ---- room in the tie list (plain C++: the kernel and a host program that replays reservations both call it) --------
// Each of a query's four lanes reserves its entries with one atomic add on the list's count: slots base .. base + ne - 1.
// The count keeps every reservation, whether it fitted or not, and the tie blocks walk min(count, cap) slots - so EVERY
// reserved slot below cap must be written by the search that reserved it, or the tie blocks apply what an earlier search
// (or nobody) left there.  A lane whose reservation crosses cap fails its query over (all four lanes: the vote in the
// kernel); `certified` is the query's state after that vote.
//   slots base .. base + nwrite - 1: the lane's real entries if `real`, else the sentinel {-1, ..} the tie blocks skip
//   slots from base + nwrite on:     nothing (they lie at or beyond cap)
#if defined(__HIPCC__)
#define KG_HD __host__ __device__
#else
#define KG_HD
#endif
struct KgTieSlots { int nwrite; bool real; };
KG_HD inline bool kg_tie_overflows(int base, int ne, int cap) { return ne > 0 && (base < 0 || base > cap - ne); }
KG_HD inline KgTieSlots kg_tie_slots(int base, int ne, int cap, bool certified) {
    KgTieSlots s;
    const int room = (base < 0 || base >= cap) ? 0 : cap - base;      // (base < 0: the count wrapped - nothing is written)
    s.nwrite = ne < room ? ne : room;
    if (s.nwrite < 0) s.nwrite = 0;
    s.real = certified;
    return s;
}

#ifndef SPHX_KG_TIE_SLOTS_ONLY           // (the host program wants the rule above and nothing of the device library)
#include "sphx_internal.h"

#ifndef KG_TCAP
#define KG_TCAP 1408                     // candidates per group tile after the cull (11 bits of a key name the slot)
#endif
#ifndef KG_RSPREAD
#define KG_RSPREAD 1.5                   // widest radius a group's tile is sized for, in units of the group's smallest
#endif
#define KG_TPRE 3072                     // candidates of the rows of cells before the per-candidate cull (row ids: u16)
#define KG_MAXROWS 512                   // NON-EMPTY rows of cells a group's tile may draw from
#define KG_ROWS_ALL 8192                 // rows of cells (empty ones included) a group's box + radius may span
static_assert(KG_TCAP <= 2048 && KG_TCAP % 64 == 0, "tile slots are named by 11 key bits");

struct KnnGroupArgs {
    int n, k, npad;
    int n_active;              // queries with id >= n_active (ghosts) are skipped
    const double *x, *y, *z;   // cell-sorted positions
    const int* id;
    const int* qorder;         // processing order (nullable: identity)
    const int* cell_start;
    GridParams g;
    const double* rsearch;     // previous h: sorted order, or by id (hint_by_id)
    int hint_by_id;
    double rscale, rbound;
    int* nbr;                  // [k][npad]
    double* h_sorted;          // one of the two
    double* h_by_id;
    int4* tie_list;            // near ties between two consecutive ranks, left to the list-mode launch's tie blocks (nullable: such queries fail over)
    int* tie_count;
    int tie_cap;
    int* fail_list;            // processing slots this kernel could not certify
    int* fail_count;
    u64* counters;
};
int sphx_knn_group(sphx_ctx* ctx, const KnnGroupArgs& a);
#endif  // SPHX_KG_TIE_SLOTS_ONLY
