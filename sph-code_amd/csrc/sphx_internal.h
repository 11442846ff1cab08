// sphx_internal.h - shared declarations of libsphx (gfx950 only; no host fallback).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <float.h>
#include <vector>
#include <functional>
#include "../../include/sphx.h"
#include "sphx_agb.h"
#include "sphx_carve.h"

#define SPHX_WAVE 64
#define SPHX_W6_C 1.5666814710608448    /* 315 / (64 pi), nsc:588 */

typedef unsigned long long u64;
typedef unsigned int u32;
struct PinnedLayout;

// ------------------------------------------------------------------------------------------
// device buffer with grow-only capacity
// ------------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    template <class T> T* as() const { return (T*)p; }
};

// Gather records.  What limits the sum passes is the number of distinct cache lines a
// (particle, neighbour) pair touches, so each pass gets ONE dense 64-B record per neighbour
// (two particles per 128-B line: cell-adjacent neighbours share lines) plus, where a ninth
// value is needed, an 8/16-B gather from a compact array (16 / 8 particles per line):
//   pass 1: RecA                      pass 2: RecB + rho_s[j]        pass 3: RecB + bc_s[j]
//   pairwise viscosity (passes 2 + 3 fused, visc_mode 1): RecB + rho_s[j] + bc_s[j].Bw
struct __attribute__((aligned(64))) RecA {
    double x, y, z;   // position
    double h2;        // h_j^2
    double c1;        // 315 / (64 pi h_j^9)                               nsc:588
    double ms;        // +m (gas), -m (dust), 0 (star): m*[t==0], m*[t==2]  nsc:605-606
    double A;         // m/mu/amu*k*T*[t==0]   pressure weight             nsc:615
    double Nw;        // m/mu/amu*[t==0]       number weight               nsc:607,626
};
struct __attribute__((aligned(64))) RecB {
    double x, y, z, h2;
    double vx, vy, vz;
    double cs;        // sqrt(gamma k T/mu/amu [t==0])   neighbour form    nsc:647
};
struct __attribute__((aligned(16))) RecBC {   // pass-3 companion
    double Bw;        // m Pi [t==0], written by pass 2                     nsc:651
                      // (pairwise viscosity: m [t==0] c1, written by sphx_prep)
    double c1;        // 315 / (64 pi h^9)
};
struct __attribute__((aligned(32))) RecSelf { // read only by the owner's thread (coalesced)
    double csi;       // sqrt(gamma k T/(mu amu) [t==0]) own form           nsc:647
    double h;         // smoothing length (crossing time)                   nsc:782
    double mg;        // m [t==0]
    double pad;
};

// the cell pyramid of the tree gravity (sphx_gravity.hip)
#define PYR_MAX 12
struct GravRef { double x, y, z; };
struct Pyr {
    int nlev;                                   // levels 1..nlev exist; level nlev is a single cell
    int nx[PYR_MAX + 1], ny[PYR_MAX + 1], nz[PYR_MAX + 1];
    long long off[PYR_MAX + 1];                 // first record of level l in the pyramid buffer
};

struct GridParams {
    double xmin, ymin, zmin;      // origin of the (robust) grid box
    double cell, inv_cell;
    int nx, ny, nz;
    int ncells;
    float fnx1, fny1, fnz1;       // (float)(nx - 1) ...: kernel arguments cost no VALU conversions
};

// Outlier levels (sphx_grid.hip, sphx_knn.hip): nested cubes around the grid box, each OLEV_N^3 cells, level l reaching
// hmax * 2^l from the box centre along every axis; the particles OUTSIDE the grid box are listed per (level, cell), each in
// the lowest level whose cube holds it (everything beyond the top cube is clamped into its boundary cells).  The grid
// itself still holds every particle (outliers in its boundary cells), so the levels are a second, complete index of
// the outliers only: a far query with a wide search sphere walks a few coarse cells instead of whole faces of the grid.
#define OLEV_N 32
#define OLEV_MAX 20
#define OLEV_MIN_RC 8.0f     // a query outside the box uses the levels when its search radius exceeds this many grid cells
struct OutLevels {
    int L;                   // levels 1..L (0: none built)
    double cx, cy, cz;       // centre of the grid box
    double hmax;             // half of its longest edge
    const int* start;        // [L * OLEV_N^3 + 1]: slice of `list` per (level - 1, cell)
    const int* list;         // storage indices of the outliers
};
// position of a particle relative to the grid box in cell units, exactly as the cell hash computes it (sub, then mul: no
// contraction possible), so "outside" means the same in the grid build, the level build and the search
__device__ __forceinline__ bool sphx_outside_box(const GridParams& g, double x, double y, double z) {
    const double tx = (x - g.xmin) * g.inv_cell, ty = (y - g.ymin) * g.inv_cell, tz = (z - g.zmin) * g.inv_cell;
    return tx < 0.0 || tx >= (double)g.nx || ty < 0.0 || ty >= (double)g.ny || tz < 0.0 || tz >= (double)g.nz;
}

// ---- blob order: the rank of a cell along the space-filling curve (sphx_grid.hip builds the order; the kernel that
// permutes the state, sphx_integrate.hip, can carry its last scatter) ----
struct BlobBits { int bx, by, bz; int hilbert; };
__device__ __forceinline__ unsigned hilbert_rank(unsigned x, unsigned y, unsigned z, int b) {
    // Skilling's transform (axes -> transposed Hilbert index), then the transposed bits interleaved
    unsigned X[3] = {x, y, z};
    const unsigned M = 1u << (b - 1);
    for (unsigned Q = M; Q > 1; Q >>= 1) {
        const unsigned P = Q - 1;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (X[i] & Q) X[0] ^= P;
            else { const unsigned t = (X[0] ^ X[i]) & P; X[0] ^= t; X[i] ^= t; }
        }
    }
    X[1] ^= X[0]; X[2] ^= X[1];
    unsigned t = 0;
    for (unsigned Q = M; Q > 1; Q >>= 1)
        if (X[2] & Q) t ^= Q - 1;
    X[0] ^= t; X[1] ^= t; X[2] ^= t;
    unsigned out = 0;
    for (int q = 0; q < b; ++q) {
        out |= ((X[2] >> q) & 1u) << (3 * q);
        out |= ((X[1] >> q) & 1u) << (3 * q + 1);
        out |= ((X[0] >> q) & 1u) << (3 * q + 2);
    }
    return out;
}
__device__ __forceinline__ unsigned blob_rank(int cx, int cy, int cz, BlobBits b) {
    if (b.hilbert) return hilbert_rank((unsigned)cx, (unsigned)cy, (unsigned)cz, b.hilbert);
    unsigned out = 0;
    int pos = 0;
    for (int q = 0; q < 11; ++q) {
        if (q < b.bx) out |= (unsigned)((cx >> q) & 1) << pos++;
        if (q < b.by) out |= (unsigned)((cy >> q) & 1) << pos++;
        if (q < b.bz) out |= (unsigned)((cz >> q) & 1) << pos++;
    }
    return out;
}

// device-resident particle state, structure of arrays (one set; `alt` is the permute target)
struct StateArrays {
    DevBuf x, y, z, vx, vy, vz, ax, ay, az;      // position, velocity, previous total accel
    DevBuf m, T, mu, gam, E, hprev;              // per-particle scalars
    DevBuf ptype;                                // f64 0/1/2 as in the reference (drv:127)
    DevBuf id;                                   // int32 persistent particle id
    DevBuf fun;                                  // (n,s) f64 composition (optional)
    DevBuf mgm, mcs;                             // mean grain mass / cross-section (drag, optional)
};

// The stage timer of a side call (the arb, rad, cool, dust and chem entry points): events on ctx->stream around its stages -
// four of them, five for chem and the dust phase.  (sphx_api.hip; a call that returns between begin and end leaves ms zeroed)
struct StageTimer {
    int stages = 4;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // created on first use
    double ms[5] = {0, 0, 0, 0, 0};
    int begin(sphx_ctx* ctx);           // creates the events, zeroes ms, records ev[0]
    int mark(sphx_ctx* ctx, int i);     // records ev[i]
    int end(sphx_ctx* ctx);             // ms[i] = ev[i] .. ev[i + 1]; after the call's last synchronise
    // (at delete ctx, behind sphx_destroy's hipSetDevice)
    ~StageTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

#define SPHX_LDS_KERNELS 16           // room in sphx_ctx::lds_raised (the LDS kernels of sphx_blob.hip and sphx_loopforms.hip: 11)

struct sphx_ctx {
    // ======== configuration: read from the environment by sphx_create, or set by sphx_set_* / sphx_state_set_* ========
    int device = 0;
    hipStream_t stream = nullptr;       // stream every launch goes to (own_stream or the caller's: sphx_set_stream)
    hipStream_t own_stream = nullptr;
    hipStream_t side_stream = nullptr;  // independent work beside the main chain (record build while the lists are deduplicated)
    sphx_constants cst;
    char tunables[1024] = {0};          // "NAME=value ..." of every SPHX_* variable sphx_create read (sphx_tunables)
    double rscale = 1.08, cell_factor = 0.55;    // search tuning (sphx_set_tuning)
    double rscale_build = 1.3;          // search radius factor on list-building steps
    bool use_verlet = false;            // opt-in (sphx_set_incremental): pays only for slow drift
    bool use_blob = true;
    int blob_curve = 0;                 // 0: Hilbert where its code space fits, 1: Morton always (SPHX_BLOB_CURVE)
    bool use_group = true;              // hinted searches by the lane-per-query grouped kernel (SPHX_KNN_GROUP=0: off)
    bool use_lds = true;                // run the step loop's passes out of LDS (needs blob order)
    bool drag_lds = true;
    bool blob_split_on = true;
    bool species_lds = true;            // SPHX_SPECIES_LDS=0: the species pass by gathers (sphx_sums.hip) also when blob lists exist
    bool species_fused = true;          // the step's species pass inside pass 1's kernel (SPHX_SPECIES_FUSED=0: a kernel of its own)
    int blob_grid = 0;                  // persistent workgroups of the LDS passes (0: not yet derived)
    int blob_slots = 1 << 20;           // distinct neighbours staged per workgroup (clamped to the image size)
    int olev_mode = 2;                  // SPHX_OUTLIER_LEVELS: 0 never, 1 whenever a particle lies outside the box, 2 auto
    // hint distrust (an experiment kept as an option, off by default): skip the grouped kernel and seed every radius
    // from the local cell counts.  Auto mode enters when the previous hinted search left more than a quarter of its
    // queries to the general kernel (a diverging run: particles move by several h per step) and leaves once fewer than
    // 5 % of the radii found lie beyond [0.5, 1.5] x hint.  Measured on the diverged cube: no faster than the grouped
    // kernel certifying what it can and the list-mode kernel re-seeding the stale hints it meets.
    int distrust_mode = 0;              // SPHX_HINT_DISTRUST: 0 never, 1 always, 2 auto
    bool cell_feedback = true;          // SPHX_CELL_FEEDBACK=0 switches it off: cells shrink while groups' tiles overflow (sphx_api.hip)
    double cell_fb_hi = 0.30, cell_fb_lo = 0.10;     // (SPHX_CELL_FB_HI / _LO)
    int64_t max_cells = 0;              // SPHX_MAX_CELLS: > 0 lowers the limit on grid cells
    double box_sigmas = 3.0;            // the grid covers mean +- this many standard deviations of the positions (SPHX_BOX_SIGMAS)
    double h_clip_factor = 8.0;         // h above this many times the previous mean is left out of the mean that sizes the cells (SPHX_HCLIP)
    double reach_cap = 0.0;             // sphx_dev_set_reach_cap: head-room of a claimed reach limited to this length (0: not)
    bool timing_detail = false;         // per-pass timing events in sphx_step (sphx_set_timing_detail)
    int clip_grad = 0;                  // physics option: neighbour-side gradient clipped beyond h_j (sphx_set_clip_grad)
    int visc_mode = 0;                  // hydro_update-mode viscosity of sphx_step and the sphx_dev_* passes (sphx_set_visc_mode)
    bool drag = false;                  // gas-dust drag enabled in the step loop (sphx_state_set_drag)
    int loop_forms = 0;                 // step mode: the loop forms of the reference's time loop (sphx_state_set_loop_forms)
    double loop_d = 0.0;                // their global d (drv:68)
    int gravity = 0;                    // 1: direct-sum self-gravity each step (sphx_state_set_gravity)
    double grav_G = 0.0;
    int grav_order = 2;                 // multipole order of the tree's cells: 1 monopoles, 2 + second moments (sphx_set_gravity_order)
    bool grav_per_thread = false;       // SPHX_GRAV_KERNEL=0: tree walk per thread instead of per wave through LDS
    int grav_ws = 1;                    // well-separatedness of the tree form (cells)
    // species pass inside the step (nsc:624-627) + per-particle metallicity + fused AGB yields (sphx_state_set_agb)
    bool agb_on = false;
    AgbTable agb;
    double dev_hmean = 0.0;             // device API: mean h of the previous search (cell size; sphx_dev_set_mean_h)

    // ======== state that lives from one C-ABI call to the next ========
    char err[512] = {0};
    sphx_stats stats;
    // ---- working set (any particle order) ----
    int64_t n = 0, npad = 0;
    int k = 0, s = 0;
    int sp = 0;                   // doubles per particle of the resident composition rows: s padded to whole 128-B lines
    bool has_state = false;
    int64_t step_count = 0;
    double dt_last = 0.0;
    // The update writes the new temperatures into alt.T (dead once the state has been permuted) and swaps it with st.T:
    // what is left in alt.T is T at the instant of the step's sums, in the step's sorted order like rho / nden - P_i = n_i
    // k_B T_i of ONE instant at no cost to the step (sphx_state_download_pressure).  (st.T and alt.T are then the same two
    // buffers at the start of every step; the other arrays of st / alt swap roles every step.)
    bool tprev_valid = false;
    // set by sphx_state_insert_rows (sphx_insert.hip): the next sphx_step's first step integrates with no previous
    // acceleration (drv:484-485; then cleared), and rho / nden / vh / F of the last step have the old row count until then
    bool no_old_once = false;
    bool sums_stale = false;
    bool ct_primed = false;             // SC_CT_BITS holds "none yet" (left so by dt_kernel)
    bool recs_pw = false;         // the records sphx_prep built last feed the pairwise viscous pass (sphx_dev_visc_pairwise checks it)
    // the K-major list in `nbr` is the caller-order list of the last array-API call with this shape
    // (a later call may pass neighbor == NULL instead of uploading the same (N, K) int64 array again)
    bool nbr_api_valid = false;
    int64_t nbr_api_n = 0;
    int nbr_api_k = 0;
    // The last sphx_step's own list, for the calls that read it BETWEEN steps (sphx_phase.hip): ctx->nbr, the order of its
    // columns (step_qorder: a copy of qorder as the step left it - other entry points reset qorder itself) and st.id are
    // still what that step wrote.  Set at the end of sphx_step; dropped (sphx_step_list_drop) by everything that rewrites
    // one of the three: sphx_knn with a K-major output, sphx_transpose_nbr, sphx_build_blob_order, sphx_permute_state,
    // sphx_state_upload.
    bool step_list_valid = false;
    const int* step_qorder = nullptr;
    int64_t step_list_n = 0;
    int step_list_k = 0;
    // ---- Verlet refresh (sphx_refresh.hip) ----
    bool list_valid = false;
    int64_t list_n = 0;
    int list_k = 0;
    // ---- the order of the last search ----
    const int* map_perm = nullptr;  // device API: sorted -> caller index (nullptr: identity)
    int map_nactive = 0;            // device API: callers' particles below this are computed
    // Processing order of the step loop: column p of the neighbour list / thread p of a pass works
    // on the particle stored at qorder[p].  Storage stays x-fastest by cell (the search walks rows);
    // the processing order follows the cells along a Morton curve, so a workgroup's particles form
    // a compact blob and share most of their neighbours (sphx_grid.hip: sphx_build_blob_order).
    const int* qorder = nullptr;    // nullptr: identity
    bool blob_lists = false;        // slot lists valid for the current neighbour list
    // decomposed runs: blobs by what they need from other ranks (sphx_blob.hip: blob_dedup_kernel's bclass)
    bool blob_split_valid = false;
    int blob_split_nblk = 0;
    int pass_part = 0;              // which blobs hydro_update's passes and the record build take: 0 all, 1 interior, 2 boundary
    bool loop2_interior_done = false;
    bool dev_ev_pending = false;  // sphx_dev_search recorded ev[1]/ev[2] around its kNN launch: not yet read
    // device-pointer API: drag terms handed to the next sphx_dev_integrate* call (sphx_dev_set_drag_terms)
    const double *dev_drag_on = nullptr, *dev_drag_re = nullptr, *dev_drag_rho = nullptr, *dev_drag_rhod = nullptr;
    // device-pointer API: gravity (n_owned,3) handed to the next sphx_dev_integrate* call (sphx_dev_set_gravity_accel)
    const double* dev_grav = nullptr;
    // ... and what sphx_dev_gravity_build left for _local / _export of the same search (sphx_dev_search clears gx_built)
    bool gx_built = false;
    int64_t gx_n = 0, gx_nowned = 0;
    Pyr gx_py;
    GravRef gx_ref;
    // ---- grid ----
    GridParams grid;
    const double* tbox = nullptr;   // device: TRUE bounding box {min xyz, max xyz} of the last grid build
    double tbox_h[6] = {0, 0, 0, 0, 0, 0};   // host copy of the true bounding box the last grid build knew (may lag a step)
    double clip_lo[3] = {0, 0, 0}, clip_hi[3] = {0, 0, 0};   // statistics window of the robust grid box
    bool clip_valid = false;
    double h_clip = 0.0;            // h above this is left out of the mean that sizes the cells (0: none)
    double cell_scale = 1.0;        // the factor cell_feedback has reached (sphx_cell_feedback)
    // what a grid build or a blob order left for a later call to finish (outputs of sphx_build_grid / sphx_build_blob_order)
    bool cells_unsorted = false;         // the per-cell member sort rides in the blob-order pass
    // the fused step's build (GridBuildOpts::count_curve): cell_scatter has written the curve's counts, and the members'
    // order is finished by the gather that permutes the state (by counting, into perm_fin - swapped with perm there)
    bool curve_counted = false;
    bool order_by_count = false;
    bool blob_scatter_pending = false;   // the blob order's last scatter rides in the state's permutation
    BlobBits blob_scatter_bits;
    const int* blob_scatter_mstart = nullptr;
    // allocations known to be all zero between uses (nullptr: memset first)
    bool bbox_ticket_zeroed = false;
    const void* cell_fill_zeroed = nullptr;   // the cell_fill allocation known to be all zero between grid builds
    const void* mcount_zeroed = nullptr;   // the blob-count allocation known to be all zero (cleaned by the deferred scatter)
    int mcount_zeroed_M = 0;
    const void* fcount_zeroed = nullptr;   // the fail-list allocation whose counter the grid build has zeroed for this step
    int64_t fcount_zeroed_n = 0;
    const void* tie_list_cleared = nullptr;   // the tie-list allocation that was filled with sentinels when it was made
    const int* tie_count_dev = nullptr;    // the last hinted search's tie count (beside the fail count; nullptr: it kept no tie list)
    int tie_cap_last = 0;                  // ... and its tie_cap
    const void* ds_cnt_zeroed = nullptr;
    const void* olev_fill_zeroed = nullptr;
    unsigned lbs_epoch[2] = {0u, 0u};
    // the kernels whose dynamic-LDS limit has been raised on this context's device (sphx_blob.hip: sphx_lds_opt_in)
    const void* lds_raised[SPHX_LDS_KERNELS] = {nullptr};
    int n_lds_raised = 0;
    // ---- what the previous search reported (read a step late) ----
    // outlier levels (see OutLevels): built for a hinted search when the previous one met enough far queries
    OutLevels olev;                 // olev.L == 0: not built for the current grid
    bool olev_ev_valid = false;
    u64 farq_seen = 0;              // SC_FARQ as last read (the counter only grows)
    int64_t farq_last = 0;          // far queries met by the previous hinted search
    int64_t list_len_last = 0;      // queries the previous hinted search left to the general kernel (sizes the list-mode grid)
    bool knn_lag_valid = false;     // knn_lag holds slots the caller of sphx_knn copied out behind the previous search (KnnIn::lag_external)
    u64 knn_lag[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // slots SC_NFAILQ .. SC_KGDBG + 2
    u64 densep_seen = 0;            // SC_DENSEP as last read
    int64_t densep_last = 0;        // particles in cells of >= DENSE_CELL members at the last grid build the host knows of
    u64 crowded_seen = 0;           // SC_CROWDED as last read (the counter only grows)
    int64_t crowded_last = 0;       // cells of 17 .. 512 members at the last grid build the host knows of
    bool distrust = false;          // hint distrust is on for the next search (distrust_mode)
    u64 badhint_seen = 0;
    // ---- timing events of the step loop, and its lagged read-backs ----
    // The fused step loop never waits for the step it is launching: its timing events live in a
    // ring (collected two steps late), and the two host read-backs that size the grid - bounding
    // box statistics and mean h - are taken from the PREVIOUS step's copies (pinned->lag; the grid
    // box only steers performance: out-of-box particles are clamped into the boundary cells, which
    // the search handles exactly).
    bool ev_detail[3] = {false, false, false};
    int ev_has07[3] = {0, 0, 0};        // bit 0 / 1: the slot's step recorded its start / end event
    unsigned ev_pending = 0;            // bit s: ring slot s holds an uncollected step
    // An event record costs the stream ~10 us: where the fused loop records one anyway right behind a read-back's copy
    // (the search's start event behind the box statistics, the side stream's join event behind the h sums), the host
    // waits on that one instead of a record of its own (the alias; nullptr: lag_bev / lag_hev were recorded).
    hipEvent_t lag_balias[2] = {nullptr, nullptr}, lag_halias[2] = {nullptr, nullptr};
    bool lag_bvalid[2] = {false, false}, lag_hvalid[2] = {false, false};
    int64_t lag_bn[2] = {0, 0};
    int lag_bslot = 0, lag_hslot = 0;

    // ======== device resources: buffers (all from sphx_ensure), events, pinned host scratch ========
    std::vector<void*> allocs;    // every live allocation of sphx_ensure: what sphx_destroy frees
    DevBuf rec1, recv;            // RecA[n], RecB[n]
    DevBuf rho_s, bc_s, self_s;   // sorted-order compact arrays: rho[n], RecBC[n], RecSelf[n]
    DevBuf drag_on, drag_re;      // (n,3) dust->gas drag and its scatter-added reaction (nsc:719-742)
    DevBuf need_pyr;              // sphx_dev_need_map: widest claim per coarse cell + the pyramid of maxima over it
    // the composition rows f_un (sp doubles each) in the ORDER OF UPLOAD, never permuted: the species pass reaches a row
    // through the particle's id (128 B per particle and step that the state's permutation does not move - beside the
    // search, where that copy cost the grouped kernel 84 us on the two-phase cloud)
    DevBuf fun_id;
    DevBuf crowded;                              // cells of 17 .. 512 members, listed by blob_count for cell_sort_crowded
    DevBuf loop_side;                            // loop-form pass 1, LDS form: gamma | dust mass | -1 per particle
    DevBuf ds_cnt, ds_start, ds_ent;             // ordered scatter of the reaction (DragScatter)
    DevBuf lrec_a, lrec_v;        // loop-form records (sphx_loopforms.hip)
    DevBuf grav, grav_sort, grav_tmp;   // (n,3) accelerations, sorted h, radix-sort scratch
    DevBuf grav_pyr, grav_cell;         // cell pyramid (mass, centre of mass), fine cell of each sorted particle
    DevBuf grav_quad;
    // gravity between parts (sphx_gravity_tree_parts): all points (AoS) and masses, the particles part by part, sorted ->
    // caller index of the part in hand, the parts' boxes, export flags / counts and their scans, counts per peer
    // (decomposed runs, sphx_dev_gravity_*: gx_pts holds the sorted positions x | y | z, gx_m the sorted masses, ghosts 0)
    DevBuf gx_pts, gx_m, gx_ord, gx_map, gx_box, gx_cflag, gx_coff, gx_pcnt, gx_poff, gx_counts;
    DevBuf list64, dref, pos0, pos4;   // Verlet refresh: int32[n][64], f64[n], f64[3n] positions at list build, f64[4n] packed current
    DevBuf nbr;                   // int32 [k][npad], K-major, -1 = missing
    DevBuf porder, mcount, mstart;      // blob order (qorder points at porder)
    DevBuf agb_knots, Zmet, agb_dust;
    DevBuf fail_list;               // queries the grouped kernel hands to the general one (+ their count)
    DevBuf olev_start, olev_fill, olev_list, olev_key;
    DevBuf lbs_state[2];                   // tile words of the look-back scan (sphx_grid.hip), per launching stream
    DevBuf cell_rank;                       // the particles' arrival numbers in their cells (grid build)
    DevBuf perm_fin;                        // the finished cell order of a build whose members the gather puts in order (then swapped with perm)
    DevBuf tie_list;                       // int4 {query slot, rank, index a, index b}: near ties the grouped search leaves to the list-mode launch's tie blocks
    // sphx_blob.hip: per-workgroup distinct-neighbour lists + 16-bit slot lists for the LDS passes
    DevBuf slot16, uniq;
    // blob_split: int list[nblk] (interior blobs, then boundary blobs), then cnt[3] {interior, boundary, idle}
    DevBuf blob_class, blob_split;
    DevBuf visc_live;             // one byte per blob: pass 2 found a row that pass 3 has to sum (the fused step's hand-over)
    // one byte per row: pass 2 found pass 3's result settled (1) or not (0) - the update's two classes of rows
    // (sphx_update_rows.h); written for every row by every pass 2 that hands on to such an update
    DevBuf row_settled;
    bool visc_rows_unfilled = false;   // the last step's update took its rows by those bytes: ctx->va, ctx->vh hold nothing for its settled rows
    DevBuf rho, rhod, nden, G, Pi, Bw, va, vh, ha, F;
    DevBuf scal;                  // small device scalars: ct bits, dt, counters
    DevBuf cell_of, cell_start, cell_fill, perm, inv, scan_tmp, bbox_tmp;      // grid
    // host-API staging
    DevBuf in_a, in_b, in_c, in_d, in_e, in_f, in_g, in_h, in_i, in_j, out_a, out_b, out_c;
    DevBuf idx64, dist_out, nontriv, h_api;
    // arbitrary-point sampling (sphx_arb.hip): records, wide records, wide flags + offsets, per-cell largest support,
    // query points, their keys / order, sort scratch (list form: the members), per-point sums, outputs, small scalars
    DevBuf arb_rec, arb_wrec, arb_flag, arb_cmax, arb_q, arb_key, arb_tmp, arb_acc, arb_out, arb_red;
    // ... and the geometry of the last grid-form call, in buffers of its own (no other entry point writes them): sorted
    // positions (SoA, 3n), cell_start, perm.  With arb_ball_id != 0 it is the ball of that id (sphx_arb_fields): a later
    // call with the same id, n and m reuses it together with the query points in arb_q and their sorted order in arb_key.
    DevBuf arb_pos, arb_cs, arb_perm;
    int64_t arb_ball_id = 0, arb_ball_n = 0, arb_ball_m = 0;
    GridParams arb_g;
    double arb_tb[6] = {0, 0, 0, 0, 0, 0};
    // events of a call: [0] start, [1] inputs on the device, [2] geometry and records built, [3] sums and gate done, [4]
    // outputs on the host (sphx_arb_last_timing)
    StageTimer arb_t;
    // radiative transfer (sphx_rad.hip), buffers of its own - a call on the resident state touches nothing the step owns:
    // staged inputs, SoA particles, rays + their outputs, the chunks' partial columns, non-star flags / offsets / list +
    // small reductions, per-particle outputs (the flags are scanned by sphx_excl_scan_int, in the grid's scratch)
    DevBuf rad_in, rad_soa, rad_ray, rad_part, rad_gas, rad_out;
    // events of a call: [0] start, [1] inputs on the device and prepared, [2] columns done, [3] spread and deposit done,
    // [4] outputs on the host (sphx_rad_last_timing)
    StageTimer rad_t;
    // The reverse list of rad_cooling, supernova_destruction and chemisputtering_2 (sphx_rev_build, sphx_side.hip: as filled
    // | sorted) and the scratch of its segmented sort: ONE pair for the three stages.  Sound because a stage's list is dead
    // when its *_run returns - the kernels that read it are queued by then, on the one stream every later writer is queued
    // on too, and CoolRes, DustRes and ChemRes carry no pointer into it - and because the stages of a context run strictly
    // one after the other: the dust phase runs sphx_chem_run, then sphx_dust_run; the radiative phase sphx_cool_run alone.
    DevBuf side_rev, side_tmp;
    // rad_cooling (sphx_cool.hip), buffers of its own: staged inputs, the list as given, the particles' records, ints (the
    // K-major list, counts, cursors, flags, slice starts), the rows' table, outputs (the counts are scanned by
    // sphx_excl_scan_int; the reverse list is side_rev)
    DevBuf cool_in, cool_nb, cool_rec, cool_int, cool_tab, cool_out;
    // events of a call: [0] start, [1] inputs on the device, records and list built, [2] rows done, [3] reverse list, gather
    // and epilogue done, [4] outputs on the host (sphx_cool_last_timing)
    StageTimer cool_t;
    // supernova_destruction (sphx_dust.hip), buffers of its own: staged inputs, the list as given, the particles' records,
    // ints (the K-major list, counts, cursors, row flags, slice starts, the accept words), outputs (eight u64 counters, the
    // knots, then the two (n,s) arrays); the reverse list is side_rev
    DevBuf dust_in, dust_nb, dust_rec, dust_int, dust_out;
    double dust_kn[40] = {0};     // the call's knots and slopes on the host (DustKnots, sphx_dust_pair.h), uploaded from here
    // events of a call: [0] start, [1] inputs on the device, records and list built, [2] reverse list sorted, [3] dust pass
    // done, [4] row pass done and outputs on the host (sphx_dust_last_timing)
    StageTimer dust_t;
    // chemisputtering_2 (sphx_chem.hip), buffers of its own: staged inputs and tables, the list as given, the particles'
    // records, ints per particle (the K-major list, dust flags and ordinals, counts, cursors, slice starts), per dust row
    // doubles (gas and reuptake weights, row scalars, new0 and the two generations of clamped sums) and ints (particle of an
    // ordinal, contributes, place of an entry in the reverse list), the first-stage losses per (pair, column), outputs (the
    // counters, num0, the final counts, mass_new, f_un_new, partial sums); the reverse list is side_rev
    DevBuf chem_in, chem_nb, chem_rec, chem_int, chem_row, chem_rowi, chem_first, chem_out;
    double chem_tab[4 * SPHX_MAX_SPECIES] = {0};   // the call's tables on the host, uploaded from here
    // events of a call: [0] start, [1] inputs on the device, records and list built, [2] row passes done, [3] reverse list
    // sorted, [4] rounds done, [5] closing correction done and outputs on the host (sphx_chem_last_timing)
    StageTimer chem_t{5};
    // the dust phase on the resident state (sphx_phase.hip): ints (column of a caller id | dense rows scratch), doubles (the
    // loop-form density, the bookkeeping's outputs and per-particle terms, the chunks' partial sums, the totals).  The
    // gathered inputs go straight into chem_in / dust_in, the translated list into chem_int.
    DevBuf phase_int, phase_out;
    double phase_tab[4 * SPHX_MAX_SPECIES] = {0};   // mu_specie | gamma | grain_mass | sigma_effective on the host, uploaded from here
    // events of a call: [0] start, [1] state gathered and list translated, [2] density, [3] chem, [4] dust, [5] bookkeeping
    // done, state written back and totals on the host (sphx_phase_last_timing)
    StageTimer phase_t{5};
    // the elementwise half of the radiative block (sphx_radphase.hip), buffers of its own: doubles (staged inputs, outputs,
    // the totals' per-particle terms, the chunks' partial sums, the totals), ints (the non-star flags and their scan)
    DevBuf radphase_buf, radphase_int;
    double radphase_tab[3 * SPHX_MAX_SPECIES] = {0};   // the call's three per-species tables on the host, uploaded from here
    // events of a call: [0] start, [1] inputs on the device and the ordinals scanned, [2] the row kernel done, [3] the
    // totals' sums done, [4] outputs on the host (sphx_radphase_last_timing)
    StageTimer radphase_t;
    // the radiative phase on the resident state (sphx_state_rad_phase): doubles (the state gathered into caller order, dense
    // composition rows, every stage's outputs), ints (column of a caller id | the translated list | source and target ids).
    // events: [0] start, [1] gathered, list translated, [2] transfer, [3] ionise + heat, [4] cooling, [5] bookkeeping,
    // write-back, outputs on the host (sphx_state_radphase_last_timing)
    DevBuf radstate_buf, radstate_int;
    double radstate_tab[8 * SPHX_MAX_SPECIES] = {0};
    StageTimer radstate_t{5};
    // supernova_impulse (sphx_sn.hip), buffers of its own: staged inputs, work (keys, histograms, scalars, the selection's
    // masses and their partial sums), the candidates (key, id), outputs (d_vels, true_mass, vel, sel_ids)
    DevBuf sn_in, sn_work, sn_cand, sn_out;
    // events of a star: [0] start, [1] keys, [2] bound, [3] compacted, [4] sorted, [5] walked, [6] kicked; the stages' times
    // are added up over the stars of a call (sphx_sn_last_timing), and so are the counts (SPHX_SN_*)
    hipEvent_t sn_ev[SPHX_SN_STAGES + 1] = {nullptr};
    double sn_ms[SPHX_SN_STAGES] = {0};
    int64_t sn_counts[SPHX_SN_NCOUNT] = {0};
    // the insertion of rows into the resident state (sphx_insert.hip): staged inputs (doubles | ints), the located slots
    // of sphx_state_download_rows and its gathered rows; events: [0] start, [1] inputs on the device, [2] grown, [3] the
    // insert kernel, [4] the search (sphx_insert_last_timing); info: buffers reallocated, rows appended, rows rewritten,
    // rows whose T the clamp moved
    DevBuf ins_in, ins_rows;
    std::vector<double> ins_host;       // the call's inputs packed on the host, uploaded from here
    std::vector<int> ins_ids;           // ... and the sorted ids of the rows to rewrite
    StageTimer ins_t;
    int64_t ins_info[4] = {0, 0, 0, 0};
    // the adaptive length scale and sizes (sphx_scale.hip), buffers of its own: staged inputs of the array calls, work (the
    // keys, one level's histogram, the device scalars), ints (reverse counts | nontrivial counts, u32 each), outputs
    // (sizes, new_smoothing, the counts as int64, each in the caller's order).  On the resident state also: the adapted
    // sizes in STORAGE-SLOT order like st.hprev (scale_sizes; they stand while scale_sizes_valid: until the next search
    // replaces the radii, drv:437) and densities_0 BY PARTICLE ID (scale_d0: it has to survive the next step's re-ordering;
    // dropped by sphx_state_upload and sphx_state_insert_rows, as the driver's length comparison drv:532 drops it).
    // events: [0] start, [1] keys, [2] selected and read back, [3] reverse counts, [4] adapted, [5] outputs on the host
    DevBuf scale_in, scale_work, scale_int, scale_out, scale_sizes, scale_d0;
    bool scale_sizes_valid = false, scale_d0_valid = false;
    StageTimer scale_t{5};
    // the census and the stellar clock (sphx_census.hip), buffers of its own - it only reads the state: staged inputs of the
    // array calls, doubles (the chunks' partial sums | the totals, the largest stellar mass and the four counts | the
    // selections' columns), ints (slot of a particle id | the selection's flags | their scan).  star_ages BY PARTICLE ID
    // like scale_d0 (no part of StateArrays: the step's permutation does not move it); it stands while star_ages_valid:
    // set by sphx_state_set_star_ages, extended by sphx_state_insert_rows, dropped by sphx_state_upload.
    // events: [0] start, [1] inputs on the device / the slot map, [2] the chunk sums, [3] the totals, [4] outputs on the host
    DevBuf census_in, census_buf, census_int, star_ages;
    bool star_ages_valid = false;
    double census_tab[SPHX_MAX_SPECIES] = {0};     // mu_specie on the host, uploaded from here
    StageTimer census_t;
    // the potential calls (sphx_gravity.hip).  gravpot_buf: phi (n) of the array calls; of the resident call phi by id |
    // 1/2 m phi | m (n each) | their chunk sums (2 x chunks) | U, sum m, eps, the count of non-finite phi (4).  The state by
    // particle id is staged in in_b, in_c, in_d, in_h like an array call's input.  The state itself is only read.
    // events: [0] start, [1] inputs on the device and eps, [2] grid and pyramid (tree), [3] the sums, [4] outputs on the host
    DevBuf gravpot_buf;
    StageTimer gravpot_t;
    // the projected maps (sphx_map.hip), buffers of its own - it only reads the state: staged inputs of the array call, the
    // footprints by particle id (SphxMapRec | the tile range, int4), ints (slot of a particle id | counts per tile | their
    // scan | the fill's cursors), the tile lists (as filled | sorted, sphx_revlist.h) and their sort's scratch, outputs (the
    // pair count and the skipped rows, u64 | the images asked for | count, int64)
    // events: [0] start, [1] footprints, [2] counts, scan and the pair count on the host, [3] tile lists filled and sorted,
    // [4] the tile kernel, [5] outputs on the host (sphx_map_last_timing)
    DevBuf map_in, map_rec, map_int, map_rev, map_tmp, map_out;
    StageTimer map_t{5};
    StateArrays st, alt;          // simulation state
    DevBuf badc;                  // failure counters, BADC_BUCKETS x BADC_STRIDE u64 (zeroed at sphx_create / sphx_reset_stats)
    DevBuf scal_tmp;                    // step_scalars_kernel's per-block partials + its ticket
    DevBuf hsum_tmp;                    // hsum_kernel's per-block partial sums + its ticket
    hipEvent_t ev_join = nullptr;
    hipEvent_t ev_perm = nullptr;       // the state's permutation split over the two streams (sphx_permute_state)
    hipEvent_t olev_ev = nullptr;   // recorded behind the copy of SC_FARQ to the host
    hipEvent_t ev[10] = {nullptr};
    hipEvent_t evring[3][10] = {{nullptr}};
    hipEvent_t lag_bev[2] = {nullptr, nullptr}, lag_hev[2] = {nullptr, nullptr};
    PinnedLayout* pinned = nullptr;     // small pinned host scratch for scalar read-back
};

int sphx_set_err(sphx_ctx* ctx, int code, const char* fmt, ...);
// Grow-only: at least `bytes` in b.  Every allocation is entered in ctx->allocs (sphx_destroy frees them all); before an
// outgrown one is freed the host waits for `in_use_on`, the stream whose queued work may still read it.
int sphx_ensure(sphx_ctx* ctx, DevBuf& b, size_t bytes, hipStream_t in_use_on);
static inline int sphx_ensure(sphx_ctx* ctx, DevBuf& b, size_t bytes) { return sphx_ensure(ctx, b, bytes, ctx->stream); }
void sphx_release(sphx_ctx* ctx, DevBuf& b);      // frees b's allocation now (the caller knows it idle)
// The keeping variant: at least `bytes` in b with its first `keep` bytes as they were (copied on ctx->stream); an outgrown
// allocation goes to `retired`, which sphx_free_retired frees behind the stream; *grown counts the reallocations.
int sphx_ensure_keep(sphx_ctx* ctx, DevBuf& b, size_t bytes, size_t keep, std::vector<void*>& retired, int* grown);
int sphx_free_retired(sphx_ctx* ctx, std::vector<void*>& retired);
// drv:386 on the grown resident state (sphx_api.hip; called by sphx_state_insert_rows)
int sphx_step_research(sphx_ctx* ctx, int k, double dist);

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return sphx_set_err(ctx, SPHX_E_HIP, "%s:%d %s -> %s", __FILE__, __LINE__,       \
                                #expr, hipGetErrorString(e_));                               \
    } while (0)
#define NEED(p)                                                                              \
    do {                                                                                     \
        if (!(p)) return sphx_set_err(ctx, SPHX_E_ARG, "%s: argument %s is NULL", __func__, #p); \
    } while (0)
#define SPHX_TRY(expr)                                                                       \
    do {                                                                                     \
        int r_ = (expr);                                                                     \
        if (r_ != SPHX_OK) return r_;                                                        \
    } while (0)

// A buffer of several arrays (sphx_carve.h): at least the layout's bytes in b, then every piece's pointer written.
template <int CAP> static inline int sphx_carve_into(sphx_ctx* ctx, DevBuf& b, const CarveN<CAP>& c) {
    if (c.overflowed()) return sphx_set_err(ctx, SPHX_E_ARG, "a buffer layout of more than %d pieces", CAP);
    SPHX_TRY(sphx_ensure(ctx, b, c.bytes()));
    c.bind(b.p);
    return SPHX_OK;
}
// Device time of the stages of a family's last call on this context, from HIP events on its stream.
static inline int last_timing(sphx_ctx* ctx, StageTimer sphx_ctx::*t, double* ms) {
    if (!ctx || !ms) return SPHX_E_ARG;
    for (int i = 0; i < (ctx->*t).stages; ++i) ms[i] = (ctx->*t).ms[i];
    return SPHX_OK;
}

static inline void sphx_step_list_drop(sphx_ctx* ctx) { ctx->step_list_valid = false; ctx->step_qorder = nullptr; }
static inline int64_t sphx_pad64(int64_t n) { return (n + 63) & ~int64_t(63); }
// workgroups of wg lanes that cover `lanes` lanes
static inline unsigned sphx_blocks(size_t lanes, unsigned wg) { return (unsigned)((lanes + wg - 1) / wg); }
// neither NaN nor inf
__host__ __device__ __forceinline__ bool sphx_finite(double v) { return v - v == 0.0; }
// an entry of a caller's (n,k) int64 neighbour list as the K-major int32 lists hold it: outside [0, n) it is missing
__device__ __forceinline__ int sphx_list_entry64(long long q, int n) { return (q >= 0 && q < n) ? (int)q : -1; }

// XCD-aware block remap: workgroups are dealt round-robin over the 8 XCDs (block b runs on
// XCD b % 8, each with its own 4 MiB L2).  Map the blocks of one XCD onto one CONTIGUOUS
// chunk of the (cell-sorted) particle range so an XCD's L2 only ever sees its own spatial
// slab plus a halo.  Bijective for any grid size; affects speed only.
__device__ __forceinline__ int xcd_block(int b, int nb) {
    const int q = nb >> 3, r = nb & 7, x = b & 7, s = b >> 3;
    return x * q + (x < r ? x : r) + s;
}
// ... and the block that xcd_block maps to position p of the range
__device__ __forceinline__ int xcd_block_inv(int p, int nb) {
    const int q = nb >> 3, r = nb & 7, head = r * (q + 1);
    const int x = p < head ? p / (q + 1) : r + (p - head) / q;       // (p >= head only where q > 0)
    const int s = p < head ? p % (q + 1) : (p - head) % q;
    return s * 8 + x;
}

// Every neighbour sum is kept as this many partial sums over the list positions k mod SPHX_SUM_PARTS,
// combined as (p0 + p1) [+ (p2 + p3)]: one fixed order for the gather kernels (sphx_sums.hip) and the
// lanes-per-particle split of the LDS kernels (sphx_blob.hip), so all variants agree bit for bit.
#ifndef SPHX_SUM_PARTS
#define SPHX_SUM_PARTS 4
#endif

// np.nan_to_num of one value (drv:233-238, 460-463, 490-491; nsc:783)
__device__ __forceinline__ double sphx_nan_to_num(double v) {
    if (v != v) return 0.0;
    if (v > DBL_MAX) return DBL_MAX;
    if (v < -DBL_MAX) return -DBL_MAX;
    return v;
}

// "no gas particle has voted a crossing time yet": the bits of +inf.  Votes are nan_to_num'ed
// (at most DBL_MAX = 0x7FEF...), so no vote can produce it and atomicMin on the bits keeps any vote.
#define SPHX_CT_NONE 0x7FF0000000000000ull
int sphx_prime_ct(sphx_ctx* ctx, u64* ct_bits);      // writes SPHX_CT_NONE on the context's stream

// scalar slots in ctx->scal (8-byte units)
enum {
    SC_CT_BITS = 0,   // u64: min crossing time (bits of a positive double)
    SC_DT = 1,        // f64: time step
    SC_CAND = 2,      // u64: candidate evaluations
    SC_RETRY = 3,     // u64: retried searches
    SC_HSUM = 4,      // f64: sum of h (for the next grid's cell size)
    SC_DISP2 = 5,     // u64: bits of the max squared displacement since the Verlet list was built
    SC_NFAIL = 6,     // u64: particles whose refreshed kNN could not be proven exact
    SC_HCNT = 7,      // f64: number of h values in SC_HSUM
    SC_GRAV_EPS = 8,  // f64: gravitational softening = median(h) of this step (nsc:358)
    SC_NFAILQ = 9,    // u32: queries of the last hinted search left to the general kernel
    SC_SHORT = 10,    // u64: searches that gave up (KNN_MAX_TRIES radii) with fewer than K neighbours although more exist
    SC_FARQ = 11,     // u64, only grows: queries outside the grid box with a search sphere wider than OLEV_MIN_RC cells
    SC_BADHINT = 12,  // u64, only grows: hinted queries (distrust mode) whose radius came out beyond [0.5, 1.5] x the hint
    SC_CROWDED = 13,  // u64, only grows: cells of 17 .. 512 members met by blob_count (sorted by a launch of their own when many)
    SC_DENSEP = 14,   // u64, only grows: particles in cells of >= DENSE_CELL members (a tile's 27 such cells overflow it)
    SC_KGDBG = 16,    // u64[8]: grouped search, queries handed on by reason (diagnostics)
    SC_SETTLED = 24,  // u64[3]: blobs pass 3 did not walk, waves of pass 2 that saturated, launches of pass 3 that found no
                      //         blob to walk (BLOB_CNT_*; since sphx_reset_stats)
    SC_NSLOTS = 27
};

// Failure counters (the reference's only guard is the nan_to_num of drv:233-238, 460-463, 490-491), u64 and
// only growing, counted by ballot where the values are in registers anyway: one atomic per wave that saw any.  Under
// hydro_update's sums EVERY particle is counted from the second step on (T < 0), so the counts are spread over
// BADC_BUCKETS cache lines by wave - 31 000 atomics per step on ONE address cost the update kernel 0.33 ms (measured), on 64
// lines nothing - and added up on the host (ctx->badc: [bucket][BADC_STRIDE] u64).
enum {
    BAD_ACCEL = 0,   // pressure / viscous / drag acceleration NaN or inf before drv:460-463's nan_to_num (rho_i = 0 or NaN, T_j < 0 ...)
    BAD_ENERGY = 1,  // E or heat x dt NaN or inf before drv:490's nan_to_num
    BAD_STATE = 2,   // updated position or velocity NaN or inf (the next step's clamp, drv:233-238, catches them)
    BAD_H = 3,       // kNN radius 0 (coincident points), NaN or inf
    BADC_BUCKETS = 64, BADC_STRIDE = 16
};
int sphx_badc_read(sphx_ctx* ctx);          // sums the buckets into ctx->stats.bad_* (waits for the stream)

// ---- ctx->pinned: who reads back what, and where (host code only) ------------------------------------
// What a side call (arb / rad / cool / dust / chem) reads back beside its reduction: the reduction's 32 bytes, a 4-byte count, arb's
// candidate counter.
struct PinnedSide { double red[4]; int count; int pad_[7]; u64 cand; };
struct PinnedLag {
    double box[32];           // a grid build's box statistics (sphx_grid.hip: BB_OUT doubles)
    double hs[32];            // SC_HSUM .. SC_KGDBG + 2: the h sums and the search's counters behind them
};
#define SPHX_CENSUS_PIN (13 + 3 * SPHX_MAX_SPECIES + 1 + 4 + 2)
struct PinnedLayout {
    // Read-backs the launching call itself waits for: sphx_step's scalar slots, a synchronous box reduction, the Verlet
    // refresh's and rad_cooling's counts (scal), the side calls' tuples (side).  side.count and side.cand lie INSIDE the
    // scalar block's bytes.  That is safe only because a step call and a side call never have copies in flight together:
    // each waits for its own copies before it returns, and a context serves one call at a time.
    union {
        u64 scal[SC_NSLOTS];
        PinnedSide side;
    };
    char pad0_[256 - SC_NSLOTS * 8];
    double hsum[4];           // SC_HSUM .. of a step that has no lagged copy to size its cells from
    char pad1_[1024 - 256 - 4 * 8];
    PinnedLag lag[2];         // the fused loop's lagged read-backs (lag_bslot / lag_hslot say which is current)
    char pad2_[3072 - 1024 - 2 * 512];
    u64 knn_lag[10];          // SC_NFAILQ .. SC_KGDBG + 2, copied out behind a hinted search (sphx_knn.hip)
    // the projected maps' read-back (sphx_map.hip): the pair count in 64 bits, the skipped rows, the scan's total
    u64 map[4];
    char pad3_[4096 - 3072 - 10 * 8 - 4 * 8];
    // the census' read-back (sphx_census.hip): 13 + 3 s totals, the largest stellar mass, four counts; a selection's count
    u64 census[SPHX_CENSUS_PIN];
    char pad4_[8192 - 4096 - SPHX_CENSUS_PIN * 8];
    u64 badc[BADC_BUCKETS * BADC_STRIDE];      // the failure buckets (sphx_badc_read)
};
static_assert(sizeof(PinnedLayout) == 16384, "ctx->pinned is 16 KiB");
static_assert(offsetof(PinnedLayout, side) == 0 && offsetof(PinnedSide, count) == 32 && offsetof(PinnedSide, cand) == 64 &&
                  offsetof(PinnedLayout, hsum) == 256 && offsetof(PinnedLayout, lag) == 1024 && sizeof(PinnedLag) == 512 &&
                  offsetof(PinnedLag, hs) == 256 && offsetof(PinnedLayout, knn_lag) == 3072 && offsetof(PinnedLayout, census) == 4096 &&
                  offsetof(PinnedLayout, badc) == 8192,
              "the offsets in use since the members were byte counts");
#define SPHX_PIN_APART(a, b) \
    static_assert(offsetof(PinnedLayout, a) + sizeof(PinnedLayout::a) <= offsetof(PinnedLayout, b), #a " overlaps " #b)
SPHX_PIN_APART(scal, hsum); SPHX_PIN_APART(side, hsum); SPHX_PIN_APART(hsum, lag); SPHX_PIN_APART(lag, knn_lag);
SPHX_PIN_APART(knn_lag, map); SPHX_PIN_APART(map, census); SPHX_PIN_APART(census, badc);
#undef SPHX_PIN_APART
static_assert(offsetof(PinnedLayout, badc) + sizeof(PinnedLayout::badc) == sizeof(PinnedLayout), "the buckets end the block");

// Copies of whole f64 arrays between host and device on ctx->stream, from a small table (sphx_api.hip).
struct CopyF64 { const void* host; const void* dev; size_t count; };       // count in doubles
int sphx_upload_f64(sphx_ctx* ctx, const CopyF64* t, int nt);      // skips an entry whose host pointer is NULL
int sphx_download_f64(sphx_ctx* ctx, const CopyF64* t, int nt);    // skips an entry with a NULL pointer or a count of 0

// ---- kernel launch wrappers (defined in the .hip files) ---------------------------------
// grid
int sphx_bbox(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z,
              double out_minmax[13], bool use_clip);
int sphx_median(sphx_ctx* ctx, int64_t n, const double* v, double* out_dev);
int sphx_gravity_launch(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z, int ps,
                        const double* m, const double* eps_dev, double eps, double G, const int* omap,
                        double* acc);
int sphx_gravity_tree_launch(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z,
                             const double* m, int ws, const double* eps_dev, double eps, double G, const int* omap,
                             double* acc);
// the direct sum with the potential beside it (pot (n), J/kg, at omap[i] or i; acc may then be NULL).  pot == NULL: the
// call above, kernel for kernel.
int sphx_gravity_pot_launch(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z, int ps,
                            const double* m, const double* eps_dev, double eps, double G, const int* omap,
                            double* acc, double* pot);
int sphx_dev_collect(sphx_ctx* ctx);
int sphx_loop_step_sums(sphx_ctx* ctx, int64_t n, int k, double d);
// defer_scatter: the order's last scatter is left to the kernel that permutes the state next (sphx_permute_state finds
// it in ctx->blob_scatter_pending / _bits / _mstart)
int sphx_build_blob_order(sphx_ctx* ctx, int64_t n, bool defer_scatter = false);
// the factor on the cell size for the next grid over n particles (cell_scale, moved one step by the last known dense share)
static inline double sphx_cell_feedback(sphx_ctx* ctx, int64_t n) {
    if (ctx->cell_feedback && n > 0) {
        const double dense = (double)ctx->densep_last / (double)n;
        if (dense > ctx->cell_fb_hi) ctx->cell_scale = ctx->cell_scale * 0.97 > 0.35 ? ctx->cell_scale * 0.97 : 0.35;
        else if (dense < ctx->cell_fb_lo) ctx->cell_scale = ctx->cell_scale * 1.01 < 1.0 ? ctx->cell_scale * 1.01 : 1.0;
    }
    return ctx->cell_scale;
}
int sphx_blob_translate(sphx_ctx* ctx, int64_t n, int k);
// lean: the pressure term itself (G; hydro_update returns G / rho in ha) is not stored
int sphx_blob_density_species(sphx_ctx* ctx, int64_t n, int k, bool lean, int S, const double* fun, const int* row_of,
                              const double* m_sorted, double* F, double* Z, double* agb, int agb_on);
int sphx_blob_density(sphx_ctx* ctx, int64_t n, int k, bool lean);
int sphx_blob_pi(sphx_ctx* ctx, int64_t n, int k, u64* ct_bits, bool hand_on, bool row_bytes);
int sphx_blob_visc(sphx_ctx* ctx, int64_t n, int k, const double* m, bool handed);
int sphx_blob_visc_pw(sphx_ctx* ctx, int64_t n, int k, const double* m, u64* ct_bits);
int sphx_blob_species(sphx_ctx* ctx, int64_t n, int k, int S, const double* fun, const int* row_of, const double* m_sorted, double* F,
                      double* Z, double* agb, int agb_on);
// Member order inside a cell (sphx_grid.hip; the counting form of sphx_integrate.hip's gather): ascending index up to
// CELL_SORT_WAVE members - one lane's insertion sort up to CELL_SORT_SERIAL, the whole wave beyond - arrival order above.
#define CELL_SORT_SERIAL 16
#define CELL_SORT_WAVE 512
// the host's cues SC_CROWDED / SC_DENSEP of the current grid, one thread per cell on `stream` (what blob_count adds up
// on the way where it runs)
int sphx_cell_cues(sphx_ctx* ctx, hipStream_t stream);
// the gather's order-finishing part alone (no array moved), for sphx_selftest_grid_order
struct OrderFinish {
    int n;
    GridParams g; BlobBits b;
    const int *perm_in, *cell_of, *cell_start, *mstart;
    int *perm_out, *porder, *mcount;
};
int sphx_finish_order_only(sphx_ctx* ctx, const OrderFinish& o);
struct GridBuildOpts {
    // the grid is sized from the previous build's box statistics, already on the host; this build's are copied out for
    // the next one (the fused loop, sphx_dev_search): the host never waits for the step it launches
    bool lagged = false;
    // lagged: an event the caller records on the stream a few launches on (before the search); the host then waits on it
    // for this build's statistics instead of on a record of the build's own (nullptr: the build records lag_bev)
    hipEvent_t alias_ev = nullptr;
    // the per-cell member sort is left to sphx_build_blob_order, which the caller runs next (ctx->cells_unsorted says so)
    bool sort_cells_later = false;
    // with sort_cells_later, from the fused step only: the caller runs sphx_build_blob_order(defer_scatter = true) and
    // sphx_permute_state next.  Where the count kernel kept the arrival numbers and the curve's code space fits, the
    // scatter then writes the curve's counts and the gather orders the members: no pass over the cells (ctx->curve_counted)
    bool count_curve = false;
    // set (all three, vx vy vz): drv:233-238 is applied to ctx->st - positions and these velocities - by the build's first pass
    double* clamp_vel[3] = {nullptr, nullptr, nullptr};
};
int sphx_build_grid(sphx_ctx* ctx, int64_t n, int k, const double* x, const double* y, const double* z, double cell_hint,
                    const GridBuildOpts& opts = GridBuildOpts());   // fills grid, cell_start, perm
// What a grid build between two steps changes on the host side of the context (and map_perm / qorder, which its caller
// clears for it): sphx_state_sample saves it, builds a grid of its own, and puts it back (sphx_grid.hip).
struct GridHostState {
    GridParams grid;
    const double* tbox;
    double tbox_h[6], clip_lo[3], clip_hi[3], cell_size;     // (olev_L: olev.L; cells, cell_size: stats.cells, stats.cell_size)
    bool clip_valid, cells_unsorted;
    int olev_L;
    int64_t cells;
    const int *map_perm, *qorder;
};
GridHostState sphx_grid_host_save(const sphx_ctx* ctx);
void sphx_grid_host_restore(sphx_ctx* ctx, const GridHostState& saved);
int sphx_excl_scan_int(sphx_ctx* ctx, const int* in, int* out, int n);   // out[0..n] = exclusive prefix sums, out[n] = total (in[n] must be 0)
// The drag reaction (nsc:741: every particle adds -f to each of its dust neighbours) as an ORDERED scatter: the
// contributions to a particle are first laid side by side (slices from a count + scan), then added in the order the
// reference's np.add.at adds them - by source particle (caller index), then list position - so the sum is the same bits on
// every run, and the reference's.  sphx_drag_scatter_plan: count + scan; the drag kernels fill; sphx_drag_scatter_reduce adds.
// (an entry is one aligned 32-byte record - key and the three components leave in one piece: written as four scattered
//  8-byte stores, the fill cost four memory sectors per reference)
struct alignas(32) DragEntry { u64 key; double x, y, z; };
struct DragScatter { int* cnt; const int* start; DragEntry* ent; };
__device__ __forceinline__ void sphx_drag_put(const DragScatter& sc, int slot, u64 key, double x, double y, double z) {
    double2* q = reinterpret_cast<double2*>(sc.ent + slot);
    q[0] = make_double2(__longlong_as_double((long long)key), x);
    q[1] = make_double2(y, z);
}
int sphx_drag_scatter_plan(sphx_ctx* ctx, int64_t n, int k, const int* nbr, const double* ptype, const int* qorder, DragScatter* out,
                           bool blob = false);
int sphx_drag_scatter_reduce(sphx_ctx* ctx, int64_t n, const DragScatter& d, double* react);
// the step's drag pass on the blob lists (sphx_blob.hip): count_only = the counting pass of the scatter plan
int sphx_blob_drag(sphx_ctx* ctx, int64_t n, int k, bool count_only, const double* m, const double* ptype, const double* mgm,
                   const double* mcs, const int* id, double* onto, const DragScatter& sc);
int sphx_build_outlier_levels(sphx_ctx* ctx, int64_t n, const double* xs, const double* ys, const double* zs);   // (sorted order)
// knn
struct KnnIn {
    const double *xs, *ys, *zs;          // positions in cell-sorted order
    const int32_t* id;                   // sorted -> caller index
    const int32_t* inv = nullptr;
    const double* rsearch = nullptr;     // search-radius hints (nullable)
    double rscale = 1.0, rbound = 0.0;
    bool hinted = false;                 // rsearch holds real previous radii: the grouped kernel may trust them
    bool hint_by_id = false;             // rsearch is in caller order
    // the caller copies SC_NFAILQ .. SC_BADHINT out behind the search and hands them back (ctx->knn_lag, knn_lag_valid)
    bool lag_external = false;
};
struct KnnOut {
    int32_t* nbr;       // [k][npad] sorted indices (nullable)
    int32_t* list64 = nullptr;   // [n][64] Verlet candidate list (nullable)
    double* dref = nullptr;      // [n] exclusion radius of list64 (nullable)
    double* h_sorted;   // [n] in sorted order (nullable)
    int64_t* idx64;     // (n,k) by id (nullable)
    double* dist;       // (n,k) by id (nullable)
    int64_t* nontriv;   // (n,) by id (nullable)
    double* h_by_id;    // (n,) by id (nullable)
};
int sphx_knn(sphx_ctx* ctx, int64_t n, int k, const KnnIn& in, const KnnOut& out);
// sums
struct PrepIn {
    const double *x, *y, *z; int ps;       // position pointers + element stride (1 SoA, 3 AoS)
    const double *vx, *vy, *vz; int vs;
    const double *m, *h, *T, *mu, *gam, *ptype;
    void pos_aos(const double* p) { x = p; y = p + 1; z = p + 2; ps = 3; }
    void vel_aos(const double* v) { vx = v; vy = v + 1; vz = v + 2; vs = 3; }
};
// the records of every pass from `in`, launched on `stream`; pairwise: they feed the pairwise viscous pass (RecBC.Bw)
int sphx_prep(sphx_ctx* ctx, int64_t n, const PrepIn& in, bool pairwise, hipStream_t stream);
int sphx_pass_density(sphx_ctx* ctx, int64_t n, int k, bool lean = false);      // lean: G is not stored
// hand_visc (both or neither; the fused single-GPU step with the LDS passes): pass 2 writes the rows of pass 3 that are
// settled (sphx_settled.h) and marks the blobs that hold another; pass 3 walks those alone.  Ignored by the gather kernels.
bool sphx_blob_can_hand_visc(sphx_ctx* ctx, int64_t n);
int sphx_blob_size_marks(sphx_ctx* ctx, int64_t n, bool row_bytes);    // ctx->visc_live (and ctx->row_settled), which pass 2 then writes
int sphx_pass_pi(sphx_ctx* ctx, int64_t n, int k, const double* h, const double* ptype, bool hand_visc = false, bool row_bytes = false);
int sphx_pass_visc(sphx_ctx* ctx, int64_t n, int k, const double* m, bool hand_visc = false);
int sphx_pass_visc_pw(sphx_ctx* ctx, int64_t n, int k, const double* m);   // passes 2 + 3 fused, visc_mode 1
int sphx_pass_species(sphx_ctx* ctx, int64_t n, int k, int s, const double* fun, double* F);
int sphx_step_species(sphx_ctx* ctx, int64_t n, int k);
// fun: composition rows; row_of (nullable: identity): the row of sorted particle j is fun + row_of[j] * SP
int sphx_species_on(sphx_ctx* ctx, int64_t n, int k, int S, int SP, const double* fun, const int* row_of, const double* m_sorted,
                    double* F, double* Z, double* agb);
int sphx_agb_table_set(sphx_ctx* ctx, int S, int nspl, const int32_t* ntx, const int32_t* nty, const double* tx, const double* ty,
                       const double* coeffs, const int32_t* mapto, double divisor, const double* mu_specie, double solar_mass);
int sphx_transpose_nbr(sphx_ctx* ctx, int64_t n, int k, const int64_t* nb_rowmajor);

// the loop-form density (nsc:693-702) on device inputs: points (n,3), the K-major list (sphx_loopforms.hip; sphx_density's kernel)
int sphx_loop_density_dev(sphx_ctx* ctx, int64_t n, int k, const int* nbr, const double* points, const double* mass,
                          const double* ptype, double d, double m_0, double* out);
// crossing_time (nsc:776-786) on device inputs: velocities (n,3), sizes, ptype (n), a K-major list; *ct_bits is primed, then
// holds the votes' minimum; sphx_loop_ct_value turns it into the function's return value (sphx_loopforms.hip)
int sphx_loop_ct_dev(sphx_ctx* ctx, int64_t n, int k, const int* nbr, const double* velocities, const double* sizes, const double* ptype,
                     u64* ct_bits);
double sphx_loop_ct_value(const sphx_ctx* ctx, u64 bits);
// ---- the middle parts of chemisputtering_2 and supernova_destruction, on device inputs (sphx_chem.hip, sphx_dust.hip) ----
struct ChemDev { double *pos, *m, *mu, *sizes, *T, *ptype, *fun, *tab; };       // (n,3), (n,) x 5, (n,s), the tables (4 s)
struct ChemPar { double d, dt, k_B, m_0, symax; };
struct ChemRes { double *mass_new, *fun_new; unsigned long long* counters; unsigned long long hc[8]; size_t M; int64_t rounds; };
int sphx_chem_check_shape(sphx_ctx* ctx, const char* who, int64_t n, int k, int s);
int sphx_chem_check_scalars(sphx_ctx* ctx, const char* who, double d, double dt, const double mrn[2], double k_B, double amu, double m_0);
int sphx_chem_tables(sphx_ctx* ctx, const char* who, int s, const double* mu_specie, const double* mineral_densities,
                     const double* sputtering_yields, const double mrn[2], double amu, double* symax_out);
struct ChemInts { int *nbr, *isd, *ord, *cnt, *cur, *start, *end; };            // ctx->chem_int; end: behind the last block
int sphx_chem_ints(sphx_ctx* ctx, int64_t n, int k, ChemInts* out);
int sphx_chem_inputs(sphx_ctx* ctx, int64_t n, int s, ChemDev* in);
int sphx_chem_run(sphx_ctx* ctx, const char* who, int64_t n, int k, int s, const ChemDev& in, const int* nbr, const ChemPar& par,
                  StageTimer* t, ChemRes* res);
void sphx_chem_counts(sphx_ctx* ctx, ChemRes* res, int64_t* counts);
struct DustDev { double *pos, *vel, *m, *mu, *sizes, *dens, *ptype, *fun; };    // (n,3) x 2, (n,) x 5, (n,s)
struct DustPar { double crit_mass, crit_density, amu; unsigned sel, si; int fraction; };
struct DustRes { double *destr, *reup; unsigned long long* counters; };
int sphx_dust_check_shape(sphx_ctx* ctx, const char* who, int64_t n, int k, int s);
int sphx_dust_check_scalars(sphx_ctx* ctx, const char* who, double crit_mass, double critical_density, int guard_mode);
int sphx_dust_params(sphx_ctx* ctx, const char* who, int s, double crit_mass, double critical_density, const int32_t* species_curve,
                     const double knots_v[8], const double knots_c[8], const double knots_si[8], int guard_mode, DustPar* par);
int sphx_dust_inputs(sphx_ctx* ctx, int64_t n, int s, DustDev* in);
int sphx_dust_run(sphx_ctx* ctx, const char* who, int64_t n, int k, int s, const DustDev& in, const int* nbr_given, const DustPar& par,
                  StageTimer* t, DustRes* res);

// ---- the middle parts of rad_transfer and rad_cooling on device inputs, for the resident radiative phase (sphx_rad.hip, sphx_cool.hip) ----
struct RadDevOut { double *lf2, *ext, *mom; int64_t ng; };                       // (ng), (ng), (ng,3) in ctx->rad_out; NULL when ng = 0
int sphx_rad_run_dev(sphx_ctx* ctx, const char* who, int64_t n, const double* x, const double* y, const double* z, const double* m,
                     const double* ptype, const double* sizes, const double* cross, const double* mu, int64_t n_src,
                     const double* src_dev, const double* lum_host, int64_t n_dst, const double* dst_dev, double dt, int mode,
                     RadDevOut* out);
struct CoolDev { const double *pos, *pt, *m, *mu, *T, *fun; };                   // (n,3), (n,) x 4, (n,s)
struct CoolRes { double *final_comp, *energy, *rec_array, *tab; };               // (n,s), (n), (s,n), (n,6)
int sphx_cool_check(sphx_ctx* ctx, const char* who, int64_t n, int k, int s, double dt, double d);
int sphx_cool_run(sphx_ctx* ctx, const char* who, int64_t n, int k, int s, const CoolDev& in, const long long* nb64, const int* kmajor,
                  double dt, double d, StageTimer* t, CoolRes* res);
// ---- supernova_impulse on device inputs (sphx_sn.hip) ----
// the outputs on the device (in ctx->sn_out, cap rows), the selections' sizes on the host; total: the rows they hold together
struct SnRes { double *d_vels, *true_mass, *vel; long long* sel_ids; std::vector<int64_t> sel_count; int64_t total; };
int sphx_sn_check(sphx_ctx* ctx, const char* who, int64_t n, int64_t n_sn, const int64_t* supernova_pos, double mass_displaced, int64_t cap);
int sphx_sn_run(sphx_ctx* ctx, const char* who, int64_t n, const double* pos, const double* mass, const double* ptype, int64_t n_sn,
                const int64_t* supernova_pos, double mass_displaced, double kick_energy, double* velocities, int64_t cap, SnRes* res);
// ---- shared by the side stages (sphx_side.hip) ----
// the reverse list of a stage: M entries, each slice sorted, valid until the next sphx_rev_build on the context
struct RevList { size_t M; const int* rev; };
int sphx_rev_build(sphx_ctx* ctx, const char* who, int64_t n, const int* cnt, int* start, size_t pairs, unsigned long long key_end,
                   const std::function<void(const int* start, int* rev_raw)>& fill, RevList* out);
// its second half for a caller that has scanned its counts and checked the total M on the host itself: the fill and the
// sort of every slice, into buffers the caller names (rev: sphx_rev_ints(M) ints, tmp: the sort's scratch)
int sphx_rev_fill_sort(sphx_ctx* ctx, int64_t n, const int* start, size_t M, unsigned long long key_end,
                       const std::function<void(const int* start, int* rev_raw)>& fill, DevBuf& rev, DevBuf& tmp, RevList* out);
// the sums over n particles of nq per-particle terms pp (nq, n), in a fixed order, queued into ctx->pinned->scal
#define SPHX_TOT_CHUNK 256
static inline size_t sphx_tot_chunks(int64_t n) { return ((size_t)n + SPHX_TOT_CHUNK - 1) / SPHX_TOT_CHUNK; }
int sphx_ordered_totals(sphx_ctx* ctx, int64_t n, int nq, const double* pp, double* part, double* tot);
// its second stage alone, on chunk sums the caller has formed: part (nq, nchunk) -> tot (nq); nothing is copied out
int sphx_ordered_totals_of_parts(sphx_ctx* ctx, size_t nchunk, int nq, const double* part, double* tot);
// slot[id[j]] = j of the resident state: where the particle with an id lies (sphx_census.hip); slot holds n ints
int sphx_slot_map(sphx_ctx* ctx, int* slot);
// ---- the stellar clock inside sphx_state_insert_rows (sphx_census.hip) ----
// ages set: the by-id array grown to n_new rows with its contents kept (grow), and -2 for the rows [n_old, n_new) (fill)
int sphx_star_ages_grow(sphx_ctx* ctx, int64_t n_old, int64_t n_new, std::vector<void*>& retired);
int sphx_star_ages_fill(sphx_ctx* ctx, int64_t n_old, int64_t n_new);
// ---- shared by the two resident phases (sphx_phase.hip) ----
// The state from the storage slots into the caller's particle order (lane p: the slot of column p, its caller id i;
// col[i] = p, sphx_phase_map.h) - m, mu, h, ptype always; col, the (n,3) positions, the SoA positions, the (n,3)
// velocities, T and E where the pointer is not NULL (sx, T, E: with their sources) - and named arrays back through st.id.
struct PhaseGather {
    int n;
    const int *qorder, *id;
    const double *x, *y, *z, *vx, *vy, *vz, *m, *mu, *h, *pt, *T, *E;
    int* col;
    double *pos, *sx, *sy, *sz, *vel, *om, *omu, *oh, *opt, *oT, *oE;
};
int sphx_phase_gather(sphx_ctx* ctx, const PhaseGather& a);
// out[q][j] = in[q][id[j]] for q < narr; vel (n,3) into vx, vy, vz the same way where vel is not NULL
struct PhaseBack { int n; const int* id; const double* vel; double *vx, *vy, *vz; int narr; const double* in[6]; double* out[6]; };
int sphx_phase_back(sphx_ctx* ctx, const PhaseBack& a);
// the refusal of a state with drag on and no per-species drag tables; gamma (and with drag the two tables) finite
int sphx_phase_check_tables(sphx_ctx* ctx, const char* who, int s, const double* gamma, const double* grain_mass,
                            const double* sigma_effective);
// what the resident phases take as `sizes`: the adapted sizes while they stand (sphx_state_length_scale with apply), else
// the step's radii; both in storage-slot order
static inline const double* sphx_phase_sizes(const sphx_ctx* ctx) {
    return ctx->scale_sizes_valid ? ctx->scale_sizes.as<double>() : ctx->st.hprev.as<double>();
}
int sphx_phase_need_list(sphx_ctx* ctx, const char* who);                          // SPHX_E_STATE unless the last step's list stands
struct PhaseInts { int *col, *list; };                                             // ctx->phase_int: npad | k npad ints
int sphx_phase_ints(sphx_ctx* ctx, int64_t n, int k, PhaseInts* out);
int sphx_phase_translate(sphx_ctx* ctx, int* col, bool col_done, int* list);       // col (n) and the caller-order K-major list (k npad)
int sphx_phase_drag_refresh(sphx_ctx* ctx, int64_t n, int s, const double* f, const double* gm, const double* se, double* mgm, double* mcs);

// integrate / layout helpers (sphx_integrate.hip)
int sphx_clamp(sphx_ctx* ctx, int64_t n, StateArrays& s);
int sphx_permute_state(sphx_ctx* ctx, int64_t n, bool split, hipEvent_t after_first);
int sphx_hsum(sphx_ctx* ctx, int64_t n, const double* h, hipStream_t stream);
int sphx_compute_dt(sphx_ctx* ctx, int first, double fixed_dt);
// no_old: drv:484-485 for every row (the step behind an insertion)
int sphx_integrate(sphx_ctx* ctx, int64_t n, int fold_dt = 0, int first = 0, double fixed_dt = 0.0, int no_old = 0, bool by_byte = false);
int sphx_settled_visc_fill(sphx_ctx* ctx, int64_t n);      // NaN into the rows of ctx->va, ctx->vh that a step by bytes left unwritten
int sphx_pass_drag(sphx_ctx* ctx, int64_t n, int k, const double* m, const double* ptype, const double* mgm,
                   const double* mcs);
int sphx_aos_to_soa3(sphx_ctx* ctx, int64_t n, const double* aos, double* x, double* y, double* z);
int sphx_soa3_to_aos_by_id(sphx_ctx* ctx, int64_t n, const int* id, const double* x, const double* y,
                           const double* z, double* aos);
int sphx_scatter_rows_by_id(sphx_ctx* ctx, int64_t n, int w, const int* id, const double* in, double* out);
int sphx_gather3(sphx_ctx* ctx, int64_t n, const int* perm, const double* x, const double* y,
                 const double* z, double* xs, double* ys, double* zs);
int sphx_iota(sphx_ctx* ctx, int64_t n, int* out);
// Verlet refresh (sphx_refresh.hip)
int sphx_knn_refresh(sphx_ctx* ctx, int64_t n, int k, const double* x, const double* y, const double* z,
                     int32_t* nbr, double* h_sorted, int64_t* nfail_out);
int sphx_save_list_positions(sphx_ctx* ctx, int64_t n, const double* x, const double* y, const double* z);
