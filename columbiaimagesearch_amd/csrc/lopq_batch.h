// Internal: what the phases of one batch search share -- the plan stage (lopq_plan.hip) and the driver, routes, tables, scans and
// selections (lopq_search.hip): the structures a batch carries from phase to phase and the plan's phase functions.
#pragma once
#include <atomic>
#include <chrono>

#include "lopq_index.h"
#include "scan_common.h"

// counters of the table groups are split GRP_SUB ways by query index: 16 k atomics on 32 addresses would serialise
static const int GRP_SUB = 32;
// words of the counters, cursors and bases of the table groups (+ 2, to an even count), then one 64-bit word per tile of k_group_bases
#define GRP_WORDS(V) (6 * (V) * GRP_SUB + 2)
#define GRP_TILES(V) ((2 * (V) * GRP_SUB + 1023) / 1024)

static const int PLAN_PAR_STAGE = 4096; // d0 / d1 staged in LDS: the kernel takes V <= 4096

// ---- front end: LOPQ-space queries, coarse type, the rank workspaces (the batch search and the owner walk of the routed search) ----
struct Front {
    const void* xc;  // the queries as the coarse quantizers read them
    int ct;          // their type: CIS_F32 or CIS_F64
    int* grp_cnt;    // [2V][GRP_SUB] tables per (split, cluster, query % GRP_SUB); the rank kernels leave the counters zeroed
};

static const float* coarse_centroids(const cis_model* m, float) { return m->d_Cs32; }
static const double* coarse_centroids(const cis_model* m, double) { return m->d_Cs64; }

struct Scan2Geom { int G, NW, U, S; size_t lds; };

// ---- what a batch runs: every predicate once -----------------------------------------------------------------------------------
struct Route {
    // route_hints: before the plan (the chunk size is part of the plan)
    bool w_pow2;        // sub-quantizers of 4, 8, 16 or 32 components
    bool split_tables;  // ... and K <= 256: tables from the projected residuals (k_tables_from_px), exact keys from them (k_adc_direct)
    bool big;           // ranked over all candidates' exact distances (use_all_path)
    bool fast;          // the float32 / fixed-point prefilter scans serve this shape
    bool tiny_cells;
    bool use3;          // lopq_scan3.hip instead of k_adc_scan2
    bool stream_hint;   // the HBM-streaming route, if the plan confirms it
    bool par_plan, fused_front;
    int seg_max;
    int64_t stream_min;
    Scan2Geom geom;
    // route_decide: with the plan totals, or their bounds
    bool direct;        // tiny cells on the all-candidates path: entries computed per candidate from px (k_adc_direct), no tables
    bool stream;
    bool drop_t32;
    Scan3Geom geom3;
    int S;              // hit slots per work item (fast kernels: a full region per wave)
};

// values the phases of one batch share
struct Batch {
    cis_index* ix;
    const void* dQ;
    int q_dtype, nq;
    int64_t quota;
    int L;
    SearchOut out;
    hipStream_t st;
    Front f;
    PlanOut* plan;
    int64_t *item_off, *tab_off, *totals;
    unsigned long long* qbound;  // per query: cross-cell bound of the scan
    int *grp_cur, *grp_base;     // cursors and exclusive scan of the table groups
    int* plan_fb;                // k_plan_par: per-query fall-back flags
    uint64_t* vis_list;
    int vis_cap;
    unsigned long long* plan_hint;
    int hint_slot;
    const int64_t* d_tot;        // the batch did not wait for the totals: n_items, n_tabs, n_cand_all are bounds, the kernels read these
    int64_t n_items, n_tabs, n_cand_all;
    WorkItem* items;
    TabDesc* tabs;
    int* tab_order;              // table indices grouped by (split, cluster)
    double *T, *px_buf;
    float* T32;
    cis_index::ProfRec pr;
    std::chrono::steady_clock::time_point t_entry;
};

static int mark(Batch& b, int i) {
    if (!b.ix->profiling) return CIS_OK;
    if (b.ix->profiling == 1 && i != 5 && i != 3) return CIS_OK;  // level 1: only the pair around the scan kernel
    CIS_CHECK_HIP(hipEventCreate(&b.pr.ev[i]));
    CIS_CHECK_HIP(hipEventRecord(b.pr.ev[i], b.st));
    return CIS_OK;
}

// ---- slot list: work items grouped by (coarse cell, chunk) with a counting sort, G per slot -------------------------------------
struct Slots {
    int* qctr;     // [8] queue counters, [8] n_slots (first), [9] queue starts, [32] fall-back header (scan3)
    int* n_slots;
    int* fhdr;
    int* slots;    // null: slot i = work item i (SLOTS_NONE)
    int* fslots;
    int64_t max_slots;
};
enum SlotMode {
    SLOTS_SORTED,    // the counting sort
    SLOTS_IDENTITY,  // huge V: slot i = work item i, written out (k_identity_slots)
    SLOTS_NONE       // one query per slot on the streaming route: no list at all (k_stream_prep counts the slots)
};

// ---- the plan's phases (lopq_plan.hip), in the order search_batch runs them -------------------------------------------------------
// LOPQ-space queries, their coarse type, the rank workspaces
int front_prepare(cis_index* ix, const void* dQ, int q_dtype, int nq, hipStream_t st, Front* f);
// coarse distances, rank and the counting pass of the multisequence walk (CT: float or double, by Front::ct)
template <typename CT>
int front_count(Batch& b, const Route& r);
// CIS_DEBUG_PLAN: how many queries of the batch the sort-based plan handed to the frontier walk
int dump_plan_fallbacks(const Batch& b);
// exclusive scan of the plan; then the totals that size the rest of the batch
int plan_totals(Batch& b, const Route& r);
// the emitting pass of the walk: work items + table list
template <typename CT>
void emit_plan(Batch& b, const Route& r);
int build_slots(const Batch& b, SlotMode mode, int G, int64_t CH /* chunks per cell that get their own slot keys */, int seg_max, Slots* s);
