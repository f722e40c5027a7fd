// The environment switches of libcis_hip.so: the one list, and the two accessors every read goes through (internal: not installed).
//   X(identifier, "CIS_NAME", kind, default, LATCHED | PER_CALL, "what it does")
// kind -- how the value is parsed:
//   PRESENT  set at all (CIS_X=0 counts as set)          NONZERO  set and atoi != 0
//   INT      atoi / atoll, the default when unset        INT_POS  as INT, and the default for a value <= 0 too
//   REAL     atof, the default when unset                STR      the raw pointer (nullptr when unset), compared by the caller
// default -- SITE: the call site passes it (it depends on the batch or on a constant of that file); 0 for PRESENT, NONZERO and STR.
// LATCHED: envsw::once<id>() -- read at the switch's first use in the process and never again (costs nothing per batch; setting it
// later silently does nothing).  PER_CALL: envsw::call<id>() -- read at every use (tests and A/B runs flip these inside one process).
// The reasons behind a default stay in the comments at the call sites; INTEGRATION.md lists every switch by subject.
#pragma once
#include <stdlib.h>

#define CIS_ENV_SWITCHES(X)                                                                                                          \
    /* search routing */                                                                                                            \
    X(force_scan, "CIS_FORCE_SCAN", INT, 0, LATCHED, "2 / 3: batches of 256 queries and more on k_adc_scan2 / the 16-bit scan, whatever the cell lengths (0: automatic)") \
    X(scan_long, "CIS_SCAN_LONG", INT, 1, LATCHED, "0: long cells stay on k_adc_scan2 instead of the sampled scan")               \
    X(small_nq, "CIS_SMALL_NQ", INT, -1, LATCHED, "largest batch that takes the all-candidates path at limit <= 440 (-1: by limit)") \
    X(scan_geom, "CIS_SCAN_GEOM", STR, 0, PER_CALL, "G,NW,U of k_adc_scan2 out of the instantiated set")                         \
    X(scan3_twopass, "CIS_SCAN3_TWOPASS", INT, SITE, PER_CALL, "form of the 16-bit scan: 0 streaming, 1 two-pass, 2 sampled (default: by chunk length)") \
    X(seg_max, "CIS_SEG_MAX", INT_POS, SITE, PER_CALL, "chunk length of long cells")                                               \
    X(workspace_gb, "CIS_WORKSPACE_GB", REAL, 24, PER_CALL, "device workspace a query batch may take, in GB")                      \
    X(no_t32, "CIS_NO_T32", NONZERO, 0, LATCHED, "no float32 copy of the tables: the scans convert the float64 entries")          \
    X(no_select, "CIS_NO_SELECT", PRESENT, 0, PER_CALL, "all-candidates path: the full segmented sort instead of k_select_topl")   \
    X(tables_ungrouped, "CIS_TABLES_UNGROUPED", PRESENT, 0, PER_CALL, "one block per table (k_tables) instead of the grouped projection; no direct entries (three sites, all per call)") \
    X(tables_valu, "CIS_TABLES_VALU", PRESENT, 0, PER_CALL, "grouped projection on the vector units (k_tables_group) instead of the float64 matrix cores") \
    /* sampled scan (k_adc_scan4) */                                                                                                \
    X(s4_m16, "CIS_S4_M16", INT, 1, LATCHED, "0: M = 16 stays on k_adc_scan2 (route_hints and scan3_geom, both latched)")         \
    X(s4_sat, "CIS_S4_SAT", REAL, 0.75, PER_CALL, "M = 16: where the pre-sample's distance lands, in units of the entry cap")      \
    X(s4_per_cu, "CIS_S4_PER_CU", INT_POS, SITE, PER_CALL, "at most n resident workgroups per CU (only below what LDS and waves allow)") \
    X(s4_zs, "CIS_S4_ZS", REAL, SITE, PER_CALL, "rank margin z on short chunks (default CIS_S4_Z = 4)")                           \
    X(s4_zl, "CIS_S4_ZL", REAL, 4.5, PER_CALL, "rank margin z on long chunks")                                                     \
    X(s4_frac, "CIS_S4_FRAC", INT, 8, PER_CALL, "long chunks: one row in n is the sample")                                         \
    X(s4_nsx, "CIS_S4_NSX", INT, 128, PER_CALL, "long chunks: at most n sample rows")                                              \
    X(s4_dyn, "CIS_S4_DYN", INT, 0, PER_CALL, "long chunks: 1 hands slots out from a counter instead of the static schedule")      \
    /* streaming route */                                                                                                           \
    X(stream_min, "CIS_STREAM_MIN", INT, 262144, LATCHED, "candidates per query from which the route is taken")                    \
    X(stream_nq, "CIS_STREAM_NQ", INT, 16, LATCHED, "largest batch that takes the route (0: never)")                               \
    X(stream_chunk, "CIS_STREAM_CHUNK", INT_POS, SITE, PER_CALL, "chunk length of its cells (default: one chunk per cell)")        \
    X(stream_seg, "CIS_STREAM_SEG", INT_POS, SITE, PER_CALL, "scan mode 6 only: chunk length after rounding (tests)")              \
    X(stream_target, "CIS_STREAM_TARGET", INT_POS, SITE, PER_CALL, "listed candidates per query the sample aims at")               \
    X(stream_ss, "CIS_STREAM_SS", INT, SITE, PER_CALL, "scan mode 6 only: sample stride (tests)")                                  \
    X(stream_k, "CIS_STREAM_K", INT, SITE, PER_CALL, "scan mode 6 and CIS_STREAM_SS set only: rank of the bucket minimum (tests)") \
    X(stream_grid, "CIS_STREAM_GRID", INT_POS, SITE, PER_CALL, "workgroups of the persistent launch")                              \
    X(stream_wait, "CIS_STREAM_WAIT", PRESENT, 0, LATCHED, "read the plan totals back even when the route is certain")             \
    /* tiny cells */                                                                                                                \
    X(no_direct, "CIS_NO_DIRECT", PRESENT, 0, PER_CALL, "float64 tables + k_adc_all_flat instead of k_adc_direct")                 \
    X(no_tiny, "CIS_NO_TINY", PRESENT, 0, PER_CALL, "exact kernels for every candidate instead of k_tiny_select")                  \
    X(tiny_min_quota, "CIS_TINY_MIN_QUOTA", INT, 8192, PER_CALL, "quota from which k_tiny_select runs")                            \
    /* plan / front end */                                                                                                          \
    X(no_par_plan, "CIS_NO_PAR_PLAN", PRESENT, 0, PER_CALL, "serial frontier walk instead of k_plan_par")                          \
    X(no_fused_front, "CIS_NO_FUSED_FRONT", PRESENT, 0, LATCHED, "V <= 64: k_sqdist_rows2 + k_rank + k_plan instead of k_front_small") \
    X(no_plan_hint, "CIS_NO_PLAN_HINT", PRESENT, 0, PER_CALL, "k_plan_par starts without the previous batch's band hint")          \
    X(rank_sort_lds, "CIS_RANK_SORT_LDS", PRESENT, 0, PER_CALL, "float32 coarse distances: the LDS form of the rank sort instead of the register form") \
    X(no_bounds, "CIS_NO_BOUNDS", PRESENT, 0, LATCHED, "always wait for the plan totals: no batch is sized from upper bounds")     \
    X(no_poll, "CIS_NO_POLL", PRESENT, 0, LATCHED, "blocking stream wait for the plan totals instead of polling the pinned word")  \
    /* encode and PCA */                                                                                                            \
    X(coarse, "CIS_COARSE", INT, -1, PER_CALL, "coarse assignment: 0 exact kernels, 1 matrix-core prefilter (-1: by V)")           \
    X(fine, "CIS_FINE", INT, 1, PER_CALL, "0: all-pairs k_fine_codes instead of k_fine_mfma")                                      \
    X(encode_two_kernel, "CIS_ENCODE_TWO_KERNEL", PRESENT, 0, PER_CALL, "projection and fine codes as two kernels instead of the fused one") \
    X(sqdist_plain, "CIS_SQDIST_PLAIN", PRESENT, 0, PER_CALL, "coarse distances by the general kernel instead of the register-tiled one (two sites, both per call)") \
    X(project_valu, "CIS_PROJECT_VALU", PRESENT, 0, PER_CALL, "local projection on the vector units instead of the float64 matrix cores") \
    X(pca_no_small, "CIS_PCA_NO_SMALL", PRESENT, 0, LATCHED, "the batched PCA product for every n instead of k_pca_small up to 8 rows") \
    X(pca_gemm, "CIS_PCA_GEMM", STR, 0, PER_CALL, "valu: the register-tiled PCA kernel; mfma: the float64 matrix cores below 128 input dims too") \
    X(pca_bk, "CIS_PCA_BK", INT, SITE, PER_CALL, "16: K 16 per stage; any other value: 32 (default: by grid size)")                \
    X(pca_tile, "CIS_PCA_TILE", INT, 0, PER_CALL, "64 / 128: force the tile size of the matrix-core PCA product (0: by grid size)") \
    X(pca_pf, "CIS_PCA_PF", INT, 1, PER_CALL, "0: the border-checked fetch instead of k_pca_gemm_mfma_pf")                         \
    /* index insert / remove */                                                                                                     \
    X(insert_slack, "CIS_INSERT_SLACK", INT, -2, LATCHED, "free items the rebuild leaves behind every cell (-1: tight packing; -2: by cell count)") \
    X(ins_no_small, "CIS_INS_NO_SMALL", PRESENT, 0, LATCHED, "inserts of up to 1024 items take the general path")                  \
    X(remove_lds_max, "CIS_REMOVE_LDS_MAX", INT, SITE, PER_CALL, "longest removal list probed in LDS, clamped to 0 ... 1024 (default 1024)") \
    /* CNN */                                                                                                                       \
    X(cnn_no_direct, "CIS_CNN_NO_DIRECT", PRESENT, 0, PER_CALL, "dlib: implicit GEMM instead of the direct 3x3 kernels (float32 and 16-bit sites, both per call)") \
    X(cnn_direct_cfg, "CIS_CNN_DIRECT_CFG", INT, 0, PER_CALL, "dlib: tile shape 0 / 1 / 2 of k_conv3x3_direct")                    \
    X(cnn_no_direct7, "CIS_CNN_NO_DIRECT7", PRESENT, 0, PER_CALL, "dlib: normalisation pass + implicit GEMM for the first layer")  \
    X(cnn_no_pool7, "CIS_CNN_NO_POOL7", PRESENT, 0, PER_CALL, "dlib: first layer and max pool as two kernels")                     \
    X(cnn_d7_tpw, "CIS_CNN_D7_TPW", INT, 4, PER_CALL, "dlib: tiles per wave 1 / 2 / 4 of k_conv7x7s2_direct")                      \
    X(cnn_no_tail, "CIS_CNN_NO_TAIL", PRESENT, 0, PER_CALL, "dlib: the six launches k_dlib_tail replaces")                         \
    X(cnn_no_splitk, "CIS_CNN_NO_SPLITK", PRESENT, 0, LATCHED, "float32 convolutions: no K split")                                 \
    X(cnn_no_bigtile, "CIS_CNN_NO_BIGTILE", PRESENT, 0, PER_CALL, "dlib: 64 x 64 tiles for the 128- / 256-channel maps")           \
    X(cnn_split_target, "CIS_CNN_SPLIT_TARGET", INT, 512, PER_CALL, "workgroups the K split of those maps aims at")                \
    X(cnn_parts, "CIS_CNN_PARTS", INT, SITE, PER_CALL, "parts of a batch in flight together (default: 2 for 128-512 dlib chips, else 1)") \
    X(cnn_threads, "CIS_CNN_THREADS", NONZERO, 0, LATCHED, "every part is enqueued from its own host thread")                      \
    X(cnn_graph, "CIS_CNN_GRAPH", NONZERO, 0, PER_CALL, "dlib forward as a captured graph")                                        \
    X(cnn_nhwc_first, "CIS_CNN_NHWC_FIRST", PRESENT, 0, PER_CALL, "DeepSentibank float32: first layer over re-laid NHWC rows")     \
    X(cnn_fc_tile, "CIS_CNN_FC_TILE", INT, SITE, PER_CALL, "tile shape 0 ... 4 of the fc layers (default: 1 from 64 rows, else 0)") \
    X(cnn_fc_splitk, "CIS_CNN_FC_SPLITK", INT, 8, PER_CALL, "DeepSentibank: K split of fc6 / fc7, 1 ... 32 (changes the summation order)") \
    X(cnn_no_xcd_remap, "CIS_CNN_NO_XCD_REMAP", PRESENT, 0, PER_CALL, "DeepSentibank: max pool + LRN tiles in blockIdx order")     \
    /* test hooks and debug output */                                                                                               \
    X(poison_alloc, "CIS_POISON_ALLOC", NONZERO, 0, LATCHED, "every new workspace is filled with 0xff bytes")                      \
    X(cnn_poison, "CIS_CNN_POISON", INT, 0, PER_CALL, "mask of CNN workspaces (act0 ... act3, part) filled with 0xff before a forward") \
    X(host_timing, "CIS_HOST_TIMING", PRESENT, 0, LATCHED, "stderr, every 400 batches: host time to enqueue the front end and to wait for the plan totals") \
    X(debug_plan, "CIS_DEBUG_PLAN", PRESENT, 0, PER_CALL, "stderr: queries the counting pass handed to the frontier walk")         \
    X(scan4_debug, "CIS_SCAN4_DEBUG", PRESENT, 0, PER_CALL, "stderr: slots the sampled scan handed to its fall-back (waits for the stream)") \
    X(stream_debug, "CIS_STREAM_DEBUG", PRESENT, 0, PER_CALL, "stderr: a line when the streaming route hands a batch back")        \
    X(tiny_debug, "CIS_TINY_DEBUG", PRESENT, 0, LATCHED, "stderr: survivor counts and phase clocks of k_tiny_select")

namespace envsw {
enum Kind { PRESENT, NONZERO, INT, INT_POS, REAL, STR };
enum When { LATCHED, PER_CALL };
constexpr double SITE = -1.0e300;
struct Switch { const char* name; Kind kind; double dflt; When when; };
#define CIS_ENV_ID(id, name, kind, dflt, when, text) id,
enum Id { CIS_ENV_SWITCHES(CIS_ENV_ID) n_switches };
#undef CIS_ENV_ID
#define CIS_ENV_ROW(id, name, kind, dflt, when, text) {name, kind, dflt, when},
constexpr Switch kSwitches[] = {CIS_ENV_SWITCHES(CIS_ENV_ROW)};
#undef CIS_ENV_ROW

// one look-up, parsed by the switch's kind.  T is the type the site computes in: (int)atoll is glibc's atoi, (float)atof as before
template <Id I, typename T>
inline auto read(T dflt) {
    constexpr Kind k = kSwitches[I].kind;
    const char* e = getenv(kSwitches[I].name);
    if constexpr (k == PRESENT) return e != nullptr;
    else if constexpr (k == NONZERO) return e != nullptr && atoi(e) != 0;
    else if constexpr (k == STR) return e;
    else if constexpr (k == REAL) return e ? (T)atof(e) : dflt;
    else {
        const T v = e ? (T)atoll(e) : dflt;
        return k == INT_POS && v <= 0 ? dflt : v;
    }
}
template <Id I>
inline auto read() {  // with the table's default: long long for INT and INT_POS, double for REAL
    static_assert(kSwitches[I].dflt != SITE, "this switch takes its default at the call site: call<id>(default)");
    if constexpr (kSwitches[I].kind == REAL) return read<I>(kSwitches[I].dflt);
    else return read<I>((long long)kSwitches[I].dflt);
}

template <Id I>
inline auto call() {
    static_assert(kSwitches[I].when == PER_CALL, "a LATCHED switch is read through once<id>()");
    return read<I>();
}
template <Id I, typename T>
inline auto call(T site_default) {
    static_assert(kSwitches[I].when == PER_CALL && kSwitches[I].dflt == SITE, "call<id>(default) is for PER_CALL switches whose default is SITE");
    return read<I>(site_default);
}
template <Id I>
inline auto once() {  // one static per switch in the library (the functions are inline, not static): latched at that switch's first use
    static_assert(kSwitches[I].when == LATCHED, "a PER_CALL switch is read through call<id>()");
    static const auto v = read<I>();
    return v;
}
}  // namespace envsw
