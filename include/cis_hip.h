/*
 * cis_hip.h -- C ABI of libcis_hip.so: the MI355X (gfx950) implementation of the
 * embed-then-index hot path of ColumbiaImageSearch.
 *
 * The reference has no FFI: its boundary is three duck-typed Python surfaces
 * (lopq.model.LOPQModel[PCA], lopq.search.LOPQSearcherBase subclasses, cufacesearch
 * GenericFeaturizer).  The Python mirrors of those surfaces in columbiaimagesearch_amd/ bind
 * exactly the entry points below through ctypes; INTEGRATION.md shows the binding a reference
 * maintainer would add.  Each entry point cites the reference code it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *  - plain pointers and sizes only; `*_dev` entry points take DEVICE pointers and a hipStream_t
 *    (passed as void*; NULL = the null stream) and never synchronise; the others take HOST
 *    pointers, copy, run and synchronise before returning;
 *  - every function returns 0 on success or a negative CIS_E* code; the message of the last
 *    failure on the calling thread is cis_last_error().  Nothing aborts or throws across the ABI
 *    (the reference's callers log per-item errors and keep going: lopq/lopq/search.py:365-367);
 *  - the library never keeps caller pointers after a call returns; handles own device memory;
 *  - HIP is initialised lazily on first use, so a process may fork before touching the library
 *    (gunicorn / multiprocessing callers); handles must not be shared across processes;
 *  - a handle (model, index, CNN) owns ONE set of device workspaces: calls on the same handle must not overlap -- neither from
 *    two threads nor on two streams (a `*_dev` call returns while its kernels are still queued: issue the next call on the
 *    same stream, or wait for the first).  An index also uses its model's workspaces.  Different handles are independent;
 *  - dtype arguments: CIS_F32 = 4, CIS_F64 = 8 (bytes per element).
 */
#ifndef CIS_HIP_H
#define CIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIS_F32 4
#define CIS_F64 8

#define CIS_OK 0
#define CIS_EINVAL -1   /* bad argument (Python wrapper raises ValueError)            */
#define CIS_EHIP -2     /* a HIP runtime call failed                                   */
#define CIS_ENOMEM -3   /* device or host allocation failed                            */
#define CIS_EUNSUPPORTED -4 /* valid in the reference but not built yet (NotImplementedError) */
#define CIS_ENODEVICE -5 /* no gfx950 device visible                                   */

typedef struct cis_model cis_model;
typedef struct cis_index cis_index;
typedef struct cis_cnn cis_cnn;

/* One ranked candidate of a (possibly partial, per-shard) result list.  Ordering key is
 * (dist, visit_rank, pos): the reference ranks with a stable sort over the retrieval order,
 * i.e. multisequence cell order then insertion order inside the cell (lopq/lopq/search.py:128-133,
 * :210).  32 bytes; this is also what travels in the RCCL all-gather of the sharded search. */
typedef struct cis_hit {
    double dist;         /* squared ADC distance, float64 (search.py:173)                 */
    uint32_t visit_rank; /* 0-based position of the candidate's cell in multisequence order */
    uint32_t pos;        /* 0-based insertion position inside that cell                   */
    int64_t id;          /* caller's item id (-1: empty slot)                             */
    int32_t cell;        /* c0 * V + c1 of the candidate's coarse cell                    */
    int32_t reserved;
} cis_hit;

/* ---- library ------------------------------------------------------------------------------ */
int cis_version(void);
const char* cis_last_error(void);
/* Device workspace growth since the process started: every handle's workspaces are grow-only, and a growth is a hipFree (which
 * waits for the device) + hipMalloc -- tens of milliseconds when it lands inside a measured loop.  A harness reads the counters
 * before and after its timed region to prove that nothing was allocated in it (bench.py does).  Either pointer may be NULL. */
int cis_alloc_stats(int64_t* n_allocs, int64_t* n_bytes);
/* Number of visible HIP devices (0 when none); never fails. */
int cis_device_count(void);
/* Select the device used by handles created afterwards by this process (default 0). */
int cis_set_device(int device);
/* Runs a device self test of the wave-level primitives the scan kernel relies on (DPP / permlane
 * lane exchanges, in-register bitonic sort); *n_errors = 0 when they behave. */
int cis_selftest(int* n_errors);

/* ---- LOPQ model: replaces lopq.model.LOPQModel / LOPQModelPCA arithmetic --------------------
 * Parameter layout = the reference's parameter tuple (lopq/lopq/model.py:461-473, :841), each
 * pair concatenated split-major and C-contiguous:
 *   Cs   [2][V][h]      coarse centroids, dtype coarse_dtype (float32 when LOPQ was trained on
 *                       float32 data, e.g. after apply_PCA; float64 otherwise)
 *   Rs   [2][V][h][h]   local rotations, applied as R[c] . r   (model.py:638)
 *   mus  [2][V][h]      mean residuals
 *   subs [M][K][w]      sub-quantizer centroids, fine split j of coarse split s at s*M/2 + j
 *   pca_P [D_in][D], pca_mu [D_in]  or NULL/NULL for a plain LOPQModel (then D_in == D)
 * with h = D/2, w = D/M.  K <= 256 and V <= 4096 in this build.
 * pca_mu_dtype: dtype the caller's pca_mu array had.  train_pca takes np.mean of the training
 * data (model.py:260), so a model trained on float32 features holds a float32 mean and
 * apply_PCA's `x - pca_mu` (model.py:965) then rounds in float32 for float32 inputs; the values
 * are passed here widened to double either way. */
int cis_model_create(cis_model** out, int D_in, int D, int V, int M, int K, int coarse_dtype,
                     const void* Cs, const double* Rs, const double* mus, const double* subs,
                     const double* pca_P, const double* pca_mu, int pca_mu_dtype, int renorm);
void cis_model_destroy(cis_model* m);

/* LOPQModelPCA.apply_PCA (model.py:961-978): out[n][D] float32.  x_dtype = dtype of X. */
int cis_apply_pca(cis_model* m, const void* X, int x_dtype, int64_t n, float* out);

/* LOPQModel.predict over n vectors (model.py:543-561, :980-1003; the loop of
 * compute_codes_notparallel, lopq/lopq/utils.py:203-218).  X is [n][D_in] of x_dtype (PCA is
 * applied first when the model has one).  coarse [n][2], fine [n][M]. */
int cis_encode(cis_model* m, const void* X, int x_dtype, int64_t n, uint16_t* coarse, uint8_t* fine);
int cis_encode_dev(cis_model* m, const void* dX, int x_dtype, int64_t n, uint16_t* d_coarse,
                   uint8_t* d_fine, void* stream);

/* The pieces of predict, exposed because the reference exposes them.  They take vectors that
 * are ALREADY in LOPQ space (i.e. after apply_PCA), [n][D] of x_dtype:
 *   predict_coarse (model.py:563-573), project (model.py:604-641) -> out [n][D] float64,
 *   predict_fine (model.py:575-602),
 *   get_subquantizer_distances (model.py:673-704) -> tables [n][M][K] float64,
 *   reconstruct (model.py:643-671) -> out [n][D] float64. */
int cis_predict_coarse(cis_model* m, const void* X, int x_dtype, int64_t n, uint16_t* coarse);
int cis_project(cis_model* m, const void* X, int x_dtype, int64_t n, const uint16_t* coarse, double* out);
int cis_predict_fine(cis_model* m, const void* X, int x_dtype, int64_t n, const uint16_t* coarse, uint8_t* fine);
int cis_subquantizer_distances(cis_model* m, const void* X, int x_dtype, int64_t n,
                               const uint16_t* coarse, double* tables);
int cis_reconstruct(cis_model* m, const uint16_t* coarse, const uint8_t* fine, int64_t n, double* out);

/* predict_cluster (lopq/lopq/utils.py:33-53) against an arbitrary centroid matrix: X [n][d], C [ncent][d];
 * distances in float32 when both are float32, else float64 (numpy promotion), numpy summation order, first
 * minimum wins.  out [n] cluster ids. */
int cis_predict_cluster(const void* X, int x_dtype, const void* C, int c_dtype, int64_t n, int ncent, int d,
                        uint32_t* out);

/* multisequence (lopq/lopq/search.py:13-82) as a list: for each of n LOPQ-space vectors X [n][2h] the first
 * max_cells (clamped to V*V) cells in multi-sequence order: cells [n][max_cells][2], dists [n][max_cells]
 * (the cell distance d0+d1 rounded in *dist_dtype = 4 or 8, the dtype the reference yields). */
int cis_multisequence(const void* X, int x_dtype, const void* C0, const void* C1, int c_dtype, int64_t n, int V,
                      int h, int max_cells, int32_t* cells, double* dists, int* dist_dtype);

/* ---- LOPQ index: replaces lopq.search.LOPQSearcher (search.py:310-382) ---------------------- */
/* The index keeps a borrowed pointer to `m`: destroy the index first. */
int cis_index_create(cis_index** out, cis_model* m);
void cis_index_destroy(cis_index* ix);
/* A search VIEW of `base`: shares its storage (codes, ids, offsets, cell sizes -- lopq/lopq/search.py:310-382's `index` dict) and
 * owns only per-batch workspaces and counters, so that two query batches can be in flight at once, each handle on its own stream
 * (the reference answers independent queries from 16 independent gunicorn workers over one LMDB index, searcher_lopqhbase.py:198-206:
 * this is the same sharing inside one process).  A view is read-only (inserts / cell reads go to the base) and should be destroyed
 * before the base: a base destroyed first ORPHANS its views -- they stay valid handles, every later search through them returns
 * CIS_EINVAL, and they must still be destroyed.  Inserts into the base must be stream-ordered against the views' searches by the
 * caller (columbiaimagesearch_amd/distributed.py:ShardedSearcher._insert_fence does it for its own lanes). */
int cis_index_create_view(cis_index** out, cis_index* base);

/* Cell-sharded operation (one process per GPU): this handle stores only the cells with
 * owner[cell] == rank but counts every cell, so that all ranks derive the same global
 * multisequence order and quota cut-off without communicating (search.py:128-133).
 * owner = NULL selects cell_id % world.  Must be called on an empty index. */
int cis_index_set_shard(cis_index* ix, int rank, int world, const int32_t* owner /* [V*V] or NULL */);
/* How the insert calls of this handle were served: counters[0] = batches written IN PLACE behind their cells' last items (O(batch):
 * the reference appends to a per-cell list, lopq/lopq/search.py:349-364), counters[1] = batches that rebuilt the layout (a cell's
 * slack was exhausted, or a bulk load). */
int cis_index_insert_counters(cis_index* ix, int64_t counters[2]);

/* Routed insert into a cell-sharded index: cis_index_add is then given only the codes of
 * the cells this rank owns; cis_index_cell_counts reads the per-cell sizes [V*V] (all shards), and
 * cis_index_add_remote_counts adds per-cell increments [V*V] for the cells owned by OTHER ranks (entries of owned cells
 * are ignored), so that every rank keeps the whole cell-size table the quota cut needs (lopq/lopq/search.py:128-133). */
int cis_index_cell_counts(cis_index* ix, int64_t* counts);
int cis_index_add_remote_counts(cis_index* ix, const int64_t* delta);
/* The same on device arrays (the all-reduce of the increments runs over RCCL on them): d_counts / d_delta [V*V]. */
int cis_index_cell_counts_dev(cis_index* ix, int64_t* d_counts, void* stream);
int cis_index_add_remote_counts_dev(cis_index* ix, const int64_t* d_delta, void* stream);
/* Routed insert without a host copy.  cis_index_route_pack_dev groups this rank's n freshly encoded items by the rank
 * that owns their cell (arrival order inside a group, so that the per-cell insertion order after the exchange is that of
 * a single index, search.py:359): d_records [n][12 + M] = id (8 B, little endian) | coarse (2 x uint16) | fine (M B),
 * d_counts [world] int64 = records per destination.  cis_index_add_records_dev inserts records received from the
 * all-to-all (same semantics and outputs as cis_index_add_dev). */
int cis_index_route_pack_dev(cis_index* ix, const int64_t* d_ids, const uint16_t* d_coarse, const uint8_t* d_fine,
                             int64_t n, uint8_t* d_records, int64_t* d_counts, void* stream);
int cis_index_add_records_dev(cis_index* ix, const uint8_t* d_records, int64_t n, int dedup, int64_t* n_added,
                              int64_t* n_invalid, int64_t* d_cell_delta, void* stream);

/* add_codes (search.py:325-369): append items in order; with dedup != 0 an id already present in
 * the SAME cell is skipped (first occurrence wins).  *n_added = items counted (all shards). */
int cis_index_add(cis_index* ix, const int64_t* ids, const uint16_t* coarse, const uint8_t* fine,
                  int64_t n, int dedup, int64_t* n_added);
/* The same insert on arrays that are already in HBM (the codes cis_encode_dev just produced: the refresh loop of
 * searcher_lopqhbase.py:743-758 without the round trip through the host).  The index lives in HBM only; an insert is a
 * stable merge by kernels on `stream` (csrc/lopq_index.hip), and the call returns after the stream has drained (the
 * accepted count is read back).  Items with out-of-range codes or negative ids are skipped and counted in *n_invalid
 * ("could not push code", search.py:365-367) -- the host entry point above rejects the whole call instead. */
int cis_index_add_dev(cis_index* ix, const int64_t* d_ids, const uint16_t* d_coarse, const uint8_t* d_fine, int64_t n,
                      int dedup, int64_t* n_added, int64_t* n_invalid, int64_t* d_cell_delta /* [V*V] accepted per cell, or NULL */,
                      void* stream);
/* Removal by id, on the device (csrc/lopq_remove.hip; the reference's dict index cannot remove).  Every stored item whose id is in
 * the list leaves the index: from every cell that holds it, every copy inside a cell (dedup = 0 inserts can store an id more than
 * once).  Kept items keep their relative order inside their cell.  Ids that are not stored, ids that occur more than once in the
 * list and negative ids are ignored; n = 0 is a no-op.  Afterwards the index equals one built by the same insert calls with the
 * removed ids filtered out of every batch (cells, counts, every search route, the duplicate test of later inserts): a removed id
 * may be inserted again and lands behind its cell's last item.  The storage of a cell does not shrink: its room stays, only its used
 * end moves down (more slack for in-place inserts), and the next rebuild of the layout renews the slack as it does today.
 * Like cis_index_add_dev the call enqueues kernels on `stream` and returns after the stream has drained (the removed count and the
 * cell-size statistics are read back: its one host round trip).  n < 2^31.  *n_removed = items removed from THIS shard's cells.
 * A view is read-only: removal through it returns CIS_EINVAL; removals from the base must be stream-ordered against the views'
 * searches by the caller, like inserts.  On a cell-sharded index every rank is given the same ids; the id-only store of the other
 * shards' cells drops them too, and the sizes of the cells that other shards own change ONLY through cis_index_sub_remote_counts
 * (whatever insert mode built the index): sum the d_cell_delta arrays over the ranks and hand the sum to it. */
int cis_index_remove_dev(cis_index* ix, const int64_t* d_ids, int64_t n, int64_t* n_removed,
                         int64_t* d_cell_delta /* [V*V] items removed per cell of THIS shard, or NULL */, void* stream);
int cis_index_remove(cis_index* ix, const int64_t* ids, int64_t n, int64_t* n_removed); /* host array: uploaded, then the above */
/* Stage times in ms of the last cis_index_remove[_dev] on this handle that ran with profiling on (cis_index_set_profiling != 0; HIP events
 * on the launch stream): ms[0] building the removal set, ms[1] the mark pass, ms[2] the touched-cell list and the compaction. */
int cis_index_remove_profile(cis_index* ix, double ms[3]);
/* The counterpart of cis_index_add_remote_counts: per-cell decrements [V*V] >= 0 for the cells owned by OTHER ranks (entries of
 * owned cells are ignored).  A first pass checks that no count would go negative; if one would, CIS_EINVAL and nothing changes. */
int cis_index_sub_remote_counts(cis_index* ix, const int64_t* delta);
int cis_index_sub_remote_counts_dev(cis_index* ix, const int64_t* d_delta, void* stream);
/* featsio.normfeatB64encode's normalisation (cufacesearch/cufacesearch/featurizer/featsio.py:13-22) on n device rows of d
 * values, in place, in the rows' dtype; zero rows stay zero. */
int cis_l2_normalize_dev(void* d_x, int dtype, int64_t n, int d, void* stream);
/* get_nb_indexed (search.py:91-92): items over all shards. */
int64_t cis_index_size(cis_index* ix);
/* get_cell (search.py:372-382): items of one cell in insertion order.  cap <= 0: *n = the cell's size (all
 * shards), nothing is copied.  cap > 0: copies at most cap items, *n = the number copied (0 for a cell that
 * another shard owns). */
int cis_index_get_cell(cis_index* ix, int c0, int c1, int64_t cap, int64_t* ids, uint8_t* fine, int64_t* n);

/* LOPQSearcherBase.search over nq queries (search.py:179-224): Q [nq][D_in] of q_dtype.
 * limit < 0 means "limit = quota" (search.py:213-214).  Outputs, with L = effective limit:
 *   ids [nq][L] (-1 padded), dists [nq][L] (NaN padded), n_found [nq], visited [nq], and
 *   optionally (may be NULL) cells [nq][L] (c0*V+c1, -1 padded) and pos [nq][L]: where each
 *   result lives, so that its code can be fetched with cis_index_get_codes (Result.code,
 *   search.py:217-222). */
int cis_index_search(cis_index* ix, const void* Q, int q_dtype, int nq, int64_t quota, int limit,
                     int64_t* ids, double* dists, int32_t* n_found, int32_t* visited,
                     int32_t* cells, uint32_t* pos);
int cis_index_search_dev(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota, int limit,
                         int64_t* d_ids, double* d_dists, int32_t* d_n_found, int32_t* d_visited,
                         int32_t* d_cells, uint32_t* d_pos, void* stream);
/* The host-pointer search in two halves (round 5): cis_index_search_async enqueues copy-in, search and copy-out on the handle's OWN
 * stream and returns once the search's launches are queued; cis_index_search_wait blocks until the results have landed in the caller's
 * buffers, which must stay valid and untouched until then.  One batch in flight per handle (a second call waits for the first); views
 * of one index (cis_index_create_view) give several -- the reference serves independent queries from 16 gunicorn workers over one
 * index (searcher_lopqhbase.py:198-206), this is that inside one process.  cis_index_search = async + wait.
 * cis_host_alloc / cis_host_free: page-locked host memory.  With Q and the outputs in it the copies are DMA transfers that overlap the
 * other handles' searches; pageable memory works too and is staged by the runtime (slower, and the call then blocks while it copies). */
int cis_index_search_async(cis_index* ix, const void* Q, int q_dtype, int nq, int64_t quota, int limit,
                           int64_t* ids, double* dists, int32_t* n_found, int32_t* visited,
                           int32_t* cells, uint32_t* pos);
int cis_index_search_wait(cis_index* ix);
int cis_host_alloc(void** out, size_t bytes);
void cis_host_free(void* p);
/* Fine codes of n stored items addressed by (cell, pos) as returned by a search.  fine [n][M].
 * Items of cells owned by another shard yield CIS_EINVAL. */
int cis_index_get_codes(cis_index* ix, const int32_t* cells, const uint32_t* pos, int64_t n, uint8_t* fine);

/* Sharded search, step 1: this shard's ranked candidates.  d_hits [nq][L] (unused slots have
 * id = -1, dist = +inf), d_visited [nq] (identical on every rank). */
int cis_index_search_partial_dev(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota,
                                 int limit, cis_hit* d_hits, int32_t* d_visited, void* stream);
/* The same, packed for the exchange: d_cnt[q] valid hits of query q at d_packed[d_off[q] ..], queries in order,
 * *d_total hits in all (d_packed needs room for nq * L records; only the first *d_total are written). */
int cis_index_search_partial_packed_dev(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota, int limit,
                                        cis_hit* d_packed, int32_t* d_cnt, int64_t* d_off, int64_t* d_total,
                                        int32_t* d_visited, void* stream);
/* Routed cell-sharded search (round 5; the all-gather protocol above replicates projection, cell ranking and walk on every rank):
 * step 0, on a query's HOME rank -- d_mask[q] bit r = rank r owns a non-empty cell among those the multisequence walk of query q
 * visits before the quota is reached (the walk of lopq/lopq/search.py:58-82,:128-133 against the cell sizes of the WHOLE index;
 * world <= 64), d_visited[q] (or NULL) = the number of cells it looks at (the `visited` of the reference's result).  Uses the
 * handle's workspaces: call it on the stream the handle's searches run on. */
int cis_index_query_owners_dev(cis_index* ix, const void* d_q, int q_dtype, int nq, int64_t quota, uint64_t* d_mask,
                               int32_t* d_visited, void* stream);
/* ... step 1: the send buffers of the query all-to-all.  d_q [nq] rows of row_bytes bytes (a multiple of 4: float32 or float64
 * queries), d_slot [world][nq]: row of query i in the block for rank d (-1: not sent; rows in query order), d_out_q [world][cap]
 * rows, d_cnt [world]: rows used per destination, *d_overflow = 1 when a destination needed more than cap rows (the caller then
 * answers the batch through the all-gather protocol). */
int cis_route_queries_dev(const void* d_q, int nq, int row_bytes, const uint64_t* d_mask, int world, int cap, void* d_out_q,
                          int32_t* d_slot, int32_t* d_cnt, int32_t* d_overflow, void* stream);

/* ... step 3, back on the home rank: where the list of home query i from rank d sits in the buffer of returned lists (rows of
 * `limit` cis_hit, grouped by answering rank; h_base [world] (HOST) = first row of rank d's group): d_off [world][nq] record
 * offsets, d_cnt [world][nq] valid hits (0: rank d was not asked) -- the inputs of cis_merge_packed_dev with stride = 0. */
int cis_routed_merge_tables_dev(const int32_t* d_slot, int world, int nq, const int64_t* h_base, const cis_hit* d_hits, int limit,
                                int64_t* d_off, int32_t* d_cnt, void* stream);

/* Sharded search, step 2 (after the all-gather): merge `world` partial lists
 * d_parts [world][nq][L] into the final ranking. */
int cis_merge_hits_dev(const cis_hit* d_parts, int world, int nq, int limit, int64_t* d_ids,
                       double* d_dists, int32_t* d_n_found, int32_t* d_cells /* or NULL */,
                       uint32_t* d_pos /* or NULL */, void* stream);

/* The same for PACKED partial lists (what travels over xGMI): shard w contributed its valid hits only, in query
 * order, d_parts[w*stride + d_off[w*nq + q] .. + d_cnt[w*nq + q]) for query q (stride = 0: ONE buffer, d_off holds absolute record
 * offsets -- the return trip of the routed search).  limit <= 3072 (one wave per query; above that the caller ranks the packed lists itself: distributed.merge_packed_sorted). */
int cis_merge_packed_dev(const cis_hit* d_parts, int world, int64_t stride, const int64_t* d_off /* [world][nq] */,
                         const int32_t* d_cnt /* [world][nq] */, int nq, int limit, int64_t* d_ids, double* d_dists,
                         int32_t* d_n_found, int32_t* d_cells /* or NULL */, uint32_t* d_pos /* or NULL */, void* stream);
/* The same merge, which also says where each result came from: everything cis_merge_packed_dev writes, bit for bit (padding
 * included), and d_src_rec [nq][limit] = the index in d_parts of the result's record (w * stride + d_off + place in the list; never
 * past what arrived of a list that the fixed exchange cut), -1 in the padding.  An array that shares d_parts' layout -- the true
 * distances of cis_rerank_packed_dev -- is read through it.  limit <= 3072 (the one-wave merge); above that CIS_EINVAL. */
int cis_merge_packed_src_dev(const cis_hit* d_parts, int world, int64_t stride, const int64_t* d_off /* [world][nq] */,
                             const int32_t* d_cnt /* [world][nq] */, int nq, int limit, int64_t* d_ids, double* d_dists,
                             int32_t* d_n_found, int32_t* d_cells /* or NULL */, uint32_t* d_pos /* or NULL */, int64_t* d_src_rec,
                             void* stream);

/* Offsets of the packed exchange, on the device ("one collective per query batch" -- no host read in between):
 * d_cnt_all [world][nq] = the all-gathered per-query hit counts -> d_off [world][nq] (exclusive scan per shard), d_totals [world],
 * *d_overflow = 1 when a shard holds more records than `stride` (the fixed per-rank size of the payload all-gather). */
int cis_exchange_offsets_dev(const int32_t* d_cnt_all, int world, int nq, int64_t stride, int64_t* d_off, int64_t* d_totals,
                             int32_t* d_overflow, void* stream);

/* Exact re-ranking with features resident in HBM (cufacesearch/cufacesearch/searcher/searcher_lopqhbase.py:864-912:
 * dist = np.linalg.norm(normed_feat - res_fts[pos]) for the first results of a query).  d_feats [n_feats][D] and
 * d_q [nq][D] in f_dtype (4 = float32, 8 = float64; the distance is computed in that type, NOT squared), d_rows [nq][L]
 * = feature row of each result (-1: not resident -> NaN, the caller keeps the ADC distance as the reference does). */
int cis_rerank_dev(const void* d_feats, int f_dtype, int64_t n_feats, int D, const void* d_q, int nq,
                   const int64_t* d_rows, int L, double* d_dists, void* stream);

/* Device id -> feature row map (csrc/lopq_rerank.hip): an open-addressing table in memory the caller owns, d_keys [cap] and
 * d_rows [cap] int64, cap a power of two >= 2 n (anything else: CIS_EINVAL).  The build fills both with -1 and inserts
 * d_ids [n] by kernels on `stream` (linear probing from a 64-bit mixed hash); a negative id is skipped and a repeated id maps
 * to its LAST row, like {k: i for i, k in enumerate(ids)}.  The look-up writes d_out[i] = row of d_ids[i] (m of them), -1 for an
 * unknown or negative id or a row >= n_feats; d_keys = d_rows = NULL is the identity map: row = id when 0 <= id < n_feats. */
int cis_idmap_build_dev(const int64_t* d_ids, int64_t n, int64_t* d_keys, int64_t* d_rows, int64_t cap, void* stream);
int cis_idmap_lookup_dev(const int64_t* d_keys, const int64_t* d_rows, int64_t cap, int64_t n_feats, const int64_t* d_ids, int64_t m,
                         int64_t* d_out, void* stream);

/* Search results -> the reference's final answer in one kernel, nothing through the host (searcher_lopqhbase.py:864-912,
 * :975-1017).  For each of nq queries the first nb <= min(L, 1024) of its results d_ids / d_adc [nq][L] (id < 0: no result) are
 * looked up in the id map (NULL, NULL: the identity), measured against d_feats [n_feats][D] (the distance of cis_rerank_dev
 * bit for bit; a result whose feature is not resident keeps its ADC distance), kept if their place BEFORE the re-order is below
 * max_returned (0: no cut) and their distance <= near_dup_th (when use_th != 0; compared as float64), and ranked by
 * (distance, place): np.argsort(kind="stable").  Outputs [nq][nb]: d_out_ids (-1 padded), d_out_dists (NaN padded), d_out_src
 * (the place a result had in d_ids, -1 padded); d_n_kept [nq].  nb > 1024 is CIS_EINVAL: such calls stay with the host path. */
int cis_rerank_select_dev(const void* d_feats, int f_dtype, int64_t n_feats, int D, const int64_t* d_map_keys,
                          const int64_t* d_map_rows, int64_t map_cap, const void* d_q, int nq, const int64_t* d_ids,
                          const double* d_adc, int L, int nb, int max_returned, int use_th, double near_dup_th,
                          int64_t* d_out_ids, double* d_out_dists, int32_t* d_out_src, int32_t* d_n_kept, void* stream);

/* The exact re-rank of the cell-sharded index (distributed.py): the features of an item live with the rank
 * that owns its cell, so a rank measures its OWN hits before the exchange, the distances travel beside the records, and the home
 * rank merges by ADC (cis_merge_packed_src_dev) and ranks by true distance (cis_rerank_select_merged_dev).
 *
 * cis_rerank_packed_dev: list q of this rank is d_recs[d_off[q] .. + d_cnt[q]) (the packed layout of
 * cis_index_search_partial_packed_dev, or the rows of a dense [rows][L] answer with d_off[q] = q * L), its query row d_q[q] (f_dtype,
 * like the features: the view of a feature store or of cis_rerank_select_dev's arguments).  d_true [n_rec] is parallel to d_recs:
 * for record i < nb of a list, the distance of cis_rerank_dev bit for bit when the record's id has a resident row, NaN when it has
 * none (or its id is negative); NaN for the records i >= nb, which no merged top-nb can hold.  Entries outside every list are left
 * alone, and a list that does not lie inside [0, n_rec) is skipped.  nb <= 1024.
 *
 * cis_rerank_select_merged_dev: d_ids / d_adc / d_src_rec [nq][L] as cis_merge_packed_src_dev wrote them, d_true [n_true] the
 * gathered distances in d_parts' layout.  The distance of result i is d_true[d_src_rec[i]], or its ADC distance where that is NaN;
 * keep, rank, outputs and padding are cis_rerank_select_dev's (d_out_src = the place in the merged ADC list). */
int cis_rerank_packed_dev(const void* d_feats, int f_dtype, int64_t n_feats, int D, const int64_t* d_map_keys,
                          const int64_t* d_map_rows, int64_t map_cap, const void* d_q, int nq, const cis_hit* d_recs, int64_t n_rec,
                          const int64_t* d_off /* [nq] */, const int32_t* d_cnt /* [nq] */, int nb, double* d_true, void* stream);
int cis_rerank_select_merged_dev(const int64_t* d_ids, const double* d_adc, const int64_t* d_src_rec, int nq, int L,
                                 const double* d_true, int64_t n_true, int nb, int max_returned, int use_th, double near_dup_th,
                                 int64_t* d_out_ids, double* d_out_dists, int32_t* d_out_src, int32_t* d_n_kept, void* stream);

/* A feature store that lives in HBM and changes by kernels (csrc/feat_store.hip): the `put` and the fetch of the reference's
 * HBase feature table (hbase_indexer_minimal.py:779-831) for the exact re-rank above, addressed by the index's device ids.  The
 * store owns a feature matrix [rows][D] in f_dtype (4 = float32, 8 = float64), the row -> id column, and an id -> row table with
 * the layout, hash, probing and -1 = empty of cis_idmap_build_dev, so cis_idmap_lookup_dev and cis_rerank_select_dev read it as it
 * is.  Rows [0, n) are always dense.  Every call enqueues kernels on `stream`; put and remove return after the stream has drained
 * (their counts are read back: one host round trip each, like cis_index_add_dev / cis_index_remove_dev); get does not wait.
 * A store belongs to the device selected when it was created; calls on one store must be stream-ordered by the caller.
 *
 * cis_featstore_reserve: room for `rows` rows and a table that takes them (and as many tombstones) without a rebuild, so that a
 * measured loop allocates nothing (cis_alloc_stats counts every block of a store).  The per-call scratch is sized by the largest
 * batch seen so far.
 *
 * cis_featstore_put_dev: d_ids [n], d_feats [n][D].  Exactly this loop, whatever the thread timing:
 *     for i in range(n):
 *         if ids[i] < 0: skipped += 1; continue
 *         if ids[i] not in row: row[ids[i]] = len(row); new += 1
 *         feats[row[ids[i]]] = batch[i]; row_ids[row[ids[i]]] = ids[i]
 * A stored id is overwritten in place (HBase put: last write wins), an id repeated inside the batch takes one row and keeps its
 * last feature, new ids take rows n, n + 1, ... in order of first occurrence; equal calls give equal bytes.  Rows and table grow as
 * needed: rows into a new block (the old one is freed after the stream has drained), the table by a rebuild from the id column at
 * the next power of two >= 4 (n + batch), which also clears the tombstones.  n <= 2^30.
 *
 * cis_featstore_remove_dev: stored ids of the list leave; unknown, negative and repeated ids are ignored; n = 0 is a no-op.  With k
 * removed and n' = n - k, the removed rows below n' (ascending) are filled by the kept rows at or above n' (ascending), one each:
 * feature row, id and table entry move.  O(k D + k log k), nothing passes over all rows or the whole table; a removed id's table
 * slot becomes a tombstone (key -2) until the next rebuild.  After a removal the row order is NOT the insertion order, and
 * cis_exact_knn_dev over the store breaks exact distance ties by row.
 *
 * cis_featstore_get_dev: d_out_feats [m][D] = the rows of d_ids [m], d_out_rows [m] (or NULL) their rows; an unknown or negative id
 * gives row -1 and a zero-filled feature row.
 *
 * cis_featstore_view: borrowed device pointers for cis_rerank_select_dev, cis_idmap_lookup_dev and cis_exact_knn_dev (any output may
 * be NULL): the matrix, the id column [n], the table (keys, rows, cap) and n.  Any later put or reserve invalidates them. */
typedef struct cis_featstore cis_featstore;
int cis_featstore_create(cis_featstore** out, int D, int f_dtype, int64_t reserve_rows);
void cis_featstore_destroy(cis_featstore* fs);
int64_t cis_featstore_size(cis_featstore* fs);
int cis_featstore_reserve(cis_featstore* fs, int64_t rows, void* stream);
int cis_featstore_put_dev(cis_featstore* fs, const int64_t* d_ids, const void* d_feats, int64_t n, int64_t* n_new,
                          int64_t* n_skipped, void* stream);
int cis_featstore_remove_dev(cis_featstore* fs, const int64_t* d_ids, int64_t n, int64_t* n_removed, void* stream);
int cis_featstore_get_dev(cis_featstore* fs, const int64_t* d_ids, int64_t m, void* d_out_feats, int64_t* d_out_rows, void* stream);
/* Rows [first, first + count) as they lie in the store, copied on `stream`: d_out_feats [count][D] and d_out_ids [count] (either may
 * be NULL).  A range that does not lie inside [0, n) is CIS_EINVAL. */
int cis_featstore_rows_dev(cis_featstore* fs, int64_t first, int64_t count, void* d_out_feats, int64_t* d_out_ids, void* stream);
int cis_featstore_view(cis_featstore* fs, const void** d_feats, const int64_t** d_row_ids, const int64_t** d_keys,
                       const int64_t** d_rows, int64_t* cap, int64_t* n);

/* Exact k nearest neighbours (csrc/lopq_eval.hip): the ground truth of lopq.eval (lopq/lopq/eval.py:7-38: scipy's cdist + argmin /
 * argsort per row).  data [m2][d] and q [m1][d], each float32 or float64 (mixed allowed: the reference promotes both to float64).
 * dist = sqrt(s), s the float64 chain s = s + (x[i] - y[i])^2 for i ascending, every operation rounded on its own -- scipy's value
 * bit for bit.  For every query the min(k, rows seen) rows with the smallest (dist, base + row) in ascending order: idx [m1][k]
 * (-1 padded), dist [m1][k] (NaN padded); equal distances order by index, so k = 1 is np.argmin.  accumulate != 0: the current
 * contents of idx / dist are candidates too (padded entries are empty), so a caller streams data in chunks, in any order, with
 * base = first row of the chunk.  k <= 1024 (CIS_EUNSUPPORTED above).  m1 == 0 or m2 == 0 is CIS_OK.  A NaN distance ranks after
 * every number.  The calls share one process-wide workspace: they must not overlap on two streams or threads.
 * cis_exact_knn_set_mode: 0 = float32 matrix-core prefilter with exact re-check (default), 1 = the exact-only path for every query
 * (tests; both give the same answer). */
int cis_exact_knn_dev(const void* d_data, int data_dtype, int64_t m2, int d, const void* d_q, int q_dtype, int m1, int k,
                      int64_t base, int accumulate, int64_t* d_idx, double* d_dist, void* stream);
int cis_exact_knn(const void* data, int data_dtype, int64_t m2, int d, const void* q, int q_dtype, int m1, int k, int64_t base,
                  int accumulate, int64_t* idx, double* dist);
int cis_exact_knn_set_mode(int mode);
/* Counters of the last internal pass of the last call (at most 8192 queries x 2^24 rows; waits for the device):
 * stats[0] its queries, stats[1] those the exact-only kernel answered, stats[2] rows the prefilter left to re-score for the others. */
int cis_exact_knn_stats(int64_t stats[3]);

/* Lloyd iterations for training the coarse and fine codebooks (lopq/lopq/model.py:339-437 uses scikit-learn k-means;
 * k-means is not bit-reproducible across libraries, so this is judged by distortion).  X [n][d] float32 (host),
 * centroids [k][d] float32: initial centroids in, trained centroids out; k * d <= 7680.  assign [n] (or NULL) and *inertia
 * (sum of squared distances, or NULL) refer to the returned centroids. */
int cis_kmeans(const float* X, int64_t n, int d, int k, int iters, float* centroids, int32_t* assign, double* inertia);

/* The same Lloyd iterations on data that is already on the device, for codebooks of any size (csrc/kmeans_mfma.hip).  Every pointer is
 * a device pointer: d_X [n][d] float32 (never written), d_centroids [k][d] float32 (initial centroids in, trained centroids out),
 * d_assign [n] int32 (or NULL) and d_inertia (one double, or NULL).  `iters` updates are followed by one more assignment pass, so
 * d_assign and *d_inertia describe the returned centroids; iters = 0 only assigns and leaves the centroids' bytes alone.  An empty
 * cluster keeps its centroid's bytes; of equally near centroids the lowest index wins.  The call only enqueues kernels on `stream`
 * and returns without waiting for the device; its grow-only workspace is allocated on the first use of a size.
 * The assignment minimises fl32(|c|^2 - 2 x.c) computed on the float32 matrix cores: with u = 2^-24 and r = |x| + max_c |c| the
 * chosen centroid's true squared distance is at most the minimum + 2 (d + 4) u r^2 (exact on small-integer data).  The inertia is
 * the direct form for the chosen centroid, acc = fmaf(x[i] - c[i], x[i] - c[i], acc) for i ascending, summed in double.  The sums of
 * an update are float32 atomics: centroids may differ in their last bits from run to run, as those of cis_kmeans may.
 * Limits (CIS_EINVAL beyond): 1 <= n <= 2^31 - 256 (int32 assignments), k >= 1, d >= 1, k * d <= 2^30 (32-bit element indices).
 * The calls share one process-wide workspace: they must not overlap on two streams or threads. */
int cis_kmeans_dev(const float* d_X, int64_t n, int d, int k, int iters, float* d_centroids, int32_t* d_assign, double* d_inertia,
                   void* stream);

/* k-means++ seeds (the D^2 draws of Arthur & Vassilvitskii) for cis_kmeans_dev, on data that is already on the device
 * (csrc/kmeans_seed.hip).  Every pointer is a device pointer: d_X [n][d] float32 (never written), d_u [k] float64 uniforms in [0, 1)
 * (the caller supplies the randomness: the call is a deterministic function of its inputs, and two calls with equal inputs give equal
 * bytes), d_centroids [k][d] float32 out (each a row of d_X), d_picked [k] int32 out (the rows; or NULL), d_potential one double out
 * (the sum over rows of the squared distance to the nearest of the k centres; or NULL).  The call only enqueues kernels on `stream`:
 * no host synchronisation, no read-back; its grow-only workspace (n floats and a double per 256 rows) is allocated on the first use
 * of a size.
 *   Centre 0 is row floor(u[0] * n).
 *   d2[r] is float32 in the direct form acc = fmaf(x[i] - c[i], x[i] - c[i], acc), in some fixed order over i: a chosen row and every
 *   copy of it have d2 == 0 exactly.  After centre j, d2[r] = min(d2[r], dist(r, centre j)).
 *   Draw j >= 1: tot = the sum of d2 in float64, t = u[j] * tot (one float64 multiply), and the pick is the smallest r with d2[r] > 0
 *   whose inclusive float64 prefix sum S(r) exceeds t, strictly: a row with d2 == 0 is never picked while tot > 0.  Sums are taken over
 *   fixed tiles of 256 rows with a fixed tree each, whatever the grid; tot and the prefix over tiles are one chain over the tile sums
 *   (the last tile's prefix equals tot bit for bit, and the prefix never decreases); S(r) inside the tile is the tile's prefix plus a
 *   fixed scan of its d2.  If rounding lets that scan run off the tile's end, the tile's last row with d2 > 0 is taken.
 *   If tot == 0 (fewer distinct rows than centres), centre j is row floor(u[j] * n).
 * On small-integer data every d2 and every sum is an exact integer and the picks equal an int64 restatement; otherwise S(r) carries
 * the relative error of the float32 d2, about (d + 2) 2^-24.
 * Limits (CIS_EINVAL beyond, refused before the device is touched): 1 <= n <= 2^31 - 256, k >= 1, d >= 1, k * d <= 2^30; d_X, d_u and
 * d_centroids not NULL.  The calls share one process-wide workspace: they must not overlap on two streams or threads. */
int cis_kmeanspp_dev(const float* d_X, int64_t n, int d, int k, const double* d_u, float* d_centroids, int32_t* d_picked,
                     double* d_potential, void* stream);

/* Training accumulations on the GPU (csrc/lopq_train.hip), float64, host pointers.  Rows of X [n][d] are sorted by group;
 * group_off [groups+1] are the row offsets (group_off[0] = 0, group_off[groups] = n).
 * cis_train_gram:    G[g] = sum_{r in g} x_r x_r^T [groups][d][d] and S[g] = sum x_r [groups][d] (S may be NULL): the np.outer
 *                    accumulators of the PCA covariance (lopq/lopq/model.py:263-267, one group) and of the per-cluster
 *                    residual covariances (:142-155).
 * cis_train_project: Y[r] = R[g] . (x_r - mu[g]) for the rows of group g (compute_local_rotations' projection, :209-234);
 *                    R [groups][d][d] row-major, mu [groups][d]. */
int cis_train_gram(const double* X, int64_t n, int d, const int64_t* group_off, int groups, double* G, double* S);
int cis_train_project(const double* X, int64_t n, int d, const int64_t* group_off, int groups, const double* R,
                      const double* mu, double* Y);

/* The same stage on data that is already on the device: every pointer below is a device pointer, and every call only enqueues
 * kernels on `stream` and returns without waiting.  Sizes are refused with CIS_EINVAL before the device is touched.
 * cis_train_residuals_dev:     d_out[r] = (double)d_X[d_order[r]] - d_C[d_assign[d_order[r]]] for r < rows.  d_X [n][d] float32,
 *                              d_C [groups][d] float64, d_assign [n] int32, d_order [rows] int64, d_out [rows][d] float64.  float32
 *                              minus float64 is exact in double: these are the host path's residuals bit for bit, in the order
 *                              of d_order.  A d_order or d_assign entry outside its array gives a row of NaN.
 * cis_train_gram_dev:          cis_train_gram on d_X [n][d] float64 with the group offsets on the device (d_S may be NULL).
 * cis_train_project_dev:       cis_train_project likewise.  max_group_rows is the largest group's row count (it sizes the grid:
 *                              rows of a group beyond it are not projected).  With d_order [n] int64 (or NULL), row r's result
 *                              goes to row d_order[r] of d_Y [n][d]: a grouped input is written back in its original order.
 *                              The two host entry points above run the same kernels and return the same bits.
 * cis_train_cov_dev:           with n_g = d_group_off[g+1] - d_group_off[g]: d_mu[g] = d_S[g] / n_g (zeros for an empty group)
 *                              and d_cov[g] = (G + G^T) / (2 (n_g - 1)) - mu mu^T from d_G [groups][d][d], or the identity matrix
 *                              where n_g < d (the reference's fallback for a cluster too small for a rotation).
 * cis_train_rotation_pack_dev: d_R[g][i][:] = d_V[g][:, d_perm[g][i]], d_perm [groups][d] int32 (the bucket allocation of the
 *                              eigenvalues), d_V as cis_sym_eig_dev writes it. */
int cis_train_residuals_dev(const float* d_X, int64_t n, int d, const double* d_C, int groups, const int32_t* d_assign,
                            const int64_t* d_order, int64_t rows, double* d_out, void* stream);
int cis_train_gram_dev(const double* d_X, int64_t n, int d, const int64_t* d_group_off, int groups, double* d_G, double* d_S,
                       void* stream);
int cis_train_project_dev(const double* d_X, int64_t n, int d, const int64_t* d_group_off, int groups, int64_t max_group_rows,
                          const double* d_R, const double* d_mu, const int64_t* d_order, double* d_Y, void* stream);
int cis_train_cov_dev(const double* d_G, const double* d_S, const int64_t* d_group_off, int groups, int d, double* d_cov,
                      double* d_mu, void* stream);
int cis_train_rotation_pack_dev(const double* d_V, const int32_t* d_perm, int groups, int d, double* d_R, void* stream);

/* Batched symmetric eigendecomposition in float64 (csrc/sym_eig.hip): cyclic Jacobi in a round-robin ordering, one workgroup per
 * matrix, the matrix in LDS.  Device pointers: d_A [batch][d][d] symmetric (never written), d_W [batch][d] the eigenvalues in
 * ascending order, d_V [batch][d][d] row-major with column j the unit eigenvector of W[j] (numpy.linalg.eigh's layout), d_info
 * [batch] int32 or NULL: the sweeps used, or -1 when the cap of 40 sweeps was reached or the input was not finite; W and V of such a
 * matrix are written and unspecified, and no other matrix of the batch is affected.  Each eigenvector's component of largest
 * magnitude is positive (the lowest index wins a tie), and a matrix's result does not depend on the batch around it.
 * A matrix is done after a full sweep that rotated nothing; a pair (p, q) is left alone when a_pq == 0 or
 * |a_pq| <= 2^-53 sqrt(|a_pp a_qq|).  Measured bounds (tests/test_sym_eig.py, u = 2^-53): |A V - V diag(W)| and |W - eigvalsh(A)|
 * within 16 d u |A|_2, |V^T V - I| within 16 d u.
 * Limits (CIS_EINVAL, before the device is touched): 1 <= d <= 128, batch >= 0 (0: nothing is launched); d_A, d_W and d_V not NULL.
 * The call only enqueues on `stream` and needs no workspace. */
int cis_sym_eig_dev(const double* d_A, int64_t batch, int d, double* d_W, double* d_V, int32_t* d_info, void* stream);

/* Symmetric eigendecomposition of ONE float64 matrix of 1 <= d <= 4096 that lives in HBM (csrc/sym_eig_block.hip): the eigh of the PCA
 * stage of training.  Cyclic two-sided block Jacobi: the matrix is cut into blocks of `block` columns (64 or 32; 0 takes the default:
 * 64 up to d = 128, 32 beyond, the faster of the two at d = 512 ... 4096), block pairs are visited in a round-robin ordering, the
 * disjoint pairs of a round at once: their 2 block x 2 block pivots are diagonalised as one batch by the solver of cis_sym_eig_dev,
 * and A <- Q^T A Q, V <- V Q are float64 tile products.  d need not be a multiple of the block: the matrix is padded with zero rows
 * and columns, which stay exactly decoupled and are dropped at the end.
 * d_A [d][d] symmetric (never written; its lower triangle is read, as by numpy.linalg.eigh), d_W [d], d_V [d][d] and the sign rule as
 * for cis_sym_eig_dev, d_info one int32 or NULL: the block sweeps used, or -1 when the input was not finite, a pivot failed or the
 * cap of 40 block sweeps was reached (W and V are then unspecified).
 * The solve is done after a block sweep in which every pivot's first sweep rotated nothing.  For d <= 128 and block 0 or 64 the
 * matrix is one pivot and d_W holds cis_sym_eig_dev's eigenvalues bit for bit.
 * Bounds (tests/test_sym_eig_large.py at d <= 320, u = 2^-53): |A V - V diag(W)| and |W - eigvalsh(A)| within C d u |A|_2 and
 * |V^T V - I| within C d u, C = 59 for blocks of 32 and 35 for blocks of 64; the pivots' orthogonality errors add up over the rounds.
 * The workspace is the caller's: d_work, device memory aligned to 256 bytes, of at least cis_sym_eig_large_workspace(d) bytes (about
 * 2 (d + 64)^2 doubles; CIS_EINVAL, returned as the int64, for a d outside 1 .. 4096).  Limits (CIS_EINVAL, before the device is
 * touched): 1 <= d <= 4096; block 0, 32 or 64; d_A, d_W, d_V and d_work not NULL; work_bytes at least the workspace.
 * The call enqueues on `stream` and blocks on one 4-byte read-back per block sweep (the status of the sweep's pivots decides whether
 * another follows): when it returns, at most the finalisation is still in flight on `stream`.  It cannot be captured into a graph. */
int64_t cis_sym_eig_large_workspace(int d);
int cis_sym_eig_large_dev(const double* d_A, int d, int block, double* d_W, double* d_V, int32_t* d_info, void* d_work,
                          int64_t work_bytes, void* stream);

/* Counters of the last search on this handle (for bench.py's roofline):
 *   stats[0] candidates scanned (sum over queries of retrieved items on this shard)
 *   stats[1] (query, cell) work items   stats[2] ADC tables built   stats[3] scan kernel launches */
int cis_index_last_stats(cis_index* ix, int64_t stats[4]);
/* Which scan kernel the last batch of this handle ran (bench.py names it in `roofline.kernel`): 0 none (all-candidates path),
 * 1 k_adc_scan (float64), 2 k_adc_scan2 (float32 prefilter), 3 k_adc_scan3 (16-bit fixed-point prefilter: streaming / two-pass form),
 * 4 k_adc_scan4 (the sampled single-pass form of the 16-bit prefilter; k_adc_scan3 then only works off its fall-back slots). */
int cis_index_last_scan_kernel(cis_index* ix);

/* Stage timing with HIP events recorded on the stream the kernels are launched on (bench.py's
 * roofline).  While enabled every search records events around its stages; read_profile waits for
 * them, returns the accumulated milliseconds since the previous read and clears the accumulators:
 *   ms[0] front end (PCA, coarse distances, rank, multisequence plan)   ms[1] ADC tables
 *   ms[2] ADC scan stage (slot list + scan kernel)                        ms[3] per-query merge
 *   ms[4] the ADC scan kernel alone (events right before and after its launch)
 *   *launches = number of scan kernel launches accumulated. */
int cis_index_set_profiling(cis_index* ix, int level /* 0 off, 1 only the pair of events around the scan kernel (ms[4]), 2 every stage */);
/* Ranking route selection: 0 = automatic (limit <= 952: a prefilter scan kernel with exact float64 re-scoring of its
 * survivors -- the 16-bit fixed-point kernel k_adc_scan3 for batches of >= 256 queries over short cells (< 8192 codes on
 * average, M <= 8, limit <= 440), the float32 kernel k_adc_scan2 otherwise; small batches, limit > 952 and indexes of tiny cells
 * (thousands of coarse clusters) take the all-candidates path instead: exact distances of every candidate, radix select;
 * exact float64 scan kernel otherwise), 1 = exact float64 scan kernel wherever it applies (limit <= 3072),
 * 2 = the float32-prefilter kernel for every batch size, 3 / 4 = the 16-bit fixed-point kernel for every batch size in its
 * streaming / two-pass (histogram threshold, then collection) form, 5 = the same kernel family's sampled single-pass form
 * (threshold from a sample of the chunk, verified after the pass; what large batches over short cells take by default),
 * 6 = the HBM-streaming route (csrc/lopq_stream.hip: what batches of <= 16 queries with >= 262144 candidates each take by
 * default -- an exhaustive quota = N run (lopq/lopq/search.py:128-133 consumes whole cells until the quota), or any quota over
 * cells of hundreds of thousands of codes: a sampled threshold per query, one pass over the codes at the HBM rate that lists the
 * few thousand candidates under it, exact float64 keys and ranking of the list, and a proof that the list holds the true top
 * `limit`; a query whose proof fails is answered again by the generic path), 7 = accepted, and sets exactly what 5 sets.
 * All routes produce identical results; the switch exists so that tests can prove it. */
int cis_index_set_scan_mode(cis_index* ix, int mode);
/* counters[0] = batches the HBM-streaming route served, counters[1] = batches it handed back to the generic path (failed proof or
 * overflowed candidate list). */
int cis_index_stream_counters(cis_index* ix, int64_t counters[2]);
int cis_index_read_profile(cis_index* ix, double ms[5], int64_t* launches);

/* ---- CNN descriptors: replaces the caffe forward behind SentiBankPyCaffeImgFeaturizer.featurize -----
 * (cufacesearch/cufacesearch/featurizer/sbpycaffe_img_featurizer.py:137-154; network
 * cufacesearch/cufacesearch/featurizer/data/pycaffe_sentibank.prototxt:1-212).
 * arch CIS_CNN_SENTIBANK: tensors = {conv1_w, conv1_b, ..., conv5_w, conv5_b, fc6_w, fc6_b, fc7_w, fc7_b}
 * (14 float32 arrays in caffe layout: conv OIHW with I = in_channels / group, fc [out][in] over the
 * CHW-flattened blob).  forward: nchw [n][3][227][227] float32 exactly as preprocess_img (:113-134)
 * produces it (BGR, mean subtracted) -> feats [n][4096] float32 = blobs['fc7'] after the in-place ReLU. */
#define CIS_CNN_SENTIBANK 1
/* arch CIS_CNN_DLIB_RESNET: dlib's face-descriptor network behind DLibFeaturizer.featurize
 * (cufacesearch/cufacesearch/featurizer/dlib_featurizer.py:86-105, compute_face_descriptor :105).  The network
 * (dlib's anet_type, 29 convolutions) is third-party and not in the reference tree: oracle/dlib_oracle.py restates it.
 * tensors (117) = conv0 {w OIHW, b, affine gamma, affine beta}, then for each of the 14 residual blocks
 * {w, b, gamma, beta} of its first and of its second 3x3 convolution, then fc [128][256] (no bias).
 * forward input: aligned face chips [n][150][150][3] float32 RGB 0..255 (channels last) -> feats [n][128]. */
#define CIS_CNN_DLIB_RESNET 2
int cis_cnn_create(cis_cnn** out, int arch, const float* const* tensors, int n_tensors);
void cis_cnn_destroy(cis_cnn* c);
int cis_cnn_feat_dim(int arch);
int cis_cnn_forward(cis_cnn* c, const float* nchw, int n, float* feats);
int cis_cnn_forward_dev(cis_cnn* c, const float* d_nchw, int n, float* d_feats, void* stream);
/* A second handle on the same network (round 5): shares the weights of `base` (which must outlive it; a view whose base was destroyed
 * answers CIS_EINVAL), owns its workspaces, streams and events.  Several BATCHES in flight -- one per handle, each on its own stream --
 * fill each other's workgroup rounds: consecutive forwards are in different layers at any time.  From the first view on, base and views
 * run a batch as ONE chain (the two-part forward of the dlib net is for a single handle).  Destroy with cis_cnn_destroy. */
int cis_cnn_create_view(cis_cnn** out, cis_cnn* base);

/* ---- aligned face chips: the image side of dlib's compute_face_descriptor(img, shape) -------------------------------------
 * (cufacesearch/cufacesearch/featurizer/dlib_featurizer.py:103-105).  The caller supplies the 68 landmarks (the shape predictor is
 * not on this path); columbiaimagesearch_amd/featurizer/face_chip.py turns them into dlib's chip_details (get_face_chip_details(shape,
 * 150, 0.25): similarity transform onto the mean face) and into the affine map chip pixel -> source pixel of extract_image_chips.
 * cis_pyramid_down2_dev: dlib's pyramid_down<2> on an RGB uint8 image [nr][nc][3] -> [(nr-3)/2][(nc-3)/2][3] (d_tmp: nr*((nc-3)/2)*3 ints).
 * cis_extract_chips_dev: n chips [n][size][size][3] float32 0..255 (the input of cis_cnn_forward, CIS_CNN_DLIB_RESNET) out of one image
 * or pyramid level by dlib's interpolate_bilinear; d_maps [n][6] float64: source (x, y) = (m0 + m1 c + m2 r, m3 + m4 c + m5 r). */
int cis_pyramid_down2_dev(const uint8_t* d_img, int nr, int nc, uint8_t* d_out, int* d_tmp, void* stream);
int cis_extract_chips_dev(const uint8_t* d_img, int nr, int nc, const double* d_maps, int n, int size, float* d_chips, void* stream);

/* ---- face landmarks: dlib's shape_predictor, the call `self.pred(img, rect)` of DLibFeaturizer.featurize ---------------------------
 * (cufacesearch/cufacesearch/featurizer/dlib_featurizer.py:103).  An ensemble of regression trees (Kazemi and Sullivan 2014) restated
 * from dlib's published image_processing/shape_predictor.h as remembered; parity with dlib itself is UNPINNED (no dlib, no model file
 * here): the yardstick is the numpy model tests/shape_model.py, which csrc/shape_predictor.hip meets bit for bit.
 * The model: P landmarks, K cascade levels of T trees of `depth` levels (S = 2^depth - 1 splits, S + 1 leaves), F feature pixels per
 * level.  initial_shape [2P] (x0, y0, x1, y1, ...), split_idx [K][T][S][2], split_thresh [K][T][S], leaves [K][T][S+1][2P],
 * anchor_idx [K][F], deltas [K][F][2] are HOST arrays; create copies them to the current device.  Limits: 2P <= 256, F <= 4096,
 * T <= 4096, depth <= 8; anchor_idx < P and split_idx < F are checked (CIS_EINVAL, nothing is launched).
 * cis_shapepred_run_dev: one image [nr][nc][3] uint8 RGB and n rectangles (left, top, right, bottom) on the device -> the P landmark
 * pixels of every rectangle, d_parts [n][P][2] (x, y), and, if d_shape is not NULL, the normalised shapes [n][2P] float32.  Only
 * enqueues on `stream`, allocates nothing, returns at once for n = 0; the handle has no workspace, so calls may overlap.
 * cis_dlib_decode_reals: HOST helper of the model reader (featurizer/shape_predictor.py): n floats of dlib's stream serialisation (each
 * an integer mantissa and an integer exponent, value = mantissa * 2^exponent) from buf[*pos...]; advances *pos; at the first bad
 * control byte or at the end of the buffer returns CIS_EINVAL with *pos ON the offending byte. */
typedef struct cis_shapepred cis_shapepred;
int cis_shapepred_create(cis_shapepred** out, int P, int K, int T, int depth, int F, const float* initial_shape,
                         const int32_t* split_idx, const float* split_thresh, const float* leaves, const int32_t* anchor_idx,
                         const float* deltas);
void cis_shapepred_destroy(cis_shapepred* sp);
int cis_shapepred_run_dev(cis_shapepred* sp, const uint8_t* d_img, int nr, int nc, const int32_t* d_rects, int n, int32_t* d_parts,
                          float* d_shape, void* stream);
int cis_dlib_decode_reals(const uint8_t* buf, size_t len, size_t* pos, float* out, size_t n);

/* ---- face detection: dlib's get_frontal_face_detector() scheme, object_detector<scan_fhog_pyramid<pyramid_down<N>>> ---------------
 * (`self.detector.run(img, up_sample, 0)`, cufacesearch/cufacesearch/detector/dlib_detector.py:33).  Restated from dlib's published
 * fhog.h, scan_fhog_pyramid.h and box_overlap_testing.h as remembered; parity with dlib itself is UNPINNED (no dlib, no detector file
 * here, and no real detector file has ever met the reader): the yardstick is the numpy model tests/fhog_model.py, which
 * csrc/hog_detector.hip meets bit for bit.  Known deviations: the saliency is the direct correlation in one stated order (dlib filters
 * separably after an SVD), and one bilinear resize stands in for pyramid_up and pyramid_down<N>.
 * cis_fhogdet_create: F filters of filter_rows x filter_cols x 31 float32 weights, w [F][31][filter_rows][filter_cols] (plane-major, the
 * order of dlib's w vector), and their thresholds [F], HOST arrays copied to the current device.  Checked with CIS_EINVAL before anything
 * is launched: F <= 16, filter sides <= 16, cell_size = 8, 0 <= 2 padding < filter sides, pyramid_n in 2..16, max_levels and the minimal
 * layer size >= 1, finite weights and thresholds, overlap thresholds in [0, 1].
 * cis_fhogdet_workspace_bytes: the workspace one call needs for an nr x nc image (every level's size follows from nr, nc on the host);
 * a negative CIS_E* code on bad arguments.  One workspace serves one call at a time; calls on different streams take different ones.
 * cis_fhogdet_run_dev: d_img [nr][nc][3] uint8 RGB; up_sample 0, 1 or 2.  Only enqueues on `stream` (up_sample + levels - 1 resizes, one
 * 16-byte memset, four kernels), allocates nothing and waits on nothing.  d_rects [max_dets][4] int32 (left, top, right, bottom), the
 * layout cis_shapepred_run_dev takes, d_scores [max_dets] float32, d_filter [max_dets] int32, in the order dlib's run returns them
 * (score descending, ties by level, filter, row, column).  At most max_dets rows are written; d_count[0] holds the number KEPT even if
 * that is larger, so a truncated answer is visible, d_count[1] the number of candidates.  The candidate buffer holds 8192 entries: past
 * that d_count[1] still counts, nothing is written out of bounds, WHICH 8192 candidates took part is arbitrary and the Python surface
 * raises.  More than 48 pyramid levels or more than 2047 cells a side (after up-sampling) are CIS_EINVAL.
 * cis_resize_bilinear_rgb_dev: the resize of the pyramid and of the up-sampling, [nr][nc][3] -> [onr][onc][3] uint8.
 * cis_fhog_extract_dev: Felzenszwalb's 31-plane HOG (dlib's extract_fhog_features) of one image: d_hist [cells_nr][cells_nc][18] float32
 * scratch (cells = (int)(n / 8 + 0.5); the cell histograms are left there), d_feat [31][cells_nr - 2 + pad_rows - 1][cells_nc - 2 +
 * pad_cols - 1] float32 PLANE-MAJOR, the layout the scorer reads, the zero border of (pad - 1) / 2 in front included; pad = 1: none.
 * Fewer than 3 cells a side: returns CIS_OK and writes nothing.
 * cis_fhog_scores_dev: a TEST entry (allocates, copies the HOST weights w and waits): the correlation of every filter at every position
 * of d_feat [31][rows][cols], d_scores [F][rows - filter_rows + 1][cols - filter_cols + 1]; nothing is written where the filter does
 * not fit. */
typedef struct cis_fhogdet cis_fhogdet;
int cis_fhogdet_create(cis_fhogdet** out, int F, int filter_rows, int filter_cols, int cell_size, int padding, int pyramid_n, int max_levels,
                       int min_layer_w, int min_layer_h, const float* w, const float* thresh, double iou_thresh, double covered_thresh);
void cis_fhogdet_destroy(cis_fhogdet* h);
int64_t cis_fhogdet_workspace_bytes(cis_fhogdet* h, int nr, int nc, int up_sample);
int cis_fhogdet_run_dev(cis_fhogdet* h, const uint8_t* d_img, int nr, int nc, int up_sample, double adjust_threshold, void* d_ws,
                        int64_t ws_bytes, int32_t* d_rects, float* d_scores, int32_t* d_filter, int max_dets, int32_t* d_count, void* stream);
/* cis_fhogdet_run_dev with HIP events around its five stages (resizes, cell histograms, features, scores, sort + NMS): WAITS for the call
 * and writes the stage times in milliseconds to the HOST array stage_ms [5] (tools/bench_hog_detector.py). */
int cis_fhogdet_profile(cis_fhogdet* h, const uint8_t* d_img, int nr, int nc, int up_sample, double adjust_threshold, void* d_ws,
                        int64_t ws_bytes, int32_t* d_rects, float* d_scores, int32_t* d_filter, int max_dets, int32_t* d_count, void* stream,
                        float* stage_ms);
int cis_resize_bilinear_rgb_dev(const uint8_t* d_in, int nr, int nc, uint8_t* d_out, int onr, int onc, void* stream);
int cis_fhog_extract_dev(const uint8_t* d_img, int nr, int nc, int cell_size, int pad_rows, int pad_cols, float* d_hist, float* d_feat,
                         void* stream);
int cis_fhog_scores_dev(const float* d_feat, int rows, int cols, int F, int filter_rows, int filter_cols, const float* w, float* d_scores,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIS_HIP_H */
