// The multisequence plan of the batch search (lopq_search.hip): coarse ranking, the frontier walk with its quota cut, the sort-based
// plan for wide vocabularies, the plan scan and the slot builder; the host phases that launch them (declared in lopq_batch.h); and
// the two entry points that are the walk alone -- cis_multisequence and the owner walk of the routed cell-sharded search.
//
// Replaces lopq/lopq/search.py: multisequence :13-82, get_result_quota :110-135.
#include "lopq_batch.h"

// ================================================================================================
// kernels: coarse ranking and multisequence plan
// ================================================================================================
// Ascending order of the V coarse distances of one (query, split).  Distances are >= 0 so their
// bit patterns order like the values (NaN sorts last, as np.argsort does).  Ties -> lower index.
template <typename CT>
__global__ void k_rank(const CT* __restrict__ dist /* [2][nq][V] */, int nq, int V,
                       uint16_t* __restrict__ order /* [nq][2][V] */, CT* __restrict__ sorted /* [nq][2][V] */,
                       int* __restrict__ grp /* [4V]: tables per (split, cluster) and cursors, zeroed here for k_plan */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* sb = reinterpret_cast<uint64_t*>(smem);
    const int q = blockIdx.x, s = blockIdx.y;
    if (q == 0 && s == 0)
        for (int i = threadIdx.x; i < 4 * V * GRP_SUB; i += blockDim.x) grp[i] = 0;
    const CT* d = dist + ((int64_t)s * nq + q) * V;
    for (int v = threadIdx.x; v < V; v += blockDim.x) sb[v] = f2bits(d[v]);
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
        const uint64_t mine = sb[v];
        int r = 0;
        for (int u = 0; u < V; ++u) {
            const uint64_t o = sb[u];
            r += (o < mine) || (o == mine && u < v);
        }
        order[((int64_t)q * 2 + s) * V + r] = (uint16_t)v;
        sorted[((int64_t)q * 2 + s) * V + r] = d[v];
    }
}

// ---- the frontier walk, written once ---------------------------------------------------------------------------------------------
// One wave per query walks the multi-index exactly like lopq/lopq/search.py:58-82.  With two
// splits the traversed set is a Young diagram: t[i] cells taken in rank-row i; the reference's heap
// holds (i, t[i]) for rows with t[i] < V and (i == 0 or t[i-1] > t[i]) and pops the smallest
// (dist, i, j) with dist = d0[i] + d1[j] rounded in the coarse compute type.
// The pieces are inlined into their four callers, so d0 / d1 / o0 / o1 keep the address space the caller has them in (LDS in
// k_front_small, global memory in the others): no generic pointers.
static const uint32_t WALK_NONE = ~0u;

// One step: the frontier's minimum over rows [0, rows), key = (dist bits, i, j) -> i << 16 | j, the same in every lane; WALK_NONE
// when the frontier is empty (cannot happen before all cells are visited).  FIRST_ALONE: skip the reduction while rows == 1 -- only
// lane 0 holds a candidate then, so the result is the same (k_front_small, whose walks are a few steps long, is compiled with it).
template <typename CT, bool FIRST_ALONE>
static __device__ __forceinline__ uint32_t walk_step(const CT* d0, const CT* d1, const int* t, int rows, int V, int lane) {
    uint64_t bk = ~0ull;
    uint32_t bij = WALK_NONE;
    for (int i = lane; i < rows; i += 64) {
        const int j = t[i];
        if (j >= V) continue;
        if (i > 0 && t[i - 1] <= j) continue;
        const CT dist = d0[i] + d1[j];
        const uint64_t kb = f2bits(dist);
        const uint32_t ij = ((uint32_t)i << 16) | (uint32_t)j;
        if (kb < bk || (kb == bk && ij < bij)) { bk = kb; bij = ij; }
    }
    if (!FIRST_ALONE || rows > 1) {  // wave-uniform
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t ok = __shfl_xor(bk, off);
            const uint32_t oij = __shfl_xor(bij, off);
            if (ok < bk || (ok == bk && oij < bij)) { bk = ok; bij = oij; }
        }
    } else {
        bij = (uint32_t)__builtin_amdgcn_readfirstlane((int)bij);
    }
    return bij;
}

// The cell (bi, bj) leaves the frontier; rows [0, rows) can be on it.
static __device__ __forceinline__ void walk_advance(int* t, int& rows, int V, int lane, int bi, int bj) {
    __syncthreads();
    if (lane == 0) t[bi] = bj + 1;
    if (bi + 2 > rows) rows = (bi + 2 < V) ? bi + 2 : V;
    __syncthreads();
}

// The walk up to the quota (search.py:128-133: the test follows the append, so one cell is always visited): visit(rank, bi, bj, cell,
// gc, ls, ll) for every cell in visit order -- gc its size over all shards, [ls, ls + ll) its candidates on this shard (LISTS; else
// only gcount is read and both are 0).  Returns the number of visited cells.
template <typename CT, bool FIRST_ALONE, bool LISTS, typename Visit>
static __device__ __forceinline__ int walk_quota(const CT* d0, const CT* d1, const uint16_t* o0, const uint16_t* o1, int* t, int V, int lane,
                                                 const int64_t* __restrict__ gcount, const int64_t* __restrict__ loff, int64_t quota, Visit visit) {
    int visited = 0;
    int64_t retrieved = 0;
    int rows = 1;
    const int64_t total_cells = (int64_t)V * V;
    while ((int64_t)visited < total_cells) {
        const uint32_t bij = walk_step<CT, FIRST_ALONE>(d0, d1, t, rows, V, lane);
        if (bij == WALK_NONE) break;
        const int bi = (int)(bij >> 16), bj = (int)(bij & 0xffff);
        const int c0 = o0[bi], c1 = o1[bj];
        const int64_t cell = (int64_t)c0 * V + c1;
        const int64_t gc = gcount[cell];
        int64_t ls = 0, ll = 0;
        if constexpr (LISTS) {
            ls = loff[cell];
            ll = loff[(int64_t)V * V + 1 + cell] - ls;  // the used end (lend = loff + ncells + 1: cells keep insert slack behind their items)
        }
        visit(visited, bi, bj, cell, gc, ls, ll);
        visited += 1;
        retrieved += gc;
        walk_advance(t, rows, V, lane, bi, bj);
        if (retrieved >= quota) break;
    }
    return visited;
}

// tables per (split, cluster): k_tables handles the tables of one cluster together (one read of R[c]); g = split * V + cluster
static __device__ __forceinline__ void count_table_group(int* __restrict__ grp_cnt, int g, int q) {
    atomicAdd(&grp_cnt[g * GRP_SUB + (q % GRP_SUB)], 1);
}

// What a counting pass of the walk leaves: the query's PlanOut and its table groups (ranks [0, max_i] and [0, max_j] of the two lists).
static __device__ __forceinline__ void walk_count_out(PlanOut* __restrict__ plan, int* __restrict__ grp_cnt, const uint16_t* o0, const uint16_t* o1,
                                                      int V, int q, int lane, int visited, int n_items, int max_i, int max_j, int64_t ncand) {
    if (lane == 0) {
        PlanOut p;
        p.visited = visited; p.n_items = n_items; p.ntab0 = max_i + 1; p.ntab1 = max_j + 1; p.ncand = ncand;
        plan[q] = p;
    }
    for (int i = lane; i < max_i + 1 + max_j + 1; i += 64)
        count_table_group(grp_cnt, i <= max_i ? (int)o0[i] : V + (int)o1[i - (max_i + 1)], q);
}

// The work items of one visited cell, one per chunk of seg_max candidates: chunks ch0, ch0 + step, ... < nch -> dst[ch].
static __device__ __forceinline__ void emit_chunks(WorkItem* __restrict__ dst, int q, int rank, int tab0, int tab1, int64_t cell, int64_t ls,
                                                   int64_t ll, int seg_max, int nch, int ch0, int step) {
    for (int ch = ch0; ch < nch; ch += step) {
        WorkItem it;
        it.q = q; it.rank = rank;
        it.tab0 = tab0;
        it.tab1 = tab1;
        it.pos0 = ch * seg_max;
        it.cell = (int)cell; it.pad = 0;
        it.start = ls + (int64_t)ch * seg_max;
        const int64_t rem = ll - (int64_t)ch * seg_max;
        it.len = (int)(rem < seg_max ? rem : seg_max);
        dst[ch] = it;
    }
}

// The plan by the frontier walk: counting pass (!EMIT), then, after the plan scan, the emitting pass.
template <typename CT, bool EMIT>
__global__ __launch_bounds__(64) void k_plan(const CT* __restrict__ sorted, const uint16_t* __restrict__ order,
                                             const int64_t* __restrict__ gcount, const int64_t* __restrict__ loff,
                                             int nq, int V, int64_t quota, int seg_max, PlanOut* __restrict__ plan,
                                             const int64_t* __restrict__ item_off, const int64_t* __restrict__ tab_off,
                                             WorkItem* __restrict__ items, TabDesc* __restrict__ tabs,
                                             int* __restrict__ grp_cnt /* [2V] */, const int* __restrict__ grp_base /* [2V] */,
                                             int* __restrict__ grp_cur /* [2V] */, int* __restrict__ tab_order /* [n_tabs] */,
                                             const int* __restrict__ only /* null, or [nq]: walk only the flagged queries (k_plan_par's fallback) */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* t = reinterpret_cast<int*>(smem);  // [V]
    const int q = blockIdx.x;
    const int lane = threadIdx.x;
    if (only && !only[q]) return;
    const CT* d0 = sorted + ((int64_t)q * 2 + 0) * V;
    const CT* d1 = sorted + ((int64_t)q * 2 + 1) * V;
    const uint16_t* o0 = order + ((int64_t)q * 2 + 0) * V;
    const uint16_t* o1 = order + ((int64_t)q * 2 + 1) * V;
    for (int i = lane; i < V; i += 64) t[i] = 0;
    __syncthreads();
    int n_items = 0, max_i = -1, max_j = -1;
    int64_t ncand = 0;
    int64_t ibase = 0, tbase = 0;
    int ntab0 = 0;
    if (EMIT) {
        ibase = item_off[q];
        tbase = tab_off[q];
        ntab0 = plan[q].ntab0;
    }
    const int visited = walk_quota<CT, false, true>(d0, d1, o0, o1, t, V, lane, gcount, loff, quota,
                                                    [&](int rank, int bi, int bj, int64_t cell, int64_t, int64_t ls, int64_t ll) {
        if (ll > 0) {
            const int nch = (int)((ll + seg_max - 1) / seg_max);
            if (EMIT) emit_chunks(items + ibase + n_items, q, rank, (int)(tbase + bi), (int)(tbase + ntab0 + bj), cell, ls, ll, seg_max, nch, lane, 64);
            n_items += nch;
            ncand += ll;
            max_i = bi > max_i ? bi : max_i;
            max_j = bj > max_j ? bj : max_j;
        }
    });
    if (!EMIT) {
        walk_count_out(plan, grp_cnt, o0, o1, V, q, lane, visited, n_items, max_i, max_j, ncand);
    } else {
        const int nt0 = plan[q].ntab0, nt1 = plan[q].ntab1;
        for (int i = lane; i < nt0 + nt1; i += 64) {
            TabDesc td;
            td.q = q; td.pad = 0;
            if (i < nt0) { td.split = 0; td.cluster = o0[i]; }
            else { td.split = 1; td.cluster = o1[i - nt0]; }
            tabs[tbase + i] = td;
            const int g = (td.split * V + td.cluster) * GRP_SUB + (q % GRP_SUB);
            tab_order[grp_base[g] + atomicAdd(&grp_cur[g], 1)] = (int)(tbase + i);  // order inside a group does not matter
        }
    }
}

// Fused front end for small coarse codebooks (V <= 64: BASELINE configs C1-C5): the exact coarse distances of k_sqdist_rows2
// (lopq/lopq/search.py:39 -> lopq/lopq/utils.py:33-53 arithmetic: numpy's pairwise order, compute type CT), the ascending rank of
// k_rank (np.argsort, ties to the lower index) and the counting pass of the multisequence walk (k_plan<CT, false>) in ONE launch, one
// wave per query: the 2 V distances never leave the CU between the three steps (three launches and two round trips through L2 of
// the [2][nq][V] arrays before).  `sorted` / `order` still go to global memory for the emit pass and the tables.
template <typename CT>
__global__ __launch_bounds__(64) void k_front_small(const CT* __restrict__ X /* [nq][D] */, int D, int h, const CT* __restrict__ Cs /* [2][V][h] */,
                                                    PwProg prog, const int64_t* __restrict__ gcount, const int64_t* __restrict__ loff,
                                                    int nq, int V, int64_t quota, int seg_max, uint16_t* __restrict__ order /* [nq][2][V] */,
                                                    CT* __restrict__ sorted /* [nq][2][V] */, PlanOut* __restrict__ plan,
                                                    int* __restrict__ grp_cnt /* zeroed by the previous batch's k_plan_scan */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* sb = reinterpret_cast<uint64_t*>(smem);            // [2V] distance bits
    CT* sd = reinterpret_cast<CT*>(sb + 2 * V);                  // [2][V] ascending distances
    uint16_t* so = reinterpret_cast<uint16_t*>(sb + 4 * V);      // [2][V] cluster of every rank (8 bytes reserved per value of sd)
    int* t = reinterpret_cast<int*>(so + 2 * V);                 // [V] frontier
    const int q = blockIdx.x, lane = threadIdx.x;
    const CT* xr = X + (int64_t)q * D;
    for (int e = lane; e < 2 * V; e += 64) {
        const int s = e / V, c = e - s * V;
        const CT* x = xr + s * h;
        const CT* cc = Cs + ((int64_t)s * V + c) * h;
        auto elem = [&](int i) -> CT { const CT df = x[i] - cc[i]; return df * df; };
        const CT d = pw_sum<CT>(prog, elem);
        sb[e] = f2bits(d);
    }
    for (int i = lane; i < V; i += 64) t[i] = 0;
    __syncthreads();
    for (int e = lane; e < 2 * V; e += 64) {
        const int s = e / V, v = e - s * V;
        const uint64_t mine = sb[e];
        int r = 0;
        for (int u = 0; u < V; ++u) {
            const uint64_t o = sb[s * V + u];
            r += (o < mine) || (o == mine && u < v);
        }
        CT d;
        if constexpr (sizeof(CT) == 4) d = __uint_as_float((uint32_t)mine);
        else d = __longlong_as_double((long long)mine);
        sd[s * V + r] = d;
        so[s * V + r] = (uint16_t)v;
        order[((int64_t)q * 2 + s) * V + r] = (uint16_t)v;
        sorted[((int64_t)q * 2 + s) * V + r] = d;
    }
    __syncthreads();
    const CT* d0 = sd;
    const CT* d1 = sd + V;
    const uint16_t* o0 = so;
    const uint16_t* o1 = so + V;
    // the counting pass of k_plan (same frontier walk, inputs in LDS)
    int n_items = 0, max_i = -1, max_j = -1;
    int64_t ncand = 0;
    const int visited = walk_quota<CT, true, true>(d0, d1, o0, o1, t, V, lane, gcount, loff, quota,
                                                   [&](int, int bi, int bj, int64_t, int64_t, int64_t, int64_t ll) {
        if (ll > 0) {
            n_items += (int)((ll + seg_max - 1) / seg_max);
            ncand += ll;
            max_i = bi > max_i ? bi : max_i;
            max_j = bj > max_j ? bj : max_j;
        }
    });
    walk_count_out(plan, grp_cnt, o0, o1, V, q, lane, visited, n_items, max_i, max_j, ncand);
}

// The same plan for indexes with thousands of coarse clusters (the reference's release configurations use V = 2048 / 4096:
// millions of tiny cells, hundreds to thousands of cells per query at quota 10000), where one frontier step per visited
// cell is the whole cost of a search.  The multisequence order is the order of the sums s(i, j) = fl(d0[i] + d1[j]) (rank
// pairs, both lists ascending): the heap of lopq/lopq/search.py:58-82 holds (s, (i, j)) keys and a cell enters it when both
// its predecessors (i-1, j), (i, j-1) have been popped.  Those are componentwise smaller, so their keys are smaller too (s is
// monotone in i and j, the pair breaks ties): by induction everything with a smaller key is popped before a given cell, i.e.
// the heap's order IS the sorted order of the keys, ties included.  So, per query and with one workgroup:
//   1. bisection on the VALUE tau (bit patterns order like the non-negative sums): count of {s <= tau} = sum over rows of a
//      prefix length (binary search along the ascending d1), until about `target` cells are inside;
//   2. the cells {s <= tau} are enumerated into LDS with the global sizes of their cells and sorted by (s, i, j) (bitonic);
//   3. a prefix sum of the cell sizes in that order finds the quota cut (search.py:128-133); too few candidates inside ->
//      target * 4 and again;
//   4. a band that cannot be cut below what the workgroup sorts (thousands of equal sums), or more visited cells than the
//      list holds: the query is flagged and the frontier walk above (k_plan with `only`) handles it.
// The count pass leaves the visited (i, j) list in global memory for the emit pass.
#ifdef CIS_PLAN_DBG  // tools/build_variant.sh plandbg -DCIS_PLAN_DBG lopq_plan: probes / bands / cycles per phase of k_plan_par's count pass
__device__ unsigned long long g_plan_dbg[12];
#define PLAN_DBG(i, v) do { if (threadIdx.x == 0) atomicAdd(&g_plan_dbg[i], (unsigned long long)(v)); } while (0)
#else
#define PLAN_DBG(i, v) do { } while (0)
#endif
static const int PLAN_PAR_CAP = 2048;   // cells a workgroup enumerates and sorts per band
static const int PLAN_NB_LOG = 10, PLAN_NB = 1 << PLAN_NB_LOG;  // buckets of a band's distribution sort

// all of d0 / d1 is staged in LDS (V <= PLAN_PAR_STAGE); read in place (no generic pointers to the LDS arrays)
#ifndef CIS_PLAN_WPE
#define CIS_PLAN_WPE 3
#endif
static const int PLAN_SP = 1024;        // ... of which the first PLAN_SP ranks of either list are staged in LDS (the rest is read in place)
template <typename CT> struct PlanKeyT { typedef uint64_t type; };
template <> struct PlanKeyT<float> { typedef uint32_t type; };
#define PL0(i) ((i) < SP ? s_d0[(i)] : d0[(i)])
#define PL1(i) ((i) < SP ? s_d1[(i)] : d1[(i)])

template <typename CT, bool EMIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CIS_PLAN_WPE))) void k_plan_par(const CT* __restrict__ sorted, const uint16_t* __restrict__ order,
                                                  const int64_t* __restrict__ gcount, const int64_t* __restrict__ loff,
                                                  int nq, int V, int64_t quota, int seg_max, PlanOut* __restrict__ plan,
                                                  const int64_t* __restrict__ item_off, const int64_t* __restrict__ tab_off,
                                                  WorkItem* __restrict__ items, TabDesc* __restrict__ tabs,
                                                  int* __restrict__ grp_cnt, const int* __restrict__ grp_base,
                                                  int* __restrict__ grp_cur, int* __restrict__ tab_order,
                                                  uint64_t* __restrict__ ent_list /* [nq][ent_cap][2]: the visited cells that hold anything, in visit
                                                  order: start (40 bits) | (i << 12 | j) << 40, then length | visit rank << 32 */,
                                                  int* __restrict__ fallback /* [nq] flags, then [nq] entries per query */, int ent_cap,
                                                  unsigned long long* __restrict__ hint /* null, or [2][2]: (cells visited, quota) summed over the
                                                  queries of the launches of either parity (count pass) */, int hint_slot) {
    __shared__ typename PlanKeyT<CT>::type s_key[PLAN_PAR_CAP];
    __shared__ uint32_t s_ij[PLAN_PAR_CAP];
    __shared__ uint32_t s_gc[PLAN_PAR_STAGE];  // row starts of the band (one per active row, <= V), then the cells' sizes (<= PLAN_PAR_CAP)
    // d0, d1: the first SP ranks of either (count pass).  A query of the release operating points touches a few hundred ranks; staging
    // all 2 x 4096 took 32 KB and held the kernel at two workgroups per CU -- it is bound by latency (barriers, dependent LDS and
    // global reads), three hide more of it.
    extern __shared__ __align__(16) unsigned char s_plan_dyn[];
    const int SP = V < PLAN_SP ? V : PLAN_SP;
    CT* s_d0 = reinterpret_cast<CT*>(s_plan_dyn);
    CT* s_d1 = s_d0 + SP;
    __shared__ int s_hist[PLAN_NB];  // the band's distribution sort: bucket sizes, then bucket starts
    __shared__ int64_t s_red[8];
    __shared__ int s_i[8];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long dbg_k0 = wall_clock64();
    (void)dbg_k0;
    const CT* d0 = sorted + ((int64_t)q * 2 + 0) * V;
    const CT* d1 = sorted + ((int64_t)q * 2 + 1) * V;
    const uint16_t* o0 = order + ((int64_t)q * 2 + 0) * V;
    const uint16_t* o1 = order + ((int64_t)q * 2 + 1) * V;
    uint64_t* ent = ent_list + (int64_t)q * ent_cap * 2;
    auto block_sum = [&](int64_t v) -> int64_t {  // every thread gets the sum
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        __syncthreads();
        if (lane == 0) s_red[wv] = v;
        __syncthreads();
        const int64_t t = s_red[0] + s_red[1] + s_red[2] + s_red[3];
        // the same value in every lane: say so (scalar registers, uniform branches on it)
        return ((int64_t)__builtin_amdgcn_readfirstlane((int)(t >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)t);
    };
    if constexpr (EMIT) {
        if (fallback[q]) return;  // the frontier walk emits this query
        const int n_ent = fallback[nq + q];
        const PlanOut pl = plan[q];
        const int64_t ibase = item_off[q], tbase = tab_off[q];
        // the ranks of either list that have a cell with candidates, as bits; a half table per set bit, numbered densely in rank order
        // (the count pass counted the same bits into ntab0 / ntab1)
        __shared__ uint32_t s_used[2 * PLAN_PAR_STAGE / 32];
        __shared__ uint16_t s_pre[2 * PLAN_PAR_STAGE / 32];
        constexpr int UW = PLAN_PAR_STAGE / 32;  // words per split
        s_used[tid] = 0u;
        __syncthreads();
        for (int idx = tid; idx < n_ent; idx += 256) {
            const uint64_t e0 = ent[2 * idx], e1 = ent[2 * idx + 1];
            if ((uint32_t)e1 > 0u) {
                const int bi = (int)(e0 >> 52), bj = (int)((e0 >> 40) & 0xfffu);
                atomicOr(&s_used[bi >> 5], 1u << (bi & 31));
                atomicOr(&s_used[UW + (bj >> 5)], 1u << (bj & 31));
            }
        }
        __syncthreads();
        {
            const int pc = __popc(s_used[tid]);
            int x = pc;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(x, d);
                if (lane >= d) x += y;
            }
            if (lane == 63) s_i[wv] = x;
            __syncthreads();
            s_pre[tid] = (uint16_t)(((wv & 1) ? s_i[wv - 1] : 0) + x - pc);  // waves 0, 1: split 0; waves 2, 3: split 1
        }
        __syncthreads();
        auto dense = [&](int split, int r) -> int {
            const int w = split * UW + (r >> 5);
            return (int)s_pre[w] + __popc(s_used[w] & ((1u << (r & 31)) - 1u));
        };
        // items: exclusive scan of the chunk counts of the listed cells, in visit order
        int run = 0;
        for (int b0 = 0; b0 < n_ent; b0 += 256) {
            const int idx = b0 + tid;
            int nch = 0, bi = 0, bj = 0, rank = 0;
            int64_t ls = 0, ll = 0;
            if (idx < n_ent) {
                const uint64_t e0 = ent[2 * idx], e1 = ent[2 * idx + 1];
                bi = (int)(e0 >> 52); bj = (int)((e0 >> 40) & 0xfffu);
                ls = (int64_t)(e0 & ((1ull << 40) - 1));
                ll = (int64_t)(uint32_t)e1;
                rank = (int)(e1 >> 32);
                nch = ll > 0 ? (int)((ll + seg_max - 1) / seg_max) : 0;
            }
            int x = nch;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(x, d);
                if (lane >= d) x += y;
            }
            __syncthreads();
            if (lane == 63) s_i[wv] = x;
            __syncthreads();
            int base = run;
            for (int w = 0; w < wv; ++w) base += s_i[w];
            const int pos = base + x - nch;
            if (nch > 0) {
                const int64_t cell = (int64_t)o0[bi] * V + o1[bj];
                const int t0 = (int)tbase + dense(0, bi), t1 = (int)tbase + pl.ntab0 + dense(1, bj);
                emit_chunks(items + ibase + pos, q, rank, t0, t1, cell, ls, ll, seg_max, nch, 0, 1);
            }
            run += s_i[0] + s_i[1] + s_i[2] + s_i[3];
        }
        // tables: a thread per rank of either list (a thread per word walking its bits ran the 16 tables of a V = 16 query one after the
        // other, each behind a load and an atomic's return)
        for (int x = tid; x < 2 * V; x += 256) {
            const int split = x >= V ? 1 : 0, r = x - split * V;
            if ((s_used[split * UW + (r >> 5)] >> (r & 31)) & 1u) {
                TabDesc td;
                td.q = q; td.pad = 0; td.split = split;
                td.cluster = split ? o1[r] : o0[r];
                const int ti = (int)tbase + (split ? pl.ntab0 : 0) + dense(split, r);
                tabs[ti] = td;
                const int g = (td.split * V + td.cluster) * GRP_SUB + (q % GRP_SUB);
                tab_order[grp_base[g] + atomicAdd(&grp_cur[g], 1)] = ti;
            }
        }
        return;
    } else {
        for (int i = tid; i < SP; i += 256) { s_d0[i] = d0[i]; s_d1[i] = d1[i]; }
        __syncthreads();
        // A thread owns the rows i = tid + 256 k and keeps three prefix lengths of each in registers: under the last band's tau
        // (`pprev`), under the bisection's lower end (`plo`: a tau below every later probe) and under its upper end (`phi`, exact).
        // A probe searches [plo, phi] only -- a step or two instead of log2 V -- and the band's enumeration needs no search at all.
        constexpr int KR = PLAN_PAR_STAGE / 256;
        int pprev[KR];
        uint32_t pbr[KR];  // plo | phi << 16 (prefix lengths <= 4096)
#pragma unroll
        for (int k = 0; k < KR; ++k) { pprev[k] = 0; pbr[k] = 0; }
        // first j of [lo_, hi_] with fl(a + d1[j]) > tau (hi_ when there is none below it)
        auto prefix_in = [&](CT a, uint64_t tau, int lo_, int hi_) -> int {
            while (lo_ < hi_) {
                const int mid = (lo_ + hi_) >> 1;
                if (f2bits((CT)(a + PL1(mid))) <= tau) lo_ = mid + 1;
                else hi_ = mid;
            }
            return lo_;
        };
        // the same over [lo_, V]: the staged part first
        auto prefix_from = [&](CT a, uint64_t tau, int lo_) -> int {
            if (SP < V && lo_ < SP) {
                if (f2bits((CT)(a + s_d1[SP - 1])) > tau) return prefix_in(a, tau, lo_, SP - 1);
                lo_ = SP;
            }
            return prefix_in(a, tau, lo_, V);
        };
        // rows with a cell under tau: first i with fl(d0[i] + d1[0]) > tau (every thread reads the same words: a uniform value)
        auto rows_under = [&](uint64_t tau) -> int {
            int lo_ = 0, hi_ = V;
            const CT b0 = s_d1[0];
            if (SP < V) {
                if (f2bits((CT)(s_d0[SP - 1] + b0)) > tau) hi_ = SP - 1;
                else lo_ = SP;
            }
            while (lo_ < hi_) {
                const int mid = (lo_ + hi_) >> 1;
                if (f2bits((CT)(PL0(mid) + b0)) <= tau) lo_ = mid + 1;
                else hi_ = mid;
            }
            return __builtin_amdgcn_readfirstlane(lo_);
        };
        // Bands of increasing tau: band b holds the cells with tau_{b-1} < s <= tau_b (at most PLAN_PAR_CAP of them), is
        // sorted on its own and appended to the visited list; the quota prefix sum carries over.
        PLAN_DBG(8, wall_clock64() - dbg_k0);
        bool fb = false, done = false;
        int visited = 0, ne_total = 0;
        int64_t cum = 0, c_prev = 0, target = 256;
        // first band: 0.6 x the cells a query of this quota visited in the previous launch (so that [target, 2 target] holds what most
        // queries need and ONE band is enumerated and sorted); 256 without a hint.  The hint only sizes the bands.
        if (hint && quota > 0) {
            const unsigned long long hv = hint[(hint_slot ^ 1) * 2], hq = hint[(hint_slot ^ 1) * 2 + 1];
            if (hq > 0) {
                const double t0 = 0.6 * (double)hv / (double)hq * (double)quota;
                target = t0 < 64.0 ? 64 : (t0 > (double)(PLAN_PAR_CAP / 2) ? PLAN_PAR_CAP / 2 : (int64_t)t0);
            }
        }
        bool have_prev = false;
        uint64_t tau_prev = 0;
        const int64_t all_cells = (int64_t)V * V;
        const uint64_t s_min = f2bits((CT)(PL0(0) + PL1(0)));
        if (quota <= 0) { target = 1; }  // the test follows the first append (search.py:131-132): one cell
        while (!done && !fb) {
            const int64_t left = all_cells - c_prev;
            if (left <= 0) break;  // every cell visited, quota not reached
            const int64_t want = target < left ? target : left;
            // tau with want <= #{tau_prev < s <= tau} <= 2 * want (or the smallest tau that reaches `want` when values repeat).
            // Upper end to start from: the a x a square of rank pairs lies under fl(d0[a-1] + d1[a-1]) (the sums are monotone in both
            // ranks), so with a * a >= c_prev + want that tau holds the band; it is ~2 x too large (the region under a tau is closer to
            // a triangle than a square), so a few probes finish -- and every probe sees few active rows (from s_max the first probes
            // searched all V rows).
            const uint64_t lo_key = have_prev ? tau_prev + 1 : s_min;
            uint64_t lo = lo_key, hi;
            {
                const int64_t need = c_prev + want;
                int64_t a = (int64_t)sqrt((double)need);
                while (a * a < need) ++a;
                while (a > 1 && (a - 1) * (a - 1) >= need) --a;
                if (a > V) a = V;
                hi = f2bits((CT)(PL0((int)a - 1) + PL1((int)a - 1)));
            }
            const long long dbg_t0 = wall_clock64();
            (void)dbg_t0;
            const int R0 = rows_under(hi);
            int64_t c_hi;
            {
                int64_t c = 0;
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    int ph = pprev[k];
                    if (k * 256 < R0) {
                        const int i = k * 256 + tid;
                        if (i < R0) ph = prefix_from(PL0(i), hi, pprev[k]);
                        c += ph;
                    }
                    pbr[k] = (uint32_t)pprev[k] | ((uint32_t)ph << 16);
                }
                c_hi = block_sum(c);
                PLAN_DBG(0, 1);
            }
            while (c_hi - c_prev > 2 * want && lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                uint16_t pm[KR];
                int64_t c = 0;
#pragma unroll
                for (int k = 0; k < KR; ++k) {
                    pm[k] = (uint16_t)(pbr[k] & 0xffffu);
                    if (k * 256 < R0) {
                        const int i = k * 256 + tid;
                        if (i < R0) pm[k] = (uint16_t)prefix_in(PL0(i), mid, (int)(pbr[k] & 0xffffu), (int)(pbr[k] >> 16));
                        c += pm[k];
                    }
                }
                c = block_sum(c);
                PLAN_DBG(0, 1);
                if (c - c_prev >= want) {
                    hi = mid; c_hi = c;
#pragma unroll
                    for (int k = 0; k < KR; ++k) pbr[k] = (pbr[k] & 0xffffu) | ((uint32_t)pm[k] << 16);
                } else {
                    lo = mid + 1;
#pragma unroll
                    for (int k = 0; k < KR; ++k) pbr[k] = (pbr[k] & 0xffff0000u) | (uint32_t)pm[k];
                }
            }
            PLAN_DBG(1, 1);
            PLAN_DBG(2, wall_clock64() - dbg_t0);
            if (c_hi - c_prev > PLAN_PAR_CAP) { fb = true; break; }
            const int cnt = (int)(c_hi - c_prev);
            // enumerate the band.  (a) per row: cells [pprev, phi); s_gc[i] = first slot of the row | pprev << 12 (rows in order)
            const int rows = rows_under(hi);
            for (int x = tid; x < PLAN_NB; x += 256) s_hist[x] = 0;
            int run = 0;
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                if (k * 256 < rows) {
                    const int i = k * 256 + tid;
                    const int p = i < rows ? (int)(pbr[k] >> 16) - pprev[k] : 0;
                    int x = p;
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) {
                        const int y = __shfl_up(x, d);
                        if (lane >= d) x += y;
                    }
                    __syncthreads();
                    if (lane == 63) s_i[wv] = x;
                    __syncthreads();
                    int base = run;
                    for (int w = 0; w < wv; ++w) base += s_i[w];
                    if (i < rows) s_gc[i] = (uint32_t)(base + x - p) | ((uint32_t)pprev[k] << 12);
                    run += s_i[0] + s_i[1] + s_i[2] + s_i[3];
                }
            }
            __syncthreads();
            PLAN_DBG(5, wall_clock64() - dbg_t0);
            // (b) one thread per cell: row by binary search over the row starts (the LAST row whose start is <= e is the
            // one that holds e: empty rows share their start with the next row), then sum, rank pair and GLOBAL cell size
            constexpr int PER = PLAN_PAR_CAP / 256;
            // (the global reads of the thread's PER cells go out together, level by level -- cluster ids, then sizes: as
            // `if (e < cnt) { ... gcount[o0[i] * V + o1[j]] }` per cell they were 2 x PER round trips in a row, ~25 us per band)
            uint32_t eij[PER];
            uint64_t ekey[PER];
            int ei[PER], ej[PER];
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int e = r * 256 + tid;
                ei[r] = 0; ej[r] = 0; ekey[r] = 0; eij[r] = 0;
                if (e < cnt) {
                    int lo_ = 0, hi_ = rows;  // first row whose start is > e
                    while (lo_ < hi_) {
                        const int mid = (lo_ + hi_) >> 1;
                        if ((int)(s_gc[mid] & 0xfffu) <= e) lo_ = mid + 1;
                        else hi_ = mid;
                    }
                    const int i = lo_ - 1;
                    const uint32_t w = s_gc[i];
                    const int j = e - (int)(w & 0xfffu) + (int)(w >> 12);
                    ekey[r] = f2bits((CT)(PL0(i) + PL1(j)));
                    eij[r] = ((uint32_t)i << 16) | (uint32_t)j;
                    ei[r] = i; ej[r] = j;
                }
            }
            uint16_t ci[PER], cj[PER];
#pragma unroll
            for (int r = 0; r < PER; ++r) { ci[r] = o0[ei[r]]; cj[r] = o1[ej[r]]; }
            int64_t gg[PER];
#pragma unroll
            for (int r = 0; r < PER; ++r) gg[r] = gcount[(int64_t)ci[r] * V + cj[r]];
            // Sort by (s, i, j) as a distribution sort: the keys lie in (tau_prev, tau], a bucket is a slice of that range (the key
            // minus its lower end, shifted down to PLAN_NB values: monotone), a cell takes the next slot of its bucket (an LDS counter),
            // the buckets' sizes are scanned, and a cell's rank is its bucket's start + the cells of the bucket that order before it (a
            // cell or two per bucket; tied sums pile up in one bucket and are ordered by the rank pair there -- quadratic only in the
            // size of a tie group).  The bitonic network this replaces was 32-47 us of a band's ~80 us.
            int bk[PER], slot[PER];
            {
                const uint64_t range = hi - lo_key;
                const int nbits = range ? 64 - __builtin_clzll(range) : 0;
                const int shift = nbits > PLAN_NB_LOG ? nbits - PLAN_NB_LOG : 0;
#pragma unroll
                for (int r = 0; r < PER; ++r) {
                    const int e = r * 256 + tid;
                    bk[r] = 0; slot[r] = 0;
                    if (e < cnt) {
                        bk[r] = (int)((ekey[r] - lo_key) >> shift);
                        slot[r] = atomicAdd(&s_hist[bk[r]], 1);
                    }
                }
            }
            __syncthreads();
            {   // exclusive scan of the bucket sizes, in place (thread t: buckets [t * NBT, (t + 1) * NBT))
                constexpr int NBT = PLAN_NB / 256;
                int hb[NBT], sum = 0;
#pragma unroll
                for (int u = 0; u < NBT; ++u) { hb[u] = s_hist[tid * NBT + u]; sum += hb[u]; }
                int x = sum;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int y = __shfl_up(x, d);
                    if (lane >= d) x += y;
                }
                if (lane == 63) s_i[wv] = x;
                __syncthreads();
                int base = x - sum;
                for (int w = 0; w < wv; ++w) base += s_i[w];
#pragma unroll
                for (int u = 0; u < NBT; ++u) { s_hist[tid * NBT + u] = base; base += hb[u]; }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int e = r * 256 + tid;
                if (e < cnt) {
                    const int pos = s_hist[bk[r]] + slot[r];
                    s_key[pos] = (typename PlanKeyT<CT>::type)ekey[r]; s_ij[pos] = eij[r];
                }
            }
            __syncthreads();
            int rk[PER];
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int e = r * 256 + tid;
                rk[r] = 0;
                if (e < cnt) {
                    const int bb = s_hist[bk[r]], be = bk[r] + 1 < PLAN_NB ? s_hist[bk[r] + 1] : cnt;
                    int rank = bb;
                    for (int p = bb; p < be; ++p) {
                        const uint64_t k2 = (uint64_t)s_key[p];
                        const uint32_t i2 = s_ij[p];
                        rank += (k2 < ekey[r] || (k2 == ekey[r] && i2 < eij[r])) ? 1 : 0;
                    }
                    rk[r] = rank;
                }
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int e = r * 256 + tid;
                if (e < cnt) {
                    s_key[rk[r]] = (typename PlanKeyT<CT>::type)ekey[r]; s_ij[rk[r]] = eij[r];
                    s_gc[rk[r]] = gg[r] > 0x7fffffffll ? 0x7fffffffu : (uint32_t)gg[r];
                }
            }
            __syncthreads();
            PLAN_DBG(6, wall_clock64() - dbg_t0);
            PLAN_DBG(7, wall_clock64() - dbg_t0);
            // quota cut inside this band: first position whose inclusive prefix of the cell sizes reaches the quota
            int64_t run64 = cum;
            int cut = -1;
            for (int b0 = 0; b0 < cnt && cut < 0; b0 += 256) {
                const int idx = b0 + tid;
                int64_t x = idx < cnt ? (int64_t)s_gc[idx] : 0;
                const int64_t own = x;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int64_t y = __shfl_up(x, d);
                    if (lane >= d) x += y;
                }
                __syncthreads();
                if (lane == 63) s_red[wv] = x;
                if (tid == 0) s_i[4] = 0x7fffffff;
                __syncthreads();
                int64_t base = run64;
                for (int w = 0; w < wv; ++w) base += s_red[w];
                const int64_t incl = base + x;
                if (idx < cnt && incl >= quota && incl - own < quota) atomicMin(&s_i[4], idx);
                const int64_t tot = s_red[0] + s_red[1] + s_red[2] + s_red[3];
                __syncthreads();
                if (s_i[4] != 0x7fffffff) cut = s_i[4];
                run64 += tot;
                __syncthreads();
            }
            PLAN_DBG(3, wall_clock64() - dbg_t0);
            PLAN_DBG(4, cnt);
            if (quota <= 0) cut = 0;
            const int take = cut >= 0 ? cut + 1 : cnt;
            if (ne_total + take > ent_cap) { fb = true; break; }
            // the cells of the band that hold anything (size over all shards > 0: the visited list is mostly empty cells at thousands
            // of coarse clusters) are appended to the query's list with their visit rank
            for (int b0 = 0; b0 < take; b0 += 256) {
                const int idx = b0 + tid;
                const int f = (idx < take && s_gc[idx] > 0u) ? 1 : 0;
                int x = f;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int y = __shfl_up(x, d);
                    if (lane >= d) x += y;
                }
                __syncthreads();
                if (lane == 63) s_i[wv] = x;
                __syncthreads();
                int base = ne_total;
                for (int w = 0; w < wv; ++w) base += s_i[w];
                if (f) {
                    const uint32_t ij = s_ij[idx];
                    const int64_t ep = (int64_t)(base + x - 1) * 2;
                    ent[ep] = (uint64_t)(((ij >> 16) << 12) | (ij & 0xfffu)) << 40;
                    ent[ep + 1] = (uint64_t)(uint32_t)(visited + idx) << 32;
                }
                ne_total += s_i[0] + s_i[1] + s_i[2] + s_i[3];
            }
            visited += take;
            if (cut >= 0) { done = true; break; }
            cum = run64;
            c_prev = c_hi;
            tau_prev = hi;
            have_prev = true;
#pragma unroll
            for (int k = 0; k < KR; ++k) pprev[k] = (int)(pbr[k] >> 16);
            // the next band: the cells the quota still needs at the candidates per cell seen so far, + 25 % (round 4).  Four times the
            // last target made the second band of a V = 2048 query 1024 ... 2048 cells when ~300 more were needed: the band's
            // enumeration and its sort (n log^2 n) were most of the count pass (tools/build_variant.sh plandbg -DCIS_PLAN_DBG lopq_plan).
            // The bands' boundaries do not change what is visited.
            {
                int64_t nxt = target * 4;
                if (cum > 0 && quota > cum) {
                    const int64_t need = ((quota - cum) * (int64_t)visited + cum - 1) / cum;
                    nxt = need + need / 4 + 16;
                }
                nxt = nxt < 64 ? 64 : nxt;
                target = nxt < PLAN_PAR_CAP / 2 ? nxt : PLAN_PAR_CAP / 2;
            }
            __syncthreads();
        }
        PLAN_DBG(9, wall_clock64() - dbg_k0);
        if (tid == 0) fallback[q] = fb ? 1 : 0;
        if (fb) return;
        if (tid == 0 && hint && quota > 0) {
            atomicAdd(&hint[hint_slot * 2], (unsigned long long)visited);
            atomicAdd(&hint[hint_slot * 2 + 1], (unsigned long long)quota);
        }
        __threadfence_block();
        __syncthreads();
        // the listed cells' own starts and lengths (this shard's), written back into the list: the emit pass reads nothing else.  The ranks
        // of either list that have a cell with candidates are bits (they alias the sort's bucket counters): a half table per set bit.
        constexpr int UW = PLAN_PAR_STAGE / 32;
        uint32_t* s_used = reinterpret_cast<uint32_t*>(s_hist);
        s_used[tid] = 0u;
        __syncthreads();
        int64_t n_items = 0, ncand = 0;
        for (int b0 = 0; b0 < ne_total; b0 += 4 * 256) {  // four cells per thread: their reads go out together, level by level
            uint64_t e0[4], e1[4];
            int64_t vc[4], l0[4], l1[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = b0 + u * 256 + tid;
                const int64_t ep = (int64_t)(idx < ne_total ? idx : 0) * 2;
                e0[u] = ent[ep]; e1[u] = ent[ep + 1];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) vc[u] = (int64_t)o0[(int)(e0[u] >> 52)] * V + o1[(int)((e0[u] >> 40) & 0xfffu)];
#pragma unroll
            for (int u = 0; u < 4; ++u) { l0[u] = loff[vc[u]]; l1[u] = loff[(int64_t)V * V + 1 + vc[u]]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = b0 + u * 256 + tid;
                if (idx < ne_total) {
                    const int64_t ll = l1[u] - l0[u];
                    ent[(int64_t)idx * 2] = e0[u] | (uint64_t)l0[u];
                    ent[(int64_t)idx * 2 + 1] = e1[u] | (uint64_t)(uint32_t)(ll > 0 ? ll : 0);
                    if (ll > 0) {
                        const int bi = (int)(e0[u] >> 52), bj = (int)((e0[u] >> 40) & 0xfffu);
                        n_items += (ll + seg_max - 1) / seg_max;
                        ncand += ll;
                        atomicOr(&s_used[bi >> 5], 1u << (bi & 31));
                        atomicOr(&s_used[UW + (bj >> 5)], 1u << (bj & 31));
                    }
                }
            }
        }
        n_items = block_sum(n_items);
        ncand = block_sum(ncand);
        const uint32_t ubits = s_used[tid];
        const int64_t ntabs = block_sum(tid < UW ? (int64_t)__popc(ubits) : ((int64_t)__popc(ubits) << 32));
        PLAN_DBG(10, wall_clock64() - dbg_k0);
        if (tid == 0) {
            PlanOut p;
            p.visited = visited; p.n_items = (int)n_items; p.ntab0 = (int)(uint32_t)ntabs; p.ntab1 = (int)(ntabs >> 32); p.ncand = ncand;
            plan[q] = p;
            fallback[nq + q] = ne_total;
        }
        for (int x = tid; x < 2 * V; x += 256) {  // (a thread per rank: see the emit pass)
            const int split = x >= V ? 1 : 0, r = x - split * V;
            if ((s_used[split * UW + (r >> 5)] >> (r & 31)) & 1u) {
                count_table_group(grp_cnt, split ? V + (int)o1[r] : (int)o0[r], q);
            }
        }
        PLAN_DBG(11, wall_clock64() - dbg_k0);
    }
}

// multisequence as a list: the first `max_cells` (dist, cell) pairs of every query, same frontier walk as k_plan
template <typename CT>
__global__ __launch_bounds__(64) void k_multiseq_list(const CT* __restrict__ sorted, const uint16_t* __restrict__ order, int V,
                                                      int max_cells, int32_t* __restrict__ cells, double* __restrict__ dists) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* t = reinterpret_cast<int*>(smem);
    const int q = blockIdx.x, lane = threadIdx.x;
    const CT* d0 = sorted + ((int64_t)q * 2 + 0) * V;
    const CT* d1 = sorted + ((int64_t)q * 2 + 1) * V;
    const uint16_t* o0 = order + ((int64_t)q * 2 + 0) * V;
    const uint16_t* o1 = order + ((int64_t)q * 2 + 1) * V;
    for (int i = lane; i < V; i += 64) t[i] = 0;
    __syncthreads();
    int rows = 1;
    for (int n = 0; n < max_cells; ++n) {
        const uint32_t bij = walk_step<CT, false>(d0, d1, t, rows, V, lane);
        if (bij == WALK_NONE) break;
        const int bi = (int)(bij >> 16), bj = (int)(bij & 0xffff);
        if (lane == 0) {
            cells[((int64_t)q * max_cells + n) * 2 + 0] = o0[bi];
            cells[((int64_t)q * max_cells + n) * 2 + 1] = o1[bj];
            dists[(int64_t)q * max_cells + n] = (double)(CT)(d0[bi] + d1[bj]);
        }
        walk_advance(t, rows, V, lane, bi, bj);
    }
}

// The table-group part of k_plan_scan for wide vocabularies: 2 V x 32 counters are 262144 words at V = 4096.  One tile of 1024 counters per
// workgroup (16-byte loads); a tile publishes its sum tagged with the batch's sequence number and takes as its base the sum of the tiles
// before it, each waited for by one thread -- every tile publishes before it waits, and tiles are dispatched in order, so nothing can wait
// for a tile that has not started.  (Round 4: one workgroup, 16384 counters per round, 0.46 ms at V = 4096 on the batch's critical path.)
static const int GROUP_TILE = 1024;
__global__ __launch_bounds__(256) void k_group_bases(int* __restrict__ grp_cnt, int* __restrict__ grp_base, int n_groups,
                                                     unsigned long long* __restrict__ agg /* [tiles] tag << 32 | sum */, uint32_t tag) {
    __shared__ int s_w[8];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, t = blockIdx.x;
    const int g = t * GROUP_TILE + tid * 4;
    int c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = g + i < n_groups ? grp_cnt[g + i] : 0;
    const int tot = c[0] + c[1] + c[2] + c[3];
    int x = tot;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    if (tid == 0)
        __hip_atomic_store(&agg[t], ((unsigned long long)tag << 32) | (unsigned long long)(uint32_t)(s_w[0] + s_w[1] + s_w[2] + s_w[3]),
                           __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    int pre = 0;
    for (int p = tid; p < t; p += 256) {
        unsigned long long v;
        do { v = __hip_atomic_load(&agg[p], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT); } while ((uint32_t)(v >> 32) != tag);
        pre += (int)(uint32_t)v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o);
    if (lane == 0) s_w[4 + wv] = pre;
    __syncthreads();
    int r = s_w[4] + s_w[5] + s_w[6] + s_w[7] + x - tot;
    for (int w = 0; w < wv; ++w) r += s_w[w];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (g + i < n_groups) {
            grp_base[g + i] = r;
            grp_cnt[g + i] = 0;              // as k_plan_scan: clean counters for the next batch, clean cursors for this batch's emit pass
            grp_cnt[n_groups + g + i] = 0;
        }
        r += c[i];
    }
}

// exclusive scans over the queries of one batch (single block of 1024 threads); totals[0]=items, [1]=tables, [2]=cands.
// Thread t owns queries t, t + 1024, ... (<= 8 rounds for a batch of 8192): every load and store of a wave is
// contiguous -- with eight consecutive queries per thread the wave touched 64 cache lines per instruction and this
// one-CU kernel took 21 us.  Round r, wave w: inclusive wave scans of all rounds at once, wave totals through LDS.
__global__ __launch_bounds__(1024) void k_plan_scan(const PlanOut* __restrict__ plan, int nq, int64_t* __restrict__ item_off,
                                                    int64_t* __restrict__ tab_off, int64_t* __restrict__ totals,
                                                    unsigned long long* __restrict__ qbound /* [nq] -> +inf */,
                                                    volatile int64_t* __restrict__ host_totals /* pinned, mapped */, int64_t seq,
                                                    int* __restrict__ grp_cnt /* read, then zeroed: the next batch's count pass finds it clean */,
                                                    int* __restrict__ grp_base, int n_groups,
                                                    unsigned long long* __restrict__ hint_zero /* null, or the two words k_plan_par's NEXT launch adds into */) {
    if (hint_zero && threadIdx.x == 0) { hint_zero[0] = 0ull; hint_zero[1] = 0ull; }
    constexpr int R = 8;  // rounds held in registers; more queries than 8192 take the slow tail loop below
    __shared__ int s_wi[R][16], s_wt[R][16];  // wave totals per round
    __shared__ int64_t s_cand[16];
    __shared__ int64_t s_base_i[R][16], s_base_t[R][16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (wv == 15 && n_groups > 0) {  // exclusive scan of the table-group counters by one wave: 64 x 16 at a time, loads issued together
        // (n_groups == 0: k_group_bases did it -- thousands of coarse clusters)
        int run = 0;
        for (int g0 = 0; g0 < n_groups; g0 += 1024) {
            int c[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int g = g0 + lane * 16 + i;
                c[i] = g < n_groups ? grp_cnt[g] : 0;
            }
            int tot = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) tot += c[i];
            int x = tot;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(x, d);
                if (lane >= d) x += y;
            }
            int r = run + x - tot;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int g = g0 + lane * 16 + i;
                if (g < n_groups) {
                    grp_base[g] = r;
                    grp_cnt[g] = 0;              // counters: clean for the next batch's count pass (k_front_small does not zero them)
                    grp_cnt[n_groups + g] = 0;   // cursors (grp_cur = grp_cnt + n_groups): clean for this batch's emit pass
                }
                r += c[i];
            }
            run += __shfl(x, 63);
        }
    }
    int ni[R], nt[R], xi[R], xt[R];
    int64_t lc = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int q = r * 1024 + tid;
        const bool on = q < nq;
        const PlanOut pl = plan[on ? q : 0];
        ni[r] = on ? pl.n_items : 0;
        nt[r] = on ? pl.ntab0 + pl.ntab1 : 0;
        lc += on ? pl.ncand : 0;
        xi[r] = ni[r]; xt[r] = nt[r];
    }
    for (int q = R * 1024 + tid; q < nq; q += 1024) lc += plan[q].ncand;  // batches above 8192 queries (not used today)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int yi = __shfl_up(xi[r], d), yt = __shfl_up(xt[r], d);
            if (lane >= d) { xi[r] += yi; xt[r] += yt; }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) lc += __shfl_xor(lc, d);
    if (lane == 63) {
#pragma unroll
        for (int r = 0; r < R; ++r) { s_wi[r][wv] = xi[r]; s_wt[r][wv] = xt[r]; }
    }
    if (lane == 0) s_cand[wv] = lc;
    __syncthreads();
    if (wv == 0) {  // exclusive scan over the R x 16 (round, wave) totals: two consecutive entries per lane
        const int e0 = 2 * lane, e1 = 2 * lane + 1;
        const int a_i = (&s_wi[0][0])[e0], b_i = (&s_wi[0][0])[e1], a_t = (&s_wt[0][0])[e0], b_t = (&s_wt[0][0])[e1];
        int64_t xi2 = (int64_t)a_i + b_i, xt2 = (int64_t)a_t + b_t;
        const int64_t own_i = xi2, own_t = xt2;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t yi = __shfl_up(xi2, d), yt = __shfl_up(xt2, d);
            if (lane >= d) { xi2 += yi; xt2 += yt; }
        }
        (&s_base_i[0][0])[e0] = xi2 - own_i; (&s_base_i[0][0])[e1] = xi2 - own_i + a_i;
        (&s_base_t[0][0])[e0] = xt2 - own_t; (&s_base_t[0][0])[e1] = xt2 - own_t + a_t;
        int64_t ri = __shfl(xi2, 63), rt = __shfl(xt2, 63);
        int64_t rc = lane < 16 ? s_cand[lane] : 0;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) rc += __shfl_xor(rc, d);
        if (lane == 0) {
            for (int q = R * 1024; q < nq; ++q) {  // queries beyond R * 1024 (slow path): sequential
                item_off[q] = ri; tab_off[q] = rt;
                qbound[q] = 0x7ff0000000000000ull;
                ri += plan[q].n_items; rt += plan[q].ntab0 + plan[q].ntab1;
            }
            totals[0] = ri; totals[1] = rt; totals[2] = rc;
            host_totals[0] = ri; host_totals[1] = rt; host_totals[2] = rc;  // straight into pinned host memory: no staged copy
            __threadfence_system();
            host_totals[3] = seq;  // the host polls this word (the totals above are visible before it)
            __threadfence_system();
            item_off[nq] = ri; tab_off[nq] = rt;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int q = r * 1024 + tid;
        if (q < nq) {
            item_off[q] = s_base_i[r][wv] + xi[r] - ni[r];
            tab_off[q] = s_base_t[r][wv] + xt[r] - nt[r];
            qbound[q] = 0x7ff0000000000000ull;
        }
    }
}

// one launch instead of three memsets: queue counters and per-cell counters to zero, slots to -1 (empty)
__global__ void k_slots_init(int* __restrict__ qctr16, int* __restrict__ cell_cnt, int ncells, int* __restrict__ slots,
                             int64_t n_slot_entries) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 64) qctr16[i] = 0;  // queue counters, slot counts, debug counters, the fall-back header of the sampled scan
    if (i < ncells) cell_cnt[i] = 0;
    if (i < n_slot_entries) slots[i] = -1;
}

// Sort key of a work item.  The slot list is cut into eight queues (one per XCD) by cell range; inside a queue the
// items of every query's FIRST visited cell come first, sorted by cell, then all the others, sorted by cell: the
// first cell usually holds the best candidates, so by the time the other cells of a query are scanned its bound
// (qbound) is already tight and they run the hot loop only.
static __device__ __forceinline__ int q8_begin(int x, int ncells) { return (int)(((int64_t)x * ncells + 7) / 8); }
// CH keys per (cell, first / other): the chunks of a cell longer than one chunk get their own slots (round 3; with one key per cell
// such items shared slots and ran as sub-slots, one chunk after the other, inside one workgroup)
static __device__ __forceinline__ int slot_key(const WorkItem& it, int ncells, int CH, int seg_max) {
    const int x = (int)(((int64_t)it.cell * 8) / ncells);
    const int b = q8_begin(x, ncells), sz = q8_begin(x + 1, ncells) - b;
    int ch = CH > 1 ? it.pos0 / seg_max : 0;
    ch = ch < CH ? ch : CH - 1;
    return (2 * b + (it.rank > 0 ? sz : 0) + (it.cell - b)) * CH + ch;
}

__global__ void k_item_hist(const WorkItem* __restrict__ items, int64_t n, int* __restrict__ cell_cnt, int ncells, int CH, int seg_max,
                            const int64_t* __restrict__ d_totals = nullptr /* the plan totals: n is a bound */) {
    if (d_totals) n = d_totals[0];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&cell_cnt[slot_key(items[i], ncells, CH, seg_max)], 1);
}

// counts -> exclusive SLOT offsets per cell (a slot holds up to G items of one cell); the counts are
// reset to zero so that the scatter can reuse them as cursors.  *n_slots = total number of slots.
__global__ __launch_bounds__(1024) void k_cell_scan(int* __restrict__ cell_cnt, int* __restrict__ slot_off, int nkeys, int G,
                                                    int* __restrict__ n_slots, int* __restrict__ qstart /* [9] first slot of every queue */, int CH) {
    // exclusive scan of the slot counts in key order: rounds of 1024 consecutive keys (coalesced), wave scans + one LDS hop per
    // round (the first version gave every thread a run of consecutive keys and walked it load by load: 23 us at 8192 keys)
    __shared__ int s_w[16];
    __shared__ int s_tot;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int run = 0;
    for (int c0 = 0; c0 < nkeys; c0 += 1024) {
        const int c = c0 + tid;
        const int x = c < nkeys ? (cell_cnt[c] + G - 1) / G : 0;
        int inc = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(inc, d);
            if (lane >= d) inc += y;
        }
        __syncthreads();
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        int base = run, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int v = s_w[w];
            if (w < wv) base += v;
            tot += v;
        }
        if (c < nkeys) {
            slot_off[c] = base + inc - x;
            cell_cnt[c] = 0;
        }
        run += tot;
    }
    if (tid == 0) { *n_slots = run; s_tot = run; }
    __threadfence();
    __syncthreads();
    if (tid < 8) {  // queue x starts at the first key of its cell range
        const int k0 = 2 * q8_begin(tid, nkeys / (2 * CH)) * CH;
        qstart[tid] = k0 < nkeys ? __hip_atomic_load(&slot_off[k0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : s_tot;
    }
    if (tid == 8) qstart[8] = s_tot;
}

// slots[(slot_off[cell] + r / G) * G + r % G] = item, r = arrival rank of the item inside its cell
__global__ void k_item_scatter(const WorkItem* __restrict__ items, int64_t n, const int* __restrict__ slot_off,
                               int* __restrict__ cursor, int G, int* __restrict__ slots, int ncells, int CH, int seg_max,
                               const int64_t* __restrict__ d_totals = nullptr /* the plan totals: n is a bound */) {
    if (d_totals) n = d_totals[0];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = slot_key(items[i], ncells, CH, seg_max);
    const int r = atomicAdd(&cursor[c], 1);
    slots[(slot_off[c] + r / G) * G + (r % G)] = (int)i;
}

// no sorting (huge V): slot i = item i alone
__global__ void k_identity_slots(int64_t n, int G, int* __restrict__ slots, int* __restrict__ n_slots, int* __restrict__ qstart) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        slots[i * G] = (int)i;
        for (int g = 1; g < G; ++g) slots[i * G + g] = -1;
    }
    if (i == 0) *n_slots = (int)n;
    if (i < 9) qstart[i] = (int)((n * i) / 8);  // equal eighths
}

// k_rank for wide coarse vocabularies (production configs go up to V = 4096): the rank by counting above is O(V^2)
// per (query, split); here the (distance bits, centroid index) pairs are sorted in LDS -- the index as second key
// reproduces "first minimum wins" among equal distances.
template <typename CT>
__global__ __launch_bounds__(256) void k_rank_sort(const CT* __restrict__ dist /* [2][nq][V] */, int nq, int V, int Vp2,
                                                   uint16_t* __restrict__ order, CT* __restrict__ sorted, int* __restrict__ grp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* ka = reinterpret_cast<uint64_t*>(smem);
    uint64_t* kb = ka + Vp2;
    const int q = blockIdx.x, s = blockIdx.y;
    if (q == 0 && s == 0)
        for (int i = threadIdx.x; i < 4 * V * GRP_SUB; i += blockDim.x) grp[i] = 0;
    const CT* d = dist + ((int64_t)s * nq + q) * V;
    if constexpr (sizeof(CT) == 4) {
        // float32 distances: (distance bits, index) is ONE 64-bit key -- half the LDS traffic of the pair sort below
        for (int v = threadIdx.x; v < Vp2; v += 256) ka[v] = v < V ? ((f2bits(d[v]) << 32) | (uint64_t)v) : ~0ull;
        __syncthreads();
        for (int k = 2; k <= Vp2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = threadIdx.x; t < (Vp2 >> 1); t += 256) {
                    const int a_ = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const int b_ = a_ + j;
                    const uint64_t x = ka[a_], y = ka[b_];
                    if ((x > y) == ((a_ & k) == 0)) { ka[a_] = y; ka[b_] = x; }
                }
                __syncthreads();
            }
        }
        for (int r = threadIdx.x; r < V; r += 256) {
            const int v = (int)(uint32_t)ka[r];
            order[((int64_t)q * 2 + s) * V + r] = (uint16_t)v;
            sorted[((int64_t)q * 2 + s) * V + r] = d[v];
        }
        return;
    }
    for (int v = threadIdx.x; v < Vp2; v += 256) {
        ka[v] = v < V ? f2bits(d[v]) : ~0ull;
        kb[v] = v < V ? (uint64_t)v : ~0ull;
    }
    __syncthreads();
    block_bitonic_rt<256, false>(ka, kb, nullptr, Vp2);
    for (int r = threadIdx.x; r < V; r += 256) {
        const int v = (int)kb[r];
        order[((int64_t)q * 2 + s) * V + r] = (uint16_t)v;
        sorted[((int64_t)q * 2 + s) * V + r] = d[v];
    }
}

// k_rank_sort for float32 distances with the sort in REGISTERS (round 4): thread t owns the NPT consecutive elements t * NPT ..., so of
// the log2(N) (log2(N) + 1) / 2 compare-exchange stages of the bitonic network those with partner distance j < NPT stay inside a thread,
// those with j < 64 NPT are one 64-bit lane exchange inside a wave, and only the 3 (N = 2048) to 6 (N = 4096) stages across waves go
// through LDS with a barrier -- the LDS form above pays a barrier and four LDS accesses per element for every one of its 66 / 78 stages.
// Same keys (distance bits << 32 | centroid index), same order: identical output.
template <int NPT>
__global__ __launch_bounds__(256) void k_rank_sort_reg(const float* __restrict__ dist /* [2][nq][V] */, int nq, int V,
                                                       uint16_t* __restrict__ order, float* __restrict__ sorted, int* __restrict__ grp) {
    constexpr int N = 256 * NPT;
    __shared__ uint64_t sx[N];
    const int q = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    if (q == 0 && s == 0)
        for (int i = tid; i < 4 * V * GRP_SUB; i += 256) grp[i] = 0;
    const float* d = dist + ((int64_t)s * nq + q) * V;
    uint64_t key[NPT];
#pragma unroll
    for (int r = 0; r < NPT; ++r) {
        const int e = tid * NPT + r;
        key[r] = e < V ? ((f2bits(d[e < V ? e : 0]) << 32) | (uint64_t)e) : ~0ull;
    }
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64 * NPT) {  // across waves: through LDS
                __syncthreads();
#pragma unroll
                for (int r = 0; r < NPT; ++r) sx[tid * NPT + r] = key[r];
                __syncthreads();
#pragma unroll
                for (int r = 0; r < NPT; ++r) {
                    const int e = tid * NPT + r;
                    const uint64_t o = sx[e ^ j];
                    const bool keep_min = ((e & j) == 0) == ((e & k) == 0);
                    key[r] = keep_min ? (o < key[r] ? o : key[r]) : (o > key[r] ? o : key[r]);
                }
            } else if (j >= NPT) {  // across lanes of the wave
                const int lj = j / NPT;
#pragma unroll
                for (int r = 0; r < NPT; ++r) {
                    const int e = tid * NPT + r;
                    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key[r], lj), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key[r] >> 32), lj);
                    const uint64_t o = ((uint64_t)hi << 32) | lo;
                    const bool keep_min = ((e & j) == 0) == ((e & k) == 0);
                    key[r] = keep_min ? (o < key[r] ? o : key[r]) : (o > key[r] ? o : key[r]);
                }
            } else {  // inside the thread
#pragma unroll
                for (int r = 0; r < NPT; ++r) {
                    if ((r & j) == 0) {
                        const int e = tid * NPT + r;
                        const bool asc = (e & k) == 0;
                        const uint64_t a = key[r], b = key[r | j];
                        const bool sw = (a > b) == asc;
                        key[r] = sw ? b : a;
                        key[r | j] = sw ? a : b;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < NPT; ++r) {
        const int e = tid * NPT + r;
        if (e < V) {
            order[((int64_t)q * 2 + s) * V + e] = (uint16_t)(uint32_t)key[r];
            sorted[((int64_t)q * 2 + s) * V + e] = __uint_as_float((uint32_t)(key[r] >> 32));
        }
    }
}

// ================================================================================================
// host: the phases of search_batch that launch the kernels above
// ================================================================================================
int front_prepare(cis_index* ix, const void* dQ, int q_dtype, int nq, hipStream_t st, Front* f) {
    cis_model* m = ix->m;
    const int V = m->V;
    // 1. LOPQ-space queries
    const void* xp = dQ;
    int xp_dtype = q_dtype;
    if (m->has_pca) {
        CIS_TRY(ix->w_xp.reserve((size_t)nq * m->D * sizeof(float)));
        CIS_TRY(cis_dev_apply_pca(m, dQ, q_dtype, nq, ix->w_xp.as<float>(), st, &ix->w_y64));
        xp = ix->w_xp.p;
        xp_dtype = CIS_F32;
    }
    CIS_TRY(cis_dev_coarse_type(m, xp, xp_dtype, nq, &f->xc, &f->ct, st, &ix->w_x64));
    const size_t csz = (f->ct == CIS_F32) ? 4 : 8;
    // 2. coarse distances, rank
    CIS_TRY(ix->w_cd.reserve((size_t)2 * nq * V * csz));
    CIS_TRY(ix->w_sorted.reserve((size_t)2 * nq * V * csz));
    CIS_TRY(ix->w_order.reserve((size_t)2 * nq * V * sizeof(uint16_t)));
    const void* grp_before = ix->w_grp.p;
    CIS_TRY(ix->w_grp.reserve((size_t)(GRP_WORDS(V) + 2 * GRP_TILES(V)) * sizeof(int)));
    if (ix->w_grp.p != grp_before)  // fresh memory: the counters start clean (afterwards every k_plan_scan leaves them clean)
        CIS_CHECK_HIP(hipMemsetAsync(ix->w_grp.p, 0, ix->w_grp.cap, st));
    f->grp_cnt = ix->w_grp.as<int>();
    return CIS_OK;
}

// Rank of the coarse distances in w_cd -> w_order / w_sorted.  reg_sorts: the caller takes the register sorts (float32 distances
// only: k_rank_sort_reg has no float64 form) where the vocabulary fits one; the owner walk keeps to k_rank_sort / k_rank.
template <typename CT>
static void launch_rank(cis_index* ix, int nq, bool reg_sorts, int* grp_cnt, hipStream_t st) {
    const int V = ix->m->V;
    int Vp2 = 64;
    while (Vp2 < V) Vp2 <<= 1;
    const CT* cd = ix->w_cd.as<CT>();
    uint16_t* order = ix->w_order.as<uint16_t>();
    CT* sorted = ix->w_sorted.as<CT>();
    if constexpr (sizeof(CT) == 4) {
        const bool sort_lds = getenv("CIS_RANK_SORT_LDS") != nullptr;  // the LDS form of the sort (A/B runs)
        if (reg_sorts && V > 256 && !sort_lds && (Vp2 == 1024 || Vp2 == 2048 || Vp2 == 4096)) {
            if (Vp2 == 1024) hipLaunchKernelGGL(k_rank_sort_reg<4>, dim3(nq, 2), dim3(256), 0, st, cd, nq, V, order, sorted, grp_cnt);
            else if (Vp2 == 2048) hipLaunchKernelGGL(k_rank_sort_reg<8>, dim3(nq, 2), dim3(256), 0, st, cd, nq, V, order, sorted, grp_cnt);
            else hipLaunchKernelGGL(k_rank_sort_reg<16>, dim3(nq, 2), dim3(256), 0, st, cd, nq, V, order, sorted, grp_cnt);
            return;
        }
    }
    if (V > 256 && Vp2 <= 4096)
        hipLaunchKernelGGL(k_rank_sort<CT>, dim3(nq, 2), dim3(256), (size_t)Vp2 * 16, st, cd, nq, V, Vp2, order, sorted, grp_cnt);
    else
        hipLaunchKernelGGL(k_rank<CT>, dim3(nq, 2), dim3(V <= 64 ? 64 : 256), (size_t)V * 8, st, cd, nq, V, order, sorted, grp_cnt);
}

#ifdef CIS_PLAN_DBG
static void dump_plan_dbg(int nq) {
    unsigned long long h[12];
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_plan_dbg), sizeof(h));
    fprintf(stderr, "[cis] k_plan_par: %d queries, probes %.1f / query, bands %.2f / query, bisection %.1f us / query, after rows %.1f, after cells %.1f, after sort %.1f, after cut %.1f us / query (cumulative), cells per band %.0f (100 MHz clock)\n",
            nq, (double)h[0] / nq, (double)h[1] / nq, (double)h[2] / nq / 100.0, (double)h[5] / nq / 100.0, (double)h[6] / nq / 100.0, (double)h[7] / nq / 100.0, (double)h[3] / nq / 100.0, h[1] ? (double)h[4] / (double)h[1] : 0.0);
    fprintf(stderr, "[cis] k_plan_par since kernel start: staged %.1f, bands done %.1f, visited pass %.1f, end %.1f us / query\n", (double)h[8] / nq / 100.0, (double)h[9] / nq / 100.0, (double)h[10] / nq / 100.0, (double)h[11] / nq / 100.0);
    memset(h, 0, sizeof(h));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_plan_dbg), h, sizeof(h));
}
#endif

// CIS_DEBUG_PLAN: how many queries of the batch the sort-based plan handed to the frontier walk
int dump_plan_fallbacks(const Batch& b) {
    std::vector<int> fbh(b.nq);
    CIS_CHECK_HIP(hipMemcpyAsync(fbh.data(), b.plan_fb, (size_t)b.nq * sizeof(int), hipMemcpyDeviceToHost, b.st));
    CIS_CHECK_HIP(hipStreamSynchronize(b.st));
    int nfb = 0;
    for (int i = 0; i < b.nq; ++i) nfb += fbh[i] != 0;
    fprintf(stderr, "[cis] k_plan_par: %d of %d queries fall back to the frontier walk (quota %lld)\n", nfb, b.nq, (long long)b.quota);
    return CIS_OK;
}

// CIS_HOST_TIMING=1: where the host spends a batch (stderr, every 400 batches): entry -> plan totals requested, the wait for them
static void host_timing(const Batch& b, std::chrono::steady_clock::time_point t0) {
    static const bool ht = getenv("CIS_HOST_TIMING") != nullptr;
    if (!ht) return;
    static std::atomic<long long> n_{0}, wait_ns{0}, front_ns{0};
    const auto t1 = std::chrono::steady_clock::now();
    wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
    front_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(t0 - b.t_entry).count();
    if (++n_ % 400 == 0)
        fprintf(stderr, "[cis] host timing over %lld batches: front-end enqueue %.1f us, wait for the plan totals %.1f us per batch\n", (long long)n_,
                front_ns / 1e3 / n_, wait_ns / 1e3 / n_);
}

// coarse distances, rank and the counting pass of the multisequence walk
template <typename CT>
int front_count(Batch& b, const Route& r) {
    cis_index* ix = b.ix;
    cis_model* m = ix->m;
    hipStream_t st = b.st;
    const int V = m->V, nq = b.nq;
    uint16_t* order = ix->w_order.as<uint16_t>();
    CT* sorted = ix->w_sorted.as<CT>();
    if (r.fused_front) {
        // coarse distances + rank + counting pass of the multisequence walk in one launch (k_front_small)
        const size_t flds = (size_t)V * (32 + 4 + 4);
        hipLaunchKernelGGL(k_front_small<CT>, dim3(nq), dim3(64), flds, st, (const CT*)b.f.xc, m->D, m->h, coarse_centroids(m, CT()), m->prog_h,
                           ix->gcount_ptr(), ix->loff_ptr(), nq, V, b.quota, r.seg_max, order, sorted, b.plan, b.f.grp_cnt);
        return CIS_OK;
    }
    CIS_TRY(cis_launch_sqdist_both(m, b.f.xc, b.f.ct, nq, ix->w_cd.p, st));
    launch_rank<CT>(ix, nq, true, b.f.grp_cnt, st);
    if (r.par_plan)
        hipLaunchKernelGGL((k_plan_par<CT, false>), dim3(nq), dim3(256), (size_t)2 * (V < PLAN_SP ? V : PLAN_SP) * sizeof(CT), st, sorted, order,
                           ix->gcount_ptr(), ix->loff_ptr(), nq, V, b.quota, r.seg_max, b.plan, nullptr, nullptr, nullptr,
                           nullptr, b.f.grp_cnt, nullptr, nullptr, nullptr, b.vis_list, b.plan_fb, b.vis_cap, b.plan_hint, b.hint_slot);
#ifdef CIS_PLAN_DBG
    if constexpr (sizeof(CT) == 4)  // (the counters are read back for float32 batches only)
        if (r.par_plan) dump_plan_dbg(nq);
#endif
    hipLaunchKernelGGL((k_plan<CT, false>), dim3(nq), dim3(64), (size_t)V * sizeof(int), st, sorted, order, ix->gcount_ptr(), ix->loff_ptr(), nq, V,
                       b.quota, r.seg_max, b.plan, nullptr, nullptr, nullptr, nullptr, b.f.grp_cnt, nullptr, nullptr, nullptr, b.plan_fb);
    return CIS_OK;
}
template int front_count<float>(Batch&, const Route&);
template int front_count<double>(Batch&, const Route&);

// the emitting pass of the walk (work items + table list)
template <typename CT>
void emit_plan(Batch& b, const Route& r) {
    cis_index* ix = b.ix;
    cis_model* m = ix->m;
    hipStream_t st = b.st;
    const int V = m->V, nq = b.nq;
    const uint16_t* order = ix->w_order.as<uint16_t>();
    const CT* sorted = ix->w_sorted.as<CT>();
    if (r.par_plan)
        hipLaunchKernelGGL((k_plan_par<CT, true>), dim3(nq), dim3(256), 0, st, sorted, order, ix->gcount_ptr(), ix->loff_ptr(), nq, V, b.quota,
                           r.seg_max, b.plan, b.item_off, b.tab_off, b.items, b.tabs, nullptr, b.grp_base, b.grp_cur, b.tab_order, b.vis_list,
                           b.plan_fb, b.vis_cap, nullptr, 0);
    hipLaunchKernelGGL((k_plan<CT, true>), dim3(nq), dim3(64), (size_t)V * sizeof(int), st, sorted, order, ix->gcount_ptr(), ix->loff_ptr(), nq, V,
                       b.quota, r.seg_max, b.plan, b.item_off, b.tab_off, b.items, b.tabs, nullptr, b.grp_base, b.grp_cur, b.tab_order, b.plan_fb);
}
template void emit_plan<float>(Batch&, const Route&);
template void emit_plan<double>(Batch&, const Route&);

// exclusive scan of the plan; then the totals that size the rest of the batch -- their bounds where those do, else the read-back
int plan_totals(Batch& b, const Route& r) {
    cis_index* ix = b.ix;
    cis_model* m = ix->m;
    hipStream_t st = b.st;
    const int V = m->V, nq = b.nq, L = b.L;
    if (!ix->h_totals) {
        CIS_CHECK_HIP(hipHostMalloc((void**)&ix->h_totals, 12 * sizeof(int64_t), hipHostMallocMapped | hipHostMallocCoherent));
        CIS_CHECK_HIP(hipHostGetDevicePointer((void**)&ix->d_h_totals, ix->h_totals, 0));
        ix->h_totals[3] = 0;
        ix->h_totals[4] = 0;  // (slots, fall-back slots) of the last sampled scan at M = 16: see m16_holdoff
        for (int i = 6; i < 12; ++i) ix->h_totals[i] = 0;  // [6] failed proofs, [7] overflowed lists, [8] sequence word of the streaming route
    }
    const int64_t seq = ++ix->plan_seq;
    const int n_groups = 2 * V * GRP_SUB;
    const bool groups_apart = n_groups > 8192;  // wide vocabularies: the group bases by their own launch (all 16 waves)
    int* grp_cnt = b.f.grp_cnt;
    if (groups_apart)
        hipLaunchKernelGGL(k_group_bases, dim3((n_groups + GROUP_TILE - 1) / GROUP_TILE), dim3(256), 0, st, grp_cnt, b.grp_base, n_groups,
                           reinterpret_cast<unsigned long long*>(grp_cnt + GRP_WORDS(V)), (uint32_t)(seq & 0x7fffffff) | 0x80000000u);
    hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(1024), 0, st, b.plan, nq, b.item_off, b.tab_off, b.totals, b.qbound, ix->d_h_totals, seq, grp_cnt, b.grp_base,
                       groups_apart ? 0 : n_groups, b.plan_hint ? b.plan_hint + (b.hint_slot ^ 1) * 2 : nullptr);
    volatile int64_t* h_tot = ix->h_totals;
    // A small batch on the all-candidates path does not wait for the plan totals: the workspace is sized by upper bounds
    // (every query stops within quota + largest cell candidates, in at most `nonempty cells` cells) and the kernels
    // below read the real totals from device memory -- no host round trip in the middle of the batch.
    b.d_tot = nullptr;
    b.n_items = b.n_tabs = b.n_cand_all = 0;
    {
        static const bool no_bounds = getenv("CIS_NO_BOUNDS") != nullptr;
        // quota <= 0 still visits one cell (search.py:131-132: the test follows the first append)
        const int64_t q_eff = b.quota < 0 ? 0 : b.quota;
        const int64_t per_q = (q_eff < ix->n_total ? q_eff : ix->n_total) + ix->max_cell;
        const int64_t items_q = ix->nonempty_cells + per_q / r.seg_max + 2;
        const bool small_all = !no_bounds && !r.stream_hint && nq <= 64 && L <= MAX_LDS_LIMIT && r.split_tables && r.big && items_q <= 4096 &&
                               (double)nq * (double)per_q < 64.0e6;
        // The streaming route when it is CERTAIN before the plan is known -- every query collects at least min(quota, n_total)
        // candidates (search.py:128-133 stops at the quota or at the end of the index), and that alone is past the route's threshold
        // (an exhaustive quota): the same bounds size the workspaces, the kernels read the real totals from device memory, and the
        // host does not stop in the middle of the batch (round 6: the read-back was a 35 us hole in a 0.5 ms exhaustive query).
        static const bool no_stream_bounds = getenv("CIS_STREAM_WAIT") != nullptr;   // A/B runs: the read-back as before
        const bool sure_stream = !no_bounds && !no_stream_bounds && r.stream_hint && r.split_tables && items_q <= 65536 &&
                                 (double)nq * (double)items_q < 4.0e6 &&
                                 (ix->force_stream || (q_eff < ix->n_total ? q_eff : ix->n_total) >= r.stream_min) && ix->n_total > 0 && nq <= 64;
        if (small_all || sure_stream) {
            b.d_tot = b.totals;
            b.n_items = (int64_t)nq * items_q;
            b.n_tabs = (int64_t)nq * 2 * V;
            b.n_cand_all = (int64_t)nq * per_q;
            ix->stats_pending_seq = seq;
        }
    }
    if (!b.d_tot) {
        // the plan totals size the rest of the batch: poll the pinned sequence word (a blocking stream synchronisation
        // wakes up tens of microseconds late); past 2 ms -- a stream busy with the caller's earlier work, or an error --
        // fall back to the blocking wait
        static const bool no_poll = getenv("CIS_NO_POLL") != nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        bool got = false;
        while (!no_poll) {
            if (__atomic_load_n(&ix->h_totals[3], __ATOMIC_ACQUIRE) == seq) { got = true; break; }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
        if (!got) {
            CIS_CHECK_HIP(hipStreamSynchronize(st));
            CIS_REQUIRE(__atomic_load_n(&ix->h_totals[3], __ATOMIC_ACQUIRE) == seq, "plan totals did not arrive");
        }
        host_timing(b, t0);
        b.n_items = h_tot[0]; b.n_tabs = h_tot[1]; b.n_cand_all = h_tot[2];
        ix->stats_pending_seq = 0;
    }
    CIS_REQUIRE(b.n_items < ((int64_t)1 << 31) && b.n_tabs < ((int64_t)1 << 31), "query batch too large");
    return CIS_OK;
}

// ---- slot list: work items grouped by (coarse cell, chunk) with a counting sort, G per slot (Slots, SlotMode: lopq_batch.h) ----
int build_slots(const Batch& b, SlotMode mode, int G, int64_t CH /* chunks per cell that get their own slot keys */, int seg_max, Slots* s) {
    cis_index* ix = b.ix;
    hipStream_t st = b.st;
    const int64_t n_items = b.n_items;
    const int64_t nkeys = 2 * ix->ncells * CH;
    const int64_t max_slots = mode == SLOTS_IDENTITY ? n_items : (n_items + nkeys) / G + nkeys + 2;
    CIS_TRY(ix->w_order2.reserve((size_t)(64 + 2 * nkeys + 2 * max_slots * G) * sizeof(int)));
    int* qctr = ix->w_order2.as<int>();
    int* n_slots = qctr + 8;
    int* qstart = qctr + 16;
    int* cell_cnt = qctr + 64;
    int* slot_off = cell_cnt + nkeys;
    int* slots = slot_off + nkeys;
    s->qctr = qctr;
    s->n_slots = n_slots;
    s->fhdr = qctr + 32;
    s->slots = mode == SLOTS_NONE ? nullptr : slots;
    s->fslots = slots + max_slots * G;
    s->max_slots = max_slots;
    if (mode == SLOTS_SORTED) {
        const int64_t ninit = max_slots * G > nkeys ? max_slots * G : nkeys;
        hipLaunchKernelGGL(k_slots_init, dim3((unsigned)ceil_div(ninit < 16 ? 16 : ninit, 256)), dim3(256), 0, st, qctr, cell_cnt, (int)nkeys, slots, max_slots * G);
        hipLaunchKernelGGL(k_item_hist, dim3((unsigned)ceil_div(n_items, 256)), dim3(256), 0, st, b.items, n_items, cell_cnt, (int)ix->ncells, (int)CH, seg_max, b.d_tot);
        hipLaunchKernelGGL(k_cell_scan, dim3(1), dim3(1024), 0, st, cell_cnt, slot_off, (int)nkeys, G, n_slots, qstart, (int)CH);
        hipLaunchKernelGGL(k_item_scatter, dim3((unsigned)ceil_div(n_items, 256)), dim3(256), 0, st, b.items, n_items, slot_off, cell_cnt, G, slots, (int)ix->ncells, (int)CH, seg_max, b.d_tot);
    } else if (mode == SLOTS_IDENTITY) {
        CIS_CHECK_HIP(hipMemsetAsync(qctr, 0, 64 * sizeof(int), st));
        hipLaunchKernelGGL(k_identity_slots, dim3((unsigned)ceil_div(n_items < 9 ? 9 : n_items, 256)), dim3(256), 0, st, n_items, G, slots, n_slots, qstart);
    }
    return CIS_OK;
}

// ================================================================================================
// entry points that are the walk alone
// ================================================================================================
extern "C" int cis_multisequence(const void* X, int x_dtype, const void* C0, const void* C1, int c_dtype, int64_t n, int V,
                                 int h, int max_cells, int32_t* cells, double* dists, int* dist_dtype) {
    CIS_REQUIRE((x_dtype == CIS_F32 || x_dtype == CIS_F64) && (c_dtype == CIS_F32 || c_dtype == CIS_F64), "dtype must be 4 or 8");
    CIS_REQUIRE(n >= 0 && V >= 1 && V <= 65535 && h >= 1 && max_cells >= 1 && (n == 0 || (X && C0 && C1 && cells && dists)),
                "bad arguments");
    if ((int64_t)max_cells > (int64_t)V * V) max_cells = V * V;
    const int ct = (x_dtype == CIS_F32 && c_dtype == CIS_F32) ? CIS_F32 : CIS_F64;
    if (dist_dtype) *dist_dtype = ct;
    if (n == 0) return CIS_OK;
    CIS_TRY(cis_lazy_init());
    const size_t csz = (size_t)ct;
    DevBuf bx, bc, bd, bs, bo, bcell, bdist;
    int rc = CIS_OK;
    auto done = [&](int r) { bx.release(); bc.release(); bd.release(); bs.release(); bo.release(); bcell.release(); bdist.release(); return r; };
    auto up = [&](const void* src, int dt, size_t cnt, DevBuf* b, size_t off_elems) -> int {
        if (dt == ct) { CIS_CHECK_HIP(hipMemcpy((char*)b->p + off_elems * csz, src, cnt * csz, hipMemcpyHostToDevice)); return CIS_OK; }
        std::vector<double> tmp(cnt);
        for (size_t i = 0; i < cnt; ++i) tmp[i] = (double)((const float*)src)[i];
        CIS_CHECK_HIP(hipMemcpy((char*)b->p + off_elems * csz, tmp.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
        return CIS_OK;
    };
    if ((rc = bx.reserve((size_t)n * 2 * h * csz)) != CIS_OK) return done(rc);
    if ((rc = bc.reserve((size_t)2 * V * h * csz)) != CIS_OK) return done(rc);
    if ((rc = up(X, x_dtype, (size_t)n * 2 * h, &bx, 0)) != CIS_OK) return done(rc);
    if ((rc = up(C0, c_dtype, (size_t)V * h, &bc, 0)) != CIS_OK) return done(rc);
    if ((rc = up(C1, c_dtype, (size_t)V * h, &bc, (size_t)V * h)) != CIS_OK) return done(rc);
    if ((rc = bd.reserve((size_t)2 * n * V * csz)) != CIS_OK) return done(rc);
    if ((rc = bs.reserve((size_t)2 * n * V * csz)) != CIS_OK) return done(rc);
    if ((rc = bo.reserve((size_t)2 * n * V * sizeof(uint16_t))) != CIS_OK) return done(rc);
    if ((rc = bcell.reserve((size_t)n * max_cells * 2 * sizeof(int32_t))) != CIS_OK) return done(rc);
    if ((rc = bdist.reserve((size_t)n * max_cells * sizeof(double))) != CIS_OK) return done(rc);
    DevBuf bgrp;
    if ((rc = bgrp.reserve((size_t)4 * V * GRP_SUB * sizeof(int))) != CIS_OK) return done(rc);
    for (int s = 0; s < 2; ++s)
        if ((rc = cis_launch_sqdist_generic(bx.p, ct, 2 * h, s * h, (char*)bc.p + (size_t)s * V * h * csz, n, V, h,
                                            (char*)bd.p + (size_t)s * n * V * csz, nullptr)) != CIS_OK) return done(rc);
    if (ct == CIS_F32) {
        hipLaunchKernelGGL(k_rank<float>, dim3((unsigned)n, 2), dim3(V <= 64 ? 64 : 256), (size_t)V * 8, nullptr, bd.as<float>(), (int)n, V,
                           bo.as<uint16_t>(), bs.as<float>(), bgrp.as<int>());
        hipLaunchKernelGGL(k_multiseq_list<float>, dim3((unsigned)n), dim3(64), (size_t)V * sizeof(int), nullptr, bs.as<float>(),
                           bo.as<uint16_t>(), V, max_cells, bcell.as<int32_t>(), bdist.as<double>());
    } else {
        hipLaunchKernelGGL(k_rank<double>, dim3((unsigned)n, 2), dim3(V <= 64 ? 64 : 256), (size_t)V * 8, nullptr, bd.as<double>(), (int)n, V,
                           bo.as<uint16_t>(), bs.as<double>(), bgrp.as<int>());
        hipLaunchKernelGGL(k_multiseq_list<double>, dim3((unsigned)n), dim3(64), (size_t)V * sizeof(int), nullptr, bs.as<double>(),
                           bo.as<uint16_t>(), V, max_cells, bcell.as<int32_t>(), bdist.as<double>());
    }
    hipError_t e = hipMemcpy(cells, bcell.p, (size_t)n * max_cells * 2 * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(dists, bdist.p, (size_t)n * max_cells * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { cis_set_error("hipMemcpy failed: %s", hipGetErrorString(e)); return done(CIS_EHIP); }
    return done(CIS_OK);
}

// ---- routed cell-sharded search (round 5): which ranks own the cells a query visits ---------------------------------------------
// The all-gather protocol hands every rank the whole batch: projection, cell ranking and walk are done `world` times over.  Routed,
// a query's HOME rank (1 / world of the batch each) walks the multisequence against the cell sizes of the whole index -- the same
// walk as k_plan (lopq/lopq/search.py:58-82, :128-133), no items -- and notes the owner of every non-empty visited cell; only those
// ranks (one or two at V = 16) receive the query (columbiaimagesearch_amd/distributed.py: RoutedSearcher).
template <typename CT>
__global__ __launch_bounds__(64) void k_plan_owners(const CT* __restrict__ sorted, const uint16_t* __restrict__ order,
                                                    const int64_t* __restrict__ gcount, const int32_t* __restrict__ owner, int world,
                                                    int nq, int V, int64_t quota, unsigned long long* __restrict__ mask,
                                                    int32_t* __restrict__ visited_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* t = reinterpret_cast<int*>(smem);  // [V]
    const int q = blockIdx.x;
    const int lane = threadIdx.x;
    const CT* d0 = sorted + ((int64_t)q * 2 + 0) * V;
    const CT* d1 = sorted + ((int64_t)q * 2 + 1) * V;
    const uint16_t* o0 = order + ((int64_t)q * 2 + 0) * V;
    const uint16_t* o1 = order + ((int64_t)q * 2 + 1) * V;
    for (int i = lane; i < V; i += 64) t[i] = 0;
    __syncthreads();
    unsigned long long mk = 0ull;
    const int visited = walk_quota<CT, false, false>(d0, d1, o0, o1, t, V, lane, gcount, nullptr, quota,
                                                     [&](int, int, int, int64_t cell, int64_t gc, int64_t, int64_t) {
        if (gc > 0) mk |= 1ull << (owner ? owner[cell] : (int)(cell % world));
    });
    if (lane == 0) {
        mask[q] = mk;
        if (visited_out) visited_out[q] = visited;
    }
}

template <typename CT>
static void launch_plan_owners(cis_index* ix, int nq, int64_t quota, int* grp_cnt, const int32_t* d_owner, uint64_t* d_mask, int32_t* d_visited,
                               hipStream_t st) {
    const int V = ix->m->V;
    launch_rank<CT>(ix, nq, false, grp_cnt, st);  // (V <= 4096: k_rank_sort for every V > 256)
    hipLaunchKernelGGL(k_plan_owners<CT>, dim3(nq), dim3(64), (size_t)V * sizeof(int), st, ix->w_sorted.as<CT>(), ix->w_order.as<uint16_t>(),
                       ix->gcount_ptr(), d_owner, ix->world, nq, V, quota, (unsigned long long*)d_mask, d_visited);
}

extern "C" int cis_index_query_owners_dev(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota, uint64_t* d_mask,
                                          int32_t* d_visited, void* stream) {
    CIS_REQUIRE(ix != nullptr, "index is NULL");
    CIS_REQUIRE(q_dtype == CIS_F32 || q_dtype == CIS_F64, "q_dtype must be 4 or 8");
    CIS_REQUIRE(nq >= 0 && (nq == 0 || (dQ && d_mask)), "NULL buffer");
    CIS_REQUIRE(!ix->orphaned, "this view's base index was destroyed: close views before their base");
    CIS_REQUIRE(ix->world >= 1 && ix->world <= 64, "owner masks hold 64 ranks");
    if (nq == 0) return CIS_OK;
    CIS_TRY(cis_index_ready(ix->base ? ix->base : ix));
    ix->sync_from_base();
    cis_model* m = ix->m;
    CIS_CHECK_HIP(hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    CIS_REQUIRE(m->V <= 4096, "owner walk: V <= 4096");
    Front f;  // the rank kernels leave the table-group counters zeroed, as every search expects to find them
    CIS_TRY(front_prepare(ix, dQ, q_dtype, nq, st, &f));
    CIS_TRY(cis_launch_sqdist_both(m, f.xc, f.ct, nq, ix->w_cd.p, st));
    const cis_index* own = ix->base ? ix->base : ix;  // a view reads the owner table of its base
    const int32_t* d_owner = own->owner.empty() ? nullptr : own->d_owner.as<int32_t>();
    CIS_REQUIRE(own->owner.empty() || d_owner != nullptr, "owner table not on the device");
    if (f.ct == CIS_F32) launch_plan_owners<float>(ix, nq, quota, f.grp_cnt, d_owner, d_mask, d_visited, st);
    else launch_plan_owners<double>(ix, nq, quota, f.grp_cnt, d_owner, d_mask, d_visited, st);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}
