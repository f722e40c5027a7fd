// Removal of items by id from the HBM-resident index (the stores of lopq_index.hip), on the device.
//
// remove(ids): every stored item whose id is in the list leaves the index -- from every cell that holds it, every copy inside a cell
// (dedup = 0 inserts can store an id more than once); kept items keep their relative order inside their cell (the reference's per-cell
// list order, lopq/lopq/search.py:359, which breaks ties in search).  Ids that are not stored, ids that occur more than once in the
// list and negative ids are ignored; an empty list is a no-op.  Afterwards the index equals one built by the same insert calls with
// the removed ids filtered out of every batch: a removed id may be inserted again and lands behind its cell's last item.
//
// Layout invariants (CellStore, lopq_index.h): a cell owns the room [loff[c], loff[c+1]) and uses [loff[c], lend[c]) of it.  A removal
// moves only lend[c] down: the room stays (more slack for the next in-place insert) and the next rebuild renews it.  cmax[c] (1 + the
// largest id stored in the cell, 0: empty) is RECOMPUTED EXACTLY for every touched cell by the compaction kernel; untouched cells
// keep theirs.  The global cell sizes (d_gcount) drop for the cells this shard owns; the id-only store of a sharded index drops the
// ids too but leaves d_gcount alone: the sizes of cells that other shards own change through cis_index_sub_remote_counts[_dev] only.
// d_plan_hint (k_plan_par: cells visited per unit of quota in the previous launches) only sizes the plan's bands, so a stale value
// cannot make a result wrong; it is reset all the same, because after a large removal it would undersize the first band.
//
// Kernels, all on one stream, the kernel boundary is the only hand-off:
//   removal set   n <= RM_LDS_MAX: k_rm_set_sort, one workgroup sorts the ids (negatives behind) -> every marking workgroup copies the
//                 sorted list into LDS and probes it by binary search.  Larger lists: an open-addressing table in global memory at
//                 load <= 0.25 (k_rm_tab_insert; splitmix64 finaliser and linear probing as lopq_rerank.hip's k_idmap_*).
//   mark          one pass over the slots of ids[cur]: 8 B per stored item, no codes.  k_rm_mark: slot-parallel, grid-stride; only a
//                 slot whose id is in the set looks up its cell (binary search in loff, as k_ins_move) and tests p < lend[c] (a cell's
//                 slack holds stale data); the per-cell counter takes ONE atomic per run of equal cells in a wave.  k_rm_mark_cells:
//                 thread per cell for millions of tiny cells (the shape k_ins_move_cells takes), no atomics.  Both write a kill flag
//                 per used slot.  Integer atomics only: equal inputs give equal bytes.
//   touched list  the cells with a non-zero counter, in cell order, by a scan of the counters (k_rm_list_small: one workgroup up to
//                 65536 cells; k_rm_touch + dev_exclusive_scan + k_rm_list beyond).
//   compact       k_rm_compact<MW>: a workgroup per touched cell (grid-stride over the list: the work is O(touched cells)) walks the
//                 cell in chunks of RM_CHUNK items: ids, code words and flags into registers, barrier, kept items to dst <= src, in
//                 place and stable; then the cell's lend, gcount, cmax and the caller's per-cell delta.  k_rm_compact_wave: a wave
//                 per cell for tiny cells.  No generation swap, no rebuild.
//   One workgroup walks a cell serially: with a few hundred cells over 10^8 items a cell holds ~10^6 items and the compaction of one
//   touched cell is a serial walk of 16 B x its items (DESIGN.md records the measured figure as the known limit).
#include <algorithm>

#include "lopq_index.h"
#include "dev_scan.h"

namespace {

constexpr int RM_LDS_MAX = 1024;   // ids the LDS form of the removal set holds (8 KB per marking workgroup); see DESIGN.md for the A/B
constexpr int RM_CT = 1024;        // threads of a compaction workgroup: one workgroup walks a cell, so a round must move many items
constexpr int RM_PER = 4;          // consecutive items per thread and chunk
constexpr int RM_CHUNK = RM_CT * RM_PER;
constexpr int RM_MARK_GRID = 2048; // marking workgroups (256 CUs x 8): each copies the LDS set once and strides over the slots
constexpr int64_t RM_EMPTY = -1;

// splitmix64's finaliser (as lopq_rerank.hip): device ids are small integers or 2^62 + slot
__device__ __forceinline__ uint64_t rm_mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

// ---- removal set ------------------------------------------------------------------------------------------------------------------
// One workgroup, n <= RM_LDS_MAX: out[0] = m, the number of ids >= 0; out[1 .. m] = those ids ascending (duplicates stay: harmless for
// the binary search)
__global__ __launch_bounds__(1024) void k_rm_set_sort(const int64_t* __restrict__ ids, int n, int64_t* __restrict__ out) {
    __shared__ uint64_t s_k[RM_LDS_MAX];
    const int i = threadIdx.x;
    uint64_t k = ~0ull;  // negative ids and padding sort behind every id
    if (i < n) {
        const int64_t id = ids[i];
        if (id >= 0) k = (uint64_t)id;
    }
    s_k[i] = k;
    int n2 = 64;
    while (n2 < n) n2 <<= 1;
    for (int kk = 2; kk <= n2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            __syncthreads();
            if (i < (n2 >> 1)) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const bool up = (lo & kk) == 0;
                const uint64_t a = s_k[lo], b = s_k[hi];
                if ((b < a) == up) { s_k[lo] = b; s_k[hi] = a; }
            }
        }
    __syncthreads();
    if (i < n) {
        const uint64_t v = s_k[i];
        if (v != ~0ull) {
            out[1 + i] = (int64_t)v;
            if (i + 1 == n || s_k[i + 1] == ~0ull) out[0] = i + 1;
        } else if (i == 0) {
            out[0] = 0;
        }
    }
}

// cap >= 4 n, a power of two, keys preset to RM_EMPTY: a chain always ends at an empty slot
__global__ __launch_bounds__(256) void k_rm_tab_insert(const int64_t* __restrict__ ids, int64_t n, int64_t* __restrict__ keys, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    if (id < 0) return;
    const uint64_t mask = (uint64_t)cap - 1;
    uint64_t h = rm_mix64((uint64_t)id) & mask;
    for (int64_t p = 0; p < cap; ++p) {
        const unsigned long long prev = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)RM_EMPTY, (unsigned long long)id);
        if (prev == (unsigned long long)RM_EMPTY || prev == (unsigned long long)id) return;
        h = (h + 1) & mask;
    }
}

// the set as a marking thread sees it: LDS = true: `s` is the sorted list in LDS, n its length; false: `s` is the table, n its capacity
template <bool LDS>
__device__ __forceinline__ bool rm_contains(const int64_t* s, int64_t n, int64_t id) {
    if (id < 0) return false;
    if constexpr (LDS) {
        if (n == 0 || id < s[0] || id > s[n - 1]) return false;
        int lo = 0, hi = (int)n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        return lo < (int)n && s[lo] == id;
    } else {
        const uint64_t mask = (uint64_t)n - 1;
        uint64_t h = rm_mix64((uint64_t)id) & mask;
        for (int64_t p = 0; p < n; ++p) {
            const int64_t k = s[h];
            if (k == id) return true;
            if (k == RM_EMPTY) return false;
            h = (h + 1) & mask;
        }
        return false;
    }
}

// every thread of the workgroup calls this (it holds a barrier); returns the set's length
template <bool LDS>
__device__ __forceinline__ int64_t rm_stage_set(const int64_t* __restrict__ set, int64_t set_n, int64_t* s_set) {
    if constexpr (LDS) {
        const int64_t m = set[0];
        for (int i = threadIdx.x; i < m; i += blockDim.x) s_set[i] = set[1 + i];
        __syncthreads();
        return m;
    } else {
        return set_n;
    }
}

// ---- mark -------------------------------------------------------------------------------------------------------------------------
// Slot-parallel.  kill[p] = 1 for a used slot whose id is in the set, 0 for every other slot below the layout's extent; rcnt[c] +=
// the cell's killed slots (rcnt is zero on entry), one atomic per run of equal cells in a wave: the slots of a wave are in position
// order, so the lanes of a cell are contiguous and a wave usually holds one or two cells.
template <bool LDS>
__global__ __launch_bounds__(256) void k_rm_mark(const int64_t* __restrict__ loff, const int64_t* __restrict__ lend, int64_t ncells,
                                                 int64_t cap_bound, const int64_t* __restrict__ ids, const int64_t* __restrict__ set,
                                                 int64_t set_n, uint8_t* __restrict__ kill, uint32_t* __restrict__ rcnt) {
    __shared__ int64_t s_set[LDS ? RM_LDS_MAX : 1];
    const int64_t sn = rm_stage_set<LDS>(set, set_n, s_set);
    const int64_t* sp = LDS ? s_set : set;
    int64_t extent = loff[ncells];
    if (extent > cap_bound) extent = cap_bound;
    const int lane = threadIdx.x & 63;
    for (int64_t p0 = (int64_t)blockIdx.x * 256; p0 < extent; p0 += (int64_t)gridDim.x * 256) {
        const int64_t p = p0 + threadIdx.x;
        bool hit = false;
        uint32_t c = 0;
        if (p < extent) {
            hit = rm_contains<LDS>(sp, sn, ids[p]);
            if (hit) {
                int64_t lo = 0, hi = ncells;  // largest c with loff[c] <= p
                while (hi - lo > 1) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (loff[mid] <= p) lo = mid;
                    else hi = mid;
                }
                c = (uint32_t)lo;
                hit = p < lend[lo];  // (a slot of the cell's slack holds stale data)
            }
            kill[p] = hit ? 1 : 0;
        }
        unsigned long long m = __ballot(hit);
        while (m) {  // wave-uniform: one round per distinct cell among the wave's hits
            const int leader = __ffsll((long long)m) - 1;
            const uint32_t cl = __shfl(c, leader);
            const unsigned long long same = __ballot(hit && c == cl);
            if (lane == leader) atomicAdd(&rcnt[cl], (uint32_t)__popcll(same));
            m &= ~same;
        }
    }
}

// Thread per cell (millions of tiny cells): no atomics, rcnt[c] is written for every cell
template <bool LDS>
__global__ __launch_bounds__(256) void k_rm_mark_cells(const int64_t* __restrict__ loff, const int64_t* __restrict__ lend, int64_t ncells,
                                                       const int64_t* __restrict__ ids, const int64_t* __restrict__ set, int64_t set_n,
                                                       uint8_t* __restrict__ kill, uint32_t* __restrict__ rcnt) {
    __shared__ int64_t s_set[LDS ? RM_LDS_MAX : 1];
    const int64_t sn = rm_stage_set<LDS>(set, set_n, s_set);
    const int64_t* sp = LDS ? s_set : set;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncells) return;
    uint32_t r = 0;
    for (int64_t p = loff[c], e = lend[c]; p < e; ++p) {
        const bool hit = rm_contains<LDS>(sp, sn, ids[p]);
        kill[p] = hit ? 1 : 0;
        r += hit ? 1u : 0u;
    }
    rcnt[c] = r;
}

// ---- touched cells ----------------------------------------------------------------------------------------------------------------
// One workgroup (ncells <= 65536): list[0 .. nt) = the cells with rcnt > 0, ascending; ntouched[0] = nt
// sum of one value per thread over a workgroup of 256 threads (valid in thread 0)
__device__ __forceinline__ unsigned long long rm_block_sum(unsigned long long v, unsigned long long* sh /* [4] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// The removed count of the store goes to stats[rem_word] from here and from k_rm_touch: a sum over the per-cell counters with one
// atomic per workgroup -- a million touched cells adding to one word from the compaction kernel took 10 ms.
__global__ __launch_bounds__(SCAN_T) void k_rm_list_small(const uint32_t* __restrict__ rcnt, int64_t ncells, uint32_t* __restrict__ list,
                                                          uint32_t* __restrict__ ntouched, int64_t* __restrict__ stats, int rem_word) {
    __shared__ uint32_t sh[SCAN_T / 64 + 1];
    __shared__ unsigned long long sh_sum[4];
    uint32_t carry = 0;
    unsigned long long removed = 0ull;
    for (int64_t b = 0; b < ncells; b += SCAN_T) {
        const int64_t c = b + threadIdx.x;
        const uint32_t r = c < ncells ? rcnt[c] : 0u;
        const uint32_t f = r > 0 ? 1u : 0u;
        uint32_t tot;
        const uint32_t e = block_excl_scan<uint32_t>(f, sh, &tot);
        if (f) list[carry + e] = (uint32_t)c;
        carry += tot;
        removed += r;
    }
    removed = rm_block_sum(removed, sh_sum);
    if (threadIdx.x == 0) {
        ntouched[0] = carry;
        stats[rem_word] += (int64_t)removed;
    }
}

// grid-stride (at most 1024 workgroups of 256): the touched flags for the scan, and the removed count
__global__ __launch_bounds__(256) void k_rm_touch(const uint32_t* __restrict__ rcnt, int64_t ncells, uint32_t* __restrict__ flag,
                                                  int64_t* __restrict__ stats, int rem_word) {
    __shared__ unsigned long long sh_sum[4];
    unsigned long long removed = 0ull;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < ncells; c += (int64_t)gridDim.x * 256) {
        const uint32_t r = rcnt[c];
        flag[c] = r > 0 ? 1u : 0u;
        removed += r;
    }
    removed = rm_block_sum(removed, sh_sum);
    if (threadIdx.x == 0 && removed) atomicAdd((unsigned long long*)&stats[rem_word], removed);
}

// pre = exclusive scan of the touched flags (in `list`'s place would race: a buffer of its own)
__global__ void k_rm_list(const uint32_t* __restrict__ rcnt, const uint32_t* __restrict__ pre, int64_t ncells, uint32_t* __restrict__ list) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < ncells && rcnt[c] > 0) list[pre[c]] = (uint32_t)c;
}

// ---- compact ----------------------------------------------------------------------------------------------------------------------
// what a touched cell's walk ends with (one thread): the used end, the largest id + 1 (exact), the cell sizes
__device__ __forceinline__ void rm_finish_cell(uint32_t c, int64_t new_end, unsigned long long mx, const uint32_t* __restrict__ rcnt,
                                               int64_t* __restrict__ lend, unsigned long long* __restrict__ cmaxp,
                                               int64_t* __restrict__ gcount, int64_t* __restrict__ delta) {
    const int64_t r = (int64_t)rcnt[c];
    lend[c] = new_end;
    cmaxp[c] = mx;
    if (gcount) gcount[c] -= r;
    if (delta) delta[c] = r;
}

// s_waitcnt vmcnt(0): this wave's global loads have returned.  A workgroup barrier orders them against the other waves' later
// stores by the memory model alone (the compiler waits only for LDS there); the in-place move states it outright -- the data is
// needed right behind the barrier anyway.
#define RM_LOADS_LANDED() __builtin_amdgcn_s_waitcnt(0x0f70)

// exclusive scan of one small count per thread over the RM_CT threads of a compaction workgroup (block_excl_scan's form at 16 waves)
__device__ __forceinline__ int rm_block_excl_scan(int v, int* sh /* [RM_CT / 64] */, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = wave_incl_scan<int>(v);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < RM_CT / 64; ++i) {
        const int x = sh[i];
        base += (i < w) ? x : 0;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// A workgroup per touched cell, grid-stride over the list.  Chunk of RM_CHUNK = 4096 items: thread t of 1024 holds items [4 t, 4 t + 4) of it.  All
// loads of a chunk come before the barriers of the prefix sum (and have landed: RM_LOADS_LANDED), all stores after them, and a
// chunk's stores end at or below the next chunk's first slot: dst <= src throughout.
// MW: code words per item (M = 4 MW); MW = 0: M bytes per item, moved a byte column at a time (a barrier between the column's loads
// and its stores; columns do not overlap); codes == nullptr: the id-only store.
template <int MW>
__global__ __launch_bounds__(RM_CT) void k_rm_compact(const uint32_t* __restrict__ list, const uint32_t* __restrict__ ntouched,
                                                    const uint32_t* __restrict__ rcnt, const int64_t* __restrict__ loff,
                                                    int64_t* __restrict__ lend, int64_t* ids, uint8_t* codes, int M,
                                                    const uint8_t* __restrict__ kill, unsigned long long* __restrict__ cmaxp,
                                                    int64_t* __restrict__ gcount, int64_t* __restrict__ delta) {
    __shared__ int sh[RM_CT / 64];
    __shared__ unsigned long long s_mx[RM_CT / 64];
    const uint32_t nt = ntouched[0];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint32_t c = list[t];
        const int64_t b = loff[c], e = lend[c];
        int64_t dst = b;
        unsigned long long mx = 0ull;
        for (int64_t p0 = b; p0 < e; p0 += RM_CHUNK) {
            const int64_t p = p0 + (int64_t)tid * RM_PER;
            int64_t id[RM_PER];
            uint32_t cw[RM_PER][MW > 0 ? MW : 1];
            bool keep[RM_PER];
            int s = 0;
#pragma unroll
            for (int j = 0; j < RM_PER; ++j) {
                const bool ok = p + j < e;
                keep[j] = ok && kill[ok ? p + j : b] == 0;
                id[j] = ok ? ids[p + j] : 0;
                if constexpr (MW > 0) {
                    if (codes) {
                        const uint32_t* src = reinterpret_cast<const uint32_t*>(codes) + (ok ? p + j : b) * MW;
#pragma unroll
                        for (int w = 0; w < MW; ++w) cw[j][w] = src[w];
                    }
                }
                s += keep[j] ? 1 : 0;
            }
            RM_LOADS_LANDED();
            int tot;
            const int base = rm_block_excl_scan(s, sh, &tot);
            int64_t d = dst + base;
            const int64_t d0 = d;
#pragma unroll
            for (int j = 0; j < RM_PER; ++j) {
                if (keep[j]) {
                    if (d != p + j) {
                        ids[d] = id[j];
                        if constexpr (MW > 0) {
                            if (codes) {
                                uint32_t* o = reinterpret_cast<uint32_t*>(codes) + d * MW;
#pragma unroll
                                for (int w = 0; w < MW; ++w) o[w] = cw[j][w];
                            }
                        }
                    }
                    const unsigned long long v = (unsigned long long)id[j] + 1ull;
                    mx = v > mx ? v : mx;
                    ++d;
                }
            }
            if constexpr (MW == 0) {
                if (codes) {
                    for (int i = 0; i < M; ++i) {  // (uniform: every thread takes every column and its barrier)
                        uint8_t v[RM_PER];
#pragma unroll
                        for (int j = 0; j < RM_PER; ++j) v[j] = keep[j] ? codes[(p + j) * M + i] : (uint8_t)0;
                        RM_LOADS_LANDED();
                        __syncthreads();
                        int64_t dd = d0;
#pragma unroll
                        for (int j = 0; j < RM_PER; ++j)
                            if (keep[j]) { codes[dd * M + i] = v[j]; ++dd; }
                    }
                    __syncthreads();  // the last column's stores are behind every thread before the next chunk's loads
                }
            }
            dst += tot;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long u = __shfl_xor(mx, o);
            mx = u > mx ? u : mx;
        }
        if (lane == 0) s_mx[wv] = mx;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < RM_CT / 64; ++w) mx = s_mx[w] > mx ? s_mx[w] : mx;
            rm_finish_cell(c, dst, mx, rcnt, lend, cmaxp, gcount, delta);
        }
        __syncthreads();
    }
}

// A wave per touched cell (tiny cells), 64 items per round, codes a byte column at a time: inside a wave every lane's load of a
// column precedes every lane's store of it (one instruction each), and columns do not overlap.
__global__ __launch_bounds__(256) void k_rm_compact_wave(const uint32_t* __restrict__ list, const uint32_t* __restrict__ ntouched,
                                                         const uint32_t* __restrict__ rcnt, const int64_t* __restrict__ loff,
                                                         int64_t* __restrict__ lend, int64_t* ids, uint8_t* codes, int M,
                                                         const uint8_t* __restrict__ kill, unsigned long long* __restrict__ cmaxp,
                                                         int64_t* __restrict__ gcount, int64_t* __restrict__ delta) {
    const uint32_t nt = ntouched[0];
    const int lane = threadIdx.x & 63;
    const uint32_t nw = gridDim.x * 4;
    for (uint32_t t = blockIdx.x * 4 + (threadIdx.x >> 6); t < nt; t += nw) {
        const uint32_t c = list[t];
        const int64_t b = loff[c], e = lend[c];
        int64_t dst = b;
        unsigned long long mx = 0ull;
        for (int64_t p0 = b; p0 < e; p0 += 64) {
            const int64_t p = p0 + lane;
            const bool ok = p < e;
            const bool keep = ok && kill[ok ? p : b] == 0;
            const int64_t id = ok ? ids[p] : 0;
            const unsigned long long km = __ballot(keep);
            const int64_t d = dst + __popcll(km & ((1ull << lane) - 1ull));
            if (keep) {
                const unsigned long long v = (unsigned long long)id + 1ull;
                mx = v > mx ? v : mx;
            }
            if (keep && d != p) ids[d] = id;
            if (codes) {
                for (int i = 0; i < M; ++i) {
                    const uint8_t v = keep ? codes[p * M + i] : (uint8_t)0;
                    if (keep && d != p) codes[d * M + i] = v;
                }
            }
            dst += __popcll(km);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long u = __shfl_xor(mx, o);
            mx = u > mx ? u : mx;
        }
        if (lane == 0) rm_finish_cell(c, dst, mx, rcnt, lend, cmaxp, gcount, delta);
    }
}

// ---- remote cell sizes ------------------------------------------------------------------------------------------------------------
// first pass: would any count go negative?  (entries of owned cells are ignored, as k_add_remote does)
__global__ void k_sub_remote_check(const int64_t* __restrict__ gcount, const int64_t* __restrict__ delta, int64_t ncells,
                                   const int32_t* __restrict__ owner, int rank, int world, int64_t* __restrict__ stats) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells) return;
    const int64_t d = delta[c];
    if (d < 0) { stats[INS_ERR] = 1; return; }
    if (d == 0) return;
    const bool mine = world <= 1 || (owner ? owner[c] == rank : (int)(c % world) == rank);
    if (!mine && gcount[c] < d) stats[INS_ERR] = 1;
}

// second pass: nothing changes when the first one raised the error word
__global__ void k_sub_remote(int64_t* __restrict__ gcount, const int64_t* __restrict__ delta, int64_t ncells,
                             const int32_t* __restrict__ owner, int rank, int world, const int64_t* __restrict__ stats) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncells || stats[INS_ERR] != 0) return;
    const int64_t d = delta[c];
    const bool mine = world <= 1 || (owner ? owner[c] == rank : (int)(c % world) == rank);
    if (d > 0 && !mine) gcount[c] -= d;
}

inline unsigned grid_for(int64_t n, int t) { return (unsigned)(n > 0 ? ceil_div(n, t) : 1); }

// the LDS form of the set up to this many ids (CIS_REMOVE_LDS_MAX lowers it for the A/B of tools/bench_remove.py; read per call)
int lds_switch() {
    const char* e = getenv("CIS_REMOVE_LDS_MAX");
    const int v = e ? atoi(e) : RM_LDS_MAX;
    return v < 0 ? 0 : (v > RM_LDS_MAX ? RM_LDS_MAX : v);
}

struct RmSet {
    const int64_t* p;  // LDS form: [0] = m, [1 .. m] sorted ids; table form: the keys
    int64_t n;         // table form: the capacity
    bool lds;
};

// mark + touched list + compact on one store; the removed count is added to stats[rem_word] (by the list kernels)
int store_remove(cis_index* ix, CellStore& s, const RmSet& set, int64_t* gcount, int64_t* d_delta, int rem_word, bool timed, hipStream_t st) {
    if (!s.init || s.n == 0 || s.cap == 0) return CIS_OK;
    const int64_t nc = ix->ncells;
    const int M = ix->M;
    CIS_TRY(ix->wi_acc.reserve((size_t)s.cap));                                    // kill flags, one byte per slot
    CIS_TRY(ix->wi_cnt.reserve((size_t)nc * sizeof(uint32_t)));                    // removed per cell
    CIS_TRY(ix->wi_cnt2.reserve((size_t)(2 * nc + 2) * sizeof(uint32_t)));         // touched cells, their number, the scan's prefix
    CIS_TRY(ix->wi_scan.reserve((size_t)(ceil_div(nc + 1, SCAN_TILE) + 2) * sizeof(int64_t) + 64));
    uint8_t* kill = ix->wi_acc.as<uint8_t>();
    uint32_t* rcnt = ix->wi_cnt.as<uint32_t>();
    uint32_t* list = ix->wi_cnt2.as<uint32_t>();
    uint32_t* ntouched = list + nc;
    uint32_t* pre = list + nc + 1;
    int64_t* loff = s.loff[s.cur].as<int64_t>();
    int64_t* lend = loff + nc + 1;
    int64_t* ids = s.ids[s.cur].as<int64_t>();
    uint8_t* codes = s.with_codes ? s.codes[s.cur].as<uint8_t>() : nullptr;
    const bool tiny = s.n / nc < 16 && nc >= 65536;  // the shape k_ins_move_cells takes
    if (tiny) {
        if (set.lds) hipLaunchKernelGGL((k_rm_mark_cells<true>), dim3(grid_for(nc, 256)), dim3(256), 0, st, (const int64_t*)loff, (const int64_t*)lend, nc,
                                        (const int64_t*)ids, set.p, set.n, kill, rcnt);
        else hipLaunchKernelGGL((k_rm_mark_cells<false>), dim3(grid_for(nc, 256)), dim3(256), 0, st, (const int64_t*)loff, (const int64_t*)lend, nc,
                                (const int64_t*)ids, set.p, set.n, kill, rcnt);
    } else {
        CIS_CHECK_HIP(hipMemsetAsync(rcnt, 0, (size_t)nc * sizeof(uint32_t), st));
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(s.cap, 256), RM_MARK_GRID);
        if (set.lds) hipLaunchKernelGGL((k_rm_mark<true>), dim3(grid), dim3(256), 0, st, (const int64_t*)loff, (const int64_t*)lend, nc, s.cap,
                                        (const int64_t*)ids, set.p, set.n, kill, rcnt);
        else hipLaunchKernelGGL((k_rm_mark<false>), dim3(grid), dim3(256), 0, st, (const int64_t*)loff, (const int64_t*)lend, nc, s.cap,
                                (const int64_t*)ids, set.p, set.n, kill, rcnt);
    }
    if (timed) CIS_CHECK_HIP(hipEventRecord(ix->rm_ev[2], st));
    int64_t* stats = ix->d_stats.as<int64_t>();
    if (nc <= 65536) {
        hipLaunchKernelGGL(k_rm_list_small, dim3(1), dim3(SCAN_T), 0, st, (const uint32_t*)rcnt, nc, list, ntouched, stats, rem_word);
    } else {
        hipLaunchKernelGGL(k_rm_touch, dim3((unsigned)std::min<int64_t>(ceil_div(nc, 256), 1024)), dim3(256), 0, st, (const uint32_t*)rcnt, nc, pre, stats,
                           rem_word);
        dev_exclusive_scan<uint32_t, uint32_t>(pre, pre, nc, ix->wi_scan.as<uint32_t>(), ntouched, nullptr, st);
        hipLaunchKernelGGL(k_rm_list, dim3(grid_for(nc, 256)), dim3(256), 0, st, (const uint32_t*)rcnt, (const uint32_t*)pre, nc, list);
    }
    unsigned long long* cmaxp = s.cmax.as<unsigned long long>();
    if (tiny) {
        const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(nc, 4), 8192);
        hipLaunchKernelGGL(k_rm_compact_wave, dim3(grid), dim3(256), 0, st, (const uint32_t*)list, (const uint32_t*)ntouched, (const uint32_t*)rcnt,
                           (const int64_t*)loff, lend, ids, codes, M, (const uint8_t*)kill, cmaxp, gcount, d_delta);
    } else {
        const unsigned grid = (unsigned)std::min<int64_t>(nc, 1024);
#define CIS_COMPACT(MW)                                                                                                                       \
    hipLaunchKernelGGL((k_rm_compact<MW>), dim3(grid), dim3(RM_CT), 0, st, (const uint32_t*)list, (const uint32_t*)ntouched, (const uint32_t*)rcnt, \
                       (const int64_t*)loff, lend, ids, codes, M, (const uint8_t*)kill, cmaxp, gcount, d_delta)
        if (!codes || M == 4) CIS_COMPACT(1);
        else if (M == 8) CIS_COMPACT(2);
        else if (M == 16) CIS_COMPACT(4);
        else if (M == 32) CIS_COMPACT(8);
        else CIS_COMPACT(0);
#undef CIS_COMPACT
    }
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

int index_remove_dev(cis_index* ix, const int64_t* d_ids, int64_t n, int64_t* n_removed, int64_t* d_cell_delta, hipStream_t st) {
    CIS_TRY(cis_index_ready(ix));
    CIS_CHECK_HIP(hipSetDevice(ix->m->device));
    if (n_removed) *n_removed = 0;
    const int64_t nc = ix->ncells;
    if (d_cell_delta) CIS_CHECK_HIP(hipMemsetAsync(d_cell_delta, 0, (size_t)nc * sizeof(int64_t), st));
    if (n == 0 || ix->own.n + ix->ghost.n == 0) return CIS_OK;
    if (ix->profiling != 0) {
        for (hipEvent_t& e : ix->rm_ev)
            if (!e) CIS_CHECK_HIP(hipEventCreate(&e));
        CIS_CHECK_HIP(hipEventRecord(ix->rm_ev[0], st));
    }
    // ---- the removal set ----
    RmSet set;
    set.lds = n <= lds_switch();
    if (set.lds) {
        CIS_TRY(ix->wi_tmp.reserve((size_t)(RM_LDS_MAX + 1) * sizeof(int64_t)));
        hipLaunchKernelGGL(k_rm_set_sort, dim3(1), dim3(1024), 0, st, d_ids, (int)n, ix->wi_tmp.as<int64_t>());
        set.p = ix->wi_tmp.as<int64_t>();
        set.n = 0;
    } else {
        int64_t cap = 1024;
        while (cap < 4 * n) cap <<= 1;  // load <= 0.25: nearly every probe is a miss, and a miss walks to the next empty slot
        CIS_TRY(ix->wi_tmp.reserve((size_t)cap * sizeof(int64_t)));
        CIS_CHECK_HIP(hipMemsetAsync(ix->wi_tmp.p, 0xff, (size_t)cap * sizeof(int64_t), st));  // RM_EMPTY
        hipLaunchKernelGGL(k_rm_tab_insert, dim3(grid_for(n, 256)), dim3(256), 0, st, d_ids, n, ix->wi_tmp.as<int64_t>(), cap);
        set.p = ix->wi_tmp.as<int64_t>();
        set.n = cap;
    }
    CIS_CHECK_HIP(hipMemsetAsync(ix->d_stats.p, 0, INS_WORDS * sizeof(int64_t), st));
    ix->stats_fresh = false;
    const bool timed = ix->profiling != 0 && ix->own.n > 0;  // (cis_index_set_profiling: tools/bench_remove.py splits a removal into its stages)
    if (timed) CIS_CHECK_HIP(hipEventRecord(ix->rm_ev[1], st));
    CIS_TRY(store_remove(ix, ix->own, set, ix->d_gcount.as<int64_t>(), d_cell_delta, INS_REM_OWN, timed, st));
    if (timed) CIS_CHECK_HIP(hipEventRecord(ix->rm_ev[3], st));
    // the id-only store of the other shards' cells: its ids leave too (a re-insert must not be taken for a duplicate); the sizes of
    // those cells change through cis_index_sub_remote_counts only
    CIS_TRY(store_remove(ix, ix->ghost, set, nullptr, nullptr, INS_REM_GHOST, false, st));
    CIS_CHECK_HIP(hipMemsetAsync(ix->d_plan_hint.p, 0, 4 * sizeof(unsigned long long), st));
    CIS_TRY(cis_index_refresh_stats(ix, st));  // the one host round trip: cell-size statistics and the removed counts
    ix->stats_fresh = true;
    if (timed)
        for (int i = 0; i < 3; ++i) {
            float ms = 0.f;
            CIS_CHECK_HIP(hipEventElapsedTime(&ms, ix->rm_ev[i], ix->rm_ev[i + 1]));
            ix->rm_ms[i] = ms;
        }
    ix->own.n -= ix->h_ins[INS_REM_OWN];
    ix->ghost.n -= ix->h_ins[INS_REM_GHOST];
    ix->n_local = ix->own.n;
    if (n_removed) *n_removed = ix->h_ins[INS_REM_OWN];
    return CIS_OK;
}

int sub_remote_dev(cis_index* ix, const int64_t* d_delta, hipStream_t st) {
    CIS_TRY(cis_index_ready(ix));
    CIS_CHECK_HIP(hipSetDevice(ix->m->device));
    const int64_t nc = ix->ncells;
    CIS_CHECK_HIP(hipMemsetAsync(ix->d_stats.p, 0, INS_WORDS * sizeof(int64_t), st));
    const int32_t* owner = ix->d_owner.as<int32_t>();
    hipLaunchKernelGGL(k_sub_remote_check, dim3(grid_for(nc, 256)), dim3(256), 0, st, (const int64_t*)ix->d_gcount.as<int64_t>(), d_delta, nc, owner,
                       ix->rank, ix->world, ix->d_stats.as<int64_t>());
    hipLaunchKernelGGL(k_sub_remote, dim3(grid_for(nc, 256)), dim3(256), 0, st, ix->d_gcount.as<int64_t>(), d_delta, nc, owner, ix->rank, ix->world,
                       (const int64_t*)ix->d_stats.as<int64_t>());
    CIS_CHECK_HIP(hipGetLastError());
    ix->stats_fresh = false;
    CIS_TRY(cis_index_refresh_stats(ix, st));
    ix->stats_fresh = true;
    CIS_REQUIRE(ix->h_ins[INS_ERR] == 0, "a per-cell count is negative or would go negative: nothing was changed");
    return CIS_OK;
}

}  // namespace

#define CIS_RM_WRITABLE(ix) \
    CIS_REQUIRE((ix)->base == nullptr && !(ix)->orphaned, "this handle is a search view (cis_index_create_view): it is read-only, remove through the base index")

extern "C" int cis_index_remove_dev(cis_index* ix, const int64_t* d_ids, int64_t n, int64_t* n_removed, int64_t* d_cell_delta,
                                    void* stream) {
    CIS_REQUIRE(ix != nullptr, "index is NULL");
    CIS_REQUIRE(n >= 0 && (n == 0 || d_ids), "NULL buffer or negative count");
    CIS_REQUIRE(n < ((int64_t)1 << 31), "at most 2^31 - 1 ids per removal call");
    CIS_RM_WRITABLE(ix);
    return index_remove_dev(ix, d_ids, n, n_removed, d_cell_delta, (hipStream_t)stream);
}

extern "C" int cis_index_remove(cis_index* ix, const int64_t* ids, int64_t n, int64_t* n_removed) {
    CIS_REQUIRE(ix != nullptr, "index is NULL");
    CIS_REQUIRE(n >= 0 && (n == 0 || ids), "NULL buffer or negative count");
    CIS_REQUIRE(n < ((int64_t)1 << 31), "at most 2^31 - 1 ids per removal call");
    CIS_RM_WRITABLE(ix);
    if (n_removed) *n_removed = 0;
    if (n == 0) return CIS_OK;
    CIS_TRY(cis_index_ready(ix));
    CIS_CHECK_HIP(hipSetDevice(ix->m->device));
    CIS_TRY(ix->wi_in_ids.reserve((size_t)n * sizeof(int64_t)));
    CIS_CHECK_HIP(hipMemcpy(ix->wi_in_ids.p, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
    return index_remove_dev(ix, ix->wi_in_ids.as<int64_t>(), n, n_removed, nullptr, nullptr);
}

extern "C" int cis_index_remove_profile(cis_index* ix, double ms[3]) {
    CIS_REQUIRE(ix != nullptr && ms != nullptr, "NULL argument");
    for (int i = 0; i < 3; ++i) ms[i] = ix->rm_ms[i];
    return CIS_OK;
}

extern "C" int cis_index_sub_remote_counts_dev(cis_index* ix, const int64_t* d_delta, void* stream) {
    CIS_REQUIRE(ix != nullptr && d_delta != nullptr, "NULL argument");
    CIS_RM_WRITABLE(ix);
    return sub_remote_dev(ix, d_delta, (hipStream_t)stream);
}

extern "C" int cis_index_sub_remote_counts(cis_index* ix, const int64_t* delta) {
    CIS_REQUIRE(ix != nullptr && delta != nullptr, "NULL argument");
    CIS_RM_WRITABLE(ix);
    for (int64_t c = 0; c < ix->ncells; ++c) CIS_REQUIRE(delta[c] >= 0, "negative count for cell %lld", (long long)c);
    CIS_TRY(cis_index_ready(ix));
    CIS_CHECK_HIP(hipSetDevice(ix->m->device));
    CIS_TRY(ix->wi_tmp.reserve((size_t)ix->ncells * sizeof(int64_t)));
    CIS_CHECK_HIP(hipMemcpy(ix->wi_tmp.p, delta, (size_t)ix->ncells * sizeof(int64_t), hipMemcpyHostToDevice));
    return sub_remote_dev(ix, ix->wi_tmp.as<int64_t>(), nullptr);
}
