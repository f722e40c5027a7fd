// A device-resident feature store that grows and shrinks by kernels: the HBase `put` / fetch of the reference's features
// (hbase_indexer_minimal.py:779-831) for the exact re-rank of lopq_rerank.hip, addressed by the index's device ids.
//
// A cis_featstore owns a feature matrix [cap_rows][D] (float32 or float64), the row -> id column row_ids [cap_rows], the id -> row
// table keys / rows [cap] (layout, hash, linear probing and -1 = empty of lopq_rerank.hip: row_of_id reads it unchanged) and the live
// row count n.  Rows [0, n) are always dense, so cis_exact_knn_dev and cis_rerank_select_dev read the matrix directly
// (cis_featstore_view).
//
// put(ids, feats) is this loop, whatever the thread timing:
//     for i in range(n):
//         if ids[i] < 0: skipped += 1; continue
//         if ids[i] not in row: row[ids[i]] = len(row); new += 1
//         feats[row[ids[i]]] = batch[i]; row_ids[row[ids[i]]] = ids[i]
// The resolve step claims table slots by CAS and settles first and last occurrence with integer atomics (the second shape of the
// two that were weighed; the other sorts (id, i) pairs): it needs no sort, its scratch is per batch element, and the only per-slot
// word it borrows is the slot's own rows[] entry, which it restores before the call ends.
//   k_fs_claim   thread per element: walks the id's probe chain (past tombstones), claims the first empty slot by CAS or finds the
//                slot that holds the id; slot[i], old[i] = rows[slot] (the id's row, -1: new; nobody writes rows[] in this kernel)
//   k_fs_first   atomicMin(rows[slot], i - nb - 1): all candidates are < -1, so the slot ends with its first occurrence, encoded
//   k_fs_last    first = rows[slot] + nb + 1; atomicMax(last[first], i); flag[i] = (i == first and old[i] < 0): a new id, at the place
//                of its first occurrence; the first occurrence is marked as the id's one writer
//   scan         rank = exclusive scan of flag (dev_scan.h), its total = n_new: new ids take rows n, n + 1, ... in order of first
//                occurrence
//   k_fs_assign  the first occurrence of an id: row = old >= 0 ? old : n + rank; rows[slot] = row (the borrowed word is restored);
//                row_ids[row] = id; copy job (batch row last[i] -> row).  Every other element: no job.
//   k_fs_copy    a wave (row < 4 KB) or a workgroup per job, 16-byte loads and stores with a scalar tail; one writer per row.
//
// remove(ids): with k removed and n' = n - k, the holes are the removed rows below n' ascending, the movers the kept rows at or above
// n' ascending; mover j moves to hole j (feature row, row_ids entry, table entry).  Sources (>= n') and destinations (< n') are
// disjoint: no staging.  Removed ids' slots become tombstones (key = -2; row_of_id walks past them).  O(k D + k log k):
//   k_fs_rm_mark  thread per list entry: finds the id's slot and swaps its key for the tombstone by CAS: of a repeated id exactly one
//                 entry wins.  The winner's row is its sort key, every other entry's key is all ones; k = the number of winners.
//   sort          the project's merge sort (lopq_sort.hip), one segment: S[0 .. k) = the removed rows ascending
//   k_fs_rm_plan  thread per tail row n' + t, t < k: removed rows are found in S by binary search; a kept one is mover
//                 j = t - (removed tail rows below it) and goes to hole S[j]: row_ids, the table entry of its id, a copy job.
//   k_fs_copy     the jobs.
// A stable compaction was weighed and rejected: it moves O(n D) bytes, 16 GB for 1M x 4096 float32.  So after a removal the row order
// is not the insertion order, and whoever breaks exact distance ties by row (cis_exact_knn_dev) sees that.
//
// What a fault would come from is checked on the host before any launch (fs_room): cap_rows >= n + batch, and
// 2 (live + tombstones + batch) <= cap, so every probe chain ends at an empty slot; every probe loop is bounded by cap besides.
// When the first would break the rows grow (new block, copy of [0, n) on the stream, the old block freed after the stream has
// drained); when the second would, the table is rebuilt from row_ids[0 : n) at the next power of two >= 4 (n + batch) by
// cis_idmap_build_dev, which is also what clears the tombstones.
#include <algorithm>

#include "common.h"
#include "dev_scan.h"

int cis_seg_sort_u64(void* temp, size_t* temp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint64_t* vals_in,
                     uint64_t* vals_out, int64_t n, int nseg, const int64_t* seg_begin, const int64_t* seg_end, hipStream_t st);

struct cis_featstore {
    int device = 0;
    int D = 0, f_dtype = 0;
    void* feats = nullptr;        // [cap_rows][D]
    int64_t* row_ids = nullptr;   // [cap_rows]
    int64_t cap_rows = 0, n = 0;
    DevBuf keys, rows;            // [cap] each (the blocks may be larger: a rebuild at a smaller cap keeps them)
    int64_t cap = 0;              // 0: no table yet
    int64_t used = 0;             // live + tombstones: slots whose key is not -1
    int64_t min_cap = 0;          // what cis_featstore_reserve asked for: a rebuild does not go below it
    DevBuf ws;                    // per-call scratch, per batch element
    DevBuf cnt;                   // FS_WORDS counters
    int64_t* h_cnt = nullptr;     // pinned: their read-back
};

namespace {

constexpr int64_t FS_EMPTY = -1, FS_TOMB = -2;
constexpr int64_t FS_MAX_CAP = (int64_t)1 << 36;   // lopq_rerank.hip's IDMAP_MAX_CAP
constexpr int64_t FS_MAX_BATCH = (int64_t)1 << 30;
constexpr int FS_CNT_A = 0, FS_CNT_NEW = 1, FS_CNT_ERR = 2, FS_WORDS = 4;  // A: skipped (put) or removed (remove)
constexpr int FS_WG_ROW_BYTES = 4096;              // a row of this size or more is copied by a workgroup, a smaller one by a wave

// splitmix64's finaliser (as lopq_rerank.hip)
__device__ __forceinline__ uint64_t fs_mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

// slot that holds `id` (>= 0), -1: not stored.  The loop is bounded by cap whatever the table holds.
__device__ __forceinline__ int64_t fs_find(const int64_t* __restrict__ keys, int64_t cap, int64_t id) {
    const uint64_t mask = (uint64_t)cap - 1;
    uint64_t h = fs_mix64((uint64_t)id) & mask;
    for (int64_t p = 0; p < cap; ++p) {
        const int64_t k = keys[h];
        if (k == id) return (int64_t)h;
        if (k == FS_EMPTY) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

// ---- put ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fs_claim(const int64_t* __restrict__ ids, int nb, int64_t* __restrict__ keys,
                                                  const int64_t* __restrict__ rows, int64_t cap, int64_t* __restrict__ slot,
                                                  int64_t* __restrict__ old, int32_t* __restrict__ last, int64_t* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    last[i] = -1;
    const int64_t id = ids[i];
    int64_t s = -1;
    if (id >= 0) {
        const uint64_t mask = (uint64_t)cap - 1;
        uint64_t h = fs_mix64((uint64_t)id) & mask;
        for (int64_t p = 0; p < cap; ++p) {
            const unsigned long long prev = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)FS_EMPTY, (unsigned long long)id);
            if (prev == (unsigned long long)FS_EMPTY || prev == (unsigned long long)id) {
                s = (int64_t)h;
                break;
            }
            h = (h + 1) & mask;
        }
        if (s < 0) atomicAdd((unsigned long long*)&cnt[FS_CNT_ERR], 1ull);  // (a full table: fs_room rules it out)
    } else {
        atomicAdd((unsigned long long*)&cnt[FS_CNT_A], 1ull);
    }
    slot[i] = s;
    old[i] = s >= 0 ? rows[s] : -1;  // an empty slot's row is -1 (k_idmap_init), a stored id's its row; nothing writes rows[] here
}

__global__ __launch_bounds__(256) void k_fs_first(const int64_t* __restrict__ slot, int nb, int64_t* __restrict__ rows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const int64_t s = slot[i];
    if (s >= 0) atomicMin((long long*)&rows[s], (long long)i - nb - 1);
}

__global__ __launch_bounds__(256) void k_fs_last(const int64_t* __restrict__ slot, const int64_t* __restrict__ old, int nb,
                                                 const int64_t* __restrict__ rows, int32_t* __restrict__ last, uint32_t* __restrict__ flag,
                                                 int64_t* __restrict__ job_dst, int64_t* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const int64_t s = slot[i];
    uint32_t f = 0;
    int64_t head = -1;
    if (s >= 0) {
        const int64_t first = rows[s] + nb + 1;
        if (first >= 0 && first < nb) {
            atomicMax(&last[first], i);
            if (first == i) {
                head = 0;
                f = old[i] < 0 ? 1u : 0u;
            }
        } else {
            atomicAdd((unsigned long long*)&cnt[FS_CNT_ERR], 1ull);  // (k_fs_first left every claimed slot in [-nb - 1, -2])
        }
    }
    flag[i] = f;
    job_dst[i] = head;  // 0: the id's first occurrence, which k_fs_assign turns into the id's copy job
}

__global__ __launch_bounds__(256) void k_fs_assign(const int64_t* __restrict__ ids, const int64_t* __restrict__ slot,
                                                   const int64_t* __restrict__ old, const int32_t* __restrict__ last,
                                                   const uint32_t* __restrict__ rank, int nb, int64_t n, int64_t cap_rows,
                                                   int64_t* __restrict__ rows, int64_t* __restrict__ row_ids, int64_t* __restrict__ job_src,
                                                   int64_t* __restrict__ job_dst, int64_t* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const int64_t s = slot[i];
    int64_t src = -1, dst = -1;
    if (s >= 0 && job_dst[i] == 0) {  // the id's first occurrence; nobody else reads or writes this slot's row here
        const int64_t o = old[i];
        const int64_t r = o >= 0 ? o : n + (int64_t)rank[i];
        if (r < cap_rows) {
            rows[s] = r;
            row_ids[r] = ids[i];
            src = last[i];
            dst = r;
        } else {
            atomicAdd((unsigned long long*)&cnt[FS_CNT_ERR], 1ull);  // (fs_room rules it out)
        }
    }
    job_src[i] = src;
    job_dst[i] = dst;
}

// ---- the copy ----------------------------------------------------------------------------------------------------------------------
// Job j: row src[j] of `from` (src == NULL: row j) to row dst[j] of `to` (dst == NULL: row j).  dst[j] < 0: no job.  src[j] < 0: no
// job, or with ZERO the destination row is filled with zeros.  TPR threads per row (64: a wave, 256: the workgroup).  vec: both blocks
// and the row size are multiples of 16 bytes.
template <int TPR, bool ZERO>
__global__ __launch_bounds__(256) void k_fs_copy(const unsigned char* __restrict__ from, unsigned char* __restrict__ to, int64_t row_bytes,
                                                 const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t njobs, int vec) {
    const int64_t j = (int64_t)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
    if (j >= njobs) return;
    const int t = threadIdx.x % TPR;
    const int64_t d = dst ? dst[j] : j;
    const int64_t s = src ? src[j] : j;
    if (d < 0 || (s < 0 && !ZERO)) return;
    unsigned char* __restrict__ o = to + d * row_bytes;
    if (ZERO && s < 0) {
        if (vec) {
            uint4* o4 = reinterpret_cast<uint4*>(o);
            for (int64_t x = t; x < row_bytes / 16; x += TPR) o4[x] = make_uint4(0u, 0u, 0u, 0u);
        } else {
            uint32_t* o1 = reinterpret_cast<uint32_t*>(o);
            for (int64_t x = t; x < row_bytes / 4; x += TPR) o1[x] = 0u;
        }
        return;
    }
    const unsigned char* __restrict__ in = from + s * row_bytes;
    if (vec) {
        const uint4* i4 = reinterpret_cast<const uint4*>(in);
        uint4* o4 = reinterpret_cast<uint4*>(o);
        const int64_t nv = row_bytes / 16;
        int64_t x = t;
        for (; x + 3 * TPR < nv; x += 4 * TPR) {  // four loads in flight per lane
            const uint4 a = i4[x], b = i4[x + TPR], c = i4[x + 2 * TPR], e = i4[x + 3 * TPR];
            o4[x] = a; o4[x + TPR] = b; o4[x + 2 * TPR] = c; o4[x + 3 * TPR] = e;
        }
        for (; x < nv; x += TPR) o4[x] = i4[x];
    } else {  // rows are multiples of 4 bytes (float32 / float64): 16-byte pieces from the first aligned address, scalar head and tail
        const uint32_t* i1 = reinterpret_cast<const uint32_t*>(in);
        uint32_t* o1 = reinterpret_cast<uint32_t*>(o);
        const int64_t nw = row_bytes / 4;
        const bool same = (((uintptr_t)in ^ (uintptr_t)o) & 15) == 0;
        int64_t head = same ? (int64_t)(((16 - ((uintptr_t)in & 15)) & 15) / 4) : nw;
        if (head > nw) head = nw;
        for (int64_t x = t; x < head; x += TPR) o1[x] = i1[x];
        if (same) {
            const int64_t nv = (nw - head) / 4;
            const uint4* i4 = reinterpret_cast<const uint4*>(i1 + head);
            uint4* o4 = reinterpret_cast<uint4*>(o1 + head);
            for (int64_t x = t; x < nv; x += TPR) o4[x] = i4[x];
            for (int64_t x = head + nv * 4 + t; x < nw; x += TPR) o1[x] = i1[x];
        }
    }
}

// ---- remove ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fs_rm_mark(const int64_t* __restrict__ ids, int nb, int64_t* __restrict__ keys,
                                                    int64_t* __restrict__ rows, int64_t cap, int64_t n, uint64_t* __restrict__ skey,
                                                    int64_t* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb) return;
    const int64_t id = ids[i];
    uint64_t key = ~0ull;
    if (id >= 0) {
        const int64_t s = fs_find(keys, cap, id);
        if (s >= 0 &&
            atomicCAS((unsigned long long*)&keys[s], (unsigned long long)id, (unsigned long long)FS_TOMB) == (unsigned long long)id) {
            const int64_t r = rows[s];  // (this thread alone owns the slot now)
            rows[s] = -1;
            if (r >= 0 && r < n) {
                key = (uint64_t)r;
                atomicAdd((unsigned long long*)&cnt[FS_CNT_A], 1ull);
            } else {
                atomicAdd((unsigned long long*)&cnt[FS_CNT_ERR], 1ull);  // (a table entry without a row: never written)
            }
        }
    }
    skey[i] = key;
}

__global__ void k_fs_seg(int64_t* __restrict__ seg, int64_t nb) {
    seg[0] = 0;
    seg[1] = nb;
}

// S[0 .. k): the removed rows ascending.  Thread t < k looks at tail row n' + t.
__global__ __launch_bounds__(256) void k_fs_rm_plan(const uint64_t* __restrict__ S, int nb, int64_t n, const int64_t* __restrict__ keys,
                                                    int64_t* __restrict__ rows, int64_t cap, int64_t* __restrict__ row_ids,
                                                    int64_t* __restrict__ job_src, int64_t* __restrict__ job_dst, int64_t* __restrict__ cnt) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nb) return;
    const int64_t k = cnt[FS_CNT_A];
    int64_t src = -1, dst = -1;
    if (t < k && k <= nb && k <= n) {
        const int64_t n2 = n - k, r = n2 + t;
        // lower bounds in S[0 .. k): of n' (the number of holes) and of r
        int64_t lo = 0, hi = k;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (S[mid] < (uint64_t)n2) lo = mid + 1;
            else hi = mid;
        }
        const int64_t holes = lo;
        hi = k;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (S[mid] < (uint64_t)r) lo = mid + 1;
            else hi = mid;
        }
        const bool removed = lo < k && S[lo] == (uint64_t)r;
        if (!removed) {
            const int64_t j = t - (lo - holes);  // the kept tail rows below r
            const int64_t hole = j >= 0 && j < holes ? (int64_t)S[j] : -1;
            const int64_t id = row_ids[r];
            const int64_t s = id >= 0 ? fs_find(keys, cap, id) : -1;
            if (hole >= 0 && hole < n2 && s >= 0) {
                rows[s] = hole;
                row_ids[hole] = id;  // (row_ids[r], r >= n', is read; row_ids[hole], hole < n', is written: disjoint)
                src = r;
                dst = hole;
            } else {
                atomicAdd((unsigned long long*)&cnt[FS_CNT_ERR], 1ull);  // (as many movers as holes, every live row in the table)
            }
        }
    }
    job_src[t] = src;
    job_dst[t] = dst;
}

inline unsigned grid_for(int64_t n, int t) { return (unsigned)(n > 0 ? ceil_div(n, t) : 1); }

int64_t pow2_at_least(int64_t x) {
    int64_t c = 64;
    while (c < x) c <<= 1;
    return c;
}

template <bool ZERO>
void launch_copy(const void* from, void* to, int64_t row_bytes, const int64_t* src, const int64_t* dst, int64_t njobs, hipStream_t st) {
    if (njobs <= 0) return;
    const int vec = (row_bytes % 16 == 0 && ((uintptr_t)from & 15) == 0 && ((uintptr_t)to & 15) == 0) ? 1 : 0;
    if (row_bytes >= FS_WG_ROW_BYTES)
        hipLaunchKernelGGL((k_fs_copy<256, ZERO>), dim3((unsigned)njobs), dim3(256), 0, st, (const unsigned char*)from, (unsigned char*)to, row_bytes,
                           src, dst, njobs, vec);
    else
        hipLaunchKernelGGL((k_fs_copy<64, ZERO>), dim3(grid_for(njobs, 4)), dim3(256), 0, st, (const unsigned char*)from, (unsigned char*)to, row_bytes,
                           src, dst, njobs, vec);
}

int counted_malloc(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        cis_set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        *p = nullptr;
        return CIS_ENOMEM;
    }
    __atomic_add_fetch(&g_cis_allocs, 1, __ATOMIC_RELAXED);
    __atomic_add_fetch(&g_cis_alloc_bytes, (long long)bytes, __ATOMIC_RELAXED);
    return CIS_OK;
}

// Rows: room for `need` rows.  The live rows move on the stream; the old blocks go after the stream has drained.
int fs_grow_rows(cis_featstore* fs, int64_t need, hipStream_t st) {
    if (need <= fs->cap_rows) return CIS_OK;
    const int64_t cap = std::max<int64_t>(need, 2 * fs->cap_rows);
    const size_t row_bytes = (size_t)fs->D * (size_t)fs->f_dtype;
    void* nf = nullptr;
    void* ni = nullptr;
    CIS_TRY(counted_malloc(&nf, (size_t)cap * row_bytes + 16));
    if (counted_malloc(&ni, (size_t)cap * sizeof(int64_t)) != CIS_OK) {
        (void)hipFree(nf);
        return CIS_ENOMEM;
    }
    if (fs->n > 0) {
        CIS_CHECK_HIP(hipMemcpyAsync(nf, fs->feats, (size_t)fs->n * row_bytes, hipMemcpyDeviceToDevice, st));
        CIS_CHECK_HIP(hipMemcpyAsync(ni, fs->row_ids, (size_t)fs->n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    }
    CIS_CHECK_HIP(hipStreamSynchronize(st));
    if (fs->feats) (void)hipFree(fs->feats);
    if (fs->row_ids) (void)hipFree(fs->row_ids);
    fs->feats = nf;
    fs->row_ids = (int64_t*)ni;
    fs->cap_rows = cap;
    return CIS_OK;
}

// Table: rebuilt from row_ids[0 : n) at `cap` slots (a power of two >= 2 n); clears the tombstones.
int fs_rebuild_table(cis_featstore* fs, int64_t cap, hipStream_t st) {
    CIS_REQUIRE(cap <= FS_MAX_CAP, "the feature store's id table would need more than 2^36 slots");
    if ((size_t)cap * sizeof(int64_t) > fs->keys.cap || (size_t)cap * sizeof(int64_t) > fs->rows.cap) {
        CIS_CHECK_HIP(hipStreamSynchronize(st));  // (DevBuf frees the old block at once)
        CIS_TRY(fs->keys.reserve((size_t)cap * sizeof(int64_t)));
        CIS_TRY(fs->rows.reserve((size_t)cap * sizeof(int64_t)));
    }
    CIS_TRY(cis_idmap_build_dev(fs->row_ids, fs->n, fs->keys.as<int64_t>(), fs->rows.as<int64_t>(), cap, st));
    fs->cap = cap;
    fs->used = fs->n;
    return CIS_OK;
}

// The two invariants a put of `batch` more ids needs, established before anything is launched
int fs_room(cis_featstore* fs, int64_t batch, hipStream_t st) {
    CIS_TRY(fs_grow_rows(fs, fs->n + batch, st));
    if (fs->cap == 0 || 2 * (fs->used + batch) > fs->cap)
        CIS_TRY(fs_rebuild_table(fs, std::max(pow2_at_least(4 * (fs->n + batch)), fs->min_cap), st));
    CIS_REQUIRE(fs->cap_rows >= fs->n + batch && 2 * (fs->used + batch) <= fs->cap, "feature store: capacity invariant broken");
    return CIS_OK;
}

// the counters of the call: the one host round trip of put and of remove
int fs_read_counters(cis_featstore* fs, hipStream_t st) {
    CIS_CHECK_HIP(hipMemcpyAsync(fs->h_cnt, fs->cnt.p, FS_WORDS * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    CIS_CHECK_HIP(hipStreamSynchronize(st));
    CIS_REQUIRE(fs->h_cnt[FS_CNT_ERR] == 0, "feature store: the id table and the rows disagree (%lld entries)", (long long)fs->h_cnt[FS_CNT_ERR]);
    return CIS_OK;
}

// scratch of a call over nb elements, carved from fs->ws (8-byte words first)
struct FsScratch {
    int64_t *slot, *old, *job_src, *job_dst, *seg;
    uint64_t *skey, *sorted, *svals;
    int32_t* last;
    uint32_t *flag, *rank, *sums;
    void* sort_tmp;
    size_t sort_bytes;
};

int fs_scratch(cis_featstore* fs, int64_t nb, FsScratch* s) {
    size_t sort_bytes = 0;
    CIS_TRY(cis_seg_sort_u64(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, nb, 1, nullptr, nullptr, nullptr));
    sort_bytes = (sort_bytes + 15) & ~(size_t)15;
    const size_t w = (size_t)nb;
    const size_t n_sums = (size_t)ceil_div(nb, SCAN_TILE) + 2;
    const size_t bytes = 7 * w * 8 + 16 + sort_bytes + 3 * w * 4 + n_sums * 4 + 64;
    CIS_TRY(fs->ws.reserve(bytes));
    unsigned char* p = fs->ws.as<unsigned char>();
    s->slot = (int64_t*)p; p += w * 8;
    s->old = (int64_t*)p; p += w * 8;
    s->job_src = (int64_t*)p; p += w * 8;
    s->job_dst = (int64_t*)p; p += w * 8;
    s->skey = (uint64_t*)p; p += w * 8;
    s->sorted = (uint64_t*)p; p += w * 8;
    s->svals = (uint64_t*)p; p += w * 8;
    s->seg = (int64_t*)p; p += 16;
    s->sort_tmp = p; p += sort_bytes;
    s->sort_bytes = sort_bytes;
    s->last = (int32_t*)p; p += w * 4;
    s->flag = (uint32_t*)p; p += w * 4;
    s->rank = (uint32_t*)p; p += w * 4;
    s->sums = (uint32_t*)p;
    return CIS_OK;
}

int fs_ready(cis_featstore* fs) {
    CIS_REQUIRE(fs != nullptr, "feature store is NULL");
    CIS_TRY(cis_lazy_init());
    CIS_CHECK_HIP(hipSetDevice(fs->device));
    return CIS_OK;
}

}  // namespace

extern "C" int cis_featstore_create(cis_featstore** out, int D, int f_dtype, int64_t reserve_rows) {
    CIS_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    CIS_REQUIRE(D > 0 && D <= (1 << 24), "the feature width must be in [1, 2^24] (D = %d)", D);
    CIS_REQUIRE(f_dtype == CIS_F32 || f_dtype == CIS_F64, "f_dtype must be 4 or 8");
    CIS_REQUIRE(reserve_rows >= 0 && reserve_rows <= FS_MAX_CAP / 8, "bad reserve_rows");
    CIS_TRY(cis_lazy_init());
    cis_featstore* fs = new cis_featstore();
    fs->device = cis_current_device();
    fs->D = D;
    fs->f_dtype = f_dtype;
    int rc = CIS_OK;
    if (hipSetDevice(fs->device) != hipSuccess || hipHostMalloc((void**)&fs->h_cnt, FS_WORDS * sizeof(int64_t)) != hipSuccess) {
        cis_set_error("feature store: no pinned block for the counters");
        fs->h_cnt = nullptr;
        rc = CIS_EHIP;
    }
    if (rc == CIS_OK) rc = fs->cnt.reserve(FS_WORDS * sizeof(int64_t));
    if (rc == CIS_OK) rc = cis_featstore_reserve(fs, reserve_rows, nullptr);
    // (the empty table was filled on the null stream; the caller's streams may be non-blocking)
    if (rc == CIS_OK && hipStreamSynchronize(nullptr) != hipSuccess) { cis_set_error("feature store: the first table build failed"); rc = CIS_EHIP; }
    if (rc != CIS_OK) {
        cis_featstore_destroy(fs);
        return rc;
    }
    *out = fs;
    return CIS_OK;
}

extern "C" void cis_featstore_destroy(cis_featstore* fs) {
    if (!fs) return;
    (void)hipSetDevice(fs->device);
    (void)hipDeviceSynchronize();
    if (fs->feats) (void)hipFree(fs->feats);
    if (fs->row_ids) (void)hipFree(fs->row_ids);
    fs->keys.release();
    fs->rows.release();
    fs->ws.release();
    fs->cnt.release();
    if (fs->h_cnt) (void)hipHostFree(fs->h_cnt);
    delete fs;
}

extern "C" int64_t cis_featstore_size(cis_featstore* fs) { return fs ? fs->n : -1; }

extern "C" int cis_featstore_reserve(cis_featstore* fs, int64_t rows, void* stream) {
    CIS_REQUIRE(rows >= 0 && rows <= FS_MAX_CAP / 8, "bad row count");
    CIS_TRY(fs_ready(fs));
    hipStream_t st = (hipStream_t)stream;
    // the table, always (an empty store answers look-ups too): at 4 x rows it takes `rows` ids and as many tombstones before a rebuild
    const int64_t cap = pow2_at_least(4 * std::max<int64_t>(rows, fs->n));
    if (cap > fs->min_cap) fs->min_cap = cap;
    if (fs->cap < fs->min_cap) CIS_TRY(fs_rebuild_table(fs, fs->min_cap, st));
    CIS_TRY(fs_grow_rows(fs, rows, st));
    return CIS_OK;
}

extern "C" int cis_featstore_put_dev(cis_featstore* fs, const int64_t* d_ids, const void* d_feats, int64_t n, int64_t* n_new,
                                     int64_t* n_skipped, void* stream) {
    CIS_REQUIRE(fs != nullptr, "feature store is NULL");
    CIS_REQUIRE(n >= 0 && (n == 0 || (d_ids && d_feats)), "NULL buffer or negative count");
    CIS_REQUIRE(n <= FS_MAX_BATCH, "at most 2^30 rows per put");
    if (n_new) *n_new = 0;
    if (n_skipped) *n_skipped = 0;
    if (n == 0) return CIS_OK;
    CIS_TRY(fs_ready(fs));
    hipStream_t st = (hipStream_t)stream;
    CIS_TRY(fs_room(fs, n, st));
    FsScratch s;
    CIS_TRY(fs_scratch(fs, n, &s));
    const int nb = (int)n;
    int64_t* cnt = fs->cnt.as<int64_t>();
    int64_t* keys = fs->keys.as<int64_t>();
    int64_t* rows = fs->rows.as<int64_t>();
    const dim3 g(grid_for(n, 256)), b(256);
    CIS_CHECK_HIP(hipMemsetAsync(cnt, 0, FS_WORDS * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_fs_claim, g, b, 0, st, d_ids, nb, keys, (const int64_t*)rows, fs->cap, s.slot, s.old, s.last, cnt);
    hipLaunchKernelGGL(k_fs_first, g, b, 0, st, (const int64_t*)s.slot, nb, rows);
    hipLaunchKernelGGL(k_fs_last, g, b, 0, st, (const int64_t*)s.slot, (const int64_t*)s.old, nb, (const int64_t*)rows, s.last, s.flag, s.job_dst,
                       cnt);
    dev_exclusive_scan<uint32_t, uint32_t>(s.flag, s.rank, n, s.sums, nullptr, cnt + FS_CNT_NEW, st);
    hipLaunchKernelGGL(k_fs_assign, g, b, 0, st, d_ids, (const int64_t*)s.slot, (const int64_t*)s.old, (const int32_t*)s.last,
                       (const uint32_t*)s.rank, nb, fs->n, fs->cap_rows, rows, fs->row_ids, s.job_src, s.job_dst, cnt);
    launch_copy<false>(d_feats, fs->feats, (int64_t)fs->D * fs->f_dtype, s.job_src, s.job_dst, n, st);
    CIS_CHECK_HIP(hipGetLastError());
    CIS_TRY(fs_read_counters(fs, st));
    const int64_t added = fs->h_cnt[FS_CNT_NEW];
    fs->n += added;
    fs->used += added;
    if (n_new) *n_new = added;
    if (n_skipped) *n_skipped = fs->h_cnt[FS_CNT_A];
    return CIS_OK;
}

extern "C" int cis_featstore_remove_dev(cis_featstore* fs, const int64_t* d_ids, int64_t n, int64_t* n_removed, void* stream) {
    CIS_REQUIRE(fs != nullptr, "feature store is NULL");
    CIS_REQUIRE(n >= 0 && (n == 0 || d_ids), "NULL buffer or negative count");
    CIS_REQUIRE(n <= FS_MAX_BATCH, "at most 2^30 ids per removal");
    if (n_removed) *n_removed = 0;
    if (n == 0 || fs->n == 0 || fs->cap == 0) return CIS_OK;
    CIS_TRY(fs_ready(fs));
    hipStream_t st = (hipStream_t)stream;
    FsScratch s;
    CIS_TRY(fs_scratch(fs, n, &s));
    const int nb = (int)n;
    int64_t* cnt = fs->cnt.as<int64_t>();
    int64_t* keys = fs->keys.as<int64_t>();
    int64_t* rows = fs->rows.as<int64_t>();
    const dim3 g(grid_for(n, 256)), b(256);
    CIS_CHECK_HIP(hipMemsetAsync(cnt, 0, FS_WORDS * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_fs_rm_mark, g, b, 0, st, d_ids, nb, keys, rows, fs->cap, fs->n, s.skey, cnt);
    hipLaunchKernelGGL(k_fs_seg, dim3(1), dim3(1), 0, st, s.seg, n);
    size_t sort_bytes = s.sort_bytes;
    CIS_TRY(cis_seg_sort_u64(s.sort_tmp, &sort_bytes, s.skey, s.sorted, s.skey, s.svals, n, 1, s.seg, s.seg + 1, st));
    hipLaunchKernelGGL(k_fs_rm_plan, g, b, 0, st, (const uint64_t*)s.sorted, nb, fs->n, (const int64_t*)keys, rows, fs->cap, fs->row_ids, s.job_src,
                       s.job_dst, cnt);
    launch_copy<false>(fs->feats, fs->feats, (int64_t)fs->D * fs->f_dtype, s.job_src, s.job_dst, n, st);
    CIS_CHECK_HIP(hipGetLastError());
    CIS_TRY(fs_read_counters(fs, st));
    const int64_t k = fs->h_cnt[FS_CNT_A];
    fs->n -= k;  // (used stays: the k slots are tombstones until the next rebuild)
    if (n_removed) *n_removed = k;
    return CIS_OK;
}

extern "C" int cis_featstore_get_dev(cis_featstore* fs, const int64_t* d_ids, int64_t m, void* d_out_feats, int64_t* d_out_rows,
                                     void* stream) {
    CIS_REQUIRE(fs != nullptr, "feature store is NULL");
    CIS_REQUIRE(m >= 0 && (m == 0 || (d_ids && d_out_feats)), "NULL buffer or negative count");
    CIS_REQUIRE(m <= FS_MAX_BATCH, "at most 2^30 ids per call");
    if (m == 0) return CIS_OK;
    CIS_TRY(fs_ready(fs));
    hipStream_t st = (hipStream_t)stream;
    int64_t* out_rows = d_out_rows;
    if (!out_rows) {
        FsScratch s;
        CIS_TRY(fs_scratch(fs, m, &s));
        out_rows = s.job_src;
    }
    CIS_REQUIRE(fs->cap > 0, "feature store: no id table");  // (cis_featstore_create builds one)
    CIS_TRY(cis_idmap_lookup_dev(fs->keys.as<int64_t>(), fs->rows.as<int64_t>(), fs->cap, fs->n, d_ids, m, out_rows, st));
    launch_copy<true>(fs->feats, d_out_feats, (int64_t)fs->D * fs->f_dtype, out_rows, nullptr, m, st);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_featstore_rows_dev(cis_featstore* fs, int64_t first, int64_t count, void* d_out_feats, int64_t* d_out_ids, void* stream) {
    CIS_REQUIRE(fs != nullptr, "feature store is NULL");
    CIS_REQUIRE(first >= 0 && count >= 0 && first <= fs->n && count <= fs->n - first, "the rows [%lld, %lld + %lld) are not all in the store (n = %lld)",
                (long long)first, (long long)first, (long long)count, (long long)fs->n);
    if (count == 0) return CIS_OK;
    CIS_TRY(fs_ready(fs));
    const size_t row_bytes = (size_t)fs->D * (size_t)fs->f_dtype;
    if (d_out_feats)
        CIS_CHECK_HIP(hipMemcpyAsync(d_out_feats, (const unsigned char*)fs->feats + (size_t)first * row_bytes, (size_t)count * row_bytes,
                                     hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (d_out_ids)
        CIS_CHECK_HIP(hipMemcpyAsync(d_out_ids, fs->row_ids + first, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CIS_OK;
}

extern "C" int cis_featstore_view(cis_featstore* fs, const void** d_feats, const int64_t** d_row_ids, const int64_t** d_keys,
                                  const int64_t** d_rows, int64_t* cap, int64_t* n) {
    CIS_REQUIRE(fs != nullptr, "feature store is NULL");
    if (d_feats) *d_feats = fs->feats;
    if (d_row_ids) *d_row_ids = fs->row_ids;
    if (d_keys) *d_keys = fs->keys.as<int64_t>();
    if (d_rows) *d_rows = fs->rows.as<int64_t>();
    if (cap) *cap = fs->cap;
    if (n) *n = fs->n;
    return CIS_OK;
}
