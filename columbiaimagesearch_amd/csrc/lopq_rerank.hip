// Exact re-ranking of search results without the host (searcher_lopqhbase.py:849-912 and :964-1017): a device id -> feature row
// map (open addressing in HBM, built by kernels from an id column that is already there) and one fused kernel per batch that
// looks up the rows of the first `nb` results of every query, measures the true L2 distance to their resident features, applies
// the near-duplicate threshold and the max_returned cut, and ranks what is left.
//
// The distance is the value of k_rerank (csrc/lopq_exchange.hip) bit for bit: lane l of one wave accumulates elements l, l+64, ...
// in ascending order with fma(df, df, acc) in the features' dtype, the same __shfl_xor butterfly (32 ... 1) folds the lanes, and the
// result is (double)(T)sqrt(acc).  Several rows are in flight per wave, each with its own accumulator, which does not change a sum.
//
// On the cell-sharded index the same steps run where the data is: k_rerank_packed measures a rank's own hits
// before the exchange (the same distance loop), k_rerank_select_merged ranks the merged list on the home rank (the same keep / rank /
// write) with the distances it finds through the merge's src_rec.
#include "common.h"

namespace {

constexpr int RR_MAX_NB = 1024;         // results per query the ranking holds in LDS (4 per thread)
constexpr int RR_ROWS = 8;              // feature rows in flight per wave (8 rows x 2 elements each: profiles/rerank_rows_in_flight_ab.txt)
constexpr int RR_STAGE_BYTES = 32768;   // a query row up to this size is staged in LDS
constexpr int64_t IDMAP_EMPTY = -1;
constexpr int64_t IDMAP_MAX_CAP = (int64_t)1 << 36;

// splitmix64's finaliser: device ids are small integers or 2^62 + slot, so the low bits alone would put whole runs on one chain
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return x;
}

__global__ __launch_bounds__(256) void k_idmap_init(int64_t* __restrict__ keys, int64_t* __restrict__ rows, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    keys[i] = IDMAP_EMPTY;
    rows[i] = -1;
}

// One thread per id: claims the first empty slot of its probe chain (or finds the slot that already holds the id) and raises the
// slot's row to its own, so a repeated id maps to its last row like {k: i for i, k in enumerate(ids)}.  cap >= 2 n: a chain always
// ends at an empty slot, and the loop is bounded by cap whatever the table holds.
__global__ __launch_bounds__(256) void k_idmap_insert(const int64_t* __restrict__ ids, int64_t n, int64_t* __restrict__ keys,
                                                      int64_t* __restrict__ rows, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    if (id < 0) return;
    const uint64_t mask = (uint64_t)cap - 1;
    uint64_t h = mix64((uint64_t)id) & mask;
    for (int64_t p = 0; p < cap; ++p) {
        const unsigned long long prev = atomicCAS((unsigned long long*)&keys[h], (unsigned long long)IDMAP_EMPTY, (unsigned long long)id);
        if (prev == (unsigned long long)IDMAP_EMPTY || prev == (unsigned long long)id) {
            atomicMax((long long*)&rows[h], (long long)i);
            return;
        }
        h = (h + 1) & mask;
    }
}

// Row of `id`: through the table, or (keys == NULL) the id itself when it names a row.  -1: unknown or negative.
__device__ __forceinline__ int64_t row_of_id(const int64_t* __restrict__ keys, const int64_t* __restrict__ rows, int64_t cap,
                                             int64_t n_feats, int64_t id) {
    if (id < 0) return -1;
    if (!keys) return id < n_feats ? id : -1;
    const uint64_t mask = (uint64_t)cap - 1;
    uint64_t h = mix64((uint64_t)id) & mask;
    for (int64_t p = 0; p < cap; ++p) {
        const int64_t k = keys[h];
        if (k == id) {
            const int64_t r = rows[h];
            return r < n_feats ? r : -1;
        }
        if (k == IDMAP_EMPTY) return -1;
        h = (h + 1) & mask;
    }
    return -1;
}

__global__ __launch_bounds__(256) void k_idmap_lookup(const int64_t* __restrict__ keys, const int64_t* __restrict__ rows, int64_t cap,
                                                      int64_t n_feats, const int64_t* __restrict__ ids, int64_t m,
                                                      int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    out[i] = row_of_id(keys, rows, cap, n_feats, ids[i]);
}

// Sort key of a distance: ascending as unsigned, -0 == +0, every NaN behind every number (np.argsort's order), and all ones for
// an entry that is not kept.
__device__ __forceinline__ uint64_t rank_key(double d) {
    if (d != d) return 0xfffffffffffffffeULL;
    const uint64_t b = (uint64_t)__double_as_longlong(d + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

// Distances of the results listed in s_work (their feature rows in s_row): one row per wave at a time, RR_ROWS rows in flight (a
// short last group repeats its first row and drops the copy).  Lane 0 hands store(result, folded sum) each result once.
template <typename T, bool STAGED, typename Store>
__device__ __forceinline__ void measure_rows(const T* __restrict__ feats, int D, const T* __restrict__ qg, const T* s_q,
                                             const uint64_t* s_row, const int* s_work, int nwork, int lane, int wave, Store store) {
    for (int t0 = wave; t0 < nwork; t0 += 4 * RR_ROWS) {
        int res[RR_ROWS];
        const T* x[RR_ROWS];
        T acc[RR_ROWS];
#pragma unroll
        for (int r = 0; r < RR_ROWS; ++r) {
            const int t = t0 + 4 * r;
            res[r] = t < nwork ? s_work[t] : -1;
            x[r] = feats + (int64_t)s_row[res[r] >= 0 ? res[r] : s_work[t0]] * D;
            acc[r] = (T)0;
        }
#pragma unroll 2
        for (int i = lane; i < D; i += 64) {
            const T qv = STAGED ? s_q[i] : qg[i];
#pragma unroll
            for (int r = 0; r < RR_ROWS; ++r) {
                const T df = qv - x[r][i];
                acc[r] = fma(df, df, acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < RR_ROWS; ++r) {
            T s = acc[r];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
            if (lane == 0 && res[r] >= 0) store(res[r], s);
        }
    }
}

// What is ranked and written: the kept results of the first nb (ids in my_id, 4 per thread; distances in s_d), by (distance, place).
struct SelectOut {
    int64_t* out_ids;
    double* out_dists;
    int32_t* out_src;
    int32_t* n_kept;
    double th;
    int nb, max_returned, use_th;
};

// The end of a re-rank for query q, after a barrier behind the last write of s_d (s_nkept zeroed before it): keep, rank, write.
__device__ __forceinline__ void keep_rank_write(const SelectOut& a, int64_t q, const int64_t (&my_id)[RR_MAX_NB / 256], const double* s_d,
                                                uint64_t* s_u, int* s_nkept, int tid) {
    const int nb = a.nb;
    // keep: a result, in front of max_returned (its place BEFORE the re-order), not above the threshold
    double my_d[RR_MAX_NB / 256];
    uint64_t my_key[RR_MAX_NB / 256];
#pragma unroll
    for (int k = 0; k < RR_MAX_NB / 256; ++k) {
        const int i = tid + 256 * k;
        my_key[k] = ~0ULL;
        my_d[k] = 0.0;
        if (i < nb) {
            const double d = s_d[i];
            const bool keep = my_id[k] >= 0 && (a.max_returned == 0 || i < a.max_returned) && (!a.use_th || d <= a.th);
            if (keep) {
                my_key[k] = rank_key(d);
                atomicAdd(s_nkept, 1);
            }
            my_d[k] = d;
            s_u[i] = my_key[k];
        }
    }
    __syncthreads();

    // rank by counting on (key, i): a stable sort; what is not kept lands behind the kept ones and becomes the padding
    int rank[RR_MAX_NB / 256] = {0, 0, 0, 0};
    for (int j = 0; j < nb; ++j) {
        const uint64_t kj = s_u[j];
#pragma unroll
        for (int k = 0; k < RR_MAX_NB / 256; ++k) rank[k] += (kj < my_key[k] || (kj == my_key[k] && j < tid + 256 * k)) ? 1 : 0;
    }
    int64_t* __restrict__ o_ids = a.out_ids + q * nb;
    double* __restrict__ o_d = a.out_dists + q * nb;
    int32_t* __restrict__ o_src = a.out_src + q * nb;
#pragma unroll
    for (int k = 0; k < RR_MAX_NB / 256; ++k) {
        const int i = tid + 256 * k;
        if (i < nb) {
            const bool keep = my_key[k] != ~0ULL;
            o_ids[rank[k]] = keep ? my_id[k] : -1;
            o_d[rank[k]] = keep ? my_d[k] : __longlong_as_double(0x7ff8000000000000LL);
            o_src[rank[k]] = keep ? i : -1;
        }
    }
    if (tid == 0) a.n_kept[q] = *s_nkept;
}

struct RerankArgs {
    const void* feats;
    int64_t n_feats;
    const int64_t* map_keys;
    const int64_t* map_rows;
    int64_t map_cap;
    const void* Q;
    const int64_t* ids;
    const double* adc;
    SelectOut o;
    int D, L;
};

// One workgroup (4 waves) per query.  STAGED: the query row sits in dynamic LDS.
template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void k_rerank_select(const RerankArgs a) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ uint64_t s_u[RR_MAX_NB];   // the feature row of result i, later its sort key
    __shared__ double s_d[RR_MAX_NB];     // the distance result i is ranked by
    __shared__ int s_work[RR_MAX_NB];     // results whose feature is resident (any order)
    __shared__ int s_nwork, s_nkept;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int D = a.D, nb = a.o.nb;
    const T* __restrict__ feats = (const T*)a.feats;
    const T* __restrict__ qg = (const T*)a.Q + q * D;
    const int64_t* __restrict__ ids = a.ids + q * a.L;
    const double* __restrict__ adc = a.adc + q * a.L;
    T* s_q = (T*)s_dyn;

    if (tid == 0) { s_nwork = 0; s_nkept = 0; }
    if (STAGED)
        for (int i = tid; i < D; i += 256) s_q[i] = qg[i];
    __syncthreads();

    // 1. rows of the results, one result per thread; a result without a resident feature is ranked by its ADC distance
    int64_t my_id[RR_MAX_NB / 256];
#pragma unroll
    for (int k = 0; k < RR_MAX_NB / 256; ++k) {
        const int i = tid + 256 * k;
        my_id[k] = -1;
        if (i < nb) {
            const int64_t id = ids[i];
            my_id[k] = id;
            const int64_t r = row_of_id(a.map_keys, a.map_rows, a.map_cap, a.n_feats, id);
            s_u[i] = (uint64_t)r;
            if (r >= 0)
                s_work[atomicAdd(&s_nwork, 1)] = i;
            else
                s_d[i] = id >= 0 ? adc[i] : 0.0;
        }
    }
    __syncthreads();

    // 2. distances
    measure_rows<T, STAGED>(feats, D, qg, s_q, s_u, s_work, s_nwork, lane, wave, [&](int i, T s) {
        const double d = (double)(T)sqrt(s);
        s_d[i] = d != d ? adc[i] : d;  // a NaN feature: the host path keeps the ADC distance too
    });
    __syncthreads();

    // 3. keep, 4. rank and write
    keep_rank_write(a.o, q, my_id, s_d, s_u, &s_nkept, tid);
}

// ---- the re-rank of the cell-sharded index (distributed.py): a rank measures its own hits before the exchange
struct PackedArgs {
    const void* feats;
    int64_t n_feats;
    const int64_t* map_keys;
    const int64_t* map_rows;
    int64_t map_cap;
    const void* Q;
    const cis_hit* recs;
    const int64_t* off;
    const int32_t* cnt;
    int64_t n_rec;
    double* true_d;
    int D, nb;
};

// One workgroup per list: record i of list q (recs[off[q] + i], i < cnt[q]) gets true_d[off[q] + i] = its distance to query row q
// when i < nb and its feature is resident, NaN otherwise.  The lists of the packed exchange and the rows of the dense [rows][L]
// layout (off = row L) look alike from here.  A list that does not lie inside [0, n_rec) is left alone.
template <typename T, bool STAGED>
__global__ __launch_bounds__(256) void k_rerank_packed(const PackedArgs a) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ uint64_t s_u[RR_MAX_NB];   // the feature row of record i
    __shared__ int s_work[RR_MAX_NB];     // records whose feature is resident (any order)
    __shared__ int s_nwork;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int c = a.cnt[q];
    const int64_t o = a.off[q];
    if (c <= 0 || o < 0 || o + c > a.n_rec) return;  // (the same for every thread of the workgroup)
    const int D = a.D;
    const int n = c < a.nb ? c : a.nb;
    const T* __restrict__ feats = (const T*)a.feats;
    const T* __restrict__ qg = (const T*)a.Q + q * D;
    const cis_hit* __restrict__ recs = a.recs + o;
    double* __restrict__ true_d = a.true_d + o;
    T* s_q = (T*)s_dyn;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    if (tid == 0) s_nwork = 0;
    if (STAGED && n > 0) {
        const size_t bytes = (size_t)D * sizeof(T);
        if ((((uintptr_t)qg | bytes) & 15) == 0) {  // 16 bytes per lane where the row allows it
            const uint4* __restrict__ src = (const uint4*)qg;
            uint4* dst = (uint4*)s_dyn;
            for (int i = tid; i < (int)(bytes >> 4); i += 256) dst[i] = src[i];
        } else {
            for (int i = tid; i < D; i += 256) s_q[i] = qg[i];
        }
    }
    __syncthreads();

    for (int i = tid; i < c; i += 256) {
        int64_t r = -1;
        if (i < n) {
            r = row_of_id(a.map_keys, a.map_rows, a.map_cap, a.n_feats, recs[i].id);
            s_u[i] = (uint64_t)r;
        }
        if (r >= 0)
            s_work[atomicAdd(&s_nwork, 1)] = i;
        else
            true_d[i] = nan;
    }
    __syncthreads();

    measure_rows<T, STAGED>(feats, D, qg, s_q, s_u, s_work, s_nwork, lane, wave, [&](int i, T s) { true_d[i] = (double)(T)sqrt(s); });
}

struct SelectMergedArgs {
    const int64_t* ids;
    const double* adc;
    const int64_t* src_rec;
    const double* true_d;
    int64_t n_true;
    SelectOut o;
    int L;
};

// k_rerank_select's keep / rank / write on a merged list whose distances were measured by the shards: d = true_d[src_rec], the ADC
// distance where that is NaN (or there is no record).  One workgroup per query.
__global__ __launch_bounds__(256) void k_rerank_select_merged(const SelectMergedArgs a) {
    __shared__ uint64_t s_u[RR_MAX_NB];
    __shared__ double s_d[RR_MAX_NB];
    __shared__ int s_nkept;

    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int64_t* __restrict__ ids = a.ids + q * a.L;
    const double* __restrict__ adc = a.adc + q * a.L;
    const int64_t* __restrict__ src = a.src_rec + q * a.L;

    if (tid == 0) s_nkept = 0;
    int64_t my_id[RR_MAX_NB / 256];
#pragma unroll
    for (int k = 0; k < RR_MAX_NB / 256; ++k) {
        const int i = tid + 256 * k;
        my_id[k] = -1;
        if (i < a.o.nb) {
            const int64_t id = ids[i];
            my_id[k] = id;
            double d = 0.0;
            if (id >= 0) {
                const int64_t r = src[i];
                d = (r >= 0 && r < a.n_true) ? a.true_d[r] : __longlong_as_double(0x7ff8000000000000LL);
                if (d != d) d = adc[i];
            }
            s_d[i] = d;
        }
    }
    __syncthreads();
    keep_rank_write(a.o, q, my_id, s_d, s_u, &s_nkept, tid);
}

bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

}  // namespace

extern "C" int cis_idmap_build_dev(const int64_t* d_ids, int64_t n, int64_t* d_keys, int64_t* d_rows, int64_t cap, void* stream) {
    CIS_REQUIRE(n >= 0, "bad id map arguments (n >= 0)");
    CIS_REQUIRE(pow2(cap) && cap <= IDMAP_MAX_CAP && cap / 2 >= n, "the id map's capacity must be a power of two >= 2 n (n = %lld, cap = %lld)",
                (long long)n, (long long)cap);
    CIS_REQUIRE(d_keys && d_rows && (n == 0 || d_ids), "NULL buffer");
    CIS_TRY(cis_lazy_init());
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_idmap_init, dim3((unsigned)ceil_div(cap, 256)), dim3(256), 0, st, d_keys, d_rows, cap);
    if (n) hipLaunchKernelGGL(k_idmap_insert, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, d_ids, n, d_keys, d_rows, cap);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_idmap_lookup_dev(const int64_t* d_keys, const int64_t* d_rows, int64_t cap, int64_t n_feats, const int64_t* d_ids,
                                    int64_t m, int64_t* d_out, void* stream) {
    CIS_REQUIRE(m >= 0 && n_feats >= 0 && m <= ((int64_t)1 << 38), "bad id look-up arguments");
    CIS_REQUIRE((d_keys == nullptr) == (d_rows == nullptr), "the id map needs both of its arrays (or neither: row = id)");
    CIS_REQUIRE(!d_keys || (pow2(cap) && cap <= IDMAP_MAX_CAP), "the id map's capacity must be a power of two (cap = %lld)", (long long)cap);
    if (m == 0) return CIS_OK;
    CIS_REQUIRE(d_ids && d_out, "NULL buffer");
    CIS_TRY(cis_lazy_init());
    hipLaunchKernelGGL(k_idmap_lookup, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, (hipStream_t)stream, d_keys, d_rows, cap, n_feats,
                       d_ids, m, d_out);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_rerank_select_dev(const void* d_feats, int f_dtype, int64_t n_feats, int D, const int64_t* d_map_keys,
                                     const int64_t* d_map_rows, int64_t map_cap, const void* d_q, int nq, const int64_t* d_ids,
                                     const double* d_adc, int L, int nb, int max_returned, int use_th, double near_dup_th,
                                     int64_t* d_out_ids, double* d_out_dists, int32_t* d_out_src, int32_t* d_n_kept, void* stream) {
    CIS_REQUIRE(f_dtype == CIS_F32 || f_dtype == CIS_F64, "f_dtype must be 4 or 8");
    CIS_REQUIRE(n_feats >= 0 && D > 0 && nq >= 0 && L >= 0 && max_returned >= 0, "bad re-ranking arguments");
    CIS_REQUIRE(nb >= 0 && nb <= L, "rerank_nb must be in [0, L] (nb = %d, L = %d)", nb, L);
    CIS_REQUIRE(nb <= RR_MAX_NB, "the device re-ranking holds at most %d results per query (nb = %d): use the host rerank", RR_MAX_NB, nb);
    CIS_REQUIRE((d_map_keys == nullptr) == (d_map_rows == nullptr), "the id map needs both of its arrays (or neither: row = id)");
    CIS_REQUIRE(!d_map_keys || (pow2(map_cap) && map_cap <= IDMAP_MAX_CAP), "the id map's capacity must be a power of two (cap = %lld)",
                (long long)map_cap);
    if (nq == 0) return CIS_OK;
    CIS_REQUIRE(d_n_kept && (nb == 0 || (d_q && d_ids && d_adc && d_out_ids && d_out_dists && d_out_src)), "NULL buffer");
    CIS_REQUIRE(nb == 0 || n_feats == 0 || d_feats, "NULL buffer");
    CIS_TRY(cis_lazy_init());
    hipStream_t st = (hipStream_t)stream;
    if (nb == 0) {
        CIS_CHECK_HIP(hipMemsetAsync(d_n_kept, 0, (size_t)nq * sizeof(int32_t), st));
        return CIS_OK;
    }
    RerankArgs a;
    a.feats = d_feats; a.n_feats = n_feats; a.map_keys = d_map_keys; a.map_rows = d_map_rows; a.map_cap = map_cap;
    a.Q = d_q; a.ids = d_ids; a.adc = d_adc; a.D = D; a.L = L;
    a.o = SelectOut{d_out_ids, d_out_dists, d_out_src, d_n_kept, near_dup_th, nb, max_returned, use_th ? 1 : 0};
    const size_t qbytes = (size_t)D * (size_t)f_dtype;
    const bool staged = qbytes <= (size_t)RR_STAGE_BYTES;
    const dim3 g((unsigned)nq), b(256);
    if (f_dtype == CIS_F32) {
        if (staged) hipLaunchKernelGGL((k_rerank_select<float, true>), g, b, qbytes, st, a);
        else hipLaunchKernelGGL((k_rerank_select<float, false>), g, b, 0, st, a);
    } else {
        if (staged) hipLaunchKernelGGL((k_rerank_select<double, true>), g, b, qbytes, st, a);
        else hipLaunchKernelGGL((k_rerank_select<double, false>), g, b, 0, st, a);
    }
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_rerank_packed_dev(const void* d_feats, int f_dtype, int64_t n_feats, int D, const int64_t* d_map_keys,
                                     const int64_t* d_map_rows, int64_t map_cap, const void* d_q, int nq, const cis_hit* d_recs,
                                     int64_t n_rec, const int64_t* d_off, const int32_t* d_cnt, int nb, double* d_true, void* stream) {
    CIS_REQUIRE(f_dtype == CIS_F32 || f_dtype == CIS_F64, "f_dtype must be 4 or 8");
    CIS_REQUIRE(n_feats >= 0 && D > 0 && nq >= 0 && n_rec >= 0, "bad re-ranking arguments");
    CIS_REQUIRE(nb >= 0 && nb <= RR_MAX_NB, "the device re-ranking holds at most %d results per query (nb = %d): use the host rerank", RR_MAX_NB, nb);
    CIS_REQUIRE((d_map_keys == nullptr) == (d_map_rows == nullptr), "the id map needs both of its arrays (or neither: row = id)");
    CIS_REQUIRE(!d_map_keys || (pow2(map_cap) && map_cap <= IDMAP_MAX_CAP), "the id map's capacity must be a power of two (cap = %lld)",
                (long long)map_cap);
    if (nq == 0 || n_rec == 0) return CIS_OK;
    CIS_REQUIRE(d_q && d_recs && d_off && d_cnt && d_true && (n_feats == 0 || d_feats), "NULL buffer");
    CIS_TRY(cis_lazy_init());
    PackedArgs a;
    a.feats = d_feats; a.n_feats = n_feats; a.map_keys = d_map_keys; a.map_rows = d_map_rows; a.map_cap = map_cap;
    a.Q = d_q; a.recs = d_recs; a.off = d_off; a.cnt = d_cnt; a.n_rec = n_rec; a.true_d = d_true; a.D = D; a.nb = nb;
    const size_t qbytes = (size_t)D * (size_t)f_dtype;
    const bool staged = qbytes <= (size_t)RR_STAGE_BYTES;
    const dim3 g((unsigned)nq), b(256);
    hipStream_t st = (hipStream_t)stream;
    if (f_dtype == CIS_F32) {
        if (staged) hipLaunchKernelGGL((k_rerank_packed<float, true>), g, b, qbytes, st, a);
        else hipLaunchKernelGGL((k_rerank_packed<float, false>), g, b, 0, st, a);
    } else {
        if (staged) hipLaunchKernelGGL((k_rerank_packed<double, true>), g, b, qbytes, st, a);
        else hipLaunchKernelGGL((k_rerank_packed<double, false>), g, b, 0, st, a);
    }
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_rerank_select_merged_dev(const int64_t* d_ids, const double* d_adc, const int64_t* d_src_rec, int nq, int L,
                                            const double* d_true, int64_t n_true, int nb, int max_returned, int use_th,
                                            double near_dup_th, int64_t* d_out_ids, double* d_out_dists, int32_t* d_out_src,
                                            int32_t* d_n_kept, void* stream) {
    CIS_REQUIRE(nq >= 0 && L >= 0 && max_returned >= 0 && n_true >= 0, "bad re-ranking arguments");
    CIS_REQUIRE(nb >= 0 && nb <= L, "rerank_nb must be in [0, L] (nb = %d, L = %d)", nb, L);
    CIS_REQUIRE(nb <= RR_MAX_NB, "the device re-ranking holds at most %d results per query (nb = %d): use the host rerank", RR_MAX_NB, nb);
    if (nq == 0) return CIS_OK;
    CIS_REQUIRE(d_n_kept && (nb == 0 || (d_ids && d_adc && d_src_rec && d_out_ids && d_out_dists && d_out_src)), "NULL buffer");
    CIS_REQUIRE(nb == 0 || n_true == 0 || d_true, "NULL buffer");
    CIS_TRY(cis_lazy_init());
    hipStream_t st = (hipStream_t)stream;
    if (nb == 0) {
        CIS_CHECK_HIP(hipMemsetAsync(d_n_kept, 0, (size_t)nq * sizeof(int32_t), st));
        return CIS_OK;
    }
    SelectMergedArgs a;
    a.ids = d_ids; a.adc = d_adc; a.src_rec = d_src_rec; a.true_d = d_true; a.n_true = n_true; a.L = L;
    a.o = SelectOut{d_out_ids, d_out_dists, d_out_src, d_n_kept, near_dup_th, nb, max_returned, use_th ? 1 : 0};
    hipLaunchKernelGGL(k_rerank_select_merged, dim3((unsigned)nq), dim3(256), 0, st, a);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}
