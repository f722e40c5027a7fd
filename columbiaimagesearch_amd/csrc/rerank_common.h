// What the re-rank kernels of lopq_rerank.hip (float32 / float64 feature rows) and feat_half.hip (float16 rows) share: the id -> row
// look-up, the sort key, the keep / rank / write end of a query and the launch operands.  Everything sits in the unnamed namespace, as
// it did inside lopq_rerank.hip, so the kernels of that file keep their names and their listings.
#pragma once
#include "common.h"

namespace {

constexpr int RR_MAX_NB = 1024;         // results per query the ranking holds in LDS (4 per thread)
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

// Sort key of a distance: ascending as unsigned, -0 == +0, every NaN behind every number (np.argsort's order), and all ones for
// an entry that is not kept.
__device__ __forceinline__ uint64_t rank_key(double d) {
    if (d != d) return 0xfffffffffffffffeULL;
    const uint64_t b = (uint64_t)__double_as_longlong(d + 0.0);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
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

// Operands of the fused look-up, re-rank and select (one workgroup per query)
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

// Operands of the re-rank of the cell-sharded index (one workgroup per list)
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

inline bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

}  // namespace
