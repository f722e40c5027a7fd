// Feature rows kept as float16 in HBM behind a float32 interface (cis_featstore_create_half): the exact re-rank of lopq_rerank.hip on
// such rows (searcher_lopqhbase.py:849-912 and :964-1017), and the conversions into and out of the store (the `put` and the fetch of
// hbase_indexer_minimal.py:779-831).  Stored features are L2-normalised, so float16 keeps 11 significant bits of every component;
// a 4096-wide row is 8 KB instead of 16, and the re-rank, which does little besides moving rows, moves half the bytes.
//
// The arithmetic contract of the distance (k_rerank_select_half, k_rerank_packed_half), which the tests hold the kernels to:
//   y  = (float)h                      exact: every float16 is a float32
//   df = q - y                         float32, the query stays float32
//   acc = fma(df, df, acc)             float32; lane l owns the halves 8 (l + 64 t) .. + 7 of trip t and keeps two accumulators, one for
//                                      its even and one for its odd elements, each in ascending order; the two are added at the end
//   the lanes fold with the __shfl_xor butterfly 32 ... 1
//   distance = (double)sqrtf(acc)      the correctly rounded float32 root (sqrtf is, under this library's flags; __fsqrt_rn compiles to the
//                                      bare v_sqrt_f32, which is one ulp off for some arguments), widened
//   a NaN result keeps the ADC distance, and so does a result without a stored row (k_rerank_select's rules).
// With D non-negative terms, two roundings each, |d - d_exact| <= (D / 2 + 8) 2^-24 d_exact whatever the order.
//
// The row loop.  One workgroup of four waves per query, one row per wave at a time, RH_ROWS rows in flight per wave: k_rerank_select's
// split, so its look-up and keep_rank_write (rerank_common.h) are used as they are.  A 2-byte element per lane would be a 128-byte wave
// load, so a lane loads 16 bytes, 8 halves: one wave load instruction covers 1 KB of one row and a 4096-wide row takes eight.  Rows are
// 16-byte aligned (D % 8 == 0 and the base is).  A last trip that is not full is predicated per lane: a lane past the end loads word 0
// of the row again and its differences are replaced by zero; there is no scalar tail.
//
// The query in LDS.  Lane l needs the floats 8 (l + 64 t) .. + 7 in trip t: in element order that is a 32-byte lane stride and both
// ds_read_b128 of a trip run into bank conflicts.  The staging loop permutes instead: 16-byte word ((2 t + h) 64 + l) holds the floats
// 8 (l + 64 t) + 4 h .. + 3, h = 0, 1, so consecutive lanes read consecutive words; words past D are zero.  Up to the 32 KB limit of
// the float32 kernels (D <= 8192); wider queries are read in place.
#include "rerank_common.h"

int cis_fs_half_scatter(const void* from_f32, void* to_f16, int D, const int64_t* src, const int64_t* dst, int64_t njobs, hipStream_t st);
int cis_fs_half_gather(const void* from_f16, void* to_f32, int D, const int64_t* src, int64_t njobs, hipStream_t st);

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int RH_ROWS = 8;            // feature rows in flight per wave, one 16-byte load per lane each (profiles/rerank_half.txt)
constexpr int RH_WG_ROW_HALVES = 2048;  // a row of this width or more is converted by a workgroup, a narrower one by a wave

// 16-byte words the staged query takes: two per lane and trip
__host__ __device__ __forceinline__ int staged_words(int D) { return (((D >> 3) + 63) >> 6) * 128; }

__device__ __forceinline__ void stage_query(const float* __restrict__ qg, int D, f32x4* s_q, int tid) {
    const int words = staged_words(D);
    for (int i = tid; i < words; i += 256) {
        const int t = i >> 7, h = (i >> 6) & 1, l = i & 63;
        const int e = 8 * (l + 64 * t) + 4 * h;
        s_q[i] = e < D ? *(const f32x4*)(qg + e) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// Distances of the results listed in s_work (their feature rows in s_row), measure_rows' contract: a short last group repeats its
// first row and drops the copy; lane 0 hands store(result, folded sum) each result once.
template <bool STAGED, typename Store>
__device__ __forceinline__ void measure_rows_half(const _Float16* __restrict__ feats, int D, const float* __restrict__ qg, const f32x4* s_q,
                                                  const uint64_t* s_row, const int* s_work, int nwork, int lane, int wave, Store store) {
    const int nv = D >> 3;          // 16-byte words of a row
    const int full = nv >> 6;       // trips in which every lane has a word
    const int rest = nv & 63;       // lanes of the last, partial trip
    for (int t0 = wave; t0 < nwork; t0 += 4 * RH_ROWS) {
        int res[RH_ROWS];
        const half8* x[RH_ROWS];
        float acc0[RH_ROWS], acc1[RH_ROWS];
#pragma unroll
        for (int r = 0; r < RH_ROWS; ++r) {
            const int t = t0 + 4 * r;
            res[r] = t < nwork ? s_work[t] : -1;
            x[r] = (const half8*)(feats + (int64_t)s_row[res[r] >= 0 ? res[r] : s_work[t0]] * D);
            acc0[r] = 0.f;
            acc1[r] = 0.f;
        }
        // trip t: this lane's word w of every row against the query's floats 8 w .. + 7; live = false replaces the differences by zero
        auto trip = [&](int t, int w, bool live) __attribute__((always_inline)) {
            half8 y[RH_ROWS];
#pragma unroll
            for (int r = 0; r < RH_ROWS; ++r) y[r] = x[r][w];
            f32x4 qa, qb;
            if (STAGED) {
                qa = s_q[(2 * t) * 64 + lane];
                qb = s_q[(2 * t + 1) * 64 + lane];
            } else {
                const f32x4* q4 = (const f32x4*)qg + 2 * w;
                qa = q4[0];
                qb = q4[1];
            }
            const float qv[8] = {qa[0], qa[1], qa[2], qa[3], qb[0], qb[1], qb[2], qb[3]};
#pragma unroll
            for (int r = 0; r < RH_ROWS; ++r) {
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    float d0 = qv[j] - (float)y[r][j], d1 = qv[j + 1] - (float)y[r][j + 1];
                    d0 = live ? d0 : 0.f;
                    d1 = live ? d1 : 0.f;
                    acc0[r] = fmaf(d0, d0, acc0[r]);
                    acc1[r] = fmaf(d1, d1, acc1[r]);
                }
            }
        };
        for (int t = 0; t < full; ++t) trip(t, lane + 64 * t, true);
        if (rest) trip(full, lane < rest ? lane + 64 * full : 0, lane < rest);
#pragma unroll
        for (int r = 0; r < RH_ROWS; ++r) {
            float s = acc0[r] + acc1[r];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
            if (lane == 0 && res[r] >= 0) store(res[r], s);
        }
    }
}

// k_rerank_select on float16 rows: one workgroup (4 waves) per query.  STAGED: the permuted query sits in dynamic LDS.  Held to three
// waves per SIMD, which is what 20 KB of static LDS beside a staged 4096-wide query allows anyway (131 / 134 VGPRs, nothing in private memory).
template <bool STAGED>
__global__ __launch_bounds__(256, 3) void k_rerank_select_half(const RerankArgs a) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ uint64_t s_u[RR_MAX_NB];   // the feature row of result i, later its sort key
    __shared__ double s_d[RR_MAX_NB];     // the distance result i is ranked by
    __shared__ int s_work[RR_MAX_NB];     // results whose feature is resident (any order)
    __shared__ int s_nwork, s_nkept;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int D = a.D, nb = a.o.nb;
    const _Float16* __restrict__ feats = (const _Float16*)a.feats;
    const float* __restrict__ qg = (const float*)a.Q + q * D;
    const int64_t* __restrict__ ids = a.ids + q * a.L;
    const double* __restrict__ adc = a.adc + q * a.L;
    f32x4* s_q = (f32x4*)s_dyn;

    if (tid == 0) { s_nwork = 0; s_nkept = 0; }
    if (STAGED) stage_query(qg, D, s_q, tid);
    __syncthreads();

    // 1. rows of the results, one result per thread; a result without a resident feature is ranked by its ADC distance
#pragma unroll
    for (int k = 0; k < RR_MAX_NB / 256; ++k) {
        const int i = tid + 256 * k;
        if (i < nb) {
            const int64_t id = ids[i];
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
    measure_rows_half<STAGED>(feats, D, qg, s_q, s_u, s_work, s_nwork, lane, wave, [&](int i, float s) {
        const double d = (double)sqrtf(s);
        s_d[i] = d != d ? adc[i] : d;  // a NaN feature keeps the ADC distance
    });
    __syncthreads();

    // 3. keep, 4. rank and write (the ids are read again here: held across the row loop they cost it eight registers)
    int64_t my_id[RR_MAX_NB / 256];
#pragma unroll
    for (int k = 0; k < RR_MAX_NB / 256; ++k) my_id[k] = tid + 256 * k < nb ? ids[tid + 256 * k] : -1;
    keep_rank_write(a.o, q, my_id, s_d, s_u, &s_nkept, tid);
}

// k_rerank_packed on float16 rows: one workgroup per list; a list that does not lie inside [0, n_rec) is left alone.
template <bool STAGED>
__global__ __launch_bounds__(256) void k_rerank_packed_half(const PackedArgs a) {
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
    const _Float16* __restrict__ feats = (const _Float16*)a.feats;
    const float* __restrict__ qg = (const float*)a.Q + q * D;
    const cis_hit* __restrict__ recs = a.recs + o;
    double* __restrict__ true_d = a.true_d + o;
    f32x4* s_q = (f32x4*)s_dyn;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    if (tid == 0) s_nwork = 0;
    if (STAGED && n > 0) stage_query(qg, D, s_q, tid);
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

    measure_rows_half<STAGED>(feats, D, qg, s_q, s_u, s_work, s_nwork, lane, wave,
                              [&](int i, float s) { true_d[i] = (double)sqrtf(s); });
}

// ---- into and out of the store -----------------------------------------------------------------------------------------------------
// k_fs_copy's jobs with a conversion.  Job j of the put: float32 row src[j] of `from` becomes float16 row dst[j] of `to`, rounded to
// nearest even (v_cvt_f16_f32: subnormals kept, overflow to +-inf, NaN to NaN -- numpy's astype(float16) bit for bit); a negative src
// or dst is no job.  TPR threads per row (64: a wave, 256: the workgroup), 8 elements each: two 16-byte loads (vec: `from` is 16-byte
// aligned; scalar loads otherwise) and one 16-byte store.
template <int TPR>
__global__ __launch_bounds__(256) void k_fs_put_half(const float* __restrict__ from, _Float16* __restrict__ to, int D,
                                                     const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t njobs, int vec) {
    const int64_t j = (int64_t)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
    if (j >= njobs) return;
    const int t = threadIdx.x % TPR;
    const int64_t d = dst[j], s = src[j];
    if (d < 0 || s < 0) return;
    const float* __restrict__ in = from + s * D;
    half8* __restrict__ o = (half8*)(to + d * D);
    for (int w = t; w < (D >> 3); w += TPR) {
        f32x4 a, b;
        if (vec) {
            a = ((const f32x4*)in)[2 * w];
            b = ((const f32x4*)in)[2 * w + 1];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = in[8 * w + e];
                b[e] = in[8 * w + 4 + e];
            }
        }
        half8 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            h[e] = (_Float16)a[e];
            h[4 + e] = (_Float16)b[e];
        }
        o[w] = h;
    }
}

// Job j of the gather: float16 row src[j] of `from` (src == NULL: row j), widened, becomes float32 row j of `to`; src[j] < 0 gives a
// row of zeros.  One 16-byte load and two 16-byte stores per thread and step (vec: `to` is 16-byte aligned).
template <int TPR>
__global__ __launch_bounds__(256) void k_fs_get_half(const _Float16* __restrict__ from, float* __restrict__ to, int D,
                                                     const int64_t* __restrict__ src, int64_t njobs, int vec) {
    const int64_t j = (int64_t)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
    if (j >= njobs) return;
    const int t = threadIdx.x % TPR;
    const int64_t s = src ? src[j] : j;
    const half8* __restrict__ in = (const half8*)(from + (s < 0 ? 0 : s) * D);
    float* __restrict__ o = to + j * D;
    for (int w = t; w < (D >> 3); w += TPR) {
        half8 h = {0, 0, 0, 0, 0, 0, 0, 0};
        if (s >= 0) h = in[w];  // (the same for every thread of the row)
        f32x4 a, b;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[e] = (float)h[e];
            b[e] = (float)h[4 + e];
        }
        if (vec) {
            ((f32x4*)o)[2 * w] = a;
            ((f32x4*)o)[2 * w + 1] = b;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[8 * w + e] = a[e];
                o[8 * w + 4 + e] = b[e];
            }
        }
    }
}

inline unsigned row_grid(int64_t njobs, int tpr) { return (unsigned)ceil_div(njobs, 256 / tpr); }

// what both re-rank entry points ask of the rows and the queries
int half_operands_ok(const void* d_feats, int D, const void* d_q) {
    CIS_REQUIRE(D % 8 == 0, "float16 feature rows need D %% 8 == 0 (D = %d)", D);
    CIS_REQUIRE((((uintptr_t)d_feats | (uintptr_t)d_q) & 15) == 0, "float16 features and their queries must be 16-byte aligned");
    return CIS_OK;
}

}  // namespace

int cis_fs_half_scatter(const void* from_f32, void* to_f16, int D, const int64_t* src, const int64_t* dst, int64_t njobs, hipStream_t st) {
    if (njobs <= 0) return CIS_OK;
    CIS_REQUIRE(D > 0 && D % 8 == 0 && ((uintptr_t)to_f16 & 15) == 0 && ((uintptr_t)from_f32 & 3) == 0 && src && dst, "bad float16 put");
    const int vec = ((uintptr_t)from_f32 & 15) == 0 ? 1 : 0;
    if (D >= RH_WG_ROW_HALVES)
        hipLaunchKernelGGL(k_fs_put_half<256>, dim3(row_grid(njobs, 256)), dim3(256), 0, st, (const float*)from_f32, (_Float16*)to_f16, D, src, dst,
                           njobs, vec);
    else
        hipLaunchKernelGGL(k_fs_put_half<64>, dim3(row_grid(njobs, 64)), dim3(256), 0, st, (const float*)from_f32, (_Float16*)to_f16, D, src, dst,
                           njobs, vec);
    return CIS_OK;
}

int cis_fs_half_gather(const void* from_f16, void* to_f32, int D, const int64_t* src, int64_t njobs, hipStream_t st) {
    if (njobs <= 0) return CIS_OK;
    CIS_REQUIRE(D > 0 && D % 8 == 0 && ((uintptr_t)from_f16 & 15) == 0 && ((uintptr_t)to_f32 & 3) == 0, "bad float16 gather");
    const int vec = ((uintptr_t)to_f32 & 15) == 0 ? 1 : 0;
    if (D >= RH_WG_ROW_HALVES)
        hipLaunchKernelGGL(k_fs_get_half<256>, dim3(row_grid(njobs, 256)), dim3(256), 0, st, (const _Float16*)from_f16, (float*)to_f32, D, src, njobs,
                           vec);
    else
        hipLaunchKernelGGL(k_fs_get_half<64>, dim3(row_grid(njobs, 64)), dim3(256), 0, st, (const _Float16*)from_f16, (float*)to_f32, D, src, njobs,
                           vec);
    return CIS_OK;
}

extern "C" int cis_rerank_select_half_dev(const void* d_feats, int64_t n_feats, int D, const int64_t* d_map_keys, const int64_t* d_map_rows,
                                          int64_t map_cap, const void* d_q, int nq, const int64_t* d_ids, const double* d_adc, int L, int nb,
                                          int max_returned, int use_th, double near_dup_th, int64_t* d_out_ids, double* d_out_dists,
                                          int32_t* d_out_src, int32_t* d_n_kept, void* stream) {
    CIS_REQUIRE(n_feats >= 0 && D > 0 && nq >= 0 && L >= 0 && max_returned >= 0, "bad re-ranking arguments");
    CIS_REQUIRE(nb >= 0 && nb <= L, "rerank_nb must be in [0, L] (nb = %d, L = %d)", nb, L);
    CIS_REQUIRE(nb <= RR_MAX_NB, "the device re-ranking holds at most %d results per query (nb = %d): use the host rerank", RR_MAX_NB, nb);
    CIS_REQUIRE((d_map_keys == nullptr) == (d_map_rows == nullptr), "the id map needs both of its arrays (or neither: row = id)");
    CIS_REQUIRE(!d_map_keys || (pow2(map_cap) && map_cap <= IDMAP_MAX_CAP), "the id map's capacity must be a power of two (cap = %lld)",
                (long long)map_cap);
    CIS_TRY(half_operands_ok(d_feats, D, d_q));
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
    const bool staged = (size_t)D * sizeof(float) <= (size_t)RR_STAGE_BYTES;
    const dim3 g((unsigned)nq), b(256);
    if (staged) hipLaunchKernelGGL(k_rerank_select_half<true>, g, b, (size_t)staged_words(D) * 16, st, a);
    else hipLaunchKernelGGL(k_rerank_select_half<false>, g, b, 0, st, a);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_rerank_packed_half_dev(const void* d_feats, int64_t n_feats, int D, const int64_t* d_map_keys, const int64_t* d_map_rows,
                                          int64_t map_cap, const void* d_q, int nq, const cis_hit* d_recs, int64_t n_rec, const int64_t* d_off,
                                          const int32_t* d_cnt, int nb, double* d_true, void* stream) {
    CIS_REQUIRE(n_feats >= 0 && D > 0 && nq >= 0 && n_rec >= 0, "bad re-ranking arguments");
    CIS_REQUIRE(nb >= 0 && nb <= RR_MAX_NB, "the device re-ranking holds at most %d results per query (nb = %d): use the host rerank", RR_MAX_NB, nb);
    CIS_REQUIRE((d_map_keys == nullptr) == (d_map_rows == nullptr), "the id map needs both of its arrays (or neither: row = id)");
    CIS_REQUIRE(!d_map_keys || (pow2(map_cap) && map_cap <= IDMAP_MAX_CAP), "the id map's capacity must be a power of two (cap = %lld)",
                (long long)map_cap);
    CIS_TRY(half_operands_ok(d_feats, D, d_q));
    if (nq == 0 || n_rec == 0) return CIS_OK;
    CIS_REQUIRE(d_q && d_recs && d_off && d_cnt && d_true && (n_feats == 0 || d_feats), "NULL buffer");
    CIS_TRY(cis_lazy_init());
    PackedArgs a;
    a.feats = d_feats; a.n_feats = n_feats; a.map_keys = d_map_keys; a.map_rows = d_map_rows; a.map_cap = map_cap;
    a.Q = d_q; a.recs = d_recs; a.off = d_off; a.cnt = d_cnt; a.n_rec = n_rec; a.true_d = d_true; a.D = D; a.nb = nb;
    const bool staged = (size_t)D * sizeof(float) <= (size_t)RR_STAGE_BYTES;
    const dim3 g((unsigned)nq), b(256);
    hipStream_t st = (hipStream_t)stream;
    if (staged) hipLaunchKernelGGL(k_rerank_packed_half<true>, g, b, (size_t)staged_words(D) * 16, st, a);
    else hipLaunchKernelGGL(k_rerank_packed_half<false>, g, b, 0, st, a);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}
