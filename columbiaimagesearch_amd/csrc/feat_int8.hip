// Feature rows kept as int8 codes with an in-row float32 scale behind a float32 interface (cis_featstore_create_int8): the exact
// re-rank of lopq_rerank.hip on such rows (searcher_lopqhbase.py:849-912 and :964-1017), and the conversions into and out of the store
// (the `put` and the fetch of hbase_indexer_minimal.py:779-831).  Stored features are L2-normalised, so a scale per row and 8-bit codes
// keep about 7 bits of every component relative to the row's largest; a 4096-wide row is 4112 bytes instead of 16 KB.
// The exact k-NN reads the same rows in place: knn_int8.hip (prefilter on the int8 matrix cores) and the Int8Rows view of lopq_eval.hip.
//
// The row: 16 + D bytes, D % 16 == 0, 16-byte aligned.  Word 0 (16 bytes) holds the float32 scale s at byte 0 and zeros behind it,
// words 1 .. D / 16 the codes, element 16 w + k in byte k of word 1 + w.  The scale travels with the row, so k_fs_copy, the removal and
// the growth copy of feat_store.hip move such rows as bytes.
//
// The quantisation contract (k_fs_put_int8), which the tests hold to a numpy model bit for bit:
//   m = max |x_i|, s = m / 127         float32, IEEE division (the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence under
//                                      this library's flags: build/feat_int8.s)
//   c_i = clip(rint(x_i / s), -127, 127)   float32 division, round half to even; -128 is never stored
//   s == 0 (a zero row, or one so small that m / 127 rounds to zero): s = 0 and zero codes
//   a non-finite component: s = NaN and zero codes, so the row reads back as NaN and its distance is NaN
//   get / rows hand back (float)c_i * s, one float32 product; an unknown id gives zeros.
//
// The arithmetic contract of the distance (k_rerank_select_int8, k_rerank_packed_int8):
//   df = fma(-(float)c, s, q)          one rounding of q - c s; the query stays float32
//   acc = fma(df, df, acc)             float32; a lane owns the 16 codes of word w = l + G t of its row in trip t and keeps two
//                                      accumulators, one for its even and one for its odd elements, each in ascending order; the two are
//                                      added at the end
//   the G lanes of a row fold with the __shfl_xor butterfly G / 2 ... 1
//   distance = (double)sqrtf(acc)      the correctly rounded float32 root (see feat_half.hip), widened
//   a NaN result keeps the ADC distance, and so does a result without a stored row (k_rerank_select's rules).
// With D non-negative terms, two roundings each, |d - d_exact| <= (D / 2 + 8) 2^-24 d_exact whatever the order, d_exact the distance to
// the DEQUANTISED row c s.
//
// The split.  One workgroup of four waves per query (or list), so the look-up and keep_rank_write of rerank_common.h are used as they
// are.  A lane loads 16 bytes = 16 codes, and a row goes to a group of G lanes, G the power of two in [4, 64] that covers its D / 16
// words (64 and several trips above 1024): at D = 128 a group is 8 lanes and ONE wave load instruction covers eight different rows, where
// a row per wave would leave 56 lanes idle.  A wave keeps R loads in flight per lane (R = 8 for G >= 16, 4 below: 4 x 64 / G x R rows per
// workgroup pass, 128 at D = 128, about one list), every lane reads its row's scale with the row, and the butterfly runs over G lanes
// only.  (R = 8 / 4 is the one setting that was built and measured, profiles/rerank_int8.txt.)  A trip that is not full is predicated per lane: a lane past the end loads word 1 again and its differences are replaced by
// zero; there is no scalar tail.
//
// The query in LDS, in the order the lanes consume it: 16-byte word ((4 t + h) G + l) holds the floats 16 (l + G t) + 4 h .. + 3,
// h = 0 .. 3, so the four ds_read_b128 of a trip read consecutive words from consecutive lanes, and with G < 64 every group of the wave
// reads the SAME words, a broadcast; words past D are zero.  Up to the 32 KB limit of the float32 kernels (D <= 8192); wider queries are
// read in place.
#include <cfloat>

#include "rerank_common.h"

int cis_fs_int8_scatter(const void* from_f32, void* to_i8, int D, const int64_t* src, const int64_t* dst, int64_t njobs, hipStream_t st);
int cis_fs_int8_gather(const void* from_i8, void* to_f32, int D, const int64_t* src, int64_t njobs, hipStream_t st);

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int RI_WG_ROW_CODES = 4096;  // a row of this width or more is converted by a workgroup, a narrower one by a wave

// lanes a row is given to: the power of two in [4, 64] that covers its 16-byte words
__host__ __device__ __forceinline__ int group_lanes(int D) {
    int g = 4;
    while (g < 64 && g < (D >> 4)) g <<= 1;
    return g;
}
// 16-byte row words in flight per lane
__host__ __device__ constexpr int rows_in_flight(int G) { return G >= 16 ? 8 : 4; }
// 16-byte words the staged query takes: four per lane of a group and trip
__host__ __device__ __forceinline__ int staged_words(int D, int G) { return (((D >> 4) + G - 1) / G) * 4 * G; }

// code k of a row word: byte k & 3 of dword k >> 2, sign-extended
__device__ __forceinline__ float code_of(const u32x4& y, int k) { return (float)(int)(int8_t)(y[k >> 2] >> (8 * (k & 3))); }

template <int G>
__device__ __forceinline__ void stage_query(const float* __restrict__ qg, int D, f32x4* s_q, int tid) {
    const int words = staged_words(D, G);
    for (int i = tid; i < words; i += 256) {
        const int t = i / (4 * G), h = (i / G) & 3, l = i & (G - 1);
        const int e = 16 * (l + G * t) + 4 * h;
        s_q[i] = e < D ? *(const f32x4*)(qg + e) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// Distances of the results listed in s_work (their feature rows in s_row), measure_rows' contract: a place past the end of the list
// takes the list's first row and drops the copy; the first lane of a group hands store(result, folded sum) each result once.
template <int G, int R, bool STAGED, typename Store>
__device__ __forceinline__ void measure_rows_int8(const unsigned char* __restrict__ feats, int D, const float* __restrict__ qg,
                                                  const f32x4* s_q, const uint64_t* s_row, const int* s_work, int nwork, int lane, int wave,
                                                  Store store) {
    constexpr int NG = 64 / G;      // rows one wave load instruction covers
    const int l = lane & (G - 1), g = lane / G;
    const int nv = D >> 4;          // 16-byte code words of a row
    const int full = nv / G;        // trips in which every lane of the group has a word
    const int rest = nv & (G - 1);  // lanes of the last, partial trip
    const int64_t row_bytes = 16 + (int64_t)D;
    for (int t0 = 0; t0 < nwork; t0 += 4 * R * NG) {
        int res[R];
        const u32x4* x[R];
        float sc[R], acc0[R], acc1[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int t = t0 + (4 * r + wave) * NG + g;
            res[r] = t < nwork ? s_work[t] : -1;
            x[r] = (const u32x4*)(feats + (int64_t)s_row[res[r] >= 0 ? res[r] : s_work[0]] * row_bytes);
            sc[r] = *(const float*)x[r];
            acc0[r] = 0.f;
            acc1[r] = 0.f;
        }
        // trip t: this lane's code word w of every row against the query's floats 16 w .. + 15; live = false replaces the differences by zero
        auto trip = [&](int t, int w, bool live) __attribute__((always_inline)) {
            u32x4 y[R];
#pragma unroll
            for (int r = 0; r < R; ++r) y[r] = x[r][1 + w];
            f32x4 qv[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) qv[h] = STAGED ? s_q[(4 * t + h) * G + l] : ((const f32x4*)qg)[4 * w + h];
#pragma unroll
            for (int r = 0; r < R; ++r) {
#pragma unroll
                for (int k = 0; k < 16; k += 2) {
                    float d0 = fmaf(-code_of(y[r], k), sc[r], qv[k >> 2][k & 3]);
                    float d1 = fmaf(-code_of(y[r], k + 1), sc[r], qv[k >> 2][(k & 3) + 1]);
                    d0 = live ? d0 : 0.f;
                    d1 = live ? d1 : 0.f;
                    acc0[r] = fmaf(d0, d0, acc0[r]);
                    acc1[r] = fmaf(d1, d1, acc1[r]);
                }
            }
        };
        for (int t = 0; t < full; ++t) trip(t, l + G * t, true);
        if (rest) trip(full, l < rest ? l + G * full : 0, l < rest);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float s = acc0[r] + acc1[r];
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
            if (l == 0 && res[r] >= 0) store(res[r], s);
        }
    }
}

// k_rerank_select on int8 rows: one workgroup (4 waves) per query, a row per group of G lanes, R row words in flight per lane.
// STAGED: the permuted query sits in dynamic LDS.  Held to three waves per SIMD, which is what 20 KB of static LDS beside a staged
// 4096-wide query allows anyway.
template <int G, int R, bool STAGED>
__global__ __launch_bounds__(256, 3) void k_rerank_select_int8(const RerankArgs a) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ uint64_t s_u[RR_MAX_NB];   // the feature row of result i, later its sort key
    __shared__ double s_d[RR_MAX_NB];     // the distance result i is ranked by
    __shared__ int s_work[RR_MAX_NB];     // results whose feature is resident (any order)
    __shared__ int s_nwork, s_nkept;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int D = a.D, nb = a.o.nb;
    const float* __restrict__ qg = (const float*)a.Q + q * D;
    const int64_t* __restrict__ ids = a.ids + q * a.L;
    const double* __restrict__ adc = a.adc + q * a.L;
    f32x4* s_q = (f32x4*)s_dyn;

    if (tid == 0) { s_nwork = 0; s_nkept = 0; }
    if (STAGED) stage_query<G>(qg, D, s_q, tid);
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
    measure_rows_int8<G, R, STAGED>((const unsigned char*)a.feats, D, qg, s_q, s_u, s_work, s_nwork, lane, wave, [&](int i, float s) {
        const double d = (double)sqrtf(s);
        s_d[i] = d != d ? adc[i] : d;  // a NaN feature keeps the ADC distance
    });
    __syncthreads();

    // 3. keep, 4. rank and write (the ids are read again here, as in k_rerank_select_half)
    int64_t my_id[RR_MAX_NB / 256];
#pragma unroll
    for (int k = 0; k < RR_MAX_NB / 256; ++k) my_id[k] = tid + 256 * k < nb ? ids[tid + 256 * k] : -1;
    keep_rank_write(a.o, q, my_id, s_d, s_u, &s_nkept, tid);
}

// k_rerank_packed on int8 rows: one workgroup per list; a list that does not lie inside [0, n_rec) is left alone.
template <int G, int R, bool STAGED>
__global__ __launch_bounds__(256) void k_rerank_packed_int8(const PackedArgs a) {
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
    const float* __restrict__ qg = (const float*)a.Q + q * D;
    const cis_hit* __restrict__ recs = a.recs + o;
    double* __restrict__ true_d = a.true_d + o;
    f32x4* s_q = (f32x4*)s_dyn;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    if (tid == 0) s_nwork = 0;
    if (STAGED && n > 0) stage_query<G>(qg, D, s_q, tid);
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

    measure_rows_int8<G, R, STAGED>((const unsigned char*)a.feats, D, qg, s_q, s_u, s_work, s_nwork, lane, wave,
                                    [&](int i, float s) { true_d[i] = (double)sqrtf(s); });
}

// ---- into and out of the store -----------------------------------------------------------------------------------------------------
// k_fs_copy's jobs with a conversion.  Job j of the put: float32 row src[j] of `from` becomes int8 row dst[j] of `to` by the contract
// at the top; a negative src or dst is no job.  TPR threads per row (64: a wave, 256: the workgroup), 16 elements per thread and step:
// four 16-byte loads (vec: `from` is 16-byte aligned; scalar loads otherwise) and one 16-byte store.  Two passes inside the kernel, the
// largest magnitude and then the codes; the second reads the row again, from cache.
template <int TPR>
__global__ __launch_bounds__(256) void k_fs_put_int8(const float* __restrict__ from, unsigned char* __restrict__ to, int D,
                                                     const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t njobs, int vec) {
    __shared__ float s_m[4];
    __shared__ int s_bad[4];
    const int64_t j = (int64_t)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
    if (j >= njobs) return;  // (the same for every thread of the row, and so are the next two)
    const int t = threadIdx.x % TPR;
    const int64_t d = dst[j], s = src[j];
    if (d < 0 || s < 0) return;
    const float* __restrict__ in = from + s * D;
    u32x4* __restrict__ o = (u32x4*)(to + d * (16 + (int64_t)D));
    const int nv = D >> 4;
    auto load16 = [&](int w, float (&x)[16]) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            f32x4 a;
            if (vec) {
                a = ((const f32x4*)in)[4 * w + h];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] = in[16 * w + 4 * h + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) x[4 * h + e] = a[e];
        }
    };
    float m = 0.f;
    int bad = 0;
    for (int w = t; w < nv; w += TPR) {
        float x[16];
        load16(w, x);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float ax = fabsf(x[e]);
            m = fmaxf(m, ax);
            bad |= !(ax <= FLT_MAX) ? 1 : 0;  // +-inf and NaN
        }
    }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
        m = fmaxf(m, __shfl_xor(m, k));
        bad |= __shfl_xor(bad, k);
    }
    if (TPR == 256) {
        if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_bad[threadIdx.x >> 6] = bad; }
        __syncthreads();
        m = fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
        bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
    }
    const float sc = bad ? __uint_as_float(0x7fc00000u) : m / 127.0f;
    const bool zero = bad || sc == 0.f;
    if (t == 0) o[0] = u32x4{__float_as_uint(sc), 0u, 0u, 0u};
    for (int w = t; w < nv; w += TPR) {
        float x[16];
        load16(w, x);
        u32x4 p = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            float r = fminf(fmaxf(rintf(x[e] / sc), -127.f), 127.f);
            r = zero ? 0.f : r;
            p[e >> 2] |= ((uint32_t)(int)r & 0xffu) << (8 * (e & 3));
        }
        o[1 + w] = p;
    }
}

// Job j of the gather: int8 row src[j] of `from` (src == NULL: row j), dequantised, becomes float32 row j of `to`; src[j] < 0 gives a
// row of zeros.  One 16-byte load and four 16-byte stores per thread and step (vec: `to` is 16-byte aligned).
template <int TPR>
__global__ __launch_bounds__(256) void k_fs_get_int8(const unsigned char* __restrict__ from, float* __restrict__ to, int D,
                                                     const int64_t* __restrict__ src, int64_t njobs, int vec) {
    const int64_t j = (int64_t)blockIdx.x * (256 / TPR) + threadIdx.x / TPR;
    if (j >= njobs) return;
    const int t = threadIdx.x % TPR;
    const int64_t s = src ? src[j] : j;
    const u32x4* __restrict__ in = (const u32x4*)(from + (s < 0 ? 0 : s) * (16 + (int64_t)D));
    float* __restrict__ o = to + j * D;
    const float sc = s >= 0 ? *(const float*)in : 0.f;  // (the same for every thread of the row)
    for (int w = t; w < (D >> 4); w += TPR) {
        u32x4 y = {0u, 0u, 0u, 0u};
        if (s >= 0) y = in[1 + w];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            f32x4 a;
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = code_of(y, 4 * h + e) * sc;
            if (vec) {
                ((f32x4*)o)[4 * w + h] = a;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[16 * w + 4 * h + e] = a[e];
            }
        }
    }
}

inline unsigned row_grid(int64_t njobs, int tpr) { return (unsigned)ceil_div(njobs, 256 / tpr); }

// what both re-rank entry points ask of the rows and the queries
int int8_operands_ok(const void* d_feats, int D, const void* d_q) {
    CIS_REQUIRE(D % 16 == 0, "int8 feature rows need D %% 16 == 0 (D = %d)", D);
    CIS_REQUIRE((((uintptr_t)d_feats | (uintptr_t)d_q) & 15) == 0, "int8 features and their queries must be 16-byte aligned");
    return CIS_OK;
}

// K<G, R, STAGED> for the width D: the group that covers the row; a query read in place is wider than 8192, a full wave per row
#define RI_LAUNCH(K, G_, ST_, lds) hipLaunchKernelGGL((K<G_, rows_in_flight(G_), ST_>), g, b, lds, st, a)
#define RI_DISPATCH(K)                                                        \
    do {                                                                      \
        const size_t lds = (size_t)staged_words(D, group_lanes(D)) * 16;      \
        if (!staged) RI_LAUNCH(K, 64, false, 0);                              \
        else switch (group_lanes(D)) {                                        \
            case 4: RI_LAUNCH(K, 4, true, lds); break;                        \
            case 8: RI_LAUNCH(K, 8, true, lds); break;                        \
            case 16: RI_LAUNCH(K, 16, true, lds); break;                      \
            case 32: RI_LAUNCH(K, 32, true, lds); break;                      \
            default: RI_LAUNCH(K, 64, true, lds); break;                      \
        }                                                                     \
    } while (0)

}  // namespace

int cis_fs_int8_scatter(const void* from_f32, void* to_i8, int D, const int64_t* src, const int64_t* dst, int64_t njobs, hipStream_t st) {
    if (njobs <= 0) return CIS_OK;
    CIS_REQUIRE(D > 0 && D % 16 == 0 && ((uintptr_t)to_i8 & 15) == 0 && ((uintptr_t)from_f32 & 3) == 0 && src && dst, "bad int8 put");
    const int vec = ((uintptr_t)from_f32 & 15) == 0 ? 1 : 0;
    if (D >= RI_WG_ROW_CODES)
        hipLaunchKernelGGL(k_fs_put_int8<256>, dim3(row_grid(njobs, 256)), dim3(256), 0, st, (const float*)from_f32, (unsigned char*)to_i8, D, src,
                           dst, njobs, vec);
    else
        hipLaunchKernelGGL(k_fs_put_int8<64>, dim3(row_grid(njobs, 64)), dim3(256), 0, st, (const float*)from_f32, (unsigned char*)to_i8, D, src,
                           dst, njobs, vec);
    return CIS_OK;
}

int cis_fs_int8_gather(const void* from_i8, void* to_f32, int D, const int64_t* src, int64_t njobs, hipStream_t st) {
    if (njobs <= 0) return CIS_OK;
    CIS_REQUIRE(D > 0 && D % 16 == 0 && ((uintptr_t)from_i8 & 15) == 0 && ((uintptr_t)to_f32 & 3) == 0, "bad int8 gather");
    const int vec = ((uintptr_t)to_f32 & 15) == 0 ? 1 : 0;
    if (D >= RI_WG_ROW_CODES)
        hipLaunchKernelGGL(k_fs_get_int8<256>, dim3(row_grid(njobs, 256)), dim3(256), 0, st, (const unsigned char*)from_i8, (float*)to_f32, D, src,
                           njobs, vec);
    else
        hipLaunchKernelGGL(k_fs_get_int8<64>, dim3(row_grid(njobs, 64)), dim3(256), 0, st, (const unsigned char*)from_i8, (float*)to_f32, D, src,
                           njobs, vec);
    return CIS_OK;
}

extern "C" int cis_rerank_select_int8_dev(const void* d_feats, int64_t n_feats, int D, const int64_t* d_map_keys, const int64_t* d_map_rows,
                                          int64_t map_cap, const void* d_q, int nq, const int64_t* d_ids, const double* d_adc, int L, int nb,
                                          int max_returned, int use_th, double near_dup_th, int64_t* d_out_ids, double* d_out_dists,
                                          int32_t* d_out_src, int32_t* d_n_kept, void* stream) {
    CIS_REQUIRE(n_feats >= 0 && D > 0 && nq >= 0 && L >= 0 && max_returned >= 0, "bad re-ranking arguments");
    CIS_REQUIRE(nb >= 0 && nb <= L, "rerank_nb must be in [0, L] (nb = %d, L = %d)", nb, L);
    CIS_REQUIRE(nb <= RR_MAX_NB, "the device re-ranking holds at most %d results per query (nb = %d): use the host rerank", RR_MAX_NB, nb);
    CIS_REQUIRE((d_map_keys == nullptr) == (d_map_rows == nullptr), "the id map needs both of its arrays (or neither: row = id)");
    CIS_REQUIRE(!d_map_keys || (pow2(map_cap) && map_cap <= IDMAP_MAX_CAP), "the id map's capacity must be a power of two (cap = %lld)",
                (long long)map_cap);
    CIS_TRY(int8_operands_ok(d_feats, D, d_q));
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
    RI_DISPATCH(k_rerank_select_int8);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_rerank_packed_int8_dev(const void* d_feats, int64_t n_feats, int D, const int64_t* d_map_keys, const int64_t* d_map_rows,
                                          int64_t map_cap, const void* d_q, int nq, const cis_hit* d_recs, int64_t n_rec, const int64_t* d_off,
                                          const int32_t* d_cnt, int nb, double* d_true, void* stream) {
    CIS_REQUIRE(n_feats >= 0 && D > 0 && nq >= 0 && n_rec >= 0, "bad re-ranking arguments");
    CIS_REQUIRE(nb >= 0 && nb <= RR_MAX_NB, "the device re-ranking holds at most %d results per query (nb = %d): use the host rerank", RR_MAX_NB, nb);
    CIS_REQUIRE((d_map_keys == nullptr) == (d_map_rows == nullptr), "the id map needs both of its arrays (or neither: row = id)");
    CIS_REQUIRE(!d_map_keys || (pow2(map_cap) && map_cap <= IDMAP_MAX_CAP), "the id map's capacity must be a power of two (cap = %lld)",
                (long long)map_cap);
    CIS_TRY(int8_operands_ok(d_feats, D, d_q));
    if (nq == 0 || n_rec == 0) return CIS_OK;
    CIS_REQUIRE(d_q && d_recs && d_off && d_cnt && d_true && (n_feats == 0 || d_feats), "NULL buffer");
    CIS_TRY(cis_lazy_init());
    PackedArgs a;
    a.feats = d_feats; a.n_feats = n_feats; a.map_keys = d_map_keys; a.map_rows = d_map_rows; a.map_cap = map_cap;
    a.Q = d_q; a.recs = d_recs; a.off = d_off; a.cnt = d_cnt; a.n_rec = n_rec; a.true_d = d_true; a.D = D; a.nb = nb;
    const bool staged = (size_t)D * sizeof(float) <= (size_t)RR_STAGE_BYTES;
    const dim3 g((unsigned)nq), b(256);
    hipStream_t st = (hipStream_t)stream;
    RI_DISPATCH(k_rerank_packed_int8);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}
