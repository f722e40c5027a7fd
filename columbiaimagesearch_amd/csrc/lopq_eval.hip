// Exact k nearest neighbours: the ground truth of lopq.eval (lopq/lopq/eval.py:7-38 is scipy's cdist plus an argmin / argsort
// per row) and ResidentFeatures.search_exact.
//
// The VALUE that ranks is scipy's: both operands promoted to float64, s = 0, then for i ascending t = x[i] - y[i]; s = s + t*t
// with every operation rounded on its own, and dist = sqrt(s).  Rows order by (dist, global index) -- np.argmin's first minimum.
// Note that the ranking key is the square-rooted value: two different s may share one sqrt(s), and then the lower index wins.
//
// Default path: prefilter on the float32 matrix cores, exact re-check of what survives (the scheme of k_coarse_mfma32 /
// k_fine_mfma in lopq_model.hip).
//   1. k_surface<MIN>: st(q, j) = fl32(|y_j|^2 - 2 x_q . y_j) from v_mfma_f32_32x32x2_f32, tiled 128 rows x 64 queries per
//      workgroup, never stored: every lane keeps the minimum of each of its 16 result registers, so the rows of a chunk fall
//      into G = 128 S disjoint groups per query (S = row splits of the grid) whose minima are written out.
//   2. k_select: v_k = the k-th smallest group minimum.  k DIFFERENT rows have st <= v_k.
//   3. k_surface<EMIT>: the same products again; rows with st <= v_k + 2 E are appended to the query's candidate list.
//   4. k_finalize: candidates (and, when accumulating, the caller's current entries) are re-scored with the exact chain and
//      ranked by (dist, index).
// The bound.  Let D(q, j) = |x - y|^2 over the reals, s(q, j) = D - |x|^2 = |y|^2 - 2 x.y, u = 2^-24, n = |x| + max_j |y_j|.
//   - inputs rounded to float32: |x^.y^ - x.y| <= (2u + u^2) |x||y|; |y|^2 is summed in float64 and rounded once: u |y|^2;
//   - a float32 dot product of length d, whatever the order and whether or not the matrix core fuses: <= d u |x^||y^|;
//   - the final fma(-2, dot, |y|^2): u (|y|^2 + 2|x||y|);
//   so |st - s| <= (d + 4) u (|y|^2 + 2 |x||y|) <= (d + 4) u n^2.  float32 flushes results below 2^-126 to zero: every one of
//   the 2d + 2 operations and the 2d + 1 conversions adds at most 2^-126 (1 + n) absolute.  The exact chain is within
//   (d + 2) 2^-53 D <= (d + 2) 2^-53 n^2 of D, and sqrt can merge two chain values at most 2^-51 apart relatively.
//   E = (d + 16) (2^-24 n^2 + 2^-124 (1 + n)) covers all of it with room to spare (evaluated in float64; the threshold is
//   rounded UP to float32).
//   Claim: a row j in the final top k has st(j) <= v_k + 2E.  k different rows have st <= v_k, hence chain value <= v_k + |x|^2
//   + E' (E' the part of E up to the chain); j ranks among the first k by (sqrt(chain), index), so its chain value cannot exceed
//   the k-th smallest chain value by more than the sqrt merge slack, i.e. s(j) <= v_k + E, and st(j) <= s(j) + E.
//   NaN anywhere makes a comparison false, and every test below is written so that "false" KEEPS the row.
// A query whose list overflows (the bound cannot separate: thousands of identical rows) is flagged and handled by the exact-only
// path: k_exact, one workgroup per flagged query, one row per lane with the sequential chain, survivors of a running
// (dist, index) threshold collected and compacted by a lexicographic rank.  Small chunks (fewer than 128 S_min rows) and
// cis_exact_knn_set_mode(1) take that path for every query.
#include <algorithm>
#include <mutex>

#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KNN_MAX_K = 1024;
constexpr int BM = 128, BN = 64, KC = 32, LDP = KC + 1;  // workgroup tile (rows x queries), dims per LDS stage, LDS row pitch
constexpr int64_t ROW_CHUNK = (int64_t)1 << 24;          // rows per internal pass (candidate rows stay far below 2^31)
constexpr int Q_CHUNK = 8192;                            // queries per internal pass (bounds the workspaces)

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000LL); }

// (da, ia) < (db, ib) with NaN after every number
__device__ __forceinline__ bool lex_less(double da, int64_t ia, double db, int64_t ib) {
    const bool na = da != da, nb = db != db;
    if (na || nb) return (!na && nb) || (na && nb && ia < ib);
    return da < db || (da == db && ia < ib);
}

// scipy's cdist value: sequential float64 chain, no fused multiply-add (the file is compiled with -ffp-contract=off), then sqrt.
template <typename TD, typename TQ>
__device__ __forceinline__ double exact_dist(const TQ* __restrict__ x, const TD* __restrict__ y, int d) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = 0; i < d; ++i) {
        const double t = (double)x[i] - (double)y[i];
        const double p = t * t;
        s = s + p;
    }
    return __dsqrt_rn(s);
}

__global__ __launch_bounds__(256) void k_knn_pad(int64_t* __restrict__ idx, double* __restrict__ dist, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        idx[i] = -1;
        dist[i] = nan64();
    }
}

// |row|^2 in float64, one wave per row: out64 (queries) or out32 + the maximum over rows as ordered bits (data)
template <typename T>
__global__ __launch_bounds__(256) void k_knn_norms(const T* __restrict__ X, int64_t n, int d, double* __restrict__ out64,
                                                   float* __restrict__ out32, unsigned long long* __restrict__ max_bits) {
    const int lane = threadIdx.x & 63;
    unsigned long long best = 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
        const T* x = X + r * d;
        double acc = 0.0;
        for (int i = lane; i < d; i += 64) {
            const double v = (double)x[i];
            acc = acc + v * v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
        if (lane == 0) {
            if (out64) out64[r] = acc;
            if (out32) out32[r] = (float)acc;
        }
        const unsigned long long b = (unsigned long long)__double_as_longlong(acc);  // acc >= 0 or NaN: NaN bits order above inf
        best = b > best ? b : best;
    }
    if (max_bits && lane == 0 && best) atomicMax(max_bits, best);
}

// st(q, j) on the matrix cores.  A operand = data rows (lane l: row l & 31, k = l >> 5), B operand = queries (lane l: k = l >> 5,
// query l & 31); result register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of query l & 31.  The four waves of a
// workgroup own 32 rows each and share the 64 queries.  The next stage's operands are fetched into registers while the matrix
// cores work on the current one.
template <typename TD, typename TQ, int EMIT>
__global__ __launch_bounds__(256) void k_knn_surface(const TD* __restrict__ data, int m2, int d, const TQ* __restrict__ Q, int m1,
                                                     const float* __restrict__ ny32, int S, float* __restrict__ gmin,
                                                     const float* __restrict__ thr, int* __restrict__ cnt,
                                                     int64_t* __restrict__ cand, int W, int cap, int64_t base) {
    __shared__ float sA[BM * LDP];
    __shared__ float sB[BN * LDP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * BN, split = blockIdx.y;
    const int ntiles = (m2 + BM - 1) / BM, nks = (d + KC - 1) / KC;
    const int my_tiles = split < ntiles ? (ntiles - split + S - 1) / S : 0;
    const int n_stages = my_tiles * nks;
    const int lr = tid >> 5, lc = tid & 31;  // this thread's row (+ 8 i) and column of a stage

    float ra[16], rb[8];
    auto fetch = [&](int st) {
        const int tile = split + (st / nks) * S, k = (st % nks) * KC + lc;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = tile * BM + lr + 8 * i;
            ra[i] = (row < m2 && k < d) ? (float)data[(int64_t)row * d + k] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = q0 + lr + 8 * i;
            rb[i] = (q < m1 && k < d) ? (float)Q[(int64_t)q * d + k] : 0.f;
        }
    };

    float mins[2][16];
    float tq[2];
    bool qok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = q0 + j * 32 + (lane & 31);
        qok[j] = q < m1;
        tq[j] = (EMIT && qok[j]) ? thr[q] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) mins[j][r] = __builtin_inff();
    }
    f32x16 acc[2];
    if (n_stages > 0) fetch(0);
    for (int st = 0; st < n_stages; ++st) {
        const int ks = st % nks;
        __syncthreads();  // the previous stage's operands have been read
#pragma unroll
        for (int i = 0; i < 16; ++i) sA[(lr + 8 * i) * LDP + lc] = ra[i];
#pragma unroll
        for (int i = 0; i < 8; ++i) sB[(lr + 8 * i) * LDP + lc] = rb[i];
        __syncthreads();
        if (st + 1 < n_stages) fetch(st + 1);
        if (ks == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        }
        const float* pa = sA + (wave * 32 + (lane & 31)) * LDP + (lane >> 5);
        const float* pb = sB + (lane & 31) * LDP + (lane >> 5);
#pragma unroll
        for (int s = 0; s < KC / 2; ++s) {
            const float av = pa[2 * s];
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, pb[j * 32 * LDP + 2 * s], acc[j], 0, 0, 0);
        }
        if (ks == nks - 1) {
            const int rowb = (split + (st / nks) * S) * BM + wave * 32 + 4 * (lane >> 5);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rowb + (r & 3) + 8 * (r >> 2);
                const bool rok = row < m2;
                const float nyv = rok ? ny32[row] : __builtin_inff();
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float sv = fmaf(-2.f, acc[j][r], nyv);
                    if (!EMIT) {
                        mins[j][r] = fminf(mins[j][r], sv);  // (a NaN is dropped: the minima only have to be attained by real rows)
                    } else if (rok && qok[j] && !(sv > tq[j])) {
                        const int q = q0 + j * 32 + (lane & 31);
                        const int pos = atomicAdd(&cnt[q], 1);
                        if (pos < cap) cand[(int64_t)q * W + pos] = base + row;
                    }
                }
            }
        }
    }
    if (!EMIT) {
        const int G = S * 128;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!qok[j]) continue;
            float* g = gmin + (int64_t)(q0 + j * 32 + (lane & 31)) * G + ((split * 4 + wave) * 2 + (lane >> 5)) * 16;
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = mins[j][r];
        }
    }
}

// thr[q] = float32 round-up of v_k + 2E: v_k the k-th smallest of the query's G group minima (G >= 2k, no NaN among them)
__global__ __launch_bounds__(256) void k_knn_select(const float* __restrict__ gmin, int G, int k, int d, const double* __restrict__ xn2,
                                                    const unsigned long long* __restrict__ ymax2_bits, float* __restrict__ thr) {
    extern __shared__ float sv[];
    const int q = blockIdx.x;
    for (int i = threadIdx.x; i < G; i += 256) sv[i] = gmin[(int64_t)q * G + i];
    __syncthreads();
    for (int i = threadIdx.x; i < G; i += 256) {
        const float vi = sv[i];
        int c = 0;
        for (int j = 0; j < G; ++j) {
            const float vj = sv[j];
            c += (vj < vi || (vj == vi && j < i)) ? 1 : 0;
        }
        if (c == k - 1) {
            const double n = __dsqrt_rn(xn2[q]) + __dsqrt_rn(__longlong_as_double((long long)*ymax2_bits));
            const double E = (double)(d + 16) * (0x1p-24 * n * n + 0x1p-124 * (1.0 + n));
            // n < 2^60 keeps every float32 intermediate finite (|x||y|, |y|^2 <= n^2 < 2^120); beyond that nothing is discarded
            const double T = n < 0x1p60 ? (double)vi + 2.0 * E : nan64();
            float f = (float)T;
            if ((double)f < T) f = nextafterf(f, __builtin_inff());
            thr[q] = f;  // NaN (a NaN or infinite input): every row is kept and the query overflows into the exact path
        }
    }
}

// Ranks buf[0, n) by (dist, index) and writes the first k to the output row, padding the rest.  All threads of the workgroup.
__device__ __forceinline__ void rank_and_write(const double* bd, const int64_t* bi, int n, int k, int64_t* oi, double* od) {
    for (int i = threadIdx.x; i < n; i += 256) {
        const double di = bd[i];
        const int64_t ii = bi[i];
        int c = 0;
        for (int j = 0; j < n && c < k; ++j) c += (j != i && (lex_less(bd[j], bi[j], di, ii) || (bd[j] == di && bi[j] == ii && j < i))) ? 1 : 0;
        if (c < k) {
            oi[c] = ii;
            od[c] = di;
        }
    }
    for (int r = n + threadIdx.x; r < k; r += 256) {
        oi[r] = -1;
        od[r] = nan64();
    }
}

// Moves the caller's current entries (index >= 0) behind buf[n0); returns the new count.  Ends with a barrier.
__device__ __forceinline__ int take_current(const int64_t* oi, const double* od, int k, double* bd, int64_t* bi, int n0, int* s_n) {
    if (threadIdx.x == 0) *s_n = n0;
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += 256) {
        const int64_t id = oi[j];
        if (id >= 0) {
            const int pos = atomicAdd(s_n, 1);
            bi[pos] = id;
            bd[pos] = od[j];
        }
    }
    __syncthreads();
    return *s_n;
}

template <typename TD, typename TQ>
__global__ __launch_bounds__(256) void k_knn_finalize(const TD* __restrict__ data, int d, const TQ* __restrict__ Q, int k, int64_t base,
                                                      const int* __restrict__ cnt, int cap, int W, int64_t* __restrict__ cand,
                                                      double* __restrict__ cdist, int* __restrict__ flag, int64_t* __restrict__ out_idx,
                                                      double* __restrict__ out_dist) {
    __shared__ int s_n;
    const int q = blockIdx.x;
    const int n = cnt[q];
    if (n > cap) {  // the bound could not separate the rows: the exact-only kernel answers this query
        if (threadIdx.x == 0) flag[q] = 1;
        return;
    }
    int64_t* bi = cand + (int64_t)q * W;
    double* bd = cdist + (int64_t)q * W;
    for (int i = threadIdx.x; i < n; i += 256) bd[i] = exact_dist(Q + (int64_t)q * d, data + (bi[i] - base) * d, d);
    const int total = take_current(out_idx + (int64_t)q * k, out_dist + (int64_t)q * k, k, bd, bi, n, &s_n);
    rank_and_write(bd, bi, total, k, out_idx + (int64_t)q * k, out_dist + (int64_t)q * k);
}

// The exact-only path: one workgroup per flagged query, one row per lane and step.  Rows below the running threshold (the k-th
// entry of the last compaction) are collected in buf [W]; when fewer than 256 free places are left the list is ranked, its first
// k entries kept (through the output row, which is free: the caller's entries were moved into buf first).
template <typename TD, typename TQ>
__global__ __launch_bounds__(256) void k_knn_exact(const TD* __restrict__ data, int m2, int d, const TQ* __restrict__ Q, int k, int64_t base,
                                                   const int* __restrict__ flag, int W, int64_t* __restrict__ cand, double* __restrict__ cdist,
                                                   int64_t* __restrict__ out_idx, double* __restrict__ out_dist) {
    __shared__ int s_n;
    const int q = blockIdx.x;
    if (!flag[q]) return;
    int64_t* bi = cand + (int64_t)q * W;
    double* bd = cdist + (int64_t)q * W;
    int64_t* oi = out_idx + (int64_t)q * k;
    double* od = out_dist + (int64_t)q * k;
    const TQ* x = Q + (int64_t)q * d;
    int n = take_current(oi, od, k, bd, bi, 0, &s_n);
    bool has_thr = false;
    double thr_d = 0.0;
    int64_t thr_i = 0;
    for (int row0 = 0; row0 < m2; row0 += 256) {
        const int row = row0 + threadIdx.x;
        if (row < m2) {
            const double dist = exact_dist(x, data + (int64_t)row * d, d);
            const int64_t gi = base + row;
            if (!has_thr || lex_less(dist, gi, thr_d, thr_i)) {
                const int pos = atomicAdd(&s_n, 1);
                bi[pos] = gi;
                bd[pos] = dist;
            }
        }
        __syncthreads();
        n = s_n;
        __syncthreads();  // (nobody appends before everybody has read the count)
        if (n > W - 256 && row0 + 256 < m2) {  // (uniform: every thread read the same count)
            rank_and_write(bd, bi, n, k, oi, od);
            __syncthreads();
            n = n < k ? n : k;
            for (int i = threadIdx.x; i < n; i += 256) {
                bi[i] = oi[i];
                bd[i] = od[i];
            }
            if (n == k) {
                has_thr = true;
                thr_d = od[k - 1];
                thr_i = oi[k - 1];
            }
            __syncthreads();
            if (threadIdx.x == 0) s_n = n;
            __syncthreads();
        }
    }
    rank_and_write(bd, bi, n, k, oi, od);
}

struct KnnWs {
    std::mutex mu;
    DevBuf cand, cdist, cnt, flag, thr, xn2, ny32, ymax, gmin;
};
KnnWs g_ws;
int g_mode = 0;  // 0: prefilter + exact re-check, 1: the exact-only path for every query
int g_last_m1 = 0;        // the last internal pass: its queries, and whether the prefilter ran (cis_exact_knn_stats)
bool g_last_fast = false;

template <typename TD, typename TQ>
int knn_chunk(const TD* data, int m2, int d, const TQ* Q, int m1, int k, int64_t base, int64_t* d_idx, double* d_dist, hipStream_t st) {
    KnnWs& w = g_ws;
    const int W = 4 * k + 512, cap = W - k;
    CIS_TRY(w.cand.reserve((size_t)m1 * W * 8));
    CIS_TRY(w.cdist.reserve((size_t)m1 * W * 8));
    CIS_TRY(w.flag.reserve((size_t)m1 * 4));
    const int ntiles = (int)ceil_div(m2, BM), nqt = (int)ceil_div(m1, BN);
    const int s_min = (int)std::max<int64_t>(2, ceil_div(2 * k, 128));  // G = 128 S >= 2k groups, and more than one tile
    const bool fast = g_mode == 0 && ntiles >= s_min;
    g_last_m1 = m1;
    g_last_fast = fast;
    if (fast) {
        const int S = std::min(ntiles, std::max(s_min, std::min(32, (int)ceil_div(512, nqt))));
        const int G = S * 128;
        CIS_TRY(w.cnt.reserve((size_t)m1 * 4));
        CIS_TRY(w.thr.reserve((size_t)m1 * 4));
        CIS_TRY(w.xn2.reserve((size_t)m1 * 8));
        CIS_TRY(w.ny32.reserve((size_t)m2 * 4));
        CIS_TRY(w.ymax.reserve(8));
        CIS_TRY(w.gmin.reserve((size_t)m1 * G * 4));
        CIS_CHECK_HIP(hipMemsetAsync(w.cnt.p, 0, (size_t)m1 * 4, st));
        CIS_CHECK_HIP(hipMemsetAsync(w.flag.p, 0, (size_t)m1 * 4, st));
        CIS_CHECK_HIP(hipMemsetAsync(w.ymax.p, 0, 8, st));
        hipLaunchKernelGGL(k_knn_norms<TD>, dim3((unsigned)std::min<int64_t>(ceil_div(m2, 4), 4096)), dim3(256), 0, st, data, (int64_t)m2, d,
                           (double*)nullptr, w.ny32.as<float>(), w.ymax.as<unsigned long long>());
        hipLaunchKernelGGL(k_knn_norms<TQ>, dim3((unsigned)std::min<int64_t>(ceil_div(m1, 4), 4096)), dim3(256), 0, st, Q, (int64_t)m1, d,
                           w.xn2.as<double>(), (float*)nullptr, (unsigned long long*)nullptr);
        const dim3 grid((unsigned)nqt, (unsigned)S);
        hipLaunchKernelGGL((k_knn_surface<TD, TQ, 0>), grid, dim3(256), 0, st, data, m2, d, Q, m1, w.ny32.as<float>(), S, w.gmin.as<float>(),
                           (const float*)nullptr, (int*)nullptr, (int64_t*)nullptr, W, cap, base);
        hipLaunchKernelGGL(k_knn_select, dim3((unsigned)m1), dim3(256), (size_t)G * 4, st, w.gmin.as<float>(), G, k, d, w.xn2.as<double>(),
                           w.ymax.as<unsigned long long>(), w.thr.as<float>());
        hipLaunchKernelGGL((k_knn_surface<TD, TQ, 1>), grid, dim3(256), 0, st, data, m2, d, Q, m1, w.ny32.as<float>(), S, (float*)nullptr,
                           w.thr.as<float>(), w.cnt.as<int>(), w.cand.as<int64_t>(), W, cap, base);
        hipLaunchKernelGGL((k_knn_finalize<TD, TQ>), dim3((unsigned)m1), dim3(256), 0, st, data, d, Q, k, base, w.cnt.as<int>(), cap, W,
                           w.cand.as<int64_t>(), w.cdist.as<double>(), w.flag.as<int>(), d_idx, d_dist);
    } else {
        CIS_CHECK_HIP(hipMemsetAsync(w.flag.p, 0xff, (size_t)m1 * 4, st));
    }
    hipLaunchKernelGGL((k_knn_exact<TD, TQ>), dim3((unsigned)m1), dim3(256), 0, st, data, m2, d, Q, k, base, w.flag.as<int>(), W,
                       w.cand.as<int64_t>(), w.cdist.as<double>(), d_idx, d_dist);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

template <typename TD, typename TQ>
int knn_all(const TD* data, int64_t m2, int d, const TQ* Q, int m1, int k, int64_t base, int64_t* d_idx, double* d_dist, hipStream_t st) {
    for (int q0 = 0; q0 < m1; q0 += Q_CHUNK) {
        const int mq = std::min(Q_CHUNK, m1 - q0);
        for (int64_t r0 = 0; r0 < m2; r0 += ROW_CHUNK) {
            const int mr = (int)std::min<int64_t>(ROW_CHUNK, m2 - r0);
            CIS_TRY(knn_chunk(data + r0 * d, mr, d, Q + (int64_t)q0 * d, mq, k, base + r0, d_idx + (int64_t)q0 * k, d_dist + (int64_t)q0 * k, st));
        }
    }
    return CIS_OK;
}

int knn_validate(int data_dtype, int64_t m2, int d, int q_dtype, int m1, int k) {
    CIS_REQUIRE(data_dtype == CIS_F32 || data_dtype == CIS_F64, "data_dtype must be 4 (float32) or 8 (float64), got %d", data_dtype);
    CIS_REQUIRE(q_dtype == CIS_F32 || q_dtype == CIS_F64, "q_dtype must be 4 (float32) or 8 (float64), got %d", q_dtype);
    CIS_REQUIRE(m2 >= 0 && m1 >= 0 && d > 0 && k >= 1, "bad exact k-NN arguments (m1 = %d, m2 = %lld, d = %d, k = %d)", m1, (long long)m2, d, k);
    if (k > KNN_MAX_K) {
        cis_set_error("exact k-NN supports k <= %d, got %d", KNN_MAX_K, k);
        return CIS_EUNSUPPORTED;
    }
    return CIS_OK;
}

}  // namespace

extern "C" int cis_exact_knn_set_mode(int mode) {
    CIS_REQUIRE(mode == 0 || mode == 1, "exact k-NN mode must be 0 (prefilter + exact re-check) or 1 (exact only), got %d", mode);
    std::lock_guard<std::mutex> lock(g_ws.mu);
    g_mode = mode;
    return CIS_OK;
}

extern "C" int cis_exact_knn_stats(int64_t stats[3]) {
    CIS_REQUIRE(stats, "NULL stats");
    std::lock_guard<std::mutex> lock(g_ws.mu);
    stats[0] = g_last_m1;
    stats[1] = stats[2] = 0;
    if (g_last_m1 == 0) return CIS_OK;
    CIS_TRY(cis_lazy_init());
    CIS_CHECK_HIP(hipDeviceSynchronize());
    std::vector<int> flag((size_t)g_last_m1), cnt((size_t)g_last_m1, 0);
    CIS_CHECK_HIP(hipMemcpy(flag.data(), g_ws.flag.p, flag.size() * 4, hipMemcpyDeviceToHost));
    if (g_last_fast) CIS_CHECK_HIP(hipMemcpy(cnt.data(), g_ws.cnt.p, cnt.size() * 4, hipMemcpyDeviceToHost));
    for (int q = 0; q < g_last_m1; ++q) {
        stats[1] += flag[q] != 0;
        stats[2] += flag[q] != 0 ? 0 : cnt[q];
    }
    return CIS_OK;
}

extern "C" int cis_exact_knn_dev(const void* d_data, int data_dtype, int64_t m2, int d, const void* d_q, int q_dtype, int m1, int k,
                                 int64_t base, int accumulate, int64_t* d_idx, double* d_dist, void* stream) {
    CIS_TRY(knn_validate(data_dtype, m2, d, q_dtype, m1, k));
    CIS_REQUIRE(m1 == 0 || (d_q && d_idx && d_dist), "NULL query or result buffer");
    CIS_REQUIRE(m2 == 0 || d_data, "NULL data buffer");
    CIS_TRY(cis_lazy_init());
    if (m1 == 0) return CIS_OK;
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g_ws.mu);
    if (!accumulate) {
        const int64_t n = (int64_t)m1 * k;
        hipLaunchKernelGGL(k_knn_pad, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, d_idx, d_dist, n);
        CIS_CHECK_HIP(hipGetLastError());
    }
    if (m2 == 0) return CIS_OK;
    if (data_dtype == CIS_F32 && q_dtype == CIS_F32) return knn_all((const float*)d_data, m2, d, (const float*)d_q, m1, k, base, d_idx, d_dist, st);
    if (data_dtype == CIS_F32) return knn_all((const float*)d_data, m2, d, (const double*)d_q, m1, k, base, d_idx, d_dist, st);
    if (q_dtype == CIS_F32) return knn_all((const double*)d_data, m2, d, (const float*)d_q, m1, k, base, d_idx, d_dist, st);
    return knn_all((const double*)d_data, m2, d, (const double*)d_q, m1, k, base, d_idx, d_dist, st);
}

extern "C" int cis_exact_knn(const void* data, int data_dtype, int64_t m2, int d, const void* q, int q_dtype, int m1, int k, int64_t base,
                             int accumulate, int64_t* idx, double* dist) {
    CIS_TRY(knn_validate(data_dtype, m2, d, q_dtype, m1, k));
    CIS_REQUIRE(m1 == 0 || (q && idx && dist), "NULL query or result buffer");
    CIS_REQUIRE(m2 == 0 || data, "NULL data buffer");
    CIS_TRY(cis_lazy_init());
    if (m1 == 0) return CIS_OK;
    DevBuf b_data, b_q, b_idx, b_dist;
    struct Free {
        DevBuf *a, *b, *c, *d;
        ~Free() { a->release(); b->release(); c->release(); d->release(); }
    } guard{&b_data, &b_q, &b_idx, &b_dist};
    const size_t n_out = (size_t)m1 * k;
    CIS_TRY(b_data.reserve(std::max<size_t>((size_t)m2 * d * data_dtype, 8)));
    CIS_TRY(b_q.reserve((size_t)m1 * d * q_dtype));
    CIS_TRY(b_idx.reserve(n_out * 8));
    CIS_TRY(b_dist.reserve(n_out * 8));
    if (m2 > 0) CIS_CHECK_HIP(hipMemcpy(b_data.p, data, (size_t)m2 * d * data_dtype, hipMemcpyHostToDevice));
    CIS_CHECK_HIP(hipMemcpy(b_q.p, q, (size_t)m1 * d * q_dtype, hipMemcpyHostToDevice));
    if (accumulate) {
        CIS_CHECK_HIP(hipMemcpy(b_idx.p, idx, n_out * 8, hipMemcpyHostToDevice));
        CIS_CHECK_HIP(hipMemcpy(b_dist.p, dist, n_out * 8, hipMemcpyHostToDevice));
    }
    CIS_TRY(cis_exact_knn_dev(b_data.p, data_dtype, m2, d, b_q.p, q_dtype, m1, k, base, accumulate, b_idx.as<int64_t>(), b_dist.as<double>(), nullptr));
    CIS_CHECK_HIP(hipStreamSynchronize(nullptr));
    CIS_CHECK_HIP(hipMemcpy(idx, b_idx.p, n_out * 8, hipMemcpyDeviceToHost));
    CIS_CHECK_HIP(hipMemcpy(dist, b_dist.p, n_out * 8, hipMemcpyDeviceToHost));
    return CIS_OK;
}
