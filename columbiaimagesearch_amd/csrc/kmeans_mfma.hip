// Lloyd iterations on device data for codebooks of any size (cis_kmeans_dev): the counterpart of kmeans.hip without its LDS limit
// (k * d <= 7680) and without its host round trips.  float32 arithmetic; judged by distortion like cis_kmeans.
//
//   k_kmd_cnorm:      |c|^2 per centroid, summed in float64 and rounded once, one wave per centroid; once per iteration.
//   k_kmd_assign:     the hot path.  st(x, c) = fl32(|c|^2 - 2 x.c) from v_mfma_f32_32x32x2_f32, never stored.  A workgroup owns 128
//                     points (32 per wave, the A operand) and walks ALL centroids in tiles of 64 (the B operand, two accumulators),
//                     staged through LDS 32 dimensions at a time with a padded pitch; the next stage is fetched into registers
//                     while the matrix cores work on the current one.  For d <= 128 a wave keeps its points' operand values in
//                     registers for the whole walk (d / 2 per lane), so a stage moves only the 64 x 32 centroid block (8 KB for
//                     0.5 MFLOP; the codebook stays in L2); beyond that the point values of a stage are fetched per stage.  Result
//                     register r of lane l is point (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the wave, centroid l & 31 of the
//                     accumulator: every lane keeps a running (score, index) minimum per register, and the 32 lanes that share a
//                     point are reduced once, at the end.  Every comparison is on the (score, index) pair: first minimum.
//                     Loads past the last point or centroid are clamped to the last row instead of predicated (a predicate per
//                     load costs registers); a padded centroid carries |c|^2 = +inf and an index >= k and never wins, a padded
//                     point is never written, padded dimensions are zeros on both sides.  A persistent grid strides over the
//                     point tiles.
//   k_kmd_accumulate: sums[assign[r]] += x_r with one global float atomic per element (64 consecutive elements per wave
//                     instruction: whole 256-byte row segments at d >= 64) and counts[assign[r]] += 1.  n * d * 4 bytes of atomics
//                     per iteration, a few per cent of the assignment's time at the sizes this file is for.
//   k_kmd_update:     C = sum / (float)count where count > 0; an empty cluster keeps its bytes.
//   k_kmd_inertia:    for the winner only, acc = fmaf(x[i] - c[i], x[i] - c[i], acc) for i ascending, one thread per point, summed
//                     in double: the direct form, without the cancellation of |c|^2 - 2 x.c.  Last pass only.
//
// The expanded form is not the direct form: with u = 2^-24 and r = |x| + max_c |c|, |st - s| <= (d + 4) u r^2 =: E (the derivation is
// at the top of lopq_eval.hip; gfx950's float32 MFMA is an fmaf chain, no extra term), so the chosen centroid's true squared distance
// is at most D_min + 2 E.  On small-integer data every product, partial sum, |c|^2 and score is an integer below 2^24 and the result
// is exact.
#include <algorithm>
#include <mutex>

#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PM = 128, CN = 64, KC = 32, LDP = KC + 1;  // points and centroids per workgroup tile, dims per LDS stage, LDS row pitch
constexpr int RES_STAGES = 4;                            // d <= 32 * RES_STAGES: the points' operand stays in registers
constexpr int MAX_GRID = 2048;                           // persistent workgroups of k_kmd_assign (8 per CU)
constexpr int64_t KMD_MAX_N = ((int64_t)1 << 31) - 256;  // int32 assignments, and n + PM stays an int
constexpr int64_t KMD_MAX_KD = (int64_t)1 << 30;         // k * d: 32-bit element indices of the [k][d] sums; k + CN and d + KC stay ints

// (sa, ia) < (sb, ib); a NaN score never wins
__device__ __forceinline__ bool pair_less(float sa, int ia, float sb, int ib) { return sa < sb || (sa == sb && ia < ib); }

__global__ __launch_bounds__(256) void k_kmd_cnorm(const float* __restrict__ C, int k, int d, float* __restrict__ cn) {
    const int lane = threadIdx.x & 63;
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < k; c += gridDim.x * 4) {
        const float* y = C + (int64_t)c * d;
        double acc = 0.0;
        for (int i = lane; i < d; i += 64) {
            const double v = (double)y[i];
            acc = acc + v * v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
        if (lane == 0) cn[c] = (float)acc;
    }
}

// NKS > 0: d <= 32 NKS and the points' operand values live in registers; NKS == 0: any d, fetched per stage.
template <int NKS>
__global__ __launch_bounds__(256, 2) void k_kmd_assign(const float* __restrict__ X, int64_t n, int d, const float* __restrict__ C, int k,
                                                    const float* __restrict__ cn, int* __restrict__ assign) {
    __shared__ float sB[CN * LDP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = tid >> 5, lc = tid & 31;  // this thread's centroid row (+ 8 i) and column of a stage
    const int nks = NKS ? NKS : (d + KC - 1) / KC;
    const int nct = (k + CN - 1) / CN;
    const int n_stages = nct * nks;
    const int64_t n_tiles = (n + PM - 1) / PM;

    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // the point this lane feeds to the A operand; a lane past the end reads the last point, whose results nobody writes
        const float* xrow = X + std::min<int64_t>(tile * PM + wave * 32 + (lane & 31), n - 1) * d;

        float xa[NKS ? NKS : 1][16];  // resident operand: dims 32 ks + 2 s + (lane >> 5)
        if (NKS) {
#pragma unroll
            for (int ks = 0; ks < (NKS ? NKS : 1); ++ks)
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int dim = ks * KC + 2 * s + (lane >> 5);
                    xa[ks][s] = (ks + 1 < NKS || dim < d) ? xrow[dim] : 0.f;  // (only the last stage can be cut: d > 32 (NKS - 1))
                }
        }
        float ra[16], rb[8];  // the next stage's operands
        auto fetch = [&](int st) {
            const int c0 = (st / nks) * CN, k0 = (st % nks) * KC;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = std::min(c0 + lr + 8 * i, k - 1);  // a padded column repeats the last centroid; its |c|^2 is +inf
                rb[i] = k0 + lc < d ? C[(int64_t)c * d + k0 + lc] : 0.f;
            }
            if (!NKS) {
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const int dim = k0 + 2 * s + (lane >> 5);
                    ra[s] = dim < d ? xrow[dim] : 0.f;
                }
            }
        };

        float best[16];
        int bidx[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            best[r] = __builtin_inff();
            bidx[r] = 0x7fffffff;
        }
        f32x16 acc[2];
        float cnv[2];
        const float* pb = sB + (lane & 31) * LDP + (lane >> 5);

        // one stage: the staged centroid block into LDS, the next one into registers, 32 MFMAs
        auto stage = [&](int st, const float (&av)[16]) {
            __syncthreads();  // the previous stage's block has been read
#pragma unroll
            for (int i = 0; i < 8; ++i) sB[(lr + 8 * i) * LDP + lc] = rb[i];
            __syncthreads();
            if (st + 1 < n_stages) fetch(st + 1);
#pragma unroll
            for (int s = 0; s < KC / 2; ++s) {
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], pb[j * 32 * LDP + 2 * s], acc[j], 0, 0, 0);
            }
        };

        fetch(0);
        for (int ct = 0; ct < nct; ++ct) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = ct * CN + j * 32 + (lane & 31);
                cnv[j] = c < k ? cn[c] : __builtin_inff();
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            }
            if (NKS) {
#pragma unroll
                for (int ks = 0; ks < (NKS ? NKS : 1); ++ks) stage(ct * nks + ks, xa[ks]);
            } else {
                for (int ks = 0; ks < nks; ++ks) {
                    float xc[16];
#pragma unroll
                    for (int s = 0; s < 16; ++s) xc[s] = ra[s];
                    stage(ct * nks + ks, xc);
                }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = ct * CN + j * 32 + (lane & 31);  // (>= k on a padded column: its score is +inf and its index loses)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float sv = fmaf(-2.f, acc[j][r], cnv[j]);
                    if (pair_less(sv, c, best[r], bidx[r])) {
                        best[r] = sv;
                        bidx[r] = c;
                    }
                }
            }
        }
        // the 32 lanes of a half wave hold 32 different centroids' minima of the same 16 points
#pragma unroll
        for (int r = 0; r < 16; ++r) {
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) {
                const float os = __shfl_xor(best[r], o);
                const int oi = __shfl_xor(bidx[r], o);
                if (pair_less(os, oi, best[r], bidx[r])) {
                    best[r] = os;
                    bidx[r] = oi;
                }
            }
        }
        if ((lane & 31) == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = tile * PM + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < n) assign[row] = bidx[r] < k ? bidx[r] : 0;  // (no score compared below +inf -- NaN input: centroid 0, like cis_kmeans)
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_kmd_accumulate(const float* __restrict__ X, int64_t n, int d, const int* __restrict__ assign,
                                                        float* __restrict__ sums /* [k][d] */, int* __restrict__ counts /* [k] */) {
    const int64_t total = n * d;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / d;
        const int i = (int)(e - r * d);
        const int a = assign[r];
        atomicAdd(&sums[(int64_t)a * d + i], X[e]);
        if (i == 0) atomicAdd(&counts[a], 1);
    }
}

__global__ __launch_bounds__(256) void k_kmd_update(float* __restrict__ C, const float* __restrict__ sums, const int* __restrict__ counts,
                                                    int k, int d) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= k * d) return;
    const int c = counts[e / d];
    if (c > 0) C[e] = sums[e] / (float)c;
}

__global__ __launch_bounds__(256) void k_kmd_inertia(const float* __restrict__ X, int64_t n, int d, const float* __restrict__ C,
                                                     const int* __restrict__ assign, double* __restrict__ inertia) {
    double local = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        const float* x = X + r * d;
        const float* c = C + (int64_t)assign[r] * d;
        float acc = 0.f;
        for (int i = 0; i < d; ++i) {
            const float df = x[i] - c[i];
            acc = fmaf(df, df, acc);
        }
        local += (double)acc;
    }
    __shared__ double s_in[256];
    s_in[threadIdx.x] = local;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_in[threadIdx.x] += s_in[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(inertia, s_in[0]);
}

struct KmdWs {
    std::mutex mu;
    DevBuf sums, counts, cn, assign;
};
KmdWs g_kmd;

template <int NKS>
void launch_assign(unsigned grid, hipStream_t st, const float* X, int64_t n, int d, const float* C, int k, const float* cn, int* assign) {
    hipLaunchKernelGGL(k_kmd_assign<NKS>, dim3(grid), dim3(256), 0, st, X, n, d, C, k, cn, assign);
}

}  // namespace

extern "C" int cis_kmeans_dev(const float* d_X, int64_t n, int d, int k, int iters, float* d_centroids, int32_t* d_assign,
                              double* d_inertia, void* stream) {
    CIS_REQUIRE(d_X && d_centroids, "NULL d_X or d_centroids");
    CIS_REQUIRE(d > 0 && k > 0, "d and k must be >= 1 (d = %d, k = %d)", d, k);
    CIS_REQUIRE(n > 0, "n must be > 0 (k-means of no points)");
    CIS_REQUIRE(n <= KMD_MAX_N, "n must be <= 2^31 - 256 (assignments are int32), got %lld", (long long)n);
    CIS_REQUIRE(iters >= 0, "iters must be >= 0");
    CIS_REQUIRE((int64_t)k * d <= KMD_MAX_KD, "k * d must be <= 2^30 (32-bit element indices of the [k][d] sums), got %lld",
                (long long)k * d);
    CIS_TRY(cis_lazy_init());
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g_kmd.mu);
    KmdWs& w = g_kmd;
    const size_t kd = (size_t)k * d;
    CIS_TRY(w.sums.reserve(kd * 4));
    CIS_TRY(w.counts.reserve((size_t)k * 4));
    CIS_TRY(w.cn.reserve((size_t)k * 4));
    CIS_TRY(w.assign.reserve((size_t)n * 4));
    const unsigned g_assign = (unsigned)std::min<int64_t>(ceil_div(n, PM), MAX_GRID);
    const unsigned g_elem = (unsigned)std::min<int64_t>(ceil_div(n * d, 256), 16384);
    const unsigned g_rows = (unsigned)std::min<int64_t>(ceil_div(n, 256), 4096);
    for (int it = 0; it <= iters; ++it) {
        const bool last = it == iters;
        int* a = (last && d_assign) ? d_assign : w.assign.as<int>();
        hipLaunchKernelGGL(k_kmd_cnorm, dim3((unsigned)std::min<int64_t>(ceil_div(k, 4), 4096)), dim3(256), 0, st, d_centroids, k, d,
                           w.cn.as<float>());
        switch (d <= KC * RES_STAGES ? (d + KC - 1) / KC : 0) {
            case 1: launch_assign<1>(g_assign, st, d_X, n, d, d_centroids, k, w.cn.as<float>(), a); break;
            case 2: launch_assign<2>(g_assign, st, d_X, n, d, d_centroids, k, w.cn.as<float>(), a); break;
            case 3: launch_assign<3>(g_assign, st, d_X, n, d, d_centroids, k, w.cn.as<float>(), a); break;
            case 4: launch_assign<4>(g_assign, st, d_X, n, d, d_centroids, k, w.cn.as<float>(), a); break;
            default: launch_assign<0>(g_assign, st, d_X, n, d, d_centroids, k, w.cn.as<float>(), a); break;
        }
        if (!last) {
            CIS_CHECK_HIP(hipMemsetAsync(w.sums.p, 0, kd * 4, st));
            CIS_CHECK_HIP(hipMemsetAsync(w.counts.p, 0, (size_t)k * 4, st));
            hipLaunchKernelGGL(k_kmd_accumulate, dim3(g_elem), dim3(256), 0, st, d_X, n, d, a, w.sums.as<float>(), w.counts.as<int>());
            hipLaunchKernelGGL(k_kmd_update, dim3((unsigned)ceil_div((int64_t)kd, 256)), dim3(256), 0, st, d_centroids, w.sums.as<float>(),
                               w.counts.as<int>(), k, d);
        } else if (d_inertia) {
            CIS_CHECK_HIP(hipMemsetAsync(d_inertia, 0, sizeof(double), st));
            hipLaunchKernelGGL(k_kmd_inertia, dim3(g_rows), dim3(256), 0, st, d_X, n, d, d_centroids, a, d_inertia);
        }
    }
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}
