// LOPQ training on the GPU beyond the k-means steps: the accumulations the reference does
// with per-sample Python loops -- np.outer sums for the PCA covariance (lopq/lopq/model.py:263-267) and for the per-cluster
// residual covariances (:142-155), and the per-cluster projection of the residuals (:209-234) -- as float64 tiled products.
// The per-cluster eigendecompositions (V matrices of h x h) are csrc/sym_eig.hip's, and the *_dev entry points below chain the whole
// local-rotation stage on device pointers; only the PCA eigendecomposition (one D x D matrix) stays on the host (LAPACK).
//   k_gram_groups:    G[g] = sum_{r in group g} x_r x_r^T (upper 64x64 tiles, mirrored), s[g] = sum x_r; rows sorted by group
//   k_project_groups: y_r = (x_r - mu[g]) . R[g]^T for the rows of group g
//   k_residuals, k_group_cov, k_rotation_pack: the elementwise steps between them (residuals in group order, covariance and mean
//   from the sums, rotation rows from the eigenvectors and the bucket permutation)
// float64 fused multiply-adds, k-ascending inside a 16-row LDS stage; results differ from numpy's BLAS by summation order
// only (tests: 1e-12 relative).  Training is judged by distortion, not bit parity.
#include "common.h"

#include <algorithm>

// grid (tiles_j, tiles_i, groups); block 256 = 16 x 16 threads, 4 x 4 outputs each (64 x 64 tile); only tiles with
// j0 >= i0 compute, the mirror is written by the same block
__global__ __launch_bounds__(256) void k_gram_groups(const double* __restrict__ X, const int64_t* __restrict__ goff /* [groups+1] */,
                                                     int d, double* __restrict__ G /* [groups][d][d] */, double* __restrict__ S /* [groups][d] */) {
    const int g = blockIdx.z, i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    if (j0 < i0) return;
    __shared__ double sa[16][64 + 1], sb[16][64 + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int64_t r0 = goff[g], r1 = goff[g + 1];
    double acc[4][4], csum[4] = {0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (int64_t r = r0; r < r1; r += 16) {
        for (int e = threadIdx.x; e < 16 * 64; e += 256) {
            const int rr = e >> 6, c = e & 63;
            const bool on = r + rr < r1;
            sa[rr][c] = (on && i0 + c < d) ? X[(r + rr) * d + i0 + c] : 0.0;
            sb[rr][c] = (on && j0 + c < d) ? X[(r + rr) * d + j0 + c] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { a[q] = sa[rr][ty * 4 + q]; b[q] = sb[rr][tx * 4 + q]; }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(a[p], b[q], acc[p][q]);
            if (i0 == 0 && ty == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) csum[q] += b[q];
            }
        }
        __syncthreads();
    }
    double* Gg = G + (int64_t)g * d * d;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + ty * 4 + p, j = j0 + tx * 4 + q;
            if (i < d && j < d) {
                Gg[(int64_t)i * d + j] = acc[p][q];
                Gg[(int64_t)j * d + i] = acc[p][q];
            }
        }
    if (S && i0 == 0 && ty == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (j0 + tx * 4 + q < d) S[(int64_t)g * d + j0 + tx * 4 + q] = csum[q];
    }
}

// grid (tiles of 64 outputs, ceil(max rows of a group / 64), groups): y[r][o] = sum_k (x[r][k] - mu[g][k]) * R[g][o][k]
__global__ __launch_bounds__(256) void k_project_groups(const double* __restrict__ X, const int64_t* __restrict__ goff, int d,
                                                        const double* __restrict__ R /* [groups][d][d] */,
                                                        const double* __restrict__ mu /* [groups][d] */, double* __restrict__ Y,
                                                        int64_t tile_base /* first row tile of this launch (groups above 4M rows take several) */,
                                                        const int64_t* __restrict__ order /* or NULL: row r of X is written to row order[r] of Y */, int64_t y_rows) {
    const int g = blockIdx.z, o0 = blockIdx.x * 64;
    const int64_t r0 = goff[g] + (tile_base + (int64_t)blockIdx.y) * 64, r1 = goff[g + 1];
    if (r0 >= r1) return;
    __shared__ double sx[16][64 + 1], sr[16][64 + 1];  // [k][row], [k][output]
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    const double* Rg = R + (int64_t)g * d * d;
    const double* mg = mu + (int64_t)g * d;
    for (int k0 = 0; k0 < d; k0 += 16) {
        for (int e = threadIdx.x; e < 16 * 64; e += 256) {
            const int kk = e & 15, c = e >> 4;  // consecutive threads walk k: contiguous in X rows and R rows
            const bool kon = k0 + kk < d;
            sx[kk][c] = (kon && r0 + c < r1) ? X[(r0 + c) * d + k0 + kk] - mg[k0 + kk] : 0.0;
            sr[kk][c] = (kon && o0 + c < d) ? Rg[(int64_t)(o0 + c) * d + k0 + kk] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { a[q] = sx[kk][ty * 4 + q]; b[q] = sr[kk][tx * 4 + q]; }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fma(a[p], b[q], acc[p][q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t r = r0 + ty * 4 + p;
            const int o = o0 + tx * 4 + q;
            if (r < r1 && o < d) {
                const int64_t dst = order ? order[r] : r;
                if (dst >= 0 && dst < y_rows) Y[dst * d + o] = acc[p][q];  // (an order entry outside Y is dropped, never written)
            }
        }
}

// out[r] = (double)X[order[r]] - C[assign[order[r]]], r < rows: float32 minus float64 is exact in double, so these are numpy's
// residuals bit for bit.  A row or a group index outside its array gives a row of NaN, never an access outside.
__global__ __launch_bounds__(256) void k_residuals(const float* __restrict__ X, int64_t n, int d, const double* __restrict__ C, int groups,
                                                   const int32_t* __restrict__ assign, const int64_t* __restrict__ order, int64_t rows,
                                                   double* __restrict__ out) {
    const int64_t total = rows * d;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / d;
        const int c = (int)(e - r * d);
        const int64_t src = order[r];
        double v = __builtin_nan("");
        if (src >= 0 && src < n) {
            const int g = assign[src];
            if (g >= 0 && g < groups) v = (double)X[src * d + c] - C[(int64_t)g * d + c];
        }
        out[e] = v;
    }
}

// grid (groups), block 256: mu[g] = S[g] / n_g (zeros for an empty group), cov[g] = (G + G^T) / (2 (n_g - 1)) - mu mu^T, the
// expression of train.local_rotations operation by operation; the identity where n_g < d (the reference's fallback: its rotation
// is then a permutation of the axes)
__global__ __launch_bounds__(256) void k_group_cov(const double* __restrict__ G, const double* __restrict__ S, const int64_t* __restrict__ goff,
                                                   int d, double* __restrict__ cov, double* __restrict__ mu) {
    const int64_t g = blockIdx.x;
    const int64_t ng = goff[g + 1] - goff[g];
    const double* Gg = G + g * d * d;
    const double* Sg = S + g * d;
    for (int i = threadIdx.x; i < d; i += 256) mu[g * d + i] = ng > 0 ? Sg[i] / (double)ng : 0.0;
    const double den = 2.0 * (double)(ng - 1);
    for (int e = threadIdx.x; e < d * d; e += 256) {
        const int i = e / d, j = e - i * d;
        double v;
        if (ng < d) v = i == j ? 1.0 : 0.0;
        else v = (Gg[e] + Gg[j * d + i]) / den - (Sg[i] / (double)ng) * (Sg[j] / (double)ng);
        cov[g * d * d + e] = v;
    }
}

// grid (groups), block 256: R[g][i][:] = V[g][:, perm[g][i]]
__global__ __launch_bounds__(256) void k_rotation_pack(const double* __restrict__ V, const int32_t* __restrict__ perm, int d, double* __restrict__ R) {
    const int64_t g = blockIdx.x;
    for (int e = threadIdx.x; e < d * d; e += 256) {
        const int i = e / d, j = e - i * d;
        const int c = perm[g * d + i];
        R[g * d * d + e] = (c >= 0 && c < d) ? V[g * d * d + (int64_t)j * d + c] : __builtin_nan("");
    }
}


namespace {

constexpr int64_t TRAIN_MAX_D = 1 << 15;  // d * d stays an int

int launch_gram(const double* dX, int d, const int64_t* dOff, int groups, double* dG, double* dS, hipStream_t st) {
    const unsigned t = (unsigned)ceil_div(d, 64);
    for (int g0 = 0; g0 < groups; g0 += 32768) {  // gridDim.z limit
        const int ng = groups - g0 < 32768 ? groups - g0 : 32768;
        hipLaunchKernelGGL(k_gram_groups, dim3(t, t, (unsigned)ng), dim3(256), 0, st, dX, dOff + g0, d, dG + (int64_t)g0 * d * d,
                           dS ? dS + (int64_t)g0 * d : nullptr);
    }
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

int launch_project(const double* dX, int64_t n, int d, const int64_t* dOff, int groups, int64_t max_rows, const double* dR, const double* dM,
                   const int64_t* dOrder, double* dY, hipStream_t st) {
    const int64_t row_tiles = ceil_div(max_rows, 64);
    for (int g0 = 0; g0 < groups; g0 += 32768) {
        const int ng = groups - g0 < 32768 ? groups - g0 : 32768;
        for (int64_t t0 = 0; t0 < row_tiles; t0 += 65535) {  // the grid's y extent holds 65535 tiles = 4M rows of a group
            const int64_t nt = row_tiles - t0 < 65535 ? row_tiles - t0 : 65535;
            hipLaunchKernelGGL(k_project_groups, dim3((unsigned)ceil_div(d, 64), (unsigned)nt, (unsigned)ng), dim3(256), 0, st, dX, dOff + g0,
                               d, dR + (int64_t)g0 * d * d, dM + (int64_t)g0 * d, dY, t0, dOrder, n);
        }
    }
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

}  // namespace

extern "C" int cis_train_residuals_dev(const float* d_X, int64_t n, int d, const double* d_C, int groups, const int32_t* d_assign,
                                       const int64_t* d_order, int64_t rows, double* d_out, void* stream) {
    CIS_REQUIRE(d_X && d_C && d_assign && d_order && d_out, "NULL pointer");
    CIS_REQUIRE(n > 0 && rows >= 0 && d > 0 && d <= TRAIN_MAX_D && groups > 0, "bad sizes (n = %lld, rows = %lld, d = %d, groups = %d)",
                (long long)n, (long long)rows, d, groups);
    if (rows == 0) return CIS_OK;
    CIS_TRY(cis_lazy_init());
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(rows * d, 256), 65536);
    hipLaunchKernelGGL(k_residuals, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_X, n, d, d_C, groups, d_assign, d_order, rows, d_out);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_train_gram_dev(const double* d_X, int64_t n, int d, const int64_t* d_group_off, int groups, double* d_G, double* d_S,
                                  void* stream) {
    CIS_REQUIRE(d_X && d_group_off && d_G, "NULL pointer");
    CIS_REQUIRE(n >= 0 && d > 0 && d <= TRAIN_MAX_D && groups > 0, "bad sizes (n = %lld, d = %d, groups = %d)", (long long)n, d, groups);
    CIS_TRY(cis_lazy_init());
    return launch_gram(d_X, d, d_group_off, groups, d_G, d_S, (hipStream_t)stream);
}

extern "C" int cis_train_project_dev(const double* d_X, int64_t n, int d, const int64_t* d_group_off, int groups, int64_t max_group_rows,
                                     const double* d_R, const double* d_mu, const int64_t* d_order, double* d_Y, void* stream) {
    CIS_REQUIRE(d_X && d_group_off && d_R && d_mu && d_Y, "NULL pointer");
    CIS_REQUIRE(n >= 0 && d > 0 && d <= TRAIN_MAX_D && groups > 0, "bad sizes (n = %lld, d = %d, groups = %d)", (long long)n, d, groups);
    CIS_REQUIRE(max_group_rows >= 0 && max_group_rows <= n, "max_group_rows must be in 0 .. n, got %lld", (long long)max_group_rows);
    if (n == 0 || max_group_rows == 0) return CIS_OK;
    CIS_TRY(cis_lazy_init());
    return launch_project(d_X, n, d, d_group_off, groups, max_group_rows, d_R, d_mu, d_order, d_Y, (hipStream_t)stream);
}

extern "C" int cis_train_cov_dev(const double* d_G, const double* d_S, const int64_t* d_group_off, int groups, int d, double* d_cov,
                                 double* d_mu, void* stream) {
    CIS_REQUIRE(d_G && d_S && d_group_off && d_cov && d_mu, "NULL pointer");
    CIS_REQUIRE(d > 0 && d <= TRAIN_MAX_D && groups > 0, "bad sizes (d = %d, groups = %d)", d, groups);
    CIS_TRY(cis_lazy_init());
    hipLaunchKernelGGL(k_group_cov, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, d_G, d_S, d_group_off, d, d_cov, d_mu);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_train_rotation_pack_dev(const double* d_V, const int32_t* d_perm, int groups, int d, double* d_R, void* stream) {
    CIS_REQUIRE(d_V && d_perm && d_R, "NULL pointer");
    CIS_REQUIRE(d > 0 && d <= TRAIN_MAX_D && groups > 0, "bad sizes (d = %d, groups = %d)", d, groups);
    CIS_TRY(cis_lazy_init());
    hipLaunchKernelGGL(k_rotation_pack, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, d_V, d_perm, d, d_R);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

// The host forms: upload, the same launches on the null stream, download.
struct TrainBufs {
    double *dX = nullptr, *dG = nullptr, *dS = nullptr, *dR = nullptr, *dM = nullptr, *dY = nullptr;
    int64_t* dOff = nullptr;
    ~TrainBufs() {
        for (void* p : {(void*)dX, (void*)dG, (void*)dS, (void*)dR, (void*)dM, (void*)dY, (void*)dOff})
            if (p) (void)hipFree(p);
    }
};

extern "C" int cis_train_gram(const double* X, int64_t n, int d, const int64_t* group_off, int groups, double* G, double* S) {
    CIS_REQUIRE(X && group_off && G && n >= 0 && d > 0, "bad arguments");
    CIS_REQUIRE(groups > 0, "groups must be > 0");
    CIS_REQUIRE(group_off[0] == 0 && group_off[groups] == n, "group offsets must cover [0, n)");
    CIS_TRY(cis_lazy_init());
    TrainBufs b;
    const size_t gx = (size_t)(n > 0 ? n : 1) * d * sizeof(double), gg = (size_t)groups * d * d * sizeof(double);
    CIS_CHECK_HIP(hipMalloc((void**)&b.dX, gx));
    CIS_CHECK_HIP(hipMalloc((void**)&b.dG, gg));
    CIS_CHECK_HIP(hipMalloc((void**)&b.dS, (size_t)groups * d * sizeof(double)));
    CIS_CHECK_HIP(hipMalloc((void**)&b.dOff, (size_t)(groups + 1) * sizeof(int64_t)));
    if (n > 0) CIS_CHECK_HIP(hipMemcpy(b.dX, X, (size_t)n * d * sizeof(double), hipMemcpyHostToDevice));
    CIS_CHECK_HIP(hipMemcpy(b.dOff, group_off, (size_t)(groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    CIS_TRY(launch_gram(b.dX, d, b.dOff, groups, b.dG, b.dS, nullptr));
    CIS_CHECK_HIP(hipMemcpy(G, b.dG, gg, hipMemcpyDeviceToHost));
    if (S) CIS_CHECK_HIP(hipMemcpy(S, b.dS, (size_t)groups * d * sizeof(double), hipMemcpyDeviceToHost));
    return CIS_OK;
}

extern "C" int cis_train_project(const double* X, int64_t n, int d, const int64_t* group_off, int groups, const double* R,
                                 const double* mu, double* Y) {
    CIS_REQUIRE(X && group_off && R && mu && Y && n >= 0 && d > 0, "bad arguments");
    CIS_REQUIRE(groups > 0, "groups must be > 0");
    CIS_REQUIRE(group_off[0] == 0 && group_off[groups] == n, "group offsets must cover [0, n)");
    if (n == 0) return CIS_OK;
    CIS_TRY(cis_lazy_init());
    TrainBufs b;
    CIS_CHECK_HIP(hipMalloc((void**)&b.dX, (size_t)n * d * sizeof(double)));
    CIS_CHECK_HIP(hipMalloc((void**)&b.dY, (size_t)n * d * sizeof(double)));
    CIS_CHECK_HIP(hipMalloc((void**)&b.dR, (size_t)groups * d * d * sizeof(double)));
    CIS_CHECK_HIP(hipMalloc((void**)&b.dM, (size_t)groups * d * sizeof(double)));
    CIS_CHECK_HIP(hipMalloc((void**)&b.dOff, (size_t)(groups + 1) * sizeof(int64_t)));
    CIS_CHECK_HIP(hipMemcpy(b.dX, X, (size_t)n * d * sizeof(double), hipMemcpyHostToDevice));
    CIS_CHECK_HIP(hipMemcpy(b.dR, R, (size_t)groups * d * d * sizeof(double), hipMemcpyHostToDevice));
    CIS_CHECK_HIP(hipMemcpy(b.dM, mu, (size_t)groups * d * sizeof(double), hipMemcpyHostToDevice));
    CIS_CHECK_HIP(hipMemcpy(b.dOff, group_off, (size_t)(groups + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    int64_t max_rows = 0;
    for (int g = 0; g < groups; ++g) max_rows = group_off[g + 1] - group_off[g] > max_rows ? group_off[g + 1] - group_off[g] : max_rows;
    CIS_TRY(launch_project(b.dX, n, d, b.dOff, groups, max_rows, b.dR, b.dM, nullptr, b.dY, nullptr));
    CIS_CHECK_HIP(hipMemcpy(Y, b.dY, (size_t)n * d * sizeof(double), hipMemcpyDeviceToHost));
    return CIS_OK;
}
