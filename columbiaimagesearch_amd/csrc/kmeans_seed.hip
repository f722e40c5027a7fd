// k-means++ seeding on device data (cis_kmeanspp_dev): the D^2 draws of Arthur & Vassilvitskii for the Lloyd iterations of
// kmeans_mfma.hip, so that the seeds of a resident training set never visit the host.  The caller supplies the k uniforms: the call is
// a deterministic function of its inputs (no float atomics; two calls with equal inputs give equal bytes).
//
// Semantics (include/cis_hip.h states them for the caller, tests/test_kmeans_seed.py pins them):
//   centre 0 is row floor(u[0] * n).
//   d2[r] is float32 in the direct form acc = fmaf(x[i] - c[i], x[i] - c[i], acc) (k_kmd_inertia's form; the order over i is a lane
//   group's: partial chains per lane, then a butterfly), so a chosen row and every copy of it have d2 == 0 exactly; after centre j,
//   d2[r] = min(d2[r], dist(r, centre j)).
//   Sums are float64 over fixed tiles of TILE rows: a tile's sum is a fixed tree over its TILE values (a butterfly inside each of the
//   four 64-row quarters, then the quarters in ascending order), whichever workgroup computes it and however large the grid is.
//   The prefix over tiles is a chain: S_tile(T) = fl(E_c + w(T)) with w(T) the ascending sum of the tiles of T's chunk up to T (a chunk
//   is ceil(tiles / 256) consecutive tiles) and E_0 = 0, E_{c+1} = fl(E_c + w(last tile of chunk c)).  tot = S_tile(last tile), so the
//   last tile's prefix IS tot, and S_tile never decreases.
//   Draw j >= 1: t = u[j] * tot (one float64 multiply).  The tile is the first T with S_tile(T) > t; inside it S(r) = fl(S_tile(T - 1) +
//   v(r)), v the inclusive float64 prefix of the tile's d2 (a fixed scan tree), and the pick is the first row with d2 > 0 and S(r) > t.
//   A row with d2 == 0 is never picked while tot > 0.  If rounding lets the scan run off the tile's end (v's tree is not the tile sum's),
//   the pick is the tile's last row with d2 > 0.  tot == 0 (fewer distinct rows than centres; also a NaN total): row floor(u[j] * n).
//   The potential is tot after centre k - 1.
//
// Two launches per draw, the kernel boundary is the hand-off (no in-launch ticket, spin wait or cooperative grid):
//   k_kpp_update: the hot path, a stream of X against the newest centre.  A row belongs to a group of G adjacent lanes (G = the power of
//                 two that covers d / 4 16-byte pieces, or d floats where d % 4 != 0 or X is not 16-byte aligned; at most 64), so a
//                 wave instruction reads 64 consecutive pieces: whole rows, coalesced.  Where a row fits one piece per lane (d <= 256
//                 aligned, d <= 64 otherwise) the lane's part of the centre is a register and four rows' loads are in flight per lane;
//                 longer rows loop over pieces with the centre in LDS (up to 8192 floats; from L2 beyond).  The group is reduced with
//                 DPP (quad_perm, row_half_mirror, row_mirror) and two shuffles, the tile's 256 distances meet in LDS, and thread r
//                 does row r's min, its coalesced 4-byte load and store of d2, and the float64 tile sum.  Loads past the last row are
//                 clamped to it (never predicated); such a row counts 0 and is not written.  Grid-stride over tiles, bounded grid.
//   k_kpp_pick:   one workgroup.  The chain over the tile sums (thread c sums chunk c, thread 0 links the 256 chunks), the scan of the
//                 tile's d2, picked[j], and the copy of the row into d_centroids[j].  Mode 0 (centre 0) and mode 2 (potential only)
//                 share the kernel.
#include <algorithm>
#include <mutex>

#include "common.h"

namespace {

constexpr int TILE = 256;                                // rows per tile sum = threads per workgroup
constexpr int MAX_GRID = 2048;                           // workgroups of k_kpp_update (8 per CU)
constexpr int CHUNKS = 256;                              // links of the chain over the tile sums
constexpr int D_LDS = 8192;                              // floats of the centre the looping forms keep in LDS
constexpr int64_t KPP_MAX_N = ((int64_t)1 << 31) - 256;  // int32 row indices, and n + TILE stays an int
constexpr int64_t KPP_MAX_KD = (int64_t)1 << 30;         // k * d, as cis_kmeans_dev

template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false);
    return v + __builtin_bit_cast(float, o);
}

// sum over the 2^LG adjacent lanes of a group; every lane of the group gets the same bits (each step adds the two halves' equal values)
template <int LG>
__device__ __forceinline__ float group_sum(float v) {
    if (LG >= 1) v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    if (LG >= 2) v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    if (LG >= 3) v = dpp_add<0x141>(v);  // row_half_mirror: the other quad of the 8
    if (LG >= 4) v = dpp_add<0x140>(v);  // row_mirror: the other 8 of the 16
    if (LG >= 5) v = v + __shfl_xor(v, 16);
    if (LG >= 6) v = v + __shfl_xor(v, 32);
    return v;
}

__device__ __forceinline__ float sq_acc(float x, float c, float acc) {
    const float df = x - c;
    return fmaf(df, df, acc);
}
__device__ __forceinline__ float sq_acc(const float4& x, const float4& c, float acc) {
    return sq_acc(x.w, c.w, sq_acc(x.z, c.z, sq_acc(x.y, c.y, sq_acc(x.x, c.x, acc))));
}

// min with the old d2, the coalesced d2 traffic and the tile's float64 sum: thread r owns row r of the tile
__device__ __forceinline__ void tile_finish(const float* s_dist, double* s_q, int64_t row0, int64_t n, bool first, float* __restrict__ d2,
                                            double* __restrict__ tsum, int64_t tile) {
    const int tid = threadIdx.x;
    const int64_t row = row0 + tid;
    float v = 0.f;
    if (row < n) {
        v = s_dist[tid];
        if (!first) v = fminf(v, d2[row]);  // (fminf drops a NaN distance where the old value is a number; a NaN row stays NaN otherwise)
        d2[row] = v;
    }
    double s = (double)v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s = s + __shfl_xor(s, o);
    if ((tid & 63) == 0) s_q[tid >> 6] = s;
    __syncthreads();  // (also: every thread has read s_dist before the next tile overwrites it)
    if (tid == 0) tsum[tile] = ((s_q[0] + s_q[1]) + s_q[2]) + s_q[3];
}

// One piece (V = float4 or float) per lane and row: G = 2^LG lanes per row, nv pieces per row (G / 2 < nv <= G, or nv = G = 1).
template <typename V, int LG>
__global__ __launch_bounds__(TILE) void k_kpp_update(const float* __restrict__ X, int64_t n, int d, const float* __restrict__ centre,
                                                     int nv, int first, float* __restrict__ d2, double* __restrict__ tsum) {
    constexpr int G = 1 << LG, RPP = TILE / G, UNR = G < 4 ? G : 4;  // rows per pass of the workgroup; passes per tile = G
    __shared__ float s_dist[TILE];
    __shared__ double s_q[4];
    const int tid = threadIdx.x, l = tid & (G - 1), grp = tid >> LG;
    const bool live = l < nv;
    const int li = live ? l : nv - 1;  // an idle lane re-reads the last piece and adds nothing
    const V c = reinterpret_cast<const V*>(centre)[li];
    const int64_t n_tiles = (n + TILE - 1) / TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * TILE;
#pragma unroll 1
        for (int p = 0; p < G; p += UNR) {
            V x[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int64_t row = std::min<int64_t>(row0 + (p + u) * RPP + grp, n - 1);
                x[u] = reinterpret_cast<const V*>(X + row * d)[li];
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const float acc = group_sum<LG>(live ? sq_acc(x[u], c, 0.f) : 0.f);
                if (l == 0) s_dist[(p + u) * RPP + grp] = acc;
            }
        }
        __syncthreads();
        tile_finish(s_dist, s_q, row0, n, first != 0, d2, tsum, tile);
    }
}

// Rows of more than 64 pieces: a wave per row, the lanes loop over the pieces; the centre in LDS (CLDS) or read through L2.
template <typename V, bool CLDS>
__global__ __launch_bounds__(TILE) void k_kpp_update_long(const float* __restrict__ X, int64_t n, int d, const float* __restrict__ centre,
                                                          int nv, int first, float* __restrict__ d2, double* __restrict__ tsum) {
    __shared__ float s_dist[TILE];
    __shared__ double s_q[4];
    __shared__ __attribute__((aligned(16))) float s_c[CLDS ? D_LDS : 4];
    const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6;
    if (CLDS) {
        for (int i = tid; i < d; i += TILE) s_c[i] = centre[i];
        __syncthreads();
    }
    const V* cv;
    if (CLDS) cv = reinterpret_cast<const V*>(s_c);
    else cv = reinterpret_cast<const V*>(centre);
    const int64_t n_tiles = (n + TILE - 1) / TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = tile * TILE;
        for (int p = 0; p < 64; ++p) {
            const int64_t row = std::min<int64_t>(row0 + p * 4 + wave, n - 1);
            const V* xv = reinterpret_cast<const V*>(X + row * d);
            float acc = 0.f;
#pragma unroll 4
            for (int i = l; i < nv; i += 64) acc = sq_acc(xv[i], cv[i], acc);
            acc = group_sum<6>(acc);
            if (l == 0) s_dist[p * 4 + wave] = acc;
        }
        __syncthreads();
        tile_finish(s_dist, s_q, row0, n, first != 0, d2, tsum, tile);
    }
}

__device__ __forceinline__ int64_t row_of_uniform(double u, int64_t n) {
    const int64_t r = (int64_t)(u * (double)n);  // floor: u >= 0
    return r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
}

// mode 0: centre 0 (no sums read); mode 1: draw j >= 1; mode 2: only *potential = tot.
__global__ __launch_bounds__(TILE) void k_kpp_pick(const float* __restrict__ X, int64_t n, int d, const float* __restrict__ d2,
                                                   const double* __restrict__ tsum, int64_t n_tiles, const double* __restrict__ u, int j,
                                                   int mode, float* __restrict__ C, int* __restrict__ picked, double* __restrict__ potential) {
    __shared__ double s_w[CHUNKS], s_E[CHUNKS + 1], s_base, s_wave[4];
    __shared__ long long s_tile;
    __shared__ int s_first, s_last;
    const int tid = threadIdx.x;
    int64_t row = -1;
    if (mode != 0) {
        const int64_t ch = (n_tiles + CHUNKS - 1) / CHUNKS;
        const int64_t t0 = std::min<int64_t>(tid * ch, n_tiles), t1 = std::min<int64_t>(t0 + ch, n_tiles);
        double w = 0.0;
        for (int64_t T = t0; T < t1; ++T) w = w + tsum[T];
        s_w[tid] = w;
        if (tid == 0) {
            s_tile = -1;
            s_first = TILE;
            s_last = -1;
        }
        __syncthreads();
        if (tid == 0) {
            double E = 0.0;
            s_E[0] = E;
            for (int c = 0; c < CHUNKS; ++c) {
                E = E + s_w[c];
                s_E[c + 1] = E;
            }
        }
        __syncthreads();
        const double tot = s_E[CHUNKS];
        if (mode == 2) {
            if (tid == 0) *potential = tot;
            return;
        }
        const double t = u[j] * tot;
        if (tot > 0.0) {
            // the chain never decreases, so at most one chunk has E_c <= t < E_{c+1}: its thread walks it again
            if (s_E[tid] <= t && t < s_E[tid + 1]) {
                const double E = s_E[tid];
                double prev = E;
                w = 0.0;
                for (int64_t T = t0; T < t1; ++T) {
                    w = w + tsum[T];
                    const double S = E + w;
                    if (S > t) {
                        s_tile = T;
                        s_base = prev;
                        break;
                    }
                    prev = S;
                }
            }
            __syncthreads();
            const int64_t T = s_tile;
            if (T >= 0) {  // (always, unless a NaN sits in the sums)
                const int64_t r = T * TILE + tid;
                const float v = r < n ? d2[r] : 0.f;
                double s = (double)v;  // inclusive scan over the tile's 256 values: inside a wave, then the waves in order
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const double up = __shfl_up(s, o);
                    if ((tid & 63) >= o) s = s + up;
                }
                if ((tid & 63) == 63) s_wave[tid >> 6] = s;
                __syncthreads();
                double off = 0.0;
                for (int q = 0; q < (tid >> 6); ++q) off = off + s_wave[q];
                s = off + s;
                if (v > 0.f) {
                    atomicMax(&s_last, tid);
                    if (s_base + s > t) atomicMin(&s_first, tid);
                }
                __syncthreads();
                if (s_first < TILE) row = T * TILE + s_first;
                else if (s_last >= 0) row = T * TILE + s_last;
            }
        }
    }
    if (row < 0) row = row_of_uniform(u[j], n);
    if (tid == 0 && picked) picked[j] = (int)row;
    const float* x = X + row * d;
    float* c = C + (int64_t)j * d;
    for (int i = tid; i < d; i += TILE) c[i] = x[i];
}

struct KppWs {
    std::mutex mu;
    DevBuf d2, tsum;
};
KppWs g_kpp;

template <typename V>
void launch_update(unsigned grid, hipStream_t st, const float* X, int64_t n, int d, const float* centre, int nv, int first, float* d2,
                   double* tsum) {
#define KPP_CASE(LG) \
    hipLaunchKernelGGL((k_kpp_update<V, LG>), dim3(grid), dim3(TILE), 0, st, X, n, d, centre, nv, first, d2, tsum)
    if (nv <= 1) KPP_CASE(0);
    else if (nv <= 2) KPP_CASE(1);
    else if (nv <= 4) KPP_CASE(2);
    else if (nv <= 8) KPP_CASE(3);
    else if (nv <= 16) KPP_CASE(4);
    else if (nv <= 32) KPP_CASE(5);
    else if (nv <= 64) KPP_CASE(6);
    else if (d <= D_LDS) hipLaunchKernelGGL((k_kpp_update_long<V, true>), dim3(grid), dim3(TILE), 0, st, X, n, d, centre, nv, first, d2, tsum);
    else hipLaunchKernelGGL((k_kpp_update_long<V, false>), dim3(grid), dim3(TILE), 0, st, X, n, d, centre, nv, first, d2, tsum);
#undef KPP_CASE
}

}  // namespace

extern "C" int cis_kmeanspp_dev(const float* d_X, int64_t n, int d, int k, const double* d_u, float* d_centroids, int32_t* d_picked,
                                double* d_potential, void* stream) {
    CIS_REQUIRE(d_X && d_u && d_centroids, "NULL d_X, d_u or d_centroids");
    CIS_REQUIRE(d > 0 && k > 0, "d and k must be >= 1 (d = %d, k = %d)", d, k);
    CIS_REQUIRE(n > 0, "n must be > 0 (seeds of no points)");
    CIS_REQUIRE(n <= KPP_MAX_N, "n must be <= 2^31 - 256 (row indices are int32), got %lld", (long long)n);
    CIS_REQUIRE((int64_t)k * d <= KPP_MAX_KD, "k * d must be <= 2^30 (as cis_kmeans_dev), got %lld", (long long)k * d);
    CIS_TRY(cis_lazy_init());
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(g_kpp.mu);
    KppWs& w = g_kpp;
    const int64_t n_tiles = ceil_div(n, TILE);
    CIS_TRY(w.d2.reserve((size_t)n * 4));
    CIS_TRY(w.tsum.reserve((size_t)n_tiles * 8));
    float* d2 = w.d2.as<float>();
    double* tsum = w.tsum.as<double>();
    const unsigned grid = (unsigned)std::min<int64_t>(n_tiles, MAX_GRID);
    // 16-byte pieces need 16-byte rows (the centre is a row of d_centroids: the same test)
    const bool vec = d % 4 == 0 && ((uintptr_t)d_X & 15) == 0 && ((uintptr_t)d_centroids & 15) == 0;
    auto update = [&](int j) {  // against centre j
        const float* centre = d_centroids + (int64_t)j * d;
        if (vec) launch_update<float4>(grid, st, d_X, n, d, centre, d / 4, j == 0, d2, tsum);
        else launch_update<float>(grid, st, d_X, n, d, centre, d, j == 0, d2, tsum);
    };
    auto pick = [&](int j, int mode) {
        hipLaunchKernelGGL(k_kpp_pick, dim3(1), dim3(TILE), 0, st, d_X, n, d, d2, tsum, n_tiles, d_u, j, mode, d_centroids, d_picked,
                           d_potential);
    };
    pick(0, 0);
    for (int j = 1; j < k; ++j) {
        update(j - 1);
        pick(j, 1);
    }
    if (d_potential) {
        update(k - 1);
        pick(k, 2);
    }
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}
