// Device-wide exclusive scan (tile sums -> scan of the sums -> add), shared by the insert (lopq_index.hip) and the removal
// (lopq_remove.hip).
#pragma once
#include "common.h"

// ================================================================================================
// device-wide exclusive scan (tile sums -> scan of the sums -> add)
// ================================================================================================
static const int SCAN_T = 256, SCAN_PER = 8, SCAN_TILE = SCAN_T * SCAN_PER;

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// exclusive scan of one value per thread over a block of SCAN_T threads; returns the block total in *total
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* sh /* [SCAN_T / 64 + 1] */, T* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const T inc = wave_incl_scan(v);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < SCAN_T / 64; ++i) {
        const T s = sh[i];
        base += (i < w) ? s : (T)0;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(SCAN_T) void k_scan_tiles(const TI* __restrict__ in, TO* __restrict__ out, TO* __restrict__ sums, int64_t n) {
    __shared__ TO sh[SCAN_T / 64 + 1];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER;
    TO v[SCAN_PER];
    TO s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_PER; ++i) {
        v[i] = (base + i < n) ? (TO)in[base + i] : (TO)0;
        s += v[i];
    }
    TO tot;
    TO run = block_excl_scan<TO>(s, sh, &tot);
#pragma unroll
    for (int i = 0; i < SCAN_PER; ++i) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// one workgroup: exclusive scan of the tile sums in place, the grand total to total[0] (and total2[0], may be null)
template <typename TO>
__global__ __launch_bounds__(SCAN_T) void k_scan_sums(TO* __restrict__ sums, int64_t m, TO* __restrict__ total, int64_t* __restrict__ total2) {
    __shared__ TO sh[SCAN_T / 64 + 1];
    TO carry = 0;
    for (int64_t b = 0; b < m; b += SCAN_T) {
        const int64_t i = b + threadIdx.x;
        const TO v = i < m ? sums[i] : (TO)0;
        TO tot;
        const TO e = block_excl_scan<TO>(v, sh, &tot);
        if (i < m) sums[i] = carry + e;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        if (total) total[0] = carry;
        if (total2) total2[0] = (int64_t)carry;
    }
}

template <typename TO>
__global__ __launch_bounds__(SCAN_T) void k_scan_add(TO* __restrict__ out, const TO* __restrict__ sums, int64_t n) {
    const TO add = sums[blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_PER;
#pragma unroll
    for (int i = 0; i < SCAN_PER; ++i)
        if (base + i < n) out[base + i] += add;
}

// out[i] = sum of in[0 .. i); total (device, may be null) = sum of all; sums: scratch of ceil(n / SCAN_TILE) + 1 elements
template <typename TI, typename TO>
static void dev_exclusive_scan(const TI* in, TO* out, int64_t n, TO* sums, TO* total, int64_t* total2, hipStream_t st) {
    const int64_t m = n > 0 ? ceil_div(n, SCAN_TILE) : 0;
    if (m > 0) hipLaunchKernelGGL((k_scan_tiles<TI, TO>), dim3((unsigned)m), dim3(SCAN_T), 0, st, in, out, sums, n);
    hipLaunchKernelGGL((k_scan_sums<TO>), dim3(1), dim3(SCAN_T), 0, st, sums, m, total, total2);
    if (m > 1) hipLaunchKernelGGL((k_scan_add<TO>), dim3((unsigned)m), dim3(SCAN_T), 0, st, out, (const TO*)sums, n);
}
