// Device helpers shared by the ADC scan kernels (lopq_search.hip: float32-prefilter scan; lopq_scan3.hip: 16-bit
// fixed-point scan): work-item layout, wave-level primitives on the VALU only, code loads, exact re-scoring; and by the
// merges of ranked hit lists (lopq_search.hip, lopq_exchange.hip); the work item, table and plan records the plan stage
// (lopq_plan.hip) writes for them.
#pragma once
#include <type_traits>

#include "lopq_model.h"

struct WorkItem {
    int q;          // query index inside the batch
    int rank;       // multisequence visit rank of the cell
    int tab0, tab1; // indices of the two half tables
    int64_t start;  // first candidate (position in codes/ids)
    int len;        // candidates in this chunk
    int pos0;       // insertion position of the first candidate inside its cell
    int cell;       // c0 * V + c1
    int pad;
};

struct TabDesc {
    int q, split, cluster, pad;
};

struct PlanOut {  // per query
    int visited, n_items, ntab0, ntab1;
    int64_t ncand;
};

// distances are >= 0, so their bit patterns order like the values
static __device__ __forceinline__ uint64_t f2bits(double d) { return (uint64_t)__double_as_longlong(d); }
static __device__ __forceinline__ uint64_t f2bits(float f) { return (uint64_t)__float_as_uint(f); }

// value of lane (l ^ LJ) for every lane l, on the VALU only (DPP / permlane swaps): the LDS pipe is the
// scan's bottleneck, so the in-register sorts must not use ds_bpermute.
template <int LJ>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
    if constexpr (LJ == 1) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    } else if constexpr (LJ == 2) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    } else if constexpr (LJ == 4) {
        const int a = __builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);      // row_half_mirror: l ^ 7
        return (uint32_t)__builtin_amdgcn_update_dpp(0, a, 0x1B, 0xF, 0xF, false);        // quad_perm [3,2,1,0]: ^ 3
    } else if constexpr (LJ == 8) {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, false);  // row_ror:8 == l ^ 8 in a row of 16
    } else if constexpr (LJ == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);  // .x = even rows twice, .y = odd rows twice
        return (threadIdx.x & 16) ? r[0] : r[1];
    } else {
        static_assert(LJ == 32, "lane_xor: LJ must be a power of two below 64");
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);  // .x = low half twice, .y = high half twice
        return (threadIdx.x & 32) ? r[0] : r[1];
    }
}

template <int NR, int KK, int J>
__device__ __forceinline__ void bitonic_step(uint32_t (&k)[NR]) {
    const int lane = threadIdx.x & 63;
    if constexpr (J < NR) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if ((r & J) == 0) {
                const bool asc = (((lane * NR + r) & KK) == 0);
                const uint32_t a = k[r], b = k[r | J];
                const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
                k[r] = asc ? lo : hi;
                k[r | J] = asc ? hi : lo;
            }
        }
    } else {
        constexpr int LJ = J / NR;
        const bool lower = ((lane & LJ) == 0);
        const bool asc = (((lane * NR) & KK) == 0);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint32_t o = lane_xor<LJ>(k[r]);
            const uint32_t mn = k[r] < o ? k[r] : o, mx = k[r] < o ? o : k[r];
            k[r] = (lower == asc) ? mn : mx;
        }
    }
}

template <int NR, int KK, int J>
__device__ __forceinline__ void bitonic_merge(uint32_t (&k)[NR]) {
    bitonic_step<NR, KK, J>(k);
    if constexpr (J > 1) bitonic_merge<NR, KK, J / 2>(k);
}

template <int NR, int KK>
__device__ __forceinline__ void bitonic_levels(uint32_t (&k)[NR]) {
    if constexpr (KK > 2) bitonic_levels<NR, KK / 2>(k);
    bitonic_merge<NR, KK, KK / 2>(k);
}

// ascending sort of the NR*64 keys of a wave, element e = lane*NR + r
template <int NR>
__device__ __forceinline__ void wave_bitonic_sort(uint32_t (&k)[NR]) {
    bitonic_levels<NR, NR * 64>(k);
}

template <int LJ>
__device__ __forceinline__ void wave_minmax_step(uint32_t& mn, uint32_t& mx) {
    const uint32_t a = lane_xor<LJ>(mn), b = lane_xor<LJ>(mx);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
}
// min and max of the lanes' values over the wave, as wave-uniform (scalar) values
static __device__ __forceinline__ void wave_minmax_all(uint32_t& mn, uint32_t& mx) {
    wave_minmax_step<1>(mn, mx); wave_minmax_step<2>(mn, mx); wave_minmax_step<4>(mn, mx);
    wave_minmax_step<8>(mn, mx); wave_minmax_step<16>(mn, mx); wave_minmax_step<32>(mn, mx);
    mn = (uint32_t)__builtin_amdgcn_readfirstlane((int)mn);
    mx = (uint32_t)__builtin_amdgcn_readfirstlane((int)mx);
}

// Smallest v with  #{valid keys <= v} >= target  == the target-th smallest key (1-based), found by
// bisection on the value range with ballots: ~4 VALU compares per probe instead of a ~650-instruction
// register sort.  lo/hi must bracket the answer (lo = min key, hi = max key is always fine).
template <int NR>
__device__ __forceinline__ uint32_t wave_kth_bisect(const uint32_t (&key)[NR], const bool (&valid)[NR], uint32_t lo,
                                                    uint32_t hi, int target) {
    while (lo < hi) {  // wave-uniform
        const uint32_t p = lo + ((hi - lo) >> 1);
        int c = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) c += __popcll(__ballot(valid[r] && key[r] <= p));
        if (c >= target) hi = p;
        else lo = p + 1;
    }
    return lo;
}

// #{kept keys <= p} over the wave
template <int NR>
__device__ __forceinline__ int wave_count_le(const bool (&keep)[NR], const uint32_t (&key)[NR], uint32_t p) {
    int c = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) c += __popcll(__ballot(keep[r] && key[r] <= p));
    return c;
}

// A value v with #{kept keys <= v} in [n, n + W]: the bisection of wave_kth_bisect, stopped at the first probe whose count falls
// inside the window.  When ties make the count jump over the window, v is the n-th smallest key.  Needs n <= #kept; [lo, hi]
// brackets the keys.
template <int NR>
__device__ __forceinline__ uint32_t wave_bisect_window(const bool (&keep)[NR], const uint32_t (&key)[NR], uint32_t lo, uint32_t hi,
                                                       int n, int W) {
    while (lo < hi) {  // wave-uniform
        const uint32_t p = lo + ((hi - lo) >> 1);
        const int c = wave_count_le<NR>(keep, key, p);
        if (c >= n) {
            hi = p;
            if (c <= n + W) break;
        } else {
            lo = p + 1;
        }
    }
    return hi;
}

// Stable compaction of a wave's NR * 64 entries (entry e = r * 64 + lane): store(r, idx) for every entry with pred(r), idx = its
// index among the kept ones.  Returns their number.  Wave-synchronous: the stores are visible to the wave on return.
template <int NR, typename P, typename S>
__device__ __forceinline__ int wave_stable_keep(P&& pred, S&& store) {
    int n = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const bool kp = pred(r);
        const unsigned long long m = __ballot(kp);
        const int idx = n + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
        if (kp) store(r, idx);
        n += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return n;
}

template <int NR>
__device__ __forceinline__ uint32_t wave_kth(const uint32_t (&k)[NR], int i) {  // i-th smallest after the sort
    uint32_t v = k[0];
#pragma unroll
    for (int r = 1; r < NR; ++r)
        if ((i % NR) == r) v = k[r];
    return (uint32_t)__builtin_amdgcn_readlane((int)v, i / NR);
}

static __device__ __forceinline__ float lds_ld(const float* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ uint64_t lds_ld(const uint64_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ uint32_t lds_ld(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ void lds_st(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ void lds_st(uint64_t* p, uint64_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
static __device__ __forceinline__ void lds_st(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// exact float64 distance from the code words (little-endian bytes = fine codes 0..M-1)
template <int M>
static __device__ __forceinline__ double adc64_words(const uint32_t (&cw)[(M + 3) / 4], int K, const double* __restrict__ t0,
                                                     const double* __restrict__ t1) {
    constexpr int nf = M / 2;
    double f[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const uint32_t c = (cw[j >> 2] >> (8 * (j & 3))) & 255u;
        f[j] = (j < nf) ? t0[j * K + c] : t1[(j - nf) * K + c];   // (non-temporal loads here: the merge 0.104 -> 0.119 ms on C2, round 6)
    }
    double d = f[0];
#pragma unroll
    for (int j = 1; j < M; ++j) d = d + f[j];
    return d;
}

// hi word -> the largest float64 bit pattern with that hi word (a distance no smaller than any
// distance whose bits start with `vhi`); infinities stay infinite
static __device__ __forceinline__ uint64_t hi_to_bound(uint32_t vhi) {
    return vhi >= 0x7ff00000u ? 0x7ff0000000000000ull : (((uint64_t)vhi << 32) | 0xffffffffull);
}

// The exact cut of both scan families (wave_compact_exact, wave_compact3_exact): of the wave's cnt entries with exact float64 keys
// (hi, lo), entry e = r * 64 + lane in region order, keep[] narrows to the top L by (key, region order).  Region entries are always
// in increasing candidate position (appends are, and the compactions are stable), so among exactly equal distances "first in the
// region" == "smallest pos": the order of the reference's stable sorted().  mn / mx: wave_minmax_all of the hi words.  Out: vhiL,
// the hi word of the L-th entry (mx when cnt < L, nothing cut), and boundL, a distance no smaller than the L kept ones (infinite
// when cnt < L).  pos_of(r): the candidate position of entry r of this lane.
template <int NR, typename POS>
__device__ __forceinline__ void wave_exact_cut(const uint32_t (&hi)[NR], const uint32_t (&lo)[NR], bool (&keep)[NR], POS&& pos_of,
                                               uint32_t mn, uint32_t mx, int cnt, int L, uint32_t& vhiL, uint64_t& boundL,
                                               uint32_t& dup_pos) {
    vhiL = mx;
    boundL = 0x7ff0000000000000ull;
    if (cnt >= L) {  // cut to this wave's own exact top-L
        const uint32_t vhi = wave_kth_bisect<NR>(hi, keep, mn, mx, L);
        vhiL = vhi;
        boundL = hi_to_bound(vhi);
        int c_less = 0, g = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            c_less += __popcll(__ballot(keep[r] && hi[r] < vhi));
            g += __popcll(__ballot(keep[r] && hi[r] == vhi));
        }
        int need = L - c_less;  // members of the group {hi == vhi} to keep, 1 <= need <= g
        if (need >= g) {
#pragma unroll
            for (int r = 0; r < NR; ++r) keep[r] = keep[r] && hi[r] <= vhi;
        } else {
            // low word of the first group member in region order; are all members equal to it?
            uint32_t lo_first = 0;
            bool found = false, uniform = true;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const bool in_g = keep[r] && hi[r] == vhi;
                const unsigned long long m = __ballot(in_g);
                if (!found && m) {
                    lo_first = (uint32_t)__builtin_amdgcn_readlane((int)lo[r], __ffsll((long long)m) - 1);
                    found = true;
                }
                if (found) uniform = uniform && (__ballot(in_g && lo[r] != lo_first) == 0ull);
            }
            uint32_t vlo = lo_first;
            if (!uniform) {
                uint32_t t2[NR];
#pragma unroll
                for (int r = 0; r < NR; ++r) t2[r] = (keep[r] && hi[r] == vhi) ? lo[r] : 0xffffffffu;
                wave_bitonic_sort<NR>(t2);
                vlo = wave_kth<NR>(t2, need - 1);
#pragma unroll
                for (int r = 0; r < NR; ++r) need -= __popcll(__ballot(keep[r] && hi[r] == vhi && lo[r] < vlo));
            }
            // exact ties (hi, lo) == (vhi, vlo): the first `need` in region order have the smallest positions
            int seen = 0;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const bool tie = keep[r] && hi[r] == vhi && lo[r] == vlo;
                const unsigned long long m = __ballot(tie);
                const int rank = seen + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
                keep[r] = keep[r] && (hi[r] < vhi || (hi[r] == vhi && (lo[r] < vlo || (tie && rank < need))));
                // The cut fell inside a group of exactly equal distances.  Remember one member: every LATER
                // candidate with the same code has the same distance and a larger position, so it loses
                // against all L entries kept here and the hot loop may skip it (duplicate codes are common).
                if (seen == 0 && m) dup_pos = (uint32_t)__builtin_amdgcn_readlane((int)pos_of(r), __ffsll((long long)m) - 1);
                seen += __popcll(m);
            }
        }
    }
}

// The bound of a query's workgroup from what its waves published (ScanShared, Scan3Shared): every wt[w] is a distance that
// ceil(limit / NW) candidates of wave w do not exceed, so `limit` candidates do not exceed their maximum; every wl[w], and ext from
// the query's other cells, is one that `limit` candidates do not exceed.  Exact float64 bits.
template <int NW, typename SH>
static __device__ __forceinline__ uint64_t block_bound(const SH* sh) {
    uint64_t t = lds_ld(&sh->wt[0]);
    uint64_t l = lds_ld(&sh->wl[0]);
#pragma unroll
    for (int i = 1; i < NW; ++i) {
        const uint64_t a = lds_ld(&sh->wt[i]), b = lds_ld(&sh->wl[i]);
        t = a > t ? a : t;
        l = b < l ? b : l;
    }
    const uint64_t e = lds_ld(&sh->ext);
    l = e < l ? e : l;
    return t < l ? t : l;
}

// one candidate's code as 32-bit words (little-endian bytes = fine codes 0..M-1)
template <int M>
struct CodeWords { uint32_t w[(M + 3) / 4]; };

template <int M>
__device__ __forceinline__ CodeWords<M> load_code(const uint8_t* __restrict__ codes, int64_t p) {
    CodeWords<M> c;
    if constexpr (M == 4) {
        c.w[0] = *reinterpret_cast<const uint32_t*>(codes + p * 4);
    } else if constexpr (M == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(codes + p * 8);
        c.w[0] = v.x; c.w[1] = v.y;
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(codes + p * 16);
        c.w[0] = v.x; c.w[1] = v.y; c.w[2] = v.z; c.w[3] = v.w;
    }
    return c;
}

template <int M>
struct RotConsts {
    uint32_t sh[4];   // bit offset of the byte used at sub-step tq inside the selected dword
    uint32_t cj[M];   // (table index << 2) for step t
    uint32_t hsel;    // which dword this lane starts with
};

template <int M>
__device__ __forceinline__ RotConsts<M> make_rot(int lane) {
    RotConsts<M> rc;
    const int r = lane & (M - 1);
    const int h = r >> 2, q = r & 3;
    rc.hsel = (uint32_t)h;
#pragma unroll
    for (int tq = 0; tq < 4; ++tq) rc.sh[tq] = 8u * (uint32_t)((q + tq) & 3);
#pragma unroll
    for (int t = 0; t < M; ++t) {
        const int th = t >> 2, tq = t & 3;
        const int j = ((h ^ th) << 2) | ((q + tq) & 3);
        rc.cj[t] = (uint32_t)j << 2;
    }
    return rc;
}

// one candidate's code words in this lane's rotated order (make_rot): D[t >> 2] holds the byte used at step t
template <int M>
__device__ __forceinline__ void rot_words(const CodeWords<M>& c, const RotConsts<M>& rc, uint32_t (&D)[(M + 3) / 4]) {
    if constexpr (M == 4) {
        D[0] = c.w[0];
    } else if constexpr (M == 8) {
        D[0] = rc.hsel ? c.w[1] : c.w[0];
        D[1] = rc.hsel ? c.w[0] : c.w[1];
    } else {
        const bool b0 = rc.hsel & 1, b1 = rc.hsel & 2;
        const uint32_t x01 = b0 ? c.w[1] : c.w[0], y01 = b0 ? c.w[0] : c.w[1];
        const uint32_t x23 = b0 ? c.w[3] : c.w[2], y23 = b0 ? c.w[2] : c.w[3];
        D[0] = b1 ? x23 : x01;
        D[1] = b1 ? y23 : y01;
        D[2] = b1 ? x01 : x23;
        D[3] = b1 ? y01 : y23;
    }
}

// The LDS address of a rotated gather: entry (k, j(t, lane)) of a table whose k-rows are 1 << SH bytes, k = the byte of D that step
// t uses.  ONE instruction where the chip has the byte dot product: v_dot4_u32_u8 addr, D, sel, c with sel = 1 << SH in the byte this
// lane uses at sub-step t & 3 and zero in the other three -- k * (1 << SH) + c, at most 255 * 128 + c: nothing carries between the
// bytes' products, and the three other bytes contribute nothing.  Else, and for rows of 256 bytes (the factor does not fit a byte), two:
// v_bfe_u32 takes the byte, v_lshl_add_u32 shifts it and adds c.  Either way c holds the table's LDS base, so that the result feeds the
// ds_read as it is (a pointer `tab + offset` costs one more add of the base per entry), and the addresses are the same numbers.
// A ds_read needs its address three wait states after a dot instruction wrote it: the callers compute the addresses of a whole
// pipeline unit before the unit's first read.  v_dot4_u32_u8 issues at the rate of either instruction it replaces (4.2 cycles per
// wave-instruction and SIMD, profiles/scan_dot4_ab.txt).  The selectors depend on the row size, which differs between the tables of
// one file, so they live beside the constants of a table (GatherConsts) and not in RotConsts.  The stream kernel (lopq_stream.hip)
// keeps the two-instruction address written out: converted, its one-query form measured 1 % slower (same file).
#if defined(__has_builtin)
#if __has_builtin(__builtin_amdgcn_udot4)
#define CIS_GATHER_DOT4 1
#endif
#endif
#ifndef CIS_GATHER_DOT4
#define CIS_GATHER_DOT4 0
#endif
template <int SH>
static constexpr bool gather_dot4() { return CIS_GATHER_DOT4 && SH <= 7; }

template <int M, int SH>
struct GatherConsts {
    uint32_t sel[4];  // dot4: the selector of sub-step tq, (1 << SH) << rc.sh[tq]; else rc.sh[tq]
    uint32_t c[M];    // LDS byte address of row 0's entry for step t
};

// tab: the table in LDS; entry (k, j) at byte (k << SH) + (j << (2 + LG)) -- rc.cj[t] << LG (rc.cj may carry more: two_copy_rot)
template <int M, int SH>
__device__ __forceinline__ GatherConsts<M, SH> make_gather(const RotConsts<M>& rc, const void* tab, int LG) {
    static_assert(SH >= 0 && (!gather_dot4<SH>() || (1 << SH) <= 255), "the row size is a factor of the byte dot product");
    GatherConsts<M, SH> gc;
    const uint32_t base = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)tab;
#pragma unroll
    for (int tq = 0; tq < 4; ++tq) gc.sel[tq] = gather_dot4<SH>() ? ((1u << SH) << rc.sh[tq]) : rc.sh[tq];
#pragma unroll
    for (int t = 0; t < M; ++t) gc.c[t] = base + (rc.cj[t] << LG);
    return gc;
}

template <int M, int SH>
__device__ __forceinline__ uint32_t gather_addr(const GatherConsts<M, SH>& gc, const uint32_t (&D)[(M + 3) / 4], int t) {
#if CIS_GATHER_DOT4
    if constexpr (gather_dot4<SH>()) return __builtin_amdgcn_udot4(D[t >> 2], gc.sel[t & 3], gc.c[t], false);
#endif
    return (__builtin_amdgcn_ubfe(D[t >> 2], gc.sel[t & 3], 8) << SH) + gc.c[t];
}

template <typename VT>
__device__ __forceinline__ VT gather_ld(uint32_t addr) {
    return *reinterpret_cast<const __attribute__((address_space(3))) VT*>((const __attribute__((address_space(3))) char*)(uintptr_t)addr);
}

// the same through a buffer descriptor that covers exactly the chunk being scanned: one 32-bit offset per
// load instead of 64-bit address arithmetic, and positions past the end of the chunk read as zero
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

template <int M>
__device__ __forceinline__ CodeWords<M> load_code_buf(__amdgpu_buffer_rsrc_t rs, int p) {
    CodeWords<M> c;
    if constexpr (M == 4) {
        c.w[0] = __builtin_amdgcn_raw_buffer_load_b32(rs, p * 4, 0, 0);
    } else if constexpr (M == 8) {
        const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(rs, p * 8, 0, 0);
        c.w[0] = v[0]; c.w[1] = v[1];
    } else {
        const u32x4_t v = __builtin_amdgcn_raw_buffer_load_b128(rs, p * 16, 0, 0);
        c.w[0] = v[0]; c.w[1] = v[1]; c.w[2] = v[2]; c.w[3] = v[3];
    }
    return c;
}

// Four consecutive float32 table entries (float4 number e4 of half table `tab`, nfK entries per half table): from the float32 copy when
// the batch has one, else converted from the float64 tables (round 5: the copy is a third of the tables kernel's writes -- 402 MB per C2
// batch -- and (float)T is the value the copy holds, so the scans see the same bits either way).
static __device__ __forceinline__ float4 tab_f4(const float* __restrict__ T32, const double* __restrict__ T, int64_t tab, int nfK, int e4) {
    if (T32) return reinterpret_cast<const float4*>(T32 + tab * nfK)[e4];   // (non-temporal loads here: no effect, round 6 same-box A/B)
    const double2* p = reinterpret_cast<const double2*>(T + tab * nfK) + 2 * e4;
    const double2 a = p[0], b = p[1];
    return make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
}
static __device__ __forceinline__ float tab_f1(const float* __restrict__ T32, const double* __restrict__ T, int64_t idx) {
    return T32 ? T32[idx] : (float)T[idx];
}

// ---- host: a run-time value as a compile-time constant -----------------------------------------------------------------------------
// f(std::integral_constant<int, V>) for the V of the list that equals v; false when none does.  Every M ladder of the launchers is one
// call of this; what a branch instantiates is narrowed with `if constexpr` inside f.
template <int... Vs, typename F>
static inline bool dispatch_int(int v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
// registers per lane of a wave's hit region (it holds NR * 64 - 8 entries): 4 up to limit 184, 8 up to 440, 16 above where NR_MAX allows
template <int NR_MAX, typename F>
static inline void dispatch_nr(int L, F&& f) {
    static_assert(NR_MAX == 8 || NR_MAX == 16, "dispatch_nr: the scans hold 8 or 16 registers per lane at most");
    if (L <= 184) f(std::integral_constant<int, 4>{});
    else if (NR_MAX == 8 || L <= 440) f(std::integral_constant<int, 8>{});
    else if constexpr (NR_MAX == 16) f(std::integral_constant<int, 16>{});
}

// ---- host: the operands of the launchers, filled once per batch ------------------------------------------------------------------------
struct SearchOut {  // any of these may be null; all are [nq][L] except n_found / visited [nq]
    cis_hit* hits;
    int64_t* ids;
    double* dists;
    int32_t* n_found;
    int32_t* cells;
    uint32_t* pos;
    int32_t* visited;
    SearchOut at(int64_t q0, int L) const {
        SearchOut o = *this;
        if (o.hits) o.hits += q0 * L;
        if (o.ids) o.ids += q0 * L;
        if (o.dists) o.dists += q0 * L;
        if (o.cells) o.cells += q0 * L;
        if (o.pos) o.pos += q0 * L;
        if (o.n_found) o.n_found += q0;
        if (o.visited) o.visited += q0;
        return o;
    }
};

// what every scan through the slot list reads and writes (run_fast_scan; the exact scan reads the work items alone)
struct ScanArgs {
    hipStream_t st;
    const WorkItem* items;
    int64_t n_items;
    int nq;
    const TabDesc* tabs;
    const int *slots, *n_slots;
    const PlanOut* plan;
    const double* T;
    const float* T32;  // null: the scans convert from T
    const uint8_t* codes;
    const int64_t* ids;
    int K, L;
    int* qctr;
    uint64_t* hits;  // survivors, S per work item (the exact scan: whole cis_hit records in the same workspace)
    int* hitn;
    float* slack;
    unsigned long long* qbound;
    int* fhdr;       // [32] zeroed: fall-back slot header of the sampled forms
    int* fslots;     // [n_slots * G]
};

// the candidate layout of the all-candidates and the streaming routes: candidates in retrieval order, query q owns seg[q] .. seg[q + 1)
struct CandArgs {
    hipStream_t st;
    const WorkItem* items;
    int64_t n_items;
    const int64_t* item_off;
    int64_t *cand_start, *seg;
    unsigned long long *qmin, *qmax;  // key range per query (null where nothing selects by it)
    int nq;
    const uint8_t* codes;
    int K;
};

// workgroups of a persistent scan: what the chip holds at `per_cu` per CU, fewer when the batch has fewer slots (of G work items) than that
static inline unsigned persistent_grid(const ScanArgs& a, int G, int per_cu) {
    const int64_t resident = 256 * (per_cu < 1 ? 1 : per_cu);
    const int64_t want = (a.n_items + G - 1) / G + 8;
    return (unsigned)(want < resident ? ((want + 7) / 8) * 8 : resident);
}

// ---- ADC scan v3 (lopq_scan3.hip): 16-bit fixed-point tables, four queries per workgroup ---------------------------
struct Scan3Geom { int G, NW, U, S, two_pass, long_chunks; size_t lds;
                   float sat = 0.f; };  // > 0: the sampled form's SATURATING scale (M = 16) -- see k_adc_scan4
bool scan3_supported(int M, int K, int L);
Scan3Geom scan3_geom(int M, int K, int L, int64_t avg_chunk /* candidates per work item of the batch */,
                     int force_two_pass /* -1: by chunk length, 0: streaming form, 1: two-pass form */);
void launch_scan3(int M, const Scan3Geom& g, const ScanArgs& a);

// ---- the HBM-streaming scan (lopq_stream.hip): few queries, very many candidates each --------------------------------------
static const int STREAM_B = 4096;     // buckets of sample minima per query (k_stream_tau: 1024 threads x 4; the k-th smallest of them, k <= B / 4, bounds the k-th smallest sample)
static const int STREAM_CAP = 16384;  // listed candidates per query at most
bool stream_supported(int M, int K, int L);
int stream_grid(int M, int G, int K, int64_t max_rows);
int stream_max_group();  // queries per slot at most (1, 2 or 4 are instantiated)
size_t stream_slot_bytes();  // one record per slot (lopq_stream.hip: StreamSlot), written by launch_stream_prep
struct StreamArgs {  // the route's own buffers, next to the candidate layout
    int M, G, L, grid;
    const int* slots;  // null: slot i = work item i alone
    int* n_slots;
    int64_t* rowoff;   // [n_slots + 1]: rows of the slots before each
    void* desc;        // [max_slots] records
    const double* T;
    const float* T32;
    float* tau;
    uint32_t* bmin;    // [nq][B] sample minima (k_stream_tau reads, then resets them)
    int B, sample_stride, flush /* sampled rows a lane folds into one bucket */;
    uint32_t* surv;    // [nq][cap] listed candidates, cnt[q] of them
    int* cnt;
    int cap;
    uint64_t* keys;    // [nq][cap] their exact keys
    const uint64_t *sel_keys, *sel_vals;  // [nq][stride] ranked pairs, nsel[q] of them
    const int* nsel;
    int64_t stride;
    const int64_t* ids;
    const PlanOut* plan;
    int* status;
};
void launch_stream_prep(const CandArgs& c, const StreamArgs& s, int64_t n_cand, const int64_t* d_totals /* null, or the plan totals: n_items and n_cand are bounds */);
void launch_stream_scan(const CandArgs& c, const StreamArgs& s, bool sample);
void launch_stream_tau(const CandArgs& c, const StreamArgs& s, int k);
void launch_stream_keys(const CandArgs& c, const StreamArgs& s);
void launch_stream_finish(const CandArgs& c, const StreamArgs& s, const SearchOut& out, int64_t* status_host_dev, int64_t seq);

// ---- merges of ranked hit lists: the work items of a query (lopq_search.hip), the shards' partial results (lopq_exchange.hip) ----
// block-wide bitonic sort of N (a power of two, chosen at run time) keys (a, b) with an optional payload, in LDS: the merge sorts
// only as many slots as it actually filled
template <int NT, bool PAY>
__device__ __forceinline__ void block_bitonic_rt(uint64_t* ka, uint64_t* kb, int64_t* pay, int N) {
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < N / 2; t += NT) {
                const int i = ((t / j) * 2 * j) + (t % j);
                const int p = i + j;
                const bool asc = ((i & k) == 0);
                const uint64_t a0 = ka[i], b0 = kb[i], a1 = ka[p], b1 = kb[p];
                const bool gt = (a0 > a1) || (a0 == a1 && b0 > b1);
                if (gt == asc) {
                    ka[i] = a1; kb[i] = b1; ka[p] = a0; kb[p] = b0;
                    if (PAY) { const int64_t x = pay[i]; pay[i] = pay[p]; pay[p] = x; }
                }
            }
            __syncthreads();
        }
    }
}

// ================================================================================================
// kernel: per-query merge of ranked lists -> top `limit` by (dist, visit_rank, pos)
// ================================================================================================
// Lists of query q: entries src[lo .. hi) in groups: list l has `stride` slots of which cnt[l]
// are valid (cnt == nullptr: a slot is valid when id >= 0).  Used twice: (a) merging the work
// items of a query, (b) merging the per-shard partial results after the all-gather.
template <int CAPM>
__device__ void merge_lists(const cis_hit* __restrict__ src, const int* __restrict__ cnt, int64_t first_list,
                            int n_lists, int64_t list_stride /* distance between lists, in hits */,
                            int slots, int limit, uint64_t* ka, uint64_t* kb, int64_t* pay, int* s_n,
                            cis_hit* __restrict__ out_hits /* [limit] or null */, int64_t* __restrict__ out_ids,
                            double* __restrict__ out_dists, int* __restrict__ out_n, int32_t* __restrict__ out_cells,
                            uint32_t* __restrict__ out_pos) {
    const int tid = threadIdx.x;
    int have = 0;      // sorted survivors currently in [0, have)
    int l = 0, e = 0;  // cursor: list l, entry e (uniform over the block)
    // rounds: append up to CAPM - have entries, sort, keep `limit`.  pay = index of the hit in src.
    while (true) {
        int n = have;
        int room = CAPM - have;
        while (l < n_lists && room > 0) {
            const int64_t lbase = (first_list + l) * list_stride;
            const int valid = cnt ? cnt[first_list + l] : slots;
            const int take = (valid - e < room) ? (valid - e) : room;
            for (int x = tid; x < take; x += blockDim.x) {
                const cis_hit hh = src[lbase + e + x];
                const bool ok = hh.id >= 0;
                ka[n + x] = ok ? (uint64_t)__double_as_longlong(hh.dist) : ~0ull;
                kb[n + x] = ok ? (((uint64_t)hh.visit_rank << 32) | hh.pos) : ~0ull;
                pay[n + x] = ok ? (lbase + e + x) : -1;
            }
            n += take;
            room -= take;
            e += take;
            if (e >= valid) { ++l; e = 0; }
        }
        int ns = 64;  // sort only the next power of two above what was filled
        while (ns < n) ns <<= 1;
        for (int x = n + tid; x < ns; x += blockDim.x) { ka[x] = ~0ull; kb[x] = ~0ull; pay[x] = -1; }
        __syncthreads();
        block_bitonic_rt<256, true>(ka, kb, pay, ns);
        have = n < limit ? n : limit;
        if (l >= n_lists) break;
    }
    // empty slots (id < 0) carry all-ones keys and therefore sit behind every real hit
    if (tid == 0) *s_n = 0;
    __syncthreads();
    int local = 0;
    for (int x = tid; x < have; x += blockDim.x) local += (pay[x] >= 0) ? 1 : 0;
    if (local) atomicAdd(s_n, local);
    __syncthreads();
    const int nv = *s_n;
    for (int x = tid; x < limit; x += blockDim.x) {
        cis_hit hh;
        if (x < nv) {
            hh = src[pay[x]];
        } else {
            hh.dist = __longlong_as_double(0x7ff0000000000000LL);
            hh.visit_rank = 0xffffffffu; hh.pos = 0xffffffffu; hh.id = -1; hh.cell = -1; hh.reserved = 0;
        }
        if (out_hits) out_hits[x] = hh;
        if (out_ids) {
            out_ids[x] = hh.id;
            out_dists[x] = (x < nv) ? hh.dist : __longlong_as_double(0x7ff8000000000000LL);
        }
        if (out_cells) out_cells[x] = hh.cell;
        if (out_pos) out_pos[x] = hh.pos;
    }
    if (tid == 0 && out_n) *out_n = nv;
}

static __device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
