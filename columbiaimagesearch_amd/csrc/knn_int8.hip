// The prefilter of the exact k nearest neighbours on int8 feature rows (cis_exact_knn_int8_dev; FeatureStore(storage=torch.int8)
// .search_exact), on the int8 matrix cores.  lopq_eval.hip keeps the driver, the exact chain, k_knn_finalize and the exact-only path;
// this file produces what k_knn_surface / k_knn_select produce there: per query the candidate rows that may be in the top k.
//
// The VALUE that ranks is lopq_eval.hip's: scipy's float64 chain and sqrt on the query and the DEQUANTISED row y_i = fl32((float)c_i s),
// the value cis_featstore_get_dev hands back (feat_int8.hip), widened.  This file only decides which rows the chain is run on.
//
// The scheme.  A float prefilter on scaled codes would have to bound the rounding of every product; an integer one has none.
//   k_knn_qdigits: per query t = max |x_i|, e its frexp exponent (t < 2^e), X_i = rint(x_i 2^(20-e)) in float64 (a power-of-two
//     scaling: exact), |X_i| <= 2^20, split into balanced base-128 digits X = 2^14 a + 2^7 b + c, b, c in [-64, 63], a in [-64, 64].
//   k_knn_rowstats_i8: per row ny32 = fl32(sum y_i^2 in float64), w_j = |s_j| sum |c_i| (the integer sum exact, the product exact in
//     float64: 24 + 23 bits), and the maxima of |y_j|^2 and w_j over the rows with a finite scale.
//   k_knn_surface_i8: A_j = sum a_i c_i, B_j, C_j on v_mfma_i32_32x32x32_i8, |.| <= 64 * 127 * d < 2^31 for d <= 65536: EXACT.  The
//     digits stay apart (2^14 A does not fit int32) until the epilogue: P = 2^14 A + 2^7 B + C = sum X_i c_i in float64, two fused
//     multiply-adds of integers below 2^44, exact; st = fl32(fma(-(s 2^(e-19)), P, ny32)) with the fma in float64: s 2^(e-19) is exact
//     (a power of two times 24 bits), so st is TWO roundings away from ny32 - 2 sum x~_i (c_i s), x~_i = X_i 2^(e-20): one in float64,
//     one to float32.  (The other way, combining in float32, rounds 2^14 A, the two adds, the product with s and the subtraction: five
//     terms in E, each u = 2^-24 of a value that can be 2^14 times the result's.  The listing at d = 128 has 16 x 2 x (3 v_cvt_f64_i32, 3
//     v_fma_f64, 1 v_mul_f64, 1 v_cvt_f32_f64) per lane and tile in float64 against 24 MFMAs of 16 passes; the float64 form was
//     chosen for the bound, it has not been timed against the float32 one.)
//
// The bound.  s(q, j) = |y|^2 - 2 x.y over the reals, u = 2^-24, n = |x| + max_j |y_j|, rows with a finite scale:
//   (a) the query's rounding: |x_i - x~_i| <= 2^(e-21), so 2 |sum (x_i - x~_i) c_i s| <= 2 2^(e-21) w_j = 2^(e-20) w_j.
//       |x~ - x| <= sqrt(d) 2^(e-21) <= 2^-12 |x| (t >= 2^(e-1), d <= 65536), so |x~| <= (1 + 2^-12) |x| below.
//   (b) y_i against c_i s, one float32 product: |y_i - c_i s| <= u |c_i s| + 2^-126 (rounding, and the underflow floor whether
//       or not subnormals are flushed), so 2 |sum x~_i (y_i - c_i s)| <= 2 u |x~||c s| + 2^-125 sqrt(d) |x~| <= 2u (1 + 2^-11) |x||y|
//       + 2^-116 n.
//   (c) ny32: the float64 sum d 2^-53 |y|^2, its one rounding u |y|^2.
//   (d) the epilogue: 2^-53 and u of |ny32| + 2 |x~||c s| <= (1 + 2^-11)(|y|^2 + 2 |x||y|), and 2^-126 for a result below the
//       float32 normals.
//   (e) the chain is within (d + 2) 2^-53 D <= (d + 2) 2^-53 n^2 of D, and sqrt merges chain values at most 2^-51 apart relatively
//       (lopq_eval.hip).
//   (b) + (c) + (d) <= 2u (1 + 2^-10) (|y|^2 + 2 |x||y|) <= 2^-22 n^2; E_q below takes 2^-21 n^2.  The float64 terms of (c), (d), (e)
//   are below (2 d + 8) 2^-53 n^2; E_q takes (d + 16) 2^-50 n^2.
//     E_q = 2^(e_q - 20) max_j w_j + (2^-21 + (d + 16) 2^-50) n^2 + 2^-116 (1 + n)
//   evaluated in float64, the threshold rounded UP to float32; n >= 2^60 keeps everything, as there.  Claim, lopq_eval.hip's: a row j
//   in the final top k has st(j) <= v_k + 2 E_q, v_k the k-th smallest group minimum.  k different rows have st <= v_k, hence chain
//   value <= v_k + |x|^2 + E'; j ranks among the first k by (sqrt(chain), index), so s(j) <= v_k + E_q and st(j) <= s(j) + E_q.
// Rows outside the bound: a row whose scale is NaN or infinite (a stored row with a non-finite component has s = NaN) gets ny32 = NaN,
// so its st is NaN, and it is left out of both maxima.  A NaN st is dropped from the group minima (they only have to be attained by
// real rows) and KEEPS the row in the emit pass: every comparison is written so that "false" keeps.  Such rows reach the chain, where
// their distance is NaN and ranks last.  A zero scale is a row of zeros: P counts for nothing, st = 0.
// Queries outside the bound: a non-finite component, or e outside [-100, 100] (inside it 2^(20-e), s 2^(e-19) >= 2^-268 and
// 2^(e-20) w are exact, normal float64 values; float32 queries of any sane scale lie inside): zero digits and a NaN threshold, so every row is
// kept, the list overflows for more than 3k + 512 rows and the exact-only kernel answers.  An all-zero query has e = 0 and zero digits.
//
// The split of k_knn_surface_i8: k_knn_surface's.  128 rows x 64 queries per workgroup of four waves, a wave owns 32 rows, grid
// (query tiles, S row splits), tiles dealt round-robin to the splits, the same 128 S groups per query, the same outputs.
//   A operand = row codes.  A lane of the 32x32x32 instruction holds 16 int8: one 16-byte row word.  Integer sums are exact in any
//   order, so which k a (lane half, byte) means is free as long as A and B agree: within a span of 128 dims = 8 words, lane half h
//   takes words 4h .. 4h + 3, one per K step, so a lane reads 64 consecutive bytes of its row with four 16-byte loads, global ->
//   VGPR -> matrix core, never through LDS.  The next span's four words are requested before the current span's 24 MFMAs issue.
//   B operand = the digits of the tile's 64 queries, staged in LDS once per span (24 KB, shared by the four waves) in the order the
//   lanes consume them: 16-byte word (((j 3 + g) 4 + s) 64 + lane) is digit g of query 32 j + (lane & 31), word 4 (lane >> 5) + s of the
//   span, so a ds_read_b128 reads 64 consecutive words: conflict-free.  k_knn_qdigits writes the workspace in exactly that order, per
//   (query tile, span), zero-filled past m1 and past d, so staging is a straight copy: six coalesced loads and six conflict-free
//   stores per thread.
//   Per K step 6 MFMAs per wave (2 query blocks x 3 digits) into 6 x 16 int32 accumulators.  d % 32 == 16: the last step's upper
//   lane half feeds zeros (row words past d are replaced by zero; the digits there are zero too); steps without any word are skipped;
//   there is no scalar tail.  Rows past m2 read row m2 - 1 and are masked in the epilogue.
#include <algorithm>
#include <climits>

#include "knn_int8.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 64;         // workgroup tile (rows x queries)
constexpr int SPAN_WORDS = 8;            // 16-byte words of a row per stage
constexpr int STAGE_WORDS = 2 * 3 * 4 * 64;  // 16-byte digit words per (query tile, span)
constexpr int FLAGGED = INT_MIN;         // qe of a query the prefilter does not serve
constexpr int E_MIN = -100, E_MAX = 100;

__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double two_to(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }  // e in [-1022, 1023]

// One query per wave, queries [0, m1 padded to 64).  Pass 1: the largest magnitude and whether a component is not finite; pass 2: the
// digits, a lane per 16-dim word, into the order of the file header.
template <typename TQ>
__global__ __launch_bounds__(256) void k_knn_qdigits(const TQ* __restrict__ Q, int m1, int d, i32x4* __restrict__ digits, int* __restrict__ qe) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nw = d >> 4, nsp = (nw + SPAN_WORDS - 1) / SPAN_WORDS;
    const TQ* x = Q + (int64_t)q * d;
    double t = 0.0;
    int bad = 0;
    if (q < m1) {
        for (int i = lane; i < d; i += 64) {
            const double a = fabs((double)x[i]);
            bad |= !(a <= 1.7976931348623157e308) ? 1 : 0;  // +-inf and NaN
            t = a > t ? a : t;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(t, o);
        t = u > t ? u : t;
        bad |= __shfl_xor(bad, o);
    }
    int e = 0;  // frexp: t in [2^(e-1), 2^e); a subnormal t reads as e = -1022 and is flagged
    if (t > 0.0) e = (int)((__double_as_longlong(t) >> 52) & 0x7ff) - 1022;
    const bool live = q < m1 && !bad && e >= E_MIN && e <= E_MAX;
    if (lane == 0) qe[q] = (live || q >= m1) ? e : FLAGGED;
    const double scale = two_to(live ? 20 - e : 0);
    i32x4* out = digits + (int64_t)(q >> 6) * nsp * STAGE_WORDS + ((q >> 5) & 1) * 3 * 4 * 64 + (q & 31);
    for (int w = lane; w < nsp * SPAN_WORDS; w += 64) {
        i32x4 p[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        if (live && w < nw) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int X = (int)rint((double)x[16 * w + i] * scale);
                const int c = ((X + 64) & 127) - 64;
                const int X1 = (X - c) >> 7;  // (exact: X - c is a multiple of 128)
                const int b = ((X1 + 64) & 127) - 64;
                const int a = (X1 - b) >> 7;
                p[0][i >> 2] |= (a & 0xff) << (8 * (i & 3));
                p[1][i >> 2] |= (b & 0xff) << (8 * (i & 3));
                p[2][i >> 2] |= (c & 0xff) << (8 * (i & 3));
            }
        }
        const int sp = w >> 3, h = (w >> 2) & 1, s = w & 3;
#pragma unroll
        for (int g = 0; g < 3; ++g) out[(int64_t)sp * STAGE_WORDS + (g * 4 + s) * 64 + h * 32] = p[g];
    }
}

// One wave per row: stat[row] = (ny32, s), or (NaN, NaN) for a scale that is not finite; the maxima over the other rows.
__global__ __launch_bounds__(256) void k_knn_rowstats_i8(const unsigned char* __restrict__ rows, int64_t m2, int d, float* __restrict__ stat,
                                                         unsigned long long* __restrict__ maxima) {
    const int lane = threadIdx.x & 63;
    const int64_t row_bytes = 16 + (int64_t)d;
    unsigned long long best_y = 0, best_w = 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < m2; r += (int64_t)gridDim.x * 4) {
        const i32x4* p = (const i32x4*)(rows + r * row_bytes);
        const float s = *(const float*)p;
        double acc = 0.0;
        int isum = 0;
        for (int w = lane; w < (d >> 4); w += 64) {
            const i32x4 v = p[1 + w];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int c = (int)(int8_t)(v[i >> 2] >> (8 * (i & 3)));
                const double y = (double)((float)c * s);
                acc = acc + y * y;
                isum += c < 0 ? -c : c;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            acc = acc + __shfl_xor(acc, o);
            isum += __shfl_xor(isum, o);
        }
        const bool finite = fabsf(s) <= 3.402823466e+38f;
        if (lane == 0) {
            stat[2 * r] = finite ? (float)acc : __uint_as_float(0x7fc00000u);
            stat[2 * r + 1] = finite ? s : __uint_as_float(0x7fc00000u);
        }
        if (finite) {
            const unsigned long long by = (unsigned long long)__double_as_longlong(acc);  // >= 0 and finite: the bits order as the values
            const unsigned long long bw = (unsigned long long)__double_as_longlong(fabs((double)s) * (double)isum);
            best_y = by > best_y ? by : best_y;
            best_w = bw > best_w ? bw : best_w;
        }
    }
    if (lane == 0 && best_y) atomicMax(maxima, best_y);
    if (lane == 0 && best_w) atomicMax(maxima + 1, best_w);
}

// st(q, j) from the int8 matrix cores: the file header.  Result register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of query
// l & 31, as for every 32x32 MFMA.
template <int EMIT>
__global__ __launch_bounds__(256) void k_knn_surface_i8(const unsigned char* __restrict__ rows, int m2, int d, const i32x4* __restrict__ digits,
                                                        const int* __restrict__ qe, int m1, const float* __restrict__ stat, int S,
                                                        float* __restrict__ gmin, const float* __restrict__ thr, int* __restrict__ cnt,
                                                        int64_t* __restrict__ cand, int W, int cap, int64_t base) {
    __shared__ i32x4 sB[STAGE_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int q0 = blockIdx.x * BN, split = blockIdx.y;
    const int nw = d >> 4, nsp = (nw + SPAN_WORDS - 1) / SPAN_WORDS;
    const int ntiles = (m2 + BM - 1) / BM;
    const int my_tiles = split < ntiles ? (ntiles - split + S - 1) / S : 0;
    const int n_stages = my_tiles * nsp;
    const int64_t row_bytes = 16 + (int64_t)d;
    const i32x4* dq = digits + (int64_t)blockIdx.x * nsp * STAGE_WORDS + tid;
    const i32x4 zero = {0, 0, 0, 0};

    i32x4 na[4], nb[6];  // the next stage's row words and this thread's share of its digits
    auto fetch = [&](int st) {
        const int tile = split + (st / nsp) * S, sp = st % nsp;
        int row = tile * BM + wave * 32 + (lane & 31);
        row = row < m2 ? row : m2 - 1;
        const int w0 = sp * SPAN_WORDS + 4 * h;
        const i32x4* rp = (const i32x4*)(rows + (int64_t)row * row_bytes) + 1 + w0;
#pragma unroll
        for (int s = 0; s < 4; ++s) na[s] = w0 + s < nw ? rp[s] : zero;
#pragma unroll
        for (int i = 0; i < 6; ++i) nb[i] = dq[(int64_t)sp * STAGE_WORDS + 256 * i];
    };

    float mins[2][16];
    float tq[2];
    double sq[2];  // 2^(e_q - 19)
    bool qok[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = q0 + j * 32 + (lane & 31);
        qok[j] = q < m1;
        tq[j] = (EMIT && qok[j]) ? thr[q] : 0.f;
        const int e = qok[j] ? qe[q] : FLAGGED;
        sq[j] = e == FLAGGED ? 0.0 : two_to(e - 19);
#pragma unroll
        for (int r = 0; r < 16; ++r) mins[j][r] = __builtin_inff();
    }
    i32x16 acc[2][3];
    if (n_stages > 0) fetch(0);
    for (int st = 0; st < n_stages; ++st) {
        const int sp = st % nsp;
        __syncthreads();  // the previous stage's digits have been read
#pragma unroll
        for (int i = 0; i < 6; ++i) sB[tid + 256 * i] = nb[i];
        i32x4 a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] = na[s];
        __syncthreads();
        if (st + 1 < n_stages) fetch(st + 1);
        if (sp == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 3; ++g)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[j][g][r] = 0;
        }
        const int steps = nw - sp * SPAN_WORDS;  // steps in which the lower lane half has a word (the same for every lane)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s < steps) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int g = 0; g < 3; ++g)
                        acc[j][g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], sB[((j * 3 + g) * 4 + s) * 64 + lane], acc[j][g], 0, 0, 0);
            }
        }
        if (sp == nsp - 1) {
            const int rowb = (split + (st / nsp) * S) * BM + wave * 32 + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rowb + (r & 3) + 8 * (r >> 2);
                const bool rok = row < m2;
                const double ny = rok ? (double)stat[2 * row] : (double)__builtin_inff();
                const double rs = rok ? (double)stat[2 * row + 1] : 0.0;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const double P = fma(16384.0, (double)acc[j][0][r], fma(128.0, (double)acc[j][1][r], (double)acc[j][2][r]));
                    const float sv = (float)fma(-(rs * sq[j]), P, ny);
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
            float* g = gmin + (int64_t)(q0 + j * 32 + (lane & 31)) * G + ((split * 4 + wave) * 2 + h) * 16;
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = mins[j][r];
        }
    }
}

// k_knn_select with this file's E_q: thr[q] = float32 round-up of v_k + 2 E_q, v_k the k-th smallest of the query's G group minima
// (G >= 2k, no NaN among them); NaN for a flagged query.
__global__ __launch_bounds__(256) void k_knn_select_i8(const float* __restrict__ gmin, int G, int k, int d, const double* __restrict__ xn2,
                                                       const int* __restrict__ qe, const unsigned long long* __restrict__ maxima,
                                                       float* __restrict__ thr) {
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
            const int e = qe[q];
            const double n = __dsqrt_rn(xn2[q]) + __dsqrt_rn(__longlong_as_double((long long)maxima[0]));
            const double wmax = __longlong_as_double((long long)maxima[1]);
            const double E = (e == FLAGGED ? 0.0 : two_to(e - 20)) * wmax + (0x1p-21 + (double)(d + 16) * 0x1p-50) * n * n + 0x1p-116 * (1.0 + n);
            // n < 2^60 keeps every float32 intermediate finite, as in k_knn_select
            const double T = (e != FLAGGED && n < 0x1p60) ? (double)vi + 2.0 * E : nan64();
            float f = (float)T;
            if ((double)f < T) f = nextafterf(f, __builtin_inff());
            thr[q] = f;  // NaN: every row is kept, and a long list overflows into the exact path
        }
    }
}

}  // namespace

int cis_knn_i8_prefilter(const KnnI8Args& a, hipStream_t st) {
    const int nqt = (int)ceil_div(a.m1, BN), G = a.S * 128;
    const dim3 grid((unsigned)nqt, (unsigned)a.S);
    i32x4* digits = (i32x4*)a.digits;
    hipLaunchKernelGGL(k_knn_rowstats_i8, dim3((unsigned)std::min<int64_t>(ceil_div(a.m2, 4), 4096)), dim3(256), 0, st, a.rows, (int64_t)a.m2,
                       a.d, a.stat, a.maxima);
    if (a.q_f64)
        hipLaunchKernelGGL(k_knn_qdigits<double>, dim3((unsigned)(nqt * BN / 4)), dim3(256), 0, st, (const double*)a.Q, a.m1, a.d, digits, a.qe);
    else
        hipLaunchKernelGGL(k_knn_qdigits<float>, dim3((unsigned)(nqt * BN / 4)), dim3(256), 0, st, (const float*)a.Q, a.m1, a.d, digits, a.qe);
    hipLaunchKernelGGL(k_knn_surface_i8<0>, grid, dim3(256), 0, st, a.rows, a.m2, a.d, digits, a.qe, a.m1, a.stat, a.S, a.gmin,
                       (const float*)nullptr, (int*)nullptr, (int64_t*)nullptr, a.W, a.cap, a.base);
    hipLaunchKernelGGL(k_knn_select_i8, dim3((unsigned)a.m1), dim3(256), (size_t)G * 4, st, a.gmin, G, a.k, a.d, a.xn2, a.qe, a.maxima, a.thr);
    hipLaunchKernelGGL(k_knn_surface_i8<1>, grid, dim3(256), 0, st, a.rows, a.m2, a.d, digits, a.qe, a.m1, a.stat, a.S, (float*)nullptr,
                       a.thr, a.cnt, a.cand, a.W, a.cap, a.base);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}
