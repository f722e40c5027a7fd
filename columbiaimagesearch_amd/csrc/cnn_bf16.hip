// DeepSentibank's convolutions and fully connected layers on the 16-bit matrix cores of gfx950 (v_mfma_f32_32x32x16_bf16),
// as two opt-in precisions of the network (cis_cnn_set_precision):
//   bf16x3  every float32 operand x is split as hi = bf16_rne(x), lo = bf16_rne(x - hi) (x - hi is exact in float32) and every product
//           is formed as a_hi*b_hi + a_hi*b_lo + a_lo*b_hi with float32 accumulation: three MFMAs per 16-deep k step where the float32
//           kernel issues eight 32x32x2 ones.  What is dropped: a_lo*b_lo and the two residues x - hi - lo, each <= 2^-16 |a||b|.
//   bf16    a_hi*b_hi alone.
// Activations stay float32 in memory between layers; pooling, LRN and the split-K reduction are the float32 forward's own kernels.
//
// One implicit-GEMM family k_conv_igemm_bf16<WM, WN, WAVES_M, WAVES_N, PLANES, NS>: M = output pixels, N = output channels of a group,
// 256 threads = 4 waves laid out WAVES_M x WAVES_N, a wave owns WM x WN tiles of 32 x 32.
//
// K stage: 32 (two MFMA k steps).  K is cut into runs of 8 consecutive k; a thread gathers one run of one pixel per pass as two 16-byte
// loads of float32 and a stage is four runs per row.  On channels-last input (ICg % 8 == 0) a run is 8 channels of one kernel tap, so
// each thread carries its own (ky, kx, ic) and a stage may straddle taps (ICg = 48).  On the first layer's NCHW planes
// (PLANES) k = (ic * KH + ky) * 4 * runq + kx as in the float32 kernel, and each of the two float4 of a run is decoded on its own
// (a 12-float kernel row is one and a half runs).  K that is no multiple of 32 (363 -> 396 -> 416, 1200) meets zero weights and zeroed
// activations in the last stage, never a scalar loop.
//
// LDS: operands as bf16, k-contiguous: A[plane][BM][40], B[plane][BN][40] (plane = hi, lo; NS = 1 has the hi plane only).  A lane's MFMA
// operand is eight consecutive k of row lane & 31 at k = 8 * (lane >> 5): one ds_read_b128.  The row stride is 40 bf16 = 80 bytes, 5 x 16 B:
// an odd number of 16-byte units, so any 8 (16) consecutive rows at the same k offset start on 8 (16) different 16-byte bank groups of a
// 32-bank (64-bank) LDS and the 64 lanes' reads pile onto no bank; the plain stride of 64 B would put every other row on the same banks.
// One stage buffer (128 x 128, NS = 3: 40 KB; four workgroups fit a CU's LDS): the next stage's operands are fetched into registers before
// the MFMAs, and written to LDS between two barriers after them; other workgroups of the CU run through the barriers.
//
// Weights are split and packed once on the host (cnn_bf16_pack): [plane][group][Kp / 8][OCg][8] bf16, so a thread's 16-byte global load is
// its 16-byte LDS store, consecutive threads take consecutive output channels, and nothing is converted in the loop.  Activations are
// split once per element when the gathered registers go to LDS; padding, rows past the tile and k past K are zeroed there (the fetch is
// unconditional loads from clamped addresses, as in cnn.hip).
//
// Order of a sum (fixed, the same for every pixel, tile shape and batch position): k ascending in steps of 16; inside a step hi*hi,
// then hi*lo (activation hi, weight lo), then lo*hi, all into the one float32 accumulator; under split-K the partial sums of the K ranges
// are added in ascending order by k_splitk_reduce.
// Epilogue as the float32 kernel: bias, the residual d.res[pixel][d.resC] for output channels below d.resC (the dlib net's add_prev),
// optional ReLU, or raw partial sums under split-K.  Tuned for the shapes of DeepSentibank; it also serves the dlib net's 3x3 layers
// that the direct kernel of cnn_bf16_direct.hip does not.  Shapes it does not serve are refused by launch_conv_bf16.
#include <vector>
#include "common.h"
#include "cnn_conv.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <int WM, int WN, int WAVES_M, int WAVES_N, bool PLANES, int NS>
__global__ __launch_bounds__(256, 2) void k_conv_igemm_bf16(const float* __restrict__ in, const uint16_t* __restrict__ Wp,
                                                           const float* __restrict__ bias, float* __restrict__ out, ConvDesc d) {
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per block");
    static_assert(NS == 1 || NS == 3, "plain or split");
    constexpr int BM = WAVES_M * WM * 32, BN = WAVES_N * WN * 32, BK = 32, LDK = 40;
    constexpr int NP = NS == 3 ? 2 : 1;              // operand planes
    constexpr int A_IT = (BM + 63) / 64;             // (row, run) passes of the gather: 64 rows x 4 runs per pass
    constexpr int B_IT = (BN * 4 + 255) / 256;       // 16-byte copies of packed weights per plane
    __shared__ __attribute__((aligned(16))) uint16_t As[NP][BM][LDK];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[NP][BN][LDK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int g = d.splitk > 1 ? 0 : blockIdx.z;
    const int ksplit = d.splitk > 1 ? blockIdx.z : 0;
    const int64_t npix = (int64_t)d.N * d.OH * d.OW;
    const int64_t pix0 = (int64_t)blockIdx.x * BM;
    const int oc0 = blockIdx.y * BN;  // inside the group
    const int run = tid & 3;          // this thread's run of 8 k inside a stage
    int iy0[A_IT], ix0[A_IT];
    int64_t pbase[A_IT];
    bool rowok[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int m = (tid >> 2) + 64 * i;
        const int64_t p = pix0 + m;
        rowok[i] = m < BM && p < npix;
        if (rowok[i]) {
            const int ox = (int)(p % d.OW);
            const int oy = (int)((p / d.OW) % d.OH);
            const int64_t img = p / ((int64_t)d.OW * d.OH);
            iy0[i] = oy * d.stride - d.pad;
            ix0[i] = ox * d.stride - d.pad;
            pbase[i] = img * d.sN + (int64_t)g * d.ICg * d.sC;
        } else {
            iy0[i] = 0; ix0[i] = 0; pbase[i] = 0;  // a valid address; zeroed on the way to LDS
        }
    }
    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int Kp8 = ((d.K + BK - 1) / BK) * (BK / 8);  // runs of the packed weights per group
    const int64_t plane_stride = (int64_t)d.groups * Kp8 * d.OCg * 8;
    const uint16_t* Wg = Wp + (int64_t)g * Kp8 * d.OCg * 8;
    const int nkt_all = Kp8 / 4;
    const int nkt_per = (nkt_all + d.splitk - 1) / d.splitk;
    const int kt_begin = ksplit * nkt_per;
    const int nkt = (kt_begin + nkt_per < nkt_all) ? kt_begin + nkt_per : nkt_all;
    // this thread's place on the K axis, carried from stage to stage
    int ky = 0, kx = 0, ic = 0;                          // channels-last: its run = 8 channels from ic of tap (ky, kx)
    int q_r[2] = {0, 0}, q_j[2] = {0, 0}, q_ic[2] = {0, 0}, q_ky[2] = {0, 0};  // PLANES: its two float4 = quad q_j of run q_r = (q_ic, q_ky)
    if constexpr (PLANES) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int kq = kt_begin * 8 + run * 2 + h;
            q_r[h] = kq / d.runq; q_j[h] = kq - q_r[h] * d.runq;
            q_ic[h] = q_r[h] / d.KH; q_ky[h] = q_r[h] - q_ic[h] * d.KH;
        }
    } else {
        const int k8 = kt_begin * BK + run * 8;
        const int t = k8 / d.ICg;
        ic = k8 - t * d.ICg;
        ky = t / d.KW; kx = t - ky * d.KW;
    }
    float4 ra[A_IT][2];
    uint4 rb[NP][B_IT];
    bool okA[A_IT][2], okB[B_IT];
    int shA[PLANES ? A_IT : 1][2];
    auto fetch = [&](int kt) {
        if constexpr (PLANES) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bool kin = q_r[h] < d.run_planes;
                const int ric = kin ? q_ic[h] : 0;
#pragma unroll
                for (int i = 0; i < A_IT; ++i) {
                    const int iy = iy0[i] + q_ky[h];
                    okA[i][h] = rowok[i] && kin;  // (pad == 0: every tap of a valid pixel is inside)
                    const int iyc = iy < d.H ? iy : d.H - 1;
                    const int64_t off = pbase[i] + (int64_t)ric * d.sC + (int64_t)(iyc * (int)d.sH + ix0[i] + q_j[h] * 4);
                    const int64_t over = off + 4 - d.in_elems;  // 1 ... 3 for the last runs of the last plane, else <= 0
                    const int sh = over > 0 ? (int)over : 0;
                    shA[i][h] = sh;
                    ra[i][h] = *reinterpret_cast<const float4*>(in + (off - sh));
                }
                q_j[h] += 8;
                while (q_j[h] >= d.runq) {
                    q_j[h] -= d.runq; ++q_r[h];
                    if (++q_ky[h] == d.KH) { q_ky[h] = 0; ++q_ic[h]; }
                }
            }
        } else {
            const bool kin = ky < d.KH;
#pragma unroll
            for (int i = 0; i < A_IT; ++i) {
                const int iy = iy0[i] + ky, ix = ix0[i] + kx;
                okA[i][0] = okA[i][1] = rowok[i] && kin && iy >= 0 && iy < d.H && ix >= 0 && ix < d.W;
                const int iyc = iy < 0 ? 0 : (iy < d.H ? iy : d.H - 1);
                const int ixc = ix < 0 ? 0 : (ix < d.W ? ix : d.W - 1);
                const float* p = in + pbase[i] + (int64_t)iyc * d.sH + (int64_t)ixc * d.sW + ic;
                ra[i][0] = *reinterpret_cast<const float4*>(p);
                ra[i][1] = *reinterpret_cast<const float4*>(p + 4);
            }
            ic += BK;
            while (ic >= d.ICg) { ic -= d.ICg; if (++kx == d.KW) { kx = 0; ++ky; } }
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int idx = tid + 256 * i;
            const int idc = idx < BN * 4 ? idx : BN * 4 - 1;
            const int kql = idc / BN, ocl = idc - kql * BN;
            okB[i] = idx < BN * 4 && oc0 + ocl < d.OCg;
            const int oc = oc0 + ocl < d.OCg ? oc0 + ocl : d.OCg - 1;
            const uint16_t* p = Wg + ((int64_t)(kt * 4 + kql) * d.OCg + oc) * 8;
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) rb[pl][i] = *reinterpret_cast<const uint4*>(p + pl * plane_stride);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const int m = (tid >> 2) + 64 * i;
            if (m < BM) {
                float v[8];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float4 q = ra[i][h];
                    if constexpr (PLANES) {  // a load that was moved back from the end of the input: its floats move down, zeros follow
                        const int sh = shA[i][h];
                        q = make_float4(sh == 0 ? q.x : (sh == 1 ? q.y : (sh == 2 ? q.z : q.w)), sh == 0 ? q.y : (sh == 1 ? q.z : (sh == 2 ? q.w : 0.f)),
                                        sh == 0 ? q.z : (sh == 1 ? q.w : 0.f), sh == 0 ? q.w : 0.f);
                    }
                    const bool ok = okA[i][h];
                    v[4 * h + 0] = ok ? q.x : 0.f; v[4 * h + 1] = ok ? q.y : 0.f;
                    v[4 * h + 2] = ok ? q.z : 0.f; v[4 * h + 3] = ok ? q.w : 0.f;
                }
                uint32_t hi[8], lo[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if constexpr (NS == 3) bf16_split(v[e], hi[e], lo[e]);
                    else hi[e] = bf16_rne(v[e]);
                }
                *reinterpret_cast<uint4*>(&As[0][m][run * 8]) =
                    make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
                if constexpr (NS == 3)
                    *reinterpret_cast<uint4*>(&As[NP - 1][m][run * 8]) =
                        make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
            }
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int idx = tid + 256 * i;
            if (idx < BN * 4) {
                const int kql = idx / BN, ocl = idx - kql * BN;
#pragma unroll
                for (int pl = 0; pl < NP; ++pl)
                    *reinterpret_cast<uint4*>(&Bs[pl][ocl][kql * 8]) = okB[i] ? rb[pl][i] : make_uint4(0u, 0u, 0u, 0u);
            }
        }
    };
    if (kt_begin < nkt) {
        fetch(kt_begin);
        stash();
    }
    __syncthreads();
    for (int kt = kt_begin; kt < nkt; ++kt) {
        if (kt + 1 < nkt) fetch(kt + 1);
#pragma unroll
        for (int ks = 0; ks < BK; ks += 16) {
            bf16x8 a[NP][WM], b[NP][WN];
            const int ko = ks + 8 * (lane >> 5);
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
                for (int i = 0; i < WM; ++i) a[pl][i] = *reinterpret_cast<const bf16x8*>(&As[pl][(wm * WM + i) * 32 + (lane & 31)][ko]);
#pragma unroll
                for (int j = 0; j < WN; ++j) b[pl][j] = *reinterpret_cast<const bf16x8*>(&Bs[pl][(wn * WN + j) * 32 + (lane & 31)][ko]);
            }
            // products in the order hi*hi, hi*lo, lo*hi; the tiles of a wave are interleaved between two products of one tile
#pragma unroll
            for (int pr = 0; pr < NS; ++pr) {
                const int pa = pr == 2 ? NP - 1 : 0, pb = pr == 1 ? NP - 1 : 0;
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa][i], b[pb][j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave has read this stage
        if (kt + 1 < nkt) stash();
        __syncthreads();
    }
    // ---- epilogue: C/D layout col = lane&31 (oc), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (pixel) ----
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int ocl = oc0 + (wn * WN + j) * 32 + (lane & 31);
        if (ocl >= d.OCg) continue;
        const float bv = bias ? bias[g * d.OCg + ocl] : 0.f;
#pragma unroll
        for (int i = 0; i < WM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                const int64_t p = pix0 + (wm * WM + i) * 32 + row;
                if (p < npix) {
                    if (d.splitk > 1) {
                        out[(int64_t)ksplit * d.part_stride + p * d.OC + ocl] = acc[i][j][r];  // raw partial sum
                    } else {
                        float v = acc[i][j][r] + bv;
                        if (d.res && ocl < d.resC) v += d.res[p * d.resC + ocl];  // (groups == 1: launch_conv_bf16)
                        if (d.relu) v = v > 0.f ? v : 0.f;
                        out[p * d.OC + g * d.OCg + ocl] = v;
                    }
                }
            }
        }
    }
}

// ================================================================================================
// host
// ================================================================================================
int cnn_bf16_pack(uint16_t** d_out, const float* w, int groups, int K, int OCg, int with_lo) {
    *d_out = nullptr;
    const int Kp8 = ((K + 31) / 32) * 4, np = with_lo ? 2 : 1;
    const size_t plane = (size_t)groups * Kp8 * OCg * 8;
    std::vector<uint16_t> pk(plane * np, 0);
    for (int g = 0; g < groups; ++g)
        for (int k = 0; k < K; ++k) {
            const float* src = w + ((size_t)g * K + k) * OCg;
            uint16_t* dst = pk.data() + ((size_t)(g * Kp8 + k / 8) * OCg) * 8 + (k & 7);
            for (int o = 0; o < OCg; ++o) {
                uint32_t hi, lo;
                bf16_split(src[o], hi, lo);
                dst[(size_t)o * 8] = (uint16_t)hi;
                if (with_lo) dst[plane + (size_t)o * 8] = (uint16_t)lo;
            }
        }
    CIS_CHECK_HIP(hipMalloc((void**)d_out, pk.size() * sizeof(uint16_t)));
    CIS_CHECK_HIP(hipMemcpy(*d_out, pk.data(), pk.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return CIS_OK;
}

template <int WM, int WN, int WAVES_M, int WAVES_N>
static void launch_bf16_cfg(const ConvDesc& d, const float* in, const uint16_t* w, const float* b, float* out, int ns, hipStream_t st) {
    constexpr int BM = WAVES_M * WM * 32, BN = WAVES_N * WN * 32;
    const int64_t npix = (int64_t)d.N * d.OH * d.OW;
    dim3 g((unsigned)ceil_div(npix, BM), (unsigned)ceil_div(d.OCg, BN), (unsigned)(d.splitk > 1 ? d.splitk : d.groups));
    if (d.run_planes > 0) {
        if (ns == 3) hipLaunchKernelGGL((k_conv_igemm_bf16<WM, WN, WAVES_M, WAVES_N, true, 3>), g, dim3(256), 0, st, in, w, b, out, d);
        else hipLaunchKernelGGL((k_conv_igemm_bf16<WM, WN, WAVES_M, WAVES_N, true, 1>), g, dim3(256), 0, st, in, w, b, out, d);
    } else {
        if (ns == 3) hipLaunchKernelGGL((k_conv_igemm_bf16<WM, WN, WAVES_M, WAVES_N, false, 3>), g, dim3(256), 0, st, in, w, b, out, d);
        else hipLaunchKernelGGL((k_conv_igemm_bf16<WM, WN, WAVES_M, WAVES_N, false, 1>), g, dim3(256), 0, st, in, w, b, out, d);
    }
}

int launch_conv_bf16(const ConvDesc& d, const float* in, const uint16_t* w, const float* b, float* out, int ns, hipStream_t st) {
    CIS_REQUIRE(ns == 1 || ns == 3, "16-bit convolution: ns must be 1 or 3");
    CIS_REQUIRE(d.splitk <= 1 || d.groups == 1, "16-bit convolution: a K split needs groups == 1");
    CIS_REQUIRE(d.res == nullptr || (d.groups == 1 && d.resC >= 1), "16-bit convolution: a residual input needs groups == 1");
    if (d.run_planes > 0) {
        CIS_REQUIRE(d.pad == 0 && d.groups == 1 && d.sW == 1 && d.runq * 4 >= d.KW && d.run_planes == d.ICg * d.KH && d.K == d.run_planes * d.runq * 4 &&
                        d.in_elems >= 4,
                    "16-bit convolution: the NCHW plane gather needs pad == 0, groups == 1 and kernel rows padded to float4");
    } else {
        CIS_REQUIRE(d.sC == 1 && d.ICg % 8 == 0 && d.K == d.KH * d.KW * d.ICg,
                    "16-bit convolution: channels-last input with a multiple of 8 channels per group (got %d)", d.ICg);
    }
    const int64_t npix = (int64_t)d.N * d.OH * d.OW;
    const int z = d.splitk > 1 ? d.splitk : d.groups;
    auto blocks = [&](int bm, int bn) { return ceil_div(npix, bm) * ceil_div(d.OCg, bn) * z; };
    const int64_t want = 2 * 256;  // at least two workgroups per CU, else a smaller tile (the tile shape does not change a sum's order)
    if (d.OCg <= 32) launch_bf16_cfg<1, 1, 4, 1>(d, in, w, b, out, ns, st);                        // 128 x 32
    else if (npix <= 2048) {                                                                      // the fc layers
        if (npix >= 64) launch_bf16_cfg<1, 2, 2, 2>(d, in, w, b, out, ns, st);                     // 64 x 128
        else launch_bf16_cfg<1, 1, 1, 4>(d, in, w, b, out, ns, st);                                // 32 x 128
    } else if (d.OCg <= 64) {
        if (blocks(128, 64) >= want) launch_bf16_cfg<2, 1, 2, 2>(d, in, w, b, out, ns, st);        // 128 x 64
        else launch_bf16_cfg<1, 1, 2, 2>(d, in, w, b, out, ns, st);                                // 64 x 64
    } else if (d.OCg % 96 == 0 && d.OCg % 128 != 0) launch_bf16_cfg<1, 3, 4, 1>(d, in, w, b, out, ns, st);  // 96, 192: 128 x 96
    else if (blocks(128, 128) >= want) launch_bf16_cfg<2, 2, 2, 2>(d, in, w, b, out, ns, st);      // 128 x 128
    else if (blocks(128, 64) >= want) launch_bf16_cfg<2, 1, 2, 2>(d, in, w, b, out, ns, st);       // 128 x 64
    else launch_bf16_cfg<1, 1, 2, 2>(d, in, w, b, out, ns, st);                                    // 64 x 64
    return CIS_OK;
}
