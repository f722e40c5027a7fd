// The dlib face ResNet's stride-1 3x3 layers on the 16-bit matrix cores of gfx950 (v_mfma_f32_32x32x16_bf16): a direct kernel for the
// two shapes that hold half of the network's multiply-adds, 35 x 35 x 32 and 17 x 17 x 64 (3x3, stride 1, pad 1, C in = C out,
// channels-last), in the two 16-bit precisions of cnn_bf16.hip (NS = 3: split bf16, a_hi*b_hi + a_hi*b_lo + a_lo*b_hi; NS = 1: a_hi*b_hi).
//
// Why not the implicit GEMM of cnn_bf16.hip: it gathers float32 activations from global memory once per tap and splits them into bf16
// on the vector units each time, nine times per pixel.  Here a workgroup's input window reaches LDS ONCE, already split, and the nine
// taps are nine shifted views of it, as in the float32 k_conv3x3_direct (cnn.hip):
//   positions are numbered on a grid with one shared zero column per row and one shared zero row per image,
//   q = (img*(H+1) + r)*(W+1) + c, so the input of output q for tap (ky, kx) is position q + (ky-1)*(W+1) + (kx-1) for EVERY q: a pure
//   row shift of the window.  The grid exists only inside the kernel: the fill decodes q and reads the ordinary NHWC activation (zero
//   for the shared column / row and outside the batch), the epilogue writes valid q only.
//
// LDS (dynamic), operands as bf16, k-contiguous, NP planes (hi, lo; NS = 1: hi only):
//   A window  [NP][BM + 2(W+2)][C + 8]   BM = NWM * WM * 32 output positions of the workgroup plus the halo of W + 2 rows on either side
//   weights   [BT][NP][C][C + 8]         one tap = C output channels x C input channels; BT = 9 (C = 32: every tap resident) or a ring
//                                        of 2 taps (C = 64: tap t + 1 is fetched into registers before the MFMAs of tap t and written to
//                                        the other slot after them, one barrier per tap)
//   The row stride is C + 8 bf16 = 80 B (C = 32) or 144 B (C = 64), an odd number of 16-byte units: a lane's ds_read_b128 of eight
//   channels of row lane & 31 meets no bank twice (as the stride of 40 in cnn_bf16.hip).
//   Budget (NS = 3 / NS = 1), two workgroups per CU inside 160 KB:
//     C = 32, BM = 128, 256 threads: A 2 x 202 x 80 = 32 320 B + weights 2 x 9 x 32 x 80 = 46 080 B = 78 400 B / 39 200 B
//     C = 64, BM =  96, 384 threads: A 2 x 134 x 144 = 38 592 B + ring 2 x 2 x 64 x 144 = 36 864 B = 75 456 B / 37 728 B
//   Measured at batch 256 against one workgroup per CU (BM = 256 at C = 32: 98 880 B; BM = 128 at C = 64: 84 672 B), split bf16:
//   80 against 109 us and 45 against 52 us per layer; those tiles are not built.
// Weights: cnn_bf16_pack of the K-major weights, k = tap * C + ic: [plane][tap][C/8][C][8] bf16, so a thread's 16-byte global load is its
// 16-byte LDS store and consecutive threads take consecutive output channels.  The float32 -> (hi, lo) split of an activation
// (bf16_split / bf16_rne of cnn_conv.h) happens once per element, on the way into the window.
//
// Order of a sum (fixed, the same for every pixel, tile shape and batch position): taps in (ky, kx) order; inside a tap channels ascending
// in steps of 16; inside a step hi*hi, then hi*lo (activation hi, weight lo), then lo*hi, all into the one float32 accumulator.
// Epilogue as k_conv3x3_direct: bias, the residual res[pixel][resC] for output channels below resC, optional ReLU.
//
// What stays float32 in the dlib forward under a 16-bit precision: the first layer (k_conv7x7s2_pool: three channels, K = 147, fused with
// the max pool), k_dlib_tail (the last block's second convolution on a 1 x 1 map, skip, average, fc), the pools and k_add_relu_pad.  Every
// other 3x3 layer goes through k_conv_igemm_bf16.  Activations stay float32 in memory between layers.
#include <atomic>
#include "common.h"
#include "cnn_conv.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int C, int H, int W, int WM, int NWM, int NWN, int NS>
__global__ __launch_bounds__(NWM * NWN * 64) void k_conv3x3_direct_bf16(const float* __restrict__ in, const uint16_t* __restrict__ Wp,
                                                                const float* __restrict__ bias, float* __restrict__ out, int N,
                                                                const float* __restrict__ res, int resC, int relu) {
    static_assert(NS == 1 || NS == 3, "plain or split");
    constexpr int P = W + 1, IMGQ = (H + 1) * P, HALO = P + 1;
    constexpr int NW = NWM * NWN, BM = NWM * WM * 32, NPOS = BM + 2 * HALO, LDC = C + 8, WN = C / 32 / NWN, NT = NW * 64;
    constexpr int NP = NS == 3 ? 2 : 1, C8 = C / 8;
    constexpr bool RING = C > 32;             // weights: a ring of two taps, else all nine resident
    constexpr int TAPW = NP * C * LDC;        // bf16 of one tap's weights in LDS
    static_assert(WN * NWN * 32 == C, "output channels split evenly over the waves");
    extern __shared__ __attribute__((aligned(16))) uint16_t smem_h[];
    uint16_t* As = smem_h;                    // [NP][NPOS][LDC]
    uint16_t* Bs = smem_h + NP * NPOS * LDC;  // [RING ? 2 : 9][NP][C][LDC]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int wm = wave / NWN, wn = wave % NWN;  // wave tile: WM*32 positions x WN*32 output channels
    const int64_t Qtot = (int64_t)N * IMGQ;
    const int64_t q0 = (int64_t)blockIdx.x * BM;
    // ---- weights of one tap: NP * C/8 * C 16-byte pieces, piece (pl, kq, oc) at Wp[((pl*9 + tap)*C8 + kq)*C + oc][8] ----
    constexpr int WQ = NP * C8 * C;
    constexpr int WIT = (WQ + NT - 1) / NT;
    u32x4 wr[RING ? 1 : 9][WIT];  // RING: the tap in flight; else all nine taps, in flight together with the window's loads
    auto wfetch = [&](int tap, int t) {
#pragma unroll
        for (int i = 0; i < WIT; ++i) {
            const int idx = tid + NT * i;
            const int idc = (WQ % NT == 0 || idx < WQ) ? idx : WQ - 1;  // a valid address; not stored
            const int pl = idc / (C8 * C), rem = idc - pl * (C8 * C);
            wr[t][i] = *reinterpret_cast<const u32x4*>(Wp + ((int64_t)(pl * 9 + tap) * (C8 * C) + rem) * 8);
        }
    };
    auto wstash = [&](int slot, int t) {
#pragma unroll
        for (int i = 0; i < WIT; ++i) {
            const int idx = tid + NT * i;
            if (WQ % NT == 0 || idx < WQ) {
                const int pl = idx / (C8 * C), rem = idx - pl * (C8 * C);
                const int kq = rem / C, oc = rem - kq * C;
                *reinterpret_cast<u32x4*>(Bs + slot * TAPW + (pl * C + oc) * LDC + kq * 8) = wr[t][i];
            }
        }
    };
#pragma unroll
    for (int t = 0; t < (RING ? 1 : 9); ++t) wfetch(t, t);
    // ---- A window: positions q0 - HALO ... q0 + BM + HALO, eight channels per piece; every load of the thread in flight before the
    // first conversion; each float32 is split exactly once ----
    constexpr int APC = NPOS * C8;
    constexpr int AIT = (APC + NT - 1) / NT;
    {
        float4 v[AIT][2];
        bool ok[AIT];
#pragma unroll
        for (int i = 0; i < AIT; ++i) {
            const int idx = tid + NT * i;
            const int j = idx / C8, f = idx - j * C8;
            const int64_t q = q0 - HALO + j;
            // unconditional loads from a clamped address (a branch per load would wait for each before the next, cnn.hip); what is
            // the zero column / row, outside the batch or past the window is zeroed below
            const int64_t qc = q < 0 ? 0 : (q < Qtot ? q : Qtot - 1);
            const int img = (int)(qc / IMGQ), rem = (int)(qc - (int64_t)img * IMGQ);
            const int r = rem / P, c = rem - r * P;
            ok[i] = idx < APC && q == qc && r < H && c < W;
            const float* p = in + (((int64_t)img * H + (r < H ? r : H - 1)) * W + (c < W ? c : W - 1)) * C + f * 8;
            v[i][0] = *reinterpret_cast<const float4*>(p);
            v[i][1] = *reinterpret_cast<const float4*>(p + 4);
        }
#pragma unroll
        for (int i = 0; i < AIT; ++i) {
            const int idx = tid + NT * i;
            if (idx < APC) {
                const int j = idx / C8, f = idx - j * C8;
                const float raw[8] = {v[i][0].x, v[i][0].y, v[i][0].z, v[i][0].w, v[i][1].x, v[i][1].y, v[i][1].z, v[i][1].w};
                uint32_t hi[8], lo[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float e = ok[i] ? raw[k] : 0.f;
                    if constexpr (NS == 3) bf16_split(e, hi[k], lo[k]);
                    else hi[k] = bf16_rne(e);
                }
                *reinterpret_cast<uint4*>(As + j * LDC + f * 8) =
                    make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
                if constexpr (NS == 3)
                    *reinterpret_cast<uint4*>(As + (NPOS + j) * LDC + f * 8) =
                        make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
            }
        }
    }
#pragma unroll
    for (int t = 0; t < (RING ? 1 : 9); ++t) wstash(t, t);
    __syncthreads();
    f32x16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const uint16_t* Abase = As + (HALO + wm * WM * 32 + l31) * LDC + 8 * h;
    const uint16_t* Bbase = Bs + (wn * WN * 32 + l31) * LDC + 8 * h;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        if constexpr (RING) {
            if (tap + 1 < 9) wfetch(tap + 1, 0);
            __builtin_amdgcn_sched_barrier(0);  // the loads are issued before the tap's MFMAs, not next to the LDS write that consumes them
        }
        const int ky = tap / 3, kx = tap - 3 * ky;
        const uint16_t* At = Abase + ((ky - 1) * P + (kx - 1)) * LDC;
        const uint16_t* Bt = Bbase + (RING ? (tap & 1) : tap) * TAPW;
#pragma unroll
        for (int ks = 0; ks < C; ks += 16) {
            bf16x8 a[NP][WM], b[NP][WN];
#pragma unroll
            for (int pl = 0; pl < NP; ++pl) {
#pragma unroll
                for (int i = 0; i < WM; ++i) a[pl][i] = *reinterpret_cast<const bf16x8*>(At + (pl * NPOS + i * 32) * LDC + ks);
#pragma unroll
                for (int j = 0; j < WN; ++j) b[pl][j] = *reinterpret_cast<const bf16x8*>(Bt + (pl * C + j * 32) * LDC + ks);
            }
#pragma unroll
            for (int pr = 0; pr < NS; ++pr) {  // hi*hi, hi*lo, lo*hi
                const int pa = pr == 2 ? NP - 1 : 0, pb = pr == 1 ? NP - 1 : 0;
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[pa][i], b[pb][j], acc[i][j], 0, 0, 0);
            }
        }
        if constexpr (RING) {
            if (tap + 1 < 9) {
                __builtin_amdgcn_sched_barrier(0);
                wstash((tap + 1) & 1, 0);  // the other slot: its readers (tap - 1) finished before the previous barrier
                __syncthreads();
            }
        }
    }
    // ---- epilogue: col = lane&31 (oc), row = (r&3) + 8*(r>>2) + 4*h (position); residual loads issued together ----
    float bv[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) bv[j] = bias[(wn * WN + j) * 32 + l31];
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        int64_t pp[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t q = q0 + (wm * WM + i) * 32 + row;
            pp[r] = -1;
            if (q < Qtot) {
                const int img = (int)(q / IMGQ), rem = (int)(q - (int64_t)img * IMGQ);
                const int y = rem / P, x = rem - y * P;
                if (y < H && x < W) pp[r] = ((int64_t)img * H + y) * W + x;
            }
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int oc = (wn * WN + j) * 32 + l31;
            float rv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) rv[r] = (res && oc < resC && pp[r] >= 0) ? res[pp[r] * resC + oc] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[i][j][r] + bv[j];
                if (res && oc < resC) v += rv[r];
                if (relu) v = v > 0.f ? v : 0.f;
                if (pp[r] >= 0) out[pp[r] * C + oc] = v;
            }
        }
    }
}

// ================================================================================================
// host
// ================================================================================================
template <int C, int H, int W, int WM, int NWM, int NWN, int NS>
static int launch_direct_cfg(const float* in, const uint16_t* wp, const float* b, float* out, int N, const float* res, int resC, int relu,
                             hipStream_t st) {
    constexpr int P = W + 1, BM = NWM * WM * 32, NPOS = BM + 2 * (P + 1), NP = NS == 3 ? 2 : 1, BT = C > 32 ? 2 : 9;
    constexpr size_t lds = ((size_t)NP * NPOS * (C + 8) + (size_t)BT * NP * C * (C + 8)) * sizeof(uint16_t);
    static_assert(lds <= 160 * 1024, "a CU has 160 KB of LDS");
    // the dynamic-LDS attribute is a per-device property of the function: one bit per device, set by whichever thread launches there
    // first (setting it twice is harmless, so the race of two first launches needs no lock)
    static std::atomic<uint64_t> attr_set{0};
    auto kern = k_conv3x3_direct_bf16<C, H, W, WM, NWM, NWN, NS>;
    int dev = 0;
    CIS_CHECK_HIP(hipGetDevice(&dev));
    const uint64_t bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        CIS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set.fetch_or(bit, std::memory_order_release);
    }
    const int64_t Qtot = (int64_t)N * (H + 1) * P;
    hipLaunchKernelGGL(kern, dim3((unsigned)ceil_div(Qtot, BM)), dim3(NWM * NWN * 64), lds, st, in, wp, b, out, N, res, resC, relu);
    return CIS_OK;
}

bool conv3x3_direct_bf16_serves(int C, int H, int W) { return (C == 32 && H == 35 && W == 35) || (C == 64 && H == 17 && W == 17); }

int launch_conv3x3_direct_bf16(int C, int H, int W, const float* in, const uint16_t* wp, const float* bias, float* out, int N, const float* res,
                               int resC, int relu, int ns, hipStream_t st) {
    CIS_REQUIRE(ns == 1 || ns == 3, "16-bit direct convolution: ns must be 1 or 3");
    CIS_REQUIRE(conv3x3_direct_bf16_serves(C, H, W), "16-bit direct convolution: built for 35 x 35 x 32 and 17 x 17 x 64 (got %d x %d x %d)", H, W, C);
    CIS_REQUIRE(in && wp && bias && out && N >= 1 && (res == nullptr || resC >= 1), "16-bit direct convolution: NULL buffer or bad count");
#define CIS_DIRECT16(C_, H_, W_, WM_, NWM_, NWN_)                                                                      \
    return ns == 3 ? launch_direct_cfg<C_, H_, W_, WM_, NWM_, NWN_, 3>(in, wp, bias, out, N, res, resC, relu, st)      \
                   : launch_direct_cfg<C_, H_, W_, WM_, NWM_, NWN_, 1>(in, wp, bias, out, N, res, resC, relu, st)
    if (C == 32) CIS_DIRECT16(32, 35, 35, 1, 4, 1);
    CIS_DIRECT16(64, 17, 17, 1, 3, 2);
#undef CIS_DIRECT16
}
