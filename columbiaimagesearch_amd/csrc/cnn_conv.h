// What cnn.hip (the float32 convolutions, the network forwards, the C ABI), cnn_bf16.hip (the 16-bit implicit GEMM) and
// cnn_bf16_direct.hip (the 16-bit direct 3x3 kernel of the dlib net) share: the description of one convolution launch, the
// float32 -> bf16 split and the entry points of the 16-bit paths.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

struct ConvDesc {
    int N, H, W, C;          // input: images, height, width, total channels
    int OH, OW, OC;          // output
    int KH, KW, stride, pad, groups;
    int ICg, OCg, K;         // per group; K = KH*KW*ICg, k = (ky*KW + kx)*ICg + ic
    int64_t sN, sC, sH, sW;  // input strides in elements (NCHW for the first layer, NHWC afterwards)
    int relu;
    int kx_fastest;          // K ordering of the packed weights: 0: k = (ky*KW+kx)*ICg+ic, 1: k = (ic*KH+ky)*KW+kx (NCHW input)
    int splitk = 1;          // > 1 (groups == 1, vector path only): blockIdx.z owns a K range and writes raw partial sums
    int64_t part_stride = 0; // elements between the partial outputs of consecutive K ranges
    int runq = 0;            // > 0: "row-run" gather of the 3-channel first layer (vector path): K is cut per kernel row into runq
                             // float4 of contiguous NHWC input (KW*C floats, zero-weight padded), k = ky*4*runq + (kx*C + ic)
    const float* res = nullptr;  // residual input [npix][resC] added before the ReLU (channels >= resC get nothing): dlib add_prev
    int resC = 0;
    int run_planes = 0;      // > 0 (with runq): the runs are taken from the caller's NCHW planes directly -- run r = ic * KH + ky is the KW
                             // contiguous floats of channel plane ic, row iy0 + ky, from column ix0 (runq float4, the tail meets zero
                             // weights), k = r * 4 * runq + kx; run_planes = ICg * KH runs; in_elems = floats in the input (the last
                             // float4 of the last run would end past it: it is loaded one to three floats earlier and shifted)
    int64_t in_elems = 0;
};

// ---- the float32 -> bf16 (hi, lo) split of both 16-bit files ----
// round-to-nearest-even on the float32 bits; Inf stays Inf, NaN stays a (quiet) NaN
static __host__ __device__ __forceinline__ uint32_t bf16_rne(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// x = hi + lo + residue, |residue| <= 2^-16 |x|.  hi not finite: lo = 0 (Inf - Inf would turn an Inf into a NaN)
static __host__ __device__ __forceinline__ void bf16_split(float x, uint32_t& hi, uint32_t& lo) {
    hi = bf16_rne(x);
    const uint32_t hb = hi << 16;
    float hf;
    __builtin_memcpy(&hf, &hb, 4);
    lo = (hi & 0x7f80u) == 0x7f80u ? 0u : bf16_rne(x - hf);
}

// ---- cnn_bf16.hip ----
// float32 weights in the K-major form of the float32 kernels, [groups][K][OCg] on the HOST, split into bf16 planes and uploaded:
// *d_out = [planes][groups][Kp / 8][OCg][8] uint16 (Kp = K rounded up to 32, the tail zero), planes = 2 (hi, lo) when lo != 0, else 1.
int cnn_bf16_pack(uint16_t** d_out, const float* w_kmajor, int groups, int K, int OCg, int with_lo);
// One convolution on the 16-bit matrix cores.  d as for launch_conv with these differences: d.K is the K of the packed weights (not
// rounded), d.runq / d.run_planes select the NCHW plane gather exactly as there, every other layer is channels-last with ICg % 8 == 0.
// ns = 3: split-bf16 (three products per k step), ns = 1: plain bf16.  Returns CIS_EINVAL for a shape the kernel does not serve.
int launch_conv_bf16(const ConvDesc& d, const float* in, const uint16_t* wp, const float* bias, float* out, int ns, hipStream_t st);

// ---- cnn_bf16_direct.hip ----
// true: (C, H, W) is a shape k_conv3x3_direct_bf16 is built for (32 x 35 x 35 and 64 x 17 x 17, the dlib net's stride-1 layers)
bool conv3x3_direct_bf16_serves(int C, int H, int W);
// 3x3 / stride 1 / pad 1, C input = C output channels, channels-last [N][H][W][C].  wp: cnn_bf16_pack of the K-major weights with
// k = (ky*3 + kx)*C + ic, which for K = 9 C (a multiple of 32) IS [plane][tap][C/8][C][8].  Epilogue: bias, then res[pixel][resC] for output
// channels below resC (res may be NULL), then the optional ReLU.
int launch_conv3x3_direct_bf16(int C, int H, int W, const float* in, const uint16_t* wp, const float* bias, float* out, int N, const float* res,
                               int resC, int relu, int ns, hipStream_t st);
