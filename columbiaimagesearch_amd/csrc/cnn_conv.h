// What cnn.hip (the float32 convolutions, the network forwards, the C ABI) and cnn_bf16.hip (the 16-bit matrix-core convolutions)
// share: the description of one convolution launch and the entry points of the 16-bit path.
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

// ---- cnn_bf16.hip ----
// float32 weights in the K-major form of the float32 kernels, [groups][K][OCg] on the HOST, split into bf16 planes and uploaded:
// *d_out = [planes][groups][Kp / 8][OCg][8] uint16 (Kp = K rounded up to 32, the tail zero), planes = 2 (hi, lo) when lo != 0, else 1.
int cnn_bf16_pack(uint16_t** d_out, const float* w_kmajor, int groups, int K, int OCg, int with_lo);
// One convolution on the 16-bit matrix cores.  d as for launch_conv with these differences: d.K is the K of the packed weights (not
// rounded), d.runq / d.run_planes select the NCHW plane gather exactly as there, every other layer is channels-last with ICg % 8 == 0.
// ns = 3: split-bf16 (three products per k step), ns = 1: plain bf16.  Returns CIS_EINVAL for a shape the kernel does not serve.
int launch_conv_bf16(const ConvDesc& d, const float* in, const uint16_t* wp, const float* bias, float* out, int ns, hipStream_t st);
