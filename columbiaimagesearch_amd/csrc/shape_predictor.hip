// Face landmarks on the MI355X: dlib's shape_predictor::operator()(img, rect), the call `self.pred(img, rect)` of the reference's
// DLibFeaturizer.featurize (cufacesearch/cufacesearch/featurizer/dlib_featurizer.py:103).  An ensemble of regression trees (Kazemi and
// Sullivan, "One millisecond face alignment with an ensemble of regression trees", CVPR 2014) restated from dlib's published
// image_processing/shape_predictor.h as remembered: dlib and its model files are not available here, so parity with dlib itself is
// UNPINNED; the yardstick is the numpy model tests/shape_model.py, which this file meets bit for bit (tests/test_shape_predictor.py).
//
// k_shape_predict: ONE launch, one workgroup of 256 threads per rectangle, the K cascade levels in a loop inside it.  Per level:
//   1. the least-squares similarity (2 x 2 part) from the initial shape onto the current one, dlib's find_tform_between_shapes, in the
//      closed form of the 2-D problem in double: with f', t' the centred points, a = sum f'.t' / sum |f'|^2, b = sum f' x t' / sum |f'|^2,
//      m = [[a, -b], [b, a]].  Umeyama's reflection branch (det(cov) < 0: the sign matrix diag(1, -1)) keeps m a ROTATION -- it only
//      replaces the scale (d0 + d1) / sigma by (d0 - d1) / sigma -- and in two dimensions a^2 + b^2 is ((d0 + d1) / sigma)^2 for
//      det >= 0 and ((d0 - d1) / sigma)^2 for det < 0, so the same a and b serve both branches (the tests compare with the SVD form
//      of featurizer/face_chip.py on reflected pairs).  sum |f'|^2 = 0 gives the identity (scale 1), P = 1 the identity as in dlib.
//      Summation order, restated by tests/shape_model.py: lane l of a wave adds the points l, l + 64, ... in turn to a zero, then
//      the 64 partial sums meet in a butterfly over lane distances 32, 16, 8, 4, 2, 1 (v = v + v[lane ^ s]: every lane ends with
//      the same bits).  Every wave computes it for itself: no broadcast, no barrier.
//   2. the F feature pixels: q = m * delta + location(cur, anchor) in float32 (two products and an add per row, then the add), the
//      image position left + q.x (right - left), top + q.y (bottom - top) in double -- unnormalizing_tform(rect) stated directly, where
//      dlib goes through find_affine_transform of three corners (a deviation, noted in DESIGN.md) -- rounded by floor(. + 0.5), the
//      grey value (R + G + B) / 3 in unsigned integer division, 0 outside the image; kept in LDS as float.
//   3. the T tree walks, one thread per tree: a split is 8 bytes (two 16-bit feature indices, the float threshold), `depth` dependent
//      loads per walk; the leaf numbers go to LDS.
//   4. cur += leaf, ONE TREE AFTER ANOTHER in tree order in float32 (dlib's order; float addition is not associative): one lane per
//      coordinate, the 2P lanes of a wave instruction read 2P consecutive floats of one leaf; the loads of 16 trees are issued before
//      their 16 adds, so the chain of adds does not wait for one load at a time.
// The library is built with -ffp-contract=off: every product and sum above rounds on its own.
#include "common.h"
#include "cis_hip.h"

#define SP_THREADS 256
#define SP_MAX_COORDS 256
#define SP_MAX_F 4096
#define SP_MAX_T 4096
#define SP_MAX_DEPTH 8
#define SP_UNROLL 16

struct SpNode {
    uint32_t idx;  // idx1 | idx2 << 16
    float thresh;
};

struct cis_shapepred {
    int device = 0;
    int P = 0, K = 0, T = 0, depth = 0, S = 0, F = 0;
    float* init = nullptr;     // [2P]
    SpNode* nodes = nullptr;   // [K][T][S]
    float* leaves = nullptr;   // [K][T][S+1][2P]
    int32_t* anchor = nullptr; // [K][F]
    float2* deltas = nullptr;  // [K][F]
};

struct SpDims {
    int P, K, T, depth, S, F;
};

__device__ __forceinline__ double sp_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
    return v;
}

// the 2 x 2 part of the similarity initial shape -> current shape, as float32 (m00, m01, m10, m11); every lane of the wave takes part
__device__ __forceinline__ void sp_similarity(const float* __restrict__ init, const float* cur, int P, int lane, float m[4]) {
    m[0] = 1.f; m[1] = 0.f; m[2] = 0.f; m[3] = 1.f;
    if (P == 1) return;
    double sfx = 0.0, sfy = 0.0, stx = 0.0, sty = 0.0;
    for (int p = lane; p < P; p += 64) {
        sfx = sfx + (double)init[2 * p];
        sfy = sfy + (double)init[2 * p + 1];
        stx = stx + (double)cur[2 * p];
        sty = sty + (double)cur[2 * p + 1];
    }
    const double n = (double)P;
    const double mfx = sp_wave_sum(sfx) / n, mfy = sp_wave_sum(sfy) / n, mtx = sp_wave_sum(stx) / n, mty = sp_wave_sum(sty) / n;
    double ff = 0.0, sd = 0.0, sc = 0.0;
    for (int p = lane; p < P; p += 64) {
        const double fx = (double)init[2 * p] - mfx, fy = (double)init[2 * p + 1] - mfy;
        const double tx = (double)cur[2 * p] - mtx, ty = (double)cur[2 * p + 1] - mty;
        ff = ff + (fx * fx + fy * fy);
        sd = sd + (fx * tx + fy * ty);
        sc = sc + (fx * ty - fy * tx);
    }
    ff = sp_wave_sum(ff);
    sd = sp_wave_sum(sd);
    sc = sp_wave_sum(sc);
    if (ff == 0.0) return;  // dlib: sigma_from == 0 -> scale 1; the SVD of a zero covariance gives the identity
    const double a = sd / ff, b = sc / ff;
    m[0] = (float)a; m[1] = (float)(-b); m[2] = (float)b; m[3] = (float)a;
}

__device__ __forceinline__ double sp_round(double v) { return floor(v + 0.5); }

__global__ __launch_bounds__(SP_THREADS) void k_shape_predict(SpDims d, const float* __restrict__ init, const SpNode* __restrict__ nodes,
                                                              const float* __restrict__ leaves, const int32_t* __restrict__ anchor,
                                                              const float2* __restrict__ deltas, const uint8_t* __restrict__ img, int nr, int nc,
                                                              const int32_t* __restrict__ rects, int32_t* __restrict__ parts,
                                                              float* __restrict__ shape) {
    __shared__ float s_cur[SP_MAX_COORDS];
    __shared__ float s_pix[SP_MAX_F];
    __shared__ uint16_t s_leaf[SP_MAX_T];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t face = blockIdx.x;
    const int C = 2 * d.P;
    const int32_t* rc = rects + face * 4;
    const double left = (double)rc[0], top = (double)rc[1];
    const double w = (double)rc[2] - left, h = (double)rc[3] - top;
    if (tid < C) s_cur[tid] = init[tid];
    __syncthreads();
    for (int k = 0; k < d.K; ++k) {
        float m[4];
        sp_similarity(init, s_cur, d.P, lane, m);
        for (int i = tid; i < d.F; i += SP_THREADS) {
            const float2 dl = deltas[(int64_t)k * d.F + i];
            const int an = anchor[(int64_t)k * d.F + i];
            const float qx = (m[0] * dl.x + m[1] * dl.y) + s_cur[2 * an];
            const float qy = (m[2] * dl.x + m[3] * dl.y) + s_cur[2 * an + 1];
            const double px = sp_round(left + (double)qx * w), py = sp_round(top + (double)qy * h);
            float v = 0.f;
            if (px >= 0.0 && px < (double)nc && py >= 0.0 && py < (double)nr) {  // (a NaN position compares false: outside)
                const uint8_t* p = img + ((int64_t)py * nc + (int64_t)px) * 3;
                v = (float)(((unsigned)p[0] + (unsigned)p[1] + (unsigned)p[2]) / 3u);
            }
            s_pix[i] = v;
        }
        __syncthreads();
        for (int t = tid; t < d.T; t += SP_THREADS) {
            const SpNode* nd = nodes + ((int64_t)k * d.T + t) * d.S;
            int i = 0;
            for (int lv = 0; lv < d.depth; ++lv) {  // a complete tree: i < S for exactly `depth` steps
                const SpNode s = nd[i];
                i = (s_pix[s.idx & 0xffffu] - s_pix[s.idx >> 16] > s.thresh) ? 2 * i + 1 : 2 * i + 2;
            }
            s_leaf[t] = (uint16_t)(i - d.S);
        }
        __syncthreads();
        if (tid < C) {
            float c = s_cur[tid];
            const int64_t tree = (int64_t)(d.S + 1) * C;
            const float* base = leaves + (int64_t)k * d.T * tree + tid;
            int t = 0;
            for (; t + SP_UNROLL <= d.T; t += SP_UNROLL) {
                float v[SP_UNROLL];
#pragma unroll
                for (int j = 0; j < SP_UNROLL; ++j) v[j] = base[(int64_t)(t + j) * tree + (int64_t)s_leaf[t + j] * C];
#pragma unroll
                for (int j = 0; j < SP_UNROLL; ++j) c = c + v[j];
            }
            for (; t < d.T; ++t) c = c + base[(int64_t)t * tree + (int64_t)s_leaf[t] * C];
            s_cur[tid] = c;
        }
        __syncthreads();
    }
    if (tid < d.P) {
        // dlib rounds into a point of longs; the two ends of int32 stand in for positions beyond them
        const double x = fmin(fmax(sp_round(left + (double)s_cur[2 * tid] * w), -2147483648.0), 2147483647.0);
        const double y = fmin(fmax(sp_round(top + (double)s_cur[2 * tid + 1] * h), -2147483648.0), 2147483647.0);
        parts[(face * d.P + tid) * 2] = (int32_t)x;
        parts[(face * d.P + tid) * 2 + 1] = (int32_t)y;
    }
    if (shape != nullptr && tid < C) shape[face * C + tid] = s_cur[tid];
}

extern "C" void cis_shapepred_destroy(cis_shapepred* sp) {
    if (!sp) return;
    (void)hipSetDevice(sp->device);
    (void)hipDeviceSynchronize();
    if (sp->init) (void)hipFree(sp->init);
    if (sp->nodes) (void)hipFree(sp->nodes);
    if (sp->leaves) (void)hipFree(sp->leaves);
    if (sp->anchor) (void)hipFree(sp->anchor);
    if (sp->deltas) (void)hipFree(sp->deltas);
    delete sp;
}

static int sp_upload(void** dst, const void* src, size_t bytes) {
    CIS_CHECK_HIP(hipMalloc(dst, bytes));
    CIS_CHECK_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return CIS_OK;
}

extern "C" int cis_shapepred_create(cis_shapepred** out, int P, int K, int T, int depth, int F, const float* initial_shape,
                                    const int32_t* split_idx, const float* split_thresh, const float* leaves, const int32_t* anchor_idx,
                                    const float* deltas) {
    CIS_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    CIS_REQUIRE(P >= 1 && 2 * P <= SP_MAX_COORDS, "shape predictor: 2P = %d coordinates, the kernel takes 2 to %d", 2 * P, SP_MAX_COORDS);
    CIS_REQUIRE(K >= 1, "shape predictor: K = %d cascade levels", K);
    CIS_REQUIRE(T >= 1 && T <= SP_MAX_T, "shape predictor: T = %d trees per level, the kernel takes 1 to %d", T, SP_MAX_T);
    CIS_REQUIRE(depth >= 1 && depth <= SP_MAX_DEPTH, "shape predictor: depth = %d, the kernel takes 1 to %d", depth, SP_MAX_DEPTH);
    CIS_REQUIRE(F >= 1 && F <= SP_MAX_F, "shape predictor: F = %d feature pixels per level, the kernel takes 1 to %d", F, SP_MAX_F);
    CIS_REQUIRE(initial_shape && split_idx && split_thresh && leaves && anchor_idx && deltas, "shape predictor: NULL array");
    const int S = (1 << depth) - 1;
    const size_t n_feat = (size_t)K * F, n_nodes = (size_t)K * T * S;
    for (size_t i = 0; i < n_feat; ++i)
        CIS_REQUIRE(anchor_idx[i] >= 0 && anchor_idx[i] < P, "shape predictor: anchor_idx[%zu][%zu] = %d is not a landmark (P = %d)", i / F, i % F,
                    (int)anchor_idx[i], P);
    for (size_t i = 0; i < 2 * n_nodes; ++i)
        CIS_REQUIRE(split_idx[i] >= 0 && split_idx[i] < F, "shape predictor: split_idx[%zu][%zu][%zu][%zu] = %d is not a feature (F = %d)",
                    i / 2 / S / T, i / 2 / S % T, i / 2 % S, i % 2, (int)split_idx[i], F);
    CIS_TRY(cis_lazy_init());
    std::vector<SpNode> nodes(n_nodes);
    for (size_t i = 0; i < n_nodes; ++i) {
        nodes[i].idx = (uint32_t)split_idx[2 * i] | ((uint32_t)split_idx[2 * i + 1] << 16);
        nodes[i].thresh = split_thresh[i];
    }
    cis_shapepred* sp = new cis_shapepred();
    sp->device = cis_current_device();
    sp->P = P; sp->K = K; sp->T = T; sp->depth = depth; sp->S = S; sp->F = F;
    int rc = hipSetDevice(sp->device) == hipSuccess ? CIS_OK : CIS_EHIP;
    if (rc != CIS_OK) cis_set_error("shape predictor: hipSetDevice(%d) failed", sp->device);
    if (rc == CIS_OK) rc = sp_upload((void**)&sp->init, initial_shape, (size_t)2 * P * sizeof(float));
    if (rc == CIS_OK) rc = sp_upload((void**)&sp->nodes, nodes.data(), n_nodes * sizeof(SpNode));
    if (rc == CIS_OK) rc = sp_upload((void**)&sp->leaves, leaves, (size_t)K * T * (S + 1) * 2 * P * sizeof(float));
    if (rc == CIS_OK) rc = sp_upload((void**)&sp->anchor, anchor_idx, n_feat * sizeof(int32_t));
    if (rc == CIS_OK) rc = sp_upload((void**)&sp->deltas, deltas, n_feat * sizeof(float2));
    if (rc != CIS_OK) {
        cis_shapepred_destroy(sp);
        return rc;
    }
    *out = sp;
    return CIS_OK;
}

extern "C" int cis_shapepred_run_dev(cis_shapepred* sp, const uint8_t* d_img, int nr, int nc, const int32_t* d_rects, int n, int32_t* d_parts,
                                     float* d_shape, void* stream) {
    CIS_REQUIRE(sp != nullptr, "shape predictor is NULL");
    CIS_REQUIRE(n >= 0 && nr >= 0 && nc >= 0, "shape predictor: bad arguments (n = %d, image %d x %d)", n, nr, nc);
    if (n == 0) return CIS_OK;
    CIS_REQUIRE(d_rects && d_parts && (d_img || nr == 0 || nc == 0), "shape predictor: NULL buffer");
    CIS_TRY(cis_lazy_init());
    const SpDims d = {sp->P, sp->K, sp->T, sp->depth, sp->S, sp->F};
    hipLaunchKernelGGL(k_shape_predict, dim3((unsigned)n), dim3(SP_THREADS), 0, (hipStream_t)stream, d, (const float*)sp->init,
                       (const SpNode*)sp->nodes, (const float*)sp->leaves, (const int32_t*)sp->anchor, (const float2*)sp->deltas, d_img, nr, nc,
                       d_rects, d_parts, d_shape);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

// ---- host only: runs of floats in dlib's stream serialisation (serialize.h, float_details.h) -------------------------------------------
// an integer: one control byte (low nibble = number of value bytes 1..8, bit 7 = negative, bits 4..6 clear), then the magnitude,
// little-endian; a float: the integer mantissa, then the integer exponent (32000 / 32001 / 32002 = +inf / -inf / nan)
static bool sp_read_int(const uint8_t* buf, size_t len, size_t* pos, int64_t* v) {
    if (*pos >= len) return false;
    const uint8_t c = buf[*pos];
    const unsigned nb = c & 0x0Fu;
    if (nb == 0 || nb > 8 || (c & 0x70u) || len - *pos - 1 < nb) return false;
    uint64_t mag = 0;
    for (unsigned i = 0; i < nb; ++i) mag |= (uint64_t)buf[*pos + 1 + i] << (8 * i);
    *v = (c & 0x80u) ? -(int64_t)mag : (int64_t)mag;
    *pos += 1 + nb;
    return true;
}

extern "C" int cis_dlib_decode_reals(const uint8_t* buf, size_t len, size_t* pos, float* out, size_t n) {
    CIS_REQUIRE(buf && pos && (out || n == 0), "cis_dlib_decode_reals: NULL argument");
    for (size_t i = 0; i < n; ++i) {
        int64_t mant = 0, e = 0;
        if (!sp_read_int(buf, len, pos, &mant) || !sp_read_int(buf, len, pos, &e)) {
            cis_set_error("dlib stream, byte %zu: float %zu of %zu: %s", *pos, i, n,
                          *pos >= len ? "the stream ends here" : "bad integer control byte, or the stream ends inside the integer");
            return CIS_EINVAL;
        }
        if (e == 32000) out[i] = __builtin_inff();
        else if (e == 32001) out[i] = -__builtin_inff();
        else if (e == 32002) out[i] = __builtin_nanf("");
        else out[i] = (float)ldexp((double)mant, (int)(e < -100000 ? -100000 : (e > 100000 ? 100000 : e)));
    }
    return CIS_OK;
}
