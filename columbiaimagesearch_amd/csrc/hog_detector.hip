// Face detection on the MI355X: dlib's get_frontal_face_detector() scheme, object_detector<scan_fhog_pyramid<pyramid_down<N>>>, the call
// `self.detector.run(img, up_sample, 0)` of the reference's DLibFaceDetector (cufacesearch/cufacesearch/detector/dlib_detector.py:33).
// Restated from dlib's published image_transforms/fhog.h, image_processing/scan_fhog_pyramid.h and box_overlap_testing.h AS REMEMBERED:
// dlib and its detector file are not available here, so parity with dlib itself is UNPINNED; the yardstick is the numpy model
// tests/fhog_model.py, which this file meets bit for bit (tests/test_hog_detector.py).  Known deviations from dlib: the saliency is the
// direct correlation in one stated order (dlib filters separably after an SVD of each plane and so rounds differently), and one
// bilinear resize stands in for pyramid_up and pyramid_down<N>.  No real detector file has ever met the reader.
//
// One call = (up-sampling rounds) + (L - 1 pyramid resizes) + 4 launches, every level in each of them through a level table that is a
// kernel argument (all sizes follow from nr, nc on the host: no read-back):
//   k_resize_bilinear   one thread per output pixel, double arithmetic: a true chain, level l + 1 is made from level l.
//   k_fhog_hist         a workgroup takes 8 x 8 cells, computes (bin, magnitude) of its 72 x 72 pixels ONCE into LDS (25.3 KiB), then
//                       every (cell, bin) is summed by one lane over the cell's 16 x 16 pixel support, row-major: a gather, no
//                       floating-point atomics anywhere.
//   k_fhog_feat         one thread per cell of the padded feature map: the 9 energies around it, the 4 normalisers, the 31 planes
//                       (plane-major [31][rows][cols], zero border written here).
//   k_fhog_score        one lane per position, 4 filters of a group side by side (4 accumulators, each walks its own filter
//                       plane-major, rows, columns: acc = acc + w * f); the weights are wave-uniform loads of [K][4] rows.  The
//                       matrix cores are not used: the order of their sums is not ours to state, and a score decides a threshold
//                       test and a sort order.  Candidates are appended through an integer atomic counter as 64-bit keys
//                       (~ordered(score) : level : filter : row : column), so their order in memory is arbitrary and the key is total.
//   k_fhog_nms          one workgroup: bitonic sort of the keys in LDS, the boxes of all candidates in parallel, a serial greedy pass.
// Built with -ffp-contract=off: every product and sum rounds on its own.  sqrtf and the float division are the correctly rounded ones
// (hipcc's default; __fsqrt_rn is NOT: without OCML_BASIC_ROUNDED_OPERATIONS it is the hardware's approximate square root).
#include "common.h"
#include "cis_hip.h"

#include <cmath>

#define FD_MAX_F 16
#define FD_MAX_SIDE 16
#define FD_MAX_LEVELS 48
#define FD_MAX_CAND 8192
#define FD_PLANES 31
#define FD_CELL 8
#define FD_GROUP 4          // filters scored side by side by one lane
#define FD_MAX_CELLS 2047   // positions per side: 11 bits of the key
#define FD_TILE 8           // cells per side of a k_fhog_hist workgroup
#define FD_PIX (FD_TILE * FD_CELL + FD_CELL)
#define FD_NMS_THREADS 1024

struct FdLevel {
    int nr, nc, cr, cc;          // image, cells
    int hr, hc, Hp, Wp;          // output cells (= positions), padded feature map
    long long img, hist, feat;   // byte offsets into the workspace (img: levels >= 1; level 0 is img0)
    int b_hist, b_feat, b_score, pad_;
};

struct FdPlan {
    int n_levels, tot_hist, tot_feat, tot_score;
    FdLevel lv[FD_MAX_LEVELS];
};

struct FdGeom {
    int F, fr, fc, padding, up;
    double ratio;  // (N - 1) / N
};

struct cis_fhogdet {
    int device = 0;
    int F = 0, fr = 0, fc = 0, padding = 0, pyramid_n = 0, max_levels = 0, min_w = 0, min_h = 0;
    double iou = 0.0, covered = 0.0;
    float* w = nullptr;       // [groups][K][FD_GROUP]
    float* thresh = nullptr;  // [F]
};

static inline size_t fd_align(size_t v) { return (v + 255) & ~(size_t)255; }

// ---- resize --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_resize_bilinear(const uint8_t* __restrict__ in, int nr, int nc, uint8_t* __restrict__ out, int onr,
                                                         int onc, double sy, double sx) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)onr * onc) return;
    const int r = (int)(idx / onc), c = (int)(idx % onc);
    const double y = (double)r * sy, x = (double)c * sx;
    int top = (int)floor(y), left = (int)floor(x);
    top = top > nr - 1 ? nr - 1 : top;
    left = left > nc - 1 ? nc - 1 : left;
    const int bot = top + 1 > nr - 1 ? nr - 1 : top + 1, right = left + 1 > nc - 1 ? nc - 1 : left + 1;
    const double fy = y - (double)top, fx = x - (double)left;
    const uint8_t* ptl = in + ((int64_t)top * nc + left) * 3;
    const uint8_t* ptr_ = in + ((int64_t)top * nc + right) * 3;
    const uint8_t* pbl = in + ((int64_t)bot * nc + left) * 3;
    const uint8_t* pbr = in + ((int64_t)bot * nc + right) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double tl = (double)ptl[ch], tr = (double)ptr_[ch], bl = (double)pbl[ch], br = (double)pbr[ch];
        const double v = (1.0 - fy) * ((1.0 - fx) * tl + fx * tr) + fy * ((1.0 - fx) * bl + fx * br);
        out[idx * 3 + ch] = (uint8_t)(int)floor(v + 0.5);
    }
}

static void fd_launch_resize(const uint8_t* in, int nr, int nc, uint8_t* out, int onr, int onc, hipStream_t st) {
    const double sy = (double)(nr - 1) / (double)(onr - 1 > 1 ? onr - 1 : 1), sx = (double)(nc - 1) / (double)(onc - 1 > 1 ? onc - 1 : 1);
    const int64_t n = (int64_t)onr * onc;
    hipLaunchKernelGGL(k_resize_bilinear, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, in, nr, nc, out, onr, onc, sy, sx);
}

// ---- FHOG ------------------------------------------------------------------------------------------------------------------------------
// the 9 unit vectors (cos, sin)(o pi / 9) as float32 literals: tests/fhog_model.py carries the same decimal strings
__device__ __forceinline__ void fd_snap(float gx, float gy, int* bin) {
    const float DX[9] = {1.0f, 0.9396926f, 0.76604444f, 0.5f, 0.17364818f, -0.17364818f, -0.5f, -0.76604444f, -0.9396926f};
    const float DY[9] = {0.0f, 0.34202015f, 0.64278764f, 0.8660254f, 0.98480775f, 0.98480775f, 0.8660254f, 0.64278764f, 0.34202015f};
    float best = 0.f;
    int bo = 0;
#pragma unroll
    for (int o = 0; o < 9; ++o) {
        const float dot = DX[o] * gx + DY[o] * gy;
        if (dot > best) {
            best = dot;
            bo = o;
        } else if (-dot > best) {
            best = -dot;
            bo = o + 9;
        }
    }
    *bin = bo;
}

__device__ __forceinline__ int fd_level_of(const FdPlan& P, int block, int which) {
    int l = 0;
    for (int i = 1; i < P.n_levels; ++i) {
        const int b = which == 0 ? P.lv[i].b_hist : (which == 1 ? P.lv[i].b_feat : P.lv[i].b_score);
        if (block >= b) l = i;
    }
    return l;
}

// bilinear weight of the pixel d rows (columns) into a cell's 16-pixel support; exact in float32
__device__ __forceinline__ float fd_weight(int d) { return d < 8 ? (float)(2 * d + 1) * 0.0625f : (float)(31 - 2 * d) * 0.0625f; }

__global__ __launch_bounds__(256) void k_fhog_hist(FdPlan P, const uint8_t* __restrict__ img0, uint8_t* __restrict__ ws) {
    __shared__ float s_mag[FD_PIX * FD_PIX];
    __shared__ uint8_t s_bin[FD_PIX * FD_PIX];
    const int tid = threadIdx.x;
    const int l = fd_level_of(P, (int)blockIdx.x, 0);
    const FdLevel& L = P.lv[l];
    const uint8_t* im = l == 0 ? img0 : ws + L.img;
    float* hist = (float*)(ws + L.hist);
    const int nr = L.nr, nc = L.nc, cr = L.cr, cc = L.cc;
    const int tiles_c = (cc + FD_TILE - 1) / FD_TILE;
    const int t = (int)blockIdx.x - L.b_hist;
    const int tr = t / tiles_c, tc = t % tiles_c;
    const int y0 = FD_CELL * FD_TILE * tr - 4, x0 = FD_CELL * FD_TILE * tc - 4;
    const int vis_r = (cr * FD_CELL < nr ? cr * FD_CELL : nr) - 1, vis_c = (cc * FD_CELL < nc ? cc * FD_CELL : nc) - 1;
    for (int i = tid; i < FD_PIX * FD_PIX; i += 256) {
        const int py = y0 + i / FD_PIX, px = x0 + i % FD_PIX;
        float mag = 0.f;
        int bin = 0;
        if (py >= 1 && py < vis_r && px >= 1 && px < vis_c) {  // vis <= size - 1: the four neighbours are inside the image
            const uint8_t* p = im + ((int64_t)py * nc + px) * 3;
            const int64_t down = (int64_t)nc * 3;
            int bv = -1, gx = 0, gy = 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int dx = (int)p[3 + ch] - (int)p[ch - 3], dy = (int)p[down + ch] - (int)p[ch - down];
                const int v = dx * dx + dy * dy;
                if (v > bv) {  // strictly: the earlier channel wins a tie
                    bv = v;
                    gx = dx;
                    gy = dy;
                }
            }
            fd_snap((float)gx, (float)gy, &bin);
            mag = sqrtf((float)bv);
        }
        s_mag[i] = mag;
        s_bin[i] = (uint8_t)bin;
    }
    __syncthreads();
    for (int item = tid; item < FD_TILE * FD_TILE * 18; item += 256) {
        const int cell = item / 18, b = item % 18;
        const int cy = cell / FD_TILE, cx = cell % FD_TILE;
        const int gr = tr * FD_TILE + cy, gc = tc * FD_TILE + cx;
        if (gr >= cr || gc >= cc) continue;
        float acc = 0.f;
        for (int dy = 0; dy < 16; ++dy) {
            const float wy = fd_weight(dy);
            const int base = (cy * FD_CELL + dy) * FD_PIX + cx * FD_CELL;
#pragma unroll
            for (int dx = 0; dx < 16; ++dx) {
                const float c = (wy * fd_weight(dx)) * s_mag[base + dx];
                acc = acc + ((int)s_bin[base + dx] == b ? c : 0.f);
            }
        }
        hist[((int64_t)gr * cc + gc) * 18 + b] = acc;
    }
}

__device__ __forceinline__ float fd_energy(const float* __restrict__ h) {
    float e = 0.f;
#pragma unroll
    for (int o = 0; o < 9; ++o) {
        const float s = h[o] + h[o + 9];
        e = e + s * s;
    }
    return e;
}

__device__ __forceinline__ float fd_min(float a, float lim) { return lim < a ? lim : a; }

// one padded feature cell: idx = pr * Wp + pc
__device__ __forceinline__ void fd_feat_cell(const float* __restrict__ hist, int cc, int hr, int hc, int Hp, int Wp, int r0, int c0, int idx,
                                             float* __restrict__ feat) {
    const int64_t ps = (int64_t)Hp * Wp;
    const int y = idx / Wp - r0, x = idx % Wp - c0;
    if (y < 0 || y >= hr || x < 0 || x >= hc) {
        for (int p = 0; p < FD_PLANES; ++p) feat[p * ps + idx] = 0.f;
        return;
    }
    float e[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) e[i][j] = fd_energy(hist + ((int64_t)(y + i) * cc + (x + j)) * 18);
    const float eps = 1e-4f;
    const float n1 = 1.0f / sqrtf(((e[1][1] + e[1][2]) + e[2][1]) + e[2][2] + eps);
    const float n2 = 1.0f / sqrtf(((e[0][1] + e[0][2]) + e[1][1]) + e[1][2] + eps);
    const float n3 = 1.0f / sqrtf(((e[1][0] + e[1][1]) + e[2][0]) + e[2][1] + eps);
    const float n4 = 1.0f / sqrtf(((e[0][0] + e[0][1]) + e[1][0]) + e[1][1] + eps);
    const float* h = hist + ((int64_t)(y + 1) * cc + (x + 1)) * 18;
    float t1 = 0.f, t2 = 0.f, t3 = 0.f, t4 = 0.f;
    for (int o = 0; o < 18; ++o) {
        const float v = h[o];
        const float h1 = fd_min(v * n1, 0.2f), h2 = fd_min(v * n2, 0.2f), h3 = fd_min(v * n3, 0.2f), h4 = fd_min(v * n4, 0.2f);
        feat[o * ps + idx] = 0.5f * (((h1 + h2) + h3) + h4);
        t1 = t1 + h1;
        t2 = t2 + h2;
        t3 = t3 + h3;
        t4 = t4 + h4;
    }
    for (int o = 0; o < 9; ++o) {
        const float v = h[o] + h[o + 9];
        const float h1 = fd_min(v * n1, 0.2f), h2 = fd_min(v * n2, 0.2f), h3 = fd_min(v * n3, 0.2f), h4 = fd_min(v * n4, 0.2f);
        feat[(18 + o) * ps + idx] = 0.5f * (((h1 + h2) + h3) + h4);
    }
    feat[27 * ps + idx] = 0.2357f * t1;
    feat[28 * ps + idx] = 0.2357f * t2;
    feat[29 * ps + idx] = 0.2357f * t3;
    feat[30 * ps + idx] = 0.2357f * t4;
}

__global__ __launch_bounds__(256) void k_fhog_feat(FdPlan P, int r0, int c0, uint8_t* __restrict__ ws) {
    const int l = fd_level_of(P, (int)blockIdx.x, 1);
    const FdLevel& L = P.lv[l];
    const int idx = ((int)blockIdx.x - L.b_feat) * 256 + (int)threadIdx.x;
    if (idx >= L.Hp * L.Wp) return;
    fd_feat_cell((const float*)(ws + L.hist), L.cc, L.hr, L.hc, L.Hp, L.Wp, r0, c0, idx, (float*)(ws + L.feat));
}

// ---- scores ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t fd_ordered(float v) {  // unsigned order = float order
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(256) void k_fhog_score(FdPlan P, FdGeom G, const uint8_t* __restrict__ ws, const float* __restrict__ w,
                                                    const float* __restrict__ thresh, double adjust, float* __restrict__ sal_out,
                                                    unsigned long long* __restrict__ cand, int* __restrict__ counter) {
    const int l = fd_level_of(P, (int)blockIdx.x, 2);
    const FdLevel& L = P.lv[l];
    const int idx = ((int)blockIdx.x - L.b_score) * 256 + (int)threadIdx.x;
    const int R = L.hr, C = L.hc;
    if (idx >= R * C) return;
    const int r = idx / C, c = idx % C;
    const int group = (int)blockIdx.y;
    const int64_t ps = (int64_t)L.Hp * L.Wp;
    const float* f0 = (const float*)(ws + L.feat) + (int64_t)r * L.Wp + c;
    const float4* wg = (const float4*)(w + (int64_t)group * FD_PLANES * G.fr * G.fc * FD_GROUP);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int k = 0;
    for (int p = 0; p < FD_PLANES; ++p)
        for (int i = 0; i < G.fr; ++i) {
            const float* row = f0 + p * ps + (int64_t)i * L.Wp;
            // the loads of a whole filter row are issued before its adds (past the row's end the last column again: in bounds, no
            // branch); the adds keep their order
            float x[FD_MAX_SIDE];
#pragma unroll
            for (int j = 0; j < FD_MAX_SIDE; ++j) x[j] = row[j < G.fc ? j : G.fc - 1];
#pragma unroll
            for (int j = 0; j < FD_MAX_SIDE; ++j)
                if (j < G.fc) {
                    const float4 wv = wg[k + j];
                    a0 = a0 + wv.x * x[j];
                    a1 = a1 + wv.y * x[j];
                    a2 = a2 + wv.z * x[j];
                    a3 = a3 + wv.w * x[j];
                }
            k += G.fc;
        }
    const float acc[FD_GROUP] = {a0, a1, a2, a3};
#pragma unroll
    for (int g = 0; g < FD_GROUP; ++g) {
        const int f = group * FD_GROUP + g;
        if (f >= G.F) break;
        const float s = acc[g], th = thresh[f];
        if (sal_out != nullptr) sal_out[((int64_t)f * R + r) * C + c] = s;  // (cis_fhog_scores_dev: one level)
        if (cand != nullptr && (double)s >= (double)th + adjust) {
            const int slot = atomicAdd(counter, 1);
            if (slot < FD_MAX_CAND) {
                const uint32_t hi = ~fd_ordered(s - th);
                const uint32_t lo = ((uint32_t)l << 26) | ((uint32_t)f << 22) | ((uint32_t)r << 11) | (uint32_t)c;
                cand[slot] = ((unsigned long long)hi << 32) | lo;
            }
        }
    }
}

// ---- boxes, sort, non-maximum suppression ----------------------------------------------------------------------------------------------
__device__ __forceinline__ double fd_to_image(int p, int off) {
    const int q = p - off;
    return (double)((q + 1) * FD_CELL + 1 + (q >= 0 ? FD_CELL / 2 : -(FD_CELL / 2)));
}

__device__ __forceinline__ int4 fd_rect(const FdGeom& G, int level, int row, int col) {
    const int bw = G.fc - 2 * G.padding, bh = G.fr - 2 * G.padding;
    const int left = col + G.fc / 2 - bw / 2, top = row + G.fr / 2 - bh / 2;
    double v[4] = {fd_to_image(left, (G.fc - 1) / 2), fd_to_image(top, (G.fr - 1) / 2), fd_to_image(left + bw - 1, (G.fc - 1) / 2),
                   fd_to_image(top + bh - 1, (G.fr - 1) / 2)};
    int out[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double x = v[i];
        for (int lv = 0; lv < level; ++lv) x = (x - 0.3) / G.ratio + 0.3;
        x = floor(x + 0.5);
        for (int u = 0; u < G.up; ++u) x = floor(((x - 0.3) * 0.5 + 0.3) + 0.5);
        out[i] = (int)fmin(fmax(x, -2147483648.0), 2147483647.0);
    }
    return make_int4(out[0], out[1], out[2], out[3]);
}

__device__ __forceinline__ long long fd_area(long long l, long long t, long long r, long long b) {
    const long long w = r - l + 1, h = b - t + 1;
    return (w > 0 ? w : 0) * (h > 0 ? h : 0);
}

__device__ __forceinline__ bool fd_overlaps(const int4 a, const int4 b, double iou, double covered) {
    const long long inner = fd_area(max(a.x, b.x), max(a.y, b.y), min(a.z, b.z), min(a.w, b.w));
    if (inner == 0) return false;
    const long long outer = fd_area(min(a.x, b.x), min(a.y, b.y), max(a.z, b.z), max(a.w, b.w));
    const double in = (double)inner;
    return in / (double)outer > iou || in / (double)fd_area(a.x, a.y, a.z, a.w) > covered || in / (double)fd_area(b.x, b.y, b.z, b.w) > covered;
}

__global__ __launch_bounds__(FD_NMS_THREADS) void k_fhog_nms(FdGeom G, double iou, double covered, const unsigned long long* __restrict__ cand,
                                                             const int* __restrict__ counter, const float* __restrict__ thresh, int4* srect,
                                                             int4* kept, int32_t* __restrict__ d_rects, float* __restrict__ d_scores,
                                                             int32_t* __restrict__ d_filter, int max_dets, int32_t* __restrict__ d_count) {
    __shared__ unsigned long long s_key[FD_MAX_CAND];
    const int tid = threadIdx.x;
    const int total = *counter;
    const int n = total < FD_MAX_CAND ? total : FD_MAX_CAND;
    int np2 = 2;
    while (np2 < n) np2 <<= 1;
    for (int i = tid; i < np2; i += FD_NMS_THREADS) s_key[i] = i < n ? cand[i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += FD_NMS_THREADS) {
                const int m = i ^ j;
                if (m > i) {
                    const unsigned long long a = s_key[i], b = s_key[m];
                    if (((i & k) == 0) ? (a > b) : (a < b)) {
                        s_key[i] = b;
                        s_key[m] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (int i = tid; i < n; i += FD_NMS_THREADS) {
        const uint32_t lo = (uint32_t)s_key[i];
        srect[i] = fd_rect(G, (int)(lo >> 26), (int)((lo >> 11) & 0x7ffu), (int)(lo & 0x7ffu));
    }
    __syncthreads();
    int nk = 0;
    for (int i = 0; i < n; ++i) {
        const int4 rc = srect[i];
        int sup = 0;
        for (int t = tid; t < nk; t += FD_NMS_THREADS) sup |= fd_overlaps(kept[t], rc, iou, covered) ? 1 : 0;
        if (__syncthreads_or(sup)) continue;
        if (tid == 0) {
            kept[nk] = rc;
            if (nk < max_dets) {
                const unsigned long long key = s_key[i];
                const uint32_t o = ~(uint32_t)(key >> 32);
                d_rects[4 * nk] = rc.x;
                d_rects[4 * nk + 1] = rc.y;
                d_rects[4 * nk + 2] = rc.z;
                d_rects[4 * nk + 3] = rc.w;
                d_scores[nk] = __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
                d_filter[nk] = (int32_t)(((uint32_t)key >> 22) & 0xfu);
            }
        }
        ++nk;
        __syncthreads();  // the new kept box is visible to the whole workgroup
    }
    if (tid == 0) {
        d_count[0] = nk;
        d_count[1] = total;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void fd_up_size(int nr, int nc, int* onr, int* onc) {  // rect_up (N = 2) of the image rectangle: 2 n - 1
    const double t = floor(((0.0 - 0.3) / 0.5 + 0.3) + 0.5);
    *onr = (int)(floor((((double)(nr - 1) - 0.3) / 0.5 + 0.3) + 0.5) - t) + 1;
    *onc = (int)(floor((((double)(nc - 1) - 0.3) / 0.5 + 0.3) + 0.5) - t) + 1;
}

struct FdLayout {
    int up_nr[3], up_nc[3];  // sizes after 0, 1, 2 rounds
    size_t up_off[3];        // workspace offsets of rounds 1, 2
    size_t cand, counter, srect, kept, total;
};

static void fd_level_dims(FdLevel* L, int nr, int nc, int pad_rows, int pad_cols) {
    L->nr = nr;
    L->nc = nc;
    L->cr = (int)((double)nr / FD_CELL + 0.5);
    L->cc = (int)((double)nc / FD_CELL + 0.5);
    L->hr = L->cr - 2 > 0 ? L->cr - 2 : 0;
    L->hc = L->cc - 2 > 0 ? L->cc - 2 : 0;
    if (L->hr == 0 || L->hc == 0) L->hr = L->hc = 0;
    L->Hp = L->hr ? L->hr + pad_rows - 1 : 0;
    L->Wp = L->hc ? L->hc + pad_cols - 1 : 0;
}

static int fd_plan(const cis_fhogdet* h, int nr, int nc, int up, FdPlan* P, FdLayout* Y) {
    CIS_REQUIRE(nr >= 1 && nc >= 1, "fhog detector: image of %d x %d", nr, nc);
    CIS_REQUIRE(up >= 0 && up <= 2, "fhog detector: up_sample = %d, 0, 1 or 2 is taken", up);
    size_t off = 0;
    Y->up_nr[0] = nr;
    Y->up_nc[0] = nc;
    for (int u = 1; u <= up; ++u) {
        fd_up_size(Y->up_nr[u - 1], Y->up_nc[u - 1], &Y->up_nr[u], &Y->up_nc[u]);
        Y->up_off[u] = off;
        off = fd_align(off + (size_t)Y->up_nr[u] * Y->up_nc[u] * 3);
    }
    int lr = Y->up_nr[up], lc = Y->up_nc[up];
    CIS_REQUIRE(lr / FD_CELL <= FD_MAX_CELLS && lc / FD_CELL <= FD_MAX_CELLS, "fhog detector: a %d x %d image (after up-sampling) has more than %d cells a side",
                lr, lc, FD_MAX_CELLS);
    memset(P, 0, sizeof(*P));
    int n = 0;
    for (;;) {
        CIS_REQUIRE(n < FD_MAX_LEVELS, "fhog detector: more than %d pyramid levels for a %d x %d image with pyramid_down<%d>", FD_MAX_LEVELS, nr, nc,
                    h->pyramid_n);
        fd_level_dims(&P->lv[n], lr, lc, h->fr, h->fc);
        ++n;
        if (n >= h->max_levels) break;
        lr = (int)(((int64_t)(h->pyramid_n - 1) * lr) / h->pyramid_n);
        lc = (int)(((int64_t)(h->pyramid_n - 1) * lc) / h->pyramid_n);
        if (lc < h->min_w || lr < h->min_h || lr < 1 || lc < 1) break;
    }
    P->n_levels = n;
    for (int l = 1; l < n; ++l) {
        P->lv[l].img = (long long)off;
        off = fd_align(off + (size_t)P->lv[l].nr * P->lv[l].nc * 3);
    }
    for (int l = 0; l < n; ++l) {
        FdLevel& L = P->lv[l];
        L.hist = (long long)off;
        off = fd_align(off + (size_t)L.cr * L.cc * 18 * sizeof(float));
        L.feat = (long long)off;
        off = fd_align(off + (size_t)FD_PLANES * L.Hp * L.Wp * sizeof(float));
        L.b_hist = P->tot_hist;
        L.b_feat = P->tot_feat;
        L.b_score = P->tot_score;
        if (L.hr > 0) {  // a level without output cells takes part in nothing
            P->tot_hist += (int)(ceil_div(L.cr, FD_TILE) * ceil_div(L.cc, FD_TILE));
            P->tot_feat += (int)ceil_div((int64_t)L.Hp * L.Wp, 256);
            P->tot_score += (int)ceil_div((int64_t)L.hr * L.hc, 256);
        }
    }
    Y->cand = off;
    off = fd_align(off + (size_t)FD_MAX_CAND * 8);
    Y->counter = off;
    off = fd_align(off + 16);
    Y->srect = off;
    off = fd_align(off + (size_t)FD_MAX_CAND * 16);
    Y->kept = off;
    off = fd_align(off + (size_t)FD_MAX_CAND * 16);
    Y->total = off;
    return CIS_OK;
}

extern "C" void cis_fhogdet_destroy(cis_fhogdet* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->w) (void)hipFree(h->w);
    if (h->thresh) (void)hipFree(h->thresh);
    delete h;
}

static int fd_upload(void** dst, const void* src, size_t bytes) {
    CIS_CHECK_HIP(hipMalloc(dst, bytes));
    CIS_CHECK_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return CIS_OK;
}

// w [F][31][fr][fc] -> [groups][K][FD_GROUP], the filters of a group side by side, missing ones zero
static std::vector<float> fd_pack_weights(int F, int fr, int fc, const float* w) {
    const int K = FD_PLANES * fr * fc, groups = (F + FD_GROUP - 1) / FD_GROUP;
    std::vector<float> out((size_t)groups * K * FD_GROUP, 0.f);
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < K; ++k) out[((size_t)(f / FD_GROUP) * K + k) * FD_GROUP + f % FD_GROUP] = w[(size_t)f * K + k];
    return out;
}

static int fd_check_filters(int F, int fr, int fc, const float* w) {
    CIS_REQUIRE(F >= 1 && F <= FD_MAX_F, "fhog detector: F = %d filters, the kernel takes 1 to %d", F, FD_MAX_F);
    CIS_REQUIRE(fr >= 1 && fr <= FD_MAX_SIDE && fc >= 1 && fc <= FD_MAX_SIDE, "fhog detector: filters of %d x %d cells, the kernel takes sides of 1 to %d",
                fr, fc, FD_MAX_SIDE);
    CIS_REQUIRE(w != nullptr, "fhog detector: NULL array");
    const size_t n = (size_t)F * FD_PLANES * fr * fc;
    for (size_t i = 0; i < n; ++i) CIS_REQUIRE(std::isfinite(w[i]), "fhog detector: weight %zu of filter %zu is not finite", i % (n / F), i / (n / F));
    return CIS_OK;
}

extern "C" int cis_fhogdet_create(cis_fhogdet** out, int F, int filter_rows, int filter_cols, int cell_size, int padding, int pyramid_n,
                                  int max_levels, int min_layer_w, int min_layer_h, const float* w, const float* thresh, double iou_thresh,
                                  double covered_thresh) {
    CIS_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    CIS_TRY(fd_check_filters(F, filter_rows, filter_cols, w));
    CIS_REQUIRE(cell_size == FD_CELL, "fhog detector: cell_size = %d, the kernel takes %d", cell_size, FD_CELL);
    CIS_REQUIRE(padding >= 0 && 2 * padding < filter_rows && 2 * padding < filter_cols, "fhog detector: padding = %d leaves no box of a %d x %d filter",
                padding, filter_rows, filter_cols);
    CIS_REQUIRE(pyramid_n >= 2 && pyramid_n <= 16, "fhog detector: pyramid_down<%d>, the kernel takes 2 to 16", pyramid_n);
    CIS_REQUIRE(max_levels >= 1 && min_layer_w >= 1 && min_layer_h >= 1, "fhog detector: max_levels = %d, min layer %d x %d: all must be at least 1",
                max_levels, min_layer_w, min_layer_h);
    CIS_REQUIRE(thresh != nullptr, "fhog detector: NULL array");
    for (int f = 0; f < F; ++f) CIS_REQUIRE(std::isfinite(thresh[f]), "fhog detector: threshold %d is not finite", f);
    CIS_REQUIRE(iou_thresh >= 0.0 && iou_thresh <= 1.0 && covered_thresh >= 0.0 && covered_thresh <= 1.0,
                "fhog detector: overlap thresholds %g, %g are not in [0, 1]", iou_thresh, covered_thresh);
    CIS_TRY(cis_lazy_init());
    const std::vector<float> packed = fd_pack_weights(F, filter_rows, filter_cols, w);
    cis_fhogdet* h = new cis_fhogdet();
    h->device = cis_current_device();
    h->F = F; h->fr = filter_rows; h->fc = filter_cols; h->padding = padding; h->pyramid_n = pyramid_n;
    h->max_levels = max_levels; h->min_w = min_layer_w; h->min_h = min_layer_h; h->iou = iou_thresh; h->covered = covered_thresh;
    int rc = hipSetDevice(h->device) == hipSuccess ? CIS_OK : CIS_EHIP;
    if (rc != CIS_OK) cis_set_error("fhog detector: hipSetDevice(%d) failed", h->device);
    if (rc == CIS_OK) rc = fd_upload((void**)&h->w, packed.data(), packed.size() * sizeof(float));
    if (rc == CIS_OK) rc = fd_upload((void**)&h->thresh, thresh, (size_t)F * sizeof(float));
    if (rc != CIS_OK) {
        cis_fhogdet_destroy(h);
        return rc;
    }
    *out = h;
    return CIS_OK;
}

extern "C" int64_t cis_fhogdet_workspace_bytes(cis_fhogdet* h, int nr, int nc, int up_sample) {
    if (h == nullptr) {
        cis_set_error("fhog detector is NULL");
        return CIS_EINVAL;
    }
    FdPlan P;
    FdLayout Y;
    const int rc = fd_plan(h, nr, nc, up_sample, &P, &Y);
    return rc != CIS_OK ? (int64_t)rc : (int64_t)Y.total;
}

// ev: NULL, or 6 events recorded around the five stages (resizes, histograms, features, scores, sort + NMS): cis_fhogdet_profile
static int fd_run(cis_fhogdet* h, const uint8_t* d_img, int nr, int nc, int up_sample, double adjust_threshold, void* d_ws, int64_t ws_bytes,
                  int32_t* d_rects, float* d_scores, int32_t* d_filter, int max_dets, int32_t* d_count, void* stream, hipEvent_t* ev) {
    CIS_REQUIRE(h != nullptr, "fhog detector is NULL");
    CIS_REQUIRE(d_img && d_ws && d_count && max_dets >= 0 && (max_dets == 0 || (d_rects && d_scores && d_filter)),
                "fhog detector: NULL buffer or max_dets = %d", max_dets);
    CIS_REQUIRE(std::isfinite(adjust_threshold), "fhog detector: adjust_threshold is not finite");
    FdPlan P;
    FdLayout Y;
    CIS_TRY(fd_plan(h, nr, nc, up_sample, &P, &Y));
    CIS_REQUIRE(ws_bytes >= (int64_t)Y.total, "fhog detector: a workspace of %lld bytes, %zu are needed for a %d x %d image at up_sample = %d",
                (long long)ws_bytes, Y.total, nr, nc, up_sample);
    CIS_TRY(cis_lazy_init());
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = (uint8_t*)d_ws;
    const uint8_t* img0 = d_img;
    if (ev) CIS_CHECK_HIP(hipEventRecord(ev[0], st));
    for (int u = 1; u <= up_sample; ++u) {
        fd_launch_resize(img0, Y.up_nr[u - 1], Y.up_nc[u - 1], ws + Y.up_off[u], Y.up_nr[u], Y.up_nc[u], st);
        img0 = ws + Y.up_off[u];
    }
    for (int l = 1; l < P.n_levels; ++l)
        fd_launch_resize(l == 1 ? img0 : ws + P.lv[l - 1].img, P.lv[l - 1].nr, P.lv[l - 1].nc, ws + P.lv[l].img, P.lv[l].nr, P.lv[l].nc, st);
    int* counter = (int*)(ws + Y.counter);
    CIS_CHECK_HIP(hipMemsetAsync(counter, 0, 16, st));
    const FdGeom G = {h->F, h->fr, h->fc, h->padding, up_sample, (double)(h->pyramid_n - 1) / (double)h->pyramid_n};
    if (ev) CIS_CHECK_HIP(hipEventRecord(ev[1], st));
    if (P.tot_hist > 0) hipLaunchKernelGGL(k_fhog_hist, dim3((unsigned)P.tot_hist), dim3(256), 0, st, P, img0, ws);
    if (ev) CIS_CHECK_HIP(hipEventRecord(ev[2], st));
    if (P.tot_hist > 0) hipLaunchKernelGGL(k_fhog_feat, dim3((unsigned)P.tot_feat), dim3(256), 0, st, P, (h->fr - 1) / 2, (h->fc - 1) / 2, ws);
    if (ev) CIS_CHECK_HIP(hipEventRecord(ev[3], st));
    if (P.tot_hist > 0)
        hipLaunchKernelGGL(k_fhog_score, dim3((unsigned)P.tot_score, (unsigned)((h->F + FD_GROUP - 1) / FD_GROUP)), dim3(256), 0, st, P, G,
                           (const uint8_t*)ws, (const float*)h->w, (const float*)h->thresh, adjust_threshold, (float*)nullptr,
                           (unsigned long long*)(ws + Y.cand), counter);
    if (ev) CIS_CHECK_HIP(hipEventRecord(ev[4], st));
    hipLaunchKernelGGL(k_fhog_nms, dim3(1), dim3(FD_NMS_THREADS), 0, st, G, h->iou, h->covered, (const unsigned long long*)(ws + Y.cand),
                       (const int*)counter, (const float*)h->thresh, (int4*)(ws + Y.srect), (int4*)(ws + Y.kept), d_rects, d_scores, d_filter,
                       max_dets, d_count);
    if (ev) CIS_CHECK_HIP(hipEventRecord(ev[5], st));
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_fhogdet_run_dev(cis_fhogdet* h, const uint8_t* d_img, int nr, int nc, int up_sample, double adjust_threshold, void* d_ws,
                                   int64_t ws_bytes, int32_t* d_rects, float* d_scores, int32_t* d_filter, int max_dets, int32_t* d_count,
                                   void* stream) {
    return fd_run(h, d_img, nr, nc, up_sample, adjust_threshold, d_ws, ws_bytes, d_rects, d_scores, d_filter, max_dets, d_count, stream, nullptr);
}

extern "C" int cis_fhogdet_profile(cis_fhogdet* h, const uint8_t* d_img, int nr, int nc, int up_sample, double adjust_threshold, void* d_ws,
                                   int64_t ws_bytes, int32_t* d_rects, float* d_scores, int32_t* d_filter, int max_dets, int32_t* d_count,
                                   void* stream, float* stage_ms) {
    CIS_REQUIRE(stage_ms != nullptr, "fhog detector: stage_ms is NULL");
    CIS_TRY(cis_lazy_init());
    hipEvent_t ev[6] = {};
    int rc = CIS_OK;
    for (int i = 0; i < 6 && rc == CIS_OK; ++i)
        if (hipEventCreate(&ev[i]) != hipSuccess) rc = CIS_EHIP;
    if (rc == CIS_OK) rc = fd_run(h, d_img, nr, nc, up_sample, adjust_threshold, d_ws, ws_bytes, d_rects, d_scores, d_filter, max_dets, d_count, stream, ev);
    if (rc == CIS_OK && hipEventSynchronize(ev[5]) != hipSuccess) rc = CIS_EHIP;
    for (int i = 0; i < 5 && rc == CIS_OK; ++i)
        if (hipEventElapsedTime(&stage_ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = CIS_EHIP;
    if (rc == CIS_EHIP) cis_set_error("fhog detector: a HIP event call failed while profiling");
    for (int i = 0; i < 6; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    return rc;
}

// ---- the stages on their own (tests, reuse) --------------------------------------------------------------------------------------------
extern "C" int cis_resize_bilinear_rgb_dev(const uint8_t* d_in, int nr, int nc, uint8_t* d_out, int onr, int onc, void* stream) {
    CIS_REQUIRE(nr >= 1 && nc >= 1 && onr >= 1 && onc >= 1, "resize: %d x %d -> %d x %d", nr, nc, onr, onc);
    CIS_REQUIRE((int64_t)nr * nc < (1ll << 30) && (int64_t)onr * onc < (1ll << 30), "resize: %d x %d -> %d x %d: more than 2^30 pixels", nr, nc, onr, onc);
    CIS_REQUIRE(d_in && d_out, "resize: NULL buffer");
    CIS_TRY(cis_lazy_init());
    fd_launch_resize(d_in, nr, nc, d_out, onr, onc, (hipStream_t)stream);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

static int fd_single_level(int nr, int nc, int cell_size, int pad_rows, int pad_cols, FdPlan* P) {
    CIS_REQUIRE(cell_size == FD_CELL, "fhog: cell_size = %d, the kernel takes %d", cell_size, FD_CELL);
    CIS_REQUIRE(nr >= 1 && nc >= 1 && nr / FD_CELL <= FD_MAX_CELLS && nc / FD_CELL <= FD_MAX_CELLS, "fhog: image of %d x %d", nr, nc);
    CIS_REQUIRE(pad_rows >= 1 && pad_rows <= FD_MAX_SIDE && pad_cols >= 1 && pad_cols <= FD_MAX_SIDE, "fhog: padding of %d x %d, 1 to %d is taken",
                pad_rows, pad_cols, FD_MAX_SIDE);
    memset(P, 0, sizeof(*P));
    P->n_levels = 1;
    fd_level_dims(&P->lv[0], nr, nc, pad_rows, pad_cols);
    return CIS_OK;
}

extern "C" int cis_fhog_extract_dev(const uint8_t* d_img, int nr, int nc, int cell_size, int pad_rows, int pad_cols, float* d_hist, float* d_feat,
                                    void* stream) {
    FdPlan P;
    CIS_TRY(fd_single_level(nr, nc, cell_size, pad_rows, pad_cols, &P));
    FdLevel& L = P.lv[0];
    if (L.hr == 0) return CIS_OK;  // fewer than 3 cells a side: no output, nothing is written
    CIS_REQUIRE(d_img && d_hist && d_feat, "fhog: NULL buffer");
    CIS_TRY(cis_lazy_init());
    // the two buffers are addressed from d_hist as the workspace base
    L.hist = 0;
    L.feat = (long long)((const uint8_t*)d_feat - (const uint8_t*)d_hist);
    P.tot_hist = (int)(ceil_div(L.cr, FD_TILE) * ceil_div(L.cc, FD_TILE));
    P.tot_feat = (int)ceil_div((int64_t)L.Hp * L.Wp, 256);
    hipLaunchKernelGGL(k_fhog_hist, dim3((unsigned)P.tot_hist), dim3(256), 0, (hipStream_t)stream, P, d_img, (uint8_t*)d_hist);
    hipLaunchKernelGGL(k_fhog_feat, dim3((unsigned)P.tot_feat), dim3(256), 0, (hipStream_t)stream, P, (pad_rows - 1) / 2, (pad_cols - 1) / 2,
                       (uint8_t*)d_hist);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

extern "C" int cis_fhog_scores_dev(const float* d_feat, int rows, int cols, int F, int filter_rows, int filter_cols, const float* w, float* d_scores,
                                   void* stream) {
    CIS_TRY(fd_check_filters(F, filter_rows, filter_cols, w));
    CIS_REQUIRE(rows >= 0 && cols >= 0 && rows <= FD_MAX_CELLS + FD_MAX_SIDE && cols <= FD_MAX_CELLS + FD_MAX_SIDE, "fhog scores: a feature map of %d x %d",
                rows, cols);
    if (rows < filter_rows || cols < filter_cols) return CIS_OK;  // the filter fits nowhere: nothing is written
    CIS_REQUIRE(d_feat && d_scores, "fhog scores: NULL buffer");
    CIS_TRY(cis_lazy_init());
    hipStream_t st = (hipStream_t)stream;
    const std::vector<float> packed = fd_pack_weights(F, filter_rows, filter_cols, w);
    float* d_w = nullptr;
    CIS_CHECK_HIP(hipMalloc((void**)&d_w, packed.size() * sizeof(float)));  // a test entry: allocates, copies and waits
    hipError_t e = hipMemcpy(d_w, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice);
    FdPlan P;
    memset(&P, 0, sizeof(P));
    P.n_levels = 1;
    FdLevel& L = P.lv[0];
    L.Hp = rows;
    L.Wp = cols;
    L.hr = rows - filter_rows + 1;
    L.hc = cols - filter_cols + 1;
    L.feat = 0;
    const FdGeom G = {F, filter_rows, filter_cols, 0, 0, 0.5};
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_fhog_score, dim3((unsigned)ceil_div((int64_t)L.hr * L.hc, 256), (unsigned)((F + FD_GROUP - 1) / FD_GROUP)), dim3(256), 0, st,
                           P, G, (const uint8_t*)d_feat, (const float*)d_w, (const float*)d_w, 0.0, d_scores, (unsigned long long*)nullptr,
                           (int*)nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipFree(d_w);
    CIS_CHECK_HIP(e);
    return CIS_OK;
}
