// What lopq_eval.hip (the driver, the exact chain, finalize and the exact-only path) and knn_int8.hip (the prefilter of the exact k-NN
// on int8 feature rows, on the int8 matrix cores) share.
#pragma once
#include "common.h"

constexpr int KNN_I8_MAX_D = 65536;  // 64 * 127 * d must stay below 2^31: the int32 accumulators of knn_int8.hip

// bytes of the permuted query digits knn_int8.hip stages from (queries padded to its tile of 64, dims to its span of 128)
static inline size_t knn_i8_digit_bytes(int m1, int d) { return (size_t)ceil_div(m1, 64) * 64 * 3 * (size_t)ceil_div(d, 128) * 128; }

struct KnnI8Args {
    const unsigned char* rows;  // the store's rows as they lie: 16 + d bytes each, the float32 scale first
    int m2, d;
    const void* Q;              // [m1][d] float32 or float64
    int q_f64, m1;
    int k, S, W, cap;           // S row splits of the grid, W / cap the pitch and the limit of a candidate list
    int64_t base;
    // workspaces; `maxima`, `cnt` are zeroed by the caller
    void* digits;               // knn_i8_digit_bytes
    int* qe;                    // [m1 padded to 64] the query's exponent, INT_MIN for a query the prefilter does not serve
    const double* xn2;          // [m1] |x|^2 in float64
    float* stat;                // [m2][2]: ny32 and the scale of every row
    unsigned long long* maxima; // [2]: max |y_j|^2 and max w_j as ordered bits of float64
    float* gmin;                // [m1][128 S]
    float* thr;                 // [m1]
    int* cnt;                   // [m1]
    int64_t* cand;              // [m1][W]
};

// Row statistics, query digits, surface<MIN>, select, surface<EMIT>: leaves cnt / cand for k_knn_finalize.
int cis_knn_i8_prefilter(const KnnI8Args& a, hipStream_t st);
