// The LDS eigensolver of sym_eig.hip for callers inside the library: cis_sym_eig_dev without the argument checks and the lazy
// initialisation (1 <= d <= 128, batch >= 1, device pointers, d_info may be NULL).  Only enqueues on `st`.
// csrc/sym_eig_block.hip solves its pivots with it.
#pragma once
#include "common.h"

int cis_sym_eig_launch(const double* d_A, int64_t batch, int d, double* d_W, double* d_V, int32_t* d_info, hipStream_t st);
