// LOPQ index + batched search on MI355X.
//
// Replaces lopq/lopq/search.py: multisequence :13-82, get_result_quota :110-135,
// compute_distances (ADC) :137-177, search :179-224, LOPQSearcher (dict index) :310-382 -- for a
// whole batch of queries per call.
//
// Data layout in HBM
//   codes  [N][M] uint8   fine codes, cell-contiguous (CSR over the V*V coarse cells), inside a
//                         cell in insertion order (= the reference's per-cell list order)
//   ids    [N]    int64   caller ids, same order
//   loff   [V*V+1] int64  CSR offsets of the cells stored on THIS shard
//   gcount [V*V]  int64   item count of every cell over ALL shards (drives the quota cut-off)
//
// Pipeline per query batch (all on one stream):
//   PCA -> coarse distances (numpy order) -> per-split rank -> multisequence plan (count) ->
//   exclusive scan -> plan (emit work items + table list) -> ADC tables -> ADC scan + block
//   top-k -> per-query merge -> ids/dists.
//
// This file: the driver (search_batch), the routes, and the kernels of the tables, the scans, the merges and the selections.
// Everything up to and including the plan -- rank, frontier walk, plan scan, slot builder, and the host phases that launch
// them -- is lopq_plan.hip; lopq_batch.h holds what the two share.
#include "lopq_batch.h"

// ================================================================================================
// kernel: ADC tables  (lopq/lopq/model.py:673-704 for one (query, split, coarse id))
// ================================================================================================
template <typename CT>
__global__ __launch_bounds__(256) void k_tables(const CT* __restrict__ X /* [nq][D] */, const CT* __restrict__ Cs,
                                                const double* __restrict__ Rt, const double* __restrict__ mus,
                                                const double* __restrict__ subs, const TabDesc* __restrict__ tabs,
                                                int V, int h, int w, int nf, int K, int D,
                                                double* __restrict__ T /* [ntab][nf][K] */, PwProg prog_w,
                                                double* __restrict__ px_out /* [ntab][h] or null */,
                                                const int* __restrict__ tab_order, int first) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* v = reinterpret_cast<double*>(smem);  // [h]
    double* px = v + h;                           // [h]
    const int tab = tab_order ? tab_order[first + blockIdx.x] : first + (int)blockIdx.x;
    const TabDesc td = tabs[tab];
    const int s = td.split, c = td.cluster;
    const CT* x = X + (int64_t)td.q * D + s * h;
    const CT* Cc = Cs + ((int64_t)s * V + c) * h;
    const double* mu = mus + ((int64_t)s * V + c) * h;
    const double* R = Rt + ((int64_t)s * V + c) * h * h;
    for (int k = threadIdx.x; k < h; k += blockDim.x) {
        const CT res = x[k] - Cc[k];  // rounds in CT (float32 when both are float32), model.py:635
        v[k] = (double)res - mu[k];
    }
    __syncthreads();
    // px[i] = sum_k R[k][i] v[k] as ONE chain of fused multiply-adds, k ascending (round 4: the arithmetic of
    // v_mfma_f64_16x16x4_f64, which k_tables_group_mfma runs the grouped tables on -- tools/probes/mfma_f64_order.hip; the
    // reference's BLAS order is unspecified anyway).  Every route to px uses this order: the routes agree bit for bit.
    for (int i = threadIdx.x; i < h; i += blockDim.x) {
        double acc = 0.0;
        for (int k = 0; k < h; ++k) acc = fma(R[(int64_t)k * h + i], v[k], acc);
        px[i] = acc;
    }
    __syncthreads();
    if (px_out) {  // two-kernel path: the distance tables are built by k_tables_from_px
        for (int i = threadIdx.x; i < h; i += blockDim.x) px_out[(int64_t)tab * h + i] = px[i];
        return;
    }
    double* out = T + (int64_t)tab * nf * K;
    for (int e = threadIdx.x; e < nf * K; e += blockDim.x) {
        const int j = e / K, k = e % K;
        const double* sc = subs + ((int64_t)(s * nf + j) * K + k) * w;
        const double* f = px + j * w;
        auto elem = [&](int i) -> double { const double df = f[i] - sc[i]; return df * df; };
        out[e] = pw_sum<double>(prog_w, elem);
    }
}

// Second half of the table build for the common sub-vector widths: one block = (chunk of 64 table
// items, fine split j, coarse split z).  Thread k keeps sub-centroid (z, j, k) in registers and walks
// the chunk, so the 32 KB sub-quantizer is read once per 64 tables instead of once per table (the
// one-kernel version was bound by L2 reads of the sub-quantizers: 160 KB per table).
// The projection px = R[c] . ((x - C[c]) - mu[c]) for TB tables of ONE (split, cluster) group per block: the tables
// arrive grouped by cluster (tab_order), so the 8*h*h bytes of R[c] are read once per TB tables instead of once per
// table (k_tables is bound by exactly that L2 traffic).  Same arithmetic as k_tables, table by table: one chain of fused
// multiply-adds over ascending k.  h <= 256, two-kernel path only (px_out).  The vector-unit form: used when h % 16 != 0
// (or CIS_TABLES_VALU=1); k_tables_group_mfma below is the default.
template <typename CT, int TB>
__global__ __launch_bounds__(256) void k_tables_group(const CT* __restrict__ X, const CT* __restrict__ Cs,
                                                      const double* __restrict__ Rt, const double* __restrict__ mus,
                                                      const TabDesc* __restrict__ tabs, const int* __restrict__ tab_order,
                                                      int n_tabs, int V, int h, int D, double* __restrict__ px_out,
                                                      const int64_t* __restrict__ d_totals /* null, or the plan totals: n_tabs is a bound */,
                                                      float* __restrict__ px32_out /* null, or a float32 copy of px (k_tiny_select's prefilter) */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (d_totals) {
        n_tabs = (int)d_totals[1];
        if ((int)blockIdx.x * TB >= n_tabs) return;
    }
    double* v = reinterpret_cast<double*>(smem);  // [TB][h]
    double* psum = v + TB * h;                     // [parts][TB][h]
    __shared__ int s_tab[TB];
    __shared__ int s_same;
    const int tid = threadIdx.x;
    const int first = blockIdx.x * TB;
    const int nt = (n_tabs - first < TB) ? (n_tabs - first) : TB;
    if (tid < TB) s_tab[tid] = tid < nt ? tab_order[first + tid] : -1;
    __syncthreads();
    const TabDesc td0 = tabs[s_tab[0]];
    if (tid == 0) {
        int same = 1;
        for (int t = 1; t < nt; ++t) {
            const TabDesc td = tabs[s_tab[t]];
            same &= (td.split == td0.split && td.cluster == td0.cluster);
        }
        s_same = same;
    }
    for (int e = tid; e < nt * h; e += 256) {
        const int t = e / h, k = e - t * h;
        const TabDesc td = tabs[s_tab[t]];
        const CT* x = X + (int64_t)td.q * D + td.split * h;
        const CT* Cc = Cs + ((int64_t)td.split * V + td.cluster) * h;
        const double* mu = mus + ((int64_t)td.split * V + td.cluster) * h;
        const CT res = x[k] - Cc[k];  // rounds in CT (float32 when both are float32), model.py:635
        v[t * h + k] = (double)res - mu[k];
    }
    __syncthreads();
    // one chain of fused multiply-adds per (table, output), k ascending (see k_tables): thread group g = tid / h takes the tables
    // t = g, g + parts, ...; sixteen elements of the thread's column of R in flight at a time
    const int parts = 256 / h;
    const int part = tid / h, i = tid - part * h;
    if (part < parts) {
        if (s_same) {
            const double* R = Rt + ((int64_t)td0.split * V + td0.cluster) * h * h;
            double acc[TB];
#pragma unroll
            for (int t = 0; t < TB; ++t) acc[t] = 0.0;
            for (int kb = 0; kb < h; kb += 16) {
                double rr[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) rr[u] = R[(int64_t)(kb + u < h ? kb + u : h - 1) * h + i];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    if (kb + u < h) {
#pragma unroll
                        for (int t = 0; t < TB; ++t)
                            if (t % parts == part) acc[t] = fma(rr[u], v[t * h + kb + u], acc[t]);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < TB; ++t)
                if (t % parts == part && t < nt) psum[t * h + i] = acc[t];
        } else {  // a block that straddles two groups: every table with its own R
            for (int t = part; t < nt; t += parts) {
                const TabDesc td = tabs[s_tab[t]];
                const double* R = Rt + ((int64_t)td.split * V + td.cluster) * h * h;
                double acc = 0.0;
                for (int k = 0; k < h; ++k) acc = fma(R[(int64_t)k * h + i], v[t * h + k], acc);
                psum[t * h + i] = acc;
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < nt * h; e += 256) {
        const int t = e / h, ii = e - t * h;
        const double acc = psum[t * h + ii];
        px_out[(int64_t)s_tab[t] * h + ii] = acc;
        if (px32_out) px32_out[(int64_t)s_tab[t] * h + ii] = (float)acc;
    }
}

// The grouped projection on the float64 matrix cores (round 4).  The VALU form above reads one broadcast LDS operand per fused
// multiply-add and waits for it (195 v_fmac_f64, 140 ds_read, 185 s_waitcnt in its listing): 1.7 ms for the 1.2 M tables of a
// V = 2048 batch, 7 % of the float64 rate.  v_mfma_f64_16x16x4_f64 takes ONE operand pair per lane for 1024 multiply-adds and is, per
// output element, exactly the chain of fused multiply-adds over ascending k that k_tables computes (tools/probes/mfma_f64_order.hip:
// 512000 results, none differs) -- so this kernel changes no bit.  A block = up to 16 tables of one (split, cluster) group: A = R
// (rows = outputs i, 16 per tile; loaded straight from global memory, 128 contiguous bytes per k), B = the tables' residuals v
// (columns = tables; staged in LDS with a pitch of h + 4), wave w owns the output tiles w, w + 4, ...  h % 16 == 0.
template <typename CT, int CH /* MFMA steps whose A operands are in flight together: 16 when h % 64 == 0, else 4 */>
__global__ __launch_bounds__(256) void k_tables_group_mfma(const CT* __restrict__ X, const CT* __restrict__ Cs,
                                                           const double* __restrict__ Rt, const double* __restrict__ mus,
                                                           const TabDesc* __restrict__ tabs, const int* __restrict__ tab_order,
                                                           int n_tabs, int V, int h, int D, double* __restrict__ px_out,
                                                           const int64_t* __restrict__ d_totals, float* __restrict__ px32_out) {
    typedef double f64x4_t __attribute__((ext_vector_type(4)));
    constexpr int TB = 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (d_totals) {
        n_tabs = (int)d_totals[1];
        if ((int)blockIdx.x * TB >= n_tabs) return;
    }
    const int pitch = h + 4;
    double* v = reinterpret_cast<double*>(smem);  // [TB][pitch]
    double* so = v + TB * pitch;                  // [TB][h + 2]: the results, so that a table's h outputs leave as one contiguous run
    const int opitch = h + 2;
    __shared__ int s_tab[TB];
    __shared__ TabDesc s_td[TB];
    __shared__ int s_first[TB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = blockIdx.x * TB;
    const int nt = (n_tabs - first < TB) ? (n_tabs - first) : TB;
    if (tid < TB) {
        const int tb = tab_order[first + (tid < nt ? tid : 0)];  // (columns past the block's tables: the first table again, masked below)
        s_tab[tid] = tid < nt ? tb : -1;
        s_td[tid] = tabs[tb];
    }
    __syncthreads();
    // s_first[t]: the first table of the block with table t's (split, cluster) -- a block that straddles groups runs one pass per group
    if (tid < TB) {
        int f = tid;
        for (int u = tid - 1; u >= 0; --u)
            if (s_td[u].split == s_td[tid].split && s_td[u].cluster == s_td[tid].cluster) f = u;
        s_first[tid] = tid < nt ? f : -1;
    }
    // residuals of the block's tables -> LDS; four elements per thread in flight (descriptors from LDS, loads unconditional)
    for (int e0 = tid; e0 < TB * h; e0 += 1024) {
        CT xv[4], cv[4];
        double mv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 256 * u < TB * h ? e0 + 256 * u : tid;
            const int t = e / h, k = e - t * h;
            const TabDesc td = s_td[t];
            xv[u] = X[(int64_t)td.q * D + td.split * h + k];
            cv[u] = Cs[((int64_t)td.split * V + td.cluster) * h + k];
            mv[u] = mus[((int64_t)td.split * V + td.cluster) * h + k];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + 256 * u;
            if (e < TB * h) {
                const int t = e / h, k = e - t * h;
                const CT res = xv[u] - cv[u];  // rounds in CT (float32 when both are float32), model.py:635
                v[t * pitch + k] = t < nt ? (double)res - mv[u] : 0.0;  // columns past the block's tables: zeros (not stored)
            }
        }
    }
    __syncthreads();
    const int t = lane & 15, kq = lane >> 4;
    for (int t0 = 0; t0 < nt; ++t0) {
        if (s_first[t0] != t0) continue;  // (uniform) one pass per (split, cluster) group present in the block: one as a rule
        const TabDesc tdg = s_td[t0];
        const double* R = Rt + ((int64_t)tdg.split * V + tdg.cluster) * h * h;
        const bool mine = t < nt && s_first[t] == t0;  // columns of other groups are computed along and not stored
        for (int it = wave; it < h / 16; it += 4) {
            f64x4_t acc = {0.0, 0.0, 0.0, 0.0};
            const double* Ra = R + (int64_t)kq * h + it * 16 + (lane & 15);  // A[row = i][k = 4 s + kq] = R[k][i]
            const double* vb = v + t * pitch + kq;                           // B[k = 4 s + kq][col = t] = v[t][k]
            for (int s0 = 0; s0 < h / 4; s0 += CH) {  // (h / 4) % CH == 0
                double ra[CH], rb[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) ra[u] = Ra[(int64_t)(s0 + u) * 4 * h];
#pragma unroll
                for (int u = 0; u < CH; ++u) rb[u] = vb[4 * (s0 + u)];
#pragma unroll
                for (int u = 0; u < CH; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[u], rb[u], acc, 0, 0, 0);
            }
            if (mine) {
                double* o = so + t * opitch + it * 16 + kq;  // result r: output i = it * 16 + kq + 4 r, table t
#pragma unroll
                for (int r = 0; r < 4; ++r) o[4 * r] = acc[r];
            }
        }
    }
    // (stored straight from the accumulators, every lane wrote four lone 8-byte values 32 bytes apart into sixteen different tables:
    // partial-sector writes, 1.2 M tables x 64 of them per V = 2048 batch)
    __syncthreads();
    for (int e = tid; e < nt * h; e += 256) {
        const int tt = e / h, i = e - tt * h;
        const double a = so[tt * opitch + i];
        px_out[(int64_t)s_tab[tt] * h + i] = a;
        if (px32_out) px32_out[(int64_t)s_tab[tt] * h + i] = (float)a;
    }
}

template <typename CT>
static void launch_tables(int64_t n_tabs, size_t tab_lds, hipStream_t st, const CT* X, const CT* Cs, const double* Rt,
                          const double* mus, const double* subs, const TabDesc* tabs, const int* tab_order, int V, int h, int w,
                          int nf, int K, int D, double* T, PwProg prog_w, double* px_out, const int64_t* d_totals = nullptr,
                          float* px32_out = nullptr) {
    constexpr int TB = 8;
    if (px_out && h <= 256 && h % 16 == 0 && !getenv("CIS_TABLES_UNGROUPED") && !getenv("CIS_TABLES_VALU")) {
        // the grouped projection on the float64 matrix cores (16 tables per block); CIS_TABLES_VALU=1: the vector form below
        const size_t lds = (size_t)16 * (h + 4 + h + 2) * sizeof(double);
        if (h % 64 == 0)
            hipLaunchKernelGGL((k_tables_group_mfma<CT, 16>), dim3((unsigned)ceil_div(n_tabs, 16)), dim3(256), lds, st, X, Cs, Rt, mus, tabs,
                               tab_order, (int)n_tabs, V, h, D, px_out, d_totals, px32_out);
        else
            hipLaunchKernelGGL((k_tables_group_mfma<CT, 4>), dim3((unsigned)ceil_div(n_tabs, 16)), dim3(256), lds, st, X, Cs, Rt, mus, tabs,
                               tab_order, (int)n_tabs, V, h, D, px_out, d_totals, px32_out);
    } else if (px_out && h <= 256 && 256 / h >= 1 && !getenv("CIS_TABLES_UNGROUPED")) {
        const size_t lds = (size_t)(TB * h + TB * h) * sizeof(double);
        hipLaunchKernelGGL((k_tables_group<CT, TB>), dim3((unsigned)ceil_div(n_tabs, TB)), dim3(256), lds, st, X, Cs, Rt, mus, tabs,
                           tab_order, (int)n_tabs, V, h, D, px_out, d_totals, px32_out);
    } else {
        hipLaunchKernelGGL(k_tables<CT>, dim3((unsigned)n_tabs), dim3(256), tab_lds, st, X, Cs, Rt, mus, subs, tabs, V, h, w, nf, K, D, T,
                           prog_w, px_out, (const int*)nullptr, 0);
    }
}

// TPB tables per block: 64 for batches (the sub-centroid a thread keeps in registers serves 64 tables), 8 when the batch has few
// tables -- a single exhaustive query has 32: two blocks per (sub-quantizer, split) then walked 16 of them one after the other, 19 us.
template <int W, int TPB = 64>
__global__ __launch_bounds__(256) void k_tables_from_px(const double* __restrict__ px /* [ntab][h] */,
                                                        TabDesc* __restrict__ tabs, int n_tabs,
                                                        const double* __restrict__ subs, int h, int nf, int K,
                                                        double* __restrict__ T /* [ntab][nf][K] */,
                                                        float* __restrict__ T32 /* [ntab][nf][K] float32 copy for the scan */,
                                                        const int64_t* __restrict__ d_totals /* null, or the plan totals: n_tabs is a bound */) {
    __shared__ double sf[TPB][W];
    __shared__ int ssplit[TPB];
    const int j = blockIdx.y, z = blockIdx.z, k = threadIdx.x;
    const int t0 = blockIdx.x * TPB;
    if (d_totals) {
        n_tabs = (int)d_totals[1];
        if (t0 >= n_tabs) return;
    }
    const int nt = (n_tabs - t0 < TPB) ? (n_tabs - t0) : TPB;
    for (int e = threadIdx.x; e < nt * W; e += 256) {
        const int t = e / W, i = e - t * W;
        sf[t][i] = px[(int64_t)(t0 + t) * h + j * W + i];
    }
    if (threadIdx.x < nt) ssplit[threadIdx.x] = tabs[t0 + threadIdx.x].split;
    __syncthreads();
    const bool on = k < K;  // all lanes stay in the loop: the per-table maximum below is a full-wave reduction
    double sc[W];
    const double* src = subs + ((int64_t)(z * nf + j) * K + (on ? k : 0)) * W;
#pragma unroll
    for (int i = 0; i < W; ++i) sc[i] = src[i];
    for (int t = 0; t < nt; ++t) {
        if (ssplit[t] != z) continue;
        const double* f = sf[t];
        auto elem = [&](int i) -> double { const double df = f[i] - sc[i]; return df * df; };
        const double v = pw_leaf<double>(elem, 0, W);
        const float v32 = (float)v;
        if (on) {
            // NON-TEMPORAL: the float64 copy (2/3 of the bytes this kernel writes) is read sparsely, by the merge, much later; written with
            // the default policy it pushed the float32 copy -- which the scan stages next -- and the codes out of L2 / Infinity Cache.
            // Round 6, same box, median of two runs each: C4 21.3 -> 21.8 M queries/s (scan 0.233 -> 0.230 ms), C2 19.7 -> 21.1 M
            // (scan 0.157 -> 0.152, merge 0.115 -> 0.105 ms).
            __builtin_nontemporal_store(v, &T[((int64_t)(t0 + t) * nf + j) * K + k]);
            if (T32) T32[((int64_t)(t0 + t) * nf + j) * K + k] = v32;  // (null: the scans convert the float64 entries themselves, see tab_f4; stored non-temporal too: no gain)
        }
        // largest float32 entry of the table (entries are >= 0: the bit patterns order like the values), for the
        // fixed-point scan's scale (lopq_scan3.hip); TabDesc::pad was zeroed when the descriptor was written
        uint32_t b = on ? __float_as_uint(v32) : 0u, dummy = 0u;
        wave_minmax_step<1>(dummy, b); wave_minmax_step<2>(dummy, b); wave_minmax_step<4>(dummy, b);
        wave_minmax_step<8>(dummy, b); wave_minmax_step<16>(dummy, b); wave_minmax_step<32>(dummy, b);
        if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned int*>(&tabs[t0 + t].pad), b);
    }
}

// float32 copy of the tables for the configurations that do not go through k_tables_from_px
__global__ void k_tables_f32(const double* __restrict__ T, int64_t n, int nf, int K, float* __restrict__ T32, TabDesc* __restrict__ tabs) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // index into T: (tab, j, k)
    if (e >= n) return;
    const float v = (float)T[e];
    T32[e] = v;
    atomicMax(reinterpret_cast<unsigned int*>(&tabs[e / ((int64_t)nf * K)].pad), __float_as_uint(v));  // see k_tables_from_px
}

// ================================================================================================
// block-wide bitonic sort of N (power of two) keys (a, b) with an optional payload, in LDS
// ================================================================================================
template <int N, int NT, bool PAY>
__device__ __forceinline__ void block_bitonic(uint64_t* ka, uint64_t* kb, int64_t* pay) {
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
// kernel: ADC scan + block top-k   (lopq/lopq/search.py:166-175, :210-215)
// ================================================================================================
// One 256-thread block per work item (a chunk of one cell for one query).  The two half tables
// sit in LDS as float64 [M][K]; every candidate's distance is ((T0[f0] + T1[f1]) + ...) in
// float64, left to right, exactly the reference's sum().  Candidates whose key (dist, pos) beats
// the running limit-th best are appended to an LDS buffer; when the buffer could overflow it is
// sorted and cut back to `limit` entries.
template <int M>
__device__ __forceinline__ double adc_one(const uint8_t* __restrict__ codes, int64_t p, const double* __restrict__ T, int K) {
    double d;
    if constexpr (M == 4) {
        const uint32_t c = *reinterpret_cast<const uint32_t*>(codes + p * 4);
        d = T[c & 255];
        d = d + T[K + ((c >> 8) & 255)];
        d = d + T[2 * K + ((c >> 16) & 255)];
        d = d + T[3 * K + (c >> 24)];
    } else if constexpr (M == 8) {
        const uint2 c = *reinterpret_cast<const uint2*>(codes + p * 8);
        d = T[c.x & 255];
        d = d + T[K + ((c.x >> 8) & 255)];
        d = d + T[2 * K + ((c.x >> 16) & 255)];
        d = d + T[3 * K + (c.x >> 24)];
        d = d + T[4 * K + (c.y & 255)];
        d = d + T[5 * K + ((c.y >> 8) & 255)];
        d = d + T[6 * K + ((c.y >> 16) & 255)];
        d = d + T[7 * K + (c.y >> 24)];
    } else if constexpr (M == 16) {
        const uint4 c = *reinterpret_cast<const uint4*>(codes + p * 16);
        const uint32_t cw[4] = {c.x, c.y, c.z, c.w};
        d = T[cw[0] & 255];
        d = d + T[K + ((cw[0] >> 8) & 255)];
        d = d + T[2 * K + ((cw[0] >> 16) & 255)];
        d = d + T[3 * K + (cw[0] >> 24)];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            d = d + T[(4 * q + 0) * K + (cw[q] & 255)];
            d = d + T[(4 * q + 1) * K + ((cw[q] >> 8) & 255)];
            d = d + T[(4 * q + 2) * K + ((cw[q] >> 16) & 255)];
            d = d + T[(4 * q + 3) * K + (cw[q] >> 24)];
        }
    } else {  // generic: M passed at run time through K's sibling argument (see caller)
        d = 0.0;
    }
    return d;
}

static __device__ __forceinline__ double adc_generic(const uint8_t* __restrict__ codes, int64_t p, int M,
                                                     const double* __restrict__ T, int K) {
    const uint8_t* c = codes + p * M;
    double d = T[c[0]];
    for (int j = 1; j < M; ++j) d = d + T[j * K + c[j]];
    return d;
}

template <int M /* 0 = generic */, int CAP, int U>
__global__ __launch_bounds__(256) void k_adc_scan(const WorkItem* __restrict__ items, const double* __restrict__ T,
                                                  const uint8_t* __restrict__ codes, const int64_t* __restrict__ ids,
                                                  int Mrt, int K, int limit, int S, const int* __restrict__ item_flag,
                                                  cis_hit* __restrict__ item_hits, int* __restrict__ item_n) {
    if (item_flag && !item_flag[blockIdx.x]) return;  // only redo what the fast kernel gave up on
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* ka = reinterpret_cast<uint64_t*>(smem);  // [CAP] dist bits
    uint64_t* kb = ka + CAP;                           // [CAP] position inside the chunk
    double* tab = reinterpret_cast<double*>(kb + CAP); // [M][K]
    int& s_cnt = *reinterpret_cast<int*>(tab + Mrt * K);  // all LDS in the dynamic region (16-B aligned carve)
    const int tid = threadIdx.x;
    const WorkItem it = items[blockIdx.x];
    const int nf = Mrt / 2;
    {
        const double* t0 = T + (int64_t)it.tab0 * nf * K;
        const double* t1 = T + (int64_t)it.tab1 * nf * K;
        for (int e = tid; e < nf * K; e += 256) {
            tab[e] = t0[e];
            tab[nf * K + e] = t1[e];
        }
    }
    if (tid == 0) s_cnt = 0;
    uint64_t tau_a = ~0ull, tau_b = ~0ull;  // running limit-th best key (everything passes at first)
    __syncthreads();
    const int len = it.len;
    for (int base = 0; base < len; base += 256 * U) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = base + u * 256 + tid;
            if (p < len) {
                double d;
                if constexpr (M == 0) d = adc_generic(codes, it.start + p, Mrt, tab, K);
                else d = adc_one<M>(codes, it.start + p, tab, K);
                const uint64_t a = f2bits(d);
                if (a < tau_a || (a == tau_a && (uint64_t)p < tau_b)) {
                    const int slot = atomicAdd(&s_cnt, 1);
                    ka[slot] = a;  // slot < CAP is guaranteed by the compaction rule below
                    kb[slot] = (uint64_t)p;
                }
            }
        }
        __syncthreads();
        const int cnt = s_cnt;
        __syncthreads();  // everybody has read the count before the next iteration's appends change it
        if (cnt > CAP - 256 * U && base + 256 * U < len) {
            for (int e = cnt + tid; e < CAP; e += 256) { ka[e] = ~0ull; kb[e] = ~0ull; }
            __syncthreads();
            block_bitonic<CAP, 256, false>(ka, kb, nullptr);
            tau_a = ka[limit - 1];
            tau_b = kb[limit - 1];
            __syncthreads();
            if (tid == 0) s_cnt = limit;
            __syncthreads();
        }
    }
    int cnt = s_cnt;
    if (cnt > limit) {
        for (int e = cnt + tid; e < CAP; e += 256) { ka[e] = ~0ull; kb[e] = ~0ull; }
        __syncthreads();
        block_bitonic<CAP, 256, false>(ka, kb, nullptr);
        cnt = limit;
    }
    cis_hit* out = item_hits + (int64_t)blockIdx.x * S;
    for (int e = tid; e < cnt; e += 256) {
        cis_hit hh;
        hh.dist = __longlong_as_double((long long)ka[e]);
        hh.visit_rank = (uint32_t)it.rank;
        hh.pos = (uint32_t)(it.pos0 + (int)kb[e]);
        hh.id = ids[it.start + (int64_t)kb[e]];
        hh.cell = it.cell; hh.reserved = 0;
        out[e] = hh;
    }
    if (tid == 0) item_n[blockIdx.x] = cnt;
}


// ================================================================================================
// kernel: ADC scan v2 -- float32 prefilter in LDS, barrier-free wave-private top-k on exact keys
// ================================================================================================
// Why a second kernel: v1 above is exact by construction (float64 tables and sums) but is bound by
// LDS bank conflicts (32 lanes gathering from one 256-entry table collide ~3.5-way), by float64
// adds and by workgroup barriers every iteration (rocprof: 59 % of wave cycles waiting).  v2 returns
// bit-identical results with a different division of labour:
//
//  * the two half tables sit in LDS as float32 in ENTRY-major order tab[k][j] (j fastest).  Bank =
//    (k*M + j) mod 32, so sub-quantizer j owns the 32/M banks {j, j+M, ...}.  Lane l walks the
//    sub-quantizers in a rotated order (step t -> table rot(l, t)), so at every step the 32 lanes of
//    an LDS lane group are spread evenly over all M tables: 32/M lanes into 32/M banks instead of
//    32 lanes into 32 banks;
//  * each candidate gets a float32 sum d32 (any order).  |d32 - d64| <= eps*d64 with
//    eps = 2*M*2^-24 (entries are >= 0: one rounding per converted entry, M-1 per add).  The hot
//    loop only REJECTS candidates with d32 > bound*(1+3eps), where `bound` is an exact float64
//    distance that at least `limit` already-seen candidates do not exceed; a rejected candidate is
//    therefore strictly worse than `limit` others and cannot be in the exact top-`limit`;
//  * everything that is not rejected is appended (position only) to a wave-private LDS region -- no
//    workgroup barrier in the loop.  When a region fills up its wave re-scores the new entries
//    EXACTLY (float64 table entries from global memory, summed left to right as search.py:173),
//    selects its own limit-th and ceil(limit/4)-th smallest exact keys (dist, pos) with register
//    bitonic sorts, publishes them, and keeps only entries that are within its own top-`limit` and
//    not above the block bound  min( max_w wt[w], min_w wl[w] )  built from the published values
//    (each is a distance that >= `limit` seen candidates do not exceed).  Exact ties -- thousands of
//    identical codes are common in real indexes -- are resolved on (dist, pos), never on float32;
//  * at the end every wave holds <= `limit` exact hits; they are written as cis_hit and the
//    per-query merge ranks them by (dist, visit_rank, pos).

#ifdef CIS_SCAN_COUNTERS
__device__ unsigned long long g_scan_ctr[16];  // compactions, rescored entries, exact-cut, second sorts, appended
#define CIS_CTR(i, v) do { if ((threadIdx.x & 63) == 0) atomicAdd(&g_scan_ctr[i], (unsigned long long)(v)); } while (0)
#define CIS_CLK() ((long long)__builtin_amdgcn_s_memtime())
#else
#define CIS_CTR(i, v) do { } while (0)
#define CIS_CLK() 0ll
#endif

struct ScanShared {  // one per query handled by the workgroup
    uint64_t wt[8];  // per wave: exact dist bits that >= ceil(limit/NW) of its candidates do not exceed
    uint64_t wl[8];  // per wave: exact dist bits that >= limit of its candidates do not exceed
    float bound_f;   // block bound rounded UP to float32 for the hot loop (refreshed at every compaction;
                     // a lost concurrent update only leaves it looser for a while)
    int pad0;
    int wcnt[8];     // survivors per wave at the end
    uint64_t ext;    // bound published by workgroups that scanned OTHER cells for the same query (qbound[q] at start)
};


static __device__ __forceinline__ float block_bound_f32(const ScanShared* sh) { return lds_ld(&sh->bound_f); }

// exact float64 distance of one candidate: table entries from global memory, summed left to right
static __device__ __forceinline__ double adc64_global(const uint8_t* __restrict__ codes, int64_t p, int M, int K,
                                                      const double* __restrict__ t0, const double* __restrict__ t1) {
    const uint8_t* c = codes + p * M;
    const int nf = M / 2;
    double d = t0[c[0]];
    for (int j = 1; j < nf; ++j) d = d + t0[j * K + c[j]];
    for (int j = 0; j < nf; ++j) d = d + t1[j * K + c[nf + j]];
    return d;
}


// Region entries during the scan are (float32 distance << 32 | candidate position): ordered by (d32, pos) as
// plain integers, appended with one ds_write_b64.  Two compactions work on them:
//  * wave_compact_approx (in the loop): float32 only, nothing leaves the CU.  It finds a distance v that at least L
//    entries do not exceed (ballot bisection that stops as soon as the count is within [L, L+W]), keeps everything
//    up to v*(1+3eps) -- an entry above that is strictly worse, in exact arithmetic, than the L entries below v --
//    and publishes the bounds v*(1+2eps) >= the exact distances of those L (resp. ceil(L/NW)) entries.
//  * wave_compact_exact (fallback when ties make the float32 cut keep too much, and once at the end): fetches the
//    codes again, re-scores every entry in float64 (table entries summed left to right as search.py:173), cuts to
//    the exact top-L by (dist, pos) and resolves exact ties by region order.
// Region entries are always in increasing candidate position (appends are, and the compactions are stable), so
// among exactly equal distances "first in the region" == "smallest pos".  Wave-synchronous: no s_barrier inside.
template <int NR, int NW>
__device__ __forceinline__ int wave_compact_approx(uint64_t* rk, int cnt, int L, int Lw, int cap, float margin, double infl,
                                                   ScanShared* sh, int w) {
    const int lane = threadIdx.x & 63;
    CIS_CTR(0, 1);
    uint32_t hi[NR], pp[NR];
    bool keep[NR];
    uint32_t mn = 0xffffffffu, mx = 0u;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int e = r * 64 + lane;
        keep[r] = e < cnt;
        const uint64_t k = keep[r] ? rk[e] : ~0ull;
        hi[r] = (uint32_t)(k >> 32);
        pp[r] = (uint32_t)k;
        mn = (keep[r] && hi[r] < mn) ? hi[r] : mn;
        mx = (keep[r] && hi[r] > mx) ? hi[r] : mx;
    }
    wave_minmax_all(mn, mx);
    // (1) v2 with #{d32 <= v2} in [Lw, Lw + W2] -> this wave's share of the block bound
    // (the bracket is empty when the wave holds fewer than Lw entries: no probe, no bound)
    const int W2 = Lw >= 16 ? (Lw >> 3) : 1;
    const uint32_t v2 = wave_bisect_window<NR>(keep, hi, cnt >= Lw ? mn : mx, mx, Lw, W2);
    const uint64_t boundW = cnt >= Lw ? (uint64_t)__double_as_longlong((double)__uint_as_float(v2) * infl) : 0x7ff0000000000000ull;
    if (lane == 0) {
        if (boundW < lds_ld(&sh->wt[w])) lds_st(&sh->wt[w], boundW);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    float bf = __double2float_ru(__longlong_as_double((long long)block_bound<NW>(sh)));
    uint32_t cut = __float_as_uint(bf * margin);  // the hot loop's test
    int W = cap - L;
    W = W > 24 ? 24 : (W < 0 ? 0 : W);
    if (wave_count_le<NR>(keep, hi, cut) > L + W) {
        // (2) the block bound does not thin this wave out (the other waves lag, the good candidates sit in this
        // wave's stripes, or many distances are equal): cut to the wave's own top L.
        // v with #{d32 <= v} in [L, L+W], or the exact L-th smallest when ties prevent that
        const uint32_t v = wave_bisect_window<NR>(keep, hi, mn, mx, L, W);
        const uint32_t vm = __float_as_uint(__double2float_ru((double)__uint_as_float(v) * (double)margin));
        if (wave_count_le<NR>(keep, hi, vm) > cap) return -1;  // a crowd of (nearly) equal distances, e.g. duplicate codes: resolve exactly
        const uint64_t boundL = (uint64_t)__double_as_longlong((double)__uint_as_float(v) * infl);
        if (lane == 0) {
            if (boundL < lds_ld(&sh->wl[w])) lds_st(&sh->wl[w], boundL);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        bf = __double2float_ru(__longlong_as_double((long long)block_bound<NW>(sh)));
        const uint32_t thr = __float_as_uint(bf * margin);
        cut = vm < thr ? vm : thr;
    }
    if (lane == 0) {
        if (bf < lds_ld(&sh->bound_f)) lds_st(&sh->bound_f, bf);
    }
    return wave_stable_keep<NR>([&](int r) { return keep[r] && hi[r] <= cut; },
                                [&](int r, int idx) { rk[idx] = ((uint64_t)hi[r] << 32) | pp[r]; });
}

// FINAL: leaves exact float64 keys in rk and positions in rp (the output format); otherwise the survivors go back
// to the (float32 rounded up, position) form.  Returns the new entry count (<= L).
template <int M, int NR, int NW, bool FINAL>
__device__ __forceinline__ int wave_compact_exact(uint64_t* rk, uint32_t* rp, int cnt, int L, int Lw,
                                                  ScanShared* sh, int w, const uint8_t* __restrict__ codes, int64_t start,
                                                  int K, const double* __restrict__ t0, const double* __restrict__ t1,
                                                  uint32_t& dup_pos) {
    const int lane = threadIdx.x & 63;
    CIS_CTR(1, 1);
    uint32_t hi[NR], lo[NR], pp[NR];
    bool keep[NR];
    uint32_t mn = 0xffffffffu, mx = 0u;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int e = r * 64 + lane;
        keep[r] = e < cnt;
        pp[r] = keep[r] ? (uint32_t)rk[e] : 0xffffffffu;
        hi[r] = 0xffffffffu;
        lo[r] = 0xffffffffu;
    }
    {
        // idle lanes of a row fetch candidate 0; rows past the end are skipped (wave-uniform)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (r * 64 >= cnt) break;
            const CodeWords<M> cw = load_code<M>(codes, start + (keep[r] ? pp[r] : 0u));
            const uint64_t k = keep[r] ? (uint64_t)__double_as_longlong(adc64_words<M>(cw.w, K, t0, t1)) : ~0ull;
            hi[r] = (uint32_t)(k >> 32);
            lo[r] = (uint32_t)k;
            mn = (keep[r] && hi[r] < mn) ? hi[r] : mn;
            mx = (keep[r] && hi[r] > mx) ? hi[r] : mx;
        }
    }
    wave_minmax_all(mn, mx);
    uint32_t vhiL;
    uint64_t boundL;
    wave_exact_cut<NR>(hi, lo, keep, [&](int r) { return pp[r]; }, mn, mx, cnt, L, vhiL, boundL, dup_pos);
    const uint64_t boundW = (cnt >= Lw) ? hi_to_bound(wave_kth_bisect<NR>(hi, keep, mn, vhiL, Lw)) : 0x7ff0000000000000ull;
    if (lane == 0) {
        if (boundW < lds_ld(&sh->wt[w])) lds_st(&sh->wt[w], boundW);
        if (boundL < lds_ld(&sh->wl[w])) lds_st(&sh->wl[w], boundL);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    const uint64_t bound = block_bound<NW>(sh);
    if (lane == 0) {
        const float bf = __double2float_ru(__longlong_as_double((long long)bound));
        if (bf < lds_ld(&sh->bound_f)) lds_st(&sh->bound_f, bf);
    }
    if constexpr (NR < 16) {
        return wave_stable_keep<NR>([&](int r) { return keep[r] && (((uint64_t)hi[r] << 32) | lo[r]) <= bound; }, [&](int r, int idx) {
            const uint64_t k = ((uint64_t)hi[r] << 32) | lo[r];
            if constexpr (FINAL) {
                rk[idx] = k;
                rp[idx] = pp[r];
            } else {
                rk[idx] = ((uint64_t)__float_as_uint(__double2float_ru(__longlong_as_double((long long)k))) << 32) | pp[r];
            }
        });
    } else {
        // wave_stable_keep spelled out: through the helper the NR = 16 instantiations spill three times the scalars and the 8192-query
        // batch at limit 500 takes 3.03 ms instead of 1.80 (profiles/scan_cut_ab.txt)
        int ncnt = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const uint64_t k = ((uint64_t)hi[r] << 32) | lo[r];
            const bool kp = keep[r] && (k <= bound);
            const unsigned long long m = __ballot(kp);
            const int idx = ncnt + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
            if (kp) {
                if constexpr (FINAL) {
                    rk[idx] = k;
                    rp[idx] = pp[r];
                } else {
                    rk[idx] = ((uint64_t)__float_as_uint(__double2float_ru(__longlong_as_double((long long)k))) << 32) | pp[r];
                }
            }
            ncnt += __popcll(m);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        return ncnt;
    }
}

// Drop (float32 distance, position) entries above the block bound, with the hot loop's test.  Stable.
template <int NR, int NW>
__device__ __forceinline__ int wave_filter_approx(uint64_t* rk, int cnt, float margin, const ScanShared* sh) {
    const int lane = threadIdx.x & 63;
    const uint64_t bound = block_bound<NW>(sh);
    const uint32_t thr = __float_as_uint(__double2float_ru(__longlong_as_double((long long)bound)) * margin);
    uint64_t k[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int e = r * 64 + lane;
        k[r] = e < cnt ? rk[e] : ~0ull;
    }
    return wave_stable_keep<NR>([&](int r) { return (r * 64 + lane < cnt) && ((uint32_t)(k[r] >> 32) <= thr); },
                                [&](int r, int idx) { rk[idx] = k[r]; });
}


// float32 ADC sums of one candidate for G queries at once: the LDS table interleaves the queries,
// tab[k][j][g], so ONE ds_read (b32 for G=1, b64 for G=2) serves all G queries of the workgroup.
// adc32_sh: log2(M * G * 4 bytes), one k-row of the table; the addresses are gather_addr's (scan_common.h): one instruction per
// entry, except at M = 16 with four queries -- rows of 256 bytes -- which keeps the two-instruction form.
template <int M, int G>
static constexpr int adc32_sh() { return ((M == 4) ? 4 : (M == 8 ? 5 : 6)) + (G == 4 ? 2 : (G == 2 ? 1 : 0)); }
template <int M, int G>
using Adc32Consts = GatherConsts<M, adc32_sh<M, G>()>;
template <int M, int G>
__device__ __forceinline__ Adc32Consts<M, G> adc32_consts(const RotConsts<M>& rc, const char* tab) {
    return make_gather<M, adc32_sh<M, G>()>(rc, tab, G == 4 ? 2 : (G == 2 ? 1 : 0));
}

// a candidate's M table reads, the addresses ahead of the reads (the hazard of gather_addr) in groups of at most eight; at M = 16 in
// groups of four: sixteen addresses ahead of the first read spilled in the one-query forms
template <int M, typename VT, typename GC>
__device__ __forceinline__ void adc32_gather(const GC& gc, const uint32_t (&D)[(M + 3) / 4], VT (&f)[M]) {
    constexpr int GRP = M == 16 ? 4 : M;
#pragma unroll
    for (int t0 = 0; t0 < M; t0 += GRP) {
        uint32_t a[GRP];
#pragma unroll
        for (int i = 0; i < GRP; ++i) a[i] = gather_addr(gc, D, t0 + i);
#pragma unroll
        for (int i = 0; i < GRP; ++i) f[t0 + i] = gather_ld<VT>(a[i]);
    }
}

template <int M, int G>
__device__ __forceinline__ void adc32g(const CodeWords<M>& c, const RotConsts<M>& rc, const Adc32Consts<M, G>& gc, float (&out)[G]) {
    uint32_t D[(M + 3) / 4];
    rot_words<M>(c, rc, D);
    if constexpr (G == 1) {
        float f[M];
        adc32_gather<M>(gc, D, f);
#pragma unroll
        for (int st = 1; st < M; st <<= 1)
#pragma unroll
            for (int t = 0; t < M; t += 2 * st) f[t] = f[t] + f[t + st];
        out[0] = f[0];
    } else {
        // the two queries' entries sit side by side: one ds_read_b64 per table entry, one packed add per tree node
        f32x2_t f[M];
        adc32_gather<M>(gc, D, f);
#pragma unroll
        for (int st = 1; st < M; st <<= 1)
#pragma unroll
            for (int t = 0; t < M; t += 2 * st) f[t] = f[t] + f[t + st];
        out[0] = f[0][0];
        out[1] = f[0][1];
    }
}

// adc32g for G = 2 or 4 queries in two halves, so that the table reads of the NEXT candidate row can be issued before
// the adds of the current one (the LDS pipe and the VALU then work at the same time inside one wave).  The G queries'
// entries sit side by side: one ds_read_b64 / ds_read_b128 per table entry, packed adds per tree node.
typedef float f32x4_t __attribute__((ext_vector_type(4)));
template <int G> struct AdcVec;
template <> struct AdcVec<2> { typedef f32x2_t type; };
template <> struct AdcVec<4> { typedef f32x4_t type; };

template <int M, int G>
__device__ __forceinline__ void adc32_issue(const CodeWords<M>& c, const RotConsts<M>& rc, const Adc32Consts<M, G>& gc,
                                            typename AdcVec<G>::type (&f)[M]) {
    typedef typename AdcVec<G>::type VT;
    uint32_t D[(M + 3) / 4];
    rot_words<M>(c, rc, D);
    adc32_gather<M>(gc, D, f);
}

template <int M, int G>
__device__ __forceinline__ void adc32_reduce(typename AdcVec<G>::type (&f)[M], float (&out)[G]) {
#pragma unroll
    for (int st = 1; st < M; st <<= 1)
#pragma unroll
        for (int t = 0; t < M; t += 2 * st) f[t] = f[t] + f[t + st];
#pragma unroll
    for (int g = 0; g < G; ++g) out[g] = f[0][g];
}

// One workgroup (NW waves) scans one cell chunk for `ng` <= G queries that all visit it.
template <int M, int NR, int U, int G, int NW>
__device__ __forceinline__ void scan2_group(const WorkItem* __restrict__ items_all, const int (&item_idx)[G], int ng,
                                            const double* __restrict__ T, const float* __restrict__ T32,
                                            const uint8_t* __restrict__ codes,
                                            const int64_t* __restrict__ ids, int K, int L, int S, float margin,
                                            uint64_t* __restrict__ item_surv, int* __restrict__ item_n,
                                            unsigned long long* __restrict__ qbound, char* smem) {
    // region capacity: 8 entries short of the NR*64 keys a wave can hold in registers, so that the
    // G=2 / 4-wave layout (16 KB tables + 8 regions) stays under 40 KB and four workgroups share a CU
    constexpr int R = NR * 64 - 8;
    // item_idx[] is wave-uniform (the slot index went through readfirstlane): the work items are scalar loads and live in
    // scalar registers instead of 10 VGPRs each (they used to spill to scratch)
    // (field by field: a local array of the 48-byte structs was kept in scratch, 24 KB of stores per slot and workgroup)
    int it_tab0[G], it_tab1[G], it_q[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        it_tab0[g] = items_all[item_idx[g]].tab0;
        it_tab1[g] = items_all[item_idx[g]].tab1;
        it_q[g] = items_all[item_idx[g]].q;
    }
    const int it0_len = items_all[item_idx[0]].len;
    const int64_t it0_start = items_all[item_idx[0]].start;
    char* tab = smem;                                                              // [K][M][G] float32
    uint64_t* rk_all = reinterpret_cast<uint64_t*>(smem + (size_t)K * M * G * 4);  // [G][NW][R] (d32, pos) entries; exact keys at the end
    uint64_t* tr_all = rk_all + G * NW * R;                                        // [G][NW][64] scratch slots of the branch-free append
    ScanShared* sh = reinterpret_cast<ScanShared*>(tr_all + G * NW * 64);          // [G]
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int nf = M / 2;
    const long long clk_begin = CIS_CLK();
    long long clk_slow = 0, clk_comp = 0, clk_exact = 0, clk_final = 0;
    (void)clk_exact; (void)clk_final;
    int n_slow = 0, n_app = 0;
    (void)clk_begin; (void)clk_slow; (void)clk_comp; (void)n_slow; (void)n_app;
    const float INF = __int_as_float(0x7f800000);
    {
        // LDS tables from the float32 copies ([nf][K] per (query, half)): 16-byte loads (four consecutive k of one
        // sub-quantizer), all in flight together, then one ds_write per entry that carries both queries' values.
        float* tf = reinterpret_cast<float*>(tab);
        const int nvec = (nf * K) >> 2;  // K is a multiple of 4 for the supported shapes
        for (int e0 = 0; e0 < nvec; e0 += NW * 64) {
            const int e = e0 + tid;
            float4 v[G][2];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const bool on = (g < ng) && (e < nvec);  // an absent second query gets +inf tables: nothing ever passes
                const int eg = e < nvec ? e : 0;
                v[g][0] = tab_f4(T32, T, it_tab0[g], nf * K, eg);
                v[g][1] = tab_f4(T32, T, it_tab1[g], nf * K, eg);
                if (!on) { v[g][0] = make_float4(INF, INF, INF, INF); v[g][1] = v[g][0]; }
            }
            if (e < nvec) {
                const int j = (4 * e) / K, k0 = 4 * e - j * K;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        float* dst = tf + ((k0 + c) * M + s2 * nf + j) * G;
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            const float4 q = v[g][s2];
                            dst[g] = c == 0 ? q.x : (c == 1 ? q.y : (c == 2 ? q.z : q.w));
                        }
                    }
                }
            }
        }
        if (tid < 8 * G) {
            const int g = tid >> 3, i = tid & 7;
            sh[g].wt[i] = 0x7ff0000000000000ull; sh[g].wl[i] = 0x7ff0000000000000ull;
            sh[g].wcnt[i] = 0;
            if (i == 0) {
                // A distance that >= L candidates of this query in already scanned cells do not exceed: candidates
                // above it are strictly worse than L others, whichever cell they are in.  Cells of one query are
                // scanned by different workgroups at different times (the slot list is sorted by cell), so the
                // later ones start with a tight bound instead of +inf.  Only the amount of work depends on timing.
                int qg = it_q[0];  // g is a thread index here: select, do not index the register array
#pragma unroll
                for (int gg = 1; gg < G; ++gg) qg = (g == gg) ? it_q[gg] : qg;
                const unsigned long long e = (g < ng) ? __hip_atomic_load(&qbound[qg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                      : 0x7ff0000000000000ull;
                sh[g].ext = e;
                // an absent second query: negative bound, nothing ever passes (its tables are +inf as well)
                sh[g].bound_f = (g < ng) ? __double2float_ru(__longlong_as_double((long long)e)) : -1.0f;
            }
        }
    }
    __syncthreads();
    const long long clk_tab_end = CIS_CLK();
    (void)clk_tab_end;
    const RotConsts<M> rc = make_rot<M>(lane);
    const Adc32Consts<M, G> gc = adc32_consts<M, G>(rc, tab);
    const int Lw = (L + NW - 1) / NW;
    // wave-uniform by construction; tell the compiler so (scalar loop control, scalar tail test)
    const int len = __builtin_amdgcn_readfirstlane(it0_len);
    const int64_t start = ((int64_t)__builtin_amdgcn_readfirstlane((int)(it0_start >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)it0_start);
    const int nit = (len + 64 * U - 1) / (64 * U);
    int cnt[G];
    constexpr double EPS32 = 2.0 * M * 5.9604644775390625e-8;  // float32 sum vs exact: |d32 - d64| <= EPS32 * d64
    const double infl = 1.0 + 2.0 * EPS32;
    CodeWords<M> dup[G];  // per query: a code whose later copies cannot enter this wave's top-L any more
    bool has_dup[G];
    bool any_dup = false;
#pragma unroll
    for (int g = 0; g < G; ++g) { cnt[g] = 0; has_dup[g] = false; dup[g] = CodeWords<M>(); }
    // buffer descriptor over this chunk's codes, built from wave-uniform values only
    __amdgpu_buffer_rsrc_t rs;
    {
        const uint64_t cbase = (uint64_t)(uintptr_t)(codes + start * M);
        const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)cbase);
        const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(cbase >> 32));
        const int nbytes = __builtin_amdgcn_readfirstlane(len * M);
        rs = __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)(((uint64_t)bhi << 32) | blo), 0, nbytes, 0x00020000);
    }
    CodeWords<M> nxt[U];
    if (w < nit) {
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[u] = load_code_buf<M>(rs, w * 64 * U + u * 64 + lane);
    }
    for (int iter = w; iter < nit; iter += NW) {
        const int base = iter * 64 * U;
        CodeWords<M> cur[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        if (iter + NW < nit) {  // software prefetch: the next iteration's codes are in flight while this one computes
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = load_code_buf<M>(rs, (iter + NW) * 64 * U + u * 64 + lane);  // tail lanes are masked below
        }
        float d[U][G];
        if constexpr (G >= 2) {
            typename AdcVec<G>::type fbuf[2][M];
            adc32_issue<M, G>(cur[0], rc, gc, fbuf[0]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (u + 1 < U) adc32_issue<M, G>(cur[u + 1], rc, gc, fbuf[(u + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                adc32_reduce<M, G>(fbuf[u & 1], d[u]);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) adc32g<M, G>(cur[u], rc, gc, d[u]);
        }
        // Fast path: one compare + ballot per (candidate row, query), ONE branch if no mask is set.  Lanes past
        // the end of the chunk (last iteration only) get NaN distances, which never compare <=; the duplicate
        // exclusion is applied in the slow path only.
        if (base + 64 * U > len) {
            const float QNAN = __int_as_float(0x7fc00000);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int g = 0; g < G; ++g) d[u][g] = (base + u * 64 + lane < len) ? d[u][g] : QNAN;
        }
        unsigned long long pm[U][G];
        unsigned long long any = 0ull;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float thrm = block_bound_f32(&sh[g]) * margin;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pm[u][g] = __ballot(d[u][g] <= thrm);
                any |= pm[u][g];
            }
        }
        if (any_dup) {  // wave-uniform, rare: drop later copies of a code that already lost a tie-break (see wave_compact_exact)
            any = 0ull;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const unsigned long long dup_on = has_dup[g] ? ~0ull : 0ull;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    bool same = true;
#pragma unroll
                    for (int i = 0; i < (M + 3) / 4; ++i) same = same && (cur[u].w[i] == dup[g].w[i]);
                    pm[u][g] &= ~(__ballot(same) & dup_on);
                    any |= pm[u][g];
                }
            }
        }
        if (any == 0ull) continue;  // the usual case: nothing in these 64*U candidates beats a bound
        const long long clk_s0 = CIS_CLK();
        ++n_slow;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g >= ng) break;
            uint64_t* rk = rk_all + (g * NW + w) * R;
            uint64_t* tr = tr_all + (g * NW + w) * 64;
            uint32_t* rp = nullptr;  // positions array of the exact compaction's final form: not used inside the loop
            int ntot = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) ntot += __popcll(pm[u][g]);
            if (ntot == 0) continue;  // only the other query has candidates in this iteration
            if (cnt[g] + ntot <= R) {
                // The usual case: everything fits.  Straight-line code, no branch per row: every lane stores, the
                // lanes that did not pass into a scratch slot of their own.
                const int trash = (int)(tr - rk) + lane;
                int c = cnt[g];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const unsigned long long m = pm[u][g];
                    const int idx = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, c));
                    int sel;
                    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(sel) : "v"(trash), "v"(idx), "s"(m));
                    rk[sel] = ((uint64_t)__float_as_uint(d[u][g]) << 32) | (uint32_t)(base + u * 64 + lane);
                    c += __popcll(m);
                }
                cnt[g] = c;
                n_app += ntot;
                continue;
            }
            // Append row after row while they fit; when one does not, compact (ONE call site per query, whatever U
            // is), re-test the rows not yet appended against the new bound and go on.  After a compaction
            // cnt <= R - 64, so the next row always fits and the loop ends after at most U compactions.
            int u0 = 0;
            while (true) {
                bool full = false;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const unsigned long long m = pm[u][g];
                    if (u < u0 || full || m == 0ull) continue;
                    const int n = __popcll(m);
                    if (cnt[g] + n > R) {
                        full = true;
                        u0 = u;
                        continue;
                    }
                    const int idx = cnt[g] + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
                    if ((m >> lane) & 1ull) rk[idx] = ((uint64_t)__float_as_uint(d[u][g]) << 32) | (uint32_t)(base + u * 64 + lane);
                    cnt[g] += n;
                    n_app += n;
                    u0 = u + 1;
                }
                if (!full) break;
                const long long clk_c0 = CIS_CLK();
                int c2 = wave_compact_approx<NR, NW>(rk, cnt[g], L, Lw, R - 64, margin, infl, &sh[g], w);
                if (c2 < 0) {
                    uint32_t dp = 0xffffffffu;
                    const long long clk_e0 = CIS_CLK();
                    c2 = wave_compact_exact<M, NR, NW, false>(rk, rp, cnt[g], L, Lw, &sh[g], w, codes, start, K, T + (int64_t)it_tab0[g] * nf * K,
                                                                  T + (int64_t)it_tab1[g] * nf * K, dp);
                    clk_exact += CIS_CLK() - clk_e0;
                    dp = (uint32_t)__builtin_amdgcn_readfirstlane((int)dp);
                    if (dp != 0xffffffffu) {
                        dup[g] = load_code<M>(codes, start + (int64_t)dp);
                        has_dup[g] = true;
                        any_dup = true;
                    }
                }
                cnt[g] = c2;
                clk_comp += CIS_CLK() - clk_c0;
                const float thrm = block_bound_f32(&sh[g]) * margin;
                const unsigned long long dup_on = has_dup[g] ? ~0ull : 0ull;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    bool same = true;
#pragma unroll
                    for (int i = 0; i < (M + 3) / 4; ++i) same = same && (cur[u].w[i] == dup[g].w[i]);
                    pm[u][g] &= __ballot(d[u][g] <= thrm) & ~(__ballot(same) & dup_on);
                }
            }
        }
        clk_slow += CIS_CLK() - clk_s0;
    }
    const long long clk_loop_end = CIS_CLK();
    (void)clk_loop_end;
    // End of the chunk.  Every wave cuts its region in float32 and publishes its bounds; after the barrier the
    // block bound is (about) the L-th smallest distance of the whole chunk, so only ~L/NW entries per wave survive
    // it.  The survivors -- a superset of the chunk's exact top L -- leave as (float32 distance, position) pairs;
    // k_merge_survivors re-scores them in float64 and ranks the query's candidates exactly.
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g >= ng) break;
        uint64_t* rk = rk_all + (g * NW + w) * R;
        if (cnt[g] > 0) cnt[g] = wave_compact_approx<NR, NW>(rk, cnt[g], L, Lw, NR * 64, margin, infl, &sh[g], w);
    }
    clk_final = CIS_CLK() - clk_loop_end;
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g >= ng) break;
        uint64_t* rk = rk_all + (g * NW + w) * R;
        cnt[g] = wave_filter_approx<NR, NW>(rk, cnt[g], margin, &sh[g]);
        if (lane == 0) sh[g].wcnt[w] = cnt[g];
        if (tid == 0) {
            const uint64_t b = block_bound<NW>(&sh[g]);
            if (b < sh[g].ext) atomicMin(&qbound[it_q[g]], (unsigned long long)b);
        }
    }
    const long long clk_exact_end = CIS_CLK();
    (void)clk_exact_end;
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g >= ng) break;
        const uint64_t* rk = rk_all + (g * NW + w) * R;
        int off = 0, total = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int c = sh[g].wcnt[i];
            off += (i < w) ? c : 0;
            total += c;
        }
        uint64_t* out = item_surv + (int64_t)item_idx[g] * S + off;  // S = NW * R >= total
        for (int e = lane; e < cnt[g]; e += 64) out[e] = rk[e];
        if (tid == 0) item_n[item_idx[g]] = total;
    }
#ifdef CIS_SCAN_COUNTERS
    CIS_CTR(3, n_slow);
    CIS_CTR(8, clk_exact);
    CIS_CTR(10, clk_exact_end - clk_loop_end);
    CIS_CTR(11, clk_tab_end - clk_begin);
    CIS_CTR(9, clk_final);
    CIS_CTR(4, n_app);
    CIS_CTR(5, clk_comp);
    CIS_CTR(6, clk_slow - clk_comp);
    CIS_CTR(7, CIS_CLK() - clk_begin);
    CIS_CTR(2, clk_loop_end - clk_begin);
#endif
}

// Persistent launch: (blocks per CU) x 256 workgroups pull SLOTS from eight queues, one per XCD.  A
// slot holds up to G work items of the same coarse cell (slots come from the cell-sorted item list);
// queue x owns the x-th eighth of the slot list, so the workgroups resident on one XCD (workgroup b
// runs on XCD b % 8 -- observed dispatch rule, used for speed only) stream the same few cells through
// that XCD's private L2.  A workgroup whose own queue is empty steals from the others, which removes
// the tail caused by unequal cell sizes.
template <int M, int NR, int U, int G, int NW>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(NR == 16 ? 2 : (G == 4 ? 2 : ((M == 16 && G == 2) ? 3 : 4)), 4))) void k_adc_scan2(const WorkItem* __restrict__ items, const int* __restrict__ slots,
                                                       const int* __restrict__ n_slots_ptr, const double* __restrict__ T,
                                                       const float* __restrict__ T32,
                                                       const uint8_t* __restrict__ codes, const int64_t* __restrict__ ids,
                                                       int K, int L, int S, float margin,
                                                       int* __restrict__ queue_ctr /* [8], zeroed */,
                                                       uint64_t* __restrict__ item_surv, int* __restrict__ item_n,
                                                       unsigned long long* __restrict__ qbound /* [nq], +inf */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int R = NR * 64 - 8;
    int* s_next = reinterpret_cast<int*>(smem + (size_t)K * M * G * 4 + (size_t)G * NW * (R + 64) * 8 + G * sizeof(ScanShared));
    const int* qs = n_slots_ptr + 8;  // [9] queue starts, written by the slot builder
    const int home = blockIdx.x & 7;
    for (int a = 0; a < 8; ++a) {
        const int x = (home + a) & 7;
        const int qstart = qs[x];
        const int count = qs[x + 1] - qstart;
        while (true) {
            __syncthreads();  // previous slot fully written out; LDS may be reused
            if (threadIdx.x == 0) *s_next = atomicAdd(&queue_ctr[x], 1);
            __syncthreads();
            const int j = __builtin_amdgcn_readfirstlane(*s_next);  // wave-uniform: the slot and its work items stay in scalar registers
            if (j >= count) break;
            const int slot = qstart + j;
            int idx[G];
            int ng = 0;
            bool same = true;  // the items of a slot must cover the same chunk of the same cell; otherwise run them one by one
#pragma unroll
            for (int g = 0; g < G; ++g) {
                idx[g] = slots[slot * G + g];
                if (idx[g] >= 0) {
                    ng = g + 1;
                    same = same && items[idx[g]].start == items[idx[0]].start && items[idx[g]].len == items[idx[0]].len;
                } else {
                    idx[g] = idx[0];
                }
            }
            if constexpr (G >= 2) {
                if (!same) {
                    for (int g2 = 0; g2 < ng; ++g2) {
                        int oi[G];
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            oi[g] = idx[0];
#pragma unroll
                            for (int gg = 1; gg < G; ++gg)
                                if (gg == g2) oi[g] = idx[gg];
                        }
                        if (g2 > 0) __syncthreads();
                        scan2_group<M, NR, U, G, NW>(items, oi, 1, T, T32, codes, ids, K, L, S, margin, item_surv, item_n, qbound, smem);
                    }
                    continue;
                }
            }
            scan2_group<M, NR, U, G, NW>(items, idx, ng, T, T32, codes, ids, K, L, S, margin, item_surv, item_n, qbound, smem);
        }
    }
}

template <int CAPM>
__global__ __launch_bounds__(256) void k_merge_items(const cis_hit* __restrict__ item_hits, const int* __restrict__ item_n,
                                                     const int64_t* __restrict__ item_off, int limit, int S,
                                                     cis_hit* __restrict__ out_hits, int64_t* __restrict__ out_ids,
                                                     double* __restrict__ out_dists, int* __restrict__ out_n,
                                                     int32_t* __restrict__ out_cells, uint32_t* __restrict__ out_pos) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* ka = reinterpret_cast<uint64_t*>(smem);
    uint64_t* kb = ka + CAPM;
    int64_t* pay = reinterpret_cast<int64_t*>(kb + CAPM);
    int* s_n = reinterpret_cast<int*>(pay + CAPM);
    const int q = blockIdx.x;
    const int64_t a = item_off[q], b = item_off[q + 1];
    const int64_t o = (int64_t)q * limit;
    merge_lists<CAPM>(item_hits, item_n, a, (int)(b - a), (int64_t)S, S, limit, ka, kb, pay, s_n,
                      out_hits ? out_hits + o : nullptr, out_ids ? out_ids + o : nullptr,
                      out_dists ? out_dists + o : nullptr, out_n ? out_n + q : nullptr,
                      out_cells ? out_cells + o : nullptr, out_pos ? out_pos + o : nullptr);
}

// The float32-prefilter scan hands over, per work item, the (float32 distance << 32 | position) pairs that survived
// its bounds: a superset of the item's exact top `limit`.  One WAVE per query (four queries per workgroup, no
// workgroup barrier: a query is a chain of dependent global loads, so what counts is how many queries a CU has in
// flight) re-scores them exactly -- the code from the index, float64 table entries summed left to right as
// search.py:173, one candidate per lane -- and ranks them by (dist, visit_rank, pos) with a bitonic sort in LDS.

// ascending bitonic sort of N (power of two >= 64) 128-bit keys (ka, kb) by one wave
static __device__ __forceinline__ void wave_bitonic_lds(uint64_t* ka, uint64_t* kb, int N) {
    const int lane = threadIdx.x & 63;
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (N >> 1); t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i + j;
                const bool asc = ((i & k) == 0);
                const uint64_t a0 = ka[i], b0 = kb[i], a1 = ka[p], b1 = kb[p];
                const bool gt = (a0 > a1) || (a0 == a1 && b0 > b1);
                if (gt == asc) { ka[i] = a1; kb[i] = b1; ka[p] = a0; kb[p] = b0; }
            }
            wave_lds_sync();
        }
    }
}

// What the merge uses of a work item.  Every lane holds the fields of the query's list (lane & 3), and a lane that needs list l
// fetches them from lane l with a cross-lane read: four lists of wave-uniform fields in scalar registers, beside the kernel's
// nineteen operands, overflow the scalar file, and the scheduler then serialises the table loads to save registers.
struct MergeList {
    int64_t start;
    int tab0, tab1, rank, pos0, len, cell;
    float slack, ub;  // item_slack: (slack, scale)
};
static __device__ __forceinline__ int from_lane(int v, int l) { return __builtin_amdgcn_ds_bpermute(l << 2, v); }
static __device__ __forceinline__ float from_lane(float v, int l) { return __int_as_float(from_lane(__float_as_int(v), l)); }
static __device__ __forceinline__ int64_t from_lane(int64_t v, int l) {
    return (int64_t)(((uint64_t)(uint32_t)from_lane((int)((uint64_t)v >> 32), l) << 32) | (uint32_t)from_lane((int)v, l));
}

template <int CAPM, int MT /* 4, 8, 16, or 0 = any M */, int NEMAX /* 4 or 8: survivors per lane the fast path may hold */>
#ifndef CIS_MERGE_WPE
#define CIS_MERGE_WPE 4
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((MT == 16 || MT == 0) ? 2 : CIS_MERGE_WPE, 8)))
void k_merge_survivors(const uint64_t* __restrict__ surv /* [n_items][S] */,
                                                         const int* __restrict__ item_n, const int64_t* __restrict__ item_off,
                                                         const WorkItem* __restrict__ items, const double* __restrict__ T,
                                                         const uint8_t* __restrict__ codes, const int64_t* __restrict__ ids,
                                                         int nq, int M, int K, int limit, int S,
                                                         cis_hit* __restrict__ out_hits, int64_t* __restrict__ out_ids,
                                                         double* __restrict__ out_dists, int* __restrict__ out_n,
                                                         int32_t* __restrict__ out_cells, uint32_t* __restrict__ out_pos,
                                                         const PlanOut* __restrict__ plan, int32_t* __restrict__ out_visited,
                                                         const float* __restrict__ item_slack /* null: the survivors' high words are float32
                                                         distances within eps of the exact ones (k_adc_scan2); else they are upper bounds of
                                                         the exact distances, at most item_slack[item] above them (k_adc_scan3) */) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wq = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform: the query's offsets and counts are scalar loads
    const int q = blockIdx.x * 4 + wq;
    if (q >= nq) return;  // whole wave; nothing below synchronises across waves
    if (lane == 0 && out_visited) out_visited[q] = plan[q].visited;
    uint64_t* ka = reinterpret_cast<uint64_t*>(smem) + (size_t)wq * 2 * CAPM;
    uint64_t* kb = ka + CAPM;  // (visit_rank << 32) | position inside the cell
    const int64_t first = item_off[q];
    const int n_lists = (int)(item_off[q + 1] - first);
    const int nf = M / 2;
    int have = 0, l = 0, e = 0, total = 0;
    bool done_fast = false;
    // Everything the query needs to know about its first four lists is read in one round trip behind item_off: none of it
    // depends on the survivors.  The output phase finds a hit's work item here again, not in global memory.
    MergeList mine{};
    int cntl[4] = {0, 0, 0, 0};
    if (n_lists >= 1) {
        const int64_t j = first + min(lane & 3, n_lists - 1);  // lists past the query's last repeat it: valid addresses, never selected
        const WorkItem it = items[j];
        const int cnt = item_n[j];
        if (item_slack) { mine.slack = item_slack[2 * j]; mine.ub = item_slack[2 * j + 1]; }
        mine.start = it.start; mine.tab0 = it.tab0; mine.tab1 = it.tab1; mine.rank = it.rank;
        mine.pos0 = it.pos0; mine.len = it.len; mine.cell = it.cell;
#pragma unroll
        for (int i = 0; i < 4; ++i) cntl[i] = i < n_lists ? __builtin_amdgcn_readlane(cnt, i) : 0;
    }
    if constexpr (MT != 0) {
        // Usual case: <= 4 lists, <= 256 survivors in all.  The survivors carry their float32 distances: find the value v
        // that `limit` of them do not exceed (ballot bisection in registers) and drop everything above v*(1+3eps) BEFORE
        // the exact re-scoring -- strictly worse, in exact arithmetic, than the `limit` entries below v (the scan's own
        // argument).  ~limit/130 of the table reads, and the sort runs on 128 keys instead of 256.
        const int n_total = cntl[0] + cntl[1] + cntl[2] + cntl[3];
        auto fast = [&](auto ne_tag) -> bool {
            constexpr int NE = decltype(ne_tag)::value;  // survivors per lane
            uint32_t hi[NE], pp[NE];
            int li[NE];
            bool valid[NE];
            uint32_t mn = 0xffffffffu, mx = 0u;
            // (the lane's NE survivors are read together, from clamped addresses: as `valid ? surv[..] : ~0` they were NE round
            // trips one after the other at the head of every query's chain of dependent loads)
            uint64_t ent[NE];
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                const int x = lane + 64 * i;
                valid[i] = x < n_total;
                int lst = 0, off = x;
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (lst == j && off >= cntl[j]) { off -= cntl[j]; lst = j + 1; }
                li[i] = lst;
                ent[i] = surv[valid[i] ? (first + lst) * (int64_t)S + off : first * (int64_t)S];
            }
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                hi[i] = valid[i] ? (uint32_t)(ent[i] >> 32) : 0xffffffffu;
                pp[i] = valid[i] ? (uint32_t)ent[i] : 0xffffffffu;
                const float ub_i = from_lane(mine.ub, li[i]);  // (every lane takes part in a cross-lane read: outside the condition)
                if (item_slack && valid[i])  // k_adc_scan3 hands over the 16-bit sum: (sum + M) * ub >= the exact distance
                    hi[i] = __float_as_uint(__double2float_ru((double)(hi[i] + (uint32_t)MT) * (double)ub_i));
                mn = (valid[i] && hi[i] < mn) ? hi[i] : mn;
                mx = (valid[i] && hi[i] > mx) ? hi[i] : mx;
            }
            uint32_t thr = 0xffffffffu;
            float vub = __int_as_float(0x7f800000);  // scan3 survivors: a distance that `limit` of them do not exceed
            if (n_total > limit) {
                wave_minmax_all(mn, mx);
                const uint32_t v = wave_kth_bisect<NE>(hi, valid, mn, mx, limit);
                if (item_slack) {
                    vub = __uint_as_float(v);
                } else {
                    const float margin = 1.0f + 3.0f * (2.0f * (float)MT * 5.9604645e-8f);
                    thr = __float_as_uint(__double2float_ru((double)__uint_as_float(v) * (double)margin));
                }
            }
            int kept = 0;
            int idx[NE];
            bool keep[NE];
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                keep[i] = valid[i] && hi[i] <= thr;
                const float s_i = from_lane(mine.slack, li[i]);
                if (item_slack) {  // strictly worse than `limit` others only if even its lower bound is above vub
                    keep[i] = valid[i] && ((double)__uint_as_float(hi[i]) - (double)s_i <= (double)vub);  // exact in float64
                }
                const unsigned long long m = __ballot(keep[i]);
                idx[i] = kept + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
                kept += __popcll(m);
            }
            if (kept > CAPM) return false;  // a crowd of equal float32 distances: the general rounds below
            // Only the kept entries are re-scored, compacted: (list, position) goes to the wave's sort region at the entry's
            // prefix index and comes back one candidate per lane, so a pass of 64 candidates holds M table entries per lane in
            // flight and no pass is spent on entries the cut dropped.
#pragma unroll
            for (int i = 0; i < NE; ++i)
                if (keep[i]) kb[idx[i]] = ((uint64_t)(uint32_t)li[i] << 32) | pp[i];
            wave_lds_sync();
#pragma unroll 1
            for (int c0 = 0; c0 < kept; c0 += 64) {
                const bool on = c0 + lane < kept;
                const int c = on ? c0 + lane : c0;  // an idle lane re-scores the pass's first candidate and drops the result
                const uint64_t lp = kb[c];
                const int lst = (int)(lp >> 32);
                const uint32_t p = (uint32_t)lp;
                const CodeWords<MT> cw = load_code<MT>(codes, from_lane(mine.start, lst) + p);
                const double d = adc64_words<MT>(cw.w, K, T + (int64_t)from_lane(mine.tab0, lst) * nf * K,
                                                 T + (int64_t)from_lane(mine.tab1, lst) * nf * K);
                const uint32_t rank = (uint32_t)from_lane(mine.rank, lst), pos0 = (uint32_t)from_lane(mine.pos0, lst);
                if (on) {
                    ka[c] = (uint64_t)__double_as_longlong(d);
                    kb[c] = ((uint64_t)rank << 32) | (pos0 + p);
                }
            }
            int ns = 64;
            while (ns < kept) ns <<= 1;
            for (int x = kept + lane; x < ns; x += 64) { ka[x] = ~0ull; kb[x] = ~0ull; }
            wave_lds_sync();
            wave_bitonic_lds(ka, kb, ns);
            total = kept;
            return true;
        };
        if (n_lists >= 1 && n_lists <= 4) {
            if (n_total <= 256) done_fast = fast(std::integral_constant<int, 4>());
            else if (NEMAX >= 8 && n_total <= 512) {
                if constexpr (NEMAX >= 8) done_fast = fast(std::integral_constant<int, 8>());
            }
        }
    }
    while (!done_fast) {  // rounds: append up to CAPM - have entries, sort, keep `limit`
        int n = have;
        int room = CAPM - have;
        while (l < n_lists && room > 0) {
            const int valid = item_n[first + l];
            const int take = (valid - e < room) ? (valid - e) : room;
            if (take > 0) {
                const WorkItem it = items[first + l];
                const double* t0 = T + (int64_t)it.tab0 * nf * K;
                const double* t1 = T + (int64_t)it.tab1 * nf * K;
                const uint64_t* src = surv + (first + l) * (int64_t)S + e;
                if constexpr (MT == 0) {
                    for (int x = lane; x < take; x += 64) {
                        const uint32_t p = (uint32_t)src[x];
                        ka[n + x] = (uint64_t)__double_as_longlong(adc64_global(codes, it.start + p, M, K, t0, t1));
                        kb[n + x] = ((uint64_t)(uint32_t)it.rank << 32) | (uint32_t)(it.pos0 + (int)p);
                    }
                } else {
                    // four candidates per lane at a time: positions, then codes, then 4 x M table entries in flight together
                    for (int x0 = 0; x0 < take; x0 += 256) {
                        uint32_t p[4];
                        bool on[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int x = x0 + i * 64 + lane;
                            on[i] = x < take;
                            p[i] = on[i] ? (uint32_t)src[x] : 0u;
                        }
                        CodeWords<MT> cw[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) cw[i] = load_code<MT>(codes, it.start + p[i]);
                        double dd[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) dd[i] = adc64_words<MT>(cw[i].w, K, t0, t1);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int x = x0 + i * 64 + lane;
                            if (on[i]) {
                                ka[n + x] = (uint64_t)__double_as_longlong(dd[i]);
                                kb[n + x] = ((uint64_t)(uint32_t)it.rank << 32) | (uint32_t)(it.pos0 + (int)p[i]);
                            }
                        }
                    }
                }
            }
            n += take;
            total += take;
            room -= take;
            e += take;
            if (e >= valid) { ++l; e = 0; }
        }
        int ns = 64;
        while (ns < n) ns <<= 1;
        for (int x = n + lane; x < ns; x += 64) { ka[x] = ~0ull; kb[x] = ~0ull; }
        wave_lds_sync();
        wave_bitonic_lds(ka, kb, ns);
        have = n < limit ? n : limit;
        if (l >= n_lists) break;
    }
    const int nv = total < limit ? total : limit;
    const int64_t o = (int64_t)q * limit;
    // the first four lists' fields, wave-uniform from here on: the ids gather is the only global load between the sort and the stores
    int64_t l_start[4];
    uint32_t l_pos0[4], l_rank[4], l_len[4];
    int l_cell[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        l_start[i] = (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)((uint64_t)mine.start >> 32), i) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)mine.start, i));
        l_pos0[i] = (uint32_t)__builtin_amdgcn_readlane(mine.pos0, i);
        l_rank[i] = (uint32_t)__builtin_amdgcn_readlane(mine.rank, i);
        l_len[i] = i < n_lists ? (uint32_t)__builtin_amdgcn_readlane(mine.len, i) : 0u;  // a list the query does not have holds nothing
        l_cell[i] = __builtin_amdgcn_readlane(mine.cell, i);
    }
    for (int x = lane; x < limit; x += 64) {
        cis_hit hh;
        hh.dist = __longlong_as_double(0x7ff0000000000000LL);
        hh.visit_rank = 0xffffffffu; hh.pos = 0xffffffffu; hh.id = -1; hh.cell = -1; hh.reserved = 0;
        if (x < nv) {
            const uint32_t rank = (uint32_t)(kb[x] >> 32), pos = (uint32_t)kb[x];
            // the work item this hit came from: same cell (visit rank), chunk that contains the position; the first such list
            int64_t src = -1;
            int cell = -1;
#pragma unroll
            for (int li = 3; li >= 0; --li) {
                const uint32_t rel = pos - l_pos0[li];
                if (l_rank[li] == rank && rel < l_len[li]) {
                    src = l_start[li] + rel;
                    cell = l_cell[li];
                }
            }
            for (int li = 4; li < n_lists && src < 0; ++li) {
                const WorkItem it = items[first + li];
                const uint32_t rel = pos - (uint32_t)it.pos0;
                if ((uint32_t)it.rank == rank && rel < (uint32_t)it.len) {
                    src = it.start + rel;
                    cell = it.cell;
                }
            }
            if (src >= 0) {
                hh.dist = __longlong_as_double((long long)ka[x]);
                hh.visit_rank = rank;
                hh.pos = pos;
                hh.id = ids[src];
                hh.cell = cell;
            }
        }
        if (out_hits) out_hits[o + x] = hh;
        if (out_ids) {
            out_ids[o + x] = hh.id;
            out_dists[o + x] = (x < nv) ? hh.dist : __longlong_as_double(0x7ff8000000000000LL);
        }
        if (out_cells) out_cells[o + x] = hh.cell;
        if (out_pos) out_pos[o + x] = hh.pos;
    }
    if (lane == 0 && out_n) out_n[q] = nv;
}

__global__ void k_copy_visited(const PlanOut* __restrict__ plan, int nq, int32_t* __restrict__ visited) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) visited[q] = plan[q].visited;
}

// ================================================================================================
// host: index object -- storage, insert and the get_cell / get_codes readers are in lopq_index.hip
// ================================================================================================

extern "C" int cis_index_set_profiling(cis_index* ix, int enable) {
    CIS_REQUIRE(ix != nullptr, "index is NULL");
    ix->profiling = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return CIS_OK;
}

// ---- device self test of the wave-level primitives (tests/test_lopq_hip_parity.py) --------------
template <int LJ>
__device__ int selftest_xor(uint32_t v) { return lane_xor<LJ>(v) != (uint32_t)__shfl_xor((int)v, LJ) ? 1 : 0; }

template <int NR>
__device__ int selftest_sort(uint32_t seed) {
    const int lane = threadIdx.x & 63;
    uint32_t k[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        uint32_t x = seed ^ (uint32_t)(lane * NR + r) * 2654435761u;
        x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        k[r] = x % 1000u;  // many duplicates
    }
    uint32_t mine[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) mine[r] = k[r];
    wave_bitonic_sort<NR>(k);
    int bad = 0;
    // sortedness: element e <= element e+1 (e = lane*NR + r)
#pragma unroll
    for (int r = 0; r + 1 < NR; ++r) bad += k[r] > k[r + 1];
    const uint32_t nxt = (uint32_t)__shfl_down((int)k[0], 1);
    if (lane < 63) bad += k[NR - 1] > nxt;
    // multiset preserved: compare sums and xors
    uint32_t s0 = 0, s1 = 0, x0 = 0, x1 = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) { s0 += mine[r]; s1 += k[r]; x0 ^= mine[r] * 40503u; x1 ^= k[r] * 40503u; }
    for (int o = 32; o > 0; o >>= 1) {
        s0 += (uint32_t)__shfl_xor((int)s0, o); s1 += (uint32_t)__shfl_xor((int)s1, o);
        x0 ^= (uint32_t)__shfl_xor((int)x0, o); x1 ^= (uint32_t)__shfl_xor((int)x1, o);
    }
    bad += (s0 != s1) + (x0 != x1);
    return bad;
}

static __device__ uint32_t selftest_hash(uint32_t x) {
    x *= 2654435761u; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
    return x;
}

// The selection primitives of scan_common.h: one wave against a serial reference that lane 0 computes from the same keys in LDS.
// Entry e = r * 64 + lane, as in a hit region; its candidate position is 7 * e + 3.  Case c picks the keys and the cut:
//   0  cnt < L: nothing cut, no bound; the bisection behind its callers' guard, and at its edge n == cnt
//   1  cnt == L                                       2  distinct hi: the cut falls between groups; W = 0
//   3  three values of hi, fifty of lo: the cut goes through a group of equal hi with different lo (sort of the low words), the
//      counts of the bisection jump over the window
//   4  three values of hi, lo follows hi: the cut goes through a group of equal keys (first `need` in region order, dup_pos)
//   5  two values of hi, distinct lo                  6  all keys equal                  7  a thousand values of hi, random lo
template <int NR>
__device__ int selftest_cut(int c, uint32_t seed) {
    __shared__ uint32_t s_hi[NR * 64], s_lo[NR * 64], s_out[NR * 64];
    const int lane = threadIdx.x & 63;
    const int cnt = NR * 64 - 8 - (int)seed * 5 - c;  // never a multiple of 64: the last row is partial
    const int L = c == 0 ? cnt + 3 : (c == 1 ? cnt : (c == 7 ? cnt / 3 : (c == 2 ? cnt * 2 / 3 : cnt / 2 - (int)seed)));
    uint32_t hi[NR], lo[NR], mn = 0xffffffffu, mx = 0u;
    bool keep[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const uint32_t e = (uint32_t)(r * 64 + lane), h = selftest_hash(seed * 4099u + e), h2 = selftest_hash(h + 1u);
        const uint32_t distinct = (e * 167u + seed) % 1021u;
        keep[r] = (int)e < cnt;
        hi[r] = c == 2 ? distinct : (c == 3 || c == 4 ? h % 3u : (c == 5 ? h % 2u : (c == 6 ? 5u : h % 1000u)));
        lo[r] = c == 3 ? h2 % 50u : (c == 4 ? hi[r] * 7u + 1u : (c == 5 ? distinct : (c == 6 ? 9u : h2)));
        s_hi[e] = hi[r]; s_lo[e] = lo[r];
        mn = (keep[r] && hi[r] < mn) ? hi[r] : mn;
        mx = (keep[r] && hi[r] > mx) ? hi[r] : mx;
    }
    wave_minmax_all(mn, mx);
    // wave_bisect_window / wave_count_le on the hi words
    const int n = L <= cnt ? L : cnt, W = c == 0 ? 3 : (c == 3 || c == 4 ? 2 : (c == 7 ? n >> 3 : 0));
    const uint32_t v = wave_bisect_window<NR>(keep, hi, mn, mx, n, W);
    const uint32_t v_guard = wave_bisect_window<NR>(keep, hi, cnt >= L ? mn : mx, mx, L, W);  // as wave_compact_approx calls it
    const int c_v = wave_count_le<NR>(keep, hi, v);
    // wave_stable_keep: nothing, everything, or about half of the entries
    const auto pred = [&](uint32_t key) { return (c & 3) == 0 ? false : ((c & 3) == 1 ? true : ((key >> 3) & 1u) != 0u); };
    const int n_kept = wave_stable_keep<NR>([&](int r) { return keep[r] && pred(lo[r]); }, [&](int r, int idx) { s_out[idx] = lo[r]; });
    wave_lds_sync();
    int bad = 0;
    if (lane == 0) {
        int c_ref = 0, j = 0;
        uint32_t nth = 0xffffffffu, k_min = 0xffffffffu, k_max = 0u;
        for (int e = 0; e < cnt; ++e) {
            int c_e = 0;
            for (int f = 0; f < cnt; ++f) c_e += s_hi[f] <= s_hi[e];
            if (c_e >= n && s_hi[e] < nth) nth = s_hi[e];  // the n-th smallest key
            c_ref += s_hi[e] <= v;
            k_min = s_hi[e] < k_min ? s_hi[e] : k_min;
            k_max = s_hi[e] > k_max ? s_hi[e] : k_max;
            if (pred(s_lo[e])) { bad += s_out[j] != s_lo[e]; ++j; }
        }
        bad += (mn != k_min) + (mx != k_max) + (c_v != c_ref) + (c_ref < n) + (c_ref > n + W && v != nth) + (j != n_kept);
        bad += (c == 3 || c == 6) && v != nth;      // ties: no value has its count inside the window
        bad += (cnt >= L ? v_guard != v : v_guard != mx);
    }
    wave_lds_sync();
    // wave_exact_cut
    uint32_t vhiL = 0u, dup_pos = 0xffffffffu;
    uint64_t boundL = 0ull;
    wave_exact_cut<NR>(hi, lo, keep, [&](int r) { return 7u * (uint32_t)(r * 64 + lane) + 3u; }, mn, mx, cnt, L, vhiL, boundL, dup_pos);
#pragma unroll
    for (int r = 0; r < NR; ++r) s_out[r * 64 + lane] = keep[r] ? 1u : 0u;
    wave_lds_sync();
    if (lane == 0) {
        // the reference's stable sorted(): entry e survives when fewer than L entries come before it by (hi, lo, e)
        int kth = -1;
        for (int e = 0; e < NR * 64; ++e) {
            int before = 0;
            for (int f = 0; f < cnt; ++f)
                before += s_hi[f] < s_hi[e] || (s_hi[f] == s_hi[e] && (s_lo[f] < s_lo[e] || (s_lo[f] == s_lo[e] && f < e)));
            bad += s_out[e] != ((e < cnt && before < L) ? 1u : 0u);
            if (e < cnt && before == L - 1) kth = e;
        }
        uint32_t dup_ref = 0xffffffffu;
        if (kth >= 0) {
            int c_less = 0, g = 0, first = -1;
            for (int e = cnt - 1; e >= 0; --e) {
                c_less += s_hi[e] < s_hi[kth];
                g += s_hi[e] == s_hi[kth];
                if (s_hi[e] == s_hi[kth] && s_lo[e] == s_lo[kth]) first = e;
            }
            if (L - c_less < g) dup_ref = 7u * (uint32_t)first + 3u;  // the cut went through the group of the L-th entry's hi word
        }
        bad += (kth >= 0) != (cnt >= L);
        bad += vhiL != (kth >= 0 ? s_hi[kth] : mx);
        bad += boundL != (kth >= 0 ? hi_to_bound(s_hi[kth]) : 0x7ff0000000000000ull);
        bad += dup_pos != dup_ref;
        bad += (c == 4 || c == 6) && dup_ref == 0xffffffffu;  // these cases are built to reach the tie rule
    }
    return bad;
}

__global__ void k_selftest(int* __restrict__ errors) {
    const uint32_t v = (uint32_t)threadIdx.x * 7919u + blockIdx.x * 104729u + 17u;
    int bad = selftest_xor<1>(v) + selftest_xor<2>(v) + selftest_xor<4>(v) + selftest_xor<8>(v) + selftest_xor<16>(v) +
              selftest_xor<32>(v);
    bad += selftest_sort<4>(blockIdx.x * 977u + 1u) + selftest_sort<8>(blockIdx.x * 31u + 5u);
    bad += selftest_cut<4>(blockIdx.x & 7, blockIdx.x >> 3) + selftest_cut<8>(blockIdx.x & 7, blockIdx.x >> 3);
    if (bad) atomicAdd(errors, bad);
}

#ifdef CIS_SCAN_COUNTERS
extern "C" int cis_debug_counters(unsigned long long* out, int reset) {
    CIS_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_scan_ctr), 16 * sizeof(unsigned long long)));
    if (reset) {
        unsigned long long z[16] = {0};
        CIS_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_scan_ctr), z, sizeof(z)));
    }
    return CIS_OK;
}
#endif

extern "C" int cis_selftest(int* n_errors) {
    CIS_REQUIRE(n_errors != nullptr, "NULL argument");
    CIS_TRY(cis_lazy_init());
    int* d = nullptr;
    CIS_CHECK_HIP(hipMalloc((void**)&d, sizeof(int)));
    CIS_CHECK_HIP(hipMemset(d, 0, sizeof(int)));
    hipLaunchKernelGGL(k_selftest, dim3(64), dim3(64), 0, nullptr, d);
    CIS_CHECK_HIP(hipMemcpy(n_errors, d, sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return CIS_OK;
}

extern "C" int cis_index_set_scan_mode(cis_index* ix, int mode) {
    CIS_REQUIRE(ix != nullptr && mode >= 0 && mode <= 7, "bad scan mode");
    if (mode == 7) mode = 5;  // 7 forced a kernel that was removed: it stays accepted and sets what 5 sets
    ix->force_stream = (mode == 6);
    ix->force_exact_scan = (mode == 1);
    ix->force_prefilter_scan = (mode >= 2 && mode <= 5);
    ix->force_scan2 = (mode == 2);
    ix->force_scan3 = (mode == 3 || mode == 4 || mode == 5);
    ix->force_two_pass = mode == 3 ? 0 : (mode == 4 ? 1 : (mode == 5 ? 2 : -1));
    return CIS_OK;
}

extern "C" int cis_index_read_profile(cis_index* ix, double ms[5], int64_t* launches) {
    CIS_REQUIRE(ix != nullptr && ms != nullptr, "NULL argument");
    for (auto& r : ix->prof) {
        hipEvent_t last = r.ev[4] ? r.ev[4] : r.ev[3];
        if (last) CIS_CHECK_HIP(hipEventSynchronize(last));
        for (int i = 0; i < 4; ++i) {
            if (!r.ev[i] || !r.ev[i + 1]) continue;
            float t = 0.f;
            CIS_CHECK_HIP(hipEventElapsedTime(&t, r.ev[i], r.ev[i + 1]));
            ix->prof_ms[i] += t;
        }
        if (r.has_scan && r.ev[5] && r.ev[3]) {
            float t = 0.f;
            CIS_CHECK_HIP(hipEventElapsedTime(&t, r.ev[5], r.ev[3]));
            ix->prof_ms[4] += t;
            ix->prof_launches += 1;
        }
        for (int i = 0; i < 6; ++i)
            if (r.ev[i]) (void)hipEventDestroy(r.ev[i]);
    }
    ix->prof.clear();
    for (int i = 0; i < 5; ++i) { ms[i] = ix->prof_ms[i]; ix->prof_ms[i] = 0; }
    if (launches) *launches = ix->prof_launches;
    ix->prof_launches = 0;
    return CIS_OK;
}

extern "C" int cis_index_last_scan_kernel(cis_index* ix) { return ix ? ix->last_scan_kernel : 0; }

extern "C" int cis_index_stream_counters(cis_index* ix, int64_t counters[2]) {
    CIS_REQUIRE(ix != nullptr && counters != nullptr, "NULL argument");
    counters[0] = ix->stream_batches;
    counters[1] = ix->stream_fallbacks;
    return CIS_OK;
}

extern "C" int cis_index_last_stats(cis_index* ix, int64_t stats[4]) {
    CIS_REQUIRE(ix != nullptr && stats != nullptr, "NULL argument");
    if (ix->stats_pending_seq) {  // the last batch ran on bounds: its totals are in the pinned words once its plan has run
        if (__atomic_load_n(&ix->h_totals[3], __ATOMIC_ACQUIRE) != ix->stats_pending_seq) CIS_CHECK_HIP(hipDeviceSynchronize());
        ix->stats[0] += ix->h_totals[2];
        ix->stats[1] += ix->h_totals[0];
        ix->stats[2] += ix->h_totals[1];
        ix->stats_pending_seq = 0;
    }
    for (int i = 0; i < 4; ++i) stats[i] = ix->stats[i];
    return CIS_OK;
}

// ================================================================================================
// host: search pipeline
// ================================================================================================
// exact float64 kernel (v1); flag != nullptr restricts it to the items the fast kernel flagged
template <int CAP, int U>
static void launch_scan_m(int M, const ScanArgs& a, int S, const int* flag) {
    const size_t lds = (size_t)CAP * 16 + (size_t)M * a.K * sizeof(double) + 16;
    dispatch_int<0, 4, 8, 16>((M == 4 || M == 8 || M == 16) ? M : 0, [&](auto m) {  // 0: any M
        hipLaunchKernelGGL((k_adc_scan<decltype(m)::value, CAP, U>), dim3((unsigned)a.n_items), dim3(256), lds, a.st, a.items, a.T, a.codes, a.ids, M, a.K, a.L, S, flag,
                           reinterpret_cast<cis_hit*>(a.hits), a.hitn);
    });
}

static void launch_scan_exact(int M, const ScanArgs& a, int S, const int* flag) {
    if (a.L <= 512) launch_scan_m<1024, 2>(M, a, S, flag);
    else if (a.L <= 1024) launch_scan_m<2048, 4>(M, a, S, flag);
    else launch_scan_m<4096, 4>(M, a, S, flag);
}

// float32-prefilter kernel (v2): M in {4, 8, 16}, K <= 256, L <= 952 (a wave region of NR * 64 - 8 entries holds L + 64; 16 registers
// per lane above 440, one query per workgroup there: 43-51 KB of LDS, three workgroups per CU)
static const int SCAN2_MAX_LIMIT = 952;
static bool scan2_supported(int M, int K, int L) {
    return (M == 4 || M == 8 || M == 16) && K <= 256 && K % 4 == 0 && L >= 1 && L <= SCAN2_MAX_LIMIT;
}

// G = 2 queries per workgroup of 8 waves (one 2-query table set shared by 8 waves) when the batch is
// large enough to find pairs; G = 1 with 4 waves for small batches (latency mode).
static Scan2Geom scan2_geom(int M, int K, int L, int nq) {
    Scan2Geom g;
    const int NR = (L <= 184) ? 4 : (L <= 440 ? 8 : 16);
    g.G = (nq >= 64 && NR < 16) ? 2 : 1;  // pairs of queries per workgroup when the batch is large enough to find pairs
    g.NW = 4;
    g.U = (g.G == 2) ? 4 : 2;
    if (const char* e = getenv("CIS_SCAN_GEOM")) {  // experiments: "G,NW,U" out of the instantiated set
        int a = 0, b = 0, c = 0;
        if (NR < 16 && sscanf(e, "%d,%d,%d", &a, &b, &c) == 3 && ((a == 1 && b == 4) || (a == 2 && b == 4) || (a == 2 && b == 8 && c == 2) || (a == 2 && (b == 1 || b == 2) && c == 4) || (a == 4 && b == 4 && c == 4 && NR == 4)) && (c == 2 || c == 4)) {
            g.G = a; g.NW = b; g.U = c;
        }
    }
    g.S = g.NW * (NR * 64 - 8);  // survivor slots per work item: a full region per wave
    g.lds = (size_t)K * M * g.G * 4 + (size_t)g.G * g.NW * (NR * 64 - 8 + 64) * 8 + g.G * sizeof(ScanShared) + 16;
    return g;
}

template <int M, int NR, int G, int NW, int U>
static void launch_scan2_t(const Scan2Geom& g, const ScanArgs& a) {
    const float eps = 2.0f * (float)M * 5.9604645e-8f;  // 2 * M * 2^-24
    const float margin = 1.0f + 3.0f * eps;
    const int per_cu = (int)(163840 / g.lds) < (32 / NW) ? (int)(163840 / g.lds) : (32 / NW);
    hipLaunchKernelGGL((k_adc_scan2<M, NR, U, G, NW>), dim3(persistent_grid(a, G, per_cu)), dim3(NW * 64), g.lds, a.st, a.items, a.slots, a.n_slots, a.T, a.T32, a.codes, a.ids,
                       a.K, a.L, g.S, margin, a.qctr, a.hits, a.hitn, a.qbound);
}

template <int M, int NR>
static void launch_scan2_mr(const Scan2Geom& g, const ScanArgs& a) {
#define CIS_SCAN2_CASE(GG, WW, UU) if (g.G == GG && g.NW == WW && g.U == UU) return launch_scan2_t<M, NR, GG, WW, UU>(g, a);
    CIS_SCAN2_CASE(1, 4, 2)
    if constexpr (NR != 16) {  // limit 441 ... 952 (NR = 16): one query per workgroup only
        CIS_SCAN2_CASE(1, 4, 4)
        CIS_SCAN2_CASE(2, 4, 4)
        CIS_SCAN2_CASE(2, 4, 2)
        CIS_SCAN2_CASE(2, 8, 2)
        CIS_SCAN2_CASE(2, 1, 4)
        CIS_SCAN2_CASE(2, 2, 4)
    }
    if constexpr (NR == 4) { CIS_SCAN2_CASE(4, 4, 4) }  // four queries per workgroup: measured slower (72 KB of LDS -> 2 workgroups per CU)
#undef CIS_SCAN2_CASE
}

static void launch_scan2(int M, const Scan2Geom& g, const ScanArgs& a) {  // (scan2_supported: M = 4, 8 or 16)
    dispatch_int<4, 8, 16>(M, [&](auto m) { dispatch_nr<16>(a.L, [&](auto nr) { launch_scan2_mr<decltype(m)::value, decltype(nr)::value>(g, a); }); });
}

// ---- large `limit` (above what the LDS top-k kernels hold): exact distance of EVERY candidate, stable segmented
// sort per query (the merge sort of csrc/lopq_sort.hip; rocPRIM until round 4).  Candidates are laid out in retrieval order (items of a query
// in visit order, positions ascending), so a stable sort on the distance alone yields the (dist, visit_rank, pos)
// ranking = the reference's stable sorted() over the retrieved list (search.py:210).
int cis_seg_sort_u64(void* temp, size_t* temp_bytes, const uint64_t* keys_in, uint64_t* keys_out, const uint64_t* vals_in,
                     uint64_t* vals_out, int64_t n, int nseg, const int64_t* seg_begin, const int64_t* seg_end, hipStream_t st);

__global__ void k_seg_begin(const int64_t* __restrict__ cand_start, const int64_t* __restrict__ item_off, int nq, int64_t n_items,
                            int64_t n_cand, int64_t* __restrict__ seg, unsigned long long* __restrict__ qmin,
                            unsigned long long* __restrict__ qmax) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q > nq) return;
    const int64_t it = item_off[q];
    seg[q] = (q == nq || it >= n_items) ? n_cand : cand_start[it];
    if (qmin && q < nq) { qmin[q] = ~0ull; qmax[q] = 0ull; }
}

// candidate layout for batches of many work items (hundreds of thousands: tiny cells): exclusive scan of the items' lengths
// over tiles of 4096 items -- tile sums, one workgroup scans them, tiles rescan with their offset -- then k_seg_begin.
// (k_cand_layout below does it all in one workgroup: the right thing for the usual few thousand items, 2 ms for a million.)
static const int CAND_TILE = 4096;
__global__ __launch_bounds__(256) void k_cand_tile_sum(const WorkItem* __restrict__ items, int64_t n_items, int64_t* __restrict__ tile_sums) {
    __shared__ int64_t s_w[4];
    const int64_t base = (int64_t)blockIdx.x * CAND_TILE;
    int64_t sum = 0;
    for (int e = threadIdx.x; e < CAND_TILE; e += 256)
        if (base + e < n_items) sum += items[base + e].len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(1024) void k_cand_tile_scan(int64_t* __restrict__ tile_sums, int64_t ntiles) {  // in place, exclusive
    __shared__ int64_t s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < ntiles; b0 += 1024) {
        const int64_t i = b0 + tid;
        const int64_t v = i < ntiles ? tile_sums[i] : 0;
        int64_t x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        __syncthreads();
        if (lane == 63) s_w[wv] = x;
        __syncthreads();
        int64_t base = carry, tot = 0;
        for (int w = 0; w < 16; ++w) { if (w < wv) base += s_w[w]; tot += s_w[w]; }
        if (i < ntiles) tile_sums[i] = base + x - v;
        carry += tot;
    }
}

__global__ __launch_bounds__(256) void k_cand_tile_apply(const WorkItem* __restrict__ items, int64_t n_items,
                                                         const int64_t* __restrict__ tile_off, int64_t* __restrict__ cand_start) {
    __shared__ int64_t s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * CAND_TILE;
    int64_t carry = tile_off[blockIdx.x];
    for (int e0 = 0; e0 < CAND_TILE; e0 += 256) {
        const int64_t i = base + e0 + tid;
        const int64_t v = i < n_items ? items[i].len : 0;
        int64_t x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        __syncthreads();
        if (lane == 63) s_w[wv] = x;
        __syncthreads();
        int64_t b = carry;
        for (int w = 0; w < wv; ++w) b += s_w[w];
        if (i < n_items) cand_start[i] = b + x - v;
        carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    }
}

// candidate layout of the all-candidates path in one launch: exclusive scan of the work items' lengths (cand_start),
// the per-query segment starts (seg[q] = first candidate of query q, seg[nq] = n_cand) and the reset of the key ranges
__global__ __launch_bounds__(1024) void k_cand_layout(const WorkItem* __restrict__ items, int64_t n_items, const int64_t* __restrict__ item_off,
                                                      int nq, int64_t n_cand, int64_t* cand_start, int64_t* __restrict__ seg,
                                                      unsigned long long* __restrict__ qmin, unsigned long long* __restrict__ qmax,
                                                      const int64_t* __restrict__ d_totals /* null, or the plan totals (arguments are bounds) */) {
    __shared__ int64_t s_w[16];
    if (d_totals) { n_items = d_totals[0]; n_cand = d_totals[2]; }
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t chunk = (n_items + 1023) / 1024;
    const int64_t lo = tid * chunk, hi = lo + chunk < n_items ? lo + chunk : n_items;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += items[i].len;
    int64_t x = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_w[wv] = x;
    __syncthreads();
    int64_t run = x - sum;
    for (int w = 0; w < wv; ++w) run += s_w[w];
    for (int64_t i = lo; i < hi; ++i) {
        __hip_atomic_store(&cand_start[i], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        run += items[i].len;
    }
    __threadfence();
    __syncthreads();
    for (int q = tid; q <= nq; q += 1024) {
        const int64_t it = item_off[q];
        seg[q] = (q == nq || it >= n_items) ? n_cand : __hip_atomic_load(&cand_start[it], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (qmin && q < nq) { qmin[q] = ~0ull; qmax[q] = 0ull; }
    }
}

// per-query range of the keys (for the selection kernel): workgroup reduction in LDS, one pair of global atomics
__device__ __forceinline__ void publish_key_range(uint64_t mn, uint64_t mx, unsigned long long* __restrict__ qmin,
                                                  unsigned long long* __restrict__ qmax, int q) {
    __shared__ unsigned long long s_mm[2];
    if (threadIdx.x == 0) { s_mm[0] = ~0ull; s_mm[1] = 0ull; }
    __syncthreads();
    if (mn <= mx) {
        atomicMin(&s_mm[0], (unsigned long long)mn);
        atomicMax(&s_mm[1], (unsigned long long)mx);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_mm[0] <= s_mm[1]) {
        atomicMin(&qmin[q], s_mm[0]);
        atomicMax(&qmax[q], s_mm[1]);
    }
}

__global__ __launch_bounds__(256) void k_adc_all(const WorkItem* __restrict__ items, const int64_t* __restrict__ cand_start,
                                                 const double* __restrict__ T, const uint8_t* __restrict__ codes, int M, int K,
                                                 uint64_t* __restrict__ keys, uint64_t* __restrict__ vals,
                                                 unsigned long long* __restrict__ qmin, unsigned long long* __restrict__ qmax,
                                                 const int64_t* __restrict__ d_totals /* null, or the plan totals: gridDim.x is a bound */) {
    if (d_totals && (int64_t)blockIdx.x >= d_totals[0]) return;
    const WorkItem it = items[blockIdx.x];
    const int nf = M / 2;
    const double* t0 = T + (int64_t)it.tab0 * nf * K;
    const double* t1 = T + (int64_t)it.tab1 * nf * K;
    const int64_t o = cand_start[blockIdx.x];
    uint64_t mn = ~0ull, mx = 0ull;
    for (int p = blockIdx.y * blockDim.x + threadIdx.x; p < it.len; p += gridDim.y * blockDim.x) {
        const uint64_t kk = (uint64_t)__double_as_longlong(adc64_global(codes, it.start + p, M, K, t0, t1));
        keys[o + p] = kk;
        mn = kk < mn ? kk : mn;
        mx = kk > mx ? kk : mx;
        if (vals) vals[o + p] = ((uint64_t)blockIdx.x << 32) | (uint32_t)p;
    }
    if (qmin) publish_key_range(mn, mx, qmin, qmax, it.q);
}

// the same with the item's two table halves staged in LDS (M in {4, 8, 16}, K <= 256): the lookups of a cell's candidates
// are random reads of 2 * nf * K float64 entries, served from LDS instead of L2
template <int MT>
__global__ __launch_bounds__(256) void k_adc_all_lds(const WorkItem* __restrict__ items, const int64_t* __restrict__ cand_start,
                                                     const double* __restrict__ T, const uint8_t* __restrict__ codes, int K,
                                                     uint64_t* __restrict__ keys, uint64_t* __restrict__ vals,
                                                     unsigned long long* __restrict__ qmin, unsigned long long* __restrict__ qmax,
                                                     const int64_t* __restrict__ d_totals /* null, or the plan totals: gridDim.x is a bound */) {
    extern __shared__ __align__(16) double adc_tab[];  // [MT][K]
    if (d_totals && (int64_t)blockIdx.x >= d_totals[0]) return;
    const WorkItem it = items[blockIdx.x];
    int nch = (it.len + 2047) / 2048;  // workgroups that share this item (<= gridDim.y): ~2048 candidates each at least
    nch = nch < 1 ? 1 : (nch > (int)gridDim.y ? (int)gridDim.y : nch);
    if ((int)blockIdx.y >= nch) return;
    constexpr int nf = MT / 2;
    const double* t0 = T + (int64_t)it.tab0 * nf * K;
    const double* t1 = T + (int64_t)it.tab1 * nf * K;
    for (int e = threadIdx.x; e < nf * K; e += 256) {
        adc_tab[e] = t0[e];
        adc_tab[nf * K + e] = t1[e];
    }
    __syncthreads();
    const double* l0 = adc_tab;
    const double* l1 = adc_tab + nf * K;
    const int64_t o = cand_start[blockIdx.x];
    const int step = nch * 256;
    int p = blockIdx.y * 256 + threadIdx.x;
    uint64_t mn = ~0ull, mx = 0ull;
    for (; p + step < it.len; p += 2 * step) {  // two candidates in flight
        const CodeWords<MT> ca = load_code<MT>(codes, it.start + p);
        const CodeWords<MT> cb = load_code<MT>(codes, it.start + p + step);
        const uint64_t ka = (uint64_t)__double_as_longlong(adc64_words<MT>(ca.w, K, l0, l1));
        const uint64_t kb = (uint64_t)__double_as_longlong(adc64_words<MT>(cb.w, K, l0, l1));
        keys[o + p] = ka;
        keys[o + p + step] = kb;
        const uint64_t lo = ka < kb ? ka : kb, hi = ka < kb ? kb : ka;
        mn = lo < mn ? lo : mn;
        mx = hi > mx ? hi : mx;
        if (vals) {
            vals[o + p] = ((uint64_t)blockIdx.x << 32) | (uint32_t)p;
            vals[o + p + step] = ((uint64_t)blockIdx.x << 32) | (uint32_t)(p + step);
        }
    }
    if (p < it.len) {
        const CodeWords<MT> ca = load_code<MT>(codes, it.start + p);
        const uint64_t ka = (uint64_t)__double_as_longlong(adc64_words<MT>(ca.w, K, l0, l1));
        keys[o + p] = ka;
        mn = ka < mn ? ka : mn;
        mx = ka > mx ? ka : mx;
        if (vals) vals[o + p] = ((uint64_t)blockIdx.x << 32) | (uint32_t)p;
    }
    if (qmin) publish_key_range(mn, mx, qmin, qmax, it.q);
}

// The same for indexes of tiny cells (thousands of coarse clusters: a query visits hundreds of cells of a few codes each):
// one workgroup row per QUERY walks the query's candidates as one flat range; a candidate finds its work item by binary
// search over the items' first-candidate positions (staged in LDS) and reads its table entries from global memory (the
// query's ~100 half tables are L2-resident).  A workgroup per work item would stage 16 KB of tables for 8 candidates.
static const int FLAT_ITEMS = 4096;  // work items of a query whose starts fit the LDS stage; above: searched in global memory
template <int MT>
__global__ __launch_bounds__(256) void k_adc_all_flat(const WorkItem* __restrict__ items, const int64_t* __restrict__ cand_start,
                                                      const int64_t* __restrict__ seg, const int64_t* __restrict__ item_off,
                                                      const double* __restrict__ T, const uint8_t* __restrict__ codes, int M, int K,
                                                      uint64_t* __restrict__ keys, uint64_t* __restrict__ vals,
                                                      unsigned long long* __restrict__ qmin, unsigned long long* __restrict__ qmax) {
    __shared__ int s_start[FLAT_ITEMS];
    const int q = blockIdx.x;
    const int64_t it0 = item_off[q], it1 = item_off[q + 1];
    const int64_t c0 = seg[q], c1 = seg[q + 1];
    const int ni = (int)(it1 - it0);
    const int64_t n = c1 - c0;
    const bool staged = ni <= FLAT_ITEMS;
    if (staged)
        for (int i = threadIdx.x; i < ni; i += 256) s_start[i] = (int)(cand_start[it0 + i] - c0);
    __syncthreads();
    const int nf = M / 2;
    uint64_t mn = ~0ull, mx = 0ull;
    for (int64_t c = (int64_t)blockIdx.y * 256 + threadIdx.x; c < n; c += (int64_t)gridDim.y * 256) {
        int lo = 0, hi = ni;  // first item whose start is > c; the item before it holds c (empty items never exist)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int64_t st_ = staged ? (int64_t)s_start[mid] : cand_start[it0 + mid] - c0;
            if (st_ <= c) lo = mid + 1;
            else hi = mid;
        }
        const int i = lo - 1;
        const WorkItem it = items[it0 + i];
        const int p = (int)(c - (staged ? (int64_t)s_start[i] : cand_start[it0 + i] - c0));
        const double* t0 = T + (int64_t)it.tab0 * nf * K;
        const double* t1 = T + (int64_t)it.tab1 * nf * K;
        double d;
        if constexpr (MT != 0) {
            const CodeWords<MT> cw = load_code<MT>(codes, it.start + p);
            d = adc64_words<MT>(cw.w, K, t0, t1);
        } else {
            d = adc64_global(codes, it.start + p, M, K, t0, t1);
        }
        const uint64_t kk = (uint64_t)__double_as_longlong(d);
        keys[c0 + c] = kk;
        mn = kk < mn ? kk : mn;
        mx = kk > mx ? kk : mx;
        if (vals) vals[c0 + c] = ((uint64_t)(it0 + i) << 32) | (uint32_t)p;
    }
    if (qmin) publish_key_range(mn, mx, qmin, qmax, q);
}

// Tiny cells, direct form: no distance tables at all.  With thousands of coarse clusters a query touches ~100 (split, cluster)
// pairs per 10 k candidates -- more table entries (100 x nf x K) than lookups (10 k x M), 8 KB of float64 per table written and
// gathered back at random (10 GB per 8192 queries at V = 2048).  Here a candidate's entry j is computed where it is needed:
// e_j = sum_i (px[tab][j w + i] - sub[j][code_j][i])^2 in predict_cluster's order -- the expression, operands and summation of
// k_tables_from_px, so the same bits -- with the sub-quantizers of a PHASE (JP of them, <= 128 KB of float64) resident in LDS and
// the projected residuals px (512 B per (query, cluster)) read through L2.  The running sum of search.py:173 crosses the phases
// through the key array: phase p adds its entries, left to right, to what phase p - 1 left.
template <int MT, int W, int JP>
__global__ __launch_bounds__(1024) void k_adc_direct(const WorkItem* __restrict__ items, const int64_t* __restrict__ cand_start,
                                                     const int64_t* __restrict__ seg, const int64_t* __restrict__ item_off,
                                                     const double* __restrict__ px, const double* __restrict__ subs,
                                                     const uint8_t* __restrict__ codes, int K, int h, int phase, int nq,
                                                     uint64_t* __restrict__ keys, uint64_t* __restrict__ vals,
                                                     unsigned long long* __restrict__ qmin, unsigned long long* __restrict__ qmax) {
    extern __shared__ __align__(16) double s_sub[];  // [JP][K][W], then the item starts of the current query
    int* s_start = reinterpret_cast<int*>(s_sub + (size_t)JP * K * W);
    constexpr int nf = MT / 2;
    constexpr int NPH = MT / JP;
    const int j0 = phase * JP;
    {
        const double2* src = reinterpret_cast<const double2*>(subs + (size_t)j0 * K * W);
        double2* dst = reinterpret_cast<double2*>(s_sub);
        for (int i = threadIdx.x; i < JP * K * W / 2; i += 1024) dst[i] = src[i];
    }
    const bool last = phase == NPH - 1;
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const int64_t it0 = item_off[q], it1 = item_off[q + 1];
        const int64_t c0 = seg[q], c1 = seg[q + 1];
        const int ni = (int)(it1 - it0);
        const int64_t n = c1 - c0;
        const bool staged = ni <= FLAT_ITEMS;
        __syncthreads();  // the previous query's starts are no longer read (and the sub-quantizers are in place)
        if (staged)
            for (int i = threadIdx.x; i < ni; i += 1024) s_start[i] = (int)(cand_start[it0 + i] - c0);
        __syncthreads();
        uint64_t mn = ~0ull, mx = 0ull;
        for (int64_t c = threadIdx.x; c < n; c += 1024) {
            int lo = 0, hi = ni;  // first item whose start is > c; the item before it holds c
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const int64_t st_ = staged ? (int64_t)s_start[mid] : cand_start[it0 + mid] - c0;
                if (st_ <= c) lo = mid + 1;
                else hi = mid;
            }
            const int i = lo - 1;
            const WorkItem it = items[it0 + i];
            const int p = (int)(c - (staged ? (int64_t)s_start[i] : cand_start[it0 + i] - c0));
            const CodeWords<MT> cw = load_code<MT>(codes, it.start + p);
            double d = phase == 0 ? 0.0 : __longlong_as_double((long long)keys[c0 + c]);
#pragma unroll
            for (int jj = 0; jj < JP; ++jj) {
                const int j = j0 + jj;
                const bool second = j >= nf;
                const double* f = px + (int64_t)(second ? it.tab1 : it.tab0) * h + (second ? j - nf : j) * W;
                const uint32_t code = (cw.w[j >> 2] >> (8 * (j & 3))) & 255u;
                const double* sc = s_sub + ((size_t)jj * K + code) * W;
                auto elem = [&](int e) -> double { const double df = f[e] - sc[e]; return df * df; };
                const double v = pw_leaf<double>(elem, 0, W);
                d = (phase == 0 && jj == 0) ? v : d + v;
            }
            const uint64_t kk = (uint64_t)__double_as_longlong(d);
            keys[c0 + c] = kk;
            if (last) {
                mn = kk < mn ? kk : mn;
                mx = kk > mx ? kk : mx;
                if (vals) vals[c0 + c] = ((uint64_t)(it0 + i) << 32) | (uint32_t)p;
            }
        }
        if (last && qmin) publish_key_range(mn, mx, qmin, qmax, q);
    }
}

// sub-quantizers per phase of the direct form: the largest divisor of M whose float64 centroids fit 128 KB of LDS; 0 = not served
static int direct_jp(int M, int K, int w) {
    if (!(M == 4 || M == 8 || M == 16) || K > 256 || K % 2 != 0 || !(w == 4 || w == 8 || w == 16 || w == 32)) return 0;
    return M < 64 / w ? M : 64 / w;  // sized for K = 256 (the instantiated set below)
}

template <int MT, int W, int JP>
static void launch_adc_direct_t(const CandArgs& c, const double* px, const double* subs, int h, uint64_t* keys, uint64_t* vals) {
    const size_t lds = (size_t)JP * c.K * W * sizeof(double) + (size_t)FLAT_ITEMS * sizeof(int);
    const unsigned grid = (unsigned)(c.nq < 256 ? c.nq : 256);
    for (int ph = 0; ph < MT / JP; ++ph)
        hipLaunchKernelGGL((k_adc_direct<MT, W, JP>), dim3(grid), dim3(1024), lds, c.st, c.items, c.cand_start, c.seg, c.item_off, px, subs, c.codes, c.K, h,
                           ph, c.nq, keys, vals, c.qmin, c.qmax);
}

static bool launch_adc_direct(int M, int w, const CandArgs& c, const double* px, const double* subs, int h, uint64_t* keys, uint64_t* vals) {
    const int jp = direct_jp(M, c.K, w);
#define CIS_DIRECT(MT, W, JP) if (M == MT && w == W && jp == JP) return launch_adc_direct_t<MT, W, JP>(c, px, subs, h, keys, vals), true;
    // K = 256: 128 KB hold 64 / w sub-quantizers
    CIS_DIRECT(8, 16, 4) CIS_DIRECT(16, 16, 4) CIS_DIRECT(4, 16, 4) CIS_DIRECT(8, 8, 8) CIS_DIRECT(16, 8, 8) CIS_DIRECT(4, 8, 4)
    CIS_DIRECT(4, 32, 2) CIS_DIRECT(8, 32, 2) CIS_DIRECT(16, 32, 2) CIS_DIRECT(4, 4, 4) CIS_DIRECT(8, 4, 8) CIS_DIRECT(16, 4, 16)
#undef CIS_DIRECT
    return false;
}

// every candidate's exact key from the float64 tables: a workgroup row per query that finds its items itself (flat: tiny cells, exact totals),
// else eight workgroups per work item
static void launch_adc_all(const CandArgs& c, const double* T, int M, uint64_t* keys, uint64_t* vals, const int64_t* d_totals, bool flat) {
    const bool m_lds = c.K <= 256 && (M == 4 || M == 8 || M == 16);  // the table of one work item in LDS, code bytes unpacked at compile time
    if (flat && c.nq > 0 && !d_totals) {
        dispatch_int<0, 4, 8, 16>(m_lds ? M : 0, [&](auto m) {
            hipLaunchKernelGGL(k_adc_all_flat<decltype(m)::value>, dim3((unsigned)c.nq, 8), dim3(256), 0, c.st, c.items, c.cand_start, c.seg, c.item_off, T, c.codes, M, c.K,
                               keys, vals, c.qmin, c.qmax);
        });
        return;
    }
    const dim3 g((unsigned)c.n_items, 8);
    if (m_lds)
        dispatch_int<4, 8, 16>(M, [&](auto m) {
            hipLaunchKernelGGL(k_adc_all_lds<decltype(m)::value>, g, dim3(256), (size_t)M * c.K * sizeof(double), c.st, c.items, c.cand_start, T, c.codes, c.K, keys, vals,
                               c.qmin, c.qmax, d_totals);
        });
    else hipLaunchKernelGGL(k_adc_all, g, dim3(256), 0, c.st, c.items, c.cand_start, T, c.codes, M, c.K, keys, vals, c.qmin, c.qmax, d_totals);
}

__global__ void k_emit_sorted(const uint64_t* __restrict__ keys, const uint64_t* __restrict__ vals, const int64_t* __restrict__ seg,
                              const int* __restrict__ nsel, int64_t stride,
                              const WorkItem* __restrict__ items, const int64_t* __restrict__ ids, int nq, int limit,
                              cis_hit* __restrict__ out_hits, int64_t* __restrict__ out_ids, double* __restrict__ out_dists,
                              int* __restrict__ out_n, int32_t* __restrict__ out_cells, uint32_t* __restrict__ out_pos) {
    const int q = blockIdx.y;
    // segments: contiguous (seg[q] .. seg[q + 1]) or, after the selection kernel, nsel[q] entries at q * stride
    const int64_t a = nsel ? (int64_t)q * stride : seg[q], n = nsel ? (int64_t)nsel[q] : seg[q + 1] - a;
    const int nv = (int)(n < limit ? n : limit);
    const int64_t o = (int64_t)q * limit;
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < limit; x += gridDim.x * blockDim.x) {
        cis_hit hh;
        hh.dist = __longlong_as_double(0x7ff0000000000000LL);
        hh.visit_rank = 0xffffffffu; hh.pos = 0xffffffffu; hh.id = -1; hh.cell = -1; hh.reserved = 0;
        if (x < nv) {
            const uint64_t v = vals[a + x];
            const WorkItem it = items[v >> 32];
            const uint32_t p = (uint32_t)v;
            hh.dist = __longlong_as_double((long long)keys[a + x]);
            hh.visit_rank = (uint32_t)it.rank;
            hh.pos = (uint32_t)it.pos0 + p;
            hh.id = ids[it.start + p];
            hh.cell = it.cell;
        }
        if (out_hits) out_hits[o + x] = hh;
        if (out_ids) {
            out_ids[o + x] = hh.id;
            out_dists[o + x] = (x < nv) ? hh.dist : __longlong_as_double(0x7ff8000000000000LL);
        }
        if (out_cells) out_cells[o + x] = hh.cell;
        if (out_pos) out_pos[o + x] = hh.pos;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && out_n) out_n[q] = nv;
}


// ---- `limit` between the float32-prefilter kernel's 440 and the candidate count: radix SELECT before any sort.
// k_adc_all has written the exact float64 distance of every candidate in retrieval order (keys; positive doubles
// order like their bit patterns).  One workgroup per query finds the `limit`-th smallest (distance, retrieval index)
// pair -- the cut of the reference's stable sorted()[:limit] (search.py:210-216):
//   A. min / max of the segment -> the bits all keys share are skipped;
//   B. most-significant-digit radix passes (11 bits, LDS histogram) narrow to the bin holding the limit-th key until
//      that bin has <= SEL_CAND keys (or every bit is fixed: a crowd of exact ties);
//   C. the bin's keys are sorted in LDS by (key, index) and the r-th is the cut; for a crowd of ties the cut index is
//      found by counting equal keys in retrieval order;
//   D. an ORDER-PRESERVING gather of everything <= cut (block prefix sums): exactly min(n, limit) pairs in retrieval
//      order.  limit <= 3072: sorted in LDS by (key, index) and written ranked; above: written in retrieval order for
//      the stable segmented sort, which now sees limit instead of n entries per query.
static const int SEL_THREADS = 1024;  // largest workgroup of the selection kernel (small batches); large batches use 512
static const int SEL_BITS = 11;
static const int SEL_CAND = 1024;
static const int SEL_PER = 4;  // consecutive keys per thread and chunk in the ordered passes

__device__ __forceinline__ int sel_wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// exclusive prefix of v over the workgroup and the total; sm: one int per wave (contains two barriers)
__device__ __forceinline__ int sel_block_excl_scan(int v, int* sm, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int inc = sel_wave_incl_scan(v);
    __syncthreads();
    if (lane == 63) sm[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const int x = sm[i];
        if (i < w) base += x;
        tot += x;
    }
    *total = tot;
    return base + inc - v;
}

__device__ __forceinline__ bool sel_pair_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
    return ka < kb || (ka == kb && ia < ib);
}

// ascending bitonic sort of n2 (power of two) (key, index) pairs in LDS by the whole workgroup
__device__ __forceinline__ void sel_block_bitonic(uint64_t* key, uint32_t* idx, int n2) {
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < (n2 >> 1); t += blockDim.x) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const bool up = (lo & k) == 0;
                const uint64_t ka = key[lo], kb = key[hi];
                const uint32_t ia = idx[lo], ib = idx[hi];
                if (sel_pair_less(kb, ib, ka, ia) == up) {
                    key[lo] = kb; key[hi] = ka;
                    idx[lo] = ib; idx[hi] = ia;
                }
            }
        }
    __syncthreads();
}

// the candidate reference (work item << 32 | offset in the item's cell) of retrieval index g (global over the batch)
__device__ __forceinline__ uint64_t sel_val_of(int64_t g, const int64_t* __restrict__ cand_start, int64_t it_lo, int64_t it_hi) {
    while (it_hi - it_lo > 1) {  // last item with cand_start <= g
        const int64_t mid = (it_lo + it_hi) >> 1;
        if (cand_start[mid] <= g) it_lo = mid; else it_hi = mid;
    }
    return ((uint64_t)it_lo << 32) | (uint32_t)(g - cand_start[it_lo]);
}

struct SelShared {
    int bin, less, cnt, cn, on;
    unsigned int cut_idx;
    int wsum[SEL_THREADS / 64];
};

template <bool SORT_LDS, int NT>
__global__ __launch_bounds__(NT) void k_select_topl(const uint64_t* __restrict__ keys, const int64_t* __restrict__ seg,
                                                              const int64_t* __restrict__ cand_start, const int64_t* __restrict__ item_off,
                                                              const unsigned long long* __restrict__ qmin,
                                                              const unsigned long long* __restrict__ qmax, int64_t n_items, int L, int P2,
                                                              int64_t stride, uint64_t* __restrict__ sel_keys,
                                                              uint64_t* __restrict__ sel_vals, int* __restrict__ nsel,
                                                              int64_t* __restrict__ seg_b, int64_t* __restrict__ seg_e,
                                                              const int* __restrict__ only = nullptr /* ranked: flagged queries only */,
                                                              // INDIRECT (the streaming route, SORT_LDS only): the keys of query q are kcnt[q] (<= kstride) entries at
                                                              // q * kstride in arbitrary order, entry i is the candidate of retrieval index rid[q * kstride + i]
                                                              // (relative to seg[q]) -- ties are broken by THAT index, as the stable sort of search.py:210 does
                                                              const uint32_t* __restrict__ rid = nullptr, const int* __restrict__ kcnt = nullptr,
                                                              int64_t kstride = 0) {
    if (only && !only[blockIdx.x]) return;
    extern __shared__ __align__(16) unsigned char sel_lds[];
    // LDS: [okey P2][oidx P2] (SORT_LDS) | union { hist 2048 u32 ; ckey 1024 u64 + cidx 1024 u32 } | SelShared
    uint64_t* okey = reinterpret_cast<uint64_t*>(sel_lds);
    uint32_t* oidx = reinterpret_cast<uint32_t*>(okey + (SORT_LDS ? P2 : 0));
    unsigned char* un = reinterpret_cast<unsigned char*>(oidx + (SORT_LDS ? P2 : 0));
    unsigned int* hist = reinterpret_cast<unsigned int*>(un);
    uint64_t* ckey = reinterpret_cast<uint64_t*>(un);
    uint32_t* cidx = reinterpret_cast<uint32_t*>(ckey + SEL_CAND);
    SelShared* sh = reinterpret_cast<SelShared*>(un + SEL_CAND * 12);
    const int q = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int64_t fa = seg[q];                           // retrieval index of the query's first candidate
    const int64_t a = rid ? (int64_t)q * kstride : fa;   // where the query's keys start
    const int64_t n64 = rid ? (int64_t)(kcnt[q] < kstride ? kcnt[q] : (int)kstride) : seg[q + 1] - a;
    const unsigned int n = (unsigned int)n64;  // a query's candidates fit 32 bits (the batch total does)
    const uint64_t* __restrict__ k = keys + a;
    const uint32_t* __restrict__ ridq = rid ? rid + a : nullptr;
    auto idx_of = [&](unsigned int i) -> uint32_t { return ridq ? ridq[i] : i; };  // the tie-breaking index of key i
    const int nv = n64 < (int64_t)L ? (int)n64 : L;
    uint64_t cut_key = ~0ull;
    unsigned int cut_idx = 0xffffffffu;
    bool gathered = false;  // SORT_LDS: the list is already in LDS (unordered)
    if (n64 > (int64_t)L) {
        // A. range of the keys: published by the distance kernel
        const uint64_t mn = qmin[q], mx = qmax[q];
        int hi_shift = (mn == mx) ? 0 : 64 - __clzll((long long)(mn ^ mx));  // bits [0, hi_shift) differ somewhere
        uint64_t prefix = hi_shift >= 64 ? 0ull : (mn >> hi_shift);
        int r = L;            // rank (1-based) of the cut among the keys that share `prefix`
        unsigned int c = n;   // keys that share `prefix`
        // B. radix passes
        while (hi_shift > 0 && c > (unsigned)SEL_CAND) {
            const int bits = hi_shift < SEL_BITS ? hi_shift : SEL_BITS;
            const int shift = hi_shift - bits;
            const unsigned int mask = (1u << bits) - 1u;
            for (int b = tid; b < (1 << SEL_BITS); b += nt) hist[b] = 0;
            __syncthreads();
#pragma unroll 4
            for (unsigned int i = tid; i < n; i += nt) {
                const uint64_t v = k[i];
                if (hi_shift >= 64 || (v >> hi_shift) == prefix) atomicAdd(&hist[(unsigned int)(v >> shift) & mask], 1u);
            }
            __syncthreads();
            constexpr int per = (1 << SEL_BITS) / NT;
            unsigned int cb[per];
            int local = 0;
#pragma unroll
            for (int j = 0; j < per; ++j) { cb[j] = hist[tid * per + j]; local += (int)cb[j]; }
            int tot;
            int run = sel_block_excl_scan(local, sh->wsum, &tot);
#pragma unroll
            for (int j = 0; j < per; ++j) {
                if (run < r && r <= run + (int)cb[j]) { sh->bin = tid * per + j; sh->less = run; sh->cnt = (int)cb[j]; }
                run += (int)cb[j];
            }
            __syncthreads();
            r -= sh->less;
            c = (unsigned int)sh->cnt;
            prefix = (prefix << bits) | (uint64_t)sh->bin;
            hi_shift = shift;
            __syncthreads();
        }
        if (c <= (unsigned)SEL_CAND) {
            // C. the threshold bin's keys, ranked in LDS
            if (tid == 0) { sh->cn = 0; sh->on = 0; }
            __syncthreads();
#pragma unroll 4
            for (unsigned int i = tid; i < n; i += nt) {
                const uint64_t v = k[i];
                const uint64_t hv = hi_shift >= 64 ? 0ull : (v >> hi_shift);
                if (hv == prefix) {
                    const int j = atomicAdd(&sh->cn, 1);
                    ckey[j] = v;
                    cidx[j] = idx_of(i);
                } else if (SORT_LDS && hv < prefix) {  // below the threshold bin: in, whatever the order (ranked in LDS below)
                    const int j = atomicAdd(&sh->on, 1);
                    okey[j] = v;
                    oidx[j] = idx_of(i);
                }
            }
            __syncthreads();
            int c2 = 64;
            while (c2 < (int)c) c2 <<= 1;
            for (int j = (int)c + tid; j < c2; j += nt) { ckey[j] = ~0ull; cidx[j] = 0xffffffffu; }
            sel_block_bitonic(ckey, cidx, c2);
            cut_key = ckey[r - 1];
            cut_idx = cidx[r - 1];
            if (SORT_LDS) {  // the first r of the bin complete the list
                const int on = sh->on;
                for (int j = tid; j < r; j += nt) { okey[on + j] = ckey[j]; oidx[on + j] = cidx[j]; }
                gathered = true;
            }
            __syncthreads();
        } else if (rid) {
            // INDIRECT: a crowd of more than SEL_CAND exact ties at the cut is not resolved here -- the query reports no result and
            // the streaming route's verification sends it to the generic path
            if (tid == 0) nsel[q] = 0;
            return;
        } else {
            // a crowd of exact ties at the cut (every bit fixed): the first r of them in retrieval order
            cut_key = prefix;
            int base = 0;
            for (unsigned int i0 = 0; i0 < n; i0 += (unsigned)nt) {
                const unsigned int i = i0 + tid;
                const int f = (i < n && k[i] == cut_key) ? 1 : 0;
                int tot;
                const int ex = sel_block_excl_scan(f, sh->wsum, &tot);
                if (f && base + ex == r - 1) sh->cut_idx = i;
                base += tot;
                if (base >= r) break;
            }
            __syncthreads();
            cut_idx = sh->cut_idx;
            __syncthreads();
        }
    }
    // D. order-preserving gather of the pairs <= cut
    const int64_t it_lo = item_off[q];
    int64_t it_hi = item_off[q + 1];
    if (it_hi > n_items) it_hi = n_items;
    const int64_t ob = (int64_t)q * stride;
    int base = 0;
    if (!gathered)
    for (unsigned int i0 = 0; i0 < n && base < nv; i0 += (unsigned)(nt * SEL_PER)) {
        const unsigned int i = i0 + tid * SEL_PER;
        uint64_t v[SEL_PER];
        int f[SEL_PER], local = 0;
#pragma unroll
        for (int j = 0; j < SEL_PER; ++j) {
            v[j] = (i + j < n) ? k[i + j] : 0ull;
            f[j] = (i + j < n) && (v[j] < cut_key || (v[j] == cut_key && (ridq ? ridq[i + j] : i + j) <= cut_idx));
            local += f[j];
        }
        int tot;
        int o = base + sel_block_excl_scan(local, sh->wsum, &tot);
#pragma unroll
        for (int j = 0; j < SEL_PER; ++j)
            if (f[j]) {
                if (SORT_LDS) {
                    okey[o] = v[j];
                    oidx[o] = idx_of(i + j);
                } else {
                    sel_keys[ob + o] = v[j];
                    sel_vals[ob + o] = sel_val_of(a + i + j, cand_start, it_lo, it_hi);
                }
                ++o;
            }
        base += tot;
    }
    if (SORT_LDS) {
        __syncthreads();
        int n2 = 64;
        while (n2 < nv) n2 <<= 1;
        for (int j = nv + tid; j < n2; j += nt) { okey[j] = ~0ull; oidx[j] = 0xffffffffu; }
        sel_block_bitonic(okey, oidx, n2);
        for (int j = tid; j < nv; j += nt) {
            sel_keys[ob + j] = okey[j];
            sel_vals[ob + j] = sel_val_of(fa + oidx[j], cand_start, it_lo, it_hi);
        }
    }
    if (tid == 0) {
        nsel[q] = nv;
        if (seg_b) { seg_b[q] = ob; seg_e[q] = ob + nv; }
    }
}


// how the all-candidates path ranks: select (k_select_topl) when it shrinks the sort, LDS-ranked for limit <= 3072
struct SelectPlan { bool select, sort_lds; int64_t stride; int p2; size_t lds; };
static SelectPlan select_plan(int L, int nq, int64_t n_cand) {
    SelectPlan sp;
    sp.stride = (int64_t)L < n_cand ? (int64_t)L : (n_cand > 0 ? n_cand : 1);
    sp.sort_lds = L <= MAX_LDS_LIMIT;
    sp.select = sp.sort_lds || (double)nq * (double)sp.stride <= 0.5 * (double)n_cand;
    if (getenv("CIS_NO_SELECT")) sp.select = sp.sort_lds = false;  // experiments: the full segmented sort
    if (!sp.select) sp.sort_lds = false;
    sp.p2 = 64;
    while (sp.p2 < L && sp.sort_lds) sp.p2 <<= 1;
    sp.lds = (sp.sort_lds ? (size_t)sp.p2 * 12 : 0) + (size_t)SEL_CAND * 12 + sizeof(SelShared) + 16;
    return sp;
}

// limit above the float32-prefilter kernel's 440: rank through the all-candidates path (the LDS top-k kernel of the exact
// scan holds up to 3072 but slows down steeply with limit)
// Largest batch at which the all-candidates path beats the float32-prefilter scan for limit <= 440 (measured with
// tools/bench_limits.py on the bench index, 40 k candidates per query): a small batch has too few (query, cell) work items
// to fill the persistent scan kernel, and its per-wave regions grow with limit, while scoring every candidate with one
// workgroup per 2048 of them and selecting per query costs the same 0.18-0.4 ms whatever the limit.
static int small_batch_nq(int L) {
    static const int forced = getenv("CIS_SMALL_NQ") ? atoi(getenv("CIS_SMALL_NQ")) : -1;  // experiments
    if (forced >= 0) return forced;
    if (L <= 184) return 63;
    if (L <= 300) return 256;
    return 512;
}

// thousands of coarse clusters: cells of a few codes each (the release configurations' V = 2048 / 4096)
static bool index_has_tiny_cells(const cis_index* ix) {
    return ix->nonempty_cells > 0 && ix->n_total / ix->nonempty_cells < 64;
}

static bool use_all_path(const cis_index* ix, int M, int K, int L, int nq) {
    if (L > MAX_LDS_LIMIT) return true;
    if (ix->force_exact_scan) return false;
    if (L > SCAN2_MAX_LIMIT) return true;
    // a scan workgroup per (query, cell) slot stages 16 KB of tables and a survivor list per work item: hopeless for cells of
    // a few codes -- every candidate's exact distance + a per-query select instead (unless a test forces a scan kernel)
    if (index_has_tiny_cells(ix) && !ix->force_prefilter_scan) return true;
    return !ix->force_prefilter_scan && nq <= small_batch_nq(L);
}

// ---- tiny cells, prefiltered (round 3): the release operating point (V = 2048 / 4096: a query visits hundreds of cells of a
// few codes each, ~10 k candidates for the 100 it returns) -----------------------------------------------------------------
// k_adc_direct computes the exact float64 distance of EVERY candidate (128 subtract-square-adds on operands gathered from LDS
// and L2: 5.8 of the 11.4 ms of an 8192-query batch) and k_select_topl then reads all keys back.  Here one workgroup per query
//   1. lays the query's candidates out in LDS (its work items, the owner item of every candidate, the half tables that have a
//      candidate at all, numbered densely);
//   2. estimates a cap on the limit-th best distance from 128 sampled candidates;
//   3. builds the query's distance tables as BYTES in LDS -- entry = min(255, floor(e / step)), step = cap / 256, e computed in
//      float32 from the projected residuals px (k_tables_group leaves a float32 copy; rows arrive through scalar loads) -- one
//      split and at most `tch` tables at a time, and adds every candidate's table bytes up (a lower bound of its distance in
//      steps: floor and min only round down);
//   4. histograms the sums: s* = the smallest sum that `limit` candidates reach; a candidate whose sum is <= 254 has no clamped
//      entry, so its distance is below (sum + M) steps, hence the limit-th best distance T < (s* + M) steps, and a candidate
//      can only be among the best `limit` if sum <= s* + M (+ 1 bin for the float32 rounding of e, which the cap test below
//      keeps under a sixteenth of a step per entry);
//   5. computes the exact float64 keys of those survivors only -- the expression, operands and summation order of
//      k_adc_direct, so the same bits -- ranks them by (key, retrieval position) by counting and writes the best `limit` in the
//      format of k_select_topl<true>.
// A query for which no bound comes out (fewer than `limit` candidates under the cap, survivors beyond the LDS list, more
// candidates than the layout holds, a cap too small for float32) gets every candidate's exact key written to the global key
// array and a flag; k_select_topl runs afterwards on the flagged queries alone.  Results are those of the exact path, bit for bit.
static const int TINY_NS = 128;     // sampled candidates per query (eight threads each)
static const int TINY_SMAX = 1024;  // survivors ranked in LDS
static const int TINY_NCMAX = 16384;
static const int TINY_TCH = 128;    // tables per chunk at most

struct TinyShared {
    int cnt, sstar, fb, nused[2];
    unsigned int cap_bits, amax_bits, cen_bits;
    int wsum[16];
};

template <int MT, int W>
__device__ __noinline__ void tiny_exact_all(const WorkItem* __restrict__ items, const int64_t* __restrict__ cand_start,
                                            const double* __restrict__ px, const double* __restrict__ subs,
                                            const uint8_t* __restrict__ codes, int h, int64_t it0, int ni, int64_t c0, int64_t n64,
                                            uint64_t* __restrict__ keys_fb,
                                            unsigned long long* __restrict__ qmin, unsigned long long* __restrict__ qmax, int q) {
    constexpr int NF = MT / 2, K = 256;
    uint64_t mn = ~0ull, mx = 0ull;
    for (int64_t c = threadIdx.x; c < n64; c += 1024) {
        int lo = 0, hi = ni;  // the item that holds candidate c
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cand_start[it0 + mid] - c0 <= c) lo = mid + 1; else hi = mid;
        }
        const int i = lo - 1;
        const WorkItem it = items[it0 + i];
        const int p = (int)(c - (cand_start[it0 + i] - c0));
        const CodeWords<MT> cw = load_code<MT>(codes, it.start + p);
        double d = 0.0;
        for (int j = 0; j < MT; ++j) {
            const bool second = j >= NF;
            const double* f = px + (int64_t)(second ? it.tab1 : it.tab0) * h + (second ? j - NF : j) * W;
            const uint32_t code = (cw.w[j >> 2] >> (8 * (j & 3))) & 255u;
            const double* sc = subs + ((size_t)j * K + code) * W;
            auto elem = [&](int e) -> double { const double df = f[e] - sc[e]; return df * df; };
            const double v = pw_leaf<double>(elem, 0, W);
            d = j == 0 ? v : d + v;
        }
        const uint64_t kk = (uint64_t)__double_as_longlong(d);
        keys_fb[c0 + c] = kk;
        mn = kk < mn ? kk : mn;
        mx = kk > mx ? kk : mx;
    }
    publish_key_range(mn, mx, qmin, qmax, q);
}

// Two rows of W float32 at wave-uniform addresses, through the scalar cache into SGPRs: one wait for both (the compiler keeps
// uniform loads of a kernel that also writes global memory on the vector path -- 1 KB of identical lanes per instruction)
typedef int tiny_i16v __attribute__((ext_vector_type(16)));
typedef int tiny_i8v __attribute__((ext_vector_type(8)));
typedef int tiny_i4v __attribute__((ext_vector_type(4)));
// rows per wait: a wave's table loop is bound by the latency of these loads (L2: the rows were just written), not by arithmetic
template <int W> struct TinyRows { static constexpr int U = W <= 16 ? 4 : 2; };
template <int W>
__device__ __forceinline__ void tiny_sload_rows(const float* const (&p)[TinyRows<W>::U], float (&f)[TinyRows<W>::U][W]) {
    if constexpr (W == 4) {
        tiny_i4v a, b, c, d;
        asm volatile("s_load_dwordx4 %0, %4, 0x0\n\ts_load_dwordx4 %1, %5, 0x0\n\ts_load_dwordx4 %2, %6, 0x0\n\ts_load_dwordx4 %3, %7, 0x0\n\t"
                     "s_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d) : "s"(p[0]), "s"(p[1]), "s"(p[2]), "s"(p[3]) : "memory");
#pragma unroll
        for (int e = 0; e < 4; ++e) { f[0][e] = __int_as_float(a[e]); f[1][e] = __int_as_float(b[e]); f[2][e] = __int_as_float(c[e]); f[3][e] = __int_as_float(d[e]); }
    } else if constexpr (W == 8) {
        tiny_i8v a, b, c, d;
        asm volatile("s_load_dwordx8 %0, %4, 0x0\n\ts_load_dwordx8 %1, %5, 0x0\n\ts_load_dwordx8 %2, %6, 0x0\n\ts_load_dwordx8 %3, %7, 0x0\n\t"
                     "s_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d) : "s"(p[0]), "s"(p[1]), "s"(p[2]), "s"(p[3]) : "memory");
#pragma unroll
        for (int e = 0; e < 8; ++e) { f[0][e] = __int_as_float(a[e]); f[1][e] = __int_as_float(b[e]); f[2][e] = __int_as_float(c[e]); f[3][e] = __int_as_float(d[e]); }
    } else if constexpr (W == 16) {
        tiny_i16v a, b, c, d;
        asm volatile("s_load_dwordx16 %0, %4, 0x0\n\ts_load_dwordx16 %1, %5, 0x0\n\ts_load_dwordx16 %2, %6, 0x0\n\ts_load_dwordx16 %3, %7, 0x0\n\t"
                     "s_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d) : "s"(p[0]), "s"(p[1]), "s"(p[2]), "s"(p[3]) : "memory");
#pragma unroll
        for (int e = 0; e < 16; ++e) { f[0][e] = __int_as_float(a[e]); f[1][e] = __int_as_float(b[e]); f[2][e] = __int_as_float(c[e]); f[3][e] = __int_as_float(d[e]); }
    } else {
        tiny_i16v a, b, c, d;
        asm volatile("s_load_dwordx16 %0, %4, 0x0\n\ts_load_dwordx16 %1, %4, 0x40\n\ts_load_dwordx16 %2, %5, 0x0\n\ts_load_dwordx16 %3, %5, 0x40\n\t"
                     "s_waitcnt lgkmcnt(0)" : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d) : "s"(p[0]), "s"(p[1]) : "memory");
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            f[0][e] = __int_as_float(a[e]); f[0][16 + e] = __int_as_float(b[e]);
            f[1][e] = __int_as_float(c[e]); f[1][16 + e] = __int_as_float(d[e]);
        }
    }
}

// Touch the first dword of four rows (no wait): the lines are in the scalar cache when tiny_sload_rows asks for them an iteration
// later.  The destination registers stay reserved until then -- the loads land asynchronously -- by passing through tiny_keep.
__device__ __forceinline__ void tiny_prefetch4(const float* p0, const float* p1, const float* p2, const float* p3, int (&pf)[4]) {
    asm volatile("s_load_dword %0, %4, 0x0\n\ts_load_dword %1, %5, 0x0\n\ts_load_dword %2, %6, 0x0\n\ts_load_dword %3, %7, 0x0"
                 : "=&s"(pf[0]), "=&s"(pf[1]), "=&s"(pf[2]), "=&s"(pf[3]) : "s"(p0), "s"(p1), "s"(p2), "s"(p3) : "memory");
}
__device__ __forceinline__ void tiny_keep(int (&pf)[4]) {  // placed right after the next wait: until here the registers are taken
    asm volatile("" : "+s"(pf[0]), "+s"(pf[1]), "+s"(pf[2]), "+s"(pf[3]));
}

struct TinyItem {       // a work item of the current query, staged in LDS
    uint32_t start;     // first candidate (position in codes/ids): the index holds fewer than 2^32 items, or the query is flagged
    uint16_t rel, len;  // first candidate inside the query's candidate range, candidates
    uint16_t t0, t1;    // the two half tables, counted from the query's first table of that split
};

template <int MT, int W>
__global__ __launch_bounds__(1024) void k_tiny_select(const WorkItem* __restrict__ items, const int64_t* __restrict__ cand_start,
                                                      const int64_t* __restrict__ seg, const int64_t* __restrict__ item_off,
                                                      const int64_t* __restrict__ tab_off, const PlanOut* __restrict__ plan,
                                                      const double* __restrict__ px, const double* __restrict__ subs,
                                                      const uint8_t* __restrict__ codes, int h, int nq, int L, int ncmax, int pool_bytes,
                                                      int64_t stride, uint64_t* __restrict__ sel_keys, uint64_t* __restrict__ sel_vals,
                                                      int* __restrict__ nsel, uint64_t* __restrict__ keys_fb,
                                                      unsigned long long* __restrict__ qmin, unsigned long long* __restrict__ qmax,
                                                      int* __restrict__ fbflag, const float* __restrict__ px32 /* [ntab][h]: float32 copy of px */,
                                                      unsigned int* __restrict__ dbg) {
    constexpr int NF = MT / 2, K = 256;
    constexpr int PAIRS = NF * K;
    constexpr int PPT = (PAIRS + 1023) / 1024;
    constexpr int CW = NF >= 4 ? NF / 4 : 1;
    extern __shared__ __align__(16) unsigned char tiny_lds[];
    uint16_t* own = reinterpret_cast<uint16_t*>(tiny_lds);
    uint16_t* sum = own + ncmax;
    unsigned char* pool = tiny_lds + (size_t)4 * ncmax;    // items | tables + px of a chunk, later the survivors' exact entries
    TinyItem* s_items = reinterpret_cast<TinyItem*>(pool);
    unsigned int* hist = reinterpret_cast<unsigned int*>(pool + pool_bytes);  // 512 bins
    float* samp = reinterpret_cast<float*>(hist + 512);                    // TINY_NS
    uint64_t* skey = reinterpret_cast<uint64_t*>(samp + TINY_NS);          // TINY_SMAX
    uint32_t* sidx = reinterpret_cast<uint32_t*>(skey + TINY_SMAX);        // TINY_SMAX
    TinyShared* sh = reinterpret_cast<TinyShared*>(sidx + TINY_SMAX);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __builtin_amdgcn_s_dcache_inv();  // the scalar cache may hold rows of an earlier batch at the addresses of px32
    long long t_last = dbg ? wall_clock64() : 0;
#define TINY_T(k_) do { if (dbg && tid == 0) { const long long now_ = wall_clock64(); atomicAdd(&dbg[4 + (k_)], (unsigned int)(now_ - t_last)); t_last = now_; } } while (0)
    // largest centroid component (float32 rounding bound), once per workgroup
    if (tid == 0) sh->cen_bits = 0u;
    __syncthreads();
    {
        float a = 0.f;
        for (int i = tid; i < MT * K * W; i += 1024) a = fmaxf(a, fabsf((float)subs[i]));
        atomicMax(&sh->cen_bits, __float_as_uint(a));
    }
    // the thread's (sub-quantizer, centroid) of BOTH splits stays in registers over the persistent loop when that is 32 floats or fewer
    // (M = 8, w = 16: the release shape; loading them per chunk cost 9 us of a 105 us query)
    constexpr bool KEEP = PPT * W <= 16;
    float cenk[2][KEEP ? PPT : 1][KEEP ? W : 1];
    if constexpr (KEEP) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int pp = 0; pp < PPT; ++pp) {
                const int pr = tid + pp * 1024;
                const double* sc = subs + ((size_t)(s2 * NF + (pr < PAIRS ? pr / K : 0)) * K + pr % K) * W;
#pragma unroll
                for (int e = 0; e < W; ++e) cenk[s2][pp][e] = (float)sc[e];
            }
    }
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        const int64_t it0 = item_off[q];
        const int ni = (int)(item_off[q + 1] - it0);
        const int64_t c0 = seg[q];
        const int64_t n64 = seg[q + 1] - c0;
        const int nv = n64 < (int64_t)L ? (int)n64 : L;
        const int64_t ob = (int64_t)q * stride;
        __syncthreads();  // the previous query's lists are no longer read
        TINY_T(0);
        if (n64 <= 0) {
            if (tid == 0) { nsel[q] = 0; fbflag[q] = 0; }
            continue;
        }
        // this query's share of the pool: its items first, the rest for tables (or the survivors' entries)
        const int ntt = plan[q].ntab0 + plan[q].ntab1;
        const int list_off = (ni * (int)sizeof(TinyItem) + 15) & ~15;           // uint16 used[ntt]: the half tables that have a candidate
        const int items_bytes = list_off + ((ntt * 2 + 15) & ~15);               // (items + lists: what stays for the whole query)
        uint16_t* used = reinterpret_cast<uint16_t*>(pool + list_off);          // split 0's list, then split 1's at used + nt0
        const int rest = pool_bytes - items_bytes;
        int tch = rest > 0 ? rest / (NF * K) : 0;
        tch = tch < TINY_TCH ? tch : TINY_TCH;
        int smax = rest > 0 ? rest / (8 * MT) : 0;
        smax = smax < TINY_SMAX ? smax : TINY_SMAX;
        uint8_t* s_tab = pool + items_bytes;
        double* e_lds = reinterpret_cast<double*>(pool + items_bytes);
        bool fall = n64 > (int64_t)ncmax || ni > 65535 || ntt > 4096 || tch < 4 || L > smax;
        const int n = (int)n64;
        const bool all_in = !fall && n <= smax && n <= (2 * L > 256 ? 2 * L : 256);  // few candidates: every one is ranked exactly
        int nsurv = 0;
        if (!fall) {
            if (tid == 0) { sh->cnt = 0; sh->sstar = 1 << 20; sh->amax_bits = 0u; sh->cap_bits = 0u; sh->fb = 0; }
            for (int b = tid; b < 512; b += 1024) hist[b] = 0u;
            // 1. the items, the half tables that have a candidate at all (155 of 198 at V = 2048: the multisequence visits empty
            //    cells too) numbered densely per split, then the owner item of every candidate
            const int64_t tbase = tab_off[q];
            const int nt0 = plan[q].ntab0;
            uint16_t* slot_of = reinterpret_cast<uint16_t*>(skey);  // [ntt], free until the survivors are ranked
            for (int i = tid; i < ntt; i += 1024) slot_of[i] = 0;
            for (int c = tid; c < n; c += 1024) sum[c] = 0;
            __syncthreads();
            for (int i = tid; i < ni; i += 1024) {
                const WorkItem it = items[it0 + i];
                TinyItem ti;
                ti.start = (uint32_t)it.start;
                ti.rel = (uint16_t)(cand_start[it0 + i] - c0);
                ti.len = (uint16_t)it.len;
                ti.t0 = (uint16_t)(it.tab0 - tbase);
                ti.t1 = (uint16_t)(it.tab1 - tbase - nt0);
                s_items[i] = ti;
                slot_of[ti.t0] = 1;
                slot_of[nt0 + ti.t1] = 1;
                if (it.start + it.len > (int64_t)0xffffffffll || it.len > 65535) sh->fb = 1;
            }
            __syncthreads();
            for (int s = 0; s < 2; ++s) {  // dense numbers: four entries per thread, one workgroup scan per split
                const int base = s ? nt0 : 0, nts = s ? ntt - nt0 : nt0;
                int fl[4], cnt = 0;
#pragma unroll
                for (int u = 0; u < 4; ++u) { const int i = tid * 4 + u; fl[u] = i < nts ? (int)slot_of[base + i] : 0; cnt += fl[u]; }
                int tot;
                int run = sel_block_excl_scan(cnt, sh->wsum, &tot);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = tid * 4 + u;
                    if (i < nts) {
                        slot_of[base + i] = fl[u] ? (uint16_t)run : (uint16_t)0xffff;
                        if (fl[u]) used[base + run] = (uint16_t)i;
                        run += fl[u];
                    }
                }
                if (tid == 0) sh->nused[s] = tot;
                __syncthreads();
            }
            for (int i = tid; i < ni; i += 1024) {
                TinyItem ti = s_items[i];
                ti.t0 = slot_of[ti.t0];
                ti.t1 = slot_of[nt0 + ti.t1];
                s_items[i] = ti;
            }
            __syncthreads();
            for (int i = wv; i < ni; i += 16) {
                const TinyItem ti = s_items[i];
                for (int p = lane; p < (int)ti.len; p += 64) own[(int)ti.rel + p] = (uint16_t)i;
            }
            __syncthreads();
            if (sh->fb) fall = true;
            if (dbg && tid == 0) atomicAdd(&dbg[15], (unsigned int)(sh->nused[0] + sh->nused[1]));
            TINY_T(1);
        }
        if (!fall && !all_in) {
            const int64_t tbase = tab_off[q];
            const int nt0 = plan[q].ntab0;
            // 2. cap from the sample: the r-th smallest of TINY_NS sampled distances (float32 arithmetic: the cap is a heuristic,
            //    the bounds below hold for any value), r / TINY_NS ~ three times limit / n
            {
                const int s = tid >> 3, sub = tid & 7;
                const int c = (int)(((int64_t)s * n + (n >> 1)) / TINY_NS);
                const TinyItem ti = s_items[own[c]];
                const CodeWords<MT> cw = load_code<MT>(codes, (int64_t)ti.start + (c - (int)ti.rel));
                float acc = 0.f;
                for (int j = sub; j < MT; j += 8) {
                    const bool second = j >= NF;
                    const double* f = reinterpret_cast<const double*>(__builtin_assume_aligned(
                        px + (tbase + (second ? nt0 + (int)used[nt0 + ti.t1] : (int)used[ti.t0])) * h + (second ? j - NF : j) * W, 16));
                    const uint32_t code = (cw.w[j >> 2] >> (8 * (j & 3))) & 255u;
                    const double* sc = reinterpret_cast<const double*>(__builtin_assume_aligned(subs + ((size_t)j * K + code) * W, 16));
#pragma unroll
                    for (int e = 0; e < W; ++e) { const float df = (float)f[e] - (float)sc[e]; acc = fmaf(df, df, acc); }
                }
                acc += __shfl_xor(acc, 1);
                acc += __shfl_xor(acc, 2);
                acc += __shfl_xor(acc, 4);
                if (sub == 0) samp[s] = acc;
            }
            __syncthreads();
            {
                const int s = tid >> 3, sub = tid & 7;
                const float v = samp[s];
                int less = 0;
                for (int k2 = sub * (TINY_NS / 8); k2 < (sub + 1) * (TINY_NS / 8); ++k2) {
                    const float u = samp[k2];
                    less += (u < v || (u == v && k2 < s)) ? 1 : 0;
                }
                less += __shfl_xor(less, 1);
                less += __shfl_xor(less, 2);
                less += __shfl_xor(less, 4);
                int r = (int)((3.0 * TINY_NS * (double)L) / (double)n) + 3;
                r = r > TINY_NS ? TINY_NS : r;
                if (sub == 0 && less == r - 1) sh->cap_bits = __float_as_uint(v);
            }
            __syncthreads();
            TINY_T(2);
            const float cap = __uint_as_float(sh->cap_bits);
            const float inv_step = cap > 0.f ? 256.0f / cap : 0.f;
            // 3. byte tables of a split, at most tch at a time; every candidate adds its entries up.  An entry is
            //    sum (px - c)^2 in float32: the thread keeps its (sub-quantizer, centroid) in registers, the px row of a table
            //    arrives through scalar loads (uniform over the wave) from the float32 copy of px that k_tables_group wrote
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int nts = sh->nused[s];            // tables of this split that have a candidate
                const int64_t tb = tbase + (s ? nt0 : 0);
                const uint16_t* lst = used + (s ? nt0 : 0);
                for (int tlo = 0; tlo < nts; tlo += tch) {
                    const int tc = nts - tlo < tch ? nts - tlo : tch;
                    __syncthreads();  // the previous chunk's tables are no longer read
                    TINY_T(3);
                    TINY_T(4);
#pragma unroll
                    for (int pp = 0; pp < PPT; ++pp) {
                        const int pr = tid + pp * 1024;
                        if (pr < PAIRS) {
                            const int jj = __builtin_amdgcn_readfirstlane(pr / K), k = pr % K;  // a wave shares its sub-quantizer
                            float cen[W];
                            if constexpr (KEEP) {
#pragma unroll
                                for (int e = 0; e < W; ++e) cen[e] = cenk[s][pp][e];
                            } else {
                                const double* sc = subs + ((size_t)(s * NF + jj) * K + k) * W;
#pragma unroll
                                for (int e = 0; e < W; ++e) cen[e] = (float)sc[e];
                            }
                            if (dbg) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TINY_T(12); }
                            const float* frow = px32 + tb * h + jj * W;
                            uint8_t* trow = s_tab + jj * K + k;
                            constexpr int U = TinyRows<W>::U;
                            typedef float tiny_f2 __attribute__((ext_vector_type(2)));
                            int cur[U];  // table numbers of the next U rows: read from LDS one iteration ahead (under the scalar loads' wait)
#pragma unroll
                            for (int u = 0; u < U; ++u) cur[u] = __builtin_amdgcn_readfirstlane((int)lst[tlo + (u < tc ? u : tc - 1)]);
                            int pf[4] = {0, 0, 0, 0};
                            for (int t = 0; t < tc; t += U) {
                                const float* rp[U];
                                int tu[U], nxt[U];
#pragma unroll
                                for (int u = 0; u < U; ++u) {
                                    tu[u] = t + u < tc ? t + u : tc - 1;
                                    rp[u] = frow + cur[u] * h;
                                    nxt[u] = (int)lst[tlo + (t + U + u < tc ? t + U + u : tc - 1)];
                                }
                                float f[U][W];
                                tiny_sload_rows<W>(rp, f);
                                if constexpr (U == 4) tiny_keep(pf);
#pragma unroll
                                for (int u = 0; u < U; ++u) cur[u] = __builtin_amdgcn_readfirstlane(nxt[u]);
                                if constexpr (U == 4) tiny_prefetch4(frow + cur[0] * h, frow + cur[1] * h, frow + cur[2] * h, frow + cur[3] * h, pf);
#pragma unroll
                                for (int u = 0; u < U; ++u) {
                                    tiny_f2 acc = {0.f, 0.f};  // packed float32 math: even and odd components apart
#pragma unroll
                                    for (int e = 0; e < W; e += 2) {
                                        const tiny_f2 c2 = {cen[e], cen[e + 1]};
                                        const tiny_f2 x = {f[u][e], f[u][e + 1]};
                                        const tiny_f2 d = x - c2;
                                        acc = __builtin_elementwise_fma(d, d, acc);
                                    }
                                    trow[tu[u] * NF * K] = (uint8_t)(int)fminf((acc.x + acc.y) * inv_step, 255.0f);
                                }
                            }
                            if constexpr (U == 4) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); tiny_keep(pf); }
                        }
                    }
                    __syncthreads();
                    TINY_T(5);
                    for (int cb = tid; cb < n; cb += 4096) {  // four candidates per thread and round: their code loads overlap
                        int tl4[4];
                        uint32_t cw4[4][CW];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int c = cb + r * 1024;
                            tl4[r] = -1;
                            if (c < n) {
                                const TinyItem ti = s_items[own[c]];
                                const int tl = (s ? (int)ti.t1 : (int)ti.t0) - tlo;
                                if ((unsigned)tl < (unsigned)tc) {
                                    tl4[r] = tl;
                                    const uint8_t* cp = codes + ((int64_t)ti.start + (c - (int)ti.rel)) * MT;
                                    if constexpr (NF == 2) cw4[r][0] = *reinterpret_cast<const uint32_t*>(cp) >> (16 * s);
                                    else {
#pragma unroll
                                        for (int u = 0; u < CW; ++u) cw4[r][u] = reinterpret_cast<const uint32_t*>(cp + s * NF)[u];
                                    }
                                }
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (tl4[r] >= 0) {
                                const int c = cb + r * 1024;
                                unsigned int acc = 0;
#pragma unroll
                                for (int jj = 0; jj < NF; ++jj)
                                    acc += s_tab[(tl4[r] * NF + jj) * K + ((cw4[r][jj >> 2] >> (8 * (jj & 3))) & 255u)];
                                sum[c] = (uint16_t)(sum[c] + acc);
                            }
                    }
                }
            }
            __syncthreads();
            TINY_T(6);
            // 4. histogram of the sums, s*, the survivors' bound
            for (int c = tid; c < n; c += 1024) {
                const int sv = sum[c];
                atomicAdd(&hist[sv < 511 ? sv : 511], 1u);
            }
            __syncthreads();
            {
                const int v = tid < 512 ? (int)hist[tid] : 0;
                int tot;
                const int ex = sel_block_excl_scan(v, sh->wsum, &tot);
                if (tid < 512) {
                    hist[tid] = (unsigned int)(ex + v);  // inclusive counts (each thread rewrites its own bin)
                    if (ex < L && L <= ex + v) sh->sstar = tid;
                }
            }
            __syncthreads();
            const int sstar = sh->sstar;
            // float32: a component difference carries an absolute error of 2^-23 amax_, amax_ = the largest operand -- |c| <= cmax_, and
            // where the entry is below the cap |px| < cmax_ + sqrt(cap) (a clamped entry only needs the RELATIVE accuracy it has);
            // an entry e < cap is off by at most 2 sqrt(W cap) 2^-23 amax_: under step / 16 = cap / 4096 when cap >= W amax_^2 / 2^20
            const float cmax_ = __uint_as_float(sh->cen_bits);
            const float amax_ = cmax_ + sqrtf(cap);
            if (sstar > 254 || !(cap >= (float)W * amax_ * amax_ * (1.0f / 1048576.0f))) fall = true;
            else {
                const int thr = sstar + MT + 1;
                nsurv = (int)hist[thr < 511 ? thr : 511];
                if (thr >= 511 || nsurv > smax) fall = true;
                else {
                    for (int c = tid; c < n; c += 1024)
                        if ((int)sum[c] <= thr) sidx[atomicAdd(&sh->cnt, 1)] = (uint32_t)c;
                }
            }
            if (dbg && tid == 0) {
                atomicAdd(&dbg[0], 1u);
                atomicAdd(&dbg[1], fall ? 1u : 0u);
                atomicAdd(&dbg[2], (unsigned int)nsurv);
                atomicAdd(&dbg[3], (unsigned int)(sstar > 254 ? 255 : sstar));
            }
            __syncthreads();
        } else if (all_in) {
            nsurv = n;
            for (int c = tid; c < n; c += 1024) sidx[c] = (uint32_t)c;
            __syncthreads();
        }
        if (fall) {
            // every candidate's exact key to the global key array; k_select_topl ranks this query
            tiny_exact_all<MT, W>(items, cand_start, px, subs, codes, h, it0, ni, c0, n64, keys_fb, qmin, qmax, q);
            if (tid == 0) fbflag[q] = 1;
            continue;
        }
        TINY_T(7);
        // 5. exact entries of the survivors, one thread per (survivor, sub-quantizer); then the running sum of search.py:173
        {
            const int64_t tbase = tab_off[q];
            const int nt0 = plan[q].ntab0;
            for (int pr = tid; pr < nsurv * MT; pr += 1024) {
                const int sv = pr / MT, j = pr % MT;
                const int c = (int)sidx[sv];
                const TinyItem ti = s_items[own[c]];
                const uint32_t code = codes[((int64_t)ti.start + (c - (int)ti.rel)) * MT + j];
                const bool second = j >= NF;
                const double* f = reinterpret_cast<const double*>(__builtin_assume_aligned(
                    px + (tbase + (second ? nt0 + (int)used[nt0 + ti.t1] : (int)used[ti.t0])) * h + (second ? j - NF : j) * W, 16));
                const double* sc = reinterpret_cast<const double*>(__builtin_assume_aligned(subs + ((size_t)j * K + code) * W, 16));
                auto elem = [&](int e) -> double { const double df = f[e] - sc[e]; return df * df; };
                e_lds[pr] = pw_leaf<double>(elem, 0, W);
            }
        }
        __syncthreads();
        TINY_T(8);
        for (int sv = tid; sv < nsurv; sv += 1024) {
            double d = e_lds[sv * MT];
#pragma unroll
            for (int j = 1; j < MT; ++j) d = d + e_lds[sv * MT + j];
            skey[sv] = (uint64_t)__double_as_longlong(d);
        }
        __syncthreads();
        TINY_T(9);
        // rank by counting: a survivor's place is the number of survivors before it in (key, retrieval position) order -- all lanes
        // read the same pair at a time (LDS broadcast), no barrier; the first `limit` places are the result
        for (int sv0 = 0; sv0 < nsurv; sv0 += 128) {  // eight threads per survivor, an eighth of the list each
            const int sv = sv0 + (tid >> 3), part = tid & 7;
            const bool on = sv < nsurv;
            const uint64_t kk = on ? skey[sv] : 0ull;
            const uint32_t cc = on ? sidx[sv] : 0u;
            const int per = (nsurv + 7) >> 3;
            const int j0 = part * per, j1 = j0 + per < nsurv ? j0 + per : nsurv;
            int place = 0;
#pragma unroll 4
            for (int j = j0; j < j1; ++j) place += sel_pair_less(skey[j], sidx[j], kk, cc) ? 1 : 0;
            place += __shfl_xor(place, 1);
            place += __shfl_xor(place, 2);
            place += __shfl_xor(place, 4);
            if (on && part == 0 && place < nv) {
                const int i = own[cc];
                sel_keys[ob + place] = kk;
                sel_vals[ob + place] = ((uint64_t)(it0 + i) << 32) | (uint32_t)((int)cc - (int)s_items[i].rel);
            }
        }
        if (tid == 0) { nsel[q] = nv; fbflag[q] = 0; }
        TINY_T(10);
    }
#undef TINY_T
}

static size_t tiny_lds_bytes(int ncmax, int pool_bytes) {
    return (size_t)4 * ncmax + (size_t)pool_bytes + 512 * 4 + TINY_NS * 4 + (size_t)TINY_SMAX * 12 + sizeof(TinyShared) + 16;
}

// bytes of the per-query pool (items, tables or survivors) next to the candidate layout; 0: the kernel does not serve this shape
static int tiny_pool(int M, int K, int w, int h, int L, int64_t ncmax_need, int* ncmax_out) {
    if (!(M == 4 || M == 8 || M == 16) || K != 256 || !(w == 4 || w == 8 || w == 16 || w == 32) || h != (M / 2) * w || h > 256) return 0;
    if (ncmax_need > TINY_NCMAX) return 0;
    int ncmax = 4096;
    while (ncmax < ncmax_need) ncmax += 2048;
    const size_t fixed = tiny_lds_bytes(ncmax, 0);
    const size_t budget = 160 * 1024 - 512;  // the static LDS of the helpers (key range, scans) comes on top
    if (fixed + 32768 > budget) return 0;
    const int pool = (int)((budget - fixed) & ~(size_t)15);
    // a query with a few hundred items must keep room for 2 * limit survivors' exact entries and a useful number of tables
    if ((pool - 8192) / (8 * M) < 2 * L || (pool - 8192) / ((M / 2) * 256) < 8) return 0;
    *ncmax_out = ncmax;
    return pool;
}

// a selection's operands: the keys it reads, where it leaves the ranked pairs of a query (sp.stride slots, nsel[q] of them filled)
struct SelectArgs {
    const uint64_t* keys;  // every candidate's exact key (k_tiny_select: written for the queries it flags)
    int L;
    SelectPlan sp;
    uint64_t *sel_keys, *sel_vals;
    int* nsel;
    int64_t *seg_b, *seg_e;  // null, or the segments of the selected pairs for the segmented sort
    const int* only;         // null, or ranked: flagged queries only
    // the streaming route's indirect keys (see k_select_topl): null / 0 elsewhere
    const uint32_t* rid;
    const int* kcnt;
    int64_t kstride;
};

struct TinyArgs {  // what k_tiny_select reads besides the candidate layout and the selection's outputs
    const int64_t* tab_off;
    const PlanOut* plan;
    const double *px, *subs;
    int h, ncmax, tch;
    uint64_t* keys_fb;  // = SelectArgs::keys, written
    int* fbflag;
    float* px32_ws;
    unsigned int* dbg;
};

template <int MT, int W>
static void launch_tiny_t(const CandArgs& c, const SelectArgs& s, const TinyArgs& t) {
    const size_t lds = tiny_lds_bytes(t.ncmax, t.tch);
    const unsigned grid = (unsigned)(c.nq < 256 ? c.nq : 256);
    hipLaunchKernelGGL((k_tiny_select<MT, W>), dim3(grid), dim3(1024), lds, c.st, c.items, c.cand_start, c.seg, c.item_off, t.tab_off, t.plan, t.px, t.subs, c.codes,
                       t.h, c.nq, s.L, t.ncmax, t.tch, s.sp.stride, s.sel_keys, s.sel_vals, s.nsel, t.keys_fb, c.qmin, c.qmax, t.fbflag, t.px32_ws, t.dbg);
}

static bool launch_tiny(int M, int w, const CandArgs& c, const SelectArgs& s, const TinyArgs& t) {
#define CIS_TINY(MT, W) if (M == MT && w == W) return launch_tiny_t<MT, W>(c, s, t), true;
    CIS_TINY(8, 16) CIS_TINY(16, 8) CIS_TINY(4, 32) CIS_TINY(16, 16) CIS_TINY(8, 32) CIS_TINY(8, 8) CIS_TINY(4, 16) CIS_TINY(16, 4)
#undef CIS_TINY
    return false;
}

template <bool SORT_LDS, int NT>
static void launch_select_nt(const CandArgs& c, const SelectArgs& s) {
    hipLaunchKernelGGL((k_select_topl<SORT_LDS, NT>), dim3((unsigned)c.nq), dim3(NT), s.sp.lds, c.st, s.keys, c.seg, c.cand_start, c.item_off, c.qmin, c.qmax, c.n_items, s.L,
                       s.sp.p2, s.sp.stride, s.sel_keys, s.sel_vals, s.nsel, s.seg_b, s.seg_e, s.only, s.rid, s.kcnt, s.kstride);
}

// fewer queries than CUs: one large workgroup per query walks its keys faster; else two 512-thread ones per CU
template <bool SORT_LDS>
static void launch_select(const CandArgs& c, const SelectArgs& s) {
    if (c.nq <= 256) launch_select_nt<SORT_LDS, 1024>(c, s);
    else launch_select_nt<SORT_LDS, 512>(c, s);
}

// one sub-batch of queries (device pointers); writes ranked partial hits [nq][L] and visited [nq]
static const int CIS_RETRY_SMALLER = 1;  // internal: the batch does not fit the workspace budget, halve it

static void route_hints(cis_index* ix, int nq, int64_t quota, int L, Route* r) {
    cis_model* m = ix->m;
    const int V = m->V, K = m->K, M = m->M;
    r->w_pow2 = m->w == 4 || m->w == 8 || m->w == 16 || m->w == 32;
    r->split_tables = r->w_pow2 && K <= 256;
    r->big = use_all_path(ix, M, K, L, nq);
    r->fast = scan2_supported(M, K, L) && !ix->force_exact_scan;
    r->tiny_cells = index_has_tiny_cells(ix);
    r->geom = scan2_geom(M, K, L, nq);
    // scan v3 (16-bit fixed-point tables, four queries per workgroup) for large batches; its region entries hold 16-bit
    // positions, so a chunk is at most 65536 candidates.  scan_mode 3 forces it for any batch size (tests).
    static const int env_scan = getenv("CIS_FORCE_SCAN") ? atoi(getenv("CIS_FORCE_SCAN")) : 0;  // A/B runs: 2 or 3
    // Automatic routing picks it where it measured faster than k_adc_scan2 (profiles/r02*): short cells (a batch that
    // visits about quota / (n_total / cells) + 1 cells per query, each shorter than 8192 codes) at M <= 8.
    const bool short_cells = ix->nonempty_cells > 0 && ix->n_total / ix->nonempty_cells < 8192 && M <= 8;
    // ... and long cells at M <= 8, limit <= 128 through its sampled single-pass form (k_adc_scan4 with a tenth of the rows as
    // the sample: profiles/r03m_*); CIS_SCAN_LONG=0 keeps them on k_adc_scan2
    static const int env_long = getenv("CIS_SCAN_LONG") ? atoi(getenv("CIS_SCAN_LONG")) : 1;
    // ... and at M = 16 with the saturating scale (round 4).  Its failure mode is expensive -- a slot whose scale missed runs again in
    // the streaming form, ~14x the time when most of them do -- so the index watches the fall-back count of its last such scan
    // (a pinned word the scan's stream writes; no wait, the value may be one batch old) and, when more than an eighth of the slots
    // fell back, serves the next 64 batches from k_adc_scan2 before it tries again.  CIS_S4_M16=0: always k_adc_scan2.
    static const int env_m16 = getenv("CIS_S4_M16") ? atoi(getenv("CIS_S4_M16")) : 1;
    if (M == 16 && env_m16 && ix->h_totals) {
        const int32_t* fb = reinterpret_cast<const int32_t*>(&ix->h_totals[4]);
        const int32_t n_s = __atomic_load_n(&fb[0], __ATOMIC_RELAXED), n_f = __atomic_load_n(&fb[1], __ATOMIC_RELAXED);
        if (ix->m16_holdoff > 0) --ix->m16_holdoff;
        else if (n_s > 0 && (int64_t)n_f * 8 > n_s) { ix->m16_holdoff = 64; ++ix->m16_backoffs; ix->h_totals[4] = 0; }
    }
    const bool long_cells = env_long != 0 && !short_cells && (M <= 8 || (env_m16 && ix->m16_holdoff == 0)) && L <= 128 && ix->ncells <= 65536;
    r->use3 = !ix->force_exact_scan && scan3_supported(M, K, L) && !r->big &&
              (ix->force_scan3 || (nq >= 256 && !ix->force_scan2 && (env_scan == 3 || (env_scan == 0 && (short_cells || long_cells)))));
    // (Splitting a shard's cells into chunks so that a cell-sharded index at world = 8 fills the chip again was measured
    // and lost: 0.516 against 0.306 ms per partial search -- more survivors, colder bounds: profiles/r02d_shard_emulation.txt.)
    int seg_max = r->use3 ? (nq >= 64 ? 65536 : 4096) : (nq >= 1024 ? (1 << 20) : (nq >= 64 ? 16384 : 4096));
    // (Round 3 cut the long cells of a shard of four or more into chunks of 20480 candidates so that its few work items spread over
    // the chip: partial search 0.343 -> 0.307 ms alone on the device.  With three batches in flight the whole-cell chunks win -- emulated
    // rank 0 of world 8: 0.227 -> 0.163 ms per step, and 0.552 -> 0.479 ms for the routed protocol's full batches
    // (profiles/archive/r05b/r05_shards.txt) -- so the rule is gone; CIS_SEG_MAX=20480 brings it back for A/B runs.)
    // The HBM-streaming route (lopq_stream.hip): few queries, very many candidates each -- an exhaustive quota, or any quota on cells
    // of hundreds of thousands of codes.  Decided here from the bound of the candidates per query (the chunk size is part of the
    // plan); the exact count confirms it in route_decide.  Chunks of 65536 candidates, longer when the largest cell would need more
    // than the slot builder's 16 chunk keys (the items of a slot must be the SAME chunk of a cell).
    static const int64_t stream_min = getenv("CIS_STREAM_MIN") ? atoll(getenv("CIS_STREAM_MIN")) : 262144;  // candidates per query from which it pays
    static const int stream_nq = getenv("CIS_STREAM_NQ") ? atoi(getenv("CIS_STREAM_NQ")) : 16;               // 0: never
    r->stream_min = stream_min;
    const bool stream_auto = !ix->stream_off && !ix->force_exact_scan && !ix->force_prefilter_scan && !ix->force_scan2 && !ix->force_scan3 &&
                             nq <= stream_nq && L <= 440 && ix->world == 1 &&
                             ((quota < ix->n_total ? (quota < 0 ? 0 : quota) : ix->n_total) + ix->max_cell) >= stream_min;
    r->stream_hint = (ix->force_stream || stream_auto) && !ix->stream_off && stream_supported(M, K, L) && (K % 4 == 0) &&
                     ix->ncells <= 65536 && !r->tiny_cells;
    if (r->stream_hint) {
        // One chunk per cell (round 6): the stream kernel cuts the ROWS of all slots into equal ranges itself, so short chunks buy
        // nothing and cost plan, slot builder and candidate layout their work items (2398 -> 256 for the exhaustive query over 200 M
        // codes).  A chunk stays below 2^31 code bytes (32-bit buffer offsets).
        const int64_t cap_len = (((int64_t)1 << 31) - 65536) / M;
        int64_t want = ix->max_cell > 65536 ? ix->max_cell : 65536;
        want = want < cap_len ? want : cap_len;
        if (const char* e = getenv("CIS_STREAM_CHUNK")) want = atoi(e) > 0 ? atoi(e) : want;  // A/B runs
        seg_max = (int)(ceil_div(want, (int64_t)1024) * 1024);
        const int64_t need = ceil_div(ix->max_cell > 0 ? ix->max_cell : 1, (int64_t)16);   // (at most 16 chunk keys per cell)
        if (need > seg_max) seg_max = (int)ceil_div(need, (int64_t)1024) * 1024;
        if (ix->force_stream && getenv("CIS_STREAM_SEG")) seg_max = atoi(getenv("CIS_STREAM_SEG")) > 0 ? atoi(getenv("CIS_STREAM_SEG")) : seg_max;  // tests: short chunks on small fixtures
    }
    if (const char* e = getenv("CIS_SEG_MAX")) seg_max = atoi(e) > 0 ? atoi(e) : seg_max;  // A/B runs (tools/emulate_shard.py)
    r->seg_max = seg_max;
    // thousands of coarse clusters (the release configurations' V = 2048 / 4096): the plan is a per-query selection + sort
    // (k_plan_par) instead of one frontier step per visited cell; queries it cannot resolve fall back to the frontier walk
    const bool no_par_plan = getenv("CIS_NO_PAR_PLAN") != nullptr;
    // ... and few queries that visit MANY cells of a small vocabulary (the streaming route's exhaustive quota: all 256 cells of V = 16):
    // the frontier walk costs ~1.3 us per visited cell and runs twice (count, emit) -- 0.67 of the 1.25 ms of a single exhaustive
    // query over 200 M codes; the sort-based plan does the same cells in one band
    const bool stream_par = r->stream_hint && V >= 8 && ix->n_total > 0 &&
                            (double)(quota < 0 ? 0 : quota) * (double)ix->nonempty_cells >= 32.0 * (double)ix->n_total;
    r->par_plan = ((V >= 128 || stream_par) && V <= PLAN_PAR_STAGE) && !no_par_plan;
    static const bool no_fused_front = getenv("CIS_NO_FUSED_FRONT") != nullptr;
    r->fused_front = V <= 64 && !r->par_plan && !no_fused_front;
}

// the emitting pass of the walk (emit_plan: lopq_plan.hip), then the tables' first stage
template <typename CT>
static void emit_and_tables(Batch& b, const Route& r) {
    cis_model* m = b.ix->m;
    const int V = m->V, h = m->h;
    const size_t tab_lds = (size_t)(2 * h + (h < 256 ? 256 : 0)) * sizeof(double);
    emit_plan<CT>(b, r);
    if (b.n_tabs > 0)
        launch_tables<CT>(b.n_tabs, tab_lds, b.st, (const CT*)b.f.xc, coarse_centroids(m, CT()), m->d_Rt, m->d_mus, m->d_subs, b.tabs, b.tab_order, V, h,
                          m->w, m->nf, m->K, m->D, b.T, m->prog_w, b.px_buf, b.d_tot, r.direct ? b.T32 : nullptr);
}

// the route, now that the totals are known; CIS_RETRY_SMALLER when the batch does not fit the workspace budget
static int route_decide(Batch& b, Route* r) {
    cis_index* ix = b.ix;
    cis_model* m = ix->m;
    const int K = m->K, M = m->M, h = m->h, nf = m->nf, nq = b.nq, L = b.L;
    r->direct = !b.d_tot && r->big && r->tiny_cells && h <= 256 && direct_jp(M, K, m->w) > 0 &&
                !getenv("CIS_TABLES_UNGROUPED") && !getenv("CIS_NO_DIRECT");
    r->stream = r->stream_hint && b.n_items > 0 && (r->w_pow2 || r->fast) &&
                (ix->force_stream || b.d_tot != nullptr || b.n_cand_all / (nq > 0 ? nq : 1) >= r->stream_min);   // (d_tot: certain, see plan_totals)
    if (!r->stream) {
        // workspace budget: per-item hit lists and the float64 tables.  A batch that would need more (e.g. an
        // exhaustive quota: every query visits every cell) is split by the caller and planned again.
        const int64_t S_ = r->fast ? r->geom.S : L;
        double need = (double)b.n_items * S_ * (r->fast ? sizeof(uint64_t) : sizeof(cis_hit)) + (double)b.n_tabs * nf * K * sizeof(double);
        if (r->big) {  // every candidate's key, plus the selected pairs or the full sort's buffers
            const SelectPlan sp_ = select_plan(L, nq, b.n_cand_all);
            need = (sp_.select ? 8.0 * (double)b.n_cand_all + (sp_.sort_lds ? 16.0 : 32.0) * (double)nq * (double)sp_.stride : 32.0 * (double)b.n_cand_all) +
                   (r->direct ? (double)b.n_tabs * h * sizeof(double) : (double)b.n_tabs * nf * K * sizeof(double));
        }
        // default 24 GB of the 288 GB: thousands of coarse clusters need ~1.6 MB of tables per query (V = 2048, quota 10000)
        const double budget = (getenv("CIS_WORKSPACE_GB") ? atof(getenv("CIS_WORKSPACE_GB")) : 24.0) * 1.0e9;
        if (need > budget && nq > 1) {
            ix->retry_fraction = 0.9 * budget / need;  // the caller plans again with this share of the batch
            return CIS_RETRY_SMALLER;
        }
    }
    if (!b.d_tot) {
        ix->stats[0] += b.n_cand_all;
        ix->stats[1] += b.n_items;
        ix->stats[2] += b.n_tabs;
    }
    r->geom3 = scan3_geom(M, K, L, b.n_items > 0 ? b.n_cand_all / b.n_items : 0, ix->force_two_pass);
    r->S = r->fast ? (r->use3 ? r->geom3.S : r->geom.S) : L;
    // The float32 copy of the tables is a third of what the tables kernel writes (8 + 4 bytes per entry: 402 MB per C2 batch, and that
    // kernel is bound by its writes); CIS_NO_T32=1 drops it -- the scans then convert the float64 entries while they stage them
    // (tab_f4: the same bits).  The tiny-cell path keeps its float32 px copy in this buffer.
    static const bool no_t32 = getenv("CIS_NO_T32") != nullptr && atoi(getenv("CIS_NO_T32")) != 0;
    r->drop_t32 = no_t32 && !r->direct && r->split_tables;
    return CIS_OK;
}

// workspaces of the emit pass, the tables and the scans' hit lists
static int reserve_batch(Batch& b, const Route& r) {
    cis_index* ix = b.ix;
    cis_model* m = ix->m;
    const int K = m->K, h = m->h, nf = m->nf;
    const int64_t n_items = b.n_items, n_tabs = b.n_tabs;
    CIS_TRY(ix->w_items.reserve((size_t)(n_items + 1) * sizeof(WorkItem)));
    CIS_TRY(ix->w_tabs.reserve((size_t)(n_tabs + 1) * sizeof(TabDesc)));
    CIS_TRY(ix->w_T.reserve(r.direct ? 256 : (size_t)(n_tabs + 1) * nf * K * sizeof(double)));
    if (!r.big && !r.stream) CIS_TRY(ix->w_hits.reserve((size_t)(n_items + 1) * r.S * (r.fast ? sizeof(uint64_t) : sizeof(cis_hit))));
    CIS_TRY(ix->w_hitn.reserve((size_t)(n_items + 1) * 2 * sizeof(int)));
    if (r.use3) CIS_TRY(ix->w_slack.reserve((size_t)(n_items + 1) * 2 * sizeof(float)));
    b.items = ix->w_items.as<WorkItem>();
    b.tabs = ix->w_tabs.as<TabDesc>();
    CIS_TRY(ix->w_tord.reserve((size_t)(n_tabs + 1) * sizeof(int)));
    b.tab_order = ix->w_tord.as<int>();
    b.T = ix->w_T.as<double>();
    // tiny cells: the float32 copy of px for k_tiny_select lives in w_T32 (no tables on that path)
    if (!r.drop_t32) CIS_TRY(ix->w_T32.reserve(r.direct ? (size_t)(n_tabs + 1) * h * sizeof(float) : (size_t)(n_tabs + 1) * nf * K * sizeof(float)));
    b.T32 = r.drop_t32 ? nullptr : ix->w_T32.as<float>();
    b.px_buf = nullptr;
    if (r.split_tables) {
        CIS_TRY(ix->w_px.reserve((size_t)(n_tabs + 1) * h * sizeof(double)));
        b.px_buf = ix->w_px.as<double>();
    }
    return CIS_OK;
}

// second stage of the tables: from the projected residuals, or the float32 copy of the float64 tables
static void finish_tables(const Batch& b, const Route& r) {
    cis_model* m = b.ix->m;
    hipStream_t st = b.st;
    const int K = m->K, h = m->h, nf = m->nf;
    const int64_t n_tabs = b.n_tabs;
    double *T = b.T, *px_buf = b.px_buf;
    float* T32 = b.T32;
    TabDesc* tabs = b.tabs;
    const int64_t* d_tot = b.d_tot;
    if (r.direct) {
    } else if (r.split_tables && n_tabs > 0) {
        const bool few = n_tabs <= 1024;   // (d_tot: n_tabs is a bound, the kernel reads the real count)
        dim3 g((unsigned)ceil_div(n_tabs, few ? 8 : 64), (unsigned)nf, 2);
#define CIS_TFP(WW)                                                                                                                                      \
        if (few) hipLaunchKernelGGL((k_tables_from_px<WW, 8>), g, dim3(256), 0, st, px_buf, tabs, (int)n_tabs, m->d_subs, h, nf, K, T, T32, d_tot);      \
        else hipLaunchKernelGGL((k_tables_from_px<WW, 64>), g, dim3(256), 0, st, px_buf, tabs, (int)n_tabs, m->d_subs, h, nf, K, T, T32, d_tot)
        switch (m->w) {
            case 4: CIS_TFP(4); break;
            case 8: CIS_TFP(8); break;
            case 16: CIS_TFP(16); break;
            default: CIS_TFP(32); break;
        }
#undef CIS_TFP
    } else if (r.fast && n_tabs > 0) {
        const int64_t ne = n_tabs * nf * K;
        hipLaunchKernelGGL(k_tables_f32, dim3((unsigned)ceil_div(ne, 256)), dim3(256), 0, st, T, ne, nf, K, T32, tabs);
    }
}

static int search_batch(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota, int L, const SearchOut& out, hipStream_t st);

// 4''. the HBM-streaming route (lopq_stream.hip): sample -> threshold -> stream -> exact keys of the listed candidates ->
// ranking (k_select_topl, ties by retrieval index) -> proof; a failed proof hands the batch to the generic path
static int run_stream(Batch& b, const Route& r) {
    cis_index* ix = b.ix;
    hipStream_t st = b.st;
    const int K = ix->m->K, M = ix->m->M, nq = b.nq, L = b.L;
    const int64_t n_items = b.n_items, n_cand_all = b.n_cand_all;
    const SearchOut& out = b.out;
    CIS_TRY(mark(b, 2));
    const uint8_t* codes = ix->codes_ptr();
    const int64_t* ids = ix->ids_ptr();
    // queries per slot: a pair costs the launch what one query costs (the codes are the bound), four cost ~1.45 of a pair
    // (profiles/r06_stream_probe.txt) -- worth it when the queries share their cells, i.e. the quota covers most of the index
    const bool shared_cells = b.quota >= ix->n_total / 2;
    const int G = (nq >= 3 && shared_cells && stream_max_group() >= 4) ? 4 : (nq >= 2 ? 2 : 1);
    const int cap = STREAM_CAP, B = STREAM_B;
    const SelectPlan sp = select_plan(L, nq, (int64_t)nq * cap);
    CIS_REQUIRE(sp.sort_lds, "streaming route: limit above the LDS-ranked range");
    // slots: the work items of one chunk of one cell, G per slot (the slot builder of the scan kernels); one query per slot:
    // slot i = work item i (k_stream_prep)
    int64_t CH = ceil_div(ix->max_cell > 0 ? ix->max_cell : 1, (int64_t)r.seg_max);
    CH = CH < 1 ? 1 : (CH > 16 ? 16 : CH);
    Slots sl;
    CIS_TRY(build_slots(b, G > 1 ? SLOTS_SORTED : SLOTS_NONE, G, CH, r.seg_max, &sl));
    const int64_t max_slots = sl.max_slots;
    // workspace: candidate layout, lists, keys, ranked pairs; the sample buckets live in their own buffer (k_stream_tau leaves them
    // clean for the next batch; fresh memory is set to "empty" here)
    {
        const size_t need = (size_t)nq * B * sizeof(uint32_t);
        if (need > ix->w_bmin.cap) {
            CIS_TRY(ix->w_bmin.reserve(need > (size_t)16 * B * sizeof(uint32_t) ? need : (size_t)16 * B * sizeof(uint32_t)));
            CIS_CHECK_HIP(hipMemsetAsync(ix->w_bmin.p, 0xff, ix->w_bmin.cap, st));
        }
    }
    const size_t n_i64 = (size_t)(n_items + 1) + (size_t)3 * (nq + 2) + (size_t)(max_slots + 2) + (size_t)(max_slots + 1) * ((stream_slot_bytes() + 7) / 8);
    const size_t bytes = n_i64 * 8 + (size_t)(nq + 2) * 4 * 4 + (size_t)nq * cap * 4 + (size_t)nq * cap * 8 + (size_t)2 * nq * sp.stride * 8 + 1024;
    CIS_TRY(ix->w_hits.reserve(bytes));
    int64_t* cand_start = ix->w_hits.as<int64_t>();
    int64_t* seg = cand_start + (n_items + 1);
    unsigned long long* qmin = reinterpret_cast<unsigned long long*>(seg + (nq + 2));
    unsigned long long* qmax = qmin + (nq + 2);
    int64_t* rowoff = reinterpret_cast<int64_t*>(qmax + (nq + 2));     // [max_slots + 1]: rows of the slots before each (k_stream_prep)
    void* sdesc = rowoff + (max_slots + 2);                             // [max_slots] slot records (k_stream_prep)
    uint64_t* skeys = reinterpret_cast<uint64_t*>(rowoff + (max_slots + 2) + (size_t)(max_slots + 1) * ((stream_slot_bytes() + 7) / 8));   // [nq][cap]
    uint64_t* sel_keys = skeys + (size_t)nq * cap;                     // [nq][stride]
    uint64_t* sel_vals = sel_keys + (size_t)nq * sp.stride;
    uint32_t* surv = reinterpret_cast<uint32_t*>(sel_vals + (size_t)nq * sp.stride);  // [nq][cap]
    uint32_t* bmin = ix->w_bmin.as<uint32_t>();                        // [nq][B]
    int* cnt = reinterpret_cast<int*>(surv + (size_t)nq * cap);        // [nq + 2]
    int* nsel = cnt + (nq + 2);
    float* tau = reinterpret_cast<float*>(nsel + (nq + 2));
    int* status = reinterpret_cast<int*>(tau + (nq + 2));
    const CandArgs c{st, b.items, n_items, b.item_off, cand_start, seg, qmin, qmax, nq, codes, K};
    StreamArgs s{};
    s.M = M; s.G = G; s.L = L;
    s.slots = sl.slots; s.n_slots = sl.n_slots; s.rowoff = rowoff; s.desc = sdesc;
    s.T = b.T; s.T32 = b.T32; s.tau = tau; s.bmin = bmin; s.B = B;
    s.surv = surv; s.cnt = cnt; s.cap = cap; s.keys = skeys;
    s.sel_keys = sel_keys; s.sel_vals = sel_vals; s.nsel = nsel; s.stride = sp.stride;
    s.ids = ids; s.plan = b.plan; s.status = status;
    // candidate layout + slot records + row offsets + resets: one launch of one workgroup
    launch_stream_prep(c, s, n_cand_all, b.d_tot);
    // sample: every SS-th row; the k-th smallest of the bucket minima lets about k * SS candidates of a query through -- aim at
    // ~max(4096, 16 limit) of them, with k >= 8 so that the count is stable (relative spread 1 / sqrt(k))
    const int64_t per_q = n_cand_all / nq;
    const int row = 64 * (16 / M);
    int64_t target = 4096 > 16 * L ? 4096 : 16 * L;
    if (const char* e = getenv("CIS_STREAM_TARGET")) target = atoll(e) > 0 ? atoll(e) : target;
    int64_t ss = per_q / row / 4096;            // ~4096 sampled rows per query
    ss = ss < 8 ? 8 : (ss > 4096 ? 4096 : ss);
    int64_t kth = target / ss;
    kth = kth < 8 ? 8 : (kth > B / 4 ? B / 4 : kth);
    if (ix->force_stream && getenv("CIS_STREAM_SS")) { ss = atoll(getenv("CIS_STREAM_SS")); kth = getenv("CIS_STREAM_K") ? atoll(getenv("CIS_STREAM_K")) : kth; }  // tests
    // a lane folds `flush` of its sampled rows into one bucket: ~4 B bucket writes per query (a query's sampled rows x 64 lanes / flush)
    int64_t flush = ceil_div(ceil_div(per_q, (int64_t)row * ss) * 64, (int64_t)4 * B);
    flush = flush < 1 ? 1 : flush;
    s.grid = stream_grid(M, G, K, ceil_div(n_cand_all, (int64_t)row) + n_items);
    s.sample_stride = (int)ss; s.flush = (int)flush;
    launch_stream_scan(c, s, true);
    launch_stream_tau(c, s, (int)kth);
    CIS_TRY(mark(b, 5));
    b.pr.has_scan = true;
    ix->last_scan_kernel = 5;
    launch_stream_scan(c, s, false);
    CIS_TRY(mark(b, 3));
    launch_stream_keys(c, s);
    launch_select_nt<true, 1024>(c, SelectArgs{skeys, L, sp, sel_keys, sel_vals, nsel, nullptr, nullptr, nullptr, surv, cnt, (int64_t)cap});
    const int64_t sseq = ++ix->stream_batches;
    launch_stream_finish(c, s, out, ix->d_h_totals + 6, sseq);
    CIS_CHECK_HIP(hipGetLastError());
    CIS_TRY(mark(b, 4));
    ix->stats[3] += 1;
    if (ix->profiling) ix->prof.push_back(b.pr);
    // the proof: two words behind a sequence number in pinned memory (this route serves scans of hundreds of microseconds and
    // more: waiting for their end costs the caller nothing it would not wait for anyway)
    {
        const auto t0 = std::chrono::steady_clock::now();
        bool got = false;
        while (!got) {
            if (__atomic_load_n(&ix->h_totals[8], __ATOMIC_ACQUIRE) == sseq) { got = true; break; }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
        }
        if (!got) {
            CIS_CHECK_HIP(hipStreamSynchronize(st));
            CIS_REQUIRE(__atomic_load_n(&ix->h_totals[8], __ATOMIC_ACQUIRE) == sseq, "the streaming route's status did not arrive");
        }
    }
    if (ix->h_totals[6] == 0 && ix->h_totals[7] == 0) return CIS_OK;
    // a failed proof (an unlucky sample) or an overflowed list (a crowd of equal codes): the generic path answers the batch
    ++ix->stream_fallbacks;
    if (getenv("CIS_STREAM_DEBUG"))
        fprintf(stderr, "[cis] streaming route: %lld failed proofs, %lld overflowed lists of %d queries -> generic path\n", (long long)ix->h_totals[6], (long long)ix->h_totals[7], nq);
    ix->stream_off = true;
    for (int i = 0; i < 3; ++i) ix->stats[i] = 0;  // (the generic pass counts the batch again)
    const int rc = search_batch(ix, b.dQ, b.q_dtype, nq, b.quota, L, out, st);
    ix->stream_off = false;
    return rc;
}

// CIS_TINY_DEBUG: counters and phase clocks of k_tiny_select, read back after the launch
static int dump_tiny_debug(const Batch& b, const unsigned int* dbg, int tch, int ncmax) {
    const int nq = b.nq;
    unsigned int hd[24];
    CIS_CHECK_HIP(hipMemcpyAsync(hd, dbg, 96, hipMemcpyDeviceToHost, b.st));
    CIS_CHECK_HIP(hipStreamSynchronize(b.st));
    fprintf(stderr, "[tiny] queries %u  flagged %u  survivors/query %.1f  mean s* %.1f  (pool %d B, ncmax %d; tables/query %.1f, items/query %.1f)\n", hd[0], hd[1],
            hd[0] ? (double)hd[2] / hd[0] : 0.0, hd[0] ? (double)hd[3] / hd[0] : 0.0, tch, ncmax, (double)b.n_tabs / nq, (double)b.n_items / nq);
    // 100 MHz ticks of thread 0 per phase, summed over all queries: us per query
    fprintf(stderr, "[tiny] us/query: top %.1f layout %.1f sample %.1f lookups %.1f rows %.1f tables %.1f last lookups %.1f hist+gather %.1f exact %.1f sums+sort %.1f out %.1f\n",
            hd[4] / 100.0 / nq, hd[5] / 100.0 / nq, hd[6] / 100.0 / nq, hd[7] / 100.0 / nq, hd[8] / 100.0 / nq, hd[9] / 100.0 / nq,
            hd[10] / 100.0 / nq, hd[11] / 100.0 / nq, hd[12] / 100.0 / nq, hd[13] / 100.0 / nq, hd[14] / 100.0 / nq);
    fprintf(stderr, "[tiny] half tables with a candidate: %.1f per query; centroid loads %.1f us/query\n", (double)hd[15] / nq, hd[16] / 100.0 / nq);
    return CIS_OK;
}

// 4'. every candidate's exact distance; then per query either a radix select of the `limit` best (ranked in LDS
// for limit <= 3072, by a stable segmented sort of the selected pairs above) or, when `limit` is of the order
// of the candidate count, the stable segmented sort of everything
static int run_all_candidates(Batch& b, const Route& r) {
    cis_index* ix = b.ix;
    cis_model* m = ix->m;
    hipStream_t st = b.st;
    const int K = m->K, M = m->M, h = m->h, nq = b.nq, L = b.L;
    const int64_t quota = b.quota, n_items = b.n_items;
    const WorkItem* items = b.items;
    const int64_t *item_off = b.item_off, *tab_off = b.tab_off, *d_tot = b.d_tot;
    double *T = b.T, *px_buf = b.px_buf;
    const bool direct = r.direct, tiny_cells = r.tiny_cells;
    const SearchOut& out = b.out;
    CIS_TRY(mark(b, 2));
    const int64_t n_cand = b.n_cand_all;
    CIS_REQUIRE(n_cand < ((int64_t)1 << 32), "query batch too large for the sorted path");
    const uint8_t* codes = ix->codes_ptr();
    const int64_t* ids = ix->ids_ptr();
    const SelectPlan sp = select_plan(L, nq, n_cand);
    const int64_t n_sel = sp.select ? (int64_t)nq * sp.stride : 0;
    size_t sort_tmp = 0;
    if (!sp.sort_lds)
        CIS_TRY(cis_seg_sort_u64(nullptr, &sort_tmp, nullptr, nullptr, nullptr, nullptr, sp.select ? n_sel : n_cand, nq, nullptr, nullptr, st));
    const size_t tmp_bytes = (sort_tmp + 255) & ~(size_t)255;
    const size_t n_i64 = (size_t)(n_items + 1) + (size_t)6 * (nq + 2);
    const size_t n_pairs = sp.select ? (size_t)(n_cand + 1) + (size_t)(sp.sort_lds ? 2 : 4) * (n_sel + 1) : (size_t)4 * (n_cand + 1);
    CIS_TRY(ix->w_hits.reserve(n_i64 * 8 + n_pairs * 8 + tmp_bytes + 256));
    int64_t* cand_start = ix->w_hits.as<int64_t>();
    int64_t* seg = cand_start + (n_items + 1);
    int64_t* seg_b = seg + (nq + 2);
    int64_t* seg_e = seg_b + (nq + 2);
    int* nsel = reinterpret_cast<int*>(seg_e + (nq + 2));
    unsigned long long* qmin = reinterpret_cast<unsigned long long*>(seg_e + 2 * (nq + 2));
    unsigned long long* qmax = qmin + (nq + 2);
    uint64_t* keys_in = reinterpret_cast<uint64_t*>(qmax + (nq + 2));
    uint64_t* b1 = keys_in + (n_cand + 1);  // full sort: keys_out, vals_in, vals_out; select: sel_keys, sel_vals[, sorted copies]
    const size_t bl = sp.select ? (size_t)(n_sel + 1) : (size_t)(n_cand + 1);
    uint64_t* b2 = b1 + bl;
    uint64_t* b3 = b2 + bl;
    uint64_t* b4 = b3 + bl;
    void* tmp = reinterpret_cast<void*>(((uintptr_t)(sp.select ? (sp.sort_lds ? b3 : b3 + 2 * bl) : b4) + 255) & ~(uintptr_t)255);
    // (the full sort selects nothing by the key range: the exact kernels do not write it there)
    const CandArgs c{st, items, n_items, item_off, cand_start, seg, sp.select ? qmin : nullptr, sp.select ? qmax : nullptr, nq, codes, K};
    if (n_items > 16384 && !d_tot) {
        const int64_t ntiles = ceil_div(n_items, CAND_TILE);
        CIS_TRY(ix->w_tiles.reserve((size_t)(ntiles + 1) * sizeof(int64_t)));
        int64_t* tile_sums = ix->w_tiles.as<int64_t>();
        hipLaunchKernelGGL(k_cand_tile_sum, dim3((unsigned)ntiles), dim3(256), 0, st, items, n_items, tile_sums);
        hipLaunchKernelGGL(k_cand_tile_scan, dim3(1), dim3(1024), 0, st, tile_sums, ntiles);
        hipLaunchKernelGGL(k_cand_tile_apply, dim3((unsigned)ntiles), dim3(256), 0, st, items, n_items, tile_sums, cand_start);
        hipLaunchKernelGGL(k_seg_begin, dim3((unsigned)ceil_div(nq + 1, 256)), dim3(256), 0, st, cand_start, item_off, nq, n_items, n_cand, seg,
                           sp.select ? qmin : (unsigned long long*)nullptr, qmax);
    } else
        hipLaunchKernelGGL(k_cand_layout, dim3(1), dim3(1024), 0, st, items, n_items, item_off, nq, n_cand, cand_start, seg,
                           sp.select ? qmin : (unsigned long long*)nullptr, qmax, d_tot);
    const uint64_t *rk = nullptr, *rv = nullptr;  // ranked pairs
    if (!sp.select) {
        uint64_t *keys_out = b1, *vals_in = b2, *vals_out = b3;
        if (n_items > 0) {
            if (!(direct && launch_adc_direct(M, m->w, c, px_buf, m->d_subs, h, keys_in, vals_in)))
                launch_adc_all(c, T, M, keys_in, vals_in, nullptr, tiny_cells);
            size_t bb = tmp_bytes;
            CIS_TRY(cis_seg_sort_u64(tmp, &bb, keys_in, keys_out, vals_in, vals_out, n_cand, nq, seg, seg + 1, st));
        }
        rk = keys_out; rv = vals_out;
    } else {
        SelectArgs s{keys_in, L, sp, b1, b2, nsel};
        // tiny cells, limit a small share of the quota: byte-table prefilter + exact keys of the survivors in ONE kernel per
        // query (k_tiny_select); the queries it flags go through the exact kernels below
        int* fbflag = nullptr;
        // (measured at V = 2048, 8192 queries, limit 100: quota 10000 5.16 against 6.35 ms for the exact kernels, quota 1000 2.19 against
        // 1.36 -- the sample, the row copies and the sort are fixed costs per query: from 8192 candidates on)
        const int64_t tiny_min_quota = getenv("CIS_TINY_MIN_QUOTA") ? atoll(getenv("CIS_TINY_MIN_QUOTA")) : 8192;
        if (direct && sp.sort_lds && n_items > 0 && (int64_t)L * 8 <= (int64_t)quota && (int64_t)quota >= tiny_min_quota && !getenv("CIS_NO_TINY")) {
            int ncmax = 0;
            const int tch = tiny_pool(M, K, m->w, h, L, (int64_t)quota + ix->max_cell, &ncmax);  // bytes of the per-query pool
            if (tch > 0) {
                fbflag = nsel + (nq + 2);
                static const bool tiny_dbg = getenv("CIS_TINY_DEBUG") != nullptr;
                unsigned int* dbg = nullptr;
                if (tiny_dbg) {
                    CIS_TRY(ix->w_slack.reserve(128));
                    dbg = ix->w_slack.as<unsigned int>();
                    CIS_CHECK_HIP(hipMemsetAsync(dbg, 0, 96, st));
                }
                if (!launch_tiny(M, m->w, c, s, TinyArgs{tab_off, b.plan, px_buf, m->d_subs, h, ncmax, tch, keys_in, fbflag, b.T32, dbg}))
                    fbflag = nullptr;
                else if (tiny_dbg)
                    CIS_TRY(dump_tiny_debug(b, dbg, tch, ncmax));
            }
        }
        if (fbflag) {
        } else
        if (n_items > 0 && !(direct && launch_adc_direct(M, m->w, c, px_buf, m->d_subs, h, keys_in, nullptr)))
            launch_adc_all(c, T, M, keys_in, nullptr, d_tot, tiny_cells);
        if (sp.sort_lds) {
            s.only = fbflag;
            launch_select<true>(c, s);
            rk = s.sel_keys; rv = s.sel_vals;
        } else {
            uint64_t *srt_keys = b3, *srt_vals = b3 + bl;
            s.seg_b = seg_b; s.seg_e = seg_e;
            launch_select<false>(c, s);
            size_t bb = tmp_bytes;
            CIS_TRY(cis_seg_sort_u64(tmp, &bb, s.sel_keys, srt_keys, s.sel_vals, srt_vals, n_sel, nq, seg_b, seg_e, st));
            rk = srt_keys; rv = srt_vals;
        }
    }
    CIS_TRY(mark(b, 3));
    hipLaunchKernelGGL(k_emit_sorted, dim3((unsigned)ceil_div(L, 1024) < 64 ? (unsigned)ceil_div(L, 1024) : 64, (unsigned)nq), dim3(256), 0, st,
                       rk, rv, seg, sp.select ? nsel : (const int*)nullptr, sp.stride, items, ids, nq, L, out.hits, out.ids, out.dists,
                       out.n_found, out.cells, out.pos);
    if (out.visited)
        hipLaunchKernelGGL(k_copy_visited, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, st, b.plan, nq, out.visited);
    CIS_CHECK_HIP(hipGetLastError());
    CIS_TRY(mark(b, 4));
    if (ix->profiling) ix->prof.push_back(b.pr);
    return CIS_OK;
}

// what the scans of this batch read and write (sl: the slot list, empty for the exact scan)
static ScanArgs scan_args(const Batch& b, const Slots& sl) {
    cis_index* ix = b.ix;
    ScanArgs a{};
    a.st = b.st; a.items = b.items; a.n_items = b.n_items; a.nq = b.nq; a.tabs = b.tabs;
    a.slots = sl.slots; a.n_slots = sl.n_slots; a.plan = b.plan;
    a.T = b.T; a.T32 = b.T32; a.codes = ix->codes_ptr(); a.ids = ix->ids_ptr();
    a.K = ix->m->K; a.L = b.L;
    a.qctr = sl.qctr; a.hits = ix->w_hits.as<uint64_t>(); a.hitn = ix->w_hitn.as<int>(); a.slack = ix->w_slack.as<float>(); a.qbound = b.qbound;
    a.fhdr = sl.fhdr; a.fslots = sl.fslots;
    return a;
}

// 4. ADC scan + block top-k through the slot list
static int run_fast_scan(Batch& b, const Route& r) {
    cis_index* ix = b.ix;
    hipStream_t st = b.st;
    const int M = ix->m->M;
    const bool use3 = r.use3;
    const Scan3Geom& geom3 = r.geom3;
    // slot list: work items grouped by coarse cell (counting sort; skipped for huge V), G per slot
    const bool sort_items = ix->ncells <= 65536;
    const int G = use3 ? geom3.G : r.geom.G;
    // chunks per cell that get their own slot keys: what the largest cell needs (all shards' sizes bound this shard's)
    int64_t CH = use3 ? ceil_div(ix->max_cell > 0 ? ix->max_cell : 1, (int64_t)r.seg_max) : 1;
    CH = CH < 1 ? 1 : (CH > 16 ? 16 : CH);
    Slots sl;
    CIS_TRY(build_slots(b, sort_items ? SLOTS_SORTED : SLOTS_IDENTITY, G, CH, r.seg_max, &sl));
    CIS_TRY(mark(b, 5));
    ix->last_scan_kernel = use3 ? (geom3.two_pass == 2 ? 4 : 3) : 2;  // 4: the sampled single-pass form k_adc_scan4 does the work (k_adc_scan3 only its fall-back slots)
    const ScanArgs a = scan_args(b, sl);
    if (use3) {
        Scan3Geom g3 = geom3;
        // M = 16 on the sampled form: the saturating scale of k_adc_scan4 (sums of the near candidates at this fraction of the entry cap)
        const float sat16 = getenv("CIS_S4_SAT") ? (float)atof(getenv("CIS_S4_SAT")) : 0.75f;
        if (M == 16 && g3.two_pass == 2) g3.sat = sat16;
        launch_scan3(M, g3, a);
        if (g3.sat > 0.f && ix->h_totals)  // (slots, fall-back slots) for the back-off in route_hints
            CIS_CHECK_HIP(hipMemcpyAsync(&ix->h_totals[4], sl.qctr + 9, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    } else
        launch_scan2(M, r.geom, a);
    return CIS_OK;
}

// survivors of the float32 scan: exact re-scoring + ranking (limit <= 440 here)
template <int CAP, int MT, int NEMAX>
static void merge_survivors(const Batch& b, const Route& r) {
    cis_index* ix = b.ix;
    hipStream_t st = b.st;
    const int nq = b.nq, L = b.L, S = r.S, M = ix->m->M, K = ix->m->K;
    const SearchOut& out = b.out;
    const uint64_t* surv = ix->w_hits.as<uint64_t>();
    const int* hitn = ix->w_hitn.as<int>();
    const uint8_t* codes = ix->codes_ptr();
    const int64_t* ids = ix->ids_ptr();
    const float* slack = r.use3 ? ix->w_slack.as<float>() : (const float*)nullptr;
    hipLaunchKernelGGL((k_merge_survivors<CAP, MT, NEMAX>), dim3((unsigned)ceil_div(nq, 4)), dim3(256), (size_t)4 * CAP * 16, st,
                       surv, hitn, b.item_off, b.items, b.T, codes, ids, nq, M, K, L, S, out.hits, out.ids, out.dists,
                       out.n_found, out.cells, out.pos, b.plan, out.visited, slack);
}

// many: several lists per query (short cells) -- the variant whose fast path holds 512 survivors per query
template <int CAP>
static void merge_survivors_m(const Batch& b, const Route& r, bool many) {
    dispatch_int<4, 8, 16>(b.ix->m->M, [&](auto m) {  // (the fast scans serve no other M)
        dispatch_int<4, 8>(many ? 8 : 4, [&](auto ne) { merge_survivors<CAP, decltype(m)::value, decltype(ne)::value>(b, r); });
    });
}

// the exact scan's hits: per-query merge of the work items' ranked lists
template <int CAPM>
static void merge_items(const Batch& b, int S) {
    const SearchOut& out = b.out;
    hipLaunchKernelGGL(k_merge_items<CAPM>, dim3(b.nq), dim3(256), (size_t)CAPM * 24 + 16, b.st, b.ix->w_hits.as<cis_hit>(), b.ix->w_hitn.as<int>(), b.item_off, b.L, S,
                       out.hits, out.ids, out.dists, out.n_found, out.cells, out.pos);
}

// 4. ADC scan + block top-k, 5. per-query merge
static int run_scan_and_merge(Batch& b, const Route& r) {
    cis_index* ix = b.ix;
    hipStream_t st = b.st;
    const int M = ix->m->M, nq = b.nq, L = b.L, S = r.S;
    const int64_t n_items = b.n_items;
    const SearchOut& out = b.out;
    CIS_TRY(mark(b, 2));
    if (n_items > 0) {
        b.pr.has_scan = true;
        if (r.fast) {
            CIS_TRY(run_fast_scan(b, r));
        } else {
            CIS_TRY(mark(b, 5));
            ix->last_scan_kernel = 1;
            launch_scan_exact(M, scan_args(b, Slots{}), S, nullptr);
        }
        ix->stats[3] += 1;
    }
    // 5. per-query merge
    CIS_TRY(mark(b, 3));
    if (r.fast) {
        const bool many = n_items > nq + nq / 4;
        if (L <= 128) merge_survivors_m<256>(b, r, many);
        else if (L <= 256) merge_survivors_m<512>(b, r, many);
        else if (L <= 440) merge_survivors_m<1024>(b, r, many);
        else merge_survivors_m<2048>(b, r, many);
    } else if (L <= 512) merge_items<1024>(b, S);
    else if (L <= 1024) merge_items<2048>(b, S);
    else merge_items<4096>(b, S);
    if (out.visited && !r.fast)  // the survivor merge writes `visited` itself
        hipLaunchKernelGGL(k_copy_visited, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, st, b.plan, nq, out.visited);
    CIS_CHECK_HIP(hipGetLastError());
    CIS_TRY(mark(b, 4));
    if (ix->profiling) ix->prof.push_back(b.pr);
    return CIS_OK;
}

static int search_batch(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota, int L, const SearchOut& out,
                        hipStream_t st) {
    const int V = ix->m->V;
    Batch b{};
    b.ix = ix; b.dQ = dQ; b.q_dtype = q_dtype; b.nq = nq; b.quota = quota; b.L = L; b.out = out; b.st = st;
    b.t_entry = std::chrono::steady_clock::now();
    ix->last_scan_kernel = 0;
    b.pr.has_scan = false;
    for (int i = 0; i < 6; ++i) b.pr.ev[i] = nullptr;
    CIS_TRY(mark(b, 0));
    // 1., 2. LOPQ-space queries, workspaces of the rank and the plan
    CIS_TRY(front_prepare(ix, dQ, q_dtype, nq, st, &b.f));
    CIS_TRY(ix->w_plan.reserve((size_t)nq * sizeof(PlanOut)));
    CIS_TRY(ix->w_off.reserve((size_t)(2 * (nq + 1) + 4 + nq) * sizeof(int64_t)));
    b.item_off = ix->w_off.as<int64_t>();
    b.tab_off = b.item_off + (nq + 1);
    b.totals = b.tab_off + (nq + 1);
    b.qbound = reinterpret_cast<unsigned long long*>(b.totals + 4);
    b.plan = ix->w_plan.as<PlanOut>();
    b.grp_cur = b.f.grp_cnt + 2 * V * GRP_SUB;
    b.grp_base = b.f.grp_cnt + 4 * V * GRP_SUB;
    Route r{};
    route_hints(ix, nq, quota, L, &r);
    b.plan_hint = (r.par_plan && !getenv("CIS_NO_PLAN_HINT")) ? ix->plan_hint_ptr() : nullptr;
    b.hint_slot = (int)((ix->plan_seq + 1) & 1);  // this batch's launches add into this parity and read the other
    // cells WITH candidates per query the fast plan lists (16 bytes each; the empty cells it walks -- most of them at thousands of coarse
    // clusters, tens of thousands for an outlier query -- are not listed): 2 GB of lists per batch at most; past the cap the query goes
    // to the serial frontier walk, ~3 us per cell
    int64_t vis_cap64 = ((int64_t)1 << 31) / ((int64_t)(nq > 0 ? nq : 1) * 16);
    if (vis_cap64 < 4096) vis_cap64 = 4096;
    if (vis_cap64 > (1 << 20)) vis_cap64 = 1 << 20;
    if (vis_cap64 > (int64_t)V * V) vis_cap64 = (int64_t)V * V;
    b.vis_cap = (int)vis_cap64;
    if (r.par_plan) {
        CIS_TRY(ix->w_planfb.reserve((size_t)2 * nq * sizeof(int)));
        CIS_TRY(ix->w_vis.reserve((size_t)nq * b.vis_cap * 2 * sizeof(uint64_t)));
        b.plan_fb = ix->w_planfb.as<int>();
        b.vis_list = ix->w_vis.as<uint64_t>();
    }
    const bool f32 = b.f.ct == CIS_F32;
    CIS_TRY(f32 ? front_count<float>(b, r) : front_count<double>(b, r));
    if (r.par_plan && getenv("CIS_DEBUG_PLAN")) CIS_TRY(dump_plan_fallbacks(b));
    CIS_TRY(plan_totals(b, r));
    CIS_TRY(route_decide(b, &r));
    // 3. emit items + table list
    CIS_TRY(mark(b, 1));  // the plan read-back above is part of the front end
    CIS_TRY(reserve_batch(b, r));
    if (f32) emit_and_tables<float>(b, r);
    else emit_and_tables<double>(b, r);
    finish_tables(b, r);
    if (r.stream) return run_stream(b, r);
    if (r.big) return run_all_candidates(b, r);
    return run_scan_and_merge(b, r);
}

static const int QUERY_BATCH = 8192;

static int search_all(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota, int L, const SearchOut& out,
                      hipStream_t st) {
    CIS_REQUIRE(ix != nullptr, "index is NULL");
    CIS_REQUIRE(q_dtype == CIS_F32 || q_dtype == CIS_F64, "q_dtype must be 4 or 8");
    CIS_REQUIRE(nq >= 0, "nq must be >= 0");
    CIS_REQUIRE(!ix->orphaned, "this view's base index was destroyed: close views before their base");
    CIS_TRY(cis_index_ready(ix->base ? ix->base : ix));
    ix->sync_from_base();  // a view reads the storage of its base
    CIS_CHECK_HIP(hipSetDevice(ix->m->device));
    for (int i = 0; i < 4; ++i) ix->stats[i] = 0;
    ix->stats_pending_seq = 0;
    // a batch that did not fit the workspace is planned again smaller; the size that fitted is remembered for the next
    // call with the same quota (the plan of a rejected batch is wasted front-end time)
    int batch = (ix->batch_hint > 0 && ix->batch_hint_quota == quota) ? ix->batch_hint : QUERY_BATCH;
    for (int a = 0; a < nq;) {
        const int bn = (nq - a < batch) ? (nq - a) : batch;
        const char* q = (const char*)dQ + (size_t)a * ix->m->D_in * q_dtype;
        int rc;
        if (L > 0) {
            rc = search_batch(ix, q, q_dtype, bn, quota, L, out.at(a, L), st);
        } else {  // limit 0: only `visited` is defined
            SearchOut o{};
            o.visited = out.visited ? out.visited + a : nullptr;
            CIS_TRY(ix->w_part.reserve((size_t)bn * sizeof(cis_hit)));
            o.hits = ix->w_part.as<cis_hit>();
            rc = search_batch(ix, q, q_dtype, bn, quota, 1, o, st);
        }
        if (rc == CIS_RETRY_SMALLER) {
            int nb = (int)((double)bn * ix->retry_fraction);
            if (nb > bn / 2 && bn / 2 >= 64) nb = nb / 64 * 64;
            if (nb >= bn) nb = bn / 2;
            batch = nb > 1 ? nb : 1;
            ix->batch_hint = batch;
            ix->batch_hint_quota = quota;
            continue;
        }
        CIS_TRY(rc);
        a += bn;
    }
    return CIS_OK;
}

// lopq_index.h: the door of the packed entry point (lopq_exchange.hip)
int cis_search_partial(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota, int L, cis_hit* d_hits, int32_t* d_n_found,
                       int32_t* d_visited, hipStream_t st) {
    SearchOut o{};
    o.hits = d_hits;
    o.n_found = d_n_found;
    o.visited = d_visited;
    return search_all(ix, dQ, q_dtype, nq, quota, L, o, st);
}

extern "C" int cis_index_search_partial_dev(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota,
                                            int limit, cis_hit* d_hits, int32_t* d_visited, void* stream) {
    int L;
    CIS_TRY(effective_limit(quota, limit, &L));
    SearchOut o{};
    o.hits = d_hits;
    o.visited = d_visited;
    return search_all(ix, dQ, q_dtype, nq, quota, L, o, (hipStream_t)stream);
}

extern "C" int cis_index_search_dev(cis_index* ix, const void* dQ, int q_dtype, int nq, int64_t quota, int limit,
                                    int64_t* d_ids, double* d_dists, int32_t* d_n_found, int32_t* d_visited,
                                    int32_t* d_cells, uint32_t* d_pos, void* stream) {
    int L;
    CIS_TRY(effective_limit(quota, limit, &L));
    if (nq == 0) return CIS_OK;
    SearchOut o{};
    o.ids = d_ids; o.dists = d_dists; o.n_found = d_n_found; o.cells = d_cells; o.pos = d_pos; o.visited = d_visited;
    if (L == 0 && d_n_found) CIS_CHECK_HIP(hipMemsetAsync(d_n_found, 0, (size_t)nq * sizeof(int32_t), (hipStream_t)stream));
    return search_all(ix, dQ, q_dtype, nq, quota, L, o, (hipStream_t)stream);
}
