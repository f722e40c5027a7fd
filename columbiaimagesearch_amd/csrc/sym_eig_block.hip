// Symmetric eigendecomposition of one float64 matrix of 1 <= d <= 4096 that lives in HBM (cis_sym_eig_large_dev): the eigh of the PCA
// stage of LOPQ training (lopq/lopq/model.py:242-287).  Cyclic two-sided block Jacobi; the pivots are solved by the LDS solver of
// sym_eig.hip (cis_sym_eig_launch).
//   The matrix (its lower triangle is read and mirrored) is cut into nb = max(2, ceil(d / b)) blocks of b columns, b = 64 or 32 (by
//   default 32 beyond d = 128, where it measured 2.1 x faster, and 64 up to there, which makes the matrix one pivot), and padded with
//   zero rows and columns to dp = nb b.  A round pairs the blocks as sym_eig.hip's tournament pairs indices (block_pair below): floor(nb / 2) disjoint pairs
//   (I, J), and with an odd nb one block that sits the round out; nb - 1 rounds (nb for an odd nb) are a block sweep.
//   Per round: k_block_gather copies every pair's pivot [[A_II, A_IJ], [A_JI, A_JJ]] (2b x 2b) into a batch, the LDS solver
//   diagonalises the batch (eigenvalues W_P ascending, eigenvectors Q_P, sweeps info_P), k_block_update_a replaces A by Q^T A Q and
//   k_block_update_vt replaces V^T by Q^T V^T, Q = diag(Q_P) over the pairs and the identity on the block that sits out.
//   k_block_status folds the info_P into one status word.  After a block sweep the host reads that word (4 bytes, the call's only
//   wait): done when every pivot reported 1 (its first sweep rotated nothing), failed when a pivot reported -1 or the input was not
//   finite, 40 block sweeps at the most.
//   Padding: the LDS solver never rotates a pair with a_pq == 0, so a padding index is never mixed with another: its row and column of
//   A stay exactly zero and its row of V^T stays a unit vector of the padding, although the pivots' sorting moves it about.  The
//   finalisation drops the rows of V^T that have a nonzero beyond column d, sorts the others by eigenvalue (ties by position: a stable
//   sort) and writes W and V in the layout and with the sign rule of cis_sym_eig_dev.
// The update kernels: a workgroup owns the tile (P, R) of two pairs, 2b x 2b entries in four b x b blocks of A.  It computes
// T = A[P,R] Q_R into LDS and then Q_P^T T, and writes that to A[P,R] and, transposed, to A[R,P]; nothing else reads or writes those
// two tiles in the launch, so the update is in place, and A stays symmetric bit for bit.  Only R >= P is computed; tile (P, P) is
// written as diag(W_P).  Both products are sums over l of outer products of two rows, x_l^T y_l: for T the rows are A[R,P][l, :]
// (= A[P,R][:, l] by symmetry) and Q_R[l, :], for the result Q_P[l, :] and T[l, :].  Rows come from global memory eight at a time,
// through registers into LDS while the previous eight are multiplied (tile_xty); T's rows are read where they lie.  256 threads as
// 16 x 16; a thread keeps (b/8)^2 sums for the rows 32 a + 2 ty + {0, 1} and columns 32 c + 2 tx + {0, 1}, so that every LDS read
// is 16 bytes: 16 consecutive slots over tx, a broadcast over ty.  Explicit fma (the file is compiled with -ffp-contract=off).
// LDS: (2b)^2 + 2 * 8 * 2b doubles: 144 KiB at b = 64 (one workgroup per CU), 40 KiB at b = 32.
#include "common.h"
#include "sym_eig.h"

namespace {

constexpr int BLK_MAX_D = 4096;
constexpr int BLK_MAX_SWEEPS = 40;
constexpr int BLK_NT = 256;
constexpr int BLK_KC = 8;         // rows staged at a time
constexpr int BLK_DEFAULT_B = 32;  // beyond d = 128; measured 2.1 x faster than 64 at d = 512 ... 4096

// status word: bit 0 a pivot rotated in this block sweep, bit 1 a pivot failed or the input was not finite
constexpr int ST_ROTATED = 1, ST_FAILED = 2;

// a 16-byte load or store of two doubles.  The compiler's own vector type: with HIP's double2 the staged rows of tile_xty (px, py)
// were kept in private memory at b = 64 (80 and 48 bytes of scratch in the listing, and a full wait behind every load)
typedef double v2d __attribute__((ext_vector_type(2)));

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct BlockPlan {
    int b, nb, dp, npairs, rounds;
    size_t off_a, off_vt, off_piv, off_q, off_wp, off_w, off_sgn, off_src, off_real, off_pinfo, off_status, bytes;
};

BlockPlan block_plan(int d, int b) {
    BlockPlan p;
    p.b = b;
    p.nb = (d + b - 1) / b < 2 ? 2 : (d + b - 1) / b;
    p.dp = p.nb * b;
    p.npairs = p.nb / 2;
    p.rounds = p.nb + (p.nb & 1) - 1;
    const size_t w = 2 * (size_t)b, mat = (size_t)p.dp * p.dp * sizeof(double), piv = (size_t)p.npairs * w * w * sizeof(double);
    size_t o = 0;
    p.off_a = o;      o += up256(mat);
    p.off_vt = o;     o += up256(mat);
    p.off_piv = o;    o += up256(piv);
    p.off_q = o;      o += up256(piv);
    p.off_wp = o;     o += up256((size_t)p.npairs * w * sizeof(double));
    p.off_w = o;      o += up256((size_t)p.dp * sizeof(double));
    p.off_sgn = o;    o += up256((size_t)p.dp * sizeof(double));
    p.off_src = o;    o += up256((size_t)p.dp * sizeof(int));
    p.off_real = o;   o += up256((size_t)p.dp * sizeof(int));
    p.off_pinfo = o;  o += up256((size_t)p.npairs * sizeof(int));
    p.off_status = o; o += 256;
    p.bytes = o;
    return p;
}

// The blocks I < J of pair k of round r over nb blocks: the seats of sym_eig.hip's tournament over m = nb rounded up to even (seat 0
// holds block 0, seat s >= 1 holds 1 + (s - 1 - r) mod (m - 1), pair k joins seats k and m - 1 - k).  With an odd nb the padding
// block m - 1 sits in seat r (seat m - 1 in round 0); its pair is left out and k counts the others.
__device__ __forceinline__ int block_seat(int m, int r, int s) { return s == 0 ? 0 : 1 + (s - 1 - r + (m - 1)) % (m - 1); }

__device__ __forceinline__ void block_pair(int nb, int r, int k, int& I, int& J) {
    const int m = nb + (nb & 1);
    if (nb & 1) {
        const int s = r == 0 ? m - 1 : r, kb = s < m - 1 - s ? s : m - 1 - s;
        if (k >= kb) ++k;
    }
    const int a = block_seat(m, r, k), b = block_seat(m, r, m - 1 - k);
    I = a < b ? a : b;
    J = a < b ? b : a;
}

// odd nb: the block that sits round r out (the one paired with the padding block)
__device__ __forceinline__ int block_bye(int nb, int r) {
    const int m = nb + 1, s = r == 0 ? m - 1 : r;
    return block_seat(m, r, m - 1 - s);
}

// A 2B x 2B tile made of four B x B blocks of a row-major matrix: element (l, i) lies at row (l < B ? r0 + l : r1 + l - B) and
// column (i < B ? c0 + i : c1 + i - B).  Every offset and ld are even and p is 16-byte aligned, so an even i is.
// r1 and c1 are kept as what the second half adds to the first (rd, cd).
struct TileView {
    const double* p;
    int64_t ld;
    int r0, rd, c0, cd;
};

template <int B>
__device__ __forceinline__ TileView tile_view(const double* p, int64_t ld, int r0, int r1, int c0, int c1) {
    return TileView{p, ld, r0, r1 - B - r0, c0, c1 - B - c0};
}

template <int B>
__device__ __forceinline__ int64_t tile_off(const TileView v, int l, int i) {
    return (int64_t)(v.r0 + l + (l >= B ? v.rd : 0)) * v.ld + (v.c0 + i + (i >= B ? v.cd : 0));
}

// the a-th of a thread's B/8 rows (t = ty) or columns (t = tx) of the tile
__device__ __forceinline__ int tile_idx(int a, int t) { return 32 * (a >> 1) + 2 * t + (a & 1); }

// acc[a][c] += sum over l < 2B of x_l[tile_idx(a, ty)] * y_l[tile_idx(c, tx)].  x_l is row l of X (global memory); y_l is row l of Y
// (global memory), or of the tile sT in LDS (Y_LDS).  sx and sy hold BLK_KC rows each.  Begins with a barrier, ends without one.
template <int B, bool Y_LDS>
__device__ __forceinline__ void tile_xty(const TileView X, const TileView Y, const double* sT, double* sx, double* sy,
                                         double (&acc)[B / 8][B / 8], int tid) {
    constexpr int W = 2 * B, N = B / 8, PER = BLK_KC * W / 2 / BLK_NT;
    static_assert(PER * BLK_NT * 2 == BLK_KC * W, "a staged chunk is a whole number of 16-byte loads per thread");
    const int ty = tid >> 4, tx = tid & 15;
    v2d px[PER], py[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int idx = tid + BLK_NT * u, l = idx / (W / 2), i = 2 * (idx % (W / 2));
        px[u] = *reinterpret_cast<const v2d*>(X.p + tile_off<B>(X, l, i));
        if (!Y_LDS) py[u] = *reinterpret_cast<const v2d*>(Y.p + tile_off<B>(Y, l, i));
    }
    for (int l0 = 0; l0 < W; l0 += BLK_KC) {
        __syncthreads();  // the previous rows have been used
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = tid + BLK_NT * u;
            *reinterpret_cast<v2d*>(sx + 2 * idx) = px[u];
            if (!Y_LDS) *reinterpret_cast<v2d*>(sy + 2 * idx) = py[u];
        }
        __syncthreads();
        if (l0 + BLK_KC < W) {  // the next rows travel while these are multiplied
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int idx = tid + BLK_NT * u, l = l0 + BLK_KC + idx / (W / 2), i = 2 * (idx % (W / 2));
                px[u] = *reinterpret_cast<const v2d*>(X.p + tile_off<B>(X, l, i));
                if (!Y_LDS) py[u] = *reinterpret_cast<const v2d*>(Y.p + tile_off<B>(Y, l, i));
            }
        }
        const double* yb = Y_LDS ? sT + l0 * W : sy;
#pragma unroll
        for (int l = 0; l < BLK_KC; ++l) {
            double x[N], y[N];
#pragma unroll
            for (int a = 0; a < N; a += 2) {
                const v2d v = *reinterpret_cast<const v2d*>(sx + l * W + tile_idx(a, ty));
                x[a] = v.x;
                x[a + 1] = v.y;
                const v2d w = *reinterpret_cast<const v2d*>(yb + l * W + tile_idx(a, tx));
                y[a] = w.x;
                y[a + 1] = w.y;
            }
#pragma unroll
            for (int a = 0; a < N; ++a)
#pragma unroll
                for (int c = 0; c < N; ++c) acc[a][c] = fma(x[a], y[c], acc[a][c]);
        }
    }
}

template <int B>
constexpr size_t tile_lds_bytes() { return ((size_t)4 * B * B + 2 * BLK_KC * 2 * B) * sizeof(double); }

}  // namespace

// grid (dp): row i of the padded copy of A and of V^T = I; a value that is not finite sets ST_FAILED
__global__ __launch_bounds__(BLK_NT) void k_block_load(const double* __restrict__ A, int d, int dp, double* __restrict__ Ap,
                                                       double* __restrict__ VT, int* __restrict__ status) {
    const int i = blockIdx.x;
    bool finite = true;
    for (int j = threadIdx.x; j < dp; j += BLK_NT) {
        double a = 0.0;
        if (i < d && j < d) {
            a = i >= j ? A[(int64_t)i * d + j] : A[(int64_t)j * d + i];  // the lower triangle, as numpy.linalg.eigh reads it
            finite = finite && (fabs(a) <= 1.7976931348623157e308);  // false for NaN and for +-Inf
        }
        Ap[(int64_t)i * dp + j] = a;
        VT[(int64_t)i * dp + j] = i == j ? 1.0 : 0.0;
    }
    if (!finite) atomicOr(status, ST_FAILED);
}

// grid (npairs): piv[k] = the 2B x 2B pivot of pair k
template <int B>
__global__ __launch_bounds__(BLK_NT) void k_block_gather(const double* __restrict__ A, int dp, int nb, int round, double* __restrict__ piv) {
    constexpr int W = 2 * B;
    int I, J;
    block_pair(nb, round, blockIdx.x, I, J);
    const TileView v = tile_view<B>(A, dp, I * B, J * B, I * B, J * B);
    double* out = piv + (int64_t)blockIdx.x * W * W;
    for (int e = threadIdx.x; e < W * W / 2; e += BLK_NT) {
        const int l = e / (W / 2), i = 2 * (e % (W / 2));
        *reinterpret_cast<v2d*>(out + l * W + i) = *reinterpret_cast<const v2d*>(A + tile_off<B>(v, l, i));
    }
}

// one workgroup: the pivots' reports of a round into the status word
__global__ __launch_bounds__(BLK_NT) void k_block_status(const int* __restrict__ pinfo, int npairs, int* __restrict__ status) {
    int s = 0;
    for (int k = threadIdx.x; k < npairs; k += BLK_NT) {
        const int v = pinfo[k];
        s |= v < 0 ? ST_FAILED : (v != 1 ? ST_ROTATED : 0);
    }
    if (s) atomicOr(status, s);
}

// grid (groups, npairs), groups = npairs + (nb & 1): tile (P = blockIdx.y, R = blockIdx.x) of A <- Q^T A Q for R >= P, and its
// mirror image.  The block that sits the round out is group npairs: a tile of one block column (Q = I on it), the rest of the tile
// is computed on zeros and not written.
template <int B>
__global__ __launch_bounds__(BLK_NT) void k_block_update_a(double* A, int dp, int nb, int round, int npairs,
                                                           const double* __restrict__ Q, const double* __restrict__ Wp) {
    constexpr int W = 2 * B, N = B / 8;
    extern __shared__ __align__(16) unsigned char blk_lds[];
    double* sT = reinterpret_cast<double*>(blk_lds);
    double* sx = sT + W * W;
    double* sy = sx + BLK_KC * W;
    const int P = blockIdx.y, R = blockIdx.x, tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    if (R < P) return;
    int pi, pj;
    block_pair(nb, round, P, pi, pj);
    const int pr0 = pi * B, pr1 = pj * B;
    if (R == P) {
        const double* w = Wp + (int64_t)P * W;
        for (int e = tid; e < W * W; e += BLK_NT) {
            const int i = e / W, j = e - i * W;
            A[(int64_t)(i < B ? pr0 + i : pr1 + i - B) * dp + (j < B ? pr0 + j : pr1 + j - B)] = i == j ? w[i] : 0.0;
        }
        return;
    }
    const bool bye = R >= npairs;
    int ri, rj;
    if (bye) {
        ri = rj = block_bye(nb, round);
    } else {
        block_pair(nb, round, R, ri, rj);
    }
    const int rr0 = ri * B, rr1 = rj * B;
    double acc[N][N];
    if (bye) {  // T = A[P, the block]: nothing to multiply on the right
        for (int e = tid; e < W * W / 2; e += BLK_NT) {
            const int i = e / (W / 2), j = 2 * (e % (W / 2));
            v2d v = {0.0, 0.0};
            if (j < B) v = *reinterpret_cast<const v2d*>(A + (int64_t)(i < B ? pr0 + i : pr1 + i - B) * dp + rr0 + j);
            *reinterpret_cast<v2d*>(sT + i * W + j) = v;
        }
    } else {    // T = A[P,R] Q_R; column l of A[P,R] is read as row l of A[R,P]
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int c = 0; c < N; ++c) acc[a][c] = 0.0;
        const TileView X = tile_view<B>(A, dp, rr0, rr1, pr0, pr1);
        const TileView Y = tile_view<B>(Q + (int64_t)R * W * W, W, 0, B, 0, B);
        tile_xty<B, false>(X, Y, nullptr, sx, sy, acc, tid);
#pragma unroll
        for (int a = 0; a < N; ++a)
#pragma unroll
            for (int c = 0; c < N; c += 2) {
                const v2d v = {acc[a][c], acc[a][c + 1]};
                *reinterpret_cast<v2d*>(sT + tile_idx(a, ty) * W + tile_idx(c, tx)) = v;
            }
    }
    // Q_P^T T (tile_xty's first barrier stands between the writes of T above and its reads)
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int c = 0; c < N; ++c) acc[a][c] = 0.0;
    const TileView X = tile_view<B>(Q + (int64_t)P * W * W, W, 0, B, 0, B);
    tile_xty<B, true>(X, X, sT, sx, sy, acc, tid);
#pragma unroll
    for (int a = 0; a < N; ++a) {
        const int i = tile_idx(a, ty), gi = i < B ? pr0 + i : pr1 + i - B;
#pragma unroll
        for (int c = 0; c < N; c += 2) {
            const int j = tile_idx(c, tx), gj = j < B ? rr0 + j : rr1 + j - B;
            if (!bye || j < B) {
                const v2d v = {acc[a][c], acc[a][c + 1]};
                *reinterpret_cast<v2d*>(A + (int64_t)gi * dp + gj) = v;
                A[(int64_t)gj * dp + gi] = v.x;
                A[(int64_t)(gj + 1) * dp + gi] = v.y;
            }
        }
    }
}

// grid (ceil(dp / 2B), npairs): rows R = blockIdx.y of V^T, 2B columns from blockIdx.x * 2B (B columns in a last odd chunk):
// V^T[R, chunk] <- Q_R^T V^T[R, chunk].  The whole tile is in LDS before anything is written.
template <int B>
__global__ __launch_bounds__(BLK_NT) void k_block_update_vt(double* VT, int dp, int nb, int round, const double* __restrict__ Q) {
    constexpr int W = 2 * B, N = B / 8;
    extern __shared__ __align__(16) unsigned char blk_lds[];
    double* sT = reinterpret_cast<double*>(blk_lds);
    double* sx = sT + W * W;
    double* sy = sx + BLK_KC * W;
    const int R = blockIdx.y, tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int c0 = blockIdx.x * W, ncol = dp - c0 < W ? dp - c0 : W;  // W or B
    int ri, rj;
    block_pair(nb, round, R, ri, rj);
    const int rr0 = ri * B, rr1 = rj * B;
    for (int e = tid; e < W * W / 2; e += BLK_NT) {
        const int l = e / (W / 2), j = 2 * (e % (W / 2));
        v2d v = {0.0, 0.0};
        if (j < ncol) v = *reinterpret_cast<const v2d*>(VT + (int64_t)(l < B ? rr0 + l : rr1 + l - B) * dp + c0 + j);
        *reinterpret_cast<v2d*>(sT + l * W + j) = v;
    }
    double acc[N][N];
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int c = 0; c < N; ++c) acc[a][c] = 0.0;
    const TileView X = tile_view<B>(Q + (int64_t)R * W * W, W, 0, B, 0, B);
    tile_xty<B, true>(X, X, sT, sx, sy, acc, tid);
#pragma unroll
    for (int a = 0; a < N; ++a) {
        const int i = tile_idx(a, ty), gi = i < B ? rr0 + i : rr1 + i - B;
#pragma unroll
        for (int c = 0; c < N; c += 2) {
            const int j = tile_idx(c, tx);
            if (j < ncol) {
                const v2d v = {acc[a][c], acc[a][c + 1]};
                *reinterpret_cast<v2d*>(VT + (int64_t)gi * dp + c0 + j) = v;
            }
        }
    }
}

// grid (dp): row j of V^T.  w[j] = A[j][j]; real[j] = 0 for a unit vector of the padding (a nonzero at a column >= d); sgn[j] makes
// the component of largest magnitude among the first d positive, the lowest index winning a tie.
__global__ __launch_bounds__(BLK_NT) void k_block_fin_rows(const double* __restrict__ A, const double* __restrict__ VT, int d, int dp,
                                                           double* __restrict__ w, double* __restrict__ sgn, int* __restrict__ real,
                                                           int* __restrict__ src) {
    __shared__ double s_abs[BLK_NT], s_val[BLK_NT];
    __shared__ int s_idx[BLK_NT], s_pad;
    const int j = blockIdx.x, tid = threadIdx.x;
    const double* row = VT + (int64_t)j * dp;
    if (tid == 0) s_pad = 0;
    __syncthreads();
    bool pad = false;
    for (int i = d + tid; i < dp; i += BLK_NT) pad = pad || row[i] != 0.0;
    if (pad) s_pad = 1;
    double best = -1.0, val = 1.0;
    int at = 0x7fffffff;
    for (int i = tid; i < d; i += BLK_NT) {
        const double x = row[i];
        if (fabs(x) > best) { best = fabs(x); val = x; at = i; }
    }
    s_abs[tid] = best;
    s_val[tid] = val;
    s_idx[tid] = at;
    __syncthreads();
    for (int h = BLK_NT / 2; h > 0; h >>= 1) {
        if (tid < h && (s_abs[tid + h] > s_abs[tid] || (s_abs[tid + h] == s_abs[tid] && s_idx[tid + h] < s_idx[tid]))) {
            s_abs[tid] = s_abs[tid + h];
            s_val[tid] = s_val[tid + h];
            s_idx[tid] = s_idx[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        w[j] = A[(int64_t)j * dp + j];
        sgn[j] = s_val[0] < 0.0 ? -1.0 : 1.0;
        real[j] = s_pad ? 0 : 1;
        if (j < d) src[j] = j;  // every slot holds a valid row, whatever k_block_fin_rank leaves unwritten
    }
}

// threads over the rows of V^T: the rank of a real row's eigenvalue among the real rows (ties by position), src[rank] = row
__global__ __launch_bounds__(BLK_NT) void k_block_fin_rank(const double* __restrict__ w, const int* __restrict__ real, int d, int dp,
                                                           double* __restrict__ W, int* __restrict__ src, int32_t* __restrict__ info,
                                                           int sweeps) {
    const int j = blockIdx.x * BLK_NT + threadIdx.x;
    if (j == 0 && info) *info = sweeps;
    if (j >= dp || !real[j]) return;
    const double wj = w[j];
    int rank = 0;
    for (int i = 0; i < dp; ++i) {
        const double wi = w[i];
        rank += (real[i] && (wi < wj || (wi == wj && i < j))) ? 1 : 0;
    }
    if (rank < d) {  // always, while exactly dp - d rows are the padding's
        src[rank] = j;
        W[rank] = wj;
    }
}

// grid (ceil(d / 32), ceil(d / 32)), block (32, 8): V[i][r] = V^T[src[r]][i] * sgn[src[r]], a 32 x 32 transpose through LDS
__global__ __launch_bounds__(256) void k_block_fin_write(const double* __restrict__ VT, const double* __restrict__ sgn,
                                                         const int* __restrict__ src, int d, int dp, double* __restrict__ V) {
    __shared__ double s[32][33];
    const int i0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x, ty = threadIdx.y;
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, i = i0 + tx;
        double x = 0.0;
        if (r < d && i < d) {
            const int sr = src[r];
            x = VT[(int64_t)sr * dp + i] * sgn[sr];
        }
        s[k][tx] = x;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int i = i0 + k, r = r0 + tx;
        if (i < d && r < d) V[(int64_t)i * d + r] = s[tx][k];
    }
}

__global__ void k_block_set_info(int32_t* info, int value) { *info = value; }

namespace {

template <int B>
int run_block_jacobi(const BlockPlan& p, const double* d_A, int d, double* d_W, double* d_V, int32_t* d_info, char* ws, hipStream_t st) {
    constexpr int W = 2 * B;
    double* Ap = reinterpret_cast<double*>(ws + p.off_a);
    double* VT = reinterpret_cast<double*>(ws + p.off_vt);
    double* piv = reinterpret_cast<double*>(ws + p.off_piv);
    double* Q = reinterpret_cast<double*>(ws + p.off_q);
    double* Wp = reinterpret_cast<double*>(ws + p.off_wp);
    double* w = reinterpret_cast<double*>(ws + p.off_w);
    double* sgn = reinterpret_cast<double*>(ws + p.off_sgn);
    int* src = reinterpret_cast<int*>(ws + p.off_src);
    int* real = reinterpret_cast<int*>(ws + p.off_real);
    int* pinfo = reinterpret_cast<int*>(ws + p.off_pinfo);
    int* status = reinterpret_cast<int*>(ws + p.off_status);
    const size_t lds = tile_lds_bytes<B>();
    CIS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_block_update_a<B>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    CIS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_block_update_vt<B>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    CIS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_block_load, dim3(p.dp), dim3(BLK_NT), 0, st, d_A, d, p.dp, Ap, VT, status);
    const int groups = p.npairs + (p.nb & 1);
    int sweeps = 0;
    bool done = false, failed = false;
    while (!done && !failed && sweeps < BLK_MAX_SWEEPS) {
        for (int r = 0; r < p.rounds; ++r) {
            hipLaunchKernelGGL(k_block_gather<B>, dim3(p.npairs), dim3(BLK_NT), 0, st, Ap, p.dp, p.nb, r, piv);
            CIS_TRY(cis_sym_eig_launch(piv, p.npairs, W, Wp, Q, pinfo, st));
            hipLaunchKernelGGL(k_block_update_a<B>, dim3(groups, p.npairs), dim3(BLK_NT), lds, st, Ap, p.dp, p.nb, r, p.npairs, Q, Wp);
            hipLaunchKernelGGL(k_block_update_vt<B>, dim3((p.dp + W - 1) / W, p.npairs), dim3(BLK_NT), lds, st, VT, p.dp, p.nb, r, Q);
            hipLaunchKernelGGL(k_block_status, dim3(1), dim3(BLK_NT), 0, st, pinfo, p.npairs, status);
        }
        CIS_CHECK_HIP(hipGetLastError());
        ++sweeps;
        int h = 0;
        CIS_CHECK_HIP(hipMemcpyAsync(&h, status, sizeof(int), hipMemcpyDeviceToHost, st));
        CIS_CHECK_HIP(hipStreamSynchronize(st));
        failed = (h & ST_FAILED) != 0;
        done = !failed && !(h & ST_ROTATED);
        if (!done && !failed) CIS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int), st));
    }
    if (!done) {
        if (d_info) hipLaunchKernelGGL(k_block_set_info, dim3(1), dim3(1), 0, st, d_info, -1);
        CIS_CHECK_HIP(hipGetLastError());
        return CIS_OK;
    }
    hipLaunchKernelGGL(k_block_fin_rows, dim3(p.dp), dim3(BLK_NT), 0, st, Ap, VT, d, p.dp, w, sgn, real, src);
    hipLaunchKernelGGL(k_block_fin_rank, dim3((p.dp + BLK_NT - 1) / BLK_NT), dim3(BLK_NT), 0, st, w, real, d, p.dp, d_W, src, d_info, sweeps);
    hipLaunchKernelGGL(k_block_fin_write, dim3((d + 31) / 32, (d + 31) / 32), dim3(32, 8), 0, st, VT, sgn, src, d, p.dp, d_V);
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

}  // namespace

extern "C" int64_t cis_sym_eig_large_workspace(int d) {
    if (d < 1 || d > BLK_MAX_D) {
        cis_set_error("d must be in 1 .. %d, got %d", BLK_MAX_D, d);
        return CIS_EINVAL;
    }
    const size_t a = block_plan(d, 32).bytes, b = block_plan(d, 64).bytes;
    return (int64_t)(a > b ? a : b);
}

extern "C" int cis_sym_eig_large_dev(const double* d_A, int d, int block, double* d_W, double* d_V, int32_t* d_info, void* d_work,
                                     int64_t work_bytes, void* stream) {
    CIS_REQUIRE(d >= 1 && d <= BLK_MAX_D, "d must be in 1 .. %d, got %d", BLK_MAX_D, d);
    CIS_REQUIRE(block == 0 || block == 32 || block == 64, "block must be 0 (the default), 32 or 64, got %d", block);
    CIS_REQUIRE(d_A && d_W && d_V && d_work, "NULL d_A, d_W, d_V or d_work");
    const int64_t need = cis_sym_eig_large_workspace(d);
    CIS_REQUIRE(work_bytes >= need, "the workspace for d = %d is %lld bytes (cis_sym_eig_large_workspace), got %lld", d, (long long)need,
                (long long)work_bytes);
    CIS_REQUIRE(((uintptr_t)d_work & 255) == 0, "d_work must be aligned to 256 bytes");
    CIS_TRY(cis_lazy_init());
    hipStream_t st = (hipStream_t)stream;
    // a matrix that is one pivot of the LDS solver (d <= 128) is cut so that it is one: its eigenvalues are cis_sym_eig_dev's
    const int b = block ? block : (d <= 128 ? 64 : BLK_DEFAULT_B);
    const BlockPlan p = block_plan(d, b);
    if (b == 64) return run_block_jacobi<64>(p, d_A, d, d_W, d_V, d_info, (char*)d_work, st);
    return run_block_jacobi<32>(p, d_A, d, d_W, d_V, d_info, (char*)d_work, st);
}
