// Batched symmetric eigendecomposition, float64, d <= 128 (cis_sym_eig_dev): the per-cluster eigh of the local-rotation stage of LOPQ
// training (lopq/lopq/model.py:158-176) on covariances that are already on the device.  One workgroup per matrix, cyclic Jacobi in a
// round-robin tournament ordering: a round holds floor(d/2) disjoint pairs (p, q), so all of its rotations commute and run at once.
//   round r of m - 1 (m = d rounded up to even): seat 0 holds index 0, seat s >= 1 holds 1 + (s - 1 - r) mod (m - 1); pair k joins
//   seats k and m - 1 - k; a pair that holds the padding index d (odd d) sits the round out.
//   rotation: tau = (a_qq - a_pp) / (2 a_pq), t = sign(tau) / (|tau| + sqrt(1 + tau^2)) (t = 1 at tau = 0), c = 1 / sqrt(1 + t^2),
//   s = t c; skipped when a_pq == 0 or |a_pq| <= 2^-53 sqrt(|a_pp a_qq|).  All column updates of a round, then all row updates, then
//   the same (c, s) on the eigenvectors.  Done after a sweep that rotated nothing; 40 sweeps at the most.
// Every product and sum below rounds on its own (the Makefile's -ffp-contract=off, and no fma()): with c == s the two products that
// cancel in a rotated off-diagonal entry are equal, so a 2 x 2 block with equal diagonal is diagonalised exactly in one rotation.
//
// Memory: A lives in LDS with a leading dimension of d | 1 doubles.  The column phase walks i for a fixed column: byte address
// 8 (i ld + p), dword bank 2 (i ld + p) mod 64 for the 8-byte reads (32-lane groups) and mod 32 for the writes (16-lane groups); an
// odd ld makes i ld mod 32 a permutation of 32 consecutive i, so neither conflicts.  The row phase walks j along a row: consecutive
// addresses.  The eigenvectors are kept transposed (row j = vector j), so their update is a row phase too.  For d <= 64 they sit in
// LDS behind A (2 x 33 KiB at d = 64: two workgroups per CU); beyond, A alone takes up to 132 KiB of the 160 KiB a workgroup may
// have, and the transposed vectors live in the matrix's own slice of d_V (128 KiB, read and written by this workgroup only, between
// barriers; it stays in the caches), which is read back into A's LDS at the end and written out in its final layout.
#include "common.h"
#include "sym_eig.h"

namespace {

constexpr int EIG_MAX_D = 128;
constexpr int EIG_MAX_SWEEPS = 40;

// LDS behind the matrices: the round's rotations, the eigenvalues, their order and signs, and two flags
struct EigSmall {
    double c[EIG_MAX_D / 2], s[EIG_MAX_D / 2], w[EIG_MAX_D], sgn[EIG_MAX_D];
    int p[EIG_MAX_D / 2], q[EIG_MAX_D / 2], src[EIG_MAX_D];
    int rotated, bad;
};

__host__ __device__ inline int eig_ld(int d) { return d | 1; }
inline size_t eig_lds_bytes(int d, bool v_in_lds) { return (size_t)(v_in_lds ? 2 : 1) * d * eig_ld(d) * sizeof(double) + sizeof(EigSmall); }

}  // namespace

// grid (batch); block NT.  VLDS: the transposed eigenvectors are in LDS (d <= 64), otherwise in this matrix's slice of V.
template <int NT, bool VLDS>
__global__ __launch_bounds__(NT) void k_sym_eig(const double* __restrict__ A, int d, double* __restrict__ W, double* V, int* __restrict__ info) {
    extern __shared__ __align__(16) unsigned char eig_lds[];
    const int ld = eig_ld(d), tid = threadIdx.x;
    double* sA = reinterpret_cast<double*>(eig_lds);
    double* sV = sA + d * ld;  // VLDS only
    EigSmall& sm = *reinterpret_cast<EigSmall*>(sA + (VLDS ? 2 : 1) * d * ld);
    const int64_t mat = blockIdx.x;
    const double* Ag = A + mat * d * d;
    double* Vg = V + mat * d * d;
    double* vt = VLDS ? sV : Vg;          // [d][vld], row j = eigenvector j
    const int vld = VLDS ? ld : d;

    if (tid == 0) { sm.rotated = 0; sm.bad = 0; }
    __syncthreads();
    bool finite = true;
    for (int e = tid; e < d * d; e += NT) {
        const int i = e / d, j = e - i * d;
        const double a = Ag[e];
        finite = finite && (fabs(a) <= 1.7976931348623157e308);  // false for NaN and for +-Inf
        sA[i * ld + j] = a;
        vt[i * vld + j] = i == j ? 1.0 : 0.0;
    }
    if (!finite) sm.bad = 1;
    __syncthreads();
    const bool bad = sm.bad != 0;

    const int m = d + (d & 1), half = m >> 1;
    int sweeps = 0;
    bool done = bad || d == 1;
    if (d == 1) sweeps = 1;
    while (!done && sweeps < EIG_MAX_SWEEPS) {
        for (int r = 0; r < m - 1; ++r) {
            if (tid < half) {
                const int k = tid, s1 = m - 1 - k;
                const int a = k == 0 ? 0 : 1 + (k - 1 - r + (m - 1)) % (m - 1);
                const int b = 1 + (s1 - 1 - r + (m - 1)) % (m - 1);
                const int p = a < b ? a : b, q = a < b ? b : a;
                double c = 1.0, s = 0.0;
                if (q < d) {
                    const double app = sA[p * ld + p], aqq = sA[q * ld + q], apq = sA[p * ld + q];
                    if (apq != 0.0 && fabs(apq) > 0x1p-53 * sqrt(fabs(app * aqq))) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double t = tau == 0.0 ? 1.0 : copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                        sm.rotated = 1;
                    }
                }
                sm.p[k] = p;
                sm.q[k] = q;
                sm.c[k] = c;
                sm.s[k] = s;
            }
            __syncthreads();
            // columns: A[:, p], A[:, q] = c A[:, p] - s A[:, q], s A[:, p] + c A[:, q]; lanes walk i
            for (int e = tid; e < half * d; e += NT) {
                const int k = e / d, i = e - k * d;
                const int q = sm.q[k];
                const double s = sm.s[k];
                if (q < d && s != 0.0) {
                    const double c = sm.c[k];
                    double* xp = sA + i * ld + sm.p[k];
                    double* xq = sA + i * ld + q;
                    const double ap = *xp, aq = *xq;
                    *xp = c * ap - s * aq;
                    *xq = s * ap + c * aq;
                }
            }
            __syncthreads();
            // rows of A and of the transposed eigenvectors; lanes walk j
            for (int e = tid; e < half * d; e += NT) {
                const int k = e / d, j = e - k * d;
                const int q = sm.q[k];
                const double s = sm.s[k];
                if (q < d && s != 0.0) {
                    const double c = sm.c[k];
                    const int p = sm.p[k];
                    double* xp = sA + p * ld + j;
                    double* xq = sA + q * ld + j;
                    const double ap = *xp, aq = *xq;
                    *xp = c * ap - s * aq;
                    *xq = s * ap + c * aq;
                    double* vp = vt + p * vld + j;
                    double* vq = vt + q * vld + j;
                    const double bp = *vp, bq = *vq;
                    *vp = c * bp - s * bq;
                    *vq = s * bp + c * bq;
                }
            }
            __syncthreads();
        }
        ++sweeps;
        done = sm.rotated == 0;
        __syncthreads();  // everybody has read the flag
        if (tid == 0) sm.rotated = 0;
        __syncthreads();
    }

    // eigenvalues ascending: a rank sort, ties by index (a stable sort); src[rank] = the vector that goes to column `rank`
    if (tid < d) {
        sm.w[tid] = sA[tid * ld + tid];
        sm.src[tid] = tid;  // every slot holds a valid index even if NaNs leave ranks unused
    }
    __syncthreads();
    if (!VLDS) {  // A is no longer needed: bring the transposed eigenvectors into its LDS
        for (int e = tid; e < d * d; e += NT) {
            const int i = e / d, j = e - i * d;
            sA[i * ld + j] = Vg[e];
        }
    }
    __syncthreads();
    const double* fv = VLDS ? sV : sA;  // [d][ld]
    if (tid < d) {
        const double wj = sm.w[tid];
        int rank = 0;
        for (int i = 0; i < d; ++i) {
            const double wi = sm.w[i];
            rank += (wi < wj || (wi == wj && i < tid)) ? 1 : 0;
        }
        // the component of largest magnitude is positive, the lowest index wins a tie
        double best = -1.0, val = 1.0;
        for (int i = 0; i < d; ++i) {
            const double x = fv[tid * ld + i];
            if (fabs(x) > best) { best = fabs(x); val = x; }
        }
        sm.sgn[tid] = val < 0.0 ? -1.0 : 1.0;
        sm.src[rank] = tid;
    }
    __syncthreads();
    if (tid < d) W[mat * d + tid] = sm.w[sm.src[tid]];
    for (int e = tid; e < d * d; e += NT) {
        const int i = e / d, j = e - i * d;
        const int sj = sm.src[j];
        Vg[e] = fv[sj * ld + i] * sm.sgn[sj];
    }
    if (info && tid == 0) info[mat] = (bad || !done) ? -1 : sweeps;
}

namespace {

template <int NT, bool VLDS>
int launch_sym_eig(const double* A, int64_t batch, int d, double* W, double* V, int* info, hipStream_t st) {
    const size_t lds = eig_lds_bytes(d, VLDS);
    CIS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sym_eig<NT, VLDS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int64_t b0 = 0; b0 < batch; b0 += (1 << 30)) {
        const int64_t nb = batch - b0 < (1 << 30) ? batch - b0 : (1 << 30);
        hipLaunchKernelGGL((k_sym_eig<NT, VLDS>), dim3((unsigned)nb), dim3(NT), lds, st, A + b0 * d * d, d, W + b0 * d, V + b0 * d * d,
                           info ? info + b0 : nullptr);
    }
    CIS_CHECK_HIP(hipGetLastError());
    return CIS_OK;
}

}  // namespace

extern "C" int cis_sym_eig_dev(const double* d_A, int64_t batch, int d, double* d_W, double* d_V, int32_t* d_info, void* stream) {
    CIS_REQUIRE(d >= 1 && d <= EIG_MAX_D, "d must be in 1 .. %d (the matrix lives in LDS), got %d", EIG_MAX_D, d);
    CIS_REQUIRE(batch >= 0, "batch must be >= 0, got %lld", (long long)batch);
    if (batch == 0) return CIS_OK;
    CIS_REQUIRE(d_A && d_W && d_V, "NULL d_A, d_W or d_V");
    CIS_TRY(cis_lazy_init());
    return cis_sym_eig_launch(d_A, batch, d, d_W, d_V, d_info, (hipStream_t)stream);
}

int cis_sym_eig_launch(const double* d_A, int64_t batch, int d, double* d_W, double* d_V, int32_t* d_info, hipStream_t st) {
    // a round has d/2 * d work items per phase: 128 threads cover d <= 32 (7 workgroups of 21 KiB per CU), 512 threads d <= 64
    // (2 x 69 KiB), 1024 threads the one workgroup a CU holds beyond
    if (d <= 32) return launch_sym_eig<128, true>(d_A, batch, d, d_W, d_V, d_info, st);
    if (d <= 64) return launch_sym_eig<512, true>(d_A, batch, d, d_W, d_V, d_info, st);
    return launch_sym_eig<1024, false>(d_A, batch, d, d_W, d_V, d_info, st);
}
