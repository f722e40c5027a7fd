"""numpy statement of the scheme of csrc/sym_eig_block.hip (cis_sym_eig_large_dev): cyclic two-sided block Jacobi with blocks of b
columns, block pairs in the round-robin ordering of jacobi_model.round_pairs (an odd block count gets a bye), every pivot solved by
jacobi_model.jacobi_eigh, A <- Q^T (A Q) with the pivot tiles written as diag(W_P) and the lower triangle mirrored from the upper
one, zero padding to a multiple of b that is dropped at the end, done after a block sweep in which every pivot reported one sweep.
The matrices and the bound of tests/test_sym_eig_large.py.  No GPU here: the model shows what the scheme alone gives on the test
matrices, and the test's bound is derived from that (the kernel's figures never enter it).

The kernel mirrors whole tiles (pair P against pair R >= P in the order of the round), the model single entries (i < j): either
keeps one of two values that the same expression gave with the roles of its operands exchanged."""
import numpy as np

import jacobi_model as J

U = J.U
MAX_SWEEPS = 40


def _mm(spec, a, b):
    """A matrix product in einsum's own loops: the same sums on every machine, whatever BLAS and however many threads it uses (the
    orthogonality figure of the graded matrix at d = 320, b = 32 moved from 19.2 to 19.4 d u between one BLAS thread and several)."""
    return np.einsum(spec, a, b)


def block_eigh(A, b=64, max_sweeps=MAX_SWEEPS):
    """(W ascending, V with unit eigenvector columns after the sign rule, block sweeps), or (None, None, -1) for an input that is not
    finite, a failed pivot or the cap."""
    A = np.array(A, dtype=np.float64)
    d = A.shape[0]
    if not np.isfinite(A).all():
        return None, None, -1
    nb = max(2, -(-d // b))
    dp = nb * b
    Ap = np.zeros((dp, dp))
    Ap[:d, :d] = np.tril(A) + np.tril(A, -1).T  # the lower triangle, as numpy.linalg.eigh reads it
    VT = np.eye(dp)
    rounds = [J.round_pairs(nb, r) for r in range(nb + (nb & 1) - 1)]
    sweeps, done = 0, False
    while not done and sweeps < max_sweeps:
        rotated = False
        for pairs in rounds:
            solved = []
            for I, K in pairs:  # the pivots of a round are disjoint: all are taken from the matrix as the round found it
                idx = np.r_[I * b:(I + 1) * b, K * b:(K + 1) * b]
                w, q, info = J.jacobi_eigh(Ap[np.ix_(idx, idx)])
                if info < 0:
                    return None, None, -1
                rotated = rotated or info != 1
                solved.append((idx, w, q))
            for idx, w, q in solved:
                Ap[:, idx] = _mm("ij,jk->ik", Ap[:, idx], q)
            for idx, w, q in solved:
                Ap[idx, :] = _mm("ji,jk->ik", q, Ap[idx, :])
                VT[idx, :] = _mm("ji,jk->ik", q, VT[idx, :])
            for idx, w, q in solved:
                Ap[np.ix_(idx, idx)] = np.diag(w)
            Ap = np.triu(Ap) + np.triu(Ap, 1).T
        sweeps += 1
        done = not rotated
    if not done:
        return None, None, -1
    real = ~(VT[:, d:] != 0).any(axis=1)  # a row with a nonzero beyond column d is a unit vector of the padding
    assert real.sum() == d
    w = np.diag(Ap)[real]
    V = VT[real, :d].T
    o = np.argsort(w, kind="stable")
    return w[o], J.fix_signs(V[:, o]), sweeps


# ---- the matrices and the bound of tests/test_sym_eig_large.py ---------------------------------------------------------------------

DIMS = (129, 192, 200, 257, 320)
KINDS = J.KINDS
# b = 32, the default beyond d = 128, runs every size (5 to 10 blocks; 129 and 200 are ragged, 129, 200 and 257 have an odd block
# count); b = 64 the ragged size (4 blocks) and the one with an odd block count (5 blocks)
BLOCK_DIMS = {32: DIMS, 64: (200, 320)}

# Per block size b: the model's worst figures over KINDS x BLOCK_DIMS[b] in units of d u (d u |A|_2 for the first and the last) --
# residual, orthogonality, eigenvalues against eigvalsh -- and its largest block sweep count, recorded from this file's own run
# (tests/test_sym_eig_large.py::test_model_stays_within_a_third_of_the_bound prints every figure).  The graded spectrum is the slow
# and the least orthogonal case: at b = 32 it takes 9, 10 and 11 block sweeps at d = 200, 257 and 320 and reaches 14.2, 17.5 and
# 19.3 d u in orthogonality (twice the rounds per block sweep and more block sweeps than at b = 64, and every round adds its
# pivots' orthogonality errors).
# C[b] = ceil(3 * the worst figure): the margin tests/test_sym_eig.py gives another operation order (58.01 -> 59, 34.05 -> 35).
MODEL_WORST = {32: (5.55, 19.34, 11.83), 64: (5.88, 11.35, 8.56)}
MODEL_SWEEPS = {32: 11, 64: 7}
C = {32: 59, 64: 35}


def matrix(kind, d):
    return J.matrix(kind, d, seed=0)


def figures(A, W, V):
    """(residual, orthogonality, eigenvalues against eigvalsh) in units of d u (times |A|_2 for the first and the last)."""
    d = A.shape[0]
    ref = np.linalg.eigvalsh(A)
    norm = np.abs(ref).max()
    scale = d * U * norm if norm > 0 else 1.0
    res = np.abs(_mm("ij,jk->ik", A, V) - V * W).max()
    orth = np.abs(_mm("ji,jk->ik", V, V) - np.eye(d)).max()
    eig = np.abs(W - ref).max()
    return res / scale, orth / (d * U), eig / scale


def check_bounds(A, W, V, sweeps, c, max_sweeps=MAX_SWEEPS, label=""):
    """Residual, eigenvalues against eigvalsh and orthogonality within c d u (times |A|_2 where it applies), W ascending, the sign
    rule, 1 <= sweeps <= max_sweeps; eigenvectors against LAPACK's to 1e-9 where the spectrum is separated as
    jacobi_model.check_bounds requires.  Returns the three figures."""
    d = A.shape[0]
    assert np.isfinite(W).all() and np.isfinite(V).all(), label
    f = figures(A, W, V)
    assert f[0] <= c, (label, "residual", f)
    assert f[1] <= c, (label, "orthogonality", f)
    assert f[2] <= c, (label, "eigenvalues", f)
    assert (np.diff(W) >= 0).all(), label
    assert (V == J.fix_signs(V)).all(), (label, "sign rule")
    assert 1 <= sweeps <= max_sweeps, (label, sweeps)
    ref = np.linalg.eigvalsh(A)
    norm = np.abs(ref).max()
    if d > 1 and norm > 0 and np.diff(ref).min() > 1e-3 * norm:
        Vref = J.fix_signs(np.linalg.eigh(A)[1])
        assert np.abs(V - Vref).max() <= 1e-9, (label, "eigenvectors", np.abs(V - Vref).max())
    return f
