"""The GPU training kernels (DESIGN.md section 1 row f) against exact references at their edges.

k_km_assign / k_km_update (csrc/kmeans.hip) and k_gram_groups / k_project_groups (csrc/lopq_train.hip), through the C ABI.

float32 atomics make the k-means sums order dependent, so the exact tests use INTEGER LATTICES: small integer data and
centroids.  Every x - c, every fmaf(df, df, acc), every LDS and global float sum is then an integer below 2^24 and exact in
float32 whatever the order, the inertia is an exact integer in double, and one Lloyd step has an int64 reference.  The same
holds in float64 (2^53) for the Gram and projection kernels with integer X, mu and R.  Each reference builder below also
runs a plain numpy float32 / float64 emulation of the kernel's arithmetic against the int64 result and asserts the
magnitudes, so the inputs are guarded: if someone widens a range until a rounding could occur, the builder fails, not the
kernel.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F24 = 1 << 24  # integers below this are exact in float32
F53 = 1 << 53  # ... in float64
CIS_EINVAL = -1


def _L():
    from columbiaimagesearch_amd import _lib
    return _lib


# --------------------------------------------------------------------------------------------------------------------
# A. cis_kmeans, one exact step on integer lattices
# --------------------------------------------------------------------------------------------------------------------

def _km(X, C0, iters, want_assign=True):
    """cis_kmeans on copies; (centroids, assign or None, inertia).  assign is pre-filled with -1: a row the copy-out or the
    kernel skipped stays visible."""
    lib = _L()
    X = np.ascontiguousarray(X, dtype=np.float32)
    C = np.array(C0, dtype=np.float32, order="C", copy=True)
    n, d = X.shape
    assign = np.full(n, -1, dtype=np.int32) if want_assign else None
    inertia = ctypes.c_double(-1.0)
    lib.check(lib.lib().cis_kmeans(lib.ptr(X), n, d, C.shape[0], int(iters), lib.ptr(C), lib.ptr(assign), ctypes.byref(inertia)))
    return C, assign, inertia.value


def _lattice_reference(X, C):
    """int64 reference of one Lloyd step on integer data: (assign, inertia, C1, counts), guarded by a float32 emulation of
    k_km_assign / k_km_update (sequential acc += df * df per dimension, first minimum, sequential float32 sums, one
    float32 division)."""
    Xi, Ci = X.astype(np.int64), C.astype(np.int64)
    assert X.dtype == np.float32 and C.dtype == np.float32 and (Xi == X).all() and (Ci == C).all()
    n, d = X.shape
    k = C.shape[0]
    assign = np.empty(n, dtype=np.int64)
    best = np.empty(n, dtype=np.int64)
    chunk = max(1, (1 << 22) // (k * d))
    for a in range(0, n, chunk):
        diff = Xi[a:a + chunk, None, :] - Ci[None]
        D = (diff * diff).sum(-1)
        # d > 1: every partial sum of squares is an exact float32 integer.  d == 1: the distance is ONE rounding of df * df
        # (fmaf(df, df, 0)), which is monotone in |df| and exact below 2^24 -- so a far centroid can neither beat nor tie
        # the minimum as long as the minimum itself is below 2^24 (asserted below)
        assert np.abs(diff).max() < F24 and (d == 1 or D.max() < F24)
        assign[a:a + chunk] = D.argmin(1)  # numpy's argmin returns the first minimum
        best[a:a + chunk] = D.min(1)
        df = X[a:a + chunk, None, :] - C[None]
        acc = np.zeros(df.shape[:2], dtype=np.float32)
        for i in range(d):
            acc = acc + df[:, :, i] * df[:, :, i]
        assert acc.dtype == np.float32
        assert (acc.argmin(1) == assign[a:a + chunk]).all() and (acc.min(1).astype(np.int64) == best[a:a + chunk]).all()
    assert best.max() < F24
    inertia = int(best.sum())
    assert inertia < F53 and float(best.astype(np.float64).sum()) == inertia
    counts = np.bincount(assign, minlength=k)
    sums = np.zeros((k, d), dtype=np.int64)
    np.add.at(sums, assign, Xi)
    mass = np.zeros((k, d), dtype=np.int64)
    np.add.at(mass, assign, np.abs(Xi))
    assert mass.max() < F24 and counts.max() < F24  # any partial sum, in any order, is an exact float32 integer
    sums32 = np.zeros((k, d), dtype=np.float32)
    np.add.at(sums32, assign, X)
    assert (sums32.astype(np.int64) == sums).all()
    C1 = C.copy()
    nz = counts > 0
    C1[nz] = sums[nz].astype(np.float32) / counts[nz, None].astype(np.float32)
    assert C1.dtype == np.float32
    return assign, inertia, C1, counts


def _eval64(X, C, assign):
    """float64 squared distances at centroids C: (minimum over the centroids, distance to the assigned one), per point."""
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    n, d = X.shape
    dmin = np.empty(n)
    dass = np.empty(n)
    chunk = max(1, (1 << 22) // (C.shape[0] * d))
    for a in range(0, n, chunk):
        D = ((X64[a:a + chunk, None, :] - C64[None]) ** 2).sum(-1)
        dmin[a:a + chunk] = D.min(1)
        dass[a:a + chunk] = D[np.arange(D.shape[0]), assign[a:a + chunk]]
    return dmin, dass


def _case_random(n, d, k, lo, hi, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(lo, hi + 1, (n, d)).astype(np.float32), rs.randint(lo, hi + 1, (k, d)).astype(np.float32)


def _case_ties():
    """Rows 2 and 6 of the centroids are equal, and the data is every point of the [-8, 8]^2 lattice three times: many
    points lie exactly half-way between two centroids ((2, y) between (0, 0) and (4, 0), the diagonal between (0, 4) and
    (4, 0), ...).  The lower index must win; cluster 6 can never win and stays empty."""
    C = np.array([[0, 0], [4, 0], [-6, 6], [0, 4], [8, 8], [-8, -8], [-6, 6], [6, -6]], dtype=np.float32)
    g = np.arange(-8, 9)
    X = np.tile(np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2), (3, 1)).astype(np.float32)
    return np.ascontiguousarray(X[np.random.RandomState(2).permutation(len(X))]), C


def _case_n_lt_k():
    """5 points, 8 centroids: each point is nearest to its own centroid (0, 2, 3, 5, 7), which moves onto it in the first
    update and stays; centroids 1, 4 and 6 are empty from the start to the end."""
    C = np.array([[-8, -8], [8, -8], [-8, 8], [0, 0], [8, 0], [8, 8], [0, -8], [-2, 6]], dtype=np.float32)
    X = np.array([[-7, -7], [-7, 7], [1, 1], [7, 7], [-2, 5]], dtype=np.float32)
    return X, C


def _case_lds_d2():
    """3840 centroids in 2-D: more than the 289 points of [-8, 8]^2, so distinct points of [-40, 40]^2 (squared distances
    <= 2 * 80^2, still exact)."""
    rs = np.random.RandomState(7)
    pick = rs.permutation(81 * 81)[:3840]
    C = np.stack([pick // 81 - 40, pick % 81 - 40], -1).astype(np.float32)
    return rs.randint(-40, 41, (4096, 2)).astype(np.float32), C


def _case_lds_d1():
    """7680 centroids in 1-D: distinct integers of [-4000, 4000] in random order.  Far squared distances exceed 2^24 and
    are rounded once, monotonically (see _lattice_reference); the minimum is a few units."""
    rs = np.random.RandomState(8)
    C = (rs.permutation(8001)[:7680] - 4000).astype(np.float32)[:, None]
    return rs.randint(-4000, 4001, (8192, 1)).astype(np.float32), np.ascontiguousarray(C)


_KM_CASES = {
    "n1000_d3_k5": lambda: _case_random(1000, 3, 5, -8, 8, 1),           # n is no multiple of 256
    "n256_d1_k1": lambda: _case_random(256, 1, 1, -8, 8, 3),
    "n5_d2_k8": _case_n_lt_k,                                            # n < k, empty clusters
    "ties": _case_ties,
    "grid_stride_n300000_d2_k16": lambda: _case_random(300000, 2, 16, -8, 8, 4),  # > 1024 * 256 rows: a second trip
    "lds_n4096_d32_k240": lambda: _case_random(4096, 32, 240, -8, 8, 5),  # k * d = 7680: 62 KB of dynamic LDS
    "lds_n4096_d2_k3840": _case_lds_d2,                                   # ... 77 KB
    "lds_n8192_d1_k7680": _case_lds_d1,                                   # ... 92 KB
}


@functools.lru_cache(maxsize=None)
def _km_case(name):
    X, C = _KM_CASES[name]()
    for a in (X, C):
        a.setflags(write=False)
    return (X, C) + _lattice_reference(X, C)


@functools.lru_cache(maxsize=None)
def _km_run(name, iters, want_assign):
    X, C = _km_case(name)[:2]
    return _km(X, C, iters, want_assign)


def test_kmeans_case_shapes():
    """The inputs are what the cases claim: k * d on the guard's edge, a tie on the duplicate rows, the grid-stride size."""
    for name in ("lds_n4096_d32_k240", "lds_n4096_d2_k3840", "lds_n8192_d1_k7680"):
        X, C = _km_case(name)[:2]
        assert C.size == 7680 and len(np.unique(C, axis=0)) == len(C)
    assert _km_case("grid_stride_n300000_d2_k16")[0].shape[0] > 1024 * 256
    X, C, assign, _, _, counts = _km_case("ties")
    assert (C[2] == C[6]).all() and counts[2] > 0 and counts[6] == 0
    D = ((X.astype(np.int64)[:, None] - C.astype(np.int64)[None]) ** 2).sum(-1)
    tied = (D == D.min(1, keepdims=True)).sum(1) > 1
    assert tied.sum() >= 100 and ((D[tied, 2] != D[tied].min(1)).sum() >= 30)  # ties other than the duplicate row's, too
    counts = _km_case("n5_d2_k8")[5]
    assert (counts == [1, 0, 1, 1, 0, 1, 0, 1]).all()


@pytest.mark.parametrize("want_assign", [True, False], ids=["assign", "null"])
@pytest.mark.parametrize("name", list(_KM_CASES))
def test_kmeans_assignment_only_is_exact(name, want_assign):
    """iters = 0: the centroids come back untouched, the assignment is the int64 argmin with the first minimum, and the
    inertia is the exact integer.  Exact counts and inertia at n = 300 000 say every row was visited once."""
    X, C, assign_ref, inertia_ref = _km_case(name)[:4]
    got_C, assign, inertia = _km_run(name, 0, want_assign)
    assert got_C.tobytes() == C.tobytes()
    assert inertia == float(inertia_ref)
    if want_assign:
        np.testing.assert_array_equal(assign, assign_ref)
    else:
        assert assign is None


@pytest.mark.parametrize("want_assign", [True, False], ids=["assign", "null"])
@pytest.mark.parametrize("name", list(_KM_CASES))
def test_kmeans_one_step_is_exact(name, want_assign):
    """iters = 1: the returned centroids EQUAL float32(sum) / float32(count) of the int64 reference (the build has no
    fast-math and the float32 division is correctly rounded, so equality, not 1 ulp), an empty cluster keeps its bytes;
    assign and inertia describe the returned centroids: every point's assigned centroid is a float64 nearest one to
    1e-5 * (minimum + 1), and the inertia matches the float64 sum over the kernel's own assignment to 1e-5."""
    X, C, _, _, C1_ref, counts = _km_case(name)
    got_C, assign, inertia = _km_run(name, 1, want_assign)
    np.testing.assert_array_equal(got_C, C1_ref)
    assert got_C[counts == 0].tobytes() == C[counts == 0].tobytes()
    if want_assign:
        assert assign.min() >= 0 and assign.max() < len(C)
        dmin, dass = _eval64(X, got_C, assign)
        bad = np.nonzero(dass > dmin + 1e-5 * (dmin + 1.0))[0]
        assert bad.size == 0, (bad[:10], dass[bad[:10]], dmin[bad[:10]])
        np.testing.assert_allclose(inertia, dass.sum(), rtol=1e-5)
    else:
        assert assign is None
        # same centroids (bytes, above) => same float32 distances; only the order of the double additions differs
        # between two launches: n terms, all positive, each addition rounds by at most 2^-53 relative
        np.testing.assert_allclose(inertia, _km_run(name, 1, True)[2], rtol=len(X) * 2.0 ** -53)


@pytest.mark.parametrize("want_assign", [True, False], ids=["assign", "null"])
def test_kmeans_empty_clusters_keep_their_centroid(want_assign):
    """n < k: the three clusters without a point come back byte-equal after 1 and after 3 iterations, the other five sit
    on their point."""
    X, C, assign_ref, _, C1_ref, counts = _km_case("n5_d2_k8")
    want = C.copy()
    want[assign_ref] = X
    np.testing.assert_array_equal(want, C1_ref)
    for iters in (1, 3):
        got_C, assign, inertia = _km(X, C, iters, want_assign)
        assert got_C[counts == 0].tobytes() == C[counts == 0].tobytes()
        np.testing.assert_array_equal(got_C, want)
        assert inertia == 0.0
        if want_assign:
            np.testing.assert_array_equal(assign, assign_ref)


# --------------------------------------------------------------------------------------------------------------------
# B. cis_kmeans, the chain over iterations on real-valued data
# --------------------------------------------------------------------------------------------------------------------

_EMPTY = 5  # row of the far-away centroid


@functools.lru_cache(maxsize=None)
def _blobs():
    """(20 000, 8) points in 11 unit-variance blobs whose centres are distinct points of 40 * {-2..2}^8 (>= 40 sigma apart);
    the start is one perturbed point per blob plus, at row 5, a centroid far away from everything.  Also a float64 Lloyd run
    from that start: (X, C0, assign [n], [C after 0, 1, .. 5 updates])."""
    rs = np.random.RandomState(11)
    n, d, nb = 20000, 8, 11
    cent = set()
    while len(cent) < nb:
        cent.add(tuple(rs.randint(-2, 3, d)))
    centres = 40.0 * np.array(sorted(cent))
    gaps = np.sqrt(((centres[:, None] - centres[None]) ** 2).sum(-1))[np.triu_indices(nb, 1)]
    assert gaps.min() >= 20.0
    label = rs.randint(0, nb, n)
    X = (centres[label] + rs.randn(n, d)).astype(np.float32)
    first = [int(np.nonzero(label == b)[0][0]) for b in range(nb)]
    C0 = (X[first] + 0.5 * rs.randn(nb, d)).astype(np.float32)
    C0 = np.ascontiguousarray(np.insert(C0, _EMPTY, np.full(d, 1000.0, dtype=np.float32), axis=0))
    X64 = X.astype(np.float64)
    Cs = [C0.astype(np.float64)]
    assigns = []
    for _ in range(6):
        D = ((X64[:, None, :] - Cs[-1][None]) ** 2).sum(-1)
        a = D.argmin(1)
        part = np.partition(D, 1, axis=1)
        assert (part[:, 1] - part[:, 0]).min() > 100.0  # no assignment is anywhere near a float32 rounding
        assigns.append(a)
        C = Cs[-1].copy()
        for c in range(nb + 1):
            if (a == c).any():
                C[c] = X64[a == c].mean(0)
        Cs.append(C)
    # the bound below relies on this: the reference's assignment never changes, and the far centroid never gets a point
    assert all((a == assigns[0]).all() for a in assigns) and not (assigns[0] == _EMPTY).any()
    assert np.bincount(assigns[0], minlength=nb + 1).tolist().count(0) == 1
    for a in (X, C0):
        a.setflags(write=False)
    return X, C0, assigns[0], Cs


def _accumulation_bound(X, assign, C):
    """Worst case of a float32 mean, per coordinate: count * 2^-24 * mean|x| for the sum (count additions, each rounding by
    2^-24 relative of a partial sum of at most sum|x|, then divided by count) + 2^-23 * |C| for the division and the
    float32 storage."""
    k = C.shape[0]
    counts = np.bincount(assign, minlength=k).astype(np.float64)
    mass = np.zeros(C.shape)
    np.add.at(mass, assign, np.abs(X.astype(np.float64)))
    mean_abs = mass / np.maximum(counts, 1.0)[:, None]
    return counts[:, None] * 2.0 ** -24 * mean_abs + 2.0 ** -23 * np.abs(C)


@pytest.mark.parametrize("T", [1, 4])
def test_kmeans_chain_over_iterations(T):
    """iters = T + 1 is one more Lloyd step after iters = T: its centroids are the float64 means of the points under the
    assignment that iters = T reported, to the worst-case float32 accumulation bound (derived from the data, see
    _accumulation_bound); the empty centroid keeps its bytes; and the end of the chain matches a float64 numpy Lloyd run
    from the same start to (T + 1) times that bound (the reference's assignment is constant on this data -- asserted in
    _blobs -- so nothing but rounding separates the two)."""
    X, C0, assign_ref, Cs = _blobs()
    C_T, a_T, inertia_T = _km(X, C0, T)
    C_T1, a_T1, _ = _km(X, C0, T + 1)
    np.testing.assert_array_equal(a_T, assign_ref)  # margins > 100 in squared distance: no rounding can move a point
    np.testing.assert_array_equal(a_T1, assign_ref)
    X64 = X.astype(np.float64)
    mean = C0.astype(np.float64)
    for c in np.unique(a_T):
        mean[c] = X64[a_T == c].mean(0)
    tol = _accumulation_bound(X, a_T, mean)
    for C in (C_T, C_T1):
        assert C[_EMPTY].tobytes() == C0[_EMPTY].tobytes()
    err = np.abs(C_T1.astype(np.float64) - mean)
    assert (err <= tol).all(), (err.max(), tol.min())
    err = np.abs(C_T1.astype(np.float64) - Cs[T + 1])
    assert (err <= (T + 1) * _accumulation_bound(X, assign_ref, Cs[T + 1])).all(), err.max()
    dass = ((X64 - C_T.astype(np.float64)[a_T]) ** 2).sum(1)
    np.testing.assert_allclose(inertia_T, dass.sum(), rtol=1e-5)


# --------------------------------------------------------------------------------------------------------------------
# C. cis_train_gram and cis_train_project, exact on integer data in float64
# --------------------------------------------------------------------------------------------------------------------

def _rows(n, d, fill=None, rs=None, lo=-4, hi=4):
    """[n][d] float64 with a non-NULL data pointer even at n = 0 (a view on one spare row)."""
    buf = np.full((n + 1, d), np.nan if fill is None else fill, dtype=np.float64)
    if rs is not None:
        buf[:n] = rs.randint(lo, hi + 1, (n, d))
    return buf[:n]


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _gram(X, off, want_S=True):
    lib = _L()
    n, d = X.shape
    groups = len(off) - 1
    G = np.full((groups, d, d), np.nan)
    S = np.full((groups, d), np.nan) if want_S else None
    lib.check(lib.lib().cis_train_gram(lib.ptr(X), n, d, lib.ptr(off), groups, lib.ptr(G), lib.ptr(S)))
    return G, S


def _project(X, off, R, mu, Y=None):
    lib = _L()
    n, d = X.shape
    Y = _rows(n, d) if Y is None else Y
    lib.check(lib.lib().cis_train_project(lib.ptr(X), n, d, lib.ptr(off), len(off) - 1, lib.ptr(R), lib.ptr(mu), lib.ptr(Y)))
    return Y


def _gram_reference(X, off):
    """int64 X_g^T X_g and column sums, guarded by a float64 emulation of k_gram_groups' order (rows ascending, one
    multiply-add per row)."""
    Xi = X.astype(np.int64)
    assert (Xi == X).all()
    groups, d = len(off) - 1, X.shape[1]
    G = np.zeros((groups, d, d), dtype=np.int64)
    S = np.zeros((groups, d), dtype=np.int64)
    for g in range(groups):
        r = Xi[off[g]:off[g + 1]]
        G[g], S[g] = r.T @ r, r.sum(0)
        assert (np.abs(r).T @ np.abs(r)).max(initial=0) < F53
        acc, csum = np.zeros((d, d)), np.zeros(d)
        for row in X[off[g]:off[g + 1]]:
            acc += np.outer(row, row)
            csum += row
        assert (acc == G[g]).all() and (csum == S[g]).all()
    return G.astype(np.float64), S.astype(np.float64)


def _project_reference(X, off, R, mu):
    """int64 (X_g - mu_g) R_g^T, guarded by a float64 emulation of k_project_groups' order (k ascending)."""
    Xi, Ri, mi = X.astype(np.int64), R.astype(np.int64), mu.astype(np.int64)
    assert (Xi == X).all() and (Ri == R).all() and (mi == mu).all()
    Y = np.zeros(X.shape, dtype=np.int64)
    for g in range(len(off) - 1):
        a, b = off[g], off[g + 1]
        Y[a:b] = (Xi[a:b] - mi[g]) @ Ri[g].T
        assert (np.abs(Xi[a:b] - mi[g]) @ np.abs(Ri[g]).T).max(initial=0) < F53
        acc = np.zeros((b - a, X.shape[1]))
        for k in range(X.shape[1]):
            acc += np.outer(X[a:b, k] - mu[g, k], R[g, :, k])
        assert (acc == Y[a:b]).all()
    return Y.astype(np.float64)


_LAYOUTS = {
    "stage_edges": [0, 1, 15, 16, 17, 0, 0, 33, 0],  # 1, 15, 16, 17 rows at the 16-row LDS stage; consecutive and trailing empty groups
    "leading_empty": [0, 40, 3],
    "one_group": [200],
    "no_rows": [0, 0, 0],
}


@pytest.mark.parametrize("layout", list(_LAYOUTS))
@pytest.mark.parametrize("d", [1, 63, 64, 65, 128, 129])
def test_gram_and_project_are_exact_on_integers(d, layout):
    """d on and around the 64-wide tile edges, group sizes on and around the 16-row stage, empty groups in every position,
    one group, no rows at all: G, S and Y equal the int64 references entry for entry (outputs are pre-filled with NaN, so
    an entry nobody wrote fails), G is exactly symmetric, a row never lands in the neighbouring group."""
    sizes = _LAYOUTS[layout]
    off = _offsets(sizes)
    n, groups = int(off[-1]), len(sizes)
    rs = np.random.RandomState(100 * d + len(sizes))
    X = _rows(n, d, rs=rs)
    R = rs.randint(-3, 4, (groups, d, d)).astype(np.float64)
    mu = rs.randint(-3, 4, (groups, d)).astype(np.float64)
    G_ref, S_ref = _gram_reference(X, off)
    G, S = _gram(X, off)
    np.testing.assert_array_equal(G, G_ref)
    np.testing.assert_array_equal(S, S_ref)
    np.testing.assert_array_equal(G, G.transpose(0, 2, 1))
    if n == 0:
        assert not G.any() and not S.any()
        Y = _project(X, off, R, mu, Y=_rows(0, d, fill=7.0))
        assert (Y.base == 7.0).all()  # CIS_OK and nothing written
        return
    np.testing.assert_array_equal(_project(X, off, R, mu), _project_reference(X, off, R, mu))


def test_gram_accepts_no_sums():
    """S = NULL: G alone."""
    off = _offsets(_LAYOUTS["stage_edges"])
    X = _rows(int(off[-1]), 65, rs=np.random.RandomState(1))
    G, S = _gram(X, off, want_S=False)
    assert S is None
    np.testing.assert_array_equal(G, _gram_reference(X, off)[0])


def test_gram_and_project_beyond_one_grid_z():
    """32 770 groups of 0, 1, 2, 3, 0, 1, ... rows at d = 2: one launch takes 32 768 groups, the last two (of 0 and 1 rows)
    run in a second launch on shifted offset / G / S / R / mu pointers.  Every group is checked, in both entry points."""
    groups, d = 32770, 2
    sizes = np.arange(groups) % 4
    off = _offsets(sizes)
    n = int(off[-1])
    assert sizes[32768:].tolist() == [0, 1] and n == off[32769] + 1
    rs = np.random.RandomState(6)
    X = _rows(n, d, rs=rs)
    R = rs.randint(-3, 4, (groups, d, d)).astype(np.float64)
    mu = rs.randint(-3, 4, (groups, d)).astype(np.float64)
    gid = np.repeat(np.arange(groups), sizes)
    Xi = X.astype(np.int64)
    G_ref = np.zeros((groups, d, d), dtype=np.int64)
    np.add.at(G_ref, gid, Xi[:, :, None] * Xi[:, None, :])
    S_ref = np.zeros((groups, d), dtype=np.int64)
    np.add.at(S_ref, gid, Xi)
    Y_ref = np.einsum("nk,nok->no", Xi - mu.astype(np.int64)[gid], R.astype(np.int64)[gid])
    # float64 emulation: with at most 3 rows and 2 columns of integers below 8 nothing comes near 2^53
    assert (np.einsum("nk,nok->no", X - mu[gid], R[gid]) == Y_ref).all()
    G64 = np.zeros((groups, d, d))
    np.add.at(G64, gid, X[:, :, None] * X[:, None, :])
    assert (G64 == G_ref).all()
    G, S = _gram(X, off)
    np.testing.assert_array_equal(G, G_ref.astype(np.float64))
    np.testing.assert_array_equal(S, S_ref.astype(np.float64))
    np.testing.assert_array_equal(_project(X, off, R, mu), Y_ref.astype(np.float64))


def test_project_beyond_one_grid_y():
    """One group of 4 194 241 rows at d = 1: 65 536 row tiles of 64, one more than the grid's y extent holds, so the last
    row is reached only by the second launch (tile_base = 65 535), in which the 70-row group behind it must write
    nothing.  All rows are checked."""
    sizes = [65535 * 64 + 1, 70]
    off = _offsets(sizes)
    n = int(off[-1])
    rs = np.random.RandomState(9)
    X = _rows(n, 1, rs=rs)
    R = np.array([[[3.0]], [[-2.0]]])
    mu = np.array([[1.0], [-3.0]])
    gid = np.repeat([0, 1], sizes)
    Y_ref = (X.astype(np.int64) - mu.astype(np.int64)[gid]) * R.astype(np.int64)[gid, 0]
    assert ((X - mu[gid]) * R[gid, 0] == Y_ref).all()  # float64 emulation: integers below 32
    Y = _project(X, off, R, mu)
    np.testing.assert_array_equal(Y, Y_ref.astype(np.float64))


def test_gram_and_project_random_floats():
    """The arithmetic, not only the indexing, at float magnitudes: (900, 130, 5) random normals against numpy, 1e-12."""
    rs = np.random.RandomState(3)
    n, d, groups = 900, 130, 5
    X = np.ascontiguousarray(rs.randn(n, d) * (1.0 + np.arange(d)) ** -0.3)
    off = _offsets([300, 0, 17, 500, 83])
    R, mu = rs.randn(groups, d, d), rs.randn(groups, d)
    G, S = _gram(X, off)
    Y = _project(X, off, R, mu)
    for g in range(groups):
        r = X[off[g]:off[g + 1]]
        np.testing.assert_allclose(G[g], r.T.dot(r), rtol=1e-12, atol=1e-10)
        np.testing.assert_allclose(S[g], r.sum(axis=0), rtol=1e-12, atol=1e-10)
        np.testing.assert_allclose(Y[off[g]:off[g + 1]], (r - mu[g]).dot(R[g].T), rtol=1e-12, atol=1e-10)


# --------------------------------------------------------------------------------------------------------------------
# D. argument checks
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d,k,iters,reason", [
    (64, 1, 7681, 1, "k * d"),
    (64, 7681, 1, 1, "k * d"),
    (0, 2, 4, 1, "n must be"),
    (64, 2, 4, -1, "iters must be"),
])
def test_kmeans_rejects_bad_arguments(n, d, k, iters, reason):
    """Refused with CIS_EINVAL -- the code of the argument checks, which come before the first HIP call -- and a message
    that names the reason; centroids, assign and inertia are untouched."""
    lib = _L()
    X = np.ones((max(n, 1), d), dtype=np.float32)
    C = np.full((k, d), 3.0, dtype=np.float32)
    assign = np.full(max(n, 1), -7, dtype=np.int32)
    inertia = ctypes.c_double(-7.0)
    rc = lib.lib().cis_kmeans(lib.ptr(X), n, d, k, iters, lib.ptr(C), lib.ptr(assign), ctypes.byref(inertia))
    assert rc == CIS_EINVAL and reason in lib.last_error(), (rc, lib.last_error())
    assert (C == 3.0).all() and (assign == -7).all() and inertia.value == -7.0
    with pytest.raises(ValueError, match=reason.replace("*", r"\*")):
        lib.check(rc)


@pytest.mark.parametrize("entry", ["gram", "project"])
@pytest.mark.parametrize("off,groups,reason", [
    ([1, 4, 10], 2, "group offsets"),   # group_off[0] != 0
    ([0, 4, 9], 2, "group offsets"),    # group_off[groups] != n
    ([0, 4, 11], 2, "group offsets"),
    ([0, 10], 0, "groups must be"),
])
def test_gram_and_project_reject_bad_arguments(entry, off, groups, reason):
    """As above for the offsets that do not cover [0, n) and for groups = 0: CIS_EINVAL, the reason, outputs untouched."""
    lib = _L()
    n, d = 10, 3
    X = np.ones((n, d))
    off = np.array(off, dtype=np.int64)
    G, S, Y = np.full((2, d, d), -7.0), np.full((2, d), -7.0), np.full((n, d), -7.0)
    R, mu = np.ones((2, d, d)), np.ones((2, d))
    if entry == "gram":
        rc = lib.lib().cis_train_gram(lib.ptr(X), n, d, lib.ptr(off), groups, lib.ptr(G), lib.ptr(S))
    else:
        rc = lib.lib().cis_train_project(lib.ptr(X), n, d, lib.ptr(off), groups, lib.ptr(R), lib.ptr(mu), lib.ptr(Y))
    assert rc == CIS_EINVAL and reason in lib.last_error(), (rc, lib.last_error())
    assert (G == -7.0).all() and (S == -7.0).all() and (Y == -7.0).all()


# --------------------------------------------------------------------------------------------------------------------
# E. the Python layer (lopq/train.py)
# --------------------------------------------------------------------------------------------------------------------

def _inertia64(X, C):
    return float(((X.astype(np.float64)[:, None, :] - C.astype(np.float64)[None]) ** 2).sum(-1).min(1).sum())


class _KmeansSpy(object):
    """The loaded library with cis_kmeans recorded: (returned centroids, reported inertia) of every call."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def cis_kmeans(self, X, n, d, k, iters, C, assign, inertia):
        rc = self._real.cis_kmeans(X, n, d, k, iters, C, assign, inertia)
        got = np.ctypeslib.as_array((ctypes.c_float * (k * d)).from_address(C.value)).reshape(k, d).copy()
        self.calls.append((got, inertia._obj.value))
        return rc


def test_kmeans_hip_returns_the_best_of_n_init(monkeypatch):
    """n_init = 3: three k-means++ seedings, three cis_kmeans calls; what comes back is the run whose centroids have the
    smallest float64 inertia.  20 tight blobs and k = 8 with one Lloyd step: where the seeds fall decides the inertia, so
    the three runs differ by far more than float32 rounding (asserted on a float64 emulation of the same three runs)."""
    from columbiaimagesearch_amd.lopq import train as T
    lib = _L()
    rs = np.random.RandomState(21)
    centres = rs.uniform(-50, 50, (20, 4))
    X = (centres[rs.randint(0, 20, 3000)] + rs.randn(3000, 4)).astype(np.float32)
    k, seed = 8, 13
    emu = []
    ers = np.random.RandomState(seed)
    for _ in range(3):
        C = np.ascontiguousarray(T.kmeans_pp_init(X, k, ers), dtype=np.float32).astype(np.float64)
        a = ((X.astype(np.float64)[:, None, :] - C[None]) ** 2).sum(-1).argmin(1)
        for c in np.unique(a):
            C[c] = X[a == c].astype(np.float64).mean(0)
        emu.append(_inertia64(X, C))
    gaps = np.abs(np.subtract.outer(emu, emu))[np.triu_indices(3, 1)]
    assert gaps.min() > 1e-3 * max(emu), emu  # the inits differ visibly: a thousand times the float32 rounding of 1e-6
    assert int(np.argmin(emu)) != 0, emu         # ... and "keep the first" would not pass

    spy = _KmeansSpy(lib.lib())
    monkeypatch.setattr(lib, "lib", lambda: spy)
    C, inertia = T.kmeans_hip(X, k, iters=1, n_init=3, random_state=seed)
    assert len(spy.calls) == 3
    seen = [_inertia64(X, c) for c, _ in spy.calls]
    np.testing.assert_allclose(seen, emu, rtol=1e-4)  # the three GPU runs are the three emulated ones
    for s, (_, reported) in zip(seen, spy.calls):
        np.testing.assert_allclose(reported, s, rtol=1e-5)
    best = int(np.argmin(seen))
    assert best == int(np.argmin(emu))
    assert C.dtype == np.float64 and C.tobytes() == spy.calls[best][0].astype(np.float64).tobytes()
    assert inertia == spy.calls[best][1]
    np.testing.assert_allclose(_inertia64(X, C), min(seen), rtol=0, atol=0)


def test_gram_hip_and_project_to_local_with_unsorted_assign():
    """The order / out[order] = Y round trip: an unsorted assignment (with an empty group) on integer data equals the
    per-group numpy loop exactly."""
    from columbiaimagesearch_amd.lopq import train as T
    rs = np.random.RandomState(17)
    n, d, groups = 700, 20, 6
    X = rs.randint(-4, 5, (n, d)).astype(np.float64)
    assign = rs.randint(0, groups, n)
    assign[assign == 4] = 1
    assert (np.diff(assign) < 0).any()
    R = rs.randint(-3, 4, (groups, d, d)).astype(np.float64)
    mu = rs.randint(-3, 4, (groups, d)).astype(np.float64)
    G, S = T.gram_hip(X, assign, groups)
    Xi = X.astype(np.int64)
    want = np.zeros((n, d), dtype=np.int64)
    for g in range(groups):
        r = Xi[assign == g]
        np.testing.assert_array_equal(G[g], (r.T @ r).astype(np.float64))
        np.testing.assert_array_equal(S[g], r.sum(0).astype(np.float64))
        want[assign == g] = (r - mu[g].astype(np.int64)) @ R[g].astype(np.int64).T
    assert not G[4].any() and not S[4].any()
    host = T.project_to_local(X, assign, R, mu)
    T.ACCUM_BACKEND = "hip"
    try:
        got = T.project_to_local(X, assign, R, mu)
    finally:
        T.ACCUM_BACKEND = "host"
    np.testing.assert_array_equal(got, want.astype(np.float64))
    np.testing.assert_array_equal(host, want.astype(np.float64))


def test_kmeans_backend_hip_leaves_large_codebooks_to_sklearn(monkeypatch):
    """KMEANS_BACKEND = "hip" with k * d > 7680: _kmeans takes the scikit-learn path and never calls kmeans_hip; on the
    edge (k * d = 7680) it does call it."""
    from columbiaimagesearch_amd.lopq import train as T

    def boom(*a, **kw):
        raise AssertionError("kmeans_hip called")

    X = np.random.RandomState(4).randn(400, 64)
    monkeypatch.setattr(T, "kmeans_hip", boom)
    backends = (T.KMEANS_BACKEND, T.ACCUM_BACKEND)
    T.KMEANS_BACKEND = "hip"
    try:
        C = T._kmeans(X, 121, 1, 1, 0)  # 121 * 64 = 7744
        assert C.shape == (121, 64) and np.isfinite(C).all()
        with pytest.raises(AssertionError, match="kmeans_hip called"):
            T._kmeans(X, 120, 1, 1, 0)  # 120 * 64 = 7680
    finally:
        T.KMEANS_BACKEND, T.ACCUM_BACKEND = backends
    assert (T.KMEANS_BACKEND, T.ACCUM_BACKEND) == ("sklearn", "host")
