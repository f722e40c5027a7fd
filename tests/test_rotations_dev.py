"""The local-rotation stage of LOPQ training on device pointers (csrc/lopq_train.hip's *_dev entry points with cis_sym_eig_dev,
train.ROTATION_BACKEND = "device"): the pieces exactly on integer lattices, the stage against numpy on descriptor-like rows, whole
fits against the host backend's own spread, and the switch."""
import numpy as np
import pytest

U = 2.0 ** -53
F53 = 2 ** 53


def _L():
    from columbiaimagesearch_amd import _lib
    return _lib


def _T():
    from columbiaimagesearch_amd.lopq import train as T
    return T


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _nan(shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


# ---- the pieces, exact on integers --------------------------------------------------------------------------------------------

def _lattice(V, d):
    """Rows in shuffled order with their groups: an empty group, a group of one row and one with at least d rows where V allows;
    n is no multiple of 64."""
    sizes = [max(150, d + 50)] if V == 1 else [0, 1, 37, max(150, d + 50), 22]
    n = sum(sizes)
    assert n % 64 and len(sizes) == V
    rs = np.random.RandomState(17 * V + d)
    assign = rs.permutation(np.repeat(np.arange(V), sizes)).astype(np.int32)
    X = rs.randint(-4, 5, (n, d)).astype(np.float32)
    C = rs.randint(-3, 4, (V, d)).astype(np.float64)
    R = rs.randint(-3, 4, (V, d, d)).astype(np.float64)
    mu = rs.randint(-3, 4, (V, d)).astype(np.float64)
    return sizes, assign, X, C, R, mu


@pytest.mark.gpu
@pytest.mark.parametrize("d", [3, 64, 100])
@pytest.mark.parametrize("V", [1, 5])
def test_pieces_are_exact_on_integers(V, d):
    import torch
    lib = _L()
    L = lib.lib()
    sizes, assign, X, C, R, mu = _lattice(V, d)
    n = X.shape[0]
    order = np.argsort(assign, kind="stable").astype(np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    Xi, Ci, Ri, mi = X.astype(np.int64), C.astype(np.int64), R.astype(np.int64), mu.astype(np.int64)
    dX, dC, dA, dO, dOff, dR, dM = _dev(X), _dev(C), _dev(assign), _dev(order), _dev(off), _dev(R), _dev(mu)

    # residuals, in group order
    res_ref = Xi[order] - Ci[assign[order]]
    res = _nan((n, d))
    lib.check(L.cis_train_residuals_dev(dX.data_ptr(), n, d, dC.data_ptr(), V, dA.data_ptr(), dO.data_ptr(), n, res.data_ptr(), _stream()))
    res_h = res.cpu().numpy()
    np.testing.assert_array_equal(res_h, res_ref.astype(np.float64))

    # Gram sums: the int64 products, and the host entry point's bits
    G, S = _nan((V, d, d)), _nan((V, d))
    lib.check(L.cis_train_gram_dev(res.data_ptr(), n, d, dOff.data_ptr(), V, G.data_ptr(), S.data_ptr(), _stream()))
    G_ref = np.stack([res_ref[off[g]:off[g + 1]].T @ res_ref[off[g]:off[g + 1]] for g in range(V)])
    S_ref = np.stack([res_ref[off[g]:off[g + 1]].sum(0) for g in range(V)])
    assert np.abs(G_ref).max() < F53
    np.testing.assert_array_equal(G.cpu().numpy(), G_ref.astype(np.float64))
    np.testing.assert_array_equal(S.cpu().numpy(), S_ref.astype(np.float64))
    G_host, S_host = np.full((V, d, d), np.nan), np.full((V, d), np.nan)
    lib.check(L.cis_train_gram(lib.ptr(res_h), n, d, lib.ptr(off), V, lib.ptr(G_host), lib.ptr(S_host)))
    assert G_host.tobytes() == G.cpu().numpy().tobytes() and S_host.tobytes() == S.cpu().numpy().tobytes()

    # projections: in group order, scattered back to the original order by the kernel, and the host entry point's bits
    Y_ref = np.zeros((n, d), dtype=np.int64)
    for g in range(V):
        Y_ref[off[g]:off[g + 1]] = (res_ref[off[g]:off[g + 1]] - mi[g]) @ Ri[g].T
    assert np.abs(Y_ref).max() < F53
    Y, Ys = _nan((n, d)), _nan((n, d))
    lib.check(L.cis_train_project_dev(res.data_ptr(), n, d, dOff.data_ptr(), V, max(sizes), dR.data_ptr(), dM.data_ptr(), None,
                                      Y.data_ptr(), _stream()))
    lib.check(L.cis_train_project_dev(res.data_ptr(), n, d, dOff.data_ptr(), V, max(sizes), dR.data_ptr(), dM.data_ptr(), dO.data_ptr(),
                                      Ys.data_ptr(), _stream()))
    np.testing.assert_array_equal(Y.cpu().numpy(), Y_ref.astype(np.float64))
    scattered = np.empty_like(Y_ref)
    scattered[order] = Y_ref
    np.testing.assert_array_equal(Ys.cpu().numpy(), scattered.astype(np.float64))
    Y_host = np.full((n, d), np.nan)
    lib.check(L.cis_train_project(lib.ptr(res_h), n, d, lib.ptr(off), V, lib.ptr(R), lib.ptr(mu), lib.ptr(Y_host)))
    assert Y_host.tobytes() == Y.cpu().numpy().tobytes()

    # covariance and mean from the sums: numpy's expression; the identity below d rows; zeros for the mean of an empty group
    cov, m = _nan((V, d, d)), _nan((V, d))
    lib.check(L.cis_train_cov_dev(G.data_ptr(), S.data_ptr(), dOff.data_ptr(), V, d, cov.data_ptr(), m.data_ptr(), _stream()))
    cov, m = cov.cpu().numpy(), m.cpu().numpy()
    computed = 0
    for g, ng in enumerate(sizes):
        mg = S_ref[g] / ng if ng else np.zeros(d)
        np.testing.assert_allclose(m[g], mg, rtol=1e-12, atol=0)
        if ng < d:
            np.testing.assert_array_equal(cov[g], np.eye(d))
        else:
            A = G_ref[g].astype(np.float64)
            want = (A + A.T) / (2.0 * (ng - 1)) - np.outer(mg, mg)
            assert np.abs(cov[g] - want).max() <= 1e-12 * np.abs(want).max()
            computed += 1
    assert computed >= 1

    # rotation rows from eigenvector columns
    rs = np.random.RandomState(d)
    vecs = rs.randn(V, d, d)
    perm = np.stack([rs.permutation(d) for _ in range(V)]).astype(np.int32)
    Rp, dV, dP = _nan((V, d, d)), _dev(vecs), _dev(perm)
    lib.check(L.cis_train_rotation_pack_dev(dV.data_ptr(), dP.data_ptr(), V, d, Rp.data_ptr(), _stream()))
    torch.cuda.synchronize()
    for g in range(V):
        np.testing.assert_array_equal(Rp[g].cpu().numpy(), vecs[g][:, perm[g]].T)


# ---- the stage ------------------------------------------------------------------------------------------------------------------

_stage_cache = {}


def _stage_inputs():
    """6000 x 32 descriptor-like rows and 8 centroids: six data rows, one pushed out along a data row until fewer than d rows
    remain with it, one far away from everything (empty)."""
    if not _stage_cache:
        import golden_inputs as gi
        T = _T()
        X = gi.descriptor_like(6000, 32, 77, np.float32)
        C = X[np.random.RandomState(5).choice(6000, 8, False)].astype(np.float64)
        C[6] = 1.6 * X[0].astype(np.float64)
        C[7] = 10.0
        assign = T.assign_clusters(X, C)
        counts = np.bincount(assign, minlength=8)
        assert 1 <= counts[6] < 32 and counts[7] == 0 and (counts[:6] >= 32).all(), counts
        _stage_cache.update(X=X, C=C, assign=assign, counts=counts)
    return _stage_cache


@pytest.mark.gpu
def test_the_stage_against_numpy():
    import torch
    T = _T()
    z = _stage_inputs()
    X, C, assign, counts = z["X"], z["C"], z["assign"], z["counts"]
    d, nb = 32, 2
    keep = (T.KMEANS_BACKEND, T.ACCUM_BACKEND)
    try:
        T.KMEANS_BACKEND, T.ACCUM_BACKEND = "sklearn", "host"
        R_h, mu_h, assign_h, res = T.local_rotations(X, C, nb)
    finally:
        T.KMEANS_BACKEND, T.ACCUM_BACKEND = keep
    assert (assign_h == assign).all()
    x = _dev(X)
    a_dev = _dev(assign.astype(np.int32))
    R, mu, a_out, W = T.local_rotations_dev(x, C, nb, assign=a_dev)
    assert a_out is a_dev and R.dtype == np.float64 and mu.dtype == np.float64
    scale = np.abs(mu_h).max()
    assert np.abs(mu - mu_h).max() <= 1e-12 * scale
    assert (mu[7] == 0).all()
    for c in range(8):
        if counts[c] < d:
            assert ((R[c] == 0) | (R[c] == 1)).all() and (R[c].sum(0) == 1).all() and (R[c].sum(1) == 1).all()  # a permutation matrix
            assert (W[c] == 1).all()
            continue
        r = res[assign == c]
        m = r.sum(axis=0) / len(r)
        A = r.T.dot(r)
        cov = (A + A.T) / (2.0 * (len(r) - 1)) - np.outer(m, m)
        norm = np.abs(np.linalg.eigvalsh(cov)).max()
        D = R[c] @ cov @ R[c].T
        assert np.abs(D - np.diag(np.diag(D))).max() <= 16 * d * U * norm, c
        want = W[c][T.eigenvalue_allocation(nb, W[c])]
        assert np.abs(np.diag(D) - want).max() <= 16 * d * U * norm, c
        assert np.abs(R[c] @ R[c].T - np.eye(d)).max() <= 16 * d * U, c
    # the projection: every row, then a sample of rows in the sample's order
    ref = np.einsum("nij,nj->ni", R[assign], res - mu[assign])
    Y = T.project_to_local_dev(x, C, a_dev, R, mu)
    assert Y.is_cuda and Y.dtype == torch.float64
    assert np.abs(Y.cpu().numpy() - ref).max() <= 1e-10
    rows = np.random.RandomState(3).choice(6000, 1500, False)
    Ys = T.project_to_local_dev(x, C, a_dev, R, mu, rows)
    assert np.abs(Ys.cpu().numpy() - ref[rows]).max() <= 1e-10
    # and the host path's own projection with the device's rotations
    np.testing.assert_allclose(T.project_to_local(res, assign, R, mu), Y.cpu().numpy(), rtol=0, atol=1e-10)


# ---- whole fits -----------------------------------------------------------------------------------------------------------------

def _fit_error(X, rotations, seed):
    from columbiaimagesearch_amd.lopq import LOPQModel
    T = _T()
    keep = (T.KMEANS_BACKEND, T.ROTATION_BACKEND)
    try:
        T.KMEANS_BACKEND, T.ROTATION_BACKEND = "device", rotations
        m = LOPQModel(V=8, M=4)
        m.fit(X, kmeans_coarse_iters=10, kmeans_local_iters=20, n_init=1, random_state=seed)
    finally:
        T.KMEANS_BACKEND, T.ROTATION_BACKEND = keep
    sample = X[:2000].astype(np.float64)
    co, fi = m.predict_batch(sample)
    rec = np.stack([m.reconstruct((tuple(c), tuple(f))) for c, f in zip(co, fi)])
    return float(((rec - sample) ** 2).sum(1).mean())


@pytest.mark.gpu
def test_fits_through_both_backends():
    """LOPQModel(V=8, M=4).fit with the k-means on the device, rotations on the host and on the device, three random_states: the
    mean squared reconstruction error of 2000 training vectors.  The eigenvector signs of the device path act as another seeding
    of the subquantizer k-means, so the device is held to the host's own spread: with r = the host's largest / smallest value over
    the three seeds, the device's mean is at most the host's largest value times 1 + 3 (r - 1).  Three draws underestimate the
    range they come from (a fourth draw from the same distribution exceeds their maximum one time in four), and the k-means sums
    are float32 atomics, so a fit repeats only to within that spread: three observed ranges above the largest value seen leave
    room for both, and stay far below the 1.1 the seeding test allows against scikit-learn, which caps the margin.
    Measured on an MI355X: r = 1.0024, margin 1.0071."""
    X = _stage_inputs()["X"]
    host = [_fit_error(X, "host", s) for s in (1, 2, 3)]
    dev = [_fit_error(X, "device", s) for s in (1, 2, 3)]
    for s, h, v in zip((1, 2, 3), host, dev):
        print("random_state %d: reconstruction error host %.6f device %.6f" % (s, h, v))
    margin = min(1.1, 1.0 + 3.0 * (max(host) / min(host) - 1.0))
    print("host spread (largest / smallest) %.4f, margin %.4f, device mean %.6f, limit %.6f"
          % (max(host) / min(host), margin, np.mean(dev), max(host) * margin))
    assert np.mean(dev) <= max(host) * margin


def test_the_switch():
    T = _T()
    assert T.ROTATION_BACKEND == "host"
    keep = (T.KMEANS_BACKEND, T.ROTATION_BACKEND)
    rs = np.random.RandomState(0)
    try:
        T.ROTATION_BACKEND, T.KMEANS_BACKEND = "device", "sklearn"
        with pytest.raises(ValueError, match="KMEANS_BACKEND"):
            T.train(rs.randn(64, 8).astype(np.float32), V=2, M=2, subquantizer_clusters=4, n_init=1, random_state=0)
        T.KMEANS_BACKEND = "device"
        with pytest.raises(ValueError, match="128"):
            T.train(rs.randn(64, 260).astype(np.float32), V=2, M=2, subquantizer_clusters=4, n_init=1, random_state=0)
        T.ROTATION_BACKEND = "gpu"
        with pytest.raises(ValueError, match="ROTATION_BACKEND"):
            T.train(rs.randn(64, 8).astype(np.float32), V=2, M=2, subquantizer_clusters=4, n_init=1, random_state=0)
    finally:
        T.KMEANS_BACKEND, T.ROTATION_BACKEND = keep
    assert T.ROTATION_BACKEND == "host"
