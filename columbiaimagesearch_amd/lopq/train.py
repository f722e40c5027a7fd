"""Host-side LOPQ training (numpy + scikit-learn), vectorised.

Restates the training recipe of the reference (lopq/lopq/model.py:19-437) without its per-sample
Python loops: covariance accumulators become matrix products.  k-means results depend on the
scikit-learn version, so training is judged by distortion/recall, not bit parity (SURVEY.md
section 8c caveat ii, section 8f row 3).  Not on the encode/search hot path.

Five switches move work to the GPU, all off by default: PCA_BACKEND ("device": train_pca's sums and eigendecomposition,
train_pca_dev with cis_sym_eig_large_dev, csrc/sym_eig_block.hip), ACCUM_BACKEND ("hip": covariance accumulations and projections),
KMEANS_BACKEND ("hip" / "device": Lloyd iterations), SEED_BACKEND ("device": the k-means++ seeds of kmeans_dev are drawn on the
resident data by cis_kmeanspp_dev, csrc/kmeans_seed.hip, and never visit the host) and ROTATION_BACKEND ("device": the whole
local-rotation stage -- residuals, covariances, eigendecompositions (cis_sym_eig_dev, csrc/sym_eig.hip), projections -- on the
data the k-means uploaded; only the eigenvalues and the rotations themselves, O(V d^2) numbers, visit the host).
"""
import logging

import numpy as np

logger = logging.getLogger(__name__)


def eigenvalue_allocation(num_buckets, eigenvalues):
    """Greedy balancing of eigenvalue log-products over buckets (OPQ section 3.2.4).
    reference: lopq/lopq/model.py:19-71.  Returns the permutation of dimensions."""
    eigenvalues = np.asarray(eigenvalues, dtype=np.float64)
    D = eigenvalues.shape[0]
    per_bucket = D // num_buckets
    nz = np.abs(eigenvalues[np.nonzero(eigenvalues)])
    scaled = eigenvalues / (nz.min() if nz.size else 1.0)  # keeps every |eigenvalue| >= 1
    with np.errstate(divide="ignore"):
        logs = np.log2(np.abs(scaled))
    load = np.zeros(num_buckets)
    fill = np.zeros(num_buckets, dtype=np.int64)
    perm = np.zeros((num_buckets, per_bucket), dtype=np.int64)
    for dim in np.argsort(scaled)[::-1]:
        open_buckets = np.nonzero(fill < per_bucket)[0]
        b = open_buckets[np.argmin(load[open_buckets])]
        load[b] += logs[dim]
        perm[b, fill[b]] = dim
        fill[b] += 1
    return perm.reshape(D)


def eigenvalue_allocation_batch(num_buckets, eigenvalues):
    """eigenvalue_allocation for every row of `eigenvalues` [G, d] at once: [G, d] int64, row g the permutation of row g.  One
    loop over the d dimensions, vector operations over the G rows.  Equal eigenvalues are taken in the reverse of a stable
    ascending sort (what the scalar function does whenever the values are distinct)."""
    W = np.asarray(eigenvalues, dtype=np.float64)
    if W.ndim != 2:
        raise ValueError("expected [G, d] eigenvalues, got shape %r" % (W.shape,))
    G, D = W.shape
    per_bucket = D // num_buckets
    if per_bucket * num_buckets != D:
        raise ValueError("%d dimensions do not split into %d buckets" % (D, num_buckets))
    smallest = np.where(W != 0, np.abs(W), np.inf).min(axis=1) if D else np.ones(G)
    scaled = W / np.where(np.isfinite(smallest), smallest, 1.0)[:, None]
    with np.errstate(divide="ignore"):
        logs = np.log2(np.abs(scaled))
    order = np.argsort(scaled, axis=1, kind="stable")[:, ::-1]
    rows = np.arange(G)
    load = np.zeros((G, num_buckets))
    fill = np.zeros((G, num_buckets), dtype=np.int64)
    perm = np.zeros((G, num_buckets, per_bucket), dtype=np.int64)
    for t in range(D):
        dim = order[:, t]
        b = np.where(fill < per_bucket, load, np.inf).argmin(axis=1)  # the first of the least loaded open buckets
        load[rows, b] += logs[rows, dim]
        perm[rows, b, fill[rows, b]] = dim
        fill[rows, b] += 1
    return perm.reshape(G, D)


def assign_clusters(data, C, chunk=8192):
    """argmin_c ||x - c||^2 with the reference's direct (x - c)^2 form (lopq/lopq/utils.py:47)."""
    out = np.empty(data.shape[0], dtype=np.int64)
    for a in range(0, data.shape[0], chunk):
        d = data[a:a + chunk, None, :] - C[None, :, :]
        out[a:a + chunk] = np.einsum("nvd,nvd->nv", d, d).argmin(axis=1)
    return out


ACCUM_BACKEND = "host"  # "hip": covariance accumulations and residual projections on the GPU (csrc/lopq_train.hip)


def _group_rows(assign, groups):
    """Stable order of the rows by group + the group offsets (what cis_train_gram / cis_train_project take)."""
    order = np.argsort(assign, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=groups))]).astype(np.int64)
    return order, off


def gram_hip(X, assign=None, groups=1):
    """(G [groups,d,d], S [groups,d]): per-group sums of x x^T and of x, float64, on the GPU."""
    from .. import _lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, d = X.shape
    if assign is None:
        off = np.array([0, n], dtype=np.int64)
    else:
        order, off = _group_rows(np.asarray(assign, dtype=np.int64), groups)
        X = np.ascontiguousarray(X[order])
    G = np.empty((groups, d, d))
    S = np.empty((groups, d))
    _lib.check(_lib.lib().cis_train_gram(_lib.ptr(X), n, d, _lib.ptr(off), groups, _lib.ptr(G), _lib.ptr(S)))
    return G, S


def local_rotations(data, C, num_buckets, dev=None):
    """Per-cluster residual mean and PCA rotation with balanced variance.
    reference: lopq/lopq/model.py:74-206.  Returns (R [V,d,d], mu [V,d], assignments, residuals).
    dev: `data` as a float32 tensor on the GPU, if the caller has one (KMEANS_BACKEND = "device" assigns from it)."""
    V, d = C.shape
    assign = assign_clusters_dev(data if dev is None else dev, C) if KMEANS_BACKEND == "device" else assign_clusters(data, C)
    residuals = np.asarray(data - C[assign], dtype=np.float64)
    R = np.zeros((V, d, d))
    mu = np.zeros((V, d))
    grams = None
    if ACCUM_BACKEND == "hip":  # all V accumulators in one launch: the reference's per-sample np.outer loop (:142-155)
        grams, sums = gram_hip(residuals, assign, V)
        counts = np.bincount(assign, minlength=V)
    for c in range(V):
        if grams is None:
            r = residuals[assign == c]
            n = r.shape[0]
            if n > 0:
                mu[c] = r.sum(axis=0) / n
        else:
            n = int(counts[c])
            if n > 0:
                mu[c] = sums[c] / n
        if n < d:
            logger.warning("Fewer points (%d) than dimensions (%d) in rotation computation for cluster %d", n, d, c)
            eigvals, vecs = np.ones(d), np.eye(d)
        else:
            A = r.T.dot(r) if grams is None else grams[c]
            cov = (A + A.T) / (2.0 * (n - 1)) - np.outer(mu[c], mu[c])
            eigvals, vecs = np.linalg.eigh(cov)
        R[c] = vecs[:, eigenvalue_allocation(num_buckets, eigvals)].T
    return R, mu, assign, residuals


def project_to_local(residuals, assign, R, mu):
    """R[a] . (res - mu[a]) for every training residual.  reference: lopq/lopq/model.py:209-234."""
    if ACCUM_BACKEND == "hip":
        from .. import _lib
        V, d = mu.shape
        order, off = _group_rows(np.asarray(assign, dtype=np.int64), V)
        X = np.ascontiguousarray(np.asarray(residuals, dtype=np.float64)[order])
        Y = np.empty_like(X)
        Rc, mc = np.ascontiguousarray(R, dtype=np.float64), np.ascontiguousarray(mu, dtype=np.float64)
        _lib.check(_lib.lib().cis_train_project(_lib.ptr(X), X.shape[0], d, _lib.ptr(off), V, _lib.ptr(Rc), _lib.ptr(mc), _lib.ptr(Y)))
        out = np.empty_like(Y)
        out[order] = Y
        return out
    out = np.zeros(residuals.shape)
    for c in np.unique(assign):
        sel = np.nonzero(assign == c)[0]
        out[sel] = (residuals[sel] - mu[c]).dot(R[c].T)
    return out


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def kmeans_pp_init(data, k, rs, sample=20000):
    """k-means++ seeding (Arthur & Vassilvitskii) on a subsample, on the host: k sequential draws."""
    n = data.shape[0]
    pick = rs.choice(n, min(n, sample), replace=False)
    if _is_tensor(data):  # resident training set: only the subsample comes to the host
        import torch
        x = data[torch.as_tensor(pick, device=data.device)].cpu().numpy().astype(np.float64)
    else:
        x = np.asarray(data[pick], dtype=np.float64)
    C = np.empty((k, x.shape[1]))
    C[0] = x[rs.randint(len(x))]
    d2 = ((x - C[0]) ** 2).sum(axis=1)
    for j in range(1, k):
        tot = d2.sum()
        C[j] = x[rs.randint(len(x))] if tot <= 0 else x[np.searchsorted(np.cumsum(d2), rs.rand() * tot)]
        d2 = np.minimum(d2, ((x - C[j]) ** 2).sum(axis=1))
    return C


def kmeans_pp_init_dev(x, k, rs, sample=20000):
    """k-means++ seeding on the GPU (cis_kmeanspp_dev, csrc/kmeans_seed.hip): [k, d] float32 centroids, rows of `x`, as a tensor on
    x's device; only enqueued on the current stream.  x: a resident float32 [n, d] tensor.  sample: an int seeds on
    rs.choice(n, min(n, sample), replace=False), gathered on the device; None seeds on all n rows without a gather.  Then
    u = rs.rand(k) is uploaded: centre 0 is row floor(u[0] * rows), draw j takes the first row whose running sum of squared
    distances exceeds u[j] * total (include/cis_hip.h).  The RandomState is consumed differently from kmeans_pp_init (k uniforms at
    once; no randint), so the two seedings give different seeds for one random_state."""
    import torch
    from .. import _lib
    x = _resident(x)
    n, d = int(x.shape[0]), int(x.shape[1])
    if sample is not None:
        pick = rs.choice(n, min(n, int(sample)), replace=False)
        x = x[torch.as_tensor(pick, device=x.device)].contiguous()
        n = int(x.shape[0])
    u = torch.from_numpy(rs.rand(int(k))).to(x.device)
    C = torch.empty((int(k), d), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().cis_kmeanspp_dev(x.data_ptr(), n, d, int(k), u.data_ptr(), C.data_ptr(), None, None,
                                           torch.cuda.current_stream(x.device).cuda_stream))
    return C


def kmeans_hip(data, k, iters, n_init=1, random_state=None):
    """Lloyd iterations on the GPU (cis_kmeans) from k-means++ seeds drawn on the host; best of n_init by inertia.
    Counterpart of the scikit-learn call of the reference (lopq/lopq/model.py:359-372,:417-432); float32."""
    from .. import _lib
    x = np.ascontiguousarray(data, dtype=np.float32)
    n, d = x.shape
    rs = np.random.RandomState(random_state)
    best, best_inertia = None, np.inf
    for _ in range(max(int(n_init), 1)):
        C = np.ascontiguousarray(kmeans_pp_init(x, k, rs), dtype=np.float32)
        inertia = _lib.ctypes.c_double(0.0)
        _lib.check(_lib.lib().cis_kmeans(_lib.ptr(x), n, d, k, int(iters), _lib.ptr(C), None, _lib.ctypes.byref(inertia)))
        if inertia.value < best_inertia:
            best, best_inertia = C, inertia.value
    return best.astype(np.float64), best_inertia


def _resident(data):
    """`data` as a contiguous float32 [n, d] tensor on the GPU: a numpy array is uploaded, a tensor must already be one."""
    import torch
    if _is_tensor(data):
        if not (data.is_cuda and data.dim() == 2 and data.dtype == torch.float32):
            raise ValueError("expected a float32 [n, d] tensor on the GPU, got %s %s on %s" % (data.dtype, tuple(data.shape), data.device))
        return data.contiguous()
    x = np.ascontiguousarray(data, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("expected an [n, d] matrix, got shape %r" % (x.shape,))
    return torch.from_numpy(x).to(torch.device("cuda", torch.cuda.current_device()))


def kmeans_dev(data, k, iters, n_init=1, random_state=None):
    """kmeans_hip for codebooks of any size, on data that stays on the GPU (cis_kmeans_dev, csrc/kmeans_mfma.hip): k-means++ seeds
    from the host (SEED_BACKEND = "host": kmeans_pp_init) or drawn on the device (SEED_BACKEND = "device": kmeans_pp_init_dev on
    SEED_SAMPLE rows, handed to cis_kmeans_dev as they are), best of n_init by reported inertia; (float64 centroids, inertia).
    data: a numpy array (uploaded once, reused by every run) or a float32 tensor on the GPU."""
    import torch
    from .. import _lib
    x = _resident(data)
    n, d = int(x.shape[0]), int(x.shape[1])
    rs = np.random.RandomState(random_state)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    inertia = torch.empty(1, dtype=torch.float64, device=x.device)
    if SEED_BACKEND not in ("host", "device"):
        raise ValueError("SEED_BACKEND must be 'host' or 'device', got %r" % (SEED_BACKEND,))
    best, best_inertia = None, np.inf
    for _ in range(max(int(n_init), 1)):
        if SEED_BACKEND == "device":
            C = kmeans_pp_init_dev(x, k, rs, SEED_SAMPLE)
        else:
            C = torch.from_numpy(np.ascontiguousarray(kmeans_pp_init(x, k, rs), dtype=np.float32)).to(x.device)
        _lib.check(_lib.lib().cis_kmeans_dev(x.data_ptr(), n, d, int(k), int(iters), C.data_ptr(), None, inertia.data_ptr(), stream))
        got = float(inertia.cpu()[0])
        if got < best_inertia:
            best, best_inertia = C.cpu().numpy(), got
    return best.astype(np.float64), best_inertia


def _assign_dev(x, C):
    """One assignment pass of cis_kmeans_dev (iters = 0) on the resident float32 `x`: int32 assignments, a tensor on x's device."""
    import torch
    from .. import _lib
    Cd = torch.from_numpy(np.ascontiguousarray(C, dtype=np.float32)).to(x.device)
    if Cd.dim() != 2 or Cd.shape[1] != x.shape[1]:
        raise ValueError("centroids %r do not match data %r" % (tuple(Cd.shape), tuple(x.shape)))
    assign = torch.empty(int(x.shape[0]), dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().cis_kmeans_dev(x.data_ptr(), int(x.shape[0]), int(x.shape[1]), int(Cd.shape[0]), 0, Cd.data_ptr(),
                                         assign.data_ptr(), None, torch.cuda.current_stream(x.device).cuda_stream))
    return assign


def assign_clusters_dev(data, C):
    """assign_clusters on the GPU: one assignment pass of cis_kmeans_dev (iters = 0) in float32, int64 assignments on the host.
    The kernel minimises |c|^2 - 2 x.c, so a point between two almost equally near centroids may go to either."""
    return _assign_dev(_resident(data), C).cpu().numpy().astype(np.int64)


def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def sym_eig_dev(A):
    """Eigendecompositions of a float64 [batch, d, d] tensor of symmetric matrices on the GPU (cis_sym_eig_dev, d <= 128):
    (W [batch, d] ascending, V [batch, d, d] with column j the eigenvector of W[:, j], info [batch] int32: the Jacobi sweeps used, or
    -1 for a matrix that was not finite or did not converge).  Tensors on A's device; only enqueued on the current stream."""
    import torch
    from .. import _lib
    if not (_is_tensor(A) and A.is_cuda and A.dim() == 3 and A.dtype == torch.float64 and A.shape[1] == A.shape[2]):
        raise ValueError("expected a float64 [batch, d, d] tensor on the GPU")
    A = A.contiguous()
    batch, d = int(A.shape[0]), int(A.shape[1])
    W = torch.empty((batch, d), dtype=torch.float64, device=A.device)
    V = torch.empty((batch, d, d), dtype=torch.float64, device=A.device)
    info = torch.empty(batch, dtype=torch.int32, device=A.device)
    _lib.check(_lib.lib().cis_sym_eig_dev(A.data_ptr(), batch, d, W.data_ptr(), V.data_ptr(), info.data_ptr(), _stream(A)))
    return W, V, info


def _groups_dev(assign, V):
    """Plumbing of the grouped kernels, on the device: (stable order of the rows by group [n] int64, group offsets [V+1] int64,
    largest group's size).  Only the last comes to the host."""
    import torch
    order = torch.argsort(assign, stable=True)
    counts = torch.bincount(assign, minlength=V)
    off = torch.zeros(V + 1, dtype=torch.int64, device=assign.device)
    off[1:] = torch.cumsum(counts, 0)
    return order, off, (int(counts.max()) if assign.numel() else 0)


def residuals_dev(x, C, assign, rows):
    """float64 [len(rows), d] tensor: x[rows] - C[assign[rows]] (cis_train_residuals_dev).  x: resident float32 [n, d], C: float64
    [V, d] tensor, assign: int32 [n] tensor, rows: int64 tensor of row numbers."""
    import torch
    from .. import _lib
    out = torch.empty((int(rows.shape[0]), int(x.shape[1])), dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().cis_train_residuals_dev(x.data_ptr(), int(x.shape[0]), int(x.shape[1]), C.data_ptr(), int(C.shape[0]),
                                                  assign.data_ptr(), rows.data_ptr(), int(rows.shape[0]), out.data_ptr(), _stream(x)))
    return out


def gram_dev(res, off, groups):
    """gram_hip on rows that are on the device and sorted by group (cis_train_gram_dev): (G [groups,d,d], S [groups,d]) tensors."""
    import torch
    from .. import _lib
    n, d = int(res.shape[0]), int(res.shape[1])
    G = torch.empty((groups, d, d), dtype=torch.float64, device=res.device)
    S = torch.empty((groups, d), dtype=torch.float64, device=res.device)
    _lib.check(_lib.lib().cis_train_gram_dev(res.data_ptr(), n, d, off.data_ptr(), groups, G.data_ptr(), S.data_ptr(), _stream(res)))
    return G, S


def local_rotations_dev(x, C, num_buckets, assign=None):
    """local_rotations on the resident float32 `x` (ROTATION_BACKEND = "device"): residuals in group order, their Gram sums, the
    covariances, one batched eigendecomposition and the rotation rows, all on the device; the eigenvalues [V, d] come to the host
    for eigenvalue_allocation_batch and the permutations go back.  Returns (R [V,d,d], mu [V,d], assign, W [V,d]): R, mu and
    the eigenvalues W as float64 numpy arrays, assign as the int32 tensor on the device it was computed from (or the one given).
    A cluster with fewer than d points gets the identity covariance, hence W = 1 and a permutation matrix R, as on the host."""
    import torch
    from .. import _lib
    L = _lib.lib()
    V, d = C.shape
    if d > 128:
        raise ValueError("ROTATION_BACKEND = 'device' holds a d x d covariance in LDS: d = D/2 must be <= 128, got %d" % d)
    if assign is None:
        assign = _assign_dev(x, C)
    st = _stream(x)
    Cd = torch.from_numpy(np.ascontiguousarray(C, dtype=np.float64)).to(x.device)
    order, off, _ = _groups_dev(assign, V)
    res = residuals_dev(x, Cd, assign, order)
    G, S = gram_dev(res, off, V)
    del res
    cov, mu = torch.empty_like(G), torch.empty_like(S)
    _lib.check(L.cis_train_cov_dev(G.data_ptr(), S.data_ptr(), off.data_ptr(), V, d, cov.data_ptr(), mu.data_ptr(), st))
    W, vecs, info = sym_eig_dev(cov)
    Wh, failed = W.cpu().numpy(), np.nonzero(info.cpu().numpy() < 0)[0]
    if failed.size:
        raise FloatingPointError("no eigendecomposition for the residual covariance of cluster(s) %s (not finite, or not converged)"
                                 % failed[:8].tolist())
    small = np.nonzero(np.diff(off.cpu().numpy()) < d)[0]
    for c in small[:16]:
        logger.warning("Fewer points than dimensions (%d) in rotation computation for cluster %d", d, c)
    perm = torch.from_numpy(eigenvalue_allocation_batch(num_buckets, Wh).astype(np.int32)).to(x.device)
    R = torch.empty_like(cov)
    _lib.check(L.cis_train_rotation_pack_dev(vecs.data_ptr(), perm.data_ptr(), V, d, R.data_ptr(), st))
    return R.cpu().numpy(), mu.cpu().numpy(), assign, Wh


def project_to_local_dev(x, C, assign, R, mu, rows=None):
    """project_to_local on the device: R[a] . (x[r] - C[a] - mu[a]) for r in `rows` (default: every row), a float64 [len(rows), d]
    tensor in the order of `rows`.  x: resident float32, assign: its int32 assignments on the device, C / R / mu: numpy arrays;
    rows: int64 row numbers (numpy or tensor).  The rows are grouped by cluster for the kernel and scattered back by it."""
    import torch
    from .. import _lib
    V, d = mu.shape
    if rows is None:
        rows = torch.arange(int(x.shape[0]), dtype=torch.int64, device=x.device)
    elif not _is_tensor(rows):
        rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(x.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(x.device)
    Cd, Rd, md = up(C), up(R), up(mu)
    order, off, max_rows = _groups_dev(assign[rows], V)
    res = residuals_dev(x, Cd, assign, rows[order].contiguous())
    Y = torch.empty_like(res)
    _lib.check(_lib.lib().cis_train_project_dev(res.data_ptr(), int(res.shape[0]), d, off.data_ptr(), V, max_rows, Rd.data_ptr(),
                                                md.data_ptr(), order.data_ptr(), Y.data_ptr(), _stream(x)))
    return Y


# "hip": Lloyd iterations on the GPU where the codebook fits the LDS kernel (k * d <= 7680), scikit-learn beyond.
# "device": every codebook, and every assignment of the training set, on the GPU (kmeans_dev / assign_clusters_dev).
KMEANS_BACKEND = "sklearn"
# Where kmeans_dev draws its k-means++ seeds.  "host": kmeans_pp_init, numpy on a subsample copied to the host (what kmeans_hip always
# does: cis_kmeans takes host pointers).  "device": kmeans_pp_init_dev on SEED_SAMPLE rows of the resident data (None: all rows); a
# different use of the RandomState, so different seeds for one random_state.
SEED_BACKEND = "host"
SEED_SAMPLE = 20000
# "host": local_rotations / project_to_local (numpy, or the ACCUM_BACKEND kernels on host arrays).  "device": local_rotations_dev /
# project_to_local_dev on the upload the coarse k-means made; needs KMEANS_BACKEND = "device" and d = D/2 <= 128 (ValueError otherwise).
ROTATION_BACKEND = "host"


def _kmeans(data, k, iters, n_init, random_state, dev=None):
    if KMEANS_BACKEND == "device":
        return kmeans_dev(data if dev is None else dev, k, iters, n_init, random_state)[0]
    if KMEANS_BACKEND == "hip" and k * data.shape[1] <= 7680:
        return kmeans_hip(data, k, iters, n_init, random_state)[0]
    from sklearn.cluster import MiniBatchKMeans
    km = MiniBatchKMeans(n_clusters=k, init="k-means++", max_iter=iters, n_init=n_init, batch_size=10000,
                         verbose=False, random_state=random_state)
    km.fit(data)
    return km.cluster_centers_


def sym_eig_large_dev(A, block=0):
    """Eigendecomposition of one float64 [d, d] symmetric tensor on the GPU, 1 <= d <= 4096 (cis_sym_eig_large_dev,
    csrc/sym_eig_block.hip: block Jacobi in HBM, blocks of `block` = 64 or 32 columns, 0 = the default): (W [d] ascending, V [d, d]
    with column j the eigenvector of W[j], info [1] int32: the block sweeps used, or -1 for a matrix that was not finite or did not
    converge).  Tensors on A's device.  The call waits for the device once per block sweep; the workspace is a torch allocation."""
    import torch
    from .. import _lib
    if not (_is_tensor(A) and A.is_cuda and A.dim() == 2 and A.dtype == torch.float64 and A.shape[0] == A.shape[1]):
        raise ValueError("expected a float64 [d, d] tensor on the GPU")
    A = A.contiguous()
    d = int(A.shape[0])
    L = _lib.lib()
    need = int(L.cis_sym_eig_large_workspace(d))
    if need < 0:
        _lib.check(need)
    W = torch.empty(d, dtype=torch.float64, device=A.device)
    V = torch.empty((d, d), dtype=torch.float64, device=A.device)
    info = torch.empty(1, dtype=torch.int32, device=A.device)
    work = torch.empty(need, dtype=torch.uint8, device=A.device)
    _lib.check(L.cis_sym_eig_large_dev(A.data_ptr(), d, int(block), W.data_ptr(), V.data_ptr(), info.data_ptr(), work.data_ptr(), need,
                                       _stream(A)))
    return W, V, info


# "host": train_pca below in numpy (its sums through cis_train_gram with ACCUM_BACKEND = "hip").  "device": train_pca_dev: the sums by
# cis_train_gram_dev and the eigendecomposition by cis_sym_eig_large_dev on data that is, or is uploaded once to, the GPU.
PCA_BACKEND = "host"
PCA_GRAM_ROWS = 32768  # rows converted to float64 and summed per cis_train_gram_dev call


def train_pca_dev(x, pca_dims=256, pca_subsample=None, stats=None):
    """train_pca on the GPU (PCA_BACKEND = "device"): the same dict and pca_dims, as numpy arrays.  x: a float32 or float64 [n, D]
    tensor on the GPU, or a numpy array, uploaded once as float32 (a float64 array as float64).  The sums G = X^T X and S = sum x
    come from cis_train_gram_dev with one group, PCA_GRAM_ROWS rows at a time as float64; mu = S / n and A = G / (n - 1) - mu mu^T
    are the host's expressions; cis_sym_eig_large_dev's last pca_dims eigenpairs are permuted by eigenvalue_allocation(2, E), which
    runs on the host on pca_dims numbers.  D <= 4096.  stats: a dict that receives the stage times in seconds (each stage waits for
    the device) and the block sweeps."""
    import time
    import torch
    if _is_tensor(x):
        if not (x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.float64)):
            raise ValueError("expected a float32 or float64 [n, D] tensor on the GPU, got %s %s on %s" % (x.dtype, tuple(x.shape), x.device))
        dev = x.device
    else:
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError("expected an [n, D] matrix, got shape %r" % (x.shape,))
        dev = torch.device("cuda", torch.cuda.current_device())
    if pca_subsample:
        x = x[:min(pca_subsample, x.shape[0])]
    n, D = int(x.shape[0]), int(x.shape[1])
    pca_dims = min(pca_dims, D)

    def lap(t0):
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    t0 = time.perf_counter()
    if not _is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64 if x.dtype == np.float64 else np.float32)).to(dev)
    t_upload = lap(t0) if stats is not None else 0.0

    t0 = time.perf_counter()
    G = torch.zeros((D, D), dtype=torch.float64, device=dev)
    S = torch.zeros(D, dtype=torch.float64, device=dev)
    for a in range(0, n, PCA_GRAM_ROWS):
        rows = x[a:a + PCA_GRAM_ROWS].to(torch.float64).contiguous()
        off = torch.tensor([0, int(rows.shape[0])], dtype=torch.int64, device=dev)
        g, s = gram_dev(rows, off, 1)
        G += g[0]
        S += s[0]
    # a division by a number on the device: torch turns a division by a host scalar into a product with its inverse
    mu = S / torch.tensor(float(n), dtype=torch.float64, device=dev)
    A = G / torch.tensor(float(n - 1), dtype=torch.float64, device=dev) - torch.outer(mu, mu)
    t_sums = lap(t0) if stats is not None else 0.0

    t0 = time.perf_counter()
    W, V, info = sym_eig_large_dev(A)
    sweeps = int(info.cpu()[0])
    t_eig = lap(t0) if stats is not None else 0.0
    if sweeps < 0:
        raise FloatingPointError("no eigendecomposition for the PCA covariance (not finite, or not converged)")

    t0 = time.perf_counter()
    E = W[D - pca_dims:].cpu().numpy()
    perm = torch.from_numpy(eigenvalue_allocation(2, E)).to(dev)
    P = V[:, D - pca_dims:][:, perm]
    out = {"mu": mu.cpu().numpy(), "P": P.cpu().numpy(), "E": E, "A": A.cpu().numpy(), "c": n}
    if stats is not None:
        stats.update(upload_s=t_upload, sums_s=t_sums, eig_s=t_eig, rest_s=lap(t0), block_sweeps=sweeps)
    return out, pca_dims


def train_pca(data, pca_dims=256, pca_subsample=None):
    """PCA basis with variance balanced over the two halves.  reference: lopq/lopq/model.py:242-287."""
    if PCA_BACKEND not in ("host", "device"):
        raise ValueError("PCA_BACKEND must be 'host' or 'device', got %r" % (PCA_BACKEND,))
    if PCA_BACKEND == "device":
        return train_pca_dev(data, pca_dims, pca_subsample)
    if pca_subsample:
        data = data[:min(pca_subsample, data.shape[0])]
    n, D = data.shape
    pca_dims = min(pca_dims, D)
    X = np.asarray(data, dtype=np.float64)
    if ACCUM_BACKEND == "hip":  # summed_covar of the reference's per-sample loop (:263-267) as one tiled product
        G, S = gram_hip(X)
        mu = S[0] / n
        A = G[0] / (n - 1) - np.outer(mu, mu)
    else:
        mu = X.mean(axis=0)
        A = X.T.dot(X) / (n - 1) - np.outer(mu, mu)
    E, P = np.linalg.eigh(A)
    E, P = E[-pca_dims:], P[:, -pca_dims:]
    P = P[:, eigenvalue_allocation(2, E)]
    return {"mu": mu, "P": P, "E": E, "A": A, "c": n}, pca_dims


def apply_pca_host(x, P, mu, renorm, dtype=np.float32):
    """Training-time apply_PCA on the host (reference: lopq/lopq/model.py:961-978)."""
    y = np.dot(x - mu, P)
    if renorm:
        y = y / np.linalg.norm(y, axis=-1, keepdims=True)
    return y.astype(dtype)


def train(data, V=8, M=4, subquantizer_clusters=256, parameters=None, kmeans_coarse_iters=10,
          kmeans_local_iters=20, n_init=10, subquantizer_sample_ratio=1.0, random_state=None, verbose=False):
    """Fit whatever is missing from `parameters`.  reference: lopq/lopq/model.py:339-437."""
    Cs = Rs = mus = subs = None
    if parameters is not None:
        Cs, Rs, mus, subs = parameters
    if Rs is None or mus is None:
        Rs = mus = None
    halves = np.split(data, 2, axis=1)
    if ROTATION_BACKEND not in ("host", "device"):
        raise ValueError("ROTATION_BACKEND must be 'host' or 'device', got %r" % (ROTATION_BACKEND,))
    on_dev = ROTATION_BACKEND == "device"
    if on_dev and KMEANS_BACKEND != "device":
        raise ValueError("ROTATION_BACKEND = 'device' works on the data KMEANS_BACKEND = 'device' uploads; KMEANS_BACKEND is %r"
                         % (KMEANS_BACKEND,))
    if on_dev and halves[0].shape[1] > 128:
        raise ValueError("ROTATION_BACKEND = 'device' holds a d x d covariance in LDS: d = D/2 must be <= 128, got %d"
                         % halves[0].shape[1])
    devs = [None, None]
    # one upload per half: the coarse k-means, the assignment and the device rotation stage share it
    if KMEANS_BACKEND == "device" and (Cs is None or Rs is None or (on_dev and subs is None)):
        devs = [_resident(h) for h in halves]
    if Cs is None:
        Cs = tuple(_kmeans(h, V, kmeans_coarse_iters, n_init, random_state, dev) for h, dev in zip(halves, devs))
    fitted = None
    if Rs is None:
        if on_dev:
            fitted = [local_rotations_dev(dev, C, M // 2) for C, dev in zip(Cs, devs)]
        else:
            fitted = [local_rotations(h, C, M // 2, dev) for h, C, dev in zip(halves, Cs, devs)]
        Rs = tuple(f[0] for f in fitted)
        mus = tuple(f[1] for f in fitted)
    if not on_dev:
        del devs
    if subs is not None:
        return tuple(Cs), tuple(Rs), tuple(mus), subs
    N = data.shape[0]
    n_sub = int(np.floor(min(subquantizer_sample_ratio, 1.0) * N))
    sample = np.random.RandomState(random_state).choice(N, n_sub, False)
    subs = []
    for s, (h, C) in enumerate(zip(halves, Cs)):
        if on_dev:  # the projected residuals stay on the GPU; each subquantizer gets its columns as one contiguous float32 block
            import torch
            assign = fitted[s][2] if fitted is not None else _assign_dev(devs[s], C)
            projected = project_to_local_dev(devs[s], C, assign, Rs[s], mus[s], sample)
            if projected.shape[1] % (M // 2):
                raise ValueError("%d dimensions do not split into %d subquantizers" % (projected.shape[1], M // 2))
            subs.append([_kmeans(None, subquantizer_clusters, kmeans_local_iters, n_init, random_state, p.to(torch.float32).contiguous())
                         for p in torch.chunk(projected, M // 2, dim=1)])
            del projected
            continue
        if fitted is not None:
            assign, residuals = fitted[s][2][sample], fitted[s][3][sample]
        else:
            hs = h[sample]
            assign = assign_clusters_dev(hs, C) if KMEANS_BACKEND == "device" else assign_clusters(hs, C)
            residuals = np.asarray(hs - C[assign], dtype=np.float64)
        projected = project_to_local(residuals, assign, Rs[s], mus[s])
        subs.append([_kmeans(p, subquantizer_clusters, kmeans_local_iters, n_init, random_state)
                     for p in np.split(projected, M // 2, axis=1)])
    return tuple(Cs), tuple(Rs), tuple(mus), tuple(subs)
