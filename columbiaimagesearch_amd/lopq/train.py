"""Host-side LOPQ training (numpy + scikit-learn), vectorised.

Restates the training recipe of the reference (lopq/lopq/model.py:19-437) without its per-sample
Python loops: covariance accumulators become matrix products.  k-means results depend on the
scikit-learn version, so training is judged by distortion/recall, not bit parity (SURVEY.md
section 8c caveat ii, section 8f row 3).  Not on the encode/search hot path.

Three switches move work to the GPU, all off by default: ACCUM_BACKEND ("hip": covariance accumulations and projections),
KMEANS_BACKEND ("hip" / "device": Lloyd iterations) and SEED_BACKEND ("device": the k-means++ seeds of kmeans_dev are drawn on the
resident data by cis_kmeanspp_dev, csrc/kmeans_seed.hip, and never visit the host).
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


def assign_clusters_dev(data, C):
    """assign_clusters on the GPU: one assignment pass of cis_kmeans_dev (iters = 0) in float32, int64 assignments on the host.
    The kernel minimises |c|^2 - 2 x.c, so a point between two almost equally near centroids may go to either."""
    import torch
    from .. import _lib
    x = _resident(data)
    Cd = torch.from_numpy(np.ascontiguousarray(C, dtype=np.float32)).to(x.device)
    if Cd.dim() != 2 or Cd.shape[1] != x.shape[1]:
        raise ValueError("centroids %r do not match data %r" % (tuple(Cd.shape), tuple(x.shape)))
    assign = torch.empty(int(x.shape[0]), dtype=torch.int32, device=x.device)
    _lib.check(_lib.lib().cis_kmeans_dev(x.data_ptr(), int(x.shape[0]), int(x.shape[1]), int(Cd.shape[0]), 0, Cd.data_ptr(),
                                         assign.data_ptr(), None, torch.cuda.current_stream(x.device).cuda_stream))
    return assign.cpu().numpy().astype(np.int64)


# "hip": Lloyd iterations on the GPU where the codebook fits the LDS kernel (k * d <= 7680), scikit-learn beyond.
# "device": every codebook, and every assignment of the training set, on the GPU (kmeans_dev / assign_clusters_dev).
KMEANS_BACKEND = "sklearn"
# Where kmeans_dev draws its k-means++ seeds.  "host": kmeans_pp_init, numpy on a subsample copied to the host (what kmeans_hip always
# does: cis_kmeans takes host pointers).  "device": kmeans_pp_init_dev on SEED_SAMPLE rows of the resident data (None: all rows); a
# different use of the RandomState, so different seeds for one random_state.
SEED_BACKEND = "host"
SEED_SAMPLE = 20000


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


def train_pca(data, pca_dims=256, pca_subsample=None):
    """PCA basis with variance balanced over the two halves.  reference: lopq/lopq/model.py:242-287."""
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
    devs = [None, None]
    if KMEANS_BACKEND == "device" and (Cs is None or Rs is None):  # one upload per half: the coarse k-means and the assignment share it
        devs = [_resident(h) for h in halves]
    if Cs is None:
        Cs = tuple(_kmeans(h, V, kmeans_coarse_iters, n_init, random_state, dev) for h, dev in zip(halves, devs))
    fitted = None
    if Rs is None:
        fitted = [local_rotations(h, C, M // 2, dev) for h, C, dev in zip(halves, Cs, devs)]
        Rs = tuple(f[0] for f in fitted)
        mus = tuple(f[1] for f in fitted)
    del devs
    if subs is not None:
        return tuple(Cs), tuple(Rs), tuple(mus), subs
    N = data.shape[0]
    n_sub = int(np.floor(min(subquantizer_sample_ratio, 1.0) * N))
    sample = np.random.RandomState(random_state).choice(N, n_sub, False)
    subs = []
    for s, (h, C) in enumerate(zip(halves, Cs)):
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
