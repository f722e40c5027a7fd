"""Evaluation of a trained model and of a searcher: counterpart of the reference's lopq/lopq/eval.py.

The six functions keep the reference's names, argument names and defaults.  What the reference does one vector at a time runs
here in batches on the GPU, and the ground truth -- scipy's ``cdist`` plus an ``argmin`` per row there -- comes from the exact
nearest-neighbour kernel of csrc/lopq_eval.hip (include/cis_hip.h:cis_exact_knn).  There is no CPU fallback.
"""
import time

import numpy as np

from .. import _lib

MAX_K = 1024  # include/cis_hip.h:cis_exact_knn


def set_exact_mode(exact_only=False):
    """Route every query of the exact nearest-neighbour search through the exact-only kernel (``exact_only=True``) instead of the
    float32 matrix-core prefilter with exact re-check.  Both return the same answer; the switch exists for the tests (in the style
    of LOPQSearcherHIP.set_scan_mode).  Process-wide."""
    _lib.check(_lib.lib().cis_exact_knn_set_mode(1 if exact_only else 0))


def exact_stats():
    """(queries, of them answered by the exact-only kernel, rows the prefilter left to re-score for the others) of the last pass of
    the last exact nearest-neighbour call (include/cis_hip.h:cis_exact_knn_stats)."""
    st = np.zeros(3, dtype=np.int64)
    _lib.check(_lib.lib().cis_exact_knn_stats(_lib.ptr(st)))
    return int(st[0]), int(st[1]), int(st[2])


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _tensor_code(t):
    import torch
    if not (t.is_cuda and t.dim() == 2 and t.dtype in (torch.float32, torch.float64)):
        raise ValueError("expected a float32/float64 [n, d] tensor on the GPU, got %s %s on %s" % (t.dtype, tuple(t.shape), t.device))
    return _lib.CIS_F32 if t.dtype == torch.float32 else _lib.CIS_F64


def exact_neighbors(data1, data2, k, chunk=None):
    """(idx, dist), each [m1, k]: for every row of data1 the k rows of data2 with the smallest (distance, index), ascending.

    dist is scipy's ``cdist`` value bit for bit (float64; equal distances order by index, so column 0 is ``np.argmin``); with
    k > m2 the tail holds -1 / NaN.  data1 and data2 are both numpy arrays (results are numpy arrays) or both torch tensors on the
    GPU (results are tensors on that device); float32 and float64 may be mixed.  data2 is streamed ``chunk`` rows at a time
    through the kernel's accumulate mode (default: 1 GiB of host data per step, everything at once for tensors)."""
    k = int(k)
    if _is_tensor(data1) != _is_tensor(data2):
        raise ValueError("data1 and data2 must both be numpy arrays or both be GPU tensors")
    L = _lib.lib()
    if _is_tensor(data1):
        import torch
        c1, c2 = _tensor_code(data1), _tensor_code(data2)
        if data1.shape[1] != data2.shape[1] or data1.device != data2.device:
            raise ValueError("data1 %r and data2 %r must have the same width and device" % (tuple(data1.shape), tuple(data2.shape)))
        data1, data2 = data1.contiguous(), data2.contiguous()
        m1, m2, d = int(data1.shape[0]), int(data2.shape[0]), int(data1.shape[1])
        idx = torch.empty((m1, max(k, 0)), dtype=torch.int64, device=data1.device)
        dist = torch.empty((m1, max(k, 0)), dtype=torch.float64, device=data1.device)
        step = m2 if not chunk else int(chunk)
        stream = torch.cuda.current_stream(data1.device).cuda_stream
        for n, a in enumerate(range(0, m2, step) if m2 else [0]):
            part = data2[a:a + step]
            _lib.check(L.cis_exact_knn_dev(part.data_ptr(), c2, int(part.shape[0]), d, data1.data_ptr(), c1, m1, k, a, int(n > 0),
                                           idx.data_ptr(), dist.data_ptr(), stream))
        return idx, dist
    data1, data2 = _lib.as_float_matrix(data1), _lib.as_float_matrix(data2)
    if data1.shape[1] != data2.shape[1]:
        raise ValueError("data1 %r and data2 %r must have the same width" % (data1.shape, data2.shape))
    m1, m2, d = data1.shape[0], data2.shape[0], data1.shape[1]
    idx = np.empty((m1, max(k, 0)), dtype=np.int64)
    dist = np.empty((m1, max(k, 0)), dtype=np.float64)
    step = int(chunk) if chunk else max(1, (1 << 30) // (d * data2.dtype.itemsize))
    for n, a in enumerate(range(0, m2, step) if m2 else [0]):
        part = data2[a:a + step]
        _lib.check(L.cis_exact_knn(_lib.ptr(part), _lib.dtype_code(part), part.shape[0], d, _lib.ptr(data1), _lib.dtype_code(data1), m1, k,
                                   a, int(n > 0), _lib.ptr(idx), _lib.ptr(dist)))
    return idx, dist


def compute_all_neighbors(data1, data2=None, just_nn=True, k=None):
    """
    For each point in data1, compute a ranked list of neighbor indices from data2.
    If data2 is not provided, compute neighbors relative to data1.  reference: lopq/lopq/eval.py:7-38.

    :param data1: an m1 x n matrix with observations on the rows (numpy array or GPU tensor)
    :param data2: an m2 x n matrix with observations on the rows
    :param int k: (this package's addition) return the k nearest neighbours, ranked, as an [m1, k] array

    :returns ndarray: int64; [m1] (the nearest neighbour: ``np.argmin`` of scipy's distances, first minimum) when just_nn and k is
        None; [m1, k] with k given; [m1, m2] (the reference's argsort) with just_nn=False, for m2 <= 1024 -- NotImplementedError above.
        Equal distances rank by index, where the reference's unstable argsort leaves the order open.
    """
    if data2 is None:
        data2 = data1
    m2 = int(data2.shape[0])
    if k is None:
        kk = 1 if just_nn else m2
        if kk > MAX_K:
            raise NotImplementedError("compute_all_neighbors(just_nn=False) ranks at most %d rows of data2 (got %d): ask for k <= %d "
                                      "neighbours instead" % (MAX_K, m2, MAX_K))
        if kk == 0:
            return np.zeros((int(data1.shape[0]),) if just_nn else (int(data1.shape[0]), 0), dtype=np.int64)
    else:
        kk = int(k)
    idx, _ = exact_neighbors(data1, data2, kk)
    if _is_tensor(idx):
        idx = idx.cpu().numpy()
    return idx[:, 0] if (k is None and just_nn) else idx


def get_proportion_nns_with_same_coarse_codes(data, model, nns=None):
    """Share of the vectors whose nearest neighbour lies in the same coarse cell.  reference: lopq/lopq/eval.py:41-63."""
    N = data.shape[0]
    if nns is None:
        nns = compute_all_neighbors(data)
    coarse = np.asarray(model.predict_coarse(np.asarray(data))).reshape(N, 2)
    same = np.all(coarse == coarse[np.asarray(nns, dtype=np.int64)], axis=1)
    return float(np.count_nonzero(same)) / N


def get_cell_histogram(data, model):
    """Number of vectors per coarse cell, with the reference's bins (lopq/lopq/eval.py:66-74): ``bins=range(V**2)`` gives V**2 - 1
    bins and the last one holds the last TWO cells.  Cell ids are c0 * V + c1 in int64: the reference run under numpy 2 overflows
    its uint8 cell ids for V > 16, which is a defect of that run and is not reproduced here."""
    coarse = np.asarray(model.predict_coarse(np.asarray(data))).reshape(-1, 2).astype(np.int64)
    cells = coarse[:, 0] * int(model.V) + coarse[:, 1]
    return np.histogram(cells, bins=range(int(model.V) ** 2))[0]


def get_proportion_of_reconstructions_with_same_codes(data, model):
    """Share of the vectors whose reconstruction encodes to the same codes.  reference: lopq/lopq/eval.py:77-89; as there, a model
    with PCA applies the PCA again to the reconstruction."""
    N = data.shape[0]
    coarse, fine = model.predict_batch(np.asarray(data))
    c = np.ascontiguousarray(coarse, dtype=np.uint16)
    f = np.ascontiguousarray(fine, dtype=np.uint8)
    recon = np.empty((N, model.dim), dtype=np.float64)
    _lib.check(_lib.lib().cis_reconstruct(model._handle(), _lib.ptr(c), _lib.ptr(f), N, _lib.ptr(recon)))
    coarse2, fine2 = model.predict_batch(recon)
    same = np.all(np.asarray(coarse) == np.asarray(coarse2), axis=1) & np.all(fine == fine2, axis=1)
    return float(np.count_nonzero(same)) / N


def _rank_hits(recall, ids, nn, thresholds):
    for j, rid in enumerate(ids):
        if rid == nn:
            for t_i, t in enumerate(thresholds):
                if j < t:
                    recall[t_i] += 1


def get_recall(searcher, queries, nns, thresholds=[1, 10, 100, 1000], normalize=True, verbose=False):
    """
    Given a searcher with indexed data and groundtruth nearest neighbors for a set of test query vectors, collect and return
    recall statistics.  reference: lopq/lopq/eval.py:92-142.

    A searcher with ``search_batch`` (LOPQSearcherHIP, LOPQSearcherLMDB) is asked once for all queries, with quota = limit =
    thresholds[-1] as ``searcher.search(d, thresholds[-1])`` means; any other searcher is asked query by query as in the reference.

    :return ndarray: recall at each threshold
    :return float: the elapsed query time (time.perf_counter)
    Both are divided by the number of queries when ``normalize`` is set.
    """
    recall = np.zeros(len(thresholds))
    query_time = 0.0
    top = thresholds[-1]
    if hasattr(searcher, "search_batch"):
        start = time.perf_counter()
        r = searcher.search_batch(np.asarray(queries), quota=top, limit=top)
        query_time += time.perf_counter() - start
        for i in range(len(queries)):
            if verbose and i % 50 == 0:
                print("%d cells visited for query %d" % (int(r["visited"][i]), i))
            _rank_hits(recall, searcher.caller_ids(r["ids"][i, :int(r["n_found"][i])]), nns[i], thresholds)
    else:
        for i, d in enumerate(queries):
            start = time.perf_counter()
            results, cells_visited = searcher.search(d, top)
            query_time += time.perf_counter() - start
            if verbose and i % 50 == 0:
                print("%d cells visited for query %d" % (cells_visited, i))
            _rank_hits(recall, [res[0] for res in results], nns[i], thresholds)
    if normalize:
        N = queries.shape[0]
        return recall / N, query_time / N
    return recall, query_time


def get_subquantizer_distortion(data, model):
    """Mean squared distance of the locally projected residuals to their nearest subquantizer centroid, one value per
    subquantizer.  reference: lopq/lopq/eval.py:145-161, which splits the projection with a hard-coded ``np.split(pall, 8, axis=1)``
    and therefore raises for M != 8; this returns the M values for any M (equal to the reference's at M = 8).
    The projection and the nearest centroids come from the model's batched GPU entry points (cis_project, cis_predict_fine), which
    compute the reference's compute_residuals + project_residuals_to_local and predict_cluster; the sums are float64."""
    X = np.asarray(data)
    coarse = model.predict_coarse(X)
    pall = np.asarray(model.project(X, coarse)).reshape(X.shape[0], -1)
    fine = np.asarray(model.predict_fine(X, coarse)).reshape(X.shape[0], -1)
    suball = list(model.subquantizers[0]) + list(model.subquantizers[1])
    out = np.empty(len(suball))
    for j, (c, p) in enumerate(zip(suball, np.split(pall, len(suball), axis=1))):
        r = p - np.asarray(c, dtype=np.float64)[fine[:, j]]
        out[j] = np.sum(np.sum(r * r, axis=1))
    return out / X.shape[0]
