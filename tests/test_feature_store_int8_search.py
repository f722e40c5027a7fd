"""search_exact on int8 feature rows (rerank.FeatureStore(storage=torch.int8); csrc/knn_int8.hip, the prefilter on the int8 matrix cores,
and the exact chain of csrc/lopq_eval.hip read through its int8 row view) against numpy: scipy's sequential float64 chain on the rows
as rows_dev dequantises them (that quantisation is pinned bit for bit by test_feature_store_int8.py), ranked by (distance, row)."""
import numpy as np
import pytest

gpu = pytest.mark.gpu
NQ = 70  # one full query tile of 64 and a partial one


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _store(m2, d):
    """(store, queries): random rows, and what the ranking can trip over."""
    import torch
    from columbiaimagesearch_amd.rerank import FeatureStore
    rs = np.random.RandomState(m2 + d)
    x = rs.randn(m2, d).astype(np.float32)
    x[[7, 50, 90]] = x[3]      # copies of one row: the tie is broken by row
    x[20] = 0.0                # a zero row: zero scale
    x[30, d // 2] = np.nan     # a NaN scale: distance NaN, behind every number
    x[60:68] = x[40][None] * (np.float32(1) + np.arange(8, dtype=np.float32)[:, None] * np.float32(2.0 ** -23))  # same codes, scales an ulp apart
    q = rs.randn(NQ, d).astype(np.float32)
    q[1] = x[3]
    q[2] = x[40] + np.float32(1e-3) * rs.randn(d).astype(np.float32)
    q[3] = 0.0
    store = FeatureStore(d, torch.float32, storage=torch.int8)
    assert store.put_dev(_dev(1000 + np.arange(m2, dtype=np.int64)), _dev(x)) == (m2, 0)
    return store, q


def _reference(store, q, k):
    """(ids, dists) [nq, k]: the chain s += t * t in float64, sqrt, np.lexsort((row, dist)); -1 / NaN past the last row."""
    rows, ids = store.rows_dev()
    y, ids, x = rows.cpu().numpy().astype(np.float64), ids.cpu().numpy(), q.astype(np.float64)
    s = np.zeros((x.shape[0], y.shape[0]))
    for i in range(y.shape[1]):  # sequential, every operation rounded on its own
        t = x[:, i, None] - y[None, :, i]
        s = s + t * t
    dist = np.sqrt(s)
    order = np.stack([np.lexsort((np.arange(y.shape[0]), dist[i]))[:k] for i in range(x.shape[0])])
    want_i, want_d = np.full((x.shape[0], k), -1, np.int64), np.full((x.shape[0], k), np.nan)
    want_i[:, :order.shape[1]], want_d[:, :order.shape[1]] = ids[order], np.take_along_axis(dist, order, axis=1)
    return want_i, want_d


def _assert_same(got, want):
    assert np.array_equal(got[0], want[0])
    assert (np.isnan(got[1]) == np.isnan(want[1])).all()
    assert np.array_equal(np.nan_to_num(got[1]).view(np.int64), np.nan_to_num(want[1]).view(np.int64))


@gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("m2", [100, 300])   # below two tiles: the exact-only path; three tiles, the last with 44 rows: the prefilter
@pytest.mark.parametrize("d", [16, 48, 144])  # one word, half a K step; an odd word count; several steps, one partial
def test_search_exact_on_int8_rows_is_the_float64_chain_on_the_dequantised_rows(d, m2, k, mode):
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.lopq.eval import exact_stats
    store, q = _store(m2, d)
    _lib.check(_lib.lib().cis_exact_knn_set_mode(mode))
    try:
        _assert_same(store.search_exact(_dev(q), k), _reference(store, q, k))
        if mode == 0 and m2 == 300:  # the matrix-core path answered, and dropped most of the rows
            n, flagged, cands = exact_stats()
            assert (n, flagged) == (NQ, 0) and 0 < cands < NQ * m2 // 2
    finally:
        _lib.check(_lib.lib().cis_exact_knn_set_mode(0))
        store.close()


@gpu
def test_float64_queries():
    store, q = _store(300, 48)
    try:
        q = q.astype(np.float64) * (1 + 2.0 ** -40)  # (not float32 values)
        _assert_same(store.search_exact(_dev(q), 10), _reference(store, q, 10))
    finally:
        store.close()


@gpu
def test_ids_go_through_the_id_column_after_a_removal_and_k_past_the_rows_pads():
    store, q = _store(300, 48)
    try:
        assert store.remove_dev(_dev(1000 + np.arange(100, 125, dtype=np.int64))) == 25  # tail rows move into the holes
        assert store.row_ids().cpu().numpy()[100:125].min() >= 1275
        _assert_same(store.search_exact(_dev(q), 10), _reference(store, q, 10))
        assert store.remove_dev(_dev(1000 + np.setdiff1d(np.arange(300), [3, 20, 30, 40, 50, 61]).astype(np.int64))) == 269
        ids, dist = got = store.search_exact(_dev(q), 10)
        _assert_same(got, _reference(store, q, 10))
        assert (ids[:, 5] == 1030).all() and np.isnan(dist[:, 5:]).all() and (ids[:, 6:] == -1).all()  # the NaN row, then the padding
    finally:
        store.close()


def test_argument_errors_need_no_device():
    from columbiaimagesearch_amd import _lib
    L, E, p = _lib.lib(), _lib.CIS_EINVAL, 4096  # (a pointer that is never followed)
    knn = lambda m1=1, k=1, d=16, rows=p, idx=p: L.cis_exact_knn_int8_dev(rows, 5, d, p, 4, m1, k, 0, 0, idx, p, None)
    assert [knn(d=24), knn(d=0), knn(d=65552), knn(rows=p + 8), knn(k=0), knn(rows=None), knn(idx=None)] == [E] * 7
    assert knn(k=1025) == _lib.CIS_EUNSUPPORTED and knn(m1=0) == _lib.CIS_OK
