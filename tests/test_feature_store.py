"""The live feature store (csrc/feat_store.hip; rerank.FeatureStore, LOPQSearcherHIP.search_by_ids_dev, BatchIngest(features=))
against the pure-Python model of its semantics (tests/featstore_model.py), byte for byte: rows, id column, counts and look-ups
after every call, through row growth, table rebuilds and tombstones; and against the static ResidentFeatures path it stands
beside, bit for bit, for the re-rank, the exact search and the live index."""
import ctypes

import numpy as np
import pytest

from conftest import has_gpu, load_golden
from featstore_model import FeatStoreModel

gpu = pytest.mark.gpu

SLOT_BASE = 1 << 62


# ---- the yardstick itself (no GPU) ----------------------------------------------------------------------------------------------
def test_model_against_hand_written_cases():
    m = FeatStoreModel(2, np.float32)
    f = lambda *v: np.array(v, dtype=np.float32).reshape(-1, 2)
    # put: negatives skipped, a repeated id takes one row and keeps its last feature, rows in order of first occurrence
    assert m.put([7, -1, 3, 7, 9], f(1, 1, 2, 2, 3, 3, 4, 4, 5, 5)) == (3, 1)
    assert m.row_ids.tolist() == [7, 3, 9] and m.feats.tolist() == [[4, 4], [3, 3], [5, 5]]
    # a stored id is overwritten in place; a new one goes behind
    assert m.put([3, 11], f(6, 6, 7, 7)) == (1, 0)
    assert m.row_ids.tolist() == [7, 3, 9, 11] and m.feats.tolist() == [[4, 4], [6, 6], [5, 5], [7, 7]]
    assert m.put([], f()) == (0, 0) and m.put([-5], f(0, 0)) == (0, 1) and len(m) == 4
    assert m.rows_of([11, 7, 8, -1]).tolist() == [3, 0, -1, -1]
    # remove the head row: n' = 3, hole 0, mover 3 (id 11); repeats, unknowns and negatives are ignored
    assert m.remove([7, 7, 100, -3]) == 1
    assert m.row_ids.tolist() == [11, 3, 9] and m.feats.tolist() == [[7, 7], [6, 6], [5, 5]] and m.row == {11: 0, 3: 1, 9: 2}
    # remove the tail row only: nothing moves
    assert m.remove([9]) == 1 and m.row_ids.tolist() == [11, 3] and m.row == {11: 0, 3: 1}
    # five rows, remove rows 0, 1 and 3: n' = 2, holes [0, 1], movers [2, 4] in that order
    m.put([20, 21, 22], f(1, 0, 2, 0, 3, 0))
    assert m.row_ids.tolist() == [11, 3, 20, 21, 22]
    assert m.remove([21, 3, 11]) == 3
    assert m.row_ids.tolist() == [20, 22] and m.feats.tolist() == [[1, 0], [3, 0]] and m.row == {20: 0, 22: 1}
    g, r = m.get([22, 5, -1, 20])
    assert r.tolist() == [1, -1, -1, 0] and g.tolist() == [[3, 0], [0, 0], [0, 0], [1, 0]]
    # everything leaves, and the store takes rows again from 0
    assert m.remove([20, 22]) == 2 and len(m) == 0 and m.feats.shape == (0, 2)
    assert m.remove([20]) == 0 and m.remove([]) == 0
    assert m.put([22], f(9, 9)) == (1, 0) and m.row == {22: 0}


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _torch_dtype(dtype):
    import torch
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _id_pool(n_small=900, n_slot=700, n_low20=600):
    """Small integers, 2^62 + slot, and values that agree in their low 20 bits."""
    return np.concatenate([np.arange(n_small, dtype=np.int64), SLOT_BASE + np.arange(n_slot, dtype=np.int64),
                           (np.arange(1, n_low20 + 1, dtype=np.int64) << 20) | 5])


def _draw(rs, pool, n, negatives=True):
    ids = pool[rs.randint(0, pool.size, n)].copy()
    if negatives and n:
        neg = rs.rand(n) < 0.04
        ids[neg] = -1 - rs.randint(0, 1 << 40, int(neg.sum()))
    return ids


def _same_as_model(store, model, probe):
    import torch
    n = len(store)
    assert n == len(model)
    feats, ids = store.rows_dev()
    assert tuple(feats.shape) == (n, model.D) and tuple(ids.shape) == (n,)
    assert np.array_equal(ids.cpu().numpy(), model.row_ids)
    assert np.array_equal(_bits(feats.cpu().numpy()), _bits(model.feats))
    got = store.rows_of_dev(_dev(probe.reshape(1, -1))).cpu().numpy()[0]
    assert np.array_equal(got, model.rows_of(probe))
    cap = store.table_capacity()
    assert cap > 0 and (cap & (cap - 1)) == 0 and cap >= 2 * n


def _put_both(store, model, ids, feats):
    got = store.put_dev(_dev(ids), _dev(feats))
    assert got == model.put(ids, feats), (got, ids.shape)


def _remove_both(store, model, ids):
    got = store.remove_dev(_dev(ids))
    assert got == model.remove(ids), (got, ids.shape)


def _run_sequence(store, model, rs, pool, ops, probe=None, check=True):
    for op, n in ops:
        if op == "put":
            _put_both(store, model, _draw(rs, pool, n), rs.standard_normal((n, model.D)).astype(model.dtype))
        else:
            _remove_both(store, model, _draw(rs, pool, n))
        if check:
            _same_as_model(store, model, probe)


# every batch size of {0, 1, 63, 64, 65, 256, 257, 1025} as a put and as a removal; small batches first, so that the rows and the
# table of a store that starts empty grow in several steps
OPS = [("put", 1), ("put", 63), ("remove", 1), ("put", 64), ("put", 65), ("remove", 63), ("put", 256), ("remove", 64), ("put", 257),
       ("put", 0), ("remove", 0), ("put", 1025), ("remove", 257), ("remove", 65), ("put", 1025), ("remove", 1025), ("put", 256),
       ("remove", 256), ("put", 257), ("put", 1025)]


# ---- 1. model parity ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 257, 4096])
def test_random_sequences_equal_the_model_byte_for_byte(D, dtype):
    """Seeded put / remove sequences from an empty store with reserve = 0: after every call the row count, the rows' bytes, the id
    column, the returned counts and the look-up of every id ever used (and of negatives) equal the model's."""
    from columbiaimagesearch_amd.rerank import FeatureStore
    rs = np.random.RandomState(D * 2 + np.dtype(dtype).itemsize)
    pool = _id_pool()
    probe = np.concatenate([pool, np.array([-1, -2, -(1 << 62), np.iinfo(np.int64).min, 1 << 61], dtype=np.int64)])
    store, model = FeatureStore(D, _torch_dtype(dtype)), FeatStoreModel(D, dtype)
    caps, sizes = set(), []
    try:
        _same_as_model(store, model, probe)
        for op in OPS:
            _run_sequence(store, model, rs, pool, [op], probe)
            caps.add(store.table_capacity())
            sizes.append(len(store))
        assert len(caps) >= 3 and max(sizes) > 1200  # the table was rebuilt at several sizes, the rows grew more than once
    finally:
        store.close()


# ---- 2. batch contents at the edges ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_batch_contents_at_the_edges(dtype):
    from columbiaimagesearch_amd.rerank import FeatureStore
    D = 33
    rs = np.random.RandomState(5)
    store, model = FeatureStore(D, _torch_dtype(dtype)), FeatStoreModel(D, dtype)
    F = lambda n: rs.standard_normal((n, D)).astype(dtype)
    probe = np.concatenate([np.arange(0, 700, dtype=np.int64), SLOT_BASE + np.arange(8, dtype=np.int64), np.array([-1, -7], dtype=np.int64)])
    try:
        # one id 257 times: one row, the last feature
        f = F(257)
        _put_both(store, model, np.full(257, SLOT_BASE + 3, dtype=np.int64), f)
        _same_as_model(store, model, probe)
        assert len(store) == 1 and np.array_equal(_bits(store.rows_dev()[0].cpu().numpy()[0]), _bits(f[256]))
        # negatives only
        assert store.put_dev(_dev(np.array([-1, -2, -3], dtype=np.int64)), _dev(F(3))) == (0, 3)
        assert model.put([-1, -2, -3], F(3)) == (0, 3)
        _same_as_model(store, model, probe)
        # 600 new rows, then a batch of stored ids only: n unchanged, bytes replaced
        _put_both(store, model, np.arange(600, dtype=np.int64), F(600))
        before = len(store)
        ids = rs.permutation(600)[:300].astype(np.int64)
        assert store.put_dev(_dev(ids), _dev(f[:1].repeat(300, 0))) == (0, 0)
        model.put(ids, f[:1].repeat(300, 0))
        assert len(store) == before
        _same_as_model(store, model, probe)
        # a removal list with repeats, unknowns and negatives
        _remove_both(store, model, np.array([5, 5, 5, 100000, -1, 7, SLOT_BASE + 9, -9, 7], dtype=np.int64))
        _same_as_model(store, model, probe)
        # only tail rows (nothing moves), only head rows (every hole is filled), more than half
        tail = model.row_ids[-40:].copy()
        _remove_both(store, model, tail)
        _same_as_model(store, model, probe)
        head = model.row_ids[:50].copy()
        _remove_both(store, model, head)
        _same_as_model(store, model, probe)
        most = model.row_ids[rs.permutation(len(model))[:(len(model) * 3) // 4]].copy()
        _remove_both(store, model, most)
        _same_as_model(store, model, probe)
        # everything, then put again
        _remove_both(store, model, model.row_ids.copy())
        assert len(store) == 0
        _same_as_model(store, model, probe)
        _remove_both(store, model, np.arange(10, dtype=np.int64))  # an empty store
        _put_both(store, model, np.array([3, SLOT_BASE + 1, 3, 650], dtype=np.int64), F(4))
        _same_as_model(store, model, probe)
        # get_dev: stored, unknown and negative ids
        ask = np.array([650, 4, -1, 3, SLOT_BASE + 1, SLOT_BASE + 2], dtype=np.int64)
        g, r = store.get_dev(_dev(ask))
        mg, mr = model.get(ask)
        assert np.array_equal(r.cpu().numpy(), mr) and np.array_equal(_bits(g.cpu().numpy()), _bits(mg))
        # the host-array conveniences
        assert store.put(np.array([900, 901]), np.ones((2, D))) == model.put([900, 901], np.ones((2, D)))
        assert store.remove([900, 3]) == model.remove([900, 3])
        _same_as_model(store, model, probe)
        with pytest.raises(ValueError):
            store.put_dev(_dev(ask), _dev(F(5)))
        with pytest.raises(ValueError):
            store.put_dev(_dev(ask[:2]), _dev(F(2).astype(np.float64 if dtype == np.float32 else np.float32)))
    finally:
        store.close()


# ---- 3. tombstones --------------------------------------------------------------------------------------------------------------
@gpu
def test_tombstones_are_cleared_by_the_rebuild():
    """100 rows; the same 64 ids leave and come back 40 times: 2560 tombstones without a rebuild, more than a table sized for 164
    rows holds.  Every call returns, look-ups stay right, and the capacity stays within 8 x the next power of two above n (the
    rebuild rule: the next power of two >= 4 (n + batch))."""
    from columbiaimagesearch_amd.rerank import FeatureStore
    D = 8
    rs = np.random.RandomState(11)
    store, model = FeatureStore(D, _torch_dtype(np.float32)), FeatStoreModel(D, np.float32)
    ids = (np.arange(100, dtype=np.int64) << 20) | 5
    probe = np.concatenate([ids, ids + 1, np.array([-1], dtype=np.int64)])
    try:
        _put_both(store, model, ids, rs.standard_normal((100, D)).astype(np.float32))
        churn = ids[18:82]
        for it in range(40):
            _remove_both(store, model, churn)
            assert len(store) == 36
            _put_both(store, model, churn, rs.standard_normal((64, D)).astype(np.float32))
            assert len(store) == 100 and store.table_capacity() <= 8 * 128
            if it % 8 == 7:
                _same_as_model(store, model, probe)
        _same_as_model(store, model, probe)
    finally:
        store.close()


# ---- 4. re-rank equivalence -----------------------------------------------------------------------------------------------------
def _churned_store(D, dtype, seed):
    """A store after a put / remove sequence, its model, and the ids the sequence drew from."""
    from columbiaimagesearch_amd.rerank import FeatureStore
    rs = np.random.RandomState(seed)
    pool = _id_pool(300, 200, 100)
    store, model = FeatureStore(D, _torch_dtype(dtype)), FeatStoreModel(D, dtype)
    _run_sequence(store, model, rs, pool, [("put", 257), ("remove", 65), ("put", 256), ("remove", 257), ("put", 64), ("remove", 63)], check=False)
    _same_as_model(store, model, pool)
    return store, model, pool, rs


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_rerank_through_the_store_equals_resident_features(dtype):
    """store.rerank_dev == ResidentFeatures(tensor built from the model, ids = the model's).rerank_dev bit for bit, and == the host
    rerank in test_rerank_dev.py's terms; the lists name stored ids, removed ids and ids never seen (they keep their ADC distance),
    with and without max_returned and near_dup_th."""
    import torch
    from columbiaimagesearch_amd.rerank import ResidentFeatures
    from test_rerank_dev import _assert_same, _gap_threshold, _np
    D, nq, L, nb = 96, 7, 70, 64
    store, model, pool, rs = _churned_store(D, dtype, 21)
    try:
        removed = np.array([k for k in pool if int(k) not in model.row], dtype=np.int64)
        assert removed.size > 50 and len(model) > 100
        rf = ResidentFeatures(_dev(model.feats).contiguous(), ids=model.row_ids.tolist())
        ids = np.where(rs.rand(nq, L) < 0.7, model.row_ids[rs.randint(0, len(model), (nq, L))], removed[rs.randint(0, removed.size, (nq, L))])
        ids[1, 50:] = -1
        ids[3, :] = -1
        adc = np.sort(rs.rand(nq, L), axis=1)
        adc[ids < 0] = np.nan
        Q = (model.feats[rs.randint(0, len(model), nq)] + 0.05 * rs.standard_normal((nq, D))).astype(dtype)
        q_t, ids_t, adc_t = _dev(Q).contiguous(), _dev(ids), _dev(adc)
        assert np.array_equal(store.rows_of_dev(ids_t).cpu().numpy(), rf.rows_of_dev(ids_t).cpu().numpy())
        plain = rf.rerank(q_t, ids, adc, rerank_nb=nb)
        t = _gap_threshold([d for _, hd in plain for d in hd])
        for kw in ({}, {"max_returned": 8}, {"near_dup_th": t}, {"max_returned": 8, "near_dup_th": t}):
            a, b = _np(store.rerank_dev(q_t, ids_t, adc_t, rerank_nb=nb, **kw)), _np(rf.rerank_dev(q_t, ids_t, adc_t, rerank_nb=nb, **kw))
            for k in ("ids", "src", "n_kept"):
                assert np.array_equal(a[k], b[k]), (k, kw)
            assert np.array_equal(a["dists"].view(np.int64), b["dists"].view(np.int64)), kw
            _assert_same(a, rf.rerank(q_t, ids, adc, rerank_nb=nb, **kw), ids, nb)
        # a removed id in a kept place keeps its ADC distance
        a = _np(store.rerank_dev(q_t, ids_t, adc_t, rerank_nb=nb))
        hit = np.argwhere((ids[:, :nb] >= 0) & (model.rows_of(ids[:, :nb]).reshape(nq, nb) < 0))
        assert hit.shape[0] > 0
        for qi, i in hit[:20]:
            p = int(np.where(a["src"][qi] == i)[0][0])
            assert a["ids"][qi, p] == ids[qi, i] and a["dists"][qi, p] == adc[qi, i]
    finally:
        store.close()


# ---- 5. search_exact ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_search_exact_equals_resident_features_in_the_stores_row_order(dtype):
    from columbiaimagesearch_amd.rerank import ResidentFeatures
    D, nq, k = 24, 9, 30
    store, model, pool, rs = _churned_store(D, dtype, 33)
    try:
        Q = rs.standard_normal((nq, D)).astype(dtype)
        # no two distances of a query tie (they would rank by row, which is the thing that may differ): checked here, in float64
        d = np.sqrt(((Q[:, None, :].astype(np.float64) - model.feats[None, :, :].astype(np.float64)) ** 2).sum(-1))
        assert (np.diff(np.sort(d, axis=1), axis=1) > 1e-6).all()
        rf = ResidentFeatures(_dev(model.feats).contiguous(), ids=model.row_ids.tolist())
        q_t = _dev(Q).contiguous()
        ids_a, d_a = store.search_exact(q_t, k)
        ids_b, d_b = rf.search_exact(q_t, k)
        assert ids_a.shape == (nq, k) and np.array_equal(ids_a, ids_b) and np.array_equal(d_a.view(np.int64), d_b.view(np.int64))
        assert np.array_equal(ids_a[:, 0], model.row_ids[np.argmin(d, axis=1)])
        # more asked for than stored: -1 / NaN behind the rows
        small = model.row_ids[5:].copy()
        _remove_both(store, model, small)
        ids_c, d_c = store.search_exact(q_t, 8)
        assert (ids_c[:, 5:] == -1).all() and np.isnan(d_c[:, 5:]).all() and (np.sort(ids_c[:, :5], axis=1) == np.sort(model.row_ids)).all()
    finally:
        store.close()


# ---- 6. / 7. the live index -----------------------------------------------------------------------------------------------------
def _tiny_codes(z, sel):
    import torch
    return (torch.as_tensor(np.ascontiguousarray(z["coarse"][sel]).view(np.int16)).cuda(),
            torch.as_tensor(np.ascontiguousarray(z["fine"][sel])).cuda())


def _same_answer(a, b):
    from test_rerank_dev import _np
    a, b = _np(a), _np(b)
    for k in ("ids", "src", "n_kept", "visited"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["dists"].view(np.int64), b["dists"].view(np.int64))
    return a


@gpu
def test_live_index_with_a_store_equals_static_builds():
    """The golden `tiny` model: codes through add_codes_dev and features through put_dev in three batches; the answers equal those
    with a static ResidentFeatures of everything; after a third of the ids left both, they equal a searcher and a ResidentFeatures
    built without them; a removed id put back with a new feature is found again."""
    import torch
    from test_lopq_hip_parity import hip_model
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.rerank import FeatureStore, ResidentFeatures
    z, X, Q = load_golden("tiny")
    n = 1500
    X = np.ascontiguousarray(X[:n])
    q_t = _dev(Q).contiguous()
    kw = dict(quota=400, limit=200, rerank_nb=200)
    s, s2 = LOPQSearcherHIP(hip_model(z)), LOPQSearcherHIP(hip_model(z))
    store = FeatureStore(X.shape[1], torch.float64)
    try:
        for a, b in ((0, 500), (500, 1000), (1000, 1500)):
            sel = np.arange(a, b)
            c, f = _tiny_codes(z, sel)
            ids = _dev(sel.astype(np.int64))
            assert s.add_codes_dev(c, f, ids) == (b - a, 0)
            assert store.put_dev(ids, _dev(X[sel])) == (b - a, 0)
        rf = ResidentFeatures(_dev(X).contiguous())
        for k2 in ({}, {"max_returned": 20}):
            got = _same_answer(s.search_rerank_dev(q_t, store, **kw, **k2), s.search_rerank_dev(q_t, rf, **kw, **k2))
        assert int(got["n_kept"].min()) > 0
        # a third leaves the index and the store
        gone = np.arange(1, n, 3).astype(np.int64)
        kept = np.setdiff1d(np.arange(n), gone)
        assert s.remove_ids_dev(_dev(gone)) == gone.size and store.remove_dev(_dev(gone)) == gone.size
        s2.add_codes_array(z["coarse"][kept], z["fine"][kept], kept.tolist())
        rf2 = ResidentFeatures(_dev(X[kept]).contiguous(), ids=kept.tolist())
        got = _same_answer(s.search_rerank_dev(q_t, store, **kw), s2.search_rerank_dev(q_t, rf2, **kw))
        assert not np.isin(got["ids"], gone).any() and int(got["n_kept"].min()) > 0
        assert (store.rows_of_dev(_dev(gone)).cpu().numpy() == -1).all()
        # one of them comes back, with a new feature
        back = int(gone[7])
        new_f = (0.5 * X[back] + 0.01).reshape(1, -1)
        c, f = _tiny_codes(z, np.array([back]))
        assert s.add_codes_dev(c, f, _dev(np.array([back], dtype=np.int64))) == (1, 0)
        assert store.put_dev(_dev(np.array([back], dtype=np.int64)), _dev(new_f)) == (1, 0)
        s2.add_codes_array(z["coarse"][[back]], z["fine"][[back]], [back])
        rf3 = ResidentFeatures(_dev(np.concatenate([X[kept], new_f])).contiguous(), ids=kept.tolist() + [back])
        qb = _dev(np.concatenate([X[back:back + 1], Q[:3]])).contiguous()
        got = _same_answer(s.search_rerank_dev(qb, store, **kw), s2.search_rerank_dev(qb, rf3, **kw))
        where = np.where(got["ids"][0] == back)[0]
        assert where.size == 1
        assert got["dists"][0, where[0]] == float(np.linalg.norm(X[back] - new_f[0])) or \
            abs(got["dists"][0, where[0]] - np.linalg.norm(X[back] - new_f[0])) < 1e-12
        g, r = store.get_dev(_dev(np.array([back], dtype=np.int64)))
        assert int(r[0]) == len(store) - 1 and np.array_equal(_bits(g.cpu().numpy()), _bits(new_f))
    finally:
        store.close()
        s.close()
        s2.close()


@gpu
def test_search_by_ids_equals_search_on_the_gathered_rows():
    import torch
    from test_lopq_hip_parity import hip_model
    from test_rerank_dev import _np
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.rerank import FeatureStore
    z, X, Q = load_golden("tiny")
    n = 1000
    s = LOPQSearcherHIP(hip_model(z))
    store = FeatureStore(X.shape[1], torch.float64)
    try:
        sel = np.arange(n)
        c, f = _tiny_codes(z, sel)
        s.add_codes_dev(c, f, _dev(sel.astype(np.int64)))
        store.put_dev(_dev(sel.astype(np.int64)), _dev(X[:n]))
        gone = np.array([17, 400], dtype=np.int64)
        s.remove_ids_dev(_dev(gone))
        store.remove_dev(_dev(gone))
        ask = np.array([3, 17, 999, 123456789, 500, -1, 400, 0], dtype=np.int64)
        want_found = np.array([True, False, True, False, True, False, False, True])
        kw = dict(quota=300, limit=50, rerank_nb=40, max_returned=30)
        out = _np(s.search_by_ids_dev(_dev(ask), store, **kw))
        q, rows = store.get_dev(_dev(ask))
        ref = _np(s.search_rerank_dev(q, store, **kw))
        assert np.array_equal(out["found"], want_found) and np.array_equal(rows.cpu().numpy() >= 0, want_found)
        for k in ("ids", "src", "n_kept", "visited"):
            assert np.array_equal(out[k][want_found], ref[k][want_found]), k
        assert np.array_equal(out["dists"][want_found].view(np.int64), ref["dists"][want_found].view(np.int64))
        assert (out["n_kept"][want_found] > 0).all()
        miss = ~want_found
        assert (out["ids"][miss] == -1).all() and np.isnan(out["dists"][miss]).all() and (out["n_kept"][miss] == 0).all()
        assert (out["src"][miss] == -1).all()
    finally:
        store.close()
        s.close()


# ---- 8. BatchIngest(features=) --------------------------------------------------------------------------------------------------
class _StubNet(object):
    """forward_dev returns the rows it is given (a copy: the ingest normalises in place)."""

    def forward_dev(self, x):
        return x.clone()

    def view(self):
        return _StubNet()

    def close(self):
        pass


@gpu
@pytest.mark.parametrize("string_ids", [False, True], ids=["tensor_ids", "string_ids"])
def test_batch_ingest_puts_the_normalised_descriptors(string_ids):
    """ingest_batches with three lanes: afterwards the store equals the model fed batch by batch with the normalised rows under
    the inserted ids (ids repeat across batches: the last feature stays), and remove_ids_dev takes them out of both."""
    import torch
    from test_lopq_hip_parity import hip_model
    from columbiaimagesearch_amd.ingest import BatchIngest, l2_normalize_dev
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.rerank import FeatureStore
    z, X, Q = load_golden("tiny")
    D = X.shape[1]
    m = hip_model(z)
    s = LOPQSearcherHIP(m)
    store, model = FeatureStore(D, torch.float64), FeatStoreModel(D, np.float64)
    ing = BatchIngest(_StubNet(), m, s, features=store)
    try:
        spans = [(0, 100), (100, 157), (157, 257), (257, 258), (258, 400)]
        num = [np.arange(a, b) for a, b in spans]
        num[2][:30] = np.arange(20, 50)  # ids of the first batch again, with other features
        batches = [_dev(X[a:b] * 3.0).contiguous() for a, b in spans]
        names = [["%040x_0" % (int(i) * 2654435761 % (1 << 61)) for i in b] for b in num]
        ids = names if string_ids else [_dev(b.astype(np.int64)) for b in num]
        ing.ingest_batches(batches, ids=ids, lanes=3)
        for b, x in zip(names if string_ids else num, batches):
            dev_ids = s.device_ids_of(b) if string_ids else np.asarray(b, dtype=np.int64)
            assert (dev_ids >= 0).all()
            model.put(dev_ids, l2_normalize_dev(x.clone()).cpu().numpy())
        probe = np.concatenate([np.arange(450, dtype=np.int64), SLOT_BASE + np.arange(450, dtype=np.int64)])
        _same_as_model(store, model, probe)
        assert len(store) == 370 and (SLOT_BASE <= model.row_ids).all() == string_ids
        # one more batch through ingest_batch, integer ids as a host array / a list of names
        extra = np.arange(1000, 1040)
        x = _dev(X[1000:1040]).contiguous()
        ing.ingest_batch(x, ["n%d" % i for i in extra] if string_ids else extra)
        dev_ids = s.device_ids_of(["n%d" % i for i in extra]) if string_ids else extra.astype(np.int64)
        model.put(dev_ids, l2_normalize_dev(x.clone()).cpu().numpy())
        _same_as_model(store, model, probe)
        # removal from both
        gone = model.row_ids[::3].copy()
        before = s.get_nb_indexed()
        removed = ing.remove_ids_dev(_dev(gone))
        model.remove(gone)
        assert removed > 0 and s.get_nb_indexed() == before - removed
        _same_as_model(store, model, probe)
    finally:
        ing.close()
        store.close()
        s.close()


@gpu
def test_batch_ingest_refuses_a_store_of_another_dtype_before_it_inserts():
    import torch
    from test_lopq_hip_parity import hip_model
    from columbiaimagesearch_amd.ingest import BatchIngest
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.rerank import FeatureStore
    z, X, Q = load_golden("tiny")
    m = hip_model(z)
    s = LOPQSearcherHIP(m)
    x = _dev(X[:50]).contiguous()
    for store in (FeatureStore(X.shape[1], torch.float32), FeatureStore(X.shape[1] + 1, torch.float64)):
        ing = BatchIngest(_StubNet(), m, s, features=store)
        try:
            with pytest.raises(ValueError, match="feature store"):
                ing.ingest_batch(x, np.arange(50))
            with pytest.raises(ValueError, match="feature store"):
                ing.ingest_batches([x], ids=[np.arange(50)], lanes=3)
            assert s.get_nb_indexed() == 0 and len(store) == 0
        finally:
            ing.close()
            store.close()
    # without a store nothing changes
    ing = BatchIngest(_StubNet(), m, s)
    assert ing.ingest_batch(x, np.arange(50)) == 50 and s.get_nb_indexed() == 50
    ing.close()
    s.close()


@gpu
def test_reserve_means_no_allocation_afterwards():
    """After reserve(rows) and one call of each kind at the batch size, puts and removals up to `rows` allocate nothing
    (cis_alloc_stats), tombstone rebuilds included."""
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.rerank import FeatureStore
    D, B = 64, 256
    store = FeatureStore(D, torch.float32, reserve=2048)
    try:
        f = torch.zeros((B, D), dtype=torch.float32, device="cuda")
        ids = torch.arange(B, dtype=torch.int64, device="cuda")
        store.put_dev(ids, f)
        store.remove_dev(ids)
        store.get_dev(ids)
        a0 = _lib.alloc_stats()
        cap = store.table_capacity()
        for it in range(40):  # 10240 tombstones in all: more than the table has slots
            store.put_dev(ids + (it % 7) * B, f)
            store.remove_dev(ids + (it % 7) * B)
        for it in range(8):
            store.put_dev(ids + it * B, f)
        assert len(store) == 2048 and _lib.alloc_stats() == a0 and store.table_capacity() == cap
    finally:
        store.close()


# ---- 9. without a GPU -----------------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    from columbiaimagesearch_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced
    h = ctypes.c_void_p()
    n64 = ctypes.c_int64(0)
    for D, dt in ((0, _lib.CIS_F32), (-3, _lib.CIS_F64), (8, 2), (8, 0), (8, 16)):
        assert L.cis_featstore_create(ctypes.byref(h), D, dt, 0) == _lib.CIS_EINVAL and h.value is None
    assert L.cis_featstore_create(None, 8, _lib.CIS_F32, 0) == _lib.CIS_EINVAL
    assert L.cis_featstore_create(ctypes.byref(h), 8, _lib.CIS_F32, -1) == _lib.CIS_EINVAL
    with pytest.raises(ValueError):
        _lib.check(_lib.CIS_EINVAL)
    assert L.cis_featstore_put_dev(p, p, p, -1, ctypes.byref(n64), ctypes.byref(n64), None) == _lib.CIS_EINVAL
    assert L.cis_featstore_put_dev(p, None, p, 4, ctypes.byref(n64), ctypes.byref(n64), None) == _lib.CIS_EINVAL
    assert L.cis_featstore_put_dev(p, p, None, 4, ctypes.byref(n64), ctypes.byref(n64), None) == _lib.CIS_EINVAL
    assert L.cis_featstore_put_dev(None, p, p, 4, ctypes.byref(n64), ctypes.byref(n64), None) == _lib.CIS_EINVAL
    assert L.cis_featstore_remove_dev(p, p, -1, ctypes.byref(n64), None) == _lib.CIS_EINVAL
    assert L.cis_featstore_remove_dev(p, None, 3, ctypes.byref(n64), None) == _lib.CIS_EINVAL
    assert L.cis_featstore_remove_dev(None, p, 3, ctypes.byref(n64), None) == _lib.CIS_EINVAL
    assert L.cis_featstore_get_dev(p, p, -1, p, None, None) == _lib.CIS_EINVAL
    assert L.cis_featstore_get_dev(p, None, 2, p, None, None) == _lib.CIS_EINVAL
    assert L.cis_featstore_get_dev(p, p, 2, None, None, None) == _lib.CIS_EINVAL
    assert L.cis_featstore_get_dev(None, p, 2, p, None, None) == _lib.CIS_EINVAL
    assert L.cis_featstore_reserve(None, 10, None) == _lib.CIS_EINVAL
    assert L.cis_featstore_rows_dev(None, 0, 0, None, None, None) == _lib.CIS_EINVAL
    assert L.cis_featstore_view(None, None, None, None, None, None, None) == _lib.CIS_EINVAL
    assert L.cis_featstore_size(None) == -1
    L.cis_featstore_destroy(None)  # a no-op
    # nothing to do is not an error (put and get return before they look at the handle)
    assert L.cis_featstore_put_dev(p, None, None, 0, ctypes.byref(n64), ctypes.byref(n64), None) == _lib.CIS_OK
    assert L.cis_featstore_get_dev(p, None, 0, None, None, None) == _lib.CIS_OK


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.rerank import FeatureStore
    with pytest.raises(_lib.HipError):
        FeatureStore(8, torch.float32)
    assert "no CPU fallback" in _lib.last_error() or "HIP" in _lib.last_error()
    with pytest.raises(ValueError):
        FeatureStore(8, torch.float16)
