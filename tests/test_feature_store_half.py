"""float16 feature rows behind a float32 interface (rerank.FeatureStore(storage=torch.float16); csrc/feat_half.hip): the conversion in
and out against numpy's astype, the re-rank kernels against exact integer arithmetic on lattice inputs and against a float64 norm
within the bound of the kernel's arithmetic contract, the exact k-NN against scipy's chain on the widened data, and the searcher
with a half store against the same searcher with a float32 store of the rounded rows."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import load_golden

gpu = pytest.mark.gpu
NAN_BITS = np.array(np.nan).view(np.int64)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _half_store(rows, ids):
    import torch
    from columbiaimagesearch_amd.rerank import FeatureStore
    store = FeatureStore(rows.shape[1], torch.float32, storage=torch.float16)
    assert store.put_dev(_dev(np.asarray(ids, dtype=np.int64)), _dev(rows.astype(np.float32))) == (len(ids), 0)
    return store


def _same_f32(got, want):
    return bool((((got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want)))).all())


# ---- 1. conversion ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D", [8, 520])
def test_put_rounds_like_numpy_and_get_widens(D):
    rs = np.random.RandomState(D)
    n = 40
    x = rs.randn(n, D).astype(np.float32)
    # ties between two halves (both parities), half subnormals and below, the largest half and beyond, zeros, NaN
    special = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, 2.0 ** -26, 1.5 * 2.0 ** -25,
                        5e-6, -5e-6, 6e-5, 65504, -65504, 65519.99, 65520, 1e6, -1e6, 0.0, -0.0, np.nan, np.inf], dtype=np.float32)
    x.flat[:special.size] = special
    x[-1, -8:] = special[3:11]
    with np.errstate(over="ignore"):
        widened = lambda a: a.astype(np.float16).astype(np.float32)
        want = widened(x)
        ids = 100 + np.arange(n, dtype=np.int64)
        store = _half_store(x, ids)
        try:
            ask = np.concatenate([ids[::-1], [7, -1]])
            g, r = store.get_dev(_dev(ask))
            assert r.cpu().numpy().tolist() == list(range(n - 1, -1, -1)) + [-1, -1]
            assert _same_f32(g.cpu().numpy(), np.concatenate([want[::-1], np.zeros((2, D), np.float32)]))
            assert _same_f32(store.rows_dev()[0].cpu().numpy(), want)
            x2 = (3 * rs.randn(5, D)).astype(np.float32)
            assert store.put_dev(_dev(ids[5:10]), _dev(x2)) == (0, 0)
            want[5:10] = widened(x2)
            assert store.remove_dev(_dev(ids[:7])) == 7  # head rows leave: tail rows move into the holes
            f, rid = store.rows_dev()
            rid = rid.cpu().numpy()
            assert sorted(rid.tolist()) == ids[7:].tolist() and rid[:7].tolist() != ids[7:14].tolist()
            assert _same_f32(f.cpu().numpy(), want[rid - 100])
            g, r = store.get_dev(_dev(ids))
            r = r.cpu().numpy()
            assert (r[:7] == -1).all() and np.array_equal(rid[r[7:]], ids[7:])
            assert _same_f32(g.cpu().numpy(), np.concatenate([np.zeros((7, D), np.float32), want[7:]]))
        finally:
            store.close()


# ---- 2. re-rank on lattice inputs: every sum is exact in float32 ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice(D, nb):
    """Inputs and expected outputs: integers in [-4, 4], so S <= 8200 * 64 < 2^24 is exact in any order and d = sqrt_f32(S)."""
    rs = np.random.RandomState(D * 31 + nb)
    n, nq, L = 48, 3, nb + 3
    rows, q = rs.randint(-4, 5, (n, D)), rs.randint(-4, 5, (nq, D))
    stored = 1000 + np.arange(n, dtype=np.int64)
    ids = stored[rs.randint(0, n, (nq, L))]
    ids[rs.rand(nq, L) < 0.1] = 5000    # no stored row: keeps its ADC distance
    ids[rs.rand(nq, L) < 0.1] = -1      # no result
    ids[:, nb - 1] = ids[:, 0] = stored[4]  # a row repeated within a query
    adc = rs.rand(nq, L) * 40.0
    S = ((q[:, None, :].astype(np.int64) - rows[np.clip(ids - 1000, 0, n - 1)].astype(np.int64)) ** 2).sum(axis=2)
    has_row = (ids >= 1000) & (ids < 1000 + n)
    true_d = np.where(has_row, np.sqrt(S.astype(np.float32)).astype(np.float64), np.nan)
    d = np.where(has_row, true_d, adc)
    u = np.unique(d[0, :nb][ids[0, :nb] >= 0])
    th = float((u[u.size // 2 - 1] + u[u.size // 2]) / 2) if u.size > 1 else 1e9  # in a gap between two distances
    mr = nb - 1 if nb > 1 else 0
    want = dict(ids=np.full((nq, nb), -1, np.int64), dists=np.full((nq, nb), np.nan), src=np.full((nq, nb), -1, np.int32),
                n_kept=np.zeros(nq, np.int32))
    for qi in range(nq):
        keep = np.array([i for i in range(nb) if ids[qi, i] >= 0 and (mr == 0 or i < mr) and d[qi, i] <= th], dtype=np.int64)
        keep = keep[np.argsort(d[qi, keep], kind="stable")]
        k = keep.size
        want["ids"][qi, :k], want["dists"][qi, :k], want["src"][qi, :k], want["n_kept"][qi] = ids[qi, keep], d[qi, keep], keep, k
    return dict(rows=rows, stored=stored, q=q.astype(np.float32), ids=ids, adc=adc, th=th, mr=mr, want=want, true_d=true_d)


@gpu
@pytest.mark.parametrize("D,nb", [(D, nb) for D in (8, 504, 512, 520, 4096, 8192, 8200) for nb in (31, 257)] +
                         [(520, nb) for nb in (1, 32, 33, 1024)])
def test_rerank_on_lattice_inputs_is_exact(D, nb):
    c = _lattice(D, nb)
    store = _half_store(c["rows"], c["stored"])
    try:
        out = store.rerank_dev(_dev(c["q"]), _dev(c["ids"]), _dev(c["adc"]), rerank_nb=nb, max_returned=c["mr"], near_dup_th=c["th"])
        for k in ("ids", "src", "n_kept"):
            assert np.array_equal(out[k].cpu().numpy(), c["want"][k]), k
        assert np.array_equal(out["dists"].cpu().numpy().view(np.int64), c["want"]["dists"].view(np.int64))
        assert int(c["want"]["n_kept"].max()) > 0 or nb == 1
    finally:
        store.close()


# ---- 3. re-rank on real data, within the bound of the arithmetic contract ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D", [128, 4096])
def test_rerank_on_unit_rows_within_the_float32_bound(D):
    rs = np.random.RandomState(D)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    yh = unit(rs.randn(64, D)).astype(np.float16)
    q = unit(rs.randn(4, D)).astype(np.float32)
    q[0] = yh[5].astype(np.float32)  # a row equal to the widened query: exactly 0
    ids = np.tile(np.arange(64, dtype=np.int64), (4, 1))
    store = _half_store(yh.astype(np.float32), ids[0])
    try:
        out = store.rerank_dev(_dev(q), _dev(ids), _dev(np.zeros((4, 64))))
        d, src = out["dists"].cpu().numpy(), out["src"].cpu().numpy()
        assert (out["n_kept"].cpu().numpy() == 64).all() and (np.sort(src, axis=1) == ids).all()
        d64 = np.linalg.norm(q[:, None, :].astype(np.float64) - yh[None].astype(np.float64), axis=2)
        d64 = np.take_along_axis(d64, src.astype(np.int64), axis=1)
        # D non-negative terms in any order, two roundings each, halved by the root; the root's and the cast's rounding
        assert (np.abs(d - d64) <= (D / 2 + 8) * 2.0 ** -24 * d64).all(), float((np.abs(d - d64) / np.maximum(d64, 1e-300)).max())
        assert d[0, 0] == 0.0 and src[0, 0] == 5
    finally:
        store.close()


# ---- 4. the sharded form ------------------------------------------------------------------------------------------------------------
@gpu
def test_packed_distances_equal_the_rerank_record_for_record():
    D, nb = 520, 33
    c = _lattice(D, nb)
    nq, L = c["ids"].shape
    recs = np.zeros((nq * L, 4), np.int64)
    recs[:, 2] = c["ids"].reshape(-1)  # cis_hit.id
    off = np.concatenate([np.arange(nq, dtype=np.int64) * L, [nq * L - 2]])   # the last list does not lie inside [0, n_rec)
    cnt = np.array([L] * nq + [5], dtype=np.int32)
    q = np.concatenate([c["q"], -c["q"][:1]])
    store = _half_store(c["rows"], c["stored"])
    try:
        got = store.distances_packed_dev(_dev(q), _dev(recs), _dev(off), _dev(cnt), nb).cpu().numpy().reshape(nq, L)
        want = c["true_d"].copy()
        want[:, nb:] = np.nan   # records past nb
        want[c["ids"] < 0] = np.nan
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
        assert np.isfinite(want[:, :nb]).sum() > nb
    finally:
        store.close()


# ---- 5. exact k-NN on float16 data --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("d", [8, 40])
@pytest.mark.parametrize("m2", [100, 300])
def test_search_exact_on_half_rows_is_scipys_chain_on_the_widened_data(m2, d, k, mode):
    from columbiaimagesearch_amd import _lib
    rs = np.random.RandomState(m2 + d)
    data = rs.randn(m2, d).astype(np.float32)
    data[[7, 50, 90]] = data[3]  # duplicated rows: the tie is broken by row
    q = rs.randn(5, d).astype(np.float32)
    q[1] = data[3].astype(np.float16).astype(np.float32)
    y, x = data.astype(np.float16).astype(np.float64), q.astype(np.float64)
    s = np.zeros((5, m2))
    for i in range(d):  # sequential, every operation rounded on its own
        t = x[:, i, None] - y[None, :, i]
        s = s + t * t
    dist = np.sqrt(s)
    order = np.stack([np.lexsort((np.arange(m2), dist[i]))[:k] for i in range(5)])
    store = _half_store(data, np.arange(m2))
    _lib.check(_lib.lib().cis_exact_knn_set_mode(mode))
    try:
        ids, got = store.search_exact(_dev(q), k)
        assert np.array_equal(ids, order)
        assert np.array_equal(got.view(np.int64), np.take_along_axis(dist, order, axis=1).view(np.int64))
    finally:
        _lib.check(_lib.lib().cis_exact_knn_set_mode(0))
        store.close()


# ---- 6. through the searcher --------------------------------------------------------------------------------------------------------
@gpu
def test_searcher_with_a_half_store_equals_a_float32_store_of_the_rounded_rows():
    import torch
    from test_lopq_hip_parity import hip_model
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.rerank import FeatureStore
    z, X, Q = load_golden("tiny")
    n = 1000
    F = np.clip(np.rint(X[:n]), -4, 4).astype(np.float32)  # lattice-valued: both kernels' sums are exact
    ids = np.arange(n, dtype=np.int64)
    s = LOPQSearcherHIP(hip_model(z))
    half = _half_store(F, ids)
    full = FeatureStore(F.shape[1], torch.float32)
    try:
        s.add_codes_array(z["coarse"][:n], z["fine"][:n], ids.tolist())
        full.put_dev(_dev(ids), half.get_dev(_dev(ids))[0])
        kw = dict(quota=300, limit=60, rerank_nb=50, max_returned=40, near_dup_th=6.2)
        ask = _dev(np.array([3, 999, 123456, 500, -1], dtype=np.int64))
        q = _dev(np.clip(np.rint(Q), -4, 4).astype(np.float32))
        for a, b in ((s.search_by_ids_dev(ask, half, **kw), s.search_by_ids_dev(ask, full, **kw)),
                     (s.search_rerank_dev(q, half, **kw), s.search_rerank_dev(q, full, **kw))):
            for key in b:
                assert np.array_equal(a[key].cpu().numpy(), b[key].cpu().numpy(), equal_nan=a[key].dtype.is_floating_point), key
            assert int(a["n_kept"].max()) > 1
    finally:
        half.close()
        full.close()
        s.close()


# ---- 7. arguments: nothing here needs a device ----------------------------------------------------------------------------------------
def test_argument_errors_need_no_device():
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.rerank import FeatureStore
    L, E = _lib.lib(), _lib.CIS_EINVAL
    h = ctypes.c_void_p()
    assert [L.cis_featstore_create_half(ctypes.byref(h), D, r) for D, r in ((12, 0), (0, 0), (8, -1))] == [E, E, E] and h.value is None
    assert L.cis_featstore_create_half(None, 8, 0) == E
    p = 4096  # (a pointer that is never followed)
    sel = lambda nq=1, L_=8, nb=4, cap=16, out=p: L.cis_rerank_select_half_dev(p, 10, 8, p, p, cap, p, nq, p, p, L_, nb, 0, 0, 0.0, out, p, p, p, None)
    assert [sel(nb=1025, L_=2000), sel(nb=9), sel(cap=12), sel(out=None)] == [E] * 4 and sel(nq=0) == _lib.CIS_OK
    pk = lambda nq=1, nb=4, cap=16, true=p, n_rec=5: L.cis_rerank_packed_half_dev(p, 10, 8, p, p, cap, p, nq, p, n_rec, p, p, nb, true, None)
    assert [pk(nb=1025), pk(cap=12), pk(true=None)] == [E] * 3 and pk(nq=0) == _lib.CIS_OK and pk(n_rec=0) == _lib.CIS_OK
    knn = lambda m1=1, k=1, d=8, idx=p, data=p: L.cis_exact_knn_half_dev(data, 5, d, p, 4, m1, k, 0, 0, idx, p, None)
    assert [knn(k=0), knn(d=0), knn(idx=None), knn(data=None)] == [E] * 4 and knn(m1=0) == _lib.CIS_OK
    for D, dtype, storage in ((8, torch.float64, torch.float16), (12, torch.float32, torch.float16), (8, torch.float32, torch.bfloat16)):
        with pytest.raises(ValueError, match="storage"):
            FeatureStore(D, dtype, storage=storage)
