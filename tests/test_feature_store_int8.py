"""int8 feature rows with an in-row scale behind a float32 interface (rerank.FeatureStore(storage=torch.int8); csrc/feat_int8.hip): the
quantisation against a numpy model bit for bit (values and stored bytes), removal, the re-rank kernels against exact arithmetic on
lattice inputs and against a float64 norm within the bound of the kernel's arithmetic contract, the packed form, and the arguments."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

gpu = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _quant(x):
    """The put contract: (scales float32 [n], codes int8 [n, D]); get hands back codes.astype(float32) * scales[:, None]."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        s = np.abs(x).max(axis=1) / np.float32(127)
        s[~np.isfinite(x).all(axis=1)] = np.nan
        c = np.clip(np.rint(x / s[:, None]), -127, 127)
        return s, np.where((s > 0)[:, None], c, 0).astype(np.int8)


def _deq(x):
    s, c = _quant(x)
    return c.astype(np.float32) * s[:, None]


def _store(rows, ids):
    import torch
    from columbiaimagesearch_amd.rerank import FeatureStore
    store = FeatureStore(rows.shape[1], torch.float32, storage=torch.int8)
    store.put_dev(_dev(np.asarray(ids, dtype=np.int64)), _dev(rows.astype(np.float32)))
    return store


def _same_f32(got, want):
    return bool(((got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))).all())


@gpu
@pytest.mark.parametrize("D", [16, 48, 128, 272, 4096])
def test_put_quantises_like_the_numpy_model_and_get_dequantises(D):
    import torch
    rs = np.random.RandomState(D)
    x = rs.randn(9, D).astype(np.float32)
    x[0] = 0.0                                                           # s = 0, zero codes
    x[1, D // 3] = -7.5                                                  # the largest component is negative: code -127
    half = np.resize(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 126.5, -126.5, 0.25, 0.75]), D)
    half[D - 1] = 127.0
    x[2] = (half * 2.0 ** -7).astype(np.float32)                         # s = 2^-7: codes on k + 0.5, rounded half to even
    x[3] = rs.randint(-2000, 2001, D).astype(np.float32) * np.float32(2.0 ** -149)  # subnormals, and a subnormal scale
    x[4, D // 2] = np.nan
    x[5, 0] = -np.inf
    ids = np.array([10, 11, 12, 13, 14, 15, 16, 17, 16], dtype=np.int64)  # the last row overwrites row 6
    s, c = _quant(x)
    assert s[0] == 0 and c[1].min() == -127 and s[2] == 2.0 ** -7 and 0 < s[3] < 2.0 ** -126 and c.min() == -127
    store = _store(x[:1], ids[:1])  # (a first put of one row, so the batch below also grows the rows)
    try:
        assert store.put_dev(_dev(ids), _dev(x)) == (7, 0) and len(store) == 8
        last = [0, 1, 2, 3, 4, 5, 8, 7]
        g, r = store.get_dev(_dev(np.concatenate([ids[:8], [99, -1]])))
        assert r.cpu().numpy().tolist() == list(range(8)) + [-1, -1]
        want = np.concatenate([c[last].astype(np.float32) * s[last, None], np.zeros((2, D), np.float32)])
        assert np.isnan(want[4]).all() and np.isnan(want[5]).all() and _same_f32(g.cpu().numpy(), want)
        assert _same_f32(store.rows_dev()[0].cpu().numpy(), want[:8])
        # the stored bytes: 16 + D a row, the scale and twelve zero bytes, then the codes
        raw = type("Raw", (), {"__cuda_array_interface__": dict(shape=(8 * (16 + D),), typestr="|u1", data=(store._view()[0], False), version=2)})()
        head = np.concatenate([s[last].view(np.uint8).reshape(8, 4), np.zeros((8, 12), np.uint8)], axis=1)
        assert np.array_equal(torch.as_tensor(raw, device="cuda").cpu().numpy().reshape(8, 16 + D), np.concatenate([head, c[last].view(np.uint8)], axis=1))
    finally:
        store.close()


@gpu
def test_remove_keeps_every_scale_with_its_row():
    import torch
    from columbiaimagesearch_amd.rerank import FeatureStore
    rs = np.random.RandomState(2)
    n, D = 300, 48
    x = (rs.randn(n, D) * rs.rand(n, 1) * 10).astype(np.float32)  # a different scale in every row
    ids = 1000 + np.arange(n, dtype=np.int64)
    gone = np.concatenate([rs.permutation(n - 10)[:70], np.arange(n - 10, n)])
    store, plain = _store(x, ids), FeatureStore(D, torch.float32)
    try:
        plain.put_dev(_dev(ids), _dev(x))
        assert store.remove_dev(_dev(ids[gone])) == plain.remove_dev(_dev(ids[gone])) == 80 and len(store) == len(plain) == n - 80
        assert np.array_equal(store.row_ids().cpu().numpy(), plain.row_ids().cpu().numpy())
        g, r = store.get_dev(_dev(ids))
        want = np.where(np.isin(np.arange(n), gone)[:, None], np.float32(0), _deq(x))
        assert _same_f32(g.cpu().numpy(), want) and np.array_equal(r.cpu().numpy() < 0, np.isin(np.arange(n), gone))
    finally:
        store.close()
        plain.close()


@functools.lru_cache(maxsize=None)
def _lattice(D):
    """Rows c 2^-7 with one |c| = 127 and the others <= 3, so s = 2^-7 exactly; queries on the same lattice, |q| <= 3 2^-7: every
    difference is an integer below 131 times 2^-7 and a sum of D <= 8208 squares stays below 2^24 2^-14, exact in any order."""
    rs = np.random.RandomState(D)
    n, nq = 48, 5
    c = rs.randint(-3, 4, (n, D))
    c[np.arange(n), rs.randint(0, D, n)] = rs.choice([-127, 127], n)
    rows = (c * 2.0 ** -7).astype(np.float32)
    rows[7, D - 1] = np.nan                       # a NaN row: its distance is NaN and keeps the ADC distance
    q = (rs.randint(-3, 4, (nq, D)) * 2.0 ** -7).astype(np.float32)
    stored = 1000 + np.arange(n, dtype=np.int64)
    ids = stored[rs.randint(0, n, (nq, 40))]
    ids[:, 3], ids[:, 4], ids[:, 5], ids[:, 0] = 5000, -1, stored[7], stored[9]   # not stored, no result, the NaN row
    ids[:, 6] = stored[9]                          # a row repeated within a query: an exact tie
    adc = rs.rand(nq, 40) * 2.0
    deq = _deq(rows)
    assert np.array_equal(np.delete(deq, 7, axis=0), np.delete(rows, 7, axis=0)) and np.isnan(deq[7]).all()
    S = ((q[:, None, :].astype(np.float64) - deq[np.clip(ids - 1000, 0, n - 1)].astype(np.float64)) ** 2).sum(axis=2)
    assert np.array_equal(S[np.isfinite(S)], S[np.isfinite(S)].astype(np.float32))
    true_d = np.float32(np.sqrt(np.float32(S))).astype(np.float64)
    true_d[(ids < 1000) | (ids >= 1000 + n)] = np.nan
    return dict(rows=rows, stored=stored, q=q, ids=ids, adc=adc, true_d=true_d, d=np.where(np.isnan(true_d), adc, true_d))


def _host_rerank(ids, d, nb, mr, th):
    nq = ids.shape[0]
    want = dict(ids=np.full((nq, nb), -1, np.int64), dists=np.full((nq, nb), np.nan), src=np.full((nq, nb), -1, np.int32), n_kept=np.zeros(nq, np.int32))
    for qi in range(nq):
        keep = np.array([i for i in range(nb) if ids[qi, i] >= 0 and (mr == 0 or i < mr) and (th is None or d[qi, i] <= th)], dtype=np.int64)
        keep, k = keep[np.argsort(d[qi, keep], kind="stable")], keep.size
        want["ids"][qi, :k], want["dists"][qi, :k], want["src"][qi, :k], want["n_kept"][qi] = ids[qi, keep], d[qi, keep], keep, k
    return want


@gpu
@pytest.mark.parametrize("nb", [1, 7, 40])
@pytest.mark.parametrize("D", [16, 128, 144, 400, 1024, 1040, 4112, 8208])  # groups of 4, 8, 16, 32, 64 lanes; full and ragged trips; 8208 in place
def test_rerank_on_lattice_inputs_is_exact(D, nb):
    c = _lattice(D)
    store = _store(c["rows"], c["stored"])
    try:
        for nq, mr, use_th in itertools.product((1, 5), (0, 5), (False, True)):
            th = float(np.median(c["d"][:nq, :nb])) if use_th else None
            out = store.rerank_dev(_dev(c["q"][:nq]), _dev(c["ids"][:nq]), _dev(c["adc"][:nq]), rerank_nb=nb, max_returned=mr, near_dup_th=th)
            want = _host_rerank(c["ids"][:nq], c["d"][:nq], nb, mr, th)
            for k in ("ids", "src", "n_kept"):
                assert np.array_equal(out[k].cpu().numpy(), want[k]), (k, nq, mr, th)
            assert np.array_equal(out["dists"].cpu().numpy().view(np.int64), want["dists"].view(np.int64)), (nq, mr, th)
    finally:
        store.close()


@gpu
@pytest.mark.parametrize("D", [128, 4096])
def test_rerank_on_unit_rows_within_the_float32_bound(D):
    rs = np.random.RandomState(D)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    x, q = unit(rs.randn(64, D)), unit(rs.randn(4, D))
    ids = np.tile(np.arange(64, dtype=np.int64), (4, 1))
    store = _store(x, ids[0])
    try:
        out = store.rerank_dev(_dev(q), _dev(ids), _dev(np.zeros((4, 64))))
        d, src = out["dists"].cpu().numpy(), out["src"].cpu().numpy()
        assert (out["n_kept"].cpu().numpy() == 64).all() and (np.sort(src, axis=1) == ids).all()
        d64 = np.linalg.norm(q[:, None, :].astype(np.float64) - _deq(x)[None].astype(np.float64), axis=2)
        d64 = np.take_along_axis(d64, src.astype(np.int64), axis=1)
        # df is one rounding and each fma one: D non-negative terms in any order, two roundings each, halved by the root; the root's
        # and the fold's roundings
        assert (np.abs(d - d64) <= (D / 2 + 8) * 2.0 ** -24 * d64).all(), float((np.abs(d - d64) / d64).max())
        assert all(np.array_equal(np.lexsort((src[i], d[i])), np.arange(64)) for i in range(4))
    finally:
        store.close()


@gpu
@pytest.mark.parametrize("D", [128, 1040, 8208])
def test_packed_distances_equal_the_rerank_record_for_record(D):
    c, nb = _lattice(D), 33
    nq, L = c["ids"].shape
    recs = np.zeros((nq * L, 4), np.int64)
    recs[:, 2] = c["ids"].reshape(-1)  # cis_hit.id
    store = _store(c["rows"], c["stored"])
    try:
        off, cnt = np.arange(nq, dtype=np.int64) * L, np.full(nq, L, np.int32)
        got = store.distances_packed_dev(_dev(c["q"]), _dev(recs), _dev(off), _dev(cnt), nb).cpu().numpy().reshape(nq, L)
        want = c["true_d"].copy()  # NaN where the re-rank keeps the ADC distance: no result, no stored row, a NaN row
        want[:, nb:] = np.nan
        assert np.array_equal(got.view(np.int64)[~np.isnan(want)], want.view(np.int64)[~np.isnan(want)]) and np.isnan(got[np.isnan(want)]).all()
        assert np.isfinite(want).sum() > nq * nb // 2
    finally:
        store.close()


def test_argument_errors_need_no_device():
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.rerank import FeatureStore
    L, E = _lib.lib(), _lib.CIS_EINVAL
    h = ctypes.c_void_p()
    assert [L.cis_featstore_create_int8(ctypes.byref(h), D, r) for D, r in ((0, 0), (8, 0), (24, 0), (16, -1))] == [E] * 4 and h.value is None
    assert L.cis_featstore_create_int8(None, 16, 0) == E
    p = 4096  # (a pointer that is never followed)
    sel = lambda nq=1, L_=8, nb=4, cap=16, out=p: L.cis_rerank_select_int8_dev(p, 10, 16, p, p, cap, p, nq, p, p, L_, nb, 0, 0, 0.0, out, p, p, p, None)
    assert [sel(nb=1025, L_=2000), sel(nb=9), sel(cap=12), sel(out=None)] == [E] * 4 and sel(nq=0) == _lib.CIS_OK
    pk = lambda nq=1, nb=4, cap=16, true=p, n_rec=5: L.cis_rerank_packed_int8_dev(p, 10, 16, p, p, cap, p, nq, p, n_rec, p, p, nb, true, None)
    assert [pk(nb=1025), pk(cap=12), pk(true=None)] == [E] * 3 and pk(nq=0) == _lib.CIS_OK and pk(n_rec=0) == _lib.CIS_OK
    for D, dtype in ((24, torch.float32), (16, torch.float64)):
        with pytest.raises(ValueError, match="storage"):
            FeatureStore(D, dtype, storage=torch.int8)
