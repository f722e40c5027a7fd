"""Search + exact re-rank on the device (csrc/lopq_rerank.hip; ResidentFeatures.device_map / rows_of_dev / rerank_dev,
LOPQSearcherHIP.device_ids_of / search_rerank_dev) against the host path it stands beside (ResidentFeatures.rerank: rows_of +
k_rerank + a Python loop) and against the restated reference loop (oracle/lopq_oracle.py:rerank).

The device distances are built to be the bits of k_rerank, so every comparison with the host path is exact: ids, counts, the int64
views of the float64 distances, the -1 / NaN padding, and ids_in[q, src] == out_ids."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

gpu = pytest.mark.gpu

N_FEATS = 500
_feats = {}


def _unit_feats(dtype, D):
    """n = 500 unit features of width D (seeded; made once per shape and left unchanged) as (numpy, ResidentFeatures)."""
    key = (np.dtype(dtype).name, D)
    if key not in _feats:
        import torch
        from columbiaimagesearch_amd.rerank import ResidentFeatures
        rs = np.random.RandomState(1000 + D)
        f = rs.randn(N_FEATS, D).astype(dtype)
        f /= np.linalg.norm(f, axis=1, keepdims=True)
        _feats[key] = (f, ResidentFeatures(torch.as_tensor(f).cuda().contiguous()))
    return _feats[key]


def _gap_threshold(dists):
    """Midpoint of the widest gap between adjacent distances near the median: no distance sits on the threshold."""
    d = np.unique(np.asarray([x for x in dists if not np.isnan(x)], dtype=np.float64))
    if d.size < 2:
        return float(d[0]) + 1.0 if d.size else 1.0
    m = d.size // 2
    lo, hi = max(m - 5, 0), min(m + 6, d.size)
    w = d[lo:hi]
    if w.size < 2:
        w = d
    g = int(np.argmax(np.diff(w)))
    return float(0.5 * (w[g] + w[g + 1]))


def _assert_same(dev, host, ids_in, nb, ident=lambda i: int(i)):
    """dev: rerank_dev's dict (numpy arrays); host: rerank's per-query (ids, dists) lists."""
    out_ids, out_d, src, n_kept = dev["ids"], dev["dists"], dev["src"], dev["n_kept"]
    assert out_ids.shape == out_d.shape == src.shape == (len(host), nb)
    for qi, (hids, hd) in enumerate(host):
        k = int(n_kept[qi])
        assert k == len(hids), (qi, k, len(hids))
        assert [ident(i) for i in out_ids[qi, :k]] == [i if isinstance(i, str) else int(i) for i in hids], qi
        assert np.array_equal(out_d[qi, :k].view(np.int64), np.asarray(hd, dtype=np.float64).view(np.int64)), qi
        assert (out_ids[qi, k:] == -1).all() and np.isnan(out_d[qi, k:]).all() and (src[qi, k:] == -1).all(), qi
        assert (src[qi, :k] >= 0).all() and (src[qi, :k] < nb).all()
        assert (ids_in[qi, src[qi, :k]] == out_ids[qi, :k]).all(), qi
        assert len(set(src[qi, :k].tolist())) == k


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


EDGE_CASES = [("D", D, 20) for D in (1, 63, 64, 65, 96, 257, 4096)] + \
             [("nb", 96, nb) for nb in (1, 2, 63, 64, 65, 100, 255, 256, 257, 1000, 1024)]


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("what,D,nb", EDGE_CASES, ids=["%s%d" % (w, D if w == "D" else nb) for w, D, nb in EDGE_CASES])
def test_bit_parity_with_the_host_path_at_the_kernels_edges(dtype, what, D, nb):
    """Widths around the wave (1, 63, 64, 65), a width that is staged in LDS for float32 and read through L1 for float64
    (4096), list lengths around one and four results per thread and the 1024 limit, a row stride L > nb, ids without a feature
    (they keep the ADC distance), a -1 / NaN tail, a query without results; with and without max_returned and near_dup_th."""
    import torch
    feats, rf = _unit_feats(dtype, D)
    for pad in (0, 7):
        for nq in (1, 7):
            rs = np.random.RandomState(nb * 131 + D + pad + nq)
            L = nb + pad
            Q = (feats[rs.randint(0, N_FEATS, nq)] + 0.05 * rs.randn(nq, D)).astype(dtype)
            ids = rs.randint(0, N_FEATS + 40, (nq, L)).astype(np.int64)  # 7 % of the ids have no feature; ids may repeat
            adc = np.sort(rs.rand(nq, L), axis=1)
            tail_row = 2 if nq > 2 else 0
            ids[tail_row, (3 * nb) // 4:] = -1
            if nq > 4:
                ids[4, :] = -1
            adc[ids < 0] = np.nan
            q_t = torch.as_tensor(Q).cuda().contiguous()
            ids_t, adc_t = torch.as_tensor(ids).cuda(), torch.as_tensor(adc).cuda()
            plain = rf.rerank(q_t, ids, adc, rerank_nb=nb)
            t = _gap_threshold([d for _, hd in plain for d in hd])
            for kw in ({}, {"max_returned": 8}, {"near_dup_th": t}, {"max_returned": 8, "near_dup_th": t}):
                host = plain if not kw else rf.rerank(q_t, ids, adc, rerank_nb=nb, **kw)
                dev = _np(rf.rerank_dev(q_t, ids_t, adc_t, rerank_nb=nb, **kw))
                _assert_same(dev, host, ids, nb)
    # rerank_nb=None takes the whole list; `out` is written in place
    out = {"ids": torch.empty((nq, L), dtype=torch.int64, device="cuda"), "dists": torch.empty((nq, L), dtype=torch.float64, device="cuda"),
           "src": torch.empty((nq, L), dtype=torch.int32, device="cuda"), "n_kept": torch.empty(nq, dtype=torch.int32, device="cuda")}
    if L <= 1024:
        got = rf.rerank_dev(q_t, ids_t, adc_t, out=out)
        assert got is out
        _assert_same(_np(out), rf.rerank(q_t, ids, adc), ids, L)
    else:
        with pytest.raises(ValueError, match="host rerank"):
            rf.rerank_dev(q_t, ids_t, adc_t, out=out)


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_rerank_matches_reference_semantics(dtype):
    """The setup of test_lopq_hip_parity.py::test_exact_rerank_matches_reference_semantics through rerank_dev, against the restated
    searcher_lopqhbase.py:864-912 loop; the threshold sits in a gap of the oracle's distances."""
    import torch
    from oracle import lopq_oracle as O
    from columbiaimagesearch_amd.rerank import ResidentFeatures
    rs = np.random.RandomState(3)
    n, D, nq, L = 500, 96, 7, 20
    feats = rs.randn(n, D).astype(dtype)
    feats /= np.linalg.norm(feats, axis=1, keepdims=True)
    Q = (feats[rs.randint(0, n, nq)] + 0.05 * rs.randn(nq, D)).astype(dtype)
    ids = np.stack([rs.choice(n + 40, L, replace=False) for _ in range(nq)]).astype(np.int64)  # some ids have no feature
    ids[2, 15:] = -1
    adc = np.sort(rs.rand(nq, L), axis=1)
    adc[2, 15:] = np.nan
    rf = ResidentFeatures(torch.as_tensor(feats).cuda().contiguous())

    def oracle(qi, kw):
        res = [(int(ids[qi, i]), float(adc[qi, i])) for i in range(L) if ids[qi, i] >= 0]
        fb = {int(i): feats[i] for i in ids[qi] if 0 <= i < n}
        return O.rerank(Q[qi], fb, res, kw["rerank_nb"], kw.get("max_returned"), kw.get("near_dup_th"))

    t = _gap_threshold([float(d) for qi in range(nq) for d in oracle(qi, dict(rerank_nb=20))[1]])
    q_t, ids_t, adc_t = torch.as_tensor(Q).cuda().contiguous(), torch.as_tensor(ids).cuda(), torch.as_tensor(adc).cuda()
    for kw in [dict(rerank_nb=12), dict(rerank_nb=20, max_returned=8), dict(rerank_nb=20, near_dup_th=t),
               dict(rerank_nb=20, max_returned=8, near_dup_th=t)]:
        got = _np(rf.rerank_dev(q_t, ids_t, adc_t, **kw))
        for qi in range(nq):
            eids, ed = oracle(qi, kw)
            k = int(got["n_kept"][qi])
            assert k == len(eids)
            assert [int(i) for i in got["ids"][qi, :k]] == [int(i) for i in eids]
            np.testing.assert_allclose(got["dists"][qi, :k], np.asarray(ed, dtype=np.float64), rtol=2e-6 if dtype == np.float32 else 1e-13)
            assert (got["ids"][qi, k:] == -1).all() and np.isnan(got["dists"][qi, k:]).all()


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ties_come_out_in_their_order_before_the_rerank(dtype):
    """Three identical feature rows at places 9, 3, 14 of one list and two results without a feature that carry one ADC value:
    equal distances rank by their place before the re-order (np.argsort(kind="stable")), and the row equals the host path's."""
    import torch
    from columbiaimagesearch_amd.rerank import ResidentFeatures
    rs = np.random.RandomState(77)
    n, D, L = 50, 33, 16
    feats = rs.randn(n, D).astype(dtype)
    feats[17] = feats[5]
    feats[30] = feats[5]
    Q = (feats[5:6] + 0.3 * rs.randn(1, D)).astype(dtype)
    ids = np.array([[1, 2, 3, 5, 4, 6, n + 3, 7, 8, 30, 9, n + 1, 10, 11, 17, 12]], dtype=np.int64)
    adc = np.sort(rs.rand(1, L), axis=1)
    adc[0, 6] = adc[0, 11] = 0.5
    rf = ResidentFeatures(torch.as_tensor(feats).cuda().contiguous())
    q_t = torch.as_tensor(Q).cuda().contiguous()
    got = _np(rf.rerank_dev(q_t, torch.as_tensor(ids).cuda(), torch.as_tensor(adc).cuda()))
    _assert_same(got, rf.rerank(q_t, ids, adc), ids, L)
    src, d = got["src"][0].tolist(), got["dists"][0]
    assert got["n_kept"][0] == L
    p = src.index(3)
    assert src[p:p + 3] == [3, 9, 14] and d[p] == d[p + 1] == d[p + 2]
    p = src.index(6)
    assert src[p:p + 2] == [6, 11] and d[p] == d[p + 1] == 0.5
    for a in range(L - 1):
        assert d[a] < d[a + 1] or (d[a] == d[a + 1] and src[a] < src[a + 1])


def _id_table(kind, n, rs):
    from columbiaimagesearch_amd.lopq.search import _SLOT_BASE
    if kind == "sequential":
        return np.arange(n, dtype=np.int64)
    if kind == "multiples_of_2^20":
        return np.arange(n, dtype=np.int64) << 20
    if kind == "random_62_bit":
        return rs.randint(0, 1 << 62, n, dtype=np.int64)
    if kind == "slots":
        return _SLOT_BASE + rs.permutation(n).astype(np.int64)
    assert kind == "duplicated"
    return rs.randint(0, n // 2 + 1, n, dtype=np.int64) * 3


@gpu
@pytest.mark.parametrize("n", [1, 2, 1000, 100003])
@pytest.mark.parametrize("kind", ["sequential", "multiples_of_2^20", "random_62_bit", "slots", "duplicated"])
def test_id_map_equals_the_host_dictionary(kind, n):
    import torch
    from columbiaimagesearch_amd.rerank import ResidentFeatures
    rs = np.random.RandomState(n % 9973 + len(kind))
    table = _id_table(kind, n, rs)
    rf = ResidentFeatures(torch.zeros((n, 1), dtype=torch.float32, device="cuda"), ids=table.tolist())
    keys, rows = rf.device_map()
    assert keys.shape == rows.shape and keys.shape[0] >= 2 * n and (keys.shape[0] & (keys.shape[0] - 1)) == 0
    assert rf.device_map()[0] is keys  # cached
    present = table if n <= 1000 else table[rs.randint(0, n, 3000)]
    absent = np.concatenate([table[:200] + 1, table[:200] + (1 << 20), rs.randint(0, 1 << 62, 200, dtype=np.int64)])
    negative = np.array([-1, -2, -5, -(1 << 62), np.iinfo(np.int64).min], dtype=np.int64)
    probe = np.concatenate([present, absent, negative, table[-3:]])
    want = np.array([rf._row.get(int(k), -1) for k in probe], dtype=np.int64)
    assert (want[:present.size] >= 0).all() and (want[present.size + absent.size:present.size + absent.size + 5] == -1).all()
    got = rf.rows_of_dev(torch.as_tensor(probe.reshape(1, -1)).cuda()).cpu().numpy()
    assert got.shape == (1, probe.size) and (got[0] == want).all()
    assert (got == rf.rows_of(probe.reshape(1, -1))).all()


@gpu
def test_id_map_identity_refusals_and_string_ids():
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.rerank import ResidentFeatures
    feats = torch.zeros((10, 2), dtype=torch.float64, device="cuda")
    rf = ResidentFeatures(feats)
    assert rf.device_map() is None  # no ids: the identity, no table
    probe = np.array([[0, 9, 10, -1, 3, 1 << 40]], dtype=np.int64)
    assert (rf.rows_of_dev(torch.as_tensor(probe).cuda()).cpu().numpy() == rf.rows_of(probe)).all()
    names = ["%040x_0" % i for i in range(10)]
    rs_ = ResidentFeatures(feats, ids=names)
    with pytest.raises(ValueError, match="dev_ids"):
        rs_.device_map()
    with pytest.raises(ValueError):
        rs_.device_map(np.arange(9))  # one per row
    dev_ids = (1 << 62) + np.arange(10, dtype=np.int64)[::-1]
    rs_.device_map(dev_ids)
    got = rs_.rows_of_dev(torch.as_tensor(np.array([(1 << 62) + 9, (1 << 62) + 0, 5, (1 << 62) + 10], dtype=np.int64)).cuda())
    assert got.cpu().numpy().tolist() == [0, 9, -1, -1]
    # the capacity: a power of two >= 2 n, checked before anything is launched (the buffers are never touched)
    keys = torch.full((16,), 7, dtype=torch.int64, device="cuda")
    rows = torch.full((16,), 7, dtype=torch.int64, device="cuda")
    ids = torch.arange(5, dtype=torch.int64, device="cuda")
    L = _lib.lib()
    for cap in (12, 8, 0, -16):
        assert L.cis_idmap_build_dev(ids.data_ptr(), 5, keys.data_ptr(), rows.data_ptr(), cap, None) == _lib.CIS_EINVAL
    torch.cuda.synchronize()
    assert (keys == 7).all() and (rows == 7).all()
    assert L.cis_idmap_build_dev(ids.data_ptr(), 5, keys.data_ptr(), rows.data_ptr(), 16, None) == _lib.CIS_OK
    torch.cuda.synchronize()
    assert sorted(keys.cpu().tolist()) == [-1] * 11 + [0, 1, 2, 3, 4]


def _fixture_searcher(name, string_ids):
    """(searcher, features with every tenth row removed, numpy inputs): the index holds every vector, the resident set does not."""
    import torch
    from test_lopq_hip_parity import hip_model
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.rerank import ResidentFeatures
    z, X, Q = load_golden(name)
    n = int(z["coarse"].shape[0])
    ids = ["%040x_0" % (i * 2654435761 % (1 << 61)) for i in range(n)] if string_ids else list(range(n))
    s = LOPQSearcherHIP(hip_model(z))
    s.add_codes_array(z["coarse"], z["fine"], ids if string_ids else None)
    keep = np.array([i for i in range(n) if i % 10 != 3])
    kept_ids = [ids[i] for i in keep]
    rf = ResidentFeatures(torch.as_tensor(np.ascontiguousarray(X[:n][keep])).cuda().contiguous(), ids=kept_ids)
    if string_ids:
        assert (s.device_ids_of(["never seen", kept_ids[0]]) == [-1, s._slot_of[kept_ids[0]] + (1 << 62)]).all()
        n_slots = len(s._id_of)
        rf.device_map(s.device_ids_of(kept_ids))
        assert len(s._id_of) == n_slots  # a pure look-up: no slot was created
    return s, rf, Q


def _host_path(s, rf, q_t, string_ids, quota, limit, **kw):
    r = s.search_batch_dev(q_t, quota=quota, limit=limit)
    ids, adc = r["ids"].cpu().numpy(), r["dists"].cpu().numpy()
    caller = ids
    if string_ids:
        caller = np.array([[s._caller_id(i) if i >= 0 else None for i in row] for row in ids], dtype=object)
    return ids, rf.rerank(q_t, caller, adc, **kw), r["visited"].cpu().numpy()


@gpu
@pytest.mark.parametrize("string_ids", [False, True], ids=["int_ids", "string_ids"])
@pytest.mark.parametrize("name", ["tiny", "c3b"])
def test_search_rerank_dev_equals_search_then_host_rerank(name, string_ids):
    """tiny (float64, no PCA) and c3b (float32; the model has PCA, the re-rank runs at the 288-wide input): search_rerank_dev ==
    search_batch_dev + the host rerank bit for bit, with integer ids and with "<sha1>_0"-style ids mapped through device_ids_of,
    a tenth of the features not resident; once more through a view() on a second stream while the base runs the same batch."""
    import torch
    s, rf, Q = _fixture_searcher(name, string_ids)
    q_t = torch.as_tensor(np.ascontiguousarray(Q)).cuda().contiguous()
    ident = (lambda i: s._caller_id(i)) if string_ids else (lambda i: int(i))
    quota, limit = 300, 60
    ids_in, plain, visited = _host_path(s, rf, q_t, string_ids, quota, limit)
    assert any(len(h[0]) for h in plain)
    missing = (rf.rows_of_dev(torch.as_tensor(ids_in).cuda()).cpu().numpy() < 0) & (ids_in >= 0)
    assert missing.any() and not missing.all()  # both branches run
    t = _gap_threshold([d for _, hd in plain for d in hd])
    for kw in ({}, {"rerank_nb": 25}, {"max_returned": 8}, {"rerank_nb": 40, "near_dup_th": t, "max_returned": 30}):
        _, host, _ = _host_path(s, rf, q_t, string_ids, quota, limit, **kw)
        dev = _np(s.search_rerank_dev(q_t, rf, quota=quota, limit=limit, **kw))
        assert (dev.pop("visited") == visited).all()
        _assert_same(dev, host, ids_in, min(kw.get("rerank_nb", limit), limit), ident)
    # two batches in flight: a view on a second stream beside the base searcher
    kw = {"rerank_nb": 40, "near_dup_th": t}
    _, host, _ = _host_path(s, rf, q_t, string_ids, quota, limit, **kw)
    v = s.view()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b = v.search_rerank_dev(q_t, rf, quota=quota, limit=limit, **kw)
    a = s.search_rerank_dev(q_t, rf, quota=quota, limit=limit, **kw)
    torch.cuda.synchronize()
    a, b = _np(a), _np(b)
    for k in ("ids", "src", "n_kept", "visited"):
        assert (a[k] == b[k]).all(), k
    assert np.array_equal(a["dists"].view(np.int64), b["dists"].view(np.int64))
    a.pop("visited")
    _assert_same(a, host, ids_in, 40, ident)
    v.close()
    s.close()


@gpu
def test_width_4096_on_c3full():
    """32 queries over the 4096-wide float32 features of c3full, limit = rerank_nb = 100 (the reference's default)."""
    import torch
    s, rf, Q = _fixture_searcher("c3full", False)
    q_t = torch.as_tensor(np.ascontiguousarray(Q[:32])).cuda().contiguous()
    ids_in, host, visited = _host_path(s, rf, q_t, False, 1000, 100, rerank_nb=100)
    dev = _np(s.search_rerank_dev(q_t, rf, quota=1000, limit=100, rerank_nb=100))
    assert (dev.pop("visited") == visited).all() and int(dev["n_kept"].min()) > 0
    _assert_same(dev, host, ids_in, 100)
    s.close()


def test_argument_errors_need_no_device():
    """Every argument check of the new entry points comes before the device is touched: CIS_EINVAL with or without a GPU."""
    from columbiaimagesearch_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced

    def select(dtype=_lib.CIS_F32, D=8, Lq=10, nb=10, keys=None, rows=None, cap=0, max_returned=0):
        return L.cis_rerank_select_dev(p, dtype, 100, D, keys, rows, cap, p, 3, p, p, Lq, nb, max_returned, 0, 0.0, p, p, p, p, None)

    assert select(Lq=2000, nb=1025) == _lib.CIS_EINVAL
    with pytest.raises(ValueError, match="host rerank"):
        _lib.check(_lib.CIS_EINVAL)
    assert select(Lq=10, nb=11) == _lib.CIS_EINVAL
    assert select(nb=-1) == _lib.CIS_EINVAL
    assert select(D=0) == _lib.CIS_EINVAL and select(D=-4) == _lib.CIS_EINVAL
    assert select(dtype=2) == _lib.CIS_EINVAL and select(dtype=0) == _lib.CIS_EINVAL
    assert select(max_returned=-1) == _lib.CIS_EINVAL
    assert select(keys=p, rows=p, cap=12) == _lib.CIS_EINVAL
    assert select(keys=p, rows=None, cap=16) == _lib.CIS_EINVAL
    assert L.cis_idmap_build_dev(p, 3, p, p, 12, None) == _lib.CIS_EINVAL   # not a power of two
    assert L.cis_idmap_build_dev(p, 5, p, p, 8, None) == _lib.CIS_EINVAL    # < 2 n
    assert L.cis_idmap_build_dev(p, -1, p, p, 8, None) == _lib.CIS_EINVAL
    assert L.cis_idmap_lookup_dev(p, p, 12, 100, p, 4, p, None) == _lib.CIS_EINVAL
    assert L.cis_idmap_lookup_dev(p, p, 16, 100, p, -1, p, None) == _lib.CIS_EINVAL
    # nothing to do is not an error, and needs no device either
    assert L.cis_rerank_select_dev(p, _lib.CIS_F64, 100, 8, None, None, 0, p, 0, p, p, 10, 10, 0, 0, 0.0, p, p, p, p, None) == _lib.CIS_OK
    assert L.cis_idmap_lookup_dev(None, None, 0, 100, p, 0, p, None) == _lib.CIS_OK
