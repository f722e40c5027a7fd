"""lopq.eval on the GPU against tests/golden/eval.npz: the exact nearest-neighbour kernel (csrc/lopq_eval.hip) against scipy's
cdist -- indices equal, distances bit-equal, on the matrix-core path and with the exact-only path forced -- and the six functions
of the module against the reference's eval.py on a small model."""
import os

import numpy as np
import pytest

import eval_cases as ec
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z():
    return dict(np.load(os.path.join(GOLDEN, "eval.npz")))


@pytest.fixture(params=["prefilter", "exact_only"])
def path(request):
    from columbiaimagesearch_amd.lopq import eval as ev
    ev.set_exact_mode(exact_only=request.param == "exact_only")
    yield request.param
    ev.set_exact_mode(exact_only=False)


def _bit_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _check(z, name, idx, dist, k=ec.K):
    assert np.array_equal(idx, z[name + "_idx"][:, :k].astype(np.int64)), name
    want = z[name + "_dist"][:, :k]
    assert np.array_equal(np.isnan(dist), np.isnan(want)) and np.all((dist == want) | np.isnan(want)), name


_RANDOM = ec.random_cases()


@pytest.mark.parametrize("case", _RANDOM, ids=[c[0] for c in _RANDOM])
def test_random_case_matches_scipy_bit_for_bit(z, path, case):
    from columbiaimagesearch_amd.lopq import eval as ev
    name, d, m2, m1, dt = case
    q, data = ec.random_inputs(*case)
    idx, dist = ev.exact_neighbors(q, data, ec.K)
    _check(z, name, idx, dist)
    idx1, dist1 = ev.exact_neighbors(q, data, 1)
    _check(z, name, idx1, dist1, k=1)
    nn = ev.compute_all_neighbors(q, data)
    assert nn.shape == (m1,) and nn.dtype == np.int64 and np.array_equal(nn, z[name + "_idx"][:, 0])
    if m2 == 50:
        full = ev.compute_all_neighbors(q, data, just_nn=False)
        assert full.shape == (m1, 50) and np.array_equal(full, z[name + "_all"])


_ENGINEERED = ["e_dup", "e_dup_f4", "e_sqrt_d2", "e_sqrt_d66", "e_same"]


@pytest.mark.parametrize("name", _ENGINEERED)
def test_engineered_rows(z, path, name):
    from columbiaimagesearch_amd.lopq import eval as ev
    q, data = ec.engineered_inputs()[name]
    idx, dist = ev.exact_neighbors(q, data, ec.K)
    _check(z, name, idx, dist)
    assert np.array_equal(ev.compute_all_neighbors(q, data), z[name + "_idx"][:, 0])
    if name.startswith("e_sqrt"):
        assert idx[0, 0] == 0 and idx[0, 1] == 1 and dist[0, 0] == dist[0, 1]  # the farther row wins on the index
    if name == "e_same":
        assert np.array_equal(idx, np.tile(np.arange(ec.K), (3, 1)))
    if name.startswith("e_dup"):
        assert dist[1, 0] == 0.0 and idx[1, 0] == 17 and idx[0, 1] - idx[0, 0] == 7 and idx[0, 2] - idx[0, 0] == 12


def test_the_prefilter_discards_and_degenerate_rows_fall_back(z):
    """The default path really is a prefilter: on random rows no query needs the exact-only kernel and the survivors are a few per
    query (k = 10: at most 4k + 502 would fit the list); 2 000 identical rows overflow every query's list into the exact-only kernel."""
    from columbiaimagesearch_amd.lopq import eval as ev
    name = "r_d130_n4099_q257_f4"
    q, data = ec.random_inputs(name, 130, 4099, 257, "f4")
    idx, dist = ev.exact_neighbors(q, data, ec.K)
    n, n_exact, n_rescored = ev.exact_stats()
    print("prefilter: %d queries, %d through the exact-only kernel, %d rows re-scored" % (n, n_exact, n_rescored))
    _check(z, name, idx, dist)
    assert (n, n_exact) == (257, 0) and 257 * ec.K <= n_rescored <= 257 * 8 * ec.K
    q, data = ec.engineered_inputs()["e_same"]
    ev.exact_neighbors(q, data, ec.K)
    assert ev.exact_stats()[:2] == (3, 3)
    ev.set_exact_mode(exact_only=True)
    try:
        ev.exact_neighbors(q, data, ec.K)
        assert ev.exact_stats() == (3, 3, 0)
    finally:
        ev.set_exact_mode(exact_only=False)


def test_self_neighbours_of_the_data_itself(path):
    from columbiaimagesearch_amd.lopq import eval as ev
    q, _ = ec.random_inputs("self", 24, 1, 300, "f8")
    assert np.array_equal(ev.compute_all_neighbors(q), np.arange(300))


@pytest.mark.parametrize("cut", [1, 64, 1000, "uneven"])
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_chunked_accumulation_equals_one_call(z, path, cut, order):
    from columbiaimagesearch_amd import _lib
    name = "r_d5_n4099_q257_f4"
    q, data = ec.random_inputs(name, 5, 4099, 257, "f4")
    q, m2 = q[:33], data.shape[0]
    edges = [0, 1, 64, 1000, 1001, 2500, m2] if cut == "uneven" else [0, cut, m2]
    chunks = list(zip(edges[:-1], edges[1:]))
    if order == "reverse":
        chunks = chunks[::-1]
    idx = np.empty((len(q), ec.K), dtype=np.int64)
    dist = np.empty((len(q), ec.K))
    for n, (a, b) in enumerate(chunks):
        part = np.ascontiguousarray(data[a:b])
        _lib.check(_lib.lib().cis_exact_knn(_lib.ptr(part), _lib.dtype_code(part), b - a, data.shape[1], _lib.ptr(q), _lib.dtype_code(q),
                                            len(q), ec.K, a, int(n > 0), _lib.ptr(idx), _lib.ptr(dist)))
    assert np.array_equal(idx, z[name + "_idx"][:33]) and _bit_equal(dist, z[name + "_dist"][:33])


def test_exact_neighbors_chunk_argument_and_tensors(z, path):
    import torch
    from columbiaimagesearch_amd.lopq import eval as ev
    name = "r_d128_n1000_q257_f4"
    q, data = ec.random_inputs(name, 128, 1000, 257, "f4")
    idx, dist = ev.exact_neighbors(q, data, ec.K, chunk=300)
    _check(z, name, idx, dist)
    tq, td = torch.from_numpy(q).cuda(), torch.from_numpy(data).cuda()
    for chunk in (None, 333):
        ti, tdist = ev.exact_neighbors(tq, td, ec.K, chunk=chunk)
        assert ti.is_cuda and tdist.dtype == torch.float64
        _check(z, name, ti.cpu().numpy(), tdist.cpu().numpy())
    assert np.array_equal(ev.compute_all_neighbors(tq, td), z[name + "_idx"][:, 0])


@pytest.mark.parametrize("dq,dd", [("f4", "f8"), ("f8", "f4")])
def test_mixed_dtypes_promote_to_float64(path, dq, dd):
    from scipy.spatial.distance import cdist
    from columbiaimagesearch_amd.lopq import eval as ev
    q, data = ec.random_inputs("mixed", 24, 1000, 9, "f8")
    q, data = q.astype(dq), data.astype(dd)
    want = cdist(q, data)
    order = np.argsort(want, axis=1, kind="stable")[:, :ec.K]
    idx, dist = ev.exact_neighbors(q, data, ec.K)
    assert np.array_equal(idx, order) and _bit_equal(dist, np.take_along_axis(want, order, axis=1))


@pytest.mark.parametrize("dt", ["f4", "f8"])
def test_wide_vectors_d4096(path, dt):
    from scipy.spatial.distance import cdist
    from columbiaimagesearch_amd.lopq import eval as ev
    q, data = ec.random_inputs("wide", 4096, 300, 5, dt)
    want = cdist(q, data)
    order = np.argsort(want, axis=1, kind="stable")[:, :ec.K]
    idx, dist = ev.exact_neighbors(q, data, ec.K)
    assert np.array_equal(idx, order) and _bit_equal(dist, np.take_along_axis(want, order, axis=1))


def test_k_beyond_the_rows_is_padded_and_no_queries_is_fine(path):
    from columbiaimagesearch_amd.lopq import eval as ev
    q, data = ec.random_inputs("pad", 5, 7, 3, "f8")
    idx, dist = ev.exact_neighbors(q, data, 12)
    assert np.all(idx[:, 7:] == -1) and np.all(np.isnan(dist[:, 7:])) and np.all(np.sort(idx[:, :7], axis=1) == np.arange(7))
    assert np.all(np.diff(dist[:, :7], axis=1) >= 0)
    idx, dist = ev.exact_neighbors(q, data[:0], 4)  # no data: everything padded
    assert np.all(idx == -1) and np.all(np.isnan(dist))
    idx, dist = ev.exact_neighbors(q[:0], data, 4)  # m1 = 0
    assert idx.shape == (0, 4) and dist.shape == (0, 4)
    full = ev.compute_all_neighbors(q, np.repeat(data, 147, axis=0)[:1024], just_nn=False)  # k = m2 = 1024, 147-fold ties
    assert full.shape == (3, 1024) and np.array_equal(np.sort(full, axis=1), np.tile(np.arange(1024), (3, 1)))


def test_many_neighbours_k_1024(path):
    from scipy.spatial.distance import cdist
    from columbiaimagesearch_amd.lopq import eval as ev
    q, data = ec.random_inputs("many", 5, 3000, 2, "f4")
    want = cdist(q, data)
    order = np.argsort(want, axis=1, kind="stable")[:, :1024]
    idx, dist = ev.exact_neighbors(q, data, 1024)
    assert np.array_equal(idx, order) and _bit_equal(dist, np.take_along_axis(want, order, axis=1))


# ---- the six functions on the small model ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(z):
    from columbiaimagesearch_amd.lopq import LOPQModel
    nf = int(z["m_num_fine_splits"])
    subs = tuple([z["m_subs"][s, j] for j in range(nf)] for s in range(2))
    m = LOPQModel(parameters=((z["m_Cs"][0], z["m_Cs"][1]), (z["m_Rs"][0], z["m_Rs"][1]), (z["m_mus"][0], z["m_mus"][1]), subs))
    X, Q = ec.model_inputs()
    return m, X, Q


def test_model_functions_against_the_reference(z, small):
    from columbiaimagesearch_amd.lopq import eval as ev
    m, X, Q = small
    assert np.array_equal(ev.compute_all_neighbors(Q, X), z["m_nns"])
    h = ev.get_cell_histogram(X, m)
    assert h.shape == (15,) and np.array_equal(h, z["m_hist"])
    assert ev.get_proportion_nns_with_same_coarse_codes(X[:ec.N_SUB], m) == float(z["m_prop_nn"])
    assert ev.get_proportion_of_reconstructions_with_same_codes(X[:ec.N_SUB], m) == float(z["m_prop_recon"])
    dist = ev.get_subquantizer_distortion(X, m)
    err = np.max(np.abs(dist - z["m_distortion"]) / z["m_distortion"])
    print("subquantizer distortion: largest relative difference to the reference %.3g" % err)
    assert dist.shape == (8,) and err <= 1e-12


@pytest.mark.parametrize("normalize", [True, False])
def test_get_recall_through_search_batch(z, small, normalize):
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP, eval as ev
    m, X, Q = small
    s = LOPQSearcherHIP(m)
    coarse, fine = m.predict_batch(X)
    s.add_codes_array(coarse, fine)
    recall, t = ev.get_recall(s, Q, z["m_nns"], thresholds=ec.THRESHOLDS, normalize=normalize)
    assert np.array_equal(recall, z["m_recall_norm" if normalize else "m_recall_raw"]) and t > 0.0
    s.close()


def test_resident_features_search_exact(z):
    import torch
    from columbiaimagesearch_amd.rerank import ResidentFeatures
    name = "r_d128_n1000_q257_f4"
    q, data = ec.random_inputs(name, 128, 1000, 257, "f4")
    ids = [1000 + 3 * i for i in range(len(data))]
    rf = ResidentFeatures(torch.from_numpy(data).cuda(), ids)
    got_ids, dists = rf.search_exact(torch.from_numpy(q).cuda(), ec.K)
    assert np.array_equal(got_ids, 1000 + 3 * z[name + "_idx"].astype(np.int64)) and _bit_equal(dists, z[name + "_dist"])
    rows, _ = ResidentFeatures(torch.from_numpy(data).cuda()).search_exact(torch.from_numpy(q[:3].astype(np.float64)).cuda(), 2)
    want = np.argsort(np.sqrt(((q[:3, None, :].astype(np.float64) - data[None]) ** 2).sum(-1)), axis=1, kind="stable")[:, :2]
    assert np.array_equal(rows, want)
