"""lopq.eval without a GPU: the module resolves under the reference's name, keeps its signatures, and its host-side logic
(recall counting, cell histogram binning, argument checks) reproduces tests/golden/eval.npz -- outputs of the reference's eval.py."""
import inspect
import json
import os

import numpy as np
import pytest

import eval_cases as ec
from conftest import GOLDEN, has_gpu


@pytest.fixture(scope="module")
def z():
    return dict(np.load(os.path.join(GOLDEN, "eval.npz")))


def test_lopq_eval_resolves_after_install_as_lopq():
    import sys
    saved = {k: v for k, v in sys.modules.items() if k == "lopq" or k.startswith("lopq.")}
    try:
        from columbiaimagesearch_amd import lopq as ours
        ours.install_as_lopq()
        from lopq import eval as ev
        import lopq.eval as ev2
        assert ev is ev2 is ours.eval and "eval" in ours.__all__
    finally:
        for k in [k for k in sys.modules if k == "lopq" or k.startswith("lopq.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_signatures_are_the_references(z):
    from columbiaimagesearch_amd.lopq import eval as ev
    ref = json.loads(str(z["signatures"]))
    assert len(ref) == 6
    for name, params in ref.items():
        got = list(inspect.signature(getattr(ev, name)).parameters.values())
        if name == "compute_all_neighbors":  # k is this package's addition, after the reference's arguments
            assert got[-1].name == "k" and got[-1].default is None
            got = got[:-1]
        assert [p.name for p in got] == [p[0] for p in params], name
        for p, (_, default) in zip(got, params):
            if default is None:
                assert p.default is inspect.Parameter.empty, (name, p.name)
            else:
                assert p.default == default[1] and type(p.default) is type(default[1]), (name, p.name)


class _ReplaySearcher(object):
    """Duck-typed searcher without search_batch: hands back the reference's ranked ids, so get_recall takes its per-query loop."""

    def __init__(self, queries, results):
        self.rows = {q.tobytes(): r for q, r in zip(queries, results)}
        self.calls = []

    def search(self, x, quota=10, limit=None, with_dists=False):
        self.calls.append((quota, limit, with_dists))
        ids = self.rows[np.asarray(x).tobytes()]
        return [(int(i), None) for i in ids if i >= 0], 3


@pytest.mark.parametrize("normalize", [True, False])
def test_get_recall_per_query_path_reproduces_the_reference(z, normalize):
    from columbiaimagesearch_amd.lopq import eval as ev
    _, Q = ec.model_inputs()
    s = _ReplaySearcher(Q, z["m_results"])
    recall, t = ev.get_recall(s, Q, z["m_nns"], thresholds=ec.THRESHOLDS, normalize=normalize)
    assert isinstance(recall, np.ndarray) and np.array_equal(recall, z["m_recall_norm" if normalize else "m_recall_raw"])
    assert isinstance(t, float) and t >= 0.0
    assert s.calls == [(ec.THRESHOLDS[-1], None, False)] * len(Q)  # searcher.search(d, thresholds[-1])
    assert np.array_equal(z["m_recall_raw"], z["m_recall_norm"] * len(Q)) and z["m_recall_raw"][-1] > 0


class _BatchSearcher(object):
    """A searcher WITH search_batch: device ids are offset by 7 and map back through caller_ids."""

    def __init__(self, results):
        self.results, self.calls = results, []

    def search_batch(self, X, quota=10, limit=None, with_codes=False):
        self.calls.append((len(X), quota, limit))
        ids = np.where(self.results >= 0, self.results + 7, -1)
        return {"ids": ids, "n_found": (ids >= 0).sum(axis=1).astype(np.int32), "visited": np.ones(len(X), dtype=np.int32)}

    def caller_ids(self, dev_ids):
        return [int(i) - 7 for i in dev_ids if i >= 0]


def test_get_recall_batched_path_is_one_call_and_maps_ids_back(z):
    from columbiaimagesearch_amd.lopq import eval as ev
    _, Q = ec.model_inputs()
    s = _BatchSearcher(z["m_results"])
    recall, _ = ev.get_recall(s, Q, z["m_nns"], thresholds=ec.THRESHOLDS)
    assert s.calls == [(len(Q), 100, 100)]
    assert np.array_equal(recall, z["m_recall_norm"])


def test_cell_histogram_keeps_the_references_bins():
    from columbiaimagesearch_amd.lopq import eval as ev

    class Stub(object):
        V = 4

        def predict_coarse(self, x):
            return np.asarray(x, dtype=np.uint8)[:, :2]

    cells = [0, 0, 5, 14, 14, 15, 15, 15, 3]
    data = np.array([[c // 4, c % 4, 9] for c in cells], dtype=np.float64)
    h = ev.get_cell_histogram(data, Stub())
    assert h.shape == (15,)  # bins=range(16): 15 bins, the last one closed on both sides
    want = np.zeros(15, dtype=np.int64)
    want[0], want[3], want[5], want[14] = 2, 1, 1, 5
    assert np.array_equal(h, want)
    Stub.V = 20  # cell ids beyond uint8: no wrap-around
    data = np.array([[19, 19, 0], [13, 0, 0]], dtype=np.float64)
    h = ev.get_cell_histogram(data, Stub())
    assert h.shape == (399,) and h[398] == 1 and h[260] == 1 and h.sum() == 2


def test_proportion_with_same_coarse_codes_uses_given_neighbours():
    from columbiaimagesearch_amd.lopq import eval as ev

    class Stub(object):
        def predict_coarse(self, x):
            return np.asarray(x, dtype=np.uint8)[:, :2]

    data = np.array([[0, 1], [0, 1], [2, 1], [2, 3]], dtype=np.float64)
    assert ev.get_proportion_nns_with_same_coarse_codes(data, Stub(), nns=np.array([1, 0, 3, 2])) == 0.5


def test_argument_errors_need_no_device():
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.lopq import eval as ev
    a = np.zeros((3, 4))
    with pytest.raises(NotImplementedError, match="1024"):
        ev.exact_neighbors(a, a, 1025)
    with pytest.raises(NotImplementedError, match="1024"):
        ev.compute_all_neighbors(a, np.zeros((1025, 4)), just_nn=False)
    with pytest.raises(ValueError):
        ev.exact_neighbors(a, np.zeros((3, 5)), 1)
    with pytest.raises(ValueError):
        ev.exact_neighbors(a, a, 0)
    idx, dist = np.zeros((3, 1), dtype=np.int64), np.zeros((3, 1))
    L = _lib.lib()
    for dt1, dt2 in ((2, 8), (8, 16), (0, 4)):
        with pytest.raises(ValueError, match="dtype"):
            _lib.check(L.cis_exact_knn(_lib.ptr(a), dt1, 3, 4, _lib.ptr(a), dt2, 3, 1, 0, 0, _lib.ptr(idx), _lib.ptr(dist)))
        with pytest.raises(ValueError, match="dtype"):
            _lib.check(L.cis_exact_knn_dev(None, dt1, 3, 4, None, dt2, 3, 1, 0, 0, None, None, None))
    with pytest.raises(ValueError):
        _lib.check(L.cis_exact_knn_set_mode(2))
    with pytest.raises(ValueError):
        _lib.check(L.cis_exact_knn(_lib.ptr(a), 8, 3, 0, _lib.ptr(a), 8, 3, 1, 0, 0, _lib.ptr(idx), _lib.ptr(dist)))


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU failure mode")
def test_no_gpu_means_loud_failure_not_fallback():
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.lopq import eval as ev
    a = np.random.RandomState(0).standard_normal((5, 4))
    with pytest.raises(_lib.HipError):
        ev.compute_all_neighbors(a)
    with pytest.raises(_lib.HipError):
        ev.exact_neighbors(a, a, 2)


def test_fixture_inputs_match_their_checksums(z):
    for name, d, m2, m1, dt in ec.random_cases():
        q, data = ec.random_inputs(name, d, m2, m1, dt)
        assert str(z[name + "_sha1"]) == ec.sha1(q) + ec.sha1(data), name
        assert z[name + "_idx"].shape == (m1, ec.K) and z[name + "_dist"].dtype == np.float64
    for name, (q, data) in ec.engineered_inputs().items():
        assert str(z[name + "_sha1"]) == ec.sha1(q) + ec.sha1(data), name
    X, Q = ec.model_inputs()
    assert str(z["m_inputs_sha1"]) == ec.sha1(X) + ec.sha1(Q)
