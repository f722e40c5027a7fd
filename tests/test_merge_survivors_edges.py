"""k_merge_survivors at its edges: the survivor merge of the fast scans (exact re-scoring of what the float32 / 16-bit scan let
through, ranking by (distance, visit rank, position)) against the oracle on small synthetic indexes.

The cases are chosen where the kernel takes another path: one wave per query (nq = 1, 5, 67, 128: the `q >= nq` exit and a partial
last workgroup), passes of 64 re-scored candidates and the padding to the sort size (limit = 1, 63, 64, 65, 100, 128), 1 / 2 / 4
lists per query (the fast path, four or eight survivors per lane) and 5 / 8 lists (the general rounds), fewer candidates than
`limit` (padding rows), a visited cell that holds nothing, and a crowd of identical vectors (more than 256 equal float32 distances
at the cut: ties break by (visit rank, position), and the fast path, where it is entered, has to give up).  Every case asserts, from
the oracle's own walk, what the oracle can see of it: lists per query, candidates, empty cells, the crowd; which path of the kernel a
query then takes follows from the launcher's rules and is not observed.

Bars: ids, n_found and visited exact; distances within 1e-9 relative (the bar of test_lopq_hip_parity.py)."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

LIMITS = (1, 63, 64, 65, 100, 128)
NQS = (1, 5, 67, 128)
LMAX = max(LIMITS)


@pytest.fixture(autouse=True, params=["prefilter", "scan3", "scan4", "scan5"])
def route(request):
    """The routes that hand survivors to k_merge_survivors whatever the batch size: "prefilter" (k_adc_scan2: survivors carry float32
    distances), "scan3" / "scan4" / "scan5" (the 16-bit kernels: survivors carry sums, bounded through item_slack)."""
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    LOPQSearcherHIP.default_prefilter_only = request.param == "prefilter"
    LOPQSearcherHIP.default_scan_mode = {"scan3": 3, "scan4": 4, "scan5": 5}.get(request.param, 0)
    yield request.param
    LOPQSearcherHIP.default_prefilter_only = False
    LOPQSearcherHIP.default_scan_mode = 0


# ---- the indexes (host only: the oracle's codes, so that the cases do not depend on the GPU encoder) ----------------------------

_built = {}


def _tiny_codes():
    """20 000 seeded vectors encoded with the `tiny` model (V = 4: 16 cells, M = 4), and 128 queries."""
    if "tiny_codes" not in _built:
        from oracle import lopq_oracle as O
        z, _, _ = load_golden("tiny")
        om = O.OracleModel.from_npz(z)
        rs = np.random.RandomState(2024)
        X = rs.randn(20000, 8)
        Q = rs.randn(128, 8)
        coarse, fine = O.compute_codes(om, X)
        _built["tiny_codes"] = (om, X, Q, np.asarray(coarse), np.asarray(fine))
    return _built["tiny_codes"]


def _take_per_cell(coarse, sizes):
    """indices of the first sizes[cell] vectors of every cell, in their original order"""
    cell = coarse[:, 0].astype(np.int64) * 4 + coarse[:, 1]
    keep = np.zeros(len(cell), dtype=bool)
    for c, n in enumerate(sizes):
        idx = np.flatnonzero(cell == c)
        assert len(idx) >= n, (c, len(idx), n)
        keep[idx[:n]] = True
    return np.flatnonzero(keep)


def index_even():
    """16 cells of exactly 256 vectors (4096 in all): a quota of k * 256 + 1 makes every query visit exactly k + 1 lists."""
    om, X, Q, coarse, fine = _tiny_codes()
    sel = _take_per_cell(coarse, [256] * 16)
    return om, coarse[sel], fine[sel], Q


def index_ragged():
    """Cells of 0, 30 and 700 vectors (4 empty, 6 short, 6 long: 4380 in all): small quotas end inside a short cell with fewer candidates
    than `limit`, and walks cross cells that hold nothing."""
    om, X, Q, coarse, fine = _tiny_codes()
    sel = _take_per_cell(coarse, [700, 30, 0, 700, 30, 700, 30, 0, 700, 0, 700, 30, 30, 700, 30, 0])
    return om, coarse[sel], fine[sel], Q


def index_crowd():
    """The even index plus 320 more copies of its first vector: one cell holds 321 identical codes.  The queries are that vector, slightly
    perturbed, so the crowd is what is nearest to them."""
    om, X, Q, coarse, fine = _tiny_codes()
    sel = _take_per_cell(coarse, [256] * 16)
    rs = np.random.RandomState(7)
    coarse_c = np.concatenate([coarse[sel], np.repeat(coarse[sel[:1]], 320, axis=0)])
    fine_c = np.concatenate([fine[sel], np.repeat(fine[sel[:1]], 320, axis=0)])
    Qc = X[sel[0]][None, :] + 0.01 * rs.randn(8, 8)
    return om, coarse_c, fine_c, Qc


def index_c4():
    """The first 32 000 vectors of the `c4` fixture (LOPQModelPCA 128 -> 128, renorm, V = 16, M = 8, K = 256) under their golden codes:
    256 cells of about 125 vectors; the fixture's 64 queries."""
    from oracle import lopq_oracle as O
    z, _, Q = load_golden("c4")
    if "c4_model" not in _built:
        _built["c4_model"] = O.OracleModel.from_npz(z)
    return _built["c4_model"], z["coarse"][:32000], z["fine"][:32000], Q


INDEXES = {"even": index_even, "ragged": index_ragged, "crowd": index_crowd, "c4": index_c4}


def walk(oi, x, quota):
    """(non-empty cells visited, cells visited, candidates) of the oracle's walk for one query: OracleCSRIndex.search's own loop"""
    from oracle import lopq_oracle as O
    m = oi.model
    if m.has_pca:
        x = O.apply_pca(m, x)
    lists, visited, n = 0, 0, 0
    for _, (c0, c1) in O.multisequence(m, x):
        cid = int(c0) * m.V + int(c1)
        size = int(oi.offsets[cid + 1] - oi.offsets[cid])
        visited += 1
        lists += size > 0
        n += size
        if n >= quota:
            break
    return lists, visited, n


def reference(name, quota):
    """Per query of index `name`: the oracle's (ids, dists, visited) at limit 128 -- a smaller limit is a prefix of it (stable sort) --
    and its walk.  Computed once."""
    key = ("ref", name, quota)
    if key not in _built:
        from oracle import lopq_oracle as O
        om, coarse, fine, Q = INDEXES[name]()
        if ("oi", name) not in _built:
            _built[("oi", name)] = O.OracleCSRIndex(om, coarse, fine)
        oi = _built[("oi", name)]
        _built[key] = ([oi.search(Q[qi], quota=quota, limit=LMAX) for qi in range(len(Q))], [walk(oi, Q[qi], quota) for qi in range(len(Q))])
    return _built[key]


def searcher(name, route):
    """one searcher per (index, route): the route is fixed when a searcher is made"""
    key = ("hip", name, route)
    if key not in _built:
        from test_lopq_hip_parity import hip_model
        from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
        z, _, _ = load_golden("c4" if name == "c4" else "tiny")
        _, coarse, fine, _ = INDEXES[name]()
        s = LOPQSearcherHIP(hip_model(z))
        s.add_codes_array(coarse, fine)
        _built[key] = s
    return _built[key]


def check(name, route, quota, limit, nq):
    import torch
    want, _ = reference(name, quota)
    Q = INDEXES[name]()[3]
    s = searcher(name, route)
    out = s.search_batch_dev(torch.as_tensor(np.ascontiguousarray(Q[:nq])).cuda(), quota=quota, limit=limit)
    r = {k: v.cpu().numpy() for k, v in out.items()}
    assert r["ids"].shape == (nq, limit)
    for qi in range(nq):
        ids, dists, visited = want[qi]
        k = min(len(ids), limit)
        where = (name, route, quota, limit, nq, qi)
        assert int(r["n_found"][qi]) == k and int(r["visited"][qi]) == visited, where
        np.testing.assert_array_equal(r["ids"][qi, :k], ids[:k], err_msg=str(where))
        np.testing.assert_allclose(r["dists"][qi, :k], dists[:k], rtol=1e-9, atol=0, err_msg=str(where))
        # the rows past the last hit: id -1 and a NaN distance, as every release wrote them
        assert (r["ids"][qi, k:] == -1).all() and np.isnan(r["dists"][qi, k:]).all(), where


# ---- the cases ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lists", [1, 2, 4, 5, 8])
def test_lists_per_query(route, lists):
    """Exactly `lists` lists for every query (even index): 1 -> four survivors per lane; 2 and 4 -> the work items exceed 1.25 nq, eight per
    lane; 5 and 8 -> the general rounds.  Every limit at nq = 128, every nq at limit = 100."""
    quota = (lists - 1) * 256 + 1
    _, walks = reference("even", quota)
    assert all(w[0] == lists and w[1] == lists for w in walks)  # the case is what it says
    for limit in LIMITS:
        check("even", route, quota, limit, 128)
    for nq in NQS[:-1]:
        check("even", route, quota, 100, nq)


@pytest.mark.parametrize("quota", [10, 40, 800])
def test_short_and_empty_cells(route, quota):
    """Ragged index: queries with fewer candidates than `limit` (padding rows), walks over cells that hold nothing, and list counts that
    differ from query to query in one batch."""
    want, walks = reference("ragged", quota)
    few = sum(1 for w in walks if w[2] < 100)
    empty = sum(1 for w in walks if w[1] > w[0])
    assert empty >= 10, empty  # queries that visit an empty cell
    if quota <= 40:
        assert few >= 10, few  # queries with fewer than 100 candidates in all
        assert any(len(ids) < 63 for ids, _, _ in want) and any(len(ids) >= 128 for ids, _, _ in want)
    else:
        assert len({w[0] for w in walks}) >= 3 and max(w[0] for w in walks) >= 5  # fast path and general rounds side by side
    for limit in LIMITS:
        check("ragged", route, quota, limit, 128)
    for nq in NQS[:-1]:
        check("ragged", route, quota, 100, nq)


@pytest.mark.parametrize("quota", [1, 600])
def test_crowd_of_equal_distances(route, quota):
    """321 identical codes in the nearest cell: at limit <= 128 the cut falls inside the crowd, so the hits are the crowd's first `limit`
    members in insertion order (ties: visit rank, position).  Asserted from the oracle: the 321 equal distances come first.  Not
    asserted, because the oracle cannot see it: which path of the kernel ranks them.  A float32 cut inside 321 equal keys keeps more
    than 256 entries (`kept > CAPM`, on to the general rounds) when the scan hands over at most 256 / 512 survivors in all; when it
    hands over more, the fast path is not entered and the general rounds rank the crowd from the start."""
    Q = index_crowd()[3]
    reference("crowd", quota)
    oi = _built[("oi", "crowd")]
    for qi in range(len(Q)):
        ids, dists, _ = oi.search(Q[qi], quota=quota, limit=400)
        assert (dists[:321] == dists[0]).all() and len(set(ids[:321].tolist()) - {0} - set(range(4096, 4416))) == 0, qi  # the crowd comes first
    for limit in LIMITS:
        check("crowd", route, quota, limit, len(Q))
    check("crowd", route, quota, 100, 1)


@pytest.mark.parametrize("quota", [1, 300, 1000])
def test_m8_with_pca(route, quota):
    """The C4 model (M = 8, PCA, K = 256) on 32 000 vectors: one list per query (quota 1), a few (300) and the general rounds (1000)."""
    _, walks = reference("c4", quota)
    n = [w[0] for w in walks]
    if quota == 1:
        assert max(n) == 1
    elif quota == 300:
        assert min(n) >= 2 and sum(1 for v in n if v <= 4) >= 16, sorted(n)
    else:
        assert sum(1 for v in n if v >= 5) >= 48, sorted(n)
    for limit in LIMITS:
        check("c4", route, quota, limit, 64)
    for nq in (1, 5, 63):
        check("c4", route, quota, 100, nq)
