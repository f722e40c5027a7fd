"""GPU: the small-V front end (csrc/lopq_plan.hip) walks each query once and fills the wave.

k_front_small computes the coarse distances, ranks them and walks the multisequence for several queries per wave, and lists the
visited cells that hold candidates (VIS_CAP = 8 records per query, csrc/lopq_batch.h); k_emit_rec writes the work items and table
descriptors from that list, and walks again only a query whose list overflowed.  The reference is the oracle
(oracle/lopq_oracle.py: multisequence, OracleCSRIndex.search), never the code under test.

Every world is a few thousand random codes placed directly into chosen cells of an untrained model (test_lopq_hip_parity._random_model),
so the cells' sizes are the test's own.  Each search runs on both routes of a small batch (the all-candidates path, which sizes the batch
by bounds, and the prefilter scan, which reads the plan totals back).
"""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

VIS_CAP = 8  # csrc/lopq_batch.h
M, K = 4, 16
NQS = (1, 3, 7, 65)  # a partly filled workgroup; an odd count with two queries per wave (V = 16); more than one workgroup


class World(object):
    def __init__(self, V, D, dtype, sizes, seed, dup_rows=()):
        """sizes: [V * V] items per cell.  dup_rows: (split, src, dst) -- centroid row dst of that half is a copy of row src."""
        from oracle import lopq_oracle as O
        from columbiaimagesearch_amd.lopq import LOPQModel, LOPQSearcherHIP
        rs = np.random.RandomState(seed)
        h, w, nf = D // 2, D // M, M // 2
        Cs = [rs.randn(V, h).astype(dtype) for _ in range(2)]
        for s, a, b in dup_rows:
            Cs[s][b] = Cs[s][a]
        Rs = [np.stack([np.linalg.qr(rs.randn(h, h))[0] for _ in range(V)]) for _ in range(2)]
        mus = [rs.randn(V, h) * 0.05 for _ in range(2)]
        subs = [[rs.randn(K, w) * 0.6 for _ in range(nf)] for _ in range(2)]
        self.Q = rs.randn(max(NQS), D).astype(dtype)  # (drawn before the items: the same for every set of sizes)
        self.V, self.D, self.dtype = V, D, dtype
        self.om = O.OracleModel(Cs, Rs, mus, subs)
        self.sizes = np.asarray(sizes, dtype=np.int64)
        cell = rs.permutation(np.repeat(np.arange(V * V), self.sizes))  # insertion order mixes the cells
        self.cell = cell
        coarse = np.stack([cell // V, cell % V], axis=1).astype(np.uint8)
        fine = rs.randint(0, K, size=(len(cell), M)).astype(np.uint8)
        self.oi = O.OracleCSRIndex(self.om, coarse, fine)
        self.s = LOPQSearcherHIP(LOPQModel(parameters=(tuple(Cs), tuple(Rs), tuple(mus), tuple(subs))))
        self.s.add_codes_array(coarse, fine)
        self._want = {}

    def centre(self, c0, c1):
        """A query whose nearest cell is (c0, c1)."""
        return np.concatenate([self.om.Cs[0][c0], self.om.Cs[1][c1]]).astype(self.dtype)

    def nonempty_visited(self, x, quota):
        """Non-empty cells the oracle's walk visits for x (what the front end has to list)."""
        from oracle import lopq_oracle as O
        n = got = 0
        for _, (c0, c1) in O.multisequence(self.om, x):
            sz = int(self.sizes[int(c0) * self.V + int(c1)])
            n += sz > 0
            got += sz
            if got >= quota:
                break
        return n

    def want(self, Q, qi, quota, limit):
        key = (id(Q), qi, quota, limit)
        if key not in self._want:
            self._want[key] = self.oi.search(Q[qi], quota=quota, limit=limit)
        return self._want[key]

    def check(self, Q, nq, quota, limit, routes=(False, True)):
        for prefilter in routes:
            self.s.set_scan_mode(prefilter_only=prefilter)
            r = self.s.search_batch(Q[:nq], quota=quota, limit=limit)
            for qi in range(nq):
                ids, dists, visited = self.want(Q, qi, quota, limit)
                n = len(ids)
                assert int(r["visited"][qi]) == visited, "visited cells (query %d, quota %d, prefilter %s)" % (qi, quota, prefilter)
                assert int(r["n_found"][qi]) == n
                np.testing.assert_array_equal(r["ids"][qi, :n], ids)
                np.testing.assert_allclose(r["dists"][qi, :n], dists, rtol=1e-9, atol=1e-12)
        self.s.set_scan_mode(prefilter_only=False)


_worlds = {}


def world(name, *a, **kw):
    if name not in _worlds:
        _worlds[name] = World(*a, **kw)
    return _worlds[name]


def _flagged(err):
    """(flagged, queries) of every batch, from the CIS_DEBUG_PLAN lines of the front end."""
    return [(int(a), int(b)) for a, b in re.findall(r"k_front_small: (\d+) of (\d+) queries fall back", err)]


# V = 4: eight queries per wave; V = 16: two, every lane on a distance (the benchmark's shape at h = 64, centroids staged in LDS for
# both types); V = 64 float32 at h = 8: one query per wave in two trips, staged; V = 64 float64 at h = 64: 64 KB of centroids, read in place
SWEEP = [(4, 16, np.float32), (4, 16, np.float64), (16, 128, np.float32), (16, 128, np.float64), (64, 16, np.float32), (64, 128, np.float64)]


@pytest.mark.parametrize("V,D,dtype", SWEEP, ids=lambda v: getattr(v, "__name__", str(v)))
def test_v_sweep(V, D, dtype):
    rs = np.random.RandomState(V)
    n = 3000
    sizes = np.bincount(rs.randint(0, V * V, size=n), minlength=V * V)  # V = 64: most cells hold one item or none
    w = world(("sweep", V, D, dtype), V, D, dtype, sizes, seed=100 + V)
    for nq in NQS:
        w.check(w.Q, nq, quota=150, limit=40)


def test_coarse_distance_ties_rank_the_lower_index_first(monkeypatch):
    V, D = 16, 128
    dups = ((0, 2, 5), (0, 2, 9), (1, 7, 3))
    w = world("ties", V, D, np.float32, np.full(V * V, 12), seed=7, dup_rows=dups)
    from oracle import lopq_oracle as O

    def stable_rank(model, x):
        """O.coarse_rank with the tie rule written out: np.argsort's default sort leaves the order of equal distances to the numpy
        build, the library ranks the lower index first, as kind="stable" does."""
        dists = [O._sqdist_rows(np.ascontiguousarray(cx), model.Cs[s]) for s, cx in enumerate(O.split_halves(x, len(model.Cs)))]
        return dists, [np.argsort(d, kind="stable") for d in dists]

    monkeypatch.setattr(O, "coarse_rank", stable_rank)
    # queries at the duplicated centroids: the tied rows are the nearest, so every quota below cuts among their cells
    Q = np.stack([w.centre(2, 7), w.centre(9, 3), w.centre(5, 0)] + list(w.Q[:4]))
    for x in Q:
        d = O.coarse_rank(w.om, x)[0]
        assert d[0][2] == d[0][5] == d[0][9] and d[1][7] == d[1][3]
    for quota in (12, 13, 30, 60, 73):
        w.check(Q, len(Q), quota=quota, limit=quota)


def test_quota_cuts():
    V, D, per = 4, 16, 50
    w = world("quota", V, D, np.float32, np.full(V * V, per), seed=11)
    # on a cell boundary, one past it, two cells, larger than the index (all 16 cells), one candidate
    for quota in (per, per + 1, 2 * per, V * V * per + 10, 1):
        w.check(w.Q, 7, quota=quota, limit=min(quota, 120))


def test_empty_cells_are_visited_and_emit_nothing():
    V, D = 4, 16
    sizes = np.full(V * V, 40)
    sizes[[0, 3, 5, 6, 9, 10, 12, 15]] = 0
    w = world("empty", V, D, np.float64, sizes, seed=13)
    Q = np.stack([w.centre(0, 0), w.centre(1, 1), w.centre(3, 3)] + list(w.Q[:4]))  # nearest cell empty for the first three
    from oracle import lopq_oracle as O
    for x in Q[:3]:
        c0, c1 = next(O.multisequence(w.om, x))[1]
        assert sizes[int(c0) * V + int(c1)] == 0
    for quota in (1, 40, 41, 200):
        w.check(Q, len(Q), quota=quota, limit=min(quota, 100))
        assert any(w.want(Q, qi, quota, min(quota, 100))[2] > w.nonempty_visited(Q[qi], quota) for qi in range(3))


def test_recorded_list_overflows(monkeypatch, capfd):
    """One item in every cell of V = 64: a quota of q visits q non-empty cells.  VIS_CAP of them fit the list; with one more the query is
    flagged and the emit pass walks it again."""
    V, D = 64, 16
    w = world("overflow", V, D, np.float32, np.ones(V * V, dtype=np.int64), seed=17)
    monkeypatch.setenv("CIS_DEBUG_PLAN", "1")
    for quota, flagged in ((VIS_CAP, 0), (VIS_CAP + 1, 65), (40, 65)):
        capfd.readouterr()
        w.check(w.Q, 65, quota=quota, limit=quota)
        assert all(w.nonempty_visited(x, quota) == quota for x in w.Q[:65])
        got = _flagged(capfd.readouterr().err)
        assert got and all(g == (flagged, 65) for g in got), got


def test_one_flagged_query_in_a_batch(monkeypatch, capfd):
    """Cells of 9 items, except the VIS_CAP + 1 cells nearest to one query, which hold one: at quota 9 that query visits all of them."""
    from oracle import lopq_oracle as O
    V, D, quota = 64, 16, VIS_CAP + 1
    probe = World(V, D, np.float32, np.zeros(V * V, dtype=np.int64), seed=19)  # the same model and queries, no items: for the walk
    target = 64
    sizes = np.full(V * V, quota)
    walk = O.multisequence(probe.om, probe.Q[target])
    for _ in range(VIS_CAP + 1):
        c0, c1 = next(walk)[1]
        sizes[int(c0) * V + int(c1)] = 1
    w = world("one_flagged", V, D, np.float32, sizes, seed=19)
    np.testing.assert_array_equal(w.Q, probe.Q)
    n_vis = [w.nonempty_visited(x, quota) for x in w.Q[:65]]
    assert n_vis[target] == VIS_CAP + 1 and sum(n > VIS_CAP for n in n_vis) == 1
    monkeypatch.setenv("CIS_DEBUG_PLAN", "1")
    capfd.readouterr()
    w.check(w.Q, 65, quota=quota, limit=quota)
    got = _flagged(capfd.readouterr().err)
    assert got and all(g == (1, 65) for g in got), got


def test_chunks_tile_their_cell(monkeypatch):
    """Cells shorter than, at, one past and several times the chunk length: with limit = quota = the cell's length every candidate of the
    cell comes back, so the work items' (start, len) tile it exactly."""
    V, D, seg = 4, 16, 64
    lens = {0: 1, 1: seg - 1, 2: seg, 3: seg + 1, 4: 2 * seg, 5: 2 * seg + 1, 6: 3 * seg + 5, 7: 6 * seg, 8: 6 * seg + 50}
    sizes = np.full(V * V, 7)
    for c, n in lens.items():
        sizes[c] = n
    w = world("chunks", V, D, np.float32, sizes, seed=23)
    monkeypatch.setenv("CIS_SEG_MAX", str(seg))
    for c, n in lens.items():
        Q = np.stack([w.centre(c // V, c % V), w.centre((c + 1) // V % V, (c + 1) % V)])
        w.check(Q, 2, quota=n, limit=n)
        ids = w.want(Q, 0, n, n)[0]
        np.testing.assert_array_equal(np.sort(ids), np.flatnonzero(w.cell == c))
