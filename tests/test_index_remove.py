"""GPU tests of removal by id (csrc/lopq_remove.hip, LOPQSearcherHIP.remove_ids[_dev], ShardedSearcher.remove_ids_dev).

The defining property: after remove(S) the index is indistinguishable from one built by the same insert calls with the items whose
id is in S filtered out of every batch -- so the expected side is always the oracle's dict index (oracle/lopq_oracle.py:OracleIndex)
fed the filtered batches; a second LOPQSearcherHIP built from the filtered batches is an extra, bit-for-bit check where stated.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

# csrc/lopq_remove.hip: RM_LDS_MAX -- up to this many ids the removal set is a sorted list in LDS, beyond it a hash table in HBM
N_SWITCH = 1024
# csrc/lopq_remove.hip: RM_CHUNK -- items a compaction workgroup moves per round (larger than 2048: a cell of two chunks plus three)
CHUNK = 4096


def _model(name):
    from test_lopq_hip_parity import hip_model
    z, X, Q = load_golden(name)
    return hip_model(z), z, X, Q


def _oracle_index(z):
    from oracle import lopq_oracle as O
    return O.OracleIndex(O.OracleModel.from_npz(z))


def _cell_counts(s):
    from columbiaimagesearch_amd import _lib
    V = s.model.V
    c = np.zeros(V * V, dtype=np.int64)
    _lib.check(_lib.lib().cis_index_cell_counts(s._ix, _lib.ptr(c)))
    return c


def _oracle_counts(oi, V):
    c = np.zeros(V * V, dtype=np.int64)
    for (a, b), items in oi.cells.items():
        c[a * V + b] = len(items)
    return c


def _assert_equals_oracle(s, oi, V, cells=None):
    from test_index_insert import _assert_same_cells
    _assert_same_cells(s, oi, V, cells)
    assert s.get_nb_indexed() == oi.nb_indexed
    np.testing.assert_array_equal(_cell_counts(s), _oracle_counts(oi, V))


def _filtered_oracle(make_oracle, batches):
    """batches: [(coarse, fine, ids, removed-after set or None)] -> the oracle fed every batch without the ids removed after it"""
    oi = make_oracle()
    for coarse, fine, ids, gone in batches:
        ids = np.asarray(ids, dtype=object) if not isinstance(ids, np.ndarray) else ids
        keep = np.array([i not in gone for i in ids.tolist()], dtype=bool) if gone else np.ones(len(ids), dtype=bool)
        oi.add_codes_arrays(coarse[keep], fine[keep], [i for i, k in zip(ids.tolist(), keep) if k])
    return oi


def _cuda(ids):
    import torch
    return torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int64)).cuda()


# ---- cell sizes on every chunk edge ------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4100, 2 * CHUNK + 3]


def _runs(n, mult):
    kill = np.zeros(n, dtype=bool)
    for m in range(mult, n, mult):  # a run of 70 straddling every multiple of `mult` inside the cell
        kill[max(m - 35, 0):min(m + 35, n)] = True
    return kill


PATTERNS = [
    ("first", lambda n: np.arange(n) == 0),
    ("last", lambda n: np.arange(n) == n - 1),
    ("all", lambda n: np.ones(n, dtype=bool)),
    ("none", lambda n: np.zeros(n, dtype=bool)),
    ("every other", lambda n: np.arange(n) % 2 == 0),
    ("all but one", lambda n: np.arange(n) != n // 2),
    ("runs at 64", lambda n: _runs(n, 64)),
    ("runs at 256", lambda n: _runs(n, 256)),
    ("runs at 1024", lambda n: _runs(n, 1024)),
    ("runs at the chunk", lambda n: _runs(n, CHUNK)),
]


def _edge_model(which):
    if which == "bytes":  # M = 6: the byte-wise code move
        from oracle import lopq_oracle as O
        from test_lopq_hip_parity import _random_model
        m, om = _random_model(4, 6, 16, 24, seed=3)
        return m, (lambda: O.OracleIndex(om)), 16
    m, z, X, Q = _model(which)  # tiny: M = 4 (one code word), c2: M = 8 (two)
    return m, (lambda: _oracle_index(z)), m.subquantizer_clusters


@pytest.mark.parametrize("which", ["c2", "tiny", "bytes"])
def test_cells_on_every_chunk_edge(which):
    """One cell per size, every removal pattern on every size (the patterns rotate over the cells from round to round)."""
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    assert SIZES[-1] == 2 * CHUNK + 3 and CHUNK > 2048
    m, make_oracle, K = _edge_model(which)
    V, M = m.V, m.M
    assert V * V >= len(SIZES)
    rs = np.random.RandomState(7)
    cell_of = np.repeat(np.arange(len(SIZES)), SIZES)
    n = cell_of.shape[0]
    order = rs.permutation(n)  # arrival order: the cells interleaved
    cell_of = cell_of[order]
    coarse = np.stack([cell_of // V, cell_of % V], axis=1).astype(np.uint16)
    fine = rs.randint(0, K, size=(n, M)).astype(np.uint8)
    ids = rs.permutation(n).astype(np.int64) * 5 + 2  # unique, not monotone
    pos_in_cell = np.zeros(n, dtype=np.int64)
    for c in range(len(SIZES)):
        sel = np.nonzero(cell_of == c)[0]
        pos_in_cell[sel] = np.arange(sel.shape[0])
    cells = [(c // V, c % V) for c in range(V * V)]
    for rnd in range(len(PATTERNS)):
        kill = np.zeros(n, dtype=bool)
        for c, size in enumerate(SIZES):
            sel = np.nonzero(cell_of == c)[0]
            kill[sel] = PATTERNS[(c + rnd) % len(PATTERNS)][1](size)[pos_in_cell[sel]]
        gone = ids[kill]
        s = LOPQSearcherHIP(m)
        assert s.add_codes_array(coarse, fine, ids) == n
        removed = s.remove_ids(rs.permutation(gone)) if rnd % 2 else s.remove_ids_dev(_cuda(rs.permutation(gone)))
        assert removed == int(kill.sum()), rnd
        oi = _filtered_oracle(make_oracle, [(coarse, fine, ids, set(gone.tolist()))])
        _assert_equals_oracle(s, oi, V, cells)
        s.close()


# ---- id edge cases -----------------------------------------------------------------------------------------------------------
def test_id_edge_cases():
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    m, z, X, Q = _model("tiny")
    V, M, K = m.V, m.M, m.subquantizer_clusters
    rs = np.random.RandomState(1)
    big = (1 << 62) - 1

    def cells_of(pairs):
        return np.array(pairs, dtype=np.uint16)

    # batch A (dedup): id 7 in three cells, id 0, the largest integer id, non-integer ids (slots at 2^62 + k)
    ids_a = [7, 11, 7, 12, 7, 0, big, "a", "b", "t1", 13, 14]
    coarse_a = cells_of([(0, 0), (0, 0), (0, 1), (0, 1), (1, 0), (1, 0), (1, 0), (2, 2), (2, 2), (2, 2), (2, 2), (0, 0)])
    fine_a = rs.randint(0, K, size=(len(ids_a), M)).astype(np.uint8)
    # batch B (dedup = False): id 9 three times in ONE cell, between other items
    ids_b = [21, 9, 22, 9, 9, 23]
    coarse_b = cells_of([(0, 0)] * 6)
    fine_b = rs.randint(0, K, size=(6, M)).astype(np.uint8)
    s = LOPQSearcherHIP(m)
    assert s.add_codes_array(coarse_a, fine_a, ids_a) == len(ids_a)
    assert s.add_codes_array(coarse_b, fine_b, np.array(ids_b), dedup=False) == 6
    assert [i for i, _ in s.get_cell((0, 0))] == [7, 11, 14, 21, 9, 22, 9, 9, 23]
    gone = set()

    def check():
        oi = _filtered_oracle(lambda: _oracle_index(z), [(coarse_a, fine_a, np.array(ids_a, dtype=object), gone),
                                                          (coarse_b, fine_b, np.array(ids_b, dtype=object), gone)])
        _assert_equals_oracle(s, oi, V)

    # every copy inside a cell (the oracle cannot hold the copies: it is compared once they are gone)
    assert s.remove_ids([9]) == 3
    gone.add(9)
    check()
    assert s.remove_ids([]) == 0 and s.remove_ids_dev(_cuda([])) == 0  # an empty list is a no-op
    check()
    # every cell that holds the id
    assert s.remove_ids_dev(_cuda([7])) == 3
    gone.add(7)
    check()
    # duplicates in the list, absent ids, a negative id, id 0, the largest id, non-integer ids known and unknown
    lst = [12, 12, 12, 123456, -1, 0, big, "a", "never seen", "t1", 9]
    assert s.remove_ids(lst) == 5
    gone.update([12, 0, big, "a", "t1"])
    check()
    assert [i for i, _ in s.get_cell((2, 2))] == ["b", 13]
    # a non-integer id keeps its slot: the re-insert reuses it and is accepted (the id is gone from the cell)
    slot = s.device_ids_of(["a"])[0]
    assert s.add_codes_array(coarse_a[7:8], fine_a[7:8], ["a"]) == 1 and s.device_ids_of(["a"])[0] == slot
    assert [i for i, _ in s.get_cell((2, 2))] == ["b", 13, "a"]


def test_list_lengths_around_the_set_switch_and_long_probe_chains():
    """Lists of 1, 2, N_SWITCH - 1, N_SWITCH, N_SWITCH + 1 ids (sorted list in LDS <-> hash table), half of them not stored; then
    5000 ids that are all multiples of 2^20 (equal low bits: the table's hash must spread them)."""
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    m, z, X, Q = _model("tiny")
    V, M, K = m.V, m.M, m.subquantizer_clusters
    rs = np.random.RandomState(2)
    n = 9000
    coarse = rs.randint(0, V, size=(n, 2)).astype(np.uint16)
    fine = rs.randint(0, K, size=(n, M)).astype(np.uint8)
    ids = rs.permutation(n).astype(np.int64) << 20
    s = LOPQSearcherHIP(m)
    assert s.add_codes_array(coarse, fine, ids) == n
    alive = np.ones(n, dtype=bool)  # by id >> 20
    gone = set()
    for k, ln in enumerate([1, 2, N_SWITCH - 1, N_SWITCH, N_SWITCH + 1, 5000]):
        if ln == 5000:
            lst = (np.arange(2000, 7000, dtype=np.int64)) << 20  # all multiples of 2^20, some of them removed before
        else:
            stored = rs.choice(np.nonzero(alive)[0], size=(ln + 1) // 2, replace=False).astype(np.int64) << 20
            absent = (rs.randint(0, n, size=ln // 2).astype(np.int64) << 20) + 1 + rs.randint(0, 1000, size=ln // 2)
            lst = rs.permutation(np.concatenate([stored, absent]))
        assert lst.shape[0] == ln
        hit = np.unique(lst[(lst & ((1 << 20) - 1)) == 0] >> 20)
        want = int(alive[hit].sum())
        got = s.remove_ids(lst) if k % 2 else s.remove_ids_dev(_cuda(lst))
        assert got == want, ln
        alive[hit] = False
        gone.update((hit << 20).tolist())
        oi = _filtered_oracle(lambda: _oracle_index(z), [(coarse, fine, ids, gone)])
        _assert_equals_oracle(s, oi, V)


# ---- random history ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", [("tiny", 0), ("c1", 1), ("c2", 2)])
def test_random_history_of_inserts_and_removals_matches_the_filtered_oracle(name, seed):
    import torch
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from test_index_insert import _random_batches
    m, z, X, Q = _model(name)
    V, M, K = m.V, m.M, m.subquantizer_clusters
    rs = np.random.RandomState(seed)
    s = LOPQSearcherHIP(m)
    history = []  # [coarse, fine, ids, set of ids removed after the batch]
    oi = _oracle_index(z)
    for b, (coarse, fine, ids) in enumerate(_random_batches(rs, V, M, K, 9, 400, 700)):
        oi.add_codes_arrays(coarse, fine, ids.tolist())  # the state before this round's removal
        if b % 3 == 0:
            s.add_codes_array(coarse, fine, ids)
        else:
            s.add_codes_dev(torch.as_tensor(coarse.view(np.int16)).cuda(), torch.as_tensor(fine).cuda(), torch.as_tensor(ids).cuda())
        assert s.get_nb_indexed() == oi.nb_indexed
        history.append([coarse, fine, ids, set()])
        lst = rs.randint(-5, 450, size=int(rs.randint(0, 160))).astype(np.int64)  # repeats, negatives, ids never inserted
        counts_before = _oracle_counts(oi, V)
        nb_before = oi.nb_indexed
        for h in history:
            h[3].update(int(i) for i in lst)
        oi = _filtered_oracle(lambda: _oracle_index(z), history)
        if b % 2:
            removed = s.remove_ids(lst)
        else:
            delta = torch.full((V * V,), -7, dtype=torch.int64, device="cuda")
            removed = s.remove_ids_dev(_cuda(lst), cell_delta=delta)
            np.testing.assert_array_equal(delta.cpu().numpy(), counts_before - _oracle_counts(oi, V))
        assert removed == nb_before - oi.nb_indexed, b
        _assert_equals_oracle(s, oi, V)
    for qi in range(4):
        want, visited = oi.search(Q[qi], quota=60, limit=25, with_dists=True)
        got, vis = s.search(Q[qi], quota=60, limit=25, with_dists=True)
        assert vis == visited and [r.id for r in got] == [r[0] for r in want]


# ---- insert after removal ----------------------------------------------------------------------------------------------------
def test_insert_after_removal():
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    m, z, X, Q = _model("tiny")
    M = m.M
    s = LOPQSearcherHIP(m)
    c = np.zeros((4, 2), dtype=np.uint16)
    f = np.arange(4 * M, dtype=np.uint8).reshape(4, M) % 8
    assert s.add_codes_array(c, f, np.array([50, 10, 20, 30]), dedup=True) == 4
    assert s.remove_ids([10, 50]) == 2
    inplace = s.insert_counters()[0]
    assert s.add_codes_array(c[:1], f[:1], np.array([10]), dedup=True) == 1   # removed: accepted again, behind the cell's last item
    assert [i for i, _ in s.get_cell((0, 0))] == [20, 30, 10]
    assert s.insert_counters()[0] == inplace + 1                              # ... on the in-place route
    assert s.add_codes_array(c[:2], f[:2], np.array([20, 30]), dedup=True) == 0  # still stored: rejected
    assert s.get_nb_indexed() == 3


def test_cell_maximum_after_the_largest_id_left():
    """test_index_insert's cmax shape with a removal of the cell's largest id in between: the recomputed maximum must keep the
    duplicate test of later inserts exact (an id below a too-small maximum would be walked needlessly; an id above a stale one of a
    removed item must still be found absent)."""
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    m, z, X, Q = _model("tiny")
    M = m.M
    s = LOPQSearcherHIP(m)
    c = np.zeros((4, 2), dtype=np.uint16)
    f = np.arange(4 * M, dtype=np.uint8).reshape(4, M) % 8
    assert s.add_codes_array(c, f, np.array([50, 10, 20, 30]), dedup=True) == 4
    assert s.remove_ids([50]) == 1                                                          # the maximum leaves: 30 is the largest now
    assert s.add_codes_array(c[:2], f[:2], np.array([100, 30]), dedup=True) == 1            # the run ends with the duplicate 30
    assert s.add_codes_array(c[:3], f[:3], np.array([100, 70, 100]), dedup=True) == 1       # 100 is stored: only 70 is new
    assert s.add_codes_array(c[:2], f[:2], np.array([50, 40]), dedup=True) == 2             # 50 is gone, 40 was never there
    assert [i for i, _ in s.get_cell((0, 0))] == [10, 20, 30, 100, 70, 50, 40]
    assert s.remove_ids([100, 70, 50, 40]) == 4
    assert s.add_codes_array(c[:2], f[:2], np.array([30, 31]), dedup=True) == 1
    assert [i for i, _ in s.get_cell((0, 0))] == [10, 20, 30, 31]


def test_a_rebuild_after_removals_keeps_the_order():
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    m, z, X, Q = _model("c2")
    V, M = m.V, m.M
    rs = np.random.RandomState(4)
    n0, n1 = 20000, 70000  # the second batch is beyond what the in-place route takes: it rebuilds the layout
    coarse0, fine0 = z["coarse"][:n0], z["fine"][:n0]
    ids0 = rs.permutation(n0).astype(np.int64) * 3
    s = LOPQSearcherHIP(m)
    assert s.add_codes_array(coarse0, fine0, ids0) == n0
    gone = rs.choice(ids0, size=3000, replace=False)
    assert s.remove_ids_dev(_cuda(gone)) == 3000
    pick = rs.randint(0, len(z["coarse"]), size=n1)
    coarse1, fine1 = z["coarse"][pick], z["fine"][pick]
    ids1 = np.concatenate([gone[:1000], 10 ** 6 + np.arange(n1 - 1000)]).astype(np.int64)  # 1000 of the removed ids come back
    rs.shuffle(ids1)
    rebuilt = s.insert_counters()[1]
    assert s.add_codes_array(coarse1, fine1, ids1) == n1
    assert s.insert_counters()[1] == rebuilt + 1
    oi = _filtered_oracle(lambda: _oracle_index(z), [(coarse0, fine0, ids0, set(gone.tolist())), (coarse1, fine1, ids1, None)])
    _assert_equals_oracle(s, oi, V)


# ---- every scan route --------------------------------------------------------------------------------------------------------
def test_every_scan_route_after_a_removal():
    """c2 with a random third of the ids removed: every scan mode answers like the oracle fed the filtered batch, and bit for bit like a
    second searcher built without those ids; the same through a view created before the removal."""
    import torch
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    m, z, X, Q = _model("c2")
    coarse, fine = z["coarse"], z["fine"]
    n = coarse.shape[0]
    rs = np.random.RandomState(9)
    ids = rs.permutation(n).astype(np.int64) * 3 + 1
    gone = rs.choice(ids, size=n // 3, replace=False)
    keep = ~np.isin(ids, gone)
    s = LOPQSearcherHIP(m)
    assert s.add_codes_array(coarse, fine, ids) == n
    v = s.view()
    torch.cuda.synchronize()
    assert s.remove_ids_dev(_cuda(gone)) == n // 3
    torch.cuda.synchronize()  # the view's searches below start after the removal has drained (the streams ordered by the test)
    s2 = LOPQSearcherHIP(m)
    assert s2.add_codes_array(coarse[keep], fine[keep], ids[keep]) == int(keep.sum())
    oi = _filtered_oracle(lambda: _oracle_index(z), [(coarse, fine, ids, set(gone.tolist()))])
    nq, quota, limit = 64, 2000, 50
    want = [oi.search(Q[qi], quota=quota, limit=limit, with_dists=True) for qi in range(nq)]  # computed once, shared by the modes
    for mode in (0, 1, 2, 3, 4, 5, 6):
        s.set_scan_mode(mode=mode)
        s2.set_scan_mode(mode=mode)
        v.set_scan_mode(mode=mode)
        r, r2, rv = s.search_batch(Q[:nq], quota=quota, limit=limit), s2.search_batch(Q[:nq], quota=quota, limit=limit), v.search_batch(Q[:nq], quota=quota, limit=limit)
        for other in (r2, rv):
            for k in ("ids", "n_found", "visited"):
                np.testing.assert_array_equal(r[k], other[k], err_msg="mode %d %s" % (mode, k))
            np.testing.assert_array_equal(r["dists"].view(np.uint64), other["dists"].view(np.uint64), err_msg="mode %d" % mode)
        for qi in range(nq):
            res, visited = want[qi]
            k = len(res)
            assert int(r["n_found"][qi]) == k and int(r["visited"][qi]) == visited, (mode, qi)
            np.testing.assert_array_equal(r["ids"][qi, :k], np.array([w[0] for w in res], dtype=np.int64))
            np.testing.assert_allclose(r["dists"][qi, :k], np.array([w[2] for w in res]), rtol=1e-9, atol=1e-12)
    assert v.get_nb_indexed() == s.get_nb_indexed() == int(keep.sum())


# ---- tiny cells --------------------------------------------------------------------------------------------------------------
def test_tiny_cells_and_an_empty_index():
    """V = 256: 65536 cells, 40 000 items -- the thread-per-cell mark and the wave-per-cell compaction."""
    from oracle import lopq_oracle as O
    from test_lopq_hip_parity import _random_model
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    V, M, K, D = 256, 4, 64, 16
    m, om = _random_model(V, M, K, D, seed=5)
    rs = np.random.RandomState(5)
    s = LOPQSearcherHIP(m)
    assert s.remove_ids([1, 2, 3]) == 0 and s.remove_ids_dev(_cuda([4])) == 0 and s.get_nb_indexed() == 0  # an empty index
    n = 40000
    coarse = rs.randint(0, V, size=(n, 2)).astype(np.uint16)
    coarse[: n // 4] = coarse[rs.randint(0, 60, size=n // 4)]  # some crowded cells (more than one wave round)
    fine = rs.randint(0, K, size=(n, M)).astype(np.uint8)
    ids = rs.permutation(n).astype(np.int64)
    assert s.add_codes_array(coarse, fine, ids, dedup=False) == n
    gone = rs.choice(ids, size=10000, replace=False)
    assert s.remove_ids_dev(_cuda(gone)) == 10000
    oi = _filtered_oracle(lambda: O.OracleIndex(om), [(coarse, fine, ids, set(gone.tolist()))])
    touched = sorted(set((int(a), int(b)) for a, b in coarse))
    _assert_equals_oracle(s, oi, V, touched[:200] + touched[-200:] + [(int(a), int(b)) for a, b in coarse[:60]])
    Q = rs.randn(3, D).astype(np.float32)
    for qi in range(3):  # cell sizes and the number of non-empty cells decide where a query stops
        want, visited = oi.search(Q[qi], quota=20, limit=20, with_dists=True)
        got, vis = s.search(Q[qi], quota=20, limit=20, with_dists=True)
        assert vis == visited and [r.id for r in got] == [r[0] for r in want]
    assert s.remove_ids(ids) == n - 10000  # all the rest
    assert s.get_nb_indexed() == 0 and int(_cell_counts(s).sum()) == 0
    assert s.get_cell((int(coarse[0, 0]), int(coarse[0, 1]))) == []
    assert s.remove_ids_dev(_cuda(ids[:10])) == 0  # a removal from an index that is empty again
    r, re = s.search_batch(Q, quota=20, limit=20), LOPQSearcherHIP(m).search_batch(Q, quota=20, limit=20)  # like a fresh index
    assert (r["n_found"] == 0).all() and (r["visited"] == re["visited"]).all()
    # and it takes items again
    assert s.add_codes_array(coarse[:500], fine[:500], ids[:500], dedup=True) == 500
    oi2 = O.OracleIndex(om)
    oi2.add_codes_arrays(coarse[:500], fine[:500], ids[:500].tolist())
    _assert_equals_oracle(s, oi2, V, [(int(a), int(b)) for a, b in coarse[:100]])


# ---- views -------------------------------------------------------------------------------------------------------------------
def test_a_view_is_read_only():
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    m, z, X, Q = _model("tiny")
    s = LOPQSearcherHIP(m)
    s.add_codes_array(z["coarse"][:100], z["fine"][:100], np.arange(100))
    before = [s.get_cell((a, b)) for a in range(m.V) for b in range(m.V)]
    v = s.view()
    with pytest.raises(ValueError):
        v.remove_ids([1])
    import torch
    with pytest.raises(ValueError):
        v.remove_ids_dev(_cuda([1]))
    n = _lib.c_int64(0)
    one = np.array([1], dtype=np.int64)
    assert _lib.lib().cis_index_remove(v._ix, _lib.ptr(one), 1, _lib.ctypes.byref(n)) == _lib.CIS_EINVAL  # the library refuses as well
    assert _lib.lib().cis_index_sub_remote_counts(v._ix, _lib.ptr(np.zeros(m.V * m.V, dtype=np.int64))) == _lib.CIS_EINVAL
    assert s.get_nb_indexed() == 100 and before == [s.get_cell((a, b)) for a in range(m.V) for b in range(m.V)]


# ---- sharded, one process ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["every item on every handle", "own cells and remote counts"])
def test_three_shards_in_one_process(build):
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    L = _lib.lib()
    m, z, X, Q = _model("tiny")
    V, M = m.V, m.M
    world = 3
    owner = (np.arange(V * V) % world).astype(np.int32)
    rs = np.random.RandomState(6)
    n = 3000
    coarse, fine = z["coarse"][:n], z["fine"][:n]
    ids = rs.randint(0, 1200, size=n).astype(np.int64)  # an id sits in several cells
    cell = coarse[:, 0].astype(np.int64) * V + coarse[:, 1]
    hs = [LOPQSearcherHIP(m, shard=(r, world, owner)) for r in range(world)]
    full = _oracle_index(z)
    full.add_codes_arrays(coarse, fine, ids.tolist())
    if build == "every item on every handle":  # the id-only store of the other shards' cells recognises their duplicates
        for h in hs:
            assert h.add_codes_array(coarse, fine, ids, dedup=True) == full.nb_indexed
    else:
        deltas = []
        for r, h in enumerate(hs):
            mine = owner[cell] == r
            before = _cell_counts(h)
            h.add_codes_array(coarse[mine], fine[mine], ids[mine], dedup=True)
            deltas.append(_cell_counts(h) - before)
        total = np.ascontiguousarray(np.sum(deltas, axis=0))
        for h in hs:
            _lib.check(L.cis_index_add_remote_counts(h._ix, _lib.ptr(total)))
    for h in hs:
        np.testing.assert_array_equal(_cell_counts(h), _oracle_counts(full, V))
    gone = rs.choice(1300, size=400, replace=False).astype(np.int64)
    oi = _filtered_oracle(lambda: _oracle_index(z), [(coarse, fine, ids, set(gone.tolist()))])
    d_gone = _cuda(gone)
    deltas, removed = [], 0
    for h in hs:
        d = torch.empty(V * V, dtype=torch.int64, device="cuda")
        removed += h.remove_ids_dev(d_gone, cell_delta=d)
        deltas.append(d.cpu().numpy())
    assert removed == full.nb_indexed - oi.nb_indexed
    for r, d in enumerate(deltas):
        assert (d[owner != r] == 0).all()  # a shard reports its own cells only
    total = torch.as_tensor(np.sum(deltas, axis=0)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    for h in hs:
        _lib.check(L.cis_index_sub_remote_counts_dev(h._ix, total.data_ptr(), stream))
    torch.cuda.synchronize()
    from test_index_insert import _assert_same_cells
    for r, h in enumerate(hs):
        np.testing.assert_array_equal(_cell_counts(h), _oracle_counts(oi, V))
        assert int(L.cis_index_size(h._ix)) == oi.nb_indexed
        _assert_same_cells(h, oi, V, [(c // V, c % V) for c in range(V * V) if owner[c] == r])
    # a delta that would drive a count negative: an error, and nothing changes
    c_foreign = int(np.nonzero(owner != 0)[0][0])
    bad = np.zeros(V * V, dtype=np.int64)
    bad[c_foreign] = _oracle_counts(oi, V)[c_foreign] + 1
    bad[(c_foreign + world) % (V * V)] = 1 if _oracle_counts(oi, V)[(c_foreign + world) % (V * V)] > 0 else 0
    before = _cell_counts(hs[0])
    assert L.cis_index_sub_remote_counts(hs[0]._ix, _lib.ptr(bad)) == _lib.CIS_EINVAL
    d_bad = torch.as_tensor(bad).cuda()
    assert L.cis_index_sub_remote_counts_dev(hs[0]._ix, d_bad.data_ptr(), stream) == _lib.CIS_EINVAL
    np.testing.assert_array_equal(_cell_counts(hs[0]), before)
    neg = np.zeros(V * V, dtype=np.int64)
    neg[c_foreign] = -1
    assert L.cis_index_sub_remote_counts(hs[0]._ix, _lib.ptr(neg)) == _lib.CIS_EINVAL
    d_neg = torch.as_tensor(neg).cuda()
    assert L.cis_index_sub_remote_counts_dev(hs[0]._ix, d_neg.data_ptr(), stream) == _lib.CIS_EINVAL
    np.testing.assert_array_equal(_cell_counts(hs[0]), before)
    if build == "every item on every handle":
        # a removed id of a cell that ANOTHER shard owns is accepted again: the id-only store dropped it
        k = next(i for i in range(n) if ids[i] in set(gone.tolist()) and owner[cell[i]] != 0)
        assert hs[0].add_codes_array(coarse[k:k + 1], fine[k:k + 1], ids[k:k + 1], dedup=True) == 1
        assert hs[0].add_codes_array(coarse[k:k + 1], fine[k:k + 1], ids[k:k + 1], dedup=True) == 0
        # ... and one that is still stored there is not
        k2 = next(i for i in range(n) if ids[i] not in set(gone.tolist()) and owner[cell[i]] != 0)
        assert hs[0].add_codes_array(coarse[k2:k2 + 1], fine[k2:k2 + 1], ids[k2:k2 + 1], dedup=True) == 0
    for h in hs:
        h.close()


# ---- ShardedSearcher over a process group --------------------------------------------------------------------------------------
def _run_ranks(world):
    """tests/tools/sharded_remove_check.py, one child process per rank over gloo on the one GPU (started like the routed insert's
    two-rank test), under a time limit of its own; a child that fails ends the run."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = os.path.join(here, "tools", "sharded_remove_check.py")
    env = dict(os.environ, CIS_CHECK_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if world > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", "29591", script]
    else:
        cmd = [sys.executable, script]
    out = subprocess.run(["timeout", "-k", "10", "300"] + cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert "world %d: sharded removal == the filtered oracle on every rank" % world in text, text[-3000:]


def test_sharded_searcher_removal_world_1():
    _run_ranks(1)


def test_sharded_searcher_removal_world_2():
    _run_ranks(2)
