"""The exact re-rank on the cell-sharded index, without a GPU: the numpy model of the protocol (rerank_sharded_model.py) on the merge
generator's lists, the routing of the features under gloo, and the argument checks of the new entry points.

What the model shows is the argument the protocol rests on: a record among a query's first nb merged results is among the first nb
of its own shard's list, so a shard that measures min(cnt, nb) records per list has measured everything the home rank ranks, and
the sharded answer is ResidentFeatures.rerank's on the merged list."""
import ctypes
import os
import socket

import numpy as np
import pytest

import exchange_gen as G
import rerank_sharded_model as M

POOL = np.concatenate([[0.0, 0.25, 0.25], np.linspace(0.1, 3.0, 20)])


def dist_of(q, i):
    """A seeded 'true distance' of (query, id): from a small pool, so that distances tie; a tenth of the ids have no feature."""
    h = (i * 2654435761 + q * 40503) % 1000003
    return np.nan if h % 10 == 3 else float(POOL[h % len(POOL)])


def _gap(dists):
    d = np.unique([x for x in dists if not np.isnan(x)])
    if d.size < 2:
        return 1.0
    g = int(np.argmax(np.diff(d)))
    return float(0.5 * (d[g] + d[g + 1]))


@pytest.mark.parametrize("limit", [1, 64, 129, 1024])
@pytest.mark.parametrize("world", [1, 3, 8, 64])
def test_model_of_the_protocol_equals_the_rerank_of_the_merged_list(world, limit):
    nq = 10
    recs, cnt = G.make_lists(31 * world + limit, world, nq, limit)
    G.check_contract(recs, cnt)
    w_of, q_of, k_in_list = M.list_index(cnt)
    for rerank_nb in sorted({1, max(1, limit // 2), limit, limit + 7}):
        nb = min(rerank_nb, limit)
        (ids, d, src, n_kept), m = M.protocol(recs, cnt, limit, rerank_nb, dist_of)
        # the local cut: the first nb merged records lie within the first nb of their own lists
        s = m["src"][:, :nb]
        assert (k_in_list[s[s >= 0]] < nb).all()
        assert ((s >= 0) == (m["ids"][:, :nb] >= 0)).all()
        np.testing.assert_array_equal(recs["id"][s[s >= 0]], m["ids"][:, :nb][s >= 0])
        plain = M.host_rerank(m["ids"], m["dists"], dist_of, rerank_nb)
        th = _gap([x for _, hd, _ in plain for x in hd])
        for kw in ({}, {"max_returned": max(1, nb // 3)}, {"near_dup_th": th}, {"max_returned": max(1, nb // 2), "near_dup_th": th}):
            (ids, d, src, n_kept), _ = M.protocol(recs, cnt, limit, rerank_nb, dist_of, **kw)
            want = M.host_rerank(m["ids"], m["dists"], dist_of, rerank_nb, **kw)
            assert ids.shape == d.shape == src.shape == (nq, nb)
            for q in range(nq):
                hi, hd, hp = want[q]
                k = int(n_kept[q])
                assert k == len(hi), (q, kw)
                assert ids[q, :k].tolist() == hi and src[q, :k].tolist() == hp, (q, kw)
                np.testing.assert_array_equal(d[q, :k].view(np.uint64), np.asarray(hd, dtype=np.float64).view(np.uint64))
                assert (ids[q, k:] == -1).all() and np.isnan(d[q, k:]).all() and (src[q, k:] == -1).all()
    # ties across lists and inside lists were part of it
    assert world == 1 or limit == 1 or len(np.unique(recs["dist"])) < recs.shape[0]


def test_packed_index_matches_the_packed_layout():
    recs, cnt = G.make_lists(5, 5, 9, 40)
    parts, off, totals = G.packed_layout(recs, cnt)
    at = M.packed_index(cnt, parts.shape[1])
    np.testing.assert_array_equal(parts.reshape(-1)[at], recs)


# ---- the routing of the features under gloo -------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _route_worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from conftest import load_golden
        from columbiaimagesearch_amd.distributed import greedy_cell_owner, route_features
        z, X, Q = load_golden("c2")
        n, V, D = 3000, 16, 24
        coarse = z["coarse"][:n]
        ids = np.arange(n, dtype=np.int64) * 3 + 1
        feats = np.random.RandomState(2).randn(n, D).astype(np.float32)
        cell = coarse[:, 0].astype(np.int64) * V + coarse[:, 1]
        owner = greedy_cell_owner(np.bincount(cell, minlength=V * V), world)
        a, b = rank * n // world + 17 * rank, (rank + 1) * n // world + 17 * (rank + 1) if rank + 1 < world else n   # ragged slices
        c16 = torch.from_numpy(np.ascontiguousarray(coarse[a:b]).astype(np.uint16).view(np.int16).copy())
        gi, gf = route_features(c16, torch.from_numpy(ids[a:b].copy()), torch.from_numpy(feats[a:b].copy()), owner, V)
        mine = owner[cell] == rank   # what this rank owns of the concatenated batch, in batch order
        ok = np.array_equal(gi.numpy(), ids[mine]) and np.array_equal(gf.numpy(), feats[mine])
        # a rank that brings nothing, and cells out of range (they go to rank 0, like their codes)
        bad = torch.tensor([[V, 0], [3, 65535 - 65536]], dtype=torch.int16)
        if rank == 1:
            gi2, gf2 = route_features(c16[:0], torch.zeros(0, dtype=torch.int64), torch.zeros((0, D)), owner, V)
        else:
            gi2, gf2 = route_features(bad, torch.tensor([7, 8]), torch.ones((2, D)), owner, V)
        ok = ok and gi2.tolist() == ([7, 8] if rank == 0 else []) and tuple(gf2.shape) == (2 if rank == 0 else 0, D)
        ret[rank] = (bool(ok), int(mine.sum()))
    finally:
        dist.destroy_process_group()


def test_features_travel_to_the_owner_of_their_cell_two_gloo_ranks():
    import torch.multiprocessing as mp
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_route_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    assert all(ret[r][0] for r in range(world)), dict(ret)
    assert ret[0][1] + ret[1][1] == 3000 and min(ret[0][1], ret[1][1]) > 0


def test_route_features_plan_is_a_stable_sort_by_owner():
    import torch
    from columbiaimagesearch_amd.distributed import route_features_plan
    rs = np.random.RandomState(8)
    V, world, n = 16, 5, 400
    owner = rs.randint(0, world, V * V)
    coarse = rs.randint(0, V, (n, 2))
    order, counts = route_features_plan(torch.from_numpy(coarse), owner, V, world)
    dst = owner[coarse[:, 0] * V + coarse[:, 1]]
    np.testing.assert_array_equal(order.numpy(), np.argsort(dst, kind="stable"))
    np.testing.assert_array_equal(counts.numpy(), np.bincount(dst, minlength=world))
    order, counts = route_features_plan(torch.zeros((0, 2), dtype=torch.int16), owner, V, world)
    assert order.numel() == 0 and counts.tolist() == [0] * world


# ---- argument checks ------------------------------------------------------------------------------------------------------------------

def test_argument_errors_need_no_device():
    from columbiaimagesearch_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)  # never dereferenced
    E = _lib.CIS_EINVAL

    def packed(dtype=_lib.CIS_F32, n_feats=100, D=8, keys=None, rows=None, cap=0, nq=3, n_rec=30, nb=10):
        return L.cis_rerank_packed_dev(p, dtype, n_feats, D, keys, rows, cap, p, nq, p, n_rec, p, p, nb, p, None)

    assert packed(dtype=2) == E and packed(dtype=0) == E
    assert packed(D=0) == E and packed(n_feats=-1) == E and packed(nq=-1) == E and packed(n_rec=-1) == E
    assert packed(nb=-1) == E and packed(nb=1025) == E
    assert packed(keys=p, rows=None, cap=16) == E and packed(keys=p, rows=p, cap=12) == E
    assert L.cis_rerank_packed_dev(p, 4, 100, 8, None, None, 0, None, 3, p, 30, p, p, 10, p, None) == E   # NULL queries
    assert packed(nq=0) == _lib.CIS_OK and packed(n_rec=0) == _lib.CIS_OK                                  # nothing to do

    def merge(world=2, stride=10, nq=3, limit=10, src=p):
        return L.cis_merge_packed_src_dev(p, world, stride, p, p, nq, limit, p, p, p, None, None, src, None)

    assert merge(world=0) == E and merge(nq=-1) == E and merge(limit=-1) == E and merge(stride=-1) == E
    assert merge(limit=3073) == E
    with pytest.raises(ValueError, match="3072"):
        _lib.check(E)
    assert merge(src=None) == E
    assert merge(nq=0) == _lib.CIS_OK

    def select(nq=3, Lq=10, n_true=30, nb=10, max_returned=0, true=p):
        return L.cis_rerank_select_merged_dev(p, p, p, nq, Lq, true, n_true, nb, max_returned, 0, 0.0, p, p, p, p, None)

    assert select(Lq=2000, nb=1025) == E
    with pytest.raises(ValueError, match="host rerank"):
        _lib.check(E)
    assert select(nb=11) == E and select(nb=-1) == E and select(max_returned=-1) == E and select(n_true=-1) == E
    assert select(nq=-1) == E and select(Lq=-1, nb=0) == E
    assert select(true=None) == E
    assert select(nq=0) == _lib.CIS_OK


def test_python_layer_refuses_before_any_launch():
    from columbiaimagesearch_amd.distributed import RoutedSearcher, ShardedSearcher, sharded_rerank_nb
    from columbiaimagesearch_amd.lopq.search import merge_packed_src_dev
    store = object()
    assert sharded_rerank_nb(store, 100, None) == 100 and sharded_rerank_nb(store, 100, 250) == 100
    assert sharded_rerank_nb(store, 3072, 1024) == 1024 and sharded_rerank_nb(store, 0, None) == 0
    with pytest.raises(ValueError, match="feature store"):
        sharded_rerank_nb(None, 100, 10)
    with pytest.raises(ValueError, match="3072"):
        sharded_rerank_nb(store, 3073, 10)
    with pytest.raises(ValueError, match="1024"):
        sharded_rerank_nb(store, 2000, 1025)
    with pytest.raises(ValueError, match="1024"):
        sharded_rerank_nb(store, 2000, None)
    with pytest.raises(ValueError):
        sharded_rerank_nb(store, 100, -1)
    with pytest.raises(ValueError, match="3072"):
        merge_packed_src_dev(None, None, None, 1, 3073)
    s = object.__new__(ShardedSearcher)    # no process group and no device: the store is asked for first
    s.features = None
    with pytest.raises(ValueError, match="feature store"):
        s.search_rerank_dev(None, quota=10, limit=10)
    with pytest.raises(ValueError, match="feature store"):
        s.put_features_routed_dev(None, None, None)
    with pytest.raises(ValueError, match="feature store"):
        s._rerank_setting(10, True, None, None, None)
    assert s._rerank_setting(10, False, None, None, None) is None
    assert hasattr(RoutedSearcher, "search_rerank_dev")
