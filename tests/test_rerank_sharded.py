"""The exact re-rank on the cell-sharded index, on the GPU (csrc/lopq_rerank.hip: k_rerank_packed, k_rerank_select_merged;
csrc/lopq_exchange.hip: the merge that reports its records; distributed.py):
* A  cis_rerank_packed_dev bit-equal to cis_rerank_dev on the same (query, row) pairs, packed and dense layout;
* B  cis_merge_packed_src_dev equal to cis_merge_packed_dev bit for bit, its src_rec against the numpy model, and the cut;
* C  cis_rerank_select_merged_dev equal to the host rerank;
* D  both protocols end to end in ONE process (the collectives assembled by slicing) equal to the single index's search_rerank_dev
     bit for bit, the routed put of the features, and the removal; once more over a real process group of two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest

import exchange_gen as G
import rerank_sharded_model as M
from conftest import load_golden
from oracle import lopq_oracle as O

gpu = pytest.mark.gpu
N_FEATS = 500
_stores = {}


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _records(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 4).copy()).cuda()


def _store(dtype, D):
    """500 features of width D under the ids 7 row + 5 (seeded, made once per shape, left unchanged; row 11 holds a NaN):
    (numpy features, ids, FeatureStore, ResidentFeatures over a copy of the store's rows under the same ids)."""
    key = (np.dtype(dtype).name, D)
    if key not in _stores:
        import torch
        from columbiaimagesearch_amd.rerank import FeatureStore, ResidentFeatures
        rs = np.random.RandomState(2000 + D)
        f = rs.randn(N_FEATS, D).astype(dtype)
        f /= np.linalg.norm(f, axis=1, keepdims=True)
        f[11, D // 2] = np.nan
        ids = np.arange(N_FEATS, dtype=np.int64) * 7 + 5
        st = FeatureStore(D, torch.float32 if dtype == np.float32 else torch.float64)
        st.put(ids, f)
        rows, row_ids = st.rows_dev()
        assert (row_ids.cpu().numpy() == ids).all()
        _stores[key] = (f, ids, st, ResidentFeatures(rows, ids=ids.tolist()))
    return _stores[key]


def _same_bits(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=what)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64), err_msg=what)


# ---- A: the distances of a shard's own hits -----------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 288, 4096])
@pytest.mark.parametrize("nq", [1, 70])
def test_packed_distances_are_the_bits_of_k_rerank(dtype, D, nq):
    """Lists with no records, fewer than nb and more than nb (the tail is NaN; more than the 32 rows four waves hold at a time),
    ids the store does not hold, negative ids, a feature row with a NaN; the packed layout and the dense one."""
    import torch
    feats, ids, st, rf = _store(dtype, D)
    rs = np.random.RandomState(D * 3 + nq)
    Q = (feats[rs.randint(12, N_FEATS, nq)] + 0.05 * rs.randn(nq, D)).astype(dtype)
    q_t = _dev(Q)
    for nb in (5, 40):
        cnt = rs.choice([0, 1, nb - 1, nb, nb + 1, nb + 9], size=nq).astype(np.int32)
        cnt[0] = nb + 9
        if nq > 3:
            cnt[1:4] = [0, nb - 1, nb]
        Lmax = int(cnt.max()) or 1
        rid = ids[rs.randint(0, N_FEATS, (nq, Lmax))]
        rid[rs.rand(nq, Lmax) < 0.1] += 1                      # ids without a feature
        rid[rs.rand(nq, Lmax) < 0.03] = -1
        rid[0, 0] = ids[11]                                    # the NaN row, wherever list 0 is not empty
        valid = np.arange(Lmax)[None, :] < cnt[:, None]
        # what cis_rerank_dev gives for the same pairs
        rows = rf.rows_of_dev(_dev(rid))
        assert torch.equal(rows, st.rows_of_dev(_dev(rid)))
        ref = rf.distances_dev(q_t, rows).cpu().numpy()
        want = np.where(valid & (np.arange(Lmax)[None, :] < nb), ref, np.nan)
        dense = np.zeros((nq, Lmax), dtype=O.HIT_DTYPE)
        dense["id"] = np.where(valid, rid, -1)
        dense["dist"] = rs.rand(nq, Lmax)
        # packed: valid records only, in query order, and spare records behind them
        off = (np.cumsum(cnt.astype(np.int64)) - cnt).astype(np.int64)
        packed = np.concatenate([dense[valid], np.zeros(3, dtype=O.HIT_DTYPE)])
        got = st.distances_packed_dev(q_t, _records(packed), _dev(off), _dev(cnt), nb).cpu().numpy()
        assert got.shape == (packed.shape[0],)
        _same_bits(got[:int(cnt.sum())], want[valid], "packed, nb %d" % nb)
        # dense: off = row L, cnt = valid hits; and cnt = L for every row (empty slots have id -1: NaN)
        offd = np.arange(nq, dtype=np.int64) * Lmax
        got = st.distances_packed_dev(q_t, _records(dense), _dev(offd), _dev(cnt), nb).cpu().numpy().reshape(nq, Lmax)
        _same_bits(got[valid], want[valid], "dense, nb %d" % nb)
        full = np.full(nq, Lmax, dtype=np.int32)
        got = st.distances_packed_dev(q_t, _records(dense), _dev(offd), _dev(full), nb).cpu().numpy().reshape(nq, Lmax)
        _same_bits(got, want, "dense, every slot, nb %d" % nb)
        assert np.isnan(want[valid]).any() and (~np.isnan(want)).any()
    # a list that does not lie inside the records is left alone, and so is what lies outside every list
    true_d = torch.full((10,), 7.5, dtype=torch.float64, device="cuda")
    from columbiaimagesearch_amd import _lib
    f, _, keys, rws, cap, n = st._view()
    recs = _records(dense.reshape(-1)[:10])
    off_bad, cnt_bad = _dev(np.array([8], dtype=np.int64)), _dev(np.array([3], dtype=np.int32))
    _lib.check(_lib.lib().cis_rerank_packed_dev(f, st._code, n, D, keys, rws, cap, q_t.data_ptr(), 1, recs.data_ptr(), 10, off_bad.data_ptr(),
                                                cnt_bad.data_ptr(), 5, true_d.data_ptr(), torch.cuda.current_stream().cuda_stream))
    off_ok, cnt_ok = _dev(np.array([2], dtype=np.int64)), _dev(np.array([3], dtype=np.int32))
    assert bool((true_d == 7.5).all())
    _lib.check(_lib.lib().cis_rerank_packed_dev(f, st._code, n, D, keys, rws, cap, q_t.data_ptr(), 1, recs.data_ptr(), 10, off_ok.data_ptr(),
                                                cnt_ok.data_ptr(), 5, true_d.data_ptr(), torch.cuda.current_stream().cuda_stream))
    t = true_d.cpu().numpy()
    assert (t[:2] == 7.5).all() and (t[5:] == 7.5).all() and not (t[2:5] == 7.5).any()


# ---- B: the merge that says where each result came from ---------------------------------------------------------------------------

SRC_CASES = [(w, L, nq) for w in (1, 3, 8, 64) for L in (1, 64, 129, 1024, 3072) for nq in (1, 5)] + [(8, 129, 1030)]


def _exchange_offsets(cnt_all, stride):
    import torch
    from columbiaimagesearch_amd import _lib
    world, nq = int(cnt_all.shape[0]), int(cnt_all.shape[1])
    off = torch.empty((world, nq), dtype=torch.int64, device="cuda")
    totals = torch.empty(world, dtype=torch.int64, device="cuda")
    overflow = torch.empty(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().cis_exchange_offsets_dev(cnt_all.data_ptr(), world, nq, int(stride), off.data_ptr(), totals.data_ptr(),
                                                   overflow.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return off, totals, overflow


def _assert_same_merge(a, b, what):
    import torch
    for k in ("ids", "n_found", "cells", "pos"):
        assert torch.equal(a[k], b[k]), (what, k)
    assert torch.equal(a["dists"].view(torch.int64), b["dists"].view(torch.int64)), what


@gpu
@pytest.mark.parametrize("world,limit,nq", SRC_CASES, ids=["w%d-L%d-nq%d" % c for c in SRC_CASES])
def test_merge_with_src_rec_equals_the_merge_and_the_model(world, limit, nq):
    import torch
    from columbiaimagesearch_amd.lopq.search import merge_packed_dev, merge_packed_src_dev
    recs, cnt = G.make_lists(500 * world + limit + nq, world, nq, limit)
    model = M.merge_with_src(recs, cnt, limit)
    parts, off_np, totals = G.packed_layout(recs, cnt)
    stride = parts.shape[1]
    at = M.packed_index(cnt, stride) if recs.shape[0] else np.zeros(1, dtype=np.int64)   # (a case nobody answers has no records)
    want_src = np.where(model["src"] >= 0, at[np.maximum(model["src"], 0)], -1)
    cnt_d, off = _dev(cnt), _dev(off_np)
    parts_d = _records(parts).reshape(world, stride, 4)
    flat_d = parts_d.reshape(-1, 4)
    off_abs = _dev(off_np + np.arange(world, dtype=np.int64)[:, None] * stride)
    for what, p, o in (("strided", parts_d, off), ("flat", flat_d, off_abs)):
        plain = merge_packed_dev(p, o, cnt_d, nq, limit, with_codes=True)
        got = merge_packed_src_dev(p, o, cnt_d, nq, limit, with_codes=True)
        _assert_same_merge(got, plain, what)
        src = got["src_rec"].cpu().numpy()
        np.testing.assert_array_equal(src, want_src, err_msg=what)
        np.testing.assert_array_equal(got["ids"].cpu().numpy(), model["ids"], err_msg=what)
        # parts[src_rec] reproduces each result; -1 in the padding
        n_found = got["n_found"].cpu().numpy()
        pad = np.arange(limit)[None, :] >= n_found[:, None]
        assert (src[pad] == -1).all() and (src[~pad] >= 0).all()
        r = parts.reshape(-1)[src[~pad]]
        np.testing.assert_array_equal(r["id"], got["ids"].cpu().numpy()[~pad])
        np.testing.assert_array_equal(r["dist"].view(np.uint64), got["dists"].cpu().numpy()[~pad].view(np.uint64))
        np.testing.assert_array_equal(r["pos"], got["pos"].cpu().numpy().view(np.uint32)[~pad])
        np.testing.assert_array_equal(r["cell"], got["cells"].cpu().numpy()[~pad])
    # without the optional outputs
    got = merge_packed_src_dev(parts_d, off, cnt_d, nq, limit)
    np.testing.assert_array_equal(got["src_rec"].cpu().numpy(), want_src)
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("world,limit,nq", [(4, 100, 37), (8, 700, 61), (64, 64, 130)], ids=["w4-L100", "w8-L700", "w64-L64"])
def test_src_rec_stops_at_the_cut_of_the_fixed_exchange(world, limit, nq):
    """The layout of test_merge_stops_at_the_cut_of_the_fixed_exchange: no src_rec reaches the sentinel guard or a record past what
    arrived of its list, and the merge equals cis_merge_packed_dev's."""
    from columbiaimagesearch_amd.lopq.search import merge_packed_dev, merge_packed_src_dev
    recs, cnt = G.make_lists(world * 31 + limit, world, nq, limit, last_min=limit)
    totals = cnt.astype(np.int64).sum(axis=1)
    stride = int(min(max(1, np.median(totals[:-1])), totals[-1] - 1))
    flat, off_np, arrived = G.cut_layout(recs, cnt, stride)
    cnt_d = _dev(cnt)
    off, _, flag = _exchange_offsets(cnt_d, stride)
    assert int(flag.item()) == 1
    buf = _records(flat)
    parts = buf[:world * stride].view(world, stride, 4)
    got = merge_packed_src_dev(parts, off, cnt_d, nq, limit, with_codes=True)
    _assert_same_merge(got, merge_packed_dev(parts, off, cnt_d, nq, limit, with_codes=True), "cut")
    src = got["src_rec"].cpu().numpy()
    s = src[src >= 0]
    assert s.size and (s < world * stride).all() and not (flat["id"][s] == G.SENTINEL_ID).any()
    np.testing.assert_array_equal(flat["id"][s], got["ids"].cpu().numpy()[src >= 0])
    # every record lies within what arrived of a list of its own query
    lo = np.arange(world)[:, None] * stride + off_np
    hi = lo + arrived
    for q in range(nq):
        sq = src[q][src[q] >= 0]
        inside = ((sq[:, None] >= lo[None, :, q]) & (sq[:, None] < hi[None, :, q])).any(axis=1)
        assert inside.all(), q


# ---- C: the select --------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("nb", [1, 255, 256, 257, 1024])
def test_select_from_the_merged_list_equals_the_host_rerank(dtype, nb):
    """The true distances of the host path (k_rerank) stored at scattered places, found through src_rec: ids without a feature rank by
    their ADC distance, max_returned cuts by the place before the re-order, the threshold sits in a gap, a -1 / NaN tail, a query
    without results, L > nb."""
    import torch
    from test_rerank_dev import _assert_same, _gap_threshold, _np
    from columbiaimagesearch_amd.rerank import rerank_select_merged_dev
    D = 33
    feats, ids, st, rf = _store(dtype, D)
    from columbiaimagesearch_amd.rerank import ResidentFeatures
    rfi = rf
    for pad, nq in ((0, 1), (7, 6)):
        rs = np.random.RandomState(nb * 7 + pad)
        L = nb + pad
        Q = (feats[rs.randint(12, N_FEATS, nq)] + 0.05 * rs.randn(nq, D)).astype(dtype)
        rid = ids[rs.randint(12, N_FEATS, (nq, L))]
        rid[rs.rand(nq, L) < 0.07] += 1
        adc = np.sort(rs.rand(nq, L), axis=1)
        if nq > 2:
            rid[2, (3 * nb) // 4:] = -1
            rid[4, :] = -1
        adc[rid < 0] = np.nan
        q_t = _dev(Q)
        true = rfi.distances_dev(q_t, rfi.rows_of(rid)).cpu().numpy()          # [nq, L], NaN without a feature
        perm = rs.permutation(nq * L + 5)[:nq * L]                              # where the shards' records would lie
        store = np.full(nq * L + 5, 123.0)
        store[perm] = true.reshape(-1)
        src = np.where(rid >= 0, perm.reshape(nq, L), -1)
        plain = rfi.rerank(q_t, rid, adc, rerank_nb=nb)
        t = _gap_threshold([d for _, hd in plain for d in hd])
        for kw in ({}, {"max_returned": 8}, {"near_dup_th": t}, {"max_returned": max(1, nb // 2), "near_dup_th": t}):
            host = plain if not kw else rfi.rerank(q_t, rid, adc, rerank_nb=nb, **kw)
            got = _np(rerank_select_merged_dev(_dev(rid), _dev(adc), _dev(src), _dev(store), rerank_nb=nb, **kw))
            _assert_same(got, host, rid, nb)
    # a src_rec outside the distances (or -1) falls back to the ADC distance
    got = _np(rerank_select_merged_dev(_dev(rid), _dev(adc), _dev(np.full_like(src, nq * L + 99)), _dev(store), rerank_nb=nb))
    none = ResidentFeatures(rf.feats[:1].contiguous(), ids=[-999])   # holds none of the ids
    _assert_same(got, none.rerank(q_t, rid, adc, rerank_nb=nb), rid, nb)


@gpu
def test_equal_true_distances_come_out_in_merged_order():
    import torch
    from columbiaimagesearch_amd.rerank import rerank_select_merged_dev
    L = 16
    ids = np.arange(100, 100 + L, dtype=np.int64)[None, :]
    adc = np.linspace(0.1, 0.9, L)[None, :]
    true = np.linspace(2.0, 1.0, L)
    true[[9, 3, 14]] = 1.5
    true[[6, 11]] = np.nan
    adc[0, 6] = adc[0, 11] = 1.25
    src = np.array([[15 - i for i in range(L)]], dtype=np.int64)
    got = rerank_select_merged_dev(_dev(ids), _dev(adc), _dev(src), _dev(true[::-1].copy()))
    s, d = got["src"][0].cpu().tolist(), got["dists"][0].cpu().numpy()
    assert int(got["n_kept"][0]) == L
    p = s.index(3)
    assert s[p:p + 3] == [3, 9, 14] and d[p] == d[p + 1] == d[p + 2] == 1.5
    p = s.index(6)
    assert s[p:p + 2] == [6, 11] and d[p] == d[p + 1] == 1.25
    for a in range(L - 1):
        assert d[a] < d[a + 1] or (d[a] == d[a + 1] and s[a] < s[a + 1])
    assert got["ids"][0].cpu().tolist() == [100 + i for i in s]


# ---- D: end to end in one process ---------------------------------------------------------------------------------------------------

def _sharded_allgather(shards, stores, q, quota, limit, nb, kw):
    """ShardedSearcher.search_rerank_dev with the all-gathers replaced by stacking."""
    import torch
    from columbiaimagesearch_amd.distributed import exchange_stride
    from columbiaimagesearch_amd.lopq.search import merge_packed_src_dev
    from columbiaimagesearch_amd.rerank import rerank_select_merged_dev
    W, nq = len(shards), int(q.shape[0])
    pp = [s.search_partial_packed_dev(q, quota=quota, limit=limit) for s in shards]
    L = pp[0]["L"]
    true = [st.distances_packed_dev(q, p["packed"], p["off"], p["cnt"], nb) for st, p in zip(stores, pp)]
    cnt_all = torch.stack([p["cnt"] for p in pp]).contiguous()
    stride = exchange_stride(nq, L, W)
    off, totals, flag = _exchange_offsets(cnt_all, stride)
    if int(flag.item()):
        stride = max(int(totals.max().item()), 1)
        off, totals, flag = _exchange_offsets(cnt_all, stride)
    parts = torch.stack([p["packed"][:stride] for p in pp]).contiguous()
    true_all = torch.stack([t[:stride] for t in true]).contiguous()
    m = merge_packed_src_dev(parts, off, cnt_all, nq, L)
    out = rerank_select_merged_dev(m["ids"], m["dists"], m["src_rec"], true_all.reshape(-1), rerank_nb=nb, **kw)
    out["visited"] = pp[0]["visited"]
    return out


def _sharded_routed(shards, stores, q, quota, limit, nb, kw):
    """RoutedSearcher.search_rerank_dev with the all-to-alls replaced by slicing (test_exchange_kernels._routed with the distances)."""
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.distributed import home_slice, route_capacity, routed_merge_tables_dev
    from columbiaimagesearch_amd.lopq.search import merge_packed_src_dev
    from columbiaimagesearch_amd.rerank import rerank_select_merged_dev
    W, nq, D = len(shards), int(q.shape[0]), int(q.shape[1])
    row_bytes = D * q.element_size()
    cap = route_capacity(-(-nq // W), row_bytes // 4, W)
    st = torch.cuda.current_stream().cuda_stream
    home = []
    for h in range(W):
        lo, hi = home_slice(nq, h, W)
        qh = q[lo:hi].contiguous()
        mask, visited = shards[h].query_owners_dev(qh, quota=quota)
        send = torch.empty((W, cap, D), dtype=q.dtype, device="cuda")
        slot = torch.empty((W, hi - lo), dtype=torch.int32, device="cuda")
        cnt = torch.empty(W, dtype=torch.int32, device="cuda")
        ov = torch.empty(1, dtype=torch.int32, device="cuda")
        _lib.check(_lib.lib().cis_route_queries_dev(qh.data_ptr(), hi - lo, row_bytes, mask.data_ptr(), W, cap, send.data_ptr(),
                                                    slot.data_ptr(), cnt.data_ptr(), ov.data_ptr(), st))
        assert int(ov.item()) == 0
        home.append({"n": hi - lo, "visited": visited, "send": send, "slot": slot, "cnt": cnt.cpu().tolist()})
    L = max(int(limit if limit is not None else quota), 0)
    answered, measured = [], []
    for d in range(W):
        rows = torch.cat([home[h]["send"][d, :home[h]["cnt"][d]] for h in range(W)]).contiguous()
        n_rows = int(rows.shape[0])
        if n_rows:
            hits, _ = shards[d].search_partial_dev(rows, quota=quota, limit=limit)
            own = hits.reshape(-1).view(torch.int64).reshape(-1, 4)
            true = stores[d].distances_packed_dev(rows, own, torch.arange(n_rows, dtype=torch.int64, device="cuda") * L,
                                                  torch.full((n_rows,), L, dtype=torch.int32, device="cuda"), nb)
        else:
            hits = torch.empty((0, L, 32), dtype=torch.uint8, device="cuda")
            true = torch.empty(0, dtype=torch.float64, device="cuda")
        answered.append(hits)
        measured.append(true.reshape(-1, L))
    outs = []
    for h in range(W):
        back, tback = [], []
        for d in range(W):
            first = sum(home[k]["cnt"][d] for k in range(h))
            back.append(answered[d][first:first + home[h]["cnt"][d]])
            tback.append(measured[d][first:first + home[h]["cnt"][d]])
        rec = torch.cat(back).reshape(-1).view(torch.int64).reshape(-1, 4)
        true_back = torch.cat(tback).reshape(-1).contiguous()
        if rec.shape[0] == 0:
            rec = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
        off, cnt = routed_merge_tables_dev(home[h]["slot"], home[h]["cnt"], rec, L)
        m = merge_packed_src_dev(rec, off, cnt, home[h]["n"], L)
        out = rerank_select_merged_dev(m["ids"], m["dists"], m["src_rec"], true_back, rerank_nb=nb, **kw)
        out["visited"] = home[h]["visited"]
        outs.append(out)
    return {k: torch.cat([o[k] for o in outs]) for k in ("ids", "dists", "src", "n_kept", "visited")}


def _assert_bit_equal(got, want, what):
    import torch
    for k in ("ids", "src", "n_kept", "visited"):
        assert torch.equal(got[k], want[k]), (what, k)
    assert torch.equal(got["dists"].view(torch.int64), want["dists"].view(torch.int64)), (what, "dists")


@gpu
@pytest.mark.parametrize("name,W", [("tiny", 16), ("c3b", 8)], ids=["tiny-w16", "c3b-w8"])
def test_sharded_rerank_in_one_process_equals_the_single_index(name, W):
    """tiny (float64) at 16 shards and c3b (float32, PCA model, 288-wide input features) at 8: every shard's store holds only the
    features of the items in the cells it owns, every tenth feature is nowhere; the all-gather and the routed protocol equal
    single.search_rerank_dev over one store of the union bit for bit.  The stores filled through route_features_plan (the
    all-to-all sliced by hand) equal the hand-filled ones, and after a removal the answers still agree."""
    import torch
    from test_lopq_hip_parity import hip_model
    from test_rerank_dev import _gap_threshold
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.distributed import greedy_cell_owner, route_features_plan
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.rerank import FeatureStore
    z, X, Q = load_golden(name)
    m = hip_model(z)
    V = m.V
    coarse, fine = z["coarse"], z["fine"]
    n = int(coarse.shape[0])
    ids = np.arange(n, dtype=np.int64)
    F = np.ascontiguousarray(X[:n])
    tdt = torch.float32 if F.dtype == np.float32 else torch.float64
    D = int(F.shape[1])
    has = ids % 10 != 3
    cell = coarse[:, 0].astype(np.int64) * V + coarse[:, 1]
    owner = greedy_cell_owner(np.bincount(cell, minlength=V * V), W)
    q = _dev(np.ascontiguousarray(Q).astype(F.dtype))
    quota = 300
    gone = np.concatenate([ids[5::7], [n + 50, -3]]).astype(np.int64)
    settings = [("l100-nb100", 100, 100, {}), ("l129-nb64", 129, 64, {"max_returned": 50, "near_dup_th": None}), ("nb>l", 60, 200, {})]
    full = FeatureStore(D, tdt)
    full.put(ids[has], F[has])
    single = LOPQSearcherHIP(m)
    try:
        single.add_codes_array(coarse, fine)
        base = single.search_rerank_dev(q, full, quota=quota, limit=129, rerank_nb=64)
        d = base["dists"].cpu().numpy()
        settings[1][3]["near_dup_th"] = _gap_threshold(d[~np.isnan(d)].tolist())
        want = {tag: single.search_rerank_dev(q, full, quota=quota, limit=L, rerank_nb=nb, **kw) for tag, L, nb, kw in settings}
        assert int(want["l100-nb100"]["n_kept"].max()) > 0
        assert single.remove_ids_dev(_dev(gone)) == len(gone) - 2
        full.remove_dev(_dev(gone))
        want_after = single.search_rerank_dev(q, full, quota=quota, limit=100, rerank_nb=100)
    finally:
        single.close()
        full.close()
    shards, stores, routed_stores = [], [], []
    try:
        for r in range(W):
            s = LOPQSearcherHIP(m, shard=(r, W, owner))
            s.add_codes_array(coarse, fine)
            shards.append(s)
            st = FeatureStore(D, tdt)
            mine = has & (owner[cell] == r)
            if mine.any():
                st.put(ids[mine], F[mine])
            stores.append(st)
            routed_stores.append(FeatureStore(D, tdt))
        for tag, L, nb, kw in settings:
            nbe = min(nb, L)
            _assert_bit_equal(_sharded_allgather(shards, stores, q, quota, L, nbe, kw), want[tag], "all-gather " + tag)
            _assert_bit_equal(_sharded_routed(shards, stores, q, quota, L, nbe, kw), want[tag], "routed " + tag)
        # put_features_routed_dev's routing, two source ranks, the all-to-all sliced by hand
        sel = np.nonzero(has)[0]
        slices = [sel[:len(sel) // 3], sel[len(sel) // 3:]]
        plans = []
        for sl in slices:
            order, counts = route_features_plan(_dev(coarse[sl].astype(np.uint16).view(np.int16)), owner, V, W)
            plans.append((_dev(ids[sl])[order], _dev(F[sl])[order], counts.cpu().tolist()))
        for r in range(W):
            gi = torch.cat([pi[sum(c[:r]):sum(c[:r + 1])] for pi, _, c in plans])
            gf = torch.cat([pf[sum(c[:r]):sum(c[:r + 1])] for _, pf, c in plans])
            if gi.shape[0]:
                routed_stores[r].put_dev(gi.contiguous(), gf.contiguous())
            assert len(routed_stores[r]) == len(stores[r])
            fa, ra = stores[r].get_dev(_dev(ids))
            fb, rb = routed_stores[r].get_dev(_dev(ids))
            assert torch.equal(ra >= 0, rb >= 0) and torch.equal(fa.view(torch.uint8), fb.view(torch.uint8)), r
            assert torch.equal((ra >= 0).cpu(), torch.from_numpy(has & (owner[cell] == r)))
        _assert_bit_equal(_sharded_allgather(shards, routed_stores, q, quota, 100, 100, {}), want["l100-nb100"], "routed stores")
        # the removal of ShardedSearcher.remove_ids_dev, rank by rank: index, the other ranks' cell sizes, the store
        deltas = []
        for s in shards:
            delta = torch.empty(V * V, dtype=torch.int64, device="cuda")
            s.remove_ids_dev(_dev(gone), cell_delta=delta)
            deltas.append(delta)
        total = torch.stack(deltas).sum(dim=0)
        assert int(total.sum().item()) == len(gone) - 2
        for s, st in zip(shards, stores):
            _lib.check(_lib.lib().cis_index_sub_remote_counts_dev(s._ix, total.data_ptr(), torch.cuda.current_stream().cuda_stream))
            st.remove_dev(_dev(gone))
            assert bool((st.rows_of_dev(_dev(gone)) < 0).all())
        _assert_bit_equal(_sharded_allgather(shards, stores, q, quota, 100, 100, {}), want_after, "all-gather after the removal")
        _assert_bit_equal(_sharded_routed(shards, stores, q, quota, 100, 100, {}), want_after, "routed after the removal")
        gone_ids = set(gone.tolist())
        assert not (set(want_after["ids"].cpu().numpy().reshape(-1).tolist()) & gone_ids)
        torch.cuda.synchronize()
    finally:
        for s in shards:
            s.close()
        for st in stores + routed_stores:
            st.close()


@gpu
def test_sharded_and_routed_searchers_over_two_gloo_ranks():
    """tests/tools/sharded_rerank_check.py, one child process per rank over gloo on the one GPU: ShardedSearcher(features=...) and
    RoutedSearcher through their own methods -- put_features_routed_dev, search_rerank_dev, search_begin / search_end,
    remove_ids_dev -- equal to the single index on every rank."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = os.path.join(here, "tools", "sharded_rerank_check.py")
    env = dict(os.environ, CIS_CHECK_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29593", script]
    out = subprocess.run(["timeout", "-k", "10", "300"] + cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    text = out.stdout.decode()
    assert out.returncode == 0, text[-3000:]
    assert "world 2: sharded re-rank == the single index on every rank" in text, text[-3000:]
