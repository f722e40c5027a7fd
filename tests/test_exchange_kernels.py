"""The kernels of the cell-sharded search at 8 to 64 ranks, in ONE process on one GPU.

The collectives between these kernels only move bytes, so a test can hold several shard indexes, assemble by hand what an
all-gather or all-to-all would have delivered, and drive the real kernels at any world size the ABI allows (64):
* A  cis_merge_packed_dev (strided and flat) and cis_merge_hits_dev against numpy lexsort on synthetic ranked shard lists;
* B  cis_exchange_offsets_dev against numpy, and the cut of the fixed-size exchange (sentinel guard region);
* C  cis_route_queries_dev and cis_routed_merge_tables_dev against their torch restatements (distributed.py);
* D  cis_index_query_owners_dev against the oracle's owner walk and the search plan's `visited`;
* E  the all-gather and the routed protocol end to end at 8 and 16 shards against the golden vectors and the single index;
* F  the routed insert (cis_index_route_pack_dev, cis_index_add_records_dev, cis_index_add_remote_counts_dev).
The generator of A and its layouts are checked on the CPU as well (test_generator_*, test_cut_layout_*)."""
import ctypes

import numpy as np
import pytest

import exchange_gen as G
from conftest import load_golden
from oracle import lopq_oracle as O

WORLDS = [1, 2, 3, 8, 16, 64]
LIMITS = [1, 64, 128, 129, 512, 513, 1024, 1025, 3072, 3073, 5000]
MERGE_CASES = ([(w, L, nq) for w in WORLDS for L in LIMITS for nq in (1, 5)]
               + [(8, L, 1030) for L in (1, 128, 129, 512, 513, 1025, 3072, 3073)]
               + [(2, 64, 1030), (3, 1024, 1030), (16, 5000, 1030), (64, 129, 1030)])
DENSE_MAX = 1 << 22   # world * nq * limit of the [world, nq, limit, 32] input of cis_merge_hits_dev (128 MB)


def _case_id(c):
    return "w%d-L%d-nq%d" % c


def _sample(nq, k=40):
    return sorted(set(np.linspace(0, nq - 1, min(nq, k)).astype(int).tolist())) if nq else []


# ---- CPU: the generator and its layouts --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world,limit,nq", [(64, 129, 12), (64, 3073, 3), (3, 1, 40), (1, 64, 9), (16, 5000, 2)])
def test_generator_obeys_the_merge_contract_and_the_oracle_agrees(world, limit, nq):
    """The lists obey the merge kernels' input contract; the vectorised reference, O.merge_partials query by query and the torch
    restatement merge_packed_sorted agree on them (at world 64 too)."""
    import torch
    from ref_merge import merge_packed_sorted
    recs, cnt = G.make_lists(7 + world + limit, world, nq, limit)
    G.check_contract(recs, cnt)
    assert int(cnt.max()) <= limit
    ref = G.reference_merge(recs, cnt, limit)
    for q in range(nq):
        m = O.merge_partials([G.list_of(recs, cnt, w, q) for w in range(world)], limit)
        n = m.shape[0]
        assert ref["n_found"][q] == n
        np.testing.assert_array_equal(ref["ids"][q, :n], m["id"])
        np.testing.assert_array_equal(ref["dists"][q, :n].view(np.uint64), m["dist"].view(np.uint64))
        np.testing.assert_array_equal(ref["pos"][q, :n], m["pos"])
        np.testing.assert_array_equal(ref["cells"][q, :n], m["cell"])
        assert (ref["ids"][q, n:] == -1).all() and np.isnan(ref["dists"][q, n:]).all()
        assert (ref["cells"][q, n:] == -1).all() and (ref["pos"][q, n:] == 0xffffffff).all()
    parts, off, _ = G.packed_layout(recs, cnt)
    got = merge_packed_sorted(torch.from_numpy(parts.view(np.int64).reshape(world, -1, 4).copy()), torch.from_numpy(off),
                              torch.from_numpy(cnt), nq, limit)
    np.testing.assert_array_equal(got["ids"].numpy(), ref["ids"])
    np.testing.assert_array_equal(got["n_found"].numpy(), ref["n_found"])
    np.testing.assert_array_equal(got["dists"].numpy().view(np.uint64), ref["dists"].view(np.uint64))
    if world * nq * limit <= DENSE_MAX and limit <= 3072:
        dense = G.dense_layout(recs, cnt, limit)
        for q in range(nq):
            m = O.merge_partials([dense[w, q] for w in range(world)], limit)
            np.testing.assert_array_equal(ref["ids"][q, :m.shape[0]], m["id"])


def test_generator_covers_the_edges():
    recs, cnt = G.make_lists(3, 8, 200, 129)
    d = recs["dist"]
    assert (d == 0.0).any() and ((d > 0) & (d < 2.2250738585072014e-308)).any() and (d > 1e300).any()
    nonempty = (cnt > 0).sum(axis=0)
    assert (nonempty == 0).any() and (nonempty == 1).any() and (nonempty >= 3).any() and (cnt == 129).any()
    cross = inside = False   # equal dists across shards (decided by visit_rank), equal (dist, visit_rank) in a list (by pos)
    for q in range(cnt.shape[1]):
        lists = [G.list_of(recs, cnt, w, q) for w in range(8)]
        allq = np.concatenate(lists)
        u, c = np.unique(allq["dist"], return_counts=True)
        for v in u[c > 1]:
            cross |= len(set((allq["visit_rank"][allq["dist"] == v] % 8).tolist())) > 1
        for lst in lists:
            pairs = list(zip(lst["dist"].tolist(), lst["visit_rank"].tolist()))
            inside |= len(set(pairs)) < len(pairs)
    assert cross and inside


def test_cut_layout_guards_every_read_past_the_cut():
    """The sentinel layout the GPU cut test relies on: the guard sits right behind world * stride rows, covers every read a merge
    that ignored the cut could make, and `arrived` is what lies before the cut."""
    world, nq = 4, 50
    recs, cnt = G.make_lists(11, world, nq, 300, last_min=5)
    totals = cnt.astype(np.int64).sum(axis=1)
    stride = max(1, int(totals[-1] * 0.6))
    flat, off, arrived = G.cut_layout(recs, cnt, stride)
    assert totals[-1] > stride
    guard = flat[world * stride:]
    assert guard.shape[0] >= int(totals[-1]) - stride and (guard["id"] == G.SENTINEL_ID).all()
    assert not (flat[:world * stride]["id"] == G.SENTINEL_ID).any() and not (recs["id"] == G.SENTINEL_ID).any()
    end = np.arange(world)[:, None] * stride + off + cnt   # the furthest row an uncut read reaches
    assert int(end.max()) <= flat.shape[0]
    np.testing.assert_array_equal(arrived, np.clip(stride - off, 0, cnt))
    for w in range(world):
        for q in range(nq):
            a, o = int(arrived[w, q]), w * stride + int(off[w, q])
            np.testing.assert_array_equal(flat[o:o + a], G.list_of(recs, cnt, w, q)[:a])


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------------------

def _dev_records(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1, 4).copy()).cuda()


def _assert_merged(out, ref, what=""):
    """ids, n_found, dists bit for bit, cells and pos -- padding included."""
    np.testing.assert_array_equal(out["ids"].cpu().numpy(), ref["ids"], err_msg=what)
    np.testing.assert_array_equal(out["n_found"].cpu().numpy(), ref["n_found"], err_msg=what)
    np.testing.assert_array_equal(out["dists"].cpu().numpy().view(np.uint64), ref["dists"].view(np.uint64), err_msg=what)
    np.testing.assert_array_equal(out["cells"].cpu().numpy(), ref["cells"], err_msg=what)
    np.testing.assert_array_equal(out["pos"].cpu().numpy().view(np.uint32), ref["pos"], err_msg=what)


def _assert_sorted_restatement(out, ref, what=""):
    np.testing.assert_array_equal(out["ids"].cpu().numpy(), ref["ids"], err_msg=what)
    np.testing.assert_array_equal(out["n_found"].cpu().numpy(), ref["n_found"], err_msg=what)
    d = out["dists"].cpu().numpy()
    np.testing.assert_array_equal(np.isnan(d), np.isnan(ref["dists"]), err_msg=what)
    np.testing.assert_array_equal(d[~np.isnan(d)].view(np.uint64), ref["dists"][~np.isnan(ref["dists"])].view(np.uint64), err_msg=what)


def _exchange_offsets(cnt_all, stride, overflow=None):
    import torch
    from columbiaimagesearch_amd import _lib
    world, nq = int(cnt_all.shape[0]), int(cnt_all.shape[1])
    off = torch.empty((world, nq), dtype=torch.int64, device="cuda")
    totals = torch.empty(world, dtype=torch.int64, device="cuda")
    overflow = torch.empty(1, dtype=torch.int32, device="cuda") if overflow is None else overflow
    _lib.check(_lib.lib().cis_exchange_offsets_dev(cnt_all.data_ptr(), world, nq, int(stride), off.data_ptr(), totals.data_ptr(),
                                                   overflow.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return off, totals, overflow


# ---- A: the merge kernels against numpy lexsort ------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("world,limit,nq", MERGE_CASES, ids=[_case_id(c) for c in MERGE_CASES])
def test_merge_kernels_match_lexsort(world, limit, nq):
    """cis_merge_packed_dev strided (offsets from cis_exchange_offsets_dev) and flat (stride = 0: absolute offsets into one buffer
    with sentinel gaps between the shards), and cis_merge_hits_dev on the dense form, against numpy lexsort -- ids, dists bit
    for bit, n_found, cells, pos and the padding (-1, NaN, -1, 0xffffffff)."""
    import torch
    from ref_merge import merge_packed_sorted
    from columbiaimagesearch_amd.lopq.search import merge_hits_dev, merge_packed_dev
    recs, cnt = G.make_lists(1000 * world + limit + nq, world, nq, limit)
    ref = G.reference_merge(recs, cnt, limit)
    for q in _sample(nq, 12):   # the vectorised reference is the oracle's merge, query by query
        m = O.merge_partials([G.list_of(recs, cnt, w, q) for w in range(world)], limit)
        assert ref["n_found"][q] == m.shape[0]
        np.testing.assert_array_equal(ref["ids"][q, :m.shape[0]], m["id"])
    # strided: [world, stride, 4] as the payload all-gather delivers it, offsets by the kernel of the fixed-size exchange
    parts, off_np, totals = G.packed_layout(recs, cnt)
    stride = parts.shape[1]
    cnt_d = torch.from_numpy(cnt).cuda().contiguous()
    off, tot_d, flag = _exchange_offsets(cnt_d, stride)
    np.testing.assert_array_equal(off.cpu().numpy(), off_np)
    np.testing.assert_array_equal(tot_d.cpu().numpy(), totals)
    assert int(flag.item()) == 0
    parts_d = _dev_records(parts).reshape(world, stride, 4)
    _assert_merged(merge_packed_dev(parts_d, off, cnt_d, nq, limit, with_codes=True), ref, what="strided")
    _assert_sorted_restatement(merge_packed_sorted(parts_d, off, cnt_d, nq, limit), ref, what="merge_packed_sorted")
    # flat (stride = 0): the shards' regions in one buffer in a shuffled order, sentinel records in the gaps between them
    rs = np.random.RandomState(nq + limit)
    gaps = rs.randint(0, 40, size=world + 1)
    base = np.zeros(world, dtype=np.int64)
    at = int(gaps[0])
    for i, w in enumerate(rs.permutation(world)):
        base[w] = at
        at += int(totals[w]) + int(gaps[i + 1])
    flat = np.zeros(max(at, 1), dtype=O.HIT_DTYPE)
    flat["id"] = G.SENTINEL_ID
    for w in range(world):
        flat[base[w]:base[w] + totals[w]] = parts[w, :totals[w]]
    off_abs = torch.from_numpy(off_np + base[:, None]).cuda().contiguous()
    _assert_merged(merge_packed_dev(_dev_records(flat), off_abs, cnt_d, nq, limit, with_codes=True), ref, what="flat")
    # dense [world, nq, limit, 32] with invalid suffixes
    if limit <= 3072 and world * nq * limit <= DENSE_MAX:
        dense = torch.from_numpy(G.dense_layout(recs, cnt, limit).view(np.uint8).reshape(world, nq, limit, 32).copy()).cuda()
        _assert_merged(merge_hits_dev(dense, with_codes=True), ref, what="dense")
    torch.cuda.synchronize()


# ---- B: offsets of the packed exchange, and its cut --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 3, 64])
@pytest.mark.parametrize("nq", [0, 1, 1023, 1024, 1025, 5000])
def test_exchange_offsets_match_numpy(world, nq):
    import torch
    rs = np.random.RandomState(world * 7919 + nq)
    cnt = rs.randint(0, 5001, size=(world, nq)).astype(np.int32)
    cnt[:, rs.rand(nq) < 0.3] = 0
    if world > 2:
        cnt[1] = 0                                  # a shard with nothing at all
    off_np = np.cumsum(cnt.astype(np.int64), axis=1) - cnt
    tot_np = cnt.astype(np.int64).sum(axis=1)
    cnt_d = torch.from_numpy(cnt).cuda().contiguous()
    big = int(tot_np.max(initial=0))
    flag = torch.ones(1, dtype=torch.int32, device="cuda")    # as an earlier call left it: the next call must clear it
    off, tot, flag = _exchange_offsets(cnt_d, big, flag)
    np.testing.assert_array_equal(off.cpu().numpy(), off_np)
    np.testing.assert_array_equal(tot.cpu().numpy(), tot_np)
    assert int(flag.item()) == 0                    # stride = the largest total: everything fits
    if big > 0:
        _, _, flag = _exchange_offsets(cnt_d, big - 1, flag)
        assert int(flag.item()) == 1                # one record too many on the largest shard
        _, _, flag = _exchange_offsets(cnt_d, 1 << 62, flag)
        assert int(flag.item()) == 0                # and the flag of that call does not stick


@pytest.mark.gpu
@pytest.mark.parametrize("world,limit,nq", [(4, 100, 37), (8, 700, 61), (5, 4000, 9), (64, 64, 130)],
                         ids=["w4-L100", "w8-L700", "w5-L4000", "w64-L64"])
def test_merge_stops_at_the_cut_of_the_fixed_exchange(world, limit, nq):
    """Shards that held more than the fixed stride were cut there (the overflow flag goes up).  The rows past the cut of the last
    shard are a guard region of sentinels inside the same allocation, those past the cut of an earlier shard are the next shard's
    real rows: a merge that read past the cut returns sentinels or foreign records.  The merge must equal the merge of what
    arrived."""
    import torch
    from columbiaimagesearch_amd.lopq.search import merge_packed_dev
    recs, cnt = G.make_lists(world * 31 + limit, world, nq, limit, last_min=limit)
    totals = cnt.astype(np.int64).sum(axis=1)
    stride = int(min(max(1, np.median(totals[:-1])), totals[-1] - 1))   # the last shard and the larger half of the others are cut
    flat, off_np, arrived = G.cut_layout(recs, cnt, stride)
    cnt_d = torch.from_numpy(cnt).cuda().contiguous()
    off, _, flag = _exchange_offsets(cnt_d, stride)
    assert int(flag.item()) == 1
    np.testing.assert_array_equal(off.cpu().numpy(), off_np)
    buf = _dev_records(flat)                                   # one allocation: layout + guard
    parts = buf[:world * stride].view(world, stride, 4)
    out = merge_packed_dev(parts, off, cnt_d, nq, limit, with_codes=True)
    assert not (out["ids"].cpu().numpy() == G.SENTINEL_ID).any()
    first = np.concatenate([[0], np.cumsum(cnt.reshape(-1).astype(np.int64))])[:-1]
    k = np.arange(recs.shape[0]) - np.repeat(first, cnt.reshape(-1))
    keep = k < np.repeat(arrived.reshape(-1), cnt.reshape(-1))
    _assert_merged(out, G.reference_merge(recs[keep], arrived, limit), what="cut")
    assert (totals[:-1] <= stride).any() and (totals[:-1] > stride).any() and totals[-1] > stride


# ---- C: the routing kernels against their torch restatements -----------------------------------------------------------------------

ROW_FORMATS = [("float32", 1), ("float32", 128), ("float64", 128), ("float32", 4096)]   # 4 B, 512 B, 1 KiB, 16 KiB rows


def _masks(rs, world, nq):
    full = (1 << world) - 1
    m = np.zeros(nq, dtype=np.uint64)
    for i in range(nq):
        u = rs.rand()
        if u < 0.15:
            continue                                               # a query no rank owns anything of
        bits = np.nonzero(rs.rand(world) < (0.5 if u < 0.6 else 2.0 / world))[0]
        m[i] = np.uint64(sum(1 << int(b) for b in bits) & full)
    if world >= 3:
        m &= np.uint64(full & ~(1 << 1))                           # rank 1 receives nothing
    if world == 64 and nq:
        m[rs.rand(nq) < 0.5] |= np.uint64(1 << 63)                 # bit 63
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 3, 8, 64])
@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 1023, 1024, 1025, 3000])
def test_route_kernels_match_torch_restatement(world, nq):
    """cis_route_queries_dev (slots, counts, overflow flag, the rows of every block; rows not used stay untouched) at caps below, at
    and above the largest block, for 4 B to 16 KiB rows; cis_routed_merge_tables_dev on returned lists with 0 to L valid hits."""
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.distributed import route_rows_torch, route_slots_torch, routed_merge_tables, routed_merge_tables_dev
    rs = np.random.RandomState(world * 100003 + nq)
    mask_np = _masks(rs, world, nq)
    mask = torch.from_numpy(mask_np.view(np.int64)).cuda().contiguous()
    bits = (mask_np[None, :] >> np.arange(world, dtype=np.uint64)[:, None]) & np.uint64(1)
    largest = int(bits.sum(axis=1).max(initial=0))
    caps = sorted({max(1, largest - 1), max(1, largest), largest + 5})
    st = torch.cuda.current_stream().cuda_stream
    slot = torch.empty((world, nq), dtype=torch.int32, device="cuda")
    cnt = torch.empty(world, dtype=torch.int32, device="cuda")
    ov = torch.ones(1, dtype=torch.int32, device="cuda")
    for dt, D in ROW_FORMATS:
        q = torch.from_numpy(rs.randn(nq, D).astype(dt)).cuda().contiguous()
        row_bytes = D * q.element_size()
        for cap in caps:
            if world * cap * row_bytes > (512 << 20):
                continue
            send = torch.full((world, cap, D), 7.25, dtype=q.dtype, device="cuda")
            _lib.check(_lib.lib().cis_route_queries_dev(q.data_ptr(), nq, row_bytes, mask.data_ptr(), world, cap, send.data_ptr(),
                                                        slot.data_ptr(), cnt.data_ptr(), ov.data_ptr(), st))
            slot_t, cnt_t, ov_t = route_slots_torch(mask, world, cap)
            what = "%s x %d, cap %d" % (dt, D, cap)
            assert torch.equal(slot, slot_t), what
            assert torch.equal(cnt, cnt_t), what
            assert int(ov.item()) == int(ov_t.item()) == (1 if largest > cap else 0), what   # (and it resets between calls)
            used = torch.arange(cap, device="cuda")[None, :] < cnt_t[:, None].long()
            rows_t = route_rows_torch(q, slot_t, cap)
            assert torch.equal(send[used], rows_t[used]), what
            assert bool((send[~used] == 7.25).all()), what
    # the merge tables of the return trip, for the largest cap: lists of L records with 0 to L valid hits
    cap = caps[-1]
    slot_t, cnt_t, _ = route_slots_torch(mask, world, cap)
    n_sent = cnt_t.tolist()
    rows = int(sum(n_sent))
    for L in (1, 7, 64):
        valid = rs.randint(0, L + 1, size=rows).astype(np.int32)
        if rows:
            valid[0], valid[-1] = 0, L
        vv = valid if rows else np.zeros(1, dtype=np.int32)
        rec_np = np.zeros((len(vv), L), dtype=O.HIT_DTYPE)
        rec_np["id"] = np.where(np.arange(L)[None, :] < vv[:, None], rs.randint(0, 1 << 40, size=(len(vv), L)), -1)
        o2, c2 = routed_merge_tables_dev(slot_t, n_sent, _dev_records(rec_np), L)
        o1, c1 = routed_merge_tables(slot_t, n_sent, torch.from_numpy(valid).cuda(), L)
        assert torch.equal(c1, c2) and torch.equal(o1, o2), L
        # the raw entry point with unused rows in front of every rank's group (h_base non-zero for rank 0 too)
        gap = 3
        base = (ctypes.c_int64 * world)()
        acc = gap
        for d in range(world):
            base[d] = acc
            acc += n_sent[d] + gap
        rec2_np = np.zeros((acc, L), dtype=O.HIT_DTYPE)
        rec2_np["id"] = -1
        vfull = np.zeros(acc, dtype=np.int32)
        for d in range(world):
            a = int(np.sum(n_sent[:d]))
            rec2_np[base[d]:base[d] + n_sent[d]] = rec_np[a:a + n_sent[d]]
            vfull[base[d]:base[d] + n_sent[d]] = valid[a:a + n_sent[d]]
        off = torch.empty((world, nq), dtype=torch.int64, device="cuda")
        cnt3 = torch.empty((world, nq), dtype=torch.int32, device="cuda")
        rec2 = _dev_records(rec2_np)
        _lib.check(_lib.lib().cis_routed_merge_tables_dev(slot_t.data_ptr(), world, nq, ctypes.cast(base, ctypes.c_void_p), rec2.data_ptr(),
                                                          L, off.data_ptr(), cnt3.data_ptr(), st))
        s = slot_t.cpu().numpy().astype(np.int64)
        row = np.array(list(base), dtype=np.int64)[:, None] + s
        np.testing.assert_array_equal(off.cpu().numpy(), np.where(s >= 0, row * L, 0))
        np.testing.assert_array_equal(cnt3.cpu().numpy(), np.where(s >= 0, vfull[np.clip(row, 0, acc - 1)], 0))
    torch.cuda.synchronize()


# ---- D: the owner walk ---------------------------------------------------------------------------------------------------------------

def _lattice(cdtype):
    """The tied-sums lattice of test_multisequence_plan_with_thousands_of_cells_and_tied_sums (V = 128, 30000 items)."""
    from columbiaimagesearch_amd.lopq import LOPQModel
    V = 128
    c = np.arange(1, V + 1, dtype=cdtype).reshape(V, 1)
    Cs = (c.copy(), c.copy())
    Rs = tuple(np.ones((V, 1, 1)) for _ in range(2))
    mus = tuple(np.zeros((V, 1)) for _ in range(2))
    subs = tuple([np.array([[-0.3], [-0.1], [0.1], [0.3]])] for _ in range(2))
    m = LOPQModel(parameters=(Cs, Rs, mus, subs))
    om = O.OracleModel(list(Cs), list(Rs), list(mus), [list(subs[0]), list(subs[1])])
    rs = np.random.RandomState(12)
    cells = rs.randint(1, V + 1, size=(30000, 2))
    X = (cells + rs.uniform(-0.4, 0.4, size=(30000, 2))).astype(np.float32)
    coarse, fine = m.predict_batch(X)
    Q = np.array([[0.0, 0.0], [-3.0, 200.0], [140.0, -1.0], [0.0, 131.0]], dtype=np.float32)
    return m, om, coarse, fine, None, Q


def _owner_model(name):
    """(hip model, oracle model, coarse, fine, ids, queries) of a model of the owner-walk tests."""
    from test_lopq_hip_parity import _random_model, hip_model
    if name.startswith("lattice"):
        return _lattice(np.float32 if name.endswith("32") else np.float64)
    if name.startswith("wide"):   # the random models of test_wide_coarse_vocabulary_matches_oracle
        V = int(name[4:])
        M, K, D = (8, 64, 32) if V == 300 else (4, 256, 16)
        m, om = _random_model(V, M, K, D, seed=V)
        rs = np.random.RandomState(1)
        X = rs.randn(6000, D).astype(np.float32)
        Q = rs.randn(10, D).astype(np.float32)
        coarse, fine = m.predict_batch(X)
        return m, om, coarse, fine, None, Q
    z, X, Q = load_golden(name)
    m, om = hip_model(z), O.OracleModel.from_npz(z)
    if name == "tiny":
        return m, om, z["coarse"][z["sel"]], z["fine"][z["sel"]], z["ids"], Q
    return m, om, z["coarse"], z["fine"], None, Q


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "c2", "c3", "wide300", "wide1024", "lattice32", "lattice64"])
def test_owner_walk_matches_oracle_and_search_plan(name):
    """mask and visited of cis_index_query_owners_dev against the oracle's walk (O.query_owners) for greedy owner tables of 8, 16 and
    64 ranks and the no-table form (cell % world); visited against search_batch_dev on the same index.  Quotas: 1, the cumulative
    size at a cell boundary of a query's walk, and (V <= 128) above the index size."""
    import torch
    from columbiaimagesearch_amd.distributed import greedy_cell_owner
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    m, om, coarse, fine, ids, Q = _owner_model(name)
    V = m.V
    oi = O.OracleCSRIndex(om, coarse, fine, ids)
    counts = np.diff(oi.offsets)
    n = int(counts.sum())
    # the cumulative size of query 0's walk at the end of its third non-empty cell
    x0 = O.apply_pca(om, Q[0]) if om.has_pca else Q[0]
    acc, bounds = 0, []
    for _, (c0, c1) in O.multisequence(om, x0):
        sz = int(counts[int(c0) * V + int(c1)])
        acc += sz
        if sz:
            bounds.append(acc)
        if len(bounds) == 3:
            break
    quotas = [1, bounds[-1]] + ([n + 1000] if V <= 128 else [])
    q = torch.as_tensor(np.ascontiguousarray(Q)).cuda()
    for W, owner in [(8, greedy_cell_owner(counts, 8)), (16, greedy_cell_owner(counts, 16)), (64, greedy_cell_owner(counts, 64)),
                     (64, None), (5, None)]:
        s = LOPQSearcherHIP(m, shard=(W - 1, W, owner))
        own = owner if owner is not None else (np.arange(V * V) % W).astype(np.int32)
        try:
            s.add_codes_array(coarse, fine, ids)
            for quota in quotas:
                mask, vis = s.query_owners_dev(q, quota=quota)
                r = s.search_batch_dev(q, quota=quota, limit=5)
                torch.cuda.synchronize()
                mask = mask.cpu().numpy().view(np.uint64)
                vis = vis.cpu().numpy()
                np.testing.assert_array_equal(vis, r["visited"].cpu().numpy(), err_msg="owner walk vs search plan, quota %d" % quota)
                for qi in range(len(Q)):
                    wm, wv = O.query_owners(oi, Q[qi], quota, own)
                    assert (int(mask[qi]), int(vis[qi])) == (wm, wv), (W, owner is None, quota, qi)
        finally:
            s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2", "wide300"])
def test_owner_walk_and_search_alternate_on_a_handle_and_its_view(name):
    """k_rank / k_rank_sort leave the table-group counters zeroed for the search that follows: owner walks and searches in turn
    on one handle and on a view of it keep giving the golden / oracle answers."""
    import torch
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    m, om, coarse, fine, ids, Q = _owner_model(name)
    oi = O.OracleCSRIndex(om, coarse, fine, ids)
    if name == "c2":
        z = load_golden("c2")[0]
        quota, limit = 1000, 100
        want_ids, want_n = z["s_q1000_l100_ids"], z["s_q1000_l100_n"]
    else:
        quota, limit = 200, 50
        want = [oi.search(Q[i], quota=quota, limit=limit) for i in range(len(Q))]
        want_ids = np.full((len(Q), limit), -1, dtype=np.int64)
        for i, (wi, _, _) in enumerate(want):
            want_ids[i, :len(wi)] = wi
        want_n = np.array([len(w[0]) for w in want])
    owners = [O.query_owners(oi, Q[i], 3 * quota, np.zeros(m.V * m.V, dtype=np.int32)) for i in range(len(Q))]
    s = LOPQSearcherHIP(m)
    v = None
    try:
        s.add_codes_array(coarse, fine, ids)
        v = s.view()
        q = torch.as_tensor(np.ascontiguousarray(Q)).cuda()
        for h in (s, v, v, s, s, v):
            mask, vis = h.query_owners_dev(q, quota=3 * quota)
            r = h.search_batch_dev(q, quota=quota, limit=limit)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(r["ids"].cpu().numpy(), want_ids)
            np.testing.assert_array_equal(r["n_found"].cpu().numpy(), want_n)
            assert [(int(a), int(b)) for a, b in zip(mask.cpu().numpy().view(np.uint64), vis.cpu().numpy())] == owners
    finally:
        if v is not None:
            v.close()
        s.close()


# ---- E: the 8- and 16-rank protocols end to end ----------------------------------------------------------------------------------

def _codes_of(name):
    """(fixture, X, queries of the golden settings, coarse, fine, ids) as the golden index holds them."""
    z, X, Q = load_golden(name)
    if name == "tiny":   # the golden index: sel (its re-adds are duplicates), then 20 copies of sel[0] under new ids
        c, f = z["coarse"][z["sel"]], z["fine"][z["sel"]]
        coarse = np.concatenate([c, np.repeat(c[:1], 20, 0)])
        fine = np.concatenate([f, np.repeat(f[:1], 20, 0)])
        ids = np.concatenate([z["ids"], z["dup_ids"]])
        Qx = np.concatenate([Q, X[z["sel"][:4]]])[:z["multiseq_cells"].shape[0]]
        return z, X, Qx, coarse, fine, ids
    return z, X, Q, z["coarse"], z["fine"], None


def _allgather(shards, q, quota, limit):
    """Every shard's packed partial search of the whole batch, stacked at the fixed exchange stride as the all-gather delivers it;
    offsets and overflow by cis_exchange_offsets_dev (the exact stride when the fixed one overflowed), cis_merge_packed_dev."""
    import torch
    from columbiaimagesearch_amd.distributed import exchange_stride
    from columbiaimagesearch_amd.lopq.search import merge_packed_dev
    W, nq = len(shards), int(q.shape[0])
    pp = [s.search_partial_packed_dev(q, quota=quota, limit=limit) for s in shards]
    L = pp[0]["L"]
    cnt_all = torch.stack([p["cnt"] for p in pp]).contiguous()
    stride = exchange_stride(nq, L, W)
    off, totals, flag = _exchange_offsets(cnt_all, stride)
    if int(flag.item()):
        stride = max(int(totals.max().item()), 1)
        off, totals, flag = _exchange_offsets(cnt_all, stride)
        assert int(flag.item()) == 0
    for p, o in zip(pp, off):
        assert torch.equal(p["off"], o) and int(p["total"].item()) <= stride
    parts = torch.stack([p["packed"][:stride] for p in pp]).contiguous()
    out = merge_packed_dev(parts, off, cnt_all, nq, L)
    out["visited"] = pp[0]["visited"]
    return out, cnt_all


def _routed(shards, q, quota, limit, cap=None):
    """RoutedSearcher.search_begin / search_end with the all-to-alls replaced by slicing: owners on the home shard, the send blocks by
    cis_route_queries_dev, each owner's partial search of the rows it received, the lists back home, cis_routed_merge_tables_dev,
    cis_merge_packed_dev (stride = 0).  Returns (results of the whole batch or None after an overflow, masks, overflow flags)."""
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.distributed import home_slice, route_capacity, routed_merge_tables_dev
    from columbiaimagesearch_amd.lopq.search import merge_packed_dev
    W, nq, D = len(shards), int(q.shape[0]), int(q.shape[1])
    row_bytes = D * q.element_size()
    cap = route_capacity(-(-nq // W), row_bytes // 4, W) if cap is None else cap
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
        home.append({"lo": lo, "hi": hi, "mask": mask, "visited": visited, "send": send, "slot": slot, "cnt": cnt.cpu().tolist(),
                     "ov": int(ov.item())})
    flags = [h["ov"] for h in home]
    masks = torch.cat([h["mask"] for h in home])
    if any(flags):
        return None, masks, flags
    L = max(int(limit if limit is not None else quota), 0)
    answered = []   # answered[d]: the lists of the rows owner d received, grouped by home rank
    for d in range(W):
        rows = torch.cat([home[h]["send"][d, :home[h]["cnt"][d]] for h in range(W)])
        if rows.shape[0]:
            hits, _ = shards[d].search_partial_dev(rows.contiguous(), quota=quota, limit=limit)
        else:
            hits = torch.empty((0, L, 32), dtype=torch.uint8, device="cuda")
        answered.append(hits)
    outs = []
    for h in range(W):
        back = []
        for d in range(W):
            first = sum(home[k]["cnt"][d] for k in range(h))
            back.append(answered[d][first:first + home[h]["cnt"][d]])
        rec = torch.cat(back).reshape(-1).view(torch.int64).reshape(-1, 4)
        if rec.shape[0] == 0:
            rec = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
        off, cnt = routed_merge_tables_dev(home[h]["slot"], home[h]["cnt"], rec, L)
        out = merge_packed_dev(rec, off, cnt, home[h]["hi"] - home[h]["lo"], L)
        out["visited"] = home[h]["visited"]
        outs.append(out)
    return {k: torch.cat([o[k] for o in outs]) for k in ("ids", "dists", "n_found", "visited")}, masks, flags


def _assert_like(got, want_ids, want_d, want_n, want_vis, what=""):
    L = want_ids.shape[1]
    np.testing.assert_array_equal(got["ids"].cpu().numpy()[:, :L], want_ids, err_msg=what)
    np.testing.assert_array_equal(got["n_found"].cpu().numpy(), want_n, err_msg=what)
    np.testing.assert_array_equal(got["visited"].cpu().numpy(), want_vis, err_msg=what)
    d = got["dists"].cpu().numpy()[:, :L]
    ok = ~np.isnan(want_d)
    np.testing.assert_allclose(d[ok], want_d[ok], rtol=1e-9, atol=1e-12, err_msg=what)
    assert np.isnan(d[~ok]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("name,W", [("c2", 8), ("c2", 16), ("tiny", 16)], ids=["c2-w8", "c2-w16", "tiny-w16"])
def test_sharded_protocols_in_one_process(name, W):
    """W shard indexes (greedy owner tables; on `tiny` most ranks own one cell or none) answer through the all-gather protocol and
    through the routed one: equal to the golden vectors at every setting of the fixture, and to the single index at limits 129, 700
    and 4000 on a batch of more than 1024 queries.  A shard's list is non-empty exactly where the owner mask has its bit; with one
    row per destination block the routed search overflows, and the all-gather protocol answers alike."""
    import torch
    from test_lopq_hip_parity import _settings, hip_model
    from columbiaimagesearch_amd.distributed import greedy_cell_owner
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    z, X, Q, coarse, fine, ids = _codes_of(name)
    m = hip_model(z)
    V = m.V
    big = np.ascontiguousarray(np.concatenate([Q, X[:1100 - len(Q)]]))     # > 1024 queries: the chunk loop of k_pack_scan
    quota_big = 20000 if name == "c2" else 100000
    single = LOPQSearcherHIP(m)   # the single index's answers first: at most 16 handles open at a time
    try:
        single.add_codes_array(coarse, fine, ids)
        assert single.get_nb_indexed() == int(z["nb_indexed"])
        want_big = {L: single.search_batch(big, quota=quota_big, limit=L) for L in (129, 700, 4000)}
    finally:
        single.close()
    counts = np.bincount(coarse[:, 0].astype(np.int64) * V + coarse[:, 1], minlength=V * V)
    owner = greedy_cell_owner(counts, W)
    shards = []
    try:
        for r in range(W):
            s = LOPQSearcherHIP(m, shard=(r, W, owner))
            s.add_codes_array(coarse, fine, ids)
            shards.append(s)
        q = torch.as_tensor(np.ascontiguousarray(Q)).cuda()
        qb = torch.as_tensor(big).cuda()
        for tag, quota, limit in _settings(z):
            want = [z["s_%s_%s" % (tag, k)] for k in ("ids", "dists", "n", "visited")]
            ag, cnt_all = _allgather(shards, q, quota, limit)
            _assert_like(ag, *want, what="all-gather %s" % tag)
            rt, mask, flags = _routed(shards, q, quota, limit)
            assert not any(flags), tag
            _assert_like(rt, *want, what="routed %s" % tag)
            # owners only: shard r holds hits for a query exactly where bit r of the query's owner mask is set
            mk = mask.cpu().numpy().view(np.uint64)
            bits = ((mk[None, :] >> np.arange(W, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(bool)
            np.testing.assert_array_equal(cnt_all.cpu().numpy() > 0, bits, err_msg="owners only, %s" % tag)
        for L, w in want_big.items():
            want = (w["ids"], w["dists"], w["n_found"], w["visited"])
            _assert_like(_allgather(shards, qb, quota_big, L)[0], *want, what="all-gather, limit %d" % L)
            rt, _, flags = _routed(shards, qb, quota_big, L)
            assert not any(flags), L
            _assert_like(rt, *want, what="routed, limit %d" % L)
        # blocks of one row: the routed search overflows; the all-gather protocol answers the batch (checked above) alike
        _, _, flags = _routed(shards, qb, quota_big, 129, cap=1)
        assert any(flags)
        torch.cuda.synchronize()
    finally:
        for s in shards:
            s.close()


# ---- F: the routed insert ------------------------------------------------------------------------------------------------------------

def _insert_batch(z, V):
    """c2's codes with 300 ids re-added and 7 out-of-range codes, shuffled."""
    coarse, fine = z["coarse"].astype(np.uint16), z["fine"]
    n = coarse.shape[0]
    ids = np.arange(n, dtype=np.int64) * 3 + 11
    rs = np.random.RandomState(5)
    re = rs.choice(n, 300, replace=False)
    coarse = np.concatenate([coarse, coarse[re]])
    fine = np.concatenate([fine, fine[re]])
    ids = np.concatenate([ids, ids[re]])
    bad = rs.choice(coarse.shape[0], 7, replace=False)
    coarse[bad[:4], 0] = V
    coarse[bad[4:], 1] = 65535
    perm = rs.permutation(coarse.shape[0])
    return np.ascontiguousarray(coarse[perm]), np.ascontiguousarray(fine[perm]), ids[perm]


def _route_pack(ix, coarse, fine, ids, M, W):
    import torch
    from columbiaimagesearch_amd import _lib
    n = int(coarse.shape[0])
    c = torch.as_tensor(np.ascontiguousarray(coarse).view(np.int16)).cuda()
    f, i = torch.as_tensor(np.ascontiguousarray(fine)).cuda(), torch.as_tensor(np.ascontiguousarray(ids)).cuda()
    send = torch.empty(max(n, 1) * (12 + M), dtype=torch.uint8, device="cuda")
    sc = torch.empty(W, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().cis_index_route_pack_dev(ix, i.data_ptr(), c.data_ptr(), f.data_ptr(), n, send.data_ptr(), sc.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream))
    return send[:n * (12 + M)], sc.cpu().numpy()


@pytest.mark.gpu
def test_routed_insert_at_8_ranks_equals_the_single_index():
    """Two source ranks pack their slices (cis_index_route_pack_dev), each owner inserts what is addressed to it in source-rank order
    (cis_index_add_records_dev), the summed per-cell deltas go to every shard (cis_index_add_remote_counts_dev); then once more with
    re-added ids.  Every shard's cells equal the single index's (same ids, same order), and so do the cell counts, the size and the
    added / invalid totals."""
    import torch
    from test_lopq_hip_parity import hip_model
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.distributed import greedy_cell_owner
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    z = load_golden("c2")[0]
    m = hip_model(z)
    V, M, W = m.V, m.M, 8
    coarse, fine, ids = _insert_batch(z, V)
    n = coarse.shape[0]
    rounds = [[(0, n // 2), (n // 2, n)], [(0, n // 6), (n // 2, n // 2 + n // 6)]]   # the second round re-adds
    Lb = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    single = LOPQSearcherHIP(m)   # the same batches on one index, in the order of the concatenated source slices
    try:
        s_added, s_bad = 0, 0
        for slices in rounds:
            sel = np.concatenate([np.arange(a, b) for a, b in slices])
            ad, bd = _lib.c_int64(0), _lib.c_int64(0)
            c, f, i = (torch.as_tensor(np.ascontiguousarray(x)).cuda() for x in (coarse[sel].view(np.int16), fine[sel], ids[sel]))
            _lib.check(Lb.cis_index_add_dev(single._ix, i.data_ptr(), c.data_ptr(), f.data_ptr(), len(sel), 1, ctypes.byref(ad),
                                            ctypes.byref(bd), None, st))
            s_added += ad.value
            s_bad += bd.value
        s_counts = np.zeros(V * V, dtype=np.int64)
        _lib.check(Lb.cis_index_cell_counts(single._ix, _lib.ptr(s_counts)))
        s_cells = {c: single.get_cell((c // V, c % V)) for c in range(V * V)}
        s_size = int(Lb.cis_index_size(single._ix))
    finally:
        single.close()
    assert s_bad >= 7 and s_size == s_added == int(s_counts.sum())
    owner = greedy_cell_owner(s_counts, W)
    shards = []
    try:
        for r in range(W):
            shards.append(LOPQSearcherHIP(m, shard=(r, W, owner)))
        added, bad = 0, 0
        for slices in rounds:
            packs = [_route_pack(shards[src]._ix, coarse[a:b], fine[a:b], ids[a:b], M, W) for src, (a, b) in enumerate(slices)]
            delta_sum = torch.zeros(V * V, dtype=torch.int64, device="cuda")
            for d in range(W):
                recv = []
                for send, sc in packs:
                    first = int(sc[:d].sum())
                    recv.append(send[first * (12 + M):(first + int(sc[d])) * (12 + M)])
                recv = torch.cat(recv).contiguous()
                nr = recv.shape[0] // (12 + M)
                delta = torch.empty(V * V, dtype=torch.int64, device="cuda")
                ad, bd = _lib.c_int64(0), _lib.c_int64(0)
                _lib.check(Lb.cis_index_add_records_dev(shards[d]._ix, recv.data_ptr() if nr else None, nr, 1, ctypes.byref(ad),
                                                        ctypes.byref(bd), delta.data_ptr(), st))
                assert d == 0 or bd.value == 0   # out-of-range codes all travel to rank 0
                added += ad.value
                bad += bd.value
                delta_sum += delta
            for s in shards:
                _lib.check(Lb.cis_index_add_remote_counts_dev(s._ix, delta_sum.data_ptr(), st))
            torch.cuda.synchronize()
        assert (added, bad) == (s_added, s_bad)
        for r, s in enumerate(shards):
            cc = np.zeros(V * V, dtype=np.int64)
            _lib.check(Lb.cis_index_cell_counts(s._ix, _lib.ptr(cc)))
            np.testing.assert_array_equal(cc, s_counts)
            assert int(Lb.cis_index_size(s._ix)) == s_size
            for c in np.nonzero(owner == r)[0]:
                got, want = s.get_cell((c // V, c % V)), s_cells[c]
                assert [i for i, _ in got] == [i for i, _ in want], c
                assert [tuple(x.fine) for _, x in got] == [tuple(x.fine) for _, x in want], c
    finally:
        for s in shards:
            s.close()


@pytest.mark.gpu
def test_route_pack_at_64_ranks_groups_by_owner_in_arrival_order():
    """cis_index_route_pack_dev at 64 ranks (greedy owner table, and the no-table form cell % 64) against a numpy stable sort by owner:
    grouping, order inside each group, counts; out-of-range codes go to rank 0."""
    from test_lopq_hip_parity import hip_model
    from columbiaimagesearch_amd.distributed import greedy_cell_owner
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    z = load_golden("c2")[0]
    m = hip_model(z)
    V, M, W = m.V, m.M, 64
    coarse, fine, ids = _insert_batch(z, V)
    counts = np.bincount(z["coarse"][:, 0].astype(np.int64) * V + z["coarse"][:, 1], minlength=V * V)
    for owner in (greedy_cell_owner(counts, W), None):
        own = owner if owner is not None else (np.arange(V * V) % W).astype(np.int32)
        c0, c1 = coarse[:, 0].astype(np.int64), coarse[:, 1].astype(np.int64)
        ok = (c0 < V) & (c1 < V)
        dst = np.where(ok, own[np.where(ok, c0 * V + c1, 0)], 0)
        order = np.argsort(dst, kind="stable")
        want = np.zeros((len(ids), 12 + M), dtype=np.uint8)
        want[:, :8] = ids[order].astype("<i8").view(np.uint8).reshape(-1, 8)
        want[:, 8:12] = coarse[order].astype("<u2").view(np.uint8).reshape(-1, 4)
        want[:, 12:] = fine[order]
        s = LOPQSearcherHIP(m, shard=(63, W, owner))
        try:
            send, sc = _route_pack(s._ix, coarse, fine, ids, M, W)
            np.testing.assert_array_equal(sc, np.bincount(dst, minlength=W))
            np.testing.assert_array_equal(send.cpu().numpy(), want.reshape(-1))
            assert int(sc[63]) > 0 and int(sc[0]) >= 7
        finally:
            s.close()
