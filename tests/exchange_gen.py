"""Seeded per-shard ranked hit lists for the merge kernels of the sharded search (numpy only; tests/test_exchange_kernels.py).

The lists obey what cis_merge_packed_dev / cis_merge_hits_dev state about their input (include/cis_hip.h):
* every (shard, query) list is sorted by (dist, visit_rank, pos);
* a cell lives on one shard, so (visit_rank, pos) never repeats across the lists of a query: shard w only uses visit ranks
  k * world + w.
Inside the contract they are built to be hard on a merge: empty lists and queries no shard answers, queries with one non-empty
list (the copy path), lists of exactly `limit`, distances drawn from a small pool so that they tie across shards (decided by
visit_rank) and inside a list (equal visit_rank too: decided by pos), 0.0, subnormal and very large finite distances."""
import numpy as np

from oracle.lopq_oracle import HIT_DTYPE

# ids of the guard records placed behind a cut exchange buffer: the generator's ids stay below 2**40
SENTINEL_ID = 0x5E5E5E5E5E5E5E5E
SPECIAL_DISTS = np.array([0.0, 5e-324, 2.2250738585072014e-308 / 3, 1e-300, 1.7976931348623157e308, 1e300])


def make_lists(seed, world, nq, limit, max_total=None, last_min=0):
    """Hit lists of `world` shards for `nq` queries: recs HIT_DTYPE [T] grouped by shard, then query, each (shard, query) list
    ranked; cnt int32 [world, nq].  A query holds at most `max_total` records over all shards (default 3 * limit + 64); the last
    shard holds at least `last_min` records of every query."""
    rs = np.random.RandomState(seed)
    max_total = 3 * limit + 64 if max_total is None else max_total
    lens = np.zeros((world, nq), dtype=np.int64)
    kind = rs.randint(0, 8, size=nq)
    for q in range(nq):
        k = kind[q]
        if k == 0:                                   # nobody answers this query
            continue
        if k == 1:                                   # one non-empty list: the copy path
            lens[rs.randint(world), q] = rs.choice([limit, rs.randint(1, limit + 1)])
            continue
        if k == 2:                                   # every shard answers, short lists
            lens[:, q] = rs.randint(0, min(limit, max(1, max_total // world)) + 1, size=world)
        else:                                        # a few shards, lengths up to exactly limit
            nz = rs.choice(world, size=min(world, rs.randint(2, 6)), replace=False)
            lens[nz, q] = np.where(rs.rand(len(nz)) < 0.3, limit, rs.randint(1, limit + 1, size=len(nz)))
        over = lens[:, q].sum() - max_total
        if over > 0:                                 # trim the longest lists down to the budget
            for w in np.argsort(-lens[:, q], kind="stable"):
                cut = min(over, lens[w, q])
                lens[w, q] -= cut
                over -= cut
                if over <= 0:
                    break
    lens[-1] = np.maximum(lens[-1], last_min)
    total = int(lens.sum())
    recs = np.zeros(total, dtype=HIT_DTYPE)
    wq = np.repeat(np.arange(world * nq), lens.reshape(-1))
    w_of, q_of = wq // nq, wq % nq
    first = np.concatenate([[0], np.cumsum(lens.reshape(-1))])[:-1]
    idx_in_list = np.arange(total) - first[wq]
    # distances from a pool small enough to tie across shards and inside lists
    pool = np.concatenate([SPECIAL_DISTS, rs.uniform(0.0, 50.0, size=max(8, min(total // 4, 4096)))])
    recs["dist"] = pool[rs.randint(0, len(pool), size=total)]
    n_ranks = max(2, limit // 16 + 2)                # few visit ranks per shard: equal (dist, visit_rank) inside a list
    recs["visit_rank"] = (rs.randint(0, n_ranks, size=total) * world + w_of).astype(np.uint32)
    recs["pos"] = (idx_in_list * 7 + rs.randint(0, 7, size=total)).astype(np.uint32)  # unique inside a list
    recs["id"] = rs.permutation(total).astype(np.int64) + rs.randint(0, 1 << 39)
    recs["cell"] = (recs["visit_rank"].astype(np.int64) * 3 + 1).astype(np.int32)
    # rank every list: (shard, query) major, then (dist, visit_rank, pos)
    order = np.lexsort((recs["pos"], recs["visit_rank"], recs["dist"], q_of, w_of))
    recs = recs[order]
    return recs, lens.astype(np.int32)


def list_of(recs, cnt, w, q):
    """Records of shard w for query q."""
    world, nq = cnt.shape
    starts = np.concatenate([[0], np.cumsum(cnt.reshape(-1).astype(np.int64))])
    i = w * nq + q
    return recs[starts[i]:starts[i + 1]]


def check_contract(recs, cnt):
    """The input contract of the merge kernels (raises AssertionError)."""
    world, nq = cnt.shape
    assert int(cnt.sum()) == recs.shape[0]
    assert (recs["id"] >= 0).all() and (recs["id"] < (1 << 40)).all()
    assert np.isfinite(recs["dist"]).all() and (recs["dist"] >= 0).all()
    for q in range(nq):
        keys = set()
        for w in range(world):
            lst = list_of(recs, cnt, w, q)
            if lst.shape[0] > 1:
                a = list(zip(lst["dist"], lst["visit_rank"], lst["pos"]))
                assert a == sorted(a), (w, q)
            assert (lst["visit_rank"] % world == w).all()
            k = set(zip(lst["visit_rank"].tolist(), lst["pos"].tolist()))
            assert len(k) == lst.shape[0] and not (k & keys), (w, q)
            keys |= k


def packed_layout(recs, cnt, stride=None):
    """[world, stride] records (shard w's lists in query order from row 0, zero rows behind), off int64 [world, nq] (exclusive scan
    per shard), totals int64 [world].  stride defaults to the largest total."""
    world, nq = cnt.shape
    totals = cnt.astype(np.int64).sum(axis=1)
    stride = max(int(totals.max()) if world else 0, 1) if stride is None else stride
    parts = np.zeros((world, stride), dtype=HIT_DTYPE)
    a = 0
    for w in range(world):
        t = int(totals[w])
        parts[w, :min(t, stride)] = recs[a:a + min(t, stride)]
        a += t
    off = np.cumsum(cnt.astype(np.int64), axis=1) - cnt
    return parts, off, totals


def cut_layout(recs, cnt, stride):
    """The fixed-size exchange cut at `stride` records per shard: a flat record buffer of world * stride rows followed by a GUARD
    region of sentinel records (id SENTINEL_ID, dist 0.0).  A cut shard other than the last one runs into the next shard's rows
    (real records), the last one into the guard.  Returns (flat HIT_DTYPE [world * stride + guard], off, arrived int32 [world, nq]
    = what a correct merge may read of every list)."""
    world, nq = cnt.shape
    parts, off, totals = packed_layout(recs, cnt, stride)
    last = world - 1
    # a merge that ignored the cut reads up to row off + cnt of a list; for the last shard that is totals[last] - stride rows past
    # the end of the layout.  The guard covers that and at least the longest list that runs past the cut.
    past = (off + cnt) > stride
    guard = max(int(totals[last]) - stride, int(cnt[past].max()) if past.any() else 0, 1)
    flat = np.zeros(world * stride + guard, dtype=HIT_DTYPE)
    flat[:world * stride] = parts.reshape(-1)
    flat[world * stride:]["id"] = SENTINEL_ID
    flat[world * stride:]["dist"] = 0.0
    flat[world * stride:]["cell"] = -7
    arrived = np.clip(stride - off, 0, cnt).astype(np.int32)
    return flat, off, arrived


def reference_merge(recs, cnt, limit):
    """Vectorised numpy merge of every query: (ids [nq, limit] -1 padded, dists NaN padded, n_found, cells -1, pos 0xffffffff).
    Equal to oracle merge_partials query by query (a lexsort with the query as major key)."""
    world, nq = cnt.shape
    q_of = np.repeat(np.tile(np.arange(nq), world), cnt.reshape(-1))
    order = np.lexsort((recs["pos"], recs["visit_rank"], recs["dist"], q_of))
    r, qs = recs[order], q_of[order]
    tot = np.bincount(qs, minlength=nq)
    start = np.cumsum(tot) - tot
    k = np.arange(qs.shape[0]) - start[qs]
    keep = k < limit
    out = {"ids": np.full((nq, limit), -1, dtype=np.int64), "dists": np.full((nq, limit), np.nan),
           "n_found": np.minimum(tot, limit).astype(np.int32), "cells": np.full((nq, limit), -1, dtype=np.int32),
           "pos": np.full((nq, limit), 0xffffffff, dtype=np.uint32)}
    qk, kk, rk = qs[keep], k[keep], r[keep]
    out["ids"][qk, kk] = rk["id"]
    out["dists"][qk, kk] = rk["dist"]
    out["cells"][qk, kk] = rk["cell"]
    out["pos"][qk, kk] = rk["pos"]
    return out


def dense_layout(recs, cnt, limit):
    """[world, nq, limit] lists with the product's invalid suffix (id -1, dist inf, visit_rank / pos 0xffffffff, cell -1): the input of
    cis_merge_hits_dev.  Every list must be at most `limit` long."""
    world, nq = cnt.shape
    assert int(cnt.max(initial=0)) <= limit
    dense = np.zeros((world, nq, limit), dtype=HIT_DTYPE)
    dense["id"] = -1
    dense["dist"] = np.inf
    dense["visit_rank"] = 0xffffffff
    dense["pos"] = 0xffffffff
    dense["cell"] = -1
    wq = np.repeat(np.arange(world * nq), cnt.reshape(-1))
    first = np.concatenate([[0], np.cumsum(cnt.reshape(-1).astype(np.int64))])[:-1]
    k = np.arange(recs.shape[0]) - first[wq]
    dense.reshape(world * nq, limit)[wq, k] = recs
    return dense
