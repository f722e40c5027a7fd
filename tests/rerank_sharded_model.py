"""A numpy model of the exact re-rank on the cell-sharded index (columbiaimagesearch_amd/distributed.py).

The lists are those of exchange_gen.make_lists: records grouped by shard, then query, every (shard, query) list ranked by
(dist, visit_rank, pos).  The protocol:
* a shard measures the first min(cnt, nb) records of each of its lists: true_d is parallel to the records, NaN for a record behind
  the local cut and for one whose feature the shard does not hold (`shard_true`);
* the home rank merges all lists by (dist, visit_rank, pos) and notes which record every result is (`merge_with_src`);
* it ranks the first nb merged results by true_d[src], or the ADC distance where that is NaN (`select`).
`host_rerank` restates ResidentFeatures.rerank (columbiaimagesearch_amd/rerank.py) with the true distances handed in, for the merged
list as a single index would produce it."""
import numpy as np


def list_index(cnt):
    """For every record (in the generator's order): (shard, query, index inside its own list)."""
    world, nq = cnt.shape
    c = cnt.reshape(-1).astype(np.int64)
    wq = np.repeat(np.arange(world * nq), c)
    first = np.concatenate([[0], np.cumsum(c)])[:-1]
    return wq // nq, wq % nq, np.arange(int(c.sum())) - first[wq]


def shard_true(recs, cnt, nb, dist_of):
    """true_d [T]: dist_of(query, id) (a float, NaN = this id has no feature) for the first nb records of every list, NaN behind."""
    _, q_of, k = list_index(cnt)
    out = np.full(recs.shape[0], np.nan)
    for i in np.nonzero(k < nb)[0]:
        out[i] = dist_of(int(q_of[i]), int(recs["id"][i]))
    return out


def merge_with_src(recs, cnt, limit):
    """exchange_gen.reference_merge plus src [nq, limit]: the record (its index in recs) of every result, -1 in the padding."""
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
           "pos": np.full((nq, limit), 0xffffffff, dtype=np.uint32), "src": np.full((nq, limit), -1, dtype=np.int64)}
    qk, kk, rk = qs[keep], k[keep], r[keep]
    out["ids"][qk, kk] = rk["id"]
    out["dists"][qk, kk] = rk["dist"]
    out["cells"][qk, kk] = rk["cell"]
    out["pos"][qk, kk] = rk["pos"]
    out["src"][qk, kk] = order[keep]
    return out


def packed_index(cnt, stride):
    """Where record i (the generator's order) lies in the flattened [world, stride] layout of exchange_gen.packed_layout."""
    w_of, _, _ = list_index(cnt)
    totals = cnt.astype(np.int64).sum(axis=1)
    first_of_shard = np.concatenate([[0], np.cumsum(totals)])[:-1]
    return w_of * stride + (np.arange(w_of.shape[0]) - first_of_shard[w_of])


def select(ids, adc, src, true_d, rerank_nb, max_returned=None, near_dup_th=None):
    """The home rank's last step.  Returns (ids [nq, nb] -1 padded, dists NaN padded, src int32 -1 padded, n_kept)."""
    nq, L = ids.shape
    nb = min(int(rerank_nb), L)
    o_ids = np.full((nq, nb), -1, dtype=np.int64)
    o_d = np.full((nq, nb), np.nan)
    o_src = np.full((nq, nb), -1, dtype=np.int32)
    n_kept = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        t = np.where(src[q, :nb] >= 0, true_d[np.maximum(src[q, :nb], 0)], np.nan) if true_d.shape[0] else np.full(nb, np.nan)
        d = np.where(np.isnan(t), adc[q, :nb], t)
        keep = [i for i in range(nb) if ids[q, i] >= 0 and (near_dup_th is None or d[i] <= near_dup_th)
                and (not max_returned or i < max_returned)]
        order = np.argsort(d[keep], kind="stable") if keep else []
        k = len(keep)
        o_ids[q, :k] = [ids[q, keep[j]] for j in order]
        o_d[q, :k] = [d[keep[j]] for j in order]
        o_src[q, :k] = [keep[j] for j in order]
        n_kept[q] = k
    return o_ids, o_d, o_src, n_kept


def protocol(recs, cnt, limit, rerank_nb, dist_of, max_returned=None, near_dup_th=None):
    """The whole sharded chain on the generator's lists.  Returns (select's tuple, the merge)."""
    nb = min(int(rerank_nb), limit)
    true_d = shard_true(recs, cnt, nb, dist_of)
    m = merge_with_src(recs, cnt, limit)
    return select(m["ids"], m["dists"], m["src"], true_d, nb, max_returned, near_dup_th), m


def host_rerank(ids, adc, dist_of, rerank_nb, max_returned=None, near_dup_th=None):
    """ResidentFeatures.rerank's loop on a merged list, the true distance of EVERY one of the first nb results looked up directly
    (no local cut): per query (ids, dists, places) in the reference's final order."""
    nq, L = ids.shape
    nb = min(int(rerank_nb), L)
    out = []
    for q in range(nq):
        valid = ids[q, :nb] >= 0
        t = np.array([dist_of(q, int(i)) if v else np.nan for i, v in zip(ids[q, :nb], valid)], dtype=np.float64).reshape(nb)
        d = np.where(np.isnan(t), adc[q, :nb], t)
        keep = [i for i in range(nb) if valid[i] and (near_dup_th is None or d[i] <= near_dup_th) and (not max_returned or i < max_returned)]
        order = np.argsort(d[keep], axis=0, kind="stable") if keep else []
        out.append(([int(ids[q, keep[j]]) for j in order], [float(d[keep[j]]) for j in order], [keep[j] for j in order]))
    return out
