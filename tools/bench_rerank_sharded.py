#!/usr/bin/env python3
"""Time the exact re-rank on the cell-sharded index, eight shards emulated in ONE process on one GPU (no collective is timed).

The shapes, the batch and the method are tools/bench_rerank.py's: 8192 queries, quota 10000, limit = rerank_nb = 100 over float32
features 1M x 128 (C2's index) and 200k x 4096 (C3 at DeepSentibank's width); medians of repetitions that add up to at least
0.5 s, HIP events on the working stream after one untimed call, the callables of a group run in turn.  Eight shard indexes (greedy
owner table) and eight feature stores, each with the features of the items in the cells its shard owns, live side by side with the
single index and one store of all features.  Per shape:

    single_search_rerank_dev_s   the yardstick: LOPQSearcherHIP.search_rerank_dev on the single index, same batch, same run
    shard0_partial_search_s      search_partial_packed_dev of shard 0 (the whole batch, its own cells)
    shard0_rerank_packed_s       cis_rerank_packed_dev alone on shard 0's finished partial result; rows_measured = the records it
                                 gathers a feature row for; gathered_over_peak = rows x D x 4 B / time / 8 TB/s (gathered bytes, not
                                 a bound: rows repeat across queries and may come from cache)
    merge_select_s               cis_merge_packed_src_dev + cis_rerank_select_merged_dev on the eight shards' gathered arrays
    one_rank_chain_s             what one rank runs per batch: shard 0's partial search and distances, then offsets, merge and select
    eight_shards_serial_s        the whole emulated chain: all eight shards' partial searches and distances one after the other on
                                 the one GPU, stacking in place of the all-gathers, offsets, merge, select

The emulated answer is compared with the single index's bit for bit (every field, every query).

    python tools/bench_rerank_sharded.py [--out profiles/rerank_sharded.txt] [--commit ID] [--small]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

HBM_PEAK = 8e12
WORLD = 8


def build(fixture, gen, n, chunk_n, dev, nq):
    """(model, codes of n generated vectors on the host, their float32 features [n, D] and the queries on the device)."""
    import numpy as np
    import torch
    import bench as B
    model, _ = B.load_model(fixture)
    P = B.mixture_centers(gen, dev)
    feats, cs, fs = None, [], []
    for c in range(n // chunk_n):
        x = B.gen_chunk(P, c, chunk_n, dev)
        if feats is None:
            feats = torch.empty((n, x.shape[1]), dtype=torch.float32, device=dev)
            q = B.make_queries(x, 0, nq, dev).float().contiguous()
        feats[c * chunk_n:(c + 1) * chunk_n] = x
        a, b = model.predict_batch_dev(x)
        cs.append(a)
        fs.append(b)
    return model, torch.cat(cs), torch.cat(fs), feats, q


def main():
    import numpy as np
    import torch
    from bench_rerank import LIMIT, NQ, QUOTA, timed_alternating
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.distributed import exchange_stride, greedy_cell_owner
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.lopq.search import merge_packed_src_dev
    from columbiaimagesearch_amd.rerank import FeatureStore, rerank_select_merged_dev
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--small", action="store_true", help="1/8 of the rows (a quick look)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    commit = args.commit
    if commit is None:
        try:
            import subprocess
            commit = subprocess.check_output(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    lines = []
    for fixture, gen, n, chunk_n in (("c4", "descriptor", 1_000_000, 125_000), ("c3full", "relu_mixture", 200_000, 25_000)):
        if args.small:
            n, chunk_n = n // 8, chunk_n // 8
        model, coarse, fine, feats, q = build(fixture, gen, n, chunk_n, dev, NQ)
        D, V = int(feats.shape[1]), model.V
        ids = torch.arange(n, dtype=torch.int64, device=dev)
        cell = (coarse.view(torch.int16).to(torch.int64) & 0xffff)
        cell = cell[:, 0] * V + cell[:, 1]
        owner = greedy_cell_owner(np.bincount(cell.cpu().numpy(), minlength=V * V), WORLD)
        own = torch.as_tensor(owner.astype(np.int64)).to(dev)[cell]
        single = LOPQSearcherHIP(model)
        single.add_codes_dev(coarse, fine, ids, dedup=False)
        full = FeatureStore(D, torch.float32, reserve=n)
        full.put_dev(ids, feats)
        shards, stores = [], []
        for r in range(WORLD):
            s = LOPQSearcherHIP(model, shard=(r, WORLD, owner))
            s.add_codes_dev(coarse, fine, ids, dedup=False)
            shards.append(s)
            mine = own == r
            st = FeatureStore(D, torch.float32, reserve=int(mine.sum().item()))
            st.put_dev(ids[mine].contiguous(), feats[mine].contiguous())
            stores.append(st)
        stream = torch.cuda.current_stream().cuda_stream
        L = LIMIT

        def offsets(cnt_all, stride):
            off = torch.empty((WORLD, NQ), dtype=torch.int64, device=dev)
            totals = torch.empty(WORLD, dtype=torch.int64, device=dev)
            flag = torch.empty(1, dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().cis_exchange_offsets_dev(cnt_all.data_ptr(), WORLD, NQ, int(stride), off.data_ptr(), totals.data_ptr(),
                                                           flag.data_ptr(), stream))
            return off, totals, flag

        def shard_part(r):
            p = shards[r].search_partial_packed_dev(q, quota=QUOTA, limit=L)
            return p, stores[r].distances_packed_dev(q, p["packed"], p["off"], p["cnt"], L)

        # the stride every batch uses: the fixed one, or the exact one when this data overflows it (decided once, outside the timing)
        parts0 = [shard_part(r) for r in range(WORLD)]
        cnt_all = torch.stack([p["cnt"] for p, _ in parts0]).contiguous()
        stride = exchange_stride(NQ, L, WORLD)
        _, totals, flag = offsets(cnt_all, stride)
        overflowed = bool(flag.item())
        if overflowed:
            stride = max(int(totals.max().item()), 1)

        def gather(pt):
            return (torch.stack([p["packed"][:stride] for p, _ in pt]).contiguous(), torch.stack([t[:stride] for _, t in pt]).contiguous(),
                    torch.stack([p["cnt"] for p, _ in pt]).contiguous())

        def merge_select(parts, true_all, cnt_all):
            off, _, _ = offsets(cnt_all, stride)
            m = merge_packed_src_dev(parts, off, cnt_all, NQ, L)
            return rerank_select_merged_dev(m["ids"], m["dists"], m["src_rec"], true_all.reshape(-1), rerank_nb=L)

        gathered = gather(parts0)

        def single_path():
            return single.search_rerank_dev(q, full, quota=QUOTA, limit=L, rerank_nb=L)

        def one_rank():
            shard_part(0)
            return merge_select(*gathered)

        def eight_serial():
            return merge_select(*gather([shard_part(r) for r in range(WORLD)]))

        want, got = single_path(), eight_serial()
        ok = all(torch.equal(got[k], want[k]) for k in ("ids", "src", "n_kept")) and \
            torch.equal(got["dists"].view(torch.int64), want["dists"].view(torch.int64))
        p0, true0 = parts0[0]
        rows_measured = int((~torch.isnan(true0[:int(p0["total"].item())])).sum().item())
        (t_single, n_single), (t_rank, n_rank), (t_eight, n_eight) = timed_alternating([single_path, one_rank, eight_serial])
        (t_part, _), (t_pack, n_pack), (t_ms, n_ms) = timed_alternating([
            lambda: shards[0].search_partial_packed_dev(q, quota=QUOTA, limit=L),
            lambda: stores[0].distances_packed_dev(q, p0["packed"], p0["off"], p0["cnt"], L),
            lambda: merge_select(*gathered)])
        bytes_gathered = float(rows_measured) * D * 4
        line = {"features": [n, D], "dtype": "float32", "shards": WORLD, "nq": NQ, "quota": QUOTA, "limit": L, "rerank_nb": L,
                "single_search_rerank_dev_s": t_single, "single_reps": n_single,
                "shard0_partial_search_s": t_part, "shard0_rerank_packed_s": t_pack, "rerank_packed_reps": n_pack,
                "shard0_records": int(p0["total"].item()), "shard0_rows_measured": rows_measured, "gathered_bytes": bytes_gathered,
                "gathered_bytes_per_s": bytes_gathered / t_pack, "gathered_over_peak_8TBs": bytes_gathered / t_pack / HBM_PEAK,
                "merge_select_s": t_ms, "merge_select_reps": n_ms, "one_rank_chain_s": t_rank, "one_rank_reps": n_rank,
                "eight_shards_serial_s": t_eight, "eight_reps": n_eight, "one_rank_over_single": t_rank / t_single,
                "exchange_stride": stride, "fixed_stride_overflowed": overflowed, "collectives": "excluded (one process, one GPU)",
                "equal_to_single_bit_for_bit": bool(ok), "commit": commit, "device": torch.cuda.get_device_name(0)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        for s in shards + [single]:
            s.close()
        for st in stores + [full]:
            st.close()
        del shards, stores, single, full, feats, q, coarse, fine, parts0, gathered, want, got
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_rerank_sharded.py: one batch of %d queries, quota %d, limit = rerank_nb = %d, %d shards emulated in one process on\n"
                    "# one GPU; seconds per batch, median of repetitions adding up to >= 0.5 s, HIP events on the working stream.  Collectives are\n"
                    "# EXCLUDED: stacking stands in for the all-gathers.  gathered_over_peak = rows measured x D x 4 B / kernel time / 8 TB/s\n"
                    "# (gathered bytes, not a bound).  Yardstick: single_search_rerank_dev_s, the single index in the same run.\n"
                    % (NQ, QUOTA, LIMIT, WORLD))
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0 if all(l["equal_to_single_bit_for_bit"] for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
