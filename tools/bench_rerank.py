#!/usr/bin/env python3
"""Time a searched and re-ranked query batch through the host re-rank and through the device re-rank (csrc/lopq_rerank.hip).

One batch of 8192 queries, quota 10000, limit = rerank_nb = 100 (the reference's default), over resident float32 features of
two shapes: 1M x 128 (the C2 index of bench.py) and 200k x 4096 (the C3 model at DeepSentibank's width).  Two paths, run in
the same process, alternating:

    (a) LOPQSearcherHIP.search_batch_dev, then ResidentFeatures.rerank: ids and distances to the host, rows_of, k_rerank, the
        distances back, a Python loop per query;
    (b) LOPQSearcherHIP.search_rerank_dev: the same answer by kernels on the working stream.

Each path runs with row = id (no table: rows_of is one numpy expression) and with an id table (a dictionary look-up per result on
the host, the hash table in HBM on the device).  Each figure is the median of repetitions that add up to at least 0.5 s, timed
with HIP events on the working stream after one untimed call.  For (b) the fused kernel is also timed alone on a finished
search result; `gathered_over_peak` is nq x nb x D x 4 bytes over that time as a share of 8 TB/s -- the bytes the kernel
gathers, not a bound: rows repeat across queries and may come from cache.

    python tools/bench_rerank.py [--out profiles/rerank_dev.txt] [--commit ID] [--small]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8e12
NQ, QUOTA, LIMIT = 8192, 10000, 100


def timed_alternating(fns, min_s=0.5, max_reps=200):
    """Median seconds of every callable in `fns`: one untimed call each, then rounds that run them in turn; a callable drops
    out once its own repetitions add up to min_s."""
    import torch
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    while True:
        todo = [i for i in range(len(fns)) if sum(ts[i]) < min_s and len(ts[i]) < max_reps]
        if not todo:
            break
        for i in todo:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fns[i]()
            e1.record()
            e1.synchronize()
            ts[i].append(e0.elapsed_time(e1) / 1e3)
    return [(sorted(t)[len(t) // 2], len(t)) for t in ts]


def build(fixture, gen, n, chunk_n, dev):
    """(searcher over n generated vectors, their float32 features [n, D], queries [NQ, D] float32)."""
    import torch
    import bench as B
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    model, _ = B.load_model(fixture)
    P = B.mixture_centers(gen, dev)
    s = LOPQSearcherHIP(model)
    feats = None
    for c in range(n // chunk_n):
        x = B.gen_chunk(P, c, chunk_n, dev)
        if feats is None:
            feats = torch.empty((n, x.shape[1]), dtype=torch.float32, device=dev)
            q = B.make_queries(x, 0, NQ, dev).float().contiguous()
        feats[c * chunk_n:(c + 1) * chunk_n] = x
        a, b = model.predict_batch_dev(x)
        s.add_codes_dev(a, b, torch.arange(c * chunk_n, (c + 1) * chunk_n, dtype=torch.int64, device=dev), dedup=False)
    return s, feats, q


def same(host, dev, nq):
    import numpy as np
    ids, d, nk = dev["ids"][:nq].cpu().numpy(), dev["dists"][:nq].cpu().numpy(), dev["n_kept"][:nq].cpu().numpy()
    for qi in range(nq):
        k = int(nk[qi])
        if k != len(host[qi][0]) or [int(i) for i in ids[qi, :k]] != [int(i) for i in host[qi][0]]:
            return False
        if not np.array_equal(d[qi, :k].view(np.int64), np.asarray(host[qi][1], dtype=np.float64).view(np.int64)):
            return False
    return True


def main():
    import torch
    from columbiaimagesearch_amd.rerank import ResidentFeatures
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
        s, feats, q = build(fixture, gen, n, chunk_n, dev)
        D = int(feats.shape[1])
        for table in (False, True):
            rf = ResidentFeatures(feats, ids=list(range(n)) if table else None)
            rf.device_map()

            def host_path():
                r = s.search_batch_dev(q, quota=QUOTA, limit=LIMIT)
                return rf.rerank(q, r["ids"].cpu().numpy(), r["dists"].cpu().numpy(), rerank_nb=LIMIT)

            def dev_path():
                return s.search_rerank_dev(q, rf, quota=QUOTA, limit=LIMIT, rerank_nb=LIMIT)

            ok = same(host_path(), dev_path(), 256)
            (t_a, n_a), (t_b, n_b) = timed_alternating([host_path, dev_path])
            r = s.search_batch_dev(q, quota=QUOTA, limit=LIMIT)
            out = rf.rerank_dev(q, r["ids"], r["dists"], rerank_nb=LIMIT)
            (t_s, n_s), (t_k, n_k) = timed_alternating([lambda: s.search_batch_dev(q, quota=QUOTA, limit=LIMIT, out=r),
                                                        lambda: rf.rerank_dev(q, r["ids"], r["dists"], rerank_nb=LIMIT, out=out)])
            gathered = float(NQ) * LIMIT * D * 4
            line = {"features": [n, D], "dtype": "float32", "ids": "table" if table else "row = id", "nq": NQ, "quota": QUOTA,
                    "limit": LIMIT, "rerank_nb": LIMIT,
                    "a_search_then_host_rerank_s": t_a, "a_reps": n_a, "b_search_rerank_dev_s": t_b, "b_reps": n_b,
                    "a_over_b": t_a / t_b, "search_alone_s": t_s, "rerank_kernel_alone_s": t_k, "kernel_reps": n_k,
                    "gathered_bytes": gathered, "gathered_bytes_per_s": gathered / t_k, "gathered_over_peak_8TBs": gathered / t_k / HBM_PEAK,
                    "mean_kept": float(out["n_kept"].float().mean().item()), "first_256_queries_equal_bit_for_bit": ok,
                    "commit": commit, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
            del rf
        s.close()
        del s, feats, q
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_rerank.py: one batch of %d queries, quota %d, limit = rerank_nb = %d; seconds per batch, median of\n"
                    "# repetitions adding up to >= 0.5 s, HIP events on the working stream; (a) search_batch_dev + ResidentFeatures.rerank,\n"
                    "# (b) search_rerank_dev; gathered_over_peak = nq x nb x D x 4 B / kernel time / 8 TB/s (gathered bytes, not a bound).\n"
                    % (NQ, QUOTA, LIMIT))
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0 if all(l["b_search_rerank_dev_s"] < l["a_search_then_host_rerank_s"] for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
