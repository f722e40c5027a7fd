#!/usr/bin/env python3
"""Time the live feature store (csrc/feat_store.hip; rerank.FeatureStore) beside what it stands next to.

    put        256 rows into a store of 1M x 256 float32 and of 100k x 4096 float32, after reserve: stored ids (overwritten in
               place) and new ids (taken out again outside the timed region); seconds per call beside the bytes the call copies;
               cis_alloc_stats before and after the loops
    remove     1024 stored ids from the same stores and from stores ten times smaller (put back outside the timed region): one
               line shows whether the time follows k or n
    rerank     search_rerank_dev through the store against search_rerank_dev through a static ResidentFeatures of the same data
               (the shapes of tools/bench_rerank.py, ids through a table both times; the kernel is the same)
    ingest     the C5 chain of tools/bench_ingest.py (batch 256: CNN, normalise, encode, insert) with and without features=

Every figure is the median of repetitions timed with HIP events on the working stream after untimed calls, with the helpers of
tools/bench_rerank.py.  put and remove read their counts back, so a call includes its one host round trip.

    python tools/bench_featstore.py [--out profiles/featstore.txt] [--small] [--skip rerank,ingest]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_rerank import LIMIT, NQ, QUOTA, build, timed_alternating  # noqa: E402


def timed_with_undo(fn, undo, reps=30):
    """Median seconds of fn(i), each followed by an untimed undo(i); two untimed rounds first."""
    import torch
    ts = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        e1.synchronize()
        undo(i)
        if i >= 2:
            ts.append(e0.elapsed_time(e1) / 1e3)
    return sorted(ts)[len(ts) // 2], len(ts)


def filled_store(n, D, dev, room):
    import torch
    from columbiaimagesearch_amd.rerank import FeatureStore
    store = FeatureStore(D, torch.float32, reserve=n + room)
    chunk = min(n, 1 << 16)
    x = torch.randn((chunk, D), dtype=torch.float32, device=dev)
    for a in range(0, n, chunk):
        b = min(a + chunk, n)
        store.put_dev(torch.arange(a, b, dtype=torch.int64, device=dev), x[:b - a].contiguous())
    assert len(store) == n
    return store


def bench_put_remove(dev, small):
    import torch
    from columbiaimagesearch_amd import _lib
    lines = []
    B, K = 256, 1024
    for n, D in ((1_000_000, 256), (100_000, 4096)):
        if small:
            n //= 8
        for scale in (1, 10):
            m = n // scale
            store = filled_store(m, D, dev, room=B)
            g = torch.Generator(device="cpu").manual_seed(n + scale)
            f = torch.randn((B, D), dtype=torch.float32, device=dev)
            old_ids = torch.randperm(m, generator=g)[:B].to(dev)
            new_ids = torch.arange(m, m + B, dtype=torch.int64, device=dev)
            rm_ids = torch.randperm(m, generator=g)[:K].to(dev)
            rm_f = torch.randn((K, D), dtype=torch.float32, device=dev)
            # untimed: every call once at its size, so that the per-call scratch has its size
            store.put_dev(new_ids, f)
            store.remove_dev(new_ids)
            store.remove_dev(rm_ids)
            store.put_dev(rm_ids, rm_f)
            torch.cuda.synchronize()
            a0 = _lib.alloc_stats()
            cap0 = store.table_capacity()
            line = {"what": "put/remove", "rows": m, "D": D, "dtype": "float32"}
            if scale == 1:
                (t_over, r_over), = timed_alternating([lambda: store.put_dev(old_ids, f)], min_s=0.2, max_reps=100)
                t_new, r_new = timed_with_undo(lambda i: store.put_dev(new_ids, f), lambda i: store.remove_dev(new_ids))
                line.update({"put_256_stored_ids_s": t_over, "put_stored_reps": r_over, "put_256_new_ids_s": t_new, "put_new_reps": r_new,
                             "put_bytes_copied": B * D * 4, "put_stored_bytes_per_s": B * D * 4 / t_over})
            t_rm, r_rm = timed_with_undo(lambda i: store.remove_dev(rm_ids), lambda i: store.put_dev(rm_ids, rm_f))
            a1 = _lib.alloc_stats()
            line.update({"remove_1024_s": t_rm, "remove_reps": r_rm, "remove_bytes_moved_at_most": K * D * 4,
                         "allocations_in_the_loops": a1[0] - a0[0], "table_capacity": cap0, "table_capacity_after": store.table_capacity(),
                         "rows_after": len(store)})
            print(json.dumps(line), flush=True)
            lines.append(line)
            store.close()
            torch.cuda.empty_cache()
    return lines


def bench_rerank(dev, small):
    import torch
    from columbiaimagesearch_amd.rerank import FeatureStore, ResidentFeatures
    lines = []
    for fixture, gen, n, chunk_n in (("c4", "descriptor", 1_000_000, 125_000), ("c3full", "relu_mixture", 200_000, 25_000)):
        if small:
            n, chunk_n = n // 8, chunk_n // 8
        s, feats, q = build(fixture, gen, n, chunk_n, dev)
        D = int(feats.shape[1])
        rf = ResidentFeatures(feats, ids=list(range(n)))
        rf.device_map()
        store = FeatureStore(D, torch.float32, reserve=n)
        for a in range(0, n, chunk_n):
            store.put_dev(torch.arange(a, a + chunk_n, dtype=torch.int64, device=dev), feats[a:a + chunk_n])
        static = lambda: s.search_rerank_dev(q, rf, quota=QUOTA, limit=LIMIT, rerank_nb=LIMIT)
        live = lambda: s.search_rerank_dev(q, store, quota=QUOTA, limit=LIMIT, rerank_nb=LIMIT)
        a, b = static(), live()
        same = all(torch.equal(a[k], b[k]) for k in ("ids", "src", "n_kept")) and torch.equal(a["dists"].view(torch.int64), b["dists"].view(torch.int64))
        (t_a, n_a), (t_b, n_b) = timed_alternating([static, live])
        (t_a2, _), (t_b2, _) = timed_alternating([static, live])
        line = {"what": "search_rerank_dev", "features": [n, D], "nq": NQ, "quota": QUOTA, "limit": LIMIT,
                "static_resident_features_s": t_a, "static_reps": n_a, "through_the_store_s": t_b, "store_reps": n_b,
                "second_pass_static_s": t_a2, "second_pass_store_s": t_b2, "store_over_static": t_b / t_a, "equal_bit_for_bit": bool(same)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        store.close()
        s.close()
        del s, feats, q, rf, store
        torch.cuda.empty_cache()
    return lines


def synthetic_c3_model(seed=0, D_in=4096, D=256, V=16, M=16, K=256):
    """The model of tools/bench_ingest.py (that file is a script: it runs when imported)."""
    import numpy as np
    from columbiaimagesearch_amd.lopq import LOPQModelPCA
    rs = np.random.RandomState(seed)
    h, w = D // 2, D // M
    P, _ = np.linalg.qr(rs.randn(D_in, D))
    Cs = tuple((rs.randn(V, h) * 0.1).astype(np.float32) for _ in range(2))
    Rs = tuple(np.stack([np.linalg.qr(rs.randn(h, h))[0] for _ in range(V)]) for _ in range(2))
    mus = tuple(rs.randn(V, h) * 0.01 for _ in range(2))
    subs = tuple([rs.randn(K, w) * 0.05 for _ in range(M // 2)] for _ in range(2))
    return LOPQModelPCA(V=V, M=M, renorm=True, parameters=(Cs, Rs, mus, subs, P, rs.randn(D_in) * 0.01))


def bench_ingest(dev, steps=20):
    import time
    import torch
    from columbiaimagesearch_amd.featurizer import SentiBankNet
    from columbiaimagesearch_amd.featurizer.synthetic import sentibank_weights
    from columbiaimagesearch_amd.ingest import BatchIngest
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.rerank import FeatureStore
    B = 256
    net = SentiBankNet(sentibank_weights(0))
    model = synthetic_c3_model()
    x = (torch.randn(B, 3, 227, 227, device=dev) * 50.0).contiguous()
    res = {}
    for with_store in (False, True, False, True):
        s = LOPQSearcherHIP(model)
        store = FeatureStore(4096, torch.float32, reserve=(steps + 4) * B) if with_store else None
        ing = BatchIngest(net, model, s, features=store)
        for _ in range(2):
            ing.ingest_batch(x)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            ing.ingest_batch(x)
        torch.cuda.synchronize()
        res.setdefault(with_store, []).append((time.perf_counter() - t) / steps)
        ing.close()
        if store is not None:
            assert len(store) == (steps + 2) * B
            store.close()
        s.close()
    line = {"what": "C5 ingest chain, batch 256", "steps": steps, "without_features_s_per_batch": res[False], "with_features_s_per_batch": res[True],
            "copied_bytes_per_batch": B * 4096 * 4}
    print(json.dumps(line), flush=True)
    return [line]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1/8 of the rows (a quick look)")
    ap.add_argument("--skip", default="", help="comma-separated: put, rerank, ingest")
    args = ap.parse_args()
    skip = set(args.skip.split(","))
    dev = torch.device("cuda:0")
    lines = []
    if "put" not in skip:
        lines += bench_put_remove(dev, args.small)
    if "rerank" not in skip:
        lines += bench_rerank(dev, args.small)
    if "ingest" not in skip:
        lines += bench_ingest(dev)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/bench_featstore.py on %s: seconds per call, medians, HIP events on the working stream (the ingest chain: wall\n"
                    "# clock over 20 batches, two runs each way); put and remove include their one read-back of the counts.\n" % torch.cuda.get_device_name(0))
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
