"""k-means++ seeding (training) on the host and on the GPU at the release shapes.

  python tools/bench_seed.py                            # k x d = 2048 x 64 and 4096 x 128 on n = 2 M resident rows
  python tools/bench_seed.py --k 2048 --d 64 --n 500000 # one shape
  python tools/bench_seed.py --out profiles/seed_bench.json

Per shape, in one process: train.kmeans_pp_init (numpy, 20 000-row subsample copied to the host; wall clock, gather and copy included)
against cis_kmeanspp_dev (csrc/kmeans_seed.hip) on the same-sized subsample and on all n rows, from HIP events on resident data:
the median of repetitions that add up to at least --seconds (default 0.5) after a warm-up.  One draw on all rows (k_kpp_update +
k_kpp_pick) is the difference between a call with 9 centres and one with 1, over 8; it is reported as a fraction of 8 TB/s counting
n * d * 4 + 8 n bytes (the rows once, d2 read and written).  train.kmeans_pp_init_dev (gather, upload of the uniforms, the call)
is timed by wall clock beside it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench_kmeans import median_ms

PEAK_HBM = 8.0e12  # B/s, MI355X
SAMPLE = 20000


def bench(n, d, k, seconds):
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.lopq import train as T
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    u = torch.from_numpy(np.random.RandomState(1).rand(k)).to(dev)
    C = torch.empty((k, d), dtype=torch.float32, device=dev)
    xs = x[torch.randperm(n, generator=g, device=dev)[:min(n, SAMPLE)]].contiguous()

    def call(rows, kk):
        _lib.check(L.cis_kmeanspp_dev(rows.data_ptr(), int(rows.shape[0]), d, kk, u.data_ptr(), C.data_ptr(), None, None, stream))

    call(x, 2)  # the workspace of the largest size
    torch.cuda.synchronize()
    allocs = _lib.alloc_stats()[0]
    t_sub, reps_sub = median_ms(lambda: call(xs, k), seconds)
    t_all, reps_all = median_ms(lambda: call(x, k), seconds)
    t_9, _ = median_ms(lambda: call(x, 9), seconds)
    t_1, _ = median_ms(lambda: call(x, 1), seconds)
    grew = _lib.alloc_stats()[0] - allocs
    t_draw = (t_9 - t_1) / 8.0
    nbytes = n * d * 4.0 + 8.0 * n

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    t_host = wall(lambda: T.kmeans_pp_init(x, k, np.random.RandomState(2)))
    T.kmeans_pp_init_dev(x, k, np.random.RandomState(2))
    t_py_sub = min(wall(lambda: T.kmeans_pp_init_dev(x, k, np.random.RandomState(2))) for _ in range(3))
    t_py_all = min(wall(lambda: T.kmeans_pp_init_dev(x, k, np.random.RandomState(2), sample=None)) for _ in range(2))
    r = {"n": n, "d": d, "k": k, "sample": int(xs.shape[0]),
         "host_kmeans_pp_init_ms": t_host,
         "dev_subsample_ms": t_sub, "dev_subsample_reps": reps_sub, "kmeans_pp_init_dev_subsample_wall_ms": t_py_sub,
         "dev_all_rows_ms": t_all, "dev_all_rows_reps": reps_all, "kmeans_pp_init_dev_all_rows_wall_ms": t_py_all,
         "one_draw_all_rows_ms": t_draw, "one_draw_bytes": nbytes, "one_draw_frac_of_8TBps": nbytes / (t_draw * 1e-3) / PEAK_HBM,
         "host_over_dev_subsample": t_host / t_py_sub, "workspace_allocations_while_timing": grew}
    print("n=%d d=%d k=%d: host kmeans_pp_init (%d rows) %.0f ms; cis_kmeanspp_dev on %d rows %.2f ms (%d reps; kmeans_pp_init_dev wall "
          "%.2f ms: %.0f x faster than the host), on all rows %.1f ms (%d reps; wall %.1f ms); one draw on all rows %.3f ms = %.1f %% of "
          "8 TB/s (n d 4 + 8 n bytes); workspace allocations while timing: %d"
          % (n, d, k, r["sample"], t_host, r["sample"], t_sub, reps_sub, t_py_sub, t_host / t_py_sub, t_all, reps_all, t_py_all, t_draw,
             100 * r["one_draw_frac_of_8TBps"], grew), flush=True)
    return r


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--k", type=int)
    ap.add_argument("--d", type=int)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", help="write the results as JSON")
    a = ap.parse_args()
    if (a.k is None) != (a.d is None):
        ap.error("--k and --d go together")
    results = [bench(a.n, d, k, a.seconds) for k, d in ([(a.k, a.d)] if a.k else [(2048, 64), (4096, 128)])]
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_seed.py", "peak_hbm_bytes_per_s": PEAK_HBM, "results": results}, f, indent=1)
            f.write("\n")
