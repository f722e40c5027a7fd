"""k-means (training) on the GPU at production-like sizes.

  python tools/bench_kmeans.py                          # the two release shapes on resident data (--backend device)
  python tools/bench_kmeans.py --k 2048 --d 64          # one shape; --n points (default 2 M)
  python tools/bench_kmeans.py --backend hip            # cis_kmeans (host pointers, k * d <= 7680) against scikit-learn

--backend device times cis_kmeans_dev (csrc/kmeans_mfma.hip) from HIP events on resident data: an assignment pass alone
(iters = 0, no outputs) and a call with one update (iters = 1: two assignment passes, the sums and the division), so one Lloyd
iteration = the difference.  Beside it, in the same run, the torch formulation tools/bench_prodv.py trains with (cdist + argmin per
65 536 rows, index_add, bincount), which materialises the n x k distances, and the same with an explicit |c|^2 - 2 x.C^T matmul.
Every figure is the median of repetitions that add up to at least --seconds (default 0.5) after a warm-up."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

PEAK_F32_MATRIX = 157.3e12  # FLOP/s, MI355X


def median_ms(fn, seconds):
    """Median HIP-event time of fn() in ms: one warm-up, then repetitions until their sum reaches `seconds` (at least 3)."""
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    while sum(times) < seconds * 1e3 or len(times) < 3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), len(times)


def bench_device(n, d, k, seconds):
    import torch
    from columbiaimagesearch_amd import _lib
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x = torch.randn((n, d), generator=g, device=dev, dtype=torch.float32)
    C0 = x[torch.randperm(n, generator=g, device=dev)[:k]].clone()
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    C = C0.clone()
    assign = torch.empty(n, dtype=torch.int32, device=dev)

    def dev_call(iters, out=False):
        C.copy_(C0)
        _lib.check(L.cis_kmeans_dev(x.data_ptr(), n, d, k, iters, C.data_ptr(), assign.data_ptr() if out else None, None, stream))

    allocs = _lib.alloc_stats()[0]
    t_copy, _ = median_ms(lambda: C.copy_(C0), 0.05)
    t_assign, reps_a = median_ms(lambda: dev_call(0), seconds)
    t_one, reps_1 = median_ms(lambda: dev_call(1), seconds)
    grew = _lib.alloc_stats()[0] - allocs
    t_assign -= t_copy
    t_iter = t_one - t_copy - t_assign
    flop = 2.0 * n * k * d

    def torch_cdist():
        a = torch.cat([torch.cdist(x[i:i + 65536], C0).argmin(1) for i in range(0, n, 65536)])
        S = torch.zeros_like(C0).index_add_(0, a, x)
        cnt = torch.bincount(a, minlength=k).clamp(min=1).unsqueeze(1)
        return S / cnt, a

    def torch_matmul():
        cn = (C0 * C0).sum(1)
        a = torch.cat([torch.addmm(cn[None], x[i:i + 65536], C0.t(), alpha=-2.0).argmin(1) for i in range(0, n, 65536)])
        S = torch.zeros_like(C0).index_add_(0, a, x)
        cnt = torch.bincount(a, minlength=k).clamp(min=1).unsqueeze(1)
        return S / cnt, a

    t_cdist, _ = median_ms(torch_cdist, seconds)
    t_mm, _ = median_ms(torch_matmul, seconds)
    dev_call(0, out=True)
    agree = float((torch_matmul()[1] == assign).float().mean())
    print("n=%d d=%d k=%d: cis_kmeans_dev assignment pass %.2f ms (%d reps; %.1f TFLOP/s = %.1f %% of the %.1f TFLOP/s f32 matrix peak, "
          "2 n k d FLOP), one Lloyd iteration (assignment + update) %.2f ms (%d reps), workspace allocations while timing (first use "
          "included): %d; torch cdist+argmin+index_add %.2f ms, torch matmul+argmin+index_add %.2f ms; assignments equal to torch's "
          "on %.4f %% of the points" % (n, d, k, t_assign, reps_a, flop / t_assign / 1e9, 100 * flop / (t_assign * 1e-3) / PEAK_F32_MATRIX,
                                        PEAK_F32_MATRIX / 1e12, t_iter, reps_1, grew, t_cdist, t_mm, 100 * agree), flush=True)


def bench_hip(n, d, k, it):
    from columbiaimagesearch_amd.lopq import train as T
    from sklearn.cluster import MiniBatchKMeans
    x = np.random.RandomState(0).randn(n, d).astype(np.float32)
    T.kmeans_hip(x[:10000], k, 1)
    t = time.time()
    C, inertia = T.kmeans_hip(x, k, it, n_init=1, random_state=1)
    dt = time.time() - t
    t = time.time()
    MiniBatchKMeans(n_clusters=k, max_iter=it, n_init=1, batch_size=10000, random_state=1).fit(x[:200000])
    ds = (time.time() - t) * n / 200000
    print("n=%d d=%d k=%d iters=%d: cis_kmeans, host <-> device copies included, %.2f s (inertia/n %.4f); scikit-learn MiniBatchKMeans "
          "(the reference's call) ~%.1f s extrapolated from 200k rows" % (n, d, k, it, dt, inertia / n, ds), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--backend", choices=("device", "hip"), default="device")
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--k", type=int)
    ap.add_argument("--d", type=int)
    ap.add_argument("--iters", type=int, default=None, help="--backend hip: Lloyd iterations (default 20 for the fine shape, 10 for the coarse one)")
    ap.add_argument("--seconds", type=float, default=0.5)
    a = ap.parse_args()
    if (a.k is None) != (a.d is None):
        ap.error("--k and --d go together")
    if a.backend == "device":
        for k, d in ([(a.k, a.d)] if a.k else [(2048, 64), (4096, 128)]):
            bench_device(a.n, d, k, a.seconds)
    else:
        for k, d, it in ([(a.k, a.d, a.iters or 10)] if a.k else [(256, 16, a.iters or 20), (16, 64, a.iters or 10)]):
            bench_hip(a.n, d, k, it)
