#!/usr/bin/env python3
"""Time lopq.eval.exact_neighbors (csrc/lopq_eval.hip) on the GPU, beside the torch matmul formulation of bench.py::exact_nn.

Shapes: 8192 x 1M x 128 float32 (the queries of a run against one C2-sized chunk) and 1024 x 1M x 4096 (DeepSentibank width).
Each figure is the median of repetitions that add up to at least 0.5 s, timed with HIP events on the stream the work runs on,
after one untimed call (workspace growth).  The torch formulation -- max dot product of unit vectors, float32, ties as the
library breaks them -- streams the data in 256k-row chunks so that its score matrix stays at 8 GB.

    python tools/bench_exact_nn.py [--out profiles/exact_nn.json] [--small]

Prints one JSON line per shape: seconds, the fraction of the 155 TFLOP/s float32 matrix rate that 2 m1 m2 d flop in that time
amount to, and the share of queries on which the two answers agree.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MATRIX = 155e12  # measured v_mfma_f32_32x32x2_f32 rate of one MI355X


def timed(fn, min_s=0.5, max_reps=50):
    import torch
    fn()
    torch.cuda.synchronize()
    ts, total = [], 0.0
    while total < min_s and len(ts) < max_reps:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
        total += ts[-1]
    ts.sort()
    return ts[len(ts) // 2], len(ts), out


def torch_nn(q, x, chunk=262144):
    import torch
    best = torch.full((q.shape[0],), -2.0, device=q.device, dtype=torch.float32)
    arg = torch.zeros(q.shape[0], dtype=torch.int64, device=q.device)
    for a in range(0, x.shape[0], chunk):
        v, i = (q @ x[a:a + chunk].t()).max(dim=1)
        upd = v > best
        best = torch.where(upd, v, best)
        arg = torch.where(upd, i + a, arg)
    return arg


def main():
    import torch
    from columbiaimagesearch_amd.lopq import eval as ev
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1/16 of the rows (a quick look)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = 1 << 20 >> (4 if args.small else 0)
    results = []
    for m1, m2, d in ((8192, rows, 128), (1024, rows, 4096)):
        g = torch.Generator(device=dev).manual_seed(m1 + d)
        x = torch.randn((m2, d), device=dev, dtype=torch.float32, generator=g)
        x /= x.norm(dim=1, keepdim=True)
        q = torch.randn((m1, d), device=dev, dtype=torch.float32, generator=g)
        q /= q.norm(dim=1, keepdim=True)
        t_hip, n_hip, (idx, _) = timed(lambda: ev.exact_neighbors(q, x, 1))
        stats = ev.exact_stats()
        t_torch, n_torch, arg = timed(lambda: torch_nn(q, x))
        flop = 2.0 * m1 * m2 * d
        r = {"shape": [m1, m2, d], "dtype": "float32", "k": 1, "exact_neighbors_s": t_hip, "exact_neighbors_reps": n_hip,
             "exact_neighbors_fraction_of_155TF": flop / t_hip / PEAK_F32_MATRIX, "torch_matmul_s": t_torch, "torch_matmul_reps": n_torch,
             "torch_matmul_fraction_of_155TF": flop / t_torch / PEAK_F32_MATRIX,
             "exact_only_queries_last_pass": stats[1], "rows_rescored_last_pass": stats[2],
             "agreement": float((idx[:, 0] == arg).float().mean().item()), "device": torch.cuda.get_device_name(0)}
        print(json.dumps(r), flush=True)
        results.append(r)
        del x, q
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
