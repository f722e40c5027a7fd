"""The PCA stage of training, train.train_pca, at the release shape (200 000 x 4096 float32 rows -> 256 dimensions) under three settings,
and cis_sym_eig_large_dev alone.

  python tools/bench_pca_fit.py [--n 200000] [--d 4096] [--pca-dims 256] [--solver-dims 512,1024,2048,4096] [--skip-host] [--out pca.json]

Legs, on the same rows (64 strong directions with log-normal scales over unit noise, made on the device and copied to the host once):
  host/host    PCA_BACKEND = "host", ACCUM_BACKEND = "host": numpy's product and numpy.linalg.eigh.  One run, wall clock.
  host/hip     PCA_BACKEND = "host", ACCUM_BACKEND = "hip": the sums through cis_train_gram on host pointers.  One run, wall clock.
  device       PCA_BACKEND = "device" from the same numpy array (the upload is part of it): the wall clock of train_pca with a device
               synchronisation at either end, repeated until the repetitions add up to 0.5 s; the median, and train_pca_dev's own
               stage times (upload, sums, eigensolver, rest; each stage waits for the device), its block sweeps and, against numpy
               on the device's own A, the three error figures in units of d u.
The host legs take seconds each, so a single run stands for them; that is stated in the output as "runs": 1.
The solver alone: covariances of 4 d Gaussian rows with log-normal column scales at each d of --solver-dims, blocks of 32 and of 64
columns; HIP events around one call (the call itself waits once per block sweep), after one warm-up call per block size at d = 256,
repeated until the repetitions add up to 0.5 s; the median and the block sweeps."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

U = 2.0 ** -53


def rows(n, d, seed=11):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    k = min(64, d)
    basis = torch.randn((k, d), dtype=torch.float32, device="cuda", generator=g) / d ** 0.5
    scale = torch.exp(torch.randn(k, dtype=torch.float32, device="cuda", generator=g)) * 8.0
    out = torch.empty((n, d), dtype=torch.float32, device="cuda")
    for a in range(0, n, 32768):
        b = min(n, a + 32768) - a
        z = torch.randn((b, k), dtype=torch.float32, device="cuda", generator=g) * scale
        out[a:a + b] = z @ basis + torch.randn((b, d), dtype=torch.float32, device="cuda", generator=g)
    return out.cpu().numpy()


def host_leg(T, X, dims, accum):
    keep = (T.PCA_BACKEND, T.ACCUM_BACKEND)
    try:
        T.PCA_BACKEND, T.ACCUM_BACKEND = "host", accum
        t0 = time.perf_counter()
        T.train_pca(X, dims)
        return {"leg": "host/" + accum, "seconds": time.perf_counter() - t0, "runs": 1}
    finally:
        T.PCA_BACKEND, T.ACCUM_BACKEND = keep


def device_leg(T, X, dims):
    import torch
    keep = T.PCA_BACKEND
    times, stats, out = [], [], None
    try:
        T.PCA_BACKEND = "device"
        T.train_pca(X[:4096, :256], 16)  # warm-up: the kernels are loaded
        while sum(times) < 0.5:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, _ = T.train_pca(X, dims)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        for _ in range(len(times)):  # the stages, in runs of their own: their synchronisations are not in the total above
            s = {}
            T.train_pca_dev(X, dims, stats=s)
            stats.append(s)
    finally:
        T.PCA_BACKEND = keep
    med = lambda k: float(np.median([s[k] for s in stats]))
    A = out["A"]
    D = A.shape[0]
    W, V, info = T.sym_eig_large_dev(torch.from_numpy(A).cuda())
    Ad = torch.from_numpy(A).cuda()
    ref = np.linalg.eigvalsh(A)
    norm = float(np.abs(ref).max())
    res = float((Ad @ V - V * W).abs().amax().cpu()) / (D * U * norm)
    orth = float((V.T @ V - torch.eye(D, dtype=torch.float64, device="cuda")).abs().amax().cpu()) / (D * U)
    eig = float(np.abs(W.cpu().numpy() - ref).max()) / (D * U * norm)
    return {"leg": "device", "seconds": float(np.median(times)), "runs": len(times),
            "upload_s": med("upload_s"), "sums_s": med("sums_s"), "eigensolver_s": med("eig_s"), "rest_s": med("rest_s"),
            "block_sweeps": int(stats[0]["block_sweeps"]), "residual_du": res, "orthogonality_du": orth, "eigenvalues_du": eig}


def covariance(d, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((4 * d, d), dtype=torch.float64, device="cuda", generator=g)
    x = x * torch.exp(torch.randn((1, d), dtype=torch.float64, device="cuda", generator=g))
    x = x - x.mean(dim=0, keepdim=True)
    c = x.T @ x / (4 * d - 1)
    return (c + c.T) / 2


def solver_alone(T, d, block):
    import torch
    A = covariance(d, 1000 + d)
    times = []
    while sum(times) < 0.5:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        W, V, info = T.sym_eig_large_dev(A, block)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    times.sort()
    resid = float(((A @ V - V * W).abs().amax() / A.abs().amax()).cpu())
    return {"d": d, "block": block, "median_s": times[len(times) // 2], "min_s": times[0], "max_s": times[-1], "repetitions": len(times),
            "block_sweeps": int(info.cpu()[0]), "relative_residual": resid}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--pca-dims", type=int, default=256)
    ap.add_argument("--solver-dims", default="512,1024,2048,4096")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from columbiaimagesearch_amd.lopq import train as T
    results = {"tool": "tools/bench_pca_fit.py", "n": a.n, "d": a.d, "pca_dims": a.pca_dims, "legs": [], "solver": []}
    for block in (32, 64):
        T.sym_eig_large_dev(covariance(256, 1), block)
    torch.cuda.synchronize()
    for d in [int(x) for x in a.solver_dims.split(",") if x]:
        for block in (32, 64):
            results["solver"].append(solver_alone(T, d, block))
            print(json.dumps(results["solver"][-1]), flush=True)
    X = rows(a.n, a.d)
    legs = [lambda: device_leg(T, X, a.pca_dims)]
    if not a.skip_host:
        legs += [lambda: host_leg(T, X, a.pca_dims, "host"), lambda: host_leg(T, X, a.pca_dims, "hip")]
    for leg in legs:
        results["legs"].append(leg())
        print(json.dumps(results["legs"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
