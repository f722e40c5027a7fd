"""cis_sym_eig_dev alone (the kernel row of DESIGN.md section 5.6): batches of covariance matrices at the two training shapes,
4096 x 64^2 (V = 2048, two halves of 128 dimensions) and 8192 x 128^2 (the Sentibank release configuration).

  python tools/bench_sym_eig.py [--out sym_eig.json]

The matrices are covariances of 4 d Gaussian rows with log-normal column scales, made on the device.  HIP events around one call;
after a warm-up call the call is repeated until the repetitions add up to 0.5 s (at least 5), and the median is reported with the
sweep counts d_info returned."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def covariances(batch, d, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((batch, d, d), dtype=torch.float64, device="cuda")
    for a in range(0, batch, 512):  # in slices: 4 d rows of d doubles per matrix
        b = min(batch, a + 512) - a
        x = torch.randn((b, 4 * d, d), dtype=torch.float64, device="cuda", generator=g)
        x = x * torch.exp(torch.randn((b, 1, d), dtype=torch.float64, device="cuda", generator=g))
        x = x - x.mean(dim=1, keepdim=True)
        c = x.transpose(1, 2) @ x / (4 * d - 1)
        out[a:a + b] = (c + c.transpose(1, 2)) / 2
    return out


def measure(batch, d):
    import torch
    from columbiaimagesearch_amd.lopq import train as T
    A = covariances(batch, d, 1000 + d)
    W, V, info = T.sym_eig_dev(A)  # warm-up
    torch.cuda.synchronize()
    times = []
    while len(times) < 5 or sum(times) < 0.5:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        W, V, info = T.sym_eig_dev(A)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    times.sort()
    info = info.cpu()
    resid = float(((A[:64] @ V[:64] - V[:64] * W[:64, None, :]).abs().amax() / A[:64].abs().amax()).cpu())
    r = {"batch": batch, "d": d, "median_s": times[len(times) // 2], "min_s": times[0], "max_s": times[-1], "repetitions": len(times),
         "matrices_per_s": batch / times[len(times) // 2], "sweeps_min": int(info.min()), "sweeps_max": int(info.max()),
         "sweeps_mean": float(info.double().mean()), "failed": int((info < 0).sum()), "relative_residual_of_64": resid}
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    a = ap.parse_args()
    results = [measure(4096, 64), measure(8192, 128)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_sym_eig.py", "results": results}, f, indent=1)
            f.write("\n")
