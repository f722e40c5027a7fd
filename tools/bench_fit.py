"""A whole LOPQ fit at the release shape, stage by stage (the table of DESIGN.md section 5.6).

  python tools/bench_fit.py                       # LOPQModel(V=2048, M=8).fit on 2 M x 128, n_init = 1 and 10, host seeds
  python tools/bench_fit.py --seed device         # the k-means++ seeds drawn on the GPU (train.SEED_BACKEND)
  python tools/bench_fit.py --rotations device    # the local-rotation stage on the device as well (train.ROTATION_BACKEND)
  python tools/bench_fit.py --n-init 1 --n 500000 --out fit.json

KMEANS_BACKEND = "device", ACCUM_BACKEND = "hip", 10 coarse / 20 local iterations, descriptor-like float32 unit vectors (the
generator of tests/golden_inputs.py).  Wall clock with a device synchronise around each stage; the stages are the functions of
lopq/train.py, timed from outside: k-means = _kmeans (all 10 codebooks), of which seeding = kmeans_pp_init / kmeans_pp_init_dev;
assignment = assign_clusters_dev; accumulations = gram_hip; projections = project_to_local; the host's eigh and
eigenvalue_allocation; rest = total minus these.  With --rotations device the same names time the device forms: assignment =
_assign_dev, accumulations = gram_dev, projections = project_to_local_dev (its residuals included), eigh = sym_eig_dev and
eigenvalue_allocation = eigenvalue_allocation_batch."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np


class Stages(object):
    def __init__(self):
        self.t = {}

    def wrap(self, owner, name, stage):
        import torch
        fn = getattr(owner, name)

        def timed(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                torch.cuda.synchronize()
                self.t[stage] = self.t.get(stage, 0.0) + time.perf_counter() - t0

        setattr(owner, name, timed)


def fit(X, n_init, seed_backend, rotations="host"):
    import torch
    from columbiaimagesearch_amd.lopq import LOPQModel
    from columbiaimagesearch_amd.lopq import train as T
    T.KMEANS_BACKEND, T.ACCUM_BACKEND = "device", "hip"
    T.SEED_BACKEND = seed_backend
    T.ROTATION_BACKEND = rotations
    st = Stages()
    keep = {}
    stages = [(T, "_kmeans", "kmeans"), (T, "kmeans_pp_init", "seeding"), (T, "kmeans_pp_init_dev", "seeding")]
    if rotations == "device":
        stages += [(T, "_assign_dev", "assignment"), (T, "gram_dev", "accumulations"), (T, "project_to_local_dev", "projections"),
                   (T, "sym_eig_dev", "eigh"), (T, "eigenvalue_allocation_batch", "eigenvalue_allocation")]
    else:
        stages += [(T, "assign_clusters_dev", "assignment"), (T, "gram_hip", "accumulations"), (T, "project_to_local", "projections"),
                   (np.linalg, "eigh", "eigh"), (T, "eigenvalue_allocation", "eigenvalue_allocation")]
    for owner, name, stage in stages:
        if hasattr(owner, name):
            keep[(owner, name)] = getattr(owner, name)
            st.wrap(owner, name, stage)
    try:
        m = LOPQModel(V=2048, M=8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.fit(X, kmeans_coarse_iters=10, kmeans_local_iters=20, n_init=n_init, random_state=1)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
    finally:
        for (owner, name), fn in keep.items():
            setattr(owner, name, fn)
        T.ROTATION_BACKEND = "host"
    r = {"n_init": n_init, "seed_backend": seed_backend, "rotations": rotations, "total_s": total}
    r.update({k + "_s": v for k, v in st.t.items()})
    r["rest_s"] = total - sum(v for k, v in st.t.items() if k != "seeding")
    sample = X[:2000].astype(np.float64)
    co, fi = m.predict_batch(sample)
    rec = np.stack([m.reconstruct((tuple(c), tuple(f))) for c, f in zip(co, fi)])
    r["reconstruction_error"] = float(((rec - sample) ** 2).sum(1).mean())
    print(json.dumps(r), flush=True)
    return r


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--n-init", type=int, action="append")
    ap.add_argument("--seed", choices=("host", "device"), default="host")
    ap.add_argument("--rotations", choices=("host", "device"), default="host")
    ap.add_argument("--out")
    a = ap.parse_args()
    import golden_inputs as gi
    X = np.concatenate([gi.descriptor_like(min(250000, a.n - s), 128, 1000 + s, np.float32) for s in range(0, a.n, 250000)])
    import logging
    logging.disable(logging.WARNING)  # (the warm-up's clusters are too small for a rotation, and say so 4096 times)
    fit(X[:50000], 1, a.seed, a.rotations)  # warm-up: the library, the workspaces' first allocations
    logging.disable(logging.NOTSET)
    results = [fit(X, ni, a.seed, a.rotations) for ni in (a.n_init or [1, 10])]
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_fit.py", "n": a.n, "results": results}, f, indent=1)
            f.write("\n")
