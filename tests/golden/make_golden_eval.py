#!/usr/bin/env python3
"""Generate tests/golden/eval.npz: the outputs of the REAL reference eval.py (lopq/lopq/eval.py) and of scipy's cdist.

Runs only where the reference is present (see make_golden.py: the python-2 package is converted in a temporary directory
outside the repository; only data is written here).  Inputs come from seeds (tests/eval_cases.py); the fixture stores their
checksums.  The archive is written with fixed time stamps, so a second run reproduces the file byte for byte.

    python tests/golden/make_golden_eval.py
"""
import inspect
import io
import json
import os
import shutil
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import eval_cases as ec  # noqa: E402
from make_golden import import_reference, model_arrays  # noqa: E402

MIN_GAP = 1e-12


def ranked(dists, k):
    """Indices and distances of the k smallest (dist, index) per row, -1 / NaN padded."""
    m1, m2 = dists.shape
    idx = -np.ones((m1, k), dtype=np.int64)
    out = np.full((m1, k), np.nan)
    order = np.argsort(dists, axis=1, kind="stable")[:, :k]
    n = order.shape[1]
    idx[:, :n] = order
    out[:, :n] = np.take_along_axis(dists, order, axis=1)
    return idx, out


def min_relative_gap(dists):
    s = np.sort(dists, axis=1)
    if s.shape[1] < 2:
        return np.inf
    return float(np.min((s[:, 1:] - s[:, :-1]) / np.maximum(s[:, 1:], np.finfo(np.float64).tiny)))


def knn_entries(name, q, data, d, engineered):
    from scipy.spatial.distance import cdist
    from lopq.eval import compute_all_neighbors
    dists = cdist(q, data)
    if not engineered:
        gap = min_relative_gap(dists)
        assert gap > MIN_GAP, "%s: relative gap %g between ranked reference distances" % (name, gap)
    idx, dd = ranked(dists, ec.K)
    nn = compute_all_neighbors(q, data)  # the reference: np.argmin per row
    assert np.array_equal(nn, idx[:, 0]), name
    d[name + "_sha1"] = np.array(ec.sha1(q) + ec.sha1(data))
    d[name + "_idx"] = idx.astype(np.int32)
    d[name + "_dist"] = dd
    if data.shape[0] == 50:  # just_nn=False: the whole ranking (unique here: the gaps are asserted above)
        full = compute_all_neighbors(q, data, just_nn=False)
        assert np.array_equal(full, np.argsort(dists, axis=1, kind="stable")), name
        d[name + "_all"] = full.astype(np.int32)
    return dists


def check_engineered(cases, dists):
    q, data = cases["e_dup"]
    for tag in ("e_dup", "e_dup_f4"):
        dd = dists[tag]
        nn = int(np.argmin(dd[0]))
        same = np.nonzero(dd[0] == dd[0, nn])[0]
        assert list(same) == [nn, nn + 7, nn + 12], (tag, same)  # the true neighbour sits between its two copies
        assert dd[1, 17] == 0.0 and int(np.argmin(dd[1])) == 17, tag
    for tag in ("e_sqrt_d2", "e_sqrt_d66"):
        q, data = cases[tag]
        assert ec.chain_sq(q[0], data[0]) > ec.chain_sq(q[0], data[1]), tag  # row 0 is strictly farther before the root ...
        assert dists[tag][0, 0] == dists[tag][0, 1] and int(np.argmin(dists[tag][0])) == 0, tag  # ... and wins after it
        assert dists[tag][0, 0] == np.sqrt(ec.chain_sq(q[0], data[0])), tag
    assert np.all(dists["e_same"] == dists["e_same"][:, :1])


def model_entries(d):
    import lopq
    from lopq import LOPQModel, LOPQSearcher
    from lopq import eval as ref_eval
    from lopq.utils import compute_codes_notparallel
    X, Q = ec.model_inputs()
    m = LOPQModel(**ec.MODEL)
    m.fit(X, n_init=1, random_state=11)
    for k, v in model_arrays(m).items():
        d["m_" + k] = v
    d["m_inputs_sha1"] = np.array(ec.sha1(X) + ec.sha1(Q))
    s = LOPQSearcher(m)
    s.add_codes(compute_codes_notparallel(X, m))
    nns = ref_eval.compute_all_neighbors(Q, X)
    d["m_nns"] = nns.astype(np.int64)
    top = ec.THRESHOLDS[-1]
    res = -np.ones((len(Q), top), dtype=np.int64)
    for i, x in enumerate(Q):
        ids = [r[0] for r in s.search(x, top)[0]]
        res[i, :len(ids)] = ids
    d["m_results"] = res
    d["m_recall_norm"] = ref_eval.get_recall(s, Q, nns, thresholds=ec.THRESHOLDS, normalize=True)[0]
    d["m_recall_raw"] = ref_eval.get_recall(s, Q, nns, thresholds=ec.THRESHOLDS, normalize=False)[0]
    d["m_hist"] = ref_eval.get_cell_histogram(X, m).astype(np.int64)
    d["m_prop_nn"] = np.float64(ref_eval.get_proportion_nns_with_same_coarse_codes(X[:ec.N_SUB], m))
    d["m_prop_recon"] = np.float64(ref_eval.get_proportion_of_reconstructions_with_same_codes(X[:ec.N_SUB], m))
    d["m_distortion"] = ref_eval.get_subquantizer_distortion(X, m)
    sigs = {}
    for name in ("compute_all_neighbors", "get_proportion_nns_with_same_coarse_codes", "get_cell_histogram",
                 "get_proportion_of_reconstructions_with_same_codes", "get_recall", "get_subquantizer_distortion"):
        sig = inspect.signature(getattr(ref_eval, name))
        sigs[name] = [[p.name, None if p.default is inspect.Parameter.empty else ["default", p.default]] for p in sig.parameters.values()]
    d["signatures"] = np.array(json.dumps(sigs, sort_keys=True))


def write_npz(path, d):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(d):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(d[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def main():
    time.clock = time.perf_counter  # gone from Python 3; the reference's get_recall times with it
    tmp = import_reference()
    try:
        d = {}
        for name, dim, m2, m1, dt in ec.random_cases():
            q, data = ec.random_inputs(name, dim, m2, m1, dt)
            knn_entries(name, q, data, d, engineered=False)
        cases = ec.engineered_inputs()
        check_engineered(cases, {name: knn_entries(name, q, data, d, engineered=True) for name, (q, data) in cases.items()})
        model_entries(d)
        out = os.path.join(HERE, "eval.npz")
        write_npz(out, d)
        print("wrote eval.npz", os.path.getsize(out) // 1024, "KiB,", len(d), "arrays")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
