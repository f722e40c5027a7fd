#!/usr/bin/env python3
"""Cycles per phase of a k_adc_scan4 slot, from the S3_CTR stamps of csrc/lopq_scan3.hip (wave 0 of every workgroup adds, at the end of
each phase, the clock ticks since the slot began).  Needs a library built with the stamps:
    tools/build_variant.sh ctr -DCIS_S3_COUNTERS lopq_scan3
    CIS_LIB_PATH=columbiaimagesearch_amd/lib/libcis_ctr.so python3 tools/debug_counters3.py --config c4 [--out FILE]
Builds the index of a bench.py configuration (c4: 10M vectors, 39 k-candidate cells, the long-chunk form; c2: 1M, 3.9 k-candidate cells,
the short-chunk form; c3: 1M vectors at M = 16, the long-chunk form with the saturating scale), runs `--batches` batches of 8192 queries
after a warm-up batch and prints ticks per slot and phase.  The stamps cost an atomic each and the fall-back launch (k_adc_scan3, normally
without slots) adds to the same counters: the figures are shares of a slot, not a benchmark."""
import argparse, ctypes, json, os, sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (counter index, phase that ends there) in the order a slot passes them; every stamp holds ticks since the slot began
PHASES = [(11, "staging issued: tables -> LDS, the sample's code rows requested"),
          (2, "B1: tables visible"),
          (3, "B2: sample pass"),
          (4, "B3: thresholds (one wave per query)"),
          (13, "main pass (wave 0's share of the rows)"),
          (12, "second gather of the recorded candidates"),
          (5, "B4: lists complete (waits for the slowest wave)"),
          (6, "B5: verification, cut, write-out (one wave per query)")]


def read_counters(lib, reset):
    out = (ctypes.c_ulonglong * 16)()
    rc = lib.cis_debug_counters3(out, 1 if reset else 0)
    if rc != 0:
        raise RuntimeError("cis_debug_counters3 failed (%d)" % rc)
    return [int(v) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["c4", "c2", "c3"], default="c4")
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--nq", type=int, default=8192)
    ap.add_argument("--out", help="also write the table here (appended)")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    import torch
    import bench as B
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    lib = _lib.lib()
    if not hasattr(lib, "cis_debug_counters3"):
        sys.exit("%s has no cis_debug_counters3: build lopq_scan3.hip with -DCIS_S3_COUNTERS (tools/build_variant.sh)" % _lib.LIB_PATH)
    lib.cis_debug_counters3.restype = ctypes.c_int
    lib.cis_debug_counters3.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    cfg = B.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    model, _ = B.load_model(cfg["fixture"])
    P = B.mixture_centers(cfg["gen"], dev)
    n, chunk_n = cfg["n"], (100_000 if cfg["d_in"] > 1024 else 1_000_000)
    s = LOPQSearcherHIP(model)
    for c in range(n // chunk_n):
        co, fi = model.predict_batch_dev(B.gen_chunk(P, c, chunk_n, dev))
        s.add_codes_dev(co, fi, torch.arange(c * chunk_n, (c + 1) * chunk_n, dtype=torch.int64, device=dev), dedup=False)
    x0 = B.gen_chunk(P, 0, chunk_n, dev)
    s.search_batch_dev(B.make_queries(x0, 0, a.nq, dev), quota=10000, limit=100)  # warm-up
    torch.cuda.synchronize()
    kernel = s.last_stats()["scan_kernel"]
    read_counters(lib, True)
    for b in range(a.batches):
        s.search_batch_dev(B.make_queries(x0, 1 + b, a.nq, dev), quota=10000, limit=100)
    torch.cuda.synchronize()
    ctr = read_counters(lib, True)
    slots, wgs = max(ctr[0], 1), max(ctr[10], 1)
    end = ctr[6] / slots
    lines = ["%s %s: %s, %d batches of %d queries, %d slots, %d workgroups; library %s" % (a.label, a.config, kernel, a.batches, a.nq, ctr[0], ctr[10],
                                                                                       os.path.basename(_lib.LIB_PATH)),
             "%10s %10s %7s  phase (ticks of the shader clock counter per slot, wave 0)" % ("until", "phase", "share")]
    prev = 0.0
    for idx, name in PHASES:
        t = ctr[idx] / slots
        lines.append("%10.0f %10.0f %6.1f%%  %s" % (t, t - prev, 100.0 * (t - prev) / end if end else 0.0, name))
        prev = t
    lines.append("%10.0f ticks per workgroup in the kernel, %.1f slots per workgroup" % (ctr[9] / wgs, slots / wgs))
    lines.append("raw " + json.dumps(ctr))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n\n")
    s.close()


if __name__ == "__main__":
    main()
