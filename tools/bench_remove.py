"""Removal by id (csrc/lopq_remove.hip) on resident indexes: ms per cis_index_remove_dev call for 1, 256, 65 536 and 1M random stored
ids, split into set build / mark / touched list + compaction (HIP events inside the library: cis_index_remove_profile), next to two
yardsticks -- the physical floor of the mark pass (8 B x the layout's slots at the Infinity-Cache rate while the ids fit its 256 MiB,
at the HBM rate beyond; rates of MI355X measurements: 8.6 TB/s cache-resident gathers, 6.29 TB/s HBM copy) and the only alternative
without removal, timed in the same run: a fresh index plus add_codes_dev of all kept items from resident tensors.

Shapes: the C4 index (10M x M = 8, V = 16: 256 cells of ~39 k items), a V = 2048 index of 10M (4.2 M tiny cells: the thread-per-cell
mark and the wave-per-cell compaction) and, with --c4x N, a C4-shaped index of N items (one workgroup walks a ~N / 256-item cell).
Every repetition removes inside the timed window (HIP events around the call) and re-inserts the removed items outside it; the
median of repetitions that add up to >= 0.5 s is reported.  --switch also times 64 ... 1024 ids with the hash table forced
(CIS_REMOVE_LDS_MAX=0) against the sorted list in LDS: where the two forms of the removal set cross.

usage: python tools/bench_remove.py [--out profiles/remove_bench.json] [--c4x 200000000] [--switch] [--shapes c4,v2048]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench as B
from columbiaimagesearch_amd import _lib
from columbiaimagesearch_amd.lopq import LOPQModel, LOPQSearcherHIP

HBM_BPS, MALL_BPS, MALL_BYTES = 6.29e12, 8.6e12, 256 * 2 ** 20
dev = torch.device("cuda", 0)


def random_model(V, M=8, K=256, D=32, seed=0):
    rs = np.random.RandomState(seed)
    h, w, nf = D // 2, D // M, M // 2
    Cs = tuple(rs.randn(V, h).astype(np.float32) for _ in range(2))
    Rs = tuple(np.broadcast_to(np.eye(h), (V, h, h)).copy() for _ in range(2))
    mus = tuple(np.zeros((V, h)) for _ in range(2))
    subs = tuple([rs.randn(K, w) for _ in range(nf)] for _ in range(2))
    return LOPQModel(parameters=(Cs, Rs, mus, subs))


def build(model, N, g):
    V, M = model.V, model.M
    s = LOPQSearcherHIP(model)
    parts = []
    for a in range(0, N, 10_000_000):
        n = min(10_000_000, N - a)
        co = torch.randint(0, V, (n, 2), generator=g, device=dev, dtype=torch.int16)
        fi = torch.randint(0, 256, (n, M), generator=g, device=dev, dtype=torch.uint8)
        s.add_codes_dev(co, fi, torch.arange(a, a + n, dtype=torch.int64, device=dev), dedup=False)
        parts.append((co, fi))
    co = torch.cat([p[0] for p in parts]) if len(parts) > 1 else parts[0][0]
    fi = torch.cat([p[1] for p in parts]) if len(parts) > 1 else parts[0][1]
    torch.cuda.synchronize()
    return s, co, fi


def timed_removal(s, co, fi, sel, min_total_ms=500.0, min_reps=5, max_reps=20000):
    L = _lib.lib()
    times, stages = [], []
    prof = np.zeros(3, dtype=np.float64)
    total = 0.0
    for rep in range(max_reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        removed = s.remove_ids_dev(sel)
        e1.record()
        torch.cuda.synchronize()
        assert removed == sel.shape[0], (removed, sel.shape[0])
        _lib.check(L.cis_index_remove_profile(s._ix, _lib.ptr(prof)))
        added, bad = s.add_codes_dev(co[sel].contiguous(), fi[sel].contiguous(), sel, dedup=False)  # outside the window: the state repeats
        assert added == sel.shape[0]
        torch.cuda.synchronize()
        if rep < 2:
            continue  # warm-up: workspaces sized, code objects loaded
        ms = e0.elapsed_time(e1)
        times.append(ms); stages.append(prof.copy()); total += ms
        if len(times) >= min_reps and total >= min_total_ms:
            break
    st = np.median(np.array(stages), axis=0)
    return {"ms": float(np.median(times)), "reps": len(times), "set_ms": float(st[0]), "mark_ms": float(st[1]), "compact_ms": float(st[2])}


def bench_shape(tag, model, N, counts, g, rebuild_alt=True, switch=False):
    s, co, fi = build(model, N, g)
    s.set_profiling(True, scan_only=True)
    V, M = model.V, model.M
    slots = int(N + N // 8 + 32 * V * V) if V * V <= 65536 else int(N + N // 8 + 2 * V * V)  # upper bound of the layout's extent
    id_bytes = 8 * N
    rate = MALL_BPS if id_bytes <= MALL_BYTES else HBM_BPS
    out = {"shape": tag, "N": N, "V": V, "M": M, "cells": V * V, "rows": [],
           "mark_floor_ms": id_bytes / rate * 1e3,
           "mark_floor_basis": "8 B x %d stored items at %s" % (N, "8.6 TB/s (80 MB of ids fit the 256 MiB Infinity Cache)" if rate == MALL_BPS
                                                               else "6.29 TB/s (HBM: the ids exceed the Infinity Cache)"),
           "layout_slots_bound": slots}
    for k in counts:
        sel = torch.randperm(N, generator=g, device=dev)[:k].contiguous()
        row = {"ids": k}
        row.update(timed_removal(s, co, fi, sel))
        if rebuild_alt:
            keep = torch.ones(N, dtype=torch.bool, device=dev); keep[sel] = False
            ck, fk, ik = co[keep].contiguous(), fi[keep].contiguous(), torch.nonzero(keep).reshape(-1).contiguous()
            alt = []
            for rep in range(3):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                s2 = LOPQSearcherHIP(model)
                s2.add_codes_dev(ck, fk, ik, dedup=False)
                e1.record(); torch.cuda.synchronize()
                alt.append(e0.elapsed_time(e1))
                s2.close()
            row["fresh_index_ms"] = float(np.median(alt))
            del ck, fk, ik, keep
        print("%s N %d: remove %7d ids %.3f ms (set %.3f, mark %.3f, list + compact %.3f; %d reps)  mark floor %.3f ms  fresh index + insert of the kept %s ms"
              % (tag, N, k, row["ms"], row["set_ms"], row["mark_ms"], row["compact_ms"], row["reps"], out["mark_floor_ms"],
                 ("%.2f" % row["fresh_index_ms"]) if "fresh_index_ms" in row else "-"), flush=True)
        out["rows"].append(row)
    if switch:
        out["switch"] = []
        for k in (64, 256, 512, 1024):
            sel = torch.randperm(N, generator=g, device=dev)[:k].contiguous()
            r = {"ids": k}
            for form, env in (("lds", None), ("table", "0")):
                if env is None:
                    os.environ.pop("CIS_REMOVE_LDS_MAX", None)
                else:
                    os.environ["CIS_REMOVE_LDS_MAX"] = env
                t = timed_removal(s, co, fi, sel, min_total_ms=200.0)
                r[form + "_ms"], r[form + "_set_ms"], r[form + "_mark_ms"] = t["ms"], t["set_ms"], t["mark_ms"]
            os.environ.pop("CIS_REMOVE_LDS_MAX", None)
            print("%s set form at %4d ids: sorted list in LDS %.3f ms (mark %.3f), hash table %.3f ms (mark %.3f)"
                  % (tag, k, r["lds_ms"], r["lds_mark_ms"], r["table_ms"], r["table_mark_ms"]), flush=True)
            out["switch"].append(r)
    s.close()
    del s, co, fi
    torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "remove_bench.json"))
    ap.add_argument("--c4x", type=int, default=0)
    ap.add_argument("--switch", action="store_true")
    ap.add_argument("--shapes", default="c4,v2048")
    ap.add_argument("--n", type=int, default=10_000_000)
    args = ap.parse_args()
    g = torch.Generator(device=dev); g.manual_seed(1)
    results = {"device": torch.cuda.get_device_name(0), "shapes": []}
    shapes = args.shapes.split(",")
    if "c4" in shapes:
        model, z = B.load_model("c4")
        results["shapes"].append(bench_shape("c4", model, args.n, [1, 256, 65536, 1_000_000], g, switch=args.switch))
    if "v2048" in shapes:
        results["shapes"].append(bench_shape("v2048", random_model(2048), args.n, [1, 256, 65536, 1_000_000], g))
    if args.c4x:
        model, z = B.load_model("c4")
        results["shapes"].append(bench_shape("c4x", model, args.c4x, [256, 1_000_000], g, rebuild_alt=False))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(results, f, indent=1)
    print("wrote", args.out)
