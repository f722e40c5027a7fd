"""The HOG face detector (csrc/hog_detector.hip): cis_fhogdet_run_dev with a synthetic model of the dimensions of
dlib's frontal face detector (5 filters of 10 x 10 cells, pyramid_down<6>) on 480 x 640 and 1080 x 1920 random-texture images at
up_sample 0 and 1: the time of one call, the per-stage times from HIP events (cis_fhogdet_profile), and images per second with four
calls in flight on four streams (four workspaces).  No threshold is set on these numbers: nothing here can run dlib to compare against.

  python tools/bench_hog_detector.py [--out profiles/hog_detector_bench.json] [--listing columbiaimagesearch_amd/csrc/build/hog_detector.s]

HIP events around one call; after a warm-up call the call is repeated until the repetitions add up to 0.5 s (at least 5), and the median
is reported.  The register and LDS figures are read from the kernels' metadata in the listing
(`make -C columbiaimagesearch_amd/csrc build/hog_detector.s`)."""
import argparse
import ctypes
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STAGES = ("resizes", "cell_histograms", "features", "scores", "sort_nms")


def timed(call, sync):
    import torch
    call()  # warm-up
    sync()
    times = []
    while len(times) < 5 or sum(times) < 0.5:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        sync()
        times.append(e0.elapsed_time(e1) / 1e3)
    times.sort()
    return {"median_s": times[len(times) // 2], "min_s": times[0], "max_s": times[-1], "repetitions": len(times)}


def listing_figures(path):
    """per kernel: vgpr_count, LDS bytes, scratch bytes, spills and the workgroups per CU they allow, from the metadata of a -S listing"""
    if not os.path.exists(path):
        return {"listing": None}
    text = open(path).read()
    meta = text[text.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
    out = {"listing": os.path.relpath(path, REPO)}
    for entry in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", entry, flags=re.M).group(1)
        name = re.search(r"k_[a-z]+(?:_[a-z]+)*", name).group(0)   # out of the mangled name
        get = lambda k: int(re.search(r"^\s+\.%s:\s+(\d+)" % k, entry, flags=re.M).group(1))
        vgpr, lds, threads = get("vgpr_count"), get("group_segment_fixed_size"), get("max_flat_workgroup_size")
        waves = min(8, 512 // max(-(-vgpr // 8) * 8, 8))
        by_vgpr = waves * 4 // max(threads // 64, 1)
        by_lds = (160 * 1024) // lds if lds else 32
        out[name] = {"vgpr_count": vgpr, "sgpr_count": get("sgpr_count"), "lds_bytes": lds, "scratch_bytes": get("private_segment_fixed_size"),
                     "vgpr_spills": get("vgpr_spill_count"), "threads": threads, "waves_per_simd_by_vgpr": waves,
                     "workgroups_per_cu": min(by_vgpr, by_lds, 32)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--listing", default=os.path.join(REPO, "columbiaimagesearch_amd", "csrc", "build", "hog_detector.s"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.detector import HOGDetectorHIP
    from columbiaimagesearch_amd.featurizer.synthetic import fhog_detector_model
    model = fhog_detector_model(seed=0)
    det = HOGDetectorHIP(model)
    L = _lib.lib()
    results = {"tool": "tools/bench_hog_detector.py", "model": {"F": model.F, "filter": [model.filter_rows, model.filter_cols], "pyramid_n": model.pyramid_n},
               "kernels": listing_figures(a.listing), "cases": []}
    rs = np.random.RandomState(1)
    for nr, nc in ((480, 640), (1080, 1920)):
        img = torch.as_tensor(rs.randint(0, 256, size=(nr, nc, 3)).astype(np.uint8)).cuda()
        for up in (0, 1):
            need = det.workspace_bytes(nr, nc, up)
            ws = [torch.empty(need, dtype=torch.uint8, device="cuda") for _ in range(4)]
            streams = [torch.cuda.Stream() for _ in range(4)]
            one = timed(lambda: det.run_dev(img, up, workspace=ws[0]), torch.cuda.synchronize)
            rects, scores, filt, count = det.run_dev(img, up, workspace=ws[0])
            kept, cands = (int(v) for v in count.cpu().numpy())
            ms = (ctypes.c_float * 5)()
            stage = []
            for _ in range(7):
                _lib.check(L.cis_fhogdet_profile(det._h, img.data_ptr(), nr, nc, up, 0.0, ws[0].data_ptr(), need, rects.data_ptr(), scores.data_ptr(),
                                                 filt.data_ptr(), int(rects.shape[0]), count.data_ptr(), torch.cuda.current_stream().cuda_stream, ms))
                stage.append(list(ms))
            stage_s = {name: sorted(s[i] for s in stage)[len(stage) // 2] / 1e3 for i, name in enumerate(STAGES)}

            def four():
                for k in range(4):
                    streams[k].wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(streams[k]):
                        det.run_dev(img, up, workspace=ws[k])
                for k in range(4):
                    torch.cuda.current_stream().wait_stream(streams[k])

            inflight = timed(four, torch.cuda.synchronize)
            r = {"image": [nr, nc], "up_sample": up, "workspace_bytes": need, "kept": kept, "candidates": cands, "one_call": one,
                 "stage_s": stage_s, "dominant_stage": max(stage_s, key=stage_s.get), "four_in_flight": inflight,
                 "images_per_s_one_stream": 1.0 / one["median_s"], "images_per_s_four_streams": 4.0 / inflight["median_s"]}
            results["cases"].append(r)
            print(json.dumps(r), flush=True)
    print(json.dumps(results["kernels"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
