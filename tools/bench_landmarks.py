"""The landmark predictor beside the network it feeds: cis_shapepred_run_dev with a synthetic model of the
dimensions of dlib's 68-point model (P = 68, K = 15, T = 500, depth 4, F = 500) on a 1080 x 1920 image at n = 256 and n = 1
rectangles (and at 1024 and 4096: several workgroups per CU), and DLibFaceNet.forward_dev at 256 chips in the same process.

  python tools/bench_landmarks.py [--out profiles/landmarks_bench.json] [--listing columbiaimagesearch_amd/csrc/build/shape_predictor.s]

HIP events around one call; after a warm-up call the call is repeated until the repetitions add up to 0.5 s (at least 5), and the median
is reported.  The leaf-read rate is the bytes the sum over the trees has to read, n K T 2P 4, over the predictor's time: an effective
rate of the whole kernel, not of its last phase.  The register and LDS figures are read from the kernel's metadata in the listing
(`make -C columbiaimagesearch_amd/csrc build/shape_predictor.s`)."""
import argparse
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DIMS = dict(P=68, K=15, T=500, depth=4, F=500)


def timed(call):
    import torch
    call()  # warm-up
    torch.cuda.synchronize()
    times = []
    while len(times) < 5 or sum(times) < 0.5:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / 1e3)
    times.sort()
    return {"median_s": times[len(times) // 2], "min_s": times[0], "max_s": times[-1], "repetitions": len(times)}


def listing_figures(path):
    """vgpr_count, LDS bytes, scratch bytes and spills of k_shape_predict from the amdhsa.kernels metadata of a -S listing"""
    if not os.path.exists(path):
        return {"listing": None}
    text = open(path).read()
    meta = text[text.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""
    for entry in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:
        if "k_shape_predict" not in entry:
            continue
        get = lambda k: int(re.search(r"^\s+\.%s:\s+(\d+)" % k, entry, flags=re.M).group(1))
        vgpr = get("vgpr_count")
        alloc = -(-vgpr // 8) * 8
        lds = get("group_segment_fixed_size")
        waves_vgpr, groups_lds = min(8, 512 // alloc), (160 * 1024) // lds
        return {"listing": os.path.relpath(path, REPO), "vgpr_count": vgpr, "sgpr_count": get("sgpr_count"), "lds_bytes": lds,
                "scratch_bytes": get("private_segment_fixed_size"), "vgpr_spills": get("vgpr_spill_count"),
                "waves_per_simd_by_vgpr": waves_vgpr, "workgroups_per_cu_by_lds": groups_lds,
                "workgroups_of_256_per_cu": min(waves_vgpr, groups_lds, 8)}
    return {"listing": os.path.relpath(path, REPO), "error": "no k_shape_predict in the listing"}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--listing", default=os.path.join(REPO, "columbiaimagesearch_amd", "csrc", "build", "shape_predictor.s"))
    a = ap.parse_args()
    import numpy as np
    import torch
    from columbiaimagesearch_amd.featurizer import DLibFaceNet
    from columbiaimagesearch_amd.featurizer.shape_predictor import ShapePredictorHIP
    from columbiaimagesearch_amd.featurizer.synthetic import dlib_weights, shape_predictor_model
    model = shape_predictor_model(seed=0, **DIMS)
    sp = ShapePredictorHIP(model)
    rs = np.random.RandomState(1)
    img = torch.as_tensor(rs.randint(0, 256, size=(1080, 1920, 3)).astype(np.uint8)).cuda()
    side = rs.randint(100, 400, size=4096)
    left, top = rs.randint(0, 1920 - side), rs.randint(0, 1080 - side)
    rects = torch.as_tensor(np.stack([left, top, left + side, top + side], axis=1).astype(np.int32)).cuda()
    leaf_bytes = DIMS["K"] * DIMS["T"] * 2 * DIMS["P"] * 4
    results = {"tool": "tools/bench_landmarks.py", "model": dict(DIMS, leaf_table_bytes=int(model.leaves.nbytes)), "image": [1080, 1920],
               "kernel": listing_figures(a.listing), "predictor": []}
    for n in (256, 1, 1024, 4096):
        r = timed(lambda: sp.predict_dev(img, rects[:n]))
        r.update(n=n, faces_per_s=n / r["median_s"], leaf_read_bytes_per_s=n * leaf_bytes / r["median_s"])
        results["predictor"].append(r)
        print(json.dumps(r), flush=True)
    net = DLibFaceNet(dlib_weights(0))
    chips = (torch.rand(256, 150, 150, 3, device="cuda") * 255).contiguous()
    out = torch.empty(256, 128, device="cuda")
    r = timed(lambda: net.forward_dev(chips, out))
    r.update(n=256, faces_per_s=256 / r["median_s"])
    results["network"] = r
    print(json.dumps(r), flush=True)
    results["predictor_over_network_faces_per_s"] = results["predictor"][0]["faces_per_s"] / r["faces_per_s"]
    print(json.dumps({"kernel": results["kernel"], "predictor_over_network_faces_per_s": results["predictor_over_network_faces_per_s"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
