"""Time the DeepSentibank forward (or, with --dlib, the dlib face ResNet's) at batch 256 on the GPU in the precisions of the network
(f32, bf16x3, bf16).

  python tools/bench_cnn.py [BATCH] [--precision P ...] [--layers] [--deviation] [--out profiles/cnn_precision.json]
  python tools/bench_cnn.py --dlib [BATCH] [--layers] [--deviation] [--out profiles/cnn_precision_dlib.json]

Every figure is a median of repetitions that add up to >= 0.5 s, timed with device events, three runs of each so that the spread
is on record.  Reported per precision: one batch at a time; four batches in flight (the net and three views on
streams.lane_streams, all precisions in this one process, so the float32 forward beside them is the yardstick); with --layers
the seven GEMM layers one by one through cis_cnn_conv_dev (device time of the layer's launches as the library measures it: the
call itself packs weights, so each figure is the median of 7 single launches, NOT of half a second of them); with --deviation
how far the descriptors move: |f_p - f_f32| / max|f_f32| on synthetic weights and images, and the share of LOPQ codes of the
c3full golden model that change.  "of peak" is useful work (2 * MACs) over the stated peak: 157.3 TFLOP/s for the float32 matrix
instructions, 2516.6 TFLOP/s (the vendor's dense bf16 figure) for both 16-bit precisions, although bf16x3 issues three products.
--dlib: the same forward figures for DLibFaceNet; --layers times the distinct 3x3 layer shapes through cis_cnn_conv3x3_dev (median of
7 single launches) and, on the two direct shapes, the 16-bit direct kernel against the 16-bit implicit GEMM on the same input
(CIS_CNN_NO_DIRECT, read per call); --deviation is |f_p - f_f32| / max|f_f32| on synthetic weights and chips.
"""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from columbiaimagesearch_amd import _lib
from columbiaimagesearch_amd.featurizer import DLibFaceNet, SentiBankNet, conv2d_dev, conv3x3_dev
from columbiaimagesearch_amd.featurizer.synthetic import dlib_chips, dlib_weights, sentibank_images, sentibank_weights
from columbiaimagesearch_amd.streams import lane_streams

SENTIBANK_MACS = 720310816
PEAK = {"f32": 157.3e12, "bf16x3": 2516.6e12, "bf16": 2516.6e12}
#          name    H    C     OC    k  s  p  g  nchw
LAYERS = [("conv1", 227, 3, 96, 11, 4, 0, 1, True), ("conv2", 27, 96, 256, 5, 1, 2, 2, False), ("conv3", 13, 256, 384, 3, 1, 1, 1, False),
          ("conv4", 13, 384, 384, 3, 1, 1, 2, False), ("conv5", 13, 384, 256, 3, 1, 1, 2, False), ("fc6", 1, 9216, 4096, 1, 1, 0, 1, False),
          ("fc7", 1, 4096, 4096, 1, 1, 0, 1, False)]

#               name          H    C   OC  s  p  resC   (the distinct 3x3 shapes of the dlib net that run in 16-bit)
DLIB_LAYERS = [("35x35x32", 35, 32, 32, 1, 1, 32), ("17x17x64", 17, 64, 64, 1, 1, 64), ("35->17 s2", 35, 32, 64, 2, 0, 0),
               ("17->8 s2", 17, 64, 128, 2, 0, 0), ("8x8x128", 8, 128, 128, 1, 1, 128), ("8->3 s2", 8, 128, 256, 2, 0, 0),
               ("3x3x256", 3, 256, 256, 1, 1, 0), ("4x4x256", 4, 256, 256, 1, 1, 256), ("4->1 s2", 4, 256, 256, 2, 0, 0)]


def dlib_macs():
    """multiply-adds of one chip: the first layer and the 28 3x3 convolutions as the block plan lays them out, and the fc"""
    macs, hw, c = 72 * 72 * 32 * 147, 35, 32
    for cin, cout, down in [(32, 32, 0)] * 3 + [(32, 64, 1)] + [(64, 64, 0)] * 3 + [(64, 128, 1)] + [(128, 128, 0)] * 2 + [(128, 256, 1)] + \
            [(256, 256, 0)] * 2 + [(256, 256, 1)]:
        oh = (hw - 3) // 2 + 1 if down else hw
        macs += oh * oh * cout * 9 * (cin + cout)
        hw = max(oh, (hw - 2) // 2 + 1) if down else hw
    return macs + 256 * 128


def median_ms(step, warmup=3, total=0.5):
    """step(): enqueue one repetition between the two events it returns"""
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    times = []
    while sum(times) < total * 1e3 or len(times) < 5:
        e0, e1 = step()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def one_at_a_time(net, x, out):
    def step():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        net.forward_dev(x, out)
        e1.record()
        return e0, e1
    return median_ms(step)


def four_in_flight(nets, xs, outs, lanes):
    main = torch.cuda.current_stream()

    def step():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(main)
        for net, x, out, s in zip(nets, xs, outs, lanes):
            s.wait_stream(main)
            with torch.cuda.stream(s):
                net.forward_dev(x, out)
        for s in lanes:
            main.wait_stream(s)
        e1.record(main)
        return e0, e1
    return median_ms(step) / len(nets)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("batch", nargs="?", type=int, default=256)
    ap.add_argument("--precision", action="append", choices=sorted(PEAK))
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--deviation", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dlib", action="store_true")
    a = ap.parse_args()
    B, precs = a.batch, a.precision or ["f32", "bf16x3", "bf16"]
    res = {"batch": B, "forward": {}, "layers": {}, "deviation": {}}
    if a.dlib:
        w, MACS = dlib_weights(0), dlib_macs()
        nets = {p: DLibFaceNet(w, precision=p) for p in precs}
        x = (torch.rand(B, 150, 150, 3, device="cuda") * 255).contiguous()
        out = torch.empty(B, 128, device="cuda")
    else:
        w, MACS = sentibank_weights(0), SENTIBANK_MACS
        nets = {p: SentiBankNet(w, precision=p) for p in precs}
        x = (torch.randn(B, 3, 227, 227, device="cuda") * 50).contiguous()
        out = torch.empty(B, 4096, device="cuda")
    for run in range(3):   # the precisions alternate inside a run
        for p in precs:
            res["forward"].setdefault(p, {"one_ms": [], "four_ms": []})["one_ms"].append(one_at_a_time(nets[p], x, out))
    lanes = lane_streams(4)
    xs, outs = [x] + [x.clone() for _ in range(3)], [out] + [torch.empty_like(out) for _ in range(3)]
    groups = {p: [nets[p]] + [nets[p].view() for _ in range(3)] for p in precs}
    for run in range(3):
        for p in precs:
            res["forward"][p]["four_ms"].append(four_in_flight(groups[p], xs, outs, lanes))
    for p in precs:
        f = res["forward"][p]
        for key in ("one_ms", "four_ms"):
            ms = float(np.median(f[key]))
            f[key[:-3] + "_of_peak"] = 2.0 * MACS * B / (ms * 1e-3) / PEAK[p]
            print("%-7s batch %d, %-4s: %.3f ms per batch (runs %s)  %.0f descriptors/s  %.3f of the %s peak" % (
                p, B, key[:-3], ms, " ".join("%.3f" % t for t in f[key]), B / ms * 1e3, f[key[:-3] + "_of_peak"], "f32" if p == "f32" else "bf16"))
    if a.layers and a.dlib:
        L = _lib.lib()
        L.cis_cnn_conv_dev_last_ms.restype = ctypes.c_float
        rs = np.random.RandomState(0)
        for name, H, C, OC, s, pad, resC in DLIB_LAYERS:
            xin = torch.randn((B, H, H, C), device="cuda")
            wl, bl = (rs.randn(OC, C, 3, 3) / np.sqrt(C * 9)).astype(np.float32), np.zeros(OC, dtype=np.float32)
            oh = (H + 2 * pad - 3) // s + 1
            r = torch.randn((B, oh, oh, resC), device="cuda") if resC else None
            macs = B * oh * oh * OC * C * 9
            direct = s == 1 and (H, C) in ((35, 32), (17, 64))
            for p in precs:
                for route in (["direct", "igemm"] if direct else ["routed"]):
                    if route == "igemm":
                        os.environ["CIS_CNN_NO_DIRECT"] = "1"
                    t = []
                    for _ in range(8):
                        conv3x3_dev(xin, wl, bl, s, pad, True, p, res=r)
                        t.append(float(L.cis_cnn_conv_dev_last_ms()))
                    os.environ.pop("CIS_CNN_NO_DIRECT", None)
                    ms = float(np.median(t[1:]))
                    res["layers"].setdefault(name, {}).setdefault(p, {})[route] = {"ms": ms, "min_ms": min(t[1:]), "max_ms": max(t[1:]), "of_peak": 2.0 * macs / (ms * 1e-3) / PEAK[p]}
                    print("%-10s %-7s %-6s %.4f ms (%.4f ... %.4f)  %.3f of peak" % (name, p, route, ms, min(t[1:]), max(t[1:]), res["layers"][name][p][route]["of_peak"]))
    elif a.layers:
        L = _lib.lib()
        L.cis_cnn_conv_dev_last_ms.restype = ctypes.c_float
        rs = np.random.RandomState(0)
        for name, H, C, OC, k, s, pad, g, nchw in LAYERS:
            xin = torch.randn((B, C, H, H) if nchw else (B, H, H, C), device="cuda")
            wl = (rs.randn(OC, C // g, k, k) / np.sqrt(C // g * k * k)).astype(np.float32)
            bl = np.zeros(OC, dtype=np.float32)
            oh = (H + 2 * pad - k) // s + 1
            macs = B * oh * oh * OC * (C // g) * k * k
            for p in precs:
                t = []
                for _ in range(8):
                    conv2d_dev(xin, wl, bl, s, pad, g, True, p, nchw=nchw)
                    t.append(float(L.cis_cnn_conv_dev_last_ms()))
                ms = float(np.median(t[1:]))
                res["layers"].setdefault(name, {})[p] = {"ms": ms, "of_peak": 2.0 * macs / (ms * 1e-3) / PEAK[p]}
                print("%-6s %-7s %.4f ms  %.3f of peak" % (name, p, ms, res["layers"][name][p]["of_peak"]))
    if a.deviation and a.dlib:
        chips = dlib_chips(256)
        base = nets["f32"].forward(chips) if "f32" in nets else DLibFaceNet(w).forward(chips)
        for p in precs:
            if p != "f32":
                dev = np.abs(nets[p].forward(chips).astype(np.float64) - base) / np.abs(base).max()
                res["deviation"][p] = {"max": float(dev.max()), "median": float(np.median(dev))}
                print("%-7s deviation %s" % (p, res["deviation"][p]))
    elif a.deviation:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        from conftest import load_golden
        from test_lopq_hip_parity import hip_model
        model = hip_model(load_golden("c3full")[0])
        imgs = sentibank_images(256)
        base = SentiBankNet(w).forward(imgs)
        c0, f0 = model.predict_batch(base / np.linalg.norm(base, axis=1, keepdims=True))
        for p in precs:
            if p == "f32":
                continue
            f = nets[p].forward(imgs)
            dev = np.abs(f.astype(np.float64) - base) / np.abs(base).max()
            c1, f1 = model.predict_batch(f / np.linalg.norm(f, axis=1, keepdims=True))
            res["deviation"][p] = {"max": float(dev.max()), "median": float(np.median(dev)), "fine_codes_changed": float((f1 != f0).mean()),
                                   "coarse_pairs_changed": float((c1 != c0).any(axis=1).mean())}
            print("%-7s deviation %s" % (p, res["deviation"][p]))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")


if __name__ == "__main__":
    main()
