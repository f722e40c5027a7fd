"""The dlib face ResNet in the precisions "bf16x3" and "bf16": csrc/cnn_bf16_direct.hip (the direct 16-bit kernel of the 35x35x32 and
17x17x64 layers) and the residual epilogue of csrc/cnn_bf16.hip.  Single layers go through featurizer.conv3x3_dev, which routes a layer
as the forward does; the network through DLibFaceNet(weights, precision=...).  References: torch conv2d in float64 on the CPU and
tests/cnn_probe.py; the host-side split is t.to(torch.bfloat16)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_probe as P

gpu = pytest.mark.gpu
PRECISIONS = ["bf16x3", "bf16"]
#          N  H=W   C   OC stride pad resC relu
SHAPES = [(2, 35, 32, 32, 1, 1, 32, 1),      # direct C = 32
          (3, 17, 64, 64, 1, 1, 64, 1),      # direct C = 64; image borders fall inside a workgroup's range
          (3, 17, 64, 64, 1, 1, 32, 1),      # the fused down block: the residual has fewer channels
          (2, 17, 64, 64, 1, 1, 0, 0),       # direct C = 64 without residual or ReLU
          (2, 35, 32, 64, 2, 0, 0, 1),       # stride 2, implicit GEMM
          (2, 8, 128, 128, 1, 1, 64, 1),     # small map with residual
          (2, 4, 256, 256, 1, 1, 256, 1),    # K = 2304: the K split with residual
          (2, 4, 256, 256, 2, 0, 0, 1)]      # dl[27], output 1 x 1
ids = lambda s: "x".join(str(int(v)) for v in s)


def conv64(a, w, shape):
    """a [N,C,H,W], w OIHW (float32 values) -> float64 [N,OH,OW,OC]"""
    return F.conv2d(torch.from_numpy(a).double(), torch.from_numpy(w).double(), None, shape[4], shape[5]).permute(0, 2, 3, 1).numpy()


def split(t):
    t = torch.from_numpy(t)
    hi = t.to(torch.bfloat16).float()
    return hi.numpy(), (t - hi).to(torch.bfloat16).float().numpy()


def run_layer(a, w, b, res, shape, precision):
    from columbiaimagesearch_amd.featurizer import conv3x3_dev
    x = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()
    r = torch.from_numpy(res).cuda() if res is not None else None
    return conv3x3_dev(x, w, b, shape[4], shape[5], shape[7], precision, res=r).cpu().numpy()


@functools.lru_cache(maxsize=None)
def lattice_layer(shape):
    """test_cnn_bf16.lattice_layer with a residual: integer activations of 11 bits, weights m / 1024 with four taps per output channel,
    integer biases and residuals: every sum is exact in float32 in any order"""
    N, HW, C, OC, stride, pad, resC, relu = shape
    rs = np.random.RandomState(7)
    a = rs.randint(-2047, 2048, size=(N, C, HW, HW)).astype(np.float32)
    w = np.zeros((OC, C * 9), dtype=np.float32)
    for o in range(OC):
        w[o, rs.choice(C * 9, 4, replace=False)] = rs.choice(np.r_[-1023:0, 1:1024], 4) / 1024.0
    w = w.reshape(OC, C, 3, 3)
    b = rs.randint(-8, 9, size=OC).astype(np.float32)
    (a_hi, a_lo), (w_hi, w_lo) = split(a), split(w)
    assert (a_hi + a_lo == a).all() and (w_hi + w_lo == w).all() and (a_lo != 0).mean() > 0.5 and (w_lo != 0).any()
    full = conv64(a, w, shape)
    res = rs.randint(-16, 17, size=full.shape[:3] + (resC,)).astype(np.float32) if resC else None
    tail = b + (np.pad(res, ((0, 0),) * 3 + ((0, OC - resC),)) if resC else 0.0)
    want = {"bf16x3": full - conv64(a_lo, w_lo, shape) + tail, "bf16": conv64(a_hi, w_hi, shape) + tail}
    for v in want.values():
        assert (v.astype(np.float32) == v).all()
    assert (want["bf16x3"] != full + tail).any() and (want["bf16"] != want["bf16x3"]).any()
    return a, w, b, res, want


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape,no_direct", [(s, False) for s in SHAPES] + [(SHAPES[0], True), (SHAPES[2], True)],
                         ids=lambda v: ids(v) if isinstance(v, tuple) else ("igemm" if v else "routed"))
def test_lattice_layers_are_exact(monkeypatch, shape, no_direct, precision):
    """bf16x3 = conv(a, w) - conv(a_lo, w_lo) + bias + res and bf16 = conv(a_hi, w_hi) + bias + res, bit for bit, on the route the
    forward takes for the shape; the two "igemm" cases send a direct shape through the implicit GEMM's own residual epilogue
    (CIS_CNN_NO_DIRECT, the A/B switch).  Equality assumes what test_cnn_bf16 assumes of the MFMA; it holds on an MI355X."""
    if no_direct:
        monkeypatch.setenv("CIS_CNN_NO_DIRECT", "1")
    a, w, b, res, want = lattice_layer(shape)
    exp = want[precision].astype(np.float32)
    np.testing.assert_array_equal(run_layer(a, w, b, res, shape, precision), np.maximum(exp, 0) if shape[7] else exp)


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES[:2], ids=ids)
def test_dense_layers_within_the_split_bound(shape, precision):
    """Gaussian operands, no residual: |got - conv64(a, w)| <= (c_p + (NS * K + 2) * 2^-23) * conv64(|a|, |w|) element by element,
    c_p = 3 * 2^-16 for bf16x3 and 2^-7 + 2^-16 for bf16 (derived in test_cnn_bf16).
    Seen on an MI355X (printed, pytest -s): largest |err| / S = 0.052, 0.032 of c_p for the two shapes in bf16x3 and
    0.126, 0.095 of c_p in bf16."""
    N, HW, C, OC, stride, pad, resC, relu = shape
    K = C * 9
    rs = np.random.RandomState(11)
    a = rs.randn(N, C, HW, HW).astype(np.float32)
    w = (rs.randn(OC, C, 3, 3) / np.sqrt(K)).astype(np.float32)
    ref, S = conv64(a, w, shape), conv64(np.abs(a), np.abs(w), shape)
    ns, cp = (3, 3 * 2.0 ** -16) if precision == "bf16x3" else (1, 2.0 ** -7 + 2.0 ** -16)
    ratio = np.abs(run_layer(a, w, None, None, shape[:7] + (0,), precision).astype(np.float64) - ref) / S
    print("%s %s: largest |err| / S = %.3g = %.3f * c_p" % (shape, precision, ratio.max(), ratio.max() / cp))
    assert (ratio <= cp + (ns * K + 2) * 2.0 ** -23).all(), ratio.max()


@functools.lru_cache(maxsize=None)
def bf16_model(which):
    """cnn_probe.dlib_forward_torch in float64 with the input and the (affine-folded, as the library folds them) weights of every
    convolution that runs in 16-bit rounded to bf16: both convolutions of blocks 0 ... 12 and the first of block 13"""
    probes, _, k = P.dlib_probes()
    w, chips = probes[which][2].weights(), P.dlib_chips_from_k(k)
    T = lambda name: torch.from_numpy(w[name])
    bf = lambda t: t.float().to(torch.bfloat16).double()
    pad_to = lambda t, s: F.pad(t, (0, s[3] - t.shape[3], 0, s[2] - t.shape[2], 0, s[1] - t.shape[1]))

    def conv(x, wn, bn, gn, betan, s, p, rounded):
        wf, bias = (T(wn) * T(gn).view(-1, 1, 1, 1)).double(), (T(gn) * T(bn) + T(betan)).double()
        return F.conv2d(bf(x), bf(wf), bias, s, p) if rounded else F.conv2d(x, wf, bias, s, p)
    x = torch.from_numpy(chips).float().permute(0, 3, 1, 2)
    x = ((x - torch.from_numpy(P.DLIB_MEAN).view(1, 3, 1, 1)) / 256.0).double()
    x = F.max_pool2d(F.relu(conv(x, "conv0_w", "conv0_b", "aff0_g", "aff0_b", 2, 0, False)), 3, 2)
    for i, (cin, cout, down) in enumerate(P.DLIB_PLAN):
        n = "b%d" % i
        y = F.relu(conv(x, n + "a_w", n + "a_b", n + "a_g", n + "a_beta", 2 if down else 1, 0 if down else 1, True))
        y = conv(y, n + "b_w", n + "b_b", n + "b_g", n + "b_beta", 1, 1, i < 13)
        skip = F.avg_pool2d(x, 2, 2) if down else x
        shape = [y.shape[0]] + [max(p, q) for p, q in zip(y.shape[1:], skip.shape[1:])]
        x = F.relu(pad_to(y, shape) + pad_to(skip, shape))
    return (x.mean(dim=(2, 3)) @ T("fc_w").double().t()).numpy()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("which", range(len(P.DLIB_SETS)))
def test_dlib_probe_features_are_exact(which, precision):
    """bf16x3 returns the probes' exact float64 reference bit for bit, as the float32 forward does (every activation that enters a 3x3
    convolution is exactly hi + lo and the weights have no lo); bf16 returns bf16_model bit for bit, which differs from the exact
    reference (asserted), so a forward that silently ran float32 fails.  Same bits alone, reversed, on the device and through a view."""
    from columbiaimagesearch_amd.featurizer import DLibFaceNet
    probes, _, k = P.dlib_probes()
    _, _, p, ref = probes[which]
    chips = P.dlib_chips_from_k(k)
    want = ref.astype(np.float32)
    if precision == "bf16":
        want = bf16_model(which).astype(np.float32)
        assert (want.astype(np.float64) == bf16_model(which)).all() and (want != ref.astype(np.float32)).any()
    net = DLibFaceNet(p.weights(), precision=precision)
    try:
        assert net.precision == precision
        np.testing.assert_array_equal(net.forward(chips), want)
        np.testing.assert_array_equal(net.forward(chips[3:4]), want[3:4])
        np.testing.assert_array_equal(net.forward(chips[::-1].copy()), want[::-1])
        np.testing.assert_array_equal(net.forward_dev(torch.from_numpy(chips).cuda()).cpu().numpy(), want)
        v = net.view()
        assert v.precision == precision
        np.testing.assert_array_equal(v.forward(chips), want)
        v.close()
    finally:
        net.close()


@gpu
def test_precision_surface(tmp_path):
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.featurizer import DLibFaceNet, DLibHIPFeaturizer, synthetic
    w, x = synthetic.dlib_weights(), synthetic.dlib_chips(3)
    with pytest.raises(ValueError):
        DLibFaceNet(w, precision="fp16")
    a, b = DLibFaceNet(w), DLibFaceNet(w, precision="f32")
    assert a.precision == b.precision == "f32"
    np.testing.assert_array_equal(a.forward(x), b.forward(x))
    c = DLibFaceNet(w, precision="bf16x3")
    v = c.view()
    assert _lib.lib().cis_cnn_precision(c._h) == _lib.lib().cis_cnn_precision(v._h) == 1
    for n in (v, a, b, c):
        n.close()
    np.savez(str(tmp_path / "w.npz"), **w)
    f = DLibHIPFeaturizer({"D_rec_path": str(tmp_path / "w.npz"), "D_pred_path": "unused", "D_precision": "bf16"}, prefix="D_")
    assert f.net.precision == "bf16"
    f.net.close()
