"""csrc/cnn_bf16.hip: DeepSentibank's GEMM layers on the 16-bit matrix cores, as the precisions "bf16x3" (operands split into
bf16 hi + lo, three products) and "bf16" (hi * hi alone).  Single layers go through featurizer.conv2d_dev, the network through
SentiBankNet(weights, precision=...).  References: torch conv2d in float64 on the CPU and tests/cnn_probe.py; the host-side
split is t.to(torch.bfloat16)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_probe as P

gpu = pytest.mark.gpu
PRECISIONS = ["bf16x3", "bf16"]
#          N  H=W   C    OC  k  stride pad groups nchw
SHAPES = [(2, 9, 96, 80, 5, 1, 2, 2, False),      # conv2's form: ICg = 48, OCg = 40 a partial channel tile, padded borders
          (3, 7, 32, 64, 3, 1, 1, 1, False),      # 147 pixels: a partial pixel tile
          (1, 13, 16, 32, 3, 2, 0, 1, False),     # stride 2, K = 144
          (5, 1, 2304, 96, 1, 1, 0, 1, False),    # the fc form with its K split
          (2, 51, 3, 96, 11, 4, 0, 1, True),      # the first layer: K = 363, runs that end at the end of the input
          (1, 3, 8, 4, 3, 1, 1, 1, False)]        # K and OC below one tile


def conv64(a, w, shape):
    """a [N,C,H,W], w OIHW (float32 values) -> float64 [N,OH,OW,OC]"""
    N, HW, C, OC, k, stride, pad, groups, nchw = shape
    return F.conv2d(torch.from_numpy(a).double(), torch.from_numpy(w).double(), None, stride, pad, 1, groups).permute(0, 2, 3, 1).numpy()


def split(t):
    t = torch.from_numpy(t)
    hi = t.to(torch.bfloat16).float()
    return hi.numpy(), (t - hi).to(torch.bfloat16).float().numpy()


def run_layer(a, w, b, shape, relu, precision):
    from columbiaimagesearch_amd.featurizer import conv2d_dev
    N, HW, C, OC, k, stride, pad, groups, nchw = shape
    x = torch.from_numpy(a if nchw else np.ascontiguousarray(a.transpose(0, 2, 3, 1))).cuda()
    return conv2d_dev(x, w, b, stride, pad, groups, relu, precision, nchw=nchw).cpu().numpy()


@functools.lru_cache(maxsize=None)
def lattice_layer(shape):
    """integer activations of 11 bits, weights m / 1024 with four taps per output channel, integer biases: every sum is exact
    in float32 in any order (all terms are multiples of 2^-10 and a row's magnitudes sum below 2^24 steps)"""
    N, HW, C, OC, k, stride, pad, groups, nchw = shape
    rs = np.random.RandomState(7)
    a = rs.randint(-2047, 2048, size=(N, C, HW, HW)).astype(np.float32)
    w = np.zeros((OC, (C // groups) * k * k), dtype=np.float32)
    for o in range(OC):
        taps = rs.choice(w.shape[1], 4, replace=False)
        w[o, taps] = rs.choice(np.r_[-1023:0, 1:1024], 4) / 1024.0
    w = w.reshape(OC, C // groups, k, k)
    b = rs.randint(-8, 9, size=OC).astype(np.float32)
    (a_hi, a_lo), (w_hi, w_lo) = split(a), split(w)
    assert (a_hi + a_lo == a).all() and (w_hi + w_lo == w).all() and (a_lo != 0).mean() > 0.5 and (w_lo != 0).any()
    want = {"bf16x3": conv64(a, w, shape) - conv64(a_lo, w_lo, shape) + b, "bf16": conv64(a_hi, w_hi, shape) + b}
    for v in want.values():
        assert (v.astype(np.float32) == v).all()
    assert (want["bf16x3"] != conv64(a, w, shape) + b).any() and (want["bf16"] != want["bf16x3"]).any()
    return a, w, b, want


@gpu
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_lattice_layers_are_exact(shape, precision, relu):
    """bf16x3 = conv(a, w) - conv(a_lo, w_lo) + bias and bf16 = conv(a_hi, w_hi) + bias, bit for bit: index maps, operand planes,
    the three products (a dropped or doubled one changes most outputs), the K tail, split-K, bias and ReLU.  Equality assumes that
    the MFMA adds its sixteen products and the accumulator without losing bits that fit in 24: it holds on an MI355X."""
    a, w, b, want = lattice_layer(shape)
    exp = want[precision].astype(np.float32)
    np.testing.assert_array_equal(run_layer(a, w, b, shape, relu, precision), np.maximum(exp, 0) if relu else exp)


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "x".join(str(int(v)) for v in s))
def test_dense_layers_within_the_split_bound(shape, precision):
    """Gaussian operands: |got - conv64(a, w)| <= (c_p + n * 2^-23) * conv64(|a|, |w|) element by element, n = NS * K + 2 terms,
    c_p = 3 * 2^-16 (two residues and the dropped lo * lo) for bf16x3 and 2^-7 + 2^-16 for bf16.
    Seen on an MI355X (printed, pytest -s): largest |err| / S = 0.024, 0.045, 0.044 of c_p for the three shapes in bf16x3 and
    0.077, 0.158, 0.129 of c_p in bf16."""
    N, HW, C, OC, k, stride, pad, groups, nchw = shape
    K = (C // groups) * k * k
    rs = np.random.RandomState(11)
    a = rs.randn(N, C, HW, HW).astype(np.float32)
    w = (rs.randn(OC, C // groups, k, k) / np.sqrt(K)).astype(np.float32)
    ref, S = conv64(a, w, shape), conv64(np.abs(a), np.abs(w), shape)
    ns, cp = (3, 3 * 2.0 ** -16) if precision == "bf16x3" else (1, 2.0 ** -7 + 2.0 ** -16)
    ratio = np.abs(run_layer(a, w, None, shape, 0, precision).astype(np.float64) - ref) / S
    print("%s %s: largest |err| / S = %.3g = %.3f * c_p" % (shape, precision, ratio.max(), ratio.max() / cp))
    assert (ratio <= cp + (ns * K + 2) * 2.0 ** -23).all(), ratio.max()


@gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("which", range(P.SENTIBANK_SETS))
def test_sentibank_probe_within_the_split_bound(which, precision):
    """The whole network on the probe weights.  The images are integers (lo = 0) and conv1's weights are +-1/2 and +-1/4: exact up
    to norm1.  From conv2 on a layer adds a relative error of at most u_p = 2^-16 (bf16x3) or 2^-8 (bf16) through the split of its
    input, norm2 amplifies conv2's by at most 1.75 (cnn_probe), conv3 ... fc7 add one each:
    |got - ref64| <= (6.75 * u_p + SENTIBANK_C * 2^-24) * |ref64|, and an exact 0 where the reference is 0.
    Seen on an MI355X: 1.4e-5 (bf16x3, bound 1.06e-4) and 7.4e-3 (bf16, bound 2.64e-2) at the most over the three sets.
    Also: equal bits alone, reversed and in the batch; forward_dev and a view give the bits of forward."""
    from columbiaimagesearch_amd.featurizer import SentiBankNet
    probes, _, x = P.sentibank_probes()
    seed, p, ref = probes[which]
    bound = 6.75 * (2.0 ** -16 if precision == "bf16x3" else 2.0 ** -8) + P.SENTIBANK_C * P.U
    net = SentiBankNet(p.weights(), precision=precision)
    try:
        assert net.precision == precision
        got = net.forward(x)
        for g, r in ((got, ref), (net.forward(x[2:3]), ref[2:3])):
            zero = r == 0
            assert g.dtype == np.float32 and (g[zero] == 0).all()
            rel = np.abs(g[~zero].astype(np.float64) - r[~zero]) / np.abs(r[~zero])
            print("set %d %s: largest relative deviation %.3g (bound %.3g)" % (which, precision, rel.max(), bound))
            assert (rel <= bound).all(), rel.max()
        for i in (0, 4):
            np.testing.assert_array_equal(net.forward(x[i:i + 1])[0], got[i])
        np.testing.assert_array_equal(net.forward(x[::-1].copy()), got[::-1])
        np.testing.assert_array_equal(net.forward_dev(torch.from_numpy(x).cuda()).cpu().numpy(), got)
        v = net.view()
        assert v.precision == precision
        np.testing.assert_array_equal(v.forward(x), got)
        v.close()
    finally:
        net.close()


@gpu
def test_precision_surface(tmp_path):
    from columbiaimagesearch_amd import _lib
    from columbiaimagesearch_amd.featurizer import DLibFaceNet, SentiBankHIPImgFeaturizer, SentiBankNet, synthetic
    w, x = synthetic.sentibank_weights(), synthetic.sentibank_images(3)
    with pytest.raises(ValueError):
        SentiBankNet(w, precision="fp16")
    a, b = SentiBankNet(w), SentiBankNet(w, precision="f32")
    assert a.precision == b.precision == "f32"
    np.testing.assert_array_equal(a.forward(x), b.forward(x))
    v, d = a.view(), DLibFaceNet(synthetic.dlib_weights())
    for h in (v._h, d._h):
        assert _lib.lib().cis_cnn_set_precision(h, 1) == _lib.CIS_EINVAL and _lib.last_error()
    for n in (v, a, b, d):
        n.close()
    np.savez(str(tmp_path / "w.npz"), **w)
    np.save(str(tmp_path / "mean.npy"), np.zeros((3, 256, 256), dtype=np.float32))
    conf = {"SB_sbcaffe_path": str(tmp_path / "w.npz"), "SB_imgmean_path": str(tmp_path / "mean.npy"), "SB_precision": "bf16"}
    f = SentiBankHIPImgFeaturizer(conf, prefix="SB_")
    assert f.net.precision == "bf16"
    f.net.close()
