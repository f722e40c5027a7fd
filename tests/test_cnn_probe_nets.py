"""csrc/cnn.hip on probe networks (tests/cnn_probe.py) whose exact output is known: whole forwards compared for EQUALITY (dlib) or
within an element-wise bound of a few ulp (DeepSentibank, whose two LRN layers are not exact), on every route.

dlib: every comparison is assert_array_equal against the float64 index-map reference cast to float32.
DeepSentibank: |got - ref64| <= c * 2^-24 * |ref64| with c = cnn_probe.SENTIBANK_C = 51.8125 (derived in cnn_probe's docstring
by counting the roundings of k_maxpool_lrn_nhwc_v4; capped at 64), and an exact 0 where the reference is 0.  The largest
relative deviation measured on an MI355X (4.78 * 2^-24) is in test_sentibank_probe_within_the_derived_bound's docstring.

What the weight sets together observe, and what they do not, is asserted in
test_union_of_the_weight_sets_observes_the_edges_and_a_floor_of_taps.  The switches cnn.hip reads once per process
(CIS_CNN_NO_SPLITK, CIS_CNN_THREADS) are not exercised here.
"""
import numpy as np
import pytest

import cnn_probe as P

gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the builders check themselves
# ---------------------------------------------------------------------------------------------------------------------
def test_sentibank_bound_constant_is_the_derivation_and_below_its_cap():
    e1 = 8.75 + P.E_SQRT_ULP + 4 * P.E_RSQRT_ULP
    assert P.SENTIBANK_C == e1 * (2.0 + 1.5 * P.P_MAX / (1.0 + P.P_MAX)) + 0.25 == 51.8125
    assert P.SENTIBANK_C <= 64


def test_dlib_lattice_inputs_are_exact_and_a_shift_changes_the_result():
    probes, cover, k = P.dlib_probes()     # builds every set under lattice_guard: a sum that could round fails there
    x = P.dlib_chips_from_k(k)
    assert x.dtype == np.float32 and k.min() >= -12 and k.max() <= 3
    assert (np.diff(k, axis=2) != 0).mean() > 0.5 and (np.diff(k, axis=1) != 0).mean() > 0.5   # neighbouring pixels differ
    _, _, p, ref = probes[0]
    shifted = np.roll(k[:2], 1, axis=2)
    assert (p.forward(shifted) != ref[:2]).any(axis=1).all()
    for family, seed, p, ref in probes:
        assert np.isfinite(ref).all() and (ref != 0).mean() > 0.3, (family, seed)
        assert (ref.astype(np.float32).astype(np.float64) == ref).all()   # the features are float32 numbers


@pytest.mark.parametrize("which", [0, len(P.DLIB_SETS) - 1])
def test_dlib_index_map_reference_equals_both_torch_restatements(which):
    """the index-map reference against forward_torch of the oracle (float32: the lattice makes it exact too) and a float64
    copy of it: equal, not close"""
    from oracle import dlib_oracle as D
    probes, _, k = P.dlib_probes()
    family, seed, p, ref = probes[which]
    w, x = p.weights(), P.dlib_chips_from_k(k[:3])
    assert sorted(w) == sorted(D.tensor_names())
    np.testing.assert_array_equal(P.dlib_forward_torch(x, w), ref[:3])
    np.testing.assert_array_equal(D.forward_torch(x, w), ref[:3].astype(np.float32))


def test_sentibank_index_map_reference_against_the_oracles():
    """float64 numpy restatement of the oracle: equal up to float64 rounding of the LRN; float32 torch restatement: within
    1e-5 (its LRN takes ~20 float32 roundings per stage; a wrong index map is off by O(1))"""
    from oracle import cnn_oracle as C
    probes, _, x = P.sentibank_probes()
    seed, p, ref = probes[0]
    w = p.weights()
    for name, ws, bs in C.layer_shapes():
        assert w[name + "_w"].shape == ws and w[name + "_b"].shape == bs
    assert (ref[:2] >= 0).all() and (ref[:2] > 0).mean() > 0.5
    np.testing.assert_allclose(C.forward_numpy(x[:2], w), ref[:2], rtol=1e-12, atol=0)
    np.testing.assert_allclose(C.forward_torch(x[:2], w), ref[:2], rtol=1e-5, atol=0)
    shifted = np.roll(x[:1], 1, axis=3)
    assert (p.forward(shifted) != ref[:1])[ref[:1] != 0].mean() > 0.5


def _edges(pos):
    return {"first row": pos[0].any(), "last row": pos[-1].any(), "first column": pos[:, 0].any(), "last column": pos[:, -1].any()}


def test_union_of_the_weight_sets_observes_the_edges_and_a_floor_of_taps():
    """The observation masks of all weight sets together (cnn_probe: walked backwards from the features, a position counts only
    where a non-zero reference value flows through it).  The union is NOT every tap: the sets observe all of dlib's conv0, fc7
    and nearly all of fc6 and dlib's fc, but only 7 - 35 % of the (ky, kx, ic) triples of the 3 x 3 layers, because the negative
    beta that keeps dlib on the lattice clamps most branch values to 0, and a DeepSentibank handle per further set costs too
    much.  So a mistake confined to ONE tap of a deep layer is seen only if that tap is among the observed ones: a cnn.hip whose
    packing zeroes tap (2, 2) of input channel 63 of b5a, or tap (2, 2) of b5a's output channel 63, passes this file (the dense
    Gaussian weights of test_cnn_hip_parity.py see both).  Asserted, so that none of it can shrink unnoticed:
      - every kernel position (ky, kx) of every convolution in every group, and floors (below) for the share of observed
        (ky, kx, ic) triples, of input channels and of output channels per layer;
      - first and last output row and column of every convolution and pool, the column that only the clipped window of the
        72 -> 35 pool reads, and the odd-sized stride-2 blocks (35 -> 17, 17 -> 8, 8 -> 3, 3 -> 1);
      - the first zero-padded channel of every widening block and half of the padded range;
      - channels 0, 1, C - 2, C - 1 of both LRN layers.
    Cannot be observed by any weights: row and column 71 of dlib's conv0 (floor((72 - 3) / 2) + 1 = 35 pooled rows end at
    row 70) and the non-centre taps of b13b (a 1 x 1 map meets padding only).  Not observed by these sets: the last row of
    b2b (its values reach the output through few paths, all clamped); listed in GAPS, which may only shrink."""
    GAPS = {("b2b", "last row")}
    _, cover, _ = P.dlib_probes()
    assert cover[("tap", "conv0")].all() and cover[("tap", "fc")].mean() >= 0.99
    for name in ("conv0", "pool0", "fc"):
        assert cover[("chan", name)].all(), name
    for i, (cin, cout, down) in enumerate(P.DLIB_PLAN):
        for name in ("b%da" % i, "b%db" % i):
            tap, chan = cover[("tap", name)], cover[("chan", name)]
            kpos = tap.any(axis=2)
            assert kpos.all() if name != "b13b" else (kpos[1, 1] and kpos.sum() == 1), name
            reachable = tap if name != "b13b" else tap[1:2, 1:2]
            assert reachable.mean() >= 1.0 / 16, (name, reachable.mean())
            assert tap.any(axis=(0, 1)).mean() >= 0.4 and chan.mean() >= 0.5, name
            missing = {(name, e) for e, seen in _edges(cover[("pos", name)]).items() if not seen}
            assert missing <= GAPS, missing
        if cout > cin:
            pad = cover[("padchan", i)]
            assert pad[cin] and pad[cin:].mean() >= 0.5 and pad[:cin].mean() >= 0.85, i
    assert all(_edges(cover[("pos", "pool0")]).values())
    c0 = cover[("pos", "conv0")]
    assert c0[0].any() and c0[:, 0].any() and c0[70].any() and c0[:, 70].any() and not c0[71].any() and not c0[:, 71].any()
    for i in (3, 7, 10, 13):   # the 2 x 2 average of an odd-sized map: its last used row and column (the one behind is never read)
        a = cover[("pos", "avg%d" % i)]
        n = 2 * (a.shape[0] // 2)
        assert a[0].any() and a[:, 0].any() and a[n - 1].any() and a[:, n - 1].any(), i

    _, cover, _ = P.sentibank_probes()
    floor = {"conv1": 0.5, "conv2": 0.125, "conv3": 0.125, "conv4": 0.125, "conv5": 0.125, "fc6": 0.99, "fc7": 1.0}
    for name, cin, cout, k, stride, pad, groups in P.SB_CONVS:
        tap, chan = cover[("tap", name)], cover[("chan", name)]
        for g in range(groups):
            t = tap[:, :, g * (cin // groups):(g + 1) * (cin // groups)]
            assert t.mean() >= floor[name], (name, g, t.mean())
            assert t.any(axis=2).all() or name == "conv1", (name, g)
        assert chan.mean() >= (1.0 if name in ("conv5", "fc6", "fc7") else 0.8), name
        assert all(_edges(cover[("pos", name)]).values()), name
    assert cover[("tap", "conv1")].any(axis=2).mean() >= 0.9 and cover[("tap", "conv1")].any(axis=(0, 1)).all()
    for name in ("pool1", "norm1", "pool2", "norm2", "pool5"):
        assert all(_edges(cover[("pos", name)]).values()), name
    for name in ("norm1", "norm2"):
        assert cover[("chan", name)][[0, 1, -2, -1]].all(), name
    for seed, p, ref in P.sentibank_probes()[0]:
        assert (ref >= 0).all()     # what the relative bound of the GPU test divides by


# ---------------------------------------------------------------------------------------------------------------------
# GPU: dlib, bit-equal
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dlib_nets():
    from columbiaimagesearch_amd.featurizer import DLibFaceNet
    probes, _, k = P.dlib_probes()
    nets = [DLibFaceNet(p.weights()) for _, _, p, _ in probes]
    yield [(net, ref.astype(np.float32)) for net, (_, _, _, ref) in zip(nets, probes)], P.dlib_chips_from_k(k)
    for net in nets:
        net.close()


def _dlib_batch(chips, ref, n):
    idx = np.arange(n) % chips.shape[0]
    return np.ascontiguousarray(chips[idx]), ref[idx]


# CIS_CNN_NO_BIGTILE and CIS_CNN_SPLIT_TARGET change the tiling only where a layer has more than 2048 output pixels or is split
# along K: at these batch sizes that is the 8 x 8 maps at batch 34 (2176 pixels) and the split layers; elsewhere they repeat the default.
DLIB_ROUTES = [{}, {"CIS_CNN_NO_DIRECT": "1"}, {"CIS_CNN_DIRECT_CFG": "0"}, {"CIS_CNN_DIRECT_CFG": "1"}, {"CIS_CNN_DIRECT_CFG": "2"},
               {"CIS_CNN_NO_DIRECT7": "1"}, {"CIS_CNN_NO_POOL7": "1"}, {"CIS_CNN_NO_TAIL": "1"}, {"CIS_CNN_NO_BIGTILE": "1"},
               {"CIS_CNN_SPLIT_TARGET": "64"}, {"CIS_CNN_SPLIT_TARGET": "4096"}, {"CIS_CNN_PARTS": "1"}, {"CIS_CNN_PARTS": "2"},
               {"CIS_CNN_PARTS": "4"}, {"CIS_CNN_NO_TAIL": "1", "CIS_CNN_NO_DIRECT": "1", "CIS_CNN_NO_DIRECT7": "1"}]


@gpu
@pytest.mark.parametrize("route", DLIB_ROUTES, ids=lambda r: "+".join("%s=%s" % kv for kv in sorted(r.items())) or "default")
def test_dlib_probe_features_are_exact_on_every_route(monkeypatch, dlib_nets, route):
    """every weight set (selector and lattice), batches of 1, 5 and 34 (34 ends inside a workgroup's image range of the tail and
    of the first layer): the 128 features of every chip equal the reference bit for bit, wherever the chip sits in the batch"""
    nets, chips = dlib_nets
    for key, val in route.items():
        monkeypatch.setenv(key, val)
    for net, ref in nets:
        for n in (1, 5, 34):
            x, want = _dlib_batch(chips, ref, n)
            np.testing.assert_array_equal(net.forward(x), want)
        np.testing.assert_array_equal(net.forward(chips[::-1].copy()), ref[::-1])   # other places in the batch: same bits


@gpu
def test_dlib_probe_features_are_exact_as_a_graph_on_the_device_and_through_a_view(monkeypatch, dlib_nets):
    import torch
    nets, chips = dlib_nets
    for net, ref in nets:
        x, want = _dlib_batch(chips, ref, 34)
        xd = torch.from_numpy(x).cuda()
        out = torch.empty((34, 128), device="cuda")
        np.testing.assert_array_equal(net.forward_dev(xd).cpu().numpy(), want)
        for graph in ("0", "1"):
            monkeypatch.setenv("CIS_CNN_GRAPH", graph)
            for _ in range(4):   # launches, capture + launch, graph, graph
                out.fill_(-1.0)
                net.forward_dev(xd, out)
                np.testing.assert_array_equal(out.cpu().numpy(), want)
        monkeypatch.delenv("CIS_CNN_GRAPH")
    net, ref = nets[-1]           # (last: a view switches its base to whole-batch overlap)
    v = net.view()
    x, want = _dlib_batch(chips, ref, 5)
    np.testing.assert_array_equal(v.forward(x), want)
    np.testing.assert_array_equal(v.forward_dev(torch.from_numpy(x).cuda()).cpu().numpy(), want)
    v.close()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: DeepSentibank, within the derived bound
# ---------------------------------------------------------------------------------------------------------------------
def _within_bound(got, ref):
    """element by element; returns the largest relative deviation"""
    assert got.shape == ref.shape and got.dtype == np.float32
    zero = ref == 0
    assert (got[zero] == 0).all(), "an exact 0 where the reference is 0"
    rel = np.abs(got[~zero].astype(np.float64) - ref[~zero]) / np.abs(ref[~zero])
    worst = float(rel.max()) if rel.size else 0.0
    print("largest relative deviation %.3g = %.2f * 2^-24 (bound %.4f * 2^-24)" % (worst, worst / P.U, P.SENTIBANK_C))
    assert (rel <= P.SENTIBANK_C * P.U).all(), "largest relative deviation %.3g > %.3g" % (worst, P.SENTIBANK_C * P.U)
    return worst


SB_ROUTES = [{"CIS_CNN_NHWC_FIRST": "1"}, {"CIS_CNN_NO_BIGTILE": "1"}, {"CIS_CNN_NO_XCD_REMAP": "1"},
             {"CIS_CNN_SPLIT_TARGET": "64"}, {"CIS_CNN_SPLIT_TARGET": "4096"}, {"CIS_CNN_PARTS": "2"}, {"CIS_CNN_PARTS": "3"}]
SB_ROUTES += [{"CIS_CNN_FC_TILE": str(t)} for t in range(5)] + [{"CIS_CNN_FC_SPLITK": str(s)} for s in (1, 2, 4, 8, 16, 32)]


@gpu
@pytest.mark.parametrize("which", range(P.SENTIBANK_SETS))
def test_sentibank_probe_within_the_derived_bound(monkeypatch, which):
    """one selector weight set: batches of 5 and 1 within the bound; a picture's features do not depend on its place (equal
    bits); forward_dev and a view give the bits of forward; set 0 also runs every per-call route switch.
    Measured on an MI355X (not the bound): the largest relative deviation is 2.85e-7 = 4.78 * 2^-24 (set 1; 4.60 and 4.61
    for sets 0 and 2, the same on every route of set 0), an eleventh of c = 51.8125.  The slack is what the derivation
    grants sqrtf / rsqrtf (2 ulp each: 27.5 of the 51.8) and five worst-case fmaf roundings per stage.  Every comparison
    prints its figure (pytest -s)."""
    import torch
    from columbiaimagesearch_amd.featurizer import SentiBankNet
    probes, _, x = P.sentibank_probes()
    seed, p, ref = probes[which]
    net = SentiBankNet(p.weights())
    try:
        got = net.forward(x)
        _within_bound(got, ref)
        for i in (0, 4):
            np.testing.assert_array_equal(net.forward(x[i:i + 1])[0], got[i])
        np.testing.assert_array_equal(net.forward(x[::-1].copy()), got[::-1])
        np.testing.assert_array_equal(net.forward_dev(torch.from_numpy(x).cuda()).cpu().numpy(), got)
        if which == 0:
            for route in SB_ROUTES:
                for key, val in route.items():
                    monkeypatch.setenv(key, val)
                _within_bound(net.forward(x), ref)
                _within_bound(net.forward(x[2:3]), ref[2:3])
                for key in route:
                    monkeypatch.delenv(key)
            v = net.view()
            np.testing.assert_array_equal(v.forward(x), got)
            v.close()
    finally:
        net.close()
