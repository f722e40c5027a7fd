"""The landmark predictor (featurizer/shape_predictor.py, csrc/shape_predictor.hip): dlib's shape_predictor restated -- parity with dlib
itself is UNPINNED (no dlib, no model file here).  The stream reader against its writer, the numpy model tests/shape_model.py on cases
worked out by hand, the closed-form similarity against the SVD form of face_chip.py, and, on the GPU, the kernel's bytes against the
model's over the shapes of the issue, the run modes, the Python surface and the featurizer's ``landmark_backend = "hip"``."""
import ctypes

import numpy as np
import pytest

import shape_model as M
from columbiaimagesearch_amd.featurizer import face_chip
from columbiaimagesearch_amd.featurizer import shape_predictor as SP
from columbiaimagesearch_amd.featurizer.synthetic import shape_predictor_model

gpu = pytest.mark.gpu

#         P   K   T   depth F    n   (the last row: the dimensions of dlib's 68-point model, once)
CASES = [(1, 1, 1, 1, 2, 1),
         (5, 3, 64, 4, 800, 3),
         (68, 3, 65, 4, 500, 65),
         (68, 2, 130, 5, 1000, 3),
         (128, 2, 63, 3, 64, 3),
         (68, 15, 500, 4, 500, 2)]
CASE_IDS = ["P%d-K%d-T%d-d%d-F%d-n%d" % c for c in CASES]


def image(which):
    """97 x 131 or 240 x 320 RGB: noise with smooth gradients mixed in"""
    nr, nc = ((97, 131), (240, 320))[which]
    rs = np.random.RandomState(40 + which)
    yy, xx = np.mgrid[0:nr, 0:nc]
    smooth = np.stack([(xx * 1.7 + yy * 0.6) % 256, 128 + 100 * np.sin(yy / 17.0) * np.cos(xx / 23.0), (xx * yy / 37.0) % 256], axis=-1)
    return (0.5 * smooth + 0.5 * rs.randint(0, 256, size=(nr, nc, 3))).astype(np.uint8)


def rect_kinds(nr, nc):
    """(left, top, right, bottom): inside, across each border, wholly outside, right == left, right < left, bottom < top"""
    return [(nc // 4, nr // 4, nc // 4 + nc // 2, nr // 4 + nr // 2),
            (-nc // 3, nr // 5, nc // 3, nr // 5 + nr // 2),
            (nc // 5, -nr // 3, nc // 5 + nc // 2, nr // 3),
            (nc - nc // 3, nr // 6, nc + nc // 3, nr // 6 + nr // 2),
            (nc // 6, nr - nr // 3, nc // 6 + nc // 2, nr + nr // 3),
            (nc + 60, nr + 50, nc + 160, nr + 170),
            (nc // 2, nr // 4, nc // 2, nr // 4 + nr // 2),
            (nc // 2 + 30, nr // 4, nc // 2 - 20, nr // 4 + nr // 2),
            (nc // 4, nr // 2 + 20, nc // 4 + nc // 2, nr // 2 - 20)]


_cases = {}


def case(i):
    """(model, image, rects int32 [n, 4], the numpy model's parts and shapes): made once, shared, never written to"""
    if i not in _cases:
        P, K, T, depth, F, n = CASES[i]
        model = shape_predictor_model(seed=100 + i, P=P, K=K, T=T, depth=depth, F=F)
        img = image(i % 2)
        kinds = rect_kinds(*img.shape[:2])
        rs = np.random.RandomState(7 + i)
        rects = [kinds[(2 * i + j) % len(kinds)] for j in range(n)]
        # past the nine kinds: the same kinds moved about by a few pixels
        rects = np.array([r if j < len(kinds) else tuple(int(v) for v in np.array(r) + rs.randint(-9, 10, size=4)) for j, r in enumerate(rects)],
                         dtype=np.int32).reshape(n, 4)
        for a in (img, rects):
            a.setflags(write=False)
        _cases[i] = (model, img, rects) + M.predict(model, img, rects)
    return _cases[i]


# ---- the stream --------------------------------------------------------------------------------------------------------------------------
def assert_same_model(a, b):
    for name, x in a.arrays().items():
        y = getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and (x.view(np.uint8) == y.view(np.uint8)).all(), name


@pytest.mark.parametrize("dims", [dict(P=5, K=2, T=3, depth=2, F=9), dict(P=68, K=2, T=5, depth=4, F=40)], ids=["P5", "P68"])
def test_stream_round_trip_both_header_signs_and_npz(dims, tmp_path):
    m = shape_predictor_model(seed=3, **dims)
    m.split_thresh[0, 0, 0] = np.inf          # the specials of the float serialiser
    m.leaves[0, 0, 0, :3] = (-np.inf, 0.0, np.float32(1e-42))
    new, old = SP.write_sp_dat(m), SP.write_sp_dat(m, negate_dims=False)
    assert new != old and len(new) == len(old)
    assert_same_model(m, SP.sp_from_dat(new))
    assert_same_model(m, SP.sp_from_dat(old))
    path = str(tmp_path / "sp.dat")
    SP.write_sp_dat(m, path)
    assert_same_model(m, SP.load_shape_predictor(path))
    SP.save_npz(m, str(tmp_path / "sp.npz"))
    assert_same_model(m, SP.sp_from_npz(str(tmp_path / "sp.npz")))
    assert_same_model(m, SP.load_shape_predictor(str(tmp_path / "sp.npz")))


def test_bulk_float_encoding_is_the_item_encoding():
    from columbiaimagesearch_amd.featurizer.dlib_dat import _Out
    rs = np.random.RandomState(0)
    x = np.concatenate([rs.randn(200) * 10.0 ** rs.randint(-30, 30, size=200), [0.0, -0.0, 1.0, -1.0, 0.5, 256.0, 65536.0, 3.0e38, 1e-45, -1e-40,
                                                                                np.inf, -np.inf, np.nan]]).astype(np.float32)
    data, ends = SP._encode_reals(x)
    o = _Out()
    want_ends = []
    for v in x:
        o.real(v, 24)
        want_ends.append(sum(len(p) for p in o.parts))
    assert data == b"".join(o.parts) and list(ends) == want_ends


def test_stream_errors_name_the_offset_or_the_offender():
    m = shape_predictor_model(seed=4, P=5, K=2, T=3, depth=2, F=9)
    data = SP.write_sp_dat(m)
    for cut in (1, len(data) // 3, len(data) // 2, len(data) - 1):
        with pytest.raises(ValueError, match=r"byte \d+"):
            SP.sp_from_dat(data[:cut])
    with pytest.raises(ValueError, match=r"byte \d+.*behind"):
        SP.sp_from_dat(data + b"\x01\x00")
    assert data[:2] == b"\x01\x01"
    with pytest.raises(ValueError, match=r"byte \d+: shape_predictor: version 2"):
        SP.sp_from_dat(b"\x01\x02" + data[2:])
    assert data[2:6] == b"\x81\x0a\x81\x01"     # the header of initial_shape, -10 x -1: the first float starts at byte 6
    with pytest.raises(ValueError, match=r"byte 6: .*control byte"):
        SP.sp_from_dat(data[:6] + b"\x7f" + data[7:])
    bad = shape_predictor_model(seed=4, P=5, K=2, T=3, depth=2, F=9)
    bad.split_idx[1, 2, 0, 1] = 9
    with pytest.raises(ValueError, match=r"split_idx\[1\]\[2\]\[0\]\[1\] = 9 is not a feature \(F = 9\)"):
        SP.sp_from_dat(SP.write_sp_dat(bad))
    bad = shape_predictor_model(seed=4, P=5, K=2, T=3, depth=2, F=9)
    bad.anchor_idx[1, 4] = 5
    with pytest.raises(ValueError, match=r"byte \d+: anchor_idx\[1\]\[4\] = 5 is not a landmark"):
        SP.sp_from_dat(SP.write_sp_dat(bad))


def test_loader_checks_name_the_offender():
    g = shape_predictor_model(seed=5, P=3, K=2, T=2, depth=2, F=4).arrays()

    def build(**kw):
        return SP.ShapePredictorModel(**dict(g, **kw))

    with pytest.raises(ValueError, match="2 splits per tree is not a power of two minus one"):
        build(split_idx=g["split_idx"][:, :, :2], split_thresh=g["split_thresh"][:, :, :2], leaves=g["leaves"][:, :, :3])
    with pytest.raises(ValueError, match="leaves has shape"):
        build(leaves=g["leaves"][:, :1])
    with pytest.raises(ValueError, match="deltas has shape"):
        build(deltas=g["deltas"][:, :3])
    a = g["anchor_idx"].copy()
    a[1, 2] = 3
    with pytest.raises(ValueError, match=r"anchor_idx\[1\]\[2\] = 3 is not a landmark \(P = 3\)"):
        build(anchor_idx=a)
    s = g["split_idx"].copy()
    s[0, 1, 2, 0] = 4
    with pytest.raises(ValueError, match=r"split_idx\[0\]\[1\]\[2\]\[0\] = 4 is not a feature \(F = 4\)"):
        build(split_idx=s)
    for what, dims in (("2P = 258", dict(P=129, K=1, T=1, depth=1, F=2)), ("F = 4097", dict(P=2, K=1, T=1, depth=1, F=4097)),
                       ("T = 4097", dict(P=1, K=1, T=4097, depth=1, F=2)), ("depth = 9", dict(P=1, K=1, T=1, depth=9, F=2))):
        with pytest.raises(ValueError, match=what):
            shape_predictor_model(seed=0, **dims)


# ---- the model on cases worked out by hand -------------------------------------------------------------------------------------------------
def test_hand_built_model_picks_the_leaf_worked_out_here():
    """P = 2, K = 1, T = 1, depth = 1, F = 2 on a 10 x 10 image whose columns 0..4 are (30, 60, 90) -- grey 180 / 3 = 60 -- and whose
    columns 5..9 are (200, 100, 60) -- grey 120.  Rectangle (0, 0, 9, 9): width and height 9.  The current shape is the initial one, so
    the similarity is the identity (a = sd / ff with sd and ff the same sums, b = a sum of exact zeros).  Feature 0 sits on landmark 0,
    (0.25, 0.5): x = 2.25 -> 2, y = 4.5 -> floor(5.0) = 5, a left pixel, 60.  Feature 1 on landmark 1, (0.75, 0.5): x = 6.75 -> 7, y = 5,
    a right pixel, 120.  The one split asks pix[0] - pix[1] = -60 > 0: no, so i = 2 and the leaf is 2 - 1 = 1.
    cur = (0.25, 0.5, 0.75, 0.5) + (0, -0.25, 0.125, 0) = (0.25, 0.25, 0.875, 0.5): parts (2.25 -> 2, 2.25 -> 2), (7.875 -> 8, 4.5 -> 5).
    Colours swapped: 60 > 0, i = 1, leaf 0: cur + (0.125, 0, 0, 0.25) = (0.375, 0.5, 0.75, 0.75): parts (3.375 -> 3, 5), (6.75 -> 7, 7)."""
    model = SP.ShapePredictorModel(initial_shape=[0.25, 0.5, 0.75, 0.5], split_idx=[[[[0, 1]]]], split_thresh=[[[0.0]]],
                                   leaves=[[[[0.125, 0, 0, 0.25], [0, -0.25, 0.125, 0]]]], anchor_idx=[[0, 1]], deltas=[[[0, 0], [0, 0]]])
    assert (model.P, model.K, model.T, model.depth, model.F) == (2, 1, 1, 1, 2)
    img = np.zeros((10, 10, 3), np.uint8)
    img[:, :5], img[:, 5:] = (30, 60, 90), (200, 100, 60)
    trace = []
    parts, shape = M.predict_one(model, img, (0, 0, 9, 9), trace=trace)
    assert trace[0].tolist() == [[2, 5], [7, 5]]
    assert shape.tolist() == [0.25, 0.25, 0.875, 0.5] and parts.tolist() == [[2, 2], [8, 5]]
    parts, shape = M.predict_one(model, img[:, ::-1], (0, 0, 9, 9))
    assert shape.tolist() == [0.375, 0.5, 0.75, 0.75] and parts.tolist() == [[3, 5], [7, 7]]
    # a rectangle off the image: both pixels read 0, 0 > 0 is false, leaf 1
    assert M.predict_one(model, img, (20, 20, 29, 29))[1].tolist() == [0.25, 0.25, 0.875, 0.5]


def svd_similarity(f, t):
    return np.eye(2) if len(f) == 1 else face_chip.find_similarity_transform(f, t)[0]


def test_closed_form_similarity_is_the_svd_form():
    rs = np.random.RandomState(11)
    for it in range(1000):
        n = int(rs.randint(2, 129))
        f = rs.rand(n, 2).astype(np.float32)
        angle = rs.uniform(-3, 3)
        c, s = np.cos(angle), np.sin(angle)
        t = (f @ (rs.uniform(0.3, 3.0) * np.array([[c, -s], [s, c]])).T + rs.randn(2) + 0.05 * rs.randn(n, 2)).astype(np.float32)
        m, want = M.similarity_closed_form(f, t), svd_similarity(f, t)
        assert np.abs(m - want).max() <= 1e-10 * np.linalg.norm(want), (it, m, want)
    # a mirrored shape: det(cov) < 0, Umeyama's sign matrix is diag(1, -1) and the result is still a rotation
    f = rs.rand(40, 2)
    t = f * np.array([-1.0, 1.0]) + 0.05 * rs.randn(40, 2)
    cov = (t - t.mean(0)).T @ (f - f.mean(0))
    assert np.linalg.det(cov) < 0
    m, want = M.similarity_closed_form(f, t), svd_similarity(f, t)
    assert np.linalg.det(want) > 0 and np.abs(m - want).max() <= 1e-10 * np.linalg.norm(want)
    # all points equal: sum |f'|^2 = 0, scale 1, the identity
    f = np.full((7, 2), 0.375)
    m, want = M.similarity_closed_form(f, rs.rand(7, 2)), svd_similarity(f, rs.rand(7, 2))
    assert (m == np.eye(2)).all() and (want == np.eye(2)).all()
    assert (M.similarity_closed_form(f[:1], f[:1] + 1) == np.eye(2)).all()


@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_gpu_case_inputs_read_the_same_pixels_under_both_forms(i):
    """A condition on the inputs of the GPU cases below, not on the kernel: the closed form and the SVD form of the similarity send
    every feature of every level to the same pixel (and so give the same shapes), and the rectangles are of the kinds they claim."""
    model, img, rects, parts, shapes = case(i)
    nr, nc = img.shape[:2]
    for j, r in enumerate(rects):
        a, b = [], []
        pa, sa = M.predict_one(model, img, r, trace=a)
        pb, sb = M.predict_one(model, img, r, similarity=svd_similarity, trace=b)
        assert sum(int((x != y).any(axis=1).sum()) for x, y in zip(a, b)) == 0
        assert (pa == parts[j]).all() and (sa.view(np.uint32) == shapes[j].view(np.uint32)).all() and (pb == pa).all()
        if tuple(r) == rect_kinds(nr, nc)[5]:
            assert all(((x[:, 0] >= nc) & (x[:, 1] >= nr)).all() for x in a)   # wholly outside: every pixel reads 0
    if CASES[i][5] == 65:
        kinds = rect_kinds(nr, nc)
        assert all(any(tuple(r) == k for r in rects) for k in kinds)
        assert any(r[2] == r[0] for r in rects) and any(r[2] < r[0] for r in rects)


def test_all_right_traversal_pins_the_order_of_the_sum():
    """Every threshold +inf: every walk goes right to the last leaf, so cur is the initial shape plus the float32 RUNNING sum of the last
    leaves in tree order -- and that is not the pairwise float32 sum nor the float64 sum at T = 500."""
    model = shape_predictor_model(seed=21, P=68, K=1, T=500, depth=4, F=500)
    model.split_thresh[:] = np.inf
    shape = M.predict_one(model, image(0), (20, 10, 90, 80))[1]
    last = model.leaves[0, :, -1, :]
    run = model.initial_shape.copy()
    for t in range(500):
        run = (run + last[t]).astype(np.float32)
    assert (shape.view(np.uint32) == run.view(np.uint32)).all()
    pairwise = model.initial_shape + np.ascontiguousarray(last.T).sum(axis=1, dtype=np.float32)   # (numpy sums a contiguous axis pairwise)
    wide = (model.initial_shape.astype(np.float64) + last.astype(np.float64).sum(axis=0)).astype(np.float32)
    assert (shape != pairwise).any() and (shape != wide).any()


def test_unknown_landmark_backend_is_a_value_error():
    from columbiaimagesearch_amd.featurizer import DLibHIPFeaturizer
    with pytest.raises(ValueError, match="landmark_backend"):
        DLibHIPFeaturizer({"DLIBFEAT_pred_path": "unused", "DLIBFEAT_rec_path": "unused.npz", "DLIBFEAT_landmark_backend": "opencv"})


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------
def create(model):
    from columbiaimagesearch_amd import _lib
    out = ctypes.c_void_p()
    _lib.check(_lib.lib().cis_shapepred_create(ctypes.byref(out), model.P, model.K, model.T, model.depth, model.F, _lib.ptr(model.initial_shape),
                                               _lib.ptr(model.split_idx), _lib.ptr(model.split_thresh), _lib.ptr(model.leaves),
                                               _lib.ptr(model.anchor_idx), _lib.ptr(model.deltas)))
    return out.value


def run(h, model, img, rects, want_shape=True, stream=None):
    """cis_shapepred_run_dev through ctypes -> (parts int32 [n, P, 2], shapes float32 [n, 2P] or None), outputs pre-filled with a mark"""
    import torch
    from columbiaimagesearch_amd import _lib
    n = len(rects)
    timg, trects = torch.as_tensor(np.array(img)).cuda(), torch.as_tensor(np.array(rects, dtype=np.int32).reshape(n, 4)).cuda()
    parts = torch.full((n, model.P, 2), -77, dtype=torch.int32, device="cuda")
    shape = torch.full((n, 2 * model.P), -77.0, dtype=torch.float32, device="cuda") if want_shape else None
    torch.cuda.synchronize()
    st = torch.cuda.current_stream() if stream is None else stream
    _lib.check(_lib.lib().cis_shapepred_run_dev(h, timg.data_ptr(), img.shape[0], img.shape[1], trects.data_ptr(), n, parts.data_ptr(),
                                                shape.data_ptr() if want_shape else None, st.cuda_stream))
    st.synchronize()
    return parts.cpu().numpy(), (shape.cpu().numpy() if want_shape else None)


@gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_kernel_is_bit_equal_to_the_numpy_model(i):
    from columbiaimagesearch_amd import _lib
    model, img, rects, want_parts, want_shapes = case(i)
    h = create(model)
    try:
        parts, shapes = run(h, model, img, rects)
    finally:
        _lib.lib().cis_shapepred_destroy(h)
    bad = np.argwhere(shapes.view(np.uint32) != want_shapes.view(np.uint32))
    assert len(bad) == 0, (len(bad), bad[:5], shapes[tuple(bad[0])], want_shapes[tuple(bad[0])])
    assert (parts == want_parts).all(), np.argwhere(parts != want_parts)[:5]


@gpu
def test_run_modes_and_create_errors():
    import torch
    from columbiaimagesearch_amd import _lib
    L = _lib.lib()
    model, img, rects, want_parts, want_shapes = case(1)
    h = create(model)
    try:
        parts, shapes = run(h, model, img, rects)
        again = run(h, model, img, rects)
        assert parts.tobytes() == again[0].tobytes() and shapes.tobytes() == again[1].tobytes()      # two runs, equal bytes
        no_shape = run(h, model, img, rects, want_shape=False)                                      # d_shape = NULL
        assert no_shape[1] is None and (no_shape[0] == want_parts).all()
        other = run(h, model, img, rects, stream=torch.cuda.Stream())                               # a second stream
        assert (other[0] == want_parts).all() and (other[1].view(np.uint32) == want_shapes.view(np.uint32)).all()
        assert L.cis_shapepred_run_dev(h, None, 0, 0, None, 0, None, None, None) == _lib.CIS_OK     # n = 0: returns at once
        empty = run(h, model, img, np.zeros((0, 4), np.int32))
        assert empty[0].shape == (0, model.P, 2)
    finally:
        L.cis_shapepred_destroy(h)
    # create: every failed check is CIS_EINVAL with a message, no handle comes back and nothing runs
    small = shape_predictor_model(seed=1, P=2, K=1, T=1, depth=1, F=2)
    big = np.zeros(1 << 16, np.float32)
    bigi = np.zeros(1 << 16, np.int32)
    far = small.split_idx.copy()
    far[0, 0, 0, 1] = 2
    for words, args in ((("2P = 258",), (129, 1, 1, 1, 2, big, bigi, big, big, bigi, big)),
                        (("F = 4097",), (2, 1, 1, 1, 4097, big, bigi, big, big, bigi, big)),
                        (("split_idx[0][0][0][1] = 2", "F = 2"), (2, 1, 1, 1, 2, small.initial_shape, far, small.split_thresh, small.leaves,
                                                                  small.anchor_idx, small.deltas))):
        out = ctypes.c_void_p()
        rc = L.cis_shapepred_create(ctypes.byref(out), *(list(args[:5]) + [_lib.ptr(a) for a in args[5:]]))
        assert rc == _lib.CIS_EINVAL and out.value is None
        assert all(w in _lib.last_error() for w in words), _lib.last_error()
        with pytest.raises(ValueError):
            _lib.check(rc)


@gpu
def test_python_surface_predict_equals_predict_dev():
    import torch
    model, img, rects, want_parts, _ = case(3)
    sp = SP.ShapePredictorHIP(model)
    dev = sp.predict_dev(torch.as_tensor(np.array(img)).cuda(), torch.as_tensor(np.array(rects)).cuda())
    assert dev.is_cuda and dev.dtype == torch.int32 and tuple(dev.shape) == (len(rects), model.P, 2)
    host = sp.predict(img, rects)
    assert host.dtype == np.int64 and (host == dev.cpu().numpy()).all() and (host == want_parts).all()
    shape = torch.empty((len(rects), 2 * model.P), dtype=torch.float32, device="cuda")
    sp.predict_dev(torch.as_tensor(np.array(img)).cuda(), torch.as_tensor(np.array(rects)).cuda(), shape_out=shape)
    assert (shape.cpu().numpy().view(np.uint32) == case(3)[4].view(np.uint32)).all()
    assert sp.predict(img, np.zeros((0, 4))).shape == (0, model.P, 2)
    with pytest.raises(ValueError):
        sp.predict_dev(torch.as_tensor(np.array(img)), torch.as_tensor(np.array(rects)).cuda())
    sp.close()
    sp.close()
    with pytest.raises(ValueError):
        sp.predict(img, rects)


BOXES = [{"left": 70, "top": 30, "right": 230, "bottom": 200, "score": 1.5}, {"left": 20, "top": 60, "right": 150, "bottom": 190, "score": 0.75},
         {"left": 150, "top": 20, "right": 300, "bottom": 170, "score": 0.25}]


@pytest.fixture(scope="module")
def face_setup(tmp_path_factory):
    from columbiaimagesearch_amd.featurizer.synthetic import dlib_weights
    d = tmp_path_factory.mktemp("faces")
    model = shape_predictor_model(seed=31, P=68, K=3, T=65, depth=4, F=500)
    SP.save_npz(model, str(d / "sp.npz"))
    np.savez(str(d / "net.npz"), **dlib_weights(0))
    conf = {"DLIBFEAT_pred_path": str(d / "sp.npz"), "DLIBFEAT_rec_path": str(d / "net.npz"), "DLIBFEAT_landmark_backend": "hip"}
    return model, image(1), conf


def close(a, b):
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-5 * max(1.0, np.abs(b).max()))


@gpu
def test_featurizer_with_the_hip_backend_end_to_end(face_setup):
    from columbiaimagesearch_amd.featurizer import DLibHIPFeaturizer
    model, img, conf = face_setup
    fz = DLibHIPFeaturizer(conf)
    assert fz._sp_hip is None                                   # loaded on first use, not in the constructor
    rects = [[b["left"], b["top"], b["right"], b["bottom"]] for b in BOXES]
    landmarks = M.predict(model, img, rects)[0].astype(np.float64)
    one = fz.featurize(img, BOXES[0])
    assert one.shape == (128,) and one.dtype == np.float64 and fz._sp_hip is not None
    close(one, fz.featurize_landmarks(img, [landmarks[0]])[0])
    close(fz._chip(img, BOXES[1]), fz._chips(img, BOXES[1:2])[0])
    dets = fz.featurize_dets(img, BOXES)
    assert dets.shape == (3, 128)
    for b, feat in zip(BOXES, dets):
        close(feat, fz.featurize(img, b))
    # the precedence of the hooks stays: landmarks=, then landmark_fn, and chip_fn over both backends
    close(fz.featurize(img, BOXES[0], landmarks=landmarks[1]), fz.featurize_landmarks(img, [landmarks[1]])[0])
    fz.landmark_fn = lambda im, bb: landmarks[2]
    close(fz.featurize(img, BOXES[0]), fz.featurize_landmarks(img, [landmarks[2]])[0])
    fz.chip_fn = lambda im, bb: np.full((150, 150, 3), 9.0, np.float32)
    close(fz.featurize(img, BOXES[0]), fz.featurize_chips(np.full((1, 150, 150, 3), 9.0, np.float32))[0])
    close(fz.featurize_dets(img, BOXES[:2]), fz.featurize_chips(np.full((2, 150, 150, 3), 9.0, np.float32)))


@gpu
def test_extractor_detector_branch_same_rows_with_and_without_chips(face_setup):
    import io
    from PIL import Image
    from columbiaimagesearch_amd.extractor.generic_extractor import GenericExtractor
    model, img, conf = face_setup

    class FakeDetector(object):
        def detect_from_buffer_noinfos(self, img_buffer, up_sample=1):
            im = np.array(Image.open(io.BytesIO(img_buffer)).convert("RGB"))
            return im, (BOXES if im.shape[0] == 240 else BOXES[:1] if im.shape[0] == 200 else [])

    class PerDetection(object):
        """the featurizer as the extractor saw it before `_chips`: one `_chip` per detection"""

        def __init__(self, fz):
            self._chip, self.featurize_chips, self.featurize = fz._chip, fz.featurize_chips, fz.featurize

    bufs = []
    for im in (img, img[:200], img[:100]):
        b = io.BytesIO()
        Image.fromarray(im).save(b, format="PNG")
        bufs.append(b.getvalue())
    ex = GenericExtractor("dlib", "dlib", "face", "ext", "DLIBFEAT_", conf, detector=FakeDetector())
    assert hasattr(ex.featurizer, "_chips")
    rows = ex.process_batch(bufs)
    base = "ext:dlib_feat_dlib_face"
    assert sorted(rows[0]) == sorted([base + "_processed", base + "_70_30_230_200_1.5", base + "_20_60_150_190_0.75", base + "_150_20_300_170_0.25"])
    assert len(rows[1]) == 2 and rows[2] == {base + "_processed": "0"}
    ex.featurizer = PerDetection(ex.featurizer)
    assert not hasattr(ex.featurizer, "_chips")
    assert ex.process_batch(bufs) == rows


@gpu
def test_dlib_backend_without_dlib_still_raises_import_error(face_setup, monkeypatch):
    import sys
    from columbiaimagesearch_amd.featurizer import DLibHIPFeaturizer
    monkeypatch.setitem(sys.modules, "dlib", None)   # `import dlib` raises ImportError, whether or not dlib is installed
    model, img, conf = face_setup
    for c in (dict(conf, DLIBFEAT_landmark_backend="dlib"), {k: v for k, v in conf.items() if k != "DLIBFEAT_landmark_backend"}):
        fz = DLibHIPFeaturizer(c)
        assert fz.landmark_backend == "dlib"
        with pytest.raises(ImportError, match="dlib is needed for the landmark predictor"):
            fz.featurize(img, BOXES[0])
        with pytest.raises(ImportError):
            fz.featurize_dets(img, BOXES)
    with pytest.raises(ValueError, match="landmark_backend"):
        DLibHIPFeaturizer(dict(conf, DLIBFEAT_landmark_backend="cpu"))
