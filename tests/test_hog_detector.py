"""The HOG face detector on the GPU (detector/hog_detector.py, csrc/hog_detector.hip): the kernels' bytes against the numpy model
tests/fhog_model.py -- resize, FHOG, scores, the whole detector on a planted image and at its edges, the chain into the landmark
predictor, the Python surface and the extractor's ``detector_backend = "hip"``.  Parity with dlib itself is UNPINNED."""
import ctypes
import io

import numpy as np
import pytest

import fhog_model as M
from columbiaimagesearch_amd.detector import hog_detector as HD
from columbiaimagesearch_amd.featurizer.synthetic import fhog_detector_model

gpu = pytest.mark.gpu
F32 = np.float32
GUARD = 64          # guard words behind every output buffer
MARK = -77


def texture(nr, nc, seed, noise=0.5):
    """noise plus smooth gradients, RGB"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:nr, 0:nc]
    smooth = np.stack([(xx * 1.7 + yy * 0.6) % 256, 128 + 100 * np.sin(yy / 17.0) * np.cos(xx / 23.0), (xx * yy / 37.0) % 256], axis=-1)
    return ((1.0 - noise) * smooth + noise * rs.randint(0, 256, size=(nr, nc, 3))).astype(np.uint8)


def template():
    """96 x 96: rings and bars with strong edges in different channels"""
    yy, xx = np.mgrid[0:96, 0:96]
    rad = np.hypot(yy - 47.5, xx - 47.5)
    r = np.where((rad // 16) % 2 == 0, 230, 25)
    g = np.where(((xx + 2 * yy) // 40) % 2 == 0, 200, 40)
    b = np.where((yy // 32) % 2 == 0, 180, 60)
    return np.stack([r, g, b], axis=-1).astype(np.uint8)


# ---- through ctypes ------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a).copy()).cuda()


def gpu_resize(img, onr, onc):
    import torch
    from columbiaimagesearch_amd import _lib
    out = torch.full((onr * onc * 3 + GUARD,), 201, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    _lib.check(_lib.lib().cis_resize_bilinear_rgb_dev(dev(img).data_ptr(), img.shape[0], img.shape[1], out.data_ptr(), onr, onc, st.cuda_stream))
    st.synchronize()
    o = out.cpu().numpy()
    assert (o[onr * onc * 3:] == 201).all()
    return o[:onr * onc * 3].reshape(onr, onc, 3)


def gpu_fhog(img, pad_rows, pad_cols):
    """-> (hist [cr, cc, 18], feat [31, Hp, Wp]) with the guard words checked; buffers are sized from the model's shapes"""
    import torch
    from columbiaimagesearch_amd import _lib
    cr, cc = M.cell_counts(*img.shape[:2])
    want = M.fhog(img, pad_rows, pad_cols)
    nh, nf = cr * cc * 18, want.size
    hist = torch.full((nh + GUARD,), float(MARK), dtype=torch.float32, device="cuda")
    feat = torch.full((nf + GUARD,), float(MARK), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    _lib.check(_lib.lib().cis_fhog_extract_dev(dev(img).data_ptr(), img.shape[0], img.shape[1], 8, pad_rows, pad_cols, hist.data_ptr(),
                                               feat.data_ptr(), st.cuda_stream))
    st.synchronize()
    h, f = hist.cpu().numpy(), feat.cpu().numpy()
    assert (h[nh:] == MARK).all() and (f[nf:] == MARK).all()
    return h[:nh].reshape(cr, cc, 18), f[:nf].reshape(want.shape)


def gpu_scores(feat, w):
    import torch
    from columbiaimagesearch_amd import _lib
    want_shape = (w.shape[0], max(feat.shape[1] - w.shape[2] + 1, 0), max(feat.shape[2] - w.shape[3] + 1, 0))
    n = int(np.prod(want_shape))
    out = torch.full((n + GUARD,), float(MARK), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    w = np.ascontiguousarray(w, dtype=F32)
    _lib.check(_lib.lib().cis_fhog_scores_dev(dev(feat).data_ptr(), feat.shape[1], feat.shape[2], w.shape[0], w.shape[2], w.shape[3], _lib.ptr(w),
                                              out.data_ptr(), st.cuda_stream))
    st.synchronize()
    o = out.cpu().numpy()
    assert (o[n:] == MARK).all()
    return o[:n].reshape(want_shape), o


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def first_diff(a, b):
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    return (len(bad), bad[:3].tolist(), [float(a[tuple(i)]) for i in bad[:3]], [float(b[tuple(i)]) for i in bad[:3]])


# ---- resize --------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape, out", [((97, 131), (80, 109)), ((3, 3), (2, 2)), ((2, 2), (1, 1)), ((97, 131), M.up_size(97, 131)), ((1, 5), (3, 9))],
                         ids=["97x131-80x109", "3x3-2x2", "2x2-1x1", "97x131-up", "1x5-3x9"])
def test_resize_equals_the_model(shape, out):
    img = texture(shape[0], shape[1], 1)
    got, want = gpu_resize(img, *out), M.resize_bilinear(img, *out)
    assert (got == want).all(), np.argwhere(got != want)[:5]


# ---- FHOG ----------------------------------------------------------------------------------------------------------------------------------
def fhog_image(name):
    if name == "grey64x200":
        return np.repeat(texture(64, 200, 2)[:, :, :1], 3, axis=2)          # three equal channels: every pixel a channel tie
    if name == "half-constant":
        img = texture(72, 120, 3)
        img[:, 60:] = 117                                                     # normalisers at eps on the right
        return img
    nr, nc = (int(v) for v in name.split("x"))
    return texture(nr, nc, nr + nc)


@gpu
@pytest.mark.parametrize("name", ["24x24", "23x40", "19x40", "97x131", "100x100", "grey64x200", "half-constant"])
@pytest.mark.parametrize("pad", [(1, 1), (10, 10), (6, 9)], ids=["pad1", "pad10", "pad6x9"])
def test_fhog_is_bit_equal_to_the_model(name, pad):
    """24 x 24: one output cell; 23 x 40: (int)(23 / 8 + 0.5) = 3 cells, one output row whose visible area the image clips; 19 x 40: 2 cells,
    no output (returns, writes nothing); 100 x 100: 13 cells, visible area clipped; 97 x 131: more than one workgroup tile each way."""
    img = fhog_image(name)
    want = M.fhog(img, *pad)
    hist, feat = gpu_fhog(img, *pad)
    if want.size == 0:
        assert (hist == MARK).all()                                           # nothing was launched
        return
    want_hist = M.cell_histograms(img)
    assert same_bits(hist, want_hist), first_diff(hist, want_hist)
    assert same_bits(feat, want), first_diff(feat, want)
    if name == "half-constant":                                               # 13 output columns; the last three see constant pixels only
        c0 = (pad[1] - 1) // 2
        assert (want[:, :, c0 + 10:] == 0).all() and (want[:, :, c0:c0 + 5] != 0).any()


# ---- scores --------------------------------------------------------------------------------------------------------------------------------
SCORE_CASES = {"F1-10x10": (1, 10, 10, (97, 131)), "F5-10x10": (5, 10, 10, (97, 131)), "F2-6x9": (2, 6, 9, (100, 100)),
               "level-smaller-than-filter": (5, 10, 10, (40, 56))}
_score_cache = {}


def score_case(name):
    """(feat, w, float32 model scores, float64 scores, sum |w f|): made once, shared, never written to"""
    if name not in _score_cache:
        F, fr, fc, shape = SCORE_CASES[name]
        feat = M.fhog(texture(shape[0], shape[1], 9), fr, fc)
        w = fhog_detector_model(seed=len(name), F=F, fr=fr, fc=fc).w
        _score_cache[name] = (feat, w, M.scores(feat, w), M.scores(feat, w, np.float64), M.abs_scores(feat, w))
        for a in _score_cache[name]:
            a.setflags(write=False)
    return _score_cache[name]


@gpu
@pytest.mark.parametrize("name", sorted(SCORE_CASES))
def test_scores_are_bit_equal_to_the_ordered_float32_sum_and_near_the_float64_sum(name):
    """The bound on the distance to the float64 sum is derived, not measured: every term w f passes through its product's rounding and at
    most K - 1 roundings of additions (the first addition, to an exact zero, is exact), K = 31 fr fc, each with a relative error of at most
    u = 2^-24: |s32 - s| <= K u sum |w f| to first order in u (the exact factor, 1 / (1 - K u), is 2e-4 larger; the float64 sum's own
    error is 2^-29 of this bound).  The largest ratio measured on the MI355X is 0.0009: the stated order is a sane sum."""
    feat, w, want, wide, mass = score_case(name)
    got, _ = gpu_scores(feat, w)
    assert got.shape[1] >= 1 and same_bits(got, want), first_diff(got, want)
    K = 31 * w.shape[2] * w.shape[3]
    err = np.abs(got.astype(np.float64) - wide)
    bound = K * 2.0 ** -24 * mass
    print("scores %s: largest |s32 - s64| / bound = %.4f" % (name, (err / bound).max()))
    assert (err <= bound).all()
    if name == "level-smaller-than-filter":
        assert feat.shape[1] - (w.shape[2] - 1) < w.shape[2]                  # 3 output rows under a 10-row filter: border windows only


@gpu
def test_filter_that_fits_nowhere_writes_nothing():
    feat = np.zeros((31, 5, 12), F32)
    _, raw = gpu_scores(feat, np.ones((2, 31, 6, 9), F32))
    assert (raw == MARK).all()


# ---- the whole detector --------------------------------------------------------------------------------------------------------------------
def planted_image():
    """230 x 310 noise plus gradients; the template at scale 1 at (24, 32) (on the cell grid), and at (6/5)^2 = 1.44, the scale of the second
    pyramid level for N = 6, at (80, 160) -- (56, 112) on level 2, near its cell grid"""
    img = texture(230, 310, 77, noise=0.06)
    t = template()
    img[24:24 + 96, 32:32 + 96] = t
    img[80:80 + 138, 160:160 + 138] = M.resize_bilinear(t, 138, 138)
    return img


def gap_threshold(sal, f, lo=16, hi=60):
    """The middle of the largest gap between consecutive sorted scores of filter f, among ranks lo..hi: nothing sits on the boundary
    (from rank 16 on: the weaker paste's peak on level 2 is the model's 15th score at up_sample 0, N = 6)"""
    s = np.sort(np.concatenate([lv[f].ravel() for lv in sal]).astype(np.float64))[::-1][:hi + 1]
    i = lo - 1 + int(np.argmax(s[lo - 1:-1] - s[lo:]))
    return F32((s[i] + s[i + 1]) / 2)


_planted = {}


def planted(up, n):
    """(model, image, level scores, model's answer at adjust 0, adjust, model's answer at adjust): made once per (up_sample, pyramid_n)"""
    if (up, n) not in _planted:
        img = planted_image()
        f = M.fhog(template())                                                # 12 cells - 2 = 10 x 10
        w = np.stack([f - f.mean(), (f - f.mean())[:, :, ::-1]])              # the template, and its mirror image as a second filter
        det = HD.FHOGDetectorModel(w, np.zeros(2, F32), pyramid_n=n)
        sal = M.level_scores(img, det, up)
        det = HD.FHOGDetectorModel(w, [gap_threshold(sal, 0), gap_threshold(sal, 1)], pyramid_n=n)
        adjust = -0.35 * float(det.thresh[0])
        img.setflags(write=False)
        _planted[(up, n)] = (det, img, sal, M.detect(img, det, up, 0.0, sal), adjust, M.detect(img, det, up, adjust, sal))
    return _planted[(up, n)]


def gpu_detect(h, img, up, adjust=0.0, max_dets=1024, stream=None):
    """cis_fhogdet_run_dev through ctypes -> (rects, scores, filter, count) numpy, the rows past the answer and the guard words checked"""
    import torch
    from columbiaimagesearch_amd import _lib
    L = _lib.lib()
    need = int(L.cis_fhogdet_workspace_bytes(h, img.shape[0], img.shape[1], up))
    assert need > 0
    ws = torch.full((need + 4 * GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    rects = torch.full((max_dets * 4 + GUARD,), MARK, dtype=torch.int32, device="cuda")
    scores = torch.full((max_dets + GUARD,), float(MARK), dtype=torch.float32, device="cuda")
    filt = torch.full((max_dets + GUARD,), MARK, dtype=torch.int32, device="cuda")
    count = torch.full((2 + GUARD,), MARK, dtype=torch.int32, device="cuda")
    timg = dev(img)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream() if stream is None else stream
    _lib.check(L.cis_fhogdet_run_dev(h, timg.data_ptr(), img.shape[0], img.shape[1], up, float(adjust), ws.data_ptr(), need, rects.data_ptr(),
                                     scores.data_ptr(), filt.data_ptr(), max_dets, count.data_ptr(), st.cuda_stream))
    st.synchronize()
    r, s, f, c = rects.cpu().numpy(), scores.cpu().numpy(), filt.cpu().numpy(), count.cpu().numpy()
    n = min(int(c[0]), max_dets)
    assert (r[4 * n:] == MARK).all() and (s[n:] == MARK).all() and (f[n:] == MARK).all() and (c[2:] == MARK).all()
    assert (ws[need:].cpu().numpy() == 0x5a).all()
    return r[:4 * n].reshape(n, 4), s[:n], f[:n], c[:2]


def create(det):
    from columbiaimagesearch_amd import _lib
    out = ctypes.c_void_p()
    _lib.check(_lib.lib().cis_fhogdet_create(ctypes.byref(out), det.F, det.filter_rows, det.filter_cols, det.cell_size, det.padding, det.pyramid_n,
                                             det.max_levels, det.min_layer_w, det.min_layer_h, _lib.ptr(det.w), _lib.ptr(det.thresh),
                                             det.iou_thresh, det.covered_thresh))
    return out.value


def assert_same_answer(got, want):
    rects, scores, filt, count = got
    w_rects, w_scores, w_filt, w_cands = want
    assert tuple(count) == (len(w_rects), w_cands), (tuple(count), len(w_rects), w_cands)
    assert (rects == w_rects).all(), (rects, w_rects)
    assert same_bits(scores, w_scores), (scores, w_scores)
    assert (filt == w_filt).all()


def test_planted_case_fires_where_it_should():
    """A condition on the inputs of the GPU cases below, not on the kernels: at up_sample 0, N = 6 the model finds both pastes, on levels 0
    and 2, suppresses neighbours, and more positions pass with the negative adjustment."""
    det, img, sal, (rects, scores, filt, n_cands), adjust, more = planted(0, 6)
    assert len(rects) >= 2 and n_cands > len(rects)                           # NMS had something to suppress
    centre = lambda r: ((r[0] + r[2]) / 2.0, (r[1] + r[3]) / 2.0)
    for cx, cy, size in ((32 + 48, 24 + 48, 96), (160 + 69, 80 + 69, 138)):
        hit = [r for r in rects if abs(centre(r)[0] - cx) <= 8 and abs(centre(r)[1] - cy) <= 8 and abs((r[2] - r[0] + 1) - size) <= 0.25 * size]
        assert hit, (cx, cy, rects)
    cands = M.candidates(sal, det, 0)
    assert {c[1] for c in cands} >= {0, 2}
    assert more[3] > n_cands and len(more[0]) >= len(rects)
    assert (np.diff(scores) <= 0).all()


@gpu
@pytest.mark.parametrize("up, n", [(0, 6), (1, 6), (0, 3), (1, 3)], ids=["up0-N6", "up1-N6", "up0-N3", "up1-N3"])
def test_planted_detections_equal_the_model(up, n):
    from columbiaimagesearch_amd import _lib
    det, img, sal, want, adjust, want_more = planted(up, n)
    h = create(det)
    try:
        assert_same_answer(gpu_detect(h, img, up), want)
        assert want_more[3] > want[3]
        assert_same_answer(gpu_detect(h, img, up, adjust), want_more)
    finally:
        _lib.lib().cis_fhogdet_destroy(h)


@gpu
def test_detector_edges():
    import torch
    from columbiaimagesearch_amd import _lib
    L = _lib.lib()
    det, img, sal, want, adjust, want_more = planted(0, 6)
    h = create(det)
    try:
        # small images: one level with border windows only (80 x 80: 8 output cells under a 10 x 10 filter), no output cells at all (19 x 19: 2 cells)
        low = HD.FHOGDetectorModel(det.w, [-1e3, 1e3], pyramid_n=6)
        hl = create(low)
        for shape in ((80, 80), (79, 200), (19, 19)):
            small = texture(shape[0], shape[1], 5)
            w = M.detect(small, low, 0)
            assert (w[3] > 0) == (shape != (19, 19))
            assert_same_answer(gpu_detect(hl, small, 0), w)
        L.cis_fhogdet_destroy(hl)
        # no candidate
        none = gpu_detect(h, texture(120, 160, 6), 0, adjust=1e6)
        assert tuple(none[3]) == (0, 0) and len(none[0]) == 0
        # max_dets = 1 with at least two survivors: one row written, the count says how many there are
        assert len(want[0]) >= 2
        r, s, f, c = gpu_detect(h, img, 0, max_dets=1)
        assert tuple(c) == (len(want[0]), want[3]) and (r == want[0][:1]).all() and same_bits(s, want[1][:1])
        # two calls in flight on two streams with two workspaces: the same bytes as alone
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a, b = gpu_detect(h, img, 0, stream=s1), gpu_detect(h, img, 0, adjust, stream=s2)
        assert_same_answer(a, want)
        assert_same_answer(b, want_more)
    finally:
        L.cis_fhogdet_destroy(h)


@gpu
def test_two_calls_enqueued_before_either_finishes():
    import torch
    det, img, sal, want, adjust, want_more = planted(0, 6)
    d = HD.HOGDetectorHIP(det)
    timg = dev(img)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = d.run_dev(timg, 0, 0.0)
    with torch.cuda.stream(s2):
        b = d.run_dev(timg, 0, adjust)
    torch.cuda.synchronize()
    for got, w in ((a, want), (b, want_more)):
        k = int(got[3][0])
        assert_same_answer((got[0][:k].cpu().numpy(), got[1][:k].cpu().numpy(), got[2][:k].cpu().numpy(), got[3].cpu().numpy()), w)


@gpu
def test_more_than_8192_candidates_are_counted_and_python_raises():
    from columbiaimagesearch_amd import _lib
    det, img, sal, want, _, _ = planted(1, 6)
    flood = HD.FHOGDetectorModel(det.w, [-1e9, -1e9], pyramid_n=6)
    positions = 2 * sum(lv[0].size for lv in sal)
    assert positions > M.MAX_CANDIDATES
    h = create(flood)
    try:
        r, s, f, c = gpu_detect(h, img, 1, max_dets=16)                       # (the guard words behind every buffer are checked in there)
        assert c[1] == positions and 1 <= c[0] <= M.MAX_CANDIDATES
    finally:
        _lib.lib().cis_fhogdet_destroy(h)
    d = HD.HOGDetectorHIP(flood)
    with pytest.raises(RuntimeError, match="%d positions passed the threshold" % positions):
        d.run(img, 1)
    with pytest.raises(RuntimeError, match="positions passed"):
        d.detect_from_img(img, 1)


# ---- the Python surface, the chain, the extractor ----------------------------------------------------------------------------------------------
@gpu
def test_python_surface():
    import torch
    det, img, sal, want, adjust, want_more = planted(1, 6)
    d = HD.HOGDetectorHIP(det)
    rects, scores, filt = d.run(img, 1)
    assert rects.dtype == np.int64 and scores.dtype == F32 and filt.dtype == np.int64
    assert (rects == want[0]).all() and same_bits(scores, want[1]) and (filt == want[2]).all()
    more = d.run(img, 1, adjust)
    assert (more[0] == want_more[0]).all() and same_bits(more[1], want_more[1])
    boxes = d.detect_from_img(img, 1)
    assert [(b["left"], b["top"], b["right"], b["bottom"]) for b in boxes] == [tuple(r) for r in want[0].tolist()]
    assert all(type(b["score"]) is float for b in boxes) and [b["score"] for b in boxes] == [float(s) for s in want[1]]
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.array(img)).save(buf, format="PNG")
    back, boxes2 = d.detect_from_buffer_noinfos(buf.getvalue(), up_sample=1)
    assert (back == img).all() and boxes2 == boxes
    grey = np.array(img)[:, :, 1]
    g3 = M.detect(np.stack([grey] * 3, axis=-1), det, 0)
    assert (d.run(grey, 0)[0] == g3[0]).all()                                 # a grey image is stacked to three channels
    out = d.run_dev(dev(img), 1, max_dets=8)
    assert all(t.is_cuda for t in out) and out[0].shape == (8, 4) and out[0].dtype == torch.int32 and out[3].shape == (2,)
    # argument errors are Python exceptions, nothing is launched
    for bad in (np.zeros((10, 10, 3), np.float32), np.zeros((10, 10, 4), np.uint8), np.zeros((2, 3, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            d.run(bad, 0)
    with pytest.raises(ValueError):
        d.run(img, 3)
    with pytest.raises(ValueError):
        d.run_dev(torch.as_tensor(np.array(img)), 0)                          # not on the GPU
    with pytest.raises(ValueError):
        d.run_dev(dev(img), 0, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
    d.close()
    d.close()
    with pytest.raises(ValueError):
        d.run(img, 0)


@gpu
def test_create_and_run_argument_errors_launch_nothing():
    from columbiaimagesearch_amd import _lib
    L = _lib.lib()
    w, th = np.zeros((17 * 31 * 16 * 16,), F32), np.zeros(17, F32)
    nan = w.copy()
    nan[31 * 100 + 5] = np.nan
    #            F  fr  fc  cell pad N  levels minw minh
    for words, a, ww in ((("F = 17",), (17, 10, 10, 8, 0, 6, 1000, 64, 64), w), (("17 x 10",), (5, 17, 10, 8, 0, 6, 1000, 64, 64), w),
                         (("cell_size = 4",), (5, 10, 10, 4, 0, 6, 1000, 64, 64), w), (("pyramid_down<1>",), (5, 10, 10, 8, 0, 1, 1000, 64, 64), w),
                         (("pyramid_down<17>",), (5, 10, 10, 8, 0, 17, 1000, 64, 64), w), (("padding = 5",), (5, 10, 10, 8, 5, 6, 1000, 64, 64), w),
                         (("weight 5 of filter 1", "not finite"), (5, 10, 10, 8, 0, 6, 1000, 64, 64), nan)):
        out = ctypes.c_void_p()
        rc = L.cis_fhogdet_create(ctypes.byref(out), *(list(a) + [_lib.ptr(ww), _lib.ptr(th), 0.5, 1.0]))
        assert rc == _lib.CIS_EINVAL and out.value is None
        assert all(x in _lib.last_error() for x in words), _lib.last_error()
        with pytest.raises(ValueError):
            _lib.check(rc)
    det = fhog_detector_model(seed=0, F=1, fr=4, fc=4)
    h = create(det)
    try:
        assert L.cis_fhogdet_workspace_bytes(h, 0, 10, 0) == _lib.CIS_EINVAL and L.cis_fhogdet_workspace_bytes(h, 10, 10, 3) == _lib.CIS_EINVAL
        assert L.cis_fhogdet_workspace_bytes(h, 20000, 100, 0) == _lib.CIS_EINVAL and "cells a side" in _lib.last_error()
        need = L.cis_fhogdet_workspace_bytes(h, 100, 100, 1)
        assert need > 0
        one = ctypes.c_void_p(256)                                            # never dereferenced: every call below fails its checks first
        assert L.cis_fhogdet_run_dev(h, one, 100, 100, 1, 0.0, one, need - 1, one, one, one, 4, one, None) == _lib.CIS_EINVAL
        assert "workspace" in _lib.last_error()
        assert L.cis_fhogdet_run_dev(h, None, 100, 100, 1, 0.0, one, need, one, one, one, 4, one, None) == _lib.CIS_EINVAL
        assert L.cis_fhogdet_run_dev(h, one, 100, 100, 1, float("nan"), one, need, one, one, one, 4, one, None) == _lib.CIS_EINVAL
        assert L.cis_resize_bilinear_rgb_dev(one, 10, 10, one, 0, 5, None) == _lib.CIS_EINVAL
        assert L.cis_fhog_extract_dev(one, 100, 100, 4, 1, 1, one, one, None) == _lib.CIS_EINVAL
        assert L.cis_fhog_extract_dev(one, 100, 100, 8, 17, 1, one, one, None) == _lib.CIS_EINVAL
    finally:
        L.cis_fhogdet_destroy(h)


@pytest.fixture(scope="module")
def face_setup(tmp_path_factory):
    from columbiaimagesearch_amd.featurizer import shape_predictor as SP
    from columbiaimagesearch_amd.featurizer.synthetic import dlib_weights, shape_predictor_model
    d = tmp_path_factory.mktemp("hogfaces")
    sp = shape_predictor_model(seed=31, P=68, K=3, T=65, depth=4, F=500)
    SP.save_npz(sp, str(d / "sp.npz"))
    np.savez(str(d / "net.npz"), **dlib_weights(0))
    det = planted(1, 6)[0]
    HD.save_npz(det, str(d / "det.npz"))
    conf = {"DLIBFEAT_pred_path": str(d / "sp.npz"), "DLIBFEAT_rec_path": str(d / "net.npz"), "DLIBFEAT_landmark_backend": "hip",
            "DLIBFEAT_detector_backend": "hip", "DLIBFEAT_det_path": str(d / "det.npz")}
    return sp, conf


@gpu
def test_detector_feeds_the_landmark_predictor_without_a_host_step(face_setup):
    import torch
    from columbiaimagesearch_amd.featurizer import shape_predictor as SP
    sp, conf = face_setup
    det, img, sal, want, _, _ = planted(1, 6)
    n = len(want[0])
    assert n >= 1
    d, p = HD.HOGDetectorHIP(det), SP.ShapePredictorHIP(sp)
    timg = dev(img)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        rects, scores, filt, count = d.run_dev(timg, 1, max_dets=n)           # [n, 4] int32: the layout predict_dev takes
        parts = p.predict_dev(timg, rects)
    st.synchronize()
    assert (rects.cpu().numpy() == want[0]).all()
    assert (parts.cpu().numpy() == p.predict(img, want[0])).all()             # the same landmarks from the host-copied rectangles


@gpu
def test_extractor_runs_the_face_configuration_without_dlib(face_setup, monkeypatch):
    import sys
    from PIL import Image
    from columbiaimagesearch_amd.extractor.generic_extractor import GenericExtractor, get_bbox_str
    monkeypatch.setitem(sys.modules, "dlib", None)                            # `import dlib` raises ImportError
    sp, conf = face_setup
    det, img, sal, want, _, _ = planted(1, 6)
    ex = GenericExtractor("dlib", "dlib", "face", "ext", "DLIBFEAT_", conf)
    assert isinstance(ex.detector, HD.HOGDetectorHIP)
    buf = io.BytesIO()
    Image.fromarray(np.array(img)).save(buf, format="PNG")
    rows = ex.process_batch([buf.getvalue()], _raise=True)
    base = "ext:dlib_feat_dlib_face"
    boxes = [{"left": int(r[0]), "top": int(r[1]), "right": int(r[2]), "bottom": int(r[3]), "score": float(s)} for r, s in zip(want[0], want[1])]
    assert len(boxes) >= 1
    assert sorted(rows[0]) == sorted([base + "_processed"] + [base + "_" + get_bbox_str(b) for b in boxes])
    assert rows[0][base + "_processed"] == "1"
    assert ex.process_buffer(buf.getvalue()) == rows[0]
