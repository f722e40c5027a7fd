"""The numpy model of the HOG detector (tests/fhog_model.py) on cases worked out by hand, the detector model's two file formats, and the
extractor's backend switch.  No GPU here: tests/test_hog_detector.py compares the kernels' bytes with this model's.  Parity with dlib
itself is UNPINNED (no dlib, no detector file here)."""
import numpy as np
import pytest

import fhog_model as M
from columbiaimagesearch_amd.detector import hog_detector as HD
from columbiaimagesearch_amd.featurizer.synthetic import fhog_detector_model

F32 = np.float32


def test_direction_literals_are_the_unit_vectors():
    o = np.arange(9) * np.pi / 9
    want = np.stack([np.cos(o), np.sin(o)], axis=1).astype(F32)
    assert np.abs(M.DIRS.astype(np.float64) - want).max() <= 2.0 ** -24     # the literal is the float32 next to the cosine (or one ulp off)
    assert M.DIRS.dtype == F32


def test_constant_image_gives_zero_features():
    img = np.full((40, 56, 3), 93, np.uint8)
    f = M.fhog(img, 10, 10)
    assert f.shape == (31, 3 + 9, 5 + 9) and (f == 0).all()
    assert M.fhog(np.zeros((19, 40, 3), np.uint8)).shape == (31, 0, 0)       # (int)(19 / 8 + 0.5) = 2 cells: no output
    assert M.fhog(np.zeros((23, 40, 3), np.uint8)).shape == (31, 1, 3)       # (int)(23 / 8 + 0.5) = 3 cells: one row


def test_vertical_step_edge_lands_where_worked_out_by_hand():
    """40 x 40, columns 0..19 black, 20..39 at 200: dx = 200 at x = 19 and x = 20 only, dy = 0: the gradient (200, 0) has its largest
    dot (200) with direction 0, so bin 0, magnitude 200.  x = 19: xp = 19.5 / 8 + 0.5 = 2.9375: 1/16 to dlib's hist column 2 and 15/16 to
    column 3; x = 20: xp = 3.0625: 15/16 to column 3, 1/16 to column 4.  Without dlib's border ring: cell columns 1, 2, 3 get 1/16, 30/16, 1/16
    of 200 times the row weights.  A cell row whose 16 support rows are all valid (rows 1..3) has row weights summing to 8: 100, 3000, 100.
    Cell row 0 covers y = -4..11, valid from y = 1: d = 5..15, weights (11 + 13 + 15 + 64) / 16 = 6.4375: 6.4375 * 1.875 * 200 = 2414.0625;
    cell row 4 the same by symmetry (y = 28..43, valid to 38).  Every product and sum here is exact in float32.
    Output cell (1, 1) = histogram cell (2, 2): the energies around it are 9e6 and 1e4, h * n = 3000 / sqrt(18020000) = 0.71 > 0.2 for all
    four normalisers: plane 0 = 0.5 * (4 * 0.2), plane 18 (bins 0 + 9 folded) the same, the other 25 orientation planes 0, the four
    texture planes 0.2357 * 0.2."""
    img = np.zeros((40, 40, 3), np.uint8)
    img[:, 20:] = 200
    bo, mag = M.gradients(img)
    assert (bo == 0).all() and (mag[1:-1, 19:21] == 200).all() and mag.sum() == 200 * 2 * 38
    h = M.cell_histograms(img)
    assert h.shape == (5, 5, 18) and (h[:, :, 1:] == 0).all()
    assert h[1:4, :, 0].tolist() == [[0, 100, 3000, 100, 0]] * 3
    assert h[0, :, 0].tolist() == [0, 6.4375 * 12.5, 2414.0625, 6.4375 * 12.5, 0] and (h[4] == h[0]).all()
    f = M.fhog(img)
    assert f.shape == (31, 3, 3)
    p0 = F32(0.5) * (((F32(0.2) + F32(0.2)) + F32(0.2)) + F32(0.2))
    assert f[0, 1, 1] == p0 and f[18, 1, 1] == p0 and (f[1:18, 1, 1] == 0).all() and (f[19:27, 1, 1] == 0).all()
    assert (f[27:31, 1, 1] == F32(0.2357) * F32(0.2)).all()
    # the 27 + 4 plane relations on every cell: with one live bin the folded plane equals the signed one, texture = 0.2357 * 2 * plane 0 / 4 ...
    assert (f[18] == f[0]).all()
    np.testing.assert_allclose(f[27:31].sum(axis=0), 0.2357 * 2 * f[0], rtol=1e-6)
    # the zero border of a 6 x 9 filter: 2 rows in front and 3 behind, 4 columns in front and 4 behind
    g = M.fhog(img, 6, 9)
    assert g.shape == (31, 8, 11) and (g[:, 2:5, 4:7] == f).all() and g.sum() == f.sum()


def test_plane_relations_on_a_textured_image():
    rs = np.random.RandomState(5)
    f = M.fhog(rs.randint(0, 256, size=(50, 66, 3)).astype(np.uint8))
    assert f.shape == (31, 4, 6) and f.min() >= 0 and f[:27].max() <= 0.4 + 1e-6
    # texture planes: 0.2357 * sum of the four clipped values over the 18 bins; 0.5 * their sum over the normalisers = the 18 planes summed
    np.testing.assert_allclose(f[27:31].sum(axis=0) * 0.5 / 0.2357, f[:18].sum(axis=0), rtol=1e-5)


def test_gather_agrees_with_dlibs_scatter_loop():
    rs = np.random.RandomState(6)
    for shape in ((37, 45), (24, 24), (40, 33)):
        img = rs.randint(0, 256, size=shape + (3,)).astype(np.uint8)
        np.testing.assert_allclose(M.cell_histograms(img), M.cell_histograms_scatter(img), rtol=2e-6, atol=1e-3)


def test_channel_tie_goes_to_the_earlier_channel():
    """R = 5 x (dx = 10, dy = 0), G = 5 y (dx = 0, dy = 10), B = 0: both have dx^2 + dy^2 = 100.  R wins: gradient (10, 0), bin 0.  With the
    two swapped R gives (0, 10): the dots with directions 4 and 5 are both 9.848, the first stays: bin 4.  Were the later channel taken, the
    two answers would change places."""
    yy, xx = np.mgrid[0:40, 0:40]
    img = np.stack([5 * xx, 5 * yy, 0 * xx], axis=-1).astype(np.uint8)
    assert (M.gradients(img)[0][1:-1, 1:-1] == 0).all()
    assert (M.gradients(img[:, :, [1, 0, 2]])[0][1:-1, 1:-1] == 4).all()
    assert (M.gradients(img[:, :, [2, 1, 0]])[0][1:-1, 1:-1] == 4).all()      # R flat: G's (0, 10) beats it, B's (10, 0) only ties G
    assert (M.gradients(img)[1][1:-1, 1:-1] == 10).all()


def test_rect_up_and_down():
    assert M.point_up(10, 2) == (10 - 0.3) / 0.5 + 0.3
    assert M.rect_up((10, 10, 20, 20), 2) == (20, 20, 40, 40) and M.rect_down((20, 20, 40, 40), 2) == (10, 10, 20, 20)
    assert M.up_size(97, 131) == (193, 261) and M.up_size(1, 1) == (1, 1)
    rs = np.random.RandomState(2)
    for n in (2, 3, 6, 16):
        for levels in (1, 2, 5):
            for _ in range(50):
                r = tuple(int(v) for v in rs.randint(-50, 400, size=4))
                assert M.rect_down(M.rect_up(r, n, levels), n, levels) == r, (n, levels, r)
    # rounded once at the end, not per level: two levels of n = 6 on 15: (15 - 0.3) * 1.2 + 0.3 = 17.94, then 21.468 -> 21; rounded per
    # level it would be 18 -> 21.54 -> 22
    assert M.rect_up((15, 0, 15, 0), 6, 2)[0] == 21 and M.rect_up((M.rect_up((15, 0, 15, 0), 6)[0],) * 4, 6)[0] == 22
    assert M.pyramid_sizes(230, 310, 6, 1000, 64, 64) == [(230, 310), (191, 258), (159, 215), (132, 179), (110, 149), (91, 124), (75, 103)]
    assert M.pyramid_sizes(230, 310, 6, 2, 64, 64) == [(230, 310), (191, 258)] and M.pyramid_sizes(20, 20, 6, 1000, 64, 64) == [(20, 20)]


def test_fhog_to_image_and_the_box_of_a_position():
    """10 x 10 filter: the zero border is 4 cells in front.  Padded cell 4 is output cell 0: (0 + 1) * 8 + 1 + 4 = 13, the centre of the
    histogram's cell 1 (pixels 8..15 shifted by the gradient's one-pixel border).  Padded cell 3 is output cell -1: (-1 + 1) * 8 + 1 - 4 = -3.
    The window at padded (0, 0): centre (5, 5), box of 10 cells from 0 to 9: -4 -> (-3) * 8 + 1 - 4 = -27 and 5 -> 6 * 8 + 1 + 4 = 53."""
    assert M.fhog_to_image((4, 4), 10, 10) == (13, 13) and M.fhog_to_image((3, 4), 10, 10) == (-3, 13)
    assert M.position_rect(0, 0, 10, 10, 0, 0, 6, 0) == (-27, -27, 53, 53)
    assert M.position_rect(4, 4, 10, 10, 0, 0, 6, 0) == (13, 13, 85, 85)
    # padding 1: the box loses one cell a side (8 cells from 1 to 8 around the same centre)
    assert M.position_rect(4, 4, 10, 10, 1, 0, 6, 0) == (21, 21, 77, 77)
    # one level up (n = 6) and one up-sampling round down: (13 - 0.3) * 1.2 + 0.3 = 15.54 -> 16 -> (16 - 0.3) / 2 + 0.3 = 8.15 -> 8
    assert M.position_rect(4, 4, 10, 10, 0, 1, 6, 1)[0] == 8


def test_overlap_test_each_ratio_decides_once():
    a, b, c = (0, 0, 9, 9), (0, 0, 9, 14), (5, 5, 14, 14)
    assert M.overlaps(a, b, 0.5, 1.0) and not M.overlaps(a, b, 0.7, 1.0)       # inner 100, outer 150: 0.667 decides; a is covered 1.0, not > 1.0
    assert M.overlaps(a, b, 0.7, 0.9)                                          # inner / area(a) = 1 > 0.9: the second ratio
    assert M.overlaps(b, a, 0.7, 0.9)                                          # inner / area(b) = 0.667, inner / area(a) = 1: the third
    assert not M.overlaps(a, c, 0.12, 1.0) and M.overlaps(a, c, 0.11, 1.0)     # outer is the BOUNDING box: 25 / 225, not 25 / 175
    assert not M.overlaps(a, (10, 0, 19, 9), 0.0, 0.0)                         # side by side: no common pixel
    assert M.overlaps(a, (9, 9, 12, 12), 0.0, 1.0)                             # one common pixel (areas are inclusive)


def test_equal_scores_are_ordered_by_level_filter_row_column():
    far = lambda i: (100 * i, 0, 100 * i + 9, 9)
    cands = [(F32(1.5), 1, 0, 0, 0, far(0)), (F32(1.5), 0, 1, 0, 0, far(1)), (F32(1.5), 0, 0, 1, 0, far(2)), (F32(1.5), 0, 0, 0, 1, far(3)),
             (F32(2.5), 3, 3, 3, 3, far(4)), (F32(1.5), 0, 0, 0, 0, far(5)), (F32(1.5), 0, 0, 0, 1, far(3))]
    kept = M.nms(cands[::-1], 0.5, 1.0)
    assert [k[1:5] for k in kept] == [(3, 3, 3, 3), (0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 0), (1, 0, 0, 0)]
    assert [k[1:5] for k in M.nms(cands, 0.5, 1.0)] == [k[1:5] for k in kept]


def test_scores_on_a_hand_case():
    feat = np.zeros((31, 3, 4), F32)
    feat[2, 1, 2], feat[30, 2, 3] = 0.25, 0.5
    w = np.zeros((2, 31, 2, 2), F32)
    w[0, 2, 0, 0], w[0, 30, 1, 1], w[1, 2, 1, 1] = 2.0, 4.0, -8.0
    s = M.scores(feat, w)
    assert s.shape == (2, 2, 3)
    assert s[0].tolist() == [[0, 0, 0], [0, 0, 2.5]] and s[1].tolist() == [[0, -2.0, 0], [0, 0, 0]]
    assert M.scores(feat, np.zeros((1, 31, 4, 2), F32)).shape == (1, 0, 0)


# ---- the model's files -------------------------------------------------------------------------------------------------------------------
def assert_same_model(a, b):
    for name, x in a.arrays().items():
        y = b.arrays()[name]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name


def test_npz_and_stream_round_trips(tmp_path):
    m = fhog_detector_model(seed=3, F=3, fr=6, fc=9, padding=1, max_levels=7, min_layer_w=40, min_layer_h=30, iou_thresh=0.4, covered_thresh=0.9)
    m.w[0, 0, 0, :3] = (0.0, F32(1e-42), -1.0)
    new, old = HD.write_fhog_dat(m), HD.write_fhog_dat(m, negate_dims=False)
    assert new != old and len(new) == len(old)
    assert_same_model(m, HD.fhog_from_dat(new))
    assert_same_model(m, HD.fhog_from_dat(old))
    assert HD.fhog_from_dat(new, pyramid_n=3).pyramid_n == 3
    HD.write_fhog_dat(m, str(tmp_path / "det.svm"))
    assert_same_model(m, HD.load_fhog_detector(str(tmp_path / "det.svm")))
    HD.save_npz(m, str(tmp_path / "det.npz"))
    assert_same_model(m, HD.load_fhog_detector(str(tmp_path / "det.npz")))


def test_corrupted_stream_names_its_byte():
    m = fhog_detector_model(seed=4, F=2, fr=4, fc=5)
    data = HD.write_fhog_dat(m)
    for cut in (1, 7, len(data) // 2, len(data) - 1):
        with pytest.raises(ValueError, match=r"byte \d+"):
            HD.fhog_from_dat(data[:cut])
    with pytest.raises(ValueError, match=r"byte \d+.*behind"):
        HD.fhog_from_dat(data + b"\x01\x00")
    assert data[:6] == b"\x01\x02\x01\x01\x01\x08"           # object_detector 2, scan_fhog_pyramid 1, cell_size 8
    with pytest.raises(ValueError, match=r"byte 2: object_detector: version 3"):       # (a version is named behind its two bytes)
        HD.fhog_from_dat(b"\x01\x03" + data[2:])
    with pytest.raises(ValueError, match=r"byte 4: cell_size = 4"):
        HD.fhog_from_dat(data[:5] + b"\x04" + data[6:])
    with pytest.raises(ValueError, match=r"byte 4: integer control byte 0x7f"):
        HD.fhog_from_dat(data[:4] + b"\x7f" + data[5:])
    where = data.index(b"\x82\x6d\x02")                       # -(31 * 4 * 5 + 1) = -621 = -0x026d in two bytes: the header of w[0]
    with pytest.raises(ValueError, match=r"byte %d: w\[0\]: a 620 x 1 matrix where 621 x 1 is expected" % (where + 5)):
        HD.fhog_from_dat(data[:where] + b"\x82\x6c\x02" + data[where + 3:])


def test_model_checks_name_the_offender():
    g = fhog_detector_model(seed=1, F=2, fr=4, fc=5)
    for words, kw in (("F = 17", dict(w=np.zeros((17, 31, 4, 5)), thresh=np.zeros(17))), ("filter_rows = 17", dict(w=np.zeros((2, 31, 17, 5)))),
                      ("w has shape", dict(w=np.zeros((2, 30, 4, 5)))), ("thresh has shape", dict(thresh=np.zeros(3))),
                      ("cell_size = 4", dict(cell_size=4)), ("padding = 2", dict(padding=2)), ("pyramid_n = 1", dict(pyramid_n=1)),
                      ("pyramid_n = 17", dict(pyramid_n=17)), ("max_levels = 0", dict(max_levels=0)), ("overlap thresholds", dict(iou_thresh=1.5))):
        with pytest.raises(ValueError, match=words):
            HD.FHOGDetectorModel(**dict(dict(w=g.w, thresh=g.thresh), **kw))
    w = g.w.copy()
    w[1, 30, 3, 4] = np.nan
    with pytest.raises(ValueError, match=r"w\[1\]\[30\]\[3\]\[4\] is not finite"):
        HD.FHOGDetectorModel(w, g.thresh)


# ---- the extractor's switch ----------------------------------------------------------------------------------------------------------------
def test_default_backend_still_asks_for_the_dlib_module(monkeypatch):
    import sys
    from columbiaimagesearch_amd.extractor.generic_extractor import GenericExtractor, get_detector
    monkeypatch.setitem(sys.modules, "dlib", None)            # `import dlib` raises ImportError, whether or not dlib is installed
    for conf in ({}, {"DLIBFEAT_detector_backend": "dlib"}):
        with pytest.raises(ImportError):
            get_detector("dlib", conf, "DLIBFEAT_")
        with pytest.raises(ImportError):
            GenericExtractor("dlib", "dlib", "face", "ext", "DLIBFEAT_", conf)
    with pytest.raises(ImportError):
        get_detector("dlib")
    assert get_detector("full", {"DLIBFEAT_detector_backend": "hip"}, "DLIBFEAT_") is None
    with pytest.raises(ValueError, match="detector_backend"):
        get_detector("dlib", {"DLIBFEAT_detector_backend": "opencv"}, "DLIBFEAT_")
    with pytest.raises(ValueError, match="DLIBFEAT_det_path"):
        get_detector("dlib", {"DLIBFEAT_detector_backend": "hip"}, "DLIBFEAT_")
