"""numpy statement of what csrc/hog_detector.hip has to compute: dlib's frontal face detector scheme,
object_detector<scan_fhog_pyramid<pyramid_down<N>>>, the call ``detector.run(img, up_sample, adjust_threshold)``, as the project restates
it from the published dlib sources AS REMEMBERED (image_transforms/fhog.h, image_processing/scan_fhog_pyramid.h, box_overlap_testing.h,
image_transforms/image_pyramid.h).  dlib is not available here: parity with dlib itself is UNPINNED.  This file is the yardstick, the
kernels meet it bit for bit (tests/test_hog_detector.py); every rounding and every summation order is stated here.

Known deviations from dlib: dlib scores with separable filters after an SVD of each filter plane, here the saliency is the direct
correlation in one stated order; dlib's pyramid_up / pyramid_down filters are replaced by one bilinear resize (the issue's choice).

Number formats: the resize and all rectangle arithmetic are float64; FHOG and the scores are float32 with every product and every sum
rounded on its own (no fused multiply-add)."""
import numpy as np

F32 = np.float32
CELL = 8
PLANES = 31
MAX_CANDIDATES = 8192

# the 9 unit vectors (cos, sin)(o * pi / 9) as float32 LITERALS: the kernel carries the same decimal strings
DIRS = np.array([[1.0, 0.0],
                 [0.9396926, 0.34202015],
                 [0.76604444, 0.64278764],
                 [0.5, 0.8660254],
                 [0.17364818, 0.98480775],
                 [-0.17364818, 0.98480775],
                 [-0.5, 0.8660254],
                 [-0.76604444, 0.64278764],
                 [-0.9396926, 0.34202015]], dtype=F32)


def _round(v):
    return np.floor(np.float64(v) + 0.5)


# ---- geometry ----------------------------------------------------------------------------------------------------------------------------
def point_up(p, n, levels=1):
    """dlib's pyramid_down<n>::point_up, `levels` times, in double and NOT rounded: p = (p - 0.3) / ratio + 0.3, ratio = (n - 1) / n"""
    ratio = np.float64(n - 1) / np.float64(n)
    p = np.float64(p)
    for _ in range(levels):
        p = (p - 0.3) / ratio + 0.3
    return p


def point_down(p, n, levels=1):
    ratio = np.float64(n - 1) / np.float64(n)
    p = np.float64(p)
    for _ in range(levels):
        p = (p - 0.3) * ratio + 0.3
    return p


def rect_up(rect, n, levels=1):
    """(l, t, r, b): every corner coordinate through point_up `levels` times, rounded ONCE at the end by floor(. + 0.5)"""
    return tuple(int(_round(point_up(v, n, levels))) for v in rect)


def rect_down(rect, n, levels=1):
    return tuple(int(_round(point_down(v, n, levels))) for v in rect)


def up_size(nr, nc):
    """The size pyramid_up gives an nr x nc image: rect_up (n = 2) of the image rectangle (0, 0, nc - 1, nr - 1): 2 nr - 1 by 2 nc - 1"""
    l, t, r, b = rect_up((0, 0, nc - 1, nr - 1), 2)
    return b - t + 1, r - l + 1


def resize_bilinear(img, onr, onc):
    """uint8 [nr, nc, 3] -> [onr, onc, 3].  Source coordinate y = r * ((nr - 1) / max(onr - 1, 1)) in double (the quotient first), top =
    floor(y), bottom = min(top + 1, nr - 1), fy = y - top; the same for x.  Per channel in double
    v = (1 - fy) * ((1 - fx) * tl + fx * tr) + fy * ((1 - fx) * bl + fx * br), the byte is floor(v + 0.5)."""
    nr, nc = img.shape[:2]
    ys = np.arange(onr, dtype=np.float64) * (np.float64(nr - 1) / np.float64(max(onr - 1, 1)))
    xs = np.arange(onc, dtype=np.float64) * (np.float64(nc - 1) / np.float64(max(onc - 1, 1)))
    top, left = np.floor(ys).astype(np.int64), np.floor(xs).astype(np.int64)
    bot, right = np.minimum(top + 1, nr - 1), np.minimum(left + 1, nc - 1)
    fy, fx = (ys - top)[:, None, None], (xs - left)[None, :, None]
    a = img.astype(np.float64)
    tl, tr = a[top][:, left], a[top][:, right]
    bl, br = a[bot][:, left], a[bot][:, right]
    v = (1.0 - fy) * ((1.0 - fx) * tl + fx * tr) + fy * ((1.0 - fx) * bl + fx * br)
    return np.floor(v + 0.5).astype(np.uint8)


def pyramid_sizes(nr, nc, n, max_levels, min_w, min_h):
    """[(nr, nc)] of the levels: level 0 is the image, always (dlib's do-while); level l + 1 is ((n-1) nr) / n by ((n-1) nc) / n in
    integer division, made while there are fewer than max_levels and it is at least min_w wide and min_h high."""
    out = [(nr, nc)]
    while len(out) < max_levels:
        nr, nc = ((n - 1) * nr) // n, ((n - 1) * nc) // n
        if nc < min_w or nr < min_h or nr < 1 or nc < 1:
            break
        out.append((nr, nc))
    return out


# ---- FHOG --------------------------------------------------------------------------------------------------------------------------------
def gradients(img):
    """(bin int [nr, nc], magnitude float32 [nr, nc]) of every pixel that has four neighbours (the others: bin 0, magnitude 0).
    Central differences per channel in integers, the channel with the largest dx^2 + dy^2 wins, the EARLIER one (R, G, B) on a tie.
    dot_o = DIRS[o].x * gx + DIRS[o].y * gy in float32 (two rounded products, one rounded sum); best_dot starts at 0 and o runs 0..8:
    dot > best -> (dot, o), else -dot > best -> (-dot, o + 9).  Magnitude = sqrtf(float(dx^2 + dy^2))."""
    a = img.astype(np.int32)
    nr, nc = a.shape[:2]
    dx, dy = np.zeros_like(a), np.zeros_like(a)
    if nc > 2:
        dx[:, 1:-1] = a[:, 2:] - a[:, :-2]
    if nr > 2:
        dy[1:-1] = a[2:] - a[:-2]
    inner = np.zeros((nr, nc), bool)
    inner[1:-1, 1:-1] = True
    v = dx * dx + dy * dy
    ch = np.argmax(v, axis=2)                                   # the first maximum: the earlier channel on a tie
    pick = lambda t: np.where(inner, np.take_along_axis(t, ch[:, :, None], axis=2)[:, :, 0], 0)
    gx, gy, vv = pick(dx).astype(F32), pick(dy).astype(F32), pick(v).astype(F32)
    best, bo = np.zeros((nr, nc), F32), np.zeros((nr, nc), np.int64)
    for o in range(9):
        dot = DIRS[o, 0] * gx + DIRS[o, 1] * gy
        assert dot.dtype == F32
        up = dot > best
        dn = ~up & (-dot > best)
        best = np.where(up, dot, np.where(dn, -dot, best))
        bo = np.where(up, o, np.where(dn, o + 9, bo))
    return bo, np.sqrt(vv)


def cell_counts(nr, nc):
    return int(nr / float(CELL) + 0.5), int(nc / float(CELL) + 0.5)


def _weight(d):
    """Bilinear weight of the pixel d rows (columns) into a cell's 16-pixel support: dlib's vy0 = yp - floor(yp), yp = (y + 0.5) / 8 + 0.5,
    for the 8 pixels in front (d < 8: (2 d + 1) / 16) and vy1 = 1 - vy0 for the 8 behind ((31 - 2 d) / 16); exact in float32."""
    return F32((2 * d + 1) / 16.0) if d < 8 else F32((31 - 2 * d) / 16.0)


def cell_histograms(img):
    """float32 [cells_nr, cells_nc, 18] (dlib's hist without its outer ring of border cells, which nothing reads).
    A GATHER: cell (r, c) sums the pixels y = 8 r - 4 + dy, x = 8 c - 4 + dx for dy = 0..15 (outer), dx = 0..15 (inner), ROW-MAJOR, starting
    from +0: acc[bin(y, x)] += (wy(dy) * wx(dx)) * magnitude(y, x), the product of the two weights first (exact), for the pixels with
    1 <= y < visible_nr and 1 <= x < visible_nc, visible = min(cells * 8, size) - 1."""
    nr, nc = img.shape[:2]
    cr, cc = cell_counts(nr, nc)
    hist = np.zeros((cr, cc, 18), F32)
    if cr == 0 or cc == 0:
        return hist
    bo, mag = gradients(img)
    vis_r, vis_c = min(cr * CELL, nr) - 1, min(cc * CELL, nc) - 1
    R, C = np.arange(cr)[:, None], np.arange(cc)[None, :]
    for dy in range(16):
        Y = CELL * R - 4 + dy
        oky = (Y >= 1) & (Y < vis_r)
        Yc = np.clip(Y, 0, nr - 1)
        for dx in range(16):
            X = CELL * C - 4 + dx
            ok = oky & (X >= 1) & (X < vis_c)
            Xc = np.clip(X, 0, nc - 1)
            w = _weight(dy) * _weight(dx)
            contrib = np.where(ok, w * mag[Yc, Xc], F32(0))
            assert contrib.dtype == F32
            b = np.where(ok, bo[Yc, Xc], 0)
            hist[R, C, b] = hist[R, C, b] + contrib            # one (cell, bin) per cell and step: no collisions
    return hist


def cell_histograms_scatter(img):
    """dlib's own loop (a scatter over the pixels) in float64 with its border ring: the gather above must agree up to summation order"""
    nr, nc = img.shape[:2]
    cr, cc = cell_counts(nr, nc)
    hist = np.zeros((cr + 2, cc + 2, 18))
    bo, mag = gradients(img)
    vis_r, vis_c = min(cr * CELL, nr) - 1, min(cc * CELL, nc) - 1
    for y in range(1, vis_r):
        yp = (y + 0.5) / CELL + 0.5
        iy = int(np.floor(yp))
        vy0 = yp - iy
        for x in range(1, vis_c):
            xp = (x + 0.5) / CELL + 0.5
            ix = int(np.floor(xp))
            vx0 = xp - ix
            m, b = float(mag[y, x]), bo[y, x]
            hist[iy, ix, b] += (1 - vy0) * (1 - vx0) * m
            hist[iy + 1, ix, b] += vy0 * (1 - vx0) * m
            hist[iy, ix + 1, b] += (1 - vy0) * vx0 * m
            hist[iy + 1, ix + 1, b] += vy0 * vx0 * m
    return hist[1:-1, 1:-1]


def fhog(img, pad_rows=1, pad_cols=1):
    """float32 [31, hog_nr + pad_rows - 1, hog_nc + pad_cols - 1], plane-major; hog = cells - 2, and shape (31, 0, 0) for fewer than 3 cells
    either way.  The zero border: (pad - 1) / 2 rows (columns) in front, the rest behind.
    energy(cell) = sum over o = 0..8, in that order from +0, of (h[o] + h[o + 9])^2.
    With e[.][.] the energies and (y, x) the output cell (cell (y + 1, x + 1) of the histogram), eps = 1e-4f:
      n1 = 1 / sqrtf(((e[y+1][x+1] + e[y+1][x+2]) + e[y+2][x+1]) + e[y+2][x+2] + eps)     n2: rows y, y+1, columns x+1, x+2
      n3: rows y+1, y+2, columns x, x+1                                                   n4: rows y, y+1, columns x, x+1
    each sum in the order (first row left, first row right, second row left, second row right, eps).
    Planes 0..17: 0.5f * (((h1 + h2) + h3) + h4), hi = min(h[o] * ni, 0.2f); planes 18..26 the same on h[o] + h[o + 9];
    planes 27..30: 0.2357f * ti, ti the running sum of hi over o = 0..17 from +0."""
    nr, nc = img.shape[:2]
    cr, cc = cell_counts(nr, nc)
    hr, hc = max(cr - 2, 0), max(cc - 2, 0)
    if hr == 0 or hc == 0:
        return np.zeros((PLANES, 0, 0), F32)
    h = cell_histograms(img)
    e = np.zeros((cr, cc), F32)
    for o in range(9):
        s = h[:, :, o] + h[:, :, o + 9]
        e = e + s * s
    eps = F32(1e-4)

    def norm(r0, c0):
        s = ((e[r0:r0 + hr, c0:c0 + hc] + e[r0:r0 + hr, c0 + 1:c0 + 1 + hc]) + e[r0 + 1:r0 + 1 + hr, c0:c0 + hc]) \
            + e[r0 + 1:r0 + 1 + hr, c0 + 1:c0 + 1 + hc] + eps
        return F32(1) / np.sqrt(s)

    n = [norm(1, 1), norm(0, 1), norm(1, 0), norm(0, 0)]
    hh = h[1:1 + hr, 1:1 + hc]
    out = np.zeros((PLANES, hr + pad_rows - 1, hc + pad_cols - 1), F32)
    r0, c0 = (pad_rows - 1) // 2, (pad_cols - 1) // 2
    t = [np.zeros((hr, hc), F32) for _ in range(4)]
    lim, half = F32(0.2), F32(0.5)
    for o in range(18):
        hs = [np.minimum(hh[:, :, o] * n[i], lim) for i in range(4)]
        out[o, r0:r0 + hr, c0:c0 + hc] = half * (((hs[0] + hs[1]) + hs[2]) + hs[3])
        t = [t[i] + hs[i] for i in range(4)]
    for o in range(9):
        s = hh[:, :, o] + hh[:, :, o + 9]
        hs = [np.minimum(s * n[i], lim) for i in range(4)]
        out[18 + o, r0:r0 + hr, c0:c0 + hc] = half * (((hs[0] + hs[1]) + hs[2]) + hs[3])
    for i in range(4):
        out[27 + i, r0:r0 + hr, c0:c0 + hc] = F32(0.2357) * t[i]
    assert out.dtype == F32
    return out


# ---- scoring -----------------------------------------------------------------------------------------------------------------------------
def scores(feat, w, dtype=F32):
    """[F, R, C]: the correlation of every filter w [F, 31, fr, fc] at every position of feat [31, Hp, Wp] where it fits (R = Hp - fr + 1).
    One accumulator per (position, filter) from +0, the terms PLANE-MAJOR, then filter rows, then filter columns:
    acc = acc + w * f, product and sum rounded on their own.  dtype = np.float64: the same sum in double (the float64 yardstick)."""
    F, P, fr, fc = w.shape
    Hp, Wp = feat.shape[1:]
    R, C = Hp - fr + 1, Wp - fc + 1
    if Hp == 0 or R < 1 or C < 1:
        return np.zeros((F, 0, 0), dtype)
    acc = np.zeros((F, R, C), dtype)
    ww, ff = w.astype(dtype), feat.astype(dtype)
    for p in range(P):
        for i in range(fr):
            for j in range(fc):
                acc = acc + ww[:, p, i, j][:, None, None] * ff[p, i:i + R, j:j + C][None]
    assert acc.dtype == dtype
    return acc


def abs_scores(feat, w):
    """sum |w * f| in double, for the derived error bound of the float32 sum"""
    return scores(np.abs(feat), np.abs(w), np.float64)


def fhog_to_image(p, fr, fc):
    """dlib's fhog_to_image of a point (x, y) in padded-feature cells -> pixel: p' = p - ((fc - 1) / 2, (fr - 1) / 2) (integer division)
    takes the zero border off, then (p' + 1) * 8 + 1 + offset: the one-cell border of the histogram, the one-pixel border of the gradient,
    and the cell centre, offset = +4 for a coordinate >= 0 and -4 for a negative one."""
    x, y = p[0] - (fc - 1) // 2, p[1] - (fr - 1) // 2
    ox, oy = (CELL // 2 if x >= 0 else -(CELL // 2)), (CELL // 2 if y >= 0 else -(CELL // 2))
    return (x + 1) * CELL + 1 + ox, (y + 1) * CELL + 1 + oy


def position_rect(row, col, fr, fc, padding, level, n, up_sample):
    """The box of the filter whose top-left feature cell is (row, col): centre (col + fc / 2, row + fr / 2) (dlib's filter centre),
    centered_rect of (fc - 2 padding) x (fr - 2 padding) cells (left = x - w / 2, right = left + w - 1), fhog_to_image of both corners,
    rect_up by `level` levels (rounded once), then one rounded rect_down (n = 2) per up-sampling round."""
    bw, bh = fc - 2 * padding, fr - 2 * padding
    left, top = col + fc // 2 - bw // 2, row + fr // 2 - bh // 2
    l, t = fhog_to_image((left, top), fr, fc)
    r, b = fhog_to_image((left + bw - 1, top + bh - 1), fr, fc)
    rect = rect_up((l, t, r, b), n, level)
    for _ in range(up_sample):
        rect = rect_down(rect, 2)
    return rect


def overlaps(a, b, iou_thresh, covered_thresh):
    """dlib's test_box_overlap: rectangles (l, t, r, b) with inclusive pixel areas; false when they do not intersect; else with inner the
    intersection's area and outer the area of the BOUNDING rectangle of both (dlib's a + b), in double:
    inner / outer > iou_thresh or inner / area(a) > covered_thresh or inner / area(b) > covered_thresh."""
    area = lambda q: max(q[2] - q[0] + 1, 0) * max(q[3] - q[1] + 1, 0)
    inner = area((max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])))
    if inner == 0:
        return False
    outer = area((min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3])))
    inner = np.float64(inner)
    return bool(inner / np.float64(outer) > iou_thresh or inner / np.float64(area(a)) > covered_thresh
                or inner / np.float64(area(b)) > covered_thresh)


def nms(cands, iou_thresh, covered_thresh):
    """cands: [(score float32, level, filter, row, col, rect)].  Ordered by score descending, ties by (level, filter, row, col) ascending
    (a total order); greedy: kept unless it overlaps an earlier kept one."""
    order = sorted(cands, key=lambda c: (-float(c[0]), c[1], c[2], c[3], c[4]))
    kept = []
    for c in order:
        if not any(overlaps(k[5], c[5], iou_thresh, covered_thresh) for k in kept):
            kept.append(c)
    return kept


def pyramid(img, det, up_sample):
    for _ in range(up_sample):
        img = resize_bilinear(img, *up_size(*img.shape[:2]))
    levels = [img]
    for nr, nc in pyramid_sizes(img.shape[0], img.shape[1], det.pyramid_n, det.max_levels, det.min_layer_w, det.min_layer_h)[1:]:
        levels.append(resize_bilinear(levels[-1], nr, nc))
    return levels


def level_scores(img, det, up_sample):
    """[float32 [F, R, C] per level]"""
    fr, fc = det.w.shape[2:]
    return [scores(fhog(lv, fr, fc), det.w) for lv in pyramid(img, det, up_sample)]


def candidates(sal, det, up_sample, adjust_threshold=0.0):
    """A position is a candidate when double(saliency) >= double(thresh) + adjust_threshold; its score is saliency - thresh in float32."""
    F, _, fr, fc = det.w.shape
    out = []
    for level, s in enumerate(sal):
        for f in range(F):
            ok = np.argwhere(s[f].astype(np.float64) >= np.float64(det.thresh[f]) + np.float64(adjust_threshold))
            for r, c in ok:
                out.append((F32(s[f, r, c] - det.thresh[f]), level, f, int(r), int(c),
                            position_rect(int(r), int(c), fr, fc, det.padding, level, det.pyramid_n, up_sample)))
    return out


def detect(img, det, up_sample=1, adjust_threshold=0.0, sal=None):
    """-> (rects int64 [n, 4] (l, t, r, b), scores float32 [n], filter index int64 [n], number of candidates) in NMS order"""
    sal = level_scores(img, det, up_sample) if sal is None else sal
    cands = candidates(sal, det, up_sample, adjust_threshold)
    kept = nms(cands, det.iou_thresh, det.covered_thresh)
    return (np.array([k[5] for k in kept], np.int64).reshape(-1, 4), np.array([k[0] for k in kept], F32),
            np.array([k[2] for k in kept], np.int64), len(cands))
