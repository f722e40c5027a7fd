"""numpy statement of what csrc/shape_predictor.hip (cis_shapepred_run_dev) has to compute: dlib's shape_predictor::operator()(img, rect)
as the project restates it (parity with dlib itself is UNPINNED: no dlib and no model file here).  float32 where dlib computes in float,
double where dlib computes in double, and the one summation order the kernel documents for the similarity transform.  No GPU here; the
tests compare the kernel's bytes with this model's."""
import numpy as np

F32 = np.float32


def ordered_sum(v):
    """The kernel's fixed order for a sum over the P points, in double: partial sum l takes the points l, l + 64, ... in turn, starting
    from zero; the 64 partial sums then meet in a butterfly over the distances 32, 16, 8, 4, 2, 1 (v = v + v[i ^ s])."""
    v = np.asarray(v, dtype=np.float64)
    rows = -(-len(v) // 64)
    pad = np.zeros(rows * 64)
    pad[:len(v)] = v
    acc = np.zeros(64)
    for r in pad.reshape(rows, 64):
        acc = acc + r
    lanes = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ s]
    assert (acc == acc[0]).all() or np.isnan(acc).any()
    return acc[0]


def similarity_closed_form(from_pts, to_pts, total=ordered_sum):
    """The 2 x 2 part of the least-squares similarity from_pts -> to_pts ([P, 2] each), in double, by the closed form of the 2-D problem:
    a = sum f'.t' / sum |f'|^2, b = sum f' x t' / sum |f'|^2 on the centred points, m = [[a, -b], [b, a]]; the identity for P = 1 and
    for sum |f'|^2 = 0.  (Umeyama's det(cov) < 0 branch changes the scale from (d0 + d1) / sigma to (d0 - d1) / sigma and keeps a
    rotation: in 2-D that is the same a and b -- test_shape_predictor.py checks it against the SVD form.)"""
    f = np.asarray(from_pts, dtype=np.float64)
    t = np.asarray(to_pts, dtype=np.float64)
    n = f.shape[0]
    if n == 1:
        return np.eye(2)
    fx, fy = f[:, 0] - total(f[:, 0]) / n, f[:, 1] - total(f[:, 1]) / n
    tx, ty = t[:, 0] - total(t[:, 0]) / n, t[:, 1] - total(t[:, 1]) / n
    ff = total(fx * fx + fy * fy)
    sd = total(fx * tx + fy * ty)
    sc = total(fx * ty - fy * tx)
    if ff == 0:
        return np.eye(2)
    a, b = sd / ff, sc / ff
    return np.array([[a, -b], [b, a]])


def _round(v):
    return np.floor(v + 0.5)


def feature_pixels(img, rect, m32, deltas, anchors, cur):
    """(values float32 [F], pixel positions float64 [F, 2]) of one level: q = m * delta + location(cur, anchor) in float32 (two products and
    an add per row, then the add), the image position in double, floor(. + 0.5), (R + G + B) / 3 in integer division, 0 outside."""
    left, top, right, bottom = [np.float64(v) for v in rect]
    dx, dy = deltas[:, 0], deltas[:, 1]
    qx = (m32[0, 0] * dx + m32[0, 1] * dy) + cur[2 * anchors]
    qy = (m32[1, 0] * dx + m32[1, 1] * dy) + cur[2 * anchors + 1]
    assert qx.dtype == F32 and qy.dtype == F32
    px = _round(left + qx.astype(np.float64) * (right - left))
    py = _round(top + qy.astype(np.float64) * (bottom - top))
    nr, nc = img.shape[:2]
    inside = (px >= 0) & (px < nc) & (py >= 0) & (py < nr)
    xi, yi = np.where(inside, px, 0).astype(np.int64), np.where(inside, py, 0).astype(np.int64)
    grey = (img[yi, xi].astype(np.uint32).sum(axis=1) // 3).astype(F32) if nr and nc else np.zeros(len(px), F32)
    return np.where(inside, grey, F32(0)).astype(F32), np.stack([px, py], axis=1)


def walk(split_idx, split_thresh, pix):
    """leaf numbers [T] of one level: i = 0; while i < S: i = 2i + 1 if pix[idx1] - pix[idx2] > thresh else 2i + 2; leaf = i - S"""
    T, S = split_thresh.shape
    i = np.zeros(T, dtype=np.int64)
    rows = np.arange(T)
    while (i < S).any():
        live = i < S
        j = np.where(live, i, 0)
        diff = pix[split_idx[rows, j, 0]] - pix[split_idx[rows, j, 1]]
        assert diff.dtype == F32
        with np.errstate(invalid="ignore"):
            left = diff > split_thresh[rows, j]
        i = np.where(live, np.where(left, 2 * i + 1, 2 * i + 2), i)
    return i - S


def sequential_sum(cur, rows):
    """cur + rows[0] + rows[1] + ... one row after another in float32 (np.add.accumulate is strictly sequential)"""
    stack = np.concatenate([cur[None].astype(F32), rows.astype(F32)], axis=0)
    return np.add.accumulate(stack, axis=0, dtype=F32)[-1]


def predict_one(model, img, rect, similarity=similarity_closed_form, trace=None):
    """(parts int32 [P, 2], shape float32 [2P]) for one rectangle (left, top, right, bottom).  `similarity` swaps the form of the
    transform (the tests run the SVD form through the same inputs); `trace` collects the feature-pixel positions of every level."""
    init = model.initial_shape
    P = model.P
    cur = init.copy()
    for k in range(model.K):
        m32 = similarity(init.reshape(P, 2), cur.reshape(P, 2)).astype(F32)
        pix, pos = feature_pixels(img, rect, m32, model.deltas[k], model.anchor_idx[k], cur)
        if trace is not None:
            trace.append(pos)
        leaf = walk(model.split_idx[k], model.split_thresh[k], pix)
        cur = sequential_sum(cur, model.leaves[k][np.arange(model.T), leaf])
    left, top, right, bottom = [np.float64(v) for v in rect]
    x = _round(left + cur[0::2].astype(np.float64) * (right - left))
    y = _round(top + cur[1::2].astype(np.float64) * (bottom - top))
    lo, hi = -2147483648.0, 2147483647.0   # the ends of int32 stand in for positions beyond them
    parts = np.stack([np.clip(x, lo, hi), np.clip(y, lo, hi)], axis=1).astype(np.int32)
    return parts, cur


def predict(model, img, rects):
    out = [predict_one(model, img, r) for r in rects]
    return (np.stack([o[0] for o in out]) if out else np.zeros((0, model.P, 2), np.int32),
            np.stack([o[1] for o in out]) if out else np.zeros((0, 2 * model.P), F32))
