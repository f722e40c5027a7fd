"""dlib's HOG face detector (``dlib.get_frontal_face_detector().run(img, up_sample, adjust_threshold)``, the reference's
cufacesearch/cufacesearch/detector/dlib_detector.py:33) as plain arrays, its stream format, and the GPU detector that runs them
(csrc/hog_detector.hip).

**Unpinned, and restated from the published dlib sources as the author remembers them** (dlib/image_processing/object_detector.h,
scan_fhog_pyramid.h, box_overlap_testing.h, dlib/image_transforms/fhog.h, dlib/serialize.h): there is no dlib and no detector file in
the build image, so the reader is tested against the writer below only, the kernels against the numpy model tests/fhog_model.py, and no
real detector file has ever met the reader.  Known deviations from dlib: the saliency is the direct correlation in one stated order
(dlib filters separably after an SVD of each filter plane and rounds differently), and one bilinear resize stands in for pyramid_up and
pyramid_down<N>.  As in dlib_dat.py the reader checks everything it reads and stops with the byte offset at the first disagreement.

The stream (what ``detector.save(path)`` writes for an ``fhog_object_detector``; it is the only way to get the frontal-face weights out
of dlib: ``dlib.get_frontal_face_detector().save("frontal_face.svm")`` where the installed dlib offers it):
  * ``int version`` (2) of object_detector;
  * the scanner, scan_fhog_pyramid: ``int version`` (1), cell_size, padding, window_width, window_height (pixels: the filter has
    (int)(window / cell_size + 0.5) + 2 padding cells a side), max_pyramid_levels, min_pyramid_layer_width, min_pyramid_layer_height,
    the nuclear norm regularisation strength (a double, not used here), the number of dimensions (31 * filter_rows * filter_cols);
  * the overlap tester, test_box_overlap: iou_thresh, percent_covered_thresh (doubles);
  * ``std::vector`` of the w vectors: its size F, then each as ``matrix<double,0,1>`` = nr, nc (the newer encoding writes both NEGATED;
    either sign is accepted), then the elements through the float serialiser, plane-major, rows, columns, the THRESHOLD last.
The pyramid's N is a template argument of the C++ type and not in the stream: the loader takes it (6 for the face detector).
"""
import ctypes
import io

import numpy as np

from .. import _lib
from ..featurizer.dlib_dat import _Out
from ..featurizer.shape_predictor import _SpIn, _encode_reals

MAX_F, MAX_SIDE, PLANES, CELL, MAX_CANDIDATES = 16, 16, 31, 8, 8192   # csrc/hog_detector.hip
_ARRAYS = ("w", "thresh")
_SCALARS = ("cell_size", "padding", "pyramid_n", "max_levels", "min_layer_w", "min_layer_h")


class FHOGDetectorModel(object):
    """w [F, 31, filter_rows, filter_cols] float32 (plane-major: the order of dlib's w vector), thresh [F] float32; cell_size (8),
    padding (cells of the filter's sides outside the box), pyramid_n (dlib's pyramid_down<N>), max_levels, min_layer_w, min_layer_h
    (pixels), iou_thresh and covered_thresh of the overlap tester."""

    def __init__(self, w, thresh, cell_size=8, padding=0, pyramid_n=6, max_levels=1000, min_layer_w=64, min_layer_h=64, iou_thresh=0.5,
                 covered_thresh=1.0):
        self.w = np.ascontiguousarray(w, dtype=np.float32)
        self.thresh = np.ascontiguousarray(thresh, dtype=np.float32)
        self.cell_size, self.padding, self.pyramid_n = int(cell_size), int(padding), int(pyramid_n)
        self.max_levels, self.min_layer_w, self.min_layer_h = int(max_levels), int(min_layer_w), int(min_layer_h)
        self.iou_thresh, self.covered_thresh = float(iou_thresh), float(covered_thresh)
        self.validate()

    F = property(lambda self: self.w.shape[0])
    filter_rows = property(lambda self: self.w.shape[2])
    filter_cols = property(lambda self: self.w.shape[3])

    def validate(self):
        """ValueError naming the offender, before anything is uploaded."""
        if self.w.ndim != 4 or self.w.shape[1] != PLANES or 0 in self.w.shape:
            raise ValueError("fhog detector: w has shape %r, expected [F, 31, filter_rows, filter_cols]" % (self.w.shape,))
        if self.thresh.shape != (self.F,):
            raise ValueError("fhog detector: thresh has shape %r, expected %r" % (self.thresh.shape, (self.F,)))
        for what, v, lim in (("F", self.F, MAX_F), ("filter_rows", self.filter_rows, MAX_SIDE), ("filter_cols", self.filter_cols, MAX_SIDE)):
            if v > lim:
                raise ValueError("fhog detector: %s = %d is beyond the kernel's limit of %d" % (what, v, lim))
        if self.cell_size != CELL:
            raise ValueError("fhog detector: cell_size = %d, the kernel takes %d" % (self.cell_size, CELL))
        if self.padding < 0 or 2 * self.padding >= min(self.filter_rows, self.filter_cols):
            raise ValueError("fhog detector: padding = %d leaves no box of a %d x %d filter" % (self.padding, self.filter_rows, self.filter_cols))
        if not 2 <= self.pyramid_n <= 16:
            raise ValueError("fhog detector: pyramid_n = %d, the kernel takes 2 to 16" % self.pyramid_n)
        if self.max_levels < 1 or self.min_layer_w < 1 or self.min_layer_h < 1:
            raise ValueError("fhog detector: max_levels = %d, min layer %d x %d: all must be at least 1"
                             % (self.max_levels, self.min_layer_w, self.min_layer_h))
        if not (0.0 <= self.iou_thresh <= 1.0 and 0.0 <= self.covered_thresh <= 1.0):
            raise ValueError("fhog detector: overlap thresholds %r, %r are not in [0, 1]" % (self.iou_thresh, self.covered_thresh))
        bad = np.argwhere(~np.isfinite(self.w))
        if len(bad):
            raise ValueError("fhog detector: w[%d][%d][%d][%d] is not finite" % tuple(bad[0]))
        bad = np.argwhere(~np.isfinite(self.thresh))
        if len(bad):
            raise ValueError("fhog detector: thresh[%d] is not finite" % bad[0, 0])

    def arrays(self):
        d = {n: getattr(self, n) for n in _ARRAYS}
        d.update({n: np.int64(getattr(self, n)) for n in _SCALARS})
        d.update(iou_thresh=np.float64(self.iou_thresh), covered_thresh=np.float64(self.covered_thresh))
        return d


def save_npz(model, path):
    np.savez(path, **model.arrays())


def fhog_from_npz(path):
    z = np.load(path)
    names = _ARRAYS + _SCALARS + ("iou_thresh", "covered_thresh")
    missing = [n for n in names if n not in z.files]
    if missing:
        raise ValueError("fhog detector .npz %s: no array %r" % (path, missing[0]))
    return FHOGDetectorModel(z["w"], z["thresh"], **{n: z[n][()] for n in names[2:]})


def fhog_from_dat(path_or_bytes, pyramid_n=6):
    """FHOGDetectorModel from dlib's serialised fhog_object_detector (see the module docstring: unpinned)."""
    buf = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else open(path_or_bytes, "rb").read()
    s = _SpIn(buf)
    s.expect_version("object_detector", (2,))
    s.expect_version("scan_fhog_pyramid", (1,))
    at = s.p
    cell, padding = s.size("cell_size", 1 << 16), s.size("padding", 1 << 16)
    if cell != CELL:
        s.p = at
        s.fail("cell_size = %d, the kernel takes %d" % (cell, CELL))
    win_w, win_h = s.size("window_width", 1 << 20), s.size("window_height", 1 << 20)
    max_levels, min_w, min_h = s.size("max_pyramid_levels", 1 << 31), s.size("min_pyramid_layer_width", 1 << 31), s.size("min_pyramid_layer_height", 1 << 31)
    s.real()                                                    # nuclear_norm_regularization_strength
    at = s.p
    dims = s.size("number of dimensions", 1 << 31)
    fc, fr = int(win_w / float(cell) + 0.5) + 2 * padding, int(win_h / float(cell) + 0.5) + 2 * padding
    if dims != PLANES * fr * fc or not (1 <= fr <= MAX_SIDE and 1 <= fc <= MAX_SIDE):
        s.p = at
        s.fail("%d dimensions for a window of %d x %d pixels with padding %d: %d x %d cells of 31 planes (sides of 1 to %d) are expected"
               % (dims, win_w, win_h, padding, fr, fc, MAX_SIDE))
    iou, covered = s.real(), s.real()
    F = s.size("w vectors", MAX_F)
    if F < 1:
        s.fail("no filter")
    w = np.empty((F, dims + 1), np.float32)
    for f in range(F):
        w[f] = s.column("w[%d]" % f, dims + 1)
    if s.p != len(s.b):
        s.fail("%d bytes behind the detector" % (len(s.b) - s.p))
    try:
        return FHOGDetectorModel(w[:, :dims].reshape(F, PLANES, fr, fc), w[:, dims], cell, padding, pyramid_n, max(max_levels, 1), max(min_w, 1),
                                 max(min_h, 1), iou, covered)
    except ValueError as e:
        raise ValueError("dlib .dat stream: %s" % e)


def write_fhog_dat(model, path=None, negate_dims=True):
    """The stream fhog_from_dat reads.  negate_dims: the newer matrix encoding (both dimensions written negated) or the older one."""
    sign = -1 if negate_dims else 1
    o = _Out()
    o.int(2)
    o.int(1)
    for v in (model.cell_size, model.padding, (model.filter_cols - 2 * model.padding) * model.cell_size,
              (model.filter_rows - 2 * model.padding) * model.cell_size, model.max_levels, model.min_layer_w, model.min_layer_h):
        o.int(v)
    o.real(0.0)
    dims = PLANES * model.filter_rows * model.filter_cols
    o.int(dims)
    o.real(model.iou_thresh)
    o.real(model.covered_thresh)
    o.int(model.F)
    for f in range(model.F):
        o.int(sign * (dims + 1)); o.int(sign * 1)
        o.parts.append(_encode_reals(np.concatenate([model.w[f].ravel(), model.thresh[f:f + 1]]))[0])
    data = b"".join(o.parts)
    if path is not None:
        with open(path, "wb") as f:
            f.write(data)
    return data


def load_fhog_detector(path, pyramid_n=6):
    """det_path of the extractor's configuration: an .npz of the model's arrays, or dlib's own serialisation of an fhog_object_detector
    (any other suffix: what ``detector.save(path)`` writes, usually .svm or .dat)"""
    path = str(path)
    if path.endswith(".npz"):
        return fhog_from_npz(path)
    return fhog_from_dat(path, pyramid_n)


# ---- the detector on the GPU -----------------------------------------------------------------------------------------------------------
class HOGDetectorHIP(object):
    """dlib's frontal face detector scheme on the MI355X (csrc/hog_detector.hip), with the surface of the reference's DLibFaceDetector."""

    max_dets = 1024   # rows of the output buffers of run / run_dev

    def __init__(self, model):
        self.model = model
        out = _lib.c_void_p()
        _lib.check(_lib.lib().cis_fhogdet_create(ctypes.byref(out), model.F, model.filter_rows, model.filter_cols, model.cell_size, model.padding,
                                                 model.pyramid_n, model.max_levels, model.min_layer_w, model.min_layer_h, _lib.ptr(model.w),
                                                 _lib.ptr(model.thresh), model.iou_thresh, model.covered_thresh))
        self._h = out.value

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().cis_fhogdet_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def workspace_bytes(self, nr, nc, up_sample):
        if self._h is None:
            raise ValueError("the detector is closed")
        n = int(_lib.lib().cis_fhogdet_workspace_bytes(self._h, int(nr), int(nc), int(up_sample)))
        if n < 0:
            _lib.check(n)
        return n

    def run_dev(self, img, up_sample=1, adjust_threshold=0.0, max_dets=None, workspace=None):
        """img: contiguous uint8 CUDA tensor [H, W, 3] RGB -> (rects int32 [max_dets, 4] (left, top, right, bottom), scores float32
        [max_dets], filter index int32 [max_dets], count int32 [2]: kept, candidates), CUDA tensors, asynchronous on the current torch
        stream, no synchronisation: the first min(count[0], max_dets) rows are the answer, and count[1] > 8192 means that candidates were
        dropped (run raises then).  workspace: a uint8 CUDA tensor of at least workspace_bytes(H, W, up_sample), else one is taken from
        torch's caching allocator."""
        import torch
        if self._h is None:
            raise ValueError("the detector is closed")
        if not (hasattr(img, "is_cuda") and img.is_cuda and img.is_contiguous() and img.dtype == torch.uint8 and img.dim() == 3
                and img.shape[2] == 3 and img.shape[0] >= 1 and img.shape[1] >= 1):
            raise ValueError("img must be a contiguous uint8 [H, W, 3] tensor on the GPU")
        if up_sample not in (0, 1, 2):
            raise ValueError("up_sample = %r: 0, 1 or 2 is taken" % (up_sample,))
        max_dets = self.max_dets if max_dets is None else int(max_dets)
        if max_dets < 1:
            raise ValueError("max_dets = %d" % max_dets)
        nr, nc = int(img.shape[0]), int(img.shape[1])
        need = self.workspace_bytes(nr, nc, up_sample)
        if workspace is None:
            workspace = torch.empty(need, dtype=torch.uint8, device=img.device)
        elif not (workspace.is_cuda and workspace.is_contiguous() and workspace.dtype == torch.uint8 and workspace.numel() >= need
                  and workspace.device == img.device):
            raise ValueError("workspace must be a contiguous uint8 tensor of at least %d bytes on the image's GPU" % need)
        rects = torch.empty((max_dets, 4), dtype=torch.int32, device=img.device)
        scores = torch.empty(max_dets, dtype=torch.float32, device=img.device)
        filt = torch.empty(max_dets, dtype=torch.int32, device=img.device)
        count = torch.empty(2, dtype=torch.int32, device=img.device)
        stream = torch.cuda.current_stream(img.device)
        _lib.check(_lib.lib().cis_fhogdet_run_dev(self._h, img.data_ptr(), nr, nc, int(up_sample), float(adjust_threshold), workspace.data_ptr(),
                                                  int(workspace.numel()), rects.data_ptr(), scores.data_ptr(), filt.data_ptr(), max_dets,
                                                  count.data_ptr(), stream.cuda_stream))
        workspace.record_stream(stream)
        return rects, scores, filt, count

    def run(self, img, up_sample=1, adjust_threshold=0.0):
        """img [H, W, 3] uint8 RGB or [H, W] grey (numpy or tensor) -> (rects np.int64 [n, 4], scores np.float32 [n], filter index np.int64
        [n]) in dlib's order.  RuntimeError when more than 8192 positions pass the threshold or more than max_dets boxes survive."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        if hasattr(img, "is_cuda"):
            timg = img if img.dim() == 3 else torch.stack([img] * 3, dim=-1)
        else:
            a = np.asarray(img)
            if a.dtype != np.uint8:
                raise ValueError("img must be uint8, got %s" % a.dtype)
            if a.ndim == 2:
                a = np.stack([a] * 3, axis=-1)      # gray2rgb, as the featurizer does
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("img must be [H, W, 3] or [H, W], got shape %r" % (a.shape,))
            timg = torch.as_tensor(np.ascontiguousarray(a).copy())
        rects, scores, filt, count = self.run_dev(timg.to(dev).contiguous(), up_sample, adjust_threshold)
        kept, cands = (int(v) for v in count.cpu().numpy())
        if cands > MAX_CANDIDATES:
            raise RuntimeError("fhog detector: %d positions passed the threshold, the candidate buffer holds %d: raise the threshold"
                               % (cands, MAX_CANDIDATES))
        if kept > rects.shape[0]:
            raise RuntimeError("fhog detector: %d detections, the output buffers hold %d (max_dets)" % (kept, rects.shape[0]))
        return rects[:kept].cpu().numpy().astype(np.int64), scores[:kept].cpu().numpy(), filt[:kept].cpu().numpy().astype(np.int64)

    # the reference's DLibFaceDetector surface (detector/dlib_detector.py, detector/generic_detector.py)
    def detect_from_img(self, img, up_sample=1):
        rects, scores, _ = self.run(img, up_sample, 0.0)
        return [{"left": int(r[0]), "top": int(r[1]), "right": int(r[2]), "bottom": int(r[3]), "score": float(s)} for r, s in zip(rects, scores)]

    def detect_from_buffer_noinfos(self, img_buffer, up_sample=1):
        from PIL import Image
        img = np.asarray(Image.open(io.BytesIO(img_buffer) if isinstance(img_buffer, (bytes, bytearray)) else img_buffer).convert("RGB"))
        return img, self.detect_from_img(img, up_sample)
