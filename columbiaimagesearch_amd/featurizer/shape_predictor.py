"""dlib's landmark predictor (``dlib.shape_predictor(pred_path)(img, rect)``, cufacesearch/cufacesearch/featurizer/dlib_featurizer.py:103)
as plain arrays, its stream format, and the GPU predictor that runs them (csrc/shape_predictor.hip).

**Unpinned, and restated from the published dlib sources as the author remembers them** (dlib/image_processing/shape_predictor.h,
dlib/serialize.h, dlib/matrix/matrix.h, dlib/geometry/vector.h): there is no dlib and no ``shape_predictor_68_face_landmarks.dat`` in the
build image, so the reader is tested against the writer below only, and the kernel against the numpy model tests/shape_model.py.  As in
dlib_dat.py the reader checks everything it reads and stops with the byte offset at the first disagreement; it never guesses.

The stream (``deserialize(path) >> sp``):
  * ``int version`` (1);
  * ``initial_shape``: ``matrix<float,0,1>`` = nr, nc (the newer encoding writes both NEGATED; either sign is accepted), then the elements
    row-major, each through the float serialiser (integer mantissa, integer exponent: dlib_dat.py's primitives);
  * ``forests``: ``std::vector<std::vector<regression_tree>>`` -- a std::vector is its size, then the items; a ``regression_tree`` is
    ``splits`` (vector of ``split_feature`` = idx1, idx2, thresh) and ``leaf_values`` (vector of ``matrix<float,0,1>``);
  * ``anchor_idx``: ``vector<vector<unsigned long>>``; ``deltas``: ``vector<vector<dlib::vector<float,2>>>`` (x, then y).
The real 68-point file holds about 16 million serialised floats: runs of them are decoded by the host helper ``cis_dlib_decode_reals``
of libcis_hip.so and encoded with numpy, not item by item.
"""
import ctypes

import numpy as np

from .. import _lib
from .dlib_dat import _In, _Out

MAX_COORDS, MAX_F, MAX_T, MAX_DEPTH = 256, 4096, 4096, 8   # csrc/shape_predictor.hip
_ARRAYS = ("initial_shape", "split_idx", "split_thresh", "leaves", "anchor_idx", "deltas")


class ShapePredictorModel(object):
    """initial_shape [2P] float32 (x0, y0, x1, y1, ...), split_idx [K, T, S, 2] int32, split_thresh [K, T, S] float32,
    leaves [K, T, S + 1, 2P] float32, anchor_idx [K, F] int32, deltas [K, F, 2] float32; S = 2**depth - 1."""

    def __init__(self, initial_shape, split_idx, split_thresh, leaves, anchor_idx, deltas):
        self.initial_shape = np.ascontiguousarray(initial_shape, dtype=np.float32)
        self.split_idx = np.ascontiguousarray(split_idx, dtype=np.int32)
        self.split_thresh = np.ascontiguousarray(split_thresh, dtype=np.float32)
        self.leaves = np.ascontiguousarray(leaves, dtype=np.float32)
        self.anchor_idx = np.ascontiguousarray(anchor_idx, dtype=np.int32)
        self.deltas = np.ascontiguousarray(deltas, dtype=np.float32)
        self.validate()

    P = property(lambda self: self.initial_shape.shape[0] // 2)
    K = property(lambda self: self.split_idx.shape[0])
    T = property(lambda self: self.split_idx.shape[1])
    S = property(lambda self: self.split_idx.shape[2])
    F = property(lambda self: self.anchor_idx.shape[1])
    depth = property(lambda self: int(self.S + 1).bit_length() - 1)

    def validate(self):
        """ValueError naming the offender, before anything is uploaded."""
        a = self.initial_shape
        if a.ndim != 1 or a.shape[0] < 2 or a.shape[0] % 2:
            raise ValueError("shape predictor: initial_shape has shape %r, expected [2P]" % (a.shape,))
        if self.split_idx.ndim != 4 or self.split_idx.shape[3] != 2 or 0 in self.split_idx.shape:
            raise ValueError("shape predictor: split_idx has shape %r, expected [K, T, S, 2]" % (self.split_idx.shape,))
        P, K, T, S = self.P, self.K, self.T, self.S
        if (S + 1) & S:
            raise ValueError("shape predictor: %d splits per tree is not a power of two minus one" % S)
        if self.anchor_idx.ndim != 2 or self.anchor_idx.shape[0] != K or self.anchor_idx.shape[1] < 1:
            raise ValueError("shape predictor: anchor_idx has shape %r, expected [K = %d, F]" % (self.anchor_idx.shape, K))
        F = self.F
        for name, want in (("split_thresh", (K, T, S)), ("leaves", (K, T, S + 1, 2 * P)), ("deltas", (K, F, 2))):
            if getattr(self, name).shape != want:
                raise ValueError("shape predictor: %s has shape %r, expected %r" % (name, getattr(self, name).shape, want))
        for what, v, lim in (("2P", 2 * P, MAX_COORDS), ("F", F, MAX_F), ("T", T, MAX_T), ("depth", self.depth, MAX_DEPTH)):
            if v > lim:
                raise ValueError("shape predictor: %s = %d is beyond the kernel's limit of %d" % (what, v, lim))
        bad = np.argwhere((self.anchor_idx < 0) | (self.anchor_idx >= P))
        if len(bad):
            k, i = bad[0]
            raise ValueError("shape predictor: anchor_idx[%d][%d] = %d is not a landmark (P = %d)" % (k, i, self.anchor_idx[k, i], P))
        bad = np.argwhere((self.split_idx < 0) | (self.split_idx >= F))
        if len(bad):
            k, t, s, j = bad[0]
            raise ValueError("shape predictor: split_idx[%d][%d][%d][%d] = %d is not a feature (F = %d)"
                             % (k, t, s, j, self.split_idx[k, t, s, j], F))

    def arrays(self):
        return {n: getattr(self, n) for n in _ARRAYS}


def save_npz(model, path):
    np.savez(path, **model.arrays())


def sp_from_npz(path):
    z = np.load(path)
    missing = [n for n in _ARRAYS if n not in z.files]
    if missing:
        raise ValueError("shape predictor .npz %s: no array %r" % (path, missing[0]))
    return ShapePredictorModel(*[z[n] for n in _ARRAYS])


# ---- the reader ------------------------------------------------------------------------------------------------------------------------
class _SpIn(_In):
    def __init__(self, buf):
        super(_SpIn, self).__init__(buf)
        self.a = np.frombuffer(self.b, dtype=np.uint8)
        self.addr = self.a.ctypes.data
        self.decode = _lib.lib().cis_dlib_decode_reals

    def reals(self, n):
        """n serialised floats in one call of the library's host decoder"""
        out = np.empty(n, dtype=np.float32)
        if n == 0:
            return out
        pos = ctypes.c_size_t(self.p)
        rc = self.decode(self.addr, self.a.size, ctypes.byref(pos), out.ctypes.data, n)
        self.p = int(pos.value)
        if rc != _lib.CIS_OK:
            self.fail(_lib.last_error().split(": ", 1)[-1])
        return out

    def size(self, what, limit):
        v = self.int()
        if v < 0 or v > limit:
            self.fail("%s of size %d (at most %d expected)" % (what, v, limit))
        return v

    def column(self, what, rows=None):
        """matrix<float,0,1>: nr, nc (both negated in the newer encoding), then the elements"""
        nr, nc = self.int(), self.int()
        if nr < 0 or nc < 0:
            nr, nc = -nr, -nc
        if nc != 1 or nr < 0 or (rows is not None and nr != rows) or nr > (1 << 24):
            self.fail("%s: a %d x %d matrix where %s x 1 is expected" % (what, nr, nc, "%d" % rows if rows is not None else "n"))
        return self.reals(nr)


def sp_from_dat(path_or_bytes):
    """ShapePredictorModel from dlib's serialised shape_predictor (see the module docstring: unpinned)."""
    buf = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else open(path_or_bytes, "rb").read()
    s = _SpIn(buf)
    s.expect_version("shape_predictor", (1,))
    initial = s.column("initial_shape")
    if initial.size < 2 or initial.size % 2:
        s.fail("initial_shape with %d elements: not a list of (x, y)" % initial.size)
    if initial.size > MAX_COORDS:
        s.fail("initial_shape with 2P = %d coordinates, the kernel's limit is %d" % (initial.size, MAX_COORDS))
    C = initial.size
    K = s.size("forests", 1 << 16)
    if K < 1:
        s.fail("no cascade level")
    T = S = None
    idx, thresh, leaves = [], [], []
    for k in range(K):
        t_k = s.size("forests[%d]" % k, MAX_T)
        if T is None:
            T = t_k
        if t_k != T or T < 1:
            s.fail("level %d has %d trees, level 0 has %d" % (k, t_k, T))
        for t in range(T):
            n_split = s.size("splits of tree [%d][%d]" % (k, t), (1 << MAX_DEPTH) - 1)
            if S is None:
                S = n_split
                if S < 1 or (S + 1) & S:
                    s.fail("tree [0][0] has %d splits: not a power of two minus one" % S)
                if K * T * (8 * S + 4 * (S + 1) * C) > len(s.b):   # a split is at least 8 bytes, a float at least 4
                    s.fail("%d levels of %d trees of %d splits and %d x %d leaf values: more than a stream of %d bytes can hold"
                           % (K, T, S, S + 1, C, len(s.b)))
                idx = np.empty((K, T, S, 2), dtype=np.int64)
                thresh = np.empty((K, T, S), dtype=np.float32)
                leaves = np.empty((K, T, S + 1, C), dtype=np.float32)
            if n_split != S:
                s.fail("tree [%d][%d] has %d splits, tree [0][0] has %d" % (k, t, n_split, S))
            for i in range(S):
                idx[k, t, i, 0], idx[k, t, i, 1] = s.size("split index", 1 << 31), s.size("split index", 1 << 31)
                thresh[k, t, i] = s.reals(1)[0]
            if s.size("leaf_values of tree [%d][%d]" % (k, t), 1 << MAX_DEPTH) != S + 1:
                s.fail("tree [%d][%d] with %d splits does not have %d leaves" % (k, t, S, S + 1))
            for i in range(S + 1):
                leaves[k, t, i] = s.column("leaf [%d][%d][%d]" % (k, t, i), C)
    if s.size("anchor_idx", 1 << 16) != K:
        s.fail("anchor_idx does not have one list per cascade level (%d)" % K)
    F = None
    anchor = None
    for k in range(K):
        f_k = s.size("anchor_idx[%d]" % k, MAX_F)
        if F is None:
            F = f_k
            anchor = np.empty((K, F), dtype=np.int64)
        if f_k != F or F < 1:
            s.fail("level %d has %d feature pixels, level 0 has %d" % (k, f_k, F))
        for i in range(F):
            anchor[k, i] = s.size("anchor index", 1 << 31)
            if anchor[k, i] >= C // 2:
                s.fail("anchor_idx[%d][%d] = %d is not a landmark (P = %d)" % (k, i, anchor[k, i], C // 2))
    if s.size("deltas", 1 << 16) != K:
        s.fail("deltas does not have one list per cascade level (%d)" % K)
    deltas = np.empty((K, F, 2), dtype=np.float32)
    for k in range(K):
        if s.size("deltas[%d]" % k, MAX_F) != F:
            s.fail("deltas[%d] does not have one entry per feature pixel (%d)" % (k, F))
        deltas[k] = s.reals(2 * F).reshape(F, 2)
    if s.p != len(s.b):
        s.fail("%d bytes behind the shape predictor" % (len(s.b) - s.p))
    bad = np.argwhere((idx < 0) | (idx >= F))
    if len(bad):
        k, t, i, j = bad[0]
        raise ValueError("dlib .dat stream: split_idx[%d][%d][%d][%d] = %d is not a feature (F = %d)" % (k, t, i, j, idx[k, t, i, j], F))
    return ShapePredictorModel(initial, idx, thresh, leaves, anchor, deltas)


# ---- the writer: the same statement of the format run backwards (tests; documents the expected file) -----------------------------------
def _encode_reals(x):
    """(bytes, end offsets [n]) of float32 values in dlib's float serialisation: float_details = (frexp mantissa * 2**24, exponent - 24)
    with the mantissa's zero low bytes shifted off, each integer as control byte + little-endian magnitude (what _Out.real(v, 24) writes)"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    n = x.size
    fin = np.isfinite(x)
    m, e = np.frexp(np.where(fin, x, 0).astype(np.float64))
    mant = (m * float(1 << 24)).astype(np.int64)
    exp = e.astype(np.int64) - 24
    for _ in range(3):
        sh = ((mant & 0xFF) == 0) & (mant != 0)
        mant = np.where(sh, mant >> 8, mant)
        exp = np.where(sh, exp + 8, exp)
    mant = np.where(fin, mant, 0)
    exp = np.where(fin, exp, np.where(np.isnan(x), 32002, np.where(x > 0, 32000, 32001)))
    cols = np.zeros((n, 8), dtype=np.uint8)   # c, m0, m1, m2, m3 | c, e0, e1
    keep = np.zeros((n, 8), dtype=bool)
    for v, base, width in ((mant, 0, 4), (exp, 5, 2)):
        mag = np.abs(v)
        nb = np.ones(n, dtype=np.int64)
        for b in range(1, width):
            nb[mag >= (1 << (8 * b))] = b + 1
        cols[:, base] = nb | np.where(v < 0, 0x80, 0)
        keep[:, base] = True
        for b in range(width):
            cols[:, base + 1 + b] = (mag >> (8 * b)) & 0xFF
            keep[:, base + 1 + b] = nb > b
    return cols[keep].tobytes(), np.cumsum(keep.sum(axis=1))


def write_sp_dat(model, path=None, negate_dims=True):
    """The stream sp_from_dat reads.  negate_dims: the newer matrix encoding (both dimensions written negated) or the older one."""
    sign = -1 if negate_dims else 1
    o = _Out()
    C = 2 * model.P

    def column(data):
        o.int(sign * C); o.int(sign * 1); o.parts.append(data)

    o.int(1)
    column(_encode_reals(model.initial_shape)[0])
    o.int(model.K)
    for k in range(model.K):
        o.int(model.T)
        lb, lend = _encode_reals(model.leaves[k])
        lend = np.concatenate([[0], lend[C - 1::C]])      # byte offset of every leaf of the level
        tb, tend = _encode_reals(model.split_thresh[k])
        tend = np.concatenate([[0], tend])
        for t in range(model.T):
            o.int(model.S)
            for i in range(model.S):
                o.int(model.split_idx[k, t, i, 0]); o.int(model.split_idx[k, t, i, 1])
                j = t * model.S + i
                o.parts.append(tb[tend[j]:tend[j + 1]])
            o.int(model.S + 1)
            for i in range(model.S + 1):
                j = t * (model.S + 1) + i
                column(lb[lend[j]:lend[j + 1]])
    o.int(model.K)
    for k in range(model.K):
        o.int(model.F)
        for i in range(model.F):
            o.int(model.anchor_idx[k, i])
    o.int(model.K)
    for k in range(model.K):
        o.int(model.F)
        o.parts.append(_encode_reals(model.deltas[k])[0])
    data = b"".join(o.parts)
    if path is not None:
        with open(path, "wb") as f:
            f.write(data)
    return data


def load_shape_predictor(path):
    """pred_path of the featurizer's configuration: dlib's .dat or an .npz of the six arrays"""
    path = str(path)
    if path.endswith(".npz"):
        return sp_from_npz(path)
    if path.endswith(".dat"):
        return sp_from_dat(path)
    raise NotImplementedError("pred_path must be dlib's shape predictor .dat or an .npz with the arrays %s" % ", ".join(_ARRAYS))


# ---- the predictor on the GPU ----------------------------------------------------------------------------------------------------------
class ShapePredictorHIP(object):
    """dlib.shape_predictor on the MI355X (csrc/shape_predictor.hip): all rectangles of an image in one launch."""

    def __init__(self, model):
        self.P = model.P
        out = _lib.c_void_p()
        _lib.check(_lib.lib().cis_shapepred_create(_lib.ctypes.byref(out), model.P, model.K, model.T, model.depth, model.F,
                                                   _lib.ptr(model.initial_shape), _lib.ptr(model.split_idx), _lib.ptr(model.split_thresh),
                                                   _lib.ptr(model.leaves), _lib.ptr(model.anchor_idx), _lib.ptr(model.deltas)))
        self._h = out.value

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().cis_shapepred_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def predict_dev(self, img, rects, shape_out=None):
        """img: contiguous uint8 CUDA tensor [H, W, 3] RGB, rects: int32 CUDA tensor [n, 4] (left, top, right, bottom) -> int32 CUDA
        tensor [n, P, 2] (x, y); asynchronous, on the current torch stream.  shape_out: optional float32 CUDA tensor [n, 2P] for the
        normalised shapes."""
        import torch
        if self._h is None:
            raise ValueError("the shape predictor is closed")
        if not (img.is_cuda and img.is_contiguous() and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3):
            raise ValueError("img must be a contiguous uint8 [H, W, 3] tensor on the GPU")
        if not (rects.is_cuda and rects.is_contiguous() and rects.dtype == torch.int32 and rects.dim() == 2 and rects.shape[1] == 4
                and rects.device == img.device):
            raise ValueError("rects must be a contiguous int32 [n, 4] tensor on the image's GPU")
        n = int(rects.shape[0])
        if shape_out is not None and not (shape_out.is_cuda and shape_out.is_contiguous() and shape_out.dtype == torch.float32
                                          and tuple(shape_out.shape) == (n, 2 * self.P) and shape_out.device == img.device):
            raise ValueError("shape_out must be a contiguous float32 [n, 2P] tensor on the image's GPU")
        parts = torch.empty((n, self.P, 2), dtype=torch.int32, device=img.device)
        _lib.check(_lib.lib().cis_shapepred_run_dev(self._h, img.data_ptr(), int(img.shape[0]), int(img.shape[1]), rects.data_ptr(), n,
                                                    parts.data_ptr(), None if shape_out is None else shape_out.data_ptr(),
                                                    torch.cuda.current_stream(img.device).cuda_stream))
        return parts

    def predict(self, img, rects):
        """img [H, W, 3] uint8 RGB (numpy or tensor), rects [n, 4] integers -> np.int64 [n, P, 2]"""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        if hasattr(img, "is_cuda"):
            timg = img
        else:
            a = np.ascontiguousarray(img, dtype=np.uint8)
            timg = torch.as_tensor(a if a.flags.writeable else a.copy())
        r = np.ascontiguousarray(np.asarray(rects, dtype=np.int64).reshape(-1, 4))
        if len(r) and (np.abs(r) > np.iinfo(np.int32).max).any():
            raise ValueError("rectangle coordinates beyond int32")
        trects = torch.as_tensor(r.astype(np.int32))
        return self.predict_dev(timg.to(dev).contiguous(), trects.to(dev)).cpu().numpy().astype(np.int64)
