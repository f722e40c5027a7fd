"""Probe networks for csrc/cnn.hip: weights for which the exact value of every output feature is known.  numpy only.

cnn.hip has no per-layer entry point, so the weights are the instrument.  A probe network has SPARSE rows: every output
channel of every convolution (and every row of the fully connected layers) has one non-zero weight (family A, "selector")
or three of them (family B, "lattice", dlib only; four in its fc).  All non-zero weights are +-1 (conv1 of DeepSentibank:
+-1/2, +-1/4; its later layers 1/2, 1, 2): with 24 bits to spend on 29 convolutions, four average pools and the global
average, larger integers in family B did not pass lattice_guard.  A wrong weight SCALE therefore shows only through gamma
(1/2 on a quarter of conv0's channels) and DeepSentibank's powers of two.  Every pre-activation is then a sum of a few
products and many exact zeros; with inputs on a binary lattice every partial sum is a multiple of one step 2^-s below
2^(24-s), i.e. exact in float32 IN ANY ORDER -- whichever tile shape, K split, tap order or fused kernel computes it.  A
whole forward can be compared for equality, on every route.

The reference is not a convolution: a layer is evaluated from its index maps (ky, kx, ic per output channel) by numpy
fancy indexing into the zero-padded input, in float64; pools, residual adds and the LRN are slices.  With cover=dict a
forward walks the same maps backwards from the output features (Sparse.back, max_pool_back, _note) and marks what a wrong
value WOULD change: a position counts only if the value that flows through it is non-zero, a max pool passes the mask to
its arg max only.  Weight sets are built one after the other, each one aiming its observed channels at the taps no earlier
set has observed.  The union is NOT everything: the negative beta that keeps dlib's magnitudes inside the lattice clamps
three quarters of every branch to 0, and a clamped path observes nothing.  What the union does cover is asserted by
tests/test_cnn_probe_nets.py::test_union_of_the_weight_sets_observes_the_edges_and_a_floor_of_taps.

dlib inputs (lattice).  The first kernel computes (x - mean_c) * 2^-8 in float32.  x = float32(mean_c) + k with an integer
k in [-12, 3] is exactly representable (x < 128: the spacing of float32 there is that of mean_c or finer), the difference
is exactly k, and the normalised input is t = k * 2^-8.  These 16 levels are coarser than the 2^-12 a chip could carry, so
a dropped bit below 2^-8 of the first layer's input cannot show.  `lattice_guard` asserts, from the float64 reference,
for every layer: all terms are multiples of one step and the sum of their magnitudes stays below 2^24 steps; and a
float32 accumulation in ascending and in descending k gives the bits of the float64 value.  If it fails the inputs /
weights are wrong and must change -- the assertion is not to be loosened.

DeepSentibank.  k_maxpool_lrn_nhwc_v4 computes  a * rsqrtf(b) * rsqrtf(sqrtf(b)),  b = 1 + (alpha / 5) * s,
s = fmaf chain of the (at most) five squares.  Equality ends at norm1; from conv2 on every observed value is a
non-negative number times powers of two with zero biases, so nothing cancels, max and ReLU are 1-Lipschitz, and a relative
error passes unchanged to fc7.  With u = 2^-24 (half an ulp, relative; an error of E ulp is at most 2 E u):
    s       five fmaf roundings of a positive sum                                  5 u
    alpha/5 float32(1e-4) and the float32 division                                 2 u
    p       = fl(alpha/5 * s)                                                      5 + 2 + 1 = 8 u
    b       = fl(1 + p): 8 u * p / b + one rounding                                <= 9 u
    b^-3/4  sensitivity 3/4                                                        6.75 u
    sqrtf   E_s ulp = 2 E_s u, halved by the rsqrt behind it                       E_s u
    rsqrtf  two of them, E_r ulp each                                              4 E_r u
    the product of the two rsqrtf, the product with a                              2 u
    one stage                                                                      e1 = (8.75 + E_s + 4 E_r) u
No ulp bound for sqrtf / rsqrtf was found in the local ROCm install (searched for "ulp" in share/doc and in the HIP headers
include/hip/amd_detail, where the device math functions are declared: no match), so E_s = E_r = 2 (the fallback): e1 = 18.75 u.
The second stage receives values with relative errors |d_i| <= e1: its own centre passes d_c on, the squares in b carry
2 d_i, weighted kq a_i^2 / b which sum to p / b, times 3/4: at most e1 * (1 + 1.5 p / b).  The builder asserts p <= P_MAX = 1
at both LRN inputs (from the reference, not from the kernel), so p / b <= 1/2:
    c = e1 * (1 + 1.75) + 0.25 (second-order terms, generously) = 51.8125  <= 64.
The bound is |got - ref64| <= c * 2^-24 * |ref64| element by element, and an exact 0 where the reference is 0.
"""
import functools

import numpy as np

F24 = float(1 << 24)
U = 2.0 ** -24
E_SQRT_ULP, E_RSQRT_ULP = 2.0, 2.0          # fallback: no documented bound found locally
LRN_STAGE_U = 8.75 + E_SQRT_ULP + 4.0 * E_RSQRT_ULP
P_MAX = 1.0
SENTIBANK_C = LRN_STAGE_U * (1.0 + 1.0 + 1.5 * P_MAX / (1.0 + P_MAX)) + 0.25
LRN_ALPHA, LRN_SIZE, LRN_BETA = 1e-4, 5, 0.75

DLIB_MEAN = np.array([122.782, 117.001, 104.298], dtype=np.float32)
DLIB_PLAN = [(32, 32, 0), (32, 32, 0), (32, 32, 0), (32, 64, 1), (64, 64, 0), (64, 64, 0), (64, 64, 0), (64, 128, 1),
             (128, 128, 0), (128, 128, 0), (128, 256, 1), (256, 256, 0), (256, 256, 0), (256, 256, 1)]
SB_CONVS = [("conv1", 3, 96, 11, 4, 0, 1), ("conv2", 96, 256, 5, 1, 2, 2), ("conv3", 256, 384, 3, 1, 1, 1),
            ("conv4", 384, 384, 3, 1, 1, 2), ("conv5", 384, 256, 3, 1, 1, 2), ("fc6", 256, 4096, 6, 1, 0, 1),
            ("fc7", 4096, 4096, 1, 1, 0, 1)]   # fc6 = a 6 x 6 convolution on pool5: OIHW flattened is caffe's CHW order


# ---------------------------------------------------------------------------------------------------------------------
# sparse layers
# ---------------------------------------------------------------------------------------------------------------------
class Sparse(object):
    """A convolution whose output channel oc has nz taps (ky, kx, ic)[oc][j] with weight w[oc][j] (0 = unused slot), a bias,
    and (dlib) the affine gamma / beta behind it.  ic is the ABSOLUTE input channel (group offset included)."""

    def __init__(self, name, cin, cout, k, stride, pad, groups=1, nz=1):
        self.name, self.cin, self.cout, self.k, self.stride, self.pad, self.groups, self.nz = name, cin, cout, k, stride, pad, groups, nz
        self.ky = np.zeros((cout, nz), dtype=np.int64)
        self.kx = np.zeros((cout, nz), dtype=np.int64)
        self.ic = np.zeros((cout, nz), dtype=np.int64)
        self.w = np.zeros((cout, nz))
        self.bias = np.zeros(cout)
        self.gamma = np.ones(cout)
        self.beta = np.zeros(cout)

    @property
    def icg(self):
        return self.cin // self.groups

    def group_of(self, oc):
        return oc // (self.cout // self.groups)

    def flat_tap(self):
        """tap number inside the group, (ky * k + kx) * icg + ic_local: the K index of the packed weights"""
        icl = self.ic - (self.group_of(np.arange(self.cout)) * self.icg)[:, None]
        return (self.ky * self.k + self.kx) * self.icg + icl

    def dense(self):
        """OIHW float32 (input channels local to the group), as caffe / dlib store it"""
        W = np.zeros((self.cout, self.icg, self.k, self.k), dtype=np.float32)
        icl = self.ic - (self.group_of(np.arange(self.cout)) * self.icg)[:, None]
        for j in range(self.nz):
            used = self.w[:, j] != 0
            assert (W[np.arange(self.cout)[used], icl[used, j], self.ky[used, j], self.kx[used, j]] == 0).all(), "a tap twice in one row"
            W[np.arange(self.cout)[used], icl[used, j], self.ky[used, j], self.kx[used, j]] = self.w[used, j]
        assert (W.astype(np.float64) != 0).sum() == (self.w != 0).sum()
        return W

    def out_hw(self, h):
        return (h + 2 * self.pad - self.k) // self.stride + 1

    def index(self, oh, ow, j):
        s = self.stride
        Y = (np.arange(oh) * s)[:, None, None] + self.ky[None, None, :, j]
        X = (np.arange(ow) * s)[None, :, None] + self.kx[None, None, :, j]
        return Y, X, np.broadcast_to(self.ic[None, None, :, j], Y.shape[:1] + X.shape[1:2] + (self.cout,))

    def terms(self, x):
        """x [n, h, w, cin] float64 -> ([nz arrays [n, oh, ow, cout]], const [cout]): the products (gamma folded in, as
        pack_conv_affine does) and gamma * bias + beta.  Indexing, not a convolution."""
        n, h, w, c = x.shape
        assert c == self.cin
        p = self.pad
        xp = np.zeros((n, h + 2 * p, w + 2 * p, c))
        xp[:, p:p + h, p:p + w] = x
        oh, ow = self.out_hw(h), self.out_hw(w)
        out = []
        for j in range(self.nz):
            Y, X, C = self.index(oh, ow, j)
            out.append(xp[:, Y, X, C] * (self.gamma * self.w[:, j]))
        return out, self.gamma * self.bias + self.beta

    def back(self, obs_out, terms, in_shape, cover):
        """mask of the input positions whose value reaches an observed output through a non-zero product"""
        n, h, w, c = in_shape
        p, s = self.pad, self.stride
        obs = np.zeros((n, h + 2 * p, w + 2 * p, c), dtype=bool)
        tap = cover.setdefault(("tap", self.name), np.zeros((self.k, self.k, self.cin), dtype=bool))
        for j in range(self.nz):
            m = obs_out & (terms[j] != 0)
            ni, oy, ox, oc = np.nonzero(m)
            obs[ni, oy * s + self.ky[oc, j], ox * s + self.kx[oc, j], self.ic[oc, j]] = True
            hit = m.any(axis=(0, 1, 2))
            tap[self.ky[hit, j], self.kx[hit, j], self.ic[hit, j]] = True
        return obs[:, p:p + h, p:p + w]


def _note(cover, name, obs, val):
    """record which channels and which positions of blob `name` are observed with a non-zero value"""
    m = obs & (val != 0)
    ch = cover.setdefault(("chan", name), np.zeros(val.shape[3], dtype=bool))
    ch |= m.any(axis=(0, 1, 2))
    pos = cover.setdefault(("pos", name), np.zeros(val.shape[1:3], dtype=bool))
    pos |= m.any(axis=(0, 3))
    return m


def max_pool(x, oh, ow):
    """3 x 3 / 2, windows clipped to the input (caffe's ceil mode and dlib's floor mode differ in oh only) -> (out, [9 slices])"""
    n, h, w, c = x.shape
    xp = np.full((n, 2 * oh + 1, 2 * ow + 1, c), -np.inf)
    xp[:, :min(h, 2 * oh + 1), :min(w, 2 * ow + 1)] = x[:, :2 * oh + 1, :2 * ow + 1]
    sl = [xp[:, dy:dy + 2 * oh:2, dx:dx + 2 * ow:2] for dy in range(3) for dx in range(3)]
    return np.maximum.reduce(sl), sl


def max_pool_back(obs_out, out, sl, in_shape):
    n, h, w, c = in_shape
    oh, ow = out.shape[1:3]
    obs = np.zeros((n, 2 * oh + 1, 2 * ow + 1, c), dtype=bool)
    done = np.zeros(out.shape, dtype=bool)
    for i, s in enumerate(sl):
        dy, dx = divmod(i, 3)
        hit = (s == out) & ~done
        done |= hit
        obs[:, dy:dy + 2 * oh:2, dx:dx + 2 * ow:2] |= hit & obs_out
    full = np.zeros(in_shape, dtype=bool)
    full[:, :min(h, 2 * oh + 1), :min(w, 2 * ow + 1)] = obs[:, :h, :w]
    return full


def avg_pool2(x):
    n, h, w, c = x.shape
    oh, ow = h // 2, w // 2
    parts = [x[:, dy:2 * oh:2, dx:2 * ow:2] for dy in range(2) for dx in range(2)]
    return ((parts[0] + parts[1]) + (parts[2] + parts[3])) * 0.25, parts


def lrn(x):
    c = x.shape[3]
    sq = np.zeros(x.shape[:3] + (c + 4,))
    sq[..., 2:c + 2] = x * x
    s = sum(sq[..., d:d + c] for d in range(5))
    p = (LRN_ALPHA / LRN_SIZE) * s
    return x / np.power(1.0 + p, LRN_BETA), p


def pad_to(x, h, w, c):
    out = np.zeros((x.shape[0], h, w, c), dtype=x.dtype)
    out[:, :x.shape[1], :x.shape[2], :x.shape[3]] = x
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the lattice guard
# ---------------------------------------------------------------------------------------------------------------------
def low_bit(v):
    """exponent of the lowest set bit of every non-zero float64 in v, minimum over v (None if all zero)"""
    v = np.asarray(v, dtype=np.float64).ravel()
    v = v[v != 0]
    if v.size == 0:
        return None
    m, e = np.frexp(np.abs(v))
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return int((e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)).min())


def lattice_guard(what, terms):
    """terms: arrays of one shape (or broadcastable) that a kernel adds up in float32 in some order.  All of them multiples of
    one step 2^s, the sum of their magnitudes below 2^24 steps => every partial sum in every order is exact.  And the float32
    sums in ascending and descending order have the bits of the float64 sum."""
    lows = [b for b in (low_bit(t) for t in terms) if b is not None]
    total64 = sum(terms)
    if not lows:
        return total64
    step = 2.0 ** min(lows)
    mag = sum(np.abs(t) for t in terms)
    assert float(np.max(mag)) < F24 * step, "%s: partial sums need %.1f bits (> 24): change the inputs, not this line" % (
        what, np.log2(float(np.max(mag)) / step))
    shape = np.broadcast(*terms).shape
    up, down = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    for t in terms:
        assert (np.float32(t).astype(np.float64) == t).all(), what
        up = up + np.float32(t)
    for t in terms[::-1]:
        down = down + np.float32(t)
    assert up.dtype == np.float32 and (up.view(np.uint32) == down.view(np.uint32)).all() and (up.astype(np.float64) == total64).all(), what
    return total64


# ---------------------------------------------------------------------------------------------------------------------
# tap assignment: observed channels take the taps nobody has observed yet
# ---------------------------------------------------------------------------------------------------------------------
def assign_taps(L, rs, observed, covered, valid=None):
    """fill L.ky / kx / ic: the observed output channels of every group walk through the group's uncovered taps (seeded
    order), everything else gets seeded taps.  `covered` [k][k][cin] is the union of the earlier sets' observation; `valid`
    masks taps that can ever meet data.  Returns the mask of input channels the observed rows point at."""
    k, icg, ocg = L.k, L.icg, L.cout // L.groups
    picked = np.zeros(L.cin, dtype=bool)
    for g in range(L.groups):
        taps = [(ky, kx, g * icg + ic) for ky in range(k) for kx in range(k) for ic in range(icg)
                if valid is None or valid[ky, kx]]
        order = rs.permutation(len(taps))
        todo = [taps[i] for i in order if not covered[taps[i]]]
        rest = [taps[i] for i in order if covered[taps[i]]]
        queue = todo + rest
        pos = 0
        ocs = np.arange(g * ocg, (g + 1) * ocg)
        for oc in list(ocs[observed[ocs]]) + list(ocs[~observed[ocs]]):
            row = sorted(queue[(pos + j) % len(queue)] for j in range(L.nz))
            assert len(set(row)) == L.nz
            pos += L.nz
            row.sort(key=lambda t: (t[0] * k + t[1]) * icg + t[2])   # ascending k: slot order = the kernels' K order
            for j, (ky, kx, ic) in enumerate(row):
                L.ky[oc, j], L.kx[oc, j], L.ic[oc, j] = ky, kx, ic
                if observed[oc]:
                    picked[ic] = True
    return picked


# ---------------------------------------------------------------------------------------------------------------------
# dlib
# ---------------------------------------------------------------------------------------------------------------------
def dlib_lattice_k(n, seed):
    """integer k [n,150,150,3] in [-12, 3]: a smooth ramp (direction and slope per chip) plus a seeded pattern, so that
    neighbouring pixels differ and a shift by one pixel changes the result"""
    rs = np.random.RandomState(1000 + seed)
    y, x = np.mgrid[0:150, 0:150]
    out = np.empty((n, 150, 150, 3), dtype=np.int64)
    for i in range(n):
        a, b = [(1, 1), (-1, 1), (1, -1), (-1, -1), (1, 0), (0, -1), (2, 1)][i % 7]
        ramp = (a * x + b * y) * 30.0 / 300.0
        ramp = ramp - ramp.min()          # 0 .. <= 30
        for c in range(3):
            out[i, :, :, c] = np.clip(np.floor(ramp / 3.0).astype(np.int64) - 12 + c + rs.randint(0, 5, size=(150, 150)), -12, 3)
    return out


def dlib_chips_from_k(k):
    """float32 chips x = float32(mean_c) + k; asserts that the kernel's float32 (x - mean) * 2^-8 is exactly k * 2^-8"""
    x = (DLIB_MEAN[None, None, None, :].astype(np.float64) + k).astype(np.float32)
    assert (x.astype(np.float64) == DLIB_MEAN.astype(np.float64) + k).all() and (x < 128).all()
    t = (x - DLIB_MEAN) * np.float32(1.0 / 256.0)
    assert t.dtype == np.float32 and (t.astype(np.float64) == k / 256.0).all()
    return x


class DlibProbe(object):
    """one weight set: .layers (conv0, b0a, b0b, ..., fc), .weights() for DLibFaceNet, .forward(k) float64 reference"""

    def __init__(self, family, seed, covered):
        self.family, self.seed = family, seed
        nz = 1 if family == "A" else 3
        rs = np.random.RandomState(77 * seed + (0 if family == "A" else 5000))
        self.conv0 = Sparse("conv0", 3, 32, 7, 2, 0, nz=nz)
        self.blocks = []
        for i, (cin, cout, down) in enumerate(DLIB_PLAN):
            a = Sparse("b%da" % i, cin, cout, 3, 2 if down else 1, 0 if down else 1, nz=nz)
            b = Sparse("b%db" % i, cout, cout, 3, 1, 1, nz=nz)
            self.blocks.append((a, b))
        self.fc = Sparse("fc", 256, 128, 1, 1, 0, nz=1 if family == "A" else 4)
        cov = lambda L: covered.setdefault(("tap", L.name), np.zeros((L.k, L.k, L.cin), dtype=bool))
        # taps, top down: what the layer above observes decides which rows matter below
        obs = assign_taps(self.fc, rs, np.ones(128, dtype=bool), cov(self.fc))
        centre = np.zeros((3, 3), dtype=bool)
        centre[1, 1] = True
        for i in range(13, -1, -1):
            a, b = self.blocks[i]
            cin = DLIB_PLAN[i][0]
            # the last block's second convolution works on a 1 x 1 map: only its centre tap ever meets data
            pa = assign_taps(b, rs, obs[:b.cout], cov(b), valid=centre if i == 13 else None)
            px = assign_taps(a, rs, pa, cov(a))
            obs = obs[:cin] | px
        assign_taps(self.conv0, rs, obs, cov(self.conv0))
        # Values.  Every doubling of a magnitude and every halving of a step costs one of float32's 24 bits, and the four
        # 2 x 2 average pools and the global average take ten.  So all magnitudes are 1, gamma = 1/2 appears in conv0 only,
        # and a block's first affine gets a negative beta (set by forward(tune=True) from the reference values) that lets
        # only the top quarter of its channel through: the branch is sparse and small, relu(skip + branch) grows slowly,
        # nothing dies, and the ReLU clamps three quarters of the branch to an exact 0.
        for L in self.layers():
            n, nz = L.cout, L.nz
            if L is self.conv0:       # lattice inputs of both signs, mostly negative
                w = np.where(rs.rand(n, nz) < 0.7, -1.0, 1.0)
            elif L is self.fc:
                w = np.where(rs.rand(n, nz) < 0.5, -1.0, 1.0)
            else:                     # inputs >= 0: one positive slot (family B: the other slots negative), a few rows all negative
                w = -np.ones((n, nz))
                keep = rs.rand(n) < (0.8 if L.name.endswith("b") else 0.95)
                w[np.arange(n)[keep], rs.randint(0, nz, size=n)[keep]] *= -1.0
            L.w[:] = w
            if L is not self.fc:
                L.bias[:] = rs.randint(-1, 2, size=n) * 2.0 ** -6
                L.beta[:] = rs.randint(-1, 1 if L.name.endswith("b") else 2, size=n) * 2.0 ** -6
            if L is self.conv0:
                L.gamma[:] = np.where(rs.rand(n) < 0.25, 0.5, 1.0)   # powers of two <= 1: folded into the weights exactly
        self.tuned = False

    def layers(self):
        return [self.conv0] + [l for ab in self.blocks for l in ab] + [self.fc]

    def weights(self):
        w = {"conv0_w": self.conv0.dense(), "conv0_b": self.conv0.bias.astype(np.float32),
             "aff0_g": self.conv0.gamma.astype(np.float32), "aff0_b": self.conv0.beta.astype(np.float32)}
        for i, (a, b) in enumerate(self.blocks):
            for h, L in (("a", a), ("b", b)):
                w["b%d%s_w" % (i, h)] = L.dense()
                w["b%d%s_b" % (i, h)] = L.bias.astype(np.float32)
                w["b%d%s_g" % (i, h)] = L.gamma.astype(np.float32)
                w["b%d%s_beta" % (i, h)] = L.beta.astype(np.float32)
        w["fc_w"] = self.fc.dense().reshape(128, 256)
        return w

    def forward(self, k, guard=False, cover=None, tune=False):
        """k: integer lattice input [n,150,150,3] -> features [n,128] float64 (exact).  guard: lattice_guard on every sum a
        kernel forms.  cover: dict that receives the observation masks of this forward (see observe)."""
        G = (lambda what, ts: lattice_guard(what, ts)) if guard else (lambda what, ts: sum(ts))
        tape = []
        t = k / 256.0
        ts, c = self.conv0.terms(t)
        pre = G("conv0", ts + [c])
        a0 = np.maximum(pre, 0.0)
        x, sl = max_pool(a0, 35, 35)
        tape.append(("conv0", t.shape, ts, a0, sl, x))
        for i, (a, b) in enumerate(self.blocks):
            cin, cout, down = DLIB_PLAN[i]
            ta, ca = a.terms(x)
            if tune:   # beta = -(3/4 or 7/8 of the channel's largest pre-activation), a multiple of the input lattice 2^-8
                top = (sum(ta) + ca).max(axis=(0, 1, 2))
                q = np.where(np.arange(cout) % 2 == 0, 0.75, 0.875)
                a.beta[:] = np.where(top > 2.0 ** -6, a.beta - np.floor(q * top * 256.0) / 256.0, a.beta)
                ta, ca = a.terms(x)
            ya = np.maximum(G(a.name, ta + [ca]), 0.0)
            tb, cb = b.terms(ya)
            if down:
                skip, parts = avg_pool2(x)
                if guard:
                    lattice_guard("avg_pool of block %d" % i, parts)
            else:
                skip, parts = x, None
            oh, ow, oc = max(ya.shape[1], skip.shape[1]), max(ya.shape[2], skip.shape[2]), max(cout, cin)
            # the fused epilogues add bias and residual to the finished sum; k_add_relu_pad adds the two finished branches
            z = G(b.name, [pad_to(v, oh, ow, oc) for v in tb] + [pad_to(np.broadcast_to(cb, tb[0].shape), oh, ow, oc), pad_to(skip, oh, ow, oc)])
            xn = np.maximum(z, 0.0)
            tape.append((i, x.shape, ta, ya, tb, skip, parts, xn))
            x = xn
        hw = [x[:, py, px] for py in range(2) for px in range(2)]
        g = G("global average", hw) / 4.0
        tf, _ = self.fc.terms(g[:, None, None, :])
        f = G("fc", tf)[:, 0, 0, :]
        if cover is not None:
            self._observe(cover, tape, x, g, tf, f)
        return f

    def _observe(self, cover, tape, x, g, tf, f):
        obs = np.ones(f.shape, dtype=bool)[:, None, None, :]
        _note(cover, "fc", obs, f[:, None, None, :])
        og = self.fc.back(obs, tf, (g.shape[0], 1, 1, 256), cover)
        obs_x = np.broadcast_to(og, x.shape) & (x != 0)
        for i in range(13, -1, -1):
            _, in_shape, ta, ya, tb, skip, parts, xn = tape[1 + i]
            cin, cout, down = DLIB_PLAN[i]
            a, b = self.blocks[i]
            m = _note(cover, "x%d" % (i + 1), obs_x, xn)
            pad = cover.setdefault(("padchan", i), np.zeros(xn.shape[3], dtype=bool))
            pad |= m.any(axis=(0, 1, 2))
            ob = m[:, :ya.shape[1], :ya.shape[2], :cout]
            _note(cover, b.name, ob, sum(tb))
            oa = b.back(ob, tb, ya.shape, cover)
            _note(cover, a.name, oa, ya)
            ox = a.back(oa & (ya != 0), ta, in_shape, cover)
            os_ = m[:, :skip.shape[1], :skip.shape[2], :cin] & (skip != 0)
            if down:
                full = np.zeros(in_shape, dtype=bool)
                for j, pp in enumerate(parts):
                    dy, dx = divmod(j, 2)
                    full[:, dy:2 * skip.shape[1]:2, dx:2 * skip.shape[2]:2] |= os_ & (pp != 0)
                ap = cover.setdefault(("pos", "avg%d" % i), np.zeros(in_shape[1:3], dtype=bool))
                ap |= full.any(axis=(0, 3))
                os_ = full
            obs_x = ox | os_
        _, t_shape, ts, a0, sl, x0 = tape[0]
        m = _note(cover, "pool0", obs_x, x0)
        o0 = max_pool_back(m, x0, sl, a0.shape)
        _note(cover, "conv0", o0, a0)
        self.conv0.back(o0 & (a0 != 0), ts, t_shape, cover)


DLIB_SETS = [("A", s) for s in range(4)] + [("B", s) for s in range(2)]
DLIB_N = 7   # distinct probe chips


@functools.lru_cache(maxsize=None)
def dlib_probes():
    """[(family, seed, DlibProbe, ref64 [DLIB_N,128])], the union of the observation masks, the chips' lattice input"""
    k = dlib_lattice_k(DLIB_N, 0)
    cover, out = {}, []
    for family, seed in DLIB_SETS:
        p = DlibProbe(family, seed, cover)
        p.forward(k, tune=True)
        ref = p.forward(k, guard=True, cover=cover)
        out.append((family, seed, p, ref))
    return out, cover, k


# ---------------------------------------------------------------------------------------------------------------------
# DeepSentibank (family A)
# ---------------------------------------------------------------------------------------------------------------------
def sentibank_images(n, seed=0):
    """NCHW float32 integers in [-100, 100]: ramps in seeded directions plus a seeded pattern"""
    rs = np.random.RandomState(2000 + seed)
    y, x = np.mgrid[0:227, 0:227]
    out = np.empty((n, 3, 227, 227), dtype=np.float32)
    for i in range(n):
        a, b = [(1, 1), (-1, -1), (1, -1), (-1, 1), (1, 0)][i % 5]
        ramp = (a * x + b * y) * 70.0 / 226.0
        for c in range(3):
            out[i, c] = np.clip(np.floor(ramp * (1 if c != 1 else -1)) + rs.randint(-30, 31, size=(227, 227)), -100, 100)
    return out


class SentibankProbe(object):
    def __init__(self, seed, covered):
        rs = np.random.RandomState(31 * seed + 7)
        self.layers = [Sparse(*cfg) for cfg in SB_CONVS]
        cov = lambda L: covered.setdefault(("tap", L.name), np.zeros((L.k, L.k, L.cin), dtype=bool))
        obs = np.ones(4096, dtype=bool)
        for L in self.layers[::-1]:
            obs = assign_taps(L, rs, obs, cov(L))
        c1 = self.layers[0]
        c1.w[:, 0] = rs.choice([0.5, -0.5, 0.25, -0.25], size=96)     # both signs before anything has been rounded
        c1.bias[:] = rs.randint(-32, 33, size=96) * 0.25
        for L in self.layers[1:]:
            L.w[:, 0] = rs.choice([1.0, 0.5, 2.0] if L.name != "conv2" else [1.0, 0.5], size=L.cout)

    def weights(self):
        w = {}
        for L in self.layers:
            d = L.dense()
            w[L.name + "_w"] = d.reshape(d.shape[0], -1) if L.name.startswith("fc") else d
            w[L.name + "_b"] = L.bias.astype(np.float32)
        return w

    def forward(self, x_nchw, cover=None):
        """[n,3,227,227] -> [n,4096] float64"""
        x = np.transpose(x_nchw.astype(np.float64), (0, 2, 3, 1))
        tape = []
        for L in self.layers:
            ts, c = L.terms(x)
            if L.name == "conv1":
                pre = lattice_guard("conv1", ts + [np.broadcast_to(c, ts[0].shape)])   # exact up to norm1
            else:
                assert (c == 0).all() and (ts[0] >= 0).all(), "from conv2 on: zero biases, nothing negative"
                pre = ts[0]
            y = np.maximum(pre, 0.0)
            rec = [L, x.shape, ts, y, None, None, None]
            if L.name in ("conv1", "conv2", "conv5"):
                oh = -(-(y.shape[1] - 3) // 2) + 1
                pooled, sl = max_pool(y, oh, oh)
                rec[4:6] = [sl, pooled]
                y2 = pooled
                if L.name != "conv5":
                    y2, p = lrn(pooled)
                    assert float(p.max()) <= P_MAX, "LRN input too large for the derivation of SENTIBANK_C"
                    rec[6] = y2
            else:
                y2 = y
            tape.append(rec)
            x = y2
        f = x[:, 0, 0, :]
        if cover is not None:
            obs = np.ones(x.shape, dtype=bool)
            for L, in_shape, ts, y, sl, pooled, normed in tape[::-1]:
                if normed is not None:
                    obs = _note(cover, "norm" + L.name[-1], obs, normed)
                if pooled is not None:
                    obs = _note(cover, "pool" + L.name[-1], obs, pooled)
                    obs = max_pool_back(obs, pooled, sl, y.shape)
                obs = _note(cover, L.name, obs, y)
                obs = L.back(obs, ts, in_shape, cover)
        return f


SENTIBANK_SETS = 3
SENTIBANK_N = 5


@functools.lru_cache(maxsize=None)
def sentibank_probes():
    """[(seed, SentibankProbe, ref64 [5,4096])], union of the observation masks, the images"""
    x = sentibank_images(SENTIBANK_N)
    cover, out = {}, []
    for seed in range(SENTIBANK_SETS):
        p = SentibankProbe(seed, cover)
        out.append((seed, p, p.forward(x, cover=cover)))
    return out, cover, x


# ---------------------------------------------------------------------------------------------------------------------
# float64 copy of oracle/dlib_oracle.forward_torch (dtype argument added here, not in the oracle)
# ---------------------------------------------------------------------------------------------------------------------
def dlib_forward_torch(chips, w, dtype=None):
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    T = lambda k: torch.from_numpy(w[k]).to(dtype)
    x = torch.from_numpy(np.ascontiguousarray(chips)).float().permute(0, 3, 1, 2)
    x = ((x - torch.from_numpy(DLIB_MEAN).view(1, 3, 1, 1)) / 256.0).to(dtype)   # the normalisation is float32 in the kernel
    aff = lambda t, g, b: t * T(g).view(1, -1, 1, 1) + T(b).view(1, -1, 1, 1)
    pad_to_ = lambda t, s: F.pad(t, (0, s[3] - t.shape[3], 0, s[2] - t.shape[2], 0, s[1] - t.shape[1]))
    with torch.no_grad():
        x = F.relu(aff(F.conv2d(x, T("conv0_w"), T("conv0_b"), stride=2, padding=0), "aff0_g", "aff0_b"))
        x = F.max_pool2d(x, 3, 2, padding=0)
        for i, (cin, cout, down) in enumerate(DLIB_PLAN):
            s, p = (2, 0) if down else (1, 1)
            y = F.relu(aff(F.conv2d(x, T("b%da_w" % i), T("b%da_b" % i), stride=s, padding=p), "b%da_g" % i, "b%da_beta" % i))
            y = aff(F.conv2d(y, T("b%db_w" % i), T("b%db_b" % i), stride=1, padding=1), "b%db_g" % i, "b%db_beta" % i)
            skip = F.avg_pool2d(x, 2, 2) if down else x
            shape = [y.shape[0]] + [max(a, b) for a, b in zip(y.shape[1:], skip.shape[1:])]
            x = F.relu(pad_to_(y, shape) + pad_to_(skip, shape))
        x = x.mean(dim=(2, 3))
        return (x @ T("fc_w").t()).numpy()
