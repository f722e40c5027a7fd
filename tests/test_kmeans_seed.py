"""cis_kmeanspp_dev (csrc/kmeans_seed.hip): k-means++ seeding on device data, and the Python layer on it (lopq/train.py).

The semantics are those of include/cis_hip.h: centre 0 is row floor(u[0] * n); d2 is the float32 direct form, min over the chosen
centres; draw j takes the smallest row with d2 > 0 whose inclusive float64 prefix sum exceeds u[j] * tot; tot == 0 falls back to row
floor(u[j] * n).  On INTEGER LATTICES (coordinates in [-8, 8], d <= 129) every d2 is an integer below 2^24 and every sum an integer
below 2^53, so the result is exact in any order and equals an int64 restatement.  On real-valued data the direct float32 form has a
relative error of at most about (d + 2) 2^-24 per row in any order, all terms are non-negative, so every sum inherits it:
eps = (d + 8) 2^-24 leaves a margin of 6 for the float64 sums, and every draw has to be a valid one within eps.
"""
import functools

import numpy as np
import pytest

import test_kmeans_dev as tkd
import test_train_kernels as tk

CIS_EINVAL = -1
TILE, MAX_GRID = 256, 2048  # rows per tile sum (= threads per workgroup) and the bound of k_kpp_update's grid (csrc/kmeans_seed.hip)
ONE_BELOW = np.nextafter(1.0, 0.0)


def _L():
    from columbiaimagesearch_amd import _lib
    return _lib


def _kpp(X, k, u, want_out=True, stream=None, shift_x=0, shift_c=0):
    """cis_kmeanspp_dev on device copies; (centroids, picked or None, potential or None).  picked is pre-filled with -1, the
    centroids and the potential with NaN, so an element nobody wrote shows; d_X must come back byte-equal.  shift_x / shift_c: floats
    by which d_X / d_centroids are moved off their allocation's (16-byte) alignment."""
    import torch
    lib = _L()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, d = X.shape
    Xbuf = torch.zeros(n * d + shift_x, dtype=torch.float32, device=dev)
    Xd = Xbuf[shift_x:].view(n, d)
    Xd.copy_(torch.from_numpy(np.array(X, dtype=np.float32, order="C", copy=True)))
    ud = torch.from_numpy(np.array(u, dtype=np.float64, copy=True)).to(dev)
    assert ud.shape == (k,)
    Cbuf = torch.full((k * d + shift_c,), float("nan"), dtype=torch.float32, device=dev)
    Cd = Cbuf[shift_c:].view(k, d)
    assert Xd.data_ptr() % 16 == 4 * (shift_x % 4) and Cd.data_ptr() % 16 == 4 * (shift_c % 4)
    p = torch.full((k,), -1, dtype=torch.int32, device=dev) if want_out else None
    P = torch.full((1,), float("nan"), dtype=torch.float64, device=dev) if want_out else None
    s = torch.cuda.current_stream(dev) if stream is None else stream
    s.wait_stream(torch.cuda.current_stream(dev))  # the uploads above
    lib.check(lib.lib().cis_kmeanspp_dev(Xd.data_ptr(), n, d, k, ud.data_ptr(), Cd.data_ptr(), p.data_ptr() if want_out else None,
                                         P.data_ptr() if want_out else None, s.cuda_stream))
    s.synchronize()
    assert Xd.cpu().numpy().tobytes() == np.ascontiguousarray(X, dtype=np.float32).tobytes()
    return Cd.cpu().numpy(), (p.cpu().numpy() if want_out else None), (float(P.cpu()[0]) if want_out else None)


def _row_of_uniform(u, n):
    return min(int(np.floor(u * float(n))), n - 1)


# --------------------------------------------------------------------------------------------------------------------
# A. exact on integer lattices
# --------------------------------------------------------------------------------------------------------------------

def _lattice_seeds(X, k, u):
    """The semantics in int64: (picked [k], potential).  Every d2 < 2^24 and every sum < 2^53 (asserted), so float32 / float64
    arithmetic in any order gives these integers."""
    Xi = X.astype(np.int64)
    n = len(Xi)
    picked = np.empty(k, dtype=np.int64)
    picked[0] = _row_of_uniform(u[0], n)
    d2 = ((Xi - Xi[picked[0]]) ** 2).sum(1)
    assert d2.max() < tk.F24
    for j in range(1, k):
        S = np.cumsum(d2)
        tot = int(S[-1])
        assert tot < 1 << 53
        if tot == 0:
            picked[j] = _row_of_uniform(u[j], n)
        else:
            picked[j] = np.searchsorted(S.astype(np.float64), u[j] * float(tot), side="right")
            assert d2[picked[j]] > 0
        d2 = np.minimum(d2, ((Xi - Xi[picked[j]]) ** 2).sum(1))
    return picked, int(d2.sum())


_GRID_N = MAX_GRID * TILE + 3 * TILE + 17  # more tiles than one trip of the bounded grid, and a cut last tile

_CASES = {
    "n1000_d64_k121": lambda: (tk._case_random(1000, 64, 121, -8, 8, 31)[0], 121),    # 16 lanes per row, 16-byte pieces
    "n257_d33_k40": lambda: (tk._case_random(257, 33, 40, -8, 8, 32)[0], 40),         # d % 4 != 0: 4-byte pieces, 64 lanes, 31 idle
    "n130_d1_k1": lambda: (tk._case_random(130, 1, 1, -8, 8, 33)[0], 1),              # no draw at all; the potential alone
    "n5_d2_k8": lambda: (tk._case_n_lt_k()[0], 8),                                    # tot == 0 once the five rows are chosen
    "n4096_d128_k193": lambda: (tk._case_random(4096, 128, 193, -8, 8, 34)[0], 193),  # 32 lanes per row, 16 tiles
    "n300_d129_k70": lambda: (tk._case_random(300, 129, 70, -8, 8, 35)[0], 70),       # rows longer than a wave: the looping form
    "n%d_d4_k9" % (TILE - 1): lambda: (tk._case_random(TILE - 1, 4, 9, -8, 8, 37)[0], 9),  # a lane per row
    "n%d_d4_k9" % TILE: lambda: (tk._case_random(TILE, 4, 9, -8, 8, 38)[0], 9),
    "n%d_d4_k9" % (TILE + 1): lambda: (tk._case_random(TILE + 1, 4, 9, -8, 8, 39)[0], 9),
    "n300_d260_k20": lambda: (tk._case_random(300, 260, 20, -4, 4, 40)[0], 20),       # 65 16-byte pieces: the looping form on float4
    "ties": lambda: (tkd._case_ties()[0], 100),                                       # every lattice point three times
    "grid_stride_n%d_d2_k70" % _GRID_N: lambda: (tk._case_random(_GRID_N, 2, 70, -8, 8, 36)[0], 70),
}


def _uniforms(k, kind, seed):
    u = np.random.RandomState(seed).rand(k)
    if kind == "edges":  # the first row with d2 > 0, and the last one
        u[::3] = ONE_BELOW
        u[1::3] = 0.0
    return u


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """(X, k, u, picked, potential) of the int64 restatement."""
    X, k = _CASES[name]()
    X = np.ascontiguousarray(X, dtype=np.float32)
    assert np.abs(X).max() <= 8 and X.shape[1] <= 260
    u = _uniforms(k, kind, 100 + len(name))
    for a in (X, u):
        a.setflags(write=False)
    return (X, k, u) + _lattice_seeds(X, k, u)


def test_case_shapes():
    """The inputs are what the cases claim (no GPU needed)."""
    assert _GRID_N > MAX_GRID * TILE and _GRID_N % TILE != 0
    X, k, u, picked, potential = _case("n5_d2_k8", "random")
    assert sorted(picked[:5]) == [0, 1, 2, 3, 4] and potential == 0  # five distinct rows, then the fallback three times
    assert (picked[5:] == [_row_of_uniform(v, 5) for v in u[5:]]).all()
    X, k, u, picked, _ = _case("ties", "edges")
    assert len(X) == 3 * 289 and len(np.unique(X[picked], axis=0)) == k  # no copy of a chosen row is ever chosen
    u = _uniforms(9, "edges", 1)
    assert u[0] == ONE_BELOW < 1.0 and u[1] == 0.0 and 0.0 < u[2] < 1.0
    for n in (TILE - 1, TILE, 1000, 4096, _GRID_N):
        assert _row_of_uniform(ONE_BELOW, n) == n - 1 and _row_of_uniform(0.0, n) == 0
    X, k, u, picked, _ = _case("grid_stride_n%d_d2_k70" % _GRID_N, "edges")
    assert picked.max() >= MAX_GRID * TILE  # a pick in the second trip of the grid


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "edges"])
@pytest.mark.parametrize("name", list(_CASES))
def test_seeds_are_exact_on_lattices(name, kind):
    """Every pick equals the int64 restatement, centroid j is byte-equal to row picked[j], the potential is the exact integer;
    d_X comes back byte-equal (checked in _kpp) and every output element was written."""
    X, k, u, picked_ref, potential_ref = _case(name, kind)
    C, picked, potential = _kpp(X, k, u)
    assert (picked >= 0).all()
    np.testing.assert_array_equal(picked, picked_ref)
    assert C.tobytes() == X[picked].tobytes()
    assert potential == float(potential_ref)


# --------------------------------------------------------------------------------------------------------------------
# B. real-valued data
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_every_draw_is_valid_on_descriptors():
    """20 000 x 64 descriptor-like unit vectors, k = 256: a float64 replay that follows the device's picks.  With the exact d2,
    its prefix S and t = u[j] * tot after the device's first j picks, pick p must satisfy S(p - 1) (1 - eps) <= t (1 + eps),
    t (1 - eps) < S(p) (1 + eps) and d2[p] > 0; the potential is within eps; a second call gives the same bytes."""
    import golden_inputs as gi
    n, d, k = 20000, 64, 256
    X = gi.descriptor_like(n, d, 17, np.float32)
    u = np.random.RandomState(18).rand(k)
    eps = (d + 8) * 2.0 ** -24
    C, picked, potential = _kpp(X, k, u)
    assert (picked >= 0).all() and (picked < n).all()
    assert C.tobytes() == X[picked].tobytes()
    assert picked[0] == _row_of_uniform(u[0], n)
    X64 = X.astype(np.float64)
    d2 = ((X64 - X64[picked[0]]) ** 2).sum(1)
    worst = 0.0
    for j in range(1, k):
        S = np.cumsum(d2)
        t = u[j] * S[-1]
        p = int(picked[j])
        below = S[p - 1] if p > 0 else 0.0
        worst = max(worst, below / t - 1.0, 1.0 - S[p] / t)
        assert below * (1 - eps) <= t * (1 + eps), (j, p, below, t)
        assert t * (1 - eps) < S[p] * (1 + eps), (j, p, S[p], t)
        assert d2[p] > 0, (j, p)
        d2 = np.minimum(d2, ((X64 - X64[p]) ** 2).sum(1))
    print("largest relative overshoot of a draw: %.3g (eps %.3g); potential %.9g, float64 %.9g" % (worst, eps, potential, d2.sum()))
    assert abs(potential - d2.sum()) <= eps * d2.sum()
    C2, picked2, potential2 = _kpp(X, k, u)
    assert picked2.tobytes() == picked.tobytes() and C2.tobytes() == C.tobytes() and potential2 == potential


# --------------------------------------------------------------------------------------------------------------------
# C. call hygiene
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_null_outputs():
    """NULL d_picked and d_potential: the same centroids."""
    for name in ("n257_d33_k40", "n1000_d64_k121"):
        X, k, u, picked_ref, _ = _case(name, "random")
        C, picked, potential = _kpp(X, k, u, want_out=False)
        assert picked is None and potential is None
        assert C.tobytes() == X[picked_ref].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("shift_x,shift_c", [(1, 0), (0, 1), (3, 2)])
@pytest.mark.parametrize("name", ["n1000_d64_k121", "n4096_d128_k193", "n300_d260_k20"])
def test_rows_off_16_byte_alignment(name, shift_x, shift_c):
    """d % 4 == 0, but d_X or d_centroids starts 4, 8 or 12 bytes past a 16-byte boundary: the 4-byte form, the same answers."""
    X, k, u, picked_ref, potential_ref = _case(name, "random")
    C, picked, potential = _kpp(X, k, u, shift_x=shift_x, shift_c=shift_c)
    np.testing.assert_array_equal(picked, picked_ref)
    assert C.tobytes() == X[picked].tobytes() and potential == float(potential_ref)


@pytest.mark.gpu
def test_on_another_stream():
    import torch
    X, k, u, picked_ref, potential_ref = _case("n4096_d128_k193", "edges")
    C, picked, potential = _kpp(X, k, u, stream=torch.cuda.Stream())
    np.testing.assert_array_equal(picked, picked_ref)
    assert C.tobytes() == X[picked].tobytes() and potential == float(potential_ref)


@pytest.mark.gpu
def test_workspace_growth_and_reuse():
    """A small call, a large one, the small one again: the grow-only workspace serves all three."""
    small, large = "n257_d33_k40", "grid_stride_n%d_d2_k70" % _GRID_N
    for name in (small, large, small):
        X, k, u, picked_ref, potential_ref = _case(name, "random")
        C, picked, potential = _kpp(X, k, u)
        np.testing.assert_array_equal(picked, picked_ref)
        assert C.tobytes() == X[picked].tobytes() and potential == float(potential_ref)


# --------------------------------------------------------------------------------------------------------------------
# D. the Python layer (lopq/train.py)
# --------------------------------------------------------------------------------------------------------------------

class _SeedSpy(tkd._DevSpy):
    """_DevSpy that also records what cis_kmeanspp_dev returned (seeds) and what cis_kmeans_dev was handed (starts)."""

    def __init__(self, real, hip):
        super(_SeedSpy, self).__init__(real, hip)
        self.seeds, self.starts = [], []

    def cis_kmeanspp_dev(self, X, n, d, k, u, C, picked, potential, stream):
        import torch
        rc = self._real.cis_kmeanspp_dev(X, n, d, k, u, C, picked, potential, stream)
        torch.cuda.synchronize()
        self.seeds.append((n, C, self._read(C, np.float32, k * d).reshape(k, d)))
        return rc

    def cis_kmeans_dev(self, X, n, d, k, iters, C, assign, inertia, stream):
        import torch
        torch.cuda.synchronize()
        self.starts.append((C, self._read(C, np.float32, k * d).reshape(k, d)))
        return super(_SeedSpy, self).cis_kmeans_dev(X, n, d, k, iters, C, assign, inertia, stream)


@pytest.fixture
def spy(monkeypatch):
    lib = _L()
    s = _SeedSpy(lib.lib(), lib._load_hip_runtime())
    monkeypatch.setattr(lib, "lib", lambda: s)
    return s


def _python_layer_data():
    rs = np.random.RandomState(21)
    centres = rs.uniform(-50, 50, (20, 4))
    return (centres[rs.randint(0, 20, 3000)] + rs.randn(3000, 4)).astype(np.float32)


@pytest.mark.gpu
def test_kmeans_dev_seeds_on_the_device(spy, monkeypatch):
    """SEED_BACKEND = "device": kmeans_dev(X, 8, 1, n_init = 3) calls cis_kmeanspp_dev three times and cis_kmeans_dev three times and
    never kmeans_pp_init; the very tensor the seeding filled goes into cis_kmeans_dev, its rows are rows of X; the best of the three
    comes back; SEED_SAMPLE below n and None both work; a numpy array and a resident tensor agree; the globals are restored."""
    import torch
    from columbiaimagesearch_amd.lopq import train as T

    def boom(*a, **kw):
        raise AssertionError("kmeans_pp_init called")

    monkeypatch.setattr(T, "kmeans_pp_init", boom)
    X = _python_layer_data()
    rows = set(r.tobytes() for r in X)
    k, seed = 8, 13
    backends = (T.KMEANS_BACKEND, T.ACCUM_BACKEND, T.SEED_BACKEND, T.SEED_SAMPLE)
    assert backends == ("sklearn", "host", "host", 20000)
    T.SEED_BACKEND = "device"
    try:
        for sample, rows_seen in ((20000, 3000), (1000, 1000), (None, 3000)):
            T.SEED_SAMPLE = sample
            del spy.calls[:], spy.seeds[:], spy.starts[:]
            C, inertia = T.kmeans_dev(X, k, iters=1, n_init=3, random_state=seed)
            assert len(spy.seeds) == len(spy.starts) == len(spy.calls) == 3
            for (n_seed, ptr_seed, seeds), (ptr_start, start) in zip(spy.seeds, spy.starts):
                assert n_seed == rows_seen and ptr_seed == ptr_start and seeds.tobytes() == start.tobytes()
                assert all(r.tobytes() in rows for r in start)
                assert len(np.unique(start, axis=0)) == k
            assert len(set(s.tobytes() for _, _, s in spy.seeds)) == 3  # three different draws
            seen = [tk._inertia64(X, c) for _, _, c, _ in spy.calls]
            for s, call in zip(seen, spy.calls):
                np.testing.assert_allclose(call[3], s, rtol=1e-5)
            best = int(np.argmin([c[3] for c in spy.calls]))
            assert C.dtype == np.float64 and C.tobytes() == spy.calls[best][2].astype(np.float64).tobytes()
            assert inertia == spy.calls[best][3]
            C2, inertia2 = T.kmeans_dev(torch.from_numpy(X).cuda(), k, iters=1, n_init=3, random_state=seed)
            assert len(spy.seeds) == 6
            for a, b in zip(spy.seeds[:3], spy.seeds[3:]):
                assert a[2].tobytes() == b[2].tobytes()  # the seeding is deterministic
            np.testing.assert_allclose(C2, C, rtol=1e-5, atol=1e-5)  # (float32 atomic sums in the Lloyd step)
            np.testing.assert_allclose(inertia2, inertia, rtol=1e-5)
    finally:
        T.KMEANS_BACKEND, T.ACCUM_BACKEND, T.SEED_BACKEND, T.SEED_SAMPLE = backends
    assert (T.KMEANS_BACKEND, T.ACCUM_BACKEND, T.SEED_BACKEND) == ("sklearn", "host", "host")


@pytest.mark.gpu
def test_kmeans_pp_init_dev_follows_the_random_state():
    """kmeans_pp_init_dev(x, k, rs, sample): rs.choice(n, sample, replace=False) rows, then u = rs.rand(k); the result is
    cis_kmeanspp_dev on those rows (the lattice restatement), as a float32 tensor on x's device.  sample = None: all rows, no
    choice drawn."""
    import torch
    from columbiaimagesearch_amd.lopq import train as T
    X, k = _case("n1000_d64_k121", "random")[:2]
    xd = torch.from_numpy(np.array(X)).cuda()
    for sample in (300, 5000, None):
        rs = np.random.RandomState(77)
        if sample is None:
            sub = X
        else:
            sub = X[rs.choice(len(X), min(len(X), sample), replace=False)]
        picked, _ = _lattice_seeds(sub, k, rs.rand(k))
        C = T.kmeans_pp_init_dev(xd, k, np.random.RandomState(77), sample)
        assert C.is_cuda and C.dtype == torch.float32 and tuple(C.shape) == (k, 64)
        assert C.cpu().numpy().tobytes() == sub[picked].tobytes()


# --------------------------------------------------------------------------------------------------------------------
# E. it seeds well
# --------------------------------------------------------------------------------------------------------------------

_BLOB_SEED = 3


@functools.lru_cache(maxsize=None)
def _blobs16():
    """Sixteen blobs of 200 points, unit variance, centres on the 4 x 4 lattice of spacing 100; (X, label, u)."""
    rs = np.random.RandomState(_BLOB_SEED)
    g = 100.0 * np.arange(4)
    centres = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(16, 2)
    label = np.repeat(np.arange(16), 200)
    X = (centres[label] + rs.randn(3200, 2)).astype(np.float32)
    perm = rs.permutation(3200)
    return np.ascontiguousarray(X[perm]), label[perm], rs.rand(16)


def _seeds64(X, k, u):
    """The semantics in float64: (picked, the smallest relative distance of a threshold t to the prefix sums on either side)."""
    X64 = X.astype(np.float64)
    n = len(X64)
    picked = [_row_of_uniform(u[0], n)]
    d2 = ((X64 - X64[picked[0]]) ** 2).sum(1)
    margin = np.inf
    for j in range(1, k):
        S = np.cumsum(d2)
        t = u[j] * S[-1]
        p = int(np.searchsorted(S, t, side="right"))
        margin = min(margin, (S[p] - t) / t, (t - (S[p - 1] if p else 0.0)) / t if t > 0 else np.inf)
        picked.append(p)
        d2 = np.minimum(d2, ((X64 - X64[p]) ** 2).sum(1))
    return np.array(picked), margin


def test_blob_reference_hits_every_blob():
    """The float64 restatement alone puts one seed into each of the sixteen blobs, and none of its thresholds is within 10 eps
    (relative; eps = (d + 8) 2^-24 bounds what the float32 d2 moves a sum by) of a prefix sum: the device has to make the same
    picks."""
    X, label, u = _blobs16()
    picked, margin = _seeds64(X, 16, u)
    assert sorted(label[picked]) == list(range(16))
    assert margin > 10 * (2 + 8) * 2.0 ** -24, margin


@pytest.mark.gpu
def test_every_blob_receives_one_seed():
    X, label, u = _blobs16()
    C, picked, potential = _kpp(X, 16, u)
    assert sorted(label[picked]) == list(range(16)), label[picked]
    np.testing.assert_array_equal(picked, _seeds64(X, 16, u)[0])
    want = ((X.astype(np.float64)[:, None] - C.astype(np.float64)[None]) ** 2).sum(-1).min(1).sum()
    assert abs(potential - want) <= (2 + 8) * 2.0 ** -24 * want


@pytest.mark.gpu
def test_model_fit_with_device_seeds():
    """test_model_fit_through_the_device_backend with SEED_BACKEND = "device", and its margins: the reported inertia of a coarse
    half is at most 1.03 x scikit-learn's full KMeans on the same data, the model's reconstruction error at most 1.1 x that of the
    scikit-learn fit."""
    from sklearn.cluster import KMeans
    from columbiaimagesearch_amd.lopq import LOPQModel
    from columbiaimagesearch_amd.lopq import train as T
    import golden_inputs as gi
    X = gi.descriptor_like(30000, 128, 6, np.float64)
    half = np.ascontiguousarray(X[:, :64])
    assert (T.KMEANS_BACKEND, T.SEED_BACKEND) == ("sklearn", "host")
    errs = {}
    try:
        T.SEED_BACKEND = "device"
        C, inertia = T.kmeans_dev(half, 128, iters=25, n_init=2, random_state=3)
        ref = KMeans(n_clusters=128, n_init=2, max_iter=25, random_state=3).fit(half)
        print("coarse half: inertia %.6f, scikit-learn %.6f" % (inertia, ref.inertia_))
        assert inertia <= 1.03 * ref.inertia_, (inertia, ref.inertia_)
        for backend in ("sklearn", "device"):
            T.KMEANS_BACKEND = backend
            m = LOPQModel(V=128, M=4, subquantizer_clusters=64)
            m.fit(X, n_init=1, random_state=5)
            T.KMEANS_BACKEND = "sklearn"
            coarse, fine = m.predict_batch(X[:5000])
            rec = np.stack([m.reconstruct((tuple(c), tuple(f))) for c, f in zip(coarse[:500], fine[:500])])
            errs[backend] = float(((X[:500] - rec) ** 2).sum(1).mean())
    finally:
        T.KMEANS_BACKEND, T.SEED_BACKEND = "sklearn", "host"
    print("reconstruction error: %r" % (errs,))
    assert errs["device"] <= 1.1 * errs["sklearn"], errs


# --------------------------------------------------------------------------------------------------------------------
# F. argument checks (refused before any HIP call: no GPU needed)
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d,k,null,reason", [
    (0, 2, 4, None, "n must be > 0"),
    (-3, 2, 4, None, "n must be > 0"),
    ((1 << 31) - 255, 2, 4, None, "n must be <= 2^31 - 256"),
    (64, 2, 4, "X", "NULL d_X"),
    (64, 2, 4, "u", "NULL d_X, d_u"),
    (64, 2, 4, "C", "NULL d_X, d_u or d_centroids"),
    (64, 0, 4, None, "d and k must be >= 1"),
    (64, 2, 0, None, "d and k must be >= 1"),
    (64, 1, (1 << 30) + 1, None, "k * d must be <= 2^30"),
    (64, (1 << 30) + 1, 1, None, "k * d must be <= 2^30"),
    (64, 1 << 15, (1 << 15) + 1, None, "k * d must be <= 2^30"),
])
def test_rejects_bad_arguments(n, d, k, null, reason):
    """CIS_EINVAL and a message that names the reason.  The pointers are never followed (the refusal comes first), so two host
    words stand in for device memory."""
    lib = _L()
    word = np.zeros(2, dtype=np.float64)
    p = lib.ptr(word)
    rc = lib.lib().cis_kmeanspp_dev(None if null == "X" else p, n, d, k, None if null == "u" else p, None if null == "C" else p,
                                    None, None, None)
    assert rc == CIS_EINVAL and reason in lib.last_error(), (rc, lib.last_error())
    assert not word.any()
    with pytest.raises(ValueError, match=reason.replace("*", r"\*").replace("^", r"\^")):
        lib.check(rc)
