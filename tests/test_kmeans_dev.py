"""cis_kmeans_dev (csrc/kmeans_mfma.hip): Lloyd iterations on device data for codebooks of any size, and the Python layer on it.

The assignment minimises st(x, c) = fl32(|c|^2 - 2 x.c) from the float32 matrix cores, not the direct (x - c)^2 form.  With
u = 2^-24 and r = |x| + max_c |c|, |st - s| <= (d + 4) u r^2 =: E (derived at the top of csrc/lopq_eval.hip), so the chosen
centroid's float64 squared distance is at most D_min + 2 E: that is the bar on real-valued data.  On INTEGER LATTICES every
product, partial sum, |c|^2 and score is an integer below 2^24 and exact in float32 in any order, so there the results equal an
int64 reference (the builders of tests/test_train_kernels.py, plus a guard for the expanded form).
"""
import ctypes
import functools

import numpy as np
import pytest

import test_train_kernels as tk

F24 = tk.F24
CIS_EINVAL = -1
PM, CN, MAX_GRID = 128, 64, 2048  # the kernel's point tile, centroid tile and persistent grid (csrc/kmeans_mfma.hip)
U = 2.0 ** -24


def _L():
    from columbiaimagesearch_amd import _lib
    return _lib


def _kmd(X, C0, iters, want_out=True, stream=None):
    """cis_kmeans_dev on device copies; (centroids, assign or None, inertia or None).  assign is pre-filled with -1 and the
    inertia with NaN, so an element nobody wrote shows; d_X must come back byte-equal."""
    import torch
    lib = _L()
    dev = torch.device("cuda", torch.cuda.current_device())
    n, d = X.shape
    Xd = torch.from_numpy(np.array(X, dtype=np.float32, order="C", copy=True)).to(dev)
    Cd = torch.from_numpy(np.array(C0, dtype=np.float32, order="C", copy=True)).to(dev)
    a = torch.full((n,), -1, dtype=torch.int32, device=dev) if want_out else None
    I = torch.full((1,), float("nan"), dtype=torch.float64, device=dev) if want_out else None
    s = torch.cuda.current_stream(dev) if stream is None else stream
    s.wait_stream(torch.cuda.current_stream(dev))  # the uploads above
    lib.check(lib.lib().cis_kmeans_dev(Xd.data_ptr(), n, d, Cd.shape[0], int(iters), Cd.data_ptr(), a.data_ptr() if want_out else None,
                                       I.data_ptr() if want_out else None, s.cuda_stream))
    s.synchronize()
    assert Xd.cpu().numpy().tobytes() == np.ascontiguousarray(X, dtype=np.float32).tobytes()
    return Cd.cpu().numpy(), (a.cpu().numpy() if want_out else None), (float(I.cpu()[0]) if want_out else None)


# --------------------------------------------------------------------------------------------------------------------
# A. exact on integer lattices
# --------------------------------------------------------------------------------------------------------------------

def _case_ties():
    """69 distinct points of the even lattice {-8, -6, .. 8}^2 as centroids, and row 67 a copy of row 3: the two copies fall into
    different 64-wide centroid tiles.  The data is every point of [-8, 8]^2 three times, so every point with an odd
    coordinate lies exactly half-way between even neighbours.  The lower index must win; cluster 67 stays empty."""
    rs = np.random.RandomState(5)
    g = np.arange(-8, 9, 2)
    even = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    C = even[rs.permutation(len(even))[:69]].astype(np.float32)
    C = np.ascontiguousarray(np.insert(C, 3 + CN, C[3], axis=0))
    g = np.arange(-8, 9)
    X = np.tile(np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2), (3, 1)).astype(np.float32)
    return np.ascontiguousarray(X[rs.permutation(len(X))]), C


_CASES = {
    "n1000_d64_k121": lambda: tk._case_random(1000, 64, 121, -8, 8, 31),     # k * d = 7744: just over cis_kmeans' 7680
    "n257_d33_k300": lambda: tk._case_random(257, 33, 300, -8, 8, 32),       # d one past a stage, five centroid tiles, n = 2 tiles + 1
    "n130_d1_k1": lambda: tk._case_random(130, 1, 1, -8, 8, 33),
    "n5_d2_k8": tk._case_n_lt_k,                                             # n < k, empty clusters
    "n4096_d128_k193": lambda: tk._case_random(4096, 128, 193, -8, 8, 34),   # the widest register-resident form, k = 3 tiles + 1
    "n300_d129_k70": lambda: tk._case_random(300, 129, 70, -8, 8, 35),       # d odd and past 128: the per-stage form
    "ties": _case_ties,
    "grid_stride_n263001_d2_k70": lambda: tk._case_random(263001, 2, 70, -8, 8, 36),  # > 2048 * 128 points: a second trip
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(X, C, assign, inertia, C1, counts) with the guards of _lattice_reference, and one for the expanded form: sum |x_i c_i|
    and |c|^2 stay below 2^24 / 4, so |c|^2 - 2 x.c and all its partial sums are exact float32 integers in any order, and a
    float32 emulation of the score has the int64 argmin (first minimum)."""
    X, C = _CASES[name]()
    assert np.abs(X).max() <= 8 and np.abs(C).max() <= 8
    for a in (X, C):
        a.setflags(write=False)
    ref = tk._lattice_reference(X, C)
    Xi, Ci = X.astype(np.int64), C.astype(np.int64)
    cn = (Ci * Ci).sum(1)
    assert cn.max() < F24 // 4
    for a in range(0, len(X), 65536):
        assert (np.abs(Xi[a:a + 65536]) @ np.abs(Ci).T).max() < F24 // 4
        st = cn[None] - 2 * (Xi[a:a + 65536] @ Ci.T)
        st32 = cn.astype(np.float32)[None] - np.float32(2) * (X[a:a + 65536] @ C.T)
        assert st32.dtype == np.float32 and (st32.astype(np.int64) == st).all()
        assert (st32.argmin(1) == ref[0][a:a + 65536]).all()
    return (X, C) + ref


@functools.lru_cache(maxsize=None)
def _run(name, iters, want_out):
    X, C = _case(name)[:2]
    return _kmd(X, C, iters, want_out)


def test_case_shapes():
    """The inputs are what the cases claim (no GPU needed)."""
    X, C = _case("n1000_d64_k121")[:2]
    assert C.size == 7744 > 7680
    assert _case("grid_stride_n263001_d2_k70")[0].shape[0] > MAX_GRID * PM
    X, C, assign, _, _, counts = _case("ties")
    assert (C[3] == C[3 + CN]).all() and 3 // CN != (3 + CN) // CN and counts[3] > 0 and counts[3 + CN] == 0
    assert len(np.unique(C, axis=0)) == len(C) - 1
    D = ((X.astype(np.int64)[:, None] - C.astype(np.int64)[None]) ** 2).sum(-1)
    tied = (D == D.min(1, keepdims=True)).sum(1) > 1
    assert tied.sum() >= 100 and (D[tied, 3] != D[tied].min(1)).sum() >= 30  # ties other than the duplicate row's, too
    lo, hi = np.sort(np.argsort(D, axis=1, kind="stable")[:, :2], axis=1).T
    assert ((lo[tied] // CN) != (hi[tied] // CN)).sum() >= 30  # ... and some between two centroid tiles
    assert (_case("n5_d2_k8")[5] == [1, 0, 1, 1, 0, 1, 0, 1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("want_out", [True, False], ids=["outputs", "null"])
@pytest.mark.parametrize("name", list(_CASES))
def test_assignment_only_is_exact(name, want_out):
    """iters = 0: the centroid bytes are untouched, the assignment is the int64 argmin with the first minimum, the inertia is
    the exact integer.  Exact inertia at n = 263 001 says every row was visited once."""
    X, C, assign_ref, inertia_ref = _case(name)[:4]
    got_C, assign, inertia = _run(name, 0, want_out)
    assert got_C.tobytes() == C.tobytes()
    if want_out:
        np.testing.assert_array_equal(assign, assign_ref)
        assert inertia == float(inertia_ref)
    else:
        assert assign is None and inertia is None


@pytest.mark.gpu
@pytest.mark.parametrize("want_out", [True, False], ids=["outputs", "null"])
@pytest.mark.parametrize("name", list(_CASES))
def test_one_step_is_exact(name, want_out):
    """iters = 1: the centroids EQUAL float32(sum) / float32(count) of the int64 reference, an empty cluster keeps its bytes
    (the higher copy of the duplicate row among them); assign and inertia describe the returned centroids: within D_min + 2 E
    of the float64 nearest, and the float64 sum over the kernel's own assignment to 1e-5."""
    X, C, _, _, C1_ref, counts = _case(name)
    got_C, assign, inertia = _run(name, 1, want_out)
    np.testing.assert_array_equal(got_C, C1_ref)
    assert got_C[counts == 0].tobytes() == C[counts == 0].tobytes()
    if want_out:
        assert assign.min() >= 0 and assign.max() < len(C)
        _check_assignment(X, got_C, assign, inertia)


def _check_assignment(X, C, assign, inertia):
    """Every point's assigned centroid has float64 squared distance <= D_min + 2 E, E = (d + 4) 2^-24 (|x| + max |c|)^2 per point;
    the inertia is the float64 sum over that assignment to rtol 1e-5 (the margin test_kmeans_one_step_is_exact sets for the same
    float32 chain)."""
    d = X.shape[1]
    dmin, dass = tk._eval64(X, C, assign)
    r = np.sqrt((X.astype(np.float64) ** 2).sum(1)) + np.sqrt((C.astype(np.float64) ** 2).sum(1).max())
    E = (d + 4) * U * r * r
    bad = np.nonzero(dass > dmin + 2 * E)[0]
    assert bad.size == 0, (bad[:10], dass[bad[:10]], dmin[bad[:10]], E[bad[:10]])
    np.testing.assert_allclose(inertia, dass.sum(), rtol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("want_out", [True, False], ids=["outputs", "null"])
def test_empty_clusters_keep_their_centroid(want_out):
    """n < k: the three clusters without a point are byte-equal after 1 and after 3 iterations, the others sit on their point."""
    X, C, assign_ref, _, C1_ref, counts = _case("n5_d2_k8")
    want = C.copy()
    want[assign_ref] = X
    for iters in (1, 3):
        got_C, assign, inertia = _kmd(X, C, iters, want_out)
        assert got_C[counts == 0].tobytes() == C[counts == 0].tobytes()
        np.testing.assert_array_equal(got_C, want)
        if want_out:
            np.testing.assert_array_equal(assign, assign_ref)
            assert inertia == 0.0


# --------------------------------------------------------------------------------------------------------------------
# B. real-valued data
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_assignment_within_the_bound_on_descriptors():
    """20 000 x 64 descriptor-like unit vectors, 150 random centroids (k * d = 9600): every assigned centroid within D_min + 2 E in
    float64, inertia to 1e-5; the same after one update."""
    import golden_inputs as gi
    X = gi.descriptor_like(20000, 64, 8, np.float32)
    C0 = np.ascontiguousarray(X[np.random.RandomState(9).permutation(len(X))[:150]] + np.float32(0.01))
    for iters in (0, 1):
        C, assign, inertia = _kmd(X, C0, iters)
        assert (C.tobytes() == C0.tobytes()) == (iters == 0)
        assert assign.min() >= 0 and assign.max() < 150
        _check_assignment(X, C, assign, inertia)


_EMPTY = 17  # row of the far-away centroid


@functools.lru_cache(maxsize=None)
def _blobs():
    """(20 000, 64) points in 150 unit-variance blobs whose centres are distinct points of 40 * {-2..2}^64 (>= 40 apart), the
    start one perturbed point per blob plus a far-away centroid at row 17 (151 x 64 = 9664 floats); and a float64 Lloyd run from
    that start: (X, C0, assign [n], [C after 0, 1, .. 5 updates]).  The reference's assignment is constant, with a margin far
    above 2 E (asserted)."""
    rs = np.random.RandomState(12)
    n, d, nb = 20000, 64, 150
    cent = set()
    while len(cent) < nb:
        cent.add(tuple(rs.randint(-2, 3, d)))
    centres = 40.0 * np.array(sorted(cent))
    label = np.concatenate([np.arange(nb), rs.randint(0, nb, n - nb)])
    X = (centres[label] + rs.randn(n, d)).astype(np.float32)
    C0 = (X[:nb] + 0.5 * rs.randn(nb, d)).astype(np.float32)
    C0 = np.ascontiguousarray(np.insert(C0, _EMPTY, np.full(d, 100.0, dtype=np.float32), axis=0))  # (|c| = 800: E stays small)
    X64 = X.astype(np.float64)
    r = np.sqrt((X64 ** 2).sum(1)).max() + np.sqrt((C0.astype(np.float64) ** 2).sum(1).max())
    E = (d + 4) * U * r * r
    Cs = [C0.astype(np.float64)]
    assigns = []
    for _ in range(6):
        C = Cs[-1]
        D = (X64 ** 2).sum(1)[:, None] - 2.0 * X64 @ C.T + (C ** 2).sum(1)[None]  # (float64: rounding ~1e-7, margins > 100)
        a = D.argmin(1)
        part = np.partition(D, 1, axis=1)
        assert (part[:, 1] - part[:, 0]).min() > 1000.0 > 20 * 2 * E  # no assignment is anywhere near the kernel's bound
        assigns.append(a)
        C = C.copy()
        for c in np.unique(a):
            C[c] = X64[a == c].mean(0)
        Cs.append(C)
    assert all((a == assigns[0]).all() for a in assigns) and not (assigns[0] == _EMPTY).any()
    assert np.bincount(assigns[0], minlength=nb + 1).tolist().count(0) == 1
    for a in (X, C0):
        a.setflags(write=False)
    return X, C0, assigns[0], Cs


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 4])
def test_chain_over_iterations(T):
    """iters = T + 1 is one more Lloyd step after iters = T: its centroids are the float64 means under the assignment that
    iters = T reported, to the worst-case float32 accumulation bound; the far centroid keeps its bytes; the end of the chain
    matches the float64 Lloyd run to (T + 1) times that bound."""
    X, C0, assign_ref, Cs = _blobs()
    C_T, a_T, inertia_T = _kmd(X, C0, T)
    C_T1, a_T1, _ = _kmd(X, C0, T + 1)
    np.testing.assert_array_equal(a_T, assign_ref)
    np.testing.assert_array_equal(a_T1, assign_ref)
    X64 = X.astype(np.float64)
    mean = C0.astype(np.float64)
    for c in np.unique(a_T):
        mean[c] = X64[a_T == c].mean(0)
    tol = tk._accumulation_bound(X, a_T, mean)
    for C in (C_T, C_T1):
        assert C[_EMPTY].tobytes() == C0[_EMPTY].tobytes()
    err = np.abs(C_T1.astype(np.float64) - mean)
    assert (err <= tol).all(), (err.max(), tol.min())
    err = np.abs(C_T1.astype(np.float64) - Cs[T + 1])
    assert (err <= (T + 1) * tk._accumulation_bound(X, assign_ref, Cs[T + 1])).all(), err.max()
    dass = ((X64 - C_T.astype(np.float64)[a_T]) ** 2).sum(1)
    np.testing.assert_allclose(inertia_T, dass.sum(), rtol=1e-5)


# --------------------------------------------------------------------------------------------------------------------
# C. stream and ownership
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_on_another_stream():
    """The same call enqueued on a non-default stream gives the lattice results (and leaves d_X alone: checked in _kmd)."""
    import torch
    name = "n257_d33_k300"
    X, C, assign_ref, inertia_ref, C1_ref, _ = _case(name)
    side = torch.cuda.Stream()
    got_C, assign, inertia = _kmd(X, C, 0, stream=side)
    assert got_C.tobytes() == C.tobytes() and inertia == float(inertia_ref)
    np.testing.assert_array_equal(assign, assign_ref)
    np.testing.assert_array_equal(_kmd(X, C, 1, stream=side)[0], C1_ref)


@pytest.mark.gpu
def test_workspace_growth_and_reuse():
    """A small call, a larger one (more points, more centroids, more dimensions), the small one again: the grow-only
    workspace serves all three, with and without the caller's assignment buffer."""
    small, large = "n257_d33_k300", "n4096_d128_k193"
    for name in (small, large, small):
        X, C, assign_ref, inertia_ref, C1_ref, _ = _case(name)
        _, assign, inertia = _kmd(X, C, 0)
        np.testing.assert_array_equal(assign, assign_ref)
        assert inertia == float(inertia_ref)
        np.testing.assert_array_equal(_kmd(X, C, 1, want_out=False)[0], C1_ref)


# --------------------------------------------------------------------------------------------------------------------
# D. argument checks (refused before any HIP call: no GPU needed)
# --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,d,k,iters,null,reason", [
    (0, 2, 4, 1, None, "n must be > 0"),
    (-3, 2, 4, 1, None, "n must be > 0"),
    ((1 << 31) - 255, 2, 4, 1, None, "n must be <= 2^31 - 256"),
    (64, 2, 4, -1, None, "iters must be"),
    (64, 2, 4, 1, "X", "NULL d_X"),
    (64, 2, 4, 1, "C", "NULL d_X or d_centroids"),
    (64, 0, 4, 1, None, "d and k must be >= 1"),
    (64, 2, 0, 1, None, "d and k must be >= 1"),
    (64, 1, (1 << 30) + 1, 1, None, "k * d must be <= 2^30"),
    (64, (1 << 30) + 1, 1, 1, None, "k * d must be <= 2^30"),
    (64, 1 << 15, (1 << 15) + 1, 1, None, "k * d must be <= 2^30"),
])
def test_rejects_bad_arguments(n, d, k, iters, null, reason):
    """CIS_EINVAL and a message that names the reason.  The pointers are never followed (the refusal comes first), so two
    host words stand in for device memory."""
    lib = _L()
    word = np.zeros(2, dtype=np.float64)
    p = lib.ptr(word)
    rc = lib.lib().cis_kmeans_dev(None if null == "X" else p, n, d, k, iters, None if null == "C" else p, None, None, None)
    assert rc == CIS_EINVAL and reason in lib.last_error(), (rc, lib.last_error())
    assert not word.any()
    with pytest.raises(ValueError, match=reason.replace("*", r"\*").replace("^", r"\^")):
        lib.check(rc)


# --------------------------------------------------------------------------------------------------------------------
# E. the Python layer (lopq/train.py)
# --------------------------------------------------------------------------------------------------------------------

class _DevSpy(object):
    """The loaded library with cis_kmeans_dev recorded: (k, d, returned centroids, reported inertia) of every call."""

    def __init__(self, real, hip):
        self._real, self._hip, self.calls = real, hip, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _read(self, ptr, dtype, count):
        out = np.empty(count, dtype=dtype)
        assert self._hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes), 2) == 0  # device to host
        return out

    def cis_kmeans_dev(self, X, n, d, k, iters, C, assign, inertia, stream):
        import torch
        rc = self._real.cis_kmeans_dev(X, n, d, k, iters, C, assign, inertia, stream)
        torch.cuda.synchronize()
        self.calls.append((k, d, self._read(C, np.float32, k * d).reshape(k, d), None if inertia is None else float(self._read(inertia, np.float64, 1)[0])))
        return rc


@pytest.fixture
def spy(monkeypatch):
    lib = _L()
    s = _DevSpy(lib.lib(), lib._load_hip_runtime())
    monkeypatch.setattr(lib, "lib", lambda: s)
    return s


@pytest.mark.gpu
def test_kmeans_dev_returns_the_best_of_n_init(spy):
    """The construction of test_kmeans_hip_returns_the_best_of_n_init: 20 tight blobs, k = 8, one Lloyd step, n_init = 3 -- three
    calls whose inertias differ visibly; the best one comes back, as float64, with its reported inertia.  A numpy array and a
    resident tensor give the same answer."""
    import torch
    from columbiaimagesearch_amd.lopq import train as T
    rs = np.random.RandomState(21)
    centres = rs.uniform(-50, 50, (20, 4))
    X = (centres[rs.randint(0, 20, 3000)] + rs.randn(3000, 4)).astype(np.float32)
    k, seed = 8, 13
    emu = []
    ers = np.random.RandomState(seed)
    for _ in range(3):
        C = np.ascontiguousarray(T.kmeans_pp_init(X, k, ers), dtype=np.float32).astype(np.float64)
        a = ((X.astype(np.float64)[:, None, :] - C[None]) ** 2).sum(-1).argmin(1)
        for c in np.unique(a):
            C[c] = X[a == c].astype(np.float64).mean(0)
        emu.append(tk._inertia64(X, C))
    gaps = np.abs(np.subtract.outer(emu, emu))[np.triu_indices(3, 1)]
    assert gaps.min() > 1e-3 * max(emu) and int(np.argmin(emu)) != 0, emu

    C, inertia = T.kmeans_dev(X, k, iters=1, n_init=3, random_state=seed)
    assert len(spy.calls) == 3
    seen = [tk._inertia64(X, c) for _, _, c, _ in spy.calls]
    np.testing.assert_allclose(seen, emu, rtol=1e-4)
    for s, call in zip(seen, spy.calls):
        np.testing.assert_allclose(call[3], s, rtol=1e-5)
    best = int(np.argmin(seen))
    assert best == int(np.argmin(emu))
    assert C.dtype == np.float64 and C.tobytes() == spy.calls[best][2].astype(np.float64).tobytes()
    assert inertia == spy.calls[best][3]
    C2, inertia2 = T.kmeans_dev(torch.from_numpy(X).cuda(), k, iters=1, n_init=3, random_state=seed)
    assert len(spy.calls) == 6
    np.testing.assert_allclose(C2, C, rtol=1e-5, atol=1e-5)  # (float32 atomic sums: the last bits may differ between two runs)
    np.testing.assert_allclose(inertia2, inertia, rtol=1e-5)


@pytest.mark.gpu
def test_backend_device_takes_every_codebook(spy, monkeypatch):
    """KMEANS_BACKEND = "device": _kmeans(X, 121, ...) at d = 64 (k * d = 7744, which "hip" leaves to scikit-learn) reaches
    cis_kmeans_dev, and so does a small codebook; neither kmeans_hip nor cis_kmeans is called.  The globals are restored."""
    from columbiaimagesearch_amd.lopq import train as T

    def boom(*a, **kw):
        raise AssertionError("kmeans_hip called")

    X = np.random.RandomState(4).randn(400, 64)
    monkeypatch.setattr(T, "kmeans_hip", boom)
    backends = (T.KMEANS_BACKEND, T.ACCUM_BACKEND)
    T.KMEANS_BACKEND = "device"
    try:
        C = T._kmeans(X, 121, 2, 3, 0)
        assert C.shape == (121, 64) and C.dtype == np.float64 and np.isfinite(C).all()
        assert [(k, d) for k, d, _, _ in spy.calls] == [(121, 64)] * 3
        best = int(np.argmin([c[3] for c in spy.calls]))
        assert C.tobytes() == spy.calls[best][2].astype(np.float64).tobytes()
        T._kmeans(X, 16, 1, 1, 0)
        assert (spy.calls[-1][0], spy.calls[-1][1]) == (16, 64) and len(spy.calls) == 4
    finally:
        T.KMEANS_BACKEND, T.ACCUM_BACKEND = backends
    assert (T.KMEANS_BACKEND, T.ACCUM_BACKEND) == ("sklearn", "host")


@pytest.mark.gpu
def test_assign_clusters_dev_equals_assign_clusters_on_a_lattice():
    """Lattice data, float64 centroids as train() holds them: the int64 first-minimum assignment, from a numpy array and from a
    resident tensor."""
    import torch
    from columbiaimagesearch_amd.lopq import train as T
    X, C, assign_ref = _case("n1000_d64_k121")[:3]
    host = T.assign_clusters(X.astype(np.float64), C.astype(np.float64))
    np.testing.assert_array_equal(host, assign_ref)
    for data in (X.astype(np.float64), torch.from_numpy(np.array(X)).cuda()):
        got = T.assign_clusters_dev(data, C.astype(np.float64))
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, host)


@pytest.mark.gpu
def test_model_fit_through_the_device_backend():
    """LOPQModel(V = 128, M = 4, 64 sub-quantizer clusters) on 30 000 x 128 descriptor-like vectors: a coarse half is 128 x 64 =
    8192 floats, beyond cis_kmeans.  The margins of test_kmeans_hip_distortion_close_to_sklearn: the reported inertia of a coarse
    half is at most 1.03 x scikit-learn's full KMeans on the same data, and the model's reconstruction error at most 1.1 x that
    of the scikit-learn fit."""
    from sklearn.cluster import KMeans
    from columbiaimagesearch_amd.lopq import LOPQModel
    from columbiaimagesearch_amd.lopq import train as T
    import golden_inputs as gi
    X = gi.descriptor_like(30000, 128, 6, np.float64)
    half = np.ascontiguousarray(X[:, :64])
    C, inertia = T.kmeans_dev(half, 128, iters=25, n_init=2, random_state=3)
    ref = KMeans(n_clusters=128, n_init=2, max_iter=25, random_state=3).fit(half)
    print("coarse half: inertia %.6f, scikit-learn %.6f" % (inertia, ref.inertia_))
    assert inertia <= 1.03 * ref.inertia_, (inertia, ref.inertia_)
    errs = {}
    for backend in ("sklearn", "device"):
        T.KMEANS_BACKEND = backend
        try:
            m = LOPQModel(V=128, M=4, subquantizer_clusters=64)
            m.fit(X, n_init=1, random_state=5)
        finally:
            T.KMEANS_BACKEND = "sklearn"
        coarse, fine = m.predict_batch(X[:5000])
        rec = np.stack([m.reconstruct((tuple(c), tuple(f))) for c, f in zip(coarse[:500], fine[:500])])
        errs[backend] = float(((X[:500] - rec) ** 2).sum(1).mean())
    print("reconstruction error: %r" % (errs,))
    assert errs["device"] <= 1.1 * errs["sklearn"], errs
