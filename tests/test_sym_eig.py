"""cis_sym_eig_dev (csrc/sym_eig.hip): batched symmetric eigendecomposition by cyclic Jacobi, one workgroup per matrix.

Exact cases, the error bounds of the design against numpy (u = 2^-53: residual and eigenvalues within 16 d u |A|_2, orthogonality
within 16 d u; the 16 is the worst figures of the numpy model of the scheme, tests/jacobi_model.py -- 2.2, 4.8, 4.0 in the
design's runs, 2.0, 5.1, 3.9 on the matrices here -- with a margin above 3x for another operation order), batches against solo
runs bit for bit, one bad matrix in a batch, argument checks.
The model itself runs here on the same matrices without a GPU, so the inputs are known to meet the bounds through the scheme alone."""
import numpy as np
import pytest

import jacobi_model as J

U = J.U


def _L():
    from columbiaimagesearch_amd import _lib
    return _lib


def _eig(A, with_info=True, side_stream=False):
    """The raw entry point on a [batch, d, d] numpy array: (W, V, info or None) as numpy arrays; outputs pre-filled with NaN / -7."""
    import torch
    lib = _L()
    A = np.ascontiguousarray(A, dtype=np.float64)
    batch, d = A.shape[0], A.shape[1]
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(dev) if side_stream else torch.cuda.current_stream(dev)
    with torch.cuda.stream(stream):
        dA = torch.from_numpy(A).to(dev)
        W = torch.full((batch, d), float("nan"), dtype=torch.float64, device=dev)
        V = torch.full((batch, d, d), float("nan"), dtype=torch.float64, device=dev)
        info = torch.full((batch,), -7, dtype=torch.int32, device=dev)
        lib.check(lib.lib().cis_sym_eig_dev(dA.data_ptr(), batch, d, W.data_ptr(), V.data_ptr(), info.data_ptr() if with_info else None,
                                            stream.cuda_stream))
        stream.synchronize()
        assert dA.cpu().numpy().tobytes() == A.tobytes()  # the input is never written
        return W.cpu().numpy(), V.cpu().numpy(), (info.cpu().numpy() if with_info else None)


_solo = {}


def _solo_run(key, A):
    """One matrix alone (batch = 1), computed once per key."""
    if key not in _solo:
        W, V, info = _eig(A[None])
        _solo[key] = (W[0], V[0], int(info[0]))
    return _solo[key]


# ---- exact cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("d", [2, 5, 33, 64, 65, 128])
def test_diagonal_matrices_are_only_sorted(d):
    """Distinct diagonal entries in shuffled order: nothing rotates, V is the sorting permutation, one sweep."""
    rs = np.random.RandomState(d)
    diag = (rs.permutation(d) - d // 2) * 1.5
    W, V, info = _eig(np.diag(diag)[None])
    o = np.argsort(diag)
    np.testing.assert_array_equal(W[0], diag[o])
    np.testing.assert_array_equal(V[0], np.eye(d)[:, o])
    assert info[0] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("d", [2, 32, 64, 128])
def test_blocks_of_3_1_1_3(d):
    """kron(I, [[3,1],[1,3]]): tau = 0 in every block, so t = 1 and c = s = fl(1/sqrt 2), within 2u of 1/sqrt 2 (two roundings of
    relative size u on a value of 0.71).  With c == s the rotated off-diagonal entries cancel exactly: one rotating sweep and a
    clean one.  Every block runs the same arithmetic, so the eigenvalues near 2 are equal bit for bit, as are those near 4; each
    is a sum of products of c with at most a dozen roundings on values up to 4: within 16 u |A|_2 of 2 and 4.  Equal eigenvalues
    keep their index order, and of two components of equal magnitude the first is made positive: (1, -1)/sqrt 2 and (1, 1)/sqrt 2."""
    A = np.kron(np.eye(d // 2), np.array([[3.0, 1.0], [1.0, 3.0]]))
    W, V, info = _eig(A[None])
    W, V = W[0], V[0]
    h = d // 2
    assert info[0] == 2
    assert (W[:h] == W[0]).all() and (W[h:] == W[h]).all()
    assert abs(W[0] - 2.0) <= 16 * U * 4 and abs(W[h] - 4.0) <= 16 * U * 4
    want = np.zeros((d, d))
    r = 1.0 / np.sqrt(2.0)
    for b in range(h):
        want[2 * b, b], want[2 * b + 1, b] = r, -r
        want[2 * b, h + b], want[2 * b + 1, h + b] = r, r
    assert (V[want == 0] == 0).all()
    assert np.abs(V - want).max() <= 2 * U


@pytest.mark.gpu
def test_one_by_one_identity_and_zero():
    W, V, info = _eig(np.array([[[-3.5]], [[0.0]], [[2.0]]]))
    np.testing.assert_array_equal(W, [[-3.5], [0.0], [2.0]])
    np.testing.assert_array_equal(V, np.ones((3, 1, 1)))
    np.testing.assert_array_equal(info, [1, 1, 1])
    for d in (3, 64, 128):
        W, V, info = _eig(np.stack([np.eye(d), np.zeros((d, d))]))
        np.testing.assert_array_equal(W, np.stack([np.ones(d), np.zeros(d)]))
        np.testing.assert_array_equal(V, np.stack([np.eye(d), np.eye(d)]))
        np.testing.assert_array_equal(info, [1, 1])


# ---- error bounds ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", J.DIMS)
def test_model_meets_the_bounds_on_the_test_matrices(d):
    """The numpy model of the scheme on the matrices of the GPU test below: every bound holds, in at most J.MODEL_SWEEPS sweeps."""
    for kind in J.KINDS:
        A = J.matrix(kind, d)
        W, V, sweeps = J.jacobi_eigh(A)
        figures = J.check_bounds(A, W, V, sweeps, max_sweeps=J.MODEL_SWEEPS, label=(kind, d))
        print("model %-18s d=%3d sweeps %2d  residual %.2f  orthogonality %.2f  eigenvalues %.2f (d u)" % ((kind, d, sweeps) + figures))


@pytest.mark.gpu
@pytest.mark.parametrize("d", J.DIMS)
def test_error_bounds(d):
    """Odd d, both sides of the d = 32 and d = 64 splits between the kernel's forms, the LDS limit d = 128; covariances (full rank
    and n = d), a spectrum graded over twelve decades, two eigenvalues repeated d/2 times, indefinite matrices with and without a
    zero diagonal, the latter scaled by 1e-150 and 1e140: one batch of the eight per d."""
    As = np.stack([J.matrix(kind, d) for kind in J.KINDS])
    W, V, info = _eig(As)
    for i, kind in enumerate(J.KINDS):
        figures = J.check_bounds(As[i], W[i], V[i], int(info[i]), label=(kind, d))
        print("device %-18s d=%3d sweeps %2d  residual %.2f  orthogonality %.2f  eigenvalues %.2f (d u)" % ((kind, d, info[i]) + figures))
        np.testing.assert_array_equal(V[i], J.fix_signs(V[i]))  # the sign rule holds on what the kernel wrote


# ---- batches ---------------------------------------------------------------------------------------------------------------------

def _pool(d, count):
    return [J.matrix(J.KINDS[i % len(J.KINDS)], d, seed=1 + i // len(J.KINDS)) for i in range(count)]


@pytest.mark.gpu
@pytest.mark.parametrize("d,batch,distinct,with_info,side_stream", [(128, 1, 8, False, False), (128, 3, 8, True, True),
                                                                     (128, 300, 8, True, False), (16, 1000, 40, True, False)])
def test_a_batch_equals_its_solo_runs_bit_for_bit(d, batch, distinct, with_info, side_stream):
    """Mixed matrices in one launch -- 300 at d = 128 is more workgroups than the chip has CUs -- against each matrix alone: no state
    leaks between workgroups, nothing depends on placement.  One batch runs on a side stream, one without d_info."""
    pool = _pool(d, distinct)
    pick = [(5 * i + 3) % distinct for i in range(batch)]
    W, V, info = _eig(np.stack([pool[p] for p in pick]), with_info=with_info, side_stream=side_stream)
    for i, p in enumerate(pick):
        w1, v1, i1 = _solo_run((d, p), pool[p])
        assert 1 <= i1 <= 40
        assert W[i].tobytes() == w1.tobytes() and V[i].tobytes() == v1.tobytes(), (i, p)
        if with_info:
            assert info[i] == i1


@pytest.mark.gpu
@pytest.mark.parametrize("d,poison", [(16, np.nan), (64, np.inf), (100, np.nan), (128, -np.inf)])
def test_a_bad_matrix_fails_alone(d, poison):
    pool = _pool(d, 5)
    As = np.stack(pool)
    As[2, d // 2, d // 3] = poison
    As[2, d // 3, d // 2] = poison
    W, V, info = _eig(As)
    assert info[2] == -1
    for i in (0, 1, 3, 4):
        w1, v1, i1 = _solo_run((d, i), pool[i])
        assert W[i].tobytes() == w1.tobytes() and V[i].tobytes() == v1.tobytes() and info[i] == i1 and i1 >= 1


# ---- arguments -------------------------------------------------------------------------------------------------------------------

def test_arguments_are_refused_before_the_device_is_touched():
    """Sizes and NULL pointers come back as CIS_EINVAL, batch = 0 as CIS_OK with nothing launched: none of these calls reads a
    pointer or needs a GPU (the addresses below are never used)."""
    lib = _L()
    f = lib.lib().cis_sym_eig_dev
    buf = np.zeros(4)
    p = lib.ptr(buf)
    assert f(p, 1, 0, p, p, None, None) == lib.CIS_EINVAL
    assert f(p, 1, 129, p, p, None, None) == lib.CIS_EINVAL
    assert "128" in lib.last_error()
    assert f(p, -1, 2, p, p, None, None) == lib.CIS_EINVAL
    assert f(None, 1, 2, p, p, None, None) == lib.CIS_EINVAL
    assert f(p, 1, 2, None, p, None, None) == lib.CIS_EINVAL
    assert f(p, 1, 2, p, None, None, None) == lib.CIS_EINVAL
    assert f(p, 0, 2, p, p, None, None) == lib.CIS_OK
    with pytest.raises(ValueError):
        lib.check(f(p, 1, 129, p, p, None, None))


@pytest.mark.gpu
def test_the_tensor_wrapper():
    import torch
    from columbiaimagesearch_amd.lopq import train as T
    A = np.stack([J.matrix("cov", 20), J.matrix("indefinite", 20)])
    W, V, info = T.sym_eig_dev(torch.from_numpy(A).cuda())
    assert W.is_cuda and V.is_cuda and info.dtype == torch.int32
    for i in range(2):
        J.check_bounds(A[i], W[i].cpu().numpy(), V[i].cpu().numpy(), int(info[i]))
    W0, V0, i0 = T.sym_eig_dev(torch.empty((0, 7, 7), dtype=torch.float64, device="cuda"))
    assert tuple(W0.shape) == (0, 7) and tuple(V0.shape) == (0, 7, 7) and tuple(i0.shape) == (0,)
    with pytest.raises(ValueError):
        T.sym_eig_dev(torch.zeros((1, 129, 129), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        T.sym_eig_dev(torch.zeros((1, 4, 4), dtype=torch.float32, device="cuda"))
