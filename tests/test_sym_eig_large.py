"""cis_sym_eig_large_dev (csrc/sym_eig_block.hip): symmetric eigendecomposition of one matrix in HBM by cyclic block Jacobi, the
pivots solved by the LDS solver of cis_sym_eig_dev.

The bound is not the 16 d u of the LDS solver: the pivots' orthogonality errors add up over the rounds.  It is derived from the
numpy model of the scheme alone (tests/block_jacobi_model.py, pivots by jacobi_model.jacobi_eigh), run on exactly the matrices of
the GPU test: the eight kinds of jacobi_model.matrix at d in {129, 192, 200, 257, 320} with blocks of 32 columns, the default
beyond d = 128 -- one column past the LDS solver, an exact multiple of both block sizes, a ragged last block, odd block counts with
their bye, five to ten blocks -- and at d in {200, 320} with blocks of 64 columns (four blocks with a ragged last one; five blocks
and a bye).  The model's worst figures in units of d u (|A|_2 d u for the first and the last):
    b = 32: residual 5.55, orthogonality 19.34, eigenvalues 11.83, at most 11 block sweeps (the graded spectrum at d = 320 gives
            the 19.34 and the 11)
    b = 64: residual 5.88, orthogonality 11.35, eigenvalues 8.56, at most 7 block sweeps (half the rounds per block sweep, and
            fewer block sweeps)
Per block size, the worst figure times 3 (the margin tests/test_sym_eig.py gives another operation order), rounded up: C = 59 at
b = 32, C = 35 at b = 64.  Every figure of the kernel is checked against C d u; the model itself is held to C / 3 and to its
recorded sweep counts here, without a GPU (minutes of numpy: the model's pivots are Python loops).  The kernel's figures never
entered C.  On an MI355X the kernel's worst figures were 5.56, 19.44, 11.80 at b = 32 and 5.89, 11.47, 8.64 at b = 64, with the
model's block sweep counts."""
import numpy as np
import pytest

import block_jacobi_model as M
import jacobi_model as J

U = M.U
C = M.C
BLOCKS = (32, 64)


def _L():
    from columbiaimagesearch_amd import _lib
    return _lib


def _eig(A, block=0, side_stream=False):
    """The raw entry point on a [d, d] numpy array: (W, V, info) with W and V numpy arrays; outputs pre-filled with NaN / -7, the
    workspace with 0xff bytes; the input buffer is compared with what was uploaded."""
    import torch
    lib = _L()
    A = np.ascontiguousarray(A, dtype=np.float64)
    d = A.shape[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.Stream(dev) if side_stream else torch.cuda.current_stream(dev)
    need = int(lib.lib().cis_sym_eig_large_workspace(d))
    assert need > 0
    with torch.cuda.stream(stream):
        dA = torch.from_numpy(A).to(dev)
        W = torch.full((d,), float("nan"), dtype=torch.float64, device=dev)
        V = torch.full((d, d), float("nan"), dtype=torch.float64, device=dev)
        info = torch.full((1,), -7, dtype=torch.int32, device=dev)
        work = torch.full((need,), 0xff, dtype=torch.uint8, device=dev)
        lib.check(lib.lib().cis_sym_eig_large_dev(dA.data_ptr(), d, block, W.data_ptr(), V.data_ptr(), info.data_ptr(), work.data_ptr(),
                                                  need, stream.cuda_stream))
        stream.synchronize()
        assert dA.cpu().numpy().tobytes() == A.tobytes()  # the input is never written
        return W.cpu().numpy(), V.cpu().numpy(), int(info.cpu()[0])


_runs = {}


def _run(kind, d, block):
    """One test matrix through the kernel, computed once."""
    key = (kind, d, block)
    if key not in _runs:
        _runs[key] = _eig(M.matrix(kind, d), block)
    return _runs[key]


# ---- error bounds ----------------------------------------------------------------------------------------------------------------

CASES = [(d, b) for b in BLOCKS for d in M.BLOCK_DIMS[b]]


@pytest.mark.parametrize("d,block", CASES)
@pytest.mark.parametrize("kind", M.KINDS)
def test_model_stays_within_a_third_of_the_bound(kind, d, block):
    """The numpy model of the scheme on a matrix of the GPU test: every figure within C / 3, in at most the recorded block sweeps."""
    A = M.matrix(kind, d)
    W, V, sweeps = M.block_eigh(A, block)
    f = M.check_bounds(A, W, V, sweeps, C[block] / 3.0, max_sweeps=M.MODEL_SWEEPS[block], label=(kind, d, block))
    print("model %-18s d=%3d b=%d block sweeps %2d  residual %.2f  orthogonality %.2f  eigenvalues %.2f (d u)" % ((kind, d, block, sweeps) + f))


@pytest.mark.gpu
@pytest.mark.parametrize("d,block", CASES)
def test_error_bounds(d, block):
    """The eight kinds per d and block size: residual, eigenvalues against eigvalsh and orthogonality within C d u, W ascending, the
    sign rule, 1 <= info <= 40, eigenvectors against LAPACK's where the spectrum is separated."""
    for kind in M.KINDS:
        A = M.matrix(kind, d)
        W, V, info = _run(kind, d, block)
        f = M.check_bounds(A, W, V, info, C[block], label=(kind, d, block))
        print("device %-18s d=%3d b=%d block sweeps %2d  residual %.2f  orthogonality %.2f  eigenvalues %.2f (d u)" % ((kind, d, block, info) + f))


@pytest.mark.gpu
def test_the_default_block_is_one_of_the_two():
    W, V, info = _run("indefinite", 200, 0)
    assert any(W.tobytes() == _run("indefinite", 200, b)[0].tobytes() and V.tobytes() == _run("indefinite", 200, b)[1].tobytes() for b in BLOCKS)


# ---- exact cases -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("d,block", [(129, 64), (200, 64), (257, 32), (320, 32)])
def test_diagonal_matrices_are_only_sorted(d, block):
    """Distinct diagonal entries in shuffled order, zero among them (the padding's eigenvalue): no pivot rotates, every Q is a
    permutation, V is the sorting permutation, one block sweep."""
    rs = np.random.RandomState(d)
    diag = (rs.permutation(d) - d // 2) * 1.5
    W, V, info = _eig(np.diag(diag), block)
    o = np.argsort(diag)
    np.testing.assert_array_equal(W, diag[o])
    np.testing.assert_array_equal(V, np.eye(d)[:, o])
    assert info == 1


@pytest.mark.gpu
@pytest.mark.parametrize("d,block", [(192, 64), (200, 32), (258, 64)])
def test_blocks_of_3_1_1_3(d, block):
    """kron(I, [[3,1],[1,3]]): every 2 x 2 block lies inside a diagonal block of the matrix, so the pivots meet it as the LDS solver
    does (tests/test_sym_eig.py): tau = 0, c = s = fl(1/sqrt 2) within 2u, the off-diagonal entries cancel exactly.  One block sweep
    rotates and a second finds nothing.  The eigenvalues near 2 are equal bit for bit, as are those near 4, within 16 u |A|_2; the
    tile products only add exact zeros, so every eigenvector has two nonzero components, (c, -c) for 2 and (c, c) for 4, in the
    rows of its block."""
    A = np.kron(np.eye(d // 2), np.array([[3.0, 1.0], [1.0, 3.0]]))
    W, V, info = _eig(A, block)
    h = d // 2
    assert info == 2
    assert (W[:h] == W[0]).all() and (W[h:] == W[h]).all()
    assert abs(W[0] - 2.0) <= 16 * U * 4 and abs(W[h] - 4.0) <= 16 * U * 4
    r = 1.0 / np.sqrt(2.0)
    seen = set()
    for j in range(d):
        nz = np.nonzero(V[:, j])[0]
        assert len(nz) == 2 and nz[0] % 2 == 0 and nz[1] == nz[0] + 1, (j, nz)
        assert abs(V[nz[0], j] - r) <= 2 * U and abs(V[nz[1], j] - (r if j >= h else -r)) <= 2 * U, (j, V[nz, j])
        seen.add((nz[0], j >= h))
    assert len(seen) == d


@pytest.mark.gpu
@pytest.mark.parametrize("d", [130, 200])
def test_the_zero_matrix(d):
    W, V, info = _eig(np.zeros((d, d)))
    np.testing.assert_array_equal(W, np.zeros(d))
    np.testing.assert_array_equal(V, np.eye(d))
    assert info == 1


@pytest.mark.gpu
def test_one_pivot_is_the_lds_solver():
    """d = 1 and d = 128 are one pivot: W is cis_sym_eig_dev's, bit for bit."""
    import torch
    from columbiaimagesearch_amd.lopq import train as T
    for A in (np.array([[-3.5]]), np.array([[0.0]]), J.matrix("cov", 128), J.matrix("indefinite", 128)):
        W, V, info = _eig(A)
        W0, V0, i0 = T.sym_eig_dev(torch.from_numpy(A[None]).cuda())
        assert W.tobytes() == W0[0].cpu().numpy().tobytes()
        assert 1 <= info <= 2
        np.testing.assert_array_equal(V, J.fix_signs(V))
        if A.shape[0] == 1:
            np.testing.assert_array_equal(V, [[1.0]])
        else:
            M.check_bounds(A, W, V, info, 16)  # the LDS solver's own bound


# ---- inputs and outputs ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("block", BLOCKS)
def test_streams_and_repeats_give_the_same_bits(block):
    """A side stream and a second call against the first run on the default stream; outputs that were NaN are fully written
    (the input buffer is checked by every call of _eig)."""
    A = M.matrix("indefinite", 200)
    W, V, info = _run("indefinite", 200, block)
    assert np.isfinite(W).all() and np.isfinite(V).all()
    for side in (True, False):
        W2, V2, i2 = _eig(A, block, side_stream=side)
        assert W2.tobytes() == W.tobytes() and V2.tobytes() == V.tobytes() and i2 == info


@pytest.mark.gpu
@pytest.mark.parametrize("d,poison,block", [(200, np.nan, 64), (200, np.inf, 32), (129, -np.inf, 64), (64, np.nan, 0)])
def test_a_bad_matrix_is_reported(d, poison, block):
    A = M.matrix("cov", d).copy()
    A[d // 2, d // 3] = poison
    A[d // 3, d // 2] = poison
    W, V, info = _eig(A, block)
    assert info == -1


# ---- arguments -------------------------------------------------------------------------------------------------------------------

def test_arguments_are_refused_before_the_device_is_touched():
    """Sizes, NULL pointers and a workspace that is too small come back as CIS_EINVAL: none of these calls reads a pointer or needs a
    GPU (the addresses below are never used)."""
    lib = _L()
    f = lib.lib().cis_sym_eig_large_dev
    ws = lib.lib().cis_sym_eig_large_workspace
    buf = np.zeros(4)
    p = lib.ptr(buf)
    big = 1 << 40
    assert f(p, 0, 0, p, p, None, p, big, None) == lib.CIS_EINVAL
    assert f(p, 4097, 0, p, p, None, p, big, None) == lib.CIS_EINVAL
    assert "4096" in lib.last_error()
    assert f(p, 200, 48, p, p, None, p, big, None) == lib.CIS_EINVAL
    assert f(None, 200, 0, p, p, None, p, big, None) == lib.CIS_EINVAL
    assert f(p, 200, 0, None, p, None, p, big, None) == lib.CIS_EINVAL
    assert f(p, 200, 0, p, None, None, p, big, None) == lib.CIS_EINVAL
    assert f(p, 200, 0, p, p, None, None, big, None) == lib.CIS_EINVAL
    need = ws(200)
    assert need >= 2 * 256 * 256 * 8
    assert f(p, 200, 0, p, p, None, p, need - 1, None) == lib.CIS_EINVAL
    assert str(need) in lib.last_error()
    assert ws(0) == lib.CIS_EINVAL and ws(4097) == lib.CIS_EINVAL
    assert "4096" in lib.last_error()
    assert 2 * 4096 * 4096 * 8 <= ws(4096) <= 2 * 4160 * 4160 * 8 + (1 << 24)
    assert all(ws(d) <= ws(d + 1) for d in (1, 63, 64, 127, 128, 129, 2047, 4095))
    with pytest.raises(ValueError):
        lib.check(f(p, 4097, 0, p, p, None, p, big, None))


@pytest.mark.gpu
def test_the_tensor_wrapper():
    import torch
    from columbiaimagesearch_amd.lopq import train as T
    A = M.matrix("cov", 150)
    for block in (0, 32, 64):
        W, V, info = T.sym_eig_large_dev(torch.from_numpy(A).cuda(), block)
        assert W.is_cuda and V.is_cuda and info.dtype == torch.int32 and tuple(W.shape) == (150,) and tuple(V.shape) == (150, 150)
        M.check_bounds(A, W.cpu().numpy(), V.cpu().numpy(), int(info.cpu()[0]), C[block or 32])
    with pytest.raises(ValueError):
        T.sym_eig_large_dev(torch.zeros((4097, 4097), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        T.sym_eig_large_dev(torch.zeros((4, 4), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        T.sym_eig_large_dev(torch.zeros((1, 4, 4), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        T.sym_eig_large_dev(torch.from_numpy(A).cuda(), 48)
