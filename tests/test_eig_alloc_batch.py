"""train.eigenvalue_allocation_batch: the bucket allocation of many spectra at once equals eigenvalue_allocation row by row."""
import numpy as np
import pytest

from columbiaimagesearch_amd.lopq import train as T


@pytest.mark.parametrize("d,buckets", [(d, b) for d in (4, 64, 128) for b in (1, 2, 4, 8) if b <= d])
def test_rows_equal_the_scalar_function(d, buckets):
    """200 random spectra with distinct values per shape, spread over ten decades; then spectra with a zero, with negative values
    only, of mixed sign, and with a zero among negative values (distinct values throughout: the scalar function's order of equal
    values is its sort's)."""
    rs = np.random.RandomState(1000 * d + buckets)
    W = rs.randn(200, d) * 10.0 ** rs.uniform(-5, 5, (200, 1))
    W[:50] = np.abs(W[:50])           # covariance-like: non-negative
    W[50:80] = -np.abs(W[50:80])      # negative only
    W[80:110, 0] = 0.0                # one zero, mixed signs
    W[110:130] = -np.abs(W[110:130])
    W[110:130, d - 1] = 0.0           # a zero among negative values
    W[130:150] = np.sort(W[130:150], axis=1)  # ascending, as an eigensolver returns them
    assert all(len(set(w)) == d for w in W)
    got = T.eigenvalue_allocation_batch(buckets, W)
    assert got.shape == (200, d) and got.dtype == np.int64
    for g in range(200):
        np.testing.assert_array_equal(got[g], T.eigenvalue_allocation(buckets, W[g]), err_msg="row %d" % g)


@pytest.mark.parametrize("buckets", [1, 2, 4, 8])
@pytest.mark.parametrize("d", [8, 64, 128])
def test_equal_spectra_give_valid_permutations(d, buckets):
    """All-equal spectra (ones: the small-cluster fallback; zeros; a negative constant): every row is a permutation of the dimensions
    with d / buckets of them per bucket, equal values in the reverse of their index order."""
    W = np.stack([np.ones(d), np.zeros(d), np.full(d, -2.5)])
    got = T.eigenvalue_allocation_batch(buckets, W)
    assert got.shape == (3, d)
    for row in got:
        assert sorted(row) == list(range(d))
        assert row.reshape(buckets, d // buckets).shape == (buckets, d // buckets)
    # ones: every log is 0, so the first bucket stays the least loaded until it is full, and so on: the reversed index order
    np.testing.assert_array_equal(got[0], np.arange(d)[::-1])


def test_shapes_are_checked():
    with pytest.raises(ValueError):
        T.eigenvalue_allocation_batch(2, np.ones(4))
    with pytest.raises(ValueError):
        T.eigenvalue_allocation_batch(3, np.ones((2, 4)))
    assert T.eigenvalue_allocation_batch(2, np.ones((0, 4))).shape == (0, 4)
