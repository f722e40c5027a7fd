"""CPU-side checks of the removal entry points (include/cis_hip.h: cis_index_remove[_dev], cis_index_sub_remote_counts[_dev]):
their argument checks come before any device call and before the handle is read, so they answer CIS_EINVAL on a machine without a
GPU too.  The GPU behaviour is in tests/test_index_remove.py."""
import ctypes

import numpy as np
import pytest


def _lib():
    from columbiaimagesearch_amd import _lib
    return _lib, _lib.lib()


@pytest.fixture()
def blank_handle():
    """A non-NULL `cis_index*` for calls that must fail on their OTHER arguments: zeroed memory that a correct entry point never
    reads (a model, and with it a real handle, needs a GPU)."""
    buf = ctypes.create_string_buffer(1 << 20)
    return ctypes.cast(buf, ctypes.c_void_p), buf


def test_null_handle_is_einval_for_the_four_entry_points():
    _lib_, L = _lib()
    ids = np.array([1, 2, 3], dtype=np.int64)
    delta = np.zeros(16, dtype=np.int64)
    n = ctypes.c_int64(7)
    assert L.cis_index_remove(None, _lib_.ptr(ids), 3, ctypes.byref(n)) == _lib_.CIS_EINVAL
    assert L.cis_index_remove_dev(None, _lib_.ptr(ids), 3, ctypes.byref(n), None, None) == _lib_.CIS_EINVAL
    assert L.cis_index_sub_remote_counts(None, _lib_.ptr(delta)) == _lib_.CIS_EINVAL
    assert L.cis_index_sub_remote_counts_dev(None, _lib_.ptr(delta), None) == _lib_.CIS_EINVAL
    assert "NULL" in _lib_.last_error()
    with pytest.raises(ValueError):
        _lib_.check(L.cis_index_remove(None, None, 0, None))


def test_null_array_with_a_positive_count_is_einval(blank_handle):
    _lib_, L = _lib()
    h, _keep = blank_handle
    n = ctypes.c_int64(0)
    assert L.cis_index_remove(h, None, 5, ctypes.byref(n)) == _lib_.CIS_EINVAL
    assert L.cis_index_remove_dev(h, None, 5, ctypes.byref(n), None, None) == _lib_.CIS_EINVAL
    assert L.cis_index_sub_remote_counts(h, None) == _lib_.CIS_EINVAL
    assert L.cis_index_sub_remote_counts_dev(h, None, None) == _lib_.CIS_EINVAL


def test_negative_count_is_einval(blank_handle):
    _lib_, L = _lib()
    h, _keep = blank_handle
    ids = np.array([1], dtype=np.int64)
    n = ctypes.c_int64(0)
    assert L.cis_index_remove(h, _lib_.ptr(ids), -1, ctypes.byref(n)) == _lib_.CIS_EINVAL
    assert L.cis_index_remove_dev(h, _lib_.ptr(ids), -1, ctypes.byref(n), None, None) == _lib_.CIS_EINVAL
    # more ids than one call takes
    assert L.cis_index_remove(h, _lib_.ptr(ids), 1 << 31, ctypes.byref(n)) == _lib_.CIS_EINVAL
    assert L.cis_index_remove_dev(h, _lib_.ptr(ids), 1 << 31, ctypes.byref(n), None, None) == _lib_.CIS_EINVAL


def test_remove_ids_on_a_closed_searcher_raises():
    from columbiaimagesearch_amd.lopq import LOPQSearcherHIP
    from columbiaimagesearch_amd.lopq.search import LOPQSearcherBase
    s = object.__new__(LOPQSearcherHIP)  # what close() leaves behind: no handle
    LOPQSearcherBase.__init__(s)
    s._ix, s._slot_of, s._id_of = None, {}, []
    with pytest.raises(ValueError):
        s.remove_ids([1, 2])
    with pytest.raises(ValueError):
        s.remove_ids_dev(None)
