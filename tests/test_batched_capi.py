"""CPU: the batched solve's C-ABI (declared, exported, argument errors) and
the host wrapper's argument checks.  No compute calls (no GPU here)."""
import ctypes

import numpy as np
import pytest

from eigen_value_amd import _lib

BATCHED = ("st_solve_batched_f32", "st_solve_batched_f64", "max_eigen_value_batched_ex",
           "st_solve_batched_max_dim")


def test_batched_symbols_are_declared_and_load():
    declared = _lib.declared_symbols()
    L = _lib.load()
    for s in BATCHED:
        assert s in declared, s
        assert getattr(L, s) is not None
    LT = _lib.load_tuning()                     # the tuning build: same sources
    for s in BATCHED:
        assert getattr(LT, s) is not None


def test_batched_max_dim():
    L = _lib.load()
    assert L.st_solve_batched_max_dim(_lib.DTYPE_F32) == 256
    assert L.st_solve_batched_max_dim(_lib.DTYPE_F64) == 128
    assert L.st_solve_batched_max_dim(7) == 0
    from eigen_value_amd import device
    assert device.batched_max_dim(np.float32) == 256 and device.batched_max_dim(np.float64) == 128
    with pytest.raises(TypeError):
        device.batched_max_dim(np.int32)


def test_batched_null_queue_is_an_error():
    L = _lib.load()
    m = np.ones((2, 4, 4), np.float32)
    ev, vec, it = np.zeros(2, np.float32), np.zeros((2, 4), np.float32), np.zeros(2, np.uint32)
    rc = L.max_eigen_value_batched_ex(None, _lib.DTYPE_F32, m.ctypes.data, ev.ctypes.data,
                                      vec.ctypes.data, 2, 4, it.ctypes.data, None, None)
    assert rc < 0 and "null queue" in _lib.last_error()
    dummy = ctypes.c_void_p(4096)               # never dereferenced: rejected first
    for fn in (L.st_solve_batched_f32, L.st_solve_batched_f64):
        rc = fn(None, dummy, 2, 4, dummy, None, ev.ctypes.data, it.ctypes.data, None, None, None)
        assert rc < 0 and "null queue" in _lib.last_error()
    rc = L.max_eigen_value_batched_ex(None, 5, m.ctypes.data, ev.ctypes.data, vec.ctypes.data,
                                      2, 4, it.ctypes.data, None, None)
    assert rc < 0 and "dtype" in _lib.last_error()


def test_batched_wrapper_argument_checks():
    # shape and dtype asserted before any library call, as in
    # similarity_transform
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device needed for the checks
    with pytest.raises(AssertionError, match=r"\(B, n, n\)"):
        ev.similarity_transform_batched(np.ones((3, 3), np.float32))
    with pytest.raises(AssertionError, match="square"):
        ev.similarity_transform_batched(np.ones((2, 3, 4), np.float32))
    with pytest.raises(AssertionError, match="float32"):
        ev.similarity_transform_batched(np.ones((2, 3, 3), np.int64))
