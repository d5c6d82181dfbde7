"""CPU: the variable-size batched solve's C-ABI (declared, exported, argument
errors), its size-class plan (pure host code) and the wrappers' argument
checks.  No compute calls (no GPU here)."""
import ctypes

import numpy as np
import pytest

from eigen_value_amd import _lib

VBATCHED = ("st_solve_vbatched_f32", "st_solve_vbatched_f64", "max_eigen_value_vbatched_ex",
            "st_vbatched_plan")
# upper bound of each class; the last one fp32 only
LIMITS = (4, 8, 16, 32, 64, 128, 256)
DIMS_F64 = [128, 1, 5, 4, 64, 65, 17, 16, 33, 9, 8, 32, 2]
DIMS_F32 = DIMS_F64 + [129, 256]


def test_vbatched_symbols_are_declared_and_load():
    declared = _lib.declared_symbols()
    L = _lib.load()
    for s in VBATCHED:
        assert s in declared, s
        assert getattr(L, s) is not None
    LT = _lib.load_tuning()                     # the tuning build: same sources
    for s in VBATCHED:
        assert getattr(LT, s) is not None
    # the tuning ABI itself did not grow
    assert len(_lib.declared_symbols(_lib.TUNING_HEADER)) == 11
    assert _lib.ST_VBATCH_CLASSES == len(LIMITS) == 7
    assert "#define ST_VBATCH_CLASSES 7" in open(_lib.HEADER).read()


def class_of(n):
    return next(k for k, lim in enumerate(LIMITS) if n <= lim)


@pytest.mark.parametrize("dtype,dims", [(_lib.DTYPE_F64, DIMS_F64), (_lib.DTYPE_F32, DIMS_F32)])
def test_vbatched_plan(dtype, dims):
    order, first, used = _lib.vbatched_plan(dims, dtype)
    order, first = [int(x) for x in order], [int(x) for x in first]
    assert sorted(order) == list(range(len(dims)))              # a permutation
    assert first[0] == 0 and first[-1] == len(dims) and len(first) == 8
    assert all(first[k] <= first[k + 1] for k in range(7))      # monotone
    lo = 0
    for k, lim in enumerate(LIMITS):
        members = order[first[k]:first[k + 1]]
        want = [b for b, n in enumerate(dims) if lo < n <= lim]  # input order: stable
        assert members == want, (k, members, want)
        assert all(class_of(dims[b]) == k for b in members)
        lo = lim
    nonempty = sum(1 for k in range(7) if first[k + 1] > first[k])
    assert used == nonempty == (7 if dtype == _lib.DTYPE_F32 else 6)
    if dtype == _lib.DTYPE_F64:
        assert first[6] == first[7]                             # the empty class: equal bounds


def test_vbatched_plan_edges():
    # one class only, and an empty batch
    order, first, used = _lib.vbatched_plan([9, 16, 10], _lib.DTYPE_F64)
    assert list(order) == [0, 1, 2] and used == 1
    assert list(first) == [0, 0, 0, 3, 3, 3, 3, 3]
    order, first, used = _lib.vbatched_plan([], _lib.DTYPE_F32)
    assert len(order) == 0 and used == 0 and list(first) == [0] * 8


@pytest.mark.parametrize("dtype,dims,idx,dim", [
    (_lib.DTYPE_F64, [3, 0, 5], 1, 0),
    (_lib.DTYPE_F32, [0], 0, 0),
    (_lib.DTYPE_F64, [128, 4, 129, 7], 2, 129),
    (_lib.DTYPE_F32, [256, 256, 8, 257], 3, 257)])
def test_vbatched_plan_rejects_bad_dims(dtype, dims, idx, dim):
    with pytest.raises(_lib.EigenValueError) as e:
        _lib.vbatched_plan(dims, dtype)
    msg = str(e.value)
    assert f"dims[{idx}]" in msg and f"= {dim}" in msg, msg


def test_vbatched_plan_rejects_bad_dtype_and_null():
    with pytest.raises(_lib.EigenValueError, match="dtype"):
        _lib.vbatched_plan([4, 5], 7)
    L = _lib.load()
    dims = np.array([4, 5], np.uint32)
    order = np.zeros(2, np.uint32)
    assert L.st_vbatched_plan(_lib.DTYPE_F32, dims.ctypes.data, 2, order.ctypes.data, None) < 0
    assert "null" in _lib.last_error()
    first = np.zeros(8, np.uint32)
    assert L.st_vbatched_plan(_lib.DTYPE_F32, None, 2, order.ctypes.data, first.ctypes.data) < 0
    assert "null" in _lib.last_error()


def test_vbatched_null_queue_is_an_error():
    L = _lib.load()
    dims = np.array([4, 3], np.uint32)
    m = np.ones(25, np.float32)
    ev, vec, it = np.zeros(2, np.float32), np.zeros(7, np.float32), np.zeros(2, np.uint32)
    rc = L.max_eigen_value_vbatched_ex(None, _lib.DTYPE_F32, m.ctypes.data, dims.ctypes.data, 2,
                                       ev.ctypes.data, vec.ctypes.data, it.ctypes.data, None, None)
    assert rc < 0 and "null queue" in _lib.last_error()
    ptrs = (ctypes.c_void_p * 2)(4096, 8192)     # never dereferenced: rejected first
    dummy = ctypes.c_void_p(4096)
    for fn in (L.st_solve_vbatched_f32, L.st_solve_vbatched_f64):
        rc = fn(None, ptrs, dims.ctypes.data, 2, dummy, None, ev.ctypes.data, it.ctypes.data,
                None, None, None)
        assert rc < 0 and "null queue" in _lib.last_error()
    rc = L.max_eigen_value_vbatched_ex(None, 5, m.ctypes.data, dims.ctypes.data, 2,
                                       ev.ctypes.data, vec.ctypes.data, it.ctypes.data, None, None)
    assert rc < 0 and "dtype" in _lib.last_error()


def test_vbatched_wrapper_argument_checks():
    # shape and dtype asserted before any library call, as in
    # similarity_transform_batched
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device needed for the checks
    with pytest.raises(AssertionError, match="square"):
        ev.similarity_transform_vbatched([np.ones((3, 3), np.float32), np.ones((3, 4), np.float32)])
    with pytest.raises(AssertionError, match="square"):
        ev.similarity_transform_vbatched([np.ones((2, 3, 3), np.float32)])
    with pytest.raises(AssertionError, match="one dtype"):
        ev.similarity_transform_vbatched([np.ones((3, 3), np.float32), np.ones((2, 2), np.float64)])
    with pytest.raises(AssertionError, match="float32"):
        ev.similarity_transform_vbatched([np.ones((3, 3), np.int64), np.ones((2, 2), np.int64)])
    from eigen_value_amd import device
    assert callable(device.DeviceSolver.solve_vbatched)
