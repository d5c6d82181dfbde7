"""CPU: the C-ABI of the batched round loop (ST_FLAG_BATCH_ROUNDS,
st_solve_batched_rounds_max_dim) and the wrappers' argument checks.  No
compute calls (no GPU here)."""
import ctypes

import numpy as np
import pytest

from eigen_value_amd import _lib

NEW = "st_solve_batched_rounds_max_dim"


def test_symbol_is_declared_and_loads_in_both_builds():
    assert NEW in _lib.declared_symbols()
    assert getattr(_lib.load(), NEW) is not None
    assert getattr(_lib.load_tuning(), NEW) is not None
    assert _lib.ST_FLAG_BATCH_ROUNDS == 32
    text = open(_lib.HEADER).read()
    assert "#define ST_FLAG_BATCH_ROUNDS 32u" in text


@pytest.mark.parametrize("loader", [_lib.load, _lib.load_tuning])
def test_rounds_max_dim_is_the_last_size_below_the_flat_threshold(loader):
    L = loader()
    want = {_lib.DTYPE_F64: 4344, _lib.DTYPE_F32: 6143}
    for dtype, lim in want.items():
        got = L.st_solve_batched_rounds_max_dim(dtype)
        assert got == lim
        assert L.st_round_flat_pays(got, got, dtype) == 0
        assert L.st_round_flat_pays(got + 1, got + 1, dtype) == 1
    assert L.st_solve_batched_rounds_max_dim(7) == 0
    assert L.st_solve_batched_rounds_max_dim(-1) == 0


def test_device_wrapper_of_the_limit():
    from eigen_value_amd import device
    assert device.batched_rounds_max_dim(np.float64) == 4344
    assert device.batched_rounds_max_dim(np.float32) == 6143
    assert device.batched_rounds_max_dim("torch.float64") == 4344
    with pytest.raises(TypeError):
        device.batched_rounds_max_dim(np.int32)


def test_null_queue_with_the_flag_is_still_null_queue():
    L = _lib.load()
    m = np.ones((2, 300, 300), np.float32)
    ev, vec, it = np.zeros(2, np.float32), np.zeros((2, 300), np.float32), np.zeros(2, np.uint32)
    opt = _lib.st_options(-1.0, 0, _lib.ST_SEM_SYCL, 0, _lib.ST_FLAG_BATCH_ROUNDS)
    rc = L.max_eigen_value_batched_ex(None, _lib.DTYPE_F32, m.ctypes.data, ev.ctypes.data,
                                      vec.ctypes.data, 2, 300, it.ctypes.data,
                                      ctypes.byref(opt), None)
    assert rc < 0 and "null queue" in _lib.last_error()
    dummy = ctypes.c_void_p(4096)               # never dereferenced: rejected first
    for fn in (L.st_solve_batched_f32, L.st_solve_batched_f64):
        rc = fn(None, dummy, 2, 300, dummy, None, ev.ctypes.data, it.ctypes.data, None,
                ctypes.byref(opt), None)
        assert rc < 0 and "null queue" in _lib.last_error()


class _NoCalls:
    """Stands in for the library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument checks")


def test_wrapper_argument_checks_run_before_any_library_call():
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device needed for the checks
    ev.so_lib, ev.sycl_q = _NoCalls(), None
    with pytest.raises(AssertionError, match=r"\(B, n, n\)"):
        ev.similarity_transform_batched(np.ones((3, 3), np.float32), round_loop=True)
    with pytest.raises(AssertionError, match="square"):
        ev.similarity_transform_batched(np.ones((2, 3, 4), np.float32), round_loop="auto")
    with pytest.raises(AssertionError, match="float32"):
        ev.similarity_transform_batched(np.ones((2, 3, 3), np.int64), round_loop=True)
    for bad in ("always", 2, "AUTO", 1.0):
        with pytest.raises(ValueError, match="round_loop"):
            ev.similarity_transform_batched(np.ones((2, 3, 3), np.float32), round_loop=bad)


def test_round_loop_keyword_to_flags():
    f = _lib.batch_rounds_flag
    assert f(None, 4000, _lib.DTYPE_F64) == 0 and f(False, 4000, _lib.DTYPE_F64) == 0
    assert f(True, 4, _lib.DTYPE_F32) == _lib.ST_FLAG_BATCH_ROUNDS
    # "auto": only beyond the one-launch kernel (128 fp64 / 256 fp32)
    assert f("auto", 128, _lib.DTYPE_F64) == 0
    assert f("auto", 129, _lib.DTYPE_F64) == _lib.ST_FLAG_BATCH_ROUNDS
    assert f("auto", 256, _lib.DTYPE_F32) == 0
    assert f("auto", 257, _lib.DTYPE_F32) == _lib.ST_FLAG_BATCH_ROUNDS
    with pytest.raises(ValueError):
        f("yes", 4, _lib.DTYPE_F32)
