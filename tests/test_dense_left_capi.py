"""CPU: the dense left-vector surface of the C-ABI - the symbols, the shape and
scratch queries and everything refused before any device work.  No GPU
needed."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from eigen_value_amd import _lib

NEW = ["st_solve_device_left_f32", "st_solve_device_left_f64", "max_eigen_value_left_ex",
       "st_colsum_f32", "st_colsum_f64", "st_mfree_left_round_f32", "st_mfree_left_round_f64",
       "st_left_scratch", "st_left_shape", "st_left_shape_desc"]
DUMMY = ctypes.c_void_p(4096)        # never dereferenced: the calls are refused first
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_and_exported():
    declared = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = _lib.load()
    for s in NEW:
        assert s in declared and s in exported, s
        assert getattr(L, s).argtypes is not None, s
    desc = L.st_left_shape_desc().decode()
    assert desc.startswith("block=") and "combine=serial" in desc


def test_version_is_unchanged_by_the_new_section():
    import eigen_value_amd
    assert eigen_value_amd.__version__ in _lib.load().st_version().decode()


def test_shape_query():
    L = _lib.load()
    rb, comb = ctypes.c_uint32(), ctypes.c_uint32()
    for dtype in (0, 1):
        last = 0
        for n in (1, 2, 2047, 2048, 4096, 16384, 131072, 2**31 - 2, 2**31 - 1):
            assert L.st_left_shape(dtype, n, ctypes.byref(rb), ctypes.byref(comb)) == 0, n
            assert 1 <= rb.value <= 65536 and rb.value >= last and comb.value in (0, 1)
            last = rb.value
        assert L.st_left_shape(dtype, 5, None, None) == 0          # either may be NULL
        for n in (0, 2**31, 2**32 - 1):
            assert L.st_left_shape(dtype, n, ctypes.byref(rb), ctypes.byref(comb)) < 0
            assert "n must be in [1, 2^31)" in _lib.last_error(L)
    for dtype in (2, 3, -1):
        assert L.st_left_shape(dtype, 5, ctypes.byref(rb), ctypes.byref(comb)) < 0
        assert "dtype must be 0 (f32) or 1 (f64)" in _lib.last_error(L)
    sh = _lib.left_shape(_lib.DTYPE_F32, 1)
    assert sh["strip"] == sh["block"] * 4 and _lib.left_shape(_lib.DTYPE_F64, 1)["w"] == 2


def test_scratch_query():
    L = _lib.load()
    for dtype in (0, 1):
        for n in (1, 2, 33, 1000, 2049, 32768, 2**31 - 1):
            rb = _lib.left_shape(dtype, n)["rows"]
            got = int(L.st_left_scratch(dtype, n))
            nrb = -(-n // rb)
            assert got == -(-n // 64) * 64 + nrb * n, (dtype, n)   # x (rounded), the partials
            assert got >= 2 * n
        for n in (0, 2**31):
            assert L.st_left_scratch(dtype, n) == 0 and "n must be" in _lib.last_error(L)
    assert L.st_left_scratch(2, 8) == 0 and "dtype must be" in _lib.last_error(L)
    assert L.st_left_scratch(-1, 8) == 0 and "dtype must be" in _lib.last_error(L)


def _device(sfx, mat=DUMMY, dim=8, opt=None, wq=None):
    L = _lib.load()
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    rc = getattr(L, f"st_solve_device_left_{sfx}")(
        wq, mat, dim, DUMMY, None, ctypes.byref(ev), ctypes.byref(it),
        ctypes.byref(opt) if opt is not None else None, None)
    return rc, _lib.last_error(L)


def _twin(dtype, mat, dim=None, opt=None, wq=None):
    L = _lib.load()
    dim = (mat.shape[0] if mat is not None else 8) if dim is None else dim
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    vec = np.zeros(max(dim, 1), np.float64)
    rc = L.max_eigen_value_left_ex(wq, dtype, None if mat is None else mat.ctypes.data,
                                   ctypes.byref(ev), vec.ctypes.data, dim, ctypes.byref(it),
                                   ctypes.byref(opt) if opt is not None else None, None)
    return rc, _lib.last_error(L)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_device_solve_rejects_before_any_device_work(sfx):
    rc, msg = _device(sfx, mat=None)
    assert rc == -1 and "null matrix" in msg
    rc, msg = _device(sfx, dim=0)
    assert rc == -1 and "dim must be > 0" in msg
    rc, msg = _device(sfx, mat=ctypes.c_void_p(4097))
    assert rc == -1 and "not aligned" in msg
    rc, msg = _device(sfx)
    assert rc == -1 and "null queue" in msg                # the arguments are fine


def test_host_twin_rejects_before_any_device_work():
    a = np.ones((8, 8), np.float32)
    rc, msg = _twin(0, None)
    assert rc == -1 and "null matrix" in msg
    rc, msg = _twin(0, a, dim=0)
    assert rc == -1 and "dim must be > 0" in msg
    for dtype in (2, 3, -1):
        rc, msg = _twin(dtype, a)
        assert rc == -1 and "dtype must be 0 (f32) or 1 (f64)" in msg
    rc, msg = _twin(0, a)
    assert rc == -1 and "null queue" in msg
    rc, msg = _twin(1, a.astype(np.float64), opt=_lib.st_options(-1.0, 0, 9, 0, 0))
    assert rc == -1 and "semantics" in msg


@pytest.mark.parametrize("flag,name", [(_lib.ST_FLAG_ROUND_LOOP, "ST_FLAG_ROUND_LOOP"),
                                       (_lib.ST_FLAG_WRITE_EVERY_ROUND,
                                        "ST_FLAG_WRITE_EVERY_ROUND"),
                                       (_lib.ST_FLAG_BATCH_ROUNDS, "ST_FLAG_BATCH_ROUNDS")])
def test_flags_of_the_writing_forms_are_refused_by_name(flag, name):
    opt = _lib.st_options(-1.0, 0, 0, 0, flag | _lib.ST_FLAG_MATRIX_FREE)
    a = np.ones((8, 8), np.float64)
    for rc, msg in (_twin(1, a, opt=opt), _device("f64", opt=opt), _device("f32", opt=opt)):
        assert rc == -1 and "not supported" in msg and name in msg and "dense left" in msg
    ok = _lib.st_options(-1.0, 0, 0, 0, _lib.ST_FLAG_MATRIX_FREE | _lib.ST_FLAG_TIME_KERNELS
                         | _lib.ST_FLAG_TRACE_SUMS)
    rc, msg = _twin(1, a, opt=ok)
    assert rc == -1 and "null queue" in msg                # accepted; only the queue is missing


@pytest.mark.parametrize("sfx,T", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_step_level_calls_name_the_argument(sfx, T):
    L = _lib.load()
    col, rnd = getattr(L, f"st_colsum_{sfx}"), getattr(L, f"st_mfree_left_round_{sfx}")
    assert col(None, DUMMY, DUMMY, 8, None) == -1 and "null matrix" in _lib.last_error(L)
    assert col(DUMMY, DUMMY, None, 8, None) == -1 and "null scratch" in _lib.last_error(L)
    assert col(DUMMY, DUMMY, DUMMY, 0, None) == -1 and "dim must be > 0" in _lib.last_error(L)
    a, b, c, d = (ctypes.c_void_p(4096 * i) for i in range(2, 6))
    scr, stt = ctypes.c_void_p(4096 * 8), ctypes.c_void_p(4096 * 9)

    def call(mat=DUMMY, s_prev=a, s_next=b, v_prev=c, v_cur=d, scratch=scr, n=8, k=1,
             max_itr=10, sem=0, state=stt):
        return rnd(mat, s_prev, s_next, v_prev, v_cur, scratch, n, T(1e-3), k, max_itr, sem,
                   state, None), _lib.last_error(L)

    for kwargs, word in ((dict(mat=None), "null matrix"), (dict(scratch=None), "null scratch"),
                         (dict(n=0), "dim must be > 0"), (dict(state=None), "null pointer"),
                         (dict(k=0), "k must be >= 1"), (dict(sem=7), "bad semantics"),
                         (dict(v_cur=c), "v_prev and v_cur must differ"),
                         (dict(s_next=a), "s_prev and s_next must differ"),
                         (dict(scratch=a), "scratch of its own")):
        rc, msg = call(**kwargs)
        assert rc == -1 and word in msg, (kwargs, msg)


def test_python_fronts_check_before_any_library_call():
    from eigen_value_amd import device
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device needed for the checks
    with pytest.raises(TypeError, match="float32 or float64"):
        ev.similarity_transform_left(np.ones((4, 4), np.float16))
    with pytest.raises(AssertionError, match="square"):
        ev.similarity_transform_left(np.ones((4, 5), np.float32))
    # the drop-in call keeps the reference's signature
    assert list(inspect.signature(EigenValue.similarity_transform).parameters) == ["self", "mat"]
    sig = inspect.signature(device.DeviceSolver.solve).parameters
    assert sig["left"].default is False and sig["left"].kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("solve_half", "solve_batched", "solve_vbatched"):
        assert "left" not in inspect.signature(getattr(device.DeviceSolver, name)).parameters


def test_the_stand_alone_program(tmp_path):
    """tests/cpp/left_sanitize.cpp, built without the sanitizer flags (make
    left_sanitize builds and runs it with them): the shape, scratch, grid and
    staging arithmetic the library's table also answers with."""
    src = os.path.join(ROOT, "tests", "cpp", "left_sanitize.cpp")
    exe = tmp_path / "left_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g",
                    "-I" + os.path.join(ROOT, "eigen_value_amd", "csrc"), src, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "left_sanitize ok" in r.stdout, r.stdout + r.stderr
