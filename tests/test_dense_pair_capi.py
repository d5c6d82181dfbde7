"""CPU: the dense Perron pair surface of the C-ABI - the symbols, the shape and
scratch queries and everything refused before any device work.  No GPU
needed."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from eigen_value_amd import _lib

NEW = ["st_solve_device_pair_f32", "st_solve_device_pair_f64", "max_eigen_value_pair_ex",
       "st_pair_sum_f32", "st_pair_sum_f64", "st_mfree_pair_round_f32",
       "st_mfree_pair_round_f64", "st_pair_scratch", "st_pair_shape", "st_pair_shape_desc"]
DUMMY = ctypes.c_void_p(4096)        # never dereferenced: the calls are refused first
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = [(_lib.ST_FLAG_TIME_KERNELS, "ST_FLAG_TIME_KERNELS"),
         (_lib.ST_FLAG_TRACE_SUMS, "ST_FLAG_TRACE_SUMS"),
         (_lib.ST_FLAG_ROUND_LOOP, "ST_FLAG_ROUND_LOOP"),
         (_lib.ST_FLAG_WRITE_EVERY_ROUND, "ST_FLAG_WRITE_EVERY_ROUND"),
         (_lib.ST_FLAG_BATCH_ROUNDS, "ST_FLAG_BATCH_ROUNDS")]


def test_new_symbols_are_declared_and_exported():
    declared = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = _lib.load()
    for s in NEW:
        assert s in declared and s in exported, s
        assert getattr(L, s).argtypes is not None, s


def test_version_is_unchanged_by_the_new_section():
    import eigen_value_amd
    assert eigen_value_amd.__version__ in _lib.load().st_version().decode()


def test_shape_query():
    L = _lib.load()
    rb, strip, cl, cr, lrb, lc = (ctypes.c_uint32() for _ in range(6))
    for dtype in (0, 1):
        for n in (1, 2, 2047, 2048, 4096, 16384, 131072, 2**31 - 2, 2**31 - 1):
            assert L.st_pair_shape(dtype, n, ctypes.byref(rb), ctypes.byref(strip),
                                   ctypes.byref(cl), ctypes.byref(cr)) == 0, n
            assert L.st_left_shape(dtype, n, ctypes.byref(lrb), ctypes.byref(lc)) == 0
            assert rb.value == lrb.value and cl.value == lc.value      # the left solve's
            assert strip.value == (512 if dtype else 1024) and cr.value == 0
        assert L.st_pair_shape(dtype, 5, None, None, None, None) == 0  # any may be NULL
        for n in (0, 2**31, 2**32 - 1):
            assert L.st_pair_shape(dtype, n, ctypes.byref(rb), None, None, None) < 0
            assert "n must be in [1, 2^31)" in _lib.last_error(L)
    for dtype in (2, 3, -1):
        assert L.st_pair_shape(dtype, 5, ctypes.byref(rb), None, None, None) < 0
        assert "dtype must be 0 (f32) or 1 (f64)" in _lib.last_error(L)
    sh = _lib.pair_shape(_lib.DTYPE_F32, 2049)
    assert sh["strip"] == sh["block"] * sh["w"] == 1024 and sh["nstrips"] == 3
    assert _lib.pair_shape(_lib.DTYPE_F64, 1)["w"] == 2


def test_shape_desc_fields():
    desc = dict(kv.split("=") for kv in _lib.load().st_pair_shape_desc().decode().split())
    left = dict(kv.split("=") for kv in _lib.load().st_left_shape_desc().decode().split())
    assert desc["block"] == "256" and desc["bytes_per_load"] == "16"
    assert desc["strip_cols"] == "1024,512" and desc["lds_rows"] == "256"
    assert desc["combine_left"] == "serial" == desc["combine_right"]
    assert desc["launches_per_round"] == "5"
    for key in ("rows_in_flight", "rows_per_block", "rows_from", "finish_block", "prep_grid",
                "nt_from_mib"):
        assert desc[key] == left[key], key                 # the left solve's, unchanged


def test_scratch_query():
    L = _lib.load()
    for dtype in (0, 1):
        S = 512 if dtype else 1024
        for n in (1, 2, 33, 1000, 2049, 32768, 2**31 - 1):
            rb = _lib.left_shape(dtype, n)["rows"]
            got = int(L.st_pair_scratch(dtype, n))
            up = lambda e: -(-e // 64) * 64                # noqa: E731
            nrb, ns = -(-n // rb), -(-n // S)
            assert got == 2 * up(n) + up(nrb * n) + ns * n, (dtype, n)
        for n in (0, 2**31):
            assert L.st_pair_scratch(dtype, n) == 0 and "n must be" in _lib.last_error(L)
    assert L.st_pair_scratch(2, 8) == 0 and "dtype must be" in _lib.last_error(L)
    assert L.st_pair_scratch(-1, 8) == 0 and "dtype must be" in _lib.last_error(L)


def _device(sfx, mat=DUMMY, dim=8, opt=None, wq=None, vals=True, vecs=DUMMY):
    L = _lib.load()
    ev, it = (ctypes.c_double * 2)(), (ctypes.c_uint32 * 2)()
    rc = getattr(L, f"st_solve_device_pair_{sfx}")(
        wq, mat, dim, vecs, None, ev if vals else None, it, None,
        ctypes.byref(opt) if opt is not None else None, None)
    return rc, _lib.last_error(L)


def _twin(dtype, mat, dim=None, opt=None, wq=None, vals=True):
    L = _lib.load()
    dim = (mat.shape[0] if mat is not None else 8) if dim is None else dim
    ev, it = np.zeros(2, np.float64), np.zeros(2, np.uint32)
    vec = np.zeros((2, max(dim, 1)), np.float64)
    rc = L.max_eigen_value_pair_ex(wq, dtype, None if mat is None else mat.ctypes.data,
                                   ev.ctypes.data if vals else None, vec.ctypes.data, dim,
                                   it.ctypes.data, None,
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
    rc, msg = _device(sfx, vals=False)
    assert rc == -1 and "null output pointer" in msg
    rc, msg = _device(sfx, vecs=None)
    assert rc == -1 and "eigenvector output" in msg
    rc, msg = _device(sfx)
    assert rc == -1 and "null queue" in msg                # the arguments are fine


def test_host_twin_refuses_in_its_order():
    """Flags, semantics, the matrix, dim, the outputs, the queue: each one
    reported while everything after it is wrong too."""
    a = np.ones((8, 8), np.float64)
    bad_sem = 9
    for flag, name in FLAGS:
        opt = _lib.st_options(-1.0, 0, bad_sem, 0, flag | _lib.ST_FLAG_MATRIX_FREE)
        rc, msg = _twin(1, None, dim=0, opt=opt, vals=False)
        assert rc == -1 and "not supported" in msg and name in msg and "dense pair" in msg
    opt = _lib.st_options(-1.0, 0, bad_sem, 0, _lib.ST_FLAG_MATRIX_FREE)
    rc, msg = _twin(1, None, dim=0, opt=opt, vals=False)
    assert rc == -1 and "semantics" in msg
    rc, msg = _twin(1, None, dim=0, vals=False)
    assert rc == -1 and "null matrix" in msg
    rc, msg = _twin(1, a, dim=0, vals=False)
    assert rc == -1 and "dim must be > 0" in msg
    rc, msg = _twin(1, a, vals=False)
    assert rc == -1 and "null output pointer" in msg
    rc, msg = _twin(1, a)
    assert rc == -1 and "null queue" in msg
    rc, msg = _twin(0, a.astype(np.float32), opt=_lib.st_options(-1.0, 0, 0, 0,
                                                                  _lib.ST_FLAG_MATRIX_FREE))
    assert rc == -1 and "null queue" in msg                # accepted and implied
    for dtype in (2, 3, -1):
        rc, msg = _twin(dtype, a)
        assert rc == -1 and "dtype must be 0 (f32) or 1 (f64)" in msg


@pytest.mark.parametrize("flag,name", FLAGS)
def test_unsupported_flags_are_refused_by_name(flag, name):
    opt = _lib.st_options(-1.0, 0, 0, 0, flag)
    for rc, msg in (_device("f64", opt=opt), _device("f32", opt=opt)):
        assert rc == -1 and "not supported" in msg and name in msg and "dense pair" in msg


@pytest.mark.parametrize("sfx,T", [("f32", ctypes.c_float), ("f64", ctypes.c_double)])
def test_step_level_calls_name_the_argument(sfx, T):
    L = _lib.load()
    psum, rnd = getattr(L, f"st_pair_sum_{sfx}"), getattr(L, f"st_mfree_pair_round_{sfx}")
    a, b = ctypes.c_void_p(8192), ctypes.c_void_p(12288)
    assert psum(None, a, b, DUMMY, 8, None) == -1 and "null matrix" in _lib.last_error(L)
    assert psum(DUMMY, a, b, None, 8, None) == -1 and "null scratch" in _lib.last_error(L)
    assert psum(DUMMY, a, b, DUMMY, 0, None) == -1 and "dim must be > 0" in _lib.last_error(L)
    assert psum(DUMMY, a, None, DUMMY, 8, None) == -1 and "null pointer" in _lib.last_error(L)
    assert psum(DUMMY, a, a, DUMMY, 8, None) == -1 and "must differ" in _lib.last_error(L)
    v = [ctypes.c_void_p(4096 * i) for i in range(2, 10)]
    scr, stt = ctypes.c_void_p(4096 * 12), ctypes.c_void_p(4096 * 13)

    def call(mat=DUMMY, vec=None, scratch=scr, n=8, k=1, max_itr=10, sem=0, state=stt):
        p = list(v)
        for i, q in (vec or {}).items():
            p[i] = q
        return rnd(mat, *p, scratch, n, T(1e-3), k, max_itr, sem, state, None), \
            _lib.last_error(L)

    # vectors: [s_prev, s_next, v_prev, v_cur] of the right side, then of the left
    for kwargs, word in ((dict(mat=None), "null matrix"), (dict(scratch=None), "null scratch"),
                         (dict(n=0), "dim must be > 0"), (dict(state=None), "null pointer"),
                         (dict(vec={5: None}), "null pointer"),
                         (dict(k=0), "k must be >= 1"), (dict(sem=7), "bad semantics"),
                         (dict(vec={3: v[2]}), "v_prev and v_cur must differ"),
                         (dict(vec={5: v[4]}), "s_prev and s_next must differ"),
                         (dict(vec={7: v[3]}), "two sides' outputs must differ"),
                         (dict(scratch=v[6]), "scratch of its own")):
        rc, msg = call(**kwargs)
        assert rc == -1 and word in msg, (kwargs, msg)


def test_python_fronts_check_before_any_library_call():
    from eigen_value_amd import device
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device needed for the checks
    with pytest.raises(TypeError, match="float32 or float64"):
        ev.similarity_transform_pair(np.ones((4, 4), np.float16))
    with pytest.raises(AssertionError, match="square"):
        ev.similarity_transform_pair(np.ones((4, 5), np.float32))
    sig = inspect.signature(device.DeviceSolver.solve_pair).parameters
    assert list(sig) == ["self", "mat", "eps", "max_itr", "semantics", "batch"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in sig.items()
               if n not in ("self", "mat"))
    assert "pair" not in inspect.signature(device.DeviceSolver.solve).parameters
    for name in ("pair_scratch", "pair_sum", "mfree_pair_round"):
        assert callable(getattr(device, name))


def test_the_stand_alone_program(tmp_path):
    """tests/cpp/pair_sanitize.cpp, built without the sanitizer flags (make
    pair_sanitize builds and runs it with them): every tile of every small size
    walked as the kernel's lanes walk it."""
    src = os.path.join(ROOT, "tests", "cpp", "pair_sanitize.cpp")
    exe = tmp_path / "pair_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g",
                    "-I" + os.path.join(ROOT, "eigen_value_amd", "csrc"), src, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "pair_sanitize ok" in r.stdout, r.stdout + r.stderr
