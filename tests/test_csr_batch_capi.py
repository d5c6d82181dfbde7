"""CPU: the batched sparse (stacked CSR) surface of the C-ABI - the symbols,
and everything the host twin and the Python fronts reject before any device
work.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from eigen_value_amd import _lib
from csr_cases import make_csr

NEW = ["st_csr_batch_create", "st_csr_batch_destroy", "st_csr_batch_get_plan",
       "st_solve_csr_batched", "max_eigen_value_csr_batched_ex", "st_csr_batch_rowsum",
       "st_csr_batch_mfree_round", "st_csr_batch_shape_desc"]
DUMMY = ctypes.c_void_p(4096)        # never dereferenced: the calls are refused first
DIMS = [(5, 3, 3), (64, 8, 7), (1, 1, 3), (30, 4, 1)]          # (n, d, seed)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stack(mats):
    """(mat_first uint32 [B + 1], row_ptr int64 [N + 1], col int32, vals)."""
    mat_first = np.concatenate([[0], np.cumsum([len(m[0]) - 1 for m in mats])]).astype(np.uint32)
    ptrs, base = [np.zeros(1, np.int64)], 0
    for ip, _, _ in mats:
        ptrs.append(ip[1:] + base)
        base += int(ip[-1])
    return (mat_first, np.concatenate(ptrs), np.concatenate([m[1] for m in mats]),
            np.concatenate([m[2] for m in mats]))


@pytest.fixture(scope="module")
def batch():
    return stack([make_csr(n, d, seed, dtype=np.float32) for n, d, seed in DIMS])


def _twin(dtype, mat_first, row_ptr, col, vals, batch=None, nnz=None, opt=None, wq=None):
    L = _lib.load()
    mat_first = np.ascontiguousarray(mat_first, np.uint32)
    row_ptr = np.ascontiguousarray(row_ptr, np.int64)
    col = np.ascontiguousarray(col, np.int32)
    b = len(mat_first) - 1 if batch is None else batch
    ev = np.zeros(max(b, 1), np.float64)
    it = np.zeros(max(b, 1), np.uint32)
    vec = np.zeros(len(row_ptr), np.float64)
    rc = L.max_eigen_value_csr_batched_ex(
        wq, dtype, b, mat_first.ctypes.data, len(vals) if nnz is None else nnz,
        row_ptr.ctypes.data, col.ctypes.data, vals.ctypes.data, ev.ctypes.data, vec.ctypes.data,
        it.ctypes.data, None, ctypes.byref(opt) if opt is not None else None, None)
    return rc, _lib.last_error(L)


def test_new_symbols_are_declared_and_exported():
    declared = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = _lib.load()
    for s in NEW:
        assert s in declared and s in exported, s
        assert getattr(L, s).argtypes is not None, s
    assert "2048 per matrix" in L.st_csr_batch_shape_desc().decode()
    assert "3d. batched sparse (CSR) solve" in open(_lib.HEADER).read()


@pytest.mark.parametrize("wq", [None, DUMMY], ids=["null-queue", "garbage-queue"])
def test_host_twin_rejects_before_any_device_work(batch, wq):
    """Every one of these is refused by host validation, which comes before
    the queue is even looked at (null or garbage alike)."""
    mf, rp, col, vals = batch
    B, N = len(mf) - 1, int(mf[-1])
    if wq is None:
        rc, msg = _twin(0, mf, rp, col, vals)
        assert rc < 0 and "null queue" in msg                   # the batch itself is fine
    for dtype in (2, 3, -1):
        rc, msg = _twin(dtype, mf, rp, col, vals, wq=wq)
        assert rc < 0 and "dtype must be 0 (f32) or 1 (f64)" in msg
    rc, msg = _twin(0, mf, rp, col, vals, batch=0, wq=wq)
    assert rc < 0 and "batch must be >= 1, got 0" in msg
    bad = mf.copy()
    bad[0] = 1
    rc, msg = _twin(0, bad, rp, col, vals, wq=wq)
    assert rc < 0 and "mat_first[0] must be 0, got 1" in msg
    for b in (0, 2, B - 1):                                     # matrix b without a row
        bad = mf.copy()
        bad[b + 1] = bad[b]
        rc, msg = _twin(0, bad, rp, col, vals, wq=wq)
        assert rc < 0 and f"mat_first does not increase at matrix {b} " in msg, msg
    bad = mf.copy()
    bad[2] = bad[1] - 1
    rc, msg = _twin(0, bad, rp, col, vals, wq=wq)
    assert rc < 0 and "mat_first does not increase at matrix 1 " in msg
    # mat_first[B] != N: N is read from mat_first, so the arrays end elsewhere
    for wrong in (N - 1, N - 7):
        bad = mf.copy()
        bad[B] = wrong
        rc, msg = _twin(0, bad, rp, col, vals, wq=wq)
        assert rc < 0 and f"matrix {B - 1}, local row" in msg and \
            "row_ptr[n] must be nnz" in msg, msg
    bad = mf.copy()
    bad[B] = 2**31
    rc, msg = _twin(0, bad, rp, col, vals, wq=wq)
    assert rc < 0 and "below 2^31" in msg
    # row_ptr: the matrix and its local row are named
    for b, lr in ((0, 2), (1, 0), (1, 63), (3, 17)):
        r = int(mf[b]) + lr
        bad = rp.copy()
        bad[r + 1] = bad[r]
        rc, msg = _twin(0, mf, bad, col, vals, wq=wq)
        assert rc < 0 and f"matrix {b}, local row {lr}: csr: row {r} is empty" in msg, msg
        bad[r + 1] = bad[r] - 1
        rc, msg = _twin(0, mf, bad, col, vals, wq=wq)
        assert rc < 0 and f"matrix {b}, local row {lr}: csr: row_ptr decreases at row {r}" in msg
    bad = rp.copy()
    bad[0] = 1
    rc, msg = _twin(0, mf, bad, col, vals, wq=wq)
    assert rc < 0 and "matrix 0, local row 0: csr: row_ptr[0] must be 0" in msg
    rc, msg = _twin(0, mf, rp, col, vals, nnz=len(vals) - 1, wq=wq)
    assert rc < 0 and "row_ptr[n] must be nnz" in msg and "matrix 3, local row 29" in msg
    # a column equal to n_b is below N for every matrix: it would couple two
    # matrices; and a column of -1
    for b, (n, d, _) in enumerate(DIMS):
        for c in (n, -1):
            for lr in (0, n - 1):
                e = int(rp[int(mf[b]) + lr])
                assert n < N
                badc = col.copy()
                badc[e] = c
                rc, msg = _twin(0, mf, rp, badc, vals, wq=wq)
                assert rc < 0 and (f"column index {c} of entry {e} (matrix {b}, local row {lr}) "
                                   f"is outside [0, {n})") in msg, msg
    # row_ptr is judged on its own first: a bad column is not even looked at
    badc = col.copy()
    badc[0] = 99
    bad = rp.copy()
    bad[7] = bad[6]
    rc, msg = _twin(0, mf, bad, badc, vals, wq=wq)
    assert rc < 0 and "matrix 1, local row 1" in msg and "is empty" in msg


@pytest.mark.parametrize("flag", [_lib.ST_FLAG_TIME_KERNELS, _lib.ST_FLAG_TRACE_SUMS,
                                  _lib.ST_FLAG_ROUND_LOOP, _lib.ST_FLAG_WRITE_EVERY_ROUND,
                                  _lib.ST_FLAG_BATCH_ROUNDS])
def test_unsupported_flags(batch, flag):
    mf, rp, col, vals = batch
    opt = _lib.st_options(-1.0, 0, 0, 0, flag | _lib.ST_FLAG_MATRIX_FREE)
    for wq in (None, DUMMY):
        rc, msg = _twin(0, mf, rp, col, vals, opt=opt, wq=wq)
        assert rc < 0 and "not supported" in msg
    ok = _lib.st_options(-1.0, 0, 0, 0, _lib.ST_FLAG_MATRIX_FREE)
    rc, msg = _twin(0, mf, rp, col, vals, opt=ok)
    assert rc < 0 and "null queue" in msg                       # accepted; only the queue is missing
    bad = _lib.st_options(-1.0, 0, 9, 0, 0)
    rc, msg = _twin(0, mf, rp, col, vals, opt=bad)
    assert rc < 0 and "semantics" in msg


def test_handle_calls_reject_what_is_no_handle():
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)                      # zeros: no magic
    single = ctypes.create_string_buffer(256)
    ctypes.memmove(single, ctypes.byref(ctypes.c_uint32(0x43535231)), 4)   # a st_csr_create handle's
    for h in (None, buf, single):
        assert L.st_csr_batch_rowsum(h, DUMMY, None) < 0 and "batch handle" in _lib.last_error(L)
        assert L.st_csr_batch_mfree_round(h, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 1e-3, 1, 10, 0,
                                          DUMMY, DUMMY, None) < 0
        assert "batch handle" in _lib.last_error(L)
        assert L.st_csr_batch_get_plan(h, None, None) < 0
        ev, it = ctypes.c_double(), ctypes.c_uint32()
        assert L.st_solve_csr_batched(DUMMY, h, DUMMY, None, ctypes.byref(ev), ctypes.byref(it),
                                      None, None, None) < 0
        assert "batch handle" in _lib.last_error(L)
    assert L.st_csr_batch_destroy(single) < 0 and "batch handle" in _lib.last_error(L)
    # and the other way round: a batch handle's first word is no CSR matrix handle
    fake = ctypes.create_string_buffer(256)
    ctypes.memmove(fake, ctypes.byref(ctypes.c_uint32(0x43535242)), 4)
    assert L.st_csr_rowsum(fake, DUMMY, None) < 0 and "handle" in _lib.last_error(L)
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    assert L.st_solve_csr(DUMMY, fake, DUMMY, None, ctypes.byref(ev), ctypes.byref(it), None,
                          None) < 0 and "handle" in _lib.last_error(L)
    assert L.st_csr_destroy(fake) < 0
    assert L.st_csr_batch_destroy(None) == 0
    out = ctypes.c_void_p(1)
    mf = np.array([0, 4], np.uint32)
    assert L.st_csr_batch_create(None, 0, 1, mf.ctypes.data, 4, DUMMY, DUMMY, DUMMY,
                                 ctypes.byref(out)) < 0
    assert "null queue" in _lib.last_error(L) and not out.value


def test_python_fronts_check_before_any_library_call():
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device, no library handle: checks only
    a = make_csr(64, 8, 7)
    b = make_csr(5, 3, 3)
    with pytest.raises(AssertionError, match="one dtype"):
        ev.similarity_transform_csr_batched([a, (b[0], b[1], b[2].astype(np.float32))])
    with pytest.raises(AssertionError, match="float32 or float64"):
        ev.similarity_transform_csr_batched([(b[0], b[1], b[2].astype(np.float16))])
    with pytest.raises(AssertionError, match="one length"):
        ev.similarity_transform_csr_batched([a, (b[0], b[1][:-1], b[2])])
    with pytest.raises(AssertionError, match="triple"):
        ev.similarity_transform_csr_batched([a, (b[0], b[1])])
    with pytest.raises(AssertionError, match="n \\+ 1"):
        ev.similarity_transform_csr_batched([(b[0][:1], b[1], b[2])])
    with pytest.raises(TypeError, match="sparse matrices"):
        ev.similarity_transform_csr_batched([np.ones((3, 3))])
    lam, vs, ts, its = ev.similarity_transform_csr_batched([])     # empty: allowed, no call
    assert lam.shape == (0,) and vs == [] and ts == 0 and its.shape == (0,)


def test_python_front_refuses_a_rectangular_scipy_matrix():
    sp = pytest.importorskip("scipy.sparse")     # the scipy form is optional, as in test_csr_capi
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)
    with pytest.raises(AssertionError, match="square"):
        ev.similarity_transform_csr_batched([sp.csr_matrix(np.ones((3, 4)))])


def test_device_fronts_check_their_arguments():
    from eigen_value_amd import device as dev
    with pytest.raises(TypeError, match="CsrBatch required"):
        dev.DeviceSolver.solve_csr_batched(object.__new__(dev.DeviceSolver), "no batch")
    with pytest.raises(ValueError, match="at least one matrix"):
        dev.CsrBatch.from_matrices([])
    with pytest.raises(TypeError, match="triples or torch.sparse_csr"):
        dev.CsrBatch.from_matrices([np.ones((2, 2))])


def test_host_validation_program_builds_and_passes(tmp_path):
    """tests/cpp/csr_batch_sanitize.cpp without the sanitizers (those are run
    by hand on the stand-alone program: see its header).  Any host C++
    compiler will do; the one the library's own build brings is the last
    resort, so the test never lacks one where the library was built."""
    cxx = (shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
           or "/opt/rocm/lib/llvm/bin/clang++")
    exe = tmp_path / "csr_batch_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "eigen_value_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "csr_batch_sanitize.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr
