"""CPU: the sparse (CSR) surface of the C-ABI - the class table, the plan and
everything the host twin rejects before any device work.  No GPU needed."""
import ctypes
import subprocess

import numpy as np
import pytest

from eigen_value_amd import _lib
from csr_cases import TABLE, class_heavy, make_csr

NEW = ["st_csr_class_limits", "st_csr_plan", "st_csr_shape_desc", "st_csr_create",
       "st_csr_destroy", "st_csr_get_plan", "st_solve_csr", "max_eigen_value_csr_ex",
       "st_csr_rowsum", "st_csr_mfree_round"]
DUMMY = ctypes.c_void_p(4096)        # never dereferenced: the calls are refused first


def test_new_symbols_are_declared_and_exported():
    declared = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = _lib.load()
    for s in NEW:
        assert s in declared and s in exported, s
        assert getattr(L, s).argtypes is not None, s
    assert L.st_csr_shape_desc().decode().startswith("lanes=")
    assert "#define ST_CSR_CLASSES 4" in open(_lib.HEADER).read()
    assert _lib.ST_CSR_CLASSES == 4


def test_class_limits():
    nnz_max, lanes = _lib.csr_class_limits(_lib.DTYPE_F32)
    nnz64, lanes64 = _lib.csr_class_limits(_lib.DTYPE_F64)
    assert list(nnz_max) == list(nnz64) and list(lanes) == list(lanes64)
    assert list(lanes) == [4, 16, 64, 256]               # a quad .. a workgroup
    assert all(a < b for a, b in zip(nnz_max, nnz_max[1:])) and nnz_max[-1] == 2**32 - 1
    L = _lib.load()
    assert L.st_csr_class_limits(2, None, None, 0) < 0 and "dtype" in _lib.last_error(L)
    two = np.zeros(4, np.uint32)
    assert L.st_csr_class_limits(0, two.ctypes.data, None, 2) == 4      # cap respected
    assert list(two) == [nnz_max[0], nnz_max[1], 0, 0]


def _class_of(k, nnz_max):
    return int(np.searchsorted(nnz_max.astype(np.int64), k, side="left"))


def test_plan_partitions_by_class_and_is_stable():
    nnz_max, _ = _lib.csr_class_limits()
    lens = [1]
    for m in nnz_max[:-1]:
        lens += [int(m) - 1, int(m), int(m) + 1, int(m), int(m) + 1]   # at and one above
    rng = np.random.default_rng(3)
    lens += [int(x) for x in rng.integers(1, 3000, size=500)]
    lens = np.array(lens, dtype=np.int64)
    rng.shuffle(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)])
    order, first, used = _lib.csr_plan(row_ptr)
    n = len(lens)
    assert sorted(order.tolist()) == list(range(n))                    # a permutation
    assert first[0] == 0 and first[-1] == n and list(first) == sorted(first)
    want = np.array([_class_of(k, nnz_max) for k in lens])
    for c in range(4):
        rows = order[first[c]:first[c + 1]]
        assert (want[rows] == c).all(), c                              # the class its nnz demands
        assert list(rows) == sorted(rows), c                           # row order kept
        assert len(rows) == (want == c).sum()
    assert used == len(set(want.tolist()))
    for m in nnz_max[:-1]:                                             # exactly at / above
        assert _class_of(int(m), nnz_max) + 1 == _class_of(int(m) + 1, nnz_max)


@pytest.mark.parametrize("case", range(len(TABLE)))
def test_plan_of_the_table_matrices(case):
    n, d, seed, heavy = TABLE[case]
    indptr, _, _ = make_csr(n, d, seed, class_heavy() if heavy else None)
    nnz_max, _ = _lib.csr_class_limits()
    order, first, used = _lib.csr_plan(indptr)
    lens = np.diff(indptr)
    for c in range(4):
        rows = order[first[c]:first[c + 1]]
        assert all(_class_of(int(lens[r]), nnz_max) == c for r in rows)
    assert used == (4 if heavy else 1)


def test_plan_errors_name_the_row():
    L = _lib.load()
    with pytest.raises(_lib.EigenValueError, match=r"row 2 is empty"):
        _lib.csr_plan([0, 3, 5, 5, 9])
    with pytest.raises(_lib.EigenValueError, match=r"decreases at row 1"):
        _lib.csr_plan([0, 3, 2, 5])
    with pytest.raises(_lib.EigenValueError, match=r"row_ptr\[0\] must be 0"):
        _lib.csr_plan([1, 3, 5])
    o = np.zeros(4, np.uint32)
    assert L.st_csr_plan(None, 3, o.ctypes.data, o.ctypes.data) < 0
    assert "null" in _lib.last_error(L)
    rp = np.array([0], np.int64)
    assert L.st_csr_plan(rp.ctypes.data, 0, o.ctypes.data, o.ctypes.data) < 0
    assert "n must be" in _lib.last_error(L)


def _twin(dtype, indptr, indices, data, n=None, nnz=None, opt=None, wq=None):
    L = _lib.load()
    indptr = np.ascontiguousarray(indptr, np.int64)
    indices = np.ascontiguousarray(indices, np.int32)
    n = len(indptr) - 1 if n is None else n
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    vec = np.zeros(n, np.float64)
    rc = L.max_eigen_value_csr_ex(wq, dtype, n, len(data) if nnz is None else nnz,
                                  indptr.ctypes.data, indices.ctypes.data, data.ctypes.data,
                                  ctypes.byref(ev), vec.ctypes.data, ctypes.byref(it),
                                  ctypes.byref(opt) if opt is not None else None, None)
    return rc, _lib.last_error(L)


def test_host_twin_rejects_before_any_device_work():
    """Null queue throughout: every one of these is refused by host validation,
    which comes first; a valid matrix then fails on the queue."""
    indptr, indices, data = make_csr(64, 8, 7)
    data = data.astype(np.float32)
    rc, msg = _twin(0, indptr, indices, data)
    assert rc < 0 and "null queue" in msg                       # the matrix itself is fine
    bad = indptr.copy()
    bad[0] = 1
    rc, msg = _twin(0, bad, indices, data)
    assert rc < 0 and "row_ptr[0] must be 0" in msg
    rc, msg = _twin(0, indptr, indices, data, nnz=len(data) - 1)
    assert rc < 0 and "row_ptr[n] must be nnz" in msg and "row 63" in msg
    bad = indptr.copy()
    bad[10] = bad[9]
    rc, msg = _twin(0, bad, indices, data)
    assert rc < 0 and "row 9 is empty" in msg
    bad = indptr.copy()
    bad[10] = bad[9] - 1
    rc, msg = _twin(0, bad, indices, data)
    assert rc < 0 and "decreases at row 9" in msg
    for col in (64, -1):
        badc = indices.copy()
        badc[8 * 5 + 3] = col
        rc, msg = _twin(0, indptr, badc, data)
        assert rc < 0 and f"column index {col} of entry 43 (row 5)" in msg, msg
    # row_ptr is judged on its own first: a bad column is not even looked at
    badc = indices.copy()
    badc[0] = 99
    bad = indptr.copy()
    bad[3] = bad[2]
    rc, msg = _twin(0, bad, badc, data)
    assert rc < 0 and "row 2 is empty" in msg
    for dtype in (2, 3, -1):
        rc, msg = _twin(dtype, indptr, indices, data)
        assert rc < 0 and "dtype must be 0 (f32) or 1 (f64)" in msg
    rc, msg = _twin(0, indptr, indices, data, n=0)
    assert rc < 0 and "n must be" in msg


@pytest.mark.parametrize("flag", [_lib.ST_FLAG_ROUND_LOOP, _lib.ST_FLAG_WRITE_EVERY_ROUND,
                                  _lib.ST_FLAG_BATCH_ROUNDS])
def test_flags_of_the_writing_forms_are_not_supported(flag):
    indptr, indices, data = make_csr(64, 8, 7)
    opt = _lib.st_options(-1.0, 0, 0, 0, flag | _lib.ST_FLAG_MATRIX_FREE)
    rc, msg = _twin(1, indptr, indices, data, opt=opt)
    assert rc < 0 and "not supported" in msg
    ok = _lib.st_options(-1.0, 0, 0, 0, _lib.ST_FLAG_MATRIX_FREE | _lib.ST_FLAG_TIME_KERNELS
                         | _lib.ST_FLAG_TRACE_SUMS)
    rc, msg = _twin(1, indptr, indices, data, opt=ok)
    assert rc < 0 and "null queue" in msg                       # accepted; only the queue is missing
    bad = _lib.st_options(-1.0, 0, 9, 0, 0)
    rc, msg = _twin(1, indptr, indices, data, opt=bad)
    assert rc < 0 and "semantics" in msg


def test_handle_calls_reject_what_is_no_handle():
    L = _lib.load()
    assert L.st_csr_rowsum(None, DUMMY, None) < 0 and "handle" in _lib.last_error(L)
    buf = ctypes.create_string_buffer(128)                      # zeros: no magic
    assert L.st_csr_rowsum(buf, DUMMY, None) < 0 and "handle" in _lib.last_error(L)
    assert L.st_csr_mfree_round(buf, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 1e-3, 1, 10, 0, DUMMY,
                                None) < 0
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    assert L.st_solve_csr(DUMMY, buf, DUMMY, None, ctypes.byref(ev), ctypes.byref(it), None,
                          None) < 0 and "handle" in _lib.last_error(L)
    assert L.st_csr_destroy(None) == 0
    out = ctypes.c_void_p(1)
    assert L.st_csr_create(None, 0, 4, 4, DUMMY, DUMMY, DUMMY, ctypes.byref(out)) < 0
    assert "null queue" in _lib.last_error(L) and not out.value


def test_python_fronts_check_before_any_library_call():
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device needed for the checks
    indptr, indices, data = make_csr(64, 8, 7)
    with pytest.raises(AssertionError, match="float32 or float64"):
        ev.similarity_transform_csr(indptr, indices, data.astype(np.float16))
    with pytest.raises(AssertionError, match="n \\+ 1"):
        ev.similarity_transform_csr(indptr, indices, data, n=65)
    with pytest.raises(TypeError, match="sparse matrix"):
        ev.similarity_transform_csr(np.ones((3, 3)))
    # the dense calls keep rejecting sparse input as before
    sp = pytest.importorskip("scipy.sparse")
    m = sp.csr_matrix((data, indices, indptr), shape=(64, 64))
    with pytest.raises(Exception):
        ev.similarity_transform(m)
    with pytest.raises(Exception):
        ev.similarity_transform_ex(m)
