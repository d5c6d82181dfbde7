"""CPU: the transposed-CSR surface of the C-ABI - the host twin of the device
transposition against its numpy definition, everything it rejects, and the
stand-alone program over st_csr_host.h.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from eigen_value_amd import _lib
from eigen_value_amd import device as dev
from csr_cases import TABLE, class_heavy, make_csr, write_bin

NEW = ["st_csr_transpose_host", "st_csr_transpose", "st_csr_transpose_scratch_bytes",
       "st_csr_transpose_shape_desc", "max_eigen_value_csr_left_ex"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = ctypes.c_void_p(4096)        # never dereferenced: the calls are refused first


def definition(indptr, indices, data):
    """T(A) as the issue defines it: a stable argsort of the columns."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int32)
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr))
    p = np.argsort(indices, kind="stable")
    t_ptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=n))]).astype(np.int64)
    return t_ptr, rows[p], np.asarray(data)[p]


def same(got, want):
    return all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def table_case(case, dtype=np.float64):
    n, d, seed, heavy = TABLE[case]
    return make_csr(n, d, seed, class_heavy(n) if heavy else None, dtype)


def test_new_symbols_are_declared_and_exported():
    declared = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = _lib.load()
    for s in NEW:
        assert s in declared and s in exported, s
        assert getattr(L, s).argtypes is not None, s


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", range(len(TABLE)))
def test_host_twin_is_the_stable_argsort_on_the_table(case, dtype):
    ip, ix, da = table_case(case, dtype)
    assert same(dev.csr_transpose_host(ip, ix, da), definition(ip, ix, da))


def dup_row():
    """Row 1 holds column 2 five times with five distinct values."""
    ip = [0, 2, 8, 10, 12]
    ix = [0, 3, 2, 2, 1, 2, 2, 2, 1, 3, 0, 2]
    return ip, ix, np.arange(1.0, 13.0)


def descending():
    rng = np.random.default_rng(5)
    n = 40
    cols = [np.sort(rng.choice(n, 7, replace=False))[::-1] for _ in range(n)]
    cols[0] = np.arange(n)[::-1]                     # no column stays empty
    ip = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    ix = np.concatenate(cols)
    return ip, ix, 1.0 - rng.random(len(ix))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("make", [dup_row, descending], ids=["duplicates", "descending"])
def test_host_twin_keeps_storage_order(make, dtype):
    ip, ix, da = make()
    da = da.astype(dtype)
    got = dev.csr_transpose_host(ip, ix, da)
    assert same(got, definition(ip, ix, da))
    if make is dup_row:      # column 2's entries of row 1 in their order
        lo, hi = got[0][2], got[0][3]
        assert list(got[1][lo:hi]) == [1, 1, 1, 1, 1, 3]
        assert list(got[2][lo:hi]) == [3.0, 4.0, 6.0, 7.0, 8.0, 12.0]


def test_host_twin_n_1():
    for k in (1, 3):
        ip, ix, da = [0, k], [0] * k, np.arange(1.0, k + 1.0)
        got = dev.csr_transpose_host(ip, ix, da)
        assert same(got, definition(ip, ix, da))
        assert list(got[0]) == [0, k] and list(got[2]) == list(da)


def test_twice_gives_the_matrix_back():
    ip, ix, da = table_case(2)       # sorted columns, no duplicates
    t = dev.csr_transpose_host(ip, ix, da)
    assert not same(t, (ip, ix, da))
    assert same(dev.csr_transpose_host(*t), (ip, ix, da))


def test_errors_name_the_lowest_empty_column():
    ip, ix, da = table_case(0)
    bad = ix.copy()
    bad[(bad == 17) | (bad == 40)] = 3
    with pytest.raises(_lib.EigenValueError, match=r"column 17 has no entry"):
        dev.csr_transpose_host(ip, bad, da)
    bad = ix.copy()
    bad[bad == 63] = 0
    with pytest.raises(_lib.EigenValueError, match=r"column 63 has no entry"):
        dev.csr_transpose_host(ip, bad, da)
    with pytest.raises(_lib.EigenValueError, match=r"column 0 has no entry"):
        dev.csr_transpose_host([0, 1, 2], [1, 1], np.ones(2))


def _twin(dtype, indptr, indices, data, n=None, nnz=None, out=True):
    L = _lib.load()
    indptr = np.ascontiguousarray(indptr, np.int64)
    indices = np.ascontiguousarray(indices, np.int32)
    n = len(indptr) - 1 if n is None else n
    tp, ti, tv = np.zeros(n + 1, np.int64), np.zeros(len(data), np.int32), np.zeros_like(data)
    rc = L.st_csr_transpose_host(dtype, n, len(data) if nnz is None else nnz,
                                 indptr.ctypes.data, indices.ctypes.data, data.ctypes.data,
                                 tp.ctypes.data if out else None, ti.ctypes.data,
                                 tv.ctypes.data)
    return rc, _lib.last_error(L)


def test_every_check_host_message_is_as_before():
    indptr, indices, data = make_csr(64, 8, 7)
    data = data.astype(np.float32)
    assert _twin(0, indptr, indices, data)[0] == 0
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
    for dtype in (2, 3, -1):
        rc, msg = _twin(dtype, indptr, indices, data)
        assert rc < 0 and "dtype must be 0 (f32) or 1 (f64)" in msg
    rc, msg = _twin(0, indptr, indices, data, n=0)
    assert rc < 0 and "n must be" in msg
    rc, msg = _twin(0, indptr, indices, data, out=False)
    assert rc < 0 and "null t_row_ptr" in msg


def test_nnz_of_2_to_32_is_refused_before_any_array_is_read():
    """Pointers that cannot be read: the call returns before looking at them."""
    L = _lib.load()
    rc = L.st_csr_transpose_host(0, 4, 2**32, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY)
    assert rc < 0 and "below 2^32" in _lib.last_error(L)
    rc = L.st_csr_transpose_host(0, 4, 2**32, None, None, None, None, None, None)
    assert rc < 0 and "below 2^32" in _lib.last_error(L)
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    rc = L.max_eigen_value_csr_left_ex(None, 0, 4, 2**32, DUMMY, DUMMY, DUMMY, ctypes.byref(ev),
                                       DUMMY, ctypes.byref(it), None, None)
    assert rc < 0 and "below 2^32" in _lib.last_error(L)
    assert L.st_csr_transpose_scratch_bytes(4, 2**32) == 0


def test_left_twin_rejects_before_any_device_work():
    L = _lib.load()
    indptr, indices, data = make_csr(64, 8, 7)
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    vec = np.zeros(64)

    def call(ip, opt=None):
        rc = L.max_eigen_value_csr_left_ex(None, 1, 64, len(data), ip.ctypes.data,
                                           indices.ctypes.data, data.ctypes.data,
                                           ctypes.byref(ev), vec.ctypes.data, ctypes.byref(it),
                                           ctypes.byref(opt) if opt is not None else None, None)
        return rc, _lib.last_error(L)
    rc, msg = call(indptr)
    assert rc < 0 and "null queue" in msg                       # the matrix itself is fine
    bad = indptr.copy()
    bad[10] = bad[9]
    rc, msg = call(bad)
    assert rc < 0 and "row 9 is empty" in msg
    rc, msg = call(indptr, _lib.st_options(-1.0, 0, 0, 0, _lib.ST_FLAG_ROUND_LOOP))
    assert rc < 0 and "not supported" in msg
    buf = ctypes.create_string_buffer(128)                      # zeros: no magic
    out = ctypes.c_void_p(1)
    assert L.st_csr_transpose(DUMMY, buf, DUMMY, DUMMY, DUMMY, ctypes.byref(out)) < 0
    assert "handle" in _lib.last_error(L) and not out.value


def test_scratch_bytes_and_shape_desc_parse():
    L = _lib.load()
    d = _lib.csr_transpose_shape()
    assert L.st_csr_transpose_shape_desc().decode().startswith("digit_bits=")
    bits, tile = d["digit_bits"], d["tile"]
    assert 1 <= bits <= 16 and tile >= 64 and tile % 64 == 0
    D = 1 << bits
    # at least the two payload buffers a second pass needs, and more with nnz
    small = L.st_csr_transpose_scratch_bytes(D, 3 * D)
    two = L.st_csr_transpose_scratch_bytes(D + 1, 3 * (D + 1))
    assert 0 < small < two and two >= 2 * 4 * 3 * (D + 1)
    assert L.st_csr_transpose_scratch_bytes(0, 5) == 0
    assert L.st_csr_transpose_scratch_bytes(1, 1) > 0           # no pass at all: the tables


def test_python_fronts_reject_a_left_of_the_wrong_type():
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device, no library: the check comes first
    indptr, indices, data = make_csr(64, 8, 7)
    for left in (1, "yes", None):
        with pytest.raises(TypeError, match="left must be a bool"):
            ev.similarity_transform_csr(indptr, indices, data, left=left)
        with pytest.raises(TypeError, match="left must be a bool"):
            dev.DeviceSolver.solve_csr(object.__new__(dev.DeviceSolver), None, left=left)


def test_the_stand_alone_program(tmp_path):
    """tests/cpp/csr_transpose_sanitize.cpp, built by the command of its header
    without the sanitizer flags, on the table matrices."""
    src = os.path.join(ROOT, "tests", "cpp", "csr_transpose_sanitize.cpp")
    exe = tmp_path / "csr_transpose_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "eigen_value_amd",
                                                                        "csrc"),
                    src, "-o", str(exe)], check=True)
    files = []
    for i in range(len(TABLE)):
        ip, ix, _ = table_case(i)
        files.append(str(tmp_path / f"table{i}.bin"))
        write_bin(files[-1], ip, ix)
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
