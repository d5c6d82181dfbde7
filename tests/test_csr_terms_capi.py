"""CPU: the low-rank-terms and empty-rows surface of the C-ABI - the symbols,
the host validation (order and messages), the flagged host transposition
against its numpy definition, the Python fronts' checks and the stand-alone
program over st_csr_host.h.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import eigen_value_amd
from eigen_value_amd import _lib
from eigen_value_amd import device as dev
from csr_cases import TABLE, class_heavy, make_csr, write_bin
import csr_terms_cases as tc

NEW = ["st_csr_create_ex", "st_csr_empty_rows", "st_csr_transpose_ex",
       "st_csr_transpose_host_ex", "st_csr_terms_create", "st_csr_terms_destroy",
       "st_csr_terms_scratch_bytes", "st_csr_terms_shape_desc", "st_solve_csr_terms",
       "max_eigen_value_csr_terms_ex", "st_csr_terms_rowsum", "st_csr_terms_round"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = ctypes.c_void_p(4096)        # never dereferenced: the calls are refused first
OK = _lib.ST_CSR_EMPTY_ROWS_OK


def test_new_symbols_are_declared_and_exported():
    declared = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = _lib.load()
    for s in NEW:
        assert s in declared and s in exported, s
        assert getattr(L, s).argtypes is not None, s
    assert eigen_value_amd.__version__ == "0.6.0"
    assert L.st_version().decode().split()[1] == "0.6.0"


def test_shape_desc_and_scratch_bytes():
    L = _lib.load()
    d = _lib.csr_terms_shape()
    assert d["terms_max"] == _lib.ST_CSR_TERMS_MAX == 4
    assert d["dot_grid"] == tc.DOT_GRID and d["lanes"] == tc.BLOCK
    assert d["launches_per_round"] == 3
    for K in (1, 4):           # dots, K x dot_grid partials and x, of 8 bytes at the most
        b = L.st_csr_terms_scratch_bytes(1000, K)
        assert b >= d["partial_offset"] + K * d["dot_grid"] * 8 + 1000 * 8 and b % 256 == 0
    assert L.st_csr_terms_scratch_bytes(1000, 0) == 0
    assert L.st_csr_terms_scratch_bytes(1000, 5) == 0
    assert L.st_csr_terms_scratch_bytes(0, 1) == 0


def call_host(indptr, indices, data, u, w, flags=0, K=None, dtype=None, opt=None):
    """max_eigen_value_csr_terms_ex with a NULL queue: everything the host
    checks comes first, a valid call ends at "null queue"."""
    L = _lib.load()
    indptr = np.ascontiguousarray(indptr, np.int64)
    indices = np.ascontiguousarray(indices, np.int32)
    n = len(indptr) - 1
    u = [np.ascontiguousarray(x, data.dtype) for x in u]
    w = [np.ascontiguousarray(x, data.dtype) for x in w]
    pu = (ctypes.c_void_p * max(len(u), 1))(*[x.ctypes.data for x in u])
    pw = (ctypes.c_void_p * max(len(w), 1))(*[x.ctypes.data for x in w])
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    vec = np.zeros(n, data.dtype)
    rc = L.max_eigen_value_csr_terms_ex(
        None, (1 if data.dtype == np.float64 else 0) if dtype is None else dtype, n, len(data),
        indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, len(u) if K is None else K,
        pu, pw, flags, ctypes.byref(ev), vec.ctypes.data, ctypes.byref(it),
        ctypes.byref(opt) if opt is not None else None, None)
    return rc, _lib.last_error(L)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_host_validation_order_and_messages(dt):
    ip, ix, da = make_csr(64, 8, 7, dtype=dt)
    u, w = tc.term_vectors(64, 2, 3, dt)
    rc, msg = call_host(ip, ix, da, u, w)
    assert rc < 0 and "null queue" in msg                    # all of it is fine
    # dtype, opt's flags, the matrix - before K and the vectors
    rc, msg = call_host(ip, ix, da, u, w, dtype=2, K=9)
    assert rc < 0 and "dtype must be 0 (f32) or 1 (f64)" in msg
    rc, msg = call_host(ip, ix, da, u, w, K=9,
                        opt=_lib.st_options(-1.0, 0, 0, 0, _lib.ST_FLAG_ROUND_LOOP))
    assert rc < 0 and "not supported" in msg
    rc, msg = call_host(ip, ix, da, u, w, flags=2)
    assert rc < 0 and "unknown flags 2" in msg
    bad = ix.copy()
    bad[43] = 64
    rc, msg = call_host(ip, bad, da, u, w, K=9)
    assert rc < 0 and "column index 64 of entry 43 (row 5)" in msg
    # a bad K
    for K in (0, 5, 9):
        rc, msg = call_host(ip, ix, da, u, w, K=K)
        assert rc < 0 and f"K must be in [1, 4], got {K}" in msg
    # a negative, NaN or inf entry: the lowest (term, u before w, index)
    for val, shown in ((-0.5, "-0.5"), (np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
        b = w.copy()
        b[1, 17] = val
        rc, msg = call_host(ip, ix, da, u, b)
        assert rc < 0 and f"w_1[17] = {shown}" in msg and "finite and >= 0" in msg, msg
    bu, bw = u.copy(), w.copy()
    bu[1, 3], bw[0, 60], bu[0, 40], bu[0, 41] = -1, -1, np.nan, -1
    rc, msg = call_host(ip, ix, da, bu, bw)
    assert rc < 0 and "u_0[40]" in msg
    bu[0, 40], bu[0, 41] = 0, 0
    rc, msg = call_host(ip, ix, da, bu, bw)
    assert rc < 0 and "w_0[60]" in msg                       # term 0 before term 1
    # zero is legal
    z = np.zeros_like(u)
    rc, msg = call_host(ip, ix, da, z, w)
    assert rc < 0 and "null queue" in msg


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_empty_rows_with_and_without_the_flag(dt):
    ip, ix, da = make_csr(64, 8, 7, dtype=dt)
    u, w = tc.term_vectors(64, 1, 3, dt)
    e = tc.empty_rows(ip, ix, da, [9, 30, 63])
    rc, msg = call_host(*e, u, w)
    assert rc < 0 and "row 9 is empty" in msg and "divided by zero" in msg   # today's text
    rc, msg = call_host(*e, u, w, flags=OK)
    assert rc < 0 and "null queue" in msg
    # with the flag row_ptr still must not decrease, and start at 0 and end at nnz
    down = e[0].copy()
    down[31] = down[30] - 1
    rc, msg = call_host(down, e[1], e[2], u, w, flags=OK)
    assert rc < 0 and "decreases at row 30" in msg
    # a row without a positive entry: empty in A and u = 0 there
    z = u.copy()
    z[0, 30] = 0
    rc, msg = call_host(*e, z, w, flags=OK)
    assert rc < 0 and "row 30 of A + Σ u wᵀ has no positive entry" in msg
    z[0, 9] = 0
    rc, msg = call_host(*e, z, w, flags=OK)
    assert rc < 0 and "row 9 of A" in msg                   # the lowest
    # w = 0 takes every term away
    rc, msg = call_host(*e, u, np.zeros_like(w), flags=OK)
    assert rc < 0 and "row 9 of A" in msg
    # nnz >= 1 stays required
    rc, msg = call_host(np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0, dt),
                        u[:, :4], w[:, :4], flags=OK)
    assert rc < 0 and "nnz must be >= 1" in msg


def definition(indptr, indices, data):
    """T(A): a stable argsort of the columns; empty columns give empty rows."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int32)
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr))
    p = np.argsort(indices, kind="stable")
    t_ptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=n))]).astype(np.int64)
    return t_ptr, rows[p], np.asarray(data)[p]


def same(got, want):
    return all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def holes(case, dtype):
    """A table matrix with rows emptied at both ends and in the middle, and
    the columns 0, 5 and n - 1 without an entry."""
    n, d, seed, heavy = TABLE[case]
    ip, ix, da = make_csr(n, d, seed, class_heavy(n) if heavy else None, dtype)
    ix = ix.copy()
    ix[(ix == 0) | (ix == 5) | (ix == n - 1)] = 1
    return tc.empty_rows(ip, ix, da, [0, 1, n // 2, n // 2 + 1, n - 1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", range(len(TABLE)))
def test_flagged_host_transposition_is_the_stable_argsort(case, dtype):
    ip, ix, da = holes(case, dtype)
    with pytest.raises(_lib.EigenValueError, match=r"row 0 is empty"):
        dev.csr_transpose_host(ip, ix, da)                   # without the flag: as before
    got = dev.csr_transpose_host(ip, ix, da, allow_empty=True)
    assert same(got, definition(ip, ix, da))
    lens = np.diff(got[0])
    assert lens[0] == lens[5] == lens[-1] == 0
    # no empty row, an empty column: only the flag decides
    n, d, seed, heavy = TABLE[case]
    ip, ix, da = make_csr(n, d, seed, None, dtype)
    ix = ix.copy()
    ix[ix == 17] = 3
    with pytest.raises(_lib.EigenValueError, match=r"column 17 has no entry"):
        dev.csr_transpose_host(ip, ix, da)
    assert same(dev.csr_transpose_host(ip, ix, da, allow_empty=True), definition(ip, ix, da))


def test_the_python_fronts_check_before_any_library_call():
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device, no library: the check comes first
    ip, ix, da = make_csr(64, 8, 7)
    u, w = tc.term_vectors(64, 2, 3)
    with pytest.raises(TypeError, match="terms must be a pair"):
        ev.similarity_transform_csr(ip, ix, da, terms=u)
    with pytest.raises(ValueError, match="allow_empty_rows needs terms"):
        ev.similarity_transform_csr(ip, ix, da, allow_empty_rows=True)
    with pytest.raises(TypeError, match="allow_empty_rows must be a bool"):
        ev.similarity_transform_csr(ip, ix, da, terms=(u, w), allow_empty_rows=1)
    ev._trace = None
    with pytest.raises(ValueError, match=r"K must be in \[1, 4\], got 5"):
        ev.similarity_transform_csr(ip, ix, da, terms=(np.ones((5, 64)), np.ones((5, 64))))
    with pytest.raises(ValueError, match="2 vectors u but 1 vectors w"):
        ev.similarity_transform_csr(ip, ix, da, terms=(u, w[:1]))
    with pytest.raises(ValueError, match=r"w_1 has shape \(63,\)"):
        ev.similarity_transform_csr(ip, ix, da, terms=(u, [w[0], w[1][:63]]))
    with pytest.raises(TypeError, match="a CsrMatrix required"):
        dev.CsrTerms(None, u, w)
    s = object.__new__(dev.DeviceSolver)
    with pytest.raises(TypeError, match="a CsrMatrix required"):
        s.pagerank(np.ones((3, 3)))
    with pytest.raises(TypeError, match="allow_empty_rows must be a bool"):
        dev.CsrMatrix(None, None, None, allow_empty_rows="yes")
    with pytest.raises(TypeError, match="allow_empty must be a bool"):
        dev.CsrMatrix.transpose(object.__new__(dev.CsrMatrix), allow_empty=1)


def test_handles_of_another_kind_are_refused_by_name():
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)                       # zeros: no magic
    out = ctypes.c_void_p(1)
    assert L.st_csr_terms_create(DUMMY, buf, 1, DUMMY, DUMMY, ctypes.byref(out)) < 0
    assert "not a CSR matrix handle" in _lib.last_error(L) and not out.value
    assert L.st_csr_terms_rowsum(buf, buf, DUMMY, DUMMY, None) < 0
    assert "not a CSR matrix handle" in _lib.last_error(L)
    assert L.st_csr_terms_destroy(buf) < 0
    assert "not a terms object" in _lib.last_error(L)
    assert L.st_csr_terms_destroy(None) == 0
    assert L.st_csr_empty_rows(buf, None, None) < 0


def test_the_stand_alone_program(tmp_path):
    """tests/cpp/csr_terms_sanitize.cpp, built without the sanitizer flags (make
    csr_terms_sanitize builds and runs it with them), on the table matrices."""
    src = os.path.join(ROOT, "tests", "cpp", "csr_terms_sanitize.cpp")
    exe = tmp_path / "csr_terms_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g",
                    "-I" + os.path.join(ROOT, "eigen_value_amd", "csrc"), src, "-o", str(exe)],
                   check=True)
    files = []
    for i in range(len(TABLE)):
        n, d, seed, heavy = TABLE[i]
        ip, ix, _ = make_csr(n, d, seed, class_heavy(n) if heavy else None)
        files.append(str(tmp_path / f"table{i}.bin"))
        write_bin(files[-1], ip, ix)
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
