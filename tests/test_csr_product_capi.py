"""CPU: the product-operator (B·A) surface of the C-ABI - the symbols, the
shape description and scratch size, the host validation (order and messages)
of the two host twins, the Python fronts' checks and the stand-alone program
over st_csr_host.h.  No GPU needed."""
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

NEW = ["st_solve_csr_product", "st_csr_apply", "st_csr_product_rowsum",
       "st_csr_product_round", "st_csr_product_scratch_bytes", "st_csr_product_shape_desc",
       "max_eigen_value_csr_product_ex", "max_eigen_value_csr_gram_ex"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = ctypes.c_void_p(4096)        # never dereferenced: the calls are refused first
OK = _lib.ST_CSR_EMPTY_ROWS_OK


def test_new_symbols_are_declared_exported_and_bound():
    declared = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = _lib.load()
    assert set(NEW) == set(_lib.CSR_PRODUCT_SYMBOLS)
    for s in NEW:
        assert s in declared and s in exported, s
        assert getattr(L, s).argtypes is not None, s
        assert not s.startswith("st_set_")
    assert eigen_value_amd.__version__ == "0.6.0"
    assert L.st_version().decode().split()[1] == "0.6.0"


def test_shape_desc_and_scratch_bytes():
    L = _lib.load()
    d = _lib.csr_product_shape()
    assert d["factors"] == 2 and d["launches_per_round"] == 3 and d["launches_k0"] == 2
    assert d["prep_grid"] == 2048 and d["x_offset"] == 0 and d["empty_rows"] == "A"
    for n in (1, 31, 32, 33, 1000, 3000):     # x and y, 8 bytes at the most, each aligned
        b = L.st_csr_product_scratch_bytes(n)
        assert b == 2 * ((n * 8 + 255) // 256 * 256) and b % 512 == 0
    assert L.st_csr_product_scratch_bytes(0) == 0
    assert L.st_csr_product_scratch_bytes(2**31) == 0


def call_product(B, A, flags=0, dtype=None, opt=None, n=None):
    """max_eigen_value_csr_product_ex with a NULL queue: everything the host
    checks comes first, a valid call ends at "null queue"."""
    L = _lib.load()
    bp, bi, bd = B
    ap, ai, ad = A
    bp, ap = np.ascontiguousarray(bp, np.int64), np.ascontiguousarray(ap, np.int64)
    bi, ai = np.ascontiguousarray(bi, np.int32), np.ascontiguousarray(ai, np.int32)
    n = len(ap) - 1 if n is None else n
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    vec = np.zeros(max(n, 1), ad.dtype)
    rc = L.max_eigen_value_csr_product_ex(
        None, (1 if ad.dtype == np.float64 else 0) if dtype is None else dtype, n,
        len(bd), bp.ctypes.data, bi.ctypes.data, bd.ctypes.data,
        len(ad), ap.ctypes.data, ai.ctypes.data, ad.ctypes.data, flags,
        ctypes.byref(ev), vec.ctypes.data, ctypes.byref(it),
        ctypes.byref(opt) if opt is not None else None, None)
    return rc, _lib.last_error(L)


def call_gram(A, side=0, flags=0, dtype=None, opt=None):
    L = _lib.load()
    ap, ai, ad = A
    ap, ai = np.ascontiguousarray(ap, np.int64), np.ascontiguousarray(ai, np.int32)
    n = len(ap) - 1
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    vec = np.zeros(n, ad.dtype)
    rc = L.max_eigen_value_csr_gram_ex(
        None, (1 if ad.dtype == np.float64 else 0) if dtype is None else dtype, n, len(ad),
        ap.ctypes.data, ai.ctypes.data, ad.ctypes.data, side, flags,
        ctypes.byref(ev), vec.ctypes.data, ctypes.byref(it),
        ctypes.byref(opt) if opt is not None else None, None)
    return rc, _lib.last_error(L)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_product_host_validation_order_and_messages(dt):
    A = make_csr(64, 8, 7, dtype=dt)
    B = make_csr(64, 8, 11, dtype=dt)
    rc, msg = call_product(B, A)
    assert rc < 0 and "null queue" in msg                    # all of it is fine
    rc, msg = call_product(A, A)
    assert rc < 0 and "null queue" in msg                    # A², the same arrays twice
    badB = (B[0], B[1].copy(), B[2])
    badB[1][43] = 64
    badA = (A[0], A[1].copy(), A[2])
    badA[1][50] = -1
    # dtype, opt's flags, `flags` - before either matrix
    rc, msg = call_product(badB, badA, dtype=2)
    assert rc < 0 and "dtype must be 0 (f32) or 1 (f64)" in msg
    rc, msg = call_product(badB, badA,
                           opt=_lib.st_options(-1.0, 0, 0, 0, _lib.ST_FLAG_ROUND_LOOP))
    assert rc < 0 and "not supported" in msg
    rc, msg = call_product(badB, badA, flags=2)
    assert rc < 0 and "unknown flags 2" in msg
    # B's triple before A's, each with the single solve's text behind the factor
    rc, msg = call_product(badB, badA)
    assert rc < 0 and "csr product: factor B: column index 64 of entry 43 (row 5)" in msg, msg
    rc, msg = call_product(B, badA)
    assert rc < 0 and "csr product: factor A: column index -1 of entry 50 (row 6)" in msg, msg
    rc, msg = call_product(B, A, n=0)
    assert rc < 0 and "factor B: n must be in [1, 2^31), got 0" in msg
    # empty rows: never in B, in A only under the flag
    eA = tc.empty_rows(*A, [9, 30, 63])
    eB = tc.empty_rows(*B, [4])
    rc, msg = call_product(eB, A, flags=OK)
    assert rc < 0 and "factor B: row 4 is empty" in msg
    rc, msg = call_product(B, eA)
    assert rc < 0 and "factor A: row 9 is empty" in msg
    rc, msg = call_product(B, eA, flags=OK)
    assert rc < 0 and "null queue" in msg
    # a row of B whose columns all hit emptied rows of A: the lowest is named
    hit20 = sorted(set(int(c) for c in B[1][B[0][20]:B[0][21]]))
    hit41 = sorted(set(int(c) for c in B[1][B[0][41]:B[0][42]]))
    gone = set(hit20) | set(hit41)
    low = min(r for r in range(64)
              if all(int(c) in gone for c in B[1][B[0][r]:B[0][r + 1]]))
    assert low <= 20
    rc, msg = call_product(B, tc.empty_rows(*A, sorted(gone)), flags=OK)
    assert rc < 0 and f"csr product: row {low} of B·A has no positive entry" in msg, msg
    rc, msg = call_product(B, tc.empty_rows(*A, hit41), flags=OK)
    assert rc < 0 and "row 41 of B·A has no positive entry" in msg, msg
    # zeros are no entries: row 20 of B zero; then the rows of A it points at
    z = B[2].copy()
    z[B[0][20]:B[0][21]] = 0
    rc, msg = call_product((B[0], B[1], z), A)
    assert rc < 0 and "row 20 of B·A has no positive entry" in msg
    za = A[2].copy()
    for c in hit20:
        za[A[0][c]:A[0][c + 1]] = 0
    rc, msg = call_product(B, (A[0], A[1], za))
    assert rc < 0 and "row 20 of B·A has no positive entry" in msg


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_gram_host_validation_order_and_messages(dt):
    A = make_csr(64, 8, 7, dtype=dt)
    for side in (_lib.ST_GRAM_ATA, _lib.ST_GRAM_AAT):
        rc, msg = call_gram(A, side)
        assert rc < 0 and "null queue" in msg
    bad = (A[0], A[1].copy(), A[2])
    bad[1][43] = 64
    rc, msg = call_gram(bad, side=2, dtype=2)
    assert rc < 0 and "side must be 0 (A^T A) or 1 (A A^T), got 2" in msg
    rc, msg = call_gram(bad, dtype=2)
    assert rc < 0 and "dtype must be 0 (f32) or 1 (f64)" in msg
    rc, msg = call_gram(bad, opt=_lib.st_options(-1.0, 0, 0, 0, _lib.ST_FLAG_BATCH_ROUNDS))
    assert rc < 0 and "not supported" in msg
    rc, msg = call_gram(bad, flags=4)
    assert rc < 0 and "unknown flags 4" in msg
    rc, msg = call_gram(bad)
    assert rc < 0 and "column index 64 of entry 43 (row 5)" in msg
    # nodes without out-links are fine for AᵀA under the flag; AAᵀ gets an empty row
    e = tc.empty_rows(*A, [9, 30])
    rc, msg = call_gram(e)
    assert rc < 0 and "row 9 is empty" in msg
    rc, msg = call_gram(e, _lib.ST_GRAM_ATA, flags=OK)
    assert rc < 0 and "null queue" in msg
    rc, msg = call_gram(e, _lib.ST_GRAM_AAT, flags=OK)
    assert rc < 0 and "factor B: row 9 is empty" in msg
    # an empty column: an empty row of Aᵀ, the left factor of AᵀA
    ix = A[1].copy()
    ix[ix == 17] = 3
    rc, msg = call_gram((A[0], ix, A[2]), _lib.ST_GRAM_ATA)
    assert rc < 0 and "factor B: row 17 is empty" in msg
    rc, msg = call_gram((A[0], ix, A[2]), _lib.ST_GRAM_AAT)
    assert rc < 0 and "null queue" in msg


def test_the_python_fronts_check_before_any_library_call():
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device, no library: the check comes first
    A = make_csr(64, 8, 7)
    A32 = make_csr(64, 8, 7, dtype=np.float32)
    small = make_csr(32, 8, 3)
    with pytest.raises(TypeError, match="triples or sparse matrices required"):
        ev.similarity_transform_csr_product(None, A)
    with pytest.raises(ValueError, match=r"differ in n \(B: 32, A: 64\)"):
        ev.similarity_transform_csr_product(small, A)
    with pytest.raises(TypeError, match="differ in dtype"):
        ev.similarity_transform_csr_product(A32, A)
    with pytest.raises(TypeError, match="allow_empty_rows must be a bool"):
        ev.similarity_transform_csr_product(A, A, allow_empty_rows=1)
    with pytest.raises(TypeError, match="B: data must be float32 or float64"):
        ev.similarity_transform_csr_product((A[0], A[1], A[2].astype(np.float16)), A)
    with pytest.raises(TypeError, match="A: indices must be an integer array"):
        ev.similarity_transform_csr_product(A, (A[0], A[1].astype(np.float64), A[2]))
    with pytest.raises(ValueError, match='side must be "ata" or "aat"'):
        ev.similarity_transform_csr_gram(A, side="left")
    with pytest.raises(ValueError, match='side must be "ata" or "aat"'):
        ev.similarity_transform_csr_gram(A, side=0)
    s = object.__new__(dev.DeviceSolver)
    with pytest.raises(TypeError, match="B: a CsrMatrix required"):
        s.solve_csr_product(None, None)
    with pytest.raises(TypeError, match="left must be a bool"):
        s.solve_csr_product(None, None, left=1)
    with pytest.raises(TypeError, match="links: a CsrMatrix required"):
        s.hits(np.ones((3, 3)))
    with pytest.raises(TypeError, match="a CsrMatrix required"):
        dev.csr_apply(None, None)
    with pytest.raises(TypeError, match="B: a CsrMatrix required"):
        dev.csr_product_rowsum(None, None, None)
    with pytest.raises(TypeError, match="B: a CsrMatrix required"):
        dev.csr_product_round(None, None, None, None, None, None, None, None)
    closed = object.__new__(dev.CsrMatrix)
    closed.handle = ctypes.c_void_p()
    with pytest.raises(ValueError, match="csr: the matrix is closed"):
        dev.csr_apply(closed, None)


def test_handles_of_another_kind_are_refused_by_name():
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)                       # zeros: no magic
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    assert L.st_solve_csr_product(DUMMY, buf, buf, DUMMY, None, ctypes.byref(ev),
                                  ctypes.byref(it), None, None) < 0
    assert "st_solve_csr_product (B): not a CSR matrix handle" in _lib.last_error(L)
    assert L.st_csr_apply(buf, DUMMY, DUMMY, None) < 0
    assert "not a CSR matrix handle" in _lib.last_error(L)
    assert L.st_csr_product_rowsum(buf, buf, DUMMY, DUMMY, None) < 0
    assert "not a CSR matrix handle" in _lib.last_error(L)
    assert L.st_csr_product_round(buf, buf, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 1e-3, 1, 10, 0,
                                  DUMMY, None) < 0
    assert "not a CSR matrix handle" in _lib.last_error(L)


def test_the_stand_alone_program(tmp_path):
    """tests/cpp/csr_product_sanitize.cpp, built without the sanitizer flags
    (make csr_product_sanitize builds and runs it with them), on the table
    matrices."""
    src = os.path.join(ROOT, "tests", "cpp", "csr_product_sanitize.cpp")
    exe = tmp_path / "csr_product_sanitize"
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
