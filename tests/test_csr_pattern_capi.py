"""CPU: the pattern-only surface of the C-ABI (section 3h) - the symbols, the
scratch size and the shape description without a device, every host refusal
of max_eigen_value_csr_pattern_ex with a NULL queue in its order and with its
message, the Python fronts' checks and the stand-alone program over
st_csr_host.h under the host sanitizers.  No GPU needed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from eigen_value_amd import _lib
from eigen_value_amd import device as dev
from csr_cases import TABLE, class_heavy, make_csr, write_bin
import csr_terms_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = ctypes.c_void_p(4096)        # never dereferenced: the calls are refused first
OK = _lib.ST_CSR_EMPTY_ROWS_OK


def test_new_symbols_are_declared_and_exported():
    declared = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L = _lib.load()
    assert len(_lib.CSR_PATTERN_SYMBOLS) == 12
    for s in _lib.CSR_PATTERN_SYMBOLS:
        assert s in declared and s in exported, s
        assert getattr(L, s).argtypes is not None, s


def test_shape_desc_and_scratch_bytes_need_no_device():
    L = _lib.load()
    d = _lib.csr_pattern_shape()
    values = dict(kv.split("=") for kv in L.st_csr_shape_desc().decode().split())
    assert d["lanes"] == values["lanes"] and d["rows"] == values["rows"]
    assert d["unroll"] == values["unroll"]                  # the values kernels' tables
    assert d["matrix_bytes_per_entry"] == 4
    assert d["launches_per_round"] == 2 and d["launches_per_round_terms"] == 3
    assert d["prep_grid"] == 2048
    for key in ("vgpr_f32", "vgpr_f64", "waves_f32", "waves_f64", "vgpr_rs_f32",
                "vgpr_rs_f64", "waves_rs_f32", "waves_rs_f64"):
        assert isinstance(d[key], int) and d[key] > 0, key
    assert 1 <= d["waves_f64"] <= d["waves_f32"] <= 8
    assert d["vgpr_f32"] <= 512 // d["waves_f32"] and d["vgpr_f64"] <= 512 // d["waves_f64"]
    # the terms' layout with z where x stands; K = 0 allowed
    for K in (1, 2, 4):
        assert L.st_csr_pattern_scratch_bytes(1000, K) == L.st_csr_terms_scratch_bytes(1000, K)
    b0 = L.st_csr_pattern_scratch_bytes(1000, 0)
    assert b0 == 256 + 8192 and b0 % 256 == 0
    assert L.st_csr_pattern_scratch_bytes(1000, 5) == 0
    assert L.st_csr_pattern_scratch_bytes(0, 1) == 0
    assert L.st_csr_pattern_scratch_bytes(2**31, 0) == 0


def call_host(indptr, indices, dt, r=None, c=None, u=(), w=(), flags=0, K=None, dtype=None,
              opt=None, n=None, null_tables=False):
    """max_eigen_value_csr_pattern_ex with a NULL queue: everything the host
    checks comes first, a valid call ends at "null queue"."""
    L = _lib.load()
    indptr = None if indptr is None else np.ascontiguousarray(indptr, np.int64)
    indices = None if indices is None else np.ascontiguousarray(indices, np.int32)
    n = (len(indptr) - 1) if n is None else n
    r = None if r is None else np.ascontiguousarray(r, dt)
    c = None if c is None else np.ascontiguousarray(c, dt)
    u = [np.ascontiguousarray(x, dt) for x in u]
    w = [np.ascontiguousarray(x, dt) for x in w]
    pu = (ctypes.c_void_p * 4)(*[x.ctypes.data for x in u])      # the rest NULL
    pw = (ctypes.c_void_p * 4)(*[x.ctypes.data for x in w])
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    vec = np.zeros(max(n, 1), dt)
    rc = L.max_eigen_value_csr_pattern_ex(
        None, (1 if dt == np.float64 else 0) if dtype is None else dtype, n,
        0 if indices is None else len(indices),
        None if indptr is None else indptr.ctypes.data,
        None if indices is None else indices.ctypes.data,
        None if r is None else r.ctypes.data, None if c is None else c.ctypes.data,
        len(u) if K is None else K, None if null_tables else pu, None if null_tables else pw,
        flags, ctypes.byref(ev), vec.ctypes.data, ctypes.byref(it),
        ctypes.byref(opt) if opt is not None else None, None)
    return rc, _lib.last_error(L)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_host_validation_order_and_messages(dt):
    ip, ix, _ = make_csr(64, 8, 7, dtype=dt)
    r = np.full(64, 0.5, dt)
    c = np.full(64, 2.0, dt)
    u, w = tc.term_vectors(64, 2, 3, dt)
    for kw in ({}, {"r": r}, {"c": c}, {"r": r, "c": c}, {"r": r, "c": c, "u": u, "w": w},
               {"null_tables": True}):
        rc, msg = call_host(ip, ix, dt, **kw)
        assert rc < 0 and "null queue" in msg, (kw.keys(), msg)    # all of it is fine
    bad_r = r.copy()
    bad_r[17] = -0.5
    # dtype, opt's flags, flags, n, the arrays - each before the scales and K
    rc, msg = call_host(ip, ix, dt, r=bad_r, dtype=2, K=9)
    assert rc < 0 and "dtype must be 0 (f32) or 1 (f64), got 2" in msg
    rc, msg = call_host(ip, ix, dt, r=bad_r, K=9,
                        opt=_lib.st_options(-1.0, 0, 0, 0, _lib.ST_FLAG_ROUND_LOOP))
    assert rc < 0 and "not supported" in msg
    rc, msg = call_host(ip, ix, dt, r=bad_r, flags=2)
    assert rc < 0 and "max_eigen_value_csr_pattern_ex: unknown flags 2" in msg
    rc, msg = call_host(ip, ix, dt, r=bad_r, n=0)
    assert rc < 0 and "n must be in [1, 2^31), got 0" in msg
    rc, msg = call_host(None, ix, dt, r=bad_r, n=64)
    assert rc < 0 and "null row_ptr / col_idx" in msg
    rc, msg = call_host(ip, None, dt, r=bad_r)
    assert rc < 0 and "null row_ptr / col_idx" in msg
    # row_ptr: its start, a decrease, an empty row, its end
    p = ip.copy()
    p[0] = 1
    rc, msg = call_host(p, ix, dt, r=bad_r)
    assert rc < 0 and "row_ptr[0] must be 0, got 1" in msg
    p = ip.copy()
    p[31] = p[30] - 1
    rc, msg = call_host(p, ix, dt, r=bad_r)
    assert rc < 0 and "decreases at row 30" in msg
    p = ip.copy()
    p[31] = p[30]
    rc, msg = call_host(p, ix, dt, r=bad_r)
    assert rc < 0 and "row 30 is empty" in msg
    rc, msg = call_host(ip, ix[:-1], dt, r=bad_r)
    assert rc < 0 and "row_ptr[n] must be nnz = 511, got 512" in msg
    # the columns, only after row_ptr passed
    bad = ix.copy()
    bad[43] = 64
    rc, msg = call_host(ip, bad, dt, r=bad_r, K=9)
    assert rc < 0 and "column index 64 of entry 43 (row 5) is outside [0, 64)" in msg
    bad[43] = -1
    rc, msg = call_host(ip, bad, dt, r=bad_r, K=9)
    assert rc < 0 and "column index -1 of entry 43" in msg
    # the scales before K
    rc, msg = call_host(ip, ix, dt, r=bad_r, K=9)
    assert rc < 0 and "row_scale[17] = -0.5 is not finite and positive" in msg, msg
    # then K and the tables
    rc, msg = call_host(ip, ix, dt, r=r, c=c, K=5)
    assert rc < 0 and "K must be in [0, 4], got 5" in msg
    for K in (1, 4):
        rc, msg = call_host(ip, ix, dt, r=r, K=K, null_tables=True)
        assert rc < 0 and "null vector table" in msg
    rc, msg = call_host(ip, ix, dt, u=u, w=w, K=3)         # the third pair is not there
    assert rc < 0 and "null u_2" in msg


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_bad_scale_is_named_the_lowest_and_row_before_column(dt):
    ip, ix, _ = make_csr(64, 8, 7, dtype=dt)
    r = np.full(64, 0.5, dt)
    c = np.full(64, 2.0, dt)
    for val, shown in ((0.0, "0"), (-0.5, "-0.5"), (np.inf, "inf"), (-np.inf, "-inf"),
                       (np.nan, "nan")):
        for name in ("row_scale", "col_scale"):
            b = (r if name == "row_scale" else c).copy()
            b[40], b[17] = val, val
            kw = {"r": b, "c": c} if name == "row_scale" else {"r": r, "c": b}
            rc, msg = call_host(ip, ix, dt, **kw)
            assert rc < 0 and f"csr pattern: {name}[17] = {shown} is not finite and positive" \
                in msg, msg
            kw = {"r": b} if name == "row_scale" else {"c": b}   # the other one NULL
            rc, msg = call_host(ip, ix, dt, **kw)
            assert rc < 0 and f"{name}[17] = {shown} " in msg, msg
        br, bc = r.copy(), c.copy()
        br[60], bc[3] = val, val
        rc, msg = call_host(ip, ix, dt, r=br, c=bc)
        assert rc < 0 and "row_scale[60]" in msg                # row_scale first, whatever the index
    tiny = np.full(64, np.finfo(dt).smallest_subnormal, dt)
    rc, msg = call_host(ip, ix, dt, r=tiny, c=np.full(64, np.finfo(dt).max, dt))
    assert rc < 0 and "null queue" in msg                       # positive and finite


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_terms_and_empty_rows(dt):
    ip, ix, da = make_csr(64, 8, 7, dtype=dt)
    u, w = tc.term_vectors(64, 2, 3, dt)
    r = np.full(64, 0.5, dt)
    # the term vectors: csr terms' predicate and text, after the scales
    b = w.copy()
    b[1, 17] = -0.5
    rc, msg = call_host(ip, ix, dt, r=r, u=u, w=b)
    assert rc < 0 and "w_1[17] = -0.5" in msg and "finite and >= 0" in msg
    br = r.copy()
    br[5] = 0
    rc, msg = call_host(ip, ix, dt, r=br, u=u, w=b)
    assert rc < 0 and "row_scale[5] = 0 " in msg
    # empty rows: refused by row_ptr without the flag, by name without terms with it
    ep, ei, _ = tc.empty_rows(ip, ix, da, [9, 30, 63])
    rc, msg = call_host(ep, ei, dt)
    assert rc < 0 and "row 9 is empty" in msg and "divided by zero" in msg
    rc, msg = call_host(ep, ei, dt, flags=OK)
    assert rc < 0 and "max_eigen_value_csr_pattern_ex: row 9 is empty (3 empty rows" in msg
    assert "st_csr_pattern_terms_create" in msg
    rc, msg = call_host(ep, ei, dt, r=r, u=u, w=w, flags=OK)
    assert rc < 0 and "null queue" in msg
    z = u.copy()
    z[:, 30] = 0
    rc, msg = call_host(ep, ei, dt, r=r, u=z, w=w, flags=OK)
    assert rc < 0 and "row 30 of A + Σ u wᵀ has no positive entry" in msg
    rc, msg = call_host(np.zeros(5, np.int64), np.zeros(0, np.int32), dt, flags=OK)
    assert rc < 0 and "nnz must be >= 1" in msg


def test_handles_of_another_kind_are_refused_by_name():
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)                       # zeros: no magic
    out = ctypes.c_void_p(1)
    assert L.st_csr_pattern_transpose(DUMMY, buf, DUMMY, DUMMY, 0, ctypes.byref(out)) < 0
    assert "not a CSR pattern handle" in _lib.last_error(L) and not out.value
    out = ctypes.c_void_p(1)
    assert L.st_csr_pattern_terms_create(DUMMY, buf, 1, DUMMY, DUMMY, ctypes.byref(out)) < 0
    assert "not a CSR pattern handle" in _lib.last_error(L) and not out.value
    for call in (lambda: L.st_csr_pattern_rowsum(buf, None, DUMMY, DUMMY, None),
                 lambda: L.st_csr_pattern_round(buf, None, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY,
                                                1e-3, 1, 10, 0, DUMMY, None),
                 lambda: L.st_solve_csr_pattern(DUMMY, buf, None, DUMMY, None, DUMMY, DUMMY,
                                                None, None),
                 lambda: L.st_csr_pattern_get_plan(buf, None, None),
                 lambda: L.st_csr_pattern_empty_rows(buf, None, None),
                 lambda: L.st_csr_pattern_destroy(buf)):
        assert call() < 0
        assert "not a CSR pattern handle" in _lib.last_error(L)
    assert L.st_csr_pattern_destroy(None) == 0


def test_the_python_fronts_check_before_any_library_call():
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device, no library: the check comes first
    ip, ix, _ = make_csr(64, 8, 7)
    u, w = tc.term_vectors(64, 2, 3)
    with pytest.raises(TypeError, match="terms must be a pair"):
        ev.similarity_transform_csr_pattern(ip, ix, terms=u)
    with pytest.raises(ValueError, match="allow_empty_rows needs terms"):
        ev.similarity_transform_csr_pattern(ip, ix, allow_empty_rows=True)
    with pytest.raises(TypeError, match="left must be a bool"):
        ev.similarity_transform_csr_pattern(ip, ix, left=1)
    with pytest.raises(ValueError, match=r"row_scale has shape \(63,\)"):
        ev.similarity_transform_csr_pattern(ip, ix, row_scale=np.ones(63))
    with pytest.raises(TypeError, match="a sparse matrix required"):
        ev.similarity_transform_csr_pattern(3.5)
    assert "values are ignored" in " ".join(
        EigenValue.similarity_transform_csr_pattern.__doc__.lower().split())
    s = object.__new__(dev.DeviceSolver)
    with pytest.raises(TypeError, match="a CsrPattern required"):
        s.solve_csr_pattern(np.ones((3, 3)))
    with pytest.raises(TypeError, match="a CsrPattern required"):
        dev.csr_pattern_rowsum(None)
    with pytest.raises(TypeError, match="allow_empty_rows must be a bool"):
        dev.CsrPattern(None, None, allow_empty_rows="yes")
    with pytest.raises(TypeError, match="allow_empty must be a bool"):
        dev.CsrPattern.transpose(object.__new__(dev.CsrPattern), allow_empty=1)


def tables(tmp_path):
    files = []
    for i in range(len(TABLE)):
        n, d, seed, heavy = TABLE[i]
        ip, ix, _ = make_csr(n, d, seed, class_heavy(n) if heavy else None)
        files.append(str(tmp_path / f"table{i}.bin"))
        write_bin(files[-1], ip, ix)
    return files


def test_the_stand_alone_program(tmp_path):
    """tests/cpp/csr_pattern_sanitize.cpp, built without the sanitizer flags,
    on the table matrices (every machine)."""
    src = os.path.join(ROOT, "tests", "cpp", "csr_pattern_sanitize.cpp")
    exe = tmp_path / "csr_pattern_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g",
                    "-I" + os.path.join(ROOT, "eigen_value_amd", "csrc"), src, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)] + tables(tmp_path), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


@pytest.mark.skipif(os.path.exists("/dev/kfd"),
                    reason="the host sanitizers run on machines without a GPU only")
def test_make_csr_pattern_sanitize_ends_clean():
    """The Makefile target: the same program under -fsanitize=address,undefined
    on the tables of csr_cases.py.  The library is taken as built (-o: the
    target only needs it to exist)."""
    lib = os.path.relpath(_lib.lib_path(), ROOT)
    r = subprocess.run(["make", "-o", lib, "PYTHON=" + sys.executable, "csr_pattern_sanitize"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
