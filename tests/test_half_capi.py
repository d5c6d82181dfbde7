"""CPU: the half-precision-storage surface of the C-ABI (st_solve_device_half,
max_eigen_value_half_ex, st_rowsum_half, st_mfree_round_half, st_narrow_f32)
and its Python fronts - what is checked on the host before anything is
enqueued.  No compute calls (no GPU here)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from eigen_value_amd import _lib

NEW = ["st_rowsum_half", "st_mfree_round_half", "st_solve_device_half",
       "max_eigen_value_half_ex", "st_narrow_f32", "st_half_shape_desc"]
DUMMY = ctypes.c_void_p(4096)        # never dereferenced: the calls are refused first


def test_new_symbols_are_declared_and_exported():
    declared = _lib.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in NEW:
        assert s in declared and s in exported, s
    assert (_lib.ST_STORE_F16, _lib.ST_STORE_BF16) == (2, 3)
    hdr = open(_lib.HEADER).read()
    assert "#define ST_STORE_F16  2" in hdr and "#define ST_STORE_BF16 3" in hdr
    # the shape the kernels were built with: a library build carries the constants
    assert _lib.load().st_half_shape_desc().decode().startswith("rows=")


def test_header_compiles_as_c_and_cxx_with_the_half_surface(tmp_path):
    inc = os.path.dirname(_lib.HEADER)
    use = ('int main(void){ int (*f)(int, const void*, float*, unsigned, unsigned, void*) = '
           '&st_rowsum_half;\n int (*g)(int, const float*, void*, uint64_t, void*) = '
           '&st_narrow_f32;\n return (f && g) ? ST_STORE_F16 + ST_STORE_BF16 - 5 : 1; }\n')
    src_c = tmp_path / "t.c"
    src_c.write_text('#include "similarity_transform.h"\n' + use)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{inc}", "-c", str(src_c),
                    "-o", str(tmp_path / "tc.o")], check=True)
    src_cc = tmp_path / "t.cc"
    src_cc.write_text('#include "similarity_transform.h"\n' + use)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{inc}", "-c", str(src_cc),
                    "-o", str(tmp_path / "tcc.o")], check=True)


def _calls(L, storage, opt=None):
    """Every half entry point with `storage`, pointers that are never read."""
    o = ctypes.byref(opt) if opt is not None else None
    ev, it = ctypes.c_float(), ctypes.c_uint32()
    return {
        "st_rowsum_half": lambda: L.st_rowsum_half(storage, DUMMY, DUMMY, 4, 4, None),
        "st_mfree_round_half": lambda: L.st_mfree_round_half(
            storage, DUMMY, DUMMY, DUMMY, DUMMY, ctypes.c_void_p(8192), 4, 4, 0, 1e-3, 1, 10, 0,
            DUMMY, None),
        "st_narrow_f32": lambda: L.st_narrow_f32(storage, DUMMY, DUMMY, 16, None),
        "st_solve_device_half": lambda: L.st_solve_device_half(
            DUMMY, storage, DUMMY, 4, DUMMY, None, ctypes.byref(ev), ctypes.byref(it), o, None),
        "max_eigen_value_half_ex": lambda: L.max_eigen_value_half_ex(
            DUMMY, storage, DUMMY, ctypes.byref(ev), DUMMY, 4, ctypes.byref(it), o, None),
    }


@pytest.mark.parametrize("storage", [0, 1, 4])
def test_other_storage_codes_are_refused_naming_the_value(storage):
    """The half entry points know 2 (fp16) and 3 (bf16) only; 0 and 1 are the
    dtype codes of the OTHER calls.  Refused on the host, first of all."""
    L = _lib.load()
    for name, call in _calls(L, storage).items():
        assert call() < 0, name
        msg = _lib.last_error(L)
        assert "storage" in msg and f"got {storage}" in msg, (name, msg)


@pytest.mark.parametrize("flag", [_lib.ST_FLAG_ROUND_LOOP, _lib.ST_FLAG_WRITE_EVERY_ROUND,
                                  _lib.ST_FLAG_BATCH_ROUNDS])
@pytest.mark.parametrize("storage", [_lib.ST_STORE_F16, _lib.ST_STORE_BF16])
def test_flags_of_the_writing_forms_are_not_supported(storage, flag):
    """Never a fallback, never silently ignored - and refused before the queue
    is even looked at."""
    L = _lib.load()
    opt = _lib.st_options(-1.0, 0, 0, 0, flag | _lib.ST_FLAG_MATRIX_FREE)
    calls = _calls(L, storage, opt)
    for name in ("st_solve_device_half", "max_eigen_value_half_ex"):
        assert calls[name]() < 0, name
        assert "not supported" in _lib.last_error(L), (name, _lib.last_error(L))


def test_step_argument_errors():
    L = _lib.load()
    f16 = _lib.ST_STORE_F16
    assert L.st_rowsum_half(f16, None, None, 4, 4, None) < 0 and "null" in _lib.last_error(L)
    assert L.st_rowsum_half(f16, DUMMY, DUMMY, 0, 4, None) == 0          # no rows: a no-op
    assert L.st_rowsum_half(f16, DUMMY, DUMMY, 4, 0, None) < 0
    assert L.st_narrow_f32(f16, None, None, 0, None) == 0               # nothing to do
    assert L.st_narrow_f32(f16, None, None, 4, None) < 0
    # an odd matrix address cannot hold 16-bit elements
    assert L.st_rowsum_half(f16, ctypes.c_void_p(4097), DUMMY, 4, 4, None) < 0
    assert "aligned" in _lib.last_error(L)
    v2 = ctypes.c_void_p(8192)

    def mf(nrows=4, ncols=4, row0=0, k=1, max_itr=10, sem=0, v_cur=v2):
        return L.st_mfree_round_half(f16, DUMMY, DUMMY, DUMMY, DUMMY, v_cur, nrows, ncols, row0,
                                     1e-3, k, max_itr, sem, DUMMY, None)
    assert mf(k=0) < 0 and "k must be >= 1" in _lib.last_error(L)
    assert mf(sem=7) < 0 and "semantics" in _lib.last_error(L)
    assert mf(nrows=0) < 0 and "empty" in _lib.last_error(L)
    assert mf(v_cur=DUMMY) < 0 and "differ" in _lib.last_error(L)
    assert mf(nrows=3, row0=2) < 0 and "exceed" in _lib.last_error(L)    # rows past the columns
    # the whole solves: null queue / null outputs come after storage and flags
    ev, it = ctypes.c_float(), ctypes.c_uint32()
    assert L.st_solve_device_half(None, f16, DUMMY, 4, DUMMY, None, ctypes.byref(ev),
                                  ctypes.byref(it), None, None) < 0
    assert "null queue" in _lib.last_error(L)
    assert L.max_eigen_value_half_ex(None, f16, DUMMY, ctypes.byref(ev), DUMMY, 4,
                                     ctypes.byref(it), None, None) < 0
    assert "null queue" in _lib.last_error(L)
    bad = _lib.st_options(-1.0, 0, 9, 0, 0)
    assert L.st_solve_device_half(DUMMY, f16, DUMMY, 4, DUMMY, None, ctypes.byref(ev),
                                  ctypes.byref(it), ctypes.byref(bad), None) < 0
    assert "semantics" in _lib.last_error(L)


def test_existing_dtype_parameters_still_know_0_and_1_only():
    L = _lib.load()
    ev, it = ctypes.c_float(), ctypes.c_uint32()
    for code in (_lib.ST_STORE_F16, _lib.ST_STORE_BF16):
        assert L.max_eigen_value_ex(DUMMY, code, DUMMY, ctypes.byref(ev), DUMMY, 4,
                                    ctypes.byref(it), None, None) < 0
        assert "dtype must be 0 (f32) or 1 (f64)" in _lib.last_error(L)
        assert L.st_solve_batched_max_dim(code) == 0


def test_python_front_asserts_before_any_library_call():
    from eigen_value_amd.similarity_transform import EigenValue
    ev = object.__new__(EigenValue)          # no device needed for the checks
    with pytest.raises(AssertionError, match="square"):
        ev.similarity_transform_half(np.ones((3, 4), np.float16))
    with pytest.raises(AssertionError, match="float16"):
        ev.similarity_transform_half(np.ones((3, 3), np.float32))
    with pytest.raises(AssertionError, match="float16"):
        ev.similarity_transform_half(np.ones((3, 3), np.uint16))           # bf16 needs storage=
    with pytest.raises(AssertionError, match="uint16"):
        ev.similarity_transform_half(np.ones((3, 3), np.float16), storage="bf16")
    with pytest.raises(AssertionError, match="storage"):
        ev.similarity_transform_half(np.ones((3, 3), np.float16), storage="fp8")
    # the old entry points keep refusing half input exactly as before
    with pytest.raises(AssertionError, match="float32"):
        ev.similarity_transform(np.ones((3, 3), np.float16))
    with pytest.raises(TypeError):
        ev.similarity_transform_ex(np.ones((3, 3), np.float16))


def test_device_front_dtype_checks_need_no_device():
    torch = pytest.importorskip("torch")
    from eigen_value_amd import device as dev
    assert dev._storage(torch.zeros(1, dtype=torch.float16)) == _lib.ST_STORE_F16
    assert dev._storage(torch.zeros(1, dtype=torch.bfloat16)) == _lib.ST_STORE_BF16
    with pytest.raises(TypeError, match="float16/bfloat16"):
        dev._storage(torch.zeros(1, dtype=torch.float32))
    with pytest.raises(TypeError, match="float32/float64"):
        dev._sfx(torch.zeros(1, dtype=torch.float16))       # the old paths: unchanged
    s = object.__new__(dev.DeviceSolver)
    with pytest.raises(TypeError, match="float16/bfloat16"):
        dev.DeviceSolver.solve_half(s, torch.zeros((2, 2), dtype=torch.float32))
    s.q = None                                              # nothing for __del__ to release
