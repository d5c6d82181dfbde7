"""Device-resident API over torch-ROCm tensors.

Torch is plumbing here (HBM allocation, streams); every kernel is the HIP
code in ``libsimilarity_transform.so`` launched through the C-ABI on the
caller's current torch stream.  Nothing in this module computes on the CPU:
a missing library raises, a non-CUDA tensor raises.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

from . import _lib

_SFX = {}


def _torch():
    import torch
    return torch


def _sfx(t) -> str:
    torch = _torch()
    if t.dtype == torch.float64:
        return "f64"
    if t.dtype == torch.float32:
        return "f32"
    raise TypeError(f"float32/float64 tensor required, got {t.dtype}")


def _check_cuda(*ts) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("device API needs tensors on a HIP device (cuda:N)")


def _stream(device=None) -> int:
    torch = _torch()
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------
# state
# --------------------------------------------------------------------------
def new_state(device="cuda"):
    """A zeroed 64-byte ``st_state`` on the device (uint8 tensor)."""
    torch = _torch()
    return torch.zeros(64, dtype=torch.uint8, device=device)


def reset_state(state) -> None:
    _check_cuda(state)
    _lib.check(_lib.load().st_state_reset(_ptr(state), _stream(state.device)), "st_state_reset")


def read_state(state) -> dict:
    raw = bytes(state.cpu().numpy().tobytes())
    s = _lib.st_state.from_buffer_copy(raw)
    return dict(done=s.done, round=s.round, iters=s.iters, stop=s.stop,
                eigen_val=s.lambda_, max=s.max, end=s.end)


# --------------------------------------------------------------------------
# generators
# --------------------------------------------------------------------------
def generate(kind: str, n: int, dtype=None, nrows: Optional[int] = None, row0: int = 0,
             seed: int = 0, device="cuda", out=None):
    """Rows [row0, row0+nrows) of an n-wide input matrix generated on device.

    kind: 'hilbert' (utils.cpp:137-154), 'random' (seeded splitmix64 U(0,1]),
    'identity' (utils.cpp:5-27)."""
    torch = _torch()
    dtype = dtype or torch.float64
    nrows = n if nrows is None else nrows
    if out is None:
        out = torch.empty((nrows, n), dtype=dtype, device=device)
    _check_cuda(out)
    L, sfx, st = _lib.load(), _sfx(out), _stream(out.device)
    if kind == "hilbert":
        rc = getattr(L, f"st_generate_hilbert_{sfx}")(_ptr(out), nrows, n, row0, st)
    elif kind == "random":
        rc = getattr(L, f"st_generate_random_{sfx}")(_ptr(out), nrows, n, row0, seed, st)
    elif kind == "identity":
        rc = getattr(L, f"st_generate_identity_{sfx}")(_ptr(out), nrows, n, row0, st)
    else:
        raise ValueError(f"unknown generator {kind!r}")
    _lib.check(rc, f"generate_{kind}")
    return out


def fill(x, value: float) -> None:
    _check_cuda(x)
    _lib.check(getattr(_lib.load(), f"st_fill_{_sfx(x)}")(_ptr(x), x.numel(), value,
                                                          _stream(x.device)), "fill")


# --------------------------------------------------------------------------
# step-level kernels
# --------------------------------------------------------------------------
def rowsum(mat, out=None):
    """s[r] = Σ_c A[r][c] for the rows of ``mat`` (sum_across_rows)."""
    _check_cuda(mat)
    assert mat.is_contiguous() and mat.dim() == 2
    if out is None:
        out = mat.new_empty(mat.shape[0])
    _lib.check(getattr(_lib.load(), f"st_rowsum_{_sfx(mat)}")(
        _ptr(mat), _ptr(out), mat.shape[0], mat.shape[1], _stream(mat.device)), "rowsum")
    return out


def rowsum_flat(mat, out, part) -> None:
    """out[r] = sum_c mat[r][c] in the flat form (st_rowsum_flat): the
    solve loops' initial pass for blocks where ``flat_round_pays``; ``part``
    is ``flat_scratch(nrows, ncols)``."""
    _check_cuda(mat, out, part)
    _lib.check(getattr(_lib.load(), f"st_rowsum_flat_{_sfx(mat)}")(
        _ptr(mat), _ptr(out), _ptr(part), mat.shape[0], mat.shape[1],
        _stream(mat.device)), "rowsum_flat")


def scale_rowsum(mat, s_cur, s_next=None, row0: int = 0,
                 semantics: int = _lib.ST_SEM_SYCL, state=None) -> None:
    """Fused round body, in place on ``mat`` (local rows row0..): see
    ``st_scale_rowsum_*`` in include/similarity_transform.h."""
    _check_cuda(mat, s_cur, s_next, state)
    assert mat.is_contiguous() and mat.dim() == 2
    nrows, ncols = mat.shape
    assert s_cur.numel() >= ncols and s_cur.numel() >= row0 + nrows
    if s_next is not None:
        assert s_next.numel() >= nrows
    _lib.check(getattr(_lib.load(), f"st_scale_rowsum_{_sfx(mat)}")(
        _ptr(mat), _ptr(s_cur), _ptr(s_next), nrows, ncols, row0, semantics,
        _ptr(state), _stream(mat.device)), "scale_rowsum")


def fused_round(mat, s_cur, s_next, v, state, row0: int = 0, eps: float = 1e-3, k: int = 0,
          max_itr: int = _lib.ST_MAX_ITR, semantics: int = _lib.ST_SEM_SYCL) -> None:
    """One whole round k in one launch (``st_round_*``): stats of the full
    s_cur, v update of the local rows, in-place transform, s_next."""
    _check_cuda(mat, s_cur, s_next, v, state)
    assert mat.is_contiguous() and mat.dim() == 2
    nrows, ncols = mat.shape
    assert s_cur.numel() >= ncols and v.numel() >= row0 + nrows and s_next.numel() >= nrows
    _lib.check(getattr(_lib.load(), f"st_round_{_sfx(mat)}")(
        _ptr(mat), _ptr(s_cur), _ptr(s_next), _ptr(v), nrows, ncols, row0, eps, k,
        max_itr, semantics, _ptr(state), _stream(mat.device)), "round")


def mfree_round(mat0, s_prev, s_next, v_prev, v_cur, state, row0: int = 0,
                eps: float = 1e-3, k: int = 1, max_itr: int = _lib.ST_MAX_ITR,
                semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Matrix-free launch k >= 1 (``st_mfree_round_*``): round k-1's stats
    and v_{k-1} (full vector) from s_prev, and s_k for the local rows of A_0."""
    _check_cuda(mat0, s_prev, s_next, v_prev, v_cur, state)
    assert mat0.is_contiguous() and mat0.dim() == 2
    nrows, ncols = mat0.shape
    assert s_prev.numel() >= ncols and v_prev.numel() >= ncols and v_cur.numel() >= ncols
    assert s_next.numel() >= nrows and row0 + nrows <= ncols
    _lib.check(getattr(_lib.load(), f"st_mfree_round_{_sfx(mat0)}")(
        _ptr(mat0), _ptr(s_prev), _ptr(s_next), _ptr(v_prev), _ptr(v_cur), nrows, ncols,
        row0, eps, k, max_itr, semantics, _ptr(state), _stream(mat0.device)), "mfree_round")


def mfree_round_flat(mat0, s_prev, s_next, v_prev, v_cur, part, state, row0: int = 0,
                     eps: float = 1e-3, k: int = 1, max_itr: int = _lib.ST_MAX_ITR,
                     semantics: int = _lib.ST_SEM_SYCL) -> None:
    """mfree_round in the flat form (``st_mfree_round_flat_*``): partial dot
    products per 4 / 8 KB piece into ``part`` (flat_scratch), then s_k and
    v_{k-1}; the solve loops' form for blocks where flat_round_pays."""
    _check_cuda(mat0, s_prev, s_next, v_prev, v_cur, part, state)
    assert mat0.is_contiguous() and mat0.dim() == 2
    nrows, ncols = mat0.shape
    assert s_prev.numel() >= ncols and v_prev.numel() >= ncols and v_cur.numel() >= ncols
    assert s_next.numel() >= nrows and row0 + nrows <= ncols
    assert part.numel() >= int(_lib.load().st_round_flat_scratch(nrows, ncols))
    _lib.check(getattr(_lib.load(), f"st_mfree_round_flat_{_sfx(mat0)}")(
        _ptr(mat0), _ptr(s_prev), _ptr(s_next), _ptr(v_prev), _ptr(v_cur), _ptr(part), nrows,
        ncols, row0, eps, k, max_itr, semantics, _ptr(state), _stream(mat0.device)),
        "mfree_round_flat")


def _dtype_code(dtype) -> int:
    torch = _torch()
    if dtype == torch.float64:
        return _lib.DTYPE_F64
    if dtype == torch.float32:
        return _lib.DTYPE_F32
    raise TypeError(f"float32/float64 required, got {dtype}")


def left_scratch(n: int, dtype, device="cuda"):
    """The scratch of ``colsum`` / ``mfree_left_round`` for an n x n matrix
    (``st_left_scratch`` elements: x, then the row-block partials)."""
    torch = _torch()
    count = int(_lib.load().st_left_scratch(_dtype_code(dtype), n))
    if count == 0:
        raise _lib.EigenValueError(f"st_left_scratch: {_lib.last_error()}")
    return torch.empty(count, dtype=dtype, device=device)


def colsum(mat, out=None):
    """s[c] = Σ_r A[r][c] for the columns of the square ``mat``, read where it
    lies (``st_colsum_*``: launch 0 of the left-vector solve), in the order
    ``st_left_shape`` publishes."""
    _check_cuda(mat, out)
    assert mat.is_contiguous() and mat.dim() == 2 and mat.shape[0] == mat.shape[1]
    n = mat.shape[0]
    if out is None:
        out = mat.new_empty(n)
    assert out.numel() >= n
    scratch = left_scratch(n, mat.dtype, mat.device)
    _lib.check(getattr(_lib.load(), f"st_colsum_{_sfx(mat)}")(
        _ptr(mat), _ptr(out), _ptr(scratch), n, _stream(mat.device)), "colsum")
    return out


def mfree_left_round(mat0, s_prev, s_next, v_prev, v_cur, scratch, state, *,
                     eps: float = 1e-3, k: int = 1, max_itr: int = _lib.ST_MAX_ITR,
                     semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Launch k >= 1 of the left-vector solve (``st_mfree_left_round_*``):
    round k-1's stats and v_{k-1} from s_prev exactly as ``mfree_round``, and
    s_k[c] = (Σ_r A_0[r][c] x[r]) / x[c]; ``scratch`` is ``left_scratch``
    (x stands at its start afterwards).  ``mat0`` is only read."""
    _check_cuda(mat0, s_prev, s_next, v_prev, v_cur, scratch, state)
    assert mat0.is_contiguous() and mat0.dim() == 2 and mat0.shape[0] == mat0.shape[1]
    n = mat0.shape[0]
    assert min(s_prev.numel(), s_next.numel(), v_prev.numel(), v_cur.numel()) >= n
    assert scratch.dtype == mat0.dtype
    assert scratch.numel() >= int(_lib.load().st_left_scratch(_dtype_code(mat0.dtype), n))
    _lib.check(getattr(_lib.load(), f"st_mfree_left_round_{_sfx(mat0)}")(
        _ptr(mat0), _ptr(s_prev), _ptr(s_next), _ptr(v_prev), _ptr(v_cur), _ptr(scratch), n,
        eps, k, max_itr, semantics, _ptr(state), _stream(mat0.device)), "mfree_left_round")


def pair_scratch(n: int, dtype, device="cuda"):
    """The scratch of ``pair_sum`` / ``mfree_pair_round`` for an n x n matrix
    (``st_pair_scratch`` elements: x_R, x_L, the column partials, the row
    partials)."""
    torch = _torch()
    count = int(_lib.load().st_pair_scratch(_dtype_code(dtype), n))
    if count == 0:
        raise _lib.EigenValueError(f"st_pair_scratch: {_lib.last_error()}")
    return torch.empty(count, dtype=dtype, device=device)


def pair_sum(mat, out_right=None, out_left=None, scratch=None):
    """(s_right, s_left): the row sums and the column sums of the square
    ``mat`` from one pass over it (``st_pair_sum_*``: launch 0 of the pair
    solve), in the orders ``st_pair_shape`` publishes."""
    _check_cuda(mat, out_right, out_left, scratch)
    assert mat.is_contiguous() and mat.dim() == 2 and mat.shape[0] == mat.shape[1]
    n = mat.shape[0]
    out_right = mat.new_empty(n) if out_right is None else out_right
    out_left = mat.new_empty(n) if out_left is None else out_left
    assert min(out_right.numel(), out_left.numel()) >= n
    if scratch is None:
        scratch = pair_scratch(n, mat.dtype, mat.device)
    assert scratch.dtype == mat.dtype
    assert scratch.numel() >= int(_lib.load().st_pair_scratch(_dtype_code(mat.dtype), n))
    _lib.check(getattr(_lib.load(), f"st_pair_sum_{_sfx(mat)}")(
        _ptr(mat), _ptr(out_right), _ptr(out_left), _ptr(scratch), n, _stream(mat.device)),
        "pair_sum")
    return out_right, out_left


def mfree_pair_round(mat0, right, left, scratch, states, *, eps: float = 1e-3, k: int = 1,
                     max_itr: int = _lib.ST_MAX_ITR,
                     semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Launch k >= 1 of the pair solve (``st_mfree_pair_round_*``).  ``right``
    and ``left`` are ``(s_prev, s_next, v_prev, v_cur)`` of their side,
    ``states`` two adjacent ``st_state`` (128 bytes: the right side's, then the
    left side's), ``scratch`` is ``pair_scratch``.  ``mat0`` is only read, once
    for both sides; a side whose state has ended gets no write."""
    _check_cuda(mat0, *right, *left, scratch, states)
    assert mat0.is_contiguous() and mat0.dim() == 2 and mat0.shape[0] == mat0.shape[1]
    n = mat0.shape[0]
    assert len(right) == 4 and len(left) == 4
    assert min(t.numel() for t in (*right, *left)) >= n
    assert scratch.dtype == mat0.dtype
    assert scratch.numel() >= int(_lib.load().st_pair_scratch(_dtype_code(mat0.dtype), n))
    assert states.numel() * states.element_size() >= 128
    _lib.check(getattr(_lib.load(), f"st_mfree_pair_round_{_sfx(mat0)}")(
        _ptr(mat0), *(_ptr(t) for t in right), *(_ptr(t) for t in left), _ptr(scratch), n,
        eps, k, max_itr, semantics, _ptr(states), _stream(mat0.device)), "mfree_pair_round")


def _storage(t) -> int:
    """The storage code of a float16 / bfloat16 tensor (ST_STORE_*)."""
    torch = _torch()
    if t.dtype == torch.float16:
        return _lib.ST_STORE_F16
    if t.dtype == torch.bfloat16:
        return _lib.ST_STORE_BF16
    raise TypeError(f"float16/bfloat16 tensor required, got {t.dtype}")


def narrow(x, dtype, out=None):
    """``x`` (float32) rounded to nearest even into a float16 / bfloat16
    tensor of the same shape (``st_narrow_f32``): how a half matrix is made
    from the fp32 generators."""
    torch = _torch()
    _check_cuda(x)
    if x.dtype != torch.float32:
        raise TypeError(f"float32 tensor required, got {x.dtype}")
    assert x.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _check_cuda(out)
    assert out.is_contiguous() and out.numel() == x.numel()
    _lib.check(_lib.load().st_narrow_f32(_storage(out), _ptr(x), _ptr(out), x.numel(),
                                         _stream(x.device)), "st_narrow_f32")
    return out


def rowsum_half(mat, out=None):
    """s[r] = Σ_c A[r][c] in float32 for a float16 / bfloat16 ``mat``
    (``st_rowsum_half``): launch 0 of the half matrix-free scheme."""
    torch = _torch()
    _check_cuda(mat)
    assert mat.is_contiguous() and mat.dim() == 2
    if out is None:
        out = torch.empty(mat.shape[0], dtype=torch.float32, device=mat.device)
    assert out.dtype == torch.float32 and out.numel() >= mat.shape[0]
    _lib.check(_lib.load().st_rowsum_half(_storage(mat), _ptr(mat), _ptr(out), mat.shape[0],
                                          mat.shape[1], _stream(mat.device)), "rowsum_half")
    return out


def mfree_round_half(mat0, s_prev, s_next, v_prev, v_cur, state, row0: int = 0,
                     eps: float = 1e-3, k: int = 1, max_itr: int = _lib.ST_MAX_ITR,
                     semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Matrix-free launch k >= 1 on a float16 / bfloat16 ``mat0``
    (``st_mfree_round_half``): mfree_round's contract with float32 vectors;
    v_cur and the state are bit for bit mfree_round's on the widened matrix."""
    torch = _torch()
    _check_cuda(mat0, s_prev, s_next, v_prev, v_cur, state)
    assert mat0.is_contiguous() and mat0.dim() == 2
    assert all(t.dtype == torch.float32 for t in (s_prev, s_next, v_prev, v_cur))
    nrows, ncols = mat0.shape
    assert s_prev.numel() >= ncols and v_prev.numel() >= ncols and v_cur.numel() >= ncols
    assert s_next.numel() >= nrows and row0 + nrows <= ncols
    _lib.check(_lib.load().st_mfree_round_half(
        _storage(mat0), _ptr(mat0), _ptr(s_prev), _ptr(s_next), _ptr(v_prev), _ptr(v_cur),
        nrows, ncols, row0, eps, k, max_itr, semantics, _ptr(state),
        _stream(mat0.device)), "mfree_round_half")


class CsrMatrix:
    """A nonnegative sparse matrix in CSR storage on the device, validated and
    planned (``st_csr_create``): the torch tensors (int64 ``crow_indices``
    [n + 1], int32 ``col_indices`` [nnz], float32 / float64 ``values`` [nnz])
    and the library's handle over them.

    Built from ``(crow_indices, col_indices, values, n)`` - device tensors;
    index dtypes are converted as needed, nothing else is copied - or from a
    ``torch.sparse_csr`` tensor (``CsrMatrix(sparse)``).  Raises
    ``EigenValueError`` naming the first offending row or entry when the
    check kernel rejects the arrays; no handle exists then.  ``solver`` is
    the ``DeviceSolver`` whose queue runs the check (one is made and closed
    when None).

    ``transpose()`` gives T(A) as a new ``CsrMatrix`` (``st_csr_transpose``: a
    stable sort of the entries by column on the device); ``.T`` is the same,
    built once, kept, and closed with this matrix.

    ``allow_empty_rows`` (``st_csr_create_ex``, ``ST_CSR_EMPTY_ROWS_OK``): rows
    without an entry are legal; ``empty_rows`` counts them and ``first_empty``
    is the lowest (n when none).  Such a matrix is solved with ``CsrTerms``
    (``solve_csr(m, terms)``, ``pagerank``); ``solve_csr(m)`` alone refuses
    it, naming the row."""

    _t = None
    allow_empty_rows = False
    empty_rows = 0

    def __init__(self, crow_indices, col_indices=None, values=None, n: Optional[int] = None,
                 *, solver: Optional["DeviceSolver"] = None, allow_empty_rows: bool = False):
        if not isinstance(allow_empty_rows, bool):
            raise TypeError("allow_empty_rows must be a bool, got "
                            f"{type(allow_empty_rows).__name__}")
        torch = _torch()
        self.handle = ctypes.c_void_p()
        self.L = _lib.load()
        if col_indices is None:
            sp = crow_indices
            if sp.layout != torch.sparse_csr:
                raise TypeError(f"a torch.sparse_csr tensor required, got layout {sp.layout}")
            assert sp.dim() == 2 and sp.shape[0] == sp.shape[1], "must be square"
            n = sp.shape[0]
            crow_indices, col_indices, values = (sp.crow_indices(), sp.col_indices(),
                                                 sp.values())
        _check_cuda(crow_indices, col_indices, values)
        self.dtype_code = 1 if _sfx(values) == "f64" else 0
        self.n = int(crow_indices.numel() - 1 if n is None else n)
        if crow_indices.numel() != self.n + 1:
            raise ValueError(f"crow_indices has {crow_indices.numel()} elements, n + 1 = "
                             f"{self.n + 1} required")
        if col_indices.numel() != values.numel():
            raise ValueError("col_indices and values differ in length")
        self.crow = crow_indices.to(torch.int64).contiguous()
        self.col = col_indices.to(torch.int32).contiguous()
        self.values = values.contiguous()
        self.nnz = int(values.numel())
        self.device = values.device
        own = solver is None
        solver = solver or DeviceSolver(self.device)
        try:
            _lib.check(self.L.st_set_stream(solver.q, _stream(self.device)), "st_set_stream")
            if allow_empty_rows:
                _lib.check(self.L.st_csr_create_ex(
                    solver.q, self.dtype_code, self.n, self.nnz, _ptr(self.crow), _ptr(self.col),
                    _ptr(self.values), _lib.ST_CSR_EMPTY_ROWS_OK, ctypes.byref(self.handle)),
                    "st_csr_create_ex")
            else:
                _lib.check(self.L.st_csr_create(solver.q, self.dtype_code, self.n, self.nnz,
                                                _ptr(self.crow), _ptr(self.col),
                                                _ptr(self.values), ctypes.byref(self.handle)),
                           "st_csr_create")
        finally:
            if own:
                solver.close()
        self.allow_empty_rows = allow_empty_rows
        self._read_empty()

    def _read_empty(self) -> None:
        k, lo = ctypes.c_uint32(), ctypes.c_uint32()
        _lib.check(self.L.st_csr_empty_rows(self.handle, ctypes.byref(k), ctypes.byref(lo)),
                   "st_csr_empty_rows")
        self.empty_rows, self.first_empty = int(k.value), int(lo.value)

    @property
    def dtype(self):
        return self.values.dtype

    def plan(self):
        """``(order, class_first)`` of the handle (``st_csr_get_plan``)."""
        import numpy as np
        order = np.zeros(self.n, dtype=np.uint32)
        first = np.zeros(_lib.ST_CSR_CLASSES + 1, dtype=np.uint32)
        _lib.check(self.L.st_csr_get_plan(self.handle, order.ctypes.data, first.ctypes.data),
                   "st_csr_get_plan")
        return order, first

    def transpose(self, solver: Optional["DeviceSolver"] = None,
                  allow_empty: bool = False) -> "CsrMatrix":
        """T(A) (``st_csr_transpose``): the entries sorted by column, those of
        one column in storage order, in tensors torch allocates - bit for bit
        ``csr_transpose_host`` of the same arrays.  Raises ``EigenValueError``
        naming the lowest column without an entry (the transposed matrix
        would have an empty row) unless ``allow_empty``
        (``st_csr_transpose_ex``): the result is then an empty-rows matrix.
        The result is independent of this matrix."""
        if not isinstance(allow_empty, bool):
            raise TypeError(f"allow_empty must be a bool, got {type(allow_empty).__name__}")
        torch = _torch()
        if not self.handle.value:
            raise ValueError("the matrix is closed")
        t = object.__new__(CsrMatrix)
        t.handle = ctypes.c_void_p()
        t.L = self.L
        t.dtype_code, t.n, t.nnz, t.device = self.dtype_code, self.n, self.nnz, self.device
        t.crow = torch.empty(self.n + 1, dtype=torch.int64, device=self.device)
        t.col = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
        t.values = torch.empty(self.nnz, dtype=self.dtype, device=self.device)
        own = solver is None
        solver = solver or DeviceSolver(self.device)
        try:
            _lib.check(self.L.st_set_stream(solver.q, _stream(self.device)), "st_set_stream")
            if allow_empty:
                _lib.check(self.L.st_csr_transpose_ex(
                    solver.q, self.handle, _ptr(t.crow), _ptr(t.col), _ptr(t.values),
                    _lib.ST_CSR_EMPTY_ROWS_OK, ctypes.byref(t.handle)), "st_csr_transpose_ex")
            else:
                _lib.check(self.L.st_csr_transpose(solver.q, self.handle, _ptr(t.crow),
                                                   _ptr(t.col), _ptr(t.values),
                                                   ctypes.byref(t.handle)), "st_csr_transpose")
        finally:
            if own:
                solver.close()
        t.allow_empty_rows = allow_empty
        t._read_empty()
        return t

    @property
    def T(self) -> "CsrMatrix":
        """``transpose()``, built at the first use and kept; closed with this
        matrix."""
        if self._t is None:
            self._t = self.transpose()
        return self._t

    def close(self) -> None:
        if self._t is not None:
            self._t.close()
            self._t = None
        if self.handle is not None and self.handle.value:
            self.L.st_csr_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CsrPattern:
    """The pattern-only operator ``diag(row_scale) · P · diag(col_scale)`` of
    an unweighted graph on the device (``st_csr_pattern_create``): int64
    ``crow_indices`` [n + 1] and int32 ``col_indices`` [nnz] - no values at
    all; ``P[i][j]`` is the number of entries of row i with column j.  The
    scales are optional tensors [n], finite and strictly positive; None means
    all ones and costs nothing.  A round reads nnz * 4 bytes of matrix.

    ``dtype`` is the scales' (they must agree); without scales it is
    ``torch.float32`` unless given.  Built from ``(crow_indices, col_indices,
    n)`` - device tensors, index dtypes converted as needed - or from a
    ``torch.sparse_csr`` tensor, whose values are ignored.  Raises
    ``EigenValueError`` naming the first offending row, entry or scale.

    ``transpose()`` gives T(P) with the scales swapped
    (``st_csr_pattern_transpose``); ``.T`` is the same, built once, kept, and
    closed with this object.  ``allow_empty_rows`` as ``CsrMatrix``: such a
    pattern is solved with ``CsrTerms`` (``solve_csr_pattern(p, terms)``,
    ``pagerank``).  Not accepted by the product operator, ``hits``, the
    multi-column and batched solves and ``csr_apply``: those take a
    ``CsrMatrix`` (with values of 1)."""

    _t = None
    allow_empty_rows = False
    empty_rows = 0

    def __init__(self, crow_indices, col_indices=None, n: Optional[int] = None, *,
                 row_scale=None, col_scale=None, allow_empty_rows: bool = False,
                 solver: Optional["DeviceSolver"] = None, dtype=None):
        if not isinstance(allow_empty_rows, bool):
            raise TypeError("allow_empty_rows must be a bool, got "
                            f"{type(allow_empty_rows).__name__}")
        torch = _torch()
        self.handle = ctypes.c_void_p()
        self.L = _lib.load()
        if col_indices is None:
            sp = crow_indices
            if sp.layout != torch.sparse_csr:
                raise TypeError(f"a torch.sparse_csr tensor required, got layout {sp.layout}")
            assert sp.dim() == 2 and sp.shape[0] == sp.shape[1], "must be square"
            n = sp.shape[0]
            crow_indices, col_indices = sp.crow_indices(), sp.col_indices()
        _check_cuda(crow_indices, col_indices, row_scale, col_scale)
        for name, x in (("row_scale", row_scale), ("col_scale", col_scale)):
            if x is None:
                continue
            if not isinstance(x, torch.Tensor):
                raise TypeError(f"{name} must be a torch tensor, got {type(x).__name__}")
            _sfx(x)
            if dtype is not None and x.dtype != dtype:
                raise TypeError(f"{name} is {x.dtype}, dtype {dtype}")
            dtype = x.dtype
        self.dtype = torch.float32 if dtype is None else dtype
        if self.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"float32/float64 required, got {self.dtype}")
        self.dtype_code = 1 if self.dtype == torch.float64 else 0
        self.n = int(crow_indices.numel() - 1 if n is None else n)
        if crow_indices.numel() != self.n + 1:
            raise ValueError(f"crow_indices has {crow_indices.numel()} elements, n + 1 = "
                             f"{self.n + 1} required")
        self.crow = crow_indices.to(torch.int64).contiguous()
        self.col = col_indices.to(torch.int32).contiguous()
        self.nnz = int(col_indices.numel())
        self.device = self.crow.device
        for name, x in (("row_scale", row_scale), ("col_scale", col_scale)):
            if x is not None and (tuple(x.shape) != (self.n,) or x.device != self.device):
                raise ValueError(f"{name} must be a tensor of shape ({self.n},) on "
                                 f"{self.device}")
        self.row_scale = None if row_scale is None else row_scale.contiguous()
        self.col_scale = None if col_scale is None else col_scale.contiguous()
        own = solver is None
        solver = solver or DeviceSolver(self.device)
        try:
            _lib.check(self.L.st_set_stream(solver.q, _stream(self.device)), "st_set_stream")
            _lib.check(self.L.st_csr_pattern_create(
                solver.q, self.dtype_code, self.n, self.nnz, _ptr(self.crow), _ptr(self.col),
                _ptr(self.row_scale), _ptr(self.col_scale),
                _lib.ST_CSR_EMPTY_ROWS_OK if allow_empty_rows else 0,
                ctypes.byref(self.handle)), "st_csr_pattern_create")
        finally:
            if own:
                solver.close()
        self.allow_empty_rows = allow_empty_rows
        self._read_empty()

    def _read_empty(self) -> None:
        k, lo = ctypes.c_uint32(), ctypes.c_uint32()
        _lib.check(self.L.st_csr_pattern_empty_rows(self.handle, ctypes.byref(k),
                                                    ctypes.byref(lo)),
                   "st_csr_pattern_empty_rows")
        self.empty_rows, self.first_empty = int(k.value), int(lo.value)

    def plan(self):
        """``(order, class_first)`` of the handle (``st_csr_pattern_get_plan``)."""
        import numpy as np
        order = np.zeros(self.n, dtype=np.uint32)
        first = np.zeros(_lib.ST_CSR_CLASSES + 1, dtype=np.uint32)
        _lib.check(self.L.st_csr_pattern_get_plan(self.handle, order.ctypes.data,
                                                  first.ctypes.data),
                   "st_csr_pattern_get_plan")
        return order, first

    def transpose(self, solver: Optional["DeviceSolver"] = None,
                  allow_empty: bool = False) -> "CsrPattern":
        """T(P) with the scales swapped (``st_csr_pattern_transpose``): the two
        index arrays are byte for byte ``CsrMatrix.transpose``'s on the same
        pattern.  Raises ``EigenValueError`` naming the lowest column without
        an entry unless ``allow_empty``.  The result shares the scale tensors
        and is otherwise independent of this object."""
        if not isinstance(allow_empty, bool):
            raise TypeError(f"allow_empty must be a bool, got {type(allow_empty).__name__}")
        torch = _torch()
        if not self.handle.value:
            raise ValueError("the pattern is closed")
        t = object.__new__(CsrPattern)
        t.handle = ctypes.c_void_p()
        t.L = self.L
        t.dtype, t.dtype_code = self.dtype, self.dtype_code
        t.n, t.nnz, t.device = self.n, self.nnz, self.device
        t.row_scale, t.col_scale = self.col_scale, self.row_scale
        t.crow = torch.empty(self.n + 1, dtype=torch.int64, device=self.device)
        t.col = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
        own = solver is None
        solver = solver or DeviceSolver(self.device)
        try:
            _lib.check(self.L.st_set_stream(solver.q, _stream(self.device)), "st_set_stream")
            _lib.check(self.L.st_csr_pattern_transpose(
                solver.q, self.handle, _ptr(t.crow), _ptr(t.col),
                _lib.ST_CSR_EMPTY_ROWS_OK if allow_empty else 0, ctypes.byref(t.handle)),
                "st_csr_pattern_transpose")
        finally:
            if own:
                solver.close()
        t.allow_empty_rows = allow_empty
        t._read_empty()
        return t

    @property
    def T(self) -> "CsrPattern":
        """``transpose()``, built at the first use and kept; closed with this
        object."""
        if self._t is None:
            self._t = self.transpose()
        return self._t

    def close(self) -> None:
        if self._t is not None:
            self._t.close()
            self._t = None
        if self.handle is not None and self.handle.value:
            self.L.st_csr_pattern_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_transpose_host(indptr, indices, data, allow_empty: bool = False):
    """T(A) of host (numpy) CSR arrays by the library's host twin
    (``st_csr_transpose_host``; no GPU): ``(t_indptr, t_indices, t_data)``.
    ``allow_empty``: empty rows and columns are legal
    (``st_csr_transpose_host_ex``)."""
    return _lib.csr_transpose_host(indptr, indices, data, allow_empty=allow_empty)


class CsrTerms:
    """The rank-one terms of the operator ``M = A + sum_j u_j w_j^T``
    (``st_csr_terms_create``): ``u`` and ``w`` are [K, n] tensors or sequences
    of K vectors [n] on the matrix's device and of its dtype, 1 <= K <=
    ``ST_CSR_TERMS_MAX``, nonnegative and finite.  The vectors are kept alive
    (contiguous copies are made only where needed).  Shapes, dtypes and
    devices are checked here before any library call; the entries and the rows
    of ``M`` on the device (``EigenValueError`` naming the term, the vector
    and the index, or the row without a positive entry).  Bound to ``csr``:
    every call refuses it with another matrix.  ``csr`` may be a
    ``CsrPattern`` (``st_csr_pattern_terms_create``): the terms then serve
    ``solve_csr_pattern`` and the ``csr_pattern_*`` steps."""

    def __init__(self, csr, u, w, *, solver: Optional["DeviceSolver"] = None):
        torch = _torch()
        if not isinstance(csr, (CsrMatrix, CsrPattern)):
            raise TypeError(f"a CsrMatrix required, got {type(csr).__name__}")
        if not csr.handle.value:
            raise ValueError("the matrix is closed")
        self.handle = ctypes.c_void_p()
        self.L = csr.L
        self.K = _lib.check_terms_arg(u, w, csr.n)
        for name, vs in (("u", u), ("w", w)):
            for j, x in enumerate(vs):
                if not isinstance(x, torch.Tensor):
                    raise TypeError(f"terms: {name}_{j} must be a torch tensor, got "
                                    f"{type(x).__name__}")
                if x.dtype != csr.dtype:
                    raise TypeError(f"terms: {name}_{j} is {x.dtype}, the matrix {csr.dtype}")
                if x.device != csr.device:
                    raise ValueError(f"terms: {name}_{j} on {x.device}, the matrix on "
                                     f"{csr.device}")
        self.csr = csr
        self.u = [x.contiguous() for x in u]
        self.w = [x.contiguous() for x in w]
        self._left = None
        pu = (ctypes.c_void_p * self.K)(*[_ptr(x) for x in self.u])
        pw = (ctypes.c_void_p * self.K)(*[_ptr(x) for x in self.w])
        own = solver is None
        solver = solver or DeviceSolver(csr.device)
        try:
            _lib.check(self.L.st_set_stream(solver.q, _stream(csr.device)), "st_set_stream")
            if isinstance(csr, CsrPattern):
                _lib.check(self.L.st_csr_pattern_terms_create(
                    solver.q, csr.handle, self.K, pu, pw, ctypes.byref(self.handle)),
                    "st_csr_pattern_terms_create")
            else:
                _lib.check(self.L.st_csr_terms_create(solver.q, csr.handle, self.K, pu, pw,
                                                      ctypes.byref(self.handle)),
                           "st_csr_terms_create")
        finally:
            if own:
                solver.close()

    def scratch(self):
        """A fresh scratch tensor for ``csr_terms_rowsum`` / ``csr_terms_round``
        (``st_csr_terms_scratch_bytes``)."""
        torch = _torch()
        nbytes = int(self.L.st_csr_terms_scratch_bytes(self.csr.n, self.K))
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.csr.device)

    def dots(self, scratch):
        """dots[K] as the last ``csr_terms_rowsum`` / ``csr_terms_round`` left
        them at the start of ``scratch``."""
        es = 8 if self.csr.dtype_code else 4
        return scratch[:self.K * es].view(self.csr.dtype).clone()

    def x(self, scratch):
        """x = v_prev * s_prev as the last ``csr_terms_round`` left it."""
        off = 256 + self.K * 2048 * 8
        es = 8 if self.csr.dtype_code else 4
        return scratch[off:off + self.csr.n * es].view(self.csr.dtype).clone()

    def close(self) -> None:
        if self._left is not None:
            tt, at = self._left
            self._left = None
            tt.close()
            at.close()
        if self.handle is not None and self.handle.value:
            self.L.st_csr_terms_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_terms_rowsum(csr: CsrMatrix, terms: CsrTerms, scratch, out=None):
    """s_0 of ``A + sum u w^T`` (``st_csr_terms_rowsum``): launch 0 with
    terms; ``terms.dots(scratch)`` is then w_j . 1."""
    torch = _torch()
    if out is None:
        out = torch.empty(csr.n, dtype=csr.dtype, device=csr.device)
    _check_cuda(out, scratch)
    assert out.dtype == csr.dtype and out.numel() >= csr.n
    _lib.check(_lib.load().st_csr_terms_rowsum(csr.handle, terms.handle, _ptr(out),
                                               _ptr(scratch), _stream(csr.device)),
               "csr_terms_rowsum")
    return out


def csr_terms_round(csr: CsrMatrix, terms: CsrTerms, s_prev, s_next, v_prev, v_cur, scratch,
                    state, *, eps: float = 1e-3, k: int = 1, max_itr: int = _lib.ST_MAX_ITR,
                    semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Launch k >= 1 on ``A + sum u w^T`` (``st_csr_terms_round``):
    ``csr_mfree_round``'s contract in three launches; ``terms.dots(scratch)``
    is then w_j . x and ``terms.x(scratch)`` x itself."""
    _check_cuda(s_prev, s_next, v_prev, v_cur, scratch, state)
    assert all(t.dtype == csr.dtype and t.numel() >= csr.n and t.is_contiguous()
               for t in (s_prev, s_next, v_prev, v_cur))
    _lib.check(_lib.load().st_csr_terms_round(
        csr.handle, terms.handle, _ptr(s_prev), _ptr(s_next), _ptr(v_prev), _ptr(v_cur),
        _ptr(scratch), float(eps), k, max_itr, semantics, _ptr(state), _stream(csr.device)),
        "csr_terms_round")


def _check_pattern(pat, name: str = "pat") -> None:
    if not isinstance(pat, CsrPattern):
        raise TypeError(f"{name}: a CsrPattern required, got {type(pat).__name__}")
    if not pat.handle.value:
        raise ValueError(f"{name}: the pattern is closed")


def _check_pattern_terms(pat, terms) -> None:
    if terms is not None:
        if not isinstance(terms, CsrTerms):
            raise TypeError(f"terms must be a CsrTerms, got {type(terms).__name__}")
        if terms.csr is not pat:
            raise ValueError("terms were made for another matrix")


def csr_pattern_scratch(pat: CsrPattern, terms: Optional[CsrTerms] = None):
    """A fresh scratch tensor for ``csr_pattern_rowsum`` / ``csr_pattern_round``
    (``st_csr_pattern_scratch_bytes(n, K)``, K = 0 without terms): dots and
    partials first (``terms.dots(scratch)``), then z (``csr_pattern_z``)."""
    torch = _torch()
    _check_pattern(pat)
    K = 0 if terms is None else terms.K
    nbytes = int(pat.L.st_csr_pattern_scratch_bytes(pat.n, K))
    return torch.zeros(nbytes, dtype=torch.uint8, device=pat.device)


def csr_pattern_z(pat: CsrPattern, scratch, terms: Optional[CsrTerms] = None):
    """z = col_scale * x as the last ``csr_pattern_round`` left it (x itself
    without a column scale)."""
    K = 0 if terms is None else terms.K
    off = 256 + K * 2048 * 8
    es = 8 if pat.dtype_code else 4
    return scratch[off:off + pat.n * es].view(pat.dtype).clone()


def csr_pattern_rowsum(pat: CsrPattern, terms: Optional[CsrTerms] = None, scratch=None,
                       out=None):
    """s_0 = row_scale * (P col_scale), plus the terms (``st_csr_pattern_rowsum``):
    launch 0 of the pattern scheme.  ``scratch`` is needed with terms only."""
    torch = _torch()
    _check_pattern(pat)
    _check_pattern_terms(pat, terms)
    if out is None:
        out = torch.empty(pat.n, dtype=pat.dtype, device=pat.device)
    if scratch is None and terms is not None:
        scratch = csr_pattern_scratch(pat, terms)
    _check_cuda(out, scratch)
    assert out.dtype == pat.dtype and out.numel() >= pat.n
    _lib.check(_lib.load().st_csr_pattern_rowsum(
        pat.handle, None if terms is None else terms.handle, _ptr(out), _ptr(scratch),
        _stream(pat.device)), "csr_pattern_rowsum")
    return out


def csr_pattern_round(pat: CsrPattern, terms: Optional[CsrTerms], s_prev, s_next, v_prev,
                      v_cur, scratch, state, *, eps: float = 1e-3, k: int = 1,
                      max_itr: int = _lib.ST_MAX_ITR,
                      semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Launch k >= 1 on the pattern operator (``st_csr_pattern_round``):
    ``csr_mfree_round``'s contract (``csr_terms_round``'s with terms); a no-op
    once the state's ``end`` is set and below k."""
    _check_pattern(pat)
    _check_pattern_terms(pat, terms)
    _check_cuda(s_prev, s_next, v_prev, v_cur, scratch, state)
    assert all(t.dtype == pat.dtype and t.numel() >= pat.n and t.is_contiguous()
               for t in (s_prev, s_next, v_prev, v_cur))
    _lib.check(_lib.load().st_csr_pattern_round(
        pat.handle, None if terms is None else terms.handle, _ptr(s_prev), _ptr(s_next),
        _ptr(v_prev), _ptr(v_cur), _ptr(scratch), float(eps), k, max_itr, semantics,
        _ptr(state), _stream(pat.device)), "csr_pattern_round")


class CsrMultiTerms:
    """C term sets on one matrix, ``M_c = A + sum_j u_cj w_cj^T``
    (``st_csr_multi_create``): ``u`` and ``w`` are [C, K, n] tensors ([C, n]
    means K = 1) or sequences of C entries ``CsrTerms`` accepts, 1 <= C <=
    ``ST_CSR_MULTI_MAX``, the same K for every column (a column that needs
    fewer terms pads with u = 0, which changes no bit).  The library packs its
    own copies [n, CP] (``self.CP`` = 2, 4 or 8 >= C), so the vectors need not
    be kept.  Shapes, dtypes and devices are checked here before any library
    call; the entries and the rows of every ``M_c`` on the device
    (``EigenValueError`` naming the column first).  Bound to ``csr``: every
    call refuses it with another matrix."""

    def __init__(self, csr: CsrMatrix, u, w, *, solver: Optional["DeviceSolver"] = None):
        torch = _torch()
        if not isinstance(csr, CsrMatrix):
            raise TypeError(f"a CsrMatrix required, got {type(csr).__name__}")
        if not csr.handle.value:
            raise ValueError("the matrix is closed")
        self.handle = ctypes.c_void_p()
        self.L = csr.L
        self.C, self.K, uu, ww = _lib.check_multi_terms_arg(u, w, csr.n)
        self.CP = _lib.csr_multi_cp(self.C)
        for name, cols in (("u", uu), ("w", ww)):
            for c, vs in enumerate(cols):
                for j, x in enumerate(vs):
                    if not isinstance(x, torch.Tensor):
                        raise TypeError(f"multi terms: column {c}: {name}_{j} must be a torch "
                                        f"tensor, got {type(x).__name__}")
                    if x.dtype != csr.dtype:
                        raise TypeError(f"multi terms: column {c}: {name}_{j} is {x.dtype}, the "
                                        f"matrix {csr.dtype}")
                    if x.device != csr.device:
                        raise ValueError(f"multi terms: column {c}: {name}_{j} on {x.device}, "
                                         f"the matrix on {csr.device}")
        self.csr = csr
        fu = [x.contiguous() for vs in uu for x in vs]           # [c * K + j], alive for the call
        fw = [x.contiguous() for vs in ww for x in vs]
        pu = (ctypes.c_void_p * len(fu))(*[_ptr(x) for x in fu])
        pw = (ctypes.c_void_p * len(fw))(*[_ptr(x) for x in fw])
        own = solver is None
        solver = solver or DeviceSolver(csr.device)
        try:
            _lib.check(self.L.st_set_stream(solver.q, _stream(csr.device)), "st_set_stream")
            _lib.check(self.L.st_csr_multi_create(solver.q, csr.handle, self.C, self.K, pu, pw,
                                                  ctypes.byref(self.handle)),
                       "st_csr_multi_create")
        finally:
            if own:
                solver.close()

    def scratch(self):
        """A fresh scratch tensor for ``csr_multi_rowsum`` / ``csr_multi_round``
        (``st_csr_multi_scratch_bytes``)."""
        torch = _torch()
        nbytes = int(self.L.st_csr_multi_scratch_bytes(self.csr.n, self.C, self.K))
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.csr.device)

    def packed(self, value: float = 1.0):
        """A packed vector [n, CP] of the matrix's dtype filled with ``value``."""
        torch = _torch()
        return torch.full((self.csr.n, self.CP), value, dtype=self.csr.dtype,
                          device=self.csr.device)

    def new_states(self):
        """C zeroed ``st_state`` ([C, 64] uint8) and the finished counter."""
        torch = _torch()
        return (torch.zeros((self.C, 64), dtype=torch.uint8, device=self.csr.device),
                torch.zeros(1, dtype=torch.int32, device=self.csr.device))

    def dots(self, scratch):
        """dots [C, K] as the last ``csr_multi_rowsum`` / ``csr_multi_round``
        left them at the start of ``scratch``."""
        es = 8 if self.csr.dtype_code else 4
        return scratch[:self.C * self.K * es].view(self.csr.dtype).clone().view(self.C, self.K)

    def x(self, scratch):
        """x [n, CP] = v_prev * s_prev as the last ``csr_multi_round`` left it."""
        off = 256 + self.CP * self.K * 2048 * 8
        es = 8 if self.csr.dtype_code else 4
        return (scratch[off:off + self.csr.n * self.CP * es].view(self.csr.dtype).clone()
                .view(self.csr.n, self.CP))

    def close(self) -> None:
        if self.handle is not None and self.handle.value:
            self.L.st_csr_multi_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_multi_rowsum(csr: CsrMatrix, mterms: CsrMultiTerms, scratch, out=None):
    """s_0 of every ``M_c``, packed [n, CP] (``st_csr_multi_rowsum``): column
    c is ``csr_terms_rowsum``'s on that column's terms, bit for bit;
    ``mterms.dots(scratch)`` is then w_cj . 1."""
    if out is None:
        out = mterms.packed()
    _check_cuda(out, scratch)
    assert out.dtype == csr.dtype and out.numel() >= csr.n * mterms.CP and out.is_contiguous()
    _lib.check(_lib.load().st_csr_multi_rowsum(csr.handle, mterms.handle, _ptr(out),
                                               _ptr(scratch), _stream(csr.device)),
               "csr_multi_rowsum")
    return out


def csr_multi_round(csr: CsrMatrix, mterms: CsrMultiTerms, s_prev, s_next, v_prev, v_cur,
                    scratch, states, finished, *, eps: float = 1e-3, k: int = 1,
                    max_itr: int = _lib.ST_MAX_ITR, semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Launch k >= 1 of every ``M_c`` (``st_csr_multi_round``) on packed
    vectors [n, CP]: one pass over the matrix for all columns, column c bit for
    bit ``csr_terms_round``'s.  ``states``: [C, 64] uint8; ``finished``: one
    int32 word.  A column whose state has ``end`` set and below k, and a
    padding column, get no write."""
    _check_cuda(s_prev, s_next, v_prev, v_cur, scratch, states, finished)
    assert all(t.dtype == csr.dtype and t.numel() >= csr.n * mterms.CP and t.is_contiguous()
               for t in (s_prev, s_next, v_prev, v_cur))
    assert states.numel() >= 64 * mterms.C and states.is_contiguous()
    _lib.check(_lib.load().st_csr_multi_round(
        csr.handle, mterms.handle, _ptr(s_prev), _ptr(s_next), _ptr(v_prev), _ptr(v_cur),
        _ptr(scratch), float(eps), k, max_itr, semantics, _ptr(states), _ptr(finished),
        _stream(csr.device)), "csr_multi_round")


def csr_rowsum(csr: CsrMatrix, out=None):
    """s[r] = the sum of row r's entries (``st_csr_rowsum``): launch 0 of the
    CSR matrix-free scheme."""
    torch = _torch()
    if out is None:
        out = torch.empty(csr.n, dtype=csr.dtype, device=csr.device)
    _check_cuda(out)
    assert out.dtype == csr.dtype and out.numel() >= csr.n
    _lib.check(_lib.load().st_csr_rowsum(csr.handle, _ptr(out), _stream(csr.device)),
               "csr_rowsum")
    return out


def csr_mfree_round(csr: CsrMatrix, s_prev, s_next, v_prev, v_cur, x, state, *,
                    eps: float = 1e-3, k: int = 1, max_itr: int = _lib.ST_MAX_ITR,
                    semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Matrix-free launch k >= 1 on a CSR matrix (``st_csr_mfree_round``):
    mfree_round's contract in two launches; ``x`` is scratch of n elements.
    v_cur and the state are bit for bit mfree_round's on the densified matrix."""
    _check_cuda(s_prev, s_next, v_prev, v_cur, x, state)
    assert all(t.dtype == csr.dtype and t.numel() >= csr.n and t.is_contiguous()
               for t in (s_prev, s_next, v_prev, v_cur, x))
    _lib.check(_lib.load().st_csr_mfree_round(
        csr.handle, _ptr(s_prev), _ptr(s_next), _ptr(v_prev), _ptr(v_cur), _ptr(x), float(eps),
        k, max_itr, semantics, _ptr(state), _stream(csr.device)), "csr_mfree_round")


def _check_csr(csr, name: str = "csr") -> None:
    if not isinstance(csr, CsrMatrix):
        raise TypeError(f"{name}: a CsrMatrix required, got {type(csr).__name__}")
    if not csr.handle.value:
        raise ValueError(f"{name}: the matrix is closed")


def _check_product_pair(B, A) -> None:
    """What every Python front checks of the factors of ``B·A`` before any
    library call, in the library's order: both alive, same n, dtype, device."""
    _check_csr(B, "B")
    _check_csr(A, "A")
    if B.n != A.n:
        raise ValueError(f"product: the factors differ in n (B: {B.n}, A: {A.n})")
    if B.dtype != A.dtype:
        raise TypeError(f"product: the factors differ in dtype (B: {B.dtype}, A: {A.dtype})")
    if B.device != A.device:
        raise ValueError(f"product: the factors live on different devices (B: {B.device}, "
                         f"A: {A.device})")


def csr_apply(csr: CsrMatrix, x, out=None):
    """``y = A x`` (``st_csr_apply``): the plain CSR row product in the solve's
    fixed summation order - a reproducible SpMV.  No division; an empty row
    gives exactly 0.  ``x`` [n] of the matrix's dtype and device; ``out`` must
    not be ``x``."""
    torch = _torch()
    _check_csr(csr)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a torch tensor, got {type(x).__name__}")
    if x.dtype != csr.dtype:
        raise TypeError(f"x is {x.dtype}, the matrix {csr.dtype}")
    if tuple(x.shape) != (csr.n,):
        raise ValueError(f"x has shape {tuple(x.shape)}, ({csr.n},) required")
    if x.device != csr.device:
        raise ValueError(f"x on {x.device}, the matrix on {csr.device}")
    x = x.contiguous()
    if out is None:
        out = torch.empty(csr.n, dtype=csr.dtype, device=csr.device)
    _check_cuda(out)
    assert out.dtype == csr.dtype and out.numel() >= csr.n and out.is_contiguous()
    _lib.check(_lib.load().st_csr_apply(csr.handle, _ptr(x), _ptr(out), _stream(csr.device)),
               "csr_apply")
    return out


def csr_product_scratch(A: CsrMatrix):
    """A fresh scratch tensor for ``csr_product_rowsum`` / ``csr_product_round``
    (``st_csr_product_scratch_bytes``): x in its first half, y in its second."""
    torch = _torch()
    nbytes = int(_lib.load().st_csr_product_scratch_bytes(A.n))
    return torch.zeros(nbytes, dtype=torch.uint8, device=A.device)


def csr_product_rowsum(B: CsrMatrix, A: CsrMatrix, scratch, out=None):
    """s_0 of ``B·A`` (``st_csr_product_rowsum``): launch 0 - the row sums of
    ``A`` into the scratch's second half, then ``B`` applied to them."""
    torch = _torch()
    _check_product_pair(B, A)
    if out is None:
        out = torch.empty(A.n, dtype=A.dtype, device=A.device)
    _check_cuda(out, scratch)
    assert out.dtype == A.dtype and out.numel() >= A.n
    _lib.check(_lib.load().st_csr_product_rowsum(B.handle, A.handle, _ptr(out), _ptr(scratch),
                                                 _stream(A.device)), "csr_product_rowsum")
    return out


def csr_product_round(B: CsrMatrix, A: CsrMatrix, s_prev, s_next, v_prev, v_cur, scratch,
                      state, *, eps: float = 1e-3, k: int = 1,
                      max_itr: int = _lib.ST_MAX_ITR,
                      semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Launch k >= 1 on ``B·A`` (``st_csr_product_round``): ``csr_mfree_round``'s
    contract in three launches - x = v_prev * s_prev, y = A x, s_next = (B y) /
    x; x and y stand in the two halves of ``scratch`` afterwards."""
    _check_product_pair(B, A)
    _check_cuda(s_prev, s_next, v_prev, v_cur, scratch, state)
    assert all(t.dtype == A.dtype and t.numel() >= A.n and t.is_contiguous()
               for t in (s_prev, s_next, v_prev, v_cur))
    _lib.check(_lib.load().st_csr_product_round(
        B.handle, A.handle, _ptr(s_prev), _ptr(s_next), _ptr(v_prev), _ptr(v_cur),
        _ptr(scratch), float(eps), k, max_itr, semantics, _ptr(state), _stream(A.device)),
        "csr_product_round")


class CsrBatch:
    """Many nonnegative sparse matrices in STACKED CSR storage on the device,
    validated and planned (``st_csr_batch_create``): ``crow_indices`` int64
    [N + 1] over the concatenated entries, ``col_indices`` int32 [nnz] LOCAL
    to their matrix, ``values`` float32 / float64 [nnz], and ``mat_first``
    (host integers [B + 1]: the first stacked row of each matrix,
    ``mat_first[B] == N``).  Index dtypes are converted as needed, nothing
    else is copied.  ``CsrBatch.from_matrices`` builds one from single
    matrices.  Raises ``EigenValueError`` naming the matrix and its local row
    or entry when the check rejects the arrays; no handle exists then."""

    def __init__(self, crow_indices, col_indices, values, mat_first, *,
                 solver: Optional["DeviceSolver"] = None):
        import numpy as np
        torch = _torch()
        self.handle = ctypes.c_void_p()
        self.L = _lib.load()
        _check_cuda(crow_indices, col_indices, values)
        mf = np.asarray(mat_first)
        if mf.ndim != 1 or mf.size < 2 or mf.dtype.kind not in "iu":
            raise ValueError("mat_first must hold B + 1 >= 2 integers")
        if (mf < 0).any() or (mf >= 2**32).any():
            raise ValueError("mat_first does not fit uint32")
        self.mat_first = np.ascontiguousarray(mf, dtype=np.uint32)
        self.batch = int(mf.size - 1)
        self.n = int(crow_indices.numel() - 1)
        if int(self.mat_first[-1]) != self.n:
            raise ValueError(f"mat_first[B] = {int(self.mat_first[-1])} must be N = "
                             f"{self.n} (crow_indices has N + 1 elements)")
        if col_indices.numel() != values.numel():
            raise ValueError("col_indices and values differ in length")
        self.dtype_code = 1 if _sfx(values) == "f64" else 0
        self.crow = crow_indices.to(torch.int64).contiguous()
        self.col = col_indices.to(torch.int32).contiguous()
        self.values = values.contiguous()
        self.nnz = int(values.numel())
        self.device = values.device
        own = solver is None
        solver = solver or DeviceSolver(self.device)
        try:
            _lib.check(self.L.st_set_stream(solver.q, _stream(self.device)), "st_set_stream")
            _lib.check(self.L.st_csr_batch_create(
                solver.q, self.dtype_code, self.batch, self.mat_first.ctypes.data, self.nnz,
                _ptr(self.crow), _ptr(self.col), _ptr(self.values),
                ctypes.byref(self.handle)), "st_csr_batch_create")
        finally:
            if own:
                solver.close()

    @classmethod
    def from_matrices(cls, mats, *, solver: Optional["DeviceSolver"] = None):
        """From a sequence of ``(crow, col, values)`` triples of device tensors
        or ``torch.sparse_csr`` tensors (square, one dtype, one device):
        concatenated on the device, ``crow`` rebased, columns left as they
        are."""
        torch = _torch()
        trip = []
        for m in mats:
            if isinstance(m, (tuple, list)):
                if len(m) != 3:
                    raise ValueError("a matrix is a (crow, col, values) triple")
                trip.append(tuple(m))
            elif getattr(m, "layout", None) == torch.sparse_csr:
                assert m.dim() == 2 and m.shape[0] == m.shape[1], "must be square"
                if m.crow_indices().numel() != m.shape[0] + 1:
                    raise ValueError("crow_indices must have n + 1 elements")
                trip.append((m.crow_indices(), m.col_indices(), m.values()))
            else:
                raise TypeError("(crow, col, values) triples or torch.sparse_csr tensors "
                                f"required, got {type(m).__name__}")
        if not trip:
            raise ValueError("a CsrBatch needs at least one matrix")
        dt = trip[0][2].dtype
        for crow, col, vals in trip:
            if vals.dtype != dt:
                raise ValueError("all matrices must have one dtype")
            if crow.numel() < 2:
                raise ValueError("every matrix needs at least one row")
            if col.numel() != vals.numel():
                raise ValueError("col_indices and values differ in length")
        mat_first = [0]
        for crow, _, _ in trip:
            mat_first.append(mat_first[-1] + int(crow.numel()) - 1)
        parts = [torch.zeros(1, dtype=torch.int64, device=trip[0][0].device)]
        base = parts[0][0]
        for crow, _, _ in trip:                    # rebased on the device
            c = crow.to(torch.int64)
            parts.append(c[1:] - c[0] + base)
            base = parts[-1][-1]
        return cls(torch.cat(parts), torch.cat([t[1].to(torch.int32) for t in trip]),
                   torch.cat([t[2] for t in trip]), mat_first, solver=solver)

    @property
    def dtype(self):
        return self.values.dtype

    def plan(self):
        """``(order, class_first)`` over the N stacked rows
        (``st_csr_batch_get_plan``): ``st_csr_plan`` of the stacked
        ``crow_indices``."""
        import numpy as np
        order = np.zeros(self.n, dtype=np.uint32)
        first = np.zeros(_lib.ST_CSR_CLASSES + 1, dtype=np.uint32)
        _lib.check(self.L.st_csr_batch_get_plan(self.handle, order.ctypes.data,
                                                first.ctypes.data), "st_csr_batch_get_plan")
        return order, first

    def close(self) -> None:
        if self.handle is not None and self.handle.value:
            self.L.st_csr_batch_destroy(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def csr_batch_rowsum(batch: CsrBatch, out=None):
    """s[r] = the sum of stacked row r's entries (``st_csr_batch_rowsum``):
    launch 0 of the batched CSR scheme."""
    torch = _torch()
    if out is None:
        out = torch.empty(batch.n, dtype=batch.dtype, device=batch.device)
    _check_cuda(out)
    assert out.dtype == batch.dtype and out.numel() >= batch.n
    _lib.check(_lib.load().st_csr_batch_rowsum(batch.handle, _ptr(out), _stream(batch.device)),
               "csr_batch_rowsum")
    return out


def csr_batch_mfree_round(batch: CsrBatch, s_prev, s_next, v_prev, v_cur, x, states, finished,
                          *, eps: float = 1e-3, k: int = 1, max_itr: int = _lib.ST_MAX_ITR,
                          semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Launch k >= 1 for a whole batch (``st_csr_batch_mfree_round``):
    ``csr_mfree_round``'s contract for every matrix at once.  Vectors are
    stacked [N]; ``states`` holds B states (64 bytes each, zero = fresh),
    ``finished`` one uint32 / int32 word counting the matrices that ended."""
    _check_cuda(s_prev, s_next, v_prev, v_cur, x, states, finished)
    assert all(t.dtype == batch.dtype and t.numel() >= batch.n and t.is_contiguous()
               for t in (s_prev, s_next, v_prev, v_cur, x))
    assert states.is_contiguous() and states.numel() * states.element_size() >= 64 * batch.batch
    assert finished.numel() * finished.element_size() >= 4
    _lib.check(_lib.load().st_csr_batch_mfree_round(
        batch.handle, _ptr(s_prev), _ptr(s_next), _ptr(v_prev), _ptr(v_cur), _ptr(x),
        float(eps), k, max_itr, semantics, _ptr(states), _ptr(finished),
        _stream(batch.device)), "csr_batch_mfree_round")


def flat_round_pays(nrows: int, ncols: int, dtype) -> bool:
    """Whether the flat round (st_round_flat) is the faster form for a block."""
    torch = _torch()
    return bool(_lib.load().st_round_flat_pays(nrows, ncols,
                                               1 if dtype == torch.float64 else 0))


def flat_scratch(nrows: int, ncols: int, dtype, device=None):
    """Partial-sum scratch for flat_round on this block."""
    torch = _torch()
    n = int(_lib.load().st_round_flat_scratch(nrows, ncols))
    return torch.empty(n, dtype=dtype, device=device or "cuda")


def flat_round(mat, s_cur, s_next, part, v, state, *, row0: int = 0, eps: float = 1e-3,
               k: int = 0, max_itr: int = _lib.ST_MAX_ITR,
               semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Round k as two launches for large blocks (st_round_flat): the
    transform in short per-piece workgroups (the first row group also takes
    the stats of the full s_cur), then the pieces' partial sums into s_next
    and the v update.  Same contract as fused_round."""
    _check_cuda(mat, s_cur, s_next, part, v, state)
    assert mat.is_contiguous() and mat.dim() == 2
    nrows, ncols = mat.shape
    assert s_cur.numel() >= ncols and s_next.numel() >= nrows and v.numel() >= ncols
    assert row0 + nrows <= ncols
    assert part.numel() >= int(_lib.load().st_round_flat_scratch(nrows, ncols))
    _lib.check(getattr(_lib.load(), f"st_round_flat_{_sfx(mat)}")(
        _ptr(mat), _ptr(s_cur), _ptr(s_next), _ptr(part), _ptr(v), nrows, ncols, row0,
        eps, k, max_itr, semantics, _ptr(state), _stream(mat.device)), "round_flat")


def set_flat_grid_limit(max_x: int = 0) -> int:
    """Testing hook (st_set_flat_grid_limit, include/st_tuning.h): the width
    past which the flat launches go 2-D (0 = the default, the dispatch
    limit).  Returns the limit in force.  The tuning build only: the
    package's library must be libsimilarity_transform_tuning.so
    (EIGEN_VALUE_LIB), whose launches the limit then moves."""
    L = _lib.load()
    if not hasattr(L, "st_set_flat_grid_limit"):
        raise _lib.EigenValueError("st_set_flat_grid_limit: the tuning build only "
                                   "(EIGEN_VALUE_LIB=" + _lib.TUNING_LIB + ")")
    return int(L.st_set_flat_grid_limit(max_x))


def defer_rounds(nrows: int, ncols: int, dtype) -> int:
    """Rounds per store of the deferred flat round on a block
    (st_defer_rounds)."""
    torch = _torch()
    return int(_lib.load().st_defer_rounds(nrows, ncols,
                                           1 if dtype == torch.float64 else 0))


def recip(s, inv) -> None:
    """inv = 1 / s elementwise (st_recip), the reciprocals the deferred round
    re-applies."""
    _check_cuda(s, inv)
    assert inv.numel() >= s.numel() and inv.dtype == s.dtype
    _lib.check(getattr(_lib.load(), f"st_recip_{_sfx(s)}")(
        _ptr(s), _ptr(inv), s.numel(), _stream(s.device)), "recip")


def flat_round_deferred(mat, s_cur, inv_cur, s_next, inv_next, part, v, state,
                        pend_s=(), pend_inv=(), *, store: bool, flush: bool = False,
                        row0: int = 0, eps: float = 1e-3, k: int = 0,
                        max_itr: int = _lib.ST_MAX_ITR,
                        semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Round k of the flat round with deferred writes
    (st_round_flat_deferred): ``mat`` holds the last STORED matrix A_j,
    ``pend_s`` / ``pend_inv`` the pending rounds' full row-sum vectors
    s_j .. s_{k-1} and their reciprocals; A_{k+1} is stored when ``store``.
    s_next / inv_next are the block's slots (as in flat_round).  ``flush``
    (with ``store``) only stores A_{k+1}.  Bit-identical to flat_round on a
    matrix stored every round."""
    import ctypes
    _check_cuda(mat, s_cur, inv_cur, part, v, state, *pend_s, *pend_inv)
    m = defer_rounds(*mat.shape, mat.dtype)
    assert len(pend_s) == len(pend_inv) < m
    # the round with m - 1 pending is the group's storing round
    assert store or len(pend_s) + 1 < m, "a round with m - 1 pending rounds must store"
    assert mat.is_contiguous() and mat.dim() == 2
    nrows, ncols = mat.shape
    assert s_cur.numel() >= ncols and inv_cur.numel() >= ncols and v.numel() >= ncols
    assert all(x.numel() >= ncols for x in (*pend_s, *pend_inv))
    assert row0 + nrows <= ncols
    assert part.numel() >= int(_lib.load().st_round_flat_scratch(nrows, ncols))
    if not flush:
        _check_cuda(s_next, inv_next)
        assert s_next.numel() >= nrows and inv_next.numel() >= nrows
    np_ = len(pend_s)
    arr_s = (ctypes.c_void_p * max(1, np_))(*[_ptr(x) for x in pend_s])
    arr_i = (ctypes.c_void_p * max(1, np_))(*[_ptr(x) for x in pend_inv])
    _lib.check(getattr(_lib.load(), f"st_round_flat_deferred_{_sfx(mat)}")(
        _ptr(mat), _ptr(s_cur), _ptr(inv_cur), None if flush else _ptr(s_next),
        None if flush else _ptr(inv_next), _ptr(part), _ptr(v), nrows, ncols, row0, eps, k,
        max_itr, semantics, arr_s, arr_i, np_, int(store), int(flush), _ptr(state),
        _stream(mat.device)), "round_flat_deferred")


SPAN_LOCAL = 1
SPAN_REMOTE = 2


def split_round(mat, s_cur, s_next, part, v, state, *, span: int, row0: int = 0,
                col0: int = 0, col1: Optional[int] = None, eps: float = 1e-3, k: int = 0,
                max_itr: int = _lib.ST_MAX_ITR, semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Half of a round (st_round_split): ``span=SPAN_LOCAL`` transforms the
    columns [col0, col1) and writes their row sums to ``part``;
    ``span=SPAN_REMOTE`` does the rest of the round (m/stop/v/state from
    the full ``s_cur``, the other columns, ``s_next = part + their sum``)."""
    _check_cuda(mat, s_cur, s_next, part, v, state)
    assert mat.is_contiguous() and mat.dim() == 2
    nrows, ncols = mat.shape
    col1 = ncols if col1 is None else col1
    assert s_cur.numel() >= ncols and part.numel() >= nrows and row0 + nrows <= ncols
    assert span == SPAN_LOCAL or (s_next is not None and s_next.numel() >= nrows
                                  and v is not None and v.numel() >= ncols)
    _lib.check(getattr(_lib.load(), f"st_round_split_{_sfx(mat)}")(
        _ptr(mat), _ptr(s_cur), _ptr(s_next), _ptr(part), _ptr(v), nrows, ncols, row0,
        col0, col1, eps, k, max_itr, semantics, span, _ptr(state),
        _stream(mat.device)), "round_split")


def split_flat_scratch(nrows: int, ncols: int, col0: int, col1: int, dtype, device=None):
    """Partial-sum scratch for split_flat_round on this block and local range."""
    torch = _torch()
    n = int(_lib.load().st_round_split_flat_scratch(nrows, ncols, col0, col1))
    return torch.empty(n, dtype=dtype, device=device or "cuda")


def split_flat_round(mat, s_cur, s_next, part, v, state, *, span: int, row0: int = 0,
                     col0: int = 0, col1: Optional[int] = None, eps: float = 1e-3,
                     k: int = 0, max_itr: int = _lib.ST_MAX_ITR,
                     semantics: int = _lib.ST_SEM_SYCL) -> None:
    """split_round in the flat form (st_round_split_flat): ``part`` is the
    split_flat_scratch of this block and range, shared by both halves."""
    _check_cuda(mat, s_cur, s_next, part, v, state)
    assert mat.is_contiguous() and mat.dim() == 2
    nrows, ncols = mat.shape
    col1 = ncols if col1 is None else col1
    need = int(_lib.load().st_round_split_flat_scratch(nrows, ncols, col0, col1))
    assert s_cur.numel() >= ncols and part.numel() >= need and row0 + nrows <= ncols
    assert span == SPAN_LOCAL or (s_next is not None and s_next.numel() >= nrows
                                  and v is not None and v.numel() >= ncols)
    _lib.check(getattr(_lib.load(), f"st_round_split_flat_{_sfx(mat)}")(
        _ptr(mat), _ptr(s_cur), _ptr(s_next), _ptr(part), _ptr(v), nrows, ncols, row0,
        col0, col1, eps, k, max_itr, semantics, span, _ptr(state),
        _stream(mat.device)), "round_split_flat")


def epilogue(s, v, state, eps: float, max_itr: int = _lib.ST_MAX_ITR,
             semantics: int = _lib.ST_SEM_SYCL) -> None:
    """Round epilogue: max, v *= s/m, stop test, λ = s[0], bookkeeping."""
    _check_cuda(s, v, state)
    _lib.check(getattr(_lib.load(), f"st_epilogue_{_sfx(s)}")(
        _ptr(s), _ptr(v), s.numel(), eps, max_itr, semantics, _ptr(state),
        _stream(s.device)), "epilogue")


# --------------------------------------------------------------------------
# whole solve on a device-resident matrix
# --------------------------------------------------------------------------
def batched_max_dim(dtype) -> int:
    """Largest n ``DeviceSolver.solve_batched`` accepts for ``dtype`` (torch
    or numpy float32 / float64): 256 / 128 (st_solve_batched_max_dim)."""
    name = str(dtype).split(".")[-1].strip("'>")
    if name not in ("float32", "float64"):
        raise TypeError(f"float32/float64 required, got {dtype}")
    return int(_lib.load().st_solve_batched_max_dim(1 if name == "float64" else 0))


def batched_rounds_max_dim(dtype) -> int:
    """Largest n ``DeviceSolver.solve_batched(..., round_loop=True)`` accepts
    for ``dtype`` (torch or numpy float32 / float64): 6143 / 4344, the sizes
    below the 144 MiB flat threshold (st_solve_batched_rounds_max_dim)."""
    name = str(dtype).split(".")[-1].strip("'>")
    if name not in ("float32", "float64"):
        raise TypeError(f"float32/float64 required, got {dtype}")
    return int(_lib.load().st_solve_batched_rounds_max_dim(1 if name == "float64" else 0))



class DeviceSolver:
    """Owns one library context bound to the current torch stream."""

    def __init__(self, device=None):
        torch = _torch()
        self.device = torch.device(device or "cuda")
        self.L = _lib.load()
        with torch.cuda.device(self.device):
            self.q = ctypes.c_void_p()
            self.L.make_queue(ctypes.byref(self.q))
        if not self.q.value:
            raise _lib.EigenValueError(f"make_queue failed: {_lib.last_error()}")

    def solve(self, mat, *, inplace: bool = False, eps: Optional[float] = None,
              max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL, batch: int = 0,
              time_kernels: bool = False, matrix_free: bool = False,
              round_loop: bool = False, write_every_round: bool = False,
              trace_sums: bool = False, left: bool = False):
        """Returns (λ: float, v: tensor, iterations: int, stats: dict).

        Matrices of n <= 128 (fp64) / 256 (fp32) run the whole solve in one
        workgroup launch (bit-identical); ``round_loop`` forces one launch per
        round instead (``ST_FLAG_ROUND_LOOP``).  Matrices of >= 144 MiB
        store the transformed matrix every 6th round
        (``defer_rounds``) and re-apply the pending scalings in registers
        (identical results and final matrix, a third to 3/8 fewer bytes);
        ``write_every_round`` stores it every round
        (``ST_FLAG_WRITE_EVERY_ROUND``).

        ``mat`` is transformed in place when ``inplace`` (it is the private
        working copy the reference makes, similarity_transform.cpp:14,19)
        and then ends at A_end, end = ``stats["rounds"]``: the stopping
        round's launch still applies its transform, one more than the
        reference loop, which breaks before compute_next_matrix (cpp:45-52).
        ``matrix_free`` runs the read-only form: the
        input is never written, so no copy is made.  ``mat`` may be a torch
        tensor or any DLPack producer (``__dlpack__``) on this device.
        ``trace_sums`` records every evaluated round's row sums
        (``ST_FLAG_TRACE_SUMS``; identical results): ``last_round_sums()``.

        ``left=True`` returns the LEFT Perron vector, ``v A = λ v``
        (``st_solve_device_left_*``: the stationary distribution of a
        row-stochastic ``mat`` is ``v / v.sum()``).  It implies the read-only
        form: ``mat`` is swept by columns where it lies, never written and
        never cloned, and no transposed copy is made; ``inplace``,
        ``round_loop`` and ``write_every_round`` are ``ValueError``s with it,
        16-bit tensors a ``TypeError``.  A non-contiguous ``mat`` whose
        transpose is contiguous (``B.T`` of a row-major ``B``) IS ``Aᵀ``
        stored row-major: the ordinary matrix-free solve then runs on that
        storage, bit for bit ``solve(B, matrix_free=True)``, again without a
        copy.  Any other non-contiguous layout is solved as its contiguous
        copy.  ``last_round_sums()`` gives the column sums after
        ``trace_sums``."""
        torch = _torch()
        if not isinstance(mat, torch.Tensor) and hasattr(mat, "__dlpack__"):
            mat = torch.from_dlpack(mat)   # any DLPack producer, zero copy
        if not isinstance(left, bool):
            raise TypeError(f"left must be a bool, got {type(left).__name__}")
        if left:
            if inplace:
                raise ValueError("left=True reads the matrix only: inplace=True cannot be "
                                 "combined with it")
            if round_loop or write_every_round:
                raise ValueError("left=True: round_loop and write_every_round belong to the "
                                 "forms that write the matrix")
            if mat.dtype in (torch.float16, torch.bfloat16):
                raise TypeError("left=True needs a float32 / float64 matrix: the 16-bit "
                                f"solve (solve_half) has no left form, got {mat.dtype}")
        _check_cuda(mat)
        if mat.device.index != (self.device.index if self.device.index is not None
                                else torch.cuda.current_device()):
            raise ValueError(f"matrix on {mat.device}, solver context on {self.device}")
        n = mat.shape[0]
        assert mat.dim() == 2 and mat.shape == (n, n), "must be square"
        if inplace and not mat.is_contiguous():
            raise ValueError("inplace needs a contiguous (row-major) matrix")
        entry = "st_solve_device"
        if left and not mat.is_contiguous() and mat.t().is_contiguous():
            # Aᵀ stored row-major: its right vector is A's left one
            work, matrix_free = mat.t(), True
        elif left:
            work, matrix_free, entry = mat.contiguous(), True, "st_solve_device_left"
        else:
            work = mat if (inplace or matrix_free) else mat.clone()
            work = work.contiguous()
        v = torch.empty(n, dtype=mat.dtype, device=mat.device)
        ev = (ctypes.c_double if mat.dtype == torch.float64 else ctypes.c_float)()
        it = ctypes.c_uint32()
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | (_lib.ST_FLAG_MATRIX_FREE if matrix_free else 0)
                 | (_lib.ST_FLAG_ROUND_LOOP if round_loop else 0)
                 | (_lib.ST_FLAG_WRITE_EVERY_ROUND if write_every_round else 0)
                 | (_lib.ST_FLAG_TRACE_SUMS if trace_sums else 0))
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        stats = _lib.st_stats()
        self._trace = (n, mat.dtype)
        _lib.check(self.L.st_set_stream(self.q, _stream(mat.device)), "st_set_stream")
        rc = getattr(self.L, f"{entry}_{_sfx(mat)}")(
            self.q, _ptr(work), n, _ptr(v), None, ctypes.byref(ev), ctypes.byref(it),
            ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(rc, entry)
        return float(ev.value), v, int(it.value), stats.as_dict()

    def solve_pair(self, mat, *, eps: Optional[float] = None, max_itr: int = 0,
                   semantics: int = _lib.ST_SEM_SYCL, batch: int = 0):
        """Both Perron vectors of a dense matrix, ``A v = λ v`` and
        ``u A = λ u``, from one pass over it per round
        (``st_solve_device_pair_*``).  Returns (λ: [2] list of float, vecs:
        [2, n] tensor, iterations: [2] list of int, stats: dict); index 0 is
        the right side (``vecs[0] = v``), index 1 the left one (``vecs[1] =
        u``, bit for bit ``solve(mat, left=True)``'s).  The two sides are
        independent iterations and stop in their own rounds;
        ``stats["converged_sides"]`` says which did before ``max_itr``.

        ``mat`` (a float32 / float64 tensor or any DLPack producer, square, on
        this device) is only read and never cloned; a non-contiguous ``mat`` is
        solved as its contiguous copy; 16-bit tensors raise ``TypeError``
        (``solve_half`` has no pair form)."""
        torch = _torch()
        if not isinstance(mat, torch.Tensor) and hasattr(mat, "__dlpack__"):
            mat = torch.from_dlpack(mat)   # any DLPack producer, zero copy
        if mat.dtype in (torch.float16, torch.bfloat16):
            raise TypeError("solve_pair needs a float32 / float64 matrix: the 16-bit "
                            f"solve (solve_half) has no pair form, got {mat.dtype}")
        _check_cuda(mat)
        if mat.device.index != (self.device.index if self.device.index is not None
                                else torch.cuda.current_device()):
            raise ValueError(f"matrix on {mat.device}, solver context on {self.device}")
        n = mat.shape[0]
        assert mat.dim() == 2 and mat.shape == (n, n), "must be square"
        work = mat.contiguous()
        vecs = torch.empty((2, n), dtype=mat.dtype, device=mat.device)
        ev = ((ctypes.c_double if mat.dtype == torch.float64 else ctypes.c_float) * 2)()
        it = (ctypes.c_uint32 * 2)()
        conv = (ctypes.c_uint32 * 2)()
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, _lib.ST_FLAG_MATRIX_FREE)
        stats = _lib.st_stats()
        _lib.check(self.L.st_set_stream(self.q, _stream(mat.device)), "st_set_stream")
        rc = getattr(self.L, f"st_solve_device_pair_{_sfx(mat)}")(
            self.q, _ptr(work), n, _ptr(vecs), None, ev, it, conv, ctypes.byref(opt),
            ctypes.byref(stats))
        _lib.check(rc, "st_solve_device_pair")
        out = stats.as_dict()
        out["converged_sides"] = [int(conv[0]), int(conv[1])]
        return [float(ev[0]), float(ev[1])], vecs, [int(it[0]), int(it[1])], out

    def solve_half(self, mat, *, eps: Optional[float] = None, max_itr: int = 0,
                   semantics: int = _lib.ST_SEM_SYCL, batch: int = 0,
                   time_kernels: bool = False, trace_sums: bool = False):
        """The matrix-free solve of a ``torch.float16`` / ``torch.bfloat16``
        matrix read where it lies, 2 bytes per element and round
        (``st_solve_device_half``); vectors, stop test and arithmetic are
        float32.  Returns (λ: float, v: float32 tensor, iterations: int,
        stats: dict).

        ``mat`` (a tensor or any DLPack producer, square, on this device) is
        never written; a non-contiguous ``mat`` is solved as its contiguous
        copy.  Other dtypes raise ``TypeError`` (``solve`` takes float32 /
        float64).  ``last_round_sums()`` works after ``trace_sums``."""
        torch = _torch()
        if not isinstance(mat, torch.Tensor) and hasattr(mat, "__dlpack__"):
            mat = torch.from_dlpack(mat)   # any DLPack producer, zero copy
        storage = _storage(mat)            # TypeError before anything else
        _check_cuda(mat)
        if mat.device.index != (self.device.index if self.device.index is not None
                                else torch.cuda.current_device()):
            raise ValueError(f"matrix on {mat.device}, solver context on {self.device}")
        n = mat.shape[0]
        assert mat.dim() == 2 and mat.shape == (n, n), "must be square"
        work = mat.contiguous()
        v = torch.empty(n, dtype=torch.float32, device=mat.device)
        ev = ctypes.c_float()
        it = ctypes.c_uint32()
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | _lib.ST_FLAG_MATRIX_FREE
                 | (_lib.ST_FLAG_TRACE_SUMS if trace_sums else 0))
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        stats = _lib.st_stats()
        self._trace = (n, torch.float32)
        _lib.check(self.L.st_set_stream(self.q, _stream(mat.device)), "st_set_stream")
        rc = self.L.st_solve_device_half(
            self.q, storage, _ptr(work), n, _ptr(v), None, ctypes.byref(ev), ctypes.byref(it),
            ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(rc, "st_solve_device_half")
        return float(ev.value), v, int(it.value), stats.as_dict()

    def solve_csr(self, csr: "CsrMatrix", terms: Optional["CsrTerms"] = None, *,
                  eps: Optional[float] = None, max_itr: int = 0,
                  semantics: int = _lib.ST_SEM_SYCL, batch: int = 0, trace: bool = False,
                  time_kernels: bool = False, left: bool = False):
        """The matrix-free solve of a sparse ``CsrMatrix`` (``st_solve_csr``):
        nnz * (b + 4) bytes per round, read where the arrays lie.  Returns
        (λ: float, v: tensor of the matrix's dtype, iterations: int, stats:
        dict), as ``solve_half``.  ``last_round_sums()`` works after
        ``trace``, ``last_round_times()`` after ``time_kernels``.

        ``left=True`` gives the LEFT Perron vector (v A = λ v; for a
        row-stochastic P the stationary distribution is ``v / v.sum()``): the
        solve of ``csr.T``, which is made on the device at the first use and
        kept - bit for bit the solve of a host-transposed copy.

        ``terms`` (a ``CsrTerms`` of ``csr``): the operator is ``A + sum_j u_j
        w_j^T`` (``st_solve_csr_terms``) - the way to solve a reducible or
        periodic matrix, or one with empty rows.  With ``left=True`` it is
        ``A^T + sum_j w_j u_j^T``: A is transposed with ``allow_empty=True``
        and the term vectors swap roles (made once per terms object, kept, and
        closed with it)."""
        if not isinstance(left, bool):
            raise TypeError(f"left must be a bool, got {type(left).__name__}")
        torch = _torch()
        if not isinstance(csr, CsrMatrix):
            raise TypeError(f"a CsrMatrix required, got {type(csr).__name__} "
                            "(solve takes dense tensors)")
        if terms is not None:
            if not isinstance(terms, CsrTerms):
                raise TypeError(f"terms must be a CsrTerms, got {type(terms).__name__}")
            if terms.csr is not csr:
                raise ValueError("terms were made for another matrix")
        if csr.device.index != (self.device.index if self.device.index is not None
                                else torch.cuda.current_device()):
            raise ValueError(f"matrix on {csr.device}, solver context on {self.device}")
        if left and terms is not None:
            if terms._left is None:
                at = csr.transpose(self, allow_empty=True)
                terms._left = (CsrTerms(at, terms.w, terms.u, solver=self), at)
            tt, at = terms._left
            return self.solve_csr(at, tt, eps=eps, max_itr=max_itr, semantics=semantics,
                                  batch=batch, trace=trace, time_kernels=time_kernels)
        if left:
            if csr._t is None:                     # csr.T, made on this solver's queue
                csr._t = csr.transpose(self)
            return self.solve_csr(csr.T, eps=eps, max_itr=max_itr, semantics=semantics,
                                  batch=batch, trace=trace, time_kernels=time_kernels)
        v = torch.empty(csr.n, dtype=csr.dtype, device=csr.device)
        ev = (ctypes.c_double if csr.dtype_code else ctypes.c_float)()
        it = ctypes.c_uint32()
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | _lib.ST_FLAG_MATRIX_FREE
                 | (_lib.ST_FLAG_TRACE_SUMS if trace else 0))
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        stats = _lib.st_stats()
        self._trace = (csr.n, csr.dtype)
        _lib.check(self.L.st_set_stream(self.q, _stream(csr.device)), "st_set_stream")
        if terms is not None:
            rc = self.L.st_solve_csr_terms(self.q, csr.handle, terms.handle, _ptr(v), None,
                                           ctypes.byref(ev), ctypes.byref(it),
                                           ctypes.byref(opt), ctypes.byref(stats))
            _lib.check(rc, "st_solve_csr_terms")
            return float(ev.value), v, int(it.value), stats.as_dict()
        rc = self.L.st_solve_csr(self.q, csr.handle, _ptr(v), None, ctypes.byref(ev),
                                 ctypes.byref(it), ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(rc, "st_solve_csr")
        return float(ev.value), v, int(it.value), stats.as_dict()

    def solve_csr_pattern(self, pat: "CsrPattern", terms: Optional["CsrTerms"] = None, *,
                          left: bool = False, eps: Optional[float] = None,
                          max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL,
                          batch: int = 0, trace: bool = False,
                          time_kernels: bool = False):
        """The matrix-free solve of a ``CsrPattern`` (``st_solve_csr_pattern``):
        nnz * 4 bytes of matrix per round.  Options and the return value are
        ``solve_csr``'s.  ``terms``: a ``CsrTerms`` made for ``pat``.
        ``left=True`` solves ``pat.T`` (scales swapped; made on the device at
        the first use and kept); with terms the pattern is transposed with
        ``allow_empty=True`` and the term vectors swap roles, kept with the
        terms object."""
        if not isinstance(left, bool):
            raise TypeError(f"left must be a bool, got {type(left).__name__}")
        torch = _torch()
        if not isinstance(pat, CsrPattern):
            raise TypeError(f"a CsrPattern required, got {type(pat).__name__} "
                            "(solve_csr takes a CsrMatrix)")
        _check_pattern_terms(pat, terms)
        if pat.device.index != (self.device.index if self.device.index is not None
                                else torch.cuda.current_device()):
            raise ValueError(f"pattern on {pat.device}, solver context on {self.device}")
        opts = dict(eps=eps, max_itr=max_itr, semantics=semantics, batch=batch,
                    trace=trace, time_kernels=time_kernels)
        if left and terms is not None:
            if terms._left is None:
                at = pat.transpose(self, allow_empty=True)
                terms._left = (CsrTerms(at, terms.w, terms.u, solver=self), at)
            tt, at = terms._left
            return self.solve_csr_pattern(at, tt, **opts)
        if left:
            if pat._t is None:
                pat._t = pat.transpose(self)
            return self.solve_csr_pattern(pat.T, **opts)
        v = torch.empty(pat.n, dtype=pat.dtype, device=pat.device)
        ev = (ctypes.c_double if pat.dtype_code else ctypes.c_float)()
        it = ctypes.c_uint32()
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | _lib.ST_FLAG_MATRIX_FREE
                 | (_lib.ST_FLAG_TRACE_SUMS if trace else 0))
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        stats = _lib.st_stats()
        self._trace = (pat.n, pat.dtype)
        _lib.check(self.L.st_set_stream(self.q, _stream(pat.device)), "st_set_stream")
        rc = self.L.st_solve_csr_pattern(
            self.q, pat.handle, None if terms is None else terms.handle, _ptr(v), None,
            ctypes.byref(ev), ctypes.byref(it), ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(rc, "st_solve_csr_pattern")
        return float(ev.value), v, int(it.value), stats.as_dict()

    def _pagerank_pattern(self, links: "CsrPattern", alpha: float, teleport, dangling,
                          solve_options):
        """``pagerank`` on a ``CsrPattern`` without scales: nothing of nnz
        elements is allocated but the two transposed index arrays."""
        torch = _torch()
        if links.row_scale is not None or links.col_scale is not None:
            raise ValueError("pagerank takes a CsrPattern without scales (the link "
                             "weights are 1; it normalises the rows itself)")
        if not links.handle.value:
            raise ValueError("the pattern is closed")
        n, dt, device = links.n, links.dtype, links.device

        def dist(x, name):
            if x is None:
                return torch.full((n,), 1.0 / n, dtype=dt, device=device)
            if not isinstance(x, torch.Tensor) or tuple(x.shape) != (n,):
                raise ValueError(f"{name} must be a tensor of shape ({n},)")
            x = x.to(device=device, dtype=dt)
            return x / x.sum()

        t = dist(teleport, "teleport")
        outdeg = (links.crow[1:] - links.crow[:-1]).to(dt)   # 0 for a dangling node
        empty = outdeg == 0
        # column c of P^T is row c of P: alpha / outdeg, 1 where no entry reads it
        scale = alpha / torch.where(empty, torch.full_like(outdeg, alpha), outdeg)
        Lt = links.transpose(self, allow_empty=True)
        Pt = CsrPattern(Lt.crow, Lt.col, n, col_scale=scale, allow_empty_rows=True,
                        solver=self)
        one = torch.ones(n, dtype=dt, device=device)
        ind = empty.to(dt)
        if dangling is None:
            u, w = [t], [(1.0 - alpha) * one + alpha * ind]
        else:
            u, w = [t, dist(dangling, "dangling")], [(1.0 - alpha) * one, alpha * ind]
        terms = None
        try:
            terms = CsrTerms(Pt, u, w, solver=self)
            lam, v, it, stats = self.solve_csr_pattern(Pt, terms, **solve_options)
        finally:
            if terms is not None:
                terms.close()
            Pt.close()
            Lt.close()
        return v / v.sum(), lam, it, stats

    def pagerank(self, A: "CsrMatrix", alpha: float = 0.85, teleport=None, dangling=None,
                 **solve_options):
        """PageRank of a link graph, on the device throughout.  ``A`` is a
        nonnegative link-weight ``CsrMatrix`` (row = source; rows without an
        entry - dangling nodes - are legal with ``allow_empty_rows=True``).
        Rows are normalised on the device (``st_csr_rowsum`` gives the
        out-weights, torch scales the values by ``alpha``), the matrix is
        transposed (``allow_empty=True``) and the Google matrix
        ``G^T = alpha P^T + t ((1 - alpha) 1 + alpha [row of P empty])^T``
        is solved as one term; a ``dangling`` distribution of its own makes it
        two, ``t ((1 - alpha) 1)^T + dangling (alpha [row empty])^T``.
        ``teleport`` / ``dangling``: nonnegative tensors [n] (normalised to
        sum 1 here), uniform when None.  ``solve_options`` are
        ``solve_csr``'s (eps, max_itr, semantics, batch, trace,
        time_kernels).

        ``A`` may also be a ``CsrPattern`` without scales (an unweighted
        graph): the out-degrees come from ``crow``, the pattern is transposed,
        ``col_scale = alpha / outdeg`` (1 where outdeg is 0: no entry reads
        it) goes on the transposed handle and the same terms are solved with
        ``solve_csr_pattern`` - no tensor of nnz values exists on that route.

        Returns ``(pi with sum 1, λ, iterations, stats)``; λ is 1 up to
        rounding."""
        torch = _torch()
        if not isinstance(A, (CsrMatrix, CsrPattern)):
            raise TypeError(f"a CsrMatrix required, got {type(A).__name__}")
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise ValueError(f"alpha must be in (0, 1), got {alpha}")
        if "left" in solve_options or "terms" in solve_options:
            raise TypeError("pagerank builds its own terms and transposition")
        if isinstance(A, CsrPattern):
            return self._pagerank_pattern(A, alpha, teleport, dangling, solve_options)
        n, dt, device = A.n, A.dtype, A.device

        def dist(x, name):
            if x is None:
                return torch.full((n,), 1.0 / n, dtype=dt, device=device)
            if not isinstance(x, torch.Tensor) or tuple(x.shape) != (n,):
                raise ValueError(f"{name} must be a tensor of shape ({n},)")
            x = x.to(device=device, dtype=dt)
            return x / x.sum()

        t = dist(teleport, "teleport")
        out_w = csr_rowsum(A)                                 # 0 for a dangling node
        empty = out_w == 0
        lens = A.crow[1:] - A.crow[:-1]
        scale = torch.where(empty, torch.ones_like(out_w), out_w)
        vals = A.values * alpha / torch.repeat_interleave(scale, lens)
        P = CsrMatrix(A.crow, A.col, vals, n, solver=self, allow_empty_rows=True)
        Pt = P.transpose(self, allow_empty=True)
        P.close()
        one = torch.ones(n, dtype=dt, device=device)
        ind = empty.to(dt)
        if dangling is None:
            u, w = [t], [(1.0 - alpha) * one + alpha * ind]
        else:
            u, w = [t, dist(dangling, "dangling")], [(1.0 - alpha) * one, alpha * ind]
        terms = CsrTerms(Pt, u, w, solver=self)
        try:
            lam, v, it, stats = self.solve_csr(Pt, terms, **solve_options)
        finally:
            terms.close()
            Pt.close()
        return v / v.sum(), lam, it, stats

    def solve_csr_product(self, B: "CsrMatrix", A: "CsrMatrix", *,
                          eps: Optional[float] = None, max_itr: int = 0,
                          semantics: int = _lib.ST_SEM_SYCL, batch: int = 0,
                          trace: bool = False, time_kernels: bool = False,
                          left: bool = False):
        """The matrix-free solve of the product operator ``B·A``
        (``st_solve_csr_product``), which is never formed: two CSR row
        products per round, both in ``solve_csr``'s summation order.  ``B``
        and ``A`` share n, dtype and device; the same matrix twice gives
        ``A²``.  ``A`` may have empty rows; every row of ``B·A`` needs a
        positive entry (``EigenValueError`` naming the lowest row without
        one).  Returns (λ, v, iterations, stats) as ``solve_csr``; with the
        identity as one factor every bit is ``solve_csr``'s on the other.

        ``left=True`` solves ``Aᵀ·Bᵀ`` - the left Perron vector of ``B·A`` -
        from the cached transposes (``.T``, made on this solver's queue at
        the first use and kept)."""
        if not isinstance(left, bool):
            raise TypeError(f"left must be a bool, got {type(left).__name__}")
        torch = _torch()
        _check_product_pair(B, A)
        if A.device.index != (self.device.index if self.device.index is not None
                              else torch.cuda.current_device()):
            raise ValueError(f"matrices on {A.device}, solver context on {self.device}")
        if left:
            if A._t is None:               # the new left factor: no empty row, so
                A._t = A.transpose(self)   # an empty column of A is refused by name
            if B._t is None:               # the new right factor may have empty rows
                B._t = B.transpose(self, allow_empty=True)
            return self.solve_csr_product(A.T, B.T, eps=eps, max_itr=max_itr,
                                          semantics=semantics, batch=batch, trace=trace,
                                          time_kernels=time_kernels)
        v = torch.empty(A.n, dtype=A.dtype, device=A.device)
        ev = (ctypes.c_double if A.dtype_code else ctypes.c_float)()
        it = ctypes.c_uint32()
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | _lib.ST_FLAG_MATRIX_FREE
                 | (_lib.ST_FLAG_TRACE_SUMS if trace else 0))
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        stats = _lib.st_stats()
        self._trace = (A.n, A.dtype)
        _lib.check(self.L.st_set_stream(self.q, _stream(A.device)), "st_set_stream")
        rc = self.L.st_solve_csr_product(self.q, B.handle, A.handle, _ptr(v), None,
                                         ctypes.byref(ev), ctypes.byref(it),
                                         ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(rc, "st_solve_csr_product")
        return float(ev.value), v, int(it.value), stats.as_dict()

    def hits(self, links: "CsrMatrix", **solve_options):
        """HITS of a link graph, on the device throughout.  ``links`` is a
        nonnegative link-weight ``CsrMatrix`` (row = source); nodes without
        out-links (empty rows, ``allow_empty_rows=True``) are fine, a node
        without in-links (an empty column) is refused by name, as
        ``transpose()`` does.  Authorities are the Perron vector of
        ``linksᵀ·links``, solved as a product (``solve_csr_product(links.T,
        links)``, the transposition made on the device); hubs are ``links``
        applied to them (``csr_apply``).  ``solve_options`` are
        ``solve_csr_product``'s (eps, max_itr, semantics, batch, trace,
        time_kernels).

        Returns ``(authorities with sum 1, hubs with sum 1, σ, iterations,
        stats)``; σ = √λ is the largest singular value of ``links``."""
        _check_csr(links, "links")
        if "left" in solve_options:
            raise TypeError("hits builds its own transposition")
        lt = links.transpose(self)
        try:
            lam, v, it, stats = self.solve_csr_product(lt, links, **solve_options)
        finally:
            lt.close()
        authorities = v / v.sum()
        h = csr_apply(links, authorities)
        hubs = h / h.sum()
        return authorities, hubs, math.sqrt(lam), it, stats

    def solve_csr_multi(self, csr: "CsrMatrix", mterms: "CsrMultiTerms", *,
                        eps: Optional[float] = None, max_itr: int = 0,
                        semantics: int = _lib.ST_SEM_SYCL, batch_rounds: int = 0):
        """The solve of C operators on one matrix (``st_solve_csr_multi``): one
        pass over the matrix per round for all columns, each stopping in its
        own round with the bits ``solve_csr(csr, CsrTerms(...))`` gives it
        alone.  ``batch_rounds``: rounds per host check (0 = 8).  Returns (λ:
        numpy [C], V: tensor [C, n], iterations: uint32 numpy [C], converged:
        uint32 numpy [C], stats: dict).  For ONE term set ``solve_csr`` is the
        call to use."""
        import numpy as np
        torch = _torch()
        if not isinstance(csr, CsrMatrix):
            raise TypeError(f"a CsrMatrix required, got {type(csr).__name__}")
        if not isinstance(mterms, CsrMultiTerms):
            raise TypeError(f"mterms must be a CsrMultiTerms, got {type(mterms).__name__}")
        if mterms.csr is not csr:
            raise ValueError("the multi terms were made for another matrix")
        if csr.device.index != (self.device.index if self.device.index is not None
                                else torch.cuda.current_device()):
            raise ValueError(f"matrix on {csr.device}, solver context on {self.device}")
        C = mterms.C
        v = torch.empty((C, csr.n), dtype=csr.dtype, device=csr.device)
        lam = np.empty(C, dtype=np.float64 if csr.dtype_code else np.float32)
        its = np.zeros(C, dtype=np.uint32)
        conv = np.zeros(C, dtype=np.uint32)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch_rounds, _lib.ST_FLAG_MATRIX_FREE)
        stats = _lib.st_stats()
        _lib.check(self.L.st_set_stream(self.q, _stream(csr.device)), "st_set_stream")
        rc = self.L.st_solve_csr_multi(self.q, csr.handle, mterms.handle, _ptr(v), None,
                                       lam.ctypes.data, its.ctypes.data, conv.ctypes.data,
                                       ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(rc, "st_solve_csr_multi")
        return lam, v, its, conv, stats.as_dict()

    def pagerank_multi(self, A: "CsrMatrix", alpha: float = 0.85, teleports=None,
                       dangling=None, **solve_options):
        """Personalised PageRank: ``pagerank`` of one link graph under many
        teleport vectors, ``teleports`` a tensor [C, n] (any C >= 1, solved in
        chunks of 8).  The graph is normalised and transposed ONCE; every chunk
        is one ``solve_csr_multi``, one pass over the matrix per round for its
        columns.  ``dangling`` (one distribution [n] for all columns, or None)
        and ``alpha`` as in ``pagerank``; ``solve_options`` are
        ``solve_csr_multi``'s (eps, max_itr, semantics, batch_rounds).

        A teleport vector must be positive wherever a node has no in-link
        (with ``dangling`` also: wherever the dangling distribution is zero
        too), or that row of the operator has no positive entry: the
        validation then names the column and the row.

        Returns ``(Π [C, n], each row summing to 1, λ numpy [C], iterations
        uint32 numpy [C], stats of the last chunk)``; row c is bit for bit
        ``pagerank(A, alpha, teleport=teleports[c], dangling=dangling)``."""
        import numpy as np
        torch = _torch()
        if not isinstance(A, CsrMatrix):
            raise TypeError(f"a CsrMatrix required, got {type(A).__name__}")
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise ValueError(f"alpha must be in (0, 1), got {alpha}")
        n, dt, device = A.n, A.dtype, A.device
        if (not isinstance(teleports, torch.Tensor) or teleports.dim() != 2
                or teleports.shape[0] < 1 or teleports.shape[1] != n):
            raise ValueError(f"teleports must be a tensor of shape (C, {n}), C >= 1")

        def dist(x, name):
            if not isinstance(x, torch.Tensor) or tuple(x.shape) != (n,):
                raise ValueError(f"{name} must be a tensor of shape ({n},)")
            x = x.to(device=device, dtype=dt)
            return x / x.sum()

        ts = [dist(teleports[c].contiguous(), f"teleports[{c}]")
              for c in range(teleports.shape[0])]
        dang = None if dangling is None else dist(dangling, "dangling")
        out_w = csr_rowsum(A)                                 # 0 for a dangling node
        empty = out_w == 0
        lens = A.crow[1:] - A.crow[:-1]
        scale = torch.where(empty, torch.ones_like(out_w), out_w)
        vals = A.values * alpha / torch.repeat_interleave(scale, lens)
        P = CsrMatrix(A.crow, A.col, vals, n, solver=self, allow_empty_rows=True)
        Pt = P.transpose(self, allow_empty=True)
        P.close()
        one = torch.ones(n, dtype=dt, device=device)
        ind = empty.to(dt)
        pis, lams, its, stats = [], [], [], {}
        try:
            for c0 in range(0, len(ts), _lib.ST_CSR_MULTI_MAX):
                chunk = ts[c0:c0 + _lib.ST_CSR_MULTI_MAX]
                if dang is None:
                    u = [[t] for t in chunk]
                    w = [[(1.0 - alpha) * one + alpha * ind]] * len(chunk)
                else:
                    u = [[t, dang] for t in chunk]
                    w = [[(1.0 - alpha) * one, alpha * ind]] * len(chunk)
                mt = CsrMultiTerms(Pt, u, w, solver=self)
                try:
                    lam, V, it, _, stats = self.solve_csr_multi(Pt, mt, **solve_options)
                finally:
                    mt.close()
                pis += [V[c] / V[c].sum() for c in range(len(chunk))]
                lams.append(lam)
                its.append(it)
        finally:
            Pt.close()
        return torch.stack(pis), np.concatenate(lams), np.concatenate(its), stats

    def solve_csr_batched(self, batch: "CsrBatch", *, eps: Optional[float] = None,
                          max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL,
                          batch_rounds: int = 0):
        """The solve of a ``CsrBatch`` (``st_solve_csr_batched``): one pair of
        launches per round for all matrices, each stopping in its own round
        with the bits ``solve_csr`` gives it alone.  ``batch_rounds``: rounds
        per host check (0 = 8).  Returns (λ: numpy [B], v: stacked tensor [N]
        - matrix b's at ``batch.mat_first[b]`` -, iterations: uint32 numpy
        [B], converged: uint32 numpy [B], stats: dict).  For ONE matrix
        ``solve_csr`` is the call to use."""
        import numpy as np
        torch = _torch()
        if not isinstance(batch, CsrBatch):
            raise TypeError(f"a CsrBatch required, got {type(batch).__name__} "
                            "(solve_csr takes a CsrMatrix)")
        if batch.device.index != (self.device.index if self.device.index is not None
                                  else torch.cuda.current_device()):
            raise ValueError(f"batch on {batch.device}, solver context on {self.device}")
        v = torch.empty(batch.n, dtype=batch.dtype, device=batch.device)
        lam = np.empty(batch.batch, dtype=np.float64 if batch.dtype_code else np.float32)
        its = np.zeros(batch.batch, dtype=np.uint32)
        conv = np.zeros(batch.batch, dtype=np.uint32)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch_rounds, _lib.ST_FLAG_MATRIX_FREE)
        stats = _lib.st_stats()
        _lib.check(self.L.st_set_stream(self.q, _stream(batch.device)), "st_set_stream")
        rc = self.L.st_solve_csr_batched(self.q, batch.handle, _ptr(v), None, lam.ctypes.data,
                                         its.ctypes.data, conv.ctypes.data, ctypes.byref(opt),
                                         ctypes.byref(stats))
        _lib.check(rc, "st_solve_csr_batched")
        return lam, v, its, conv, stats.as_dict()

    def last_round_times(self):
        """Per-round kernel times (ms) of the last solve made with
        ``time_kernels=True`` (``st_last_round_times``; empty otherwise)."""
        import numpy as np
        n = _lib.check(self.L.st_last_round_times(self.q, None, 0), "st_last_round_times",
                       self.L)
        out = np.zeros(n, dtype=np.float32)
        if n:
            _lib.check(self.L.st_last_round_times(self.q, out.ctypes.data, n),
                       "st_last_round_times", self.L)
        return out

    def solve_batched(self, mats, *, inplace: bool = False, eps: Optional[float] = None,
                      max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL,
                      round_loop=None, batch: int = 0):
        """Many small matrices in ONE launch, a workgroup per matrix
        (``st_solve_batched_*``).  ``mats``: a torch tensor or DLPack producer
        of shape (B, n, n) on this solver's device, n <= ``batched_max_dim``.

        ``round_loop=True`` runs one launch per ROUND for the whole batch
        instead (``ST_FLAG_BATCH_ROUNDS``, k_round_batched): any n up to
        ``batched_rounds_max_dim`` (4344 fp64 / 6143 fp32), every entry
        bit-identical to ``solve`` on that matrix alone at every n;
        ``batch`` rounds are enqueued per host check (0 = 8) and
        ``stats["fused_launches"]`` counts the rounds enqueued.
        ``round_loop="auto"`` does so only where n > ``batched_max_dim``;
        ``None`` is the one-launch kernel.

        Returns (λ: host tensor[B], v: device tensor[B, n], iterations: host
        tensor[B] (int64), stats: dict).  ``stats["converged_each"]`` is a
        uint32 array[B]; ``stats["rounds"]`` the largest round count of the
        batch and ``stats["converged"]`` 1 only if every matrix converged.

        For n % (16 / element size) == 0 every entry equals ``solve`` on that
        matrix alone bit for bit (λ, v, count and, with ``inplace``, the
        final matrix); other n agree to rounding.  ``inplace`` transforms
        ``mats`` itself (it must be contiguous); otherwise a copy is made."""
        import numpy as np
        torch = _torch()
        if not isinstance(mats, torch.Tensor) and hasattr(mats, "__dlpack__"):
            mats = torch.from_dlpack(mats)   # any DLPack producer, zero copy
        _check_cuda(mats)
        if mats.device.index != (self.device.index if self.device.index is not None
                                 else torch.cuda.current_device()):
            raise ValueError(f"matrices on {mats.device}, solver context on {self.device}")
        assert mats.dim() == 3 and mats.shape[1] == mats.shape[2], "must be (B, n, n)"
        sfx = _sfx(mats)
        b, n = mats.shape[0], mats.shape[1]
        flags = _lib.batch_rounds_flag(round_loop, n, 1 if sfx == "f64" else 0)
        if inplace and not mats.is_contiguous():
            raise ValueError("inplace needs a contiguous (B, n, n) tensor")
        work = (mats if inplace else mats.clone()).contiguous()
        v = torch.empty((b, n), dtype=mats.dtype, device=mats.device)
        npdt = np.float64 if mats.dtype == torch.float64 else np.float32
        lam = np.zeros(b, dtype=npdt)
        it = np.zeros(b, dtype=np.uint32)
        conv = np.zeros(b, dtype=np.uint32)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        stats = _lib.st_stats()
        _lib.check(self.L.st_set_stream(self.q, _stream(mats.device)), "st_set_stream")
        rc = getattr(self.L, f"st_solve_batched_{sfx}")(
            self.q, _ptr(work), b, n, _ptr(v), None, lam.ctypes.data, it.ctypes.data,
            conv.ctypes.data, ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(rc, "st_solve_batched")
        out = stats.as_dict()
        out["converged_each"] = conv
        return (torch.from_numpy(lam), v, torch.from_numpy(it.astype(np.int64)), out)

    def solve_vbatched(self, mats, *, inplace: bool = False, eps: Optional[float] = None,
                       max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL):
        """Many small matrices of DIFFERENT sizes in one call
        (``st_solve_vbatched_*``): one launch per workgroup-shape class
        (n <= 4, 8, 16, 32, 64, 128, 256), a workgroup per matrix.  ``mats``:
        a sequence of square 2-D torch tensors (or DLPack producers) of one
        dtype on this solver's device, each n <= ``batched_max_dim``; an empty
        sequence is allowed.

        With ``inplace`` every matrix must be contiguous and is transformed
        where it lies (its own storage pointer is passed, nothing is
        concatenated; the matrices must not overlap).  Otherwise they are
        copied into one workspace, each at a 16-byte aligned offset, and the
        inputs stay untouched.

        Returns (λ: host tensor[B], vs: list of B device views into one
        packed v tensor, iterations: host tensor[B] (int64), stats: dict).
        ``stats["converged_each"]`` is a uint32 array[B], ``stats["rounds"]``
        the largest round count, ``stats["fused_launches"]`` the number of
        class launches.  Every entry equals ``solve_batched`` on that matrix
        alone as a (1, n, n) batch bit for bit, whatever its alignment."""
        import numpy as np
        torch = _torch()
        mats = [torch.from_dlpack(m) if not isinstance(m, torch.Tensor) and hasattr(m, "__dlpack__")
                else m for m in mats]
        _check_cuda(*mats)
        here = (self.device.index if self.device.index is not None
                else torch.cuda.current_device())
        dtype = mats[0].dtype if mats else torch.float32
        for m in mats:
            if m.device.index != here:
                raise ValueError(f"matrix on {m.device}, solver context on {self.device}")
            assert m.dim() == 2 and m.shape[0] == m.shape[1], "must be square"
            if m.dtype != dtype:
                raise TypeError(f"one dtype required, got {dtype} and {m.dtype}")
            if inplace and not m.is_contiguous():
                raise ValueError("inplace needs contiguous (row-major) matrices")
        if dtype not in (torch.float32, torch.float64):
            raise TypeError(f"float32/float64 tensor required, got {dtype}")
        sfx = "f64" if dtype == torch.float64 else "f32"
        b = len(mats)
        dims = np.array([m.shape[0] for m in mats], dtype=np.uint32)
        dev_ = torch.device("cuda", here)
        if inplace:
            work = mats
        else:
            # one workspace, each matrix at a 16-byte aligned offset
            per16 = 16 // (8 if sfx == "f64" else 4)
            offs, total = [], 0
            for n in dims.tolist():
                offs.append(total)
                total += -(-n * n // per16) * per16
            space = torch.empty(total, dtype=dtype, device=dev_)
            work = [space[o:o + n * n].view(n, n) for o, n in zip(offs, dims.tolist())]
            for w, m in zip(work, mats):
                w.copy_(m)
        ptrs = (ctypes.c_void_p * max(1, b))(*[_ptr(w) for w in work])
        voff = np.concatenate([[0], np.cumsum(dims, dtype=np.int64)])
        v = torch.empty(int(voff[-1]), dtype=dtype, device=dev_)
        npdt = np.float64 if sfx == "f64" else np.float32
        lam = np.zeros(b, dtype=npdt)
        it = np.zeros(b, dtype=np.uint32)
        conv = np.zeros(b, dtype=np.uint32)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics, 0, 0)
        stats = _lib.st_stats()
        _lib.check(self.L.st_set_stream(self.q, _stream(dev_)), "st_set_stream")
        rc = getattr(self.L, f"st_solve_vbatched_{sfx}")(
            self.q, ptrs, dims.ctypes.data, b, _ptr(v) if b else None, None, lam.ctypes.data,
            it.ctypes.data, conv.ctypes.data, ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(rc, "st_solve_vbatched")
        out = stats.as_dict()
        out["converged_each"] = conv
        vs = [v[int(voff[i]):int(voff[i + 1])] for i in range(b)]
        return (torch.from_numpy(lam), vs, torch.from_numpy(it.astype(np.int64)), out)

    def last_round_sums(self):
        """Row sums s_0 .. s_{rounds-1} of the last ``solve(trace_sums=True)``
        as a (rounds, n) numpy array (empty if that solve was not traced)."""
        import numpy as np
        n, dt = getattr(self, "_trace", (0, None))
        npdt = np.float64 if dt is not None and dt == _torch().float64 else np.float32
        return _lib.round_sums(self.L, self.q, n, npdt)

    def close(self) -> None:
        if self.q is not None and self.q.value:
            self.L.destroy_queue(self.q)
            self.q = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
