"""Drop-in Python wrapper: same class, method and return tuple as the
reference's ``wrapper/python/similarity_transform.py`` (class ``EigenValue``,
lines 18-78), backed by the MI355X library instead of the SYCL one.

    import eigen_value_amd.similarity_transform as st
    ev = st.EigenValue()
    λ, v, ts, itr = ev.similarity_transform(mat)     # mat: float32 (n, n)

Differences, all additive:

* ``so_path`` resolves to the in-tree ``eigen_value_amd/lib/`` build
  (``EIGEN_VALUE_LIB`` overrides); the reference used a CWD-relative
  ``'../libsimilarity_transform.so'`` (line 19).
* float64 matrices are accepted and dispatched to ``max_eigen_value_f64``
  (the reference asserts float32, line 57); float32 behaviour is unchanged.
* ``iter_cnt`` is a ``uint32`` buffer, matching the C ``uint*`` (the
  reference passes ``np.uint`` = uint64, lines 63-64,73).
* a negative return from the library raises ``EigenValueError`` with the
  library's message (the reference had no error path).
* ``close()`` / context manager release the device context (the reference
  leaks its queue).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _lib


class EigenValue:
    so_path: str = _lib.lib_path()
    sycl_q: ctypes.c_void_p = None   # name kept for drop-in compatibility
    so_lib: ctypes.CDLL = None

    def __init__(self) -> None:
        """Load the shared library and create a device context (queue)."""
        import os
        if not os.path.exists(self.so_path):
            raise Exception(
                f'failed to find shared library `{os.path.abspath(self.so_path)}`')
        self.so_lib = _lib.load(None if self.so_path == _lib.lib_path() else self.so_path)
        self.sycl_q = ctypes.c_void_p()
        self.so_lib.make_queue(ctypes.byref(self.sycl_q))
        if self.sycl_q.value is None:
            raise Exception(f'failed to get default HIP queue: {_lib.last_error(self.so_lib)}')

    # ------------------------------------------------------------------
    def similarity_transform(self, mat: np.ndarray) -> Tuple[np.floating, np.ndarray, int, int]:
        """Largest eigenvalue λ and eigenvector v of a positive square matrix.

        Returns ``(λ, v, ts_ms, iterations)`` exactly as the reference
        (wrapper/python/similarity_transform.py:42-78): λ is ``np.float32``
        for float32 input (``np.float64`` for float64), ``ts`` the elapsed
        milliseconds reported by the library (host->device copy included,
        as in similarity_transform.cpp:36-58), ``iterations`` the number of
        similarity transforms applied before convergence.  ``A v ≈ λ v``.
        """
        m, n = mat.shape
        assert m == n, "must be square matrix of floating points !"
        assert mat.dtype.num in (11, 12), "dtype of input matrix must be float32 (or float64) !"
        mat = np.ascontiguousarray(mat)
        eigen_val = np.empty(1, dtype=mat.dtype)
        eigen_vec = np.empty(n, dtype=mat.dtype)
        iter_cnt = np.zeros(1, dtype=np.uint32)
        fn = self.so_lib.max_eigen_value if mat.dtype == np.float32 else self.so_lib.max_eigen_value_f64
        ts = fn(self.sycl_q, mat.ctypes.data, eigen_val.ctypes.data,
                eigen_vec.ctypes.data, n, iter_cnt.ctypes.data)
        _lib.check(ts, "max_eigen_value", self.so_lib)
        return eigen_val[0], eigen_vec, int(ts), int(iter_cnt[0])

    # ------------------------------------------------------------------
    def similarity_transform_ex(self, mat: np.ndarray, *, eps: Optional[float] = None,
                                max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL,
                                batch: int = 0, time_kernels: bool = False,
                                matrix_free: bool = False, round_loop: bool = False,
                                write_every_round: bool = False, trace_sums: bool = False):
        """Extended call: options + statistics (``max_eigen_value_ex``).
        ``round_loop`` keeps one launch per round where the whole solve would
        fit one workgroup (``ST_FLAG_ROUND_LOOP``; identical results);
        ``write_every_round`` stores the matrix every round where the flat
        round would store it every 6th (``ST_FLAG_WRITE_EVERY_ROUND``;
        identical results); ``trace_sums`` records every evaluated round's
        row sums (``ST_FLAG_TRACE_SUMS``; identical results), read back with
        ``last_round_sums()``.

        Returns ``(λ, v, ts_ms, iterations, stats_dict)``."""
        m, n = mat.shape
        assert m == n, "must be square matrix of floating points !"
        mat = np.ascontiguousarray(mat)
        if mat.dtype not in (np.float32, np.float64):
            raise TypeError("float32 or float64 matrix required")
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | (_lib.ST_FLAG_MATRIX_FREE if matrix_free else 0)
                 | (_lib.ST_FLAG_ROUND_LOOP if round_loop else 0)
                 | (_lib.ST_FLAG_WRITE_EVERY_ROUND if write_every_round else 0)
                 | (_lib.ST_FLAG_TRACE_SUMS if trace_sums else 0))
        self._trace = (n, mat.dtype)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        stats = _lib.st_stats()
        eigen_val = np.empty(1, dtype=mat.dtype)
        eigen_vec = np.empty(n, dtype=mat.dtype)
        iter_cnt = np.zeros(1, dtype=np.uint32)
        dtype = _lib.DTYPE_F32 if mat.dtype == np.float32 else _lib.DTYPE_F64
        ts = self.so_lib.max_eigen_value_ex(
            self.sycl_q, dtype, mat.ctypes.data, eigen_val.ctypes.data,
            eigen_vec.ctypes.data, n, iter_cnt.ctypes.data,
            ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(ts, "max_eigen_value_ex", self.so_lib)
        return eigen_val[0], eigen_vec, int(ts), int(iter_cnt[0]), stats.as_dict()

    # ------------------------------------------------------------------
    def similarity_transform_left(self, mat: np.ndarray, *, eps: Optional[float] = None,
                                  max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL,
                                  batch: int = 0, time_kernels: bool = False,
                                  trace_sums: bool = False):
        """The LEFT Perron vector of a dense matrix, ``u A = λ u``
        (``max_eigen_value_left_ex``): the matrix-free solve swept by columns
        on the matrix as it is stored - no transposed copy on the host or on
        the device.  For a row-stochastic matrix the stationary distribution
        is ``u / u.sum()``.  ``trace_sums`` records every evaluated round's
        COLUMN sums (``last_round_sums()``).

        Returns ``(λ, u, ts_ms, iterations, stats_dict)`` in the dtype of
        ``mat`` (float32 or float64)."""
        m, n = mat.shape
        assert m == n, "must be square matrix of floating points !"
        mat = np.ascontiguousarray(mat)
        if mat.dtype not in (np.float32, np.float64):
            raise TypeError("float32 or float64 matrix required")
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | _lib.ST_FLAG_MATRIX_FREE
                 | (_lib.ST_FLAG_TRACE_SUMS if trace_sums else 0))
        self._trace = (n, mat.dtype)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        stats = _lib.st_stats()
        eigen_val = np.empty(1, dtype=mat.dtype)
        eigen_vec = np.empty(n, dtype=mat.dtype)
        iter_cnt = np.zeros(1, dtype=np.uint32)
        dtype = _lib.DTYPE_F32 if mat.dtype == np.float32 else _lib.DTYPE_F64
        ts = self.so_lib.max_eigen_value_left_ex(
            self.sycl_q, dtype, mat.ctypes.data, eigen_val.ctypes.data,
            eigen_vec.ctypes.data, n, iter_cnt.ctypes.data,
            ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(ts, "max_eigen_value_left_ex", self.so_lib)
        return eigen_val[0], eigen_vec, int(ts), int(iter_cnt[0]), stats.as_dict()

    # ------------------------------------------------------------------
    def similarity_transform_pair(self, mat: np.ndarray, *, eps: Optional[float] = None,
                                  max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL,
                                  batch: int = 0):
        """Both Perron vectors of a dense matrix, ``A v = λ v`` and
        ``u A = λ u`` (``max_eigen_value_pair_ex``): two independent
        iterations that share one pass over the matrix per round, on the matrix
        as it is stored - one copy in, no transposed copy.  Index 0 is the
        right side, index 1 the left one; each side stops in its own round.

        Returns ``(λ [2], vecs [2, n], ts_ms, iterations [2])`` in the dtype
        of ``mat`` (float32 or float64); ``last_pair_stats`` holds the call's
        stats and ``converged`` by side."""
        m, n = mat.shape
        assert m == n, "must be square matrix of floating points !"
        mat = np.ascontiguousarray(mat)
        if mat.dtype not in (np.float32, np.float64):
            raise TypeError("float32 or float64 matrix required")
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, _lib.ST_FLAG_MATRIX_FREE)
        stats = _lib.st_stats()
        eigen_vals = np.empty(2, dtype=mat.dtype)
        eigen_vecs = np.empty((2, n), dtype=mat.dtype)
        iter_cnts = np.zeros(2, dtype=np.uint32)
        converged = np.zeros(2, dtype=np.uint32)
        dtype = _lib.DTYPE_F32 if mat.dtype == np.float32 else _lib.DTYPE_F64
        ts = self.so_lib.max_eigen_value_pair_ex(
            self.sycl_q, dtype, mat.ctypes.data, eigen_vals.ctypes.data,
            eigen_vecs.ctypes.data, n, iter_cnts.ctypes.data, converged.ctypes.data,
            ctypes.byref(opt), ctypes.byref(stats))
        _lib.check(ts, "max_eigen_value_pair_ex", self.so_lib)
        self.last_pair_stats = dict(stats.as_dict(), converged_sides=converged.tolist())
        return eigen_vals, eigen_vecs, int(ts), iter_cnts.astype(np.int64)

    # ------------------------------------------------------------------
    def similarity_transform_batched(self, mats: np.ndarray, *, eps: Optional[float] = None,
                                     max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL,
                                     round_loop=None):
        """Many small matrices in one launch (``max_eigen_value_batched_ex``):
        ``mats`` is a float32 or float64 array of shape ``(B, n, n)``, n up to
        ``st_solve_batched_max_dim`` (256 / 128).  Every matrix is solved
        exactly as ``similarity_transform`` would solve it alone, by its own
        workgroup.

        ``round_loop=True`` takes one launch per round for the whole batch
        instead (``ST_FLAG_BATCH_ROUNDS``): n up to
        ``st_solve_batched_rounds_max_dim`` (6143 / 4344), results
        bit-identical to per-matrix ``similarity_transform`` calls at every n.
        ``round_loop="auto"`` does so only where n is beyond the one-launch
        kernel; ``None`` is the one-launch kernel.

        Returns ``(λ[B], v[B, n], ts_ms, iterations[B])``: numpy arrays of the
        input dtype (``uint32`` for the counts)."""
        assert mats.ndim == 3, "must be a (B, n, n) batch of square matrices !"
        b, m, n = mats.shape
        assert m == n, "must be square matrices of floating points !"
        assert mats.dtype.num in (11, 12), "dtype of input matrices must be float32 or float64 !"
        dtype = _lib.DTYPE_F32 if mats.dtype == np.float32 else _lib.DTYPE_F64
        flags = _lib.batch_rounds_flag(round_loop, n, dtype)
        mats = np.ascontiguousarray(mats)
        eigen_vals = np.empty(b, dtype=mats.dtype)
        eigen_vecs = np.empty((b, n), dtype=mats.dtype)
        iter_cnts = np.zeros(b, dtype=np.uint32)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics, 0, flags)
        ts = self.so_lib.max_eigen_value_batched_ex(
            self.sycl_q, dtype, mats.ctypes.data, eigen_vals.ctypes.data,
            eigen_vecs.ctypes.data, b, n, iter_cnts.ctypes.data, ctypes.byref(opt), None)
        _lib.check(ts, "max_eigen_value_batched_ex", self.so_lib)
        return eigen_vals, eigen_vecs, int(ts), iter_cnts

    def similarity_transform_vbatched(self, mats, *, eps: Optional[float] = None,
                                      max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL):
        """Many small matrices of DIFFERENT sizes in one call
        (``max_eigen_value_vbatched_ex``): ``mats`` is a sequence of square
        float32 or float64 arrays of one dtype, each n up to
        ``st_solve_batched_max_dim`` (256 / 128); an empty sequence is allowed.
        They are packed into one buffer, copied once, and solved with one
        launch per workgroup-shape class.  Every matrix is solved exactly as
        ``similarity_transform_batched`` would solve it as a batch of one.

        Returns ``(λ[B], [v_0 .. v_{B-1}], ts_ms, iterations[B])``: λ of the
        input dtype (float32 for an empty sequence), a list of B eigenvector
        arrays, ``uint32`` counts."""
        mats = list(mats)
        for m in mats:
            assert isinstance(m, np.ndarray) and m.ndim == 2 and m.shape[0] == m.shape[1], \
                "must be square matrices of floating points !"
        dt = mats[0].dtype if mats else np.dtype(np.float32)
        for m in mats:
            assert m.dtype == dt, "all matrices must have one dtype !"
        assert dt.num in (11, 12), "dtype of input matrices must be float32 or float64 !"
        b = len(mats)
        dims = np.array([m.shape[0] for m in mats], dtype=np.uint32)
        packed = (np.concatenate([np.ravel(m) for m in mats]) if b else np.zeros(0, dt))
        packed = np.ascontiguousarray(packed, dtype=dt)
        offs = np.concatenate([[0], np.cumsum(dims, dtype=np.int64)])
        eigen_vals = np.empty(b, dtype=dt)
        eigen_vecs = np.empty(int(offs[-1]), dtype=dt)
        iter_cnts = np.zeros(b, dtype=np.uint32)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics, 0, 0)
        dtype = _lib.DTYPE_F32 if dt == np.float32 else _lib.DTYPE_F64
        ts = self.so_lib.max_eigen_value_vbatched_ex(
            self.sycl_q, dtype, packed.ctypes.data, dims.ctypes.data, b, eigen_vals.ctypes.data,
            eigen_vecs.ctypes.data, iter_cnts.ctypes.data, ctypes.byref(opt), None)
        _lib.check(ts, "max_eigen_value_vbatched_ex", self.so_lib)
        vs = [eigen_vecs[int(offs[i]):int(offs[i + 1])] for i in range(b)]
        return eigen_vals, vs, int(ts), iter_cnts

    def similarity_transform_half(self, mat: np.ndarray, storage: Optional[str] = None, *,
                                  eps: Optional[float] = None, max_itr: int = 0,
                                  semantics: int = _lib.ST_SEM_SYCL, batch: int = 0,
                                  time_kernels: bool = False, trace_sums: bool = False):
        """The matrix-free solve of a matrix stored in 16 bits per element
        (``max_eigen_value_half_ex``): the device reads N^2 * 2 bytes per round
        and widens them in registers; vectors, stop test and arithmetic are
        float32.  ``mat`` is a ``np.float16`` array (``storage`` None or
        ``"f16"``) or, with ``storage="bf16"``, a ``np.uint16`` array of
        bfloat16 bit patterns (numpy has no bfloat16).

        Returns ``(λ, v, ts_ms, iterations)``, λ and v float32."""
        m, n = mat.shape
        assert m == n, "must be square matrix of floating points !"
        assert storage in (None, "f16", "bf16"), 'storage must be None, "f16" or "bf16" !'
        if storage == "bf16":
            assert mat.dtype == np.uint16, \
                "dtype of a bf16 input matrix must be uint16 (bfloat16 bit patterns) !"
            code = _lib.ST_STORE_BF16
        else:
            assert mat.dtype == np.float16, "dtype of input matrix must be float16 !"
            code = _lib.ST_STORE_F16
        mat = np.ascontiguousarray(mat)
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | _lib.ST_FLAG_MATRIX_FREE
                 | (_lib.ST_FLAG_TRACE_SUMS if trace_sums else 0))
        self._trace = (n, np.float32)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        eigen_val = np.empty(1, dtype=np.float32)
        eigen_vec = np.empty(n, dtype=np.float32)
        iter_cnt = np.zeros(1, dtype=np.uint32)
        ts = self.so_lib.max_eigen_value_half_ex(
            self.sycl_q, code, mat.ctypes.data, eigen_val.ctypes.data,
            eigen_vec.ctypes.data, n, iter_cnt.ctypes.data, ctypes.byref(opt), None)
        _lib.check(ts, "max_eigen_value_half_ex", self.so_lib)
        return eigen_val[0], eigen_vec, int(ts), int(iter_cnt[0])

    def similarity_transform_csr(self, indptr, indices=None, data=None, n: Optional[int] = None,
                                 *, eps: Optional[float] = None, max_itr: int = 0,
                                 semantics: int = _lib.ST_SEM_SYCL, batch: int = 0,
                                 time_kernels: bool = False, trace_sums: bool = False,
                                 left: bool = False, terms=None,
                                 allow_empty_rows: bool = False):
        """The matrix-free solve of a nonnegative SPARSE matrix in CSR storage
        (``max_eigen_value_csr_ex``): ``indptr`` [n + 1], ``indices`` [nnz] and
        ``data`` [nnz] (float32 or float64) as in ``scipy.sparse.csr_matrix``;
        index arrays of any integer dtype are converted to int64 / int32.  A
        ``scipy.sparse`` matrix or a ``torch.sparse_csr`` tensor passed as the
        first argument is accepted too (converted to CSR on the host).  The
        matrix is validated on the host - no empty row, every column inside
        [0, n) - before anything is copied; the device reads nnz * (b + 4)
        bytes per round.

        ``left=True`` gives the LEFT Perron vector, v A = λ v
        (``max_eigen_value_csr_left_ex``): the matrix is transposed on the
        device by a stable sort and the same solve runs on the result, bit for
        bit the solve of a host-transposed copy.  A column without any entry
        is refused by name.  For a row-stochastic matrix the stationary
        distribution is ``v / v.sum()``.

        ``terms=(u, w)`` solves ``A + sum_j u_j w_j^T``
        (``max_eigen_value_csr_terms_ex``): ``u`` and ``w`` are [K, n] arrays
        or sequences of K vectors, 1 <= K <= 4, nonnegative and finite - how a
        reducible or periodic matrix is made primitive.  ``allow_empty_rows``
        (with terms only) accepts rows without an entry.  Everything is
        validated on the host, the error naming the term, the vector and the
        index, or the row of the operator without a positive entry.  With
        ``left=True`` the arrays are transposed on the host first and the term
        vectors swap roles.

        Returns ``(λ, v, ts_ms, iterations)`` in the dtype of ``data``."""
        if not isinstance(left, bool):
            raise TypeError(f"left must be a bool, got {type(left).__name__}")
        if not isinstance(allow_empty_rows, bool):
            raise TypeError("allow_empty_rows must be a bool, got "
                            f"{type(allow_empty_rows).__name__}")
        if terms is None and allow_empty_rows:
            raise ValueError("allow_empty_rows needs terms: a row sum of the matrix alone "
                             "would be divided by zero")
        if terms is not None and (not isinstance(terms, (tuple, list)) or len(terms) != 2):
            raise TypeError("terms must be a pair (u, w)")
        if indices is None:
            sp = indptr
            if hasattr(sp, "crow_indices"):          # a torch.sparse_csr tensor
                assert sp.dim() == 2 and sp.shape[0] == sp.shape[1], \
                    "must be square matrix of floating points !"
                n = sp.shape[0]
                indptr, indices, data = (sp.crow_indices().cpu().numpy(),
                                         sp.col_indices().cpu().numpy(),
                                         sp.values().cpu().numpy())
            elif hasattr(sp, "tocsr"):               # any scipy.sparse matrix / array
                sp = sp.tocsr()
                assert sp.shape[0] == sp.shape[1], "must be square matrix of floating points !"
                n = sp.shape[0]
                indptr, indices, data = sp.indptr, sp.indices, sp.data
            else:
                raise TypeError("indptr, indices, data arrays or a sparse matrix required, got "
                                f"{type(sp).__name__}")
        data = np.ascontiguousarray(data)
        assert data.dtype.num in (11, 12), "dtype of data must be float32 or float64 !"
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.asarray(indices)
        assert indices.dtype.kind in "iu", "indices must be an integer array !"
        if indices.size and (indices.min() < -2**31 or indices.max() >= 2**31):
            raise _lib.EigenValueError("csr: a column index does not fit int32")
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        n = len(indptr) - 1 if n is None else int(n)
        assert len(indptr) == n + 1, "indptr must have n + 1 elements !"
        assert len(indices) == len(data), "indices and data must have one length !"
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | _lib.ST_FLAG_MATRIX_FREE
                 | (_lib.ST_FLAG_TRACE_SUMS if trace_sums else 0))
        self._trace = (n, data.dtype)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        eigen_val = np.empty(1, dtype=data.dtype)
        eigen_vec = np.empty(n, dtype=data.dtype)
        iter_cnt = np.zeros(1, dtype=np.uint32)
        dtype = _lib.DTYPE_F32 if data.dtype == np.float32 else _lib.DTYPE_F64
        if terms is not None:
            u, w = terms
            K = _lib.check_terms_arg(u, w, n)
            u = [np.ascontiguousarray(x, dtype=data.dtype) for x in u]
            w = [np.ascontiguousarray(x, dtype=data.dtype) for x in w]
            if left:
                indptr, indices, data = _lib.csr_transpose_host(
                    indptr, indices, data, self.so_lib, allow_empty=True)
                u, w = w, u
            pu = (ctypes.c_void_p * K)(*[x.ctypes.data for x in u])
            pw = (ctypes.c_void_p * K)(*[x.ctypes.data for x in w])
            ts = self.so_lib.max_eigen_value_csr_terms_ex(
                self.sycl_q, dtype, n, len(data), indptr.ctypes.data, indices.ctypes.data,
                data.ctypes.data, K, pu, pw,
                _lib.ST_CSR_EMPTY_ROWS_OK if (allow_empty_rows or left) else 0,
                eigen_val.ctypes.data, eigen_vec.ctypes.data, iter_cnt.ctypes.data,
                ctypes.byref(opt), None)
            _lib.check(ts, "max_eigen_value_csr_terms_ex", self.so_lib)
            return eigen_val[0], eigen_vec, int(ts), int(iter_cnt[0])
        name = "max_eigen_value_csr_left_ex" if left else "max_eigen_value_csr_ex"
        ts = getattr(self.so_lib, name)(
            self.sycl_q, dtype, n, len(data), indptr.ctypes.data, indices.ctypes.data,
            data.ctypes.data, eigen_val.ctypes.data, eigen_vec.ctypes.data,
            iter_cnt.ctypes.data, ctypes.byref(opt), None)
        _lib.check(ts, name, self.so_lib)
        return eigen_val[0], eigen_vec, int(ts), int(iter_cnt[0])

    def similarity_transform_csr_pattern(self, indptr, indices=None, n: Optional[int] = None,
                                         row_scale=None, col_scale=None, terms=None,
                                         left: bool = False, *, dtype=None,
                                         allow_empty_rows: bool = False,
                                         eps: Optional[float] = None, max_itr: int = 0,
                                         semantics: int = _lib.ST_SEM_SYCL, batch: int = 0,
                                         time_kernels: bool = False,
                                         trace_sums: bool = False):
        """The matrix-free solve of the PATTERN-ONLY operator ``diag(row_scale)
        · P · diag(col_scale)`` of an unweighted graph
        (``max_eigen_value_csr_pattern_ex``): ``indptr`` [n + 1] and ``indices``
        [nnz] as in ``scipy.sparse.csr_matrix``, ``P[i][j]`` the number of
        entries of row i with column j; no value array is read or copied, and
        the device reads nnz * 4 bytes of matrix per round.  A ``scipy.sparse``
        matrix or a ``torch.sparse_csr`` tensor passed as the first argument
        is accepted too: ITS VALUES ARE IGNORED, only its structure is used
        (a float32 / float64 matrix sets the default ``dtype``).

        ``row_scale`` / ``col_scale``: None (all ones) or arrays [n], finite
        and strictly positive - 1 / outdeg as ``row_scale`` gives the
        row-stochastic matrix, d^-1/2 twice the symmetric normalised one.
        ``dtype`` (np.float32 / np.float64) is the vectors'; default: the
        scales', the terms', the sparse matrix's, else float32.
        ``terms=(u, w)`` adds ``sum_j u_j w_j^T`` as in
        ``similarity_transform_csr``; ``allow_empty_rows`` (with terms only)
        accepts rows without an entry.  ``left=True`` solves the transposed
        operator: the pattern is transposed on the host, the scales swap, and
        so do the term vectors.  Everything is validated on the host, the
        error naming the row, the entry, the scale (``row_scale`` before
        ``col_scale``) or the term.

        Returns ``(λ, v, ts_ms, iterations)`` in ``dtype``."""
        if not isinstance(left, bool):
            raise TypeError(f"left must be a bool, got {type(left).__name__}")
        if not isinstance(allow_empty_rows, bool):
            raise TypeError("allow_empty_rows must be a bool, got "
                            f"{type(allow_empty_rows).__name__}")
        if terms is None and allow_empty_rows:
            raise ValueError("allow_empty_rows needs terms: a row sum of the matrix alone "
                             "would be divided by zero")
        if terms is not None and (not isinstance(terms, (tuple, list)) or len(terms) != 2):
            raise TypeError("terms must be a pair (u, w)")
        sp_dtype = None
        if indices is None:
            sp = indptr
            if hasattr(sp, "crow_indices"):          # a torch.sparse_csr tensor
                assert sp.dim() == 2 and sp.shape[0] == sp.shape[1], "must be square !"
                n = sp.shape[0]
                sp_dtype = {"torch.float32": np.float32,
                            "torch.float64": np.float64}.get(str(sp.dtype))
                indptr, indices = (sp.crow_indices().cpu().numpy(),
                                   sp.col_indices().cpu().numpy())
            elif hasattr(sp, "tocsr"):               # any scipy.sparse matrix / array
                sp = sp.tocsr()
                assert sp.shape[0] == sp.shape[1], "must be square !"
                n = sp.shape[0]
                if sp.dtype in (np.float32, np.float64):
                    sp_dtype = sp.dtype.type
                indptr, indices = sp.indptr, sp.indices
            else:
                raise TypeError("indptr, indices arrays or a sparse matrix required, got "
                                f"{type(sp).__name__}")
        if dtype is None:
            for x in (row_scale, col_scale) + (tuple(terms[0]) if terms is not None else ()):
                if x is not None and getattr(x, "dtype", None) in (np.float32, np.float64):
                    dtype = x.dtype
                    break
            else:
                dtype = sp_dtype or np.float32
        dt = np.dtype(dtype)
        assert dt.num in (11, 12), "dtype must be float32 or float64 !"
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.asarray(indices)
        assert indices.dtype.kind in "iu", "indices must be an integer array !"
        if indices.size and (indices.min() < -2**31 or indices.max() >= 2**31):
            raise _lib.EigenValueError("csr: a column index does not fit int32")
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        n = len(indptr) - 1 if n is None else int(n)
        assert len(indptr) == n + 1, "indptr must have n + 1 elements !"

        def scale(x, name):
            if x is None:
                return None
            x = np.ascontiguousarray(x, dtype=dt)
            if x.shape != (n,):
                raise ValueError(f"{name} has shape {x.shape}, ({n},) required")
            return x

        row_scale, col_scale = scale(row_scale, "row_scale"), scale(col_scale, "col_scale")
        K, u, w = 0, [], []
        if terms is not None:
            u, w = terms
            K = _lib.check_terms_arg(u, w, n)
            u = [np.ascontiguousarray(x, dtype=dt) for x in u]
            w = [np.ascontiguousarray(x, dtype=dt) for x in w]
        if left:
            indptr, indices, _ = _lib.csr_transpose_host(
                indptr, indices, np.ones(len(indices), dtype=np.float32), self.so_lib,
                allow_empty=terms is not None)
            row_scale, col_scale = col_scale, row_scale
            u, w = w, u
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | _lib.ST_FLAG_MATRIX_FREE
                 | (_lib.ST_FLAG_TRACE_SUMS if trace_sums else 0))
        self._trace = (n, dt)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch, flags)
        eigen_val = np.empty(1, dtype=dt)
        eigen_vec = np.empty(n, dtype=dt)
        iter_cnt = np.zeros(1, dtype=np.uint32)
        pu = (ctypes.c_void_p * K)(*[x.ctypes.data for x in u]) if K else None
        pw = (ctypes.c_void_p * K)(*[x.ctypes.data for x in w]) if K else None
        ts = self.so_lib.max_eigen_value_csr_pattern_ex(
            self.sycl_q, _lib.DTYPE_F32 if dt == np.float32 else _lib.DTYPE_F64, n,
            len(indices), indptr.ctypes.data, indices.ctypes.data,
            None if row_scale is None else row_scale.ctypes.data,
            None if col_scale is None else col_scale.ctypes.data, K, pu, pw,
            _lib.ST_CSR_EMPTY_ROWS_OK if (allow_empty_rows or (left and K)) else 0,
            eigen_val.ctypes.data, eigen_vec.ctypes.data, iter_cnt.ctypes.data,
            ctypes.byref(opt), None)
        _lib.check(ts, "max_eigen_value_csr_pattern_ex", self.so_lib)
        return eigen_val[0], eigen_vec, int(ts), int(iter_cnt[0])

    def similarity_transform_csr_multi(self, indptr, indices=None, data=None, *, terms=None,
                                       eps: Optional[float] = None, max_itr: int = 0,
                                       semantics: int = _lib.ST_SEM_SYCL, batch_rounds: int = 0,
                                       allow_empty_rows: bool = False):
        """C operators on ONE sparse matrix, ``M_c = A + sum_j u_cj w_cj^T``
        (``max_eigen_value_csr_multi_ex``): the matrix as
        ``similarity_transform_csr`` takes it (arrays, a ``scipy.sparse``
        matrix or a ``torch.sparse_csr`` tensor), ``terms=(U, W)`` with U, W
        [C, K, n] arrays ([C, n] means K = 1), 1 <= C <= 8, 1 <= K <= 4.  One
        pass over the matrix per round serves every column; each column gets
        the bits ``similarity_transform_csr(..., terms=(U[c], W[c]))`` gives
        it.  Everything is validated on the host, the error naming the column
        first.  Returns ``(λ [C], V [C, n], ts_ms, iterations uint32 [C],
        converged uint32 [C])`` in the dtype of ``data``."""
        if not isinstance(allow_empty_rows, bool):
            raise TypeError("allow_empty_rows must be a bool, got "
                            f"{type(allow_empty_rows).__name__}")
        if not isinstance(terms, (tuple, list)) or len(terms) != 2:
            raise TypeError("terms must be a pair (U, W)")
        if indices is None:
            indptr, indices, data, _ = self._csr_triple(indptr)
        data = np.ascontiguousarray(data)
        assert data.dtype.num in (11, 12), "dtype of data must be float32 or float64 !"
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices = np.asarray(indices)
        assert indices.dtype.kind in "iu", "indices must be an integer array !"
        if indices.size and (indices.min() < -2**31 or indices.max() >= 2**31):
            raise _lib.EigenValueError("csr: a column index does not fit int32")
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        n = len(indptr) - 1
        assert len(indices) == len(data), "indices and data must have one length !"
        C, K, uu, ww = _lib.check_multi_terms_arg(terms[0], terms[1], n)
        fu = [np.ascontiguousarray(x, dtype=data.dtype) for vs in uu for x in vs]
        fw = [np.ascontiguousarray(x, dtype=data.dtype) for vs in ww for x in vs]
        pu = (ctypes.c_void_p * len(fu))(*[x.ctypes.data for x in fu])
        pw = (ctypes.c_void_p * len(fw))(*[x.ctypes.data for x in fw])
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch_rounds, _lib.ST_FLAG_MATRIX_FREE)
        eigen_vals = np.empty(C, dtype=data.dtype)
        eigen_vecs = np.empty((C, n), dtype=data.dtype)
        iter_cnts = np.zeros(C, dtype=np.uint32)
        converged = np.zeros(C, dtype=np.uint32)
        dtype = _lib.DTYPE_F32 if data.dtype == np.float32 else _lib.DTYPE_F64
        ts = self.so_lib.max_eigen_value_csr_multi_ex(
            self.sycl_q, dtype, n, len(data), indptr.ctypes.data, indices.ctypes.data,
            data.ctypes.data, C, K, pu, pw,
            _lib.ST_CSR_EMPTY_ROWS_OK if allow_empty_rows else 0,
            eigen_vals.ctypes.data, eigen_vecs.ctypes.data, iter_cnts.ctypes.data,
            converged.ctypes.data, ctypes.byref(opt), None)
        _lib.check(ts, "max_eigen_value_csr_multi_ex", self.so_lib)
        return eigen_vals, eigen_vecs, int(ts), iter_cnts, converged

    def _csr_host(self, m, name: str):
        """One host matrix of a product front as checked contiguous arrays:
        (indptr int64, indices int32, data float32 / float64, n)."""
        indptr, indices, data, n = self._csr_triple(m)
        data = np.ascontiguousarray(data)
        if data.dtype not in (np.float32, np.float64):
            raise TypeError(f"{name}: data must be float32 or float64, got {data.dtype}")
        indices = np.asarray(indices)
        if indices.dtype.kind not in "iu":
            raise TypeError(f"{name}: indices must be an integer array, got {indices.dtype}")
        if indices.size and (indices.min() < -2**31 or indices.max() >= 2**31):
            raise _lib.EigenValueError(f"{name}: a column index does not fit int32")
        if len(indices) != len(data):
            raise ValueError(f"{name}: indices and data differ in length")
        return (np.ascontiguousarray(indptr, dtype=np.int64),
                np.ascontiguousarray(indices, dtype=np.int32), data, n)

    def _product_options(self, n, dtype, eps, max_itr, semantics, batch, time_kernels,
                         trace_sums):
        flags = ((_lib.ST_FLAG_TIME_KERNELS if time_kernels else 0)
                 | _lib.ST_FLAG_MATRIX_FREE
                 | (_lib.ST_FLAG_TRACE_SUMS if trace_sums else 0))
        self._trace = (n, dtype)
        return _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                               batch, flags)

    def similarity_transform_csr_product(self, B, A, *, eps: Optional[float] = None,
                                         max_itr: int = 0,
                                         semantics: int = _lib.ST_SEM_SYCL, batch: int = 0,
                                         time_kernels: bool = False, trace_sums: bool = False,
                                         allow_empty_rows: bool = False):
        """The matrix-free solve of the PRODUCT ``B·A`` of two nonnegative
        sparse matrices (``max_eigen_value_csr_product_ex``); the product is
        never formed - two CSR row products per round.  ``B`` and ``A`` are
        each an ``(indptr, indices, data)`` triple of numpy arrays, a
        ``scipy.sparse`` matrix or a ``torch.sparse_csr`` tensor, square of
        one size and one dtype (float32 or float64).  ``allow_empty_rows``
        accepts rows of ``A`` without an entry.  Everything is validated on
        the host - the two matrices, then every row of ``B·A`` for a positive
        entry, the error naming the lowest row without one.

        Returns ``(λ, v, ts_ms, iterations)`` in the dtype of the data."""
        if not isinstance(allow_empty_rows, bool):
            raise TypeError("allow_empty_rows must be a bool, got "
                            f"{type(allow_empty_rows).__name__}")
        bp, bi, bd, bn = self._csr_host(B, "B")
        ap, ai, ad, an = self._csr_host(A, "A")
        if bn != an:
            raise ValueError(f"product: the factors differ in n (B: {bn}, A: {an})")
        if bd.dtype != ad.dtype:
            raise TypeError(f"product: the factors differ in dtype (B: {bd.dtype}, "
                            f"A: {ad.dtype})")
        n = an
        opt = self._product_options(n, ad.dtype, eps, max_itr, semantics, batch, time_kernels,
                                    trace_sums)
        eigen_val = np.empty(1, dtype=ad.dtype)
        eigen_vec = np.empty(n, dtype=ad.dtype)
        iter_cnt = np.zeros(1, dtype=np.uint32)
        dtype = _lib.DTYPE_F32 if ad.dtype == np.float32 else _lib.DTYPE_F64
        ts = self.so_lib.max_eigen_value_csr_product_ex(
            self.sycl_q, dtype, n, len(bd), bp.ctypes.data, bi.ctypes.data, bd.ctypes.data,
            len(ad), ap.ctypes.data, ai.ctypes.data, ad.ctypes.data,
            _lib.ST_CSR_EMPTY_ROWS_OK if allow_empty_rows else 0,
            eigen_val.ctypes.data, eigen_vec.ctypes.data, iter_cnt.ctypes.data,
            ctypes.byref(opt), None)
        _lib.check(ts, "max_eigen_value_csr_product_ex", self.so_lib)
        return eigen_val[0], eigen_vec, int(ts), int(iter_cnt[0])

    def similarity_transform_csr_gram(self, A, side: str = "ata", *,
                                      eps: Optional[float] = None, max_itr: int = 0,
                                      semantics: int = _lib.ST_SEM_SYCL, batch: int = 0,
                                      time_kernels: bool = False, trace_sums: bool = False,
                                      allow_empty_rows: bool = False):
        """The Gram operators of ONE sparse matrix
        (``max_eigen_value_csr_gram_ex``): ``side="ata"`` solves ``AᵀA`` (λ is
        the square of the spectral norm of ``A``, v the HITS authorities),
        ``side="aat"`` solves ``AAᵀ`` (the hubs).  ``A`` as
        ``similarity_transform_csr_product`` takes a factor; it is transposed
        on the device.  Returns ``(λ, v, ts_ms, iterations)``."""
        if not isinstance(allow_empty_rows, bool):
            raise TypeError("allow_empty_rows must be a bool, got "
                            f"{type(allow_empty_rows).__name__}")
        code = _lib.gram_side(side)
        ap, ai, ad, n = self._csr_host(A, "A")
        opt = self._product_options(n, ad.dtype, eps, max_itr, semantics, batch, time_kernels,
                                    trace_sums)
        eigen_val = np.empty(1, dtype=ad.dtype)
        eigen_vec = np.empty(n, dtype=ad.dtype)
        iter_cnt = np.zeros(1, dtype=np.uint32)
        dtype = _lib.DTYPE_F32 if ad.dtype == np.float32 else _lib.DTYPE_F64
        ts = self.so_lib.max_eigen_value_csr_gram_ex(
            self.sycl_q, dtype, n, len(ad), ap.ctypes.data, ai.ctypes.data, ad.ctypes.data,
            code, _lib.ST_CSR_EMPTY_ROWS_OK if allow_empty_rows else 0,
            eigen_val.ctypes.data, eigen_vec.ctypes.data, iter_cnt.ctypes.data,
            ctypes.byref(opt), None)
        _lib.check(ts, "max_eigen_value_csr_gram_ex", self.so_lib)
        return eigen_val[0], eigen_vec, int(ts), int(iter_cnt[0])

    @staticmethod
    def _csr_triple(m):
        """(indptr, indices, data, n) of one matrix of a sparse batch."""
        if isinstance(m, (tuple, list)):
            assert len(m) == 3, "a matrix is an (indptr, indices, data) triple !"
            indptr, indices, data = (np.asarray(a) for a in m)
            assert indptr.ndim == 1 and indices.ndim == 1 and data.ndim == 1, \
                "indptr, indices and data must be one-dimensional !"
            assert len(indptr) >= 2, "indptr must have n + 1 >= 2 elements !"
            return indptr, indices, data, len(indptr) - 1
        if hasattr(m, "crow_indices"):               # a torch.sparse_csr tensor
            assert m.dim() == 2 and m.shape[0] == m.shape[1], \
                "must be square matrices of floating points !"
            return (m.crow_indices().cpu().numpy(), m.col_indices().cpu().numpy(),
                    m.values().cpu().numpy(), int(m.shape[0]))
        if hasattr(m, "tocsr"):                      # any scipy.sparse matrix / array
            assert m.shape[0] == m.shape[1], "must be square matrices of floating points !"
            m = m.tocsr()
            return m.indptr, m.indices, m.data, int(m.shape[0])
        raise TypeError("(indptr, indices, data) triples or sparse matrices required, got "
                        f"{type(m).__name__}")

    def similarity_transform_csr_batched(self, mats, *, eps: Optional[float] = None,
                                         max_itr: int = 0, semantics: int = _lib.ST_SEM_SYCL,
                                         batch_rounds: int = 0):
        """MANY sparse matrices in one call (``max_eigen_value_csr_batched_ex``):
        ``mats`` is a sequence of ``(indptr, indices, data)`` triples,
        ``scipy.sparse`` matrices or ``torch.sparse_csr`` tensors, all square
        and of one dtype (float32 or float64), sizes free; an empty sequence is
        allowed.  They are concatenated into stacked CSR storage (``indptr``
        rebased, columns stay local), validated on the host and solved with
        one pair of launches per round for the whole batch; every matrix stops
        in its own round and gets the bits ``similarity_transform_csr`` gives
        it alone.  ``batch_rounds``: rounds per host check (0 = 8).

        Returns ``(λ[B], [v_0 .. v_{B-1}], ts_ms, iterations[B])``, the shape
        of ``similarity_transform_vbatched``'s result."""
        trip = [self._csr_triple(m) for m in mats]
        dt = np.asarray(trip[0][2]).dtype if trip else np.dtype(np.float32)
        for indptr, indices, data, n in trip:
            assert data.dtype == dt, "all matrices must have one dtype !"
            assert len(indptr) == n + 1, "indptr must have n + 1 elements !"
            assert n >= 1, "every matrix needs at least one row !"
            assert len(indices) == len(data), "indices and data must have one length !"
            assert np.asarray(indices).dtype.kind in "iu", "indices must be an integer array !"
        assert dt.num in (11, 12), "dtype of data must be float32 or float64 !"
        b = len(trip)
        if b == 0:
            return np.empty(0, dt), [], 0, np.zeros(0, np.uint32)
        for _, indices, _, _ in trip:
            if indices.size and (indices.min() < -2**31 or indices.max() >= 2**31):
                raise _lib.EigenValueError("csr: a column index does not fit int32")
        mat_first = np.concatenate([[0], np.cumsum([t[3] for t in trip])]).astype(np.int64)
        assert mat_first[-1] < 2**31, "the batch must have fewer than 2^31 rows in all !"
        mat_first = mat_first.astype(np.uint32)
        ptrs, base = [np.zeros(1, np.int64)], 0
        for indptr, _, _, _ in trip:               # rebase; validation is the library's
            ip = np.asarray(indptr, dtype=np.int64)
            ptrs.append(ip[1:] - ip[0] + base)
            base = int(ptrs[-1][-1])
        row_ptr = np.ascontiguousarray(np.concatenate(ptrs))
        col = np.ascontiguousarray(np.concatenate([t[1] for t in trip]), dtype=np.int32)
        vals = np.ascontiguousarray(np.concatenate([t[2] for t in trip]), dtype=dt)
        eigen_vals = np.empty(b, dtype=dt)
        eigen_vecs = np.empty(int(mat_first[-1]), dtype=dt)
        iter_cnts = np.zeros(b, dtype=np.uint32)
        opt = _lib.st_options(-1.0 if eps is None else float(eps), max_itr, semantics,
                              batch_rounds, _lib.ST_FLAG_MATRIX_FREE)
        dtype = _lib.DTYPE_F32 if dt == np.float32 else _lib.DTYPE_F64
        ts = self.so_lib.max_eigen_value_csr_batched_ex(
            self.sycl_q, dtype, b, mat_first.ctypes.data, len(vals), row_ptr.ctypes.data,
            col.ctypes.data, vals.ctypes.data, eigen_vals.ctypes.data, eigen_vecs.ctypes.data,
            iter_cnts.ctypes.data, None, ctypes.byref(opt), None)
        _lib.check(ts, "max_eigen_value_csr_batched_ex", self.so_lib)
        vs = [eigen_vecs[int(mat_first[i]):int(mat_first[i + 1])] for i in range(b)]
        return eigen_vals, vs, int(ts), iter_cnts

    def last_round_times(self) -> np.ndarray:
        """Per-round kernel times (ms) of the last ``similarity_transform_ex``
        call made with ``time_kernels=True`` (empty otherwise)."""
        L = self.so_lib
        n = _lib.check(L.st_last_round_times(self.sycl_q, None, 0), "st_last_round_times", L)
        out = np.zeros(n, dtype=np.float32)
        if n:
            _lib.check(L.st_last_round_times(self.sycl_q, out.ctypes.data, n),
                       "st_last_round_times", L)
        return out

    def last_round_sums(self) -> np.ndarray:
        """Row sums s_0 .. s_{rounds-1} of the last ``similarity_transform_ex``
        call made with ``trace_sums=True``, shape (rounds, n) (empty
        otherwise)."""
        n, dt = getattr(self, "_trace", (0, np.float32))
        return _lib.round_sums(self.so_lib, self.sycl_q, n, dt)

    # ------------------------------------------------------------------
    def close(self) -> None:
        if self.so_lib is not None and self.sycl_q is not None and self.sycl_q.value:
            self.so_lib.destroy_queue(self.sycl_q)
            self.sycl_q = ctypes.c_void_p()

    def __enter__(self) -> "EigenValue":
        return self

    def __exit__(self, *exc) -> None:
        self.close()
