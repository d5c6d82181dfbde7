"""Seeded sparse test matrices and a numpy model of the iteration.

TEST INFRASTRUCTURE (imported by tests/test_csr_capi.py, tests/test_gpu_csr.py
and tools/bench_csr.py; plain numpy, no device).

make_csr(n, d, seed, heavy): row r holds k = heavy.get(r, d) distinct columns,
default_rng(seed).choice(n, k, replace=False) sorted, with values
1 - rng.random(k) in (0, 1] - one generator, row after row.
"""
from __future__ import annotations

import numpy as np

# (n, d, seed, heavy?) - the whole-solve matrices; heavy = class_heavy()
TABLE = [(64, 8, 7, False), (3000, 32, 7, False), (3000, 32, 7, True)]


def class_limits():
    from eigen_value_amd import _lib
    return _lib.csr_class_limits()


def class_heavy(n: int = 3000) -> dict:
    """Rows on both sides of every class boundary of the library's table, a
    full row and two short ones; no row holds its diagonal alone."""
    nnz_max, _ = class_limits()
    m0, m1, m2 = (int(x) for x in nnz_max[:3])
    return {0: m0 + 1, 1: m0, 2: 2, 5: m1 + 1, 6: m1, 7: m2 + 1, 8: m2, 9: n, 11: 3}


def make_csr(n: int, d: int, seed: int, heavy: dict | None = None, dtype=np.float64):
    """(indptr int64 [n + 1], indices int32 [nnz], data dtype [nnz])."""
    heavy = heavy or {}
    rng = np.random.default_rng(seed)
    cols, vals, lens = [], [], []
    for r in range(n):
        k = min(int(heavy.get(r, d)), n)
        cols.append(np.sort(rng.choice(n, k, replace=False)))
        vals.append(1.0 - rng.random(k))
        lens.append(k)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (indptr, np.concatenate(cols).astype(np.int32),
            np.concatenate(vals).astype(dtype))


def densify(indptr, indices, data, n=None) -> np.ndarray:
    """The dense n x n matrix (duplicates add up, in storage order)."""
    n = len(indptr) - 1 if n is None else n
    a = np.zeros((n, n), dtype=data.dtype)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    np.add.at(a, (rows, indices), data)
    return a


def stop_test(s: np.ndarray, eps, cyclic: bool) -> bool:
    e = s.dtype.type(eps)
    d = np.abs(s - np.roll(s, -1))
    if not cyclic:
        d = d[:-1]
    return bool((d < e).all())


def model(a: np.ndarray, eps=1e-3, cyclic: bool = True, max_itr: int = 1000):
    """The matrix-free iteration in a's dtype on the dense matrix: (break
    index, converged, the list of s_k evaluated, v)."""
    T = a.dtype.type
    v = np.ones(a.shape[0], dtype=a.dtype)
    s = a.sum(axis=1, dtype=a.dtype)
    sums = []
    for k in range(max_itr):
        sums.append(s)
        stop = stop_test(s, eps, cyclic)
        m = T(max(T(0), s.max()))
        x = v * s
        v = v * (s / m)
        if stop:
            return k, True, sums, v
        s = (a @ x) / x
    return max_itr, False, sums, v


def count_of(break_index: int, converged: bool, cyclic: bool, max_itr: int = 1000) -> int:
    """iter_cnt as the library reports it (cpp:54 / main.py:47)."""
    if not converged:
        return max_itr
    return break_index if cyclic else break_index + 1


def write_bin(path, indptr, indices) -> None:
    """int64 n, int64 nnz, int64 row_ptr[n + 1], int32 col_idx[nnz]: the input
    of tests/cpp/csr_sanitize.cpp."""
    with open(path, "wb") as f:
        np.array([len(indptr) - 1, len(indices)], dtype=np.int64).tofile(f)
        np.ascontiguousarray(indptr, dtype=np.int64).tofile(f)
        np.ascontiguousarray(indices, dtype=np.int32).tofile(f)


if __name__ == "__main__":      # python tests/csr_cases.py DIR
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    for i, (n_, d_, seed_, heavy_) in enumerate(TABLE):
        ip_, ix_, _ = make_csr(n_, d_, seed_, class_heavy(n_) if heavy_ else None)
        write_bin(os.path.join(out, f"table{i}.bin"), ip_, ix_)
