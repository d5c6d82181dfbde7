"""Seeded cases for the CSR solve with low-rank terms and empty rows.

TEST INFRASTRUCTURE (imported by tests/test_csr_terms_capi.py,
tests/test_gpu_csr_terms.py and tools/bench_csr_terms.py; plain numpy, no
device).  The sparse matrices, the dense model and the counts come from
csr_cases.py; here are the link graph of the PageRank test, the dense
operator M = A + sum_j u_j w_j^T, the swap of the term vectors for the left
solve and matrices with rows emptied.
"""
from __future__ import annotations

import numpy as np

BLOCK = 256
DOT_GRID = 2048                     # the vector pass's workgroup cap (st_csr_terms_shape_desc)


def graph(n, seed=5):                      # n >= 12
    """A reducible, periodic link graph with dangling nodes: the first half
    links among itself, the second half is one directed cycle, the last 10
    rows have no out-links."""
    rng = np.random.default_rng(seed); A = np.zeros((n, n)); h = n // 2
    for r in range(h):
        A[r, rng.choice(h, rng.integers(1, 6), replace=False)] = 1
    for r in range(h, n - 10):
        A[r, h + (r - h + 1) % (n - 10 - h)] = 1     # one directed cycle
    A[0, n - 1] = 1; A[1, n - 2] = 1                   # last 10 rows: no out-links
    return A


def to_csr(a: np.ndarray, dtype=np.float64):
    """(indptr, indices, data) of the nonzeros of a dense matrix, columns
    ascending; rows without one are empty."""
    rows, cols = np.nonzero(a)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=a.shape[0]))])
    return indptr.astype(np.int64), cols.astype(np.int32), a[rows, cols].astype(dtype)


def empty_rows(indptr, indices, data, rows):
    """The matrix with the given rows emptied."""
    indptr = np.asarray(indptr, np.int64)
    keep = np.ones(len(indices), dtype=bool)
    lens = np.diff(indptr).copy()
    for r in rows:
        keep[indptr[r]:indptr[r + 1]] = False
        lens[r] = 0
    return (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), indices[keep], data[keep])


def term_vectors(n, K, seed, dtype=np.float64, lo=0.01, hi=0.05):
    """K seeded pairs of positive vectors: (u [K, n], w [K, n])."""
    rng = np.random.default_rng(seed)
    u = (lo + (hi - lo) * rng.random((K, n))).astype(dtype)
    w = (lo + (hi - lo) * rng.random((K, n))).astype(dtype)
    return u, w


def dense_m(a: np.ndarray, u, w) -> np.ndarray:
    """A + sum_j u_j w_j^T in a's dtype, term after term."""
    m = a.copy()
    for uj, wj in zip(u, w):
        m = m + np.outer(np.asarray(uj, a.dtype), np.asarray(wj, a.dtype))
    return m


def swap(u, w):
    """The terms of M^T = A^T + sum_j w_j u_j^T."""
    return w, u


def google(A: np.ndarray, alpha=0.85, teleport=None, dangling=None):
    """(P^T scaled by alpha as a dense matrix, u [K, n], w [K, n], dense G^T)
    of the link graph A, as DeviceSolver.pagerank builds them."""
    n = A.shape[0]
    out = A.sum(axis=1)
    empty = out == 0
    P = A / np.where(empty, 1.0, out)[:, None]
    t = np.full(n, 1.0 / n) if teleport is None else teleport / teleport.sum()
    one, ind = np.ones(n), empty.astype(np.float64)
    if dangling is None:
        u, w = [t], [(1.0 - alpha) * one + alpha * ind]
    else:
        u, w = [t, dangling / dangling.sum()], [(1.0 - alpha) * one, alpha * ind]
    aPt = alpha * P.T
    return aPt, np.array(u), np.array(w), dense_m(aPt, u, w)


def dot_depth(n: int) -> int:
    """The roundings a value passes through in a dot of n elements, from the
    order st_csr_terms.h fixes: G = min(ceil(n / 256), 2048) workgroups; a
    lane's ceil(n / (256 G)) fmas, the 6 levels of the wave tree, 3 serial
    adds of the wave sums; then the combine: a lane's ceil(G / 256) adds, 6
    levels, 3 adds."""
    g = min(-(-n // BLOCK), DOT_GRID)
    return -(-n // (BLOCK * g)) + 6 + 3 + -(-g // BLOCK) + 6 + 3
