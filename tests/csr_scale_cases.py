"""Matrices of millions of rows for the CSR tests at scale, and a vectorised
host model of their short rows, exact to the bit.

TEST INFRASTRUCTURE (numpy; no device).

big(n, seed, dtype, heavy)  rows of 1 + r % 4 entries, no empty column, a few
                            rows of the three longer classes where asked -
                            built with array operations (csr_cases.make_csr
                            loops over the rows)
pad4, sum4                  a row of at most 4 entries is of class 0: 4 lanes,
                            one entry each, and csr_order_model.tree pairs
                            neighbours: (l0 + l1) + (l2 + l3)
rowsum_model, round_model   K0 and one round of every row in the matrix's
                            dtype; the heavy rows through
                            csr_order_model.matvec
transpose_argsort           T(A) by numpy's stable argsort of the columns

Why the short-row model is exact: a lane of such a row runs one fused
multiply-add from +0, fma(a, x, +0), which is the product rounded once - what
numpy's multiply in that dtype gives; the lanes without an entry hold +0, and
t + 0 = t for every t >= 0; the two levels of the tree are one IEEE addition
each, numpy's again; so is the division by x[r].  Inputs are finite and
nonnegative (no -0 arises).
"""
from __future__ import annotations

import numpy as np

import csr_order_model as om

HEAVY_LENS = (17, 129, 2049)          # one more than the limits of classes 0, 1, 2


def heavy_at(rows):
    """{row: length} with HEAVY_LENS cycled over rows, in their order."""
    return {int(r): HEAVY_LENS[i % len(HEAVY_LENS)] for i, r in enumerate(rows)}


def big(n, seed, dtype, heavy=None):
    """(indptr, indices, data): row r holds 1 + r % 4 entries (heavy: {row:
    length} instead); the first of each row from a permutation of 0 .. n - 1,
    so no column is empty, the others from integers(0, n) - duplicates are
    legal; values 1 - random(), in (0, 1]."""
    rng = np.random.default_rng(seed)
    lens = 1 + np.arange(n, dtype=np.int64) % 4
    for r, k in (heavy or {}).items():
        assert 0 <= r < n
        lens[r] = k
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    nnz = int(indptr[-1])
    indices = rng.integers(0, n, size=nnz, dtype=np.int32)
    indices[indptr[:-1]] = rng.permutation(n).astype(np.int32)
    data = (1.0 - rng.random(nnz)).astype(dtype)
    return indptr, indices, data


def pad4(indptr, arr):
    """[n, 4]: entry j of row r, +0 past the row's end (of a longer row its
    first four: such rows are overwritten by the callers)."""
    n = len(indptr) - 1
    lens = np.diff(indptr)
    out = np.zeros((n, 4), dtype=arr.dtype)
    for j in range(4):
        has = lens > j
        out[has, j] = arr[indptr[:-1][has] + j]
    return out


def sum4(p):
    """The tree over 4 lanes, every add rounded in p's dtype."""
    return (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])


def sum4_serial(p):
    """A wrong order, for the tests' power condition: ((l0 + l1) + l2) + l3."""
    return ((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]


def _heavy_rows(indptr):
    return [int(r) for r in np.flatnonzero(np.diff(indptr) > 4)]


def rowsum_model(indptr, data):
    """K0: s[r] = the sum of row r in the kernel's order, in data's dtype."""
    dt = data.dtype
    s = sum4(pad4(indptr, data))
    heavy = _heavy_rows(indptr)
    if heavy:
        tot, _ = om.matvec(indptr, None, data, None, dt, ones=True, rows=heavy)
        s[heavy] = tot[heavy]
    return s


def product_model(indptr, indices, data, x):
    """(A x)[r] in the kernel's order (before the division), in data's dtype."""
    dt = data.dtype
    assert x.dtype == dt
    prod = pad4(indptr, data) * pad4(indptr, x[indices])     # fma(a, x, +0), rounded once
    y = sum4(prod)
    heavy = _heavy_rows(indptr)
    if heavy:
        tot, _ = om.matvec(indptr, indices, data, x, dt, rows=heavy)
        y[heavy] = tot[heavy]
    return y


def round_model(indptr, indices, data, s_prev, v_prev, m):
    """One round: x = v o s, s_next = (A x) / x, v_cur = v * (s / m) with m the
    published maximum of s_prev; all in data's dtype."""
    dt = data.dtype
    assert s_prev.dtype == dt and v_prev.dtype == dt
    x = v_prev * s_prev
    s_next = product_model(indptr, indices, data, x) / x
    v_cur = v_prev * (s_prev / dt.type(m))
    return {"x": x, "s_next": s_next, "v_cur": v_cur}


def transpose_argsort(indptr, indices, data):
    """T(A) by a stable argsort of the columns: the entries of one column keep
    their storage order (an empty column gives an empty row)."""
    n = len(indptr) - 1
    perm = np.argsort(indices, kind="stable")
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(indptr))
    t_indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(indices, minlength=n), out=t_indptr[1:])
    return t_indptr, rows[perm], data[perm]
