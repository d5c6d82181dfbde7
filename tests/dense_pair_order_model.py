"""A host model of the summation order of the RIGHT side of the dense Perron
pair kernels (k_pair_sum, k_pair_sweep), exact to the bit.

TEST INFRASTRUCTURE (numpy, csr_order_model's exact chain and tree,
dense_order_model.fma32; no device).  The left side of the pair is the left
solve's order: dense_left_order_model.columns models it unchanged.

st_pair.h documents the order of a row: the row is cut into strips of S
columns (st_pair_shape's strip_cols: 1024 in fp32, 512 in fp64, the last one
shorter); in a strip, lane l of 256 takes the Wc = 16 / itemsize adjacent
columns from strip * S + l * Wc in ascending order, one fused multiply-add
each from 0 (launch 0: the same fma with 1), columns past n left out and a
lane without a column holding +0; the 64 lanes of each of the four waves go
through the balanced tree, the four wave sums are added serially in wave
order; the strip values are added serially in ascending strip order, starting
from strip 0's value.  S is read from the library, nothing else enters.

  row(a, x, dt, strip)          one row's sum (x None: launch 0)
  rows(A, x, dt, which)         the model's sums of the chosen rows of A
  wrong_row(kind, ...)          the same data in one of the WRONG orders the
                                CPU test uses to show the inputs can tell
                                orders apart
  bound_ulps(n, strip)          the roundings a row's value passes through + 1
  model_rows(n, rb)             the rows a GPU test models

What follows the sum in the kernels - the division by x[r], v_prev * (s_prev /
m) - is one IEEE operation each and is numpy's on that dtype.
"""
from __future__ import annotations

import numpy as np

import csr_order_model as com
import dense_order_model as dom

BLOCK = com.BLOCK
SEED = 13
WRONG = ("lane_chain", "strips_tree", "mul_add", "half_strip", "waves_tree", "drop_last")


def shape(dtname, n):
    """(RB, S, combine_right) of an n x n matrix of dtname, from the library."""
    from eigen_value_amd import _lib
    code = _lib.DTYPE_F64 if np.dtype(dtname) == np.float64 else _lib.DTYPE_F32
    sh = _lib.pair_shape(code, int(n))
    return sh["rows"], sh["strip"], sh["combine_right"]


def lane_cols(dt):
    return 16 // np.dtype(dt).itemsize


def _lanes(a, x, dt, lo, hi, wc, lanes=BLOCK):
    """The lane values of the strip [lo, hi): lane l = the fma chain from 0
    over columns lo + l * wc + i, i ascending, below hi; +0 without a column."""
    dt = np.dtype(dt)
    am, ae = com._split(np.asarray(a, dtype=dt))
    xm, xe = (None, None) if x is None else com._split(np.asarray(x, dtype=dt))
    out = np.zeros(lanes, dtype=dt)
    for l in range(lanes):
        c = lo + l * wc
        if c >= hi:
            break
        out[l] = com._value(*com._chain(am, ae, xm, xe, range(c, min(c + wc, hi)),
                                        com.FORMAT[dt]), dt)
    return out


def _serial(vals, dt):
    t = dt.type(vals[0])
    for v in vals[1:]:
        t = dt.type(t + dt.type(v))
    return t


def row(a, x, dt, strip):
    """The sum of one row: a [n] its entries left to right, x [n] or None
    (launch 0), strip = S."""
    dt = np.dtype(dt)
    n, wc = len(a), lane_cols(dt)
    assert strip == BLOCK * wc
    vals = [com.block_sum(_lanes(a, x, dt, lo, min(lo + strip, n), wc))
            for lo in range(0, n, strip)]
    return _serial(vals, dt)


def wrong_row(kind, a, x, dt, strip):
    """One row in a WRONG order:
      lane_chain   a lane's chain runs on across the strips (k_mfree's own
                   order: one tree at the row's end)
      strips_tree  the strip values in a balanced tree (padded with +0)
      mul_add      the product rounded, then the sum rounded
      half_strip   strips of S / 2 columns (128 lanes of the tree hold +0)
      waves_tree   the four wave sums as (w0 + w1) + (w2 + w3)
      drop_last    the matrix's last column left out"""
    dt = np.dtype(dt)
    a = np.asarray(a, dtype=dt)
    xs = None if x is None else np.asarray(x, dtype=dt)
    n, wc = len(a), lane_cols(dt)
    starts = range(0, n, strip)
    if kind == "drop_last":
        if n == 1:
            return dt.type(0)
        return row(a[:-1], None if xs is None else xs[:-1], dt, strip)
    if kind == "half_strip":
        half = strip // 2
        vals = [com.block_sum(_lanes(a, xs, dt, lo, min(lo + half, n), wc))
                for lo in range(0, n, half)]
        return _serial(vals, dt)
    if kind == "strips_tree":
        vals = [com.block_sum(_lanes(a, xs, dt, lo, min(lo + strip, n), wc)) for lo in starts]
        size = 1
        while size < len(vals):
            size *= 2
        return com.tree(np.array(vals + [dt.type(0)] * (size - len(vals)), dtype=dt))
    if kind == "waves_tree":
        vals = []
        for lo in starts:
            lanes = _lanes(a, xs, dt, lo, min(lo + strip, n), wc)
            w = [com.tree(lanes[i:i + com.WAVE]) for i in range(0, BLOCK, com.WAVE)]
            vals.append(dt.type(dt.type(w[0] + w[1]) + dt.type(w[2] + w[3])))
        return _serial(vals, dt)
    if kind == "lane_chain":
        am, ae = com._split(a)
        xm, xe = (None, None) if xs is None else com._split(xs)
        lanes = np.zeros(BLOCK, dtype=dt)
        for l in range(BLOCK):
            idx = [c for lo in starts for c in range(lo + l * wc, min(lo + l * wc + wc, n))
                   if c < min(lo + strip, n)]
            if idx:
                lanes[l] = com._value(*com._chain(am, ae, xm, xe, idx, com.FORMAT[dt]), dt)
        return com.block_sum(lanes)
    if kind == "mul_add":
        vals = []
        for lo in starts:
            hi = min(lo + strip, n)
            lanes = np.zeros(BLOCK, dtype=dt)
            for l in range(BLOCK):
                for c in range(lo + l * wc, min(lo + l * wc + wc, hi)):
                    p = a[c] if xs is None else dt.type(a[c] * xs[c])
                    lanes[l] = dt.type(lanes[l] + p)
            vals.append(com.block_sum(lanes))
        return _serial(vals, dt)
    raise ValueError(kind)


def _rows_f32(A, x, strip):
    """fp32, vectorised over the rows: dense_order_model.fma32 lane by lane."""
    m, n = A.shape
    wc = lane_cols(np.float32)
    ns = -(-n // strip)
    pad = ns * strip - n
    Ap = np.concatenate([A, np.zeros((m, pad), np.float32)], axis=1).reshape(m, ns, BLOCK, wc)
    xv = np.ones(n, np.float32) if x is None else np.asarray(x, np.float32)
    xp = np.concatenate([xv, np.zeros(pad, np.float32)]).reshape(ns, BLOCK, wc)
    acc = np.zeros((m, ns, BLOCK), np.float32)
    for i in range(wc):                       # fma(0, 0, acc) = acc past n
        acc = dom.fma32(Ap[..., i], xp[None, ..., i], acc)
    vals = com.block_sum(acc)                 # [m, ns]
    t = vals[:, 0]
    for j in range(1, ns):
        t = t + vals[:, j]
    return t


def rows(A, x, dt, which=None, strip=None):
    """The model's sums of rows `which` (all when None) of the square A against
    x (None: launch 0): an array over which."""
    dt = np.dtype(dt)
    n = A.shape[0]
    if strip is None:
        strip = shape(dt, n)[1]
    which = list(range(n)) if which is None else list(which)
    if dt == np.float32:
        return _rows_f32(np.ascontiguousarray(A[which]), x, strip)
    return np.array([row(A[r], x, dt, strip) for r in which], dtype=dt)


def exact_row(a, x=None):
    return com.exact_row(np.asarray(a), None if x is None else np.asarray(x))


def bound_ulps(n, strip, dt=None):
    """The roundings a row's value passes through, plus one: Wc serial fmas in
    a lane, 6 tree levels, 3 serial wave adds, nstrips - 1 serial strip adds.
    (Each rounds a partial sum of nonnegative terms, so each adds at most one
    ulp of the final sum: dense_left_order_model.bound_ulps' derivation.)"""
    wc = strip // BLOCK
    return wc + 6 + 3 + (-(-n // strip) - 1) + 1


def model_rows(n, rb, limit=80, seed=SEED, in_flight=8):
    """The rows a GPU test models: all of them up to `limit`, else the tile
    boundaries, the tails (the last tile's rows past the last whole group of
    rows in flight) and a few seeded ones."""
    if n <= limit:
        return list(range(n))
    last0 = (n - 1) // rb * rb                     # the last tile's first row
    tail0 = last0 + (n - last0) // in_flight * in_flight
    want = {0, 1, in_flight - 1, in_flight, rb - 1, rb, rb + 1, 2 * rb - 1, 2 * rb, last0 - 1,
            last0, tail0 - 1, tail0, n - 1, n - 2, n - 3}
    rng = np.random.default_rng(seed + n)
    want |= {int(r) for r in rng.integers(0, n, size=6)}
    return sorted(r for r in want if 0 <= r < n)
