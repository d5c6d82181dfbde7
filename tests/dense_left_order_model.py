"""A host model of the summation order of the dense left-vector kernels, exact
to the bit.

TEST INFRASTRUCTURE (numpy and csr_order_model's exact arithmetic; no device).

st_left.h documents the order of a column: the rows are cut into blocks of RB
consecutive rows (the last one shorter); within a block one accumulator starts
from 0 and takes the rows in ascending order, one fused multiply-add each
(launch 0: the same fma with 1); the block values are combined in the form
st_left_shape reports - 0: serially in ascending block order, starting from
block 0's value; 1: a balanced pairwise tree over the block index (padded
with +0 to a power of two).  RB and the form are read from the library
(st_left_shape), nothing else enters.

  column(a, x, dt, rb, comb)      one column's sum (x None: launch 0)
  columns(A, x, dt, cols)         the model's sums of the chosen columns of A
  wrong_column(kind, ...)         the same data in one of the WRONG orders the
                                  CPU test uses to show the inputs can tell
                                  orders apart

What follows the sum in the kernels - the division by x[c], v_prev * (s_prev /
m) - is one IEEE operation each and is numpy's on that dtype.

The second half builds the case set: dense matrices of any n in the four value
regimes of csr_order_model (benign, wide exponents, underflow, stored zeros).
"""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

import csr_order_model as com

REGIMES = com.REGIMES
SEED = 11
WRONG = ("descending", "sub_blocks", "mul_add", "rb_plus", "rb_minus", "drop_last",
         "other_combine")


def shape(dtname, n):
    """(RB, combine) of an n x n matrix of dtname, from the library."""
    from eigen_value_amd import _lib
    code = _lib.DTYPE_F64 if np.dtype(dtname) == np.float64 else _lib.DTYPE_F32
    sh = _lib.left_shape(code, int(n))
    return sh["rows"], sh["combine"]


def strip_of(dtname, n):
    """The columns of one workgroup for this n: block * W, W = 16 bytes of
    elements when n * b is a multiple of 16, else 1 (it does not enter the
    order; the tests pick sizes around it)."""
    from eigen_value_amd import _lib
    code = _lib.DTYPE_F64 if np.dtype(dtname) == np.float64 else _lib.DTYPE_F32
    sh = _lib.left_shape(code, int(n))
    return sh["block"] * (sh["w"] if n % sh["w"] == 0 else 1)


def _blocks(n, rb):
    return [(lo, min(lo + rb, n)) for lo in range(0, n, rb)]


def _combine(vals, comb, dt):
    vals = [dt.type(v) for v in vals]
    if comb == 0:
        t = vals[0]
        for v in vals[1:]:
            t = dt.type(t + v)
        return t
    size = 1
    while size < len(vals):
        size *= 2
    return com.tree(np.array(vals + [dt.type(0)] * (size - len(vals)), dtype=dt))


def column(a, x, dt, rb, comb):
    """The sum of one column: a [n] its entries top to bottom, x [n] or None
    (launch 0)."""
    dt = np.dtype(dt)
    am, ae = com._split(np.asarray(a, dtype=dt))
    xm, xe = (None, None) if x is None else com._split(np.asarray(x, dtype=dt))
    vals = [com._value(*com._chain(am, ae, xm, xe, range(lo, hi), com.FORMAT[dt]), dt)
            for lo, hi in _blocks(len(a), rb)]
    return _combine(vals, comb, dt)


def wrong_column(kind, a, x, dt, rb, comb):
    """One column in a WRONG order:
      descending     a block's rows from its last to its first
      sub_blocks     a block cut into 4 contiguous runs of rows, one accumulator
                     each (what a lane would do if its column accumulators took
                     consecutive rows instead of consecutive columns), added in
                     run order
      mul_add        the product rounded, then the sum rounded
      rb_plus / rb_minus   blocks of RB + 1 / RB - 1 rows
      drop_last      the matrix's last row left out
      other_combine  the block values in the other form (tree for serial)"""
    dt = np.dtype(dt)
    a = np.asarray(a, dtype=dt)
    xs = None if x is None else np.asarray(x, dtype=dt)
    if kind == "rb_plus":
        return column(a, xs, dt, rb + 1, comb)
    if kind == "rb_minus":
        return column(a, xs, dt, rb - 1, comb)
    if kind == "drop_last":
        return column(a[:-1], None if xs is None else xs[:-1], dt, rb, comb)
    if kind == "other_combine":
        return column(a, xs, dt, rb, comb ^ 1)
    am, ae = com._split(a)
    xm, xe = (None, None) if xs is None else com._split(xs)
    fmt = com.FORMAT[dt]
    vals = []
    for lo, hi in _blocks(len(a), rb):
        if kind == "descending":
            vals.append(com._value(*com._chain(am, ae, xm, xe, range(hi - 1, lo - 1, -1), fmt),
                                   dt))
        elif kind == "sub_blocks":
            run = -(-(hi - lo) // 4)
            t = None
            for q in range(lo, hi, run):
                v = com._value(*com._chain(am, ae, xm, xe, range(q, min(q + run, hi)), fmt), dt)
                t = v if t is None else dt.type(t + v)
            vals.append(t)
        elif kind == "mul_add":
            acc = dt.type(0)
            for r in range(lo, hi):
                acc = dt.type(acc + (a[r] if xs is None else dt.type(a[r] * xs[r])))
            vals.append(acc)
        else:
            raise ValueError(kind)
    return _combine(vals, comb, dt)


def columns(A, x, dt, cols=None, rb=None, comb=None):
    """The model's sums of columns `cols` (all when None) of the square A
    against x (None: launch 0): an array over cols."""
    dt = np.dtype(dt)
    n = A.shape[0]
    if rb is None:
        rb, comb = shape(dt, n)
    cols = range(n) if cols is None else cols
    return np.array([column(A[:, c], x, dt, rb, comb) for c in cols], dtype=dt)


def exact_column(a, x=None) -> Fraction:
    return com.exact_row(np.asarray(a), None if x is None else np.asarray(x))


def bound_ulps(n, rb, comb):
    """The roundings a column's value passes through, plus one: RB serial fmas,
    then nrb - 1 serial adds (or ceil(log2 nrb) tree levels)."""
    nrb = -(-n // rb)
    levels = nrb - 1 if comb == 0 else (nrb - 1).bit_length()
    return min(rb, n) + levels + 1


def model_columns(n, strip, w, limit=80, seed=SEED):
    """The columns a GPU test models: all of them up to `limit`, else the ones
    where a tail or a strip boundary would show, and a few seeded ones."""
    if n <= limit:
        return list(range(n))
    want = {0, 1, 2, 3, w - 1, w, w + 1, strip - 1, strip, strip + 1, 2 * strip - 1, 2 * strip,
            2 * strip + 1, n - 1, n - 2, n - 3, n - w, n - w - 1}
    rng = np.random.default_rng(seed + n)
    want |= {int(c) for c in rng.integers(0, n, size=8)}
    return sorted(c for c in want if 0 <= c < n)


# ---------------------------------------------------------------------------
# the case set: dense matrices in four value regimes
# ---------------------------------------------------------------------------
def _mant(rng, shape_):
    return 1.0 - 0.5 * rng.random(shape_)                 # (0.5, 1]


def _pow2(rng, lo, hi, shape_):
    return np.ldexp(1.0, rng.integers(lo, hi + 1, size=shape_))


@functools.lru_cache(maxsize=64)
def regime(name, dtname, n, seed=SEED):
    """(A [n, n], s_prev [n], v_prev [n]) of one regime in dtype dtname,
    read-only; x = v_prev * s_prev in that dtype.

    A  benign: entries in (0, 1], s and v in [0.5, 2)
    B  a wide range: a = 2^e m, e in +-20 (fp32) / +-200 (fp64), s and v
       2^f m', f in +-5, m in (0.5, 1]
    C  underflow: a ~ 2^-100 .. 2^-80 and x ~ 2^-40 (fp32), a ~ 2^-1000 ..
       2^-956 and x ~ 2^-60 (fp64): subnormal products, partial sums on both
       sides of the smallest normal; the last column's entries are subnormal
       themselves
    D  A with a tenth of the entries +0, and (n >= 3) column 1 all zero"""
    dt = np.dtype(dtname)
    f32 = dt == np.float32
    rng = np.random.default_rng(seed * 1000 + REGIMES.index(name) * 10 + (0 if f32 else 1) + 7 * n)
    if name in ("A", "D"):
        A = 1.0 - rng.random((n, n))
        s = 0.5 + 1.5 * rng.random(n)
        v = 0.5 + 1.5 * rng.random(n)
        if name == "D":
            A[rng.random((n, n)) < 0.1] = 0.0
            if n >= 3:
                A[:, 1] = 0.0
    elif name == "B":
        A = _pow2(rng, *((-20, 20) if f32 else (-200, 200)), (n, n)) * _mant(rng, (n, n))
        s = _pow2(rng, -5, 5, n) * _mant(rng, n)
        v = _pow2(rng, -5, 5, n) * _mant(rng, n)
    else:
        A = _pow2(rng, *((-100, -80) if f32 else (-1000, -956)), (n, n)) * _mant(rng, (n, n))
        h = -20 if f32 else -30
        s = np.ldexp(0.5 + 1.5 * rng.random(n), h)
        v = np.ldexp(0.5 + 1.5 * rng.random(n), h)
        A[:, n - 1] = np.ldexp(_mant(rng, n), -140 if f32 else -1040)
    A, s, v = np.ascontiguousarray(A.astype(dt)), s.astype(dt), v.astype(dt)
    for arr in (A, s, v):
        arr.setflags(write=False)
    return A, s, v
