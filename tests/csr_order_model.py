"""A host model of the summation order of the CSR kernels, exact to the bit.

TEST INFRASTRUCTURE (numpy and fractions; no device).

st_csr.h documents the order of a row product and st_csr_terms.h that of a
dot.  This module computes both in exact arithmetic, one IEEE rounding where
the kernel has one, so that a device result can be compared with tobytes():

  fma(a, x, acc, dt)   the exactly rounded fused multiply-add of fp32 / fp64
  row(a, x, dt)        one row: lane t of the row's L lanes starts from 0 and
                       takes entries t, t + L, ... in storage order, one fma
                       each; the L lane values are summed by the balanced
                       pairwise tree over the lane index (what wave_sum's DPP
                       steps amount to in the row's last lane); L = 256 adds
                       the four wave sums as ((w0 + w1) + w2) + w3
  dot(w, x, dt)        w . x in the order of k_csr_prep's vector pass and
                       k_csr_dots
  matvec, add_terms    every row of a matrix; the terms after the tree

L comes from the library (st_csr_class_limits).  kRows and kUnroll do not
enter: the documentation says they change no result.  What follows the tree
in the kernels - the division by x[r], v_prev * (s_prev / m) - is one IEEE
operation each and is numpy's on that dtype.

Inputs are finite and nonnegative, as the library requires of a matrix; the
sign of a zero is not modelled (every zero is +0).

The second half builds the case set the order tests share: one structure with
every row length that changes the path, and four value regimes on it.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

BLOCK = 256            # kBlock: lanes of a workgroup
WAVE = 64
DOT_GRID = 2048        # workgroup cap of the vector pass (st_csr_shape_desc: prep_grid)

# significand bits, exponent of the smallest subnormal, exponent past the largest finite
FORMAT = {np.dtype(np.float32): (24, -149, 128), np.dtype(np.float64): (53, -1074, 1024)}


# ---------------------------------------------------------------------------
# exact arithmetic
# ---------------------------------------------------------------------------
def round_fraction(q: Fraction, dt):
    """q rounded once to dt: nearest, ties to even, gradual underflow, inf past
    the largest finite value."""
    dt = np.dtype(dt)
    p, qmin, emax = FORMAT[dt]
    if q == 0:
        return dt.type(0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    # 2^e <= q < 2^(e + 1)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    lsb = max(e - p + 1, qmin)                  # exponent of the result's last place
    scaled = q / Fraction(2) ** lsb
    m = scaled.numerator // scaled.denominator
    rem = scaled - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    if m.bit_length() + lsb > emax:
        return dt.type(sign * math.inf)
    return dt.type(sign * math.ldexp(m, lsb))  # m < 2^53: exact in a double, then in dt


def fma(a, x, acc, dt):
    """a * x + acc with one rounding, in dt (a, x finite and nonnegative; an
    accumulator that has overflowed stays inf)."""
    if math.isinf(float(acc)):
        return np.dtype(dt).type(acc)
    return round_fraction(Fraction(float(a)) * Fraction(float(x)) + Fraction(float(acc)), dt)


def _split(v):
    """Finite floats as integer pairs: v[i] = m[i] * 2^e[i] exactly (lists)."""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))      # fp32 -> fp64 is exact
    return np.ldexp(m, 53).astype(np.int64).tolist(), (e - 53).tolist()


def _chain(am, ae, xm, xe, idx, fmt):
    """acc = 0; acc = fma(a[i], x[i], acc) for i in idx, on integer pairs
    (nonnegative data): (M, e) with acc = M * 2^e, M < 2^p; M = None is inf.
    xm = None: x == 1."""
    p, qmin, emax = fmt
    M, e = 0, 0
    for i in idx:
        if xm is None:
            pm, pe = am[i], ae[i]
        else:
            pm, pe = am[i] * xm[i], ae[i] + xe[i]
        if M is None:
            continue
        if M == 0:
            M, e = pm, pe
        elif pm != 0:
            if pe < e:
                M, e = (M << (e - pe)) + pm, pe
            else:
                M += pm << (pe - e)
        if M == 0:
            continue
        lsb = max(e + M.bit_length() - p, qmin)
        if lsb > e:                                       # inexact: one rounding
            sh = lsb - e
            rem, half = M & ((1 << sh) - 1), 1 << (sh - 1)
            M >>= sh
            if rem > half or (rem == half and M & 1):
                M += 1
            e = lsb
        if M.bit_length() + e > emax:
            M = None
    return M, e


def _value(M, e, dt):
    return dt.type(math.inf) if M is None else dt.type(math.ldexp(M, e))


def lane_sums(a, x, dt, L, ones=False, entries=None):
    """The L lane values of a row before the tree: lane t = the fma chain over
    entries t, t + L, ... from 0 (x: the gathered x[col], entry by entry).
    entries(t): another lane's share, for the tests' wrong orders."""
    dt = np.dtype(dt)
    a = np.asarray(a, dtype=dt)
    am, ae = _split(a)
    xm, xe = (None, None) if ones else _split(np.asarray(x, dtype=dt))
    out = np.zeros(L, dtype=dt)
    for t in range(L):
        idx = range(t, len(a), L) if entries is None else entries(t)
        out[t] = _value(*_chain(am, ae, xm, xe, idx, FORMAT[dt]), dt)
    return out


def tree(v):
    """The balanced pairwise sum over the lane index (len(v) a power of two),
    every add rounded: pairs, quads, the quads of a row of 16, then the rows -
    for 64 lanes (R3 + R2) + (R1 + R0)."""
    v = np.asarray(v)
    assert len(v) & (len(v) - 1) == 0
    while len(v) > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def combine(lanes):
    """The lanes of a row (4, 16, 64 or 256) to its sum."""
    if len(lanes) <= WAVE:
        return tree(lanes)
    w = [tree(lanes[i:i + WAVE]) for i in range(0, len(lanes), WAVE)]
    tot = w[0]
    for s in w[1:]:                                       # ((w0 + w1) + w2) + w3
        tot = tot + s
    return tot


@functools.lru_cache(maxsize=None)
def class_table():
    from eigen_value_amd import _lib
    nnz_max, lanes = _lib.csr_class_limits()
    return tuple(int(x) for x in nnz_max), tuple(int(x) for x in lanes)


@functools.lru_cache(maxsize=None)
def shape_desc():
    """st_csr_shape_desc (no GPU) as a dict of integer tuples: lanes, nnz_max
    (its last, unbounded class left out), rows, unroll, prep_grid."""
    from eigen_value_amd import _lib
    d = dict(kv.split("=") for kv in _lib.load().st_csr_shape_desc().decode().split())
    return {k: tuple(int(x) for x in v.split(",") if x.isdigit()) for k, v in d.items()}


def lanes_of(k):
    """L of a row of k entries (the first class with k <= nnz_max)."""
    nnz_max, lanes = class_table()
    return lanes[int(np.searchsorted(np.array(nnz_max, np.int64), k, side="left"))]


def bound_ulps(k):
    """test_gpu_csr.bound_ulps: the roundings a value passes through, plus one."""
    L = lanes_of(k)
    t = int(math.log2(L)) if L <= WAVE else 6 + 3
    return -(-k // L) + t + 1


def row(a, x, dt, ones=False):
    """The sum of one row as csr_rows leaves it after the tree; an empty row
    gives +0."""
    dt = np.dtype(dt)
    if len(a) == 0:
        return dt.type(0)
    return combine(lane_sums(a, x, dt, lanes_of(len(a)), ones))


def matvec(indptr, indices, vals, x, dt, ones=False, rows=None):
    """(tot [n], lanes): tot[r] = row() of row r against x (ones: x == 1, K0),
    lanes[r] the row's lane values; rows: only those (the others stay 0 /
    None)."""
    dt = np.dtype(dt)
    n = len(indptr) - 1
    vals = np.asarray(vals, dtype=dt)
    tot, lanes = np.zeros(n, dtype=dt), [None] * n
    for r in (range(n) if rows is None else rows):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        if hi == lo:
            continue
        xs = None if ones else np.asarray(x, dtype=dt)[indices[lo:hi]]
        lanes[r] = lane_sums(vals[lo:hi], xs, dt, lanes_of(hi - lo), ones)
        tot[r] = combine(lanes[r])
    return tot, lanes


def add_terms(tot, u, dots, dt):
    """tot[r] = fma(u[j][r], dots[j], tot[r]) for ascending j (u: [K, n])."""
    dt = np.dtype(dt)
    out = np.array(tot, dtype=dt)
    for j in range(len(u)):
        for r in range(len(out)):
            out[r] = fma(u[j][r], dots[j], out[r], dt)
    return out


def block_sum(v):
    """256 lane values of a workgroup: wave_sum of each wave, the four wave
    sums in wave order (vectorised over leading axes)."""
    v = np.asarray(v)
    w = v.reshape(v.shape[:-1] + (BLOCK // WAVE, WAVE))
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def dot_grid(n):
    return min(-(-n // BLOCK), DOT_GRID)


def dot(w, x, dt, ones=False):
    """w . x as the vector pass and k_csr_dots compute it (ones: x == 1, K0's
    k_csr_wsum)."""
    dt = np.dtype(dt)
    n = len(w)
    g = dot_grid(n)
    wm, we = _split(np.asarray(w, dtype=dt))
    xm, xe = (None, None) if ones else _split(np.asarray(x, dtype=dt))
    acc = np.zeros(g * BLOCK, dtype=dt)                   # lane t of workgroup b: b * 256 + t
    for i in range(min(n, g * BLOCK)):
        acc[i] = _value(*_chain(wm, we, xm, xe, range(i, n, g * BLOCK), FORMAT[dt]), dt)
    partial = block_sum(acc.reshape(g, BLOCK))
    lanes = np.zeros(BLOCK, dtype=dt)                     # k_csr_dots: plain adds from 0
    for i in range(0, g, BLOCK):
        part = partial[i:i + BLOCK]
        lanes[:len(part)] = lanes[:len(part)] + part
    return block_sum(lanes)


def exact_row(a, x=None):
    """The exact sum of a[i] * x[i] (x None: of a[i]) as a Fraction."""
    am, ae = _split(a)
    if x is not None:
        xm, xe = _split(x)
        am, ae = [p * q for p, q in zip(am, xm)], [p + q for p, q in zip(ae, xe)]
    if not am:
        return Fraction(0)
    lo = min(ae)
    return Fraction(sum(m << (e - lo) for m, e in zip(am, ae))) * Fraction(2) ** lo


def err_ulps(s, exact: Fraction, dt):
    """|s - exact| in units of dt's spacing at exact (the subnormal spacing
    below the smallest normal)."""
    p, qmin, _ = FORMAT[np.dtype(dt)]
    if exact == 0:
        return 0.0 if s == 0 else math.inf
    e = exact.numerator.bit_length() - exact.denominator.bit_length()
    if Fraction(2) ** e > exact:
        e -= 1
    return float(abs(Fraction(float(s)) - exact) / Fraction(2) ** max(e - p + 1, qmin))


# ---------------------------------------------------------------------------
# the case set: one structure, four value regimes
# ---------------------------------------------------------------------------
REGIMES = ("A", "B", "C", "D")
SEED = 9               # chosen so that test_csr_order_model's power condition holds
ZERO_ROWS = 3          # regime D: rows that hold only stored zeros
TINY_ROWS = 8          # regime C: rows whose entries are subnormal themselves


def row_lengths(seed=SEED, n_rows=336):
    """Every length that changes the path, several rows at each class limit
    (a limit off by one shows in rows of exactly that length), a dozen rows of
    every class, the rest short."""
    nnz_max, lanes = class_table()
    rng = np.random.default_rng(seed)
    lens = [1, 2]
    for L in lanes:
        lens += [L - 1, L, L + 1]
    for m in nnz_max[:-1]:                                # 16, 128: cheap; 2048: 9 each
        lens += [m, m + 1] * (16 if m <= 128 else 9)
    for L, u in zip(lanes, shape_desc()["unroll"]):       # the trips of the sweep
        lens += [u * L - 1, u * L, u * L + 1, 2 * u * L - 1, 2 * u * L, 2 * u * L + 1]
    lens += [int(x) for x in rng.integers(2050, 2600, size=4)]     # class 3: 17 rows in all
    lens += [int(x) for x in rng.integers(130, 600, size=6)]       # class 2
    lens += [int(x) for x in rng.integers(1, 200, size=n_rows - len(lens))]
    lens = np.array(lens, dtype=np.int64)
    rng.shuffle(lens)
    first = int(np.flatnonzero(lens == 1)[0])             # row 0 holds one entry: entry 0, to
    lens[[0, first]] = lens[[first, 0]]                   # which loads past a row's end go
    return lens


@functools.lru_cache(maxsize=None)
def structure(seed=SEED):
    """(indptr, indices) of the square case matrix: n = 336, rows shuffled so
    that the classes interleave in the plan, columns unsorted, rows longer
    than n with duplicate columns."""
    lens = row_lengths(seed)
    n = len(lens)
    rng = np.random.default_rng(seed + 1000)
    cols = [rng.choice(n, int(k), replace=False) if k <= n else rng.integers(0, n, size=int(k))
            for k in lens]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return indptr, np.concatenate(cols).astype(np.int32)


def _mant(rng, k):
    return 1.0 - 0.5 * rng.random(k)                      # (0.5, 1]


def _pow2(rng, lo, hi, k):
    return np.ldexp(1.0, rng.integers(lo, hi + 1, size=k))


@functools.lru_cache(maxsize=None)
def regime(name, dtname, seed=SEED):
    """(vals, s_prev, v_prev) of one regime in dtype dtname on structure(seed);
    x = v_prev * s_prev in that dtype.

    A  the benign data of the other CSR tests: values in (0, 1], s and v in
       [0.5, 2); x[col[0]] is made exactly 4 (s = v = 2 there), so that a
       dropped product of a poisoned entry 0 is inf
    B  a wide range: a = 2^e m, e in +-20 (fp32) / +-200 (fp64), x = 2^f m', f
       in +-10, m in (0.5, 1]
    C  underflow: a ~ 2^-100 .. 2^-80 and x ~ 2^-40 (fp32), a ~ 2^-1000 ..
       2^-956 and x ~ 2^-60 (fp64): subnormal products, partial sums on both
       sides of the smallest normal; TINY_ROWS rows hold subnormal entries
    D  A with a tenth of the entries +0 and ZERO_ROWS rows all zero"""
    dt = np.dtype(dtname)
    f32 = dt == np.float32
    indptr, indices = structure(seed)
    n, nnz = len(indptr) - 1, len(indices)
    rng = np.random.default_rng(seed * 100 + REGIMES.index(name) * 10 + (0 if f32 else 1))
    if name in ("A", "D"):
        vals = 1.0 - rng.random(nnz)
        s = 0.5 + 1.5 * rng.random(n)
        v = 0.5 + 1.5 * rng.random(n)
        s[indices[0]] = v[indices[0]] = 2.0
        if name == "D":
            zero = rng.random(nnz) < 0.1
            zero[0] = False                               # entry 0 stays an ordinary value
            vals[zero] = 0.0
            lens = np.diff(indptr)
            short = np.flatnonzero((lens > 2) & (lens < 100))
            for r in list(rng.choice(short, ZERO_ROWS - 1, replace=False)) + \
                    [int(np.flatnonzero(lens > 2048)[0])]:
                vals[indptr[r]:indptr[r + 1]] = 0.0
    elif name == "B":
        vals = _pow2(rng, *((-20, 20) if f32 else (-200, 200)), nnz) * _mant(rng, nnz)
        vals[0] = np.ldexp(vals[0], (20 if f32 else 200) - int(np.frexp(vals[0])[1]))
        s = _pow2(rng, -5, 5, n) * _mant(rng, n)
        v = _pow2(rng, -5, 5, n) * _mant(rng, n)
    else:
        vals = _pow2(rng, *((-100, -80) if f32 else (-1000, -956)), nnz) * _mant(rng, nnz)
        h = -20 if f32 else -30
        s = np.ldexp(0.5 + 1.5 * rng.random(n), h)
        v = np.ldexp(0.5 + 1.5 * rng.random(n), h)
        lens = np.diff(indptr)
        for r in rng.choice(np.flatnonzero(lens > 2), TINY_ROWS, replace=False):
            k = int(lens[r])
            vals[indptr[r]:indptr[r + 1]] = np.ldexp(_mant(rng, k), -140 if f32 else -1040)
    vals, s, v = vals.astype(dt), s.astype(dt), v.astype(dt)
    for arr in (vals, s, v):
        arr.setflags(write=False)
    return vals, s, v


_MODEL = {}


def model(name, dtname, seed=SEED):
    """The model's pass over one regime, computed once and left unchanged:
    dict with x = v * s, sum0 / lanes0 (K0: x == 1) and sum / lanes (against
    x)."""
    key = (name, dtname, seed)
    if key not in _MODEL:
        indptr, indices = structure(seed)
        vals, s, v = regime(name, dtname, seed)
        x = v * s
        sum0, lanes0 = matvec(indptr, indices, vals, None, dtname, ones=True)
        tot, lanes = matvec(indptr, indices, vals, x, dtname)
        for arr in (x, sum0, tot):
            arr.setflags(write=False)
        _MODEL[key] = {"x": x, "sum0": sum0, "lanes0": lanes0, "sum": tot, "lanes": lanes}
    return _MODEL[key]


@functools.lru_cache(maxsize=None)
def second_structure(seed=SEED):
    """Another matrix of the same size, B of the product tests and a member of
    the batch: structure(seed + 1), except that no entry gathers column 0 (a
    poisoned entry 0 of A makes y[0] inf or NaN, and every other row of B y
    must stay clean) and that its own entry 0 gathers the longest row of A,
    where y is far above 1 (so that its dropped products overflow)."""
    indptr, indices = structure(seed + 1)
    indices = indices.copy()
    indices[indices == 0] = 1
    indices[0] = int(np.argmax(np.diff(structure(seed)[0])))
    indices.setflags(write=False)
    return indptr, indices


PLAN_N = 65536 + 300


@functools.lru_cache(maxsize=None)
def plan_structure(seed=SEED):
    """(indptr, indices, heavy rows) of a matrix whose plan takes more than 256
    blocks of 256 rows, so that each lane of k_csr_scan sums a span of several
    blocks: rows of two entries, and in every span one row each of two of the
    three other classes, in turn."""
    n = PLAN_N
    rng = np.random.default_rng(seed + 2000)
    nblk = -(-n // BLOCK)
    span = -(-nblk // BLOCK) * BLOCK                      # rows per lane of the scan
    assert nblk > BLOCK
    lens = np.full(n, 2, dtype=np.int64)
    heavy = []
    for i, lo in enumerate(range(0, n, span)):
        rows = lo + rng.choice(min(span, n - lo), 2, replace=False)
        for r, c in zip(rows, (i % 3, (i + 1) % 3)):
            lens[r] = (rng.integers(17, 129), rng.integers(129, 400), rng.integers(2049, 2052))[c]
            heavy.append(int(r))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = rng.integers(0, n, size=int(indptr[-1])).astype(np.int32)
    return indptr, indices, tuple(sorted(heavy))
