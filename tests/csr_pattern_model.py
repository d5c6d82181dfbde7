"""A host model of the pattern-only CSR row (st_csr_pattern.h), exact to the bit.

TEST INFRASTRUCTURE (numpy and fractions; no device).

The operator is diag(r) P diag(c), P the 0/1 pattern of (indptr, indices) with
duplicates counted.  The model is csr_order_model's, with the weights moved
out of the sweep as the kernels have it:

  x = round(v * s), z = round(c * x)      one rounding each (c None: z = x)
  lane t of the row's L lanes             acc = acc + z[col] over entries t,
                                          t + L, ... - lane_sums with a == 1:
                                          fma(1, z, acc) is acc + z
  tree / combine                          csr_order_model's
  tot = round(r[row] * tot)               r None: nothing
  terms                                   add_terms, dots = dot(w_j, x) on x
  s_next = tot / x[row]                   one IEEE division, numpy's

Launch 0 is the same with z = c (or ones) and no division.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import csr_order_model as om


def mul(a, b, dt):
    """Elementwise a * b in dt, one rounding each (finite inputs)."""
    dt = np.dtype(dt)
    a, b = np.asarray(a, dtype=dt), np.asarray(b, dtype=dt)
    out = np.zeros(a.shape, dtype=dt)
    for i in range(a.size):
        out.flat[i] = om.round_fraction(Fraction(float(a.flat[i])) * Fraction(float(b.flat[i])),
                                        dt)
    return out


def row(zs, dt, ones=False):
    """The sum of one pattern row over its gathered z (ones: z == 1) as the
    kernel leaves it after the tree; an empty row gives +0."""
    dt = np.dtype(dt)
    if len(zs) == 0:
        return dt.type(0)
    one = np.ones(len(zs), dtype=dt)
    return om.combine(om.lane_sums(one, None if ones else zs, dt, om.lanes_of(len(zs)), ones))


def sweep(indptr, indices, z, dt, rows=None):
    """tot[i] = row() of row i against z (z None: ones)."""
    dt = np.dtype(dt)
    n = len(indptr) - 1
    tot = np.zeros(n, dtype=dt)
    zz = None if z is None else np.asarray(z, dtype=dt)
    for i in (range(n) if rows is None else rows):
        lo, hi = int(indptr[i]), int(indptr[i + 1])
        cols = indices[lo:hi]
        tot[i] = row(np.ones(hi - lo, dtype=dt) if zz is None else zz[cols], dt, ones=zz is None)
    return tot


def rowsum(indptr, indices, r, c, dt, u=None, w=None):
    """Launch 0: s_0 = r * (P c), then the terms with dots = w_j . 1."""
    tot = sweep(indptr, indices, c, dt)
    if r is not None:
        tot = mul(r, tot, dt)
    if u is not None and len(u):
        dots = np.array([om.dot(w[j], None, dt, ones=True) for j in range(len(w))], dtype=dt)
        tot = om.add_terms(tot, u, dots, dt)
    return tot


def round_(indptr, indices, r, c, s, v, dt, u=None, w=None):
    """Launch k >= 1: dict with x, z, dots, s_next, v_cur."""
    dt = np.dtype(dt)
    s, v = np.asarray(s, dtype=dt), np.asarray(v, dtype=dt)
    x = mul(v, s, dt)
    z = x if c is None else mul(c, x, dt)
    tot = sweep(indptr, indices, z, dt)
    if r is not None:
        tot = mul(r, tot, dt)
    dots = np.zeros(0, dtype=dt)
    if u is not None and len(u):
        dots = np.array([om.dot(w[j], x, dt) for j in range(len(w))], dtype=dt)
        tot = om.add_terms(tot, u, dots, dt)
    return {"x": x, "z": z, "dots": dots, "s_next": tot / x, "v_cur": v * (s / s.max())}


def pow2_scales(n, seed, dt):
    """(r, c): powers of two in 2^-8 .. 2^8."""
    rng = np.random.default_rng(seed)
    return (np.ldexp(1.0, rng.integers(-8, 9, size=n)).astype(dt),
            np.ldexp(1.0, rng.integers(-8, 9, size=n)).astype(dt))


def general_scales(n, seed, dt, wide, x, indices):
    """(r, c) seeded in (0.5, 2], times 2^e, e in +-20 (fp32) / +-200 (fp64)
    when wide; c[col[0]] is then raised to a power of two that makes
    z[col[0]] = c * x the largest z: a redirected load that was added instead
    of dropped would show in every row."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed)
    r = 2.0 - 1.5 * rng.random(n)
    c = 2.0 - 1.5 * rng.random(n)
    if wide:
        e = 20 if dt == np.float32 else 200
        r = r * np.ldexp(1.0, rng.integers(-e, e + 1, size=n))
        c = c * np.ldexp(1.0, rng.integers(-e, e + 1, size=n))
    r, c = r.astype(dt), c.astype(dt)
    c0 = int(indices[0])
    z = c.astype(np.float64) * np.asarray(x, dtype=np.float64)
    z[c0] = 0
    c[c0] = dt.type(np.ldexp(1.0, int(np.ceil(np.log2(z.max() / float(x[c0])))) + 1))
    return r, c
