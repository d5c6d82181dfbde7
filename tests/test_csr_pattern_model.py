"""CPU: the host model of the pattern-only row (csr_pattern_model.py) against
csr_order_model's row on the matrices it must reproduce bit for bit.

1  r = c = 1: every row is row(ones, x)
2  r, c powers of two in 2^-8 .. 2^8 on regime A: every row is
   row(vals = r[row] * c[col], x) - scaling by 2^k commutes with every rounding
   while nothing under- or overflows
"""
import numpy as np
import pytest

import csr_order_model as om
import csr_pattern_model as pm

DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.uint8).reshape(len(got), -1)
                         != want.view(np.uint8).reshape(len(want), -1))
    assert got.tobytes() == want.tobytes(), (what, bad[:8])


def test_mul_rounds_once():
    a = np.array([1.0 + 2.0 ** -23, 3.0, 2.0 ** -100], dtype=np.float32)
    b = np.array([1.0 + 2.0 ** -23, 1.0 / 3.0, 2.0 ** -60], dtype=np.float32)
    same(pm.mul(a, b, np.float32), a * b, "fp32 products")
    a64, b64 = a.astype(np.float64) + 2.0 ** -50, b.astype(np.float64)
    same(pm.mul(a64, b64, np.float64), a64 * b64, "fp64 products")


@pytest.mark.parametrize("dt", DTYPES)
def test_without_scales_every_row_is_the_ones_matrix(dt):
    name = np.dtype(dt).name
    indptr, indices = om.structure()
    _, s, v = om.regime("A", name)
    ones = np.ones(len(indices), dtype=dt)
    x = v * s
    want0, _ = om.matvec(indptr, indices, ones, None, name, ones=True)
    want, _ = om.matvec(indptr, indices, ones, x, name)
    same(pm.rowsum(indptr, indices, None, None, name), want0, "launch 0")
    got = pm.round_(indptr, indices, None, None, s, v, name)
    same(got["x"], x, "x")
    same(got["z"], x, "z")
    same(got["s_next"], want / x, "s_next")


@pytest.mark.parametrize("which", ["c", "r", "rc"])
@pytest.mark.parametrize("dt", DTYPES)
def test_power_of_two_scales_are_the_scaled_values_matrix(dt, which):
    name = np.dtype(dt).name
    indptr, indices = om.structure()
    n = len(indptr) - 1
    _, s, v = om.regime("A", name)
    r, c = pm.pow2_scales(n, 77, dt)
    r = r if "r" in which else None
    c = c if "c" in which else None
    rows = np.repeat(np.arange(n), np.diff(indptr))
    vals = ((1 if r is None else r[rows]) * (1 if c is None else c[indices])
            * np.ones(len(indices))).astype(dt)
    x = v * s
    want0, _ = om.matvec(indptr, indices, vals, None, name, ones=True)
    want, _ = om.matvec(indptr, indices, vals, x, name)
    same(pm.rowsum(indptr, indices, r, c, name), want0, "launch 0")
    same(pm.round_(indptr, indices, r, c, s, v, name)["s_next"], want / x, "s_next")


def test_general_scales_put_the_largest_z_at_column_of_entry_0():
    indptr, indices = om.structure()
    n = len(indptr) - 1
    assert indptr[1] - indptr[0] == 1
    for dt, wide in ((np.float32, False), (np.float32, True), (np.float64, True)):
        _, s, v = om.regime("B" if wide else "A", np.dtype(dt).name)
        x = v * s
        r, c = pm.general_scales(n, 5, dt, wide, x, indices)
        z = pm.mul(c, x, dt)
        assert np.isfinite(z).all() and (r > 0).all() and (c > 0).all()
        assert int(np.argmax(z)) == int(indices[0]) and (z[indices[0]] > np.delete(z, indices[0])).all()
