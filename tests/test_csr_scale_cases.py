"""The generator and the vectorised model of csr_scale_cases.py, on the CPU:

1  the vectorised model of rows of 1 - 4 entries equals csr_order_model.matvec
   byte for byte, on values whose exponents spread so widely that the tree's
   grouping shows (asserted: the serial grouping differs on several rows)
2  the generator leaves no column empty and puts its heavy rows where asked
3  its transposition by a stable argsort is the library's host twin's
"""
import numpy as np
import pytest

import csr_order_model as om
import csr_scale_cases as sc
from eigen_value_amd import _lib
from eigen_value_amd import device as dev

DTYPES = [pytest.param("float32", id="f32"), pytest.param("float64", id="f64")]


def wide(rng, k, dt):
    """Mantissas in (0.5, 1] over 2^-12 .. 2^12: neighbours of very different
    size, so that nearly every addition rounds."""
    return (np.ldexp(1.0 - 0.5 * rng.random(k), rng.integers(-12, 13, size=k))).astype(dt)


@pytest.mark.parametrize("dtname", DTYPES)
def test_vectorised_model_is_the_order_model(dtname):
    dt = np.dtype(dtname)
    n = 2000
    ip, ix, _ = sc.big(n, 5, dt)
    assert sorted(set(np.diff(ip).tolist())) == [1, 2, 3, 4]
    rng = np.random.default_rng(17)
    da = wide(rng, len(ix), dt)
    s, v = wide(rng, n, dt), wide(rng, n, dt)
    # K0
    want0, _ = om.matvec(ip, ix, da, None, dt, ones=True)
    got0 = sc.rowsum_model(ip, da)
    assert got0.dtype == dt and got0.tobytes() == want0.tobytes()
    # a round
    x = v * s
    want, _ = om.matvec(ip, ix, da, x, dt)
    got = sc.product_model(ip, ix, da, x)
    assert got.dtype == dt and got.tobytes() == want.tobytes()
    m = s.max()
    r = sc.round_model(ip, ix, da, s, v, m)
    assert r["x"].tobytes() == x.tobytes()
    assert r["s_next"].tobytes() == (want / x).tobytes()
    assert r["v_cur"].tobytes() == (v * (s / m)).tobytes()
    # the power condition: the other grouping of four is visible
    p0 = sc.pad4(ip, da)
    p1 = p0 * sc.pad4(ip, x[ix])
    assert (sc.sum4_serial(p0) != got0).sum() >= 3
    assert (sc.sum4_serial(p1) != got).sum() >= 3
    # rows of fewer than 4 entries hold +0 in the idle lanes
    lens = np.diff(ip)
    assert (p0[lens == 1, 1:] == 0).all() and (p0[lens == 3, 3] == 0).all()


@pytest.mark.parametrize("dtname", DTYPES)
def test_heavy_rows_go_through_the_order_model(dtname):
    dt = np.dtype(dtname)
    n = 3000
    heavy = sc.heavy_at([0, 1500, n - 1])
    ip, ix, da = sc.big(n, 6, dt, heavy)
    rng = np.random.default_rng(3)
    x = (0.5 + rng.random(n)).astype(dt)
    want0, _ = om.matvec(ip, ix, da, None, dt, ones=True)
    want, _ = om.matvec(ip, ix, da, x, dt)
    assert sc.rowsum_model(ip, da).tobytes() == want0.tobytes()
    assert sc.product_model(ip, ix, da, x).tobytes() == want.tobytes()


def test_generator_covers_every_column_and_places_heavy_rows():
    n = 100_003
    rows = [0, 4095, 4096, 65535, 65536, n - 1]
    heavy = sc.heavy_at(rows)
    assert [heavy[r] for r in rows] == [17, 129, 2049, 17, 129, 2049]
    nnz_max, lanes = _lib.csr_class_limits()
    assert [int(np.searchsorted(np.array(nnz_max, np.int64), k)) for k in sc.HEAVY_LENS] == \
        [1, 2, 3]
    ip, ix, da = sc.big(n, 1, np.float32, heavy)
    lens = np.diff(ip)
    assert ip[0] == 0 and ip[-1] == len(ix) == len(da) and ip.dtype == np.int64
    assert ix.dtype == np.int32 and da.dtype == np.float32
    assert np.bincount(ix, minlength=n).min() >= 1 and ix.min() >= 0 and ix.max() < n
    assert (da > 0).all() and (da <= 1).all()
    plain = np.ones(n, bool)
    plain[rows] = False
    assert np.array_equal(lens[plain], (1 + np.arange(n) % 4)[plain])
    assert [int(lens[r]) for r in rows] == [heavy[r] for r in rows]
    # the same seed, the same matrix; another seed, another
    again = sc.big(n, 1, np.float32, heavy)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((ip, ix, da), again))
    assert sc.big(n, 2, np.float32, heavy)[1].tobytes() != ix.tobytes()


@pytest.mark.parametrize("dtname", DTYPES)
def test_argsort_transposition_is_the_host_twin(dtname):
    dt = np.dtype(dtname)
    n = 5000
    ip, ix, da = sc.big(n, 9, dt, sc.heavy_at([7, n - 1]))
    got = sc.transpose_argsort(ip, ix, da)
    want = dev.csr_transpose_host(ip, ix, da)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    # with empty columns, through the twin's allow_empty form
    ix2 = ix.copy()
    ix2[ix2 == 11] = 12
    got = sc.transpose_argsort(ip, ix2, da)
    want = dev.csr_transpose_host(ip, ix2, da, allow_empty=True)
    assert got[0][12] == got[0][11]
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
