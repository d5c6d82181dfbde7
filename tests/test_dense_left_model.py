"""CPU: the host model of the dense left-vector order (dense_left_order_model)
and the power of its inputs - every wrong order tried must show in at least
three columns of every value regime and dtype, or a device test that compares
bytes with the model would prove nothing.  No GPU needed."""
import numpy as np
import pytest

import csr_order_model as com
import dense_left_order_model as dlm

DTYPES = ("float32", "float64")
MIN_COLUMNS = 3


def _n():
    """Five row blocks, the last of 5 rows: serial and tree differ from four
    blocks on, RB - 1 / RB + 1 shift every block boundary, odd n."""
    rb, _ = dlm.shape("float32", 1)
    n = 4 * rb + 5
    for dt in DTYPES:
        assert dlm.shape(dt, n)[0] == rb
    return n


@pytest.fixture(scope="module")
def sums():
    """{(regime, dtype): (model [n], {wrong: [n]})} of the round's numerators,
    computed once."""
    n = _n()
    out = {}
    for name in dlm.REGIMES:
        for dt in DTYPES:
            A, s, v = dlm.regime(name, dt, n)
            x = v * s
            rb, comb = dlm.shape(dt, n)
            model = dlm.columns(A, x, dt)
            wrong = {k: np.array([dlm.wrong_column(k, A[:, c], x, dt, rb, comb)
                                  for c in range(n)], dtype=dt) for k in dlm.WRONG}
            out[name, dt] = (model, wrong)
    return out


def test_shape_is_sane_and_a_function_of_dtype_and_n():
    for dt in DTYPES:
        last = 0
        for n in (1, 2, 31, 32, 33, 2047, 2048, 4095, 4096, 16383, 16384, 131072):
            rb, comb = dlm.shape(dt, n)
            assert rb >= 1 and comb in (0, 1)
            assert rb >= last                         # never smaller for a larger matrix
            assert dlm.shape(dt, n) == (rb, comb)     # asked twice, the same
            last = rb


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", dlm.REGIMES)
def test_every_wrong_order_shows_in_three_columns(sums, name, dt):
    model, wrong = sums[name, dt]
    for kind, got in wrong.items():
        differ = int((got.view(np.uint8).reshape(len(got), -1)
                      != model.view(np.uint8).reshape(len(model), -1)).any(axis=1).sum())
        assert differ >= MIN_COLUMNS, (name, dt, kind, differ)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", dlm.REGIMES)
def test_launch0_wrong_orders_show_too(name, dt):
    """The column sums (x == 1): multiply-then-add is the same arithmetic
    there, every other wrong order must show."""
    n = _n()
    A, _, _ = dlm.regime(name, dt, n)
    rb, comb = dlm.shape(dt, n)
    model = dlm.columns(A, None, dt)
    for kind in dlm.WRONG:
        if kind == "mul_add":
            continue
        got = np.array([dlm.wrong_column(kind, A[:, c], None, dt, rb, comb) for c in range(n)],
                       dtype=dt)
        assert int((got != model).sum()) >= MIN_COLUMNS, (name, dt, kind)


@pytest.mark.parametrize("dt", DTYPES)
def test_model_agrees_with_plain_arithmetic(dt):
    """fma by fma through round_fraction, and the serial combine by numpy adds:
    the model's fast path is the documented order."""
    n = 70
    A, s, v = dlm.regime("A", dt, n)
    x = v * s
    rb, comb = dlm.shape(dt, n)
    assert comb == 0
    t = np.dtype(dt).type
    for c in (0, 1, n - 1):
        blocks = []
        for lo in range(0, n, rb):
            acc = t(0)
            for r in range(lo, min(lo + rb, n)):
                acc = com.fma(A[r, c], x[r], acc, dt)
            blocks.append(acc)
        want = blocks[0]
        for b in blocks[1:]:
            want = t(want + b)
        assert dlm.column(A[:, c], x, dt, rb, comb).tobytes() == want.tobytes()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", dlm.REGIMES)
def test_model_is_within_its_bound_of_the_exact_sum(sums, name, dt):
    n = _n()
    A, s, v = dlm.regime(name, dt, n)
    x = v * s
    rb, comb = dlm.shape(dt, n)
    model, _ = sums[name, dt]
    bound = dlm.bound_ulps(n, rb, comb)
    for c in range(0, n, 7):
        exact = dlm.exact_column(A[:, c], x)
        assert com.err_ulps(model[c], exact, dt) <= bound, (name, dt, c)


def test_regimes_hold_what_they_claim():
    n = _n()
    for dt in DTYPES:
        tiny = np.finfo(dt).tiny
        A, s, v = dlm.regime("C", dt, n)
        assert (A[:, n - 1] < tiny).all() and (A[:, n - 1] > 0).all()
        prod = (A[:, 0].astype(np.longdouble) * (v * s).astype(np.longdouble))
        assert (prod < tiny).any()                    # subnormal products
        A, _, _ = dlm.regime("D", dt, n)
        assert (A[:, 1] == 0).all() and 0.05 < (A == 0).mean() < 0.2
        A, _, _ = dlm.regime("B", dt, n)
        assert A.max() / A.min() > 2.0 ** 30
