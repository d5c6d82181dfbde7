"""CPU: the host model of the right side's order of the dense pair kernels
(dense_pair_order_model) and the power of its inputs - every wrong order tried
must show in at least one modelled row of every value regime and dtype, at a
size the GPU test runs, or a device test that compares bytes with the model
would prove nothing.  No GPU needed."""
import numpy as np
import pytest

import csr_order_model as com
import dense_left_order_model as dlm
import dense_pair_order_model as dpm

DTYPES = ("float32", "float64")


def _sizes(dt):
    """The sizes of test_gpu_dense_pair.sizes that separate the orders: one
    lane, a partial wave, all four waves of one strip, two strips, four."""
    _, S, _ = dpm.shape(dt, 1)
    return [1, 3, 65, S, S + 1, 3 * S + 5]


# which sizes can tell a wrong order from the model at all (the others give
# the same bytes by construction: one strip, fewer than four waves or strips)
def _tells(kind, dt):
    _, S, _ = dpm.shape(dt, 1)
    return {"lane_chain": [S + 1, 3 * S + 5], "strips_tree": [3 * S + 5],
            "mul_add": [65, S], "half_strip": [S, S + 1], "waves_tree": [S, S + 1],
            "drop_last": [1, 3, 65, S + 1]}[kind]


def _rows_of(n, rb):
    r = dpm.model_rows(n, rb)
    return r if len(r) <= 6 else [r[0], r[1], r[len(r) // 2], r[-2], r[-1]]


def test_shape_is_sane_and_a_function_of_dtype_and_n():
    for dt in DTYPES:
        for n in (1, 2, 31, 2047, 2048, 4096, 16384, 131072):
            rb, S, comb = dpm.shape(dt, n)
            assert (rb, S, comb) == dpm.shape(dt, n)
            assert rb == dlm.shape(dt, n)[0] and comb == 0
            assert S == 256 * dpm.lane_cols(dt) == (1024 if dt == "float32" else 512)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", dlm.REGIMES)
@pytest.mark.parametrize("kind", dpm.WRONG)
def test_every_wrong_order_shows_in_a_modelled_row(kind, name, dt):
    """Launch 1 (x = v * s) or launch 0 (x == 1; multiply-then-add is the same
    arithmetic there): some modelled row of some size differs in its bytes."""
    for n in _tells(kind, dt):
        rb, S, _ = dpm.shape(dt, n)
        A, s, v = dlm.regime(name, dt, n)
        for x in ((v * s), None):
            if x is None and kind == "mul_add":
                continue
            for r in dpm.model_rows(n, rb):           # (returns at the first that differs)
                good = dpm.row(A[r], x, dt, S)
                bad = dpm.wrong_row(kind, A[r], x, dt, S)
                if np.asarray(good).tobytes() != np.asarray(bad).tobytes():
                    return
    pytest.fail(f"{kind} never shows in regime {name}, {dt}")


@pytest.mark.parametrize("name", dlm.REGIMES)
def test_the_vectorised_fp32_path_is_the_exact_chain(name):
    """rows() runs fp32 through dense_order_model.fma32, row() through the
    integer chain: the same bytes, launch 0 and launch 1."""
    dt = "float32"
    for n in (5, 65, 1025, 2051):
        rb, S, _ = dpm.shape(dt, n)
        A, s, v = dlm.regime(name, dt, n)
        which = _rows_of(n, rb)
        for x in (v * s, None):
            want = np.array([dpm.row(A[r], x, dt, S) for r in which], dtype=dt)
            assert dpm.rows(A, x, dt, which).tobytes() == want.tobytes(), (name, n)


@pytest.mark.parametrize("dt", DTYPES)
def test_model_agrees_with_plain_arithmetic(dt):
    """fma by fma through round_fraction, the tree and the serial adds by numpy:
    the model's fast path is the documented order."""
    _, S, _ = dpm.shape(dt, 1)
    n = S + 7
    wc = dpm.lane_cols(dt)
    A, s, v = dlm.regime("A", dt, n)
    x = v * s
    t = np.dtype(dt).type
    for r in (0, n - 1):
        vals = []
        for lo in range(0, n, S):
            lanes = np.zeros(256, dtype=dt)
            for l in range(256):
                acc = t(0)
                for c in range(lo + l * wc, min(lo + l * wc + wc, lo + S, n)):
                    acc = com.fma(A[r, c], x[c], acc, dt)
                lanes[l] = acc
            w = [com.tree(lanes[i:i + 64]) for i in range(0, 256, 64)]
            vals.append(t(t(t(w[0] + w[1]) + w[2]) + w[3]))
        want = vals[0]
        for b in vals[1:]:
            want = t(want + b)
        assert np.asarray(dpm.row(A[r], x, dt, S)).tobytes() == np.asarray(want).tobytes()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", dlm.REGIMES)
def test_model_is_within_its_bound_of_the_exact_sum(name, dt):
    for n in (65, 133, dpm.shape(dt, 1)[1] + 1):
        rb, S, _ = dpm.shape(dt, n)
        A, s, v = dlm.regime(name, dt, n)
        x = v * s
        bound = dpm.bound_ulps(n, S)
        assert bound == dpm.lane_cols(dt) + 6 + 3 + (-(-n // S) - 1) + 1
        which = list(range(0, n, 9))
        for xx in (x, None):
            got = dpm.rows(A, xx, dt, which)
            for r, g in zip(which, got):
                exact = dpm.exact_row(A[r], xx)
                assert com.err_ulps(g, exact, dt) <= bound, (name, dt, n, r)


def test_model_rows_hold_the_boundaries():
    for n, rb in ((65, 32), (133, 32), (1025, 32), (2051, 64)):
        rows = dpm.model_rows(n, rb)
        assert rows == sorted(set(rows)) and rows == dpm.model_rows(n, rb)
        if n <= 80:
            assert rows == list(range(n))
            continue
        last0 = (n - 1) // rb * rb
        assert {0, rb - 1, rb, last0, n - 1} <= set(rows)
        assert (n - last0) % 8 == 0 or last0 + (n - last0) // 8 * 8 in rows   # the tail's first row
