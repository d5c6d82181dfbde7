"""CPU: the host model of the dense left-vector order (dense_left_order_model)
and the power of its inputs - every wrong order tried must show in at least
three columns of every value regime and dtype, or a device test that compares
bytes with the model would prove nothing.  No GPU needed.

The second half does the same for the large sizes of
test_gpu_dense_left_large.py (dense_left_large): what the size list holds, and
that the slabs tell every wrong order and every other value of the
rows-per-block table apart at every one of those sizes."""
import numpy as np
import pytest

import csr_order_model as com
import dense_left_large as dll
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


# ---------------------------------------------------------------------------
# the large sizes (test_gpu_dense_left_large.py)
# ---------------------------------------------------------------------------
LARGE = [(dt, role) for dt in dll.DTYPES for role in dll.ROLES]   # (nothing loaded to list them)


def test_large_sizes_hold_what_the_kernels_branch_on():
    for dt in DTYPES:
        S = sorted(dll.sizes(dt).values())
        assert len(set(S)) == len(dll.ROLES)              # no role repeats another's size
        F = {n: dll.facts(dt, n) for n in S}
        table, lanes = F[S[0]]["table"], F[S[0]]["lanes"]
        assert lanes > 1 and len(table) >= 2 and table == sorted(table)
        # every value of the table, with 16-byte lanes and element-wide
        for rb in table:
            assert {F[n]["w"] for n in S if F[n]["rb"] == rb} == {1, lanes}, (dt, rb)
        # one below and one on every step
        for step in F[S[0]]["from"][1:]:
            assert step - 1 in S and step in S and F[step - 1]["rb"] < F[step]["rb"], (dt, step)
        # both sides of the non-temporal threshold in both lane widths, adjacent to it
        n0 = dll.first_nt(dt)
        edge = dll.nt_edge(dt)
        assert set(edge) == {(nt, w) for nt in (False, True) for w in (1, lanes)}
        for (nt, w), n in edge.items():
            assert n in S and (F[n]["nt"], F[n]["w"]) == (nt, w), (dt, n)
            assert n0 - lanes <= n < n0 + lanes
        assert n0 - 1 in S and n0 in S
        # more than one strip of 16-byte lanes in every class from the second on
        for rb in table[1:]:
            assert any(F[n]["rb"] == rb and F[n]["w"] > 1 and F[n]["nstrips"] >= 2 for n in S)
        # a last block shorter than the rows in flight, with a partial last strip
        for rb in table[1:]:
            assert any(F[n]["rb"] == rb and F[n]["w"] > 1 and F[n]["last"] < F[n]["in_flight"]
                       and n % F[n]["strip"] for n in S), (dt, rb)
        # the finish's 16-wide loop: more than two trips, and whole trips without a remainder
        assert any(F[n]["nrb"] > 33 for n in S)
        assert any(F[n]["nrb"] > 33 and (F[n]["nrb"] - 1) % 16 == 0 for n in S)
        assert all(8 * n < 2 ** 24 for n in S)            # the exact-input test's claim


def test_large_columns_hold_the_boundaries():
    for dt, role in LARGE:
        n = dll.sizes(dt)[role]
        f = dll.facts(dt, n)
        cols = dll.model_columns(dt, n)
        w, strip = f["w"], f["strip"]
        assert len(cols) == dll.COLUMNS == len(set(cols)) and cols == sorted(cols)
        assert {0, w - 1, w, strip - 1, strip, strip + 1, (f["nstrips"] - 1) * strip, n - w - 1,
                n - w, n - 1} <= set(cols), (dt, n)
        assert dll.model_columns(dt, n) == cols


def test_large_slabs_hold_what_they_claim():
    for dt in DTYPES:
        n = dll.sizes(dt)["below1"]
        cols = tuple(dll.model_columns(dt, n))
        tiny = np.finfo(dt).tiny
        S, s, v = dll.slab("C", dt, n, cols)
        assert S.shape == (n, len(cols)) and S.dtype == np.dtype(dt)
        assert (S[:, dll.SUBNORMAL_AT] < tiny).all() and (S[:, dll.SUBNORMAL_AT] > 0).all()
        prod = S[:, 0].astype(np.longdouble) * (v * s).astype(np.longdouble)
        assert (prod < tiny).any()                    # subnormal products
        S, _, _ = dll.slab("D", dt, n, cols)
        assert (S[:, dll.ZERO_AT] == 0).all() and 0.05 < (S[:, :dll.PINNED] == 0).mean() < 0.2
        S, _, _ = dll.slab("B", dt, n, cols)
        assert S.max() / S.min() > 2.0 ** 30
        S, s, v = dll.slab("A", dt, n, cols)
        assert S.min() > 0 and S.max() <= 1 and 0.5 <= min(s.min(), v.min())
        # a function of (name, dtype, n, number of columns, draw): drawn again, the same bytes
        again = dll.slab("A", dt, n, tuple(reversed(cols)))
        assert all(a.tobytes() == b.tobytes() for a, b in zip((S, s, v), again))
        draw = dll.golden()[dt][str(n)]["draw"]["A"]
        assert S.tobytes() != dll.slab("A", dt, n, cols, draw + 1)[0].tobytes()
        S, _, _ = dll.slab("B", dt, n, cols)
        assert (S[n - 1] >= S.max() / 2).all()        # the last row at the top of the range


@pytest.mark.parametrize("dt,role", LARGE)
def test_large_slabs_tell_wrong_orders_and_other_table_values_apart(dt, role):
    """For every regime, launch 1 and launch 0: each wrong order of dlm.WRONG,
    and the model run with each OTHER value of the rows-per-block table - what
    an edit of the table would compute - differs from the model with the
    library's value in at least MIN_COLUMNS of the slab's 16 columns
    (dense_left_large.unseen).  One column does not always separate two table
    values, hence a claim over the set.

    The model's own bytes on the first columns are pinned in
    tests/golden/dense_left_large_order.json: an edit of the table fails here,
    without a GPU, at exactly the sizes whose order it changes."""
    assert dll.MIN_COLUMNS == MIN_COLUMNS and len(dlm.WRONG) == 7
    n = dll.sizes(dt)[role]
    f = dll.facts(dt, n)
    assert (f["rb"], f["combine"]) == dlm.shape(dt, n) and len(set(f["table"])) == 4
    value = {name: {} for name in dlm.REGIMES}
    unseen = {name: dll.unseen(name, dt, n, None, value[name]) for name in dlm.REGIMES}
    assert dll.digest(dt, n, value) == dll.golden()[dt][str(n)]["order"], \
        (dt, n, f["rb"], "the expected bytes of this size changed")
    assert not any(unseen.values()), (dt, n, unseen)
