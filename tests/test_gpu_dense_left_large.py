"""GPU: the dense left-vector kernels past n = 2049 - every value of the
rows-per-block table with and without 16-byte loads, more than one strip of
16-byte lanes, last blocks shorter than the rows in flight, and both sides of
the non-temporal threshold (dense_left_large.sizes, derived from the library's
own table; test_dense_left_model.py asserts what the list holds and that the
slabs tell every wrong order and every other table value apart).

The matrices are filled on the device and never drawn on the host; the order
and error tests overwrite 16 columns with a host-built slab
(dense_left_large.slab) and model those.  One device run per (dtype, size)
serves both (`run`).  Every column of every size is compared in the
exact-input test, which needs no model.

Nothing here sets the rows per block: the point is the library's own dispatch
at the real sizes."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import csr_order_model as com                      # noqa: E402
import dense_left_large as dll                     # noqa: E402
import dense_left_order_model as dlm               # noqa: E402
import test_gpu_dense_left as small                # noqa: E402
from eigen_value_amd import _lib                   # noqa: E402
from eigen_value_amd import device as dev          # noqa: E402
from test_gpu_dense_left import DEV, TD, dev_t, host, left_round   # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(dt, role) for dt in dll.DTYPES for role in dll.ROLES]    # (nothing loaded to list them)
CHUNK = 1024            # rows of one step of the fp64 reference sums


def device_matrix(n, dt, seed):
    """n x n entries in (0, 1] from a seeded device generator, no second
    buffer; the values are never compared against anything."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    A = torch.empty((n, n), dtype=TD[dt], device=DEV)
    return A.uniform_(0.0, 1.0, generator=g).neg_().add_(1.0)


def partials(scratch, n, nrb, idx=None):
    """The row-block partials a round left in its scratch, [nrb, n] (columns
    idx), on the host."""
    xe = -(-n // 64) * 64
    part = scratch[xe:xe + nrb * n].view(nrb, n)
    return host(part if idx is None else part[:, idx])


def serial(part):
    """The partials added as k_left_finish adds them."""
    num = part[0].copy()
    for j in range(1, part.shape[0]):
        num = num + part[j]
    return num


@functools.lru_cache(maxsize=None)
def run(dt, n):
    """(cols, {regime: what the device gave}) of one size: the slab's columns
    of launch 0, launch 1's s_next and partials on those columns, v_cur whole."""
    f = dll.facts(dt, n)
    cols = tuple(dll.model_columns(dt, n))
    idx = torch.tensor(cols, device=DEV)
    A = device_matrix(n, dt, seed=n)
    out = {}
    for name in dlm.REGIMES:
        S, s, v = dll.slab(name, dt, n, cols)
        A.index_copy_(1, idx, dev_t(S))
        got0 = host(dev.colsum(A)[idx])
        s_next, v_cur, _, scratch = left_round(A, s, v)
        out[name] = {"s0": got0, "s_next": s_next[list(cols)], "v_cur": v_cur,
                     "part": partials(scratch, n, f["nrb"], idx)}
        del scratch
    del A
    torch.cuda.empty_cache()
    return cols, out


# ---------------------------------------------------------------------------
# order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,role", CASES)
def test_order_matches_the_host_model(dt, role):
    """test_gpu_dense_left's order test at the large sizes, on the slab's
    columns, without the round on a transposed copy (it would double the
    memory)."""
    n = dll.sizes(dt)[role]
    cols, got = run(dt, n)
    f = dll.facts(dt, n)
    for name in dlm.REGIMES:
        S, s, v = dll.slab(name, dt, n, cols)
        x = v * s
        g = got[name]
        want0 = np.array([dlm.column(S[:, j], None, dt, f["rb"], f["combine"])
                          for j in range(len(cols))], dtype=dt)
        assert g["s0"].tobytes() == want0.tobytes(), (name, dt, n, "colsum", cols, g["s0"], want0)
        num = np.array([dlm.column(S[:, j], x, dt, f["rb"], f["combine"])
                        for j in range(len(cols))], dtype=dt)
        with np.errstate(all="ignore"):
            want = num / x[list(cols)]
            want_v = v * (s / s.max())
        assert g["s_next"].tobytes() == want.tobytes(), (name, dt, n, "s_next", cols, g["s_next"],
                                                         want)
        assert g["v_cur"].tobytes() == want_v.tobytes(), (name, dt, n, "v_cur")


# ---------------------------------------------------------------------------
# every column, exact inputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,role", CASES)
def test_exact_inputs_equal_integer_sums_in_every_column(dt, role):
    """Entries in {1, 2, 3, 4}, s in {1, 2}, v = 1: every partial sum of launch
    0 is an integer <= 4 n and of launch 1 <= 8 n < 2^24, exact in fp32 in any
    order, so every column must equal the integer sum - taken on the device in
    fp64, exact below 2^53 in any order.  A missed or doubled tile, a wrong
    strip decode or a wrong tail shows in the column it hits."""
    n = dll.sizes(dt)[role]
    assert 8 * n < 2 ** 24
    g = torch.Generator(device=DEV)
    g.manual_seed(100 + n)
    A = torch.randint(1, 5, (n, n), generator=g, device=DEV, dtype=TD[dt])
    rng = np.random.default_rng(200 + n)
    s = rng.integers(1, 3, size=n).astype(dt)
    assert s.min() == 1 and s.max() == 2
    ones = np.ones(n, dt)
    xd = dev_t(s).double()
    ref0 = torch.zeros(n, dtype=torch.float64, device=DEV)
    ref1 = torch.zeros(n, dtype=torch.float64, device=DEV)
    for r0 in range(0, n, CHUNK):
        rows = A[r0:r0 + CHUNK].double()
        ref0 += rows.sum(dim=0)
        ref1 += (rows * xd[r0:r0 + CHUNK, None]).sum(dim=0)
    del rows
    ref0, ref1 = host(ref0), host(ref1)
    assert ref0.min() >= n and ref1.max() <= 8 * n
    s0 = host(dev.colsum(A))
    bad = np.flatnonzero(s0.astype(np.float64) != ref0)
    assert bad.size == 0, (dt, n, "colsum", bad[:8], s0[bad[:8]], ref0[bad[:8]])
    s_next, v_cur, _, scratch = left_round(A, s, ones)
    num = s_next.astype(np.float64) * s.astype(np.float64)     # x = s: a division by 1 or 2
    bad = np.flatnonzero(num != ref1)
    assert bad.size == 0, (dt, n, "round", bad[:8], num[bad[:8]], ref1[bad[:8]])
    f = dll.facts(dt, n)
    added = serial(partials(scratch, n, f["nrb"]))
    assert added.astype(np.float64).tobytes() == ref1.tobytes(), (dt, n, "partials")
    assert v_cur.tobytes() == (s / np.dtype(dt).type(2)).tobytes(), (dt, n, "v_cur")
    del A, scratch
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# the same bits on every path
# ---------------------------------------------------------------------------
# one size of 16-byte lanes in every class of the table from the second on (a
# short last block and a partial last strip each), and the first non-temporal
# size of 16-byte lanes
PATH_ROLES = [r for r in dll.ROLES if r.startswith("short")] + ["nt_w"]


@pytest.mark.parametrize("dt,role", [(dt, r) for dt in dll.DTYPES for r in PATH_ROLES])
def test_element_wide_and_16_byte_loads_give_the_same_bits(dt, role):
    """The same matrix one element into a larger buffer: its rows are not
    16-byte aligned, so the launch takes the element-wide path, with other
    strips and another grid; colsum, s_next, v_cur and the state must keep
    every bit over all columns.  The padding is NaN and the results finite, so
    nothing outside the matrix is read by the tall blocks and the non-temporal
    loads either.

    Cached against non-temporal loads has no such pair: the kind of load is a
    function of n alone, and nothing but a setter could force the other one.
    That half is carried by the order and the exact-input tests on both sides
    of the threshold, in both lane widths."""
    n = dll.sizes(dt)[role]
    f = dll.facts(dt, n)
    assert f["w"] > 1 and (f["rb"] >= f["table"][1] or f["nt"])
    assert len({dll.facts(dt, dll.sizes(dt)[r])["rb"] for r in PATH_ROLES}) == dll.STEPS
    plain = device_matrix(n, dt, seed=300 + n)
    buf = torch.full((n * n + 2,), float("nan"), dtype=TD[dt], device=DEV)
    inside = buf[1:1 + n * n].view(n, n)
    inside.copy_(plain)
    assert plain.data_ptr() % 16 == 0 and inside.data_ptr() % 16 != 0
    rng = np.random.default_rng(400 + n)
    s = (0.5 + 1.5 * rng.random(n)).astype(dt)
    v = (0.5 + 1.5 * rng.random(n)).astype(dt)
    c_in, c_pl = host(dev.colsum(inside)), host(dev.colsum(plain))
    assert c_in.tobytes() == c_pl.tobytes(), (dt, n, np.flatnonzero(c_in != c_pl)[:8])
    got, gv, gs, _ = left_round(inside, s, v)
    want, wv, ws, _ = left_round(plain, s, v)
    assert got.tobytes() == want.tobytes(), (dt, n, np.flatnonzero(got != want)[:8])
    assert gv.tobytes() == wv.tobytes() and gs == ws, (dt, n)
    assert np.isfinite(c_in).all() and np.isfinite(got).all() and np.isfinite(gv).all()
    assert torch.isnan(buf[0]) and torch.isnan(buf[-1])
    del plain, buf, inside
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# error
# ---------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("dt,role", CASES)
def test_error_is_within_the_bound_of_the_tall_blocks(dt, role, capsys):
    """Every modelled column of the order test - launch 0, and launch 1's
    numerator read back from the partials - against the exact rational sum:
    within dense_left_order_model.bound_ulps of this n's rows per block."""
    n = dll.sizes(dt)[role]
    cols, got = run(dt, n)
    f = dll.facts(dt, n)
    bound = dlm.bound_ulps(n, f["rb"], f["combine"])
    worst = 0.0
    for name in dlm.REGIMES:
        S, s, v = dll.slab(name, dt, n, cols)
        x = v * s
        g = got[name]
        num = serial(g["part"])
        with np.errstate(all="ignore"):
            assert (num / x[list(cols)]).tobytes() == g["s_next"].tobytes(), (dt, n, name)
        for j, c in enumerate(cols):
            e0 = com.err_ulps(g["s0"][j], dlm.exact_column(S[:, j]), dt)
            e1 = com.err_ulps(num[j], dlm.exact_column(S[:, j], x), dt)
            assert e0 <= bound and e1 <= bound, (dt, n, name, c, e0, e1, bound)
            worst = max(worst, e0, e1)
    WORST[dt] = max(WORST.get(dt, 0.0), worst)
    with capsys.disabled():
        print(f"\n[dense left large] {dt} n = {n} (RB = {f['rb']}): largest error {worst:.3f} "
              f"ulps, bound {bound}; {dt} so far {WORST[dt]:.3f}")


# ---------------------------------------------------------------------------
# whole solve
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


# the first size of the table's third class and the first non-temporal size of
# 16-byte lanes, per dtype, the semantics alternating
SOLVES = [("float32", "on2", _lib.ST_SEM_SYCL), ("float32", "nt_w", _lib.ST_SEM_MAINPY),
          ("float64", "on2", _lib.ST_SEM_MAINPY), ("float64", "nt_w", _lib.ST_SEM_SYCL)]


@pytest.mark.parametrize("dt,role,sem", SOLVES)
def test_whole_solve_against_the_solve_of_a_transposed_copy(solver, dt, role, sem):
    """test_gpu_dense_left's whole-solve test itself - its assertions, its
    tolerances, its fp32 stop parity - on dev.generate("random") at these
    sizes."""
    n = dll.sizes(dt)[role]
    f = dll.facts(dt, n)
    assert f["w"] > 1 and (f["nt"] if role == "nt_w" else f["rb"] == f["table"][2])
    small.test_whole_solve_against_the_solve_of_a_transposed_copy(solver, n, "random", dt, sem)
    torch.cuda.empty_cache()
