"""GPU: the sparse (CSR) solve - st_csr_rowsum / st_csr_mfree_round / st_solve_csr.

1  every row sum against an exact sum, in ulps, at every row length that
   changes the path (1, L-1, L, L+1, every class limit and limit + 1, a full
   row, duplicates)
2  a row's result depends on its own entries and x only (bitwise)
3  v_cur and the whole st_state are st_mfree_round_*'s on the densified matrix
4  the stop test and the max at every boundary of k_csr_prep's partition
5  the whole solve against the dense matrix-free solve
6  the eigenvalue itself (Collatz-Wielandt bracket of numpy's spectral radius)
7  the solve equals its steps; 8 determinism; 9 options; 10 validation
"""
import ctypes
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import csr_cases as cc  # noqa: E402
import exact_sums as xs  # noqa: E402
import stats_vectors as sv  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from eigen_value_amd.similarity_transform import EigenValue  # noqa: E402

DEV = "cuda:0"
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
SEMS = [pytest.param(_lib.ST_SEM_SYCL, id="sycl"), pytest.param(_lib.ST_SEM_MAINPY, id="mainpy")]
BLOCK = 256
PREP_GRID = 2048                     # k_csr_prep's workgroup cap (st_csr_shape_desc)
MAX_ITR = 1000


def tdt(dt):
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def csr_of(solver, indptr, indices, data, n=None):
    return dev.CsrMatrix(up(np.asarray(indptr, np.int64)), up(np.asarray(indices, np.int32)),
                         up(data), n, solver=solver)


def limits():
    nnz_max, lanes = _lib.csr_class_limits()
    return [int(x) for x in nnz_max], [int(x) for x in lanes]


def lanes_of(k):
    nnz_max, lanes = limits()
    return lanes[int(np.searchsorted(np.array(nnz_max, np.int64), k, side="left"))]


def bound_ulps(k):
    """'levels + 1' for this order: a lane's ceil(k / L) fused multiply-adds,
    the log2(L) levels of the tree (L = 256: 6 in the wave, 3 serial adds),
    plus one; all terms positive, every value passes through that many
    roundings."""
    L = lanes_of(k)
    tree = int(math.log2(L)) if L <= 64 else 6 + 3
    return -(-k // L) + tree + 1


def test_shape_desc_matches_what_the_tests_assume():
    d = dict(kv.split("=") for kv in _lib.load().st_csr_shape_desc().decode().split())
    nnz_max, lanes = limits()
    assert d["lanes"] == ",".join(map(str, lanes))
    assert d["nnz_max"].split(",")[:3] == [str(x) for x in nnz_max[:3]]
    assert int(d["prep_grid"]) == PREP_GRID


# ---------------------------------------------------------------------------
# the step-level matrix: n = 300, every interesting row length
# ---------------------------------------------------------------------------
STEP_N = 300


@functools.lru_cache(maxsize=None)
def step_matrix(seed=11):
    nnz_max, lanes = limits()
    lens = [1, STEP_N]
    for L in lanes:
        lens += [L - 1, L, L + 1]
    for m in nnz_max[:-1]:
        lens += [m, m + 1]
    rng = np.random.default_rng(seed)
    lens += [int(x) for x in rng.integers(1, 200, size=STEP_N - len(lens))]
    lens = np.array(lens, dtype=np.int64)
    rng.shuffle(lens)
    cols, vals = [], []
    for k in lens:
        k = int(k)
        if k <= STEP_N:      # distinct, deliberately unsorted
            cols.append(rng.choice(STEP_N, k, replace=False))
        else:                # longer than the row is wide: duplicates, which add up
            cols.append(rng.integers(0, STEP_N, size=k))
        vals.append(1.0 - rng.random(k))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return indptr, np.concatenate(cols).astype(np.int32), np.concatenate(vals)


def padded_rows(indptr, vals):
    """[n, longest row] with zeros past each row's end (exact_rowsum's input)."""
    lens = np.diff(indptr)
    out = np.zeros((len(lens), int(lens.max())), dtype=vals.dtype)
    mask = np.arange(out.shape[1])[None, :] < lens[:, None]
    out[mask] = vals
    return out


@pytest.mark.parametrize("dt", DTYPES)
def test_rowsum_against_the_exact_sum(solver, dt):
    indptr, indices, data = step_matrix()
    data = data.astype(dt)
    m = csr_of(solver, indptr, indices, data, STEP_N)
    s = dev.csr_rowsum(m).cpu().numpy()
    err = np.abs(xs.err_ulps_of(s, xs.exact_rowsum(padded_rows(indptr, data)), dt))
    bound = np.array([bound_ulps(int(k)) for k in np.diff(indptr)])
    print("rowsum max |err| ulps per class:",
          {L: float(err[[lanes_of(int(k)) == L for k in np.diff(indptr)]].max())
           for L in limits()[1]})
    assert (err <= bound).all(), (err - bound).max()


def positive(n, dt, seed, lo=0.5, hi=2.0):
    rng = np.random.default_rng(seed)
    return (lo + (hi - lo) * rng.random(n)).astype(dt)


def run_round(m, s_prev, v_prev, k=1, eps=1e-3, sem=_lib.ST_SEM_SYCL, max_itr=MAX_ITR,
              state=None):
    """One st_csr_mfree_round: (s_next, v_cur, x, state bytes) as numpy."""
    t = tdt(s_prev.dtype)
    n = m.n
    s_next = torch.full((n,), -1.0, dtype=t, device=DEV)
    v_cur = torch.full((n,), -1.0, dtype=t, device=DEV)
    x = torch.full((n,), -1.0, dtype=t, device=DEV)
    state = dev.new_state(DEV) if state is None else state
    dev.csr_mfree_round(m, up(s_prev), s_next, up(v_prev), v_cur, x, state, eps=eps, k=k,
                        max_itr=max_itr, semantics=sem)
    return s_next.cpu().numpy(), v_cur.cpu().numpy(), x.cpu().numpy(), state.cpu().numpy()


@pytest.mark.parametrize("dt", DTYPES)
def test_round_sums_against_the_exact_quotient(solver, dt):
    """s_next[r] against the exact (sum of a x[col]) / x[r] with x the fp
    product the kernel defines: one more ulp for the division."""
    indptr, indices, data = step_matrix()
    data = data.astype(dt)
    m = csr_of(solver, indptr, indices, data, STEP_N)
    s_prev, v_prev = positive(STEP_N, dt, 1), positive(STEP_N, dt, 2)
    s_next, _, x, _ = run_round(m, s_prev, v_prev)
    assert np.array_equal(x, v_prev * s_prev)            # the product in dt, bit for bit
    wide = np.float64 if np.dtype(dt) == np.float32 else np.longdouble
    assert np.finfo(wide).nmant >= (52 if wide is np.float64 else 63)
    prod = padded_rows(indptr, data.astype(wide) * x.astype(wide)[indices])
    exact = prod.sum(axis=1) / x.astype(wide)
    err = np.abs(xs.err_ulps_of(s_next, exact, dt))
    bound = np.array([bound_ulps(int(k)) + 1 for k in np.diff(indptr)])
    print("round max |err| ulps:", float(err.max()), "largest bound", int(bound.max()))
    assert (err <= bound).all(), (err - bound).max()


# ---------------------------------------------------------------------------
# 2. row independence
# ---------------------------------------------------------------------------
def permuted(indptr, indices, data, perm, cols=None):
    """Rows perm[0], perm[1], ... of the matrix, each row's entries in their
    stored order; column c renamed cols[c]."""
    lens = np.diff(indptr)
    idx = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in perm])
    ci = indices[idx]
    return (np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.int64),
            (ci if cols is None else cols[ci]).astype(np.int32), data[idx])


@pytest.mark.parametrize("dt", DTYPES)
def test_permuting_rows_permutes_the_sums_bitwise(solver, dt):
    indptr, indices, data = step_matrix()
    data = data.astype(dt)
    n = STEP_N
    perm = np.random.default_rng(5).permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    a = csr_of(solver, indptr, indices, data, n)
    s0 = dev.csr_rowsum(a).cpu().numpy()
    # rows alone (K0 reads no x)
    b = csr_of(solver, *permuted(indptr, indices, data, perm), n)
    assert np.array_equal(dev.csr_rowsum(b).cpu().numpy(), s0[perm])
    # the round: P A P^T with x' = P x - the same operands in the same order
    s_prev, v_prev = positive(n, dt, 1), positive(n, dt, 2)
    s_next, v_cur, _, _ = run_round(a, s_prev, v_prev)
    c = csr_of(solver, *permuted(indptr, indices, data, perm, cols=inv), n)
    s_next_p, v_cur_p, _, _ = run_round(c, s_prev[perm], v_prev[perm])
    assert np.array_equal(s_next_p, s_next[perm])
    assert np.array_equal(v_cur_p, v_cur[perm])


@pytest.mark.parametrize("dt", DTYPES)
def test_appending_rows_of_other_classes_changes_no_bit(solver, dt):
    indptr, indices, data = step_matrix()
    data = data.astype(dt)
    n, extra = STEP_N, 47
    rng = np.random.default_rng(9)
    lens = np.array([200] * 40 + [2100] * 3 + [2] * 4)       # other classes, new columns too
    cols = [rng.integers(0, n + extra, size=k) for k in lens]
    indptr2 = np.concatenate([indptr, indptr[-1] + np.cumsum(lens)])
    indices2 = np.concatenate([indices] + cols).astype(np.int32)
    data2 = np.concatenate([data, (1.0 - rng.random(int(lens.sum()))).astype(dt)])
    a = csr_of(solver, indptr, indices, data, n)
    b = csr_of(solver, indptr2, indices2, data2, n + extra)
    assert np.array_equal(dev.csr_rowsum(b).cpu().numpy()[:n], dev.csr_rowsum(a).cpu().numpy())
    s_prev, v_prev = positive(n + extra, dt, 1), positive(n + extra, dt, 2)
    sa, _, _, _ = run_round(a, s_prev[:n], v_prev[:n])
    sb, _, _, _ = run_round(b, s_prev, v_prev)
    assert np.array_equal(sb[:n], sa)


def test_device_plan_is_the_host_plan(solver):
    indptr, indices, data = step_matrix()
    m = csr_of(solver, indptr, indices, data, STEP_N)
    order, first = m.plan()
    h_order, h_first, _ = _lib.csr_plan(indptr)
    assert np.array_equal(order, h_order) and np.array_equal(first, h_first)
    # several blocks of 256 rows and all four classes
    ip, ix, da = cc.make_csr(3000, 32, 7, cc.class_heavy())
    m = csr_of(solver, ip, ix, da, 3000)
    order, first = m.plan()
    h_order, h_first, used = _lib.csr_plan(ip)
    assert used == 4 and np.array_equal(order, h_order) and np.array_equal(first, h_first)


# ---------------------------------------------------------------------------
# 3. v_cur and st_state: st_mfree_round_* on the densified matrix
# ---------------------------------------------------------------------------
def dense_round(a, s_prev, v_prev, k, eps, sem, max_itr, state):
    t = tdt(a.dtype)
    n = a.shape[0]
    s_next = torch.full((n,), -1.0, dtype=t, device=DEV)
    v_cur = torch.full((n,), -1.0, dtype=t, device=DEV)
    dev.mfree_round(up(a), up(s_prev), s_next, up(v_prev), v_cur, state, eps=eps, k=k,
                    max_itr=max_itr, semantics=sem)
    return s_next.cpu().numpy(), v_cur.cpu().numpy(), state.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
@pytest.mark.parametrize("dt", DTYPES)
def test_state_and_v_parity_with_the_dense_round(solver, dt, n):
    ip, ix, da = cc.make_csr(n, min(n, 5), 3, {0: min(n, 70)})
    da = da.astype(dt)
    a = cc.densify(ip, ix, da)
    m = csr_of(solver, ip, ix, da, n)
    noisy = positive(n, dt, 1)
    flat = np.full(n, 1.5, dtype=dt)
    flat[n // 2] += dt(1e-4)
    v_prev = positive(n, dt, 2)
    for sem in (_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY):
        # (s_prev, k, max_itr): goes on / stops / exhausts
        for s_prev, k, max_itr in ((noisy, 3, MAX_ITR), (flat, 4, MAX_ITR), (noisy, 7, 7)):
            st_c, st_d = dev.new_state(DEV), dev.new_state(DEV)
            s_c, v_c, _, b_c = run_round(m, s_prev, v_prev, k, 1e-3, sem, max_itr, st_c)
            s_d, v_d, b_d = dense_round(a, s_prev, v_prev, k, 1e-3, sem, max_itr, st_d)
            assert b_c.tobytes() == b_d.tobytes(), (sem, k, dev.read_state(st_c),
                                                    dev.read_state(st_d))
            assert np.array_equal(v_c, v_d)
            st = _lib.st_state.from_buffer_copy(b_c.tobytes())
            assert (st.arrivals, st.max_bits, st.fail) == (0, 0, 0)      # scratch left zero
            stops = n < 2 or s_prev is flat
            assert st.stop == int(stops) and st.done == int(stops or k >= max_itr)
            np.testing.assert_allclose(s_c, s_d, rtol=64 * np.finfo(dt).eps)
            if st.done:      # launch k + 1 is a no-op in both: nothing is written
                s2, v2, x2, b2 = run_round(m, s_prev, v_prev, k + 1, 1e-3, sem, max_itr, st_c)
                _, vd2, bd2 = dense_round(a, s_prev, v_prev, k + 1, 1e-3, sem, max_itr, st_d)
                assert b2.tobytes() == bd2.tobytes() == b_c.tobytes()
                assert (s2 == -1).all() and (v2 == -1).all() and (x2 == -1).all()
                assert (vd2 == -1).all()


# ---------------------------------------------------------------------------
# 4. the stop test and the max at every boundary of k_csr_prep's partition
# ---------------------------------------------------------------------------
def diagonal_plus(solver, n, dt):
    """Two entries per row (the diagonal and the next column): any s_prev goes."""
    r = np.arange(n)
    indptr = 2 * np.arange(n + 1, dtype=np.int64)
    indices = np.stack([r, (r + 1) % n], axis=1).reshape(-1).astype(np.int32)
    return csr_of(solver, indptr, indices, np.ones(2 * n, dtype=dt), n)


def prep_positions(n, cyclic):
    """Lane, wave and workgroup boundaries of the vector pass - workgroup b of
    G = min(ceil(n / 256), 2048) takes the elements b * 256 + t + j * G * 256 -,
    the grid-stride seam where n has one, the ragged tail and the wrap."""
    g = min(-(-n // BLOCK), PREP_GRID)
    if g * BLOCK < n - BLOCK:     # a grid-stride seam: that, the ends, and little else
        p = {0, 63, 64, 255, 256, g * BLOCK - 1, g * BLOCK, g * BLOCK + 255, g * BLOCK + 256,
             n - 2, n - 1}
    else:
        p = {0, 1, 2, 62, 63, 64, 127, 128, 191, 192, 254, 255, 256, 257, 511, 512, 767, 768,
             n - 66, n - 65, n - 3, n - 2, n - 1}
    last = n if cyclic else n - 1
    return sorted(q for q in p if 0 <= q < last)


def expect_state(s, eps, sem, k, max_itr=MAX_ITR):
    cyclic = sem == _lib.ST_SEM_SYCL
    stop = not sv.failing_pairs(s, eps, cyclic)
    e = _lib.st_state()
    e.lambda_ = float(s[0])
    e.max = float(sv.find_max(s))
    e.stop = int(stop)
    e.round = k - 1
    if stop:
        e.iters, e.end, e.done = (k - 1 if cyclic else k), k, 1
    elif k >= max_itr:
        e.iters, e.end, e.done = max_itr, k, 1
    return bytes(e)


@pytest.mark.parametrize("n", [3 * BLOCK + 37, PREP_GRID * BLOCK + BLOCK + 37])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_stop_and_max_at_every_boundary_of_the_vector_pass(solver, dt, sem, n):
    cyclic = sem == _lib.ST_SEM_SYCL
    m = diagonal_plus(solver, n, dt)
    t = tdt(dt)
    k = 2
    v_prev = up(np.ones(n, dtype=dt))
    s_next = torch.empty(n, dtype=t, device=DEV)
    v_cur = torch.empty(n, dtype=t, device=DEV)
    x = torch.empty(n, dtype=t, device=DEV)
    cases = []
    for p in prep_positions(n, cyclic):
        cases += [(sv.one_fail(n, p, dt, sv.EPS, cyclic), sv.EPS),
                  (sv.all_pass(n, p, dt, sv.EPS, cyclic), sv.EPS),
                  (sv.exact_eps(n, p, dt, "fail", cyclic), sv.EXACT_EPS),
                  (sv.exact_eps(n, p, dt, "pass", cyclic), sv.EXACT_EPS),
                  (sv.max_at(n, p, dt, sv.EPS, decoys=True), sv.EPS),
                  (sv.max_at(n, p, dt, sv.EPS), sv.EPS),
                  (sv.nan_at(n, p, dt), sv.EPS)]
    # the wrap pair (n - 1, 0) alone: decisive under SYCL semantics, absent under main.py's
    wrap = sv.one_fail(n, n - 1, dt, sv.EPS, True)
    assert sv.failing_pairs(wrap, sv.EPS, True) == [n - 1]
    assert sv.failing_pairs(wrap, sv.EPS, False) == []
    cases.append((wrap, sv.EPS))
    states = torch.zeros((len(cases), 64), dtype=torch.uint8, device=DEV)
    for j, (s, eps) in enumerate(cases):
        dev.csr_mfree_round(m, up(s), s_next, v_prev, v_cur, x, states[j], eps=eps, k=k,
                            max_itr=MAX_ITR, semantics=sem)
    got = states.cpu().numpy()
    for j, (s, eps) in enumerate(cases):
        assert got[j].tobytes() == expect_state(s, eps, sem, k), (j, dev.read_state(states[j]))
    # the last case's v: v_prev * (s / m) with the published m
    s, _ = cases[-1]
    assert np.array_equal(v_cur.cpu().numpy(), np.ones(n, dt) * (s / sv.find_max(s)))
    stops = [_lib.st_state.from_buffer_copy(g.tobytes()).stop for g in got]
    assert 0 in stops and 1 in stops
    assert stops[-1] == int(not cyclic)


# ---------------------------------------------------------------------------
# 5 - 9. whole solves
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table_case(i):
    n, d, seed, heavy = cc.TABLE[i]
    return (n,) + cc.make_csr(n, d, seed, cc.class_heavy(n) if heavy else None)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("case", range(len(cc.TABLE)))
def test_solve_against_the_dense_solve_fp64(solver, case, sem):
    n, ip, ix, da = table_case(case)
    dense = up(cc.densify(ip, ix, da))
    m = csr_of(solver, ip, ix, da, n)
    lam, v, it, st = solver.solve_csr(m, semantics=sem)
    lam_d, v_d, it_d, st_d = solver.solve(dense, matrix_free=True, semantics=sem)
    assert (it, st["converged"], st["rounds"]) == (it_d, st_d["converged"], st_d["rounds"])
    assert st["converged"] == 1
    assert abs(lam - lam_d) <= 1e-10 * abs(lam_d)
    v, v_d = v.cpu().numpy(), v_d.cpu().numpy()
    assert (np.abs(v - v_d) <= 1e-10 * np.abs(v_d)).all()
    # the count the numpy model derives (the break index of the issue's table)
    kb, conv, _, _ = cc.model(cc.densify(ip, ix, da), 1e-3, sem == _lib.ST_SEM_SYCL)
    assert conv and it == cc.count_of(kb, conv, sem == _lib.ST_SEM_SYCL)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("case", range(len(cc.TABLE)))
def test_solve_fp32(solver, case, sem):
    """Equal iteration counts (the last round's max |ds| sits hundreds of fp32
    ulps from eps), and lambda and every v[i] within the summed bounds of the
    row sums over the rounds run, against the same iteration in fp64 on the
    same (fp32-valued) matrix.  Budget per round: the largest row bound of
    test_round_sums_against_the_exact_quotient (division included) plus one
    ulp for the v update's division and product; s = (A x) / x does not
    change when x is scaled, so what x carries from earlier rounds enters the
    numerator and the denominator alike and the rounds' budgets add.
    Observed (MI355X, one run, the same under both semantics), in relative
    ulps, lambda / largest v[i]: 0.84 / 2.25 (n = 64, budget 70), 1.53 / 3.26
    (n = 3000, budget 63), 0.66 / 2.41 (mixed classes, budget 369); the test
    prints its own figures."""
    n, ip, ix, da = table_case(case)
    da32 = da.astype(np.float32)
    m32 = csr_of(solver, ip, ix, da32, n)
    m64 = csr_of(solver, ip, ix, da32.astype(np.float64), n)
    lam, v, it, st = solver.solve_csr(m32, semantics=sem)
    lam_r, v_r, it_r, st_r = solver.solve_csr(m64, semantics=sem)
    lam_d, _, it_d, st_d = solver.solve(up(cc.densify(ip, ix, da32)), matrix_free=True,
                                        semantics=sem)
    assert it == it_r == it_d and st["converged"] == st_r["converged"] == st_d["converged"] == 1
    per_round = max(bound_ulps(int(k)) + 1 for k in np.diff(ip)) + 1
    budget = per_round * st["rounds"]
    ulp = float(np.finfo(np.float32).eps)            # of 1; relative spacing is at most this
    e_lam = abs(lam - lam_r) / (ulp * abs(lam_r))
    v, v_r = v.cpu().numpy().astype(np.float64), v_r.cpu().numpy()
    e_v = float((np.abs(v - v_r) / (ulp * np.abs(v_r))).max())
    print(f"fp32 vs fp64 case {case}: lambda {e_lam:.2f} v {e_v:.2f} relative ulps, "
          f"budget {budget} ({per_round} x {st['rounds']} rounds)")
    assert e_lam <= budget and e_v <= budget


@functools.lru_cache(maxsize=None)
def spectral_radius(case):
    n, ip, ix, da = table_case(case)
    a = cc.densify(ip, ix, da.astype(np.float32).astype(np.float64))
    return float(np.abs(np.linalg.eigvals(a)).max())


@pytest.mark.parametrize("case", [0, 2])
@pytest.mark.parametrize("dt", DTYPES)
def test_the_eigenvalue_is_bracketed_by_the_last_sums(solver, dt, case):
    """Collatz-Wielandt: min s <= rho <= max s for the row sums of any positive
    similarity transform; fp32-valued data for both dtypes, so one rho."""
    n, ip, ix, da = table_case(case)
    m = csr_of(solver, ip, ix, da.astype(np.float32).astype(dt), n)
    lam, v, it, st = solver.solve_csr(m, trace=True)
    sums = solver.last_round_sums()
    assert sums.shape == (st["rounds"], n) and sums.dtype == np.dtype(dt)
    s = sums[-1].astype(np.float64)
    rho = spectral_radius(case)
    slack = 4 * float(np.finfo(dt).eps) * rho
    assert s.min() - slack <= rho <= s.max() + slack, (s.min(), rho, s.max())
    assert lam == float(sums[-1][0])


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_solve_equals_its_steps(solver, dt, sem):
    n, ip, ix, da = table_case(2)
    m = csr_of(solver, ip, ix, da.astype(dt), n)
    lam, v, it, st = solver.solve_csr(m, trace=True, semantics=sem)
    sums = solver.last_round_sums()
    t = tdt(dt)
    s = [torch.empty(n, dtype=t, device=DEV) for _ in range(2)]
    vv = [torch.ones(n, dtype=t, device=DEV), torch.empty(n, dtype=t, device=DEV)]
    x = torch.empty(n, dtype=t, device=DEV)
    state = dev.new_state(DEV)
    dev.csr_rowsum(m, out=s[0])
    trace = []
    for k in range(MAX_ITR):
        trace.append(s[k & 1].cpu().numpy())
        dev.csr_mfree_round(m, s[k & 1], s[(k + 1) & 1], vv[k & 1], vv[(k + 1) & 1], x, state,
                            eps=1e-3, k=k + 1, max_itr=MAX_ITR, semantics=sem)
        if dev.read_state(state)["done"]:
            break
    fin = dev.read_state(state)
    assert fin["end"] == st["rounds"] == len(trace) and fin["iters"] == it
    assert np.array_equal(np.stack(trace), sums)
    assert fin["eigen_val"] == lam
    assert np.array_equal(vv[fin["end"] & 1].cpu().numpy(), v.cpu().numpy())


def test_determinism_and_the_three_input_forms(solver):
    sp = pytest.importorskip("scipy.sparse")
    n, ip, ix, da = table_case(2)
    m = csr_of(solver, ip, ix, da, n)
    a = solver.solve_csr(m, trace=True)
    sums_a = solver.last_round_sums()
    b = solver.solve_csr(m, trace=True)
    assert a[0] == b[0] and a[2] == b[2] and torch.equal(a[1], b[1])
    assert np.array_equal(sums_a, solver.last_round_sums())
    with EigenValue() as ev:
        r1 = ev.similarity_transform_csr(ip, ix, da)
        r2 = ev.similarity_transform_csr(sp.csr_matrix((da, ix, ip), shape=(n, n)))
        r3 = ev.similarity_transform_csr(
            torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)),
                                    torch.from_numpy(da), size=(n, n)))
    for r in (r1, r2, r3):
        assert r[0] == a[0] and r[3] == a[2] and r[0].dtype == np.float64
        assert np.array_equal(r[1], a[1].cpu().numpy())
    # a torch.sparse_csr tensor on the device goes straight into a CsrMatrix
    spt = torch.sparse_csr_tensor(up(ip), up(ix.astype(np.int64)), up(da), size=(n, n))
    c = solver.solve_csr(dev.CsrMatrix(spt, solver=solver))
    assert c[0] == a[0] and c[2] == a[2] and torch.equal(c[1], a[1])


@pytest.mark.parametrize("dt", DTYPES)
def test_options(solver, dt):
    n, ip, ix, da = table_case(1)
    da = da.astype(dt)
    m = csr_of(solver, ip, ix, da, n)
    dense = up(cc.densify(ip, ix, da))
    for sem in (_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY):
        lam, v, it, st = solver.solve_csr(m, max_itr=3, semantics=sem)
        lam_d, v_d, it_d, st_d = solver.solve(dense, matrix_free=True, max_itr=3, semantics=sem)
        assert st["converged"] == st_d["converged"] == 0
        assert (it, st["rounds"]) == (it_d, st_d["rounds"]) == (3, 3)
    lam, v, it, st = solver.solve_csr(m, time_kernels=True)
    ms = solver.last_round_times()
    assert len(ms) == st["rounds"] == st["fused_launches"] and (ms > 0).all()
    # n = 1
    one = csr_of(solver, [0, 1], [0], np.array([2.5], dtype=dt), 1)
    lam, v, it, st = solver.solve_csr(one)
    assert lam == 2.5 and v.cpu().numpy().tolist() == [1.0] and st["converged"] == 1
    lam_d, v_d, it_d, _ = solver.solve(up(np.array([[2.5]], dtype=dt)), matrix_free=True)
    assert (lam, it) == (lam_d, it_d)


# ---------------------------------------------------------------------------
# 10. device-side validation: no handle, so no gather on unvalidated indices
# ---------------------------------------------------------------------------
def test_the_check_kernel_names_the_entry(solver):
    n, ip, ix, da = table_case(0)
    for col in (n, -1, 2**31 - 1):
        bad = ix.copy()
        bad[8 * 5 + 3] = col
        with pytest.raises(_lib.EigenValueError,
                           match=rf"column index {col} of entry 43 \(row 5\)"):
            csr_of(solver, ip, bad, da, n)
    bad = ix.copy()
    bad[100], bad[17] = n + 3, n               # the FIRST offending entry is named
    with pytest.raises(_lib.EigenValueError, match=r"entry 17 \(row 2\)"):
        csr_of(solver, ip, bad, da, n)
    empty = ip.copy()
    empty[10] = empty[9]
    with pytest.raises(_lib.EigenValueError, match=r"row 9 is empty"):
        csr_of(solver, empty, ix, da, n)
    down = ip.copy()
    down[10] = down[9] - 1
    with pytest.raises(_lib.EigenValueError, match=r"decreases at row 9"):
        csr_of(solver, down, ix, da, n)
    first = ip.copy()
    first[0] = 1
    with pytest.raises(_lib.EigenValueError, match=r"row_ptr\[0\] must be 0"):
        csr_of(solver, first, ix, da, n)
    with pytest.raises(_lib.EigenValueError, match=r"row_ptr\[n\] must be nnz"):
        dev.CsrMatrix(up(ip), up(ix[:-1]), up(da[:-1]), n, solver=solver)
    # row_ptr is judged first: with it broken the column indices are not read
    bad = ix.copy()
    bad[0] = n
    with pytest.raises(_lib.EigenValueError, match=r"row 9 is empty"):
        csr_of(solver, empty, bad, da, n)
    # creation failed, so there is no handle to launch anything with
    try:
        m = csr_of(solver, ip, bad, da, n)
    except _lib.EigenValueError:
        m = None
    assert m is None
    # and the solver is still good for a valid matrix
    ok = csr_of(solver, ip, ix, da, n)
    assert solver.solve_csr(ok)[3]["converged"] == 1
    # dense entry points keep rejecting sparse input
    spt = torch.sparse_csr_tensor(up(ip), up(ix.astype(np.int64)), up(da), size=(n, n))
    with pytest.raises(Exception):
        solver.solve(spt)
    with pytest.raises(TypeError):
        solver.solve_csr(up(cc.densify(ip, ix, da)))
