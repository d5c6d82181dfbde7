"""GPU: the CSR solve on A + sum_j u_j w_j^T and on matrices with empty rows -
st_csr_terms_rowsum / st_csr_terms_round / st_solve_csr_terms / pagerank.

1  the dot alone against an exact sum, in ulps, and bitwise: run to run,
   under another matrix, K = 3 against each term alone
2  a round with terms (all four row classes, empty rows at the plan's edges
   and at a workgroup boundary of class 0) against the exact quotient
3  a zero term changes no bit
4  the stop test and the max at every boundary of the new vector pass
5  the whole solve against the dense solve of the densified operator
6  left=True with terms against host-transposed arrays with swapped terms
7  PageRank on a reducible, periodic graph with dangling nodes
8  errors on the device path
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import csr_cases as cc  # noqa: E402
import csr_terms_cases as tc  # noqa: E402
import exact_sums as xs  # noqa: E402
import stats_vectors as sv  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from test_gpu_csr import (BLOCK, DEV, DTYPES, MAX_ITR, PREP_GRID, SEMS, bound_ulps,  # noqa: E402
                          csr_of, diagonal_plus, expect_state, limits, padded_rows, positive,
                          prep_positions, run_round, step_matrix, table_case, tdt, up)


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def wide_of(dt):
    wide = np.float64 if np.dtype(dt) == np.float32 else np.longdouble
    assert np.finfo(wide).nmant >= (52 if wide is np.float64 else 63)
    return wide


def terms_of(solver, m, u, w):
    return dev.CsrTerms(m, [up(x) for x in u], [up(x) for x in w], solver=solver)


def terms_round(m, t, s_prev, v_prev, k=1, eps=1e-3, sem=_lib.ST_SEM_SYCL, max_itr=MAX_ITR,
                state=None):
    """One st_csr_terms_round: (s_next, v_cur, x, dots, state bytes) as numpy."""
    td = tdt(s_prev.dtype)
    s_next = torch.full((m.n,), -1.0, dtype=td, device=DEV)
    v_cur = torch.full((m.n,), -1.0, dtype=td, device=DEV)
    scratch = t.scratch()
    state = dev.new_state(DEV) if state is None else state
    dev.csr_terms_round(m, t, up(s_prev), s_next, up(v_prev), v_cur, scratch, state, eps=eps,
                        k=k, max_itr=max_itr, semantics=sem)
    return (s_next.cpu().numpy(), v_cur.cpu().numpy(), t.x(scratch).cpu().numpy(),
            t.dots(scratch).cpu().numpy(), state.cpu().numpy())


def test_shape_desc_matches_what_the_tests_assume():
    d = _lib.csr_terms_shape()
    assert d["dot_grid"] == PREP_GRID == tc.DOT_GRID and d["lanes"] == BLOCK == tc.BLOCK
    assert d["terms_max"] == 4


# ---------------------------------------------------------------------------
# 1. the dot alone
# ---------------------------------------------------------------------------
DOT_N = [1, 63, 64, 65, 255, 256, 257, 3 * 256 + 37, PREP_GRID * 256 - 1,
         PREP_GRID * 256 + 256 + 37]


def diagonal_only(solver, n, dt):
    return csr_of(solver, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32),
                  np.full(n, 2.0, dtype=dt), n)


@pytest.mark.parametrize("n", DOT_N)
@pytest.mark.parametrize("dt", DTYPES)
def test_the_dot_against_the_exact_sum_and_bitwise(solver, dt, n):
    """dots[j] = w_j . x through the step-level call, against the sum of the
    exact products of the stored w and the stored x (x = v_prev * s_prev in dt,
    as the kernel defines it), in ulps of dt at the exact sum.

    The bound is 'levels + 1' for the order st_csr_terms.h fixes
    (csr_terms_cases.dot_depth): every element passes through its lane's
    ceil(n / (256 G)) fused multiply-adds, the 6 levels of the wave tree and
    the 3 serial adds of the wave sums, then through the combine's ceil(G /
    256) adds, 6 levels and 3 adds, G = min(ceil(n / 256), 2048); all terms are
    positive, so no partial sum exceeds the total and every rounding errs by
    at most half an ulp of the total; plus one.  The same for w . 1 (launch
    0).  Observed maximum on MI355X over all the sizes (one run; also in
    DESIGN.md, "Low-rank terms and empty rows"): 1.52 ulps in fp32, 1.29 in
    fp64, against bounds of 21 to 29; the test prints its own."""
    wide = wide_of(dt)
    a, b = diagonal_plus(solver, n, dt), diagonal_only(solver, n, dt)
    rng = np.random.default_rng(n)
    w = (0.5 + rng.random((3, n))).astype(dt)
    zero = np.zeros((3, n), dtype=dt)
    s_prev, v_prev = positive(n, dt, 1), positive(n, dt, 2)
    t3 = terms_of(solver, a, zero, w)
    _, _, x, d3, _ = terms_round(a, t3, s_prev, v_prev)
    assert np.array_equal(x, v_prev * s_prev)
    bound = tc.dot_depth(n) + 1
    worst = 0.0
    for j in range(3):
        exact = (w[j].astype(wide) * x.astype(wide)).sum()
        err = abs(float(xs.err_ulps_of(d3[j:j + 1], np.array([exact]), dt)[0]))
        worst = max(worst, err)
        assert err <= bound, (j, err, bound)
    # launch 0: w . 1 in the same order
    scratch = t3.scratch()
    dev.csr_terms_rowsum(a, t3, scratch)
    d0 = t3.dots(scratch).cpu().numpy()
    for j in range(3):
        exact = w[j].astype(wide).sum()
        err = abs(float(xs.err_ulps_of(d0[j:j + 1], np.array([exact]), dt)[0]))
        worst = max(worst, err)
        assert err <= bound, (j, err, bound)
    print(f"dot n = {n} {np.dtype(dt).name}: max |err| {worst:.2f} ulps, bound {bound}")
    # run to run
    _, _, _, again, _ = terms_round(a, t3, s_prev, v_prev)
    assert again.tobytes() == d3.tobytes()
    # another matrix of the same n
    tb = terms_of(solver, b, zero, w)
    _, _, _, other, _ = terms_round(b, tb, s_prev, v_prev)
    assert other.tobytes() == d3.tobytes()
    # K = 3 against each term alone
    for j in range(3):
        t1 = terms_of(solver, a, zero[j:j + 1], w[j:j + 1])
        _, _, _, alone, _ = terms_round(a, t1, s_prev, v_prev)
        assert alone.tobytes() == d3[j:j + 1].tobytes(), j
        t1.close()
    t3.close()
    tb.close()


# ---------------------------------------------------------------------------
# 2. a round with terms
# ---------------------------------------------------------------------------
ROUND_N = 1300


@functools.lru_cache(maxsize=None)
def round_matrix():
    """step_matrix's rows (every row length that changes the path, all four
    classes), then 1000 short rows, so that class 0 fills more than one
    workgroup (8 * 256 / 4 = 512 rows); emptied: the plan's first row, class
    0's last row, and class 0's rows at the plan positions 511 and 512, the
    two sides of its first workgroup boundary."""
    ip, ix, da = step_matrix()
    n0, n = len(ip) - 1, ROUND_N
    rng = np.random.default_rng(21)
    lens = rng.integers(1, 4, size=n - n0)
    cols = np.concatenate([rng.choice(n, int(k), replace=False) for k in lens])
    ip = np.concatenate([ip, ip[-1] + np.cumsum(lens)]).astype(np.int64)
    ix = np.concatenate([ix, cols]).astype(np.int32)
    da = np.concatenate([da, 1.0 - rng.random(int(lens.sum()))])
    nnz_max, _ = limits()
    cls0 = np.flatnonzero(np.diff(ip) <= nnz_max[0])
    assert len(cls0) > 520
    gone = sorted({int(cls0[0]), int(cls0[511]), int(cls0[512]), int(cls0[-1])})
    return tc.empty_rows(ip, ix, da, gone) + (gone,)


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("dt", DTYPES)
def test_round_with_terms_against_the_exact_quotient(solver, dt, K):
    """s_next[r] against the exact (sum of a x[col] + sum_j u_j[r] d_j) / x[r]
    with x and d_j the stored values the kernels define: the row's own bound
    (test_gpu_csr.bound_ulps), one ulp for each of the K fused multiply-adds
    and one for the division."""
    ip, ix, da, gone = round_matrix()
    da = da.astype(dt)
    n = ROUND_N
    m = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=True)
    assert (m.empty_rows, m.first_empty) == (len(gone), gone[0])
    order, first = m.plan()
    assert order[0] == gone[0] and order[first[1] - 1] == gone[-1]
    assert order[511] == gone[1] and order[512] == gone[2] and (first[1:] > first[:-1]).all()
    u, w = tc.term_vectors(n, K, 4, dt)
    t = terms_of(solver, m, u, w)
    s_prev, v_prev = positive(n, dt, 1), positive(n, dt, 2)
    s_next, v_cur, x, d, _ = terms_round(m, t, s_prev, v_prev)
    assert np.array_equal(x, v_prev * s_prev)
    wide = wide_of(dt)
    prod = padded_rows(ip, da.astype(wide) * x.astype(wide)[ix])
    tot = prod.sum(axis=1)
    for j in range(K):
        tot = tot + u[j].astype(wide) * d[j].astype(wide)
    err = np.abs(xs.err_ulps_of(s_next, tot / x.astype(wide), dt))
    bound = np.array([bound_ulps(int(k)) + K + 1 for k in np.diff(ip)])
    print(f"terms round K = {K} {np.dtype(dt).name}: max |err| {float(err.max()):.2f} ulps, "
          f"empty rows {err[gone].max():.2f}, largest bound {int(bound.max())}")
    assert (err <= bound).all(), (err - bound).max()
    assert (s_next[gone] > 0).all()
    m_prev = sv.find_max(s_prev)
    assert np.array_equal(v_cur, v_prev * (s_prev / m_prev))
    # launch 0 the same way
    scratch = t.scratch()
    s0 = dev.csr_terms_rowsum(m, t, scratch).cpu().numpy()
    d0 = t.dots(scratch).cpu().numpy()
    tot = padded_rows(ip, da.astype(wide)).sum(axis=1)
    for j in range(K):
        tot = tot + u[j].astype(wide) * d0[j].astype(wide)
    err = np.abs(xs.err_ulps_of(s0, tot, dt))
    assert (err <= bound - 1).all(), (err - bound).max()
    # without terms an empty row sums to 0 and the round is refused
    assert (dev.csr_rowsum(m).cpu().numpy()[gone] == 0).all()
    t.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_permuting_rows_and_u_permutes_the_sums_bitwise(solver, dt):
    """Rows of A together with the entries of u_j: a row's result depends on
    its own entries, its own u and the dots only.  The columns stay, so x is a
    constant vector (s_prev = 1.5, v_prev = 1): the gathers, the dots and the
    divisor do not change under the permutation."""
    ip, ix, da, gone = round_matrix()
    da = da.astype(dt)
    n = ROUND_N
    perm = np.random.default_rng(5).permutation(n)
    lens = np.diff(ip)
    idx = np.concatenate([np.arange(ip[r], ip[r + 1]) for r in perm]).astype(np.int64)
    ipp = np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.int64)
    u, w = tc.term_vectors(n, 2, 4, dt)
    a = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=True)
    b = dev.CsrMatrix(up(ipp), up(ix[idx]), up(da[idx]), n, solver=solver,
                      allow_empty_rows=True)
    ta, tb = terms_of(solver, a, u, w), terms_of(solver, b, u[:, perm], w)
    s0a = dev.csr_terms_rowsum(a, ta, ta.scratch()).cpu().numpy()
    s0b = dev.csr_terms_rowsum(b, tb, tb.scratch()).cpu().numpy()
    assert np.array_equal(s0b, s0a[perm])
    s_prev, v_prev = np.full(n, 1.5, dtype=dt), np.ones(n, dtype=dt)
    sa, va, _, da_, _ = terms_round(a, ta, s_prev, v_prev)
    sb, vb, _, db_, _ = terms_round(b, tb, s_prev, v_prev)
    assert da_.tobytes() == db_.tobytes()
    assert np.array_equal(sb, sa[perm]) and np.array_equal(vb, va[perm])
    ta.close()
    tb.close()


# ---------------------------------------------------------------------------
# 3. a zero term changes no bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("case", range(len(cc.TABLE)))
def test_a_zero_term_changes_no_bit(solver, case, sem, K):
    n, ip, ix, da = table_case(case)
    m = csr_of(solver, ip, ix, da, n)
    w = (0.5 + np.random.default_rng(K).random((K, n)))
    t = terms_of(solver, m, np.zeros((K, n)), w)
    lam, v, it, st = solver.solve_csr(m, trace=True, semantics=sem)
    sums = solver.last_round_sums()
    lam_t, v_t, it_t, st_t = solver.solve_csr(m, t, trace=True, semantics=sem)
    sums_t = solver.last_round_sums()
    assert (lam_t, it_t, st_t["rounds"], st_t["converged"]) == (lam, it, st["rounds"],
                                                                st["converged"])
    assert torch.equal(v_t, v) and np.array_equal(sums_t, sums)
    # the 64-byte state, vectors and sums of a round, step by step
    s_prev, v_prev = positive(n, np.float64, 1), positive(n, np.float64, 2)
    for k, max_itr in ((3, MAX_ITR), (7, 7)):
        s1, v1, x1, b1 = run_round(m, s_prev, v_prev, k, 1e-3, sem, max_itr)
        s2, v2, x2, _, b2 = terms_round(m, t, s_prev, v_prev, k, 1e-3, sem, max_itr)
        assert b1.tobytes() == b2.tobytes()
        assert np.array_equal(s1, s2) and np.array_equal(v1, v2) and np.array_equal(x1, x2)
    t.close()


# ---------------------------------------------------------------------------
# 4. the stop test and the max at every boundary of the new vector pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3 * BLOCK + 37, PREP_GRID * BLOCK + BLOCK + 37])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_stop_and_max_at_every_boundary_of_the_vector_pass_with_terms(solver, dt, sem, n):
    """test_gpu_csr's deciding-pair sweep through k_csr_prep<T, CsrDots<T>>."""
    cyclic = sem == _lib.ST_SEM_SYCL
    m = diagonal_plus(solver, n, dt)
    t = terms_of(solver, m, np.zeros((1, n), dtype=dt),
                 (0.5 + np.random.default_rng(3).random((1, n))).astype(dt))
    td = tdt(dt)
    k = 2
    v_prev = up(np.ones(n, dtype=dt))
    s_next = torch.empty(n, dtype=td, device=DEV)
    v_cur = torch.empty(n, dtype=td, device=DEV)
    scratch = t.scratch()
    cases = []
    for p in prep_positions(n, cyclic):
        cases += [(sv.one_fail(n, p, dt, sv.EPS, cyclic), sv.EPS),
                  (sv.all_pass(n, p, dt, sv.EPS, cyclic), sv.EPS),
                  (sv.exact_eps(n, p, dt, "fail", cyclic), sv.EXACT_EPS),
                  (sv.exact_eps(n, p, dt, "pass", cyclic), sv.EXACT_EPS),
                  (sv.max_at(n, p, dt, sv.EPS, decoys=True), sv.EPS),
                  (sv.max_at(n, p, dt, sv.EPS), sv.EPS),
                  (sv.nan_at(n, p, dt), sv.EPS)]
    wrap = sv.one_fail(n, n - 1, dt, sv.EPS, True)
    assert sv.failing_pairs(wrap, sv.EPS, True) == [n - 1]
    assert sv.failing_pairs(wrap, sv.EPS, False) == []
    cases.append((wrap, sv.EPS))
    states = torch.zeros((len(cases), 64), dtype=torch.uint8, device=DEV)
    for j, (s, eps) in enumerate(cases):
        dev.csr_terms_round(m, t, up(s), s_next, v_prev, v_cur, scratch, states[j], eps=eps,
                            k=k, max_itr=MAX_ITR, semantics=sem)
    got = states.cpu().numpy()
    for j, (s, eps) in enumerate(cases):
        assert got[j].tobytes() == expect_state(s, eps, sem, k), (j, dev.read_state(states[j]))
    s, _ = cases[-1]
    assert np.array_equal(v_cur.cpu().numpy(), np.ones(n, dt) * (s / sv.find_max(s)))
    stops = [_lib.st_state.from_buffer_copy(g.tobytes()).stop for g in got]
    assert 0 in stops and 1 in stops
    assert stops[-1] == int(not cyclic)
    t.close()


# ---------------------------------------------------------------------------
# 5. the whole solve against the dense solve of the densified operator
# ---------------------------------------------------------------------------
def margins(sums, cyclic):
    """max |ds| of the deciding round and of the round before it."""
    def worst(s):
        d = np.abs(s.astype(np.float64) - np.roll(s, -1).astype(np.float64))
        return float((d if cyclic else d[:-1]).max())
    return worst(sums[-1]), worst(sums[-2]) if len(sums) > 1 else float("inf")


def model_with_margin(dense, dt, cyclic, eps=1e-3):
    """The numpy model of the dense operator in dt: (break index, converged).
    First it asserts that the deciding round's max |ds| and that of the round
    before sit away from eps by more than the rounding noise, so that a count
    difference on the device would name its cause.  The noise is measured on
    the model itself: the same iteration in fp32 and in fp64 on the same
    operator differs in those two figures by fp32's rounding (numpy's order is
    not the device's, so 8 times that difference is allowed for); fp64's noise
    is the same scaled by the ratio of the two machine epsilons."""
    kb, conv, sums, _ = cc.model(dense.astype(np.float64), eps, cyclic)
    kb32, conv32, sums32, _ = cc.model(dense.astype(np.float32), eps, cyclic)
    last, before = margins(sums, cyclic)
    assert conv and conv32 and kb32 == kb
    last32, before32 = margins(sums32, cyclic)
    noise = 8 * max(abs(last - last32), abs(before - before32))
    if np.dtype(dt) == np.float64:
        noise *= float(np.finfo(np.float64).eps / np.finfo(np.float32).eps)
    print(f"model: break {kb}, deciding max|ds| {last:.3e}, before {before:.3e}, "
          f"noise allowed for {noise:.1e}")
    assert last < eps - noise and before > eps + noise, (last, before, noise)
    return kb, conv


def per_round_ulps(ip, n, K):
    """The largest row bound of test_round_with_terms_against_the_exact_quotient
    (K fmas and the division included), the relative error of a dot (its share
    of a row's total is below 1) and one ulp for the v update's division and
    product."""
    return max(bound_ulps(int(k)) + K + 1 for k in np.diff(ip)) + tc.dot_depth(n) + 1 + 1


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("case", [0, 2])
def test_solve_against_the_dense_solve_fp64(solver, case, sem, K):
    n, ip, ix, da = table_case(case)
    cyclic = sem == _lib.ST_SEM_SYCL
    u, w = tc.term_vectors(n, K, 10 + case, np.float64)
    dense = tc.dense_m(cc.densify(ip, ix, da), u, w)
    kb, conv = model_with_margin(dense, np.float64, cyclic)
    m = csr_of(solver, ip, ix, da, n)
    t = terms_of(solver, m, u, w)
    lam, v, it, st = solver.solve_csr(m, t, semantics=sem)
    lam_d, v_d, it_d, st_d = solver.solve(up(dense), matrix_free=True, semantics=sem)
    assert (it, st["converged"], st["rounds"]) == (it_d, st_d["converged"], st_d["rounds"])
    assert st["converged"] == 1 and it == cc.count_of(kb, conv, cyclic)
    assert abs(lam - lam_d) <= 1e-10 * abs(lam_d)
    v, v_d = v.cpu().numpy(), v_d.cpu().numpy()
    assert (np.abs(v - v_d) <= 1e-10 * np.abs(v_d)).all()
    t.close()


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("case", [0, 2])
def test_solve_fp32(solver, case, sem, K):
    """As test_gpu_csr.test_solve_fp32 decides it: equal counts, and lambda and
    every v[i] within the summed per-round bounds against the same iteration
    in fp64 on the same fp32-valued operator."""
    n, ip, ix, da = table_case(case)
    cyclic = sem == _lib.ST_SEM_SYCL
    da32 = da.astype(np.float32)
    u, w = tc.term_vectors(n, K, 10 + case, np.float32)
    dense = tc.dense_m(cc.densify(ip, ix, da32.astype(np.float64)), u.astype(np.float64),
                       w.astype(np.float64))
    kb, conv = model_with_margin(dense, np.float32, cyclic)
    per_round = per_round_ulps(ip, n, K)
    m32 = csr_of(solver, ip, ix, da32, n)
    m64 = csr_of(solver, ip, ix, da32.astype(np.float64), n)
    t32 = terms_of(solver, m32, u, w)
    t64 = terms_of(solver, m64, u.astype(np.float64), w.astype(np.float64))
    lam, v, it, st = solver.solve_csr(m32, t32, semantics=sem)
    lam_r, v_r, it_r, st_r = solver.solve_csr(m64, t64, semantics=sem)
    lam_d, _, it_d, st_d = solver.solve(up(dense.astype(np.float32)), matrix_free=True,
                                        semantics=sem)
    assert it == it_r == it_d == cc.count_of(kb, conv, cyclic)
    assert st["converged"] == st_r["converged"] == st_d["converged"] == 1
    budget = per_round * st["rounds"]
    ulp = float(np.finfo(np.float32).eps)
    e_lam = abs(lam - lam_r) / (ulp * abs(lam_r))
    v, v_r = v.cpu().numpy().astype(np.float64), v_r.cpu().numpy()
    e_v = float((np.abs(v - v_r) / (ulp * np.abs(v_r))).max())
    print(f"fp32 vs fp64 case {case} K = {K}: lambda {e_lam:.2f} v {e_v:.2f} relative ulps, "
          f"budget {budget} ({per_round} x {st['rounds']} rounds)")
    assert e_lam <= budget and e_v <= budget
    t32.close()
    t64.close()


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_solve_equals_its_steps(solver, dt, sem):
    n, ip, ix, da = table_case(2)
    m = csr_of(solver, ip, ix, da.astype(dt), n)
    u, w = tc.term_vectors(n, 2, 12, dt)
    t = terms_of(solver, m, u, w)
    lam, v, it, st = solver.solve_csr(m, t, trace=True, semantics=sem)
    sums = solver.last_round_sums()
    td = tdt(dt)
    s = [torch.empty(n, dtype=td, device=DEV) for _ in range(2)]
    vv = [torch.ones(n, dtype=td, device=DEV), torch.empty(n, dtype=td, device=DEV)]
    scratch = t.scratch()
    state = dev.new_state(DEV)
    dev.csr_terms_rowsum(m, t, scratch, out=s[0])
    trace = []
    for k in range(MAX_ITR):
        trace.append(s[k & 1].cpu().numpy())
        dev.csr_terms_round(m, t, s[k & 1], s[(k + 1) & 1], vv[k & 1], vv[(k + 1) & 1], scratch,
                            state, eps=1e-3, k=k + 1, max_itr=MAX_ITR, semantics=sem)
        if dev.read_state(state)["done"]:
            break
    fin = dev.read_state(state)
    assert fin["end"] == st["rounds"] == len(trace) and fin["iters"] == it
    assert np.array_equal(np.stack(trace), sums)
    assert fin["eigen_val"] == lam
    assert np.array_equal(vv[fin["end"] & 1].cpu().numpy(), v.cpu().numpy())
    t.close()


# ---------------------------------------------------------------------------
# 6. left=True with terms
# ---------------------------------------------------------------------------
def holes(dt):
    """TABLE case 0 with rows 0, 9, 30 and 63 emptied and the columns 5 and 63
    without an entry."""
    n, ip, ix, da = table_case(0)
    ix = ix.copy()
    ix[(ix == 5) | (ix == 63)] = 6
    return (n,) + tc.empty_rows(ip, ix, da.astype(dt), [0, 9, 30, 63])


@pytest.mark.parametrize("dt", DTYPES)
def test_left_with_terms_is_the_solve_of_the_host_transposed_arrays(solver, dt):
    n, ip, ix, da = holes(dt)
    u, w = tc.term_vectors(n, 2, 6, dt)
    a = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=True)
    t = terms_of(solver, a, u, w)
    lam, v, it, st = solver.solve_csr(a, t, left=True, trace=True)
    sums = solver.last_round_sums()
    # the device transposition of a source with empty rows against the host twin
    at_dev = a.transpose(solver, allow_empty=True)
    tp, ti, tv = dev.csr_transpose_host(ip, ix, da, allow_empty=True)
    assert np.array_equal(at_dev.crow.cpu().numpy(), tp)
    assert np.array_equal(at_dev.col.cpu().numpy(), ti)
    assert np.array_equal(at_dev.values.cpu().numpy(), tv)
    empties = np.flatnonzero(np.diff(tp) == 0)
    assert list(empties) == [5, 63] and (at_dev.empty_rows, at_dev.first_empty) == (2, 5)
    with pytest.raises(_lib.EigenValueError, match=r"column 5 has no entry"):
        a.transpose(solver)                                  # without the flag: as before
    at = dev.CsrMatrix(up(tp), up(ti), up(tv), n, solver=solver, allow_empty_rows=True)
    us, ws = tc.swap(u, w)
    tt = terms_of(solver, at, us, ws)
    lam_h, v_h, it_h, st_h = solver.solve_csr(at, tt, trace=True)
    assert (lam, it, st["rounds"], st["converged"]) == (lam_h, it_h, st_h["rounds"], 1)
    assert torch.equal(v, v_h) and np.array_equal(sums, solver.last_round_sums())
    # and it is the left vector of M
    M = tc.dense_m(cc.densify(ip, ix, da.astype(np.float64), n), u, w)
    vv = v.cpu().numpy().astype(np.float64)
    r = vv @ M - lam * vv
    assert np.abs(r).max() <= 1e-2 * np.abs(lam * vv).max()
    for x in (t, tt, at_dev, at, a):
        x.close()


# ---------------------------------------------------------------------------
# 7. PageRank
# ---------------------------------------------------------------------------
# (n, break round at fp64 eps 1e-10, break round at eps 1e-3)
PAGERANK = [(12, 86, 23), (67, 135, 36), (300, 128, 28)]


@functools.lru_cache(maxsize=None)
def pagerank_reference(n):
    A = tc.graph(n)
    dang = np.random.default_rng(9).random(n)
    aPt, u, w, G = tc.google(A, 0.85, None, dang)
    ev, V = np.linalg.eig(G)
    p = np.abs(V[:, np.argmax(ev.real)].real)
    return A, dang, aPt, G, p / p.sum()


@pytest.mark.parametrize("n,k10,k3", PAGERANK)
@pytest.mark.parametrize("dt,eps", [pytest.param(np.float64, 1e-10, id="f64-1e-10"),
                                    pytest.param(np.float64, 1e-3, id="f64-1e-3"),
                                    pytest.param(np.float32, 1e-3, id="f32-1e-3")])
def test_pagerank_on_a_reducible_periodic_graph_with_dangling_nodes(solver, dt, eps, n, k10, k3):
    """The graph of csr_terms_cases.graph, alpha = 0.85, uniform teleport, a
    seeded dangling distribution (K = 2), against the numpy model on the dense
    G^T and against numpy.linalg.eig's vector.  Largest distance of pi from
    eig's vector at eps 1e-10, measured on MI355X (one run): 6.88e-11, 5.06e-13
    and 1.27e-13 for n = 12, 67, 300 - what the CPU model gives (6.9e-11,
    5.1e-13, 1.3e-13), 0.69 eps at the worst against the cap of 10 eps; pi is
    within 1.4e-15 relative of the model's pi.  At eps 1e-3: 6.71e-4, 5.65e-6,
    1.76e-6 in both dtypes.  The test prints its own."""
    A, dang, aPt, G, p_eig = pagerank_reference(n)
    kb, conv, sums, v_m = cc.model(G.astype(dt), eps, True)
    assert conv and kb == (k10 if eps == 1e-10 else k3)
    pi_m = (v_m / v_m.sum()).astype(np.float64)
    ip, ix, da = tc.to_csr(A, dt)
    links = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=True)
    dangling_rows = np.flatnonzero(A.sum(axis=1) == 0)   # the last 10 (n = 12: the last 6)
    assert len(dangling_rows) == min(10, n - n // 2) and dangling_rows[-1] == n - 1
    assert (links.empty_rows, links.first_empty) == (len(dangling_rows), dangling_rows[0])
    # without terms P^T is refused, an empty row named
    pt = links.transpose(solver, allow_empty=True)
    assert pt.empty_rows == int((A.sum(axis=0) == 0).sum()) > 0
    with pytest.raises(_lib.EigenValueError, match=rf"row {pt.first_empty} is empty"):
        solver.solve_csr(pt)
    pt.close()
    pi, lam, it, st = solver.pagerank(links, 0.85, dangling=up(dang.astype(dt)), eps=eps,
                                      trace=True)
    s = solver.last_round_sums()[-1].astype(np.float64)
    assert it == cc.count_of(kb, conv, True) and st["converged"] == 1
    pi = pi.cpu().numpy().astype(np.float64)
    dist = float(np.abs(pi - p_eig).max())
    print(f"pagerank n = {n} {np.dtype(dt).name} eps {eps:g}: {it} rounds, "
          f"max |pi - eig| {dist:.2e}, max rel to the model "
          f"{float((np.abs(pi - pi_m) / pi_m).max()):.2e}")
    if np.dtype(dt) == np.float64:
        assert (np.abs(pi - pi_m) <= 1e-10 * pi_m).all()
    assert dist <= 10 * eps
    fe = float(np.finfo(dt).eps)
    assert abs(pi.sum() - 1.0) <= n * fe
    assert s.min() - 4 * fe <= 1.0 <= s.max() + 4 * fe and s.max() - s.min() < n * eps
    assert abs(lam - 1.0) <= n * eps
    if eps == 1e-10:
        # the one-term form against the same operator built as K = 2
        one, _, _, _ = solver.pagerank(links, 0.85, eps=eps)
        two, _, _, _ = solver.pagerank(links, 0.85, eps=eps,
                                       dangling=torch.full((n,), 1.0 / n, dtype=tdt(dt),
                                                           device=DEV))
        one, two = one.cpu().numpy(), two.cpu().numpy()
        assert (np.abs(one - two) <= 1e-10 * np.abs(two)).all()
    links.close()


# ---------------------------------------------------------------------------
# 8. errors on the device path
# ---------------------------------------------------------------------------
def test_device_validation_names_what_it_found(solver):
    n, ip, ix, da = table_case(0)
    m = csr_of(solver, ip, ix, da, n)
    u, w = tc.term_vectors(n, 2, 3)
    for val, shown in ((-0.5, "-0.5"), (np.nan, "nan"), (np.inf, "inf")):
        b = w.copy()
        b[1, 17] = val
        with pytest.raises(_lib.EigenValueError, match=rf"w_1\[17\] = {shown}"):
            terms_of(solver, m, u, b)
    bu, bw = u.copy(), w.copy()
    bu[1, 3], bw[0, 60], bu[0, 40], bu[0, 41] = -1, -1, np.nan, -1
    with pytest.raises(_lib.EigenValueError, match=r"u_0\[40\]"):
        terms_of(solver, m, bu, bw)
    bu[0, 40], bu[0, 41] = 0, 0
    with pytest.raises(_lib.EigenValueError, match=r"w_0\[60\]"):
        terms_of(solver, m, bu, bw)
    # a row of the operator without a positive entry: the lowest is named
    e = tc.empty_rows(ip, ix, da, [9, 30])
    with pytest.raises(_lib.EigenValueError, match=r"row 9 is empty"):
        csr_of(solver, *e, n)                                  # st_csr_create: as before
    me = dev.CsrMatrix(up(e[0]), up(e[1]), up(e[2]), n, solver=solver, allow_empty_rows=True)
    z = u.copy()
    z[:, 30] = 0
    with pytest.raises(_lib.EigenValueError, match=r"row 30 of A \+ Σ u wᵀ has no positive"):
        terms_of(solver, me, z, w)
    z[:, 9] = 0
    with pytest.raises(_lib.EigenValueError, match=r"row 9 of A \+ Σ u wᵀ"):
        terms_of(solver, me, z, w)
    # an empty-rows handle where a row sum of A alone would be divided
    with pytest.raises(_lib.EigenValueError, match=r"st_solve_csr: row 9 is empty \(2 empty"):
        solver.solve_csr(me)
    s, v = up(positive(n, np.float64, 1)), up(positive(n, np.float64, 2))
    o1, o2, x = torch.empty_like(s), torch.empty_like(s), torch.empty_like(s)
    with pytest.raises(_lib.EigenValueError, match=r"st_csr_mfree_round: row 9 is empty"):
        dev.csr_mfree_round(me, s, o1, v, o2, x, dev.new_state(DEV))
    # nnz >= 1 stays required
    with pytest.raises(_lib.EigenValueError, match=r"nnz must be >= 1"):
        dev.CsrMatrix(up(np.zeros(5, np.int64)), up(np.zeros(0, np.int32)), up(np.zeros(0)), 4,
                      solver=solver, allow_empty_rows=True)
    # and the good one solves
    t = terms_of(solver, me, u, w)
    assert solver.solve_csr(me, t)[3]["converged"] == 1
    t.close()


def test_terms_are_bound_to_their_matrix(solver):
    n, ip, ix, da = table_case(0)
    m = csr_of(solver, ip, ix, da, n)
    other = csr_of(solver, ip, ix, da, n)
    m32 = csr_of(solver, ip, ix, da.astype(np.float32), n)
    u, w = tc.term_vectors(n, 1, 3)
    t = terms_of(solver, m, u, w)
    L = _lib.load()
    # the Python fronts, before any library call
    with pytest.raises(ValueError, match="another matrix"):
        solver.solve_csr(other, t)
    with pytest.raises(TypeError, match="the matrix torch.float32"):
        terms_of(solver, m32, u, w)
    with pytest.raises(ValueError, match="the matrix on"):
        dev.CsrTerms(m, [torch.from_numpy(u[0])], [up(w[0])], solver=solver)
    with pytest.raises(TypeError, match="terms must be a CsrTerms"):
        solver.solve_csr(m, (u, w))
    # the library itself
    v = torch.empty(n, dtype=torch.float64, device=DEV)
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    for h in (other, m32):
        rc = L.st_solve_csr_terms(solver.q, h.handle, t.handle, v.data_ptr(), None,
                                  ctypes.byref(ev), ctypes.byref(it), None, None)
        assert rc < 0 and "belongs to another matrix handle" in _lib.last_error(L)
        assert L.st_csr_terms_rowsum(h.handle, t.handle, v.data_ptr(), v.data_ptr(), None) < 0
        assert "belongs to another matrix handle" in _lib.last_error(L)
    # a handle of another kind, either way round
    rc = L.st_solve_csr_terms(solver.q, t.handle, t.handle, v.data_ptr(), None,
                              ctypes.byref(ev), ctypes.byref(it), None, None)
    assert rc < 0 and "not a CSR matrix handle" in _lib.last_error(L)
    rc = L.st_solve_csr_terms(solver.q, m.handle, m.handle, v.data_ptr(), None,
                              ctypes.byref(ev), ctypes.byref(it), None, None)
    assert rc < 0 and "not a terms object" in _lib.last_error(L)
    # a closed matrix
    closed = csr_of(solver, ip, ix, da, n)
    closed.close()
    with pytest.raises(ValueError, match="closed"):
        dev.CsrTerms(closed, [up(u[0])], [up(w[0])], solver=solver)
    # K out of range, by the library
    pu = (ctypes.c_void_p * 5)(*[v.data_ptr()] * 5)
    out = ctypes.c_void_p()
    for K in (0, 5):
        assert L.st_csr_terms_create(solver.q, m.handle, K, pu, pu, ctypes.byref(out)) < 0
        assert f"K must be in [1, 4], got {K}" in _lib.last_error(L) and not out.value
    assert solver.solve_csr(m, t)[3]["converged"] == 1
    # a closed terms object
    t.close()
    assert not t.handle.value
    with pytest.raises(_lib.EigenValueError, match="not a terms object"):
        solver.solve_csr(m, t)
