"""GPU: many term sets on one CSR matrix - st_csr_multi_rowsum /
st_csr_multi_round / st_solve_csr_multi / pagerank_multi.  Every comparison is
bitwise (tobytes() equality) against the single path on the same device:
column c of the multi call against st_csr_terms_* / solve_csr(m, CsrTerms) /
pagerank on that column's terms alone.

1  step level: K0 and two rounds, per column s, v, x, dots and the state
2  the vector pass at its boundaries: the deciding pair of one column at the
   first, the last and a wave-boundary element while the other columns pass
3  a finished column, and the padding columns, get no writes
4  whole solves: columns with different round counts, a max_itr that some
   columns exhaust, a u = 0 column against the plain solve
5  pagerank_multi against pagerank, also C = 11 in chunks of 8 and 3
6  validation names the column; the object is bound to its matrix
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
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from test_gpu_csr import (BLOCK, DEV, DTYPES, MAX_ITR, PREP_GRID, SEMS, csr_of,  # noqa: E402
                          diagonal_plus, positive, table_case, tdt, up)

EMPTIED = [0, 5, 1500, 2999]          # rows of table case 2 taken away (3000 rows)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def pack(cols, cp, fill=1.0):
    """[C][n] -> the packed [n, CP] array, padding columns holding `fill`."""
    cols = np.asarray(cols)
    out = np.full((cols.shape[1], cp), fill, dtype=cols.dtype)
    out[:, :cols.shape[0]] = cols.T
    return out


def multi_of(solver, m, U, W):
    return dev.CsrMultiTerms(m, up(np.asarray(U)), up(np.asarray(W)), solver=solver)


def single_of(solver, m, u, w):
    return dev.CsrTerms(m, [up(x) for x in u], [up(x) for x in w], solver=solver)


def single_round(m, t, s_prev, v_prev, k, eps, sem, max_itr=MAX_ITR):
    """One st_csr_terms_round from a fresh state: (s_next, v_cur, x, dots,
    state bytes) as numpy."""
    td = tdt(s_prev.dtype)
    s_next = torch.full((m.n,), SENTINEL, dtype=td, device=DEV)
    v_cur = torch.full((m.n,), SENTINEL, dtype=td, device=DEV)
    scratch = t.scratch()
    state = dev.new_state(DEV)
    dev.csr_terms_round(m, t, up(s_prev), s_next, up(v_prev), v_cur, scratch, state, eps=eps,
                        k=k, max_itr=max_itr, semantics=sem)
    return (s_next.cpu().numpy(), v_cur.cpu().numpy(), t.x(scratch).cpu().numpy(),
            t.dots(scratch).cpu().numpy(), state.cpu().numpy())


def multi_round(m, mt, s_prev, v_prev, k, eps, sem, max_itr=MAX_ITR, states=None):
    """One st_csr_multi_round on packed numpy inputs: (s_next, v_cur, x, dots
    [C, K], states [C, 64], finished) as numpy; outputs start as SENTINEL."""
    s_next, v_cur = mt.packed(SENTINEL), mt.packed(SENTINEL)
    scratch = mt.scratch()
    fresh, finished = mt.new_states()
    states = fresh if states is None else states
    dev.csr_multi_round(m, mt, up(s_prev), s_next, up(v_prev), v_cur, scratch, states, finished,
                        eps=eps, k=k, max_itr=max_itr, semantics=sem)
    return (s_next.cpu().numpy(), v_cur.cpu().numpy(), mt.x(scratch).cpu().numpy(),
            mt.dots(scratch).cpu().numpy(), states.cpu().numpy(), int(finished.item()))


def test_shape_desc_matches_what_the_tests_assume():
    d = _lib.csr_multi_shape()
    assert d["dot_grid"] == PREP_GRID == tc.DOT_GRID and d["lanes"] == BLOCK == tc.BLOCK
    assert d["multi_max"] == 8 and d["widths"] == (2, 4, 8) and d["partial_offset"] == 256


# ---------------------------------------------------------------------------
# 1. step level
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_arrays(emptied, dtname):
    n, ip, ix, da = table_case(2)
    da = da.astype(dtname)
    if emptied:
        ip, ix, da = tc.empty_rows(ip, ix, da, EMPTIED)
    return n, ip, ix, da


def step_terms(n, K, dt):
    """Seeded terms of 8 columns, [8, K, n]; a call with C columns takes the
    first C, so one single-path reference serves every C."""
    u, w = tc.term_vectors(n, 8 * K, 17, dt)
    return u.reshape(8, K, n), w.reshape(8, K, n)


_STEP_REF = {}


def step_reference(solver, emptied, K, dt):
    """The single path, column by column, computed once per (matrix, K, dtype):
    K0, then launches 1 and 2, each from a fresh state."""
    key = (emptied, K, np.dtype(dt).name)
    if key in _STEP_REF:
        return _STEP_REF[key]
    n, ip, ix, da = step_arrays(emptied, np.dtype(dt).name)
    m = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=True)
    U, W = step_terms(n, K, dt)
    ref = []
    for c in range(8):
        t = single_of(solver, m, U[c], W[c])
        scratch = t.scratch()
        s0 = dev.csr_terms_rowsum(m, t, scratch).cpu().numpy()
        d0 = t.dots(scratch).cpu().numpy()
        r1 = single_round(m, t, s0, np.ones(n, dtype=dt), 1, 1e-3, _lib.ST_SEM_SYCL)
        r2 = single_round(m, t, r1[0], r1[1], 2, 1e-3, _lib.ST_SEM_SYCL)
        ref.append((s0, d0, r1, r2))
        t.close()
    m.close()
    _STEP_REF[key] = ref
    return ref


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("C", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("emptied", [False, True], ids=["full", "emptied"])
@pytest.mark.parametrize("dt", DTYPES)
def test_steps_equal_the_single_steps_per_column(solver, dt, emptied, C, K):
    ref = step_reference(solver, emptied, K, dt)
    n, ip, ix, da = step_arrays(emptied, np.dtype(dt).name)
    m = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=True)
    assert m.empty_rows == (len(EMPTIED) if emptied else 0)
    assert (np.diff(m.plan()[1]) > 0).all()                    # all four row classes
    U, W = step_terms(n, K, dt)
    mt = multi_of(solver, m, U[:C], W[:C])
    assert (mt.C, mt.K, mt.CP) == (C, K, _lib.csr_multi_cp(C))
    scratch = mt.scratch()
    s0 = dev.csr_multi_rowsum(m, mt, scratch).cpu().numpy()
    d0 = mt.dots(scratch).cpu().numpy()
    for c in range(C):
        assert same(s0[:, c], ref[c][0]) and same(d0[c], ref[c][1]), c
    # launch 1 from (s_0, v = 1), launch 2 from launch 1's outputs, fresh states each
    v0 = np.ones((n, mt.CP), dtype=dt)
    r1 = multi_round(m, mt, s0, v0, 1, 1e-3, _lib.ST_SEM_SYCL)
    # launch 2 reads launch 1's s_next / v_cur: the padding slots were never written, so
    # give them finite values as the solve loop's buffers have
    s1, v1 = r1[0].copy(), r1[1].copy()
    assert (s1[:, C:] == SENTINEL).all() and (v1[:, C:] == SENTINEL).all()
    s1[:, C:], v1[:, C:] = 1.0, 1.0
    r2 = multi_round(m, mt, s1, v1, 2, 1e-3, _lib.ST_SEM_SYCL)
    for k, got in ((1, r1), (2, r2)):
        for c in range(C):
            want = ref[c][2 + k - 1]
            assert same(got[0][:, c], want[0]), ("s_next", k, c)
            assert same(got[1][:, c], want[1]), ("v_cur", k, c)
            assert same(got[2][:, c], want[2]), ("x", k, c)
            assert same(got[3][c], want[3]), ("dots", k, c)
            assert same(got[4][c], want[4]), ("state", k, c)
        assert got[5] == 0                                     # nothing ended
    mt.close()
    m.close()


# ---------------------------------------------------------------------------
# 2. the vector pass at its boundaries
# ---------------------------------------------------------------------------
PASS_N = [1, 2, 255, 256, 257, 3 * 256 + 37, PREP_GRID * 256 + 256 + 37]


def state_of(raw):
    return _lib.st_state.from_buffer_copy(bytes(np.ascontiguousarray(raw).tobytes()))


@pytest.mark.parametrize("n", PASS_N)
@pytest.mark.parametrize("dt", DTYPES)
def test_the_vector_pass_at_its_boundaries(solver, dt, n):
    """C = 8, K = 1 on a diagonal-plus-one-entry matrix.  Every column's s_prev
    is flat (every pair passes) except that column DEC carries one raised
    element - at the first, the last and a wave-boundary position in turn - so
    that only its stop test fails.  Dots, max, stop and the whole state per
    column against the single pass."""
    DEC, eps, k = 5, 1e-3, 2
    m = diagonal_plus(solver, n, dt)
    rng = np.random.default_rng(n)
    W = (0.5 + rng.random((8, 1, n))).astype(dt)
    U = np.zeros((8, 1, n), dtype=dt)
    mt = multi_of(solver, m, U, W)
    flat = np.array([1.25 + 0.125 * c for c in range(8)], dtype=dt)   # a max of its own each
    v_prev = np.stack([positive(n, dt, 40 + c) for c in range(8)])
    singles = [single_of(solver, m, U[c], W[c]) for c in range(8)]
    positions = sorted({0, n - 1, min(63, n - 1), min(64, n - 1)})
    sems = [_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY] if n < 4096 else [_lib.ST_SEM_SYCL]
    passing = {}                       # the seven other columns do not depend on the position
    for sem in sems:
        for p in positions:
            s_prev = np.repeat(flat[:, None], n, axis=1)
            s_prev[DEC, p] += dt(0.5)
            got = multi_round(m, mt, pack(s_prev, 8), pack(v_prev, 8), k, eps, sem)
            stops = []
            for c in range(8):
                if c == DEC or (sem, c) not in passing:
                    want = single_round(m, singles[c], s_prev[c], v_prev[c], k, eps, sem)
                    if c != DEC:
                        passing[(sem, c)] = want
                else:
                    want = passing[(sem, c)]
                assert same(got[3][c], want[3]), ("dots", sem, p, c)
                assert same(got[4][c], want[4]), ("state", sem, p, c)
                assert same(got[2][:, c], want[2]), ("x", sem, p, c)
                st = state_of(got[4][c])
                assert st.max == float(s_prev[c].max()) and st.round == k - 1
                stops.append(st.stop)
            # only DEC's stop changes (a single element has no pair that differs)
            expect = [1] * 8
            if n >= 2:
                expect[DEC] = 0
            assert stops == expect, (sem, p, stops)
            assert got[5] == sum(expect)                       # the stopped columns ended
    for t in singles:
        t.close()
    mt.close()
    m.close()


# ---------------------------------------------------------------------------
# 3. a finished column gets no writes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,gone", [(3, 1), (5, 0), (8, 7)])
@pytest.mark.parametrize("dt", DTYPES)
def test_a_finished_column_and_the_padding_get_no_writes(solver, dt, C, gone):
    ref = step_reference(solver, False, 1, dt)
    n, ip, ix, da = step_arrays(False, np.dtype(dt).name)
    m = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=True)
    U, W = step_terms(n, 1, dt)
    mt = multi_of(solver, m, U[:C], W[:C])
    cp = mt.CP
    # launch 2's inputs: the single path's launch 1 outputs, column by column
    s1 = pack([ref[c][2][0] for c in range(C)], cp)
    v1 = pack([ref[c][2][1] for c in range(C)], cp)
    states, _ = mt.new_states()
    ended = _lib.st_state()
    ended.end, ended.done, ended.stop, ended.iters, ended.max = 1, 1, 1, 1, 3.5
    raw = np.zeros((C, 64), dtype=np.uint8)
    raw[gone] = np.frombuffer(bytes(ended), dtype=np.uint8)
    states.copy_(up(raw))
    got = multi_round(m, mt, s1, v1, 2, 1e-3, _lib.ST_SEM_SYCL, states=states)
    # the ended column: not one slot, not one state byte
    assert (got[0][:, gone] == SENTINEL).all() and (got[1][:, gone] == SENTINEL).all()
    assert same(got[4][gone], raw[gone])
    # the padding columns
    assert (got[0][:, C:] == SENTINEL).all() and (got[1][:, C:] == SENTINEL).all()
    # every other column: the single step
    for c in range(C):
        if c == gone:
            continue
        want = ref[c][3]
        assert same(got[0][:, c], want[0]) and same(got[1][:, c], want[1]), c
        assert same(got[3][c], want[3]) and same(got[4][c], want[4]), c
    assert got[5] == 0
    # every column ended: nothing at all is written
    raw[:] = np.frombuffer(bytes(ended), dtype=np.uint8)
    states.copy_(up(raw))
    got = multi_round(m, mt, s1, v1, 2, 1e-3, _lib.ST_SEM_SYCL, states=states)
    assert (got[0] == SENTINEL).all() and (got[1] == SENTINEL).all() and same(got[4], raw)
    mt.close()
    m.close()


# ---------------------------------------------------------------------------
# 4. whole solves
# ---------------------------------------------------------------------------
SCALES = [0.02, 8.0, 60.0, 200.0, 0.0]  # the size of column c's terms; the last: u = 0


def solve_terms(n, K, dt, seed=23):
    """[5, K, n] terms whose size differs from column to column, so that the
    columns stop in different rounds; the last column has u = 0."""
    U, W = [], []
    for c, f in enumerate(SCALES):
        u, w = tc.term_vectors(n, K, seed + c, dt, lo=0.01, hi=0.05)
        U.append((u * dt(f)).astype(dt))
        W.append(w)
    return np.array(U), np.array(W)


@functools.lru_cache(maxsize=None)
def model_counts(case, K, dtname, cyclic):
    """(break index, converged) of the numpy model on the dense M_c, per column."""
    n, ip, ix, da = table_case(case)
    a = cc.densify(ip, ix, da.astype(dtname))
    U, W = solve_terms(n, K, np.dtype(dtname).type)
    out = []
    for c in range(len(SCALES)):
        kb, conv, _, _ = cc.model(tc.dense_m(a, U[c], W[c]), 1e-3, cyclic)
        out.append((kb, conv))
    return out


def check_multi_solve(solver, m, U, W, sem, max_itr=0, plain_last=False):
    """solve_csr_multi against C calls of solve_csr(m, CsrTerms): (iterations,
    converged) per column."""
    C = len(U)
    mt = multi_of(solver, m, U, W)
    lam, V, its, conv, stats = solver.solve_csr_multi(m, mt, semantics=sem, max_itr=max_itr)
    assert V.shape == (C, m.n) and V.is_contiguous()
    V = V.cpu().numpy()
    for c in range(C):
        t = single_of(solver, m, U[c], W[c])
        l1, v1, i1, st = solver.solve_csr(m, t, semantics=sem, max_itr=max_itr)
        t.close()
        assert same(np.array(lam[c]), np.array(l1, dtype=lam.dtype)), c
        assert same(V[c], v1.cpu().numpy()), c
        assert (int(its[c]), int(conv[c])) == (i1, st["converged"]), c
    if plain_last:                       # u = 0: every bit is the solve without terms
        l0, v0, i0, st0 = solver.solve_csr(m, semantics=sem, max_itr=max_itr)
        assert same(np.array(lam[-1]), np.array(l0, dtype=lam.dtype))
        assert same(V[-1], v0.cpu().numpy()) and int(its[-1]) == i0
    assert stats["rounds"] >= 1 and stats["converged"] == int(conv.all())
    mt.close()
    return its, conv


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("case", [0, 2])
@pytest.mark.parametrize("dt", DTYPES)
def test_solves_equal_the_single_solves_per_column(solver, dt, case, sem, K):
    cyclic = sem == _lib.ST_SEM_SYCL
    counts = model_counts(case, K, np.dtype(dt).name, cyclic)
    assert all(conv for _, conv in counts)
    assert len({kb for kb, _ in counts}) >= 3, counts          # on the CPU, before the GPU runs
    n, ip, ix, da = table_case(case)
    m = csr_of(solver, ip, ix, da.astype(dt), n)
    U, W = solve_terms(n, K, dt)
    its, conv = check_multi_solve(solver, m, U, W, sem, plain_last=True)
    assert conv.all() and len(set(its.tolist())) >= 3
    m.close()


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_a_max_itr_that_some_columns_exhaust(solver, dt, sem):
    cyclic = sem == _lib.ST_SEM_SYCL
    counts = model_counts(2, 1, np.dtype(dt).name, cyclic)
    breaks = sorted(kb for kb, _ in counts)
    # the library evaluates rounds 0 .. max_itr - 1: a column that breaks at index kb
    # converges when kb < max_itr.  Between the fastest and the slowest column:
    max_itr = breaks[len(breaks) // 2]
    assert breaks[0] < max_itr <= breaks[-1], (breaks, max_itr)
    n, ip, ix, da = table_case(2)
    m = csr_of(solver, ip, ix, da.astype(dt), n)
    U, W = solve_terms(n, 1, dt)
    its, conv = check_multi_solve(solver, m, U, W, sem, max_itr=max_itr)
    assert 0 < int(conv.sum()) < len(conv), (conv, breaks, max_itr)   # both kinds
    assert (its[conv == 0] == max_itr).all()
    m.close()


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_one_row_and_two_rows_by_hand(solver, dt, sem):
    for n, ip, ix, da in ((1, [0, 1], [0], [2.0]),
                          (2, [0, 2, 4], [0, 1, 0, 1], [1.0, 2.0, 3.0, 4.0])):
        m = csr_of(solver, np.array(ip), np.array(ix), np.array(da, dtype=dt), n)
        U = np.array([[[0.5] * n], [[0.0] * n], [[3.0] * n]], dtype=dt)       # C = 3, K = 1
        W = np.array([[[0.25] * n], [[1.0] * n], [[0.125, 2.0][:n]]], dtype=dt)
        check_multi_solve(solver, m, U, W, sem)
        check_multi_solve(solver, m, U, W, sem, max_itr=2)
        m.close()


# ---------------------------------------------------------------------------
# 5. pagerank_multi
# ---------------------------------------------------------------------------
def teleports_of(n, C, dt):
    rng = np.random.default_rng(31)
    uni = np.full(n, 1.0 / n)
    hot = np.zeros(n)
    hot[n // 3] = 1.0
    t = [uni, 0.5 * uni + 0.5 * hot, 0.05 + rng.random(n)]
    while len(t) < C:
        t.append(0.05 + rng.random(n))
    return np.array(t[:C]).astype(dt)


@pytest.mark.parametrize("with_dangling", [False, True], ids=["one-term", "dangling"])
@pytest.mark.parametrize("n", [12, 67, 300])
@pytest.mark.parametrize("dt", DTYPES)
def test_pagerank_multi_equals_pagerank_per_teleport(solver, dt, n, with_dangling):
    ip, ix, da = tc.to_csr(tc.graph(n), dt)
    links = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=True)
    dang = up(np.random.default_rng(9).random(n).astype(dt)) if with_dangling else None
    T = up(teleports_of(n, 3, dt))
    Pi, lam, its, stats = solver.pagerank_multi(links, 0.85, teleports=T, dangling=dang)
    assert Pi.shape == (3, n) and lam.shape == (3,) and its.shape == (3,)
    for c in range(3):
        pi, l1, i1, _ = solver.pagerank(links, 0.85, teleport=T[c], dangling=dang)
        assert same(Pi[c].cpu().numpy(), pi.cpu().numpy()), c
        assert same(np.array(lam[c]), np.array(l1, dtype=lam.dtype)) and int(its[c]) == i1, c
    assert torch.allclose(Pi.sum(dim=1), torch.ones(3, dtype=Pi.dtype, device=DEV))
    with pytest.raises(ValueError, match="teleport must be a tensor of shape"):
        solver.pagerank(links, 0.85, teleport=T)               # pagerank itself: as before
    links.close()


def test_pagerank_multi_in_chunks_of_8_and_3(solver):
    n, dt = 67, np.float64
    ip, ix, da = tc.to_csr(tc.graph(n), dt)
    links = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=True)
    T = up(teleports_of(n, 11, dt))
    Pi, lam, its, _ = solver.pagerank_multi(links, 0.85, teleports=T, eps=1e-8)
    assert Pi.shape == (11, n) and lam.shape == (11,) and its.shape == (11,)
    for c in range(11):
        pi, l1, i1, _ = solver.pagerank(links, 0.85, teleport=T[c], eps=1e-8)
        assert same(Pi[c].cpu().numpy(), pi.cpu().numpy()), c
        assert same(np.array(lam[c]), np.array(l1)) and int(its[c]) == i1, c
    links.close()


# ---------------------------------------------------------------------------
# 6. validation names the column
# ---------------------------------------------------------------------------
def test_device_validation_names_the_column(solver):
    n, ip, ix, da = table_case(0)
    m = csr_of(solver, ip, ix, da, n)
    u, w = tc.term_vectors(n, 8, 3)
    U, W = u.reshape(4, 2, n), w.reshape(4, 2, n)
    for val, shown in ((-0.5, "-0.5"), (np.nan, "nan"), (np.inf, "inf")):
        b = U.copy()
        b[2, 1, 17] = val
        with pytest.raises(_lib.EigenValueError, match=rf"column 2: u_1\[17\] = {shown}"):
            multi_of(solver, m, b, W)
    # the lowest offender: column first, then term, u before w, index
    bu, bw = U.copy(), W.copy()
    bu[3, 0, 0], bw[1, 1, 5], bu[1, 1, 60] = -1, -1, -1
    with pytest.raises(_lib.EigenValueError, match=r"column 1: u_1\[60\]"):
        multi_of(solver, m, bu, bw)
    bu[1, 1, 60] = 0
    with pytest.raises(_lib.EigenValueError, match=r"column 1: w_1\[5\]"):
        multi_of(solver, m, bu, bw)
    # a row of M_c without a positive entry; a later column's bad entry does not hide it
    e = tc.empty_rows(ip, ix, da, [9, 30])
    me = dev.CsrMatrix(up(e[0]), up(e[1]), up(e[2]), n, solver=solver, allow_empty_rows=True)
    z = U.copy()
    z[1, :, 30] = 0
    with pytest.raises(_lib.EigenValueError,
                       match=r"column 1: row 30 of A \+ Σ u wᵀ has no positive entry"):
        multi_of(solver, me, z, W)
    zw = W.copy()
    zw[2, 0, 3] = -2
    with pytest.raises(_lib.EigenValueError, match=r"column 1: row 30 of A"):
        multi_of(solver, me, z, zw)
    mt = multi_of(solver, me, U, W)                            # and the good one solves
    assert solver.solve_csr_multi(me, mt)[3].all()
    mt.close()
    # a one-hot teleport leaves every other node without an in-link without a positive entry
    g = tc.graph(67)
    ip, ix, da = tc.to_csr(g)
    links = dev.CsrMatrix(up(ip), up(ix), up(da), 67, solver=solver, allow_empty_rows=True)
    hot = 22
    no_in = [int(r) for r in np.flatnonzero(g.sum(axis=0) == 0) if r != hot]
    assert no_in                                               # on the CPU, before the GPU runs
    T = teleports_of(67, 3, np.float64)
    T[1] = 0
    T[1, hot] = 1
    with pytest.raises(_lib.EigenValueError,
                       match=rf"column 1: row {no_in[0]} of A \+ Σ u wᵀ has no positive entry"):
        solver.pagerank_multi(links, 0.85, teleports=up(T))
    links.close()


def test_the_object_is_bound_to_its_matrix(solver):
    n, ip, ix, da = table_case(0)
    m = csr_of(solver, ip, ix, da, n)
    other = csr_of(solver, ip, ix, da, n)
    m32 = csr_of(solver, ip, ix, da.astype(np.float32), n)
    u, w = tc.term_vectors(n, 3, 3)
    mt = multi_of(solver, m, u, w)                             # [C, n]: K = 1
    assert (mt.C, mt.K, mt.CP) == (3, 1, 4)
    single = single_of(solver, m, u[:1], w[:1])
    L = _lib.load()
    with pytest.raises(ValueError, match="another matrix"):
        solver.solve_csr_multi(other, mt)
    with pytest.raises(TypeError, match="the matrix torch.float32"):
        multi_of(solver, m32, u, w)
    with pytest.raises(TypeError, match="mterms must be a CsrMultiTerms"):
        solver.solve_csr_multi(m, single)
    V = torch.empty((3, n), dtype=torch.float64, device=DEV)
    lam, its = np.zeros(3), np.zeros(3, np.uint32)
    for h in (other, m32):
        rc = L.st_solve_csr_multi(solver.q, h.handle, mt.handle, V.data_ptr(), None,
                                  lam.ctypes.data, its.ctypes.data, None, None, None)
        assert rc < 0 and "belongs to another matrix handle" in _lib.last_error(L)
        assert L.st_csr_multi_rowsum(h.handle, mt.handle, V.data_ptr(), V.data_ptr(), None) < 0
        assert "belongs to another matrix handle" in _lib.last_error(L)
    # a handle of another kind, either way round
    rc = L.st_solve_csr_multi(solver.q, mt.handle, mt.handle, V.data_ptr(), None,
                              lam.ctypes.data, its.ctypes.data, None, None, None)
    assert rc < 0 and "not a CSR matrix handle" in _lib.last_error(L)
    for wrong in (m, single):
        rc = L.st_solve_csr_multi(solver.q, m.handle, wrong.handle, V.data_ptr(), None,
                                  lam.ctypes.data, its.ctypes.data, None, None, None)
        assert rc < 0 and "not a multi terms object" in _lib.last_error(L)
    # C and K out of range, by the library
    pu = (ctypes.c_void_p * 45)(*[V.data_ptr()] * 45)
    out = ctypes.c_void_p()
    for C, K, what in ((0, 1, "C must be in [1, 8], got 0"), (9, 1, "C must be in [1, 8], got 9"),
                       (2, 0, "K must be in [1, 4], got 0"), (2, 5, "K must be in [1, 4], got 5")):
        assert L.st_csr_multi_create(solver.q, m.handle, C, K, pu, pu, ctypes.byref(out)) < 0
        assert what in _lib.last_error(L) and not out.value
    assert solver.solve_csr_multi(m, mt)[3].all()
    # a closed object
    mt.close()
    assert not mt.handle.value
    with pytest.raises(_lib.EigenValueError, match="not a multi terms object"):
        solver.solve_csr_multi(m, mt)
    single.close()
