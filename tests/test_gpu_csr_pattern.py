"""GPU: the pattern-only CSR solve (section 3h) - st_csr_pattern_create /
transpose / terms_create, st_csr_pattern_rowsum / round, st_solve_csr_pattern,
pagerank on a CsrPattern.  Comparisons are of bytes unless said otherwise.

1  no scales = the values kernels on the ones matrix (rowsum, one round with
   its state, the solve with its trace, terms K = 1, 2, 4 and emptied rows)
2  power-of-two scales = the values kernels on vals[e] = r[row] * c[col]
3  general scales (and a +-20 / +-200 exponent range) against the host model
   csr_pattern_model, K = 0 and 2; z[col[0]] is the largest z
4  rows stand alone: the rows permuted, every row's result keeps its bits
5  transposition: st_csr_transpose_ex's arrays, the scales swapped, left
6  gating: a round beyond the end writes nothing
7  PageRank on a CsrPattern: test_gpu_csr_terms' cases and tolerances, and no
   tensor of nnz values allocated
8  validation on the device and the cross-refusals of the two handle kinds
9  numpy / scipy / torch.sparse_csr give the same bytes; two runs do too
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
import csr_order_model as om  # noqa: E402
import csr_pattern_model as pm  # noqa: E402
import csr_terms_cases as tc  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from test_gpu_csr import DEV, DTYPES, MAX_ITR, SEMS, tdt  # noqa: E402
from test_gpu_csr_order import assert_same  # noqa: E402
from test_gpu_csr_terms import PAGERANK, pagerank_reference  # noqa: E402

SENTINEL = -7.0
AB = [pytest.param(r, id=r) for r in ("A", "B")]


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def up(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # a copy: the cases are read-only


def name_of(dt):
    return np.dtype(dt).name


def values_of(solver, indptr, indices, data, n, **kw):
    return dev.CsrMatrix(up(np.asarray(indptr, np.int64)), up(np.asarray(indices, np.int32)),
                         up(data), n, solver=solver, **kw)


def pattern_of(solver, indptr, indices, n, dt, r=None, c=None, **kw):
    return dev.CsrPattern(up(np.asarray(indptr, np.int64)), up(np.asarray(indices, np.int32)), n,
                          row_scale=None if r is None else up(r),
                          col_scale=None if c is None else up(c), dtype=tdt(dt), solver=solver,
                          **kw)


def scaled_values(indptr, indices, r, c, dt):
    """vals[e] = r[row] * c[col] (exact for powers of two)."""
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    v = np.ones(len(indices), dtype=dt)
    if r is not None:
        v = v * r[rows]
    if c is not None:
        v = v * c[indices]
    return v.astype(dt)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def values_round(m, s_prev, v_prev, k=1, sem=_lib.ST_SEM_SYCL, state=None):
    t = tdt(s_prev.dtype)
    s_next = torch.full((m.n,), SENTINEL, dtype=t, device=DEV)
    v_cur = torch.full((m.n,), SENTINEL, dtype=t, device=DEV)
    x = torch.full((m.n,), SENTINEL, dtype=t, device=DEV)
    state = dev.new_state(DEV) if state is None else state
    dev.csr_mfree_round(m, up(s_prev), s_next, up(v_prev), v_cur, x, state, eps=1e-3, k=k,
                        max_itr=MAX_ITR, semantics=sem)
    return s_next.cpu().numpy(), v_cur.cpu().numpy(), x.cpu().numpy(), state.cpu().numpy()


def pattern_round(p, s_prev, v_prev, terms=None, k=1, sem=_lib.ST_SEM_SYCL, state=None):
    """One st_csr_pattern_round on sentinel-filled outputs: (s_next, v_cur, z,
    state bytes, dots)."""
    t = tdt(s_prev.dtype)
    s_next = torch.full((p.n,), SENTINEL, dtype=t, device=DEV)
    v_cur = torch.full((p.n,), SENTINEL, dtype=t, device=DEV)
    scratch = dev.csr_pattern_scratch(p, terms)
    K = 0 if terms is None else terms.K
    es = 8 if p.dtype_code else 4
    off = 256 + K * 2048 * 8
    scratch[off:off + p.n * es].view(p.dtype).fill_(SENTINEL)
    state = dev.new_state(DEV) if state is None else state
    dev.csr_pattern_round(p, terms, up(s_prev), s_next, up(v_prev), v_cur, scratch, state,
                          eps=1e-3, k=k, max_itr=MAX_ITR, semantics=sem)
    dots = None if terms is None else terms.dots(scratch).cpu().numpy()
    return (s_next.cpu().numpy(), v_cur.cpu().numpy(),
            dev.csr_pattern_z(p, scratch, terms).cpu().numpy(), state.cpu().numpy(), dots)


def solve_both(solver, p, m, sem, pt=None, mt=None, eps=1e-3, max_itr=60):
    """(λ, v, count, rounds, converged, trace) of the pattern solve and of the
    values solve."""
    out = []
    for call, mat, terms in ((solver.solve_csr_pattern, p, pt), (solver.solve_csr, m, mt)):
        lam, v, it, st = call(mat, terms, eps=eps, max_itr=max_itr, semantics=sem, trace=True)
        out.append((lam, v.cpu().numpy(), it, st["rounds"], st["converged"],
                    solver.last_round_sums().copy()))
    return out


def assert_same_solve(got, want, what):
    assert got[0] == want[0] and got[2:5] == want[2:5], (what, got[0], want[0], got[2:5],
                                                         want[2:5])
    assert same_bits(got[1], want[1]), what + ": v"
    assert same_bits(got[5], want[5]), what + ": the traced sums"
    assert got[3] >= 2, what                                   # more than one round ran


# ---------------------------------------------------------------------------
# 1. no scales = the ones matrix
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", AB)
@pytest.mark.parametrize("dt", DTYPES)
def test_without_scales_rowsum_and_round_are_the_ones_matrix(solver, dt, name, sem):
    indptr, indices = om.structure()
    n = len(indptr) - 1
    _, s, v = om.regime(name, name_of(dt))
    m = values_of(solver, indptr, indices, np.ones(len(indices), dtype=dt), n)
    p = pattern_of(solver, indptr, indices, n, dt)
    assert (np.diff(p.plan()[1]) > 0).all()                    # all four row classes
    assert all(np.array_equal(a, b) for a, b in zip(p.plan(), m.plan()))
    assert p.dtype == tdt(dt) and p.nnz == m.nnz and p.empty_rows == 0
    assert_same(dev.csr_pattern_rowsum(p).cpu().numpy(), dev.csr_rowsum(m).cpu().numpy(),
                "rowsum")
    want = values_round(m, s, v, sem=sem)
    got = pattern_round(p, s, v, sem=sem)
    assert_same(got[0], want[0], "s_next", lens=np.diff(indptr))
    assert_same(got[1], want[1], "v_cur")
    assert_same(got[2], want[2], "z = x")
    assert got[3].tobytes() == want[3].tobytes() and len(got[3]) == 64
    p.close()
    m.close()


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_without_scales_the_solve_is_solve_csr(solver, dt, sem):
    indptr, indices = om.structure()
    n = len(indptr) - 1
    m = values_of(solver, indptr, indices, np.ones(len(indices), dtype=dt), n)
    p = pattern_of(solver, indptr, indices, n, dt)
    got, want = solve_both(solver, p, m, sem)
    assert_same_solve(got, want, "solve")
    p.close()
    m.close()


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("dt", DTYPES)
def test_without_scales_terms_and_emptied_rows_are_solve_csr_terms(solver, dt, K):
    indptr, indices = om.structure()
    n = len(indptr) - 1
    ip, ix, da = tc.empty_rows(indptr, indices, np.ones(len(indices), dtype=dt), [5, 100, n - 1])
    u, w = tc.term_vectors(n, K, 3, dt)
    m = values_of(solver, ip, ix, da, n, allow_empty_rows=True)
    p = pattern_of(solver, ip, ix, n, dt, allow_empty_rows=True)
    assert (p.empty_rows, p.first_empty) == (m.empty_rows, m.first_empty) == (3, 5)
    mt = dev.CsrTerms(m, [up(x) for x in u], [up(x) for x in w], solver=solver)
    pt = dev.CsrTerms(p, [up(x) for x in u], [up(x) for x in w], solver=solver)
    sm, sp = mt.scratch(), dev.csr_pattern_scratch(p, pt)
    assert sm.numel() == sp.numel()
    assert_same(dev.csr_pattern_rowsum(p, pt, sp).cpu().numpy(),
                dev.csr_terms_rowsum(m, mt, sm).cpu().numpy(), "rowsum with terms")
    assert same_bits(pt.dots(sp).cpu().numpy(), mt.dots(sm).cpu().numpy())
    for sem in (_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY):
        got, want = solve_both(solver, p, m, sem, pt, mt)
        assert_same_solve(got, want, f"solve with {K} terms")
    for x in (pt, mt, p, m):
        x.close()


# ---------------------------------------------------------------------------
# 2. power-of-two scales = the scaled values matrix
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("which", ["c", "r", "rc"])
@pytest.mark.parametrize("dt", DTYPES)
def test_power_of_two_scales_are_the_scaled_values_matrix(solver, dt, which, sem):
    indptr, indices = om.structure()
    n = len(indptr) - 1
    _, s, v = om.regime("A", name_of(dt))
    r, c = pm.pow2_scales(n, 77, dt)
    r = r if "r" in which else None
    c = c if "c" in which else None
    m = values_of(solver, indptr, indices, scaled_values(indptr, indices, r, c, dt), n)
    p = pattern_of(solver, indptr, indices, n, dt, r, c)
    assert_same(dev.csr_pattern_rowsum(p).cpu().numpy(), dev.csr_rowsum(m).cpu().numpy(),
                "rowsum", lens=np.diff(indptr))
    want = values_round(m, s, v, sem=sem)
    got = pattern_round(p, s, v, sem=sem)
    assert_same(got[0], want[0], "s_next", lens=np.diff(indptr))
    assert_same(got[1], want[1], "v_cur")
    assert_same(got[2], want[2] if c is None else c * want[2], "z = c x")
    assert got[3].tobytes() == want[3].tobytes()
    got, want = solve_both(solver, p, m, sem, max_itr=40)
    assert_same_solve(got, want, "solve")
    p.close()
    m.close()


# ---------------------------------------------------------------------------
# 3. general scales against the host model
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_case(dtname, wide, K):
    """The scales, the vectors and the model's launch 0 and round, computed
    once and left unchanged."""
    indptr, indices = om.structure()
    n = len(indptr) - 1
    _, s, v = om.regime("B" if wide else "A", dtname)
    x = pm.mul(v, s, dtname)
    r, c = pm.general_scales(n, 5, dtname, wide, x, indices)
    u, w = (tc.term_vectors(n, K, 31, dtname) if K else (None, None))
    return {"r": r, "c": c, "s": s, "v": v, "u": u, "w": w,
            "s0": pm.rowsum(indptr, indices, r, c, dtname, u, w),
            "round": pm.round_(indptr, indices, r, c, s, v, dtname, u, w)}


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("K", [0, 2])
@pytest.mark.parametrize("wide", [pytest.param(False, id="unit"), pytest.param(True, id="wide")])
@pytest.mark.parametrize("dt", DTYPES)
def test_general_scales_are_the_host_model(solver, dt, wide, K, sem):
    indptr, indices = om.structure()
    lens = np.diff(indptr)
    n = len(lens)
    case = general_case(name_of(dt), wide, K)
    mdl = case["round"]
    # a redirected load reads col[0]: its z is the largest, its row one entry long
    assert lens[0] == 1 and int(np.argmax(mdl["z"])) == int(indices[0])
    p = pattern_of(solver, indptr, indices, n, dt, case["r"], case["c"])
    t = None
    if K:
        t = dev.CsrTerms(p, [up(x) for x in case["u"]], [up(x) for x in case["w"]], solver=solver)
    assert_same(dev.csr_pattern_rowsum(p, t).cpu().numpy(), case["s0"], "launch 0", lens=lens)
    s_next, v_cur, z, state, dots = pattern_round(p, case["s"], case["v"], t, sem=sem)
    assert_same(z, mdl["z"], "z")
    if K:
        assert_same(dots, mdl["dots"], "dots (on x, not on z)")
    assert_same(s_next, mdl["s_next"], "s_next", lens=lens)
    assert_same(v_cur, mdl["v_cur"], "v_cur")
    if t is not None:
        t.close()
    p.close()


# ---------------------------------------------------------------------------
# 4. rows stand alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_rows_permuted_keep_their_bits(solver, dt):
    """Row j of the permuted matrix holds the entries of row perm[j] and its
    row scale; the columns, c, and a constant x (s and v constant) stay, so
    that z and every divisor are the same: launch 0 and the round give row j
    what they gave row perm[j], wherever the plan now puts it."""
    indptr, indices = om.structure()
    lens = np.diff(indptr)
    n = len(lens)
    case = general_case(name_of(dt), False, 0)
    r, c = case["r"], case["c"]
    perm = np.random.default_rng(12).permutation(n)
    ip2 = np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.int64)
    ix2 = np.concatenate([indices[indptr[i]:indptr[i + 1]] for i in perm]).astype(np.int32)
    s = np.full(n, 1.5, dtype=dt)
    v = np.full(n, 1.25, dtype=dt)
    p1 = pattern_of(solver, indptr, indices, n, dt, r, c)
    p2 = pattern_of(solver, ip2, ix2, n, dt, r[perm], c)
    assert not np.array_equal(p1.plan()[0], p2.plan()[0])
    a0, b0 = dev.csr_pattern_rowsum(p1).cpu().numpy(), dev.csr_pattern_rowsum(p2).cpu().numpy()
    assert_same(b0, a0[perm], "launch 0", lens=lens[perm])
    a, b = pattern_round(p1, s, v), pattern_round(p2, s, v)
    assert_same(b[0], a[0][perm], "s_next", lens=lens[perm])
    assert_same(b[2], a[2], "z")
    p1.close()
    p2.close()


# ---------------------------------------------------------------------------
# 5. transposition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_transposition_is_the_values_one_with_the_scales_swapped(solver, dt):
    indptr, indices = om.structure()
    n = len(indptr) - 1
    assert n > 256 and _lib.csr_transpose_shape()["digit_bits"] == 8      # two digit passes
    r, c = pm.pow2_scales(n, 78, dt)
    m = values_of(solver, indptr, indices, np.ones(len(indices), dtype=dt), n)
    p = pattern_of(solver, indptr, indices, n, dt, r, c)
    mt, pt = m.transpose(solver), p.transpose(solver)
    assert pt.crow.dtype == torch.int64 and pt.col.dtype == torch.int32
    assert torch.equal(pt.crow, mt.crow) and torch.equal(pt.col, mt.col)
    assert all(np.array_equal(a, b) for a, b in zip(pt.plan(), mt.plan()))
    assert pt.row_scale is p.col_scale and pt.col_scale is p.row_scale
    # the swap as the kernels see it: T(D_r P D_c) = D_c P^T D_r
    direct = pattern_of(solver, mt.crow.cpu().numpy(), mt.col.cpu().numpy(), n, dt, c, r)
    assert_same(dev.csr_pattern_rowsum(pt).cpu().numpy(),
                dev.csr_pattern_rowsum(direct).cpu().numpy(), "rowsum of T")
    mv = values_of(solver, indptr, indices, scaled_values(indptr, indices, r, c, dt), n)
    assert_same(dev.csr_pattern_rowsum(pt).cpu().numpy(),
                dev.csr_rowsum(mv.transpose(solver)).cpu().numpy(), "rowsum of T (values)")
    left = solver.solve_csr_pattern(p, left=True, eps=1e-3, max_itr=40, trace=True)
    sums_left = solver.last_round_sums().copy()
    right = solver.solve_csr_pattern(p.T, eps=1e-3, max_itr=40, trace=True)
    assert left[0] == right[0] and left[2] == right[2] and left[3]["rounds"] >= 2
    assert same_bits(left[1].cpu().numpy(), right[1].cpu().numpy())
    assert same_bits(sums_left, solver.last_round_sums())
    for x in (direct, pt, mt, mv, p, m):
        x.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_an_empty_column_is_refused_by_name_without_allow_empty(solver, dt):
    indptr, indices = om.structure()
    n = len(indptr) - 1
    ix = indices.copy()
    ix[ix == 17] = 3
    ix[ix == 200] = 3
    p = pattern_of(solver, indptr, ix, n, dt)
    with pytest.raises(_lib.EigenValueError, match=r"column 17 has no entry"):
        p.transpose(solver)
    with pytest.raises(_lib.EigenValueError, match=r"column 17 has no entry"):
        solver.solve_csr_pattern(p, left=True)
    t = p.transpose(solver, allow_empty=True)
    assert (t.empty_rows, t.first_empty) == (2, 17)
    m = values_of(solver, indptr, ix, np.ones(len(ix), dtype=dt), n)
    mt = m.transpose(solver, allow_empty=True)
    assert torch.equal(t.crow, mt.crow) and torch.equal(t.col, mt.col)
    with pytest.raises(_lib.EigenValueError, match=r"st_solve_csr_pattern: row 17 is empty"):
        solver.solve_csr_pattern(t)
    # overlap: the outputs must not be the inputs
    out = ctypes.c_void_p(1)
    rc = _lib.load().st_csr_pattern_transpose(solver.q, p.handle, p.crow.data_ptr(),
                                              t.col.data_ptr(), 0, ctypes.byref(out))
    assert rc < 0 and "overlaps the input row_ptr" in _lib.last_error() and not out.value
    for x in (t, mt, m, p):
        x.close()


# ---------------------------------------------------------------------------
# 6. gating
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 2])
@pytest.mark.parametrize("dt", DTYPES)
def test_a_round_beyond_the_end_writes_nothing(solver, dt, K):
    indptr, indices = om.structure()
    n = len(indptr) - 1
    case = general_case(name_of(dt), False, K)
    p = pattern_of(solver, indptr, indices, n, dt, case["r"], case["c"])
    t = None
    if K:
        t = dev.CsrTerms(p, [up(x) for x in case["u"]], [up(x) for x in case["w"]], solver=solver)
    flat = np.full(n, 1.5, dtype=dt)
    state = dev.new_state(DEV)
    s1, v1, z1, b1, _ = pattern_round(p, flat, case["v"], t, k=4, state=state)     # stops
    st = _lib.st_state.from_buffer_copy(b1.tobytes())
    assert st.done == 1 and st.end == 4
    assert not (s1 == SENTINEL).any() and not (z1 == SENTINEL).any()
    for k in (5, 6, 40):
        s2, v2, z2, b2, _ = pattern_round(p, case["s"], case["v"], t, k=k, state=state)
        assert b2.tobytes() == b1.tobytes()
        for got in (s2, v2, z2):
            assert same_bits(got, np.full(n, SENTINEL, dtype=dt))
    if t is not None:
        t.close()
    p.close()


# ---------------------------------------------------------------------------
# 7. PageRank
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,k10,k3", PAGERANK)
@pytest.mark.parametrize("dt,eps", [pytest.param(np.float64, 1e-10, id="f64-1e-10"),
                                    pytest.param(np.float64, 1e-3, id="f64-1e-3"),
                                    pytest.param(np.float32, 1e-3, id="f32-1e-3")])
def test_pagerank_on_a_pattern(solver, dt, eps, n, k10, k3):
    """test_gpu_csr_terms' PageRank cases with `links` a CsrPattern: the same
    round counts and that test's tolerances."""
    A, dang, aPt, G, p_eig = pagerank_reference(n)
    kb, conv, sums, v_m = cc.model(G.astype(dt), eps, True)
    assert conv and kb == (k10 if eps == 1e-10 else k3)
    pi_m = (v_m / v_m.sum()).astype(np.float64)
    ip, ix, da = tc.to_csr(A, dt)
    assert (da == 1).all()
    links = pattern_of(solver, ip, ix, n, dt, allow_empty_rows=True)
    assert links.empty_rows == min(10, n - n // 2)
    pi, lam, it, st = solver.pagerank(links, 0.85, dangling=up(dang.astype(dt)), eps=eps)
    assert it == cc.count_of(kb, conv, True) and st["converged"] == 1
    pi = pi.cpu().numpy().astype(np.float64)
    dist = float(np.abs(pi - p_eig).max())
    print(f"pattern pagerank n = {n} {np.dtype(dt).name} eps {eps:g}: {it} rounds, "
          f"max |pi - eig| {dist:.2e}, max rel to the model "
          f"{float((np.abs(pi - pi_m) / pi_m).max()):.2e}")
    if np.dtype(dt) == np.float64:
        assert (np.abs(pi - pi_m) <= 1e-10 * pi_m).all()
    assert dist <= 10 * eps
    fe = float(np.finfo(dt).eps)
    assert abs(pi.sum() - 1.0) <= n * fe
    assert abs(lam - 1.0) <= n * eps
    # a pattern with scales is not a link graph
    scaled = pattern_of(solver, ip, ix, n, dt, c=np.ones(n, dtype=dt), allow_empty_rows=True)
    with pytest.raises(ValueError, match="without scales"):
        solver.pagerank(scaled)
    scaled.close()
    links.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_pagerank_on_a_pattern_allocates_nothing_of_nnz_values(solver, dt):
    """torch's peak during pagerank(CsrPattern) stays within the two transposed
    index arrays plus 48 vectors of n elements - below those arrays plus one
    tensor of nnz values, which the CsrMatrix route needs three of."""
    n, d = 4096, 128
    rng = np.random.default_rng(3)
    ix = np.concatenate([rng.choice(n, d, replace=False) for _ in range(n)]).astype(np.int32)
    ip = (d * np.arange(n + 1)).astype(np.int64)
    nnz, es = n * d, np.dtype(dt).itemsize
    links = pattern_of(solver, ip, ix, n, dt, allow_empty_rows=True)
    index_bytes = 8 * (n + 1) + 4 * nnz
    allowed = index_bytes + 48 * n * 8
    assert allowed < index_bytes + nnz * es
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pi, lam, it, st = solver.pagerank(links, 0.85, eps=1e-3)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"pattern pagerank n = {n} nnz = {nnz} {np.dtype(dt).name}: peak {extra} bytes over "
          f"the start, allowed {allowed}, one tensor of nnz values {nnz * es}")
    assert extra <= allowed
    assert st["converged"] == 1 and abs(lam - 1.0) <= n * 1e-3
    links.close()


# ---------------------------------------------------------------------------
# 8. validation on the device, cross-refusals
# ---------------------------------------------------------------------------
def test_the_create_names_what_it_found(solver):
    indptr, indices = om.structure()
    n = len(indptr) - 1
    for dt in (np.float32, np.float64):
        r = np.full(n, 0.5, dtype=dt)
        c = np.full(n, 2.0, dtype=dt)
        for val, shown in ((0.0, "0"), (-0.5, "-0.5"), (np.inf, "inf"), (np.nan, "nan")):
            br, bc = r.copy(), c.copy()
            br[200], br[17], bc[3] = val, val, val
            with pytest.raises(_lib.EigenValueError,
                               match=rf"row_scale\[17\] = {shown} is not finite and positive"):
                pattern_of(solver, indptr, indices, n, dt, br, bc)
            with pytest.raises(_lib.EigenValueError, match=rf"col_scale\[3\] = {shown} is not"):
                pattern_of(solver, indptr, indices, n, dt, r, bc)
            with pytest.raises(_lib.EigenValueError, match=rf"col_scale\[3\] = {shown} is not"):
                pattern_of(solver, indptr, indices, n, dt, None, bc)
    bad = indptr.copy()
    bad[31] = bad[30]
    with pytest.raises(_lib.EigenValueError, match=r"row 30 is empty"):
        pattern_of(solver, bad, indices, n, np.float32)
    bad[31] = bad[30] - 1
    with pytest.raises(_lib.EigenValueError, match=r"decreases at row 30"):
        pattern_of(solver, bad, indices, n, np.float32, allow_empty_rows=True)
    ix = indices.copy()
    ix[43] = n
    with pytest.raises(_lib.EigenValueError, match=rf"column index {n} of entry 43"):
        pattern_of(solver, indptr, ix, n, np.float64, np.full(n, -1.0))   # before the scales
    with pytest.raises(TypeError, match="row_scale is torch.float64"):
        dev.CsrPattern(up(indptr), up(indices), n, row_scale=up(np.ones(n)),
                       dtype=torch.float32, solver=solver)


def lib_pattern_solve(solver, handle, terms, n, t):
    """st_solve_csr_pattern through the library alone (no Python check)."""
    L = _lib.load()
    v = torch.full((n,), SENTINEL, dtype=t, device=DEV)
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    rc = L.st_solve_csr_pattern(solver.q, handle, terms, v.data_ptr(), None, ctypes.byref(ev),
                                ctypes.byref(it), None, None)
    return rc, _lib.last_error(L), v.cpu().numpy()


@pytest.mark.parametrize("dt", DTYPES)
def test_the_solve_and_the_two_handle_kinds_refuse_each_other(solver, dt):
    L = _lib.load()
    indptr, indices = om.structure()
    n = len(indptr) - 1
    t = tdt(dt)
    untouched = np.full(n, SENTINEL, dtype=dt)
    p = pattern_of(solver, indptr, indices, n, dt)
    m = values_of(solver, indptr, indices, np.ones(len(indices), dtype=dt), n)
    u, w = tc.term_vectors(n, 1, 3, dt)
    # empty rows without terms
    ip, ix, _ = tc.empty_rows(indptr, indices, np.ones(len(indices)), [9, 30])
    pe = pattern_of(solver, ip, ix, n, dt, allow_empty_rows=True)
    rc, msg, v = lib_pattern_solve(solver, pe.handle, None, n, t)
    assert rc < 0 and "st_solve_csr_pattern: row 9 is empty (2 empty rows" in msg
    assert same_bits(v, untouched)
    with pytest.raises(_lib.EigenValueError, match="st_csr_pattern_round: row 9 is empty"):
        pattern_round(pe, np.ones(n, dtype=dt), np.ones(n, dtype=dt))
    # terms of another pattern handle, of a values handle, and pattern terms in a values call
    te = dev.CsrTerms(pe, [up(x) for x in u], [up(x) for x in w], solver=solver)
    tm = dev.CsrTerms(m, [up(x) for x in u], [up(x) for x in w], solver=solver)
    tp = dev.CsrTerms(p, [up(x) for x in u], [up(x) for x in w], solver=solver)
    for terms in (te, tm):
        rc, msg, v = lib_pattern_solve(solver, p.handle, terms.handle, n, t)
        assert rc < 0 and "belongs to another handle" in msg and same_bits(v, untouched)
    with pytest.raises(ValueError, match="terms were made for another matrix"):
        solver.solve_csr_pattern(p, te)
    v = torch.full((n,), SENTINEL, dtype=t, device=DEV)
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    rc = L.st_solve_csr_terms(solver.q, m.handle, tp.handle, v.data_ptr(), None,
                              ctypes.byref(ev), ctypes.byref(it), None, None)
    assert rc < 0 and "belongs to another matrix handle" in _lib.last_error(L)
    assert same_bits(v.cpu().numpy(), untouched)
    # a pattern handle in the values calls
    rc = L.st_solve_csr(solver.q, p.handle, v.data_ptr(), None, ctypes.byref(ev),
                        ctypes.byref(it), None, None)
    assert rc < 0 and "st_solve_csr: not a CSR matrix handle" in _lib.last_error(L)
    x = torch.ones(n, dtype=t, device=DEV)
    rc = L.st_csr_apply(p.handle, x.data_ptr(), v.data_ptr(), None)
    assert rc < 0 and "not a CSR matrix handle" in _lib.last_error(L)
    for b, a in ((p, m), (m, p)):
        rc = L.st_solve_csr_product(solver.q, b.handle, a.handle, v.data_ptr(), None,
                                    ctypes.byref(ev), ctypes.byref(it), None, None)
        assert rc < 0 and "not a CSR matrix handle" in _lib.last_error(L)
    out = ctypes.c_void_p(1)
    pu = (ctypes.c_void_p * 1)(up(u[0]).data_ptr())
    rc = L.st_csr_multi_create(solver.q, p.handle, 1, 1, pu, pu, ctypes.byref(out))
    assert rc < 0 and "not a CSR matrix handle" in _lib.last_error(L) and not out.value
    torch.cuda.synchronize()
    assert same_bits(v.cpu().numpy(), untouched)
    # a values handle in the pattern calls
    rc, msg, v2 = lib_pattern_solve(solver, m.handle, None, n, t)
    assert rc < 0 and "st_solve_csr_pattern: not a CSR pattern handle" in msg
    assert same_bits(v2, untouched)
    out = ctypes.c_void_p(1)
    rc = L.st_csr_pattern_terms_create(solver.q, m.handle, 1, pu, pu, ctypes.byref(out))
    assert rc < 0 and "not a CSR pattern handle" in _lib.last_error(L) and not out.value
    with pytest.raises(TypeError, match="a CsrPattern required"):
        solver.solve_csr_pattern(m)
    with pytest.raises(TypeError, match="a CsrMatrix required"):
        solver.solve_csr(p)
    for x in (te, tm, tp, pe, p, m):
        x.close()


# ---------------------------------------------------------------------------
# 9. input forms and determinism
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_numpy_scipy_and_torch_inputs_give_the_same_bytes(solver, dt):
    import scipy.sparse as sp
    from eigen_value_amd.similarity_transform import EigenValue
    indptr, indices = om.structure()
    n = len(indptr) - 1
    r, c = pm.general_scales(n, 5, dt, False, np.ones(n), indices)
    data = np.random.default_rng(4).random(len(indices)).astype(dt) + 0.5   # ignored
    with EigenValue() as ev:
        kw = dict(row_scale=r, col_scale=c, eps=1e-3, max_itr=40)
        a = ev.similarity_transform_csr_pattern(indptr, indices, **kw)
        b = ev.similarity_transform_csr_pattern(indptr, indices, n, **kw)
        # scipy sums duplicates when it converts, so it is given its CSR arrays as they are
        m = sp.csr_matrix((data, indices, indptr), shape=(n, n))
        s = ev.similarity_transform_csr_pattern(m, **kw)
        tcsr = torch.sparse_csr_tensor(torch.from_numpy(np.array(indptr)),
                                       torch.from_numpy(indices.astype(np.int64)),
                                       torch.from_numpy(data), size=(n, n))
        t = ev.similarity_transform_csr_pattern(tcsr, **kw)
    p = pattern_of(solver, indptr, indices, n, dt, r, c)
    lam, v, it, st = solver.solve_csr_pattern(p, eps=1e-3, max_itr=40)
    assert a[1].dtype == np.dtype(dt) and st["rounds"] >= 2
    for other in (b, s, t):
        assert a[0] == other[0] and a[3] == other[3] and same_bits(a[1], other[1])
    assert float(a[0]) == lam and a[3] == it and same_bits(a[1], v.cpu().numpy())
    p.close()
