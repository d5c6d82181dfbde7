"""GPU: the stable device transposition of a CSR matrix (st_csr_transpose) and
the left Perron vector through it.

1  device T(A) == the host twin, exactly, at every digit-pass boundary of n
   and every tile boundary of nnz (both read from st_csr_transpose_shape_desc)
2  stability across tiles (columns of thousands of entries spread over the
   whole array) and with duplicates; twice in one process, identical bytes
3  solve_csr(left=True) == solve_csr on the host-transposed arrays, bit for
   bit, through every front; the eigenvalue bracketed by the last sums
4  a Markov chain: the right solve says nothing, the left one is the
   stationary distribution's
5  errors on the device path
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
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from eigen_value_amd.similarity_transform import EigenValue  # noqa: E402
from test_gpu_csr import spectral_radius  # noqa: E402  (one rho per case, cached there)

DEV = "cuda:0"
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
SEMS = [pytest.param(_lib.ST_SEM_SYCL, id="sycl"), pytest.param(_lib.ST_SEM_MAINPY, id="mainpy")]
SHAPE = _lib.csr_transpose_shape()
D, TILE = 1 << SHAPE["digit_bits"], SHAPE["tile"]


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


def arrays(m):
    return m.crow.cpu().numpy(), m.col.cpu().numpy(), m.values.cpu().numpy()


def same(got, want):
    return all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def table_case(i):
    n, d, seed, heavy = cc.TABLE[i]
    return (n,) + cc.make_csr(n, d, seed, cc.class_heavy(n) if heavy else None)


@functools.lru_cache(maxsize=None)
def table_transposed(i, dt):
    """(n, host T(A) of case i with fp32-valued data in dtype dt)."""
    n, ip, ix, da = table_case(i)
    return (n,) + dev.csr_transpose_host(ip, ix, da.astype(np.float32).astype(dt))


def perm_plus(n, lens, seed):
    """Rows of lens[r] entries: the first from a permutation of 0 .. n-1 (no
    column stays empty), the rest from integers(0, n); values in (0, 1]."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ix = rng.integers(0, n, size=int(ip[-1])).astype(np.int32)
    ix[ip[:-1]] = rng.permutation(n).astype(np.int32)
    return ip, ix, 1.0 - rng.random(int(ip[-1]))


def check_against_twin(solver, ip, ix, da):
    m = csr_of(solver, ip, ix, da)
    t = m.transpose(solver)
    want = dev.csr_transpose_host(ip, ix, da)
    assert same(arrays(t), want)
    assert t.n == m.n and t.nnz == m.nnz and t.dtype == m.dtype
    # the handle is of st_csr_create's grade: its plan is the host plan
    order, first = t.plan()
    o, f, _ = _lib.csr_plan(want[0])
    assert np.array_equal(order, o) and np.array_equal(first, f)
    t.close()
    m.close()


# ---------------------------------------------------------------------------
# 1. digit-pass and tile boundaries
# ---------------------------------------------------------------------------
def test_the_shape_is_what_the_cases_assume():
    assert D >= 2 and TILE >= 64
    assert 3 * (D * D + 1) < 200_000, "the largest case must stay small"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [1, 2, D - 1, D, D + 1, D * D - 1, D * D, D * D + 1])
def test_digit_pass_boundaries(solver, n, dt):
    ip, ix, da = perm_plus(n, np.full(n, 3), seed=n)
    assert np.bincount(ix, minlength=n).min() >= 1
    check_against_twin(solver, ip, ix, da.astype(dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nnz", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_tile_boundaries(solver, nnz, dt):
    n = 100
    lens = np.full(n, nnz // n)
    lens[:nnz % n] += 1
    ip, ix, da = perm_plus(n, lens, seed=nnz)
    assert ip[-1] == nnz
    check_against_twin(solver, ip, ix, da.astype(dt))


# ---------------------------------------------------------------------------
# 2. stability
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_stability_across_tiles(solver, dt):
    """The input is T(TABLE[2]): its column 9 holds 3000 entries and column 7
    holds 2049, one per row, spread over the whole array.  TABLE[2] has sorted
    columns and no duplicates, so the device result is TABLE[2] itself."""
    n, ip, ix, da = table_case(2)
    da = da.astype(dt)
    tp, ti, tv = dev.csr_transpose_host(ip, ix, da)
    counts = np.bincount(ti, minlength=n)
    assert counts[9] == 3000 and counts[7] == 2049 and len(ti) > 4 * TILE
    m = csr_of(solver, tp, ti, tv, n)
    t = m.transpose(solver)
    assert same(arrays(t), (ip, ix, da))
    order, first = t.plan()
    o, f, used = _lib.csr_plan(ip)
    assert np.array_equal(order, o) and np.array_equal(first, f) and used == 4
    assert (np.diff(first) > 0).all()


def dup_row():
    ip = [0, 2, 8, 10, 12]
    ix = [0, 3, 2, 2, 1, 2, 2, 2, 1, 3, 0, 2]
    return np.array(ip, np.int64), np.array(ix, np.int32), np.arange(1.0, 13.0)


def two_columns(n=3 * TILE // 4 + 5):
    """Every entry in column 0 or column n - 1, plus a permutation: two columns
    that each span several tiles."""
    rng = np.random.default_rng(21)
    ends = np.where(rng.random((n, 5)) < 0.5, 0, n - 1).astype(np.int32)
    ix = np.concatenate([rng.permutation(n).astype(np.int32)[:, None], ends], axis=1).ravel()
    ip = np.arange(0, 6 * n + 1, 6, dtype=np.int64)
    return ip, ix, 1.0 - rng.random(6 * n)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("make", [dup_row, two_columns], ids=["five_fold", "two_columns"])
def test_stability_with_duplicates(solver, make, dt):
    ip, ix, da = make()
    da = da.astype(dt)
    want = dev.csr_transpose_host(ip, ix, da)
    m = csr_of(solver, ip, ix, da)
    a = m.transpose(solver)
    b = m.transpose(solver)
    assert same(arrays(a), arrays(b))
    assert same(arrays(a), want)
    if make is dup_row:
        lo, hi = want[0][2], want[0][3]
        assert arrays(a)[2][lo:hi].tolist() == [3.0, 4.0, 6.0, 7.0, 8.0, 12.0]


# ---------------------------------------------------------------------------
# 3. the solve
# ---------------------------------------------------------------------------
def result(r):
    lam, v, it, st = r
    return lam, v.cpu().numpy().tobytes(), it, st["rounds"], st["converged"]


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", range(len(cc.TABLE)))
def test_left_solve_is_the_solve_of_the_host_transposed_matrix(solver, case, dt, sem):
    n, ip, ix, da = table_case(case)
    m = csr_of(solver, ip, ix, da.astype(np.float32).astype(dt), n)
    ref = csr_of(solver, *table_transposed(case, dt)[1:], n)
    got = solver.solve_csr(m, left=True, semantics=sem)
    want = solver.solve_csr(ref, semantics=sem)
    assert result(got) == result(want)
    assert got[1].dtype == m.dtype and got[1].numel() == n
    # left=False is what it was
    assert result(solver.solve_csr(m, left=False, semantics=sem)) == \
        result(solver.solve_csr(m, semantics=sem))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", range(len(cc.TABLE)))
def test_left_solve_through_the_host_fronts(solver, case, dt):
    """EigenValue.similarity_transform_csr(left=True) in its three input forms -
    arrays, scipy.sparse, torch.sparse_csr - and max_eigen_value_csr_left_ex
    itself, with its stats."""
    sp = pytest.importorskip("scipy.sparse")
    n, ip, ix, da = table_case(case)
    da = da.astype(np.float32).astype(dt)
    want = solver.solve_csr(csr_of(solver, *table_transposed(case, dt)[1:], n))
    with EigenValue() as ev:
        r1 = ev.similarity_transform_csr(ip, ix, da, left=True)
        r2 = ev.similarity_transform_csr(sp.csr_matrix((da, ix, ip), shape=(n, n)), left=True)
        r3 = ev.similarity_transform_csr(
            torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)),
                                    torch.from_numpy(da), size=(n, n)), left=True)
        right = ev.similarity_transform_csr(ip, ix, da)
    for r in (r1, r2, r3):
        assert r[0] == want[0] and r[3] == want[2] and r[0].dtype == np.dtype(dt)
        assert r[1].tobytes() == want[1].cpu().numpy().tobytes()
    assert right[1].tobytes() != r1[1].tobytes()
    L = _lib.load()
    lam = np.zeros(1, dt)
    vec = np.zeros(n, dt)
    it = ctypes.c_uint32()
    stats = _lib.st_stats()
    rc = L.max_eigen_value_csr_left_ex(solver.q, 1 if np.dtype(dt) == np.float64 else 0, n,
                                       len(da), ip.ctypes.data, ix.ctypes.data, da.ctypes.data,
                                       lam.ctypes.data, vec.ctypes.data, ctypes.byref(it), None,
                                       ctypes.byref(stats))
    _lib.check(rc, "max_eigen_value_csr_left_ex", L)
    assert (float(lam[0]), vec.tobytes(), it.value) == \
        (want[0], want[1].cpu().numpy().tobytes(), want[2])
    assert (stats.rounds, stats.converged) == (want[3]["rounds"], want[3]["converged"])
    assert stats.transpose_us > 0 and stats.loop_ms > 0 and stats.h2d_ms > 0


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", range(len(cc.TABLE)))
def test_left_and_right_sums_bracket_the_spectral_radius(solver, dt, case):
    """Collatz-Wielandt for A and for its transpose, which share rho; the slack
    of test_the_eigenvalue_is_bracketed_by_the_last_sums."""
    n, ip, ix, da = table_case(case)
    m = csr_of(solver, ip, ix, da.astype(np.float32).astype(dt), n)
    rho = spectral_radius(case)
    slack = 4 * float(np.finfo(dt).eps) * rho
    for left in (False, True):
        lam, v, it, st = solver.solve_csr(m, trace=True, left=left)
        sums = solver.last_round_sums()
        assert sums.shape == (st["rounds"], n) and sums.dtype == np.dtype(dt)
        s = sums[-1].astype(np.float64)
        print(f"case {case} left={left}: {s.min()!r} <= {rho!r} <= {s.max()!r}")
        assert s.min() - slack <= rho <= s.max() + slack, (left, s.min(), rho, s.max())
        assert lam == float(sums[-1][0])


# ---------------------------------------------------------------------------
# 4. a Markov chain
# ---------------------------------------------------------------------------
def test_markov_chain(solver):
    """P = TABLE[0] with every row divided by its sum (fp64).  P 1 = 1: the
    right solve stops at once with v = 1.  pi P = pi: the left solve is the
    solve of the host-transposed P, and its last sums bracket 1."""
    n, ip, ix, da = table_case(0)
    rows = np.repeat(np.arange(n), np.diff(ip))
    p = da / np.add.reduceat(da, ip[:-1])[rows]
    m = csr_of(solver, ip, ix, p, n)
    lam, v, it, st = solver.solve_csr(m)
    assert st["converged"] == 1 and abs(lam - 1.0) < 1e-3
    assert (np.abs(v.cpu().numpy() - 1.0) < 1e-3).all()          # the stop rule's eps
    ref = csr_of(solver, *dev.csr_transpose_host(ip, ix, p), n)
    got = solver.solve_csr(m, left=True, trace=True)
    sums = solver.last_round_sums()
    want = solver.solve_csr(ref)
    assert result(got) == result(want) and got[3]["converged"] == 1
    s = sums[-1]
    slack = 4 * float(np.finfo(np.float64).eps)
    assert s.min() - slack <= 1.0 <= s.max() + slack, (s.min(), s.max())
    pi = got[1].cpu().numpy()
    pi = pi / pi.sum()
    assert pi.min() > 0 and np.abs(pi @ cc.densify(ip, ix, p) - pi).max() < 1e-3
    assert not (np.abs(pi * n - 1.0) < 1e-6).all()                # not the uniform vector


# ---------------------------------------------------------------------------
# 5. errors on the device path
# ---------------------------------------------------------------------------
def test_an_empty_column_is_named_and_leaves_no_handle(solver):
    n, ip, ix, da = table_case(0)
    bad = ix.copy()
    bad[(bad == 17) | (bad == 40)] = 3
    m = csr_of(solver, ip, bad, da, n)
    with pytest.raises(_lib.EigenValueError, match=r"column 17 has no entry"):
        m.transpose(solver)
    with pytest.raises(_lib.EigenValueError, match=r"column 17 has no entry"):
        m.T
    assert m._t is None
    with pytest.raises(_lib.EigenValueError, match=r"column 17 has no entry"):
        solver.solve_csr(m, left=True)
    L = _lib.load()
    t = [torch.empty(n + 1, dtype=torch.int64, device=DEV),
         torch.empty(m.nnz, dtype=torch.int32, device=DEV),
         torch.empty(m.nnz, dtype=torch.float64, device=DEV)]
    out = ctypes.c_void_p(1)
    assert L.st_csr_transpose(solver.q, m.handle, t[0].data_ptr(), t[1].data_ptr(),
                              t[2].data_ptr(), ctypes.byref(out)) < 0
    assert "column 17 has no entry" in _lib.last_error(L) and not out.value
    # the right solve and the solver are as good as before
    assert solver.solve_csr(m)[3]["converged"] == 1


def test_aliasing_and_foreign_handles_are_refused(solver):
    n, ip, ix, da = table_case(0)
    m = csr_of(solver, ip, ix, da, n)
    L = _lib.load()
    t = [torch.empty(n + 1, dtype=torch.int64, device=DEV),
         torch.empty(m.nnz, dtype=torch.int32, device=DEV),
         torch.empty(m.nnz, dtype=torch.float64, device=DEV)]
    ptr = [x.data_ptr() for x in t]
    out = ctypes.c_void_p(1)

    def call(handle, p):
        rc = L.st_csr_transpose(solver.q, handle, p[0], p[1], p[2], ctypes.byref(out))
        return rc, _lib.last_error(L)
    for i, inp in enumerate((m.crow, m.col, m.values)):          # an output IS an input
        p = list(ptr)
        p[i] = inp.data_ptr()
        rc, msg = call(m.handle, p)
        assert rc < 0 and "overlaps the input" in msg and not out.value
    rc, msg = call(m.handle, [ptr[0], ptr[1], m.values.data_ptr() + 8 * (m.nnz - 1)])
    assert rc < 0 and "overlaps the input vals" in msg            # by range, not by start
    rc, msg = call(m.handle, [ptr[0], ptr[1], ptr[1]])
    assert rc < 0 and "outputs" in msg and "overlap" in msg
    rc, msg = call(m.handle, [ptr[0], None, ptr[2]])
    assert rc < 0 and "null" in msg
    # a batch handle is no matrix handle
    trip = (up(ip), up(ix), up(da))
    b = dev.CsrBatch.from_matrices([trip, trip], solver=solver)
    rc, msg = call(b.handle, ptr)
    assert rc < 0 and "not a CSR matrix handle" in msg
    # ... and a transposed handle is refused by the batch calls, as any matrix handle
    tm = m.transpose(solver)
    assert L.st_csr_batch_rowsum(tm.handle, ptr[2], None) < 0
    assert "handle" in _lib.last_error(L)
    rc, msg = call(m.handle, ptr)                                  # and a good call still works
    assert rc == 0 and out.value
    assert L.st_csr_destroy(out) == 0
    b.close()


def test_T_is_cached_and_closed_with_its_parent(solver):
    n, ip, ix, da = table_case(0)
    m = csr_of(solver, ip, ix, da, n)
    t = m.T
    assert m.T is t and t.handle.value
    assert same(arrays(t), dev.csr_transpose_host(ip, ix, da))
    assert m.transpose(solver) is not t                            # transpose() is a new matrix
    m.close()
    assert not t.handle.value and not m.handle.value and m._t is None
    with pytest.raises(ValueError, match="closed"):
        m.transpose(solver)
