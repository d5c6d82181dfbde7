"""GPU: the batched sparse (stacked CSR) solve - st_csr_batch_rowsum /
st_csr_batch_mfree_round / st_solve_csr_batched.

1  bit-identity with st_solve_csr on every matrix alone (device, host twin /
   EigenValue, reversed order)
2  the steps equal the single steps after every launch; finished counts the ends
3  a matrix is frozen after its stop
4  the stop test and the max at the boundaries of each matrix's own slice
5  the plan is st_csr_plan of the stacked row_ptr
6  the eigenvalue itself; 7 determinism; 8 validation on the device

The reference batch (12 matrices, N = 5210 stacked rows, max_itr = 50) has
ends of both parities, a stop in round 0 (a circulant) and a matrix that
exhausts max_itr (a reducible one); the assertions are against the single
solve, not against a model.
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
import stats_vectors as sv  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from eigen_value_amd.similarity_transform import EigenValue  # noqa: E402

DEV = "cuda:0"
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
SEMS = [pytest.param(_lib.ST_SEM_SYCL, id="sycl"), pytest.param(_lib.ST_SEM_MAINPY, id="mainpy")]
MAX_ITR = 50
SEEDED = [(1, 1, 3), (2, 2, 3), (5, 3, 3), (64, 8, 7), (255, 4, 5), (256, 16, 5), (257, 40, 5),
          (300, 8, 9), (1000, 3, 2)]


def tdt(dt):
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def circulant(n=40):
    r = np.arange(n)
    cols = np.stack([r, (r + 1) % n, (r + 5) % n], axis=1).reshape(-1).astype(np.int32)
    vals = np.tile(np.array([0.5, 0.25, 0.125]), n)
    return 3 * np.arange(n + 1, dtype=np.int64), cols, vals


def reducible():
    ip, ix, da = cc.make_csr(30, 4, 1)
    k = int(ip[1])                       # row 0 -> its diagonal alone
    return (np.concatenate([[0], ip[1:] - k + 1]).astype(np.int64),
            np.concatenate([[0], ix[k:]]).astype(np.int32), np.concatenate([[1.0], da[k:]]))


@functools.lru_cache(maxsize=None)
def reference_batch():
    """[(indptr, indices, data fp64)]: the nine seeded matrices, the TABLE
    matrix with all four classes between small ones, the circulant, the
    reducible one."""
    m = [cc.make_csr(n, d, seed) for n, d, seed in SEEDED]
    n, d, seed, heavy = cc.TABLE[2]
    assert (n, d, seed, heavy) == (3000, 32, 7, True)
    big = cc.make_csr(n, d, seed, cc.class_heavy(n))
    return [m[0], m[1], m[2], big, m[3], circulant(), m[4], m[5], m[6], reducible(), m[7], m[8]]


def stacked(mats, dt):
    """(mat_first, row_ptr, col, vals in dt) of a list of host matrices."""
    mat_first = np.concatenate([[0], np.cumsum([len(m[0]) - 1 for m in mats])]).astype(np.uint32)
    ptrs, base = [np.zeros(1, np.int64)], 0
    for ip, _, _ in mats:
        ptrs.append(ip[1:] + base)
        base += int(ip[-1])
    return (mat_first, np.concatenate(ptrs), np.concatenate([m[1] for m in mats]),
            np.concatenate([m[2] for m in mats]).astype(dt))


def batch_of(solver, mats, dt):
    mf, rp, col, vals = stacked(mats, dt)
    return dev.CsrBatch(up(rp), up(col), up(vals), mf, solver=solver)


def single_of(solver, m, dt):
    ip, ix, da = m
    return dev.CsrMatrix(up(ip), up(ix), up(da.astype(dt)), len(ip) - 1, solver=solver)


_SINGLES = {}


def singles(solver, dt, sem):
    """solve_csr of every reference matrix alone: [(lam, v numpy, it, stats)],
    computed once per (dtype, semantics) and left unchanged."""
    key = (np.dtype(dt).name, sem)
    if key not in _SINGLES:
        out = []
        for m in reference_batch():
            lam, v, it, st = solver.solve_csr(single_of(solver, m, dt), max_itr=MAX_ITR,
                                              semantics=sem)
            out.append((np.dtype(dt).type(lam), v.cpu().numpy(), it, st))
        _SINGLES[key] = out
    return _SINGLES[key]


def assert_same_as_singles(ref, order, mf, lam, v, its, conv):
    for j, b in enumerate(order):
        r_lam, r_v, r_it, r_st = ref[b]
        assert lam[j].tobytes() == r_lam.tobytes(), (j, b, lam[j], r_lam)
        assert int(its[j]) == r_it and int(conv[j]) == r_st["converged"], (j, b)
        assert np.array_equal(v[int(mf[j]):int(mf[j + 1])], r_v), (j, b)


# ---------------------------------------------------------------------------
# 1. bit-identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_batched_solve_is_the_single_solve_bit_for_bit(solver, dt, sem):
    mats = reference_batch()
    ref = singles(solver, dt, sem)
    B = len(mats)
    bt = batch_of(solver, mats, dt)
    lam, v, its, conv, st = solver.solve_csr_batched(bt, max_itr=MAX_ITR, semantics=sem)
    assert lam.dtype == np.dtype(dt) and v.dtype == tdt(dt) and v.numel() == bt.n
    assert_same_as_singles(ref, range(B), bt.mat_first, lam, v.cpu().numpy(), its, conv)
    ends = [r[3]["rounds"] for r in ref]
    print("rounds evaluated per matrix:", ends, "converged:", [int(c) for c in conv])
    # the spread the batch is there for
    assert {e & 1 for e in ends} == {0, 1} and 1 in ends and MAX_ITR in ends
    assert [int(c) for c in conv].count(0) == 1 and int(conv[9]) == 0
    assert st["rounds"] == max(ends) == MAX_ITR and st["converged"] == 0
    assert st["fused_launches"] == MAX_ITR
    # reversed order: reversed results
    rev = list(range(B))[::-1]
    bt_r = batch_of(solver, [mats[b] for b in rev], dt)
    lam_r, v_r, its_r, conv_r, _ = solver.solve_csr_batched(bt_r, max_itr=MAX_ITR, semantics=sem)
    assert_same_as_singles(ref, rev, bt_r.mat_first, lam_r, v_r.cpu().numpy(), its_r, conv_r)
    # built on the device from the single matrices
    bt_m = dev.CsrBatch.from_matrices([(up(ip), up(ix), up(da.astype(dt))) for ip, ix, da in mats],
                                      solver=solver)
    assert np.array_equal(bt_m.mat_first, bt.mat_first) and torch.equal(bt_m.crow, bt.crow)
    lam_m, v_m, its_m, conv_m, _ = solver.solve_csr_batched(bt_m, max_itr=MAX_ITR, semantics=sem)
    assert lam_m.tobytes() == lam.tobytes() and torch.equal(v_m, v)
    assert np.array_equal(its_m, its) and np.array_equal(conv_m, conv)
    # a batch without the exhausted matrix converges as a whole, earlier
    conv_only = [b for b in range(B) if b != 9]
    bt_c = batch_of(solver, [mats[b] for b in conv_only], dt)
    lam_c, v_c, its_c, conv_c, st_c = solver.solve_csr_batched(bt_c, max_itr=MAX_ITR,
                                                               semantics=sem, batch_rounds=3)
    assert_same_as_singles(ref, conv_only, bt_c.mat_first, lam_c, v_c.cpu().numpy(), its_c, conv_c)
    assert st_c["converged"] == 1 and st_c["rounds"] == max(ends[b] for b in conv_only)
    assert st_c["rounds"] <= st_c["fused_launches"] < MAX_ITR
    for h in (bt, bt_r, bt_m, bt_c):
        h.close()


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_host_twin_through_eigenvalue(solver, dt, sem):
    mats = [(ip, ix, da.astype(dt)) for ip, ix, da in reference_batch()]
    ref = singles(solver, dt, sem)
    with EigenValue() as ev:
        lam, vs, ts, its = ev.similarity_transform_csr_batched(mats, max_itr=MAX_ITR,
                                                               semantics=sem)
        assert lam.dtype == np.dtype(dt) and len(vs) == len(mats) and its.dtype == np.uint32
        for b, (r_lam, r_v, r_it, _) in enumerate(ref):
            assert lam[b].tobytes() == r_lam.tobytes() and int(its[b]) == r_it, b
            assert vs[b].dtype == np.dtype(dt) and np.array_equal(vs[b], r_v), b
        # the other input forms, on a few of them
        few = [4, 5, 0]
        forms = [torch.sparse_csr_tensor(torch.from_numpy(mats[b][0]),
                                         torch.from_numpy(mats[b][1].astype(np.int64)),
                                         torch.from_numpy(mats[b][2]),
                                         size=(len(mats[b][0]) - 1,) * 2) for b in few]
        lam_t, vs_t, _, its_t = ev.similarity_transform_csr_batched(forms, max_itr=MAX_ITR,
                                                                    semantics=sem)
        for j, b in enumerate(few):
            assert lam_t[j].tobytes() == ref[b][0].tobytes() and int(its_t[j]) == ref[b][2]
            assert np.array_equal(vs_t[j], ref[b][1])
        lam_e, vs_e, ts_e, its_e = ev.similarity_transform_csr_batched([])
        assert lam_e.shape == (0,) and vs_e == [] and its_e.shape == (0,)


def test_scipy_matrices_through_eigenvalue(solver):
    sp = pytest.importorskip("scipy.sparse")     # the scipy form is optional, as in test_gpu_csr
    mats = reference_batch()
    ref = singles(solver, np.float64, _lib.ST_SEM_SYCL)
    few = [4, 5, 0, 3]
    forms = [sp.csr_matrix((mats[b][2], mats[b][1], mats[b][0]),
                           shape=(len(mats[b][0]) - 1,) * 2) for b in few]
    with EigenValue() as ev:
        lam, vs, _, its = ev.similarity_transform_csr_batched(forms, max_itr=MAX_ITR)
    for j, b in enumerate(few):
        assert lam[j].tobytes() == ref[b][0].tobytes() and int(its[j]) == ref[b][2]
        assert np.array_equal(vs[j], ref[b][1])


# ---------------------------------------------------------------------------
# 2, 3. the steps, after every launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_steps_equal_the_single_steps_and_a_stopped_matrix_is_frozen(solver, dt, sem, order):
    """The batch on its buffers, and every matrix alone on its own slices of a
    second set of buffers with a state of its own: after every launch the
    five vectors and all B states are equal bytes; finished counts the states
    with end != 0; and once a matrix has ended, its slices of s (both), v
    (both) and x never change again.  Reversed, the batch starts with its
    1000-row matrix and ends with the one of a single row: entry 0, to which
    loads past a row's end are redirected, then holds a column far beyond the
    last matrix's size, and x is exactly N elements long."""
    perm = list(range(len(reference_batch())))
    if order == "reversed":
        perm = perm[::-1]
        assert len(reference_batch()[perm[0]][0]) - 1 == 1000 and reference_batch()[perm[0]][1][0] > 1
        assert len(reference_batch()[perm[-1]][0]) - 1 == 1
    mats = [reference_batch()[b] for b in perm]
    B = len(mats)
    bt = batch_of(solver, mats, dt)
    one = [single_of(solver, m, dt) for m in mats]
    mf = [int(x) for x in bt.mat_first]
    N, t = bt.n, tdt(dt)

    def buffers():
        s = [torch.full((N,), -1.0, dtype=t, device=DEV) for _ in range(2)]
        v = [torch.ones(N, dtype=t, device=DEV), torch.full((N,), -1.0, dtype=t, device=DEV)]
        return s, v, torch.full((N,), -1.0, dtype=t, device=DEV)

    (s_b, v_b, x_b), (s_1, v_1, x_1) = buffers(), buffers()
    st_b = torch.zeros((B, 64), dtype=torch.uint8, device=DEV)
    st_1 = torch.zeros((B, 64), dtype=torch.uint8, device=DEV)
    fin = torch.zeros(1, dtype=torch.int32, device=DEV)
    dev.csr_batch_rowsum(bt, out=s_b[0])
    for b in range(B):
        dev.csr_rowsum(one[b], out=s_1[0][mf[b]:mf[b + 1]])
    assert torch.equal(s_b[0], s_1[0])
    frozen = {}                                   # b -> its slices when it ended
    seen_ends = []
    for k in range(1, MAX_ITR + 1):
        p, c = (k - 1) & 1, k & 1
        dev.csr_batch_mfree_round(bt, s_b[p], s_b[c], v_b[p], v_b[c], x_b, st_b, fin, eps=1e-3,
                                  k=k, max_itr=MAX_ITR, semantics=sem)
        for b in range(B):
            lo, hi = mf[b], mf[b + 1]
            dev.csr_mfree_round(one[b], s_1[p][lo:hi], s_1[c][lo:hi], v_1[p][lo:hi],
                                v_1[c][lo:hi], x_1[lo:hi], st_1[b], eps=1e-3, k=k,
                                max_itr=MAX_ITR, semantics=sem)
        got = [a.cpu().numpy() for a in (s_b[0], s_b[1], v_b[0], v_b[1], x_b)]
        want = [a.cpu().numpy() for a in (s_1[0], s_1[1], v_1[0], v_1[1], x_1)]
        for name, g, w in zip(("s0", "s1", "v0", "v1", "x"), got, want):
            assert g.tobytes() == w.tobytes(), (k, name, np.flatnonzero(g != w)[:4])
        sb, s1 = st_b.cpu().numpy(), st_1.cpu().numpy()
        assert sb.tobytes() == s1.tobytes(), (k, [b for b in range(B) if (sb[b] != s1[b]).any()])
        ends = [_lib.st_state.from_buffer_copy(sb[b].tobytes()).end for b in range(B)]
        assert int(fin.item()) == sum(e != 0 for e in ends), (k, ends)
        for b in range(B):
            lo, hi = mf[b], mf[b + 1]
            if ends[b] != 0 and b not in frozen:
                assert ends[b] == k
                frozen[b] = [g[lo:hi].copy() for g in got]
            elif b in frozen:
                for name, g, f in zip(("s0", "s1", "v0", "v1", "x"), got, frozen[b]):
                    assert g[lo:hi].tobytes() == f.tobytes(), (k, b, name)
        seen_ends = ends
    assert all(e != 0 for e in seen_ends) and int(fin.item()) == B
    ref = [singles(solver, dt, sem)[b] for b in perm]
    assert seen_ends == [r[3]["rounds"] for r in ref]
    for b in range(B):                            # and the steps are the solve
        assert np.array_equal(frozen[b][2 + (seen_ends[b] & 1)], ref[b][1]), b
    bt.close()


# ---------------------------------------------------------------------------
# 4. the stop test and the max at the boundaries of each matrix's slice
# ---------------------------------------------------------------------------
DIAG_SIZES = [1, 255, 256, 257, 1, 513, 2, 64, 65]


def expect_state(s, eps, sem, k, max_itr):
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
    return e


def one_pair(n, p, dt, cyclic):
    """A vector of n elements whose pair starting at p (p = n - 1: the wrap
    pair n - 1 -> 0) is the only one that differs by eps or more - where such
    a vector exists: sv.one_fail's ramp needs n >= 9 for the cyclic form, the
    open form is a step.  For n = 2 the two cyclic pairs are one difference."""
    if p == n - 1 or (cyclic and n >= 9):
        if n >= 9:
            return sv.one_fail(n, p, dt, sv.EPS, True)
        s = np.ones(n, dtype=dt)            # n = 2: [1, 1 + 4 eps]
        s[n - 1] += 4 * sv.EPS
        return s
    return sv.one_fail(n, p, dt, sv.EPS, False)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_stop_and_max_at_the_boundaries_of_every_matrix(solver, dt, sem):
    cyclic = sem == _lib.ST_SEM_SYCL
    B = len(DIAG_SIZES)
    mf = np.concatenate([[0], np.cumsum(DIAG_SIZES)]).astype(np.uint32)
    N = int(mf[-1])
    col = np.concatenate([np.arange(n) for n in DIAG_SIZES]).astype(np.int32)
    bt = dev.CsrBatch(up(np.arange(N + 1, dtype=np.int64)), up(col), up(np.ones(N, dtype=dt)),
                      mf, solver=solver)
    base = np.concatenate([np.full(n, 10.0 * (b + 1)) for b, n in enumerate(DIAG_SIZES)]).astype(dt)
    cases = [("const", None, base)]                                         # (a)
    for b, n in enumerate(DIAG_SIZES):                                       # (b)
        if n == 1:
            continue
        for p in sorted({0, n - 2, n - 1}):
            s = base.copy()
            s[int(mf[b]):int(mf[b + 1])] = one_pair(n, p, dt, cyclic)
            cases.append(("pair", (b, p), s))
    for b, n in enumerate(DIAG_SIZES):                                       # (c)
        for p in sorted({0, n // 2, n - 1}):
            s = base.copy()
            s[int(mf[b]) + p] += np.dtype(dt).type(sv.EPS) / 4
            cases.append(("max", (b, p), s))
    t = tdt(dt)
    v_prev = torch.ones(N, dtype=t, device=DEV)
    s_next, v_cur, x = (torch.empty(N, dtype=t, device=DEV) for _ in range(3))
    states = torch.zeros((len(cases), B, 64), dtype=torch.uint8, device=DEV)
    fins = torch.zeros(len(cases), dtype=torch.int32, device=DEV)
    for j, (_, _, s) in enumerate(cases):
        dev.csr_batch_mfree_round(bt, up(s), s_next, v_prev, v_cur, x, states[j], fins[j:j + 1],
                                  eps=sv.EPS, k=1, max_itr=MAX_ITR, semantics=sem)
    got = states.cpu().numpy()
    fins = fins.cpu().numpy()
    for j, (kind, where, s) in enumerate(cases):
        st = [_lib.st_state.from_buffer_copy(got[j, b].tobytes()) for b in range(B)]
        for b in range(B):
            own = s[int(mf[b]):int(mf[b + 1])]
            want = expect_state(own, sv.EPS, sem, 1, MAX_ITR)
            assert got[j, b].tobytes() == bytes(want), (kind, where, b, st[b].stop, st[b].max)
        assert int(fins[j]) == sum(x_.end != 0 for x_ in st)
        stops = [x_.stop for x_ in st]
        if kind == "const":
            assert stops == [1] * B
            assert [x_.max for x_ in st] == [10.0 * (b + 1) for b in range(B)]
            assert [x_.lambda_ for x_ in st] == [10.0 * (b + 1) for b in range(B)]
        elif kind == "pair":
            b, p = where
            n = DIAG_SIZES[b]
            others = [stops[i] for i in range(B) if i != b]
            assert others == [1] * (B - 1), (where, stops)
            if n >= 9:
                if p == n - 1:      # the wrap pair: SYCL semantics only
                    assert stops[b] == int(not cyclic), (where, stops)
                else:
                    assert stops[b] == 0, (where, stops)
                    assert sv.failing_pairs(s[int(mf[b]):int(mf[b + 1])], sv.EPS, cyclic) == [p]
            else:                   # n = 2: both cyclic pairs are the one difference
                assert stops[b] == 0
        else:
            b, p = where
            assert stops == [1] * B
            for i in range(B):
                up_ = float(np.dtype(dt).type(10.0 * (b + 1)) + np.dtype(dt).type(sv.EPS) / 4)
                assert st[i].max == (up_ if i == b else 10.0 * (i + 1)), (where, i)
    bt.close()


# ---------------------------------------------------------------------------
# 5. the plan
# ---------------------------------------------------------------------------
def test_batch_plan_is_the_plan_of_the_stacked_row_ptr(solver):
    mats = reference_batch()
    bt = batch_of(solver, mats, np.float32)
    order, first = bt.plan()
    h_order, h_first, used = _lib.csr_plan(stacked(mats, np.float32)[1])
    assert np.array_equal(order, h_order) and np.array_equal(first, h_first) and used == 4
    assert all(first[c + 1] > first[c] for c in range(4))      # all four classes in one launch
    bt.close()


# ---------------------------------------------------------------------------
# 6. the eigenvalue itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_the_eigenvalues_are_bracketed_by_the_last_sums(solver, dt):
    """Collatz-Wielandt, as for the single solve: min s <= rho <= max s for the
    row sums of the last round, with rho numpy's spectral radius of the
    (fp32-valued) matrix and lambda_b = s[0] of those sums, and the single
    test's slack of 4 eps rho.  The circulant's rho is known exactly (its
    constant row sum), so numpy's own error does not enter there."""
    mats = [(ip, ix, da.astype(np.float32).astype(np.float64)) for ip, ix, da in reference_batch()]
    bt = batch_of(solver, mats, dt)
    lam, v, its, conv, _ = solver.solve_csr_batched(bt, max_itr=MAX_ITR)
    checked = 0
    for b, m in enumerate(mats):
        n = len(m[0]) - 1
        if not conv[b] or n > 300:
            continue
        lam_1, _, _, st = solver.solve_csr(single_of(solver, m, dt), max_itr=MAX_ITR, trace=True)
        s = solver.last_round_sums()[-1]
        assert lam[b] == s[0] == np.dtype(dt).type(lam_1)
        a = cc.densify(*m)
        sums = a.sum(axis=1)
        if b == 5:      # the circulant: constant row sums, exact in fp64, ARE rho
            assert (sums == 0.875).all()
            rho = 0.875  # (numpy's eigvals returns 0.875 + 15 eps64 here)
        else:
            rho = float(np.abs(np.linalg.eigvals(a)).max())
        slack = 4 * float(np.finfo(dt).eps) * rho       # the single test's
        s = s.astype(np.float64)
        assert s.min() - slack <= rho <= s.max() + slack, (b, s.min(), rho, s.max())
        assert s.min() - slack <= float(lam[b]) <= s.max() + slack
        checked += 1
    assert checked == 9
    bt.close()


# ---------------------------------------------------------------------------
# 7. determinism
# ---------------------------------------------------------------------------
def test_two_runs_give_equal_bits(solver):
    bt = batch_of(solver, reference_batch(), np.float32)
    a = solver.solve_csr_batched(bt, max_itr=MAX_ITR)
    b = solver.solve_csr_batched(bt, max_itr=MAX_ITR)
    assert a[0].tobytes() == b[0].tobytes() and torch.equal(a[1], b[1])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert a[4]["rounds"] == b[4]["rounds"]
    bt.close()


# ---------------------------------------------------------------------------
# 8. validation on the device: the host twin's messages, and no handle
# ---------------------------------------------------------------------------
def host_message(mf, rp, col, vals):
    L = _lib.load()
    mf = np.ascontiguousarray(mf, np.uint32)
    rp, col = np.ascontiguousarray(rp, np.int64), np.ascontiguousarray(col, np.int32)
    out = np.zeros(len(mf), np.float64)
    vec = np.zeros(len(rp), np.float64)
    it = np.zeros(len(mf), np.uint32)
    rc = L.max_eigen_value_csr_batched_ex(
        None, 0 if vals.dtype == np.float32 else 1, len(mf) - 1, mf.ctypes.data, len(vals),
        rp.ctypes.data, col.ctypes.data, vals.ctypes.data, out.ctypes.data, vec.ctypes.data,
        it.ctypes.data, None, None, None)
    assert rc < 0
    return _lib.last_error(L)


def test_the_device_check_gives_the_host_messages(solver):
    mats = [cc.make_csr(n, d, seed, dtype=np.float32) for n, d, seed in
            [(5, 3, 3), (64, 8, 7), (1, 1, 3), (300, 8, 9)]]
    mf, rp, col, vals = stacked(mats, np.float32)
    B, N = len(mf) - 1, int(mf[-1])
    assert "null queue" in host_message(mf, rp, col, vals)      # the batch itself is fine

    def refused(mf_, rp_, col_, vals_=vals, expect=None):
        msg = host_message(mf_, rp_, col_, vals_)
        assert "null queue" not in msg and (expect is None or expect in msg), msg
        h = None
        with pytest.raises(_lib.EigenValueError) as ei:
            h = dev.CsrBatch(up(rp_), up(col_), up(vals_), mf_, solver=solver)
        assert msg in str(ei.value), (msg, str(ei.value))
        assert h is None                                        # no handle exists

    bad = mf.copy()
    bad[0] = 1
    refused(bad, rp, col, expect="mat_first[0] must be 0")
    bad = mf.copy()
    bad[2] = bad[1]
    refused(bad, rp, col, expect="does not increase at matrix 1 ")
    for b, lr in ((0, 4), (1, 0), (3, 299 - 1), (3, 150)):
        r = int(mf[b]) + lr
        e = rp.copy()
        e[r + 1] = e[r]
        refused(mf, e, col, expect=f"matrix {b}, local row {lr}: csr: row {r} is empty")
        e[r + 1] = e[r] - 1
        refused(mf, e, col, expect=f"matrix {b}, local row {lr}: csr: row_ptr decreases")
    e = rp.copy()
    e[0] = 1
    refused(mf, e, col, expect="row_ptr[0] must be 0")
    refused(mf, rp, col[:-1], vals[:-1], expect="row_ptr[n] must be nnz")
    for b in range(B):
        n = int(mf[b + 1] - mf[b])
        for c in (n, -1, 2**31 - 1):                            # n_b < N: the cross-matrix case
            for lr in (0, n - 1):
                at = int(rp[int(mf[b]) + lr])
                badc = col.copy()
                badc[at] = c
                refused(mf, rp, badc, expect=f"column index {c} of entry {at} (matrix {b}, "
                                             f"local row {lr}) is outside [0, {n})")
    badc = col.copy()                                           # the LOWEST offending entry
    badc[int(rp[200])], badc[int(rp[70]) + 1] = N + 3, 300
    refused(mf, rp, badc, expect=f"entry {int(rp[70]) + 1} (matrix 3, local row 0)")
    # row_ptr is judged first: with it broken the columns are not read
    e = rp.copy()
    e[10] = e[9]
    badc = col.copy()
    badc[0] = 5
    refused(mf, e, badc, expect="matrix 1, local row 4")
    # mat_first[B] != N is the front's own check (the C call reads N from mat_first)
    bad = mf.copy()
    bad[B] = N - 1
    with pytest.raises(ValueError, match="must be N"):
        dev.CsrBatch(up(rp), up(col), up(vals), bad, solver=solver)
    # bad dtype and batch = 0: the Python front never sends them, so straight
    # to st_csr_batch_create on a live queue, against the host twin's words
    L = _lib.load()
    d_rp, d_col, d_vals = up(rp), up(col), up(vals)

    def create(dtype, batch):
        out = ctypes.c_void_p(1)
        rc = L.st_csr_batch_create(solver.q, dtype, batch, mf.ctypes.data, len(vals),
                                   d_rp.data_ptr(), d_col.data_ptr(), d_vals.data_ptr(),
                                   ctypes.byref(out))
        return rc, _lib.last_error(L), out

    def twin(dtype, batch):
        o, v_, it = np.zeros(B, np.float64), np.zeros(N, np.float64), np.zeros(B, np.uint32)
        rc = L.max_eigen_value_csr_batched_ex(
            None, dtype, batch, mf.ctypes.data, len(vals), rp.ctypes.data, col.ctypes.data,
            vals.ctypes.data, o.ctypes.data, v_.ctypes.data, it.ctypes.data, None, None, None)
        assert rc < 0
        return _lib.last_error(L)

    for dtype, batch, words in ((2, B, "dtype must be 0 (f32) or 1 (f64), got 2"),
                                (-1, B, "dtype must be 0 (f32) or 1 (f64), got -1"),
                                (0, 0, "batch must be >= 1, got 0")):
        want = twin(dtype, batch)
        rc, msg, out = create(dtype, batch)
        assert rc < 0 and words in msg and msg == want and not out.value, (msg, want)
    rc, msg, out = create(0, B)                                 # the call itself is sound
    assert rc == 0 and out.value, msg
    assert L.st_csr_batch_destroy(out) == 0
    # handles of the other kind are refused, not dereferenced
    ok = dev.CsrBatch(up(rp), up(col), up(vals), mf, solver=solver)
    one = dev.CsrMatrix(up(mats[1][0]), up(mats[1][1]), up(mats[1][2]), 64, solver=solver)
    L = _lib.load()
    s = torch.empty(N, dtype=torch.float32, device=DEV)
    assert L.st_csr_rowsum(ok.handle, s.data_ptr(), None) < 0
    assert "not a CSR matrix handle" in _lib.last_error(L)
    assert L.st_csr_batch_rowsum(one.handle, s.data_ptr(), None) < 0
    assert "not a CSR batch handle" in _lib.last_error(L)
    with pytest.raises(TypeError):
        solver.solve_csr_batched(one)
    with pytest.raises(TypeError):
        solver.solve_csr(ok)
    # and the solver is still good for the valid batch
    lam, v, its, conv, st = solver.solve_csr_batched(ok)
    assert st["converged"] == 1 and conv.tolist() == [1] * B
    ok.close()
    assert not ok.handle.value
