"""GPU: the sparse (CSR) solve on a product operator B·A that is never formed -
st_csr_apply / st_csr_product_rowsum / st_csr_product_round /
st_solve_csr_product / hits.

1  the identity as one factor: every bit is the single-matrix round's / solve's
2  csr_apply: the row sums with x = 1, row independence, empty rows, exact sums
3  a genuine product against the exact rational quotient, in derived ulps
4  the solve equals its steps; 5 the solve against the dense model
6  gating; 7 validation on the device; 8 hits; 9 determinism and input forms

All comparisons are of bytes unless said otherwise.
"""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import csr_cases as cc  # noqa: E402
import csr_terms_cases as tc  # noqa: E402
import exact_sums as xs  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from eigen_value_amd.similarity_transform import EigenValue  # noqa: E402

DEV = "cuda:0"
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
SEMS = [pytest.param(_lib.ST_SEM_SYCL, id="sycl"), pytest.param(_lib.ST_SEM_MAINPY, id="mainpy")]
MAX_ITR = 1000
SENTINEL = -7.0


def tdt(dt):
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def csr_of(solver, indptr, indices, data, n=None, empty=False):
    return dev.CsrMatrix(up(np.asarray(indptr, np.int64)), up(np.asarray(indices, np.int32)),
                         up(data), n, solver=solver, allow_empty_rows=empty)


def identity(solver, n, dt):
    return csr_of(solver, np.arange(n + 1), np.arange(n), np.ones(n, dtype=dt), n)


def limits():
    nnz_max, lanes = _lib.csr_class_limits()
    return [int(x) for x in nnz_max], [int(x) for x in lanes]


def lanes_of(k):
    nnz_max, lanes = limits()
    return lanes[int(np.searchsorted(np.array(nnz_max, np.int64), k, side="left"))]


def depth(k):
    """d(k) of a row of k entries: a lane's ceil(k / L) fused multiply-adds,
    the log2(L) levels of the tree (L = 256: 6 in the wave, 3 serial adds),
    plus one - the bound st_csr.h's order gives a row product, in ulps."""
    if k == 0:
        return 0
    L = lanes_of(k)
    tree = int(math.log2(L)) if L <= 64 else 6 + 3
    return -(-k // L) + tree + 1


def positive(n, dt, seed, lo=0.5, hi=2.0):
    rng = np.random.default_rng(seed)
    return (lo + (hi - lo) * rng.random(n)).astype(dt)


@functools.lru_cache(maxsize=None)
def table_case(i):
    n, d, seed, heavy = cc.TABLE[i]
    return (n,) + cc.make_csr(n, d, seed, cc.class_heavy(n) if heavy else None)


def mfree_round(m, s_prev, v_prev, k=1, eps=1e-3, sem=_lib.ST_SEM_SYCL, max_itr=MAX_ITR,
                state=None):
    """One st_csr_mfree_round: (s_next, v_cur, x, state bytes) as numpy."""
    t = tdt(s_prev.dtype)
    n = m.n
    s_next = torch.full((n,), SENTINEL, dtype=t, device=DEV)
    v_cur = torch.full((n,), SENTINEL, dtype=t, device=DEV)
    x = torch.full((n,), SENTINEL, dtype=t, device=DEV)
    state = dev.new_state(DEV) if state is None else state
    dev.csr_mfree_round(m, up(s_prev), s_next, up(v_prev), v_cur, x, state, eps=eps, k=k,
                        max_itr=max_itr, semantics=sem)
    return s_next.cpu().numpy(), v_cur.cpu().numpy(), x.cpu().numpy(), state.cpu().numpy()


def scratch_of(A, value=SENTINEL):
    """The product round's scratch, both halves prefilled; (bytes, x view, y view)."""
    raw = dev.csr_product_scratch(A)
    half = raw.numel() // 2
    es = 8 if A.dtype_code else 4
    xv = raw[:A.n * es].view(A.dtype)
    yv = raw[half:half + A.n * es].view(A.dtype)
    xv.fill_(value)
    yv.fill_(value)
    return raw, xv, yv


def product_round(B, A, s_prev, v_prev, k=1, eps=1e-3, sem=_lib.ST_SEM_SYCL, max_itr=MAX_ITR,
                  state=None):
    """One st_csr_product_round: (s_next, v_cur, x, y, state bytes) as numpy."""
    t = tdt(s_prev.dtype)
    n = A.n
    s_next = torch.full((n,), SENTINEL, dtype=t, device=DEV)
    v_cur = torch.full((n,), SENTINEL, dtype=t, device=DEV)
    raw, xv, yv = scratch_of(A)
    state = dev.new_state(DEV) if state is None else state
    dev.csr_product_round(B, A, up(s_prev), s_next, up(v_prev), v_cur, raw, state, eps=eps, k=k,
                          max_itr=max_itr, semantics=sem)
    return (s_next.cpu().numpy(), v_cur.cpu().numpy(), xv.cpu().numpy(), yv.cpu().numpy(),
            state.cpu().numpy())


def same_bits(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_shape_desc_matches_what_the_tests_assume():
    d = _lib.csr_product_shape()
    assert d["launches_per_round"] == 3 and d["factors"] == 2 and d["x_offset"] == 0


# ---------------------------------------------------------------------------
# 1. the identity as one factor: fma(1, x, 0) = x exactly
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
@pytest.mark.parametrize("dt", DTYPES)
def test_round_with_an_identity_factor_is_the_single_round(solver, dt, n):
    ip, ix, da = cc.make_csr(n, min(n, 5), 3, {0: min(n, 70)})
    da = da.astype(dt)
    m = csr_of(solver, ip, ix, da, n)
    eye = identity(solver, n, dt)
    noisy = positive(n, dt, 1)
    flat = np.full(n, 1.5, dtype=dt)
    flat[n // 2] += dt(1e-4)
    v_prev = positive(n, dt, 2)
    for sem in (_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY):
        # (s_prev, k, max_itr): goes on / stops / exhausts
        for s_prev, k, max_itr in ((noisy, 3, MAX_ITR), (flat, 4, MAX_ITR), (noisy, 7, 7)):
            s_c, v_c, x_c, b_c = mfree_round(m, s_prev, v_prev, k, 1e-3, sem, max_itr)
            for B, A in ((m, eye), (eye, m)):
                s_p, v_p, x_p, y_p, b_p = product_round(B, A, s_prev, v_prev, k, 1e-3, sem,
                                                        max_itr)
                assert b_p.tobytes() == b_c.tobytes(), (sem, k, B is m)
                assert same_bits(s_p, s_c) and same_bits(v_p, v_c) and same_bits(x_p, x_c)
                if A is eye:
                    assert same_bits(y_p, x_c)                 # I x = x
            st = _lib.st_state.from_buffer_copy(b_c.tobytes())
            stops = n < 2 or s_prev is flat
            assert st.stop == int(stops) and st.done == int(stops or k >= max_itr)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", [0, 2])
def test_solve_with_an_identity_factor_is_solve_csr(solver, case, dt, sem):
    """The heavy matrix (all four lane classes, a full row) once as A - pins
    k_csrp_apply in every class - and once as B - pins k_csrp_final."""
    n, ip, ix, da = table_case(case)
    m = csr_of(solver, ip, ix, da.astype(dt), n)
    eye = identity(solver, n, dt)
    lam, v, it, st = solver.solve_csr(m, semantics=sem, trace=True)
    sums = solver.last_round_sums()
    for B, A in ((eye, m), (m, eye)):
        lam_p, v_p, it_p, st_p = solver.solve_csr_product(B, A, semantics=sem, trace=True)
        assert lam_p == lam and it_p == it and torch.equal(v_p, v)
        assert (st_p["rounds"], st_p["converged"]) == (st["rounds"], st["converged"])
        assert np.array_equal(solver.last_round_sums(), sums)
    assert st["converged"] == 1


# ---------------------------------------------------------------------------
# 2. csr_apply
# ---------------------------------------------------------------------------
def padded_rows(indptr, vals):
    """[n, longest row] with zeros past each row's end (exact_rowsum's input)."""
    lens = np.diff(indptr)
    out = np.zeros((len(lens), int(lens.max())), dtype=vals.dtype)
    mask = np.arange(out.shape[1])[None, :] < lens[:, None]
    out[mask] = vals
    return out


def permuted(indptr, indices, data, perm):
    lens = np.diff(indptr)
    idx = np.concatenate([np.arange(indptr[r], indptr[r + 1]) for r in perm])
    return (np.concatenate([[0], np.cumsum(lens[perm])]).astype(np.int64),
            indices[idx].astype(np.int32), data[idx])


@pytest.mark.parametrize("dt", DTYPES)
def test_apply(solver, dt):
    n, ip, ix, da = table_case(2)
    da = da.astype(dt)
    m = csr_of(solver, ip, ix, da, n)
    t = tdt(dt)
    # x = 1: the row sums, bit for bit (the same fma against 1)
    ones = torch.ones(n, dtype=t, device=DEV)
    assert same_bits(dev.csr_apply(m, ones).cpu().numpy(), dev.csr_rowsum(m).cpu().numpy())
    x = positive(n, dt, 4)
    y = dev.csr_apply(m, up(x)).cpu().numpy()
    # against the exact sum of the exact products (an fma rounds once): d(k) ulps
    wide = np.float64 if np.dtype(dt) == np.float32 else np.longdouble
    exact = padded_rows(ip, da.astype(wide) * x.astype(wide)[ix]).sum(axis=1)
    err = np.abs(xs.err_ulps_of(y, exact, dt))
    bound = np.array([depth(int(k)) for k in np.diff(ip)])
    print("apply max |err| ulps:", float(err.max()), "largest bound", int(bound.max()))
    assert (err <= bound).all(), (err - bound).max()
    # permuting rows permutes y bitwise
    perm = np.random.default_rng(5).permutation(n)
    p = csr_of(solver, *permuted(ip, ix, da, perm), n)
    assert same_bits(dev.csr_apply(p, up(x)).cpu().numpy(), y[perm])
    # appending rows of other classes (and new columns) changes no bit
    extra = 47
    rng = np.random.default_rng(9)
    lens = np.array([200] * 40 + [2100] * 3 + [2] * 4)
    cols = [rng.integers(0, n + extra, size=k) for k in lens]
    ip2 = np.concatenate([ip, ip[-1] + np.cumsum(lens)])
    ix2 = np.concatenate([ix] + cols).astype(np.int32)
    da2 = np.concatenate([da, (1.0 - rng.random(int(lens.sum()))).astype(dt)])
    big = csr_of(solver, ip2, ix2, da2, n + extra)
    x2 = np.concatenate([x, positive(extra, dt, 6)])
    assert same_bits(dev.csr_apply(big, up(x2)).cpu().numpy()[:n], y)
    # emptied rows come back as exactly +0.0 in an output prefilled with NaN
    gone = [0, 1, 9, n // 2, n - 1]
    e = csr_of(solver, *tc.empty_rows(ip, ix, da, gone), n, empty=True)
    out = torch.full((n,), float("nan"), dtype=t, device=DEV)
    ye = dev.csr_apply(e, up(x), out=out).cpu().numpy()
    assert same_bits(ye[gone], np.zeros(len(gone), dtype=dt))       # +0.0, not -0.0
    keep = np.setdiff1d(np.arange(n), gone)
    assert same_bits(ye[keep], y[keep])


# ---------------------------------------------------------------------------
# 3. a genuine product against the exact quotient
# ---------------------------------------------------------------------------
def as_ints(a, shift):
    """The floats a * 2^shift as exact Python integers (object array)."""
    scaled = np.ldexp(np.asarray(a, dtype=np.float64), shift)
    assert np.array_equal(scaled, np.floor(scaled)) and np.isfinite(scaled).all()
    return np.array([int(v) for v in scaled], dtype=object)


def exact_quotient(B, A, x):
    """(B (A x)) / x as Fractions, in integer arithmetic: values are in (0, 1]
    with at most 53 significant bits, so a * 2^110 is an integer; x in (1/8, 8)
    likewise under 2^60."""
    (bp, bi, bd), (ap, ai, ad) = B, A
    xi = as_ints(x, 60)
    y = np.add.reduceat(as_ints(ad, 110) * xi[ai], ap[:-1])          # * 2^170
    tot = np.add.reduceat(as_ints(bd, 110) * y[bi], bp[:-1])         # * 2^280
    return [Fraction(int(t), int(d) << 220) for t, d in zip(tot, xi)]


def ulps_from(got, exact, dt):
    nm = xs.NMANT[np.dtype(dt)]
    out = np.empty(len(exact))
    for r, (g, e) in enumerate(zip(got, exact)):
        lo = e.numerator.bit_length() - e.denominator.bit_length()
        if Fraction(2) ** lo > e:
            lo -= 1                                                   # 2^lo <= e < 2^(lo + 1)
        out[r] = float(abs(Fraction(float(g)) - e) / Fraction(2) ** (lo - nm))
    return out


@pytest.mark.parametrize("swap", [False, True], ids=["heavyB", "heavyA"])
@pytest.mark.parametrize("dt", DTYPES)
def test_product_round_against_the_exact_quotient(solver, dt, swap):
    """s_next[r] within d_B(r) + max over the row's columns c of d_A(c) + 1
    ulps of (B (A x)) / x: y[c] carries d_A(c) roundings, the row of B adds its
    own d_B(r) on top of the largest of them, the division one more."""
    n, ip2, ix2, da2 = table_case(2)
    _, ip1, ix1, da1 = table_case(1)
    Bh = (ip2, ix2, da2.astype(dt))
    Ah = (ip1, ix1, da1.astype(dt))
    if swap:
        Bh, Ah = Ah, Bh
    assert np.diff(Bh[0]).min() >= 1 and np.diff(Ah[0]).min() >= 1    # reduceat's rows
    B, A = csr_of(solver, *Bh, n), csr_of(solver, *Ah, n)
    s_prev, v_prev = positive(n, dt, 1), positive(n, dt, 2)
    s_next, v_cur, x, y, b_p = product_round(B, A, s_prev, v_prev)
    assert same_bits(x, v_prev * s_prev)
    assert same_bits(y, dev.csr_apply(A, up(x)).cpu().numpy())
    err = ulps_from(s_next, exact_quotient(Bh, Ah, x), dt)
    d_a = np.array([depth(int(k)) for k in np.diff(Ah[0])])
    bound = np.array([depth(int(Bh[0][r + 1] - Bh[0][r])) + d_a[Bh[1][Bh[0][r]:Bh[0][r + 1]]].max()
                      + 1 for r in range(n)])
    print("product round max |err| ulps:", float(err.max()), "bounds", int(bound.min()), "-",
          int(bound.max()))
    assert (err <= bound).all(), (err - bound).max()
    # v_cur and the state depend on s_prev and v_prev only
    _, v_c, _, b_c = mfree_round(B, s_prev, v_prev)
    assert same_bits(v_cur, v_c) and b_p.tobytes() == b_c.tobytes()


# ---------------------------------------------------------------------------
# 4. the solve equals its steps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_solve_equals_its_steps(solver, dt, sem):
    n, ip2, ix2, da2 = table_case(2)
    _, ip1, ix1, da1 = table_case(1)
    B = csr_of(solver, ip2, ix2, da2.astype(dt), n)
    A = csr_of(solver, ip1, ix1, da1.astype(dt), n)
    lam, v, it, st = solver.solve_csr_product(B, A, trace=True, semantics=sem)
    sums = solver.last_round_sums()
    t = tdt(dt)
    s = [torch.empty(n, dtype=t, device=DEV) for _ in range(2)]
    vv = [torch.ones(n, dtype=t, device=DEV), torch.empty(n, dtype=t, device=DEV)]
    raw, _, _ = scratch_of(A)
    state = dev.new_state(DEV)
    dev.csr_product_rowsum(B, A, raw, out=s[0])
    trace = []
    for k in range(MAX_ITR):
        trace.append(s[k & 1].cpu().numpy())
        dev.csr_product_round(B, A, s[k & 1], s[(k + 1) & 1], vv[k & 1], vv[(k + 1) & 1], raw,
                              state, eps=1e-3, k=k + 1, max_itr=MAX_ITR, semantics=sem)
        if dev.read_state(state)["done"]:
            break
    fin = dev.read_state(state)
    assert fin["end"] == st["rounds"] == len(trace) and fin["iters"] == it
    assert same_bits(np.stack(trace), sums)
    assert fin["eigen_val"] == lam and st["converged"] == 1
    assert same_bits(vv[fin["end"] & 1].cpu().numpy(), v.cpu().numpy())


# ---------------------------------------------------------------------------
# 5. against the dense model
# ---------------------------------------------------------------------------
HOLES = [9, 30, 63]
HOLES_SEED = 7


def irreducible(m):
    """Strong connectivity of the directed graph of a dense nonnegative matrix."""
    adj = m > 0
    for g in (adj, adj.T):
        seen = np.zeros(len(g), dtype=bool)
        seen[0] = True
        todo = [0]
        while todo:
            nxt = np.flatnonzero(g[todo.pop()] & ~seen)
            seen[nxt] = True
            todo.extend(nxt.tolist())
        if not seen.all():
            return False
    return True


@functools.lru_cache(maxsize=None)
def dense_case(name):
    """(B triple, A triple, A has empty rows) in fp64."""
    if name == "ata":
        _, ip, ix, da = table_case(1)
        return dev.csr_transpose_host(ip, ix, da), (ip, ix, da), False
    if name == "square":
        _, ip, ix, da = table_case(0)
        return (ip, ix, da), (ip, ix, da), False
    ip, ix, da = tc.empty_rows(*cc.make_csr(64, 8, HOLES_SEED), HOLES)
    return dev.csr_transpose_host(ip, ix, da, allow_empty=True), (ip, ix, da), True


DENSE_CASES = ["ata", "square", "holes"]


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", DENSE_CASES)
def test_solve_against_the_dense_model_fp64(solver, name, sem):
    Bh, Ah, holes = dense_case(name)
    n = len(Ah[0]) - 1
    M = cc.densify(*Bh) @ cc.densify(*Ah)
    if holes:
        assert np.diff(Bh[0]).min() >= 1 and irreducible(M)       # AᵀA stays irreducible
    cyclic = sem == _lib.ST_SEM_SYCL
    B = csr_of(solver, *Bh, n)
    A = csr_of(solver, *Ah, n, empty=holes)
    lam, v, it, st = solver.solve_csr_product(B, A, semantics=sem, trace=True)
    sums = solver.last_round_sums()
    kb, conv, _, _ = cc.model(M, 1e-3, cyclic)
    assert conv and st["converged"] == 1 and it == cc.count_of(kb, conv, cyclic)
    lam_d, v_d, it_d, st_d = solver.solve(up(M), matrix_free=True, semantics=sem)
    assert (it, st["rounds"]) == (it_d, st_d["rounds"])
    assert abs(lam - lam_d) <= 1e-10 * abs(lam_d)
    v, v_d = v.cpu().numpy(), v_d.cpu().numpy()
    assert (np.abs(v - v_d) <= 1e-10 * np.abs(v_d)).all()
    assert sums[-1].min() <= lam <= sums[-1].max() and lam == float(sums[-1][0])


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("name", DENSE_CASES)
def test_solve_fp32(solver, name, sem):
    """test_gpu_csr.py::test_solve_fp32's treatment: equal iteration counts
    against the same iteration in fp64 on the same (fp32-valued) matrices and
    against the dense fp32 solve of B @ A, and lambda and every v[i] within the
    summed per-round budgets - the largest row bound of
    test_product_round_against_the_exact_quotient plus one ulp for the v
    update."""
    Bh, Ah, holes = dense_case(name)
    n = len(Ah[0]) - 1
    b32, a32 = Bh[2].astype(np.float32), Ah[2].astype(np.float32)
    B32 = csr_of(solver, Bh[0], Bh[1], b32, n)
    A32 = csr_of(solver, Ah[0], Ah[1], a32, n, empty=holes)
    B64 = csr_of(solver, Bh[0], Bh[1], b32.astype(np.float64), n)
    A64 = csr_of(solver, Ah[0], Ah[1], a32.astype(np.float64), n, empty=holes)
    lam, v, it, st = solver.solve_csr_product(B32, A32, semantics=sem, trace=True)
    sums = solver.last_round_sums()
    lam_r, v_r, it_r, st_r = solver.solve_csr_product(B64, A64, semantics=sem)
    M32 = (cc.densify(Bh[0], Bh[1], b32.astype(np.float64))
           @ cc.densify(Ah[0], Ah[1], a32.astype(np.float64))).astype(np.float32)
    lam_d, _, it_d, st_d = solver.solve(up(M32), matrix_free=True, semantics=sem)
    assert it == it_r == it_d and st["converged"] == st_r["converged"] == st_d["converged"] == 1
    d_a = np.array([depth(int(k)) for k in np.diff(Ah[0])])
    per_round = max(depth(int(Bh[0][r + 1] - Bh[0][r]))
                    + int(d_a[Bh[1][Bh[0][r]:Bh[0][r + 1]]].max()) + 1 for r in range(n)) + 1
    budget = per_round * st["rounds"]
    ulp = float(np.finfo(np.float32).eps)
    e_lam = abs(lam - lam_r) / (ulp * abs(lam_r))
    v, v_r = v.cpu().numpy().astype(np.float64), v_r.cpu().numpy()
    e_v = float((np.abs(v - v_r) / (ulp * np.abs(v_r))).max())
    print(f"fp32 vs fp64 {name}: lambda {e_lam:.2f} v {e_v:.2f} relative ulps, budget {budget} "
          f"({per_round} x {st['rounds']} rounds)")
    assert e_lam <= budget and e_v <= budget
    assert sums[-1].min() <= np.float32(lam) <= sums[-1].max()


# ---------------------------------------------------------------------------
# 6. gating
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_a_round_beyond_the_end_writes_nothing(solver, dt):
    n, ip, ix, da = table_case(0)
    A = csr_of(solver, ip, ix, da.astype(dt), n)
    flat = np.full(n, 1.5, dtype=dt)
    v_prev = positive(n, dt, 2)
    state = dev.new_state(DEV)
    s1, v1, x1, y1, b1 = product_round(A, A, flat, v_prev, k=4, state=state)     # stops
    st = _lib.st_state.from_buffer_copy(b1.tobytes())
    assert st.done == 1 and st.end == 4 and not (s1 == SENTINEL).any()
    for k in (5, 6, 40):
        s2, v2, x2, y2, b2 = product_round(A, A, positive(n, dt, k), v_prev, k=k, state=state)
        assert b2.tobytes() == b1.tobytes()
        for got in (s2, v2, x2, y2):
            assert same_bits(got, np.full(n, SENTINEL, dtype=dt))


# ---------------------------------------------------------------------------
# 7. validation on the device
# ---------------------------------------------------------------------------
def lib_solve(solver, B, A):
    """st_solve_csr_product through the library alone (no Python check)."""
    L = _lib.load()
    v = torch.empty(A.n, dtype=A.dtype, device=DEV)
    ev, it = ctypes.c_double(), ctypes.c_uint32()
    rc = L.st_solve_csr_product(solver.q, B.handle, A.handle, v.data_ptr(), None,
                                ctypes.byref(ev), ctypes.byref(it), None, None)
    return rc, _lib.last_error(L)


def test_validation_on_the_device(solver):
    n, ip, ix, da = table_case(0)
    ipb, ixb, dab = cc.make_csr(n, 8, 11)
    B = csr_of(solver, ipb, ixb, dab, n)
    A = csr_of(solver, ip, ix, da, n)
    assert solver.solve_csr_product(B, A)[3]["converged"] == 1
    # a row of B whose columns all hit emptied rows of A: the lowest is named
    hit20 = sorted(set(int(c) for c in ixb[ipb[20]:ipb[21]]))
    hit41 = sorted(set(int(c) for c in ixb[ipb[41]:ipb[42]]))
    gone = set(hit20) | set(hit41)
    low = min(r for r in range(n) if all(int(c) in gone for c in ixb[ipb[r]:ipb[r + 1]]))
    assert low <= 20
    Ae = csr_of(solver, *tc.empty_rows(ip, ix, da, sorted(gone)), n, empty=True)
    with pytest.raises(_lib.EigenValueError, match=rf"row {low} of B·A has no positive entry"):
        solver.solve_csr_product(B, Ae)
    Ae = csr_of(solver, *tc.empty_rows(ip, ix, da, hit41), n, empty=True)
    with pytest.raises(_lib.EigenValueError, match=r"row 41 of B·A has no positive entry"):
        solver.solve_csr_product(B, Ae)
    # an empty row of B
    Be = csr_of(solver, *tc.empty_rows(ipb, ixb, dab, [4, 50]), n, empty=True)
    with pytest.raises(_lib.EigenValueError, match=r"row 4 of B·A has no positive entry"):
        solver.solve_csr_product(Be, A)
    # the solver is still good
    assert solver.solve_csr_product(B, A)[3]["converged"] == 1
    # mismatches, in the stated order: alive, n, dtype, device
    small32 = csr_of(solver, *cc.make_csr(32, 8, 3, dtype=np.float32), 32)
    A32 = csr_of(solver, ip, ix, da.astype(np.float32), n)
    rc, msg = lib_solve(solver, small32, A)
    assert rc < 0 and "differ in n (B: 32, A: 64)" in msg
    rc, msg = lib_solve(solver, A32, A)
    assert rc < 0 and "differ in dtype (B: 0, A: 1" in msg
    with pytest.raises(ValueError, match=r"differ in n \(B: 32, A: 64\)"):
        solver.solve_csr_product(small32, A)
    with pytest.raises(TypeError, match="differ in dtype"):
        solver.solve_csr_product(A32, A)
    dead = csr_of(solver, ip, ix, da, n)
    dead.close()
    with pytest.raises(ValueError, match="B: the matrix is closed"):
        solver.solve_csr_product(dead, small32)
    L = _lib.load()
    raw = dev.csr_product_scratch(A)
    s = torch.empty(n, dtype=torch.float64, device=DEV)
    assert L.st_csr_product_rowsum(small32.handle, A.handle, s.data_ptr(), raw.data_ptr(),
                                   None) < 0
    assert "differ in n" in _lib.last_error(L)
    assert L.st_csr_product_rowsum(A32.handle, A.handle, s.data_ptr(), raw.data_ptr(), None) < 0
    assert "differ in dtype" in _lib.last_error(L)
    if torch.cuda.device_count() > 1:
        other = torch.device("cuda:1")
        s1 = dev.DeviceSolver(other)
        try:
            A1 = dev.CsrMatrix(torch.from_numpy(ip).to(other),
                               torch.from_numpy(ix).to(other),
                               torch.from_numpy(da).to(other), n, solver=s1)
            rc, msg = lib_solve(solver, A1, A)
            assert rc < 0 and "different devices" in msg
            with pytest.raises(ValueError, match="different devices"):
                solver.solve_csr_product(A1, A)
            A1.close()
        finally:
            s1.close()
            torch.cuda.set_device(0)


# ---------------------------------------------------------------------------
# 8. hits
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def link_graph(n):
    """A seeded link graph: 6 links per node, every node linked to (node r
    links to r + 1), some nodes without out-links."""
    rng = np.random.default_rng(n)
    a = np.zeros((n, n))
    for r in range(n):
        a[r, rng.choice(n, 6, replace=False)] = 1.0 - rng.random(6)
        a[r, (r + 1) % n] = 1.0
    sinks = [3, n // 2, n - 2]
    for r in sinks:                       # their in-links come from r - 1, kept
        a[r, :] = 0
    assert (a.sum(axis=0) > 0).all() and irreducible(a.T @ a)
    return a, sinks


@pytest.mark.parametrize("n", [64, 300])
def test_hits(solver, n):
    a, sinks = link_graph(n)
    trip = tc.to_csr(a)
    links = csr_of(solver, *trip, n, empty=True)
    assert links.empty_rows == len(sinks)
    auth, hubs, sigma, it, st = solver.hits(links, eps=1e-11, trace=True)
    sums = solver.last_round_sums()
    assert st["converged"] == 1
    # authorities = v / sum(v) of the product solve, hubs = links applied to them
    lt = links.transpose(solver)
    lam, v, it2, st2 = solver.solve_csr_product(lt, links, eps=1e-11)
    assert it2 == it and sigma == math.sqrt(lam)
    assert torch.equal(auth, v / v.sum())
    h = dev.csr_apply(links, auth)
    assert torch.equal(hubs, h / h.sum())
    assert (hubs[sinks] == 0).all()
    # sigma^2 inside the last sums' bracket, and sigma the largest singular value
    assert sums[-1].min() <= sigma * sigma <= sums[-1].max()
    sv = float(np.linalg.svd(a, compute_uv=False)[0])
    print(f"hits n = {n}: {it} rounds, sigma {sigma!r} svd {sv!r}, bracket width "
          f"{float(sums[-1].max() - sums[-1].min()):.3g}")
    assert abs(sigma - sv) <= 1e-10 * sv
    # a graph with a node nobody links to: refused by name
    b = a.copy()
    b[:, 5] = 0
    bad = csr_of(solver, *tc.to_csr(b), n, empty=True)
    with pytest.raises(_lib.EigenValueError, match=r"column 5 has no entry"):
        solver.hits(bad)


# ---------------------------------------------------------------------------
# 9. determinism and input forms
# ---------------------------------------------------------------------------
def test_determinism_and_the_three_input_forms(solver):
    sp = pytest.importorskip("scipy.sparse")
    n, ip2, ix2, da2 = table_case(2)
    _, ip1, ix1, da1 = table_case(1)
    B, A = csr_of(solver, ip2, ix2, da2, n), csr_of(solver, ip1, ix1, da1, n)
    a = solver.solve_csr_product(B, A, trace=True)
    sums_a = solver.last_round_sums()
    b = solver.solve_csr_product(B, A, trace=True)
    assert a[0] == b[0] and a[2] == b[2] and torch.equal(a[1], b[1])
    assert same_bits(sums_a, solver.last_round_sums())

    def forms(ip, ix, da):
        return ((ip, ix, da), sp.csr_matrix((da, ix, ip), shape=(n, n)),
                torch.sparse_csr_tensor(torch.from_numpy(ip), torch.from_numpy(ix.astype(np.int64)),
                                        torch.from_numpy(da), size=(n, n)))

    left = solver.solve_csr_product(B, A, left=True)
    ata = solver.solve_csr_product(A.T, A)
    aat = solver.solve_csr_product(A, A.T)
    with EigenValue() as ev:
        for fb, fa in zip(forms(ip2, ix2, da2), forms(ip1, ix1, da1)):
            r = ev.similarity_transform_csr_product(fb, fa)
            assert r[0] == a[0] and r[3] == a[2] and r[0].dtype == np.float64
            assert same_bits(r[1], a[1].cpu().numpy())
            g = ev.similarity_transform_csr_gram(fa, side="ata")
            assert g[0] == ata[0] and g[3] == ata[2] and same_bits(g[1], ata[1].cpu().numpy())
            g = ev.similarity_transform_csr_gram(fa, side="aat")
            assert g[0] == aat[0] and g[3] == aat[2] and same_bits(g[1], aat[1].cpu().numpy())
        # the left vector of B A is the right one of Aᵀ Bᵀ
        t2 = dev.csr_transpose_host(ip2, ix2, da2)
        t1 = dev.csr_transpose_host(ip1, ix1, da1)
        r = ev.similarity_transform_csr_product(t1, t2)
        assert r[0] == left[0] and r[3] == left[2] and same_bits(r[1], left[1].cpu().numpy())
