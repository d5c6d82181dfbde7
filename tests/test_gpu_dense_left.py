"""GPU: the dense left-vector kernels (k_colsum, k_left_sweep, k_left_finish)
and solve(A, left=True).

The sizes: RB (rows per block) and the strip (columns per workgroup) come from
the shape query; S holds the small sizes, the sizes around one and two row
blocks and around one and two strips, odd ones among them (rows that are not
16-byte aligned take the element-wide path).

The order test compares bytes with the host model (dense_left_order_model) on
the columns model_columns picks - all of them up to n = 80, above that the
columns at the tails and strip boundaries plus seeded ones (the model is
exact integer arithmetic in Python, ~1 us per multiply-add); every column of
every size is compared byte for byte in the exact-input test, which needs no
model.

No launch knob of the tuning build applies to these kernels: their grids are
exact (one workgroup per tile, no cap), so the independence test has no
grid-limit half."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import csr_order_model as com                      # noqa: E402
import dense_left_order_model as dlm               # noqa: E402
from eigen_value_amd import _lib                   # noqa: E402
from eigen_value_amd import device as dev          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ("float32", "float64")
TD = {"float32": torch.float32, "float64": torch.float64}
CODE = {"float32": _lib.DTYPE_F32, "float64": _lib.DTYPE_F64}


def sizes(dt):
    rb = _lib.left_shape(CODE[dt], 1)["rows"]
    strip = _lib.left_shape(CODE[dt], 1)["strip"]
    table = 2049        # past the first step of the rows-per-block table, odd
    return sorted({1, 2, 3, 5, 63, 64, 65, rb - 1, rb, rb + 1, 2 * rb + 1, strip - 1, strip,
                   strip + 1, 2 * strip + 3, table})


def test_sizes_hold_what_the_kernels_branch_on():
    for dt in DTYPES:
        S = sizes(dt)
        w = _lib.left_shape(CODE[dt], 1)["w"]
        assert any(n % w for n in S) and any(n % w == 0 and n > 1 for n in S)
        assert len({dlm.shape(dt, n)[0] for n in S}) >= 2      # more than one RB of the table
        assert any(-(-n // dlm.shape(dt, n)[0]) > 16 for n in S)   # the finish's unrolled trips


def dev_t(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)   # (regimes are read-only)


def host(t):
    return t.cpu().numpy()


def left_round(A, s, v, *, k=1, eps=1e-3, max_itr=1000, sem=_lib.ST_SEM_SYCL, state=None,
               v_cur=None):
    """One launch on the device matrix A from host vectors: (s_next, v_cur,
    state bytes, scratch)."""
    n = A.shape[0]
    state = dev.new_state(DEV) if state is None else state
    s_next = torch.full((n,), -7.0, dtype=A.dtype, device=DEV)
    v_cur = torch.full((n,), -7.0, dtype=A.dtype, device=DEV) if v_cur is None else v_cur
    scratch = dev.left_scratch(n, A.dtype, DEV)
    dev.mfree_left_round(A, dev_t(s), s_next, dev_t(v), v_cur, scratch, state, eps=eps, k=k,
                         max_itr=max_itr, semantics=sem)
    return host(s_next), host(v_cur), host(state).tobytes(), scratch


def right_round(At, s, v, *, k=1, eps=1e-3, max_itr=1000, sem=_lib.ST_SEM_SYCL, state=None,
                v_cur=None):
    """The same launch of the existing matrix-free round on the transposed
    copy."""
    n = At.shape[0]
    state = dev.new_state(DEV) if state is None else state
    s_next = torch.full((n,), -7.0, dtype=At.dtype, device=DEV)
    v_cur = torch.full((n,), -7.0, dtype=At.dtype, device=DEV) if v_cur is None else v_cur
    dev.mfree_round(At, dev_t(s), s_next, dev_t(v), v_cur, state, eps=eps, k=k, max_itr=max_itr,
                    semantics=sem)
    return host(s_next), host(v_cur), host(state).tobytes()


# ---------------------------------------------------------------------------
# order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", dlm.REGIMES)
def test_order_matches_the_host_model(name, dt):
    sh = _lib.left_shape(CODE[dt], 1)
    for n in sizes(dt):
        A, s, v = dlm.regime(name, dt, n)
        cols = dlm.model_columns(n, sh["strip"], sh["w"])
        At = dev_t(A)
        got0 = host(dev.colsum(At))
        want0 = dlm.columns(A, None, dt, cols)
        assert got0[cols].tobytes() == want0.tobytes(), (name, dt, n, "colsum")
        x = v * s
        s_next, v_cur, state, _ = left_round(At, s, v)
        num = dlm.columns(A, x, dt, cols)
        with np.errstate(all="ignore"):
            want = num / x[cols]
            want_v = v * (s / s.max())
        assert s_next[cols].tobytes() == want.tobytes(), (name, dt, n, "s_next")
        assert v_cur.tobytes() == want_v.tobytes(), (name, dt, n, "v_cur")
        _, v_ref, state_ref = right_round(dev_t(A.T), s, v)
        assert state == state_ref and v_cur.tobytes() == v_ref.tobytes(), (name, dt, n, "state")


# ---------------------------------------------------------------------------
# exact inputs against the existing kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_exact_inputs_equal_the_round_on_a_transposed_copy(dt):
    """Entries in {1, 2, 3, 4}: every partial sum of launch 0 and launch 1 is
    an integer <= 16 n^2 <= 2^24, exact in fp32 in any order, so every column
    must equal the existing kernels' rows of the transposed copy bit for bit.
    (Later launches are not exact and are not claimed.)"""
    for n in [m for m in sizes(dt) if m <= 1024]:
        rng = np.random.default_rng(100 + n)
        A = rng.integers(1, 5, size=(n, n)).astype(dt)
        Ad, Atd = dev_t(A), dev_t(A.T)
        s0 = host(dev.colsum(Ad))
        assert s0.tobytes() == host(dev.rowsum(Atd)).tobytes(), (dt, n)
        assert s0.tobytes() == A.sum(axis=0, dtype=np.float64).astype(dt).tobytes()
        ones = np.ones(n, dt)
        s_next, v_cur, state, _ = left_round(Ad, s0, ones)
        r_next, r_cur, r_state = right_round(Atd, s0, ones)
        assert s_next.tobytes() == r_next.tobytes(), (dt, n)
        assert v_cur.tobytes() == r_cur.tobytes() and state == r_state, (dt, n)


# ---------------------------------------------------------------------------
# v and state
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY])
@pytest.mark.parametrize("dt", DTYPES)
def test_v_and_state_equal_mfree_round_over_three_launches(dt, sem):
    """Going-on, stopping and exhausted rounds over launches 1 .. 3, both
    kernels fed the same vectors: v_cur and the 64 bytes of the state depend
    on the vectors only."""
    for n in (65, 1025):
        rng = np.random.default_rng(7 + n)
        A = (1.0 - rng.random((n, n))).astype(dt)
        Ad, Atd = dev_t(A), dev_t(A.T)
        rough = [(1.0 + rng.random(n)).astype(dt) for _ in range(3)]
        flat = np.full(n, 2.0, dt)
        # the open chain ignores the pair (n-1, 0): steps of eps / 2, so that
        # every adjacent pair passes and the two ends are 32 eps or more apart
        open_only = (2.0 + 5e-4 * np.arange(n) * (64.0 / (n - 1))).astype(dt) if n > 65 \
            else (2.0 + 5e-4 * np.arange(n)).astype(dt)
        plans = {"going_on": (rough, 1000), "stop_at_2": ([rough[0], flat, rough[2]], 1000),
                 "exhaust_at_2": (rough, 2), "wrap_pair": ([rough[0], open_only, rough[2]], 1000)}
        for tag, (svecs, max_itr) in plans.items():
            st_l, st_r = dev.new_state(DEV), dev.new_state(DEV)
            v = np.ones(n, dt)
            vl = [torch.full((n,), -7.0, dtype=TD[dt], device=DEV) for _ in range(2)]
            vr = [torch.full((n,), -7.0, dtype=TD[dt], device=DEV) for _ in range(2)]
            for k in (1, 2, 3):
                _, v_l, b_l, _ = left_round(Ad, svecs[k - 1], v, k=k, max_itr=max_itr, sem=sem,
                                            state=st_l, v_cur=vl[k & 1])
                _, v_r, b_r = right_round(Atd, svecs[k - 1], v, k=k, max_itr=max_itr, sem=sem,
                                          state=st_r, v_cur=vr[k & 1])
                assert v_l.tobytes() == v_r.tobytes(), (dt, sem, n, tag, k)
                assert b_l == b_r, (dt, sem, n, tag, k, dev.read_state(st_l), dev.read_state(st_r))
                if (v_l != -7.0).all():
                    v = v_l
            end = dev.read_state(st_l)["end"]
            assert (end == 2) == (tag in ("stop_at_2", "exhaust_at_2") or
                                  (tag == "wrap_pair" and sem == _lib.ST_SEM_MAINPY)), (tag, end)


def test_launches_after_the_stop_write_nothing():
    n = 300
    A = dev_t(np.random.default_rng(3).random((n, n)) + 0.5)
    flat = np.full(n, 2.0)
    state = dev.new_state(DEV)
    left_round(A, flat, np.ones(n), k=1, state=state)
    assert dev.read_state(state)["end"] == 1
    s_next, v_cur, _, scratch = left_round(A, flat + 1.0, np.ones(n), k=2, state=state)
    assert (s_next == -7.0).all() and (v_cur == -7.0).all()


# ---------------------------------------------------------------------------
# error
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_error_is_within_the_bound_of_the_order(dt, capsys):
    """Every column of colsum and every numerator of a round against the exact
    rational sum: at most RB serial fmas + the combine's adds + 1 roundings
    (dense_left_order_model.bound_ulps; DESIGN.md records the largest seen).
    The numerator is read back from the partials the round leaves in the
    scratch, added as k_left_finish adds them."""
    rb = _lib.left_shape(CODE[dt], 1)["rows"]
    worst = 0.0
    for n in (2 * rb + 1, 4 * rb + 5):
        rbn, comb = dlm.shape(dt, n)
        bound = dlm.bound_ulps(n, rbn, comb)
        for name in dlm.REGIMES:
            A, s, v = dlm.regime(name, dt, n)
            x = v * s
            Ad = dev_t(A)
            s0 = host(dev.colsum(Ad))
            s_next, _, _, scratch = left_round(Ad, s, v)
            xe = -(-n // 64) * 64
            part = host(scratch)[xe:xe + -(-n // rbn) * n].reshape(-1, n)
            num = part[0].copy()
            for j in range(1, part.shape[0]):
                num = num + part[j]
            with np.errstate(all="ignore"):
                assert (num / x).tobytes() == s_next.tobytes(), (dt, n, name)
            for c in range(n):
                e0 = com.err_ulps(s0[c], dlm.exact_column(A[:, c]), dt)
                e1 = com.err_ulps(num[c], dlm.exact_column(A[:, c], x), dt)
                assert e0 <= bound and e1 <= bound, (dt, n, name, c, e0, e1, bound)
                worst = max(worst, e0, e1)
    with capsys.disabled():
        print(f"\n[dense left] {dt}: largest error {worst:.3f} ulps")


# ---------------------------------------------------------------------------
# independence
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_a_column_does_not_depend_on_the_others(dt):
    strip = _lib.left_shape(CODE[dt], 1)["strip"]
    n = 2 * strip + 3
    A, s, v = dlm.regime("A", dt, n)
    keep = np.array(sorted({0, 1, strip - 1, strip, 2 * strip, n - 2, n - 1}))
    B = (1.0 - np.random.default_rng(5).random((n, n))).astype(dt)
    B[:, keep] = A[:, keep]
    a0, b0 = host(dev.colsum(dev_t(A))), host(dev.colsum(dev_t(B)))
    a1, _, _, _ = left_round(dev_t(A), s, v)
    b1, _, _, _ = left_round(dev_t(B), s, v)
    assert a0[keep].tobytes() == b0[keep].tobytes() and a1[keep].tobytes() == b1[keep].tobytes()
    assert (a0 != b0).sum() > n // 2 and (a1 != b1).sum() > n // 2   # the others did change


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("pad", [64, 1])
def test_nothing_outside_the_matrix_is_read(dt, pad):
    """A inside a larger buffer filled with NaN on both sides (pad = 1: the
    matrix is not 16-byte aligned either): unchanged results, so nothing
    outside A entered a sum."""
    strip = _lib.left_shape(CODE[dt], 1)["strip"]
    for n in (5, 65, strip, strip + 1, 2 * strip + 3):
        A, s, v = dlm.regime("A", dt, n)
        plain = dev_t(A)
        buf = torch.full((n * n + 2 * pad,), float("nan"), dtype=TD[dt], device=DEV)
        inside = buf[pad:pad + n * n].view(n, n)
        inside.copy_(plain)
        assert host(dev.colsum(inside)).tobytes() == host(dev.colsum(plain)).tobytes(), (dt, n)
        got, gv, gs, _ = left_round(inside, s, v)
        want, wv, ws, _ = left_round(plain, s, v)
        assert got.tobytes() == want.tobytes() and gv.tobytes() == wv.tobytes() and gs == ws
        assert np.isfinite(got).all()
        assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + n * n:]).all()


# ---------------------------------------------------------------------------
# whole solve
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def _matrix(kind, n, dt):
    if kind == "hilbert":
        return dev.generate("hilbert", n, TD[dt], device=DEV)
    return dev.generate("random", n, TD[dt], seed=17 + n, device=DEV)


@pytest.mark.parametrize("sem", [_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", ["hilbert", "random"])
@pytest.mark.parametrize("n", [5, 64, 257, 1000, 2049])
def test_whole_solve_against_the_solve_of_a_transposed_copy(solver, n, kind, dt, sem):
    import stop_parity as sp
    A = _matrix(kind, n, dt)
    keep = A.clone()
    At = A.T.contiguous()
    max_itr = 200
    lam, u, itr, st = solver.solve(A, left=True, semantics=sem, max_itr=max_itr, trace_sums=True)
    sums_l = solver.last_round_sums()
    lam_r, v_r, itr_r, st_r = solver.solve(At, matrix_free=True, semantics=sem, max_itr=max_itr,
                                           trace_sums=True)
    sums_r = solver.last_round_sums()
    assert torch.equal(A, keep)
    assert sums_l.shape == (st["rounds"], n) and sums_l.dtype == np.dtype(dt)
    u, v_r = host(u), host(v_r)
    if dt == "float64":
        assert itr == itr_r and st["rounds"] == st_r["rounds"], (itr, itr_r)
        assert abs(lam - lam_r) <= 1e-10 * abs(lam_r)
        assert np.max(np.abs(u - v_r)) <= 1e-10 * np.max(np.abs(v_r))
        # u A = lambda u, directly: after the stopping round every column sum
        # of the scaled matrix is within (n - 1) eps of lambda
        a = host(A)
        if st["converged"]:
            resid = np.abs(u @ a - lam * u)
            assert (resid <= (n * 1e-3 + 1e-9 * lam) * u).all(), float((resid / u).max())
    else:
        cmp = sp.compare(sums_l, sums_r, np.float32(1e-3), sem == _lib.ST_SEM_SYCL, max_itr,
                         matrix_free=True)
        if sp.assert_stop_parity(cmp, (n, kind, sem)):
            assert itr == itr_r
            assert abs(lam - lam_r) <= 2e-5 * abs(lam_r)
            assert np.max(np.abs(u - v_r)) <= 5e-4 * np.max(np.abs(v_r))


def test_solve_options_work_on_the_left_operator(solver):
    """Gated batches, timing, exhaustion: solve_device's, on the new kind."""
    A = _matrix("random", 700, "float64")
    base = solver.solve(A, left=True)
    for batch in (1, 3, 50):
        lam, u, itr, st = solver.solve(A, left=True, batch=batch, time_kernels=True)
        assert lam == base[0] and itr == base[2] and torch.equal(u, base[1])
        assert len(solver.last_round_times()) == st["rounds"]
    lam, u, itr, st = solver.solve(A, left=True, eps=0.0, max_itr=5)
    lam_r, v_r, itr_r, st_r = solver.solve(A.T.contiguous(), matrix_free=True, eps=0.0, max_itr=5)
    assert st["rounds"] == st_r["rounds"] == 5 and itr == itr_r and not st["converged"]
    assert abs(lam - lam_r) <= 1e-10 * lam_r


def test_markov_chain_stationary_distribution(solver):
    n = 300
    P = np.random.default_rng(2024).random((n, n)) + 0.01
    P /= P.sum(axis=1, keepdims=True)
    Pd = dev_t(P)
    lam, v, itr, st = solver.solve(Pd)                  # row sums are 1: round 0 stops
    assert st["rounds"] == 1 and st["converged"] and abs(lam - 1.0) < 1e-12
    assert np.allclose(host(v), 1.0, rtol=0, atol=1e-12)
    lam, u, itr, st = solver.solve(Pd, left=True, eps=1e-9)
    assert st["converged"] and abs(lam - 1.0) < 1e-6
    pi = host(u) / host(u).sum()
    assert np.max(np.abs(pi @ P - pi)) < 1e-6
    assert (pi > 0).all() and abs(pi.sum() - 1.0) < 1e-12


def test_no_copy_of_the_matrix(solver):
    n = 4096
    A = dev.generate("random", n, torch.float32, seed=1, device=DEV)
    keep = A.clone()
    solver.solve(A, left=True, max_itr=3)               # workspaces exist from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    solver.solve(A, left=True, max_itr=20)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < A.numel() * A.element_size() // 2
    assert torch.equal(A, keep)


@pytest.mark.parametrize("dt", DTYPES)
def test_stored_transpose_runs_the_ordinary_solve_without_a_copy(solver, dt):
    n = 2049
    B = dev.generate("random", n, TD[dt], seed=3, device=DEV)
    want = solver.solve(B, matrix_free=True, max_itr=50)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    got = solver.solve(B.T, left=True, max_itr=50)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < B.numel() * B.element_size() // 2
    assert got[0] == want[0] and got[2] == want[2] and torch.equal(got[1], want[1])


def test_refusals_by_name(solver):
    A = dev.generate("random", 64, torch.float32, seed=1, device=DEV)
    with pytest.raises(ValueError, match="inplace"):
        solver.solve(A, left=True, inplace=True)
    for flag in ("round_loop", "write_every_round"):
        with pytest.raises(ValueError, match=flag):
            solver.solve(A, left=True, **{flag: True})
    for half in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="16-bit"):
            solver.solve(A.to(half), left=True)
    with pytest.raises(TypeError, match="left"):
        solver.solve_half(A.to(torch.float16), left=True)
    stack = A.reshape(1, 64, 64)
    with pytest.raises(TypeError, match="left"):
        solver.solve_batched(stack, left=True)
    with pytest.raises(TypeError, match="left"):
        solver.solve_vbatched([A], left=True)
    # the C entry refuses the writing forms' flags by name
    ev, it = ctypes.c_float(), ctypes.c_uint32()
    v = torch.empty(64, dtype=torch.float32, device=DEV)
    opt = _lib.st_options(-1.0, 0, 0, 0, _lib.ST_FLAG_BATCH_ROUNDS)
    rc = solver.L.st_solve_device_left_f32(solver.q, A.data_ptr(), 64, v.data_ptr(), None,
                                           ctypes.byref(ev), ctypes.byref(it),
                                           ctypes.byref(opt), None)
    assert rc == -1 and "ST_FLAG_BATCH_ROUNDS" in _lib.last_error(solver.L)
