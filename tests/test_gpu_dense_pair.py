"""GPU: the dense Perron pair kernels (k_pair_sum, k_pair_sweep with
k_csr_prep and k_left_finish) and solve_pair(A).

The sizes: RB (rows per block) and S (the strip, columns per workgroup) come
from the shape query; the set holds the small sizes, the sizes around one and
two tiles and around one, two and (past the issue's list, for the serial
combine of more than three strips) three strips, odd ones among them (rows
that are not 16-byte aligned take the element-wide path).

The right side's order is compared by bytes with the host model
(dense_pair_order_model) on the rows model_rows picks; the left side is
compared by bytes with the left solve's own kernels on every column; every row
of every size up to 1024 is compared byte for byte with the existing
matrix-free round in the exact-input test, which needs no model."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import csr_order_model as com                      # noqa: E402
import dense_left_order_model as dlm               # noqa: E402
import dense_pair_order_model as dpm               # noqa: E402
from eigen_value_amd import _lib                   # noqa: E402
from eigen_value_amd import device as dev          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = ("float32", "float64")
TD = {"float32": torch.float32, "float64": torch.float64}
CODE = {"float32": _lib.DTYPE_F32, "float64": _lib.DTYPE_F64}
SYCL, MAINPY = _lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY
POISON = -7.0
IN_FLIGHT = 8


def sizes(dt):
    sh = _lib.pair_shape(CODE[dt], 1)
    rb, S = sh["rows"], sh["strip"]
    return sorted({1, 2, 3, 5, 63, 64, 65, rb - 1, rb, rb + 1, 2 * rb + 1, S - 1, S, S + 1,
                   2 * S + 3, 2049, 3 * S + 5})


def test_sizes_hold_what_the_kernels_branch_on():
    for dt in DTYPES:
        S = sizes(dt)
        sh = {n: _lib.pair_shape(CODE[dt], n) for n in S}
        w, strip = sh[1]["w"], sh[1]["strip"]
        assert {1, 2, 3, 5, 63, 64, 65, 2049, strip - 1, strip, strip + 1, 2 * strip + 3} <= set(S)
        assert any(n % w for n in S) and any(n % w == 0 and n > 1 for n in S)   # both loads
        assert {1, 2} <= {sh[n]["nstrips"] for n in S}                 # one and two strips
        assert any(sh[n]["nstrips"] >= 4 for n in S)     # serial differs from a tree from 4 on
        tiles = {n: -(-n // sh[n]["rows"]) for n in S}
        assert 1 in tiles.values() and any(t > 2 for t in tiles.values())
        # a last tile shorter than the rows in flight, and one with a tail after whole groups
        last = {n: n - (tiles[n] - 1) * sh[n]["rows"] for n in S}
        assert any(l < IN_FLIGHT for l in last.values())
        assert any(l > IN_FLIGHT and l % IN_FLIGHT for l in last.values())
        assert len({sh[n]["rows"] for n in S}) >= 2                    # the table's second row
        assert any(n % strip and n % strip <= 192 * w for n in S if n > strip)  # idle waves
        assert sh[1]["rows_in_flight"] == IN_FLIGHT


def dev_t(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)   # (regimes are read-only)


def host(t):
    return t.cpu().numpy()


def state_bytes(end=0, done=0):
    st = _lib.st_state()
    st.end, st.done = end, done
    return bytes(st)


def new_states(right=None, left=None):
    raw = (right or state_bytes()) + (left or state_bytes())
    return torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).to(DEV)


def offsets(dt, n):
    """(x_left, colpart, rowpart, total) of the scratch, in elements."""
    sh = _lib.pair_shape(CODE[dt], n)
    up = lambda e: -(-e // 64) * 64                        # noqa: E731
    col = 2 * up(n)
    row = col + up(-(-n // sh["rows"]) * n)
    return up(n), col, row, row + sh["nstrips"] * n


def pair_round(A, sr, vr, sl, vl, *, k=1, eps=1e-3, max_itr=1000, sem=SYCL, states=None,
               poison_scratch=False):
    """One launch on the device matrix A from host vectors, every output
    prefilled with POISON: a dict of host arrays, the two states' bytes and the
    scratch."""
    n, td = A.shape[0], A.dtype
    states = new_states() if states is None else states
    out = {key: torch.full((n,), POISON, dtype=td, device=DEV)
           for key in ("s_r", "v_r", "s_l", "v_l")}
    scratch = dev.pair_scratch(n, td, DEV)
    if poison_scratch:
        scratch.fill_(POISON)
    dev.mfree_pair_round(A, (dev_t(sr), out["s_r"], dev_t(vr), out["v_r"]),
                         (dev_t(sl), out["s_l"], dev_t(vl), out["v_l"]), scratch, states,
                         eps=eps, k=k, max_itr=max_itr, semantics=sem)
    res = {key: host(t) for key, t in out.items()}
    raw = host(states).tobytes()
    res["st_r"], res["st_l"], res["scratch"], res["states"] = raw[:64], raw[64:], scratch, states
    return res


def left_round(A, s, v, *, k=1, eps=1e-3, max_itr=1000, sem=SYCL, state=None):
    n = A.shape[0]
    state = dev.new_state(DEV) if state is None else state
    s_next = torch.full((n,), POISON, dtype=A.dtype, device=DEV)
    v_cur = torch.full((n,), POISON, dtype=A.dtype, device=DEV)
    scratch = dev.left_scratch(n, A.dtype, DEV)
    dev.mfree_left_round(A, dev_t(s), s_next, dev_t(v), v_cur, scratch, state, eps=eps, k=k,
                         max_itr=max_itr, semantics=sem)
    return host(s_next), host(v_cur), host(state).tobytes()


def right_round(A, s, v, *, k=1, eps=1e-3, max_itr=1000, sem=SYCL, state=None):
    n = A.shape[0]
    state = dev.new_state(DEV) if state is None else state
    s_next = torch.full((n,), POISON, dtype=A.dtype, device=DEV)
    v_cur = torch.full((n,), POISON, dtype=A.dtype, device=DEV)
    dev.mfree_round(A, dev_t(s), s_next, dev_t(v), v_cur, state, eps=eps, k=k, max_itr=max_itr,
                    semantics=sem)
    return host(s_next), host(v_cur), host(state).tobytes()


# ---------------------------------------------------------------------------
# 1. the right side's order; v and the states of both sides
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", dlm.REGIMES)
def test_right_order_matches_the_host_model(name, dt):
    for n in sizes(dt):
        rb, S, _ = dpm.shape(dt, n)
        A, s, v = dlm.regime(name, dt, n)
        rows = dpm.model_rows(n, rb)
        Ad = dev_t(A)
        s0_r, s0_l = (host(t) for t in dev.pair_sum(Ad))
        assert s0_r[rows].tobytes() == dpm.rows(A, None, dt, rows).tobytes(), (name, dt, n, "sum")
        assert s0_l.tobytes() == host(dev.colsum(Ad)).tobytes(), (name, dt, n, "colsum")
        # the two sides get different vectors: the left one the regime's, swapped
        res = pair_round(Ad, s, v, v, s)
        x = v * s
        num = dpm.rows(A, x, dt, rows)
        with np.errstate(all="ignore"):
            want = num / x[rows]
        assert res["s_r"][rows].tobytes() == want.tobytes(), (name, dt, n, "s_next")
        _, v_ref, st_ref = right_round(Ad, s, v)
        assert res["v_r"].tobytes() == v_ref.tobytes() and res["st_r"] == st_ref, (name, dt, n)
        l_next, l_cur, l_state = left_round(Ad, v, s)
        assert res["s_l"].tobytes() == l_next.tobytes(), (name, dt, n, "left s_next")
        assert res["v_l"].tobytes() == l_cur.tobytes() and res["st_l"] == l_state, (name, dt, n)


# ---------------------------------------------------------------------------
# 2. the left side is the left solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sem", [SYCL, MAINPY])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", dlm.REGIMES)
def test_left_side_equals_the_left_round_over_three_launches(name, dt, sem):
    """Going-on, stopping and exhausted rounds over launches 1 .. 3 at every
    size: s_next, v_cur and the 64 bytes of the state of the pair's left side
    are mfree_left_round's, whatever the right side (fed the regime's own
    vectors throughout) does."""
    for n in sizes(dt):
        A, s, v = dlm.regime(name, dt, n)
        Ad = dev_t(A)
        rng = np.random.default_rng(7 + n)
        rough = [(1.0 + rng.random(n)).astype(dt) for _ in range(3)]
        flat = np.full(n, 2.0, dt)
        plans = {"going_on": (rough, 1000), "stop_at_2": ([rough[0], flat, rough[2]], 1000),
                 "exhaust_at_2": (rough, 2)}
        for tag, (svecs, max_itr) in plans.items():
            st_pair, st_left = new_states(), dev.new_state(DEV)
            vl = np.ones(n, dt)
            for k in (1, 2, 3):
                res = pair_round(Ad, s, v, svecs[k - 1], vl, k=k, max_itr=max_itr, sem=sem,
                                 states=st_pair)
                l_next, l_cur, l_state = left_round(Ad, svecs[k - 1], vl, k=k, max_itr=max_itr,
                                                    sem=sem, state=st_left)
                key = (name, dt, sem, n, tag, k)
                assert res["s_l"].tobytes() == l_next.tobytes(), key
                assert res["v_l"].tobytes() == l_cur.tobytes() and res["st_l"] == l_state, key
                if (l_cur != POISON).all():
                    vl = l_cur
            end = dev.read_state(st_left)["end"]
            if n > 1:                       # (one entry: the stop test has no pair to fail)
                assert (end == 2) == (tag != "going_on"), (name, dt, n, tag, end)


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


@pytest.mark.parametrize("sem", [SYCL, MAINPY])
@pytest.mark.parametrize("dt", DTYPES)
def test_whole_solve_left_side_is_solve_left(solver, dt, sem):
    S = _lib.pair_shape(CODE[dt], 1)["strip"]
    for n in (1, 5, 65, 300, S + 1, 2049):
        A = dev.generate("random", n, TD[dt], seed=17 + n, device=DEV)
        keep = A.clone()
        lam, vecs, its, st = solver.solve_pair(A, semantics=sem, max_itr=200)
        lam_l, u, it_l, st_l = solver.solve(A, left=True, semantics=sem, max_itr=200)
        assert torch.equal(A, keep)
        assert lam[1] == lam_l and its[1] == it_l and torch.equal(vecs[1], u), (dt, n)
        assert st["converged_sides"][1] == st_l["converged"]
        lam_r, v, it_r, st_r = solver.solve(A, matrix_free=True, semantics=sem, max_itr=200)
        tol = 1e-10 if dt == "float64" else 2e-5
        assert abs(lam[0] - lam_r) <= tol * abs(lam_r), (dt, n)
        assert st["rounds"] == max(dev_rounds(its, st, sem))
        assert st["converged"] == int(all(st["converged_sides"]))


def dev_rounds(its, st, sem):
    """The launch that ended each side, from its count (SYCL: the stopping
    round's index; main.py: one more; exhausted: max_itr either way)."""
    return [it + 1 if (sem == SYCL and c) else it for it, c in zip(its, st["converged_sides"])]


# ---------------------------------------------------------------------------
# 3. exact inputs against the existing kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_exact_inputs_equal_the_existing_rounds(dt):
    """Entries in {1, 2, 3, 4}: every partial sum of launch 0 and launch 1 is
    an integer <= 16 n^2 <= 2^24, exact in fp32 in any order, so every row must
    equal k_rowsum's / k_mfree's and every column k_colsum's / k_left_sweep's
    bit for bit.  (Later launches are not exact and are not claimed.)"""
    for n in [m for m in sizes(dt) if m <= 1024]:
        rng = np.random.default_rng(100 + n)
        A = rng.integers(1, 5, size=(n, n)).astype(dt)
        Ad = dev_t(A)
        s0_r, s0_l = (host(t) for t in dev.pair_sum(Ad))
        assert s0_r.tobytes() == host(dev.rowsum(Ad)).tobytes(), (dt, n)
        assert s0_r.tobytes() == A.sum(axis=1, dtype=np.float64).astype(dt).tobytes()
        assert s0_l.tobytes() == A.sum(axis=0, dtype=np.float64).astype(dt).tobytes()
        ones = np.ones(n, dt)
        res = pair_round(Ad, s0_r, ones, s0_l, ones)
        r_next, r_cur, r_state = right_round(Ad, s0_r, ones)
        assert res["s_r"].tobytes() == r_next.tobytes(), (dt, n)
        assert res["v_r"].tobytes() == r_cur.tobytes() and res["st_r"] == r_state, (dt, n)
        l_next, l_cur, l_state = left_round(Ad, s0_l, ones)
        assert res["s_l"].tobytes() == l_next.tobytes(), (dt, n)
        assert res["v_l"].tobytes() == l_cur.tobytes() and res["st_l"] == l_state, (dt, n)


# ---------------------------------------------------------------------------
# 4. error
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_right_error_is_within_the_bound_of_the_order(dt, capsys):
    """Every row of pair_sum and every numerator of a round against the exact
    rational sum: at most Wc + 6 + 3 + (nstrips - 1) + 1 roundings
    (dense_pair_order_model.bound_ulps; DESIGN.md records the largest seen).
    The numerator is read back from the row partials the round leaves in the
    scratch, added as k_left_finish adds them."""
    worst = 0.0
    for n in (65, 133):
        _, S, _ = dpm.shape(dt, n)
        bound = dpm.bound_ulps(n, S)
        _, _, row0, total = offsets(dt, n)
        for name in dlm.REGIMES:
            A, s, v = dlm.regime(name, dt, n)
            x = v * s
            Ad = dev_t(A)
            s0 = host(dev.pair_sum(Ad)[0])
            res = pair_round(Ad, s, v, s, v)
            part = host(res["scratch"])[row0:total].reshape(-1, n)
            num = part[0].copy()
            for j in range(1, part.shape[0]):
                num = num + part[j]
            with np.errstate(all="ignore"):
                assert (num / x).tobytes() == res["s_r"].tobytes(), (dt, n, name)
            for r in range(n):
                e0 = com.err_ulps(s0[r], dpm.exact_row(A[r]), dt)
                e1 = com.err_ulps(num[r], dpm.exact_row(A[r], x), dt)
                assert e0 <= bound and e1 <= bound, (dt, n, name, r, e0, e1, bound)
                worst = max(worst, e0, e1)
    with capsys.disabled():
        print(f"\n[dense pair] {dt}: largest right-side error {worst:.3f} ulps")


# ---------------------------------------------------------------------------
# 5. the sides stop alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_a_stochastic_matrix_stops_one_side_at_round_zero(solver, dt):
    for n in (65, 133, 300):
        P = np.random.default_rng(2024 + n).random((n, n)) + 0.01
        P = (P / P.sum(axis=1, keepdims=True)).astype(dt)
        for M, early, late in ((P, 0, 1), (np.ascontiguousarray(P.T), 1, 0)):
            Md = dev_t(M)
            lam, vecs, its, st = solver.solve_pair(Md)
            lam_r, v, it_r, st_r = solver.solve(Md, matrix_free=True)
            lam_l, u, it_l, st_l = solver.solve(Md, left=True)
            assert lam[1] == lam_l and its[1] == it_l and torch.equal(vecs[1], u), (dt, n)
            ref = (it_r, it_l)
            assert its[early] == ref[early] == 0, (dt, n, its, ref)    # round 0, v = 1
            assert np.allclose(host(vecs[early]), 1.0, rtol=0, atol=1e-5)
            assert its[late] > 0 and st["converged_sides"] == [1, 1], (dt, n, its)
            assert abs(lam[0] - lam_r) <= (1e-10 if dt == "float64" else 2e-5) * abs(lam_r)
            assert st["rounds"] == its[late] + 1


@pytest.mark.parametrize("dt", DTYPES)
def test_a_side_does_not_depend_on_whether_the_other_is_live(dt):
    """Launch 2 with each side's state live (fresh) or ended (end = 1): what a
    live side writes - s_next, v_cur, its state, its x and its partials - is the
    same bytes either way; an ended side's outputs, x and partials keep their
    prefill; with both ended nothing at all is written."""
    S = _lib.pair_shape(CODE[dt], 1)["strip"]
    ended = state_bytes(end=1, done=1)
    for n in (65, S + 1):
        A, s, v = dlm.regime("A", dt, n)
        Ad = dev_t(A)
        xl, col, row, total = offsets(dt, n)
        run = {}
        for r_live in (True, False):
            for l_live in (True, False):
                st = new_states(None if r_live else ended, None if l_live else ended)
                res = pair_round(Ad, s, v, v, s, k=2, states=st, poison_scratch=True)
                res["scratch"] = host(res["scratch"])
                run[r_live, l_live] = res
        both = run[True, True]
        sc = both["scratch"]
        assert not (both["s_r"] == POISON).any() and not (both["s_l"] == POISON).any()
        assert not (sc[:n] == POISON).any() and not (sc[xl:xl + n] == POISON).any()
        nrb = -(-n // _lib.pair_shape(CODE[dt], n)["rows"])
        assert not (sc[col:col + nrb * n] == POISON).any() and not (sc[row:total] == POISON).any()
        one = run[True, False]                       # the right side alone
        for key in ("s_r", "v_r"):
            assert one[key].tobytes() == both[key].tobytes(), (dt, n, key)
        assert one["st_r"] == both["st_r"] and one["st_l"] == ended
        assert one["scratch"][:n].tobytes() == sc[:n].tobytes()
        assert one["scratch"][row:total].tobytes() == sc[row:total].tobytes()
        assert (one["s_l"] == POISON).all() and (one["v_l"] == POISON).all()
        assert (one["scratch"][xl:row] == POISON).all()          # x_L and the column partials
        one = run[False, True]                       # the left side alone
        for key in ("s_l", "v_l"):
            assert one[key].tobytes() == both[key].tobytes(), (dt, n, key)
        assert one["st_l"] == both["st_l"] and one["st_r"] == ended
        assert one["scratch"][xl:row].tobytes() == sc[xl:row].tobytes()
        assert (one["s_r"] == POISON).all() and (one["v_r"] == POISON).all()
        assert (one["scratch"][:xl] == POISON).all() and (one["scratch"][row:] == POISON).all()
        none = run[False, False]
        assert all((none[key] == POISON).all() for key in ("s_r", "v_r", "s_l", "v_l", "scratch"))
        assert none["st_r"] == ended and none["st_l"] == ended


# ---------------------------------------------------------------------------
# 6. lane width and bounds
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_the_kind_of_load_does_not_enter_and_nothing_outside_is_read(dt):
    """A placed one element into a NaN-filled buffer (not 16-byte aligned: the
    element-wide loads) at sizes that are multiples of the lane's columns (the
    aligned copy takes 16-byte loads): the same bytes on both sides, all
    finite, so nothing outside A entered a sum."""
    sh = _lib.pair_shape(CODE[dt], 1)
    S, rb, w = sh["strip"], sh["rows"], sh["w"]
    for n in (S, 2 * S, 2 * rb * w + w):
        assert n % w == 0
        A, s, v = dlm.regime("A", dt, n)
        plain = dev_t(A)
        buf = torch.full((n * n + 2,), float("nan"), dtype=TD[dt], device=DEV)
        inside = buf[1:1 + n * n].view(n, n)
        inside.copy_(plain)
        assert plain.data_ptr() % 16 == 0 and inside.data_ptr() % 16 != 0
        for a, b in zip(dev.pair_sum(inside), dev.pair_sum(plain)):
            assert host(a).tobytes() == host(b).tobytes(), (dt, n)
            assert np.isfinite(host(a)).all()
        got, want = pair_round(inside, s, v, v, s), pair_round(plain, s, v, v, s)
        for key in ("s_r", "v_r", "s_l", "v_l", "st_r", "st_l"):
            g, w_ = got[key], want[key]
            assert (g if isinstance(g, bytes) else g.tobytes()) == \
                (w_ if isinstance(w_, bytes) else w_.tobytes()), (dt, n, key)
        assert np.isfinite(got["s_r"]).all() and np.isfinite(got["s_l"]).all()
        assert torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + n * n:]).all()


# ---------------------------------------------------------------------------
# 7. the whole solve against numpy
# ---------------------------------------------------------------------------
def test_whole_solve_against_numpy(solver):
    """Collatz-Wielandt: lambda lies between min and max of s, and at the stop
    adjacent entries of s differ by less than eps, so s[0] is within (n - 1) eps
    of lambda; the returned vector is A x / (m m') for the x of the stopping
    round, whose residual is at most that bound times the vector, entry by
    entry."""
    eps = 1e-9
    for n in (65, 300):
        A = np.random.default_rng(31 + n).random((n, n)) + 0.5
        lam, vecs, its, st = solver.solve_pair(dev_t(A), eps=eps, max_itr=500)
        assert st["converged_sides"] == [1, 1] and st["converged"] == 1
        top = np.max(np.abs(np.linalg.eigvals(A)))
        slack = 64 * n * np.finfo(np.float64).eps * top
        bound = (n - 1) * eps + slack
        assert abs(lam[0] - top) <= bound and abs(lam[1] - top) <= bound, (n, lam, top)
        v, u = host(vecs[0]), host(vecs[1])
        assert (v > 0).all() and (u > 0).all()
        assert np.max(np.abs(A @ v - lam[0] * v)) <= bound * v.max(), n
        assert np.max(np.abs(u @ A - lam[1] * u)) <= bound * u.max(), n


# ---------------------------------------------------------------------------
# 8. refusals and options
# ---------------------------------------------------------------------------
def test_refusals_by_name(solver):
    A = dev.generate("random", 64, torch.float32, seed=1, device=DEV)
    for half in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="solve_half"):
            solver.solve_pair(A.to(half))
    elsewhere = object.__new__(dev.DeviceSolver)      # a context on another device: only
    elsewhere.device = torch.device("cuda:1")         # the check before any call is reached
    with pytest.raises(ValueError, match="solver context on"):
        dev.DeviceSolver.solve_pair(elsewhere, A)
    ev, it = (ctypes.c_float * 2)(), (ctypes.c_uint32 * 2)()
    v = torch.empty((2, 64), dtype=torch.float32, device=DEV)
    for flag, name in ((_lib.ST_FLAG_TIME_KERNELS, "ST_FLAG_TIME_KERNELS"),
                       (_lib.ST_FLAG_TRACE_SUMS, "ST_FLAG_TRACE_SUMS"),
                       (_lib.ST_FLAG_ROUND_LOOP, "ST_FLAG_ROUND_LOOP"),
                       (_lib.ST_FLAG_WRITE_EVERY_ROUND, "ST_FLAG_WRITE_EVERY_ROUND"),
                       (_lib.ST_FLAG_BATCH_ROUNDS, "ST_FLAG_BATCH_ROUNDS")):
        opt = _lib.st_options(-1.0, 0, 0, 0, flag)
        rc = solver.L.st_solve_device_pair_f32(solver.q, A.data_ptr(), 64, v.data_ptr(), None,
                                               ev, it, None, ctypes.byref(opt), None)
        msg = _lib.last_error(solver.L)
        assert rc == -1 and "not supported" in msg and name in msg, (name, msg)


@pytest.mark.parametrize("dt", DTYPES)
def test_options(solver, dt):
    A = dev.generate("random", 700, TD[dt], seed=5, device=DEV)
    lam, vecs, its, st = solver.solve_pair(A, max_itr=1)
    assert st["converged_sides"] == [0, 0] and st["converged"] == 0 and its == [1, 1]
    base = solver.solve_pair(A, batch=1)
    for batch in (8, 3):
        lam, vecs, its, st = solver.solve_pair(A, batch=batch)
        assert lam == base[0] and its == base[2] and torch.equal(vecs, base[1]), (dt, batch)
        assert st["fused_launches"] >= st["rounds"]
    B = A.t()                                      # non-contiguous: solved as its copy
    lam, vecs, its, st = solver.solve_pair(B)
    want = solver.solve_pair(B.contiguous())
    assert lam == want[0] and torch.equal(vecs, want[1])


@pytest.mark.parametrize("dt", DTYPES)
def test_numpy_front_equals_the_device_solver(solver, dt):
    from eigen_value_amd.similarity_transform import EigenValue
    n = 133
    A = (np.random.default_rng(9).random((n, n)) + 0.25).astype(dt)
    with EigenValue() as ev:
        lam, vecs, ts, its = ev.similarity_transform_pair(A)
    lam_d, vecs_d, its_d, st = solver.solve_pair(dev_t(A))
    assert lam.dtype == np.dtype(dt) and vecs.shape == (2, n) and ts >= 0
    assert [float(x) for x in lam] == lam_d and list(its) == its_d
    assert vecs.tobytes() == host(vecs_d).tobytes()
    assert ev.last_pair_stats["converged_sides"] == st["converged_sides"]
