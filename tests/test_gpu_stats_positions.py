"""GPU: the stop test and the maximum at every boundary position.

Every round kernel folds m_k = max(0, max s_k) and stop_k = all
|s_i - s_{i+1}| < eps into its own sweep of s_k (stats_at in k_round /
k_round_split, k_flat's first row group merged per piece with atomics,
mfree_group, k_epilogue, the per-thread forms of k_solve_small and
k_solve_batched).  The other step-level tests feed them random s (every pair
fails) or constant s (every pair passes); here the ONE pair that decides, or
the one element that is the maximum, sits in turn at each vector, lane, wave,
unroll-step, tail, piece, split-range and wrap boundary
(tests/stats_vectors.py, whose constructions tests/test_stats_vectors.py
proves on the CPU), so a kernel that drops one pair or one element fails.

Everything is equality: the state against the oracle (orc.stop /
orc.find_max) and numpy in the same dtype, v against numpy's v0 * (s / m)
in the dtype (NaN entries compare as NaN).  No tolerance.

The block is 5 rows at row0 = 3 of an n-long s: n = 9, 257 and 1031 take the
element-wide path (W = 1), 1032 ... 8200 the vector path; a flat piece is
1024 columns in every form, so 1032 / 2056 / 4104 / 8200 leave an 8-column
last piece after 1 / 2 / 4 / 8 whole ones.

Not reachable from here: the non-temporal instantiations (blocks of 2 GiB
and more; the full-size solve tests run them) and k_stats as a launch of
its own (the three-launch form is compiled out).
"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
import stats_vectors as sv  # noqa: E402

DEV = "cuda:0"
TD = {np.float64: torch.float64, np.float32: torch.float32}
SEMS = [_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY]
NROWS, ROW0 = 5, 3
K = 2                    # the round number of the step-level launches
MAX_ITR = 1000

STATE_DT = np.dtype([("done", "<u4"), ("round", "<u4"), ("iters", "<u4"), ("stop", "<u4"),
                     ("eigen_val", "<f8"), ("max", "<f8"), ("end", "<u4"),
                     ("arrivals", "<u4"), ("max_bits", "<u8"), ("fail", "<u4"),
                     ("pad0", "<u4"), ("pad", "<u8")])
assert STATE_DT.itemsize == 64


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


# ---------------------------------------------------------------------------
# the cases: built once per (n, dtype, semantics), never written
# ---------------------------------------------------------------------------
_CASES = {}


def cases(orc, n, dt, cyclic, only=None):
    """tags, S (case, n), eps, and what the oracle and numpy say of each row:
    stop and m.  `only`: restrict the positions (the full-size leg)."""
    key = (n, np.dtype(dt).name, cyclic, None if only is None else tuple(only))
    if key in _CASES:
        return _CASES[key]
    eps, ee = dt(sv.EPS), dt(sv.EXACT_EPS)
    rows = []                                       # (tag, s, eps, designed stop)
    # `only`: those positions, where the semantics has a pair / an element there
    pick = (lambda ps: [p for p in sorted(only) if p <= ps[-1]]) if only is not None else (
        lambda ps: ps)
    for p in pick(sv.positions(n, dt, cyclic)):
        rows += [(("one_fail", p), sv.one_fail(n, p, dt, eps, cyclic), eps, 0),
                 (("all_pass", p), sv.all_pass(n, p, dt, eps, cyclic), eps, 1),
                 (("exact_fail", p), sv.exact_eps(n, p, dt, "fail", cyclic), ee, 0),
                 (("exact_pass", p), sv.exact_eps(n, p, dt, "pass", cyclic), ee, 1)]
    for p in pick(sv.positions(n, dt, True)):       # an element, not a pair: p = n - 1 too
        rows += [(("max_at", p), sv.max_at(n, p, dt, eps), eps, 1),
                 (("max_decoys", p), sv.max_at(n, p, dt, eps, decoys=True), eps, 0),
                 (("nan_at", p), sv.nan_at(n, p, dt), eps, 0)]
    c = types.SimpleNamespace(n=n, dt=dt, cyclic=cyclic)
    c.tags = [r[0] for r in rows]
    c.S = np.stack([r[1] for r in rows])
    c.eps = np.array([r[2] for r in rows], dtype=dt)
    c.stop = np.array([int(orc.stop(r[1], r[2], cyclic)) for r in rows])
    c.m = np.array([orc.find_max(r[1]) for r in rows], dtype=dt)
    # the oracle, numpy and the construction agree before any kernel is asked
    assert c.stop.tolist() == [r[3] for r in rows]
    assert c.stop.tolist() == [int(not sv.failing_pairs(r[1], r[2], cyclic)) for r in rows]
    assert c.m.tolist() == [sv.find_max(r[1]) for r in rows]
    for a in (c.S, c.eps, c.stop, c.m):
        a.setflags(write=False)
    _CASES[key] = c
    return c


def same(got, exp):
    """Elementwise equality with NaN == NaN (a NaN in s gives a NaN in v and,
    at index 0, in lambda; everything else is compared bit for bit)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.dtype.kind != "f":
        return got == exp
    return (got == exp) | (np.isnan(got) & np.isnan(exp))


def check(what, got, exp, jobs, c):
    ok = same(got, exp)
    if ok.ndim > 1:
        ok = ok.all(axis=tuple(range(1, ok.ndim)))
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (what, c.n, np.dtype(c.dt).name, "cyclic" if c.cyclic else "open",
                           f"{bad.size} of {ok.size}",
                           [(c.tags[jobs[b][0]], jobs[b][1]) for b in bad[:6]])


def expect_v(c, ci, v0, full):
    with np.errstate(invalid="ignore"):
        upd = v0[None, :] * (c.S[ci] / c.m[ci][:, None])        # cpp:260, in the dtype
    assert upd.dtype == c.dt
    if full:
        return upd
    out = np.tile(v0, (len(ci), 1))
    out[:, ROW0:ROW0 + NROWS] = upd[:, ROW0:ROW0 + NROWS]
    return out


def sweep(orc, dt, sem, n, launch, *, full_v=False, flat=False, rk=K, epilogue=False,
          jobs_of=None, setup=None):
    """Run `launch(x, j, ci, extra)` for every job (case ci, extra), each with
    its own v and state, read everything back once and compare."""
    cyclic = sem == _lib.ST_SEM_SYCL
    c = cases(orc, n, dt, cyclic)
    jobs = [(ci, None) for ci in range(len(c.tags))] if jobs_of is None else jobs_of(c)
    v0 = orc.random_matrix(n, 5, dt, nrows=1)[0]
    x = types.SimpleNamespace(n=n, sem=sem, c=c)
    x.mat = torch.from_numpy(orc.random_matrix(n, 3, dt, nrows=NROWS, row0=ROW0)).to(DEV)
    x.S = torch.tensor(c.S, device=DEV)
    x.v0 = torch.from_numpy(v0).to(DEV)
    x.V = x.v0.repeat(len(jobs), 1)
    x.ST = torch.zeros((len(jobs), 64), dtype=torch.uint8, device=DEV)
    x.s_next = torch.empty(n, dtype=TD[dt], device=DEV)
    x.eps = [float(e) for e in c.eps]
    if setup is not None:
        setup(x)
    for j, (ci, extra) in enumerate(jobs):
        launch(x, j, ci, extra)
    torch.cuda.synchronize()
    st = np.frombuffer(x.ST.cpu().numpy().tobytes(), dtype=STATE_DT)
    ci = np.array([job[0] for job in jobs])
    stop = c.stop[ci]
    check("stop", st["stop"], stop, jobs, c)
    check("max", st["max"], c.m[ci].astype(np.float64), jobs, c)
    check("eigen_val", st["eigen_val"], c.S[ci, 0].astype(np.float64), jobs, c)
    check("done", st["done"], stop, jobs, c)
    if epilogue:     # k_epilogue counts the rounds itself and has no `end`
        check("round", st["round"], 1 - stop, jobs, c)
        check("iters", st["iters"], stop * (0 if cyclic else 1), jobs, c)
        check("end", st["end"], 0 * stop, jobs, c)
    else:            # test_round_stop_and_gating's bookkeeping, round rk
        check("round", st["round"], rk + 0 * stop, jobs, c)
        check("iters", st["iters"], stop * (rk if cyclic else rk + 1), jobs, c)
        check("end", st["end"], stop * (rk + 1), jobs, c)
    if flat:         # the scratch words are left zeroed
        for w in ("arrivals", "max_bits", "fail"):
            check(w, st[w], 0 * stop, jobs, c)
    check("v", x.V.cpu().numpy(), expect_v(c, ci, v0, full_v), jobs, c)


def split_ranges(n, dt, p):
    """Local column ranges [col0, col1) that put the pair starting at p in
    turn just before col0, at col0, at col1 - 1, at col1 and far from both
    (in vectors where n takes the vector path, whose ranges are multiples of
    W), and one odd range, which takes the element-wide path at any n."""
    w = 16 // np.dtype(dt).itemsize
    if n % w:
        w = 1
    span = 40 * w + (0 if w > 1 else 3)
    lo, hi = (p // w) * w, min(n, (p // w + 1) * w)
    out = [(hi, min(n, hi + span)),                 # p in the last vector before col0
           (lo, min(n, lo + span)),                 # p in the first vector of the range
           (max(0, hi - span), hi),                 # p in the last vector of the range
           (max(0, lo - span), lo),                 # p in the first vector after col1
           ((3 * n // 4) // w * w, n) if p < n // 2 else (0, (n // 4) // w * w)]
    odd0 = p | 1
    if odd0 < n:
        out.append((odd0, min(n, odd0 + 33)))       # p (or p + 1) = col0, odd
    assert all(0 <= a <= b <= n for a, b in out)
    return out


def split_jobs(c):
    # the pair positions only matter against col0 / col1; the element cases
    # (max, NaN) take every range too
    return [(ci, r) for ci, tag in enumerate(c.tags)
            for r in split_ranges(c.n, c.dt, tag[1])]


PARAMS = [pytest.param(dt, sem, n, id=f"{np.dtype(dt).name}-{'sycl' if sem == 0 else 'mainpy'}-{n}")
          for dt in (np.float64, np.float32) for sem in SEMS for n in sv.SIZES]


# ---------------------------------------------------------------------------
# 1 - 7: the step-level kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,sem,n", PARAMS)
def test_fused_round(orc, dt, sem, n):
    """k_round: stats_at in round_group's unrolled body and sweep_tail."""
    def launch(x, j, ci, _):
        dev.fused_round(x.mat, x.S[ci], x.s_next, x.V[j], x.ST[j], row0=ROW0, eps=x.eps[ci],
                        k=K, max_itr=MAX_ITR, semantics=sem)
    sweep(orc, dt, sem, n, launch)


@pytest.mark.parametrize("dt,sem,n", PARAMS)
def test_split_round(orc, dt, sem, n):
    """k_round_split local then remote: the remote sweep's two spans and the
    extra pass over the local range [q0, q1)."""
    def setup(x):
        x.part = torch.empty(NROWS, dtype=TD[dt], device=DEV)

    def launch(x, j, ci, r):
        kw = dict(row0=ROW0, col0=r[0], col1=r[1], eps=x.eps[ci], k=K, max_itr=MAX_ITR,
                  semantics=sem)
        dev.split_round(x.mat, x.S[ci], None, x.part, None, x.ST[j], span=dev.SPAN_LOCAL, **kw)
        dev.split_round(x.mat, x.S[ci], x.s_next, x.part, x.V[j], x.ST[j],
                        span=dev.SPAN_REMOTE, **kw)
    sweep(orc, dt, sem, n, launch, jobs_of=split_jobs, setup=setup)


@pytest.mark.parametrize("dt,sem,n", PARAMS)
def test_flat_round(orc, dt, sem, n):
    """k_flat's first row group (one stats_publish per piece) + k_parts."""
    def setup(x):
        x.part = dev.flat_scratch(NROWS, n, TD[dt], DEV)

    def launch(x, j, ci, _):
        dev.flat_round(x.mat, x.S[ci], x.s_next, x.part, x.V[j], x.ST[j], row0=ROW0,
                       eps=x.eps[ci], k=K, max_itr=MAX_ITR, semantics=sem)
    sweep(orc, dt, sem, n, launch, flat=True, setup=setup)


@pytest.mark.parametrize("dt,sem,n", PARAMS)
def test_split_flat_round(orc, dt, sem, n):
    """k_flat SPLIT = 1 then SPLIT = 2 (stats over every piece, masked
    columns) + k_parts with the local partials."""
    def setup(x):
        x.part = dev.split_flat_scratch(NROWS, n, 0, n, TD[dt], DEV)   # the largest range

    def launch(x, j, ci, r):
        kw = dict(row0=ROW0, col0=r[0], col1=r[1], eps=x.eps[ci], k=K, max_itr=MAX_ITR,
                  semantics=sem)
        dev.split_flat_round(x.mat, x.S[ci], None, x.part, None, x.ST[j],
                             span=dev.SPAN_LOCAL, **kw)
        dev.split_flat_round(x.mat, x.S[ci], x.s_next, x.part, x.V[j], x.ST[j],
                             span=dev.SPAN_REMOTE, **kw)
    sweep(orc, dt, sem, n, launch, flat=True, jobs_of=split_jobs, setup=setup)


@pytest.mark.parametrize("npend", [0, 2])
@pytest.mark.parametrize("dt,sem,n", PARAMS)
def test_flat_round_deferred(orc, dt, sem, n, npend):
    """k_flat<NP> read-only rounds: nothing pending, and two pending rounds of
    unit scales (x * (1 * 1) = x: the stats see the same s)."""
    def setup(x):
        x.part = dev.flat_scratch(NROWS, n, TD[dt], DEV)
        x.INV = torch.empty_like(x.S)
        dev.recip(x.S.view(-1), x.INV.view(-1))
        x.inv_next = torch.empty(n, dtype=TD[dt], device=DEV)
        x.ones = [torch.ones(n, dtype=TD[dt], device=DEV) for _ in range(2 * npend)]

    def launch(x, j, ci, _):
        dev.flat_round_deferred(x.mat, x.S[ci], x.INV[ci], x.s_next, x.inv_next, x.part,
                                x.V[j], x.ST[j], x.ones[:npend], x.ones[npend:], store=False,
                                row0=ROW0, eps=x.eps[ci], k=K, max_itr=MAX_ITR, semantics=sem)
    sweep(orc, dt, sem, n, launch, flat=True, setup=setup)


@pytest.mark.parametrize("flat", [False, True], ids=["k_mfree", "flat"])
@pytest.mark.parametrize("dt,sem,n", PARAMS)
def test_mfree_round(orc, dt, sem, n, flat):
    """Launch k = 1 of the matrix-free forms evaluates round 0 on s_prev:
    end = k on a stop, v_cur = v_prev * (s_prev / m) over the FULL vector."""
    def setup(x):
        x.part = dev.flat_scratch(NROWS, n, TD[dt], DEV)

    def launch(x, j, ci, _):
        args = (x.mat, x.S[ci], x.s_next, x.v0, x.V[j])
        kw = dict(row0=ROW0, eps=x.eps[ci], k=1, max_itr=MAX_ITR, semantics=sem)
        if flat:
            dev.mfree_round_flat(*args, x.part, x.ST[j], **kw)
        else:
            dev.mfree_round(*args, x.ST[j], **kw)
    sweep(orc, dt, sem, n, launch, full_v=True, flat=flat, rk=0, setup=setup)


@pytest.mark.parametrize("dt,sem,n", PARAMS)
def test_epilogue(orc, dt, sem, n):
    """k_epilogue: one workgroup of kEpiBlock lanes over the full vector."""
    def launch(x, j, ci, _):
        dev.epilogue(x.S[ci], x.V[j], x.ST[j], eps=x.eps[ci], max_itr=MAX_ITR, semantics=sem)
    sweep(orc, dt, sem, n, launch, full_v=True, epilogue=True)


# ---------------------------------------------------------------------------
# 8 - 11: the kernels that derive s_k themselves.  A = diag(d), max_itr = 1: a
# row's sum is exactly d[r] in any summation order (the rest are zeros), so
# round 0's stop test runs on s_0 = d, v_0 = 1 * (d / m) = d / m
# ---------------------------------------------------------------------------
def expect_solve(c, ci):
    stop = c.stop[ci]
    iters = np.where(stop == 1, 0 if c.cyclic else 1, 1)     # cpp:54 / py:47; else max_itr
    with np.errstate(invalid="ignore"):
        v = c.S[ci] / c.m[ci][:, None]
    return stop, iters, v


def solve_each(solver, orc, dt, sem, n, only=None, mat=None, **kw):
    c = cases(orc, n, dt, sem == _lib.ST_SEM_SYCL, only)
    D = torch.tensor(c.S, device=DEV)
    a = torch.zeros((n, n), dtype=TD[dt], device=DEV) if mat is None else mat
    lam, its, conv, vs = [], [], [], []
    for ci in range(len(c.tags)):
        if kw.get("inplace"):      # the last solve transformed it (a NaN spreads over 0 * NaN)
            a.zero_()
        a.diagonal().copy_(D[ci])
        l, v, it, st = solver.solve(a, eps=float(c.eps[ci]), max_itr=1, semantics=sem, **kw)
        lam.append(l), its.append(it), conv.append(st["converged"]), vs.append(v)
    jobs = [(ci, None) for ci in range(len(c.tags))]
    ci = np.arange(len(jobs))
    stop, iters, v = expect_solve(c, ci)
    check("converged", np.array(conv), stop, jobs, c)
    check("iterations", np.array(its), iters, jobs, c)
    check("lambda", np.array(lam, dtype=np.float64), c.S[:, 0].astype(np.float64), jobs, c)
    torch.cuda.synchronize()
    check("v", torch.stack(vs).cpu().numpy(), v, jobs, c)


SMALL = [(np.float64, 9), (np.float64, 64), (np.float64, 127), (np.float64, 128),
         (np.float32, 9), (np.float32, 255), (np.float32, 256)]


@pytest.mark.parametrize("mode", [{}, {"round_loop": True}, {"matrix_free": True}],
                         ids=["default", "round_loop", "matrix_free"])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt,n", SMALL)
def test_solve_small(solver, orc, dt, n, sem, mode):
    """k_solve_small's per-thread pair (n a multiple of the vector width, up
    to 128 fp64 / 256 fp32), and the same sizes through the round loop and
    the matrix-free loop."""
    solve_each(solver, orc, dt, sem, n, **mode)


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1032, 2056])
def test_solve_round_loop_sizes(solver, orc, dt, n, sem):
    """The k_round loop as the solve launches it (its own row groups and grid)."""
    solve_each(solver, orc, dt, sem, n)


def batched(solver, orc, dt, sem, n, **kw):
    """One diagonal matrix per case, stacked: entry b must stop, or not, on
    its own (one batch per eps: the batch shares it)."""
    c = cases(orc, n, dt, sem == _lib.ST_SEM_SYCL)
    for e in np.unique(c.eps):
        idx = np.nonzero(c.eps == e)[0]
        mats = torch.zeros((len(idx), n, n), dtype=TD[dt], device=DEV)
        mats.diagonal(dim1=1, dim2=2).copy_(torch.from_numpy(c.S[idx]).to(DEV))
        lam, v, it, st = solver.solve_batched(mats, inplace=True, eps=float(e), max_itr=1,
                                              semantics=sem, **kw)
        jobs = [(int(ci), None) for ci in idx]
        stop, iters, vexp = expect_solve(c, idx)
        assert 0 < stop.sum() < len(idx)               # both kinds in one batch
        check("converged_each", st["converged_each"], stop, jobs, c)
        check("iterations", it.numpy(), iters, jobs, c)
        check("lambda", lam.numpy().astype(np.float64), c.S[idx, 0].astype(np.float64), jobs, c)
        check("v", v.cpu().numpy(), vexp, jobs, c)
        assert st["converged"] == 0 and st["rounds"] == 1


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt,n", [(np.float64, 9), (np.float64, 63), (np.float64, 128),
                                  (np.float32, 9), (np.float32, 256)])
def test_solve_batched(solver, orc, dt, n, sem):
    """k_solve_batched, one launch: each workgroup's stop is its own."""
    batched(solver, orc, dt, sem, n)


@pytest.mark.parametrize("batch", [1, 0], ids=["batch1", "default"])
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [9, 128, 1032])
def test_solve_batched_round_loop(solver, orc, dt, n, sem, batch):
    """k_round_batched: one launch per round for the whole batch."""
    batched(solver, orc, dt, sem, n, round_loop=True, batch=batch)


@pytest.mark.parametrize("sem", SEMS)
def test_solve_flat_deferred_size(solver, orc, sem):
    """4352^2 fp64 (145 MiB), where the solve's own policy runs the flat loop
    with deferred writes: k_flat_sum + k_parts, the NP = 0 read-only round and
    the flush.  Six positions: 0, the piece boundary 1023 / 1024, n - 2, n - 1
    and one seeded."""
    n, dt = 4352, np.float64
    assert dev.flat_round_pays(n, n, TD[dt])
    rnd = sorted(set(sv.positions(n, dt, True)) - set(sv.positions(n, dt, True, nrandom=0)))[0]
    a = torch.zeros((n, n), dtype=TD[dt], device=DEV)
    solve_each(solver, orc, dt, sem, n, only=(0, 1023, 1024, n - 2, n - 1, rnd), mat=a,
               inplace=True)
