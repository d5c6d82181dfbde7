"""GPU: the batched solve (k_solve_batched, a workgroup per matrix) against
the existing single solve and the CPU oracle.

Tolerances:
  * n % (16 / element size) == 0: every batch entry BIT-identical to
    ``DeviceSolver.solve(..., inplace=True)`` on that matrix alone (λ, v,
    iteration count, converged flag, final matrix);
  * other n (the single solve sums those rows element-wide, in another
    order): against the oracle, iteration counts equal, λ relative and v
    (max-abs over the vector's largest element) <= 1e-10 fp64 / 1e-5 fp32.
    The oracle's stop decision is at least 64 ulps of the row sum from eps in
    every round of every such case (asserted), so the counts cannot differ
    by rounding.
"""
import ctypes
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import eigen_value_amd as ev  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402

DEV = "cuda:0"
SEMS = [_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY]
TOL = {np.float64: 1e-10, np.float32: 1e-5}
TD = {np.float64: torch.float64, np.float32: torch.float32}


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


@pytest.fixture(scope="module")
def eigen():
    e = ev.EigenValue()
    yield e
    e.close()


def batch_of(orc, n, dt, seeds=range(8), hilbert=True):
    mats = [orc.random_matrix(n, s, dt) for s in seeds]
    if hilbert:
        mats.append(orc.hilbert(n, dt))
    return np.stack(mats)


def assert_equals_singles(solver, mats, entries=None, **kw):
    """solve_batched(mats) against solve() on each (listed) matrix alone:
    everything bitwise.  Returns the batched result."""
    a = torch.from_numpy(mats).to(DEV)
    lam, v, it, st = solver.solve_batched(a, inplace=True, **kw)
    assert lam.shape == (len(mats),) and v.shape == mats.shape[:2] and it.shape == lam.shape
    for b in (range(len(mats)) if entries is None else entries):
        one = torch.from_numpy(mats[b]).to(DEV)
        l1, v1, it1, st1 = solver.solve(one, inplace=True, **kw)
        assert lam[b].item() == l1, (b, lam[b].item(), l1)
        assert int(it[b]) == it1, (b, int(it[b]), it1)
        assert int(st["converged_each"][b]) == st1["converged"], b
        assert torch.equal(v[b], v1), b
        assert torch.equal(a[b], one), b
    return lam, v, it, st


# ---------------------------------------------------------------------------
# vector sizes: bit-identical to the single solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,n", [(np.float64, 2), (np.float64, 6), (np.float64, 64),
                                  (np.float64, 128), (np.float32, 4), (np.float32, 8),
                                  (np.float32, 100), (np.float32, 252), (np.float32, 256)])
@pytest.mark.parametrize("sem", SEMS)
def test_batched_bitwise_vs_single(solver, orc, dt, n, sem):
    mats = batch_of(orc, n, dt)
    lam, v, it, st = assert_equals_singles(solver, mats, semantics=sem)
    counts = [int(x) for x in it]
    print(f"{np.dtype(dt).name} n={n} sem={sem}: iterations {counts}")
    assert st["rounds"] >= max(counts) and st["converged"] == 1
    if (dt, n) in ((np.float64, 2), (np.float32, 4)):
        # entries stop in different rounds (what a shared or misindexed state
        # would break); reference semantics: 21 4 1 17 3 6 4 11 / 6 4 4 5 3 5 6 6
        assert len(set(counts[:8])) > 1
        if sem == _lib.ST_SEM_SYCL:
            assert counts[:8] == ([21, 4, 1, 17, 3, 6, 4, 11] if n == 2
                                  else [6, 4, 4, 5, 3, 5, 6, 6])


# ---------------------------------------------------------------------------
# ragged sizes: against the oracle
# ---------------------------------------------------------------------------
def oracle_batch(orc, mats, sem, check_margin, **kw):
    """The oracle's solve of every matrix; with
    ``check_margin`` its stop decisions are >= 64 ulps of the row sum from
    eps in every round, so a few ulps of summation order cannot move them."""
    osem = orc.SEM_SYCL if sem == _lib.ST_SEM_SYCL else orc.SEM_MAINPY
    out = []
    for b, m in enumerate(mats):
        r = orc.similarity_transform(m, osem, trace=True, **kw)
        if check_margin:
            eps = float(m.dtype.type(orc.EPS_F32 if m.dtype == np.float32 else orc.EPS_F64))
            for k in range(r.rounds_evaluated):
                ulp = float(np.spacing(np.abs(r.row_sums[k]).max().astype(m.dtype)))
                margin = abs(float(r.max_dsum[k]) - eps) / ulp
                assert margin >= 64, ("marginal stop decision in the fixture", b, k, margin)
        out.append(r)
    return out


def assert_matches_oracle(mats, refs, lam, v, it, tol):
    worst_l = worst_v = 0.0
    for b, r in enumerate(refs):
        worst_l = max(worst_l, abs(lam[b].item() - float(r.eigen_val)) / abs(float(r.eigen_val)))
        worst_v = max(worst_v, float(np.max(np.abs(v[b] - r.eigen_vec)) / np.max(np.abs(r.eigen_vec))))
    counts, want = [int(x) for x in it], [r.iter_count for r in refs]
    print(f"{mats.dtype.name} n={mats.shape[1]}: iterations {counts} (oracle {want}), "
          f"worst rel dλ {worst_l:.3e}, worst dv {worst_v:.3e} (tolerance {tol:g})")
    assert counts == want
    assert worst_l <= tol and worst_v <= tol


@pytest.mark.parametrize("dt,n", [(np.float64, 1), (np.float64, 33), (np.float64, 127),
                                  (np.float32, 1), (np.float32, 3), (np.float32, 50)])
@pytest.mark.parametrize("sem", SEMS)
def test_batched_ragged_vs_oracle(solver, orc, dt, n, sem):
    # fp32 n = 3: seed 0 stops 26.6 ulps from eps, so seeds 1 .. 7
    mats = batch_of(orc, n, dt, seeds=range(1, 8) if n == 3 else range(8))
    refs = oracle_batch(orc, mats, sem, check_margin=True)
    a = torch.from_numpy(mats).to(DEV)
    lam, v, it, st = solver.solve_batched(a, semantics=sem)
    assert torch.equal(a, torch.from_numpy(mats).to(DEV))       # not inplace: untouched
    assert_matches_oracle(mats, refs, lam, v.cpu().numpy(), it, TOL[dt])
    assert st["converged"] == 1 and list(st["converged_each"]) == [1] * len(mats)
    assert st["rounds"] == max(r.rounds_evaluated for r in refs)


@pytest.mark.parametrize("dt,n", [(np.float32, 255), (np.float64, 127)])
def test_batched_ragged_large_fixed_rounds(solver, orc, dt, n):
    # 16 rows per wave with a tail lane; a fixed round count, because the
    # stop margin at this size is only 3 - 36 ulps
    mats = batch_of(orc, n, dt)
    refs = oracle_batch(orc, mats, _lib.ST_SEM_SYCL, check_margin=False, eps=0.0, max_itr=5)
    lam, v, it, st = solver.solve_batched(torch.from_numpy(mats).to(DEV), eps=0.0, max_itr=5)
    assert [int(x) for x in it] == [5] * len(mats)
    assert list(st["converged_each"]) == [0] * len(mats)
    assert st["converged"] == 0 and st["rounds"] == 5
    assert_matches_oracle(mats, refs, lam, v.cpu().numpy(), it, TOL[dt])


# ---------------------------------------------------------------------------
# options and edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,n", [(np.float64, 6), (np.float32, 8)])
def test_batched_options(solver, orc, dt, n):
    mats = batch_of(orc, n, dt)
    for kw in (dict(eps=1e-6), dict(max_itr=1), dict(eps=0.0, max_itr=7)):
        lam, v, it, st = assert_equals_singles(solver, mats, **kw)
        if "max_itr" in kw:
            assert st["rounds"] == kw["max_itr"]
    lam, v, it, st = solver.solve_batched(torch.from_numpy(mats).to(DEV), max_itr=1)
    assert st["rounds"] == 1 and int(it.max()) <= 1
    # a tighter eps takes at least as many rounds
    loose = solver.solve_batched(torch.from_numpy(mats).to(DEV))[2]
    tight = solver.solve_batched(torch.from_numpy(mats).to(DEV), eps=1e-6)[2]
    assert bool((tight >= loose).all()) and int(tight.sum()) > int(loose.sum())


@pytest.mark.parametrize("dt,n", [(np.float64, 128), (np.float32, 256), (np.float64, 16)])
def test_batch_of_one_equals_single(solver, orc, dt, n):
    assert_equals_singles(solver, orc.random_matrix(n, 3, dt)[None])


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_empty_batch_is_a_noop(solver, dt):
    a = torch.empty((0, 4, 4), dtype=TD[dt], device=DEV)
    lam, v, it, st = solver.solve_batched(a)
    assert lam.shape == (0,) and v.shape == (0, 4) and it.shape == (0,)
    assert st["rounds"] == 0 and len(st["converged_each"]) == 0


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_batched_rejects_large_dim_and_flags(solver, orc, dt):
    lim = dev.batched_max_dim(dt)
    assert lim == (128 if dt == np.float64 else 256)
    big = torch.ones((2, lim + 1, lim + 1), dtype=TD[dt], device=DEV)
    with pytest.raises(_lib.EigenValueError, match="exceeds the one-workgroup limit"):
        solver.solve_batched(big)
    # every flag the batched solve does not support is an error, not a
    # fallback
    n = 8
    a = torch.from_numpy(batch_of(orc, n, dt)).to(DEV)
    keep = a.clone()
    v = torch.empty((len(a), n), dtype=a.dtype, device=DEV)
    lam, it = np.zeros(len(a), dt), np.zeros(len(a), np.uint32)
    fn = getattr(solver.L, "st_solve_batched_" + ("f64" if dt == np.float64 else "f32"))
    for flag in (_lib.ST_FLAG_MATRIX_FREE, _lib.ST_FLAG_TIME_KERNELS, _lib.ST_FLAG_TRACE_SUMS,
                 _lib.ST_FLAG_ROUND_LOOP):
        opt = _lib.st_options(-1.0, 0, _lib.ST_SEM_SYCL, 0, flag)
        with pytest.raises(_lib.EigenValueError, match="not supported"):
            _lib.check(fn(solver.q, a.data_ptr(), len(a), n, v.data_ptr(), None, lam.ctypes.data,
                          it.ctypes.data, None, ctypes.byref(opt), None), "st_solve_batched")
    opt = _lib.st_options(-1.0, 0, _lib.ST_SEM_SYCL, 0, 0)
    with pytest.raises(_lib.EigenValueError, match="dim must be > 0"):
        _lib.check(fn(solver.q, a.data_ptr(), len(a), 0, v.data_ptr(), None, lam.ctypes.data,
                      it.ctypes.data, None, ctypes.byref(opt), None), "st_solve_batched")
    with pytest.raises(_lib.EigenValueError, match="null"):
        _lib.check(fn(solver.q, a.data_ptr(), len(a), n, v.data_ptr(), None, None,
                      it.ctypes.data, None, ctypes.byref(opt), None), "st_solve_batched")
    torch.cuda.synchronize()
    assert torch.equal(a, keep)                 # nothing ran


def test_batched_on_a_side_stream(solver, orc):
    mats = batch_of(orc, 64, np.float64)
    want = solver.solve_batched(torch.from_numpy(mats).to(DEV))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        a = torch.from_numpy(mats).to(DEV)
        got = solver.solve_batched(a, inplace=True)
    side.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert torch.equal(got[1], want[1])
    assert not torch.equal(a, torch.from_numpy(mats).to(DEV))   # transformed in place


# ---------------------------------------------------------------------------
# host-pointer path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,n", [(np.float32, 8), (np.float64, 6)])
def test_host_batched_equals_per_matrix_calls(eigen, orc, dt, n):
    mats = batch_of(orc, n, dt)
    keep = mats.copy()
    lam, v, ts, it = eigen.similarity_transform_batched(mats)
    assert lam.dtype == dt and v.dtype == dt and it.dtype == np.uint32
    assert lam.shape == (9,) and v.shape == (9, n) and it.shape == (9,) and ts >= 0
    assert np.array_equal(mats, keep)           # mats is read only
    for b in range(len(mats)):
        l1, v1, _, it1 = eigen.similarity_transform(mats[b])
        assert lam[b] == l1 and int(it[b]) == it1 and np.array_equal(v[b], v1), b
    lam0, v0, _, it0 = eigen.similarity_transform_batched(np.zeros((0, n, n), dt))
    assert lam0.shape == (0,) and v0.shape == (0, n) and it0.shape == (0,)


# ---------------------------------------------------------------------------
# more workgroups than the machine holds at once
# ---------------------------------------------------------------------------
def test_batched_2048_matrices(solver, orc):
    mats = np.stack([orc.random_matrix(16, s, np.float64) for s in range(2048)])
    lam, v, it, st = assert_equals_singles(solver, mats, entries=(0, 1, 1023, 2047))
    assert st["converged"] == 1 and bool((st["converged_each"] == 1).all())
    assert st["rounds"] >= int(it.max()) >= 1


# ---------------------------------------------------------------------------
# speed sanity: one launch against 64 round trips
# ---------------------------------------------------------------------------
def test_batched_is_faster_than_sequential_solves(solver, orc):
    n, dt = 128, np.float64
    mats = np.stack([orc.hilbert(n, dt) if s % 2 else orc.random_matrix(n, s, dt)
                     for s in range(64)])
    base = torch.from_numpy(mats).to(DEV)
    best_b = best_s = float("inf")
    for _ in range(5):
        a = base.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.solve_batched(a, inplace=True)
        best_b = min(best_b, time.perf_counter() - t0)
        a = base.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(64):
            solver.solve(a[b], inplace=True)
        best_s = min(best_s, time.perf_counter() - t0)
    print(f"64 x 128^2 f64: solve_batched {best_b * 1e3:.3f} ms, "
          f"64 sequential solves {best_s * 1e3:.3f} ms")
    assert best_b < best_s
