"""GPU: the batched round loop (ST_FLAG_BATCH_ROUNDS, k_round_batched: one
launch per round for the whole batch) against the single solve.

Everything is bitwise (``torch.equal`` / ``==``): every matrix of a batch
runs the kernel instantiation of its single solve on the same lane layout,
so there is no tolerance at any n, ragged sizes included.
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


_BATCHES = {}


def batch_of(orc, n, dt, seeds=range(4)):
    """Random seeds plus Hilbert, built once per (n, dtype) and never written."""
    key = (n, np.dtype(dt).name, tuple(seeds))
    if key not in _BATCHES:
        mats = np.stack([orc.random_matrix(n, s, dt) for s in seeds] + [orc.hilbert(n, dt)])
        mats.setflags(write=False)
        _BATCHES[key] = mats
    return _BATCHES[key]


def assert_equals_singles(solver, mats, entries=None, **kw):
    """solve_batched(mats, round_loop=True) against solve() on each (listed)
    matrix alone: everything bitwise.  Returns the batched result."""
    a = mats.clone() if isinstance(mats, torch.Tensor) else torch.from_numpy(mats.copy()).to(DEV)
    src = mats if isinstance(mats, torch.Tensor) else None
    skw = {k: v for k, v in kw.items() if k != "batch"}
    lam, v, it, st = solver.solve_batched(a, inplace=True, round_loop=True, **kw)
    nb, n = a.shape[0], a.shape[1]
    assert lam.shape == (nb,) and v.shape == (nb, n) and it.shape == lam.shape
    for b in (range(nb) if entries is None else entries):
        one = src[b].clone() if src is not None else torch.from_numpy(mats[b].copy()).to(DEV)
        l1, v1, it1, st1 = solver.solve(one, inplace=True, **skw)
        assert lam[b].item() == l1, (b, lam[b].item(), l1)
        assert int(it[b]) == it1, (b, int(it[b]), it1)
        assert int(st["converged_each"][b]) == st1["converged"], b
        assert torch.equal(v[b], v1), b
        assert torch.equal(a[b], one), b
    return lam, v, it, st


# ---------------------------------------------------------------------------
# 1. bitwise against the single solve on every entry
# ---------------------------------------------------------------------------
# fp64 130: vector path, 1 row per group; fp64 129 / fp32 258: element-wide;
# fp64 1024: first size with 2 rows per group; fp64 1025: element-wide plus a
# remainder row group
@pytest.mark.parametrize("dt,n", [(np.float64, 130), (np.float64, 129), (np.float32, 258),
                                  (np.float64, 192), (np.float32, 260), (np.float64, 1024),
                                  (np.float64, 1025)])
@pytest.mark.parametrize("sem", SEMS)
def test_rounds_bitwise_vs_single(solver, orc, dt, n, sem):
    mats = batch_of(orc, n, dt, seeds=range(2) if n >= 1024 else range(4))
    assert len(mats) == (3 if n >= 1024 else 5)
    lam, v, it, st = assert_equals_singles(solver, mats, semantics=sem)
    counts = [int(x) for x in it]
    print(f"{np.dtype(dt).name} n={n} sem={sem}: iterations {counts}, rounds {st['rounds']}, "
          f"round launches {st['fused_launches']}")
    # entries stop in different rounds, and Hilbert runs past the first
    # 8-round host check.  (CPU oracle, Hilbert: 9 9 10 11 11 13 13 in the
    # SYCL semantics at n = 129 130 192 258 260 1024 1025; main.py's count
    # at n = 129 is exactly 8, the one case that ends on the check itself.)
    assert len(set(counts)) > 1
    assert max(counts) > 8 or (sem == _lib.ST_SEM_MAINPY and n == 129 and max(counts) == 8)
    assert st["converged"] == 1 and st["rounds"] >= max(counts)


# ---------------------------------------------------------------------------
# 2. the other launch classes
# ---------------------------------------------------------------------------
# fp64 2052: above 32 MiB; fp64 4096: 128 MiB, 4 rows per group; fp32 6143:
# the limit
@pytest.mark.parametrize("dt,n", [(np.float64, 2052), (np.float64, 4096), (np.float32, 6143)])
def test_rounds_large_classes_bitwise_vs_single(solver, dt, n):
    a = torch.empty((2, n, n), dtype=TD[dt], device=DEV)
    for b in range(2):
        dev.generate("random", n, TD[dt], seed=b, device=DEV, out=a[b])
    if dt == np.float32:
        assert n == dev.batched_rounds_max_dim(dt)
    lam, v, it, st = assert_equals_singles(solver, a)
    print(f"{np.dtype(dt).name} n={n}: iterations {[int(x) for x in it]}")
    assert st["converged"] == 1


def test_rounds_non_temporal_batch_bitwise_vs_single(solver):
    # 64 x 2048^2 fp64 is 2 GiB in total: the launch turns non-temporal there
    # (the cache policy must not change a bit)
    nb, n = 64, 2048
    tall = dev.generate("random", n, torch.float64, nrows=nb * n, seed=9, device=DEV)
    lam, v, it, st = assert_equals_singles(solver, tall.view(nb, n, n), entries=(0, 31, 63))
    assert st["converged"] == 1 and st["rounds"] >= int(it.max()) >= 1


# ---------------------------------------------------------------------------
# 3. against the one-launch kernel
# ---------------------------------------------------------------------------
def assert_same_result(got, want):
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(got[2], want[2])
    assert np.array_equal(got[3]["converged_each"], want[3]["converged_each"])
    assert got[3]["converged"] == want[3]["converged"] and got[3]["rounds"] == want[3]["rounds"]


def test_rounds_equal_one_launch_kernel(solver, orc):
    mats = np.stack([orc.random_matrix(64, s, np.float64) for s in range(8)]
                    + [orc.hilbert(64, np.float64)])
    a, b = torch.from_numpy(mats).to(DEV), torch.from_numpy(mats).to(DEV)
    got = solver.solve_batched(a, inplace=True, round_loop=True)
    want = solver.solve_batched(b, inplace=True)
    assert_same_result(got, want)
    assert torch.equal(a, b)


def test_rounds_batch_past_the_grid_y_limit(solver):
    nb = 65540
    tall = dev.generate("random", 4, torch.float64, nrows=nb * 4, seed=5, device=DEV)
    a = tall.reshape(nb, 4, 4).clone()
    b = tall.reshape(nb, 4, 4).clone()
    got = solver.solve_batched(a, inplace=True, round_loop=True)
    want = solver.solve_batched(b, inplace=True)
    assert_same_result(got, want)
    assert torch.equal(a, b)
    assert len(set(int(x) for x in got[2])) > 1


# ---------------------------------------------------------------------------
# 4. options
# ---------------------------------------------------------------------------
def test_rounds_options(solver, orc):
    mats = batch_of(orc, 130, np.float64)
    for kw in (dict(eps=1e-6), dict(max_itr=1), dict(eps=0.0, max_itr=7)):
        lam, v, it, st = assert_equals_singles(solver, mats, **kw)
        if "max_itr" in kw:
            assert st["rounds"] == kw["max_itr"]
    # eps = 0 never converges: exhausted everywhere
    assert list(st["converged_each"]) == [0] * len(mats)
    assert st["converged"] == 0 and st["rounds"] == 7
    assert [int(x) for x in it] == [7] * len(mats)


def test_rounds_host_check_interval_does_not_change_bits(solver, orc):
    mats = batch_of(orc, 130, np.float64)
    base = torch.from_numpy(mats.copy()).to(DEV)
    want = solver.solve_batched(base, inplace=True, round_loop=True)
    for batch in (1, 3):
        a = torch.from_numpy(mats.copy()).to(DEV)
        got = solver.solve_batched(a, inplace=True, round_loop=True, batch=batch)
        assert_same_result(got, want)
        assert torch.equal(a, base)
        assert got[3]["fused_launches"] % batch == 0


# ---------------------------------------------------------------------------
# 5. the loop stops early
# ---------------------------------------------------------------------------
def test_rounds_loop_stops_enqueuing(solver, orc):
    mats = batch_of(orc, 130, np.float64)
    lam, v, it, st = solver.solve_batched(torch.from_numpy(mats.copy()).to(DEV), round_loop=True)
    print(f"rounds {st['rounds']}, round launches {st['fused_launches']}")
    assert st["fused_launches"] >= st["rounds"]
    # two 8-round batches in flight plus rounding up
    assert st["fused_launches"] <= st["rounds"] + 24


# ---------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------
def test_rounds_not_inplace_leaves_the_input(solver, orc):
    mats = batch_of(orc, 130, np.float64)
    a = torch.from_numpy(mats.copy()).to(DEV)
    keep = a.clone()
    solver.solve_batched(a, round_loop=True)
    assert torch.equal(a, keep)


def test_rounds_on_a_side_stream(solver, orc):
    mats = batch_of(orc, 130, np.float64)
    base = torch.from_numpy(mats.copy()).to(DEV)
    want = solver.solve_batched(base, inplace=True, round_loop=True)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        a = torch.from_numpy(mats.copy()).to(DEV)
        got = solver.solve_batched(a, inplace=True, round_loop=True)
    side.synchronize()
    assert_same_result(got, want)
    assert torch.equal(a, base)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_rounds_empty_batch_is_a_noop(solver, dt):
    a = torch.empty((0, 300, 300), dtype=TD[dt], device=DEV)
    lam, v, it, st = solver.solve_batched(a, round_loop=True)
    assert lam.shape == (0,) and v.shape == (0, 300) and it.shape == (0,)
    assert st["rounds"] == 0 and st["fused_launches"] == 0 and len(st["converged_each"]) == 0


def test_auto_picks_the_kernel_by_size(solver, orc):
    small = np.stack([orc.random_matrix(64, s, np.float64) for s in range(3)])
    got = solver.solve_batched(torch.from_numpy(small).to(DEV), round_loop="auto")
    want = solver.solve_batched(torch.from_numpy(small).to(DEV))
    assert_same_result(got, want)
    assert got[3]["fused_launches"] == 0        # the one-launch kernel ran
    mats = batch_of(orc, 130, np.float64)
    got = solver.solve_batched(torch.from_numpy(mats.copy()).to(DEV), round_loop="auto")
    want = solver.solve_batched(torch.from_numpy(mats.copy()).to(DEV), round_loop=True)
    assert_same_result(got, want)
    assert got[3]["fused_launches"] == want[3]["fused_launches"] > 0


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_rounds_reject_dim_above_the_limit(solver, dt):
    lim = dev.batched_rounds_max_dim(dt)
    assert lim == (4344 if dt == np.float64 else 6143)
    big = torch.ones((2, lim + 1, lim + 1), dtype=TD[dt], device=DEV)
    with pytest.raises(_lib.EigenValueError, match="exceeds the round-loop limit"):
        solver.solve_batched(big, inplace=True, round_loop=True)
    torch.cuda.synchronize()
    assert bool((big == 1).all())               # nothing ran


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_rounds_reject_unsupported_flags(solver, orc, dt):
    n = 8
    a = torch.from_numpy(np.stack([orc.random_matrix(n, s, dt) for s in range(3)])).to(DEV)
    keep = a.clone()
    v = torch.empty((len(a), n), dtype=a.dtype, device=DEV)
    lam, it = np.zeros(len(a), dt), np.zeros(len(a), np.uint32)
    fn = getattr(solver.L, "st_solve_batched_" + ("f64" if dt == np.float64 else "f32"))
    for flag in (_lib.ST_FLAG_MATRIX_FREE, _lib.ST_FLAG_TIME_KERNELS, _lib.ST_FLAG_TRACE_SUMS,
                 _lib.ST_FLAG_ROUND_LOOP):
        opt = _lib.st_options(-1.0, 0, _lib.ST_SEM_SYCL, 0, flag | _lib.ST_FLAG_BATCH_ROUNDS)
        with pytest.raises(_lib.EigenValueError, match="not supported"):
            _lib.check(fn(solver.q, a.data_ptr(), len(a), n, v.data_ptr(), None, lam.ctypes.data,
                          it.ctypes.data, None, ctypes.byref(opt), None), "st_solve_batched")
    torch.cuda.synchronize()
    assert torch.equal(a, keep)                 # nothing ran


# ---------------------------------------------------------------------------
# 7. host-pointer path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,n", [(np.float64, 130), (np.float32, 258)])
def test_host_rounds_equal_per_matrix_calls(eigen, orc, dt, n):
    mats = batch_of(orc, n, dt).copy()
    keep = mats.copy()
    lam, v, ts, it = eigen.similarity_transform_batched(mats, round_loop="auto")
    assert lam.dtype == dt and v.dtype == dt and it.dtype == np.uint32
    assert lam.shape == (5,) and v.shape == (5, n) and it.shape == (5,) and ts >= 0
    assert np.array_equal(mats, keep)           # mats is read only
    for b in range(len(mats)):
        l1, v1, _, it1 = eigen.similarity_transform(mats[b])
        assert lam[b] == l1 and int(it[b]) == it1 and np.array_equal(v[b], v1), b


# ---------------------------------------------------------------------------
# 8. speed sanity: one launch per round against 32 solves
# ---------------------------------------------------------------------------
def test_rounds_are_faster_than_sequential_solves(solver):
    nb, n = 32, 512
    base = torch.empty((nb, n, n), dtype=torch.float64, device=DEV)
    for b in range(nb):
        dev.generate("hilbert" if b % 2 else "random", n, torch.float64, seed=b, device=DEV,
                     out=base[b])
    best_b = best_s = float("inf")
    for _ in range(5):
        a = base.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.solve_batched(a, inplace=True, round_loop=True)
        best_b = min(best_b, time.perf_counter() - t0)
        a = base.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(nb):
            solver.solve(a[b], inplace=True)
        best_s = min(best_s, time.perf_counter() - t0)
    print(f"32 x 512^2 f64: solve_batched(round_loop=True) {best_b * 1e3:.3f} ms, "
          f"32 sequential solves {best_s * 1e3:.3f} ms")
    assert best_b < best_s
