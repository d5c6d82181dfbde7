"""GPU: the variable-size batched solve (k_solve_vbatched: one launch per
workgroup-shape class, a workgroup per matrix) against the project's own
``solve_batched`` on each matrix alone as a (1, n, n) batch.

No tolerance anywhere: λ, v, iteration count, converged flag and final matrix
are compared with ``==`` / ``torch.equal``.  The single-entry references are
computed once per (matrix, options) and shared by the tests.
"""
import ctypes

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
SFX = {np.float64: "f64", np.float32: "f32"}
DIMS = {np.float64: [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128]}
DIMS[np.float32] = DIMS[np.float64] + [129, 252, 255, 256]
SENTINEL = -777.25
# stop rounds of random_matrix(2, seed 0..7, float64) under ST_SEM_SYCL
# (pinned in test_gpu_batched.py::test_batched_bitwise_vs_single)
N2_COUNTS = [21, 4, 1, 17, 3, 6, 4, 11]


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


_SINGLES = {}


def single(solver, m, **kw):
    """solve_batched on ``m`` alone as a (1, n, n) batch, in place on a copy:
    (λ, v, count, converged, rounds, final matrix).  Cached, never modified."""
    key = (m.dtype.str, m.shape[0], m.tobytes(), tuple(sorted(kw.items())))
    if key not in _SINGLES:
        a = torch.from_numpy(m[None].copy()).to(DEV)
        lam, v, it, st = solver.solve_batched(a, inplace=True, **kw)
        _SINGLES[key] = (lam[0].item(), v[0].clone(), int(it[0]), int(st["converged_each"][0]),
                         int(st["rounds"]), a[0].clone())
    return _SINGLES[key]


def assert_entries_equal_singles(solver, mats, work, lam, vs, it, st, entries=None, **kw):
    """Every (listed) entry of a vbatched result against its single: all bitwise."""
    rounds = 0
    for b in (range(len(mats)) if entries is None else entries):
        l1, v1, it1, c1, r1, fin1 = single(solver, mats[b], **kw)
        n = mats[b].shape[0]
        assert lam[b].item() == l1, (b, n, lam[b].item(), l1)
        assert int(it[b]) == it1, (b, n, int(it[b]), it1)
        assert int(st["converged_each"][b]) == c1, (b, n)
        assert vs[b].shape == (n,) and torch.equal(vs[b], v1), (b, n)
        assert torch.equal(work[b], fin1), (b, n)
        rounds = max(rounds, r1)
    return rounds


def mixed(orc, dt, dims, seed0=0):
    return [orc.hilbert(n, dt) if (i % 5 == 4 and n > 1) else orc.random_matrix(n, seed0 + i, dt)
            for i, n in enumerate(dims)]


def raw_call(solver, dt, ptrs, dims, d_v, opt=None, stats=None):
    """st_solve_vbatched_* itself.  Returns (rc, message, λ, counts, converged)."""
    b = len(dims)
    arr = (ctypes.c_void_p * max(1, b))(*ptrs)
    dims = np.asarray(dims, np.uint32)
    lam, it, conv = np.zeros(b, dt), np.zeros(b, np.uint32), np.zeros(b, np.uint32)
    _lib.check(solver.L.st_set_stream(solver.q, torch.cuda.current_stream(DEV).cuda_stream),
               "st_set_stream")
    rc = getattr(solver.L, "st_solve_vbatched_" + SFX[dt])(
        solver.q, arr, dims.ctypes.data, b, d_v, None, lam.ctypes.data, it.ctypes.data,
        conv.ctypes.data, None if opt is None else ctypes.byref(opt),
        None if stats is None else ctypes.byref(stats))
    return rc, _lib.last_error(solver.L), lam, it, conv


# ---------------------------------------------------------------------------
# 1. every class boundary, both dtypes, both semantics
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("sem", SEMS)
def test_every_class_boundary_bitwise_vs_single(solver, orc, dt, sem):
    dims = DIMS[dt] + DIMS[dt]                          # each dim twice, other seeds
    perm = np.random.RandomState(5).permutation(len(dims))
    dims = [dims[p] for p in perm]
    mats = [orc.random_matrix(n, 3 + int(p), dt) for n, p in zip(dims, perm)]
    work = [torch.from_numpy(m).to(DEV) for m in mats]
    lam, vs, it, st = solver.solve_vbatched(work, inplace=True, semantics=sem)
    assert lam.shape == (len(mats),) and it.shape == lam.shape and len(vs) == len(mats)
    rounds = assert_entries_equal_singles(solver, mats, work, lam, vs, it, st, semantics=sem)
    classes = _lib.vbatched_plan(dims, 1 if dt == np.float64 else 0)[2]
    print(f"{np.dtype(dt).name} sem={sem}: {len(mats)} matrices, {classes} classes, "
          f"iterations {[int(x) for x in it]}")
    assert classes == (6 if dt == np.float64 else 7)
    assert st["fused_launches"] == classes
    assert st["rounds"] == rounds and st["converged"] == 1


# ---------------------------------------------------------------------------
# 2. independent stopping across classes
# ---------------------------------------------------------------------------
def test_entries_stop_independently_across_classes(solver, orc):
    dt = np.float64
    mats, small = [], []
    for s in range(8):
        small.append(len(mats))
        mats.append(orc.random_matrix(2, s, dt))
        mats.append(orc.random_matrix(128, s, dt) if s % 2 else orc.random_matrix(33, s, dt))
    work = [torch.from_numpy(m).to(DEV) for m in mats]
    lam, vs, it, st = solver.solve_vbatched(work, inplace=True, semantics=_lib.ST_SEM_SYCL)
    assert [int(it[b]) for b in small] == N2_COUNTS
    rounds = assert_entries_equal_singles(solver, mats, work, lam, vs, it, st,
                                          semantics=_lib.ST_SEM_SYCL)
    assert st["rounds"] == rounds >= 22           # the 21-count entry evaluated 22 rounds
    assert st["converged"] == 1 and list(st["converged_each"]) == [1] * len(mats)
    assert st["fused_launches"] == 3


# ---------------------------------------------------------------------------
# 3. nothing outside the matrices and the eigenvectors is written
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,dims", [(np.float64, [1, 3, 128, 5, 17, 64, 33, 127, 2, 9]),
                                     (np.float32, [255, 1, 256, 3, 100, 6, 129, 17, 64, 33])])
def test_nothing_outside_is_written(solver, orc, dt, dims):
    gap = 64
    mats = mixed(orc, dt, dims)
    total = gap + sum(n * n + gap for n in dims)
    buf = torch.full((total,), SENTINEL, dtype=TD[dt], device=DEV)
    work, off = [], gap
    for m in mats:
        n = m.shape[0]
        w = buf[off:off + n * n].view(n, n)
        w.copy_(torch.from_numpy(m))
        work.append(w)
        off += n * n + gap
    nv = sum(dims)
    v = torch.full((nv + gap,), SENTINEL, dtype=TD[dt], device=DEV)
    stats = _lib.st_stats()
    rc, msg, lam, it, conv = raw_call(solver, dt, [w.data_ptr() for w in work], dims,
                                      v.data_ptr(), stats=stats)
    assert rc >= 0, msg
    torch.cuda.synchronize()
    sent = torch.full((gap,), SENTINEL, dtype=TD[dt], device=DEV)
    off = 0
    for n in dims:                                      # the gap in front of each matrix
        assert torch.equal(buf[off:off + gap], sent), (n, off)
        off += gap + n * n
    assert torch.equal(buf[off:off + gap], sent) and off + gap == total
    assert torch.equal(v[nv:], sent)
    vo = np.concatenate([[0], np.cumsum(dims)])
    vs = [v[int(vo[i]):int(vo[i + 1])] for i in range(len(dims))]
    st = {"converged_each": conv}
    assert_entries_equal_singles(solver, mats, work, torch.from_numpy(lam), vs, it, st)
    assert not bool((v[:nv] == SENTINEL).any())        # every eigenvector slot was written


# ---------------------------------------------------------------------------
# 4. a base one element off 16-byte alignment
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,n", [(np.float64, 64), (np.float32, 128)])
@pytest.mark.parametrize("sem", SEMS)
def test_misaligned_base_changes_no_bit(solver, orc, dt, n, sem):
    mats = [orc.random_matrix(n, 21, dt), orc.hilbert(n, dt)]
    aligned = [torch.from_numpy(m).to(DEV) for m in mats]
    per16 = 16 // np.dtype(dt).itemsize
    stride = n * n + per16                              # keeps every slot's alignment
    buf = torch.zeros(len(mats) * stride + 1, dtype=TD[dt], device=DEV)
    assert buf.data_ptr() % 16 == 0
    off1 = [buf[1 + i * stride:1 + i * stride + n * n].view(n, n) for i in range(len(mats))]
    for w, m in zip(off1, mats):
        w.copy_(torch.from_numpy(m))
        assert w.data_ptr() % 16 == np.dtype(dt).itemsize
    assert all(a.data_ptr() % 16 == 0 for a in aligned)
    la, va, ita, sta = solver.solve_vbatched(aligned, inplace=True, semantics=sem)
    lm, vm, itm, stm = solver.solve_vbatched(off1, inplace=True, semantics=sem)
    assert torch.equal(la, lm) and torch.equal(ita, itm)
    assert list(sta["converged_each"]) == list(stm["converged_each"])
    for b in range(len(mats)):
        assert torch.equal(va[b], vm[b]) and torch.equal(aligned[b], off1[b]), b
    assert_entries_equal_singles(solver, mats, off1, lm, vm, itm, stm, semantics=sem)


# ---------------------------------------------------------------------------
# 5. one class only: the uniform batched solve
# ---------------------------------------------------------------------------
def test_one_class_equals_uniform_batched(solver, orc):
    n, dt = 64, np.float64
    mats = np.stack([orc.random_matrix(n, s, dt) for s in range(8)] + [orc.hilbert(n, dt)])
    a = torch.from_numpy(mats).to(DEV)
    lam_u, v_u, it_u, st_u = solver.solve_batched(a, inplace=True)
    work = [torch.from_numpy(m).to(DEV) for m in mats]
    lam, vs, it, st = solver.solve_vbatched(work, inplace=True)
    assert st["fused_launches"] == 1
    assert torch.equal(lam, lam_u) and torch.equal(it, it_u)
    assert torch.equal(torch.stack(vs), v_u) and torch.equal(torch.stack(work), a)
    assert np.array_equal(st["converged_each"], st_u["converged_each"])
    assert st["rounds"] == st_u["rounds"] and st["converged"] == st_u["converged"]


# ---------------------------------------------------------------------------
# 6. max_itr = 2
# ---------------------------------------------------------------------------
def test_max_itr_2(solver, orc):
    dt = np.float64
    mats = [orc.random_matrix(2, s, dt) for s in range(8)]
    mats += [orc.random_matrix(33, 1, dt), orc.hilbert(128, dt), orc.random_matrix(9, 2, dt)]
    full = [single(solver, m)[2] for m in mats]         # counts of the unbounded solves
    work = [torch.from_numpy(m).to(DEV) for m in mats]
    lam, vs, it, st = solver.solve_vbatched(work, inplace=True, max_itr=2)
    assert_entries_equal_singles(solver, mats, work, lam, vs, it, st, max_itr=2)
    conv = [int(c) for c in st["converged_each"]]
    for b, c in enumerate(full):
        # ST_SEM_SYCL: a count c is a stop in round c, evaluated only if c < 2
        assert conv[b] == (1 if c < 2 else 0), (b, c)
        assert int(it[b]) == (c if c < 2 else 2), (b, c)
    assert 0 in conv and 1 in conv
    assert st["rounds"] == 2 and st["converged"] == 0


# ---------------------------------------------------------------------------
# 7. errors solve nothing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_errors_solve_nothing(solver, orc, dt):
    dims = [8, 5, 64, 3]
    lim = dev.batched_max_dim(dt)
    mats = mixed(orc, dt, dims)
    work = [torch.from_numpy(m).to(DEV) for m in mats]
    keep = [w.clone() for w in work]
    ptrs = [w.data_ptr() for w in work]
    v = torch.full((sum(dims),), SENTINEL, dtype=TD[dt], device=DEV)

    def refused(ptrs_, dims_, flags=0):
        opt = _lib.st_options(-1.0, 0, _lib.ST_SEM_SYCL, 0, flags)
        rc, msg, *_ = raw_call(solver, dt, ptrs_, dims_, v.data_ptr(), opt=opt)
        assert rc < 0
        return msg

    msg = refused(ptrs, [8, 0, 64, 3])
    assert "dims[1]" in msg and "= 0" in msg, msg
    msg = refused(ptrs, [8, 5, lim + 1, 3])
    assert "dims[2]" in msg and f"= {lim + 1}" in msg and "limit" in msg, msg
    msg = refused(ptrs[:3] + [None], dims)
    assert "d_mat_ptrs[3]" in msg and "NULL" in msg, msg
    for flag in (_lib.ST_FLAG_MATRIX_FREE, _lib.ST_FLAG_TIME_KERNELS, _lib.ST_FLAG_TRACE_SUMS,
                 _lib.ST_FLAG_ROUND_LOOP, _lib.ST_FLAG_BATCH_ROUNDS):
        assert "not supported" in refused(ptrs, dims, flag)
    torch.cuda.synchronize()
    for w, k in zip(work, keep):
        assert torch.equal(w, k)                        # nothing ran
    assert bool((v == SENTINEL).all())
    # an empty batch is a no-op
    stats = _lib.st_stats()
    stats.converged = 0
    rc, msg, *_ = raw_call(solver, dt, [], [], None, stats=stats)
    assert rc == 0 and stats.converged == 1 and stats.fused_launches == 0, msg
    lam, vs, it, st = solver.solve_vbatched([])
    assert lam.shape == (0,) and vs == [] and it.shape == (0,) and st["converged"] == 1
    # the wrapper raises the library's message
    big = torch.ones((lim + 1, lim + 1), dtype=TD[dt], device=DEV)
    with pytest.raises(_lib.EigenValueError, match=r"dims\[1\]"):
        solver.solve_vbatched([work[0], big])
    assert torch.equal(work[0], keep[0])


# ---------------------------------------------------------------------------
# 8. fronts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt,dims", [(np.float64, [3, 8, 5, 128, 33, 1, 64]),
                                     (np.float32, [5, 256, 3, 8, 100, 1, 129])])
def test_host_front_equals_device_front(solver, eigen, orc, dt, dims):
    mats = mixed(orc, dt, dims)
    keep = [m.copy() for m in mats]
    lam_h, vs_h, ts, it_h = eigen.similarity_transform_vbatched(mats)
    assert lam_h.dtype == dt and it_h.dtype == np.uint32 and ts >= 0 and len(vs_h) == len(mats)
    assert all(np.array_equal(m, k) for m, k in zip(mats, keep))        # read only
    # the tight packing puts some matrices off 16-byte alignment
    offs = np.concatenate([[0], np.cumsum([n * n for n in dims])])[:-1] * np.dtype(dt).itemsize
    assert any(int(o) % 16 for o in offs) and any(int(o) % 16 == 0 for o in offs)
    inputs = [torch.from_numpy(m).to(DEV) for m in mats]
    lam, vs, it, st = solver.solve_vbatched(inputs)                     # not inplace
    for a, k in zip(inputs, keep):
        assert torch.equal(a, torch.from_numpy(k).to(DEV))              # inputs untouched
    assert np.array_equal(lam.numpy(), lam_h) and np.array_equal(it.numpy(), it_h.astype(np.int64))
    for b in range(len(mats)):
        assert vs_h[b].shape == (dims[b],) and np.array_equal(vs[b].cpu().numpy(), vs_h[b]), b
        l1, v1, it1, _, _, _ = single(solver, mats[b])
        assert lam_h[b] == l1 and int(it_h[b]) == it1 and np.array_equal(vs_h[b], v1.cpu().numpy())
    lam0, vs0, _, it0 = eigen.similarity_transform_vbatched([])
    assert lam0.shape == (0,) and vs0 == [] and it0.shape == (0,)


def test_dlpack_producers_and_argument_checks(solver, orc):
    class Producer:
        def __init__(self, t):
            self.t = t

        def __dlpack__(self, **kw):
            return self.t.__dlpack__(**kw)

        def __dlpack_device__(self):
            return self.t.__dlpack_device__()

    mats = mixed(orc, np.float64, [6, 17])
    ts = [torch.from_numpy(m).to(DEV) for m in mats]
    want = solver.solve_vbatched(ts)
    got = solver.solve_vbatched([Producer(ts[0]), ts[1]])
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    assert all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
    # in place through a producer: the producer's storage is transformed
    solver.solve_vbatched([Producer(ts[0]), Producer(ts[1])], inplace=True)
    assert torch.equal(ts[0], single(solver, mats[0])[5])
    with pytest.raises(ValueError, match="contiguous"):
        solver.solve_vbatched([torch.from_numpy(mats[0]).to(DEV).t()], inplace=True)
    with pytest.raises(TypeError):
        solver.solve_vbatched([ts[0], ts[1].float()])
    with pytest.raises(ValueError):
        solver.solve_vbatched([torch.from_numpy(mats[0])])              # a host tensor
    with pytest.raises(AssertionError, match="square"):
        solver.solve_vbatched([torch.ones((2, 3), dtype=torch.float64, device=DEV)])
    # a transposed (non-contiguous) input is fine when copied
    lam_t = solver.solve_vbatched([torch.from_numpy(mats[0].T.copy()).to(DEV).t()])[0]
    assert lam_t[0].item() == single(solver, mats[0])[0]


# ---------------------------------------------------------------------------
# 9. context reuse: grown buffers, then the other solves on the same context
# ---------------------------------------------------------------------------
def test_context_reuse(orc):
    s = dev.DeviceSolver(DEV)
    try:
        dt = np.float64
        dims = [int(x) for x in np.random.RandomState(9).randint(1, 17, size=3000)]
        mats = [orc.random_matrix(n, 1000 + i, dt) for i, n in enumerate(dims)]
        work = [torch.from_numpy(m).to(DEV) for m in mats]
        lam, vs, it, st = s.solve_vbatched(work, inplace=True)
        spots = [0, 1, 2, 7, 100, 511, 999, 1000, 1500, 2047, 2048, 2500, 2900, 2997, 2998, 2999]
        assert_entries_equal_singles(s, mats, work, lam, vs, it, st, entries=spots)
        assert st["converged"] == 1 and st["fused_launches"] == 3
        assert bool((st["converged_each"] == 1).all()) and int(it.min()) >= 0
        # a small batch in the grown buffers
        dims5 = [128, 2, 33, 2, 64]
        mats5 = mixed(orc, dt, dims5, seed0=40)
        work5 = [torch.from_numpy(m).to(DEV) for m in mats5]
        lam5, vs5, it5, st5 = s.solve_vbatched(work5, inplace=True)
        assert_entries_equal_singles(s, mats5, work5, lam5, vs5, it5, st5)
        # the uniform batched solve and the single solve on the same context
        n = 16
        stack = np.stack([orc.random_matrix(n, q, dt) for q in range(4)])
        a = torch.from_numpy(stack).to(DEV)
        lam_u, v_u, it_u, st_u = s.solve_batched(a, inplace=True)
        for b in range(4):
            l1, v1, it1, c1, _, fin1 = single(s, stack[b])
            assert lam_u[b].item() == l1 and int(it_u[b]) == it1 and torch.equal(v_u[b], v1)
            assert torch.equal(a[b], fin1)
        one = torch.from_numpy(stack[2]).to(DEV)
        l1, v1, it1, st1 = s.solve(one, inplace=True)
        assert l1 == lam_u[2].item() and it1 == int(it_u[2]) and torch.equal(v1, v_u[2])
    finally:
        s.close()
