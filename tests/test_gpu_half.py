"""GPU: the matrix-free round, K0 and the whole solve on a matrix stored in
16 bits (fp16 / bf16), fp32 vectors and arithmetic.

  1. indexing, independent of the summation order: integer data on which
     every product and partial sum is exact, so s_next and the K0 sums must
     EQUAL numpy's integers - at every boundary of the sweep (a chunk is 8
     columns per lane, 8 * 256 = 2048 per workgroup pass, the unrolled stride
     2 * 2048 = 4096), on the 16-byte and the element-wide path, in every
     launch shape (1, 2 and 8 rows per group, cached and non-temporal);
  2. what does not touch the matrix - v_cur and the whole st_state - is
     bitwise st_mfree_round_f32's on the widened matrix;
  3. row sums against an exact sum, within (levels + 1) ulps (+ 1 for the
     division), levels written below from the kernel's own order;
  4. whole solves against the fp32 matrix-free solve of the widened matrix;
  5. behaviour of the fronts, and st_narrow_f32 against torch's rounding.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import eigen_value_amd as ev  # noqa: E402
import exact_sums as xs  # noqa: E402
import stop_parity as sp  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402

DEV = "cuda:0"
STORAGES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
SYCL, MAINPY = _lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY

# the sweep of st_half.h: 8 columns per lane and chunk, 256 lanes, U = 2
W, BLOCK = 8, xs.BLOCK
U = int(dict(kv.split("=") for kv in
             _lib.load().st_half_shape_desc().decode().split())["unroll"])
CHUNK = W * BLOCK            # columns one pass of the workgroup covers
STRIDE = U * CHUNK           # columns of the unrolled loop's step


def levels_half(ncols: int) -> int:
    """Rounding additions on the longest path of a row sum of half_group
    (st_half.h): lane t holds the chunks t, t + 256, ... of 8 columns and adds
    one fused multiply-add per element in column order - 8 * chunks - 1 past
    the first, which meets a zero accumulator - then wave_sum's tree over the
    lanes that hold a chunk and the serial add of the wave partials (the
    structure of exact_sums._sweep_levels with w = 8, fused)."""
    nch = -(-ncols // W)
    chunks = -(-nch // BLOCK)
    return (W * chunks - 1) + xs._tree(nch) + xs._wave_combine(nch)


def test_levels_half_by_hand():
    assert levels_half(1) == 7            # one lane: 8 slots, 7 adds past the first
    assert levels_half(8) == 7
    assert levels_half(9) == 7 + 1        # two lanes: one tree level
    assert levels_half(300) == 7 + 6      # 38 lanes of one wave
    assert levels_half(2048) == 7 + 6 + 3  # 256 lanes: the tree, 3 wave adds
    assert levels_half(2056) == 15 + 6 + 3  # lane 0 holds a second chunk
    assert levels_half(4104) == 23 + 6 + 3


def state_bytes(state) -> bytes:
    return state.cpu().numpy().tobytes()


def sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 1. exact arithmetic: the indexing test
# ---------------------------------------------------------------------------
def int_case(nrows, ncols, seed, off2=False):
    """Integers 1..8 as float32 (exact in fp16 and bf16); s in {1, 2, 4}."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 9, size=(nrows, ncols)).astype(np.float32)
    s = rng.choice(np.array([1, 2, 4], np.float32), size=ncols)
    return a, s


def half_tensor(a32: np.ndarray, dt, off2=False):
    """a32 as a contiguous `dt` device tensor; off2: 2 bytes past a 16-byte
    boundary (the element-wide path at an ncols that is a multiple of 8)."""
    t = torch.from_numpy(a32).to(dt)
    if not off2:
        return t.to(DEV)
    flat = torch.empty(t.numel() + 1, dtype=dt, device=DEV)
    assert flat.data_ptr() % 16 == 0
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    return view


def run_exact(dt, nrows, ncols, row0, seed, off2=False, k=1):
    a, s = int_case(nrows, ncols, seed)
    h = half_tensor(a, dt, off2)
    # K0
    got0 = dev.rowsum_half(h).cpu().numpy()
    want0 = a.astype(np.float64).sum(axis=1)
    assert want0.max() < 2 ** 24
    assert np.array_equal(got0.astype(np.float64), want0), (nrows, ncols, "K0")
    if row0 + nrows > ncols:
        return
    s_prev = torch.from_numpy(s).to(DEV)
    v_prev = torch.ones(ncols, dtype=torch.float32, device=DEV)
    v_cur = torch.empty_like(v_prev)
    s_next = torch.full((nrows,), -1.0, dtype=torch.float32, device=DEV)
    st = dev.new_state(DEV)
    dev.mfree_round_half(h, s_prev, s_next, v_prev, v_cur, st, row0=row0, eps=0.0, k=k,
                         max_itr=100)
    x = s.astype(np.float64)
    t = a.astype(np.float64) @ x
    assert t.max() < 2 ** 24
    want = t / x[row0:row0 + nrows]
    assert np.array_equal(s_next.cpu().numpy().astype(np.float64), want), (nrows, ncols, row0)


BOUNDARY_NCOLS = [1, 2, 7, 8, 9, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1,
                  STRIDE - 1, STRIDE, STRIDE + 1]


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
@pytest.mark.parametrize("ncols", BOUNDARY_NCOLS)
def test_exact_at_every_sweep_boundary(dt, ncols):
    for nrows in (1, 5, 9):
        run_exact(dt, nrows, ncols, 0, seed=ncols * 16 + nrows)
    if ncols >= 16:                                    # a block inside the vector
        run_exact(dt, 5, ncols, ncols - 7, seed=ncols, k=2)


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
def test_exact_misaligned_matrix_takes_the_element_path(dt):
    """ncols % 8 == 0 but the matrix starts 2 bytes past a 16-byte boundary:
    the element-wide path, the same integers."""
    for ncols in (16, CHUNK + 8, STRIDE + 8):
        run_exact(dt, 5, ncols, 3, seed=ncols + 1, off2=True)


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
def test_exact_every_ncols_to_64(dt):
    for ncols in range(1, 65):
        run_exact(dt, 3, ncols, 0, seed=1000 + ncols)


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
@pytest.mark.parametrize("nrows,ncols,row0", [
    (1029, 1040, 11),       # 8 rows per group (<= 64 MiB): 128 groups + 5 remainder rows
    (1029, 1037, 3),        # the same on the element-wide path
    (4099, 8200, 101),      # 2 rows per group (64 .. 280 MiB), cached, + 1 remainder row
], ids=["rows8", "rows8-elementwide", "rows2"])
def test_exact_in_the_grouped_launch_shapes(dt, nrows, ncols, row0):
    """From 1024 rows the launch groups rows (the table of k_mfree read with
    N^2 * 2 bytes): main groups and remainder rows, odd launch index k = the
    reversed walk."""
    run_exact(dt, nrows, ncols, row0, seed=nrows, k=3)


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
def test_exact_in_the_nontemporal_shape(dt):
    """A block of >= 512 MiB takes non-temporal loads, 8 rows per group.
    Integer data generated and summed on the device (fp64 matmul of small
    integers is exact in any order)."""
    nrows, ncols, row0 = 16389, 16400, 5              # 513 MiB, 2048 groups + 5 rows
    g = torch.Generator(device=DEV).manual_seed(5)
    h = torch.randint(1, 9, (nrows, ncols), device=DEV, generator=g,
                      dtype=torch.int32).to(dt)
    s_prev = (2.0 ** torch.randint(0, 3, (ncols,), device=DEV, generator=g)).float()
    x = s_prev.double()
    want0 = torch.empty(nrows, dtype=torch.float64, device=DEV)
    want = torch.empty(nrows, dtype=torch.float64, device=DEV)
    for r in range(0, nrows, 2048):
        blk = h[r:r + 2048].double()
        want0[r:r + 2048] = blk.sum(dim=1)
        want[r:r + 2048] = (blk @ x) / x[row0 + r:row0 + r + blk.shape[0]]
    assert float(want0.max()) < 2 ** 24 and float((want * x.max()).max()) < 2 ** 24
    assert torch.equal(dev.rowsum_half(h).double(), want0)
    v_prev = torch.ones(ncols, dtype=torch.float32, device=DEV)
    v_cur = torch.empty_like(v_prev)
    s_next = torch.full((nrows,), -1.0, dtype=torch.float32, device=DEV)
    st = dev.new_state(DEV)
    dev.mfree_round_half(h, s_prev, s_next, v_prev, v_cur, st, row0=row0, eps=0.0, k=1,
                         max_itr=100)
    assert torch.equal(s_next.double(), want)


# ---------------------------------------------------------------------------
# 2. matrix-independent outputs: bitwise the fp32 kernel's
# ---------------------------------------------------------------------------
def s_vectors(n):
    rng = np.random.default_rng(n)
    ramp = (1.0 + 1e-4 * np.arange(n)).astype(np.float32)
    return {
        "running": (1.0 + rng.random(n)).astype(np.float32),       # no pair below eps
        "stopping": np.full(n, 5.0, np.float32),                    # every pair equal
        # neighbours 1e-4 apart, the ends n * 1e-4 apart: stops only where the
        # pair (n - 1, 0) is not inspected
        "open-only": ramp,
    }


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
@pytest.mark.parametrize("sem", [SYCL, MAINPY])
@pytest.mark.parametrize("n", [300, 2056, CHUNK + 5])
def test_v_and_state_are_bitwise_the_fp32_kernels(dt, sem, n):
    rng = np.random.default_rng(7 * n)
    a = rng.random((n, n), dtype=np.float32) + np.float32(0.25)
    h = torch.from_numpy(a).to(dt).to(DEV)
    w = h.float()
    v_np = (0.5 + rng.random(n)).astype(np.float32)
    eps = 1e-3
    for name, s_np in s_vectors(n).items():
        for k, max_itr in ((3, 10), (4, 4)):                       # (4, 4): exhaustion
            s_prev = torch.from_numpy(s_np).to(DEV)
            v_prev = torch.from_numpy(v_np).to(DEV)
            out = {}
            for which in ("half", "f32"):
                st = dev.new_state(DEV)
                v_cur = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
                s_next = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
                if which == "half":
                    dev.mfree_round_half(h, s_prev, s_next, v_prev, v_cur, st, eps=eps, k=k,
                                         max_itr=max_itr, semantics=sem)
                else:
                    dev.mfree_round(w, s_prev, s_next, v_prev, v_cur, st, eps=eps, k=k,
                                    max_itr=max_itr, semantics=sem)
                sync()
                out[which] = (v_cur.cpu().numpy().tobytes(), state_bytes(st),
                              dev.read_state(st), s_next, st)
            tag = (name, k, max_itr, sem, n)
            assert out["half"][0] == out["f32"][0], ("v_cur", tag)
            assert out["half"][1] == out["f32"][1], ("state", tag, out["half"][2], out["f32"][2])
            state = out["half"][2]
            stops = name == "stopping" or (name == "open-only" and sem == MAINPY)
            assert state["stop"] == int(stops), tag
            assert state["round"] == k - 1 and state["eigen_val"] == float(s_np[0]), tag
            assert state["max"] == float(s_np.max()), tag
            ended = stops or k >= max_itr
            assert (state["done"], state["end"]) == ((1, k) if ended else (0, 0)), tag
            if ended:
                want = (k - 1 if sem == SYCL else k) if stops else max_itr
                assert state["iters"] == want, tag
            # the row sums differ from the fp32 kernel's in association only
            assert torch.allclose(out["half"][3], out["f32"][3], rtol=1e-5, atol=0), tag
            if ended:                                   # a later launch is a no-op
                st = out["half"][4]
                v2 = torch.full((n,), -9.0, dtype=torch.float32, device=DEV)
                s2 = torch.full((n,), -9.0, dtype=torch.float32, device=DEV)
                dev.mfree_round_half(h, s_prev, s2, v_prev, v2, st, eps=eps, k=k + 1,
                                     max_itr=max_itr + 5, semantics=sem)
                sync()
                assert float(v2.max()) == -9.0 and float(v2.min()) == -9.0, tag
                assert float(s2.max()) == -9.0 and float(s2.min()) == -9.0, tag
                assert state_bytes(st) == out["half"][1], tag


# ---------------------------------------------------------------------------
# 3. row sums against an exact sum, in ulps
# ---------------------------------------------------------------------------
ACC_SHAPES = [(9, 2056), (9, STRIDE + 8), (300, 300)]


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
@pytest.mark.parametrize("shape", ACC_SHAPES, ids=[f"{r}x{c}" for r, c in ACC_SHAPES])
def test_row_sums_within_levels_of_the_exact_sum(dt, shape):
    """|s_next - exact| <= levels + 1 ulps + 1 for the division; K0 levels + 1.
    exact: x = fl32(v * s) as the kernel forms it, the fp64 products A * x
    (exact: 11 x 24 bits) summed by math.fsum, divided by x[r] in fp64."""
    nrows, ncols = shape
    rng = np.random.default_rng(nrows * 100003 + ncols)
    a = (1.0 - rng.random((nrows, ncols))).astype(np.float32)           # (0, 1]
    h = torch.from_numpy(a).to(dt).to(DEV)
    w = h.float()
    a64 = w.cpu().numpy().astype(np.float64)                            # the stored values
    s_np = (0.5 + rng.random(ncols)).astype(np.float32)
    v_np = (0.5 + rng.random(ncols)).astype(np.float32)
    x32 = v_np * s_np                                                   # fl32(v * s)
    x = x32.astype(np.float64)
    exact = np.array([math.fsum(a64[r] * x) for r in range(nrows)]) / x[:nrows]
    exact0 = np.array([math.fsum(a64[r]) for r in range(nrows)])
    s_prev, v_prev = torch.from_numpy(s_np).to(DEV), torch.from_numpy(v_np).to(DEV)
    got = {}
    for which in ("half", "f32"):
        st = dev.new_state(DEV)
        v_cur = torch.empty(ncols, dtype=torch.float32, device=DEV)
        s_next = torch.empty(nrows, dtype=torch.float32, device=DEV)
        if which == "half":
            dev.mfree_round_half(h, s_prev, s_next, v_prev, v_cur, st, eps=0.0, k=1, max_itr=9)
        else:
            dev.mfree_round(w, s_prev, s_next, v_prev, v_cur, st, eps=0.0, k=1, max_itr=9)
        got[which] = np.abs(xs.err_ulps_of(s_next.cpu().numpy(), exact, np.float32)).max()
    e0 = np.abs(xs.err_ulps_of(dev.rowsum_half(h).cpu().numpy(), exact0, np.float32)).max()
    e0_f32 = np.abs(xs.err_ulps_of(dev.rowsum(w).cpu().numpy(), exact0, np.float32)).max()
    L = levels_half(ncols)
    print(f"half rowsum error {IDS[STORAGES.index(dt)]} {nrows}x{ncols}: s_next max|e| "
          f"{got['half']:.3f} ulps (fp32 k_mfree {got['f32']:.3f}), K0 {e0:.3f} "
          f"(fp32 k_fused {e0_f32:.3f}), levels {L}")
    assert got["half"] <= L + 1 + 1, (got, L)
    assert e0 <= L + 1, (e0, L)


# ---------------------------------------------------------------------------
# 4. whole solves against the fp32 matrix-free solve of the widened matrix
# ---------------------------------------------------------------------------
SOLVE_N = [1, 3, 8, 100, 257, 1024, 2056]
SOLVE_CASES = [(kind, n, dt) for kind in ("random", "hilbert") for n in SOLVE_N
               for dt in STORAGES]
SOLVE_IDS = [f"{k}-{n}-{IDS[STORAGES.index(d)]}" for k, n, d in SOLVE_CASES]
SEED = 3
_SOLVED = {}


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def half_input(orc, kind, n, dt):
    a = orc.hilbert(n, np.float32) if kind == "hilbert" else orc.random_matrix(n, SEED, np.float32)
    return dev.narrow(torch.from_numpy(np.ascontiguousarray(a)).to(DEV), dt)


def solved(orc, solver, kind, n, dt):
    """Both solves of one case and the comparison of their traces, once."""
    key = (kind, n, dt)
    if key not in _SOLVED:
        h = half_input(orc, kind, n, dt)
        w = h.float()
        lam, v, it, st = solver.solve_half(h, trace_sums=True)
        tr = solver.last_round_sums()
        lam_w, v_w, it_w, st_w = solver.solve(w, matrix_free=True, trace_sums=True)
        tr_w = solver.last_round_sums()
        cmp = sp.compare(tr, tr_w, xs.EPS_F32, True, _lib.ST_MAX_ITR, matrix_free=True)
        _SOLVED[key] = dict(lam=lam, v=v.cpu().numpy(), it=it, st=st, lam_w=lam_w,
                            v_w=v_w.cpu().numpy(), it_w=it_w, st_w=st_w, cmp=cmp,
                            w=w.cpu().numpy() if n == 100 else None)
    return _SOLVED[key]


@pytest.mark.parametrize("kind,n,dt", SOLVE_CASES, ids=SOLVE_IDS)
def test_solve_matches_the_fp32_matrix_free_solve(orc, solver, kind, n, dt):
    r = solved(orc, solver, kind, n, dt)
    assert r["st"]["converged"] == 1 and r["st_w"]["converged"] == 1
    assert abs(r["lam"] - r["lam_w"]) <= 1e-5 * abs(r["lam_w"]), (r["lam"], r["lam_w"])
    assert np.max(np.abs(r["v"] - r["v_w"])) <= 1e-4
    same = sp.assert_stop_parity(r["cmp"], (kind, n, str(dt)))
    if same:
        assert r["it"] == r["it_w"], (r["it"], r["it_w"])
    print(f"half solve {kind} {n} {dt}: {r['it']} rounds (fp32 {r['it_w']}), "
          f"max row-sum deviation {r['cmp']['max_dev_ulps']} ulps, straddle {r['cmp']['straddle']}")


def test_solve_straddles_at_most_once_over_all_cases(orc, solver):
    """The cap of the parametrisation above (fixed seeds): at most 1 case whose
    two traces put a round's max |ds| on opposite sides of EPS."""
    straddles = [k for k in SOLVE_CASES if solved(orc, solver, *k)["cmp"]["straddle"] is not None]
    assert len(straddles) <= 1, straddles


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
def test_solve_matches_the_cpu_oracle_on_the_widened_matrix(orc, solver, dt):
    r = solved(orc, solver, "random", 100, dt)
    ref = orc.similarity_transform(r["w"], orc.SEM_SYCL)
    assert r["it"] == ref.iter_count, (r["it"], ref.iter_count)
    assert abs(r["lam"] - float(ref.eigen_val)) <= 1e-5 * abs(float(ref.eigen_val))
    assert np.max(np.abs(r["v"] - ref.eigen_vec)) <= 1e-4


# ---------------------------------------------------------------------------
# 5. behaviour
# ---------------------------------------------------------------------------
def np_bits(h):
    """A half tensor as the numpy array the host front takes."""
    if h.dtype == torch.float16:
        return h.cpu().numpy(), None
    return h.view(torch.int16).cpu().numpy().view(np.uint16), "bf16"


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
def test_input_is_never_written_and_views_are_solved_as_copies(orc, solver, dt):
    h = half_input(orc, "random", 264, dt)
    before = h.clone()
    lam, v, it, st = solver.solve_half(h)
    assert torch.equal(h.view(torch.int16), before.view(torch.int16))
    t = h.t()                                           # a non-contiguous view
    assert not t.is_contiguous()
    lam_t, v_t, it_t, _ = solver.solve_half(t)
    lam_c, v_c, it_c, _ = solver.solve_half(t.contiguous())
    assert (lam_t, it_t) == (lam_c, it_c) and torch.equal(v_t, v_c)
    assert torch.equal(h.view(torch.int16), before.view(torch.int16))
    assert v.dtype == torch.float32 and isinstance(lam, float)


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
def test_fixed_rounds_timing_and_trace(orc, solver, dt):
    h = half_input(orc, "random", 520, dt)
    lam, v, it, st = solver.solve_half(h, eps=0.0, max_itr=7, time_kernels=True,
                                       trace_sums=True)
    assert (it, st["rounds"], st["converged"]) == (7, 7, 0)
    ms = solver.last_round_times()
    assert ms.shape == (7,) and (ms > 0).all() and st["fused_launches"] == 7
    tr = solver.last_round_sums()
    assert tr.shape == (7, 520) and tr.dtype == np.float32
    assert np.array_equal(tr[0], dev.rowsum_half(h).cpu().numpy())      # s_0 is K0's
    assert float(tr[6][0]) == lam                                       # lambda = s_6[0]
    for sem in (SYCL, MAINPY):                          # batch: same results
        a = solver.solve_half(h, semantics=sem)
        b = solver.solve_half(h, semantics=sem, batch=1)
        assert (a[0], a[2]) == (b[0], b[2]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
def test_host_front_equals_device_front_bit_for_bit(orc, solver, dt):
    h = half_input(orc, "random", 300, dt)
    lam, v, it, _ = solver.solve_half(h)
    arr, storage = np_bits(h)
    with ev.EigenValue() as e:
        lam_h, v_h, ts, it_h = e.similarity_transform_half(arr, storage=storage)
    assert lam_h.dtype == np.float32 and v_h.dtype == np.float32 and ts >= 0
    assert float(lam_h) == lam and it_h == it
    assert v_h.tobytes() == v.cpu().numpy().tobytes()


def test_other_dtypes_are_type_errors(solver):
    with pytest.raises(TypeError, match="float16/bfloat16"):
        solver.solve_half(torch.ones((4, 4), dtype=torch.float32, device=DEV))
    with pytest.raises(TypeError, match="float32/float64"):
        solver.solve(torch.ones((4, 4), dtype=torch.float16, device=DEV))
    with pytest.raises(TypeError):
        dev.narrow(torch.ones(4, dtype=torch.float64, device=DEV), torch.float16)
    with pytest.raises(TypeError):
        dev.narrow(torch.ones(4, dtype=torch.float32, device=DEV), torch.float32)


@pytest.mark.parametrize("dt", STORAGES, ids=IDS)
def test_narrow_is_torchs_round_to_nearest_even(dt):
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(10000) * np.exp(rng.uniform(-8, 8, 10000))).astype(np.float32)
    ties = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,
                     -(1 + 2.0 ** -11), -(1 + 2.0 ** -8), 0.0, -0.0, 65504.0, 65520.0, 1e5,
                     3e38, 3.4e38, 1e-8, 6e-8, np.inf, -np.inf], np.float32)
    t = torch.from_numpy(np.concatenate([x, ties])).to(DEV)
    got = dev.narrow(t, dt)
    want = t.to(dt)
    assert got.dtype == dt and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert float(dev.narrow(t[10000:10001], dt)[0]) == 1.0              # the tie: to even
    nan = dev.narrow(torch.tensor([float("nan")], device=DEV), dt)
    assert bool(torch.isnan(nan.float())[0])
