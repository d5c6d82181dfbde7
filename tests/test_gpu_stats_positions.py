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

k_mfree_half (st_half.h) has a fold of its own, half_group's, in which a lane
takes 8 columns per chunk: its sweeps place the positions by that width
(sv.positions(..., w=8)), on the 16-byte and the element-wide path, the
latter also at n % 8 == 0 with a matrix off 16 bytes.

From 1024 rows every launcher groups rows and takes other instantiations:
k_mfree 2 or 4 rows per group with cached or non-temporal loads, k_mfree_half
2 (one chunk in flight) or 8, k_round 2.  There every workgroup computes m
itself and scales its own slice of v with it, the walk is reversed on odd k,
and workgroup 0's first group - the one whose fold reaches the state - can be
a remainder row.  The *_grouped sweeps run blocks of 2049 / 4097 / 4099 /
16389 rows, at both parities of k, and assert the launch shape they mean to
test: k_mfree_half's non-temporal shape on a 513 MiB block, k_mfree's (which
the table takes from 512 MiB) on 2049 rows through the tuning build's
st_set_mfree_shape(3).

Not reachable from here: the non-temporal instantiations of k_round (blocks
of 1 GiB and more) and k_flat (2 GiB; the full-size solve tests run both) and
k_stats as a launch of its own (the three-launch form is compiled out).
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


def cases(orc, n, dt, cyclic, only=None, w=None):
    """tags, S (case, n), eps, and what the oracle and numpy say of each row:
    stop and m.  `only`: restrict the positions (the full-size leg).  `w`: the
    columns a lane takes per chunk (sv.positions; None = one 16-byte vector)."""
    key = (n, np.dtype(dt).name, cyclic, None if only is None else tuple(only), w)
    if key in _CASES:
        return _CASES[key]
    eps, ee = dt(sv.EPS), dt(sv.EXACT_EPS)
    rows = []                                       # (tag, s, eps, designed stop)
    # `only`: those positions, where the semantics has a pair / an element there
    pick = (lambda ps: [p for p in sorted(only) if p <= ps[-1]]) if only is not None else (
        lambda ps: ps)
    for p in pick(sv.positions(n, dt, cyclic, w=w)):
        rows += [(("one_fail", p), sv.one_fail(n, p, dt, eps, cyclic), eps, 0),
                 (("all_pass", p), sv.all_pass(n, p, dt, eps, cyclic), eps, 1),
                 (("exact_fail", p), sv.exact_eps(n, p, dt, "fail", cyclic), ee, 0),
                 (("exact_pass", p), sv.exact_eps(n, p, dt, "pass", cyclic), ee, 1)]
    for p in pick(sv.positions(n, dt, True, w=w)):  # an element, not a pair: p = n - 1 too
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
    assert 0 < c.stop.sum() < len(rows)             # stopping and non-stopping jobs
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


def expect_v(c, ci, v0, full, block=(NROWS, ROW0)):
    nrows, row0 = block
    with np.errstate(invalid="ignore"):
        upd = v0[None, :] * (c.S[ci] / c.m[ci][:, None])        # cpp:260, in the dtype
    assert upd.dtype == c.dt
    if full:
        return upd
    out = np.tile(v0, (len(ci), 1))
    out[:, row0:row0 + nrows] = upd[:, row0:row0 + nrows]
    return out


def sweep(orc, dt, sem, n, launch, *, full_v=False, flat=False, rk=K, epilogue=False,
          jobs_of=None, setup=None, block=(NROWS, ROW0), launch_k=None, w=None, mat=None):
    """Run `launch(x, j, ci, extra)` for every job (case ci, extra), each with
    its own v and state, read everything back once and compare.

    block     (nrows, row0) of the matrix block; x.nrows / x.row0
    launch_k  the launch index k of a matrix-free launch (x.k), which
              evaluates round rk = k - 1; otherwise `rk` is the round itself
    w         the chunk width of the positions (cases)
    mat       x -> the block on the device, for blocks too large to generate
              on the host (default: the oracle's seeded random rows)"""
    cyclic = sem == _lib.ST_SEM_SYCL
    nrows, row0 = block
    assert row0 + nrows <= n
    if launch_k is not None:
        rk = launch_k - 1
    c = cases(orc, n, dt, cyclic, w=w)
    jobs = [(ci, None) for ci in range(len(c.tags))] if jobs_of is None else jobs_of(c)
    v0 = orc.random_matrix(n, 5, dt, nrows=1)[0]
    x = types.SimpleNamespace(n=n, sem=sem, c=c, nrows=nrows, row0=row0, k=launch_k)
    if mat is None:
        x.mat = torch.from_numpy(orc.random_matrix(n, 3, dt, nrows=nrows, row0=row0)).to(DEV)
    else:
        x.mat = mat(x)
    assert tuple(x.mat.shape) == (nrows, n)
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
    check("v", x.V.cpu().numpy(), expect_v(c, ci, v0, full_v, block), jobs, c)


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
# the 16-bit-storage round: half_group's own fold, 8 columns per lane and chunk
# ---------------------------------------------------------------------------
F32 = np.float32
HALF_W = 8
STORAGES = [pytest.param(torch.float16, id="f16"), pytest.param(torch.bfloat16, id="bf16")]
SEM_PARAMS = [pytest.param(s, id="sycl" if s == _lib.ST_SEM_SYCL else "mainpy") for s in SEMS]
MIB = 1 << 20


def half_desc():
    return {k: int(v) for k, v in (kv.split("=") for kv in
                                   _lib.load().st_half_shape_desc().decode().split())}


def device_block(x):
    """The block generated on the device (the library's seeded generator)."""
    dt = torch.float64 if x.c.dt == np.float64 else torch.float32
    return dev.generate("random", x.n, dt, nrows=x.nrows, row0=x.row0, seed=3, device=DEV)


def half_block(storage, off2=False):
    """x -> the fp32 block narrowed to `storage` by st_narrow_f32; off2: 2
    bytes past a 16-byte boundary (test_gpu_half.half_tensor's way)."""
    def make(x):
        a = device_block(x)
        if not off2:
            h = dev.narrow(a, storage)
            assert h.data_ptr() % 16 == 0
            return h
        flat = torch.empty(a.numel() + 1, dtype=storage, device=DEV)
        assert flat.data_ptr() % 16 == 0
        h = flat[1:].view(a.shape)
        dev.narrow(a, storage, out=h)
        assert h.data_ptr() % 16 == 2 and h.is_contiguous()
        return h
    return make


def half_block_of_integers(storage):
    """x -> small integers generated on the device (exact in both formats), as
    test_gpu_half.test_exact_in_the_nontemporal_shape makes its matrix."""
    def make(x):
        g = torch.Generator(device=DEV).manual_seed(5)
        return torch.randint(1, 9, (x.nrows, x.n), device=DEV, generator=g,
                             dtype=torch.int32).to(storage)
    return make


def half_launch(x, j, ci, _):
    dev.mfree_round_half(x.mat, x.S[ci], x.s_next, x.v0, x.V[j], x.ST[j], row0=x.row0,
                         eps=x.eps[ci], k=x.k, max_itr=MAX_ITR, semantics=x.sem)


def vector_path(x):
    """What mfree_half's vec_ok reads (st_half.hip)."""
    return (x.n % HALF_W == 0 and x.mat.data_ptr() % 16 == 0 and x.v0.data_ptr() % 16 == 0
            and all(x.S[ci].data_ptr() % 16 == 0 for ci in range(x.S.shape[0])))


@pytest.mark.parametrize("n", sv.SIZES)
@pytest.mark.parametrize("sem", SEM_PARAMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_mfree_half_round(orc, storage, sem, n):
    """k_mfree_half, 1 row per group: the STATS block of half_group at every
    chunk (7|8), wave (511|512), workgroup-pass (2047|2048) and unrolled-stride
    (4095|4096) boundary, in sweep_tail, in the ragged last chunk and at the
    wrap.  n = 9, 257, 1031: the element-wide path (zeros past the row); the
    others the 16-byte path."""
    def setup(x):
        assert vector_path(x) == (n % HALF_W == 0)
    sweep(orc, F32, sem, n, half_launch, full_v=True, launch_k=1, w=HALF_W,
          mat=half_block(storage), setup=setup)


@pytest.mark.parametrize("sem", SEM_PARAMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_mfree_half_round_misaligned_matrix(orc, storage, sem):
    """n = 1032 with the matrix 2 bytes past a 16-byte boundary: the
    element-wide path at n % 8 == 0, where no column lies past the row."""
    def setup(x):
        assert not vector_path(x) and x.mat.data_ptr() % 16 == 2
    sweep(orc, F32, sem, 1032, half_launch, full_v=True, launch_k=1, w=HALF_W,
          mat=half_block(storage, off2=True), setup=setup)


def half_grouped_shape(nrows, ncols):
    """(rows per group, chunks in flight, non-temporal, groups + remainder
    rows, workgroups, groups of workgroup 0) of mfree_half's launch - from the
    library's own description of its table and the block's bytes, so that a
    retuned table fails the shape assertions below instead of moving the
    sweeps to another instantiation unnoticed."""
    d = half_desc()
    b = nrows * ncols * 2
    assert nrows >= 1024 and d["xvec"] == 0
    if b >= d["nt_mib"] * MIB:
        rows, u, nt = d["rows"], d["unroll"], True
    elif 64 * MIB < b < 280 * MIB:
        rows, u, nt = 2, d["unroll_mid"], False
    else:
        rows, u, nt = d["rows"], d["unroll"], False
    ng = nrows // rows + nrows % rows
    grid = min(ng, d["grid"])
    return rows, u, nt, (nrows // rows, nrows % rows), grid, (ng - 1) // grid + 1


HALF_GROUPED = {
    # 32 MiB: 8 rows per group, 512 groups + 1 remainder row on 512 workgroups:
    # workgroup 0 holds group 0 and the remainder row, and starts on the
    # remainder row (the 1-row instantiation folds the stats) where the walk
    # is reversed, k = 1, on group 0 (the 8-row instantiation) at k = 2
    "rows8": ((4097, 4104, 3), (8, 2, False, (512, 1), 512, 2)),
    # 64.1 MiB: the cached 2-row shape, one chunk in flight, 5 groups per workgroup
    "rows2": ((4099, 8200, 101), (2, 1, False, (2049, 1), 512, 5)),
    # 513 MiB: non-temporal, 8 rows per group
    "nontemporal": ((16389, 16400, 5), (8, 2, True, (2048, 5), 512, 5)),
}


def half_grouped(orc, storage, sem, name, k):
    (nrows, n, row0), shape = HALF_GROUPED[name]
    assert half_grouped_shape(nrows, n) == shape, (name, half_desc())

    def setup(x):
        assert vector_path(x)
    big = nrows * n * 2 >= 256 * MIB
    sweep(orc, F32, sem, n, half_launch, full_v=True, launch_k=k, w=HALF_W, block=(nrows, row0),
          mat=half_block_of_integers(storage) if big else half_block(storage), setup=setup)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("sem", SEM_PARAMS)
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("name", ["rows8", "rows2"])
def test_mfree_half_round_grouped(orc, name, storage, sem, k):
    """k_mfree_half's grouped launches (from 1024 rows): every workgroup folds
    the stats in its first group and scales its own slice of v_cur with its
    own m; the walk is reversed on odd k."""
    half_grouped(orc, storage, sem, name, k)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("sem", SEM_PARAMS)
def test_mfree_half_round_nontemporal(orc, sem, k):
    """The same in the non-temporal shape (a 513 MiB block, bf16)."""
    half_grouped(orc, torch.bfloat16, sem, "nontemporal", k)


# ---------------------------------------------------------------------------
# the grouped launches of k_mfree and k_round (from 1024 rows)
# ---------------------------------------------------------------------------
GROUPED = (2049, 3)          # 2049 = 4 * 512 + 1 = 2 * 1024 + 1: a remainder row either way
GROUPED_PARAMS = [pytest.param(dt, sem, id=f"{np.dtype(dt).name}-{'sycl' if sem == 0 else 'mainpy'}")
                  for dt in (np.float64, np.float32) for sem in SEMS]


def policy(L, dt, nrows, ncols, form):
    """st_launch_policy_query of the library `L` (the tuning build answers
    with its own, overridden, table)."""
    import ctypes
    out = _lib.st_launch_policy()
    _lib.check(L.st_launch_policy_query(1 if dt == np.float64 else 0, nrows, ncols, form, 0,
                                        ctypes.byref(out)), "st_launch_policy_query", L)
    return _lib.KERNEL_NAMES[out.kernel], out.rows, bool(out.load_nt), out.grid


def mfree_launch_through(L):
    """dev.mfree_round through the library `L`."""
    def launch(x, j, ci, _):
        sfx = "f64" if x.c.dt == np.float64 else "f32"
        s, v = x.S[ci], x.V[j]
        assert x.mat.is_contiguous() and s.numel() >= x.n and v.numel() >= x.n
        assert x.s_next.numel() >= x.nrows and x.row0 + x.nrows <= x.n
        _lib.check(getattr(L, f"st_mfree_round_{sfx}")(
            x.mat.data_ptr(), s.data_ptr(), x.s_next.data_ptr(), x.v0.data_ptr(), v.data_ptr(),
            x.nrows, x.n, x.row0, x.eps[ci], x.k, MAX_ITR, x.sem, x.ST[j].data_ptr(),
            torch.cuda.current_stream(DEV).cuda_stream), "mfree_round", L)
    return launch


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", [2056, 2059])
@pytest.mark.parametrize("dt,sem", GROUPED_PARAMS)
def test_mfree_round_grouped(orc, dt, sem, n, k):
    """k_mfree on 2049 rows: 4 rows per group, 512 groups + 1 remainder row on
    512 workgroups.  k = 1 (reversed walk): workgroup 0 folds the stats in the
    1-row remainder instantiation; k = 2: in the 4-row one.  n = 2059: the
    element-wide path."""
    nrows, row0 = GROUPED
    L = _lib.load()
    # (the query takes whole 16-byte chunks per row; the table reads rows and bytes)
    assert policy(L, dt, nrows, 2056, _lib.ST_FORM_MFREE) == ("k_mfree", 4, False, 512)
    assert policy(L, dt, nrows, 2064, _lib.ST_FORM_MFREE) == ("k_mfree", 4, False, 512)
    sweep(orc, dt, sem, n, mfree_launch_through(L), full_v=True, launch_k=k, block=GROUPED,
          mat=device_block)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("shape,rows,nt", [(1, 2, False), (2, 4, False), (3, 4, True)],
                         ids=["cached2", "cached4", "nontemporal4"])
@pytest.mark.parametrize("dt,sem", GROUPED_PARAMS)
def test_mfree_round_grouped_shapes(orc, dt, sem, shape, rows, nt, k):
    """The other instantiations of k_mfree - 2 rows per group (1024 groups +
    1 row: 3 groups per workgroup), and 4 rows with non-temporal loads, which
    the table takes from 512 MiB - on the same 2049 x 2056 block, through the
    tuning build (st_set_mfree_shape; its kernels are the product's)."""
    nrows, row0 = GROUPED
    n = 2056
    L = _lib.load_tuning()
    saved = L.st_set_mfree_shape(0)
    try:
        assert L.st_set_mfree_shape(shape) >= 0
        assert policy(L, dt, nrows, n, _lib.ST_FORM_MFREE) == ("k_mfree", rows, nt, 512)
        sweep(orc, dt, sem, n, mfree_launch_through(L), full_v=True, launch_k=k, block=GROUPED,
              mat=device_block)
    finally:
        L.st_set_mfree_shape(saved)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("dt,sem", GROUPED_PARAMS)
def test_fused_round_grouped(orc, dt, sem, k):
    """k_round on 2049 x 2056: 2 rows per group, 1024 groups + 1 remainder row
    (fp64, 32.1 MiB: on 512 workgroups; fp32 on 1024), forward at k = 2 and
    reversed at k = 3."""
    nrows, row0 = GROUPED
    n = 2056
    kernel, rows, nt, grid = policy(_lib.load(), dt, nrows, n, _lib.ST_FORM_ROUND)
    assert (kernel, rows, nt) == ("k_round", 2, False)
    assert grid == (512 if dt == np.float64 else 1024)

    def launch(x, j, ci, _):
        dev.fused_round(x.mat, x.S[ci], x.s_next, x.V[j], x.ST[j], row0=row0, eps=x.eps[ci],
                        k=k, max_itr=MAX_ITR, semantics=sem)
    sweep(orc, dt, sem, n, launch, rk=k, block=GROUPED, mat=device_block)


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


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1032, 2056])
def test_solve_matrix_free_loop_sizes(solver, orc, dt, n, sem):
    """The same sizes through the matrix-free loop: K0 and k_mfree at a
    grouped launch shape (from 1024 rows), as the solve launches them."""
    assert _lib.launch_policy("f64" if dt == np.float64 else "f32", n, n,
                              _lib.ST_FORM_MFREE)["rows"] == 4
    solve_each(solver, orc, dt, sem, n, matrix_free=True)


@pytest.mark.parametrize("n", [9, 257, 1032, 2056])
@pytest.mark.parametrize("sem", SEM_PARAMS)
@pytest.mark.parametrize("storage,bits", [pytest.param(torch.float16, 11, id="f16"),
                                          pytest.param(torch.bfloat16, 8, id="bf16")])
def test_solve_half(solver, orc, storage, bits, sem, n):
    """solve_half (k_rowsum_half, then k_mfree_half as the solve launches it;
    8 rows per group from 1024 rows).  No 16-bit format holds these s, so row
    r of the matrix holds the three pieces of 1024 * s[r] (sv.split_rows, each
    exact in the storage format) at columns r, r + 1, r + 2 (mod n) and zeros:
    K0's row sum is 1024 * s[r] bit for bit in any order, and with eps scaled
    by the same power of two every comparison, s / m and the stop decision
    are those of s."""
    cyclic = sem == _lib.ST_SEM_SYCL
    c = cases(orc, n, F32, cyclic, w=HALF_W)
    ncase = len(c.tags)
    P = np.stack(sv.split_rows(c.S, bits), axis=1)              # (case, 3, n)
    Hd = dev.narrow(torch.from_numpy(P).to(DEV), storage)       # st_narrow_f32
    assert same(Hd.cpu().float().numpy(), P).all()              # the narrowing is exact
    h = torch.zeros((n, n), dtype=storage, device=DEV)
    # piece d of row r at column (r + d) % n: the diagonals 0, 1, 2 and their
    # wrapped ends (n - 1, 0), (n - 2, 0), (n - 1, 1); the same 3 n slots each time
    slots = [(h.diagonal(0), 0, 0, n), (h.diagonal(1), 1, 0, n - 1),
             (h.diagonal(1 - n), 1, n - 1, n), (h.diagonal(2), 2, 0, n - 2),
             (h.diagonal(2 - n), 2, n - 2, n)]
    assert sum(view.numel() for view, *_ in slots) == 3 * n
    lam, its, conv, vs = [], [], [], []
    for ci in range(ncase):
        for view, d, lo, hi in slots:
            view.copy_(Hd[ci, d, lo:hi])
        l, v, it, st = solver.solve_half(h, eps=1024.0 * float(c.eps[ci]), max_itr=1,
                                         semantics=sem)
        lam.append(l), its.append(it), conv.append(st["converged"]), vs.append(v)
    last = h.cpu().float().numpy()                              # the last case's matrix
    r = np.arange(n)
    for d in range(3):
        assert same(last[r, (r + d) % n], P[ncase - 1, d]).all()
        last[r, (r + d) % n] = 0
    assert not last.any()                                       # zeros elsewhere
    jobs = [(ci, None) for ci in range(ncase)]
    stop, iters, v = expect_solve(c, np.arange(ncase))
    check("converged", np.array(conv), stop, jobs, c)
    check("iterations", np.array(its), iters, jobs, c)
    check("lambda", np.array(lam, dtype=np.float64),
          (np.float32(1024) * c.S[:, 0]).astype(np.float64), jobs, c)
    torch.cuda.synchronize()
    check("v", torch.stack(vs).cpu().numpy(), v, jobs, c)


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


VDIMS = {np.float64: [9, 63, 64, 127, 128], np.float32: [9, 63, 64, 127, 128, 255, 256]}


@pytest.mark.parametrize("misaligned", [False, True], ids=["aligned", "off1"])
@pytest.mark.parametrize("sem", SEM_PARAMS)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_solve_vbatched(solver, orc, dt, sem, misaligned):
    """k_solve_vbatched: diagonal matrices of every dim in ONE call per eps
    (each workgroup-shape class one launch, dims interleaved), every entry
    with a stop decision of its own; once on 16-byte aligned bases and once
    with every base one element past a 16-byte boundary (the layout of
    test_gpu_vbatched.test_misaligned_base_changes_no_bit), where the kernel
    takes its element-wide loads."""
    cyclic = sem == _lib.ST_SEM_SYCL
    item = np.dtype(dt).itemsize
    per16 = 16 // item
    cs = {n: cases(orc, n, dt, cyclic) for n in VDIMS[dt]}
    Sd = {n: torch.tensor(c.S, device=DEV) for n, c in cs.items()}
    for e in np.unique(np.concatenate([c.eps for c in cs.values()])):
        # interleave the dims: entry order by case index, then dim
        entries = sorted((int(ci), n) for n, c in cs.items() for ci in np.nonzero(c.eps == e)[0])
        offs, total = [], int(misaligned)
        for _, n in entries:
            offs.append(total)
            total += -(-n * n // per16) * per16 + per16        # keeps every base's alignment
        buf = torch.zeros(total, dtype=TD[dt], device=DEV)
        assert buf.data_ptr() % 16 == 0
        work = [buf[o:o + n * n].view(n, n) for o, (_, n) in zip(offs, entries)]
        for w_, (ci, n) in zip(work, entries):
            assert w_.data_ptr() % 16 == (item if misaligned else 0) and w_.is_contiguous()
            w_.diagonal().copy_(Sd[n][ci])
        lam, vs, it, st = solver.solve_vbatched(work, inplace=True, eps=float(e), max_itr=1,
                                                semantics=sem)
        assert st["converged"] == 0 and st["rounds"] == 1
        torch.cuda.synchronize()
        conv, lam, it = st["converged_each"], lam.numpy(), it.numpy()
        for n, c in cs.items():
            sel = [b for b, (_, m) in enumerate(entries) if m == n]
            idx = np.array([entries[b][0] for b in sel])
            jobs = [(int(ci), None) for ci in idx]
            stop, iters, vexp = expect_solve(c, idx)
            assert 0 < stop.sum() < len(idx)                   # both kinds at every dim
            check("converged_each", conv[sel], stop, jobs, c)
            check("iterations", it[sel], iters, jobs, c)
            check("lambda", lam[sel].astype(np.float64), c.S[idx, 0].astype(np.float64), jobs, c)
            assert all(vs[b].shape == (n,) for b in sel)
            check("v", torch.stack([vs[b] for b in sel]).cpu().numpy(), vexp, jobs, c)


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
