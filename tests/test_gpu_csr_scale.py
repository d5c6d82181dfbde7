"""GPU: the CSR create-time passes and the transposition past their first trip.

Every kernel below is capped at a fixed number of workgroups and walks a
longer array in grid-stride trips, or scans a table in spans of several items
per lane.  The other CSR tests stay inside the first trip and at one item per
lane; these sizes do not.  The caps are read from the shape descriptors and
every test asserts that its size crosses the one it is about.

A  one matrix of CHECK + 256 + 37 rows (csr_scale_cases.big): plan, K0 and a
   round against the vectorised model, the column check and the row-pointer
   check naming entries and rows beyond the first trip
B  the transposition: k_tr_scan and k_tr_top at 2 and 3 items per lane, both
   grid caps, stability across spans, four digit passes, the empty-column
   refusal beyond block 255, the left solve
C  terms, multi and product on A's matrix: validation beyond the first trip,
   pack and collect, the identities with u = 0 and an identity factor
D  a batch of 664 947 stacked rows: collect, the seam inside one matrix, the
   column check's later trips

Comparisons are tobytes() equality.  A large array is built and uploaded once
per module; a test changes single elements on the device and puts them back.
A test that expects a refusal only creates the object.
"""
import contextlib
import functools
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import csr_order_model as om  # noqa: E402
import csr_scale_cases as sc  # noqa: E402
import stats_vectors as sv  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from test_gpu_csr import expect_state, run_round  # noqa: E402
from test_gpu_csr_batch import expect_state as batch_expect_state  # noqa: E402
from test_gpu_csr_batch import host_message, one_pair  # noqa: E402

DEV = "cuda:0"
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
SEMS = [pytest.param(_lib.ST_SEM_SYCL, id="sycl"), pytest.param(_lib.ST_SEM_MAINPY, id="mainpy")]
BLOCK = 256

CSR = om.shape_desc()
PREP = CSR["prep_grid"][0] * BLOCK            # elements of one trip of the vector pass
CHECK = CSR["check_grid"][0] * BLOCK          # entries / rows of one trip of a create-time pass
TR = _lib.csr_transpose_shape()
D, TILE, COLB = 1 << TR["digit_bits"], TR["tile"], TR["col_block"]
TR_TRIP = TR["grid"] * BLOCK                  # entries of one trip of k_tr_count / k_tr_gather


def _caps(shape):
    assert shape["check_grid"] * BLOCK == CHECK
    return shape


TERMS, MULTI, PRODUCT = (_caps(_lib.csr_terms_shape()), _caps(_lib.csr_multi_shape()),
                         _caps(_lib.csr_product_shape()))
BATCH_DESC = _lib.load().st_csr_batch_shape_desc().decode()
_m = re.search(r"at most (\d+) per matrix.*collect_grid=(\d+); check: (\d+) lanes per row, "
               r"at most (\d+) workgroups", BATCH_DESC)
assert _m, BATCH_DESC
BATCH_PREP = int(_m.group(1)) * BLOCK                  # elements of one trip of k_csrb_prep
COLLECT = int(_m.group(2)) * BLOCK                     # stacked rows of one trip of k_csrb_collect
CHECK_ROWS = int(_m.group(4)) * (BLOCK // int(_m.group(3)))   # and of k_csrb_check_col

N_A = CHECK + BLOCK + 37
HEAVY_A = (0, PREP - 1, PREP, CHECK - 1, CHECK, N_A - 1)
MAX_ITR = 3


def tdt(dt):
    return torch.float64 if np.dtype(dt) == np.float64 else torch.float32


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(DEV)


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def same(got, want):
    return all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def arrays(m):
    return m.crow.cpu().numpy(), m.col.cpu().numpy(), m.values.cpu().numpy()


def numpy_plan(indptr):
    """The plan by its definition: the rows sorted by class, their order kept
    within a class (an empty row is of class 0)."""
    nnz_max, _ = om.class_table()
    cls = np.searchsorted(np.array(nnz_max[:-1], np.int64), np.diff(indptr),
                          side="left").astype(np.uint8)
    first = np.zeros(len(nnz_max) + 1, dtype=np.uint32)
    np.cumsum(np.bincount(cls, minlength=len(nnz_max)), out=first[1:])
    return np.argsort(cls, kind="stable").astype(np.uint32), first


@contextlib.contextmanager
def poked(t, changes):
    """Single elements of a device tensor changed for the block: {index: value}."""
    idx = torch.tensor(sorted(changes), dtype=torch.int64, device=t.device)
    old = t[idx].clone()
    try:
        for i in sorted(changes):
            t[i] = changes[i]
        yield
    finally:
        t[idx] = old


def refused(make, *expect):
    """make() must raise EigenValueError holding every text of expect; if it
    wrongly returns an object, that is closed and the test fails."""
    obj = None
    try:
        obj = make()
    except _lib.EigenValueError as e:
        for text in expect:
            assert text in str(e), (text, str(e))
        return str(e)
    obj.close()
    pytest.fail(f"creation wrongly succeeded where {expect} was expected")


def row_of(ip, e):
    return int(np.searchsorted(ip, e, side="right")) - 1


# ---------------------------------------------------------------------------
# A's matrix: host arrays once per dtype, device arrays once per module
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_a(dtname):
    ip, ix, da = sc.big(N_A, 41, np.dtype(dtname), sc.heavy_at(HEAVY_A))
    for a in (ip, ix, da):
        a.setflags(write=False)
    return ip, ix, da


@functools.lru_cache(maxsize=None)
def host_a_transposed(dtname):
    return dev.csr_transpose_host(*host_a(dtname))


_DEV_A = {}


def dev_a(dt):
    """(d_ip, d_ix, d_da) of A's matrix; the structure is one pair of tensors
    for both dtypes."""
    name = np.dtype(dt).name
    if "ip" not in _DEV_A:
        ip, ix, _ = host_a(name)
        _DEV_A["ip"], _DEV_A["ix"] = up(ip), up(ix)
    if name not in _DEV_A:
        _DEV_A[name] = up(host_a(name)[2])
    return _DEV_A["ip"], _DEV_A["ix"], _DEV_A[name]


def matrix_a(solver, dt, **kw):
    d_ip, d_ix, d_da = dev_a(dt)
    return dev.CsrMatrix(d_ip, d_ix, d_da, N_A, solver=solver, **kw)


def test_the_descriptors_hold_the_caps_and_the_sizes_cross_them():
    assert CSR["check_grid"] == (8192,) and CSR["prep_grid"] == (2048,) and TR["grid"] == 8192
    assert (BATCH_PREP, COLLECT, CHECK_ROWS) == (2048 * BLOCK, 2048 * BLOCK, 8192 * 16)
    ip, ix, _ = host_a("float32")
    assert ip.tobytes() == host_a("float64")[0].tobytes()
    assert ix.tobytes() == host_a("float64")[1].tobytes()
    lens = np.diff(ip)
    assert [int(lens[r]) for r in HEAVY_A] == [17, 129, 2049, 17, 129, 2049]
    assert N_A > CHECK + BLOCK and len(ix) > CHECK + 2 * BLOCK


# ---------------------------------------------------------------------------
# A1, A2. plan, K0 and one round
# ---------------------------------------------------------------------------
def test_plan_of_two_million_rows(solver):
    ip = host_a("float32")[0]
    assert -(-N_A // BLOCK) > 2 * BLOCK            # k_csr_scan: more than 2 blocks per lane
    m = matrix_a(solver, np.float32)
    order, first = m.plan()
    m.close()
    h_order, h_first, used = _lib.csr_plan(ip)
    assert used == 4
    assert order.tobytes() == h_order.tobytes() and first.tobytes() == h_first.tobytes()
    n_order, n_first = numpy_plan(ip)
    assert order.tobytes() == n_order.tobytes() and first.tobytes() == n_first.tobytes()


@pytest.mark.parametrize("dt", DTYPES)
def test_rowsum_and_round_against_the_vectorised_model(solver, dt):
    ip, ix, da = host_a(np.dtype(dt).name)
    assert N_A > CHECK > PREP and all(r in HEAVY_A for r in (PREP, CHECK, N_A - 1))
    m = matrix_a(solver, dt)
    s0 = dev.csr_rowsum(m).cpu().numpy()
    assert s0.tobytes() == sc.rowsum_model(ip, da).tobytes()
    rng = np.random.default_rng(77)
    s_prev = (0.5 + rng.random(N_A)).astype(dt)
    v_prev = (0.5 + rng.random(N_A)).astype(dt)
    s_next, v_cur, x, state = run_round(m, s_prev, v_prev, k=1, eps=1e-3, max_itr=1000)
    m.close()
    want = sc.round_model(ip, ix, da, s_prev, v_prev, sv.find_max(s_prev))
    assert x.tobytes() == want["x"].tobytes()
    bad = np.flatnonzero(s_next != want["s_next"])
    assert s_next.tobytes() == want["s_next"].tobytes(), (len(bad), bad[:8])
    assert v_cur.tobytes() == want["v_cur"].tobytes()
    assert state.tobytes() == expect_state(s_prev, 1e-3, _lib.ST_SEM_SYCL, 1, 1000)


# ---------------------------------------------------------------------------
# A3. the column check: k_csr_check_col's second trip
# ---------------------------------------------------------------------------
def col_message(ip, e, c):
    return f"column index {c} of entry {e} (row {row_of(ip, e)}) is outside [0, {N_A})"


@pytest.mark.parametrize("dt", DTYPES)
def test_column_check_names_the_entry_beyond_the_first_trip(solver, dt):
    ip, ix, _ = host_a(np.dtype(dt).name)
    d_ip, d_ix, d_da = dev_a(dt)
    nnz = len(ix)
    assert nnz > CHECK + 2 * BLOCK                 # entries CHECK .. are the second trip's
    at = [0, 255, 256, CHECK - 1, CHECK, CHECK + 255, CHECK + 256, nnz - 1]
    values = [N_A, -1, 2**31 - 1]
    for i, e in enumerate(at):
        c = values[i % 3]
        with poked(d_ix, {e: c}):
            refused(lambda: matrix_a(solver, dt), col_message(ip, e, c))
    # every bad value in the second trip as well
    for e, c in ((CHECK, N_A), (CHECK + 255, -1), (nnz - 1, 2**31 - 1), (CHECK + 256, N_A)):
        with poked(d_ix, {e: c}):
            refused(lambda: matrix_a(solver, dt), col_message(ip, e, c))
    # two offenders: the lower entry, whichever trip holds it
    with poked(d_ix, {CHECK - 7: -1, CHECK + 300: N_A}):
        refused(lambda: matrix_a(solver, dt), col_message(ip, CHECK - 7, -1))
    with poked(d_ix, {CHECK + 300: N_A + 5, nnz - 1: -1}):
        refused(lambda: matrix_a(solver, dt), col_message(ip, CHECK + 300, N_A + 5))
    with poked(d_ix, {2 * CHECK + 11: -3, CHECK + 12: N_A}):     # third trip against second
        assert nnz > 2 * CHECK + 11
        refused(lambda: matrix_a(solver, dt), col_message(ip, CHECK + 12, N_A))
    # everything was put back: the arrays are the host's and the matrix is good
    assert d_ix.cpu().numpy().tobytes() == ix.tobytes()
    matrix_a(solver, dt).close()


# ---------------------------------------------------------------------------
# A4. the row-pointer check far from block 0
# ---------------------------------------------------------------------------
PTR_ROWS = [255, 256, 65535, 65536, CHECK - 1, CHECK, N_A - 1]


@pytest.mark.parametrize("dt", DTYPES)
def test_row_pointer_check_names_rows_far_from_block_0(solver, dt):
    ip, ix, _ = host_a(np.dtype(dt).name)
    d_ip, d_ix, d_da = dev_a(dt)
    nnz = len(ix)
    assert N_A - 1 > CHECK > 65536 > BLOCK
    for r in PTR_ROWS:
        a = int(ip[r])
        with poked(d_ip, {r + 1: a}):
            refused(lambda: matrix_a(solver, dt),
                    f"csr: row {r} is empty (row_ptr[{r}] = row_ptr[{r + 1}] = {a})")
        with poked(d_ip, {r + 1: a - 1}):
            refused(lambda: matrix_a(solver, dt),
                    f"csr: row_ptr decreases at row {r} (row_ptr[{r}] = {a}, "
                    f"row_ptr[{r + 1}] = {a - 1})")
    # row_ptr[n] against a shortened col / vals: views of the same tensors
    refused(lambda: dev.CsrMatrix(d_ip, d_ix[:-1], d_da[:-1], N_A, solver=solver),
            f"csr: row_ptr[n] must be nnz = {nnz - 1}, got {nnz} (row {N_A - 1})")
    # two bad rows: the lower one
    for lo, hi in ((65536, CHECK), (CHECK, N_A - 1), (CHECK - 1, CHECK + BLOCK)):
        with poked(d_ip, {lo + 1: int(ip[lo]), hi + 1: int(ip[hi]) - 1}):
            refused(lambda: matrix_a(solver, dt), f"csr: row {lo} is empty")
        with poked(d_ip, {lo + 1: int(ip[lo]) - 1, hi + 1: int(ip[hi])}):
            refused(lambda: matrix_a(solver, dt), f"csr: row_ptr decreases at row {lo} ")
    # row_ptr is judged first: with it broken the columns are not read
    with poked(d_ip, {CHECK + 1: int(ip[CHECK])}), poked(d_ix, {0: N_A, nnz - 1: -1}):
        refused(lambda: matrix_a(solver, dt), f"csr: row {CHECK} is empty")
    assert d_ip.cpu().numpy().tobytes() == ip.tobytes()
    assert d_ix.cpu().numpy().tobytes() == ix.tobytes()
    matrix_a(solver, dt).close()


# ---------------------------------------------------------------------------
# B. the transposition
# ---------------------------------------------------------------------------
def check_transposition(solver, ip, ix, da, allow_empty=False, m=None):
    """m.transpose() against the host twin and, independently, numpy's stable
    argsort; its plan against the host plan.  Returns the transposed arrays."""
    n = len(ip) - 1
    own = m is None
    if own:
        m = dev.CsrMatrix(up(ip), up(ix), up(da), n, solver=solver, allow_empty_rows=allow_empty)
    t = m.transpose(solver, allow_empty=allow_empty)
    got = arrays(t)
    order, first = t.plan()
    assert (t.n, t.nnz, t.dtype) == (m.n, m.nnz, m.dtype)
    t.close()
    if own:
        m.close()
    assert same(got, dev.csr_transpose_host(ip, ix, da, allow_empty=allow_empty))
    assert same(got, sc.transpose_argsort(ip, ix, da))
    o, f = numpy_plan(got[0])
    assert order.tobytes() == o.tobytes() and first.tobytes() == f.tobytes()
    if not allow_empty:
        o, f, _ = _lib.csr_plan(got[0])
        assert order.tobytes() == o.tobytes() and first.tobytes() == f.tobytes()
    return got


def perm_plus(lens, seed, dt, hi_col=None):
    """Rows of lens[r] >= 1 entries: the first from a permutation of 0 .. n - 1
    (no empty column), the others from integers(0, hi_col or n); values in
    (0, 1]."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    assert lens.min() >= 1
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=ip[1:])
    nnz = int(ip[-1])
    ix = rng.integers(0, n if hi_col is None else hi_col, size=nnz, dtype=np.int32)
    ix[ip[:-1]] = rng.permutation(n).astype(np.int32)
    return ip, ix, (1.0 - rng.random(nnz)).astype(dt)


def spread(n, nnz, seed, dt, hi_col=None):
    """nnz entries over n rows as evenly as they go."""
    lens = np.full(n, nnz // n, dtype=np.int64)
    lens[:nnz % n] += 1
    return perm_plus(lens, seed, dt, hi_col)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("ntiles,per", [(256, 1), (257, 2), (512, 2), (513, 3)])
def test_scan_of_the_tile_table_with_several_tiles_per_lane(solver, ntiles, per, dt):
    """k_tr_scan: lane t takes tiles t * per .. t * per + per - 1; at 257 tiles
    only lanes 0 .. 128 hold any."""
    n = 1000
    nnz = (ntiles - 1) * TILE + 37
    assert -(-nnz // TILE) == ntiles and -(-ntiles // BLOCK) == per
    check_transposition(solver, *spread(n, nnz, ntiles, dt))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n,per", [(256 * COLB, 1), (256 * COLB + 1, 2), (512 * COLB + 1, 3)])
def test_scan_of_the_column_blocks_with_several_blocks_per_lane(solver, n, per, dt):
    """k_tr_top over ceil(n / col_block) block sums; 1 - 2 entries per row."""
    blocks = -(-n // COLB)
    assert -(-blocks // BLOCK) == per
    ip, ix, da = perm_plus(1 + np.arange(n, dtype=np.int64) % 2, n, dt)
    assert np.bincount(ix, minlength=n).min() >= 1
    check_transposition(solver, ip, ix, da)


@pytest.mark.parametrize("dt", DTYPES)
def test_both_grid_caps_and_stability_across_the_spans_of_the_scan(solver, dt):
    """nnz beyond one trip of k_tr_count / k_tr_gather and of the column check;
    every column's ~512 entries lie all over the array.  Column n - 1 holds
    only the entries placed here, in tiles 0, 256, 257, the two tiles on
    either side of a span boundary of k_tr_scan, and the last tile - distinct
    values, whose order in T(A) is their storage order."""
    n = 4096
    nnz = CHECK + TILE + 37
    ntiles = -(-nnz // TILE)
    per = -(-ntiles // BLOCK)
    assert nnz > CHECK and nnz > TR_TRIP and per >= 2
    ip, ix, da = spread(n, nnz, 5, dt, hi_col=n - 1)
    ix[ix == n - 1] = 0                            # the permutation's one entry of column n - 1
    tiles = [0, 256, 257, 100 * per - 1, 100 * per, ntiles - 1]
    assert tiles == sorted(tiles) and 257 < 100 * per - 1 and 100 * per < ntiles - 1
    at = [t * TILE + 5 + 2 * i for i, t in enumerate(tiles[:-1])] + [nnz - 3]
    assert [e // TILE for e in at] == tiles
    marks = (np.arange(1, len(at) + 1) / 8.0).astype(dt)
    ix[at], da[at] = n - 1, marks
    counts = np.bincount(ix, minlength=n)
    assert counts[n - 1] == len(at) and counts.min() >= 1 and counts[:n - 1].min() > 300
    tp, ti, tv = check_transposition(solver, ip, ix, da)
    lo, hi = int(tp[n - 1]), int(tp[n])
    assert tv[lo:hi].tobytes() == marks.tobytes()
    assert ti[lo:hi].tolist() == [row_of(ip, e) for e in at]


@pytest.mark.parametrize("dt", DTYPES)
def test_transposition_of_the_matrix_of_two_million_rows(solver, dt):
    name = np.dtype(dt).name
    ip, ix, da = host_a(name)
    assert len(ix) > TR_TRIP and -(-len(ix) // TILE) > BLOCK and -(-N_A // COLB) > BLOCK
    m = matrix_a(solver, dt)
    got = check_transposition(solver, ip, ix, da, m=m)
    m.close()
    assert same(got, host_a_transposed(name))


def four_pass_case(n, seed=3):
    """nnz = 2 * 256 * tile + 37 entries on rows spread over 0 .. n - 1 (most
    rows are empty), columns over the whole range: each of the three low
    digits takes more than 200 values, the top digit every value it can (0,
    and 1 for column 2^24 when n - 1 = 2^24).  Column n - 1 and column 0 occur
    at least 3 times each, in different tiles."""
    nnz = 2 * BLOCK * TILE + 37
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.integers(0, n, size=nnz))
    rows[0], rows[-1] = 0, n - 1
    ip = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ip[1:])
    ix = rng.integers(0, n, size=nnz, dtype=np.int32)
    for i, t in enumerate((1, 300, 511)):
        ix[t * TILE + 11 + i] = n - 1
        ix[t * TILE + 900 + i] = 0
    da = (1.0 - rng.random(nnz)).astype(np.float32)
    return ip, ix, da


@pytest.mark.parametrize("n,passes", [(D ** 3 + 1, 4), (D ** 3, 3)])
def test_four_digit_passes_and_the_last_size_with_three(solver, n, passes):
    """With 4 passes, pass 2 writes the keys buffer pass 0 wrote while it reads
    the other, and the index buffers alternate twice."""
    bits = int(n - 1).bit_length()
    assert -(-bits // TR["digit_bits"]) == passes and (n - 1 >= D ** 3) == (passes == 4)
    ip, ix, da = four_pass_case(n)
    nnz = len(ix)
    assert -(-nnz // TILE) > 2 * BLOCK
    for p in range(3):
        assert len(np.unique((ix >> (8 * p)) & 255)) >= 200
    assert sorted(np.unique(ix >> 24).tolist()) == ([0, 1] if passes == 4 else [0])
    for c in (0, n - 1):
        assert len({int(e) // TILE for e in np.flatnonzero(ix == c)}) >= 3
    got = check_transposition(solver, ip, ix, da, allow_empty=True)
    assert int(got[0][-1]) == nnz


@pytest.mark.parametrize("dt", DTYPES)
def test_an_empty_column_beyond_block_255_is_named(solver, dt):
    """k_tr_colsum's atomicMin over more than 256 column blocks, fed by a
    count whose entries lie in later trips of k_tr_count."""
    ip, ix, _ = host_a(np.dtype(dt).name)
    d_ip, d_ix, d_da = dev_a(dt)
    edge = COLB * BLOCK
    assert N_A - 1 > edge and len(ix) > TR_TRIP

    def emptied(*cols):
        ch = {}
        for c in cols:
            for e in np.flatnonzero(ix == c):
                ch[int(e)] = 0
        assert ch
        return ch

    def transposed():
        m = matrix_a(solver, dt)
        try:
            return m.transpose(solver)
        finally:
            assert m._t is None
            m.close()

    for c in (edge - 1, edge, N_A - 1):
        with poked(d_ix, emptied(c)):
            refused(transposed, f"column {c} has no entry")
    with poked(d_ix, emptied(edge, N_A - 1)):
        refused(transposed, f"column {edge} has no entry")
    with poked(d_ix, emptied(N_A - 1, edge - 1)):
        refused(transposed, f"column {edge - 1} has no entry")
    assert d_ix.cpu().numpy().tobytes() == ix.tobytes()


def result(r):
    lam, v, it, st = r
    return lam, v.cpu().numpy().tobytes(), it, st["rounds"], st["converged"]


@pytest.mark.parametrize("dt", DTYPES)
def test_left_solve_of_two_million_rows(solver, dt):
    name = np.dtype(dt).name
    assert len(host_a(name)[1]) > TR_TRIP
    m = matrix_a(solver, dt)
    got = result(solver.solve_csr(m, left=True, max_itr=MAX_ITR))
    m.close()
    tp, ti, tv = host_a_transposed(name)
    ref = dev.CsrMatrix(up(tp), up(ti), up(tv), N_A, solver=solver)
    want = result(solver.solve_csr(ref, max_itr=MAX_ITR))
    ref.close()
    assert got == want and got[2:] == (MAX_ITR, MAX_ITR, 0)


# ---------------------------------------------------------------------------
# C. terms, multi and product on A's matrix
# ---------------------------------------------------------------------------
_VEC = {}


def term_vectors(dt, K):
    """Device [K, n]: u = 1e-7 (0.5 + random), w = 0.5 + random (teleport-like);
    built once per (dtype, K) and put back by every test."""
    key = (np.dtype(dt).name, K)
    if key not in _VEC:
        rng = np.random.default_rng(1000 + K)
        u = (1e-7 * (0.5 + rng.random((K, N_A)))).astype(dt)
        w = (0.5 + rng.random((K, N_A))).astype(dt)
        _VEC[key] = (up(u), up(w))
    return _VEC[key]


FAR = [CHECK - 1, CHECK, N_A - 1]


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("dt", DTYPES)
def test_terms_validation_beyond_the_first_trip(solver, dt, K):
    """k_csr_terms_check: one lane per index, capped as the column check is."""
    assert N_A > CHECK + BLOCK and TERMS["check_grid"] * BLOCK == CHECK
    m = matrix_a(solver, dt)
    u, w = term_vectors(dt, K)

    def make():
        return dev.CsrTerms(m, list(u), list(w), solver=solver)

    for j in sorted({0, K - 1}):
        for i in FAR:
            with poked(u[j], {i: -1.0}):
                refused(make, f"csr terms: u_{j}[{i}] = -1:")
            with poked(w[j], {i: float("nan")}):
                refused(make, f"csr terms: w_{j}[{i}] = nan:")
            with poked(u[j], {i: float("inf")}):
                refused(make, f"csr terms: u_{j}[{i}] = inf:")
    # two offenders: the key is ((2 j + which) << 32 | i), u before w
    j = K - 1
    with poked(u[j], {CHECK + 5: -1.0, N_A - 1: -2.0}):
        refused(make, f"u_{j}[{CHECK + 5}] = -1:")
    with poked(u[j], {CHECK + 5: -1.0}), poked(w[j], {CHECK - 1: -2.0}):
        refused(make, f"u_{j}[{CHECK + 5}] = -1:")                # u_j before w_j at a lower i
    with poked(w[0], {N_A - 1: -2.0}), poked(w[j], {CHECK: -1.0}):
        refused(make, f"w_0[{N_A - 1}] = -2:" if K > 1 else f"w_0[{CHECK}] = -1:")
    if K > 1:
        with poked(u[j], {CHECK - 1: -1.0}), poked(w[0], {N_A - 1: -2.0}):
            refused(make, f"w_0[{N_A - 1}] = -2:")                # term 0 before term K - 1
    make().close()
    m.close()


def emptied_rows(ip, rows):
    """{index: value} for row_ptr that leaves these rows without an entry: row
    q < n - 1 hands its entries to row q + 1, row n - 1 to row n - 2."""
    n = len(ip) - 1
    new = ip.copy()
    for q in sorted(rows):
        if q == n - 1:
            assert n - 2 not in rows
            new[q] = new[n]
        else:
            new[q + 1] = new[q]
    idx = np.flatnonzero(new != ip)
    assert ((np.diff(new) == 0) == np.isin(np.arange(n), list(rows))).all()
    return {int(i): int(new[i]) for i in idx}


@pytest.mark.parametrize("dt", DTYPES)
def test_rows_without_a_positive_entry_beyond_the_first_trip(solver, dt):
    """k_csr_terms_check_s0, k_csrm_check_s0 and k_csrp_check_s0."""
    ip = host_a(np.dtype(dt).name)[0]
    d_ip, d_ix, d_da = dev_a(dt)
    assert N_A > CHECK + BLOCK
    assert MULTI["check_grid"] * BLOCK == PRODUCT["check_grid"] * BLOCK == CHECK
    u, w = term_vectors(dt, 1)
    C = 3
    mu = [u[0].clone() for _ in range(C)]
    eye = dev.CsrMatrix(torch.arange(N_A + 1, dtype=torch.int64, device=DEV),
                        torch.arange(N_A, dtype=torch.int32, device=DEV),
                        torch.ones(N_A, dtype=tdt(dt), device=DEV), N_A, solver=solver)
    for rows in ([CHECK - 1], [CHECK], [N_A - 1], [CHECK, N_A - 1], [CHECK - 1, CHECK]):
        q = min(rows)
        with poked(d_ip, emptied_rows(ip, rows)):
            me = matrix_a(solver, dt, allow_empty_rows=True)
            assert me.empty_rows == len(rows) and me.first_empty == q
            zero = {r: 0.0 for r in rows}
            with poked(u[0], zero):
                refused(lambda: dev.CsrTerms(me, [u[0]], [w[0]], solver=solver),
                        f"csr terms: row {q} of A + Σ u wᵀ has no positive entry")
            with poked(mu[1], zero):
                refused(lambda: dev.CsrMultiTerms(me, [[x] for x in mu], [[w[0]]] * C,
                                                  solver=solver),
                        f"csr terms: column 1: row {q} of A + Σ u wᵀ has no positive entry")
            if len(rows) == 2:                    # another column's higher row does not win
                with poked(mu[2], {rows[1]: 0.0}), poked(mu[0], {rows[1]: 0.0}):
                    refused(lambda: dev.CsrMultiTerms(me, [[x] for x in mu], [[w[0]]] * C,
                                                      solver=solver),
                            f"csr terms: column 0: row {rows[1]} of A + Σ u wᵀ")
            # with u > 0 there the operator is fine
            dev.CsrTerms(me, [u[0]], [w[0]], solver=solver).close()
            try:
                solver.solve_csr_product(eye, me, max_itr=MAX_ITR)
            except _lib.EigenValueError as e:
                assert f"csr product: row {q} of B·A has no positive entry" in str(e), str(e)
            else:
                pytest.fail("the product with an empty row was solved")
            me.close()
    eye.close()
    assert d_ip.cpu().numpy().tobytes() == ip.tobytes()


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("dt", DTYPES)
def test_multi_pack_and_collect_beyond_the_first_trip(solver, dt, C):
    """k_csrm_pack and k_csrm_collect: u is zero except on rows >= CHECK, so
    what the columns differ in reaches the solve only through the pack's
    second trip; v comes back through the collect's."""
    assert N_A > CHECK + BLOCK and MULTI["check_grid"] * BLOCK == CHECK
    assert _lib.csr_multi_cp(3) == 4 and _lib.csr_multi_cp(8) == 8
    m = matrix_a(solver, dt)
    rng = np.random.default_rng(50 + C)
    tail = N_A - CHECK
    us, ws = [], []
    for c in range(C):
        u = torch.zeros(N_A, dtype=tdt(dt), device=DEV)
        u[CHECK:] = up((1e-6 * (c + 1) * (0.5 + rng.random(tail))).astype(dt))
        us.append(u)
        ws.append(up((0.5 + rng.random(N_A)).astype(dt)))
    mt = dev.CsrMultiTerms(m, [[x] for x in us], [[x] for x in ws], solver=solver)
    lam, V, its, conv, st = solver.solve_csr_multi(m, mt, max_itr=MAX_ITR)
    mt.close()
    V = V.cpu().numpy()
    seen = set()
    for c in range(C):
        t = dev.CsrTerms(m, [us[c]], [ws[c]], solver=solver)
        r_lam, r_v, r_it, r_st = solver.solve_csr(m, t, max_itr=MAX_ITR)
        t.close()
        r_v = r_v.cpu().numpy()
        assert lam[c].tobytes() == np.dtype(dt).type(r_lam).tobytes(), (c, lam[c], r_lam)
        assert (int(its[c]), int(conv[c])) == (r_it, r_st["converged"]) == (MAX_ITR, 0)
        assert V[c].tobytes() == r_v.tobytes(), c
        seen.add(r_v[CHECK:].tobytes())
    assert len(seen) == C and st["rounds"] == MAX_ITR
    m.close()


@pytest.mark.parametrize("dt", DTYPES)
def test_zero_terms_and_an_identity_factor_change_no_bit(solver, dt):
    assert N_A > CHECK + BLOCK
    m = matrix_a(solver, dt)
    want = result(solver.solve_csr(m, max_itr=MAX_ITR))
    zero = torch.zeros(N_A, dtype=tdt(dt), device=DEV)
    w = term_vectors(dt, 1)[1][0]
    t = dev.CsrTerms(m, [zero], [w], solver=solver)
    assert result(solver.solve_csr(m, t, max_itr=MAX_ITR)) == want
    t.close()
    C = 3
    mt = dev.CsrMultiTerms(m, [[zero]] * C, [[w]] * C, solver=solver)
    lam, V, its, conv, _ = solver.solve_csr_multi(m, mt, max_itr=MAX_ITR)
    mt.close()
    V = V.cpu().numpy()
    for c in range(C):
        assert (float(lam[c]), V[c].tobytes(), int(its[c]), int(conv[c])) == \
            (want[0], want[1], want[2], want[4])
    eye = dev.CsrMatrix(torch.arange(N_A + 1, dtype=torch.int64, device=DEV),
                        torch.arange(N_A, dtype=torch.int32, device=DEV),
                        torch.ones(N_A, dtype=tdt(dt), device=DEV), N_A, solver=solver)
    assert result(solver.solve_csr_product(eye, m, max_itr=MAX_ITR)) == want
    assert result(solver.solve_csr_product(m, eye, max_itr=MAX_ITR)) == want
    eye.close()
    m.close()


# ---------------------------------------------------------------------------
# D. a batch beyond every cap
# ---------------------------------------------------------------------------
BATCH_SIZES = [300, PREP + BLOCK + 37, 65, 140_000, 1]
BIG_B, BIG_N = 1, PREP + BLOCK + 37


@functools.lru_cache(maxsize=None)
def batch_mats():
    heavy = {1: sc.heavy_at([0, PREP - 1, PREP, BIG_N - 1]), 3: sc.heavy_at([7, 139_999])}
    return tuple(sc.big(n, 60 + b, np.float64, heavy.get(b)) for b, n in enumerate(BATCH_SIZES))


@functools.lru_cache(maxsize=None)
def batch_stack():
    """(mat_first, row_ptr, col) of the stack: columns local to their matrix."""
    mats = batch_mats()
    mf = np.concatenate([[0], np.cumsum(BATCH_SIZES)]).astype(np.uint32)
    ptrs, base = [np.zeros(1, np.int64)], 0
    for ip, _, _ in mats:
        ptrs.append(ip[1:] + base)
        base += int(ip[-1])
    return mf, np.concatenate(ptrs), np.concatenate([m[1] for m in mats])


def batch_vals(dt):
    return np.concatenate([m[2] for m in batch_mats()]).astype(dt)


def test_the_batch_crosses_every_cap():
    mf, rp, col = batch_stack()
    N = int(mf[-1])
    assert BATCH_PREP == PREP                      # BATCH_SIZES is written in terms of PREP
    assert N == 664_947 and N > COLLECT and N > 5 * CHECK_ROWS
    assert BIG_N > BATCH_PREP + BLOCK and int(mf[3]) > CHECK_ROWS
    for b, n in enumerate(BATCH_SIZES):
        own = col[int(rp[mf[b]]):int(rp[mf[b + 1]])]
        assert own.min() == 0 and own.max() == n - 1


@pytest.mark.parametrize("dt", DTYPES)
def test_batched_solve_beyond_the_collect_cap_is_the_single_solves(solver, dt):
    mf, rp, col = batch_stack()
    assert int(mf[-1]) > COLLECT and int(mf[2]) > COLLECT      # matrices 2, 3, 4: second trip
    bt = dev.CsrBatch(up(rp), up(col), up(batch_vals(dt)), mf, solver=solver)
    lam, v, its, conv, st = solver.solve_csr_batched(bt, max_itr=MAX_ITR)
    bt.close()
    v = v.cpu().numpy()
    for b, (ip, ix, da) in enumerate(batch_mats()):
        m = dev.CsrMatrix(up(ip), up(ix), up(da.astype(dt)), len(ip) - 1, solver=solver)
        r_lam, r_v, r_it, r_st = solver.solve_csr(m, max_itr=MAX_ITR)
        m.close()
        assert lam[b].tobytes() == np.dtype(dt).type(r_lam).tobytes(), (b, lam[b], r_lam)
        assert (int(its[b]), int(conv[b])) == (r_it, r_st["converged"]), b
        assert v[int(mf[b]):int(mf[b + 1])].tobytes() == r_v.cpu().numpy().tobytes(), b
    assert int(conv[4]) == 1 and int(conv[1]) == 0               # n = 1 stops; the rest exhaust


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_stop_and_max_at_the_seam_inside_one_matrix_of_a_batch(solver, dt, sem):
    """k_csrb_prep: matrix 1 takes 2048 workgroups, so its elements from PREP
    on belong to the second trip of its own workgroups, while the matrices
    around it keep theirs."""
    cyclic = sem == _lib.ST_SEM_SYCL
    B = len(BATCH_SIZES)
    mf = batch_stack()[0]
    N = int(mf[-1])
    assert BIG_N > BATCH_PREP + BLOCK and BATCH_PREP == PREP
    col = np.concatenate([np.arange(n) for n in BATCH_SIZES]).astype(np.int32)
    bt = dev.CsrBatch(up(np.arange(N + 1, dtype=np.int64)), up(col), up(np.ones(N, dtype=dt)),
                      mf, solver=solver)
    base = np.concatenate([np.full(n, 10.0 * (b + 1)) for b, n in enumerate(BATCH_SIZES)]).astype(dt)
    inside = [0, 255, 256, PREP - 1, PREP, PREP + 255, BIG_N - 2, BIG_N - 1]
    where = [(BIG_B, p) for p in inside] + [(0, 150), (2, 31), (3, 139_999)]
    cases = [("const", None, base)]
    for b, p in where:
        n = BATCH_SIZES[b]
        s = base.copy()
        s[int(mf[b]):int(mf[b + 1])] = one_pair(n, p, dt, cyclic)
        cases.append(("pair", (b, p), s))
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
                                  eps=sv.EPS, k=1, max_itr=50, semantics=sem)
    got = states.cpu().numpy()
    fins = fins.cpu().numpy()
    bt.close()
    for j, (kind, at, s) in enumerate(cases):
        st = [_lib.st_state.from_buffer_copy(got[j, b].tobytes()) for b in range(B)]
        for b in range(B):
            own = s[int(mf[b]):int(mf[b + 1])]
            want = batch_expect_state(own, sv.EPS, sem, 1, 50)
            assert got[j, b].tobytes() == bytes(want), (kind, at, b, st[b].stop, st[b].max)
        assert int(fins[j]) == sum(x_.end != 0 for x_ in st)
        stops = [x_.stop for x_ in st]
        if kind == "pair":
            b, p = at
            assert [stops[i] for i in range(B) if i != b] == [1] * (B - 1), (at, stops)
            wrap = p == BATCH_SIZES[b] - 1
            assert stops[b] == (int(not cyclic) if wrap else 0), (at, stops)
        else:
            assert stops == [1] * B, (kind, at, stops)
            if kind == "max":
                b, p = at
                top = float(np.dtype(dt).type(10.0 * (b + 1)) + np.dtype(dt).type(sv.EPS) / 4)
                assert [x_.max for x_ in st] == [top if i == b else 10.0 * (i + 1)
                                                 for i in range(B)], at


def test_batch_column_check_beyond_the_first_trip(solver):
    """k_csrb_check_col: 16 lanes per row, 131 072 stacked rows per trip."""
    mf, rp, col = batch_stack()
    vals = batch_vals(np.float32)
    N = int(mf[-1])
    assert int(mf[3]) > CHECK_ROWS and N - 1 > 5 * CHECK_ROWS
    d_rp, d_col, d_vals = up(rp), up(col), up(vals)

    def make():
        return dev.CsrBatch(d_rp, d_col, d_vals, mf, solver=solver)

    def check(changes, expect):
        bad = col.copy()
        for e, c in changes.items():
            bad[e] = c
        msg = host_message(mf, rp, bad, vals)
        assert "null queue" not in msg and expect in msg, msg
        with poked(d_col, changes):
            refused(make, msg)

    far = CHECK_ROWS + 1000                                    # a row of matrix 1, second trip
    assert mf[1] <= far < mf[2]
    e_far = int(rp[far])
    check({e_far: BIG_N}, f"column index {BIG_N} of entry {e_far} (matrix 1, local row "
                          f"{far - int(mf[1])}) is outside [0, {BIG_N})")
    e_last = int(rp[N]) - 1                                    # the last stacked row: n_b = 1
    check({e_last: 1}, f"column index 1 of entry {e_last} (matrix 4, local row 0) is outside "
                       "[0, 1)")
    check({e_last: -1}, f"column index -1 of entry {e_last} (matrix 4, local row 0)")
    # legal for the stack, not for its own matrix of 140 000 rows
    for lr in (0, 70_000, 139_999):
        e = int(rp[int(mf[3]) + lr + 1]) - 1                   # the row's last entry
        check({e: 140_000}, f"column index 140000 of entry {e} (matrix 3, local row {lr}) is "
                            "outside [0, 140000)")
    # two offenders: the lower entry
    e_hi = int(rp[int(mf[3]) + 5])
    check({e_far: N - 1, e_hi: 140_000}, f"of entry {e_far} (matrix 1,")
    check({e_hi: 2**31 - 1, e_last: 7}, f"of entry {e_hi} (matrix 3, local row 5)")
    assert d_col.cpu().numpy().tobytes() == col.tobytes()
    make().close()
