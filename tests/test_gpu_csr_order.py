"""GPU: the CSR row products and dots bit for bit against the host model of
their documented order (csr_order_model.py).  Every comparison is tobytes()
equality.

1  csr_rowsum, csr_apply and csr_mfree_round on one structure with every row
   length that changes the path, in four value regimes: benign (A), a wide
   dynamic range (B), underflow (C), stored zeros (D)
2  the product B.A, the terms (K = 1, 4), the multi round (CP = 2, 8) and the
   batch round against the same model
3  the dot alone at the boundaries of the vector pass
4  entry 0 poisoned (largest finite, inf, NaN): the loads past a row's end are
   redirected to it and their products must be dropped, not multiplied away
5  a plan of more than 256 blocks with all classes in every span of the scan
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import csr_order_model as om  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from test_gpu_csr import DEV, DTYPES, MAX_ITR, diagonal_plus, tdt  # noqa: E402

SENTINEL = -7.0
SEM = _lib.ST_SEM_SYCL
REGIMES = [pytest.param(r, id=r) for r in om.REGIMES]
AB = [pytest.param(r, id=r) for r in ("A", "B")]


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


def up(a):
    return torch.from_numpy(np.array(a)).to(DEV)        # a copy: the cases are read-only


def csr_of(solver, indptr, indices, data, n):
    return dev.CsrMatrix(up(np.asarray(indptr, np.int64)), up(np.asarray(indices, np.int32)),
                         up(data), n, solver=solver)


def name_of(dt):
    return np.dtype(dt).name


def assert_same(got, want, what, rows=None, lens=None):
    """Bytes; the message names the rows that differ and their lengths."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    index = np.arange(len(got))
    if rows is not None:
        got, want, index = got[rows], want[rows], index[rows]
    if got.tobytes() == want.tobytes():
        return
    bits = got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)
    bad = index[bits.any(axis=1)]
    detail = [(int(r), None if lens is None else int(lens[r])) for r in bad[:8]]
    raise AssertionError(f"{what}: {len(bad)} rows differ from the model; (row, length): {detail}")


def test_shape_desc_matches_what_the_model_assumes():
    d = om.shape_desc()
    nnz_max, lanes = om.class_table()
    assert d["lanes"] == lanes == (4, 16, 64, 256) and d["nnz_max"] == nnz_max[:3]
    assert len(d["unroll"]) == len(d["rows"]) == 4
    assert d["prep_grid"] == (om.DOT_GRID,) and om.BLOCK == 256


# ---------------------------------------------------------------------------
# the model of a round, computed once per case and left unchanged
# ---------------------------------------------------------------------------
def v_update(s, v):
    """v_cur = v_prev * (s_prev / m), m the maximum of s_prev (found from 0)."""
    return v * (s / s.max())


@functools.lru_cache(maxsize=None)
def second_model(name, dtname):
    """om.model's pass over the second matrix (second_structure, the values
    and vectors of regime `name` under the next seed)."""
    indptr, indices = om.second_structure()
    vals, s, v = om.regime(name, dtname, om.SEED + 1)
    x = v * s
    sum0, _ = om.matvec(indptr, indices, vals, None, dtname, ones=True)
    tot, _ = om.matvec(indptr, indices, vals, x, dtname)
    return {"x": x, "sum0": sum0, "sum": tot}


def run_round(m, s_prev, v_prev, k=1):
    t = tdt(s_prev.dtype)
    s_next = torch.full((m.n,), SENTINEL, dtype=t, device=DEV)
    v_cur = torch.full((m.n,), SENTINEL, dtype=t, device=DEV)
    x = torch.full((m.n,), SENTINEL, dtype=t, device=DEV)
    dev.csr_mfree_round(m, up(s_prev), s_next, up(v_prev), v_cur, x, dev.new_state(DEV),
                        eps=1e-3, k=k, max_itr=MAX_ITR, semantics=SEM)
    return s_next.cpu().numpy(), v_cur.cpu().numpy(), x.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. one matrix
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", REGIMES)
@pytest.mark.parametrize("dt", DTYPES)
def test_rowsum_apply_and_round_are_the_model(solver, dt, name):
    """Regime C on the MI355X: gradual underflow throughout, as IEEE has it -
    subnormal entries, products and partial sums, a product below half the
    smallest subnormal gone to +0, the division of a subnormal sum; equal to
    the model in every row."""
    indptr, indices = om.structure()
    lens = np.diff(indptr)
    vals, s, v = om.regime(name, name_of(dt))
    mdl = om.model(name, name_of(dt))
    m = csr_of(solver, indptr, indices, vals, len(lens))
    assert (np.diff(m.plan()[1]) > 0).all()                    # all four row classes
    assert_same(dev.csr_rowsum(m).cpu().numpy(), mdl["sum0"], "csr_rowsum", lens=lens)
    assert_same(dev.csr_apply(m, up(mdl["x"])).cpu().numpy(), mdl["sum"], "csr_apply", lens=lens)
    s_next, v_cur, x = run_round(m, s, v)
    assert_same(x, mdl["x"], "x")
    assert_same(s_next, mdl["sum"] / mdl["x"], "s_next", lens=lens)
    assert_same(v_cur, v_update(s, v), "v_cur")
    if name == "D":
        zero = [r for r in range(len(lens)) if not vals[indptr[r]:indptr[r + 1]].any()]
        assert len(zero) == om.ZERO_ROWS
        assert all(s_next[r].tobytes() == np.zeros(1, dt).tobytes() for r in zero)   # +0 exactly
    print(f"{name} {name_of(dt)}: {len(lens)} rows in each of rowsum, apply, round")
    m.close()


# ---------------------------------------------------------------------------
# 2. the product, the terms, the multi round, the batch
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def product_model(name, dtname):
    """K0 (s0 = B (A 1)) and one round (y = A x, s_next = (B y) / x) of B.A."""
    mdl = om.model(name, dtname)
    ipb, ixb = om.second_structure()
    vb, _, _ = om.regime(name, dtname, om.SEED + 1)
    s0, _ = om.matvec(ipb, ixb, vb, mdl["sum0"], dtname)
    by, _ = om.matvec(ipb, ixb, vb, mdl["sum"], dtname)
    return {"s0": s0, "y0": mdl["sum0"], "y": mdl["sum"], "by": by, "s_next": by / mdl["x"]}


def product_halves(A, raw):
    half = raw.numel() // 2
    es = 8 if A.dtype_code else 4
    return (raw[:A.n * es].view(A.dtype).cpu().numpy(),
            raw[half:half + A.n * es].view(A.dtype).cpu().numpy())


def run_product_round(B, A, s, v):
    t = tdt(s.dtype)
    s_next = torch.full((A.n,), SENTINEL, dtype=t, device=DEV)
    v_cur = torch.full((A.n,), SENTINEL, dtype=t, device=DEV)
    raw = dev.csr_product_scratch(A)
    dev.csr_product_round(B, A, up(s), s_next, up(v), v_cur, raw, dev.new_state(DEV), eps=1e-3,
                          k=1, max_itr=MAX_ITR, semantics=SEM)
    return (s_next.cpu().numpy(), v_cur.cpu().numpy()) + product_halves(A, raw)


def factors(solver, name, dt):
    indptr, indices = om.structure()
    ipb, ixb = om.second_structure()
    va, s, v = om.regime(name, name_of(dt))
    vb, _, _ = om.regime(name, name_of(dt), om.SEED + 1)
    n = len(indptr) - 1
    return csr_of(solver, ipb, ixb, vb, n), csr_of(solver, indptr, indices, va, n), s, v


@pytest.mark.parametrize("name", AB)
@pytest.mark.parametrize("dt", DTYPES)
def test_product_rowsum_and_round_are_the_model(solver, dt, name):
    B, A, s, v = factors(solver, name, dt)
    assert (np.diff(A.plan()[1]) > 0).all() and (np.diff(B.plan()[1]) > 0).all()
    assert not torch.equal(A.col, B.col)
    mdl, pm = om.model(name, name_of(dt)), product_model(name, name_of(dt))
    lens_b = np.diff(om.second_structure()[0])
    raw = dev.csr_product_scratch(A)
    s0 = dev.csr_product_rowsum(B, A, raw).cpu().numpy()
    assert_same(product_halves(A, raw)[1], pm["y0"], "product K0: y")
    assert_same(s0, pm["s0"], "product K0: s0", lens=lens_b)
    s_next, v_cur, x, y = run_product_round(B, A, s, v)
    assert_same(x, mdl["x"], "product: x")
    assert_same(y, pm["y"], "product: y", lens=np.diff(om.structure()[0]))
    assert_same(s_next, pm["s_next"], "product: s_next", lens=lens_b)
    assert_same(v_cur, v_update(s, v), "product: v_cur")
    B.close()
    A.close()


def term_vectors(name, dtname, n, count, seed):
    """count pairs (u, w) [count, n]: benign under A, a range of 2^+-10 under B."""
    rng = np.random.default_rng(seed)
    u, w = 0.01 + rng.random((count, n)), 0.01 + rng.random((count, n))
    if name == "B":
        u = u * np.ldexp(1.0, rng.integers(-10, 11, size=(count, n)))
        w = w * np.ldexp(1.0, rng.integers(-10, 11, size=(count, n)))
    return u.astype(dtname), w.astype(dtname)


@functools.lru_cache(maxsize=None)
def terms_model(name, dtname, K):
    mdl = om.model(name, dtname)
    n = len(mdl["x"])
    u, w = term_vectors(name, dtname, n, K, 31)
    dots0 = np.array([om.dot(w[j], None, dtname, ones=True) for j in range(K)], dtype=dtname)
    dots = np.array([om.dot(w[j], mdl["x"], dtname) for j in range(K)], dtype=dtname)
    return {"u": u, "w": w, "dots0": dots0, "dots": dots,
            "s0": om.add_terms(mdl["sum0"], u, dots0, dtname),
            "s_next": om.add_terms(mdl["sum"], u, dots, dtname) / mdl["x"]}


def run_terms_round(m, t, s, v):
    td = tdt(s.dtype)
    s_next = torch.full((m.n,), SENTINEL, dtype=td, device=DEV)
    v_cur = torch.full((m.n,), SENTINEL, dtype=td, device=DEV)
    scratch = t.scratch()
    dev.csr_terms_round(m, t, up(s), s_next, up(v), v_cur, scratch, dev.new_state(DEV),
                        eps=1e-3, k=1, max_itr=MAX_ITR, semantics=SEM)
    return (s_next.cpu().numpy(), v_cur.cpu().numpy(), t.x(scratch).cpu().numpy(),
            t.dots(scratch).cpu().numpy())


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("name", AB)
@pytest.mark.parametrize("dt", DTYPES)
def test_terms_rowsum_and_round_are_the_model(solver, dt, name, K):
    indptr, indices = om.structure()
    lens = np.diff(indptr)
    vals, s, v = om.regime(name, name_of(dt))
    mdl, tm = om.model(name, name_of(dt)), terms_model(name, name_of(dt), K)
    m = csr_of(solver, indptr, indices, vals, len(lens))
    t = dev.CsrTerms(m, [up(x) for x in tm["u"]], [up(x) for x in tm["w"]], solver=solver)
    scratch = t.scratch()
    s0 = dev.csr_terms_rowsum(m, t, scratch).cpu().numpy()
    assert_same(t.dots(scratch).cpu().numpy(), tm["dots0"], "terms K0: dots")
    assert_same(s0, tm["s0"], "terms K0: s0", lens=lens)
    s_next, v_cur, x, dots = run_terms_round(m, t, s, v)
    assert_same(x, mdl["x"], "terms: x")
    assert_same(dots, tm["dots"], "terms: dots")
    assert_same(s_next, tm["s_next"], "terms: s_next", lens=lens)
    assert_same(v_cur, v_update(s, v), "terms: v_cur")
    t.close()
    m.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 256 + 37, 2048 * 256 + 256 + 37])
@pytest.mark.parametrize("dt", DTYPES)
def test_the_dot_alone_is_the_model(solver, dt, n):
    """w . 1 (K0) and w . x (a round) on a matrix of two entries per row, w and
    x over a range of 2^+-10 and 2^+-6; the last n is the smallest whose grid
    takes a second sweep (a lane's chain of two fmas)."""
    rng = np.random.default_rng(n)
    K = 2 if n < 4096 else 1
    w = ((1.0 - 0.5 * rng.random((K, n))) * np.ldexp(1.0, rng.integers(-10, 11, (K, n)))).astype(dt)
    u = np.full((K, n), 0.5, dtype=dt)
    s = ((1.0 - 0.5 * rng.random(n)) * np.ldexp(1.0, rng.integers(-3, 4, n))).astype(dt)
    v = ((1.0 - 0.5 * rng.random(n)) * np.ldexp(1.0, rng.integers(-3, 4, n))).astype(dt)
    m = diagonal_plus(solver, n, dt)
    t = dev.CsrTerms(m, [up(x) for x in u], [up(x) for x in w], solver=solver)
    scratch = t.scratch()
    dev.csr_terms_rowsum(m, t, scratch)
    want0 = np.array([om.dot(w[j], None, dt, ones=True) for j in range(K)], dtype=dt)
    assert_same(t.dots(scratch).cpu().numpy(), want0, "w . 1")
    _, _, x, dots = run_terms_round(m, t, s, v)
    assert_same(x, v * s, "x")
    assert_same(dots, np.array([om.dot(w[j], x, dt) for j in range(K)], dtype=dt), "w . x")
    t.close()
    m.close()


def pack(cols, cp, fill=1.0):
    """[C][n] -> the packed [n, CP] array, padding columns holding `fill`."""
    cols = np.asarray(cols)
    out = np.full((cols.shape[1], cp), fill, dtype=cols.dtype)
    out[:, :cols.shape[0]] = cols.T
    return out


MULTI_K = 2


@functools.lru_cache(maxsize=None)
def multi_model(name, dtname, c):
    """Column c of a multi round: its own s, v (column 0: the regime's; the
    others rescaled by a power of two and a factor near 1, x[col[0]] kept) and
    its own terms."""
    dt = np.dtype(dtname)
    indptr, indices = om.structure()
    vals, s, v = om.regime(name, dtname)
    if c:
        rng = np.random.default_rng(50 + c)
        keep = s[indices[0]], v[indices[0]]
        s = (s * (1.0 + 0.25 * rng.random(len(s))) * 2.0 ** (c % 3 - 1)).astype(dt)
        v = (v * (1.0 + 0.25 * rng.random(len(v)))).astype(dt)
        s[indices[0]], v[indices[0]] = keep
        x = v * s
        tot, _ = om.matvec(indptr, indices, vals, x, dtname)
    else:
        x, tot = om.model(name, dtname)["x"], om.model(name, dtname)["sum"]
    u, w = term_vectors(name, dtname, len(s), MULTI_K, 70 + c)
    dots = np.array([om.dot(w[j], x, dtname) for j in range(MULTI_K)], dtype=dt)
    return {"s": s, "v": v, "x": x, "u": u, "w": w, "dots": dots,
            "s_next": om.add_terms(tot, u, dots, dtname) / x, "v_cur": v_update(s, v)}


def run_multi_round(m, mt, cols):
    cp = mt.CP
    s_next, v_cur = mt.packed(SENTINEL), mt.packed(SENTINEL)
    scratch = mt.scratch()
    states, finished = mt.new_states()
    dev.csr_multi_round(m, mt, up(pack([c["s"] for c in cols], cp)), s_next,
                        up(pack([c["v"] for c in cols], cp)), v_cur, scratch, states, finished,
                        eps=1e-3, k=1, max_itr=MAX_ITR, semantics=SEM)
    return (s_next.cpu().numpy(), v_cur.cpu().numpy(), mt.x(scratch).cpu().numpy(),
            mt.dots(scratch).cpu().numpy())


def check_multi(got, cols, rows, lens):
    s_next, v_cur, x, dots = got
    for c, col in enumerate(cols):
        assert_same(x[:, c], col["x"], f"multi column {c}: x")
        assert_same(dots[c], col["dots"], f"multi column {c}: dots")
        assert_same(s_next[:, c], col["s_next"], f"multi column {c}: s_next", rows=rows, lens=lens)
        assert_same(v_cur[:, c], col["v_cur"], f"multi column {c}: v_cur")
    assert (s_next[:, len(cols):] == SENTINEL).all() and (v_cur[:, len(cols):] == SENTINEL).all()


def multi_of(solver, m, cols):
    return dev.CsrMultiTerms(m, up(np.array([c["u"] for c in cols])),
                             up(np.array([c["w"] for c in cols])), solver=solver)


@pytest.mark.parametrize("C", [2, 8])
@pytest.mark.parametrize("dt", DTYPES)
def test_multi_round_is_the_model(solver, dt, C):
    indptr, indices = om.structure()
    vals, _, _ = om.regime("B", name_of(dt))
    cols = [multi_model("B", name_of(dt), c) for c in range(C)]
    m = csr_of(solver, indptr, indices, vals, len(indptr) - 1)
    mt = multi_of(solver, m, cols)
    assert mt.CP == C and mt.K == MULTI_K
    check_multi(run_multi_round(m, mt, cols), cols, slice(None), np.diff(indptr))
    mt.close()
    m.close()


def batch_case(name, dtname):
    """Three stacked matrices: the structure, a small one that has ended, the
    second structure.  (matrices, s, v stacked, what each live matrix gives)."""
    first, second = om.model(name, dtname), second_model(name, dtname)
    ip1, ix1 = om.structure()
    ip2, ix2 = om.second_structure()
    a1, s1, v1 = om.regime(name, dtname)
    a2, s2, v2 = om.regime(name, dtname, om.SEED + 1)
    k = 40
    small = (3 * np.arange(k + 1, dtype=np.int64),
             np.stack([np.arange(k), (np.arange(k) + 1) % k, (np.arange(k) + 7) % k],
                      axis=1).reshape(-1).astype(np.int32), np.full(3 * k, 0.25, dtype=dtname))
    ones = np.ones(k, dtype=dtname)
    want = [(first["x"], first["sum"] / first["x"], v_update(s1, v1)), None,
            (second["x"], second["sum"] / second["x"], v_update(s2, v2))]
    return ([(ip1, ix1, a1), small, (ip2, ix2, a2)], np.concatenate([s1, ones, s2]),
            np.concatenate([v1, ones, v2]), want)


def run_batch_round(solver, mats, s, v, dt, poison=None):
    """Launch 2 of the batch with matrix 1 ended in launch 1: per matrix (x,
    s_next, v_cur) and the state bytes."""
    mat_first = np.concatenate([[0], np.cumsum([len(m[0]) - 1 for m in mats])]).astype(np.uint32)
    ptrs, base = [np.zeros(1, np.int64)], 0
    for ip, _, _ in mats:
        ptrs.append(ip[1:] + base)
        base += int(ip[-1])
    bt = dev.CsrBatch(up(np.concatenate(ptrs)), up(np.concatenate([m[1] for m in mats])),
                      up(np.concatenate([m[2] for m in mats])), mat_first, solver=solver)
    if poison is not None:
        bt.values[0] = poison
    t = tdt(dt)
    out = [torch.full((bt.n,), SENTINEL, dtype=t, device=DEV) for _ in range(3)]
    ended = _lib.st_state()
    ended.end, ended.done, ended.stop, ended.iters, ended.max = 1, 1, 1, 1, 3.5
    raw = np.zeros((len(mats), 64), dtype=np.uint8)
    raw[1] = np.frombuffer(bytes(ended), dtype=np.uint8)
    states = up(raw)
    fin = torch.ones(1, dtype=torch.int32, device=DEV)
    dev.csr_batch_mfree_round(bt, up(s), out[0], up(v), out[1], out[2], states, fin, eps=1e-3,
                              k=2, max_itr=MAX_ITR, semantics=SEM)
    s_next, v_cur, x = (o.cpu().numpy() for o in out)
    mf = [int(i) for i in mat_first]
    got = [(x[mf[b]:mf[b + 1]], s_next[mf[b]:mf[b + 1]], v_cur[mf[b]:mf[b + 1]])
           for b in range(len(mats))]
    assert states.cpu().numpy()[1].tobytes() == raw[1].tobytes()
    bt.close()
    return got


def check_batch(got, want, first_rows):
    for part in got[1]:                       # the ended matrix: the sentinel kept
        assert (part == SENTINEL).all()
    for b in (0, 2):
        rows = first_rows if b == 0 else slice(None)
        assert_same(got[b][0], want[b][0], f"batch matrix {b}: x")
        assert_same(got[b][1], want[b][1], f"batch matrix {b}: s_next", rows=rows)
        assert_same(got[b][2], want[b][2], f"batch matrix {b}: v_cur")


@pytest.mark.parametrize("dt", DTYPES)
def test_batch_round_is_the_model(solver, dt):
    mats, s, v, want = batch_case("B", name_of(dt))
    check_batch(run_batch_round(solver, mats, s, v, dt), want, slice(None))


# ---------------------------------------------------------------------------
# 4. entry 0 poisoned
# ---------------------------------------------------------------------------
POISONS = [pytest.param("max", id="max"), pytest.param("inf", id="inf"),
           pytest.param("nan", id="nan")]


@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("dt", DTYPES)
def test_a_poisoned_entry_0_reaches_no_other_row(solver, dt, poison):
    """Regime A, where x[col[0]] = 4: with vals[0] the largest finite value
    every product of a redirected load is inf (NaN, inf for the other two
    poisons), and a select drops it where a multiplication by a mask would
    leave NaN.  Row 0 holds entry 0 alone; every other row of every call must
    be the unpoisoned model's.  No step call validates the values (creation
    does, for the terms: those objects are made before the poison is set), so
    every call accepts all three poisons."""
    dtname = name_of(dt)
    value = {"max": float(np.finfo(dt).max), "inf": np.inf, "nan": np.nan}[poison]
    indptr, indices = om.structure()
    lens = np.diff(indptr)
    n = len(lens)
    assert lens[0] == 1
    rest = slice(1, None)
    vals, s, v = om.regime("A", dtname)
    mdl = om.model("A", dtname)
    assert mdl["x"][indices[0]] == 4
    m = csr_of(solver, indptr, indices, vals, n)
    tm = terms_model("A", dtname, 4)
    t = dev.CsrTerms(m, [up(x) for x in tm["u"]], [up(x) for x in tm["w"]], solver=solver)
    cols = [multi_model("A", dtname, c) for c in range(3)]
    assert all(c["x"][indices[0]] == 4 for c in cols)
    mt = multi_of(solver, m, cols)
    m.values[0] = value
    bad = dev.csr_rowsum(m).cpu().numpy()
    assert np.isnan(bad[0]) if poison == "nan" else bad[0] == value        # the poison is in
    assert_same(bad, mdl["sum0"], "csr_rowsum", rows=rest, lens=lens)
    assert_same(dev.csr_apply(m, up(mdl["x"])).cpu().numpy(), mdl["sum"], "csr_apply", rows=rest,
                lens=lens)
    s_next, v_cur, x = run_round(m, s, v)
    assert not np.isfinite(s_next[0])
    assert_same(s_next, mdl["sum"] / mdl["x"], "s_next", rows=rest, lens=lens)
    assert_same(v_cur, v_update(s, v), "v_cur")
    s_next, v_cur, x, dots = run_terms_round(m, t, s, v)
    assert_same(dots, tm["dots"], "terms: dots")
    assert_same(s_next, tm["s_next"], "terms: s_next", rows=rest, lens=lens)
    check_multi(run_multi_round(m, mt, cols), cols, rest, lens)
    mt.close()
    t.close()
    m.close()
    # the product: the poison in A (B never gathers y[0]), then in B
    pm = product_model("A", dtname)
    lens_b = np.diff(om.second_structure()[0])
    B, A, _, _ = factors(solver, "A", dt)
    A.values[0] = value
    s_next, v_cur, x, y = run_product_round(B, A, s, v)
    assert not np.isfinite(y[0])
    assert_same(y, pm["y"], "product, A poisoned: y", rows=rest, lens=lens)
    assert_same(s_next, pm["s_next"], "product, A poisoned: s_next", lens=lens_b)
    A.values[0] = float(vals[0])
    B.values[0] = value
    assert pm["y"][om.second_structure()[1][0]] > 16         # the dropped product overflows
    s_next, v_cur, x, y = run_product_round(B, A, s, v)
    assert_same(y, pm["y"], "product, B poisoned: y")
    assert not np.isfinite(s_next[0])
    assert_same(s_next, pm["s_next"], "product, B poisoned: s_next", rows=rest, lens=lens_b)
    B.close()
    A.close()
    # the batch: entry 0 of matrix 0; its redirected loads read col[0] with no base
    mats, sb, vb, want = batch_case("A", dtname)
    check_batch(run_batch_round(solver, mats, sb, vb, dt, poison=value), want, rest)


# ---------------------------------------------------------------------------
# 5. a plan beyond 256 blocks with all classes in every span
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_a_plan_of_more_than_256_blocks(solver, dt):
    indptr, indices, heavy = om.plan_structure()
    n = om.PLAN_N
    vals = (1.0 - np.random.default_rng(8).random(len(indices))).astype(dt)
    m = csr_of(solver, indptr, indices, vals, n)
    order, first = m.plan()
    h_order, h_first, used = _lib.csr_plan(indptr)
    assert used == 4 and np.array_equal(first, h_first) and np.array_equal(order, h_order)
    short = np.setdiff1d(np.arange(n), heavy)
    rows = np.concatenate([np.array(heavy), np.random.default_rng(9).choice(short, 200, False)])
    want, _ = om.matvec(indptr, indices, vals, None, dt, ones=True, rows=rows)
    assert_same(dev.csr_rowsum(m).cpu().numpy(), want, "csr_rowsum", rows=rows,
                lens=np.diff(indptr))
    m.close()
