"""GPU: the dense row sums against the host model of their order, bit for bit.

tests/dense_order_model.py restates the summation order of every dense kernel
in IEEE arithmetic; here the device's bytes are compared with it (tobytes()
equality, no tolerance):

  1. every variant of rowsum_kernels.VARIANTS and the two 16-bit kernels, on
     every shape of dense_order_model.SHAPES that fits, in four value regimes
     (A benign, B wide range with hot elements at every level of the order, C
     underflow, D stored zeros): s, and for the flat forms every piece partial
     and the row sum of the device's own partials; the deferred variants on
     every round, the read-only ones against a matrix built on the host;
  2. the grouped launch shapes (2, 4, 8 rows per workgroup, remainder rows,
     both walk directions), with the launch shape asserted;
  3. partition independence: the same 64 rows alone and inside a 2113-row
     block, through four kernels;
  4. one poisoned element (the largest finite value, inf, NaN): its own row
     shows it, every other row keeps the model's bytes.

The matrix-free kernels get a rounded x = v * s (scales `random + 0.5`).  In
fp64 their model (an exact integer chain) runs on dense_order_model.subset_rows.
test_dense_order_model.py shows on the CPU that these inputs tell the model
from each wrong order of its list.  No seeds are looped over and nothing is
retried: a mismatch is a finding.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import dense_order_model as dm  # noqa: E402
import exact_sums as xs  # noqa: E402
import rowsum_kernels as rk  # noqa: E402
import test_gpu_stats_positions as sp  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402

DTNAMES = ("float32", "float64")
STORES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
MFREE = ("mfree_round", "mfree_round_flat")


def diff(name, got, want, rows=None):
    """[] when the bytes agree, else one line naming the rows that differ."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype,
                                                                 got.shape, want.shape)
    bits = f"u{got.dtype.itemsize}"
    bad = np.argwhere(got.view(bits) != want.view(bits))
    if not len(bad):
        return []
    first = tuple(bad[0])
    where = [int(b[0]) if rows is None else int(rows[b[0]]) for b in bad[:8]]
    return [f"{name}: {len(bad)} of {got.size} differ, rows {where}..., first {first}: device "
            f"{got[first]!r} ({got[first].tobytes().hex()}) model {want[first]!r} "
            f"({want[first].tobytes().hex()})"]


# ---------------------------------------------------------------------------
# the inputs: built once per (dtype, regime), the current pair kept
# ---------------------------------------------------------------------------
_INPUT = {"key": None}


def _cache(dtname, regime):
    if _INPUT["key"] != (dtname, regime):
        _INPUT.clear()
        _INPUT["key"] = (dtname, regime)
    return _INPUT


def base(orc, dtname, shape):
    return orc.generate_c("random", shape[1], xs.SEED, np.dtype(dtname).type, nrows=shape[0])


def matrix(orc, regime, dtname, shape, fma):
    """The regime's matrix for the add-only kernels, or (fma) for the
    matrix-free ones: regime C with subnormal products.  D's all-zero row goes
    to both: v_prev[r] * s_prev[r] is never zero, and 0 / x must be +0."""
    c = _cache(dtname, regime)
    key = ("a", shape, fma and regime == "C")
    if key not in c:
        c[key] = dm.matrix(regime, dtname, shape, base(orc, dtname, shape), fma=fma)
        c[key].setflags(write=False)
    return c[key]


def vectors(orc, regime, dtname, n, fma, count=1, seed=9):
    return [dm.scale_vector(orc, n, dtname, seed + k, regime, fma) for k in range(count)]


def half_matrix(orc, regime, store, shape):
    """(the 16-bit torch tensor on the host, its exact fp32 widening):
    dense_order_model.half_case, the input of the CPU power check too."""
    c = _cache(store, regime)
    key = ("h", shape)
    if key not in c:
        wide = dm.half_case(regime, store, shape, base(orc, "float32", shape))
        h = torch.from_numpy(wide).to(STORES[store])
        assert h.float().numpy().tobytes() == wide.tobytes()      # the storage type holds it
        c[key] = (h, wide)
    return c[key]


# ---------------------------------------------------------------------------
# 1. every variant, every shape, four regimes
# ---------------------------------------------------------------------------
def check_variant(orc, variant, sem, regime, dtname, shape):
    """One kernel on one case: the lines that differ from the model."""
    nrows, ncols = shape
    base_kind, transforms, in_block, flat = rk.VARIANTS[variant]
    fma = variant in MFREE
    a = matrix(orc, regime, dtname, shape, fma)
    row0 = rk.block_row0(nrows, ncols) if in_block else 0
    n_full = max(ncols, row0 + nrows)
    tag = f"{variant} sem{sem} {regime} {dtname} {shape}"
    kw, out = {}, []
    if fma:
        kw["s_prev"], kw["v_prev"] = (vectors(orc, regime, dtname, ncols, True, 1, seed)[0]
                                      for seed in (9, 10))
    elif base_kind == "flat_round_deferred":
        kw["scale"] = vectors(orc, regime, dtname, ncols, False, int(variant[-1]) + 1)
        kw["rounds"] = True
    elif transforms:
        kw["scale"] = vectors(orc, regime, dtname, n_full, False)[0]
    r = rk.run(orc, variant, a, sem, row0, **kw)
    stored, s = r["stored"], r["s"]
    if not transforms:
        assert stored.tobytes() == a.tobytes()
    if fma:
        rows = dm.subset_rows(nrows, ncols) if dtname == "float64" else None
        sel = slice(None) if rows is None else rows
        if variant == "mfree_round":
            want = dm.mfree(a, kw["s_prev"], kw["v_prev"], row0, rows=rows)
            return diff(f"{tag} s", s[sel], want, rows)
        want = dm.mfree_flat_pieces(a, kw["s_prev"], kw["v_prev"], rows=rows)
        out += diff(f"{tag} part", r["part"][sel], want, rows)
        return out + diff(f"{tag} s of the device's part", s,
                          dm.mparts(r["part"], kw["s_prev"], kw["v_prev"], row0))
    if base_kind == "flat_round_deferred":
        # every round, the read-only ones on the matrix that exists in registers only
        mainpy = sem == rk.MAINPY
        m = a
        with np.errstate(under="ignore"):
            for k, (sk, ik) in enumerate(zip(r["pend_s"], r["pend_inv"])):
                m = dm.scaled(m, sk, row0, mainpy, inv=ik)
                out += diff(f"{tag} round {k} part", r["part_rounds"][k], dm.flat_pieces(m))
                out += diff(f"{tag} round {k} s", r["s_rounds"][k], dm.parts(r["part_rounds"][k]))
        return out + diff(f"{tag} stored", stored, m)
    if flat:
        out += diff(f"{tag} part", r["part"], dm.flat_pieces(stored))
        return out + diff(f"{tag} s of the device's part", s, dm.parts(r["part"]))
    if base_kind == "split_round":
        return diff(f"{tag} s", s, dm.split_round(stored, r["col0"], r["col1"])[1])
    if base_kind == "split_flat_round":
        # the two partial buffers per piece (the remote one without the pieces
        # k_parts skips: no workgroup past row group 0 writes them), and s from
        # the device's own partials
        c0, c1 = r["col0"], r["col1"]
        _, _, ppr, _, npl, pa, nfull = dm.split_flat_layout(stored.dtype, ncols, c0, c1)
        remote, local, _ = dm.split_flat(stored, c0, c1)
        off = nrows * -(-ncols // dm.BLOCK)               # split_flat_local_off
        got_r = r["split_part"][:nrows * ppr].reshape(nrows, ppr).copy()
        got_l = r["split_part"][off:off + nrows * npl].reshape(nrows, npl)
        got_r[:, pa:pa + nfull] = 0
        out += diff(f"{tag} remote part", got_r, remote)
        out += diff(f"{tag} local part", got_l, local)
        return out + diff(f"{tag} s of the device's parts", s,
                          dm.parts_split(got_r, pa, nfull, got_l))
    return diff(f"{tag} s", s, dm.fused(stored))


EVERY = [(dtname, regime, variant, sem) for dtname in DTNAMES for regime in dm.REGIMES
         for variant, sem in rk.cases()]


@pytest.mark.parametrize("dtname,regime,variant,sem", EVERY,
                         ids=[f"{d}-{r}-{v}-sem{s}" for d, r, v, s in EVERY])
def test_every_variant_equals_the_model(orc, dtname, regime, variant, sem):
    """s (and part, and every deferred round) of one kernel in one regime, on
    every shape that fits: the model's bytes."""
    bad = []
    for shape in dm.SHAPES:
        if rk.fits(variant, *shape):
            bad += check_variant(orc, variant, sem, regime, dtname, shape)
    assert not bad, "\n".join(bad[:12])


HALVES = [(store, regime, variant) for store in STORES for regime in dm.REGIMES
          for variant in rk.HALF]


@pytest.mark.parametrize("store,regime,variant", HALVES, ids=["-".join(h) for h in HALVES])
def test_the_half_kernels_equal_the_model(orc, store, regime, variant):
    """rowsum_half and mfree_round_half on fp16 / bf16 matrices: the fp32 sums
    of the exactly widened matrix, 8 columns per lane and chunk; C: stored
    subnormals of the 16-bit type."""
    bad = []
    for shape in dm.SHAPES:
        nrows, ncols = shape
        tag = f"{variant} {store} {regime} {shape}"
        if variant == "rowsum_half":
            h, wide = half_matrix(orc, regime, store, shape)
            r = rk.run(orc, variant, h)
            bad += diff(tag, r["s"], dm.half_rowsum(wide))
        elif nrows <= ncols:
            h, wide = half_matrix(orc, regime, store, shape)
            row0 = rk.block_row0(nrows, ncols)
            s, v = (vectors(orc, "A", "float32", ncols, False, 1, seed)[0] for seed in (9, 10))
            r = rk.run(orc, variant, h, row0=row0, s_prev=s, v_prev=v)
            bad += diff(tag, r["s"], dm.mfree(wide, s, v, row0, w=dm.HALF_W))
    assert not bad, "\n".join(bad[:12])


# ---------------------------------------------------------------------------
# 2. the grouped launch shapes (regime B)
# ---------------------------------------------------------------------------
GROUPED_N = 2056
DT = {"float32": np.float32, "float64": np.float64}


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(rk.DEV)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("sem", [rk.SYCL, rk.MAINPY])
@pytest.mark.parametrize("dtname", DTNAMES)
def test_fused_round_grouped(orc, dtname, sem, k):
    """k_round on 2049 x 2056 (test_gpu_stats_positions' block): 2 rows per
    group and a remainder row, walked forward (k = 2) and backwards (k = 3)."""
    nrows, row0 = sp.GROUPED
    shape = (nrows, GROUPED_N)
    kernel, rows, nt, _ = sp.policy(_lib.load(), DT[dtname], nrows, GROUPED_N, _lib.ST_FORM_ROUND)
    assert (kernel, rows, nt) == ("k_round", 2, False)
    a = matrix(orc, "B", dtname, shape, False)
    ta, s_next = _d(a), torch.empty(nrows, dtype=rk.TD[a.dtype], device=rk.DEV)
    dev.fused_round(ta, _d(vectors(orc, "B", dtname, GROUPED_N, False)[0]), s_next,
                    torch.ones(GROUPED_N, dtype=rk.TD[a.dtype], device=rk.DEV),
                    dev.new_state(rk.DEV), row0=row0, eps=0.0, k=k, semantics=sem)
    bad = diff(f"fused_round k={k}", rk.to_np(s_next), dm.fused(rk.to_np(ta)))
    assert not bad, bad


def _mfree_through(L, dtname, a, s, v, row0, k):
    nrows, ncols = a.shape
    tdt = rk.TD[a.dtype]
    ta, ts, tv = _d(a), _d(s), _d(v)
    s_next = torch.empty(nrows, dtype=tdt, device=rk.DEV)
    v_cur = torch.empty(ncols, dtype=tdt, device=rk.DEV)
    state = dev.new_state(rk.DEV)
    sfx = "f64" if dtname == "float64" else "f32"
    _lib.check(getattr(L, f"st_mfree_round_{sfx}")(
        ta.data_ptr(), ts.data_ptr(), s_next.data_ptr(), tv.data_ptr(), v_cur.data_ptr(), nrows,
        ncols, row0, 0.0, k, _lib.ST_MAX_ITR, rk.SYCL, state.data_ptr(),
        torch.cuda.current_stream(rk.DEV).cuda_stream), "mfree_round", L)
    return rk.to_np(s_next)


def _mfree_grouped(orc, L, dtname, k):
    nrows, row0 = sp.GROUPED
    a = matrix(orc, "B", dtname, (nrows, GROUPED_N), True)
    s, v = (vectors(orc, "B", dtname, GROUPED_N, True, 1, seed)[0] for seed in (9, 10))
    rows = dm.subset_rows(nrows, GROUPED_N) if dtname == "float64" else None
    got = _mfree_through(L, dtname, a, s, v, row0, k)
    return diff(f"mfree_round k={k}", got[slice(None) if rows is None else rows],
                dm.mfree(a, s, v, row0, rows=rows), rows)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("dtname", DTNAMES)
def test_mfree_round_grouped(orc, dtname, k):
    """k_mfree on 2049 x 2056: 4 rows per group, 512 groups and a remainder
    row; k = 1 walks backwards."""
    L = _lib.load()
    assert sp.policy(L, DT[dtname], sp.GROUPED[0], GROUPED_N, _lib.ST_FORM_MFREE) == \
        ("k_mfree", 4, False, 512)
    bad = _mfree_grouped(orc, L, dtname, k)
    assert not bad, bad


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("shape,rows,nt", [(1, 2, False), (2, 4, False), (3, 4, True)],
                         ids=["cached2", "cached4", "nontemporal4"])
@pytest.mark.parametrize("dtname", DTNAMES)
def test_mfree_round_grouped_shapes(orc, dtname, shape, rows, nt, k):
    """k_mfree's other instantiations on the same block, through the tuning
    build (st_set_mfree_shape): 2 rows, 4 rows, 4 rows with non-temporal loads."""
    L = _lib.load_tuning()
    saved = L.st_set_mfree_shape(0)
    try:
        assert L.st_set_mfree_shape(shape) >= 0
        assert sp.policy(L, DT[dtname], sp.GROUPED[0], GROUPED_N, _lib.ST_FORM_MFREE) == \
            ("k_mfree", rows, nt, 512)
        bad = _mfree_grouped(orc, L, dtname, k)
    finally:
        L.st_set_mfree_shape(saved)
    assert not bad, bad


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("name", ["rows8", "rows2"])
def test_mfree_half_round_grouped(orc, name, store, k):
    """k_mfree_half's 8-row (4097 x 4104) and 2-row (4099 x 8200) shapes, taken
    from st_half_shape_desc, at both parities of k."""
    (nrows, n, row0), shape = sp.HALF_GROUPED[name]
    assert sp.half_grouped_shape(nrows, n) == shape, (name, sp.half_desc())
    h, wide = half_matrix(orc, "B", store, (nrows, n))
    s, v = (vectors(orc, "A", "float32", n, False, 1, seed)[0] for seed in (9, 10))
    s_next = torch.empty(nrows, dtype=torch.float32, device=rk.DEV)
    dev.mfree_round_half(h.to(rk.DEV), _d(s), s_next, _d(v),
                         torch.empty(n, dtype=torch.float32, device=rk.DEV),
                         dev.new_state(rk.DEV), row0=row0, eps=0.0, k=k, semantics=rk.SYCL)
    bad = diff(f"mfree_round_half {name} k={k}", rk.to_np(s_next),
               dm.mfree(wide, s, v, row0, w=dm.HALF_W))
    assert not bad, bad


# ---------------------------------------------------------------------------
# 3. partition independence (regime B, unit scales)
# ---------------------------------------------------------------------------
PART_ROWS, PART_BLOCK = 64, 2113
PART_AT = (0, 1000, PART_BLOCK - PART_ROWS)
PART_KERNELS = ("rowsum", "rowsum_flat", "fused_round", "flat_round")


@pytest.mark.parametrize("ncols", [4096, 4099])
@pytest.mark.parametrize("variant", PART_KERNELS)
@pytest.mark.parametrize("dtname", DTNAMES)
def test_a_row_sum_does_not_depend_on_the_partition(orc, dtname, variant, ncols):
    """The same 64 rows alone, and as rows 0 .. 63, 1000 .. 1063 and the last 64
    of a 2113-row block (2 rows per workgroup and a remainder row; other
    workgroups, waves and grid strides each time): the same bytes, and the
    model's.  Unit scales: a transforming kernel stores the block as it is."""
    rows = matrix(orc, "B", dtname, (PART_ROWS, ncols), False)
    fill = matrix(orc, "B", dtname, (PART_BLOCK, ncols), False)
    flat = variant in ("rowsum_flat", "flat_round")
    want = dm.parts(dm.flat_pieces(rows)) if flat else dm.fused(rows)
    alone = rk.run(orc, variant, np.array(rows), unit=True)
    bad = diff(f"{variant} alone", alone["s"], want)
    for at in PART_AT:
        blk = np.array(fill)
        blk[at:at + PART_ROWS] = rows
        r = rk.run(orc, variant, blk, unit=True)
        assert r["stored"].tobytes() == blk.tobytes()
        bad += diff(f"{variant} as rows {at} ..", r["s"][at:at + PART_ROWS], want)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------
# 4. one poisoned element
# ---------------------------------------------------------------------------
POISONS = ("max", "inf", "nan")


def poison_value(kind, dt):
    return {"max": np.finfo(dt).max, "inf": np.inf, "nan": np.nan}[kind]


def check_poison(name, kind, got, clean, poisoned_want, row):
    """Every row but `row` keeps the clean model's bytes; `row` equals the
    model for the finite poison, is inf for inf and NaN for NaN."""
    other = np.arange(len(got)) != row
    bad = diff(f"{name}: the other rows", got[other], clean[other])
    if kind == "max":
        bad += diff(f"{name}: row {row}", got[row:row + 1], poisoned_want[row:row + 1])
    elif kind == "inf" and not np.isposinf(got[row]):
        bad.append(f"{name}: row {row} is {got[row]!r}, not inf")
    elif kind == "nan" and not np.isnan(got[row]):
        bad.append(f"{name}: row {row} is {got[row]!r}, not NaN")
    return bad


# rows of a 2061 x 4096 block (k_fused: 2 rows per group and a remainder row;
# k_flat_sum: pairs through one tree): both members of a pair, a remainder row
FUSED_POISON = ((2061, 4096), (0, 1, 1030, 1031, 2060))
# pieces per row 6, 12 (k_parts_seg<16>: 4 rows per wave) and 17 (<32>: 2 rows
# per wave): the first and last row that share a wave, the first and last piece
SEG_POISON = [((37, 6144), (0, 3, 32, 35, 36)), ((37, 12288), (4, 7)),
              ((37, 17000), (0, 1, 34, 35))]


@pytest.mark.parametrize("kind", POISONS)
@pytest.mark.parametrize("dtname", DTNAMES)
def test_poison_in_the_row_sum_kernels(orc, dtname, kind):
    """rowsum (k_fused) and rowsum_flat (k_flat_sum, k_parts_seg) with one
    poisoned element: the even and the odd row of a 2-row group (in fp32
    k_flat_sum's wave_sum_pair), a remainder row, the first and last row of a
    k_parts_seg wave; in the first and in the last piece."""
    dt = DT[dtname]
    # the launch shapes meant: k_fused with 2 rows per group on the 2061-row
    # block; k_flat_sum with 2 rows per workgroup - one wave_sum_pair - in fp32
    # and 1 row in fp64 (there the pairs are mfree_round_flat's, poisoned
    # below).  The query answers for the K0 form of a block the flat round pays
    # for; the step call takes the same rows per workgroup at any size.  The
    # rows per k_parts_seg wave (64 / 16 and 64 / 32) follow from the piece
    # counts and are not exposed by any query.
    sfx = "f64" if dtname == "float64" else "f32"
    k0 = _lib.launch_policy(sfx, *FUSED_POISON[0], _lib.ST_FORM_ROWSUM)
    assert (k0["kernel"], k0["rows"]) == ("k_fused", 2)
    k0 = _lib.launch_policy(sfx, 8192, 8192, _lib.ST_FORM_ROWSUM)
    assert (k0["kernel"], k0["rows"]) == ("k_flat_sum", 2 if dtname == "float32" else 1)
    assert [xs.pieces_per_row(dt, c) for (_, c), _ in SEG_POISON] == [6, 12, 17]
    bad = []
    with np.errstate(over="ignore", invalid="ignore"):
        for shape, rows in [FUSED_POISON] + SEG_POISON:
            a = np.array(matrix(orc, "A", dtname, shape, False))
            clean = {"rowsum": dm.fused(a), "rowsum_flat": dm.parts(dm.flat_pieces(a))}
            for row in rows:
                for col in (5, shape[1] - 3):
                    p = a.copy()
                    p[row, col] = poison_value(kind, dt)
                    for variant in ("rowsum", "rowsum_flat"):
                        if variant == "rowsum" and shape != FUSED_POISON[0]:
                            continue
                        want = dm.fused(p[row:row + 1]) if variant == "rowsum" else dm.parts(
                            dm.flat_pieces(p[row:row + 1]))
                        full = clean[variant].copy()
                        full[row] = want[0]
                        got = rk.run(orc, variant, p)["s"]
                        bad += check_poison(f"{variant} {shape} poison at ({row}, {col})", kind,
                                            got, clean[variant], full, row)
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("kind", POISONS)
@pytest.mark.parametrize("variant", MFREE)
@pytest.mark.parametrize("dtname", DTNAMES)
def test_poison_in_the_matrix_free_groups(orc, dtname, variant, kind):
    """mfree_round (4 rows per group from 1024 rows) and mfree_round_flat (8
    rows per workgroup, pairs through one tree) on 1031 x 4096: the poison in
    each slot of the first group, in the last full group and in a remainder
    row.  Every other row keeps its bytes: the model's in fp32; in fp64, whose
    model is the integer chain, the model's inside the poisoned row's group and
    those of the device's own clean run (equal to the model inside each group
    visited) outside it.  The slots 0 .. 7 are each slot of a group of 8, 4 or
    2: k_mfree's 4 rows are asserted, k_flat<MF>'s 8 are in no query."""
    dt = DT[dtname]
    shape = (1031, 4096)
    assert _lib.launch_policy("f64" if dtname == "float64" else "f32", 1031, 4096,
                              _lib.ST_FORM_MFREE)["rows"] == 4
    a = np.array(matrix(orc, "A", dtname, shape, True))
    s, v = (vectors(orc, "A", dtname, 4096, True, 1, seed)[0] for seed in (9, 10))
    row0 = rk.block_row0(*shape)
    slots = range(8) if variant == "mfree_round_flat" else range(4)
    bad = []

    def model(m, rows):
        if variant == "mfree_round":
            return dm.mfree(m, s, v, row0, rows=rows)
        return dm.mparts(dm.mfree_flat_pieces(m, s, v, rows=rows), s, v, row0, rows=rows)

    clean_of = {}
    clean_dev = rk.run(orc, variant, a, rk.SYCL, row0, s_prev=s, v_prev=v)["s"]
    with np.errstate(over="ignore", invalid="ignore"):
        for row in list(slots) + [1023, 1030]:
            grp = 8 if variant == "mfree_round_flat" else 4
            g0 = row // grp * grp
            # the model: fp32 on every row; fp64 (the integer chain) on the poisoned
            # row's group, the rows outside it against the device's own clean run
            rows = (list(range(shape[0])) if dtname == "float32" else
                    list(range(g0, min(g0 + grp, shape[0]))))
            if rows[0] not in clean_of:
                clean_of[rows[0]] = model(a, rows)
                bad += diff(f"{variant} clean rows {rows[0]} ..", clean_dev[rows],
                            clean_of[rows[0]])
            clean = clean_of[rows[0]]
            outside = np.ones(shape[0], dtype=bool)
            outside[rows] = False
            for col in (5, 4093):
                p = a.copy()
                p[row, col] = poison_value(kind, dt)
                want = clean.copy()
                if kind == "max":
                    want[rows.index(row)] = model(p, [row])[0]
                got = rk.run(orc, variant, p, rk.SYCL, row0, s_prev=s, v_prev=v)["s"]
                name = f"{variant} poison at ({row}, {col})"
                bad += check_poison(name, kind, got[rows], clean, want, rows.index(row))
                bad += diff(f"{name}: rows outside the group", got[outside], clean_dev[outside])
    assert not bad, "\n".join(bad[:12])
