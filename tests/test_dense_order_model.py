"""The host model of the dense summation order (dense_order_model.py), on the
CPU:

1  fma32, the vectorised fp32 fused multiply-add, against csr_order_model.fma
   on the hard cases of test_csr_order_model.py and on 10^5 random triples
2  hand cases: the model on inputs where each step is visible
3  levels: in regime A the model meets the bound exact_sums.levels gives the
   kernels (it is one of the orders that bound admits)
4  power: every wrong order of the list differs from the model in at least 3
   modelled rows, in the regimes A, B and D, for every dtype and every shape
   class it applies to - a condition on the inputs, asserted so that it
   cannot rot.  `identical` says where a wrong order is the right one by
   construction.
"""
import dataclasses
import math

import numpy as np
import pytest

import dense_order_model as dm
import exact_sums as xs
import test_csr_order_model as csr_tests

DTYPES = [pytest.param("float32", id="f32"), pytest.param("float64", id="f64")]
f32 = np.float32


def two(e):
    return math.ldexp(1.0, e)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# 1. fma32
# ---------------------------------------------------------------------------
def test_fma32_on_the_hard_cases():
    for a, x, acc, want in csr_tests.hard_cases(f32):
        got = dm.fma32(np.array([a], f32), np.array([x], f32), np.array([acc], f32))
        ref = dm.fma(f32(a), f32(x), f32(acc), f32)
        assert got.dtype == np.float32 and float(ref) == want
        assert got[0].tobytes() == ref.tobytes(), (a, x, acc, float(got[0]), want)
    # above a tie of fp32 by less than a double sum keeps (test_csr_order_model)
    a, acc = f32(1 + two(-12)), f32(two(-72))
    got = dm.fma32(np.array([a]), np.array([a]), np.array([acc]))
    assert got[0] == f32(1 + two(-11) + two(-23))


def test_fma32_on_random_triples():
    """10^5 triples: exponents over the whole range, accumulators from far
    below the product to far above, subnormal results and overflow."""
    rng = np.random.default_rng(11)
    n = 100000
    with np.errstate(over="ignore", under="ignore"):
        ea = rng.integers(-75, 64, n)
        ex = rng.integers(-75, 64, n)
        ea[-5000:], ex[-5000:] = rng.integers(60, 64, 5000), rng.integers(62, 68, 5000)   # the top
        a = np.ldexp(1 + rng.random(n), ea).astype(f32)
        x = np.ldexp(1 + rng.random(n), ex).astype(f32)
        near = rng.random(n) < 0.7                        # accumulator near the product
        ec = np.where(near, ea + ex + rng.integers(-30, 30, n), rng.integers(-149, 127, n))
        acc = np.ldexp(1 + rng.random(n), np.clip(ec, -160, 127)).astype(f32)
        acc[rng.random(n) < 0.05] = 0
        # ties: a product of two short significands and an accumulator of one bit
        k = n // 10
        a[:k] = np.ldexp(1 + rng.integers(0, 1 << 11, k) / 2048.0, ea[:k]).astype(f32)
        x[:k] = np.ldexp(1 + rng.integers(0, 1 << 12, k) / 4096.0, ex[:k]).astype(f32)
        acc[:k] = np.ldexp(1.0, ea[:k] + ex[:k] - rng.integers(20, 28, k)).astype(f32)
    ok = np.isfinite(a) & np.isfinite(x) & np.isfinite(acc)
    a, x, acc = a[ok], x[ok], acc[ok]
    assert len(a) >= 99000
    got = dm.fma32(a, x, acc)
    ref = np.array([dm.fma(a[i], x[i], acc[i], f32) for i in range(len(a))], dtype=f32)
    bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, [(a[i], x[i], acc[i], got[i], ref[i]) for i in bad[:5]]
    tiny = float(np.finfo(f32).tiny)
    assert ((ref > 0) & (ref < tiny)).sum() >= 100 and np.isinf(ref).sum() >= 100


def test_fma32_passes_non_finite_values_on():
    big = np.finfo(f32).max
    got = dm.fma32(np.array([big, np.inf, np.nan, big], f32), np.array([4, 1, 1, 1], f32),
                   np.array([0, 1, 1, np.inf], f32))
    assert np.isinf(got[0]) and np.isinf(got[1]) and np.isnan(got[2]) and np.isinf(got[3])


# ---------------------------------------------------------------------------
# 2. hand cases
# ---------------------------------------------------------------------------
E = f32(two(-24))          # half an ulp of 1 in fp32: 1 + E is a tie and rounds to 1


def test_one_vector_is_summed_serially():
    """((1 + E) + E) + E = 1, every add a tie to even; pairwise it is 1 + 2E."""
    a = np.array([[1, E, E, E]], dtype=f32)
    assert dm.fused(a)[0] == f32(1)
    assert (f32(1) + E) + (E + E) == f32(1) + 2 * E
    b = np.array([[1, two(-53), two(-53), 0]], dtype=np.float64)     # two vectors of 2
    assert dm.fused(b)[0] == 1.0                          # (1 + e) + (e + 0)


def test_257_vectors_lane_0_takes_a_second_chunk():
    """fp32, 1028 columns: lane 0 holds vectors 0 and 256 and adds hsum(y_256)
    = 2E to its 1 (element by element, 1 + E + E would stay 1); lane 1's E
    then meets 1 + 2E in the tree: a tie, to the even 1 + 4E."""
    a = np.zeros((1, 1028), dtype=f32)
    a[0, 0] = 1
    a[0, 1024:1026] = E
    a[0, 4] = E
    assert dm.fused(a)[0] == f32(1) + 4 * E
    a[0, 4] = 0
    assert dm.fused(a)[0] == f32(1) + 2 * E
    # the same columns ragged (1029: element-wide): lane 0 holds columns 0, 256,
    # 512, 768, 1024: (1 + E) + 0 ... = 1, column 1025 is lane 1's
    b = np.zeros((1, 1029), dtype=f32)
    b[0, 0] = 1
    b[0, 1024:1026] = E
    assert dm.fused(b)[0] == f32(1)                       # (1 + E) = 1, then 1 + E = 1 in the tree


def test_1025_vectors_five_chunks_and_four_waves():
    """fp32, 4100 columns.  Lane 0 adds 5 chunks in order; the wave sums are
    added as ((w0 + w1) + w2) + w3."""
    a = np.zeros((2, 4100), dtype=f32)
    a[0, 0] = 1                                           # lane 0: 1, E, E, E, 2E in chunk order
    for u in (1, 2, 3):
        a[0, u * 1024] = E
    a[0, 4096] = 2 * E
    # serial: 1 + E = 1 three times, then 1 + 2E; backwards it would be 1 + 4E
    assert dm.fused(a)[0] == f32(1) + 2 * E
    # row 1: one element per wave, lanes 0, 64, 128, 192: w = 1, E, E, 2E
    a[1, 0], a[1, 64 * 4], a[1, 128 * 4], a[1, 192 * 4] = 1, E, E, 2 * E
    assert dm.fused(a)[1] == f32(1) + 2 * E               # ((1 + E) + E) + 2E
    assert (f32(1) + E) + (E + 2 * E) == f32(1) + 4 * E   # the pairwise combine differs


def test_the_tree_pairs_neighbours_first():
    """Lanes 0 .. 3 hold 1, E, E, E: the tree adds (1 + E) + (E + E)."""
    a = np.zeros((1, 16), dtype=f32)
    a[0, 0], a[0, 4], a[0, 8], a[0, 12] = 1, E, E, E      # lanes 0 .. 3, one vector each
    assert dm.fused(a)[0] == f32(1) + 2 * E               # serially it would be 1
    b = np.zeros((1, 256), dtype=f32)                     # one value per row of 16 lanes
    b[0, 0], b[0, 64], b[0, 128], b[0, 192] = 1, E, E, E
    assert dm.fused(b)[0] == f32(1) + 2 * E               # (R0 + R1) + (R2 + R3); serially 1
    p = np.zeros((1, 64), dtype=f32)                      # the same through the partials' wave
    p[0, 0], p[0, 16], p[0, 32], p[0, 48] = 1, E, E, E
    assert dm.parts(p)[0] == f32(1) + 2 * E
    assert dm.wave_sum(p[0]) == f32(1) + 2 * E


def test_the_multiply_add_is_fused_and_x_is_rounded_once():
    """257 columns (element-wide): lane 0 holds columns 0 and 256.  (1 + 2^-12)^2
    + 2^-72 lies above a tie that the rounded product sits on.  And with a = 3,
    v = s = 1 + 2^-23: x = 1 + 2^-22 and 3 x = 3 + 3 ulps exactly, where
    fma(3 v, s, 0) with 3 v rounded first gives 3 + 4 ulps."""
    a = np.zeros((2, 257), dtype=f32)
    s, v = np.ones(257, dtype=f32), np.ones(257, dtype=f32)
    a[0, 0], a[0, 256] = two(-72), 1 + two(-12)
    v[256] = 1 + two(-12)
    a[1, 1] = 3
    s[1] = v[1] = 1 + two(-23)
    got = dm.mfree_sum(a, s, v)
    assert got[0] == f32(1 + two(-11) + two(-23))
    assert f32(f32(a[0, 256] * v[256]) + a[0, 0]) == f32(1 + two(-11))
    assert got[1] == f32(3 + 3 * two(-22))
    assert dm.fma32(f32(3) * v[1:2], s[1:2], np.zeros(1, f32))[0] == f32(3 + 4 * two(-22))
    b = a.astype(np.float64)                              # the integer chain, the same cases
    b[0, 0], b[0, 256] = two(-160), 1 + two(-26)
    s64, v64 = np.ones(257), np.ones(257)
    v64[256] = 1 + two(-26)
    s64[1] = v64[1] = 1 + two(-52)
    got = dm.mfree_sum(b, s64, v64)
    assert got[0] == 1 + two(-25) + two(-52) and got[1] == 3 + 3 * two(-51)
    # the division: one IEEE operation by v_prev[r] * s_prev[r] of the block's row
    t32 = dm.mfree_sum(a, s, v)
    assert dm.mfree(a, s, v, row0=0)[1] == t32[1] / (v[1] * s[1])
    assert dm.mfree(a, s, v, row0=1)[0] == t32[0] / (v[1] * s[1])


def test_a_piece_of_one_vector():
    """fp32, 1024 + 4 columns: the second piece is one vector, summed by lane 0
    alone; the first piece is a row of 256 vectors."""
    rng = np.random.default_rng(3)
    a = rng.random((3, 1028)).astype(f32)
    part = dm.flat_pieces(a)
    assert part.shape == (3, 2)
    assert same(part[:, 1], ((a[:, 1024] + a[:, 1025]) + a[:, 1026]) + a[:, 1027])
    assert same(part[:, 0], dm.fused(a[:, :1024]))
    assert same(dm.parts(part), part[:, 0] + part[:, 1])  # lanes 0 and 1, the first tree step


def test_65_partials_lane_0_adds_the_last_one_first():
    """Partials 1, E, 0 ..., 2E (the 65th): lane 0 holds 1 + 2E before the tree
    meets lane 1's E - a tie, to the even 1 + 4E; serially over p, 1 + E = 1 and
    the sum is 1 + 2E."""
    part = np.zeros((1, 65), dtype=f32)
    part[0, 0], part[0, 1], part[0, 64] = 1, E, 2 * E
    assert dm.parts(part)[0] == f32(1) + 4 * E
    assert dm.parts(part[:, :64])[0] == f32(1)
    # k_parts_seg's claim: a row of at most 16 / 32 partials sums as in a whole wave
    p16 = np.random.default_rng(4).random((5, 16)).astype(f32)
    assert same(dm.parts(p16), np.array([dm.tree(r) for r in p16], dtype=f32))


def test_the_split_round():
    """Empty remote side: s = part + 0 = the fused sum.  Empty local side: part
    = 0 and the remote sweep restarts its lanes at q1 = q0.  Local range at
    either end: one remote span."""
    rng = np.random.default_rng(5)
    a = rng.random((4, 4096)).astype(f32)
    part, s = dm.split_round(a, 0, 4096)
    assert same(part, dm.fused(a)) and same(s, part)
    part, s = dm.split_round(a, 1000, 1000)               # q0 = q1 = 250: no multiple of 256
    assert not part.any()
    spans = [dm.strided(dm._vectors(a[:, :1000], 4)), dm.strided(dm._vectors(a[:, 1000:], 4))]
    lanes = dm.lane_adds(np.concatenate(spans, axis=1), dm.ORDER)
    assert same(s, dm.block_sum(lanes))
    part, s = dm.split_round(a, 0, 1000)
    assert same(part, dm.fused(a[:, :1000])) and same(s, part + dm.fused(a[:, 1000:]))
    part, s = dm.split_round(a, 3000, 4096)
    assert same(part, dm.fused(a[:, 3000:])) and same(s, part + dm.fused(a[:, :3000]))
    # one accumulator over both remote spans: lane 0 holds vector 0 of [0, 2) and
    # vectors 4 and 260 of [4, 1024): (1 + E) + E = 1; span by span, 1 + (E + E)
    h = np.zeros((1, 4096), dtype=f32)
    h[0, 0], h[0, 16], h[0, 1040] = 1, E, E
    part, s = dm.split_round(h, 8, 16)
    assert part[0] == 0 and s[0] == f32(1)
    # an unaligned boundary makes the whole round element-wide
    part, s = dm.split_round(a, 1001, 2000)
    assert same(part, dm.sweep(a[:, 1001:2000], 1))


def test_the_split_flat_layout():
    """Local range [1000, 3100) of 4096 columns, pieces of 1024: the local
    launch covers pieces 0 .. 3, k_parts skips piece 1 of the remote buffer
    (wholly local: columns 1024 .. 2047)."""
    w, pc, ppr, p_lo, npl, pa, nfull = dm.split_flat_layout(np.dtype(f32), 4096, 1000, 3100)
    assert (w, pc, ppr, p_lo, npl, pa, nfull) == (4, 1024, 4, 0, 4, 1, 2)
    rng = np.random.default_rng(6)
    a = rng.random((3, 4096)).astype(f32)
    remote, local, s = dm.split_flat(a, 1000, 3100)
    assert not remote[:, 1:3].any() and same(remote[:, 3], dm.fused(
        np.concatenate([np.zeros((3, 3100 - 3072), f32), a[:, 3100:]], axis=1)))
    assert same(s, dm.parts(remote) + dm.parts(local))
    assert dm.split_flat_layout(np.dtype(f32), 4096, 0, 4096)[3:] == (0, 4, 0, 4)
    assert dm.split_flat_layout(np.dtype(f32), 4096, 8, 8)[3:] == (0, 0, 1, 0)


def test_the_half_sweep_takes_8_columns_per_lane():
    """Lane 0 of the 16-bit kernels holds columns 0 .. 7 and 2048 .. 2055; the
    plain row sum is an element-serial chain of adds."""
    a = np.zeros((1, 2056), dtype=f32)
    a[0, 0] = 1
    a[0, 1:8] = E
    assert dm.half_rowsum(a)[0] == f32(1)                 # 1 + E seven times
    a[0, 2048:2050] = 2 * E
    assert dm.half_rowsum(a)[0] == f32(1) + 4 * E
    b = np.zeros((1, 13), dtype=f32)                      # ragged: zeros past the row
    b[0, 0], b[0, 12] = 1, E
    assert dm.half_rowsum(b)[0] == f32(1)                 # lanes 0 and 1: a tie, to even


def test_the_subset_of_rows():
    for n in (5, 16, 37, 257, 1031, 2050):
        rows = dm.subset_rows(n, 1 << 20)
        assert rows == sorted(set(rows)) and rows[0] == 0 and rows[-1] == n - 1
        assert len(rows) <= 64 + 64 * (n > 1000)
        if n > 16:
            for g in (2, 4, 8):
                full = n // g
                want = {0, g - 1, full * g - g, full * g - 1, (full // 2) * g} | \
                    set(range(full * g, n))
                assert want <= set(rows), (n, g)
            assert {0, 1, 2, 3} <= set(rows)
    assert dm.subset_rows(257, 257) == list(range(257))


# ---------------------------------------------------------------------------
# the modelled cases of 3 and 4
# ---------------------------------------------------------------------------
_BASE, _CASE = {}, {}


def base(orc, dtname, shape):
    key = (dtname, shape)
    if key not in _BASE:
        _BASE[key] = orc.generate_c("random", shape[1], xs.SEED, np.dtype(dtname).type,
                                    nrows=shape[0])
    return _BASE[key]


def case(orc, regime, dtname, shape):
    """(a, a of the fma kernels, s, v, row0, rows) of one regime and shape;
    rows: the rows the fp64 fma model runs on (None: all)."""
    key = (regime, dtname, shape)
    if key not in _CASE:
        b = base(orc, dtname, shape)
        a = dm.matrix(regime, dtname, shape, b)
        af = dm.matrix(regime, dtname, shape, b, fma=True) if regime == "C" else a
        s = dm.scale_vector(orc, shape[1], dtname, 9, regime, True)
        v = dm.scale_vector(orc, shape[1], dtname, 10, regime, True)
        row0 = max(0, (shape[1] - shape[0]) // 2) & ~3
        rows = dm.subset_rows(*shape) if dtname == "float64" else None
        _CASE[key] = (a, af, s, v, row0, rows)
    return _CASE[key]


STRUCTURES = ("fused", "flat", "split_round", "split_flat", "mfree", "mfree_flat", "half",
              "half_rowsum")


def modelled(orc, regime, dtname, shape, o=dm.ORDER, parts=dm.parts, split_round=dm.split_round,
             only=STRUCTURES):
    """structure -> the sums (before any division) of one case under the order
    `o`: what the power check compares."""
    nrows, ncols = shape
    if dtname in STORES:
        return modelled_half(orc, regime, dtname, shape, o, only)
    a, af, s, v, row0, rows = case(orc, regime, dtname, shape)
    fits = nrows <= ncols
    out = {}
    for st in only:
        if st == "fused":
            out[st] = dm.fused(a, o)
        elif st == "flat":
            out[st] = parts(dm.flat_pieces(a, o), o)
        elif st == "split_round" and fits:
            out[st] = split_round(a, row0, row0 + nrows, o)[1]
        elif st == "split_flat" and fits:
            remote, local, _ = dm.split_flat(a, row0, row0 + nrows, o)
            pa, nfull = dm.split_flat_layout(a.dtype, ncols, row0, row0 + nrows, o)[5:]
            remote[:, pa:pa + nfull] = 0
            out[st] = parts(remote, o) + parts(local, o)
        elif st == "mfree":
            out[st] = dm.mfree_sum(af, s, v, o, rows=rows)
        elif st == "mfree_flat":
            out[st] = parts(dm.mfree_flat_pieces(af, s, v, o, rows=rows), o)
    return out


STORES = ("float16", "bfloat16")
_HALF = {}


def half_case(orc, regime, store, shape):
    """(the narrowed matrix, s, v) of the 16-bit kernels: dense_order_model's
    half_case, which test_gpu_dense_order.py uploads, and fp32 vectors."""
    key = (regime, store, shape)
    if key not in _HALF:
        a = dm.half_case(regime, store, shape, base(orc, "float32", shape))
        s, v = (dm.scale_vector(orc, shape[1], "float32", seed) for seed in (9, 10))
        _HALF[key] = (a, s, v)
    return _HALF[key]


def modelled_half(orc, regime, store, shape, o, only):
    a, s, v = half_case(orc, regime, store, shape)
    w = o.width("half", shape[1])
    out = {}
    if "half" in only and shape[0] <= shape[1]:
        out["half"] = dm.mfree_sum(a, s, v, o, w=w)
    if "half_rowsum" in only:
        out["half_rowsum"] = dm.mfree_sum(a, np.ones_like(s), np.ones_like(v), o, w=w)
    return out


def half_aware(width):
    """Order.width that also answers for the 16-bit kernels ("half": 8)."""
    return lambda dtype, ncols, *also: dm.HALF_W if isinstance(dtype, str) else width(
        dtype, ncols, *also)


MODEL = dataclasses.replace(dm.ORDER, width=half_aware(xs._vec_width))


@pytest.mark.parametrize("dtname", DTYPES)
def test_the_regimes_are_what_they_say(orc, dtname):
    """B: a background and hot elements far above it, every sum finite.  C:
    elements and sums on both sides of the smallest normal (add-only), products
    below it (fma).  D: most entries zero - whole vectors, lanes and pieces of
    rows 1 .. 3, all of row 4 - and positive scales."""
    dt = np.dtype(dtname)
    tiny = np.finfo(dt).tiny
    for shape in [(1031, 4099), (64, 12288), (8, 65540)]:
        nrows, ncols = shape
        b = dm.matrix("B", dtname, shape, None)
        lo, span, hi = dm.B_RANGE[dtname]
        hot = b >= two(hi - 3)
        assert (b > 0).all() and b.max() < two(hi + 1) and b.min() >= two(lo)
        assert hot.any(axis=1).all() and b[~hot].max() < two(hi - 3)
        per_row = hot.sum(axis=1)
        assert (per_row[np.arange(nrows) % 6 == 0] <= 8).all()     # a vector and its neighbour
        assert np.isfinite(dm.fused(b)).all()
        c = dm.matrix("C", dtname, shape, None)
        sums = dm.fused(c)
        assert ((c > 0) & (c < tiny)).mean() > 0.3 and (c >= tiny).mean() > 0.05
        lanes = dm.lane_adds(dm.strided(dm._vectors(c[:4], 1)), dm.ORDER)
        assert (lanes[1] > 0).all() and (lanes[1] < tiny).all() and (lanes[0] >= tiny).any()
        deep = np.arange(nrows) % 3 == 1
        assert (sums[~deep] >= tiny).all() and (sums[deep] > 0).all()
        assert ncols > 12288 or (sums[deep] < tiny).all()
        cf = dm.matrix("C", dtname, shape, None, fma=True)
        s, v = (dm.scale_vector(orc, ncols, dtname, seed, "C", True) for seed in (9, 10))
        with np.errstate(under="ignore"):
            prod = cf[:4] * (v * s)[None]
        assert (prod < tiny).mean() > 0.8 and (prod > 0).mean() > 0.8
        d = dm.matrix("D", dtname, shape, None)
        assert (d == 0).mean() > 0.8 and not d[4].any() and d[[0, 1, 2, 3, 5]].any(axis=1).all()
        w = 16 // dt.itemsize
        vec = np.pad(d[1], (0, -ncols % w)).reshape(-1, w)
        assert (~vec.any(axis=1)).mean() > 0.5                             # whole vectors
        lane = (np.arange(ncols) // w) % dm.BLOCK
        assert sum(not d[2, lane == l].any() for l in range(dm.BLOCK)) >= 100   # whole lanes
        assert not d[3, :dm.PIECE].any() and d[3, dm.PIECE:2 * dm.PIECE].any()  # whole pieces
        assert dm.matrix("D", dtname, shape, None, zero_row=False)[4].any()
    assert dm.PIECE == xs.piece_cols(dt)
    s = dm.scale_vector(orc, 4099, dtname, 9)
    assert (s >= 0.5).all() and (s < 1.5).all()


# ---------------------------------------------------------------------------
# 3. levels
# ---------------------------------------------------------------------------
def _exact_products(a, x):
    wide = xs._wide(a.dtype) or np.longdouble
    return (a.astype(wide) * x.astype(wide)[None, :a.shape[1]]).sum(axis=1)


@pytest.mark.parametrize("shape", dm.SHAPES, ids=[f"{n}x{c}" for n, c in dm.SHAPES])
@pytest.mark.parametrize("dtname", DTYPES)
def test_the_model_is_within_levels(orc, dtname, shape):
    """Regime A: every structure of the model within exact_sums.levels + 1 ulps
    of the exact sum, per stage for the flat forms."""
    dt = np.dtype(dtname)
    a, af, s, v, row0, rows = case(orc, "A", dtname, shape)
    nrows, ncols = shape
    sel = slice(None) if rows is None else rows
    x = v * s
    exact = xs.exact_rowsum(a)
    seen = {}

    def check(name, got, ex, levels):
        e = float(np.abs(xs.err_ulps_of(got, ex, dt)).max())
        seen[name] = (round(e, 3), levels)
        assert e <= levels + 1, (name, e, levels)

    check("fused", dm.fused(a), exact, xs.levels("rowsum", dt, ncols))
    part = dm.flat_pieces(a)
    pc = xs.piece_cols(dt)
    for p in range(part.shape[1]):
        check(f"piece{p}", part[:, p], xs.exact_rowsum(a[:, p * pc:(p + 1) * pc]),
              xs.levels("rowsum_flat", dt, ncols, "piece"))
    check("parts", dm.parts(part), xs.exact_rowsum(part),
          xs.levels("rowsum_flat", dt, ncols, "parts"))
    check("flat", dm.parts(part), exact, xs.levels("rowsum_flat", dt, ncols))
    if nrows <= ncols:
        c0, c1 = row0, row0 + nrows
        check("split_round", dm.split_round(a, c0, c1)[1], exact,
              xs.levels("split_round", dt, ncols, col0=c0, col1=c1))
        check("split_flat", dm.split_flat(a, c0, c1)[2], exact,
              xs.levels("split_flat_round", dt, ncols, col0=c0, col1=c1))
    ex_x = _exact_products(a, x)[sel]
    check("mfree", dm.mfree_sum(a, s, v, rows=rows), ex_x, xs.levels("mfree_round", dt, ncols))
    mpart = dm.mfree_flat_pieces(a, s, v, rows=rows)
    check("mfree_flat", dm.parts(mpart), ex_x, xs.levels("mfree_round_flat", dt, ncols))
    if dt == np.float32:
        # half_group: mfree's structure with 8 columns per lane and chunk
        lv = xs._sweep_levels(dm.HALF_W, -(-ncols // dm.HALF_W), True)
        check("half", dm.mfree_sum(a, s, v, w=dm.HALF_W), ex_x, lv)
        check("half_rowsum", dm.half_rowsum(a), exact, lv)
    print(dtname, shape, seen)


# ---------------------------------------------------------------------------
# 4. power: the wrong orders
# ---------------------------------------------------------------------------
def tree_last(v):
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def serial_last(v):
    t = v[..., 0]
    for i in range(1, v.shape[-1]):
        t = t + v[..., i]
    return t


def _waves(v):
    return v.reshape(v.shape[:-1] + (-1, dm.WAVE))


# 1 pairwise hsum
def hsum_pairwise(y):
    return tree_last(y)


# 2 element-serial: acc += y[i]
def lane_element_serial(y, o):
    acc = np.zeros((y.shape[0], dm.BLOCK), dtype=y.dtype)
    for u in range(y.shape[1]):
        for i in range(y.shape[3]):
            acc = acc + y[:, u, :, i]
    return acc


# 3 one accumulator per unroll slot (U = 2), combined at the end
def lane_two_slots(y, o):
    acc = dm.lane_adds(y[:, 0::2], o)
    return acc + dm.lane_adds(y[:, 1::2], o) if y.shape[1] > 1 else acc


def lane_fma_two_slots(y, vy, sy, o):
    acc = dm.lane_fmas(y[:, 0::2], vy[0::2], sy[0::2], o)
    return acc + dm.lane_fmas(y[:, 1::2], vy[1::2], sy[1::2], o) if y.shape[1] > 1 else acc


# 4 a lane takes a contiguous run of vectors
def contiguous(v):
    rows, nvec, w = v.shape
    chunks = max(1, -(-nvec // dm.BLOCK))
    y = np.zeros((rows, chunks * dm.BLOCK, w), dtype=v.dtype)
    y[:, :nvec] = v
    return np.ascontiguousarray(y.reshape(rows, dm.BLOCK, chunks, w).transpose(0, 2, 1, 3))


# 5 the lane tree summed serially
def block_serial_tree(v):
    return serial_last(serial_last(_waves(v)))


def wave_serial_tree(v):
    return serial_last(v)


# 6 the last tree step as ((R0 + R1) + R2) + R3
def _wave_rows_serial(v):
    return serial_last(tree_last(v.reshape(v.shape[:-1] + (4, 16))))


def block_last_step(v):
    return serial_last(_wave_rows_serial(_waves(v)))


# 7 the wave combine as (w0 + w1) + (w2 + w3)
def block_pair_combine(v):
    return tree_last(tree_last(_waves(v)))


# 8 the element-wide path where the vector path is meant (the 16-bit kernels:
# k_mfree<float>'s 4 columns per lane where 8 are meant)
def width_other(dtype, ncols, *also):
    return 4 if isinstance(dtype, str) else 1


# 9 multiply, then add
def lane_mul_add(y, vy, sy, o):
    x = vy * sy
    acc = np.zeros((y.shape[0], dm.BLOCK), dtype=y.dtype)
    for u in range(y.shape[1]):
        for i in range(y.shape[3]):
            acc = acc + y[:, u, :, i] * x[None, u, :, i]
    return acc


# 10 x not rounded once: fma(a * v, s, acc), the product a * v rounded instead
def lane_fma_x_folded(y, vy, sy, o):
    if y.dtype == np.float32:
        acc = np.zeros((y.shape[0], dm.BLOCK), dtype=np.float32)
        for u in range(y.shape[1]):
            for i in range(y.shape[3]):
                acc = dm.fma32(y[:, u, :, i] * vy[None, u, :, i], sy[None, u, :, i], acc)
        return acc
    return np.concatenate([dm.chain_lanes(y[r:r + 1] * vy[None], sy) for r in range(y.shape[0])])


# 11 a piece one vector longer
def piece_longer(dtype, w):
    return xs.piece_cols(dtype) + w


# 12 the partials summed serially over p
def parts_serial(part, o):
    return serial_last(np.atleast_2d(part))


# 13 the two spans of the remote half in separate accumulators
def split_round_two_accumulators(a, col0, col1, o):
    w = o.width(a.dtype, a.shape[1], col0, col1)
    v = dm._vectors(a, w)
    q0, q1 = col0 // w, col1 // w
    part = o.block(o.lane(o.layout(v[:, q0:q1]), o))
    lanes = o.lane(o.layout(v[:, :q0]), o) + o.lane(o.layout(v[:, q1:]), o)
    return part, part + o.block(lanes)


# 14 the local part added as a lane value, before the remote tree
def split_round_part_as_lane(a, col0, col1, o):
    w = o.width(a.dtype, a.shape[1], col0, col1)
    v = dm._vectors(a, w)
    q0, q1 = col0 // w, col1 // w
    part = o.block(o.lane(o.layout(v[:, q0:q1]), o))
    lanes = o.lane(np.concatenate([o.layout(v[:, :q0]), o.layout(v[:, q1:])], axis=1), o).copy()
    lanes[:, 0] = lanes[:, 0] + part
    return part, o.block(lanes)


def _order(**kw):
    return dict(o=dataclasses.replace(MODEL, **kw))


ADD = ("fused", "flat", "split_round", "split_flat")
FMA = ("mfree", "mfree_flat", "half")
FLATS = ("flat", "split_flat", "mfree_flat")
WRONG = {                      # name -> (how `modelled` is called, the structures it touches)
    "01-pairwise-hsum": (_order(hsum=hsum_pairwise), ADD),
    "02-element-serial": (_order(lane=lane_element_serial), ADD),
    "03-accumulator-per-slot": (_order(lane=lane_two_slots, lane_fma=lane_fma_two_slots),
                                ADD + FMA + ("half_rowsum",)),
    "04-contiguous-lanes": (_order(layout=contiguous), ADD + FMA + ("half_rowsum",)),
    "05-serial-tree": (_order(block=block_serial_tree, wave=wave_serial_tree),
                       ADD + FMA + ("half_rowsum",)),
    "06-last-tree-step": (_order(block=block_last_step, wave=_wave_rows_serial),
                          ADD + FMA + ("half_rowsum",)),
    "07-pairwise-combine": (_order(block=block_pair_combine), ADD + FMA + ("half_rowsum",)),
    "08-other-width": (_order(width=width_other), ADD + FMA + ("half_rowsum",)),
    "09-multiply-then-add": (_order(lane_fma=lane_mul_add), FMA),
    "10-x-not-rounded-once": (_order(lane_fma=lane_fma_x_folded), FMA),
    "11-piece-one-vector-longer": (_order(piece=piece_longer), FLATS),
    "12-serial-partials": (dict(parts=parts_serial), FLATS),
    "13-remote-two-accumulators": (dict(split_round=split_round_two_accumulators),
                                   ("split_round",)),
    "14-part-as-lane-value": (dict(split_round=split_round_part_as_lane), ("split_round",)),
}

POWER_REGIMES = ("A", "B", "D")
# wrong orders that are the model's own on every shape of a dtype
NOWHERE = {("01-pairwise-hsum", "float64"): "a 16-byte vector holds 2 elements"}


def widths(st, dtname, shape):
    """(W, pieces) of structure `st` on a shape."""
    nrows, ncols = shape
    if st in ("half", "half_rowsum"):
        return dm.HALF_W, 1
    if st in ("split_round", "split_flat"):
        row0 = max(0, (ncols - nrows) // 2) & ~3
        w = xs._vec_width(dtname, ncols, row0, row0 + nrows)
    else:
        w = xs._vec_width(dtname, ncols)
    return w, (-(-ncols // xs.piece_cols(dtname)) if st in FLATS else 1)


def shape_class(st, dtname, shape):
    """The class a shape falls in for a structure: the path a row takes
    (element-wide or vector) and, for the flat forms, whether partials are
    summed at all.  (What only more than 64 partials can show - lane 0's second
    trip - is a hand case above, and regime B's rows of (8, 65540).)"""
    w, ppr = widths(st, dtname, shape)
    path = "8 columns" if w == dm.HALF_W else "element-wide" if w == 1 else "vector"
    if st not in FLATS:
        return path
    return path, "1 piece" if ppr == 1 else "several pieces"


def identical(name, st, dtname, shape):
    """Why the wrong order `name` is the model's own on structure `st` at this
    shape, by construction (None: it can show)."""
    nrows, ncols = shape
    w, ppr = widths(st, dtname, shape)
    nvec = -(-ncols // w)
    vec_chunks = 2 if dtname == "float64" else 1         # chunks of a vector-path piece (kFlatU)
    flat = st in FLATS
    chunks = (4 if w == 1 else vec_chunks) if flat else -(-nvec // dm.BLOCK)
    if flat:
        chunks = min(chunks, -(-nvec // dm.BLOCK))
    if st == "split_round":                               # the remote lanes sweep two spans
        row0 = max(0, (ncols - nrows) // 2) & ~3
        q0, q1 = row0 // w, (row0 + nrows) // w
        chunks = max(-(-(q1 - q0) // dm.BLOCK), -(-q0 // dm.BLOCK) + -(-(nvec - q1) // dm.BLOCK))
    n = name[:2]
    add = st in ADD
    if n == "01" and w <= 2:
        return "a vector of 1 or 2 elements has one association"
    if n == "02" and (w == 1 or chunks == 1):
        return "a vector of one element; or one chunk per lane: ((0 + y0) + y1) + ... is hsum"
    if n == "03" and (chunks == 1 or (add and chunks == 2)):
        return "one chunk per lane; or two of an add-only sweep: h0 + h1 either way"
    if n == "04" and chunks == 1:
        return "one chunk per lane: a run of one vector is the strided vector"
    if n == "05" and nvec <= 2 and ppr <= 2:
        return "at most two lanes hold data"
    if n == "06" and nvec <= 32 and ppr <= 32:
        return "at most two rows of 16 lanes hold data"
    if n == "07" and nvec <= 3 * dm.WAVE:
        return "the fourth wave holds no data: (w0 + w1) + (w2 + 0)"
    if n == "08" and w == 1:
        return ("the element-wide path is meant, and a ragged row has no whole number of "
                "vectors for the reverse")
    if n == "09" and st == "half_rowsum":
        return "x = 1: the product is exact"
    if n == "10" and st == "half_rowsum":
        return "x = 1"
    if n == "11" and ncols <= xs.piece_cols(dtname) + w:
        return "one piece either way"
    if n == "12" and ppr <= 3:
        return "at most 3 partials: (p0 + p1) + (p2 + 0) either way"
    if n == "13":
        row0 = max(0, (ncols - nrows) // 2) & ~3
        if -(-((ncols - row0 - nrows) // w) // dm.BLOCK) < 2 or row0 == 0:
            return "one chunk per lane in the second span, or no first span: h1 + h2 either way"
    return None


_RIGHT = {}


def right_order(orc, regime, dtname, shape, only):
    """The model's own sums of a case, once."""
    out = {}
    for st in only:
        key = (regime, dtname, shape, st)
        if key not in _RIGHT:
            _RIGHT[key] = modelled(orc, regime, dtname, shape, MODEL, only=(st,)).get(st)
        if _RIGHT[key] is not None:
            out[st] = _RIGHT[key]
    return out


# Cells whose input cannot show a wrong order, and why.  Regime A is the
# generator of the other tests and stays as it is: uniform values in [0, 1)
# narrowed to 11 (fp16) or 8 (bf16) significant bits.  rowsum_half adds them in
# fp32, where a lane's 8 .. 264 adds of such values almost never round: the
# lane accumulators are the exact sums in over 98 % of the lanes (checked
# below), and an accumulator per unroll slot regroups exact sums - it changed
# 2 (fp16) and 0 (bf16) rows of 4173.  Regimes B and D show it in the same
# kernel (642 / 184 and 83 / 7 rows), and mfree_round_half in all three.
CANNOT = {
    ("03-accumulator-per-slot", store, "A", "half_rowsum"):
        "a lane's fp32 adds of 16-bit uniform values are exact"
    for store in ("float16", "bfloat16")}


def exact_lane_share(orc, regime, store):
    """The share of rowsum_half's lane accumulators, over all shapes, that
    equal the exact sum of the lane's elements."""
    lanes = exact = 0
    for shape in dm.SHAPES:
        a = half_case(orc, regime, store, shape)[0]
        y = dm.strided(dm._vectors(dm._pad_cols(a, dm.HALF_W), dm.HALF_W))
        got = dm.fma_lanes(y, np.ones(y.shape[1:], dtype=np.float32))
        exact += int((got.astype(np.float64) == y.astype(np.float64).sum(axis=(1, 3))).sum())
        lanes += got.size
    return exact / lanes


HALVES = ("half", "half_rowsum")
POWER = [(name, dtname) for name in WRONG for dtname in ("float32", "float64") + STORES
         if dtname not in STORES or set(WRONG[name][1]) & set(HALVES)]


@pytest.mark.parametrize("name,dtname", POWER, ids=[f"{n}-{d}" for n, d in POWER])
def test_every_wrong_order_shows_in_three_rows(orc, name, dtname):
    """In each of the regimes A, B and D the wrong order changes the bytes of
    at least 3 modelled rows of every structure it touches, in every shape
    class of that structure (`shape_class`) in which some shape can show it;
    where it is the model's own order by construction (`identical`) no byte
    changes.  The shapes and inputs are those the device is compared on: for
    fp16 / bf16 the narrowed matrices of dense_order_model.half_case.  `CANNOT`
    lists the cells whose input cannot show an order, each with a reason that
    is checked."""
    how, touched = WRONG[name]
    shown, skipped, bad = {}, {}, []
    for regime in POWER_REGIMES:
        for shape in dm.SHAPES:
            right = right_order(orc, regime, dtname, shape, touched)
            live = [st for st in right if identical(name, st, dtname, shape) is None]
            wrong = modelled(orc, regime, dtname, shape, **{"o": MODEL, **how}, only=touched)
            for st in right:
                bits = f"u{right[st].dtype.itemsize}"
                differ = int(np.sum(right[st].view(bits) != wrong[st].view(bits)))
                key = (regime, st, shape_class(st, dtname, shape))
                if st in live:
                    shown[key] = shown.get(key, 0) + differ
                else:
                    skipped.setdefault(key, 0)
                    if differ and name[:2] != "11":     # (a longer piece: the last one only)
                        bad.append((key, shape, "not identical", differ))
    print(name, dtname, {k: v for k, v in shown.items()})
    for (regime, st, _), why in [(k, CANNOT.get((name, dtname) + k[:2])) for k in list(shown)]:
        if why is not None:                               # recorded, and its reason checked
            assert exact_lane_share(orc, regime, dtname) > 0.98, why
            del shown[regime, st, _]
    bad += [(k, v) for k, v in shown.items() if v < 3]
    assert (shown or (name, dtname) in NOWHERE) and not bad, bad
