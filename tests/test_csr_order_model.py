"""The host model of the CSR summation order (csr_order_model.py), on the CPU:

1  its fma against hard cases and against a second implementation
2  its tree on hand-made inputs whose result depends on the pairing
3  the model itself meets the ulp bound the existing tests ask of the kernel
4  the case set has the rows it promises
5  the power condition: every wrong order we could think of differs from the
   model in at least three rows of every regime and dtype - a condition on
   the inputs (seeds, row counts), asserted so that it cannot rot
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import csr_order_model as om

DTYPES = [pytest.param("float32", id="f32"), pytest.param("float64", id="f64")]


def two(e):
    return math.ldexp(1.0, e)


# ---------------------------------------------------------------------------
# 1. fma
# ---------------------------------------------------------------------------
def hard_cases(dt):
    """(a, x, acc, expected) with p the precision: eps = 2^-p is half an ulp of 1."""
    p, qmin, emax = om.FORMAT[np.dtype(dt)]
    eps, ulp = two(-p), two(1 - p)
    i, j = p // 2, p - p // 2
    big = float(np.finfo(dt).max)
    return [
        # ties go to even
        (1.0, 1.0, eps, 1.0),
        (1.0 + ulp, 1.0, eps, 1.0 + 2 * ulp),
        (eps, 1.0 + ulp, 1.0, 1.0 + ulp),                    # just above the tie
        # the product is not rounded on its own: (1 + 2^-i)(1 + 2^-j), i + j = p, ends in
        # eps: a tie, and an accumulator far below the last place of a double breaks it
        (1.0 + two(-i), 1.0 + two(-j), 0.0, 1.0 + two(-i) + two(-j)),
        (1.0 + two(-i), 1.0 + two(-j), two(-3 * p), 1.0 + two(-i) + two(-j) + ulp),
        # gradual underflow
        (two(qmin + 49), two(-49), 0.0, two(qmin)),           # the smallest subnormal, exact
        (two(qmin + 49), two(-50), 0.0, 0.0),                 # half of it: a tie, to even (0)
        (two(qmin + 49), two(-50), two(qmin), two(qmin + 1)),  # 1.5 -> 2 of them
        (two(qmin + 49), two(-50) + two(-70), 0.0, two(qmin)),  # above the half
        (1.5 * two(qmin + 60), two(-59), two(qmin), 4 * two(qmin)),
        # overflow
        (big, 2.0, 0.0, math.inf),
        (big, 1.0, two(emax - p - 1), math.inf),              # half an ulp of max: to 2^emax
        (big, 1.0, two(emax - p - 2), big),
        # an exact zero somewhere
        (0.0, 3.0, 1.25, 1.25),
        (3.0, 0.0, 0.0, 0.0),
        (1.0 + ulp, 1.0 + ulp, 0.0, 1.0 + 2 * ulp),          # 1 + 2u + u^2 -> 1 + 2u
    ]


@pytest.mark.parametrize("dtname", DTYPES)
def test_fma_hard_cases(dtname):
    dt = np.dtype(dtname).type
    for a, x, acc, want in hard_cases(dt):
        for v in (a, x, acc, want):
            assert float(dt(v)) == v, ("the case is not representable", v)
        got = om.fma(dt(a), dt(x), dt(acc), dt)
        assert got.dtype == np.dtype(dt) and float(got) == want, (a, x, acc, float(got), want)
        # the integer chain rows are summed with: acc enters as the entry acc * 1
        chain = om.lane_sums(np.array([acc, a], dtype=dt), np.array([1.0, x], dtype=dt), dt, 1)[0]
        assert chain.tobytes() == got.tobytes(), (a, x, acc, float(chain), want)


def test_fma_fp32_is_not_a_double_sum_rounded_again():
    """(1 + 2^-12)^2 + 2^-72 = 1 + 2^-11 + 2^-24 + 2^-72: above a tie of fp32.
    A double sum loses the 2^-72, lands on the tie and rounds to even."""
    f = np.float32
    a, acc = f(1 + two(-12)), f(two(-72))
    assert om.fma(a, a, acc, f) == f(1 + two(-11) + two(-23))
    assert f(np.float64(a) * np.float64(a) + np.float64(acc)) == f(1 + two(-11))


@pytest.mark.parametrize("dtname", DTYPES)
def test_the_chain_is_the_fma_on_random_data(dtname):
    """Exponents over the whole range of the type, subnormals and overflow
    included: the integer chain against the Fraction fma, entry by entry."""
    dt = np.dtype(dtname).type
    p, qmin, emax = om.FORMAT[np.dtype(dt)]
    rng = np.random.default_rng(5)
    span = emax - 8
    seen_sub = seen_inf = 0
    for trial in range(300):
        k = int(rng.integers(1, 9))
        center = int(rng.integers(-span, span))
        if trial % 3:                                     # two thirds near the ends of the range
            center = (span + 16 - int(rng.integers(0, 40))) * (1 if trial % 3 == 1 else -1)
        with np.errstate(over="ignore", under="ignore"):
            a = (np.ldexp(rng.random(k), rng.integers(-12, 12, k) + center // 2)).astype(dt)
            x = (np.ldexp(rng.random(k), rng.integers(-12, 12, k) + center - center // 2)).astype(dt)
        if not (np.isfinite(a).all() and np.isfinite(x).all()):
            continue
        acc = dt(0)
        for i in range(k):
            acc = om.fma(a[i], x[i], acc, dt)
        got = om.lane_sums(a, x, dt, 1)[0]
        assert got.tobytes() == acc.tobytes(), (a, x, got, acc)
        seen_sub += 0 < float(acc) < float(np.finfo(dt).tiny)
        seen_inf += math.isinf(float(acc))
    assert seen_sub >= 3 and seen_inf >= 3


# ---------------------------------------------------------------------------
# 2. the tree
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtname", DTYPES)
def test_tree_on_inputs_whose_sum_depends_on_the_pairing(dtname):
    dt = np.dtype(dtname).type
    e = dt(two(-om.FORMAT[np.dtype(dt)][0]))               # half an ulp of 1: 1 + e -> 1
    alive, dead = dt(1) + dt(2) * e, dt(1)

    def at(L, where):
        v = np.zeros(L, dtype=dt)
        for i, val in where.items():
            v[i] = val
        return v

    for L in (4, 16, 64):
        q = L // 4                                       # the four parts of the top two levels
        # the small ones meet each other first: they survive ...
        assert om.tree(at(L, {0: 1, 2 * q: e, 3 * q: e})) == alive
        assert om.tree(at(L, {0: e, q: e, 2 * q: 1})) == alive
        # ... and die when each meets the 1 alone: a pairing by stride (0 with 2, 1 with
        # 3), a rotation the other way ((P3 + P0) + (P1 + P2)) or a serial sum would
        # give the other answer on one of these
        assert om.tree(at(L, {0: 1, q: e, 3 * q: e})) == dead
        assert om.tree(at(L, {0: 1, q: e, 2 * q: e})) == dead
        assert om.tree(at(L, {q: e, 2 * q: e, 3 * q: 1})) == dead
        # inside the lowest level: lanes 0 and 1 are a pair
        assert om.tree(at(L, {0: e, 1: e, 2: 1})) == alive
        assert om.tree(at(L, {0: e, 1: 1, 2: e})) == dead
    # L = 256: the wave sums serially, ((w0 + w1) + w2) + w3
    assert om.combine(at(256, {0: 1, 128: e, 192: e})) == dead      # pairwise: alive
    assert om.combine(at(256, {0: e, 64: e, 128: 1})) == alive
    assert om.combine(at(256, {0: 1, 64: e, 128: e})) == dead
    # and inside a wave the tree
    assert om.combine(at(256, {64: 1, 64 + 32: e, 64 + 48: e})) == alive
    # block_sum (the dots) is the same thing, vectorised
    v = np.random.default_rng(1).random((3, 256)).astype(dt)
    assert all(om.block_sum(v)[i] == om.combine(v[i]) for i in range(3))


@pytest.mark.parametrize("dtname", DTYPES)
def test_row_strides_its_lanes_and_an_empty_row_is_zero(dtname):
    dt = np.dtype(dtname).type
    e = dt(two(-om.FORMAT[np.dtype(dt)][0]))
    assert om.lanes_of(5) == 4 and om.lanes_of(16) == 4 and om.lanes_of(17) == 16
    assert om.lanes_of(2048) == 64 and om.lanes_of(2049) == 256
    # five entries on four lanes: entry 4 follows entry 0 in lane 0, so e, e in entries 0
    # and 4 meet each other before the 1 of entry 1 (a lane of a contiguous block would
    # put entries 0 and 1 together)
    a = np.array([e, 1, 0, 0, e], dtype=dt)
    assert om.row(a, None, dt, ones=True) == dt(1) + dt(2) * e
    assert om.row(np.array([e, e, 0, 0, 1], dtype=dt), None, dt, ones=True) == dt(1)
    assert om.row(np.array([1, e, 0, 0, e], dtype=dt), None, dt, ones=True) == dt(1)
    z = om.row(np.zeros(0, dtype=dt), None, dt, ones=True)
    assert z == 0 and not np.signbit(z)
    # x enters through the fma
    assert om.row(np.array([3], dtype=dt), np.array([0.5], dtype=dt), dt) == dt(1.5)


@pytest.mark.parametrize("dtname", DTYPES)
def test_dot_follows_the_grid(dtname):
    """Lanes, workgroups, and n past one sweep of the grid: lane t of
    workgroup 0 takes elements t and t + G * 256 one after the other, from 0."""
    dt = np.dtype(dtname).type
    e = dt(two(-om.FORMAT[np.dtype(dt)][0]))
    assert om.dot_grid(1) == 1 and om.dot_grid(257) == 2 and om.dot_grid(10 ** 7) == om.DOT_GRID
    for n in (1, 255, 256, 257):
        w = np.random.default_rng(n).random(n).astype(dt)
        exact = om.exact_row(w, w)
        assert om.err_ulps(om.dot(w, w, dt), exact, dt) <= 2 * (1 + 6 + 3) + 1
    w = np.zeros(3 * 256, dtype=dt)
    w[[0, 1, 256]] = [1, e, e]                             # lanes 0, 1 of workgroup 0; lane 0 of 1
    assert om.dot(w, np.ones_like(w), dt) == dt(1)         # (1 + e) in the tree: dies
    w[[0, 1, 256]] = [e, e, 1]
    assert om.dot(w, np.ones_like(w), dt) == dt(1) + dt(2) * e
    assert om.dot(w, None, dt, ones=True) == dt(1) + dt(2) * e
    seam = om.DOT_GRID * 256
    w = np.zeros(seam + 2, dtype=dt)
    w[[0, 1, seam]] = [e, 1, e]                            # e, e in lane 0's chain: 2e survives
    assert om.dot(w, np.ones_like(w), dt) == dt(1) + dt(2) * e
    w[[0, 1, seam]] = [1, e, e]                            # 1 then e in the chain, e beside it
    assert om.dot(w, np.ones_like(w), dt) == dt(1)


# ---------------------------------------------------------------------------
# 3, 4. the case set
# ---------------------------------------------------------------------------
def test_the_structure_has_the_rows_it_promises():
    indptr, indices = om.structure()
    lens = np.diff(indptr)
    n = len(lens)
    nnz_max, lanes = om.class_table()
    assert n >= 300 and len(indices) <= 100_000
    assert lens[0] == 1
    want = {1, 2, 4095, 4096, 4097, 2049}
    for L, u in zip(lanes, om.shape_desc()["unroll"]):
        want |= {L - 1, L, L + 1, u * L - 1, u * L, u * L + 1, 2 * u * L + 1}
    assert want <= set(int(k) for k in lens)
    for m in nnz_max[:-1]:
        assert (lens == m).sum() >= 3 and (lens == m + 1).sum() >= 3
    per_class = np.bincount([lanes.index(om.lanes_of(int(k))) for k in lens], minlength=4)
    assert (per_class >= 12).all(), per_class
    order = [om.lanes_of(int(k)) for k in lens]
    assert sum(a != b for a, b in zip(order, order[1:])) > n // 3      # the classes interleave
    long = int(np.flatnonzero(lens > n)[0])
    cols = indices[indptr[long]:indptr[long + 1]]
    assert len(set(cols.tolist())) < len(cols)                        # duplicates
    unsorted = sum((np.diff(indices[indptr[r]:indptr[r + 1]]) < 0).any() for r in range(n))
    assert unsorted > n // 2


@pytest.mark.parametrize("name", om.REGIMES)
@pytest.mark.parametrize("dtname", DTYPES)
def test_the_regimes_are_what_they_say(dtname, name):
    dt = np.dtype(dtname)
    indptr, indices = om.structure()
    vals, s, v = om.regime(name, dtname)
    mdl = om.model(name, dtname)
    x, tiny = mdl["x"], np.finfo(dt).tiny
    assert vals.dtype == s.dtype == v.dtype == dt
    assert np.isfinite(vals).all() and (vals >= 0).all() and (x > 0).all()
    assert np.isfinite(mdl["sum"]).all() and np.isfinite(mdl["sum0"]).all()
    if name == "A":
        assert x[indices[0]] == 4 and (vals > 0).all() and vals.max() <= 1
    if name == "B":
        _, e = np.frexp(vals)
        assert e.max() - e.min() >= (38 if dt == np.float32 else 390)
    if name == "C":
        prod = vals * x[indices]
        assert ((prod > 0) & (prod < tiny)).mean() > 0.3               # subnormal products
        assert ((mdl["sum"] > 0) & (mdl["sum"] < tiny)).sum() >= 5     # and sums,
        assert (mdl["sum"] >= tiny).sum() >= 100                       # on both sides
        assert ((mdl["sum0"] > 0) & (mdl["sum0"] < tiny)).sum() >= 3   # subnormal entries, K0
    if name == "D":
        assert 0.05 < (vals == 0).mean() < 0.2 and not np.signbit(vals).any()
        zero = [r for r in range(len(s)) if not vals[indptr[r]:indptr[r + 1]].any()]
        assert len(zero) == om.ZERO_ROWS
        assert any(indptr[r + 1] - indptr[r] > 2048 for r in zero)
        for r in zero:
            assert mdl["sum"][r] == 0 and mdl["sum0"][r] == 0 and mdl["sum"][r] / x[r] == 0


@pytest.mark.parametrize("name", om.REGIMES)
@pytest.mark.parametrize("dtname", DTYPES)
def test_the_model_is_within_the_bound_asked_of_the_kernel(dtname, name):
    indptr, indices = om.structure()
    vals, _, _ = om.regime(name, dtname)
    mdl = om.model(name, dtname)
    worst = 0.0
    for r in range(len(indptr) - 1):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        bound = om.bound_ulps(hi - lo)
        e0 = om.err_ulps(mdl["sum0"][r], om.exact_row(vals[lo:hi]), dtname)
        e1 = om.err_ulps(mdl["sum"][r], om.exact_row(vals[lo:hi], mdl["x"][indices[lo:hi]]),
                         dtname)
        assert e0 <= bound and e1 <= bound, (r, hi - lo, e0, e1, bound)
        worst = max(worst, e0 / bound, e1 / bound)
    print(f"{name} {dtname}: the model reaches {worst:.2f} of the bound")


# ---------------------------------------------------------------------------
# 5. the power condition
# ---------------------------------------------------------------------------
FULL_COUNT = False     # True: count every row a mutant shows in (when choosing seeds)


def one_lane(a, x, dt, idx, ones):
    idx = list(idx)
    return om.lane_sums(a[idx], None if ones else x[idx], dt, 1, ones)[0]


def serial(v):
    tot = v[0]
    for s in v[1:]:
        tot = tot + s
    return tot


def mul_add_lanes(a, x, dt, L, ones):
    """A separate multiply and add: two roundings per entry."""
    out = np.zeros(L, dtype=dt)
    p = a if ones else a * x
    for t in range(L):
        acc = out[t]
        for v in p[t::L]:
            acc = acc + v
        out[t] = acc
    return out


def mutants(limits, lanes):
    """name -> (rows it can touch: a predicate on the length k, f(row data) ->
    the row's sum).  Row data: a, x (gathered; None under ones), dt, L, the
    model's lanes, ones, the poison (vals[0], x[col[0]])."""
    SHORT = 300          # the ones that need a new fma pass run on rows up to this length

    def block(a, x, dt, L, lv, ones, e0):
        c = -(-len(a) // L)
        return om.combine(om.lane_sums(a, x, dt, L, ones,
                                       entries=lambda t: range(t * c, min((t + 1) * c, len(a)))))

    def serial_lanes(a, x, dt, L, lv, ones, e0):
        if L <= om.WAVE:
            return serial(lv)
        return serial([serial(lv[i:i + 64]) for i in range(0, L, 64)])

    def mul_add(a, x, dt, L, lv, ones, e0):
        return om.combine(mul_add_lanes(a, x, dt, L, ones))

    def pairwise_waves(a, x, dt, L, lv, ones, e0):
        w = [om.tree(lv[i:i + 64]) for i in range(0, L, 64)]
        return (w[0] + w[1]) + (w[2] + w[3])

    def drop_last(a, x, dt, L, lv, ones, e0):
        k, lv = len(a), lv.copy()
        lv[(k - 1) % L] = one_lane(a, x, dt, range((k - 1) % L, k - 1, L), ones)
        return om.combine(lv)

    def redirected(a, x, dt, L, lv, ones, e0):
        k, lv = len(a), lv.copy()
        t = k % L                                     # the first lane whose next load is past the end
        aa = np.append(a[t::L], e0[0]).astype(dt)
        xx = None if ones else np.append(x[t::L], e0[1]).astype(dt)
        lv[t] = om.lane_sums(aa, xx, dt, 1, ones)[0]
        return om.combine(lv)

    def with_lanes(Lw):
        return lambda a, x, dt, L, lv, ones, e0: om.combine(om.lane_sums(a, x, dt, Lw, ones))

    out = {
        "block striding": (lambda k: 4 < k <= SHORT, block),
        "serial lane sum": (lambda k: k > 2, serial_lanes),
        "multiply then add": (lambda k: k <= SHORT, mul_add),
        "pairwise wave combine": (lambda k: k > limits[2], pairwise_waves),
        "last entry dropped": (lambda k: True, drop_last),
        "one redirected product added": (lambda k: True, redirected),
    }
    for c, m in enumerate(limits[:3]):
        # the limit one lower: a row of m entries goes to the next class; one higher: a row
        # of m + 1 stays in this one
        out[f"class limit {m} - 1"] = (lambda k, m=m: k == m, with_lanes(lanes[c + 1]))
        out[f"class limit {m} + 1"] = (lambda k, m=m: k == m + 1, with_lanes(lanes[c]))
    return out


def shown_rows(name, dtname, seed=om.SEED):
    """mutant -> the rows in which it differs from the model, in K0 (x == 1) or
    in the product with x: the two calls every regime is compared in."""
    dt = np.dtype(dtname)
    indptr, indices = om.structure(seed)
    vals, _, _ = om.regime(name, dtname, seed)
    mdl = om.model(name, dtname, seed)
    limits, lanes = om.class_table()
    lens = np.diff(indptr)
    e0 = (vals[0], mdl["x"][indices[0]])
    shown = {}
    for mname, (touches, f) in mutants(limits, lanes).items():
        rows = set()
        for r in np.flatnonzero([touches(int(k)) for k in lens]):
            lo, hi = int(indptr[r]), int(indptr[r + 1])
            for ones in (True, False):
                if ones and mname == "multiply then add":     # a * 1 is a: nothing to tell
                    continue
                xs = None if ones else mdl["x"][indices[lo:hi]]
                got = f(vals[lo:hi], xs, dt, om.lanes_of(hi - lo),
                        mdl["lanes0" if ones else "lanes"][r], ones, e0)
                if dt.type(got).tobytes() != mdl["sum0" if ones else "sum"][r].tobytes():
                    rows.add(int(r))
            if len(rows) >= 3 and not FULL_COUNT:
                break
        shown[mname] = rows
    return shown


@pytest.mark.parametrize("name", om.REGIMES)
@pytest.mark.parametrize("dtname", DTYPES)
def test_every_wrong_order_shows_in_three_rows(dtname, name):
    """The class-limit mutants touch only rows of one length and the wave
    combine only class 3: their three rows are of that kind by construction.
    Two correct-looking orders of a long row of positive numbers agree in
    three rows of four (both are within half an ulp of the truth), which is why
    the structure holds ten rows at 2048, ten at 2049 and seventeen of class 3."""
    shown = shown_rows(name, dtname)
    print(name, dtname, {k: len(v) for k, v in shown.items()})
    weak = {k: sorted(v) for k, v in shown.items() if len(v) < 3}
    assert not weak, weak


def test_a_fraction_is_rounded_once():
    """round_fraction on its own: a value no product of two floats gives."""
    third = Fraction(1, 3)
    assert om.round_fraction(third, np.float32) == np.float32(1 / 3)
    assert om.round_fraction(third, np.float64) == 1 / 3
    assert om.round_fraction(-third, np.float64) == -1 / 3
    assert om.round_fraction(Fraction(0), np.float32) == 0
