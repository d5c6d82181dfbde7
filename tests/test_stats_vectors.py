"""tests/stats_vectors.py does what it says (CPU; numpy and the oracle).

The position sweeps on the GPU (test_gpu_stats_positions.py) are only as good
as their inputs: a vector meant to have ONE failing pair at p that has two,
or none, would let a kernel drop that pair unnoticed.  So every construction
is checked here at every size, dtype, semantics and position the sweeps use -
with a lane's chunk one 16-byte vector of the dtype, and 8 columns for the
16-bit-storage kernels - : the failing pairs in plain numpy (in the vector's
dtype) and the decision and the maximum through the oracle's orc_stop /
orc_find_max.  split_rows, which turns such a vector into the three diagonals
of a 16-bit matrix whose row sums are that vector times 1024 bit for bit, is
proved on the same vectors.
"""
import itertools

import numpy as np
import pytest

import stats_vectors as sv

HALF_W = 8                   # columns per lane and chunk of half_group (st_half.h)
BIG = 16400                  # the non-temporal shape of the half sweep
HALF_SOLVE_N = (9, 257, 1032, 2056)      # test_gpu_stats_positions.test_solve_half


def constructions(orc, dt, cyclic, n, w=None):
    eps, ee = dt(sv.EPS), dt(sv.EXACT_EPS)
    pos = sv.positions(n, dt, cyclic, w=w)
    assert pos and pos[0] == 0 and pos[-1] == (n - 1 if cyclic else n - 2)
    for p in pos:
        s = sv.one_fail(n, p, dt, eps, cyclic)
        assert s.dtype == dt and s.shape == (n,)
        assert sv.failing_pairs(s, eps, cyclic) == [p]
        assert not orc.stop(s, eps, cyclic)
        s = sv.all_pass(n, p, dt, eps, cyclic)
        assert sv.failing_pairs(s, eps, cyclic) == []
        assert orc.stop(s, eps, cyclic)
        s = sv.exact_eps(n, p, dt, "fail", cyclic)
        assert s.dtype == dt and abs(s[p] - s[(p + 1) % n]) == ee
        assert sv.failing_pairs(s, ee, cyclic) == [p]
        assert not orc.stop(s, ee, cyclic)
        s = sv.exact_eps(n, p, dt, "pass", cyclic)
        assert abs(s[p] - s[(p + 1) % n]) == np.nextafter(dt(1) + ee, dt(0)) - dt(1)
        assert sv.failing_pairs(s, ee, cyclic) == []
        assert orc.stop(s, ee, cyclic)
    # the maximum and the NaN sit on an element, not a pair: every index class
    for p in sv.positions(n, dt, True, w=w):
        s = sv.max_at(n, p, dt, eps)
        assert s[p] > 1 and np.count_nonzero(s != 1) == 1
        assert orc.find_max(s) == s[p] == sv.find_max(s) == s.max()
        assert orc.stop(s, eps, cyclic) and sv.failing_pairs(s, eps, cyclic) == []
        s = sv.max_at(n, p, dt, eps, decoys=True)
        assert orc.find_max(s) == s[p] == sv.find_max(s)
        assert np.isnan(s).sum() == (p >= 1) and (s == -7).sum() == (p + 1 < n)
        assert not orc.stop(s, eps, cyclic)           # -7 or the NaN fails a pair
        s = sv.nan_at(n, p, dt)
        assert np.isnan(s[p]) and np.isnan(s).sum() == 1
        assert orc.find_max(s) == 1 == sv.find_max(s)
        assert not orc.stop(s, eps, cyclic) and sv.failing_pairs(s, eps, cyclic)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("cyclic", [True, False])
@pytest.mark.parametrize("n", sv.SIZES)
def test_constructions(orc, dt, cyclic, n):
    constructions(orc, dt, cyclic, n)


@pytest.mark.parametrize("cyclic", [True, False])
@pytest.mark.parametrize("n", sv.SIZES + (BIG,))
def test_constructions_chunks_of_8(orc, cyclic, n):
    """The positions of the 16-bit-storage sweeps: fp32 vectors, 8 columns
    per lane and chunk."""
    constructions(orc, np.float32, cyclic, n, w=HALF_W)


def positions_before_w(n, dt, cyclic=True, nrandom=8):
    """The rule of `positions` as it stood before it took `w`, verbatim."""
    w = 16 // np.dtype(dt).itemsize
    cls = {0, 1, w - 1, w, 2 * w - 1, 63, 64, 64 * w - 1, 64 * w, 255, 256,
           256 * w - 1, 256 * w, 1023, 1024, 2047, 2048, 4095, 4096,
           n - w - 1, n - w, n - 2, n - 1}
    last = n if cyclic else n - 1
    rng = np.random.default_rng(1000003 * n + 2 * w + int(cyclic))
    cls |= {int(x) for x in rng.integers(0, last, size=nrandom)}
    return sorted(p for p in cls if 0 <= p < last)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("cyclic", [True, False])
@pytest.mark.parametrize("n", sv.SIZES)
def test_default_positions_are_unchanged(dt, cyclic, n):
    """Without `w` the sweeps merged earlier get the positions they got."""
    assert sv.positions(n, dt, cyclic) == positions_before_w(n, dt, cyclic)
    assert sv.positions(n, dt, cyclic, nrandom=0) == positions_before_w(n, dt, cyclic, 0)
    assert sv.positions(n, dt, cyclic, w=16 // np.dtype(dt).itemsize) == \
        positions_before_w(n, dt, cyclic)


def test_positions_hold_every_boundary_class():
    """Both sides of each boundary, where the size reaches it."""
    for dt, w in ((np.float64, 2), (np.float32, 4)):
        pos = set(sv.positions(8200, dt, True))
        for b in (w, 64, 64 * w, 256, 256 * w, 1024, 2048, 4096, 8200 - w):
            assert {b - 1, b} <= pos, (dt, b)
        assert {0, 1, 8198, 8199} <= pos
        assert 8199 not in sv.positions(8200, dt, False)       # open: no wrap pair
        assert set(sv.positions(9, dt, True)) >= {0, 1, w - 1, w, 7, 8}
        assert sv.positions(8200, dt, True) == sv.positions(8200, dt, True)   # seeded
    # half_group: a chunk is 8 columns, a wave 512, a workgroup pass 2048, the
    # unrolled stride 4096; the ragged / last chunk starts at n - 8
    pos = set(sv.positions(8200, np.float32, True, w=HALF_W))
    for b in (8, 512, 2048, 4096, 8200 - 8):
        assert {b - 1, b} <= pos, b
    assert {0, 1, 8198, 8199} <= pos
    for n in sv.SIZES + (BIG,):
        pos = set(sv.positions(n, np.float32, True, w=HALF_W))
        want = {0, 1, 7, 8, 15, 511, 512, 2047, 2048, 4095, 4096, n - 9, n - 8, n - 2, n - 1}
        assert {p for p in want if 0 <= p < n} <= pos, n
        assert n - 1 not in sv.positions(n, np.float32, False, w=HALF_W)


# ---------------------------------------------------------------------------
# split_rows: three storable pieces that add up to 1024 * s in any order
# ---------------------------------------------------------------------------
def half_vectors(n, cyclic):
    """Every vector test_solve_half makes a matrix of (fp32, chunks of 8)."""
    dt = np.float32
    eps = dt(sv.EPS)
    out = []
    for p in sv.positions(n, dt, cyclic, w=HALF_W):
        out += [sv.one_fail(n, p, dt, eps, cyclic), sv.all_pass(n, p, dt, eps, cyclic),
                sv.exact_eps(n, p, dt, "fail", cyclic), sv.exact_eps(n, p, dt, "pass", cyclic)]
    for p in sv.positions(n, dt, True, w=HALF_W):
        out += [sv.max_at(n, p, dt, eps), sv.max_at(n, p, dt, eps, decoys=True),
                sv.nan_at(n, p, dt)]
    return np.stack(out)


def same_bits(a, b):
    """Equal as numbers (so +0 == -0), NaN where and only where the other is."""
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("bits,name", [(11, "float16"), (8, "bfloat16")])
@pytest.mark.parametrize("cyclic", [True, False])
@pytest.mark.parametrize("n", HALF_SOLVE_N)
def test_split_rows(n, cyclic, bits, name):
    torch = pytest.importorskip("torch")
    S = half_vectors(n, cyclic)
    pieces = sv.split_rows(S, bits)
    want = S * np.float32(1024)
    assert same_bits(want / np.float32(1024), S)              # the scaling is exact
    assert all(p.dtype == np.float32 and p.shape == S.shape for p in pieces)
    nan = np.isnan(S)
    assert nan.any() and np.array_equal(np.isnan(pieces[0]), nan)
    assert not np.isnan(pieces[1]).any() and not np.isnan(pieces[2]).any()
    assert not pieces[1][nan].any() and not pieces[2][nan].any()
    with np.errstate(invalid="ignore"):
        for a, b, c in itertools.permutations(pieces):        # all six orders, fp32
            t = a + b
            assert t.dtype == np.float32
            assert same_bits(t + c, want)
    tdt = getattr(torch, name)
    for p in pieces:                                          # storable as it is
        back = torch.from_numpy(p).to(tdt).to(torch.float32).numpy()
        assert same_bits(back, p)
        if bits == 11:                                        # no binary16 subnormal
            mag = np.abs(p[~np.isnan(p)])
            assert np.all((mag == 0) | (mag >= 2.0 ** -14))
    # not vacuous: the lower pieces are in use
    assert pieces[1].any() and (pieces[2].any() or bits == 11)


def test_split_rows_truncates_to_the_storage_width():
    s = np.array([1 + 2.0 ** -23, 1.0, -7.0, 1 + 2.0 ** -10 + 2.0 ** -20], np.float32)
    p0, p1, p2 = sv.split_rows(s, 8)
    assert p0.tolist() == [1024.0, 1024.0, -7168.0, 1024.0]
    assert p1.tolist() == [2.0 ** -13, 0.0, 0.0, 1.0]
    assert p2.tolist() == [0.0, 0.0, 0.0, 2.0 ** -10]
    p0, p1, p2 = sv.split_rows(s, 11)
    assert p0.tolist() == [1024.0, 1024.0, -7168.0, 1025.0]
    assert p1.tolist() == [2.0 ** -13, 0.0, 0.0, 2.0 ** -10]
    assert not p2.any()
