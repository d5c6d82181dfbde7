"""CPU: the premises tests/test_gpu_rowsum_exact.py rests on.

  * exact_rowsum is exact (math.fsum per row), wide exponent spreads included;
  * the oracle's numpy-pairwise row sums obey their own `levels` bound on
    every shape the GPU tests use;
  * the fp32 circulants of exact_sums.CIRC_CASES have their one row sum S in
    [2048, 4096) - EPS = 1e-3f is then 4.1 ulps - the oracle's row sums of
    them spread over at most 2 ulps (under half of EPS), and the oracle's
    solve stops in round 0 under both semantics;
  * circulant row blocks have equal exact sums, fsum(x).

If one of these breaks, this file fails; no GPU test is relaxed for it.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_sums as xs

DTYPES = [np.float32, np.float64]


def fsum_rows(a):
    return [math.fsum(r.tolist()) for r in np.atleast_2d(a)]


def as_exact(x):
    """A wide-type value as (hi, lo) doubles: long double -> two doubles is
    exact for a 64-bit significand."""
    hi = np.float64(x)
    return float(hi), float(np.float64(x - np.longdouble(hi)))


@pytest.mark.parametrize("dt", DTYPES)
def test_exact_rowsum_is_fsum(orc, dt):
    rng = np.random.default_rng(20261020)
    cases = [orc.random_matrix(1001, 3, dt, nrows=7),
             orc.random_matrix(3, 4, dt, nrows=5),
             orc.random_matrix(8200, 5, dt, nrows=3),
             # wide exponent spread: 2^-40 ... 2^40, and a few huge terms
             # among many tiny ones
             (rng.random((6, 4099)) * np.exp2(rng.integers(-40, 41, (6, 4099)))).astype(dt),
             np.concatenate([np.full((2, 5000), 1e-7), np.full((2, 3), 1e7),
                             np.full((2, 5000), 3e-8)], axis=1).astype(dt)]
    nm = xs.NMANT[np.dtype(dt)]
    for a in cases:
        got = xs.exact_rowsum(a)
        assert got.dtype != np.dtype(dt) and got.shape == (a.shape[0],)
        for g, want, row in zip(got, fsum_rows(a), a):
            hi, lo = as_exact(g)
            # the true sum as a rational; math.fsum is its correctly rounded
            # double, and exact_rowsum must lie within 2^-16 (fp32 rows) /
            # 2^-6 (fp64 rows) of an ulp of the dtype from it
            truth = sum((Fraction(v) for v in row.tolist()), Fraction(0))
            assert float(truth) == want
            err = abs(Fraction(hi) + Fraction(lo) - truth)
            ulp = Fraction(2) ** (math.frexp(want)[1] - 1 - nm)
            assert err <= ulp / (2 ** 16 if dt == np.float32 else 2 ** 6)
    # err_ulps: a sum one spacing above / below the exact one is +-1
    a = np.array([[1.0, 2.0, 4.0], [0.5, 0.25, 0.125]], dtype=dt)
    s = a.sum(axis=1)
    assert np.array_equal(xs.err_ulps(s, a), [0.0, 0.0])
    assert np.array_equal(xs.err_ulps(np.nextafter(s, dt(np.inf)), a), [1.0, 1.0])
    assert np.array_equal(xs.err_ulps(np.nextafter(s, dt(0)), a), [-1.0, -1.0])


def test_levels_formulas():
    """The oracle's order and the kernels' stages, by hand."""
    L = xs._oracle_levels
    assert [L(n) for n in (1, 3, 7, 8, 9, 128)] == [0, 2, 6, 3, 4, 18]
    assert L(129) == 1 + max(L(64), L(65)) and L(8192) == 6 + L(128)
    assert L(8200) == L(8192) + 1 and L(33800) == L(8192) + 4
    # k_fused, 4096 fp32 columns: hsum 3, 4 chunks per lane, 6 tree levels, 3 waves
    assert xs.levels("rowsum", np.float32, 4096) == 3 + 3 + 6 + 3
    assert xs.levels("fused_round", np.float64, 4096) == 1 + 7 + 6 + 3
    assert xs.levels("rowsum", np.float32, 3) == 2          # 3 lanes of one wave
    assert xs.levels("mfree_round", np.float32, 4096) == 15 + 6 + 3
    assert xs.levels("split_round", np.float32, 4096, col0=0, col1=4096) == 15
    assert xs.levels("split_round", np.float32, 4096, col0=1024, col1=3072) == 3 + 1 + 9 + 1


def test_flat_levels_follow_the_policy():
    """The flat forms' pieces come from st_launch_policy_query (a host-side
    call): 1024 columns for both dtypes in the cached form."""
    for dt in DTYPES:
        pc = xs.piece_cols(dt)
        assert pc == 1024 and xs.pieces_per_row(dt, 4099) == 5
        assert [xs.pieces_per_row(dt, n) for n in (6144, 8200, 12288, 17000, 33800)] == \
            [6, 9, 12, 17, 34]
    assert xs.piece_cols(np.float64, nt=True) == 512
    # fp32 vector path: hsum 3, one chunk, tree 6, 3 waves; 6 pieces: 3 tree levels
    assert xs.levels("flat_round", np.float32, 6144, "piece") == 3 + 0 + 9
    assert xs.levels("flat_round", np.float32, 6144, "parts") == 3
    assert xs.levels("flat_round", np.float32, 6144) == 15
    # fp64: two chunks of 2-wide vectors; element-wide: 4 chunks
    assert xs.levels("rowsum_flat", np.float64, 6144, "piece") == 1 + 1 + 9
    assert xs.levels("rowsum_flat", np.float32, 4099, "piece") == 0 + 3 + 9
    assert xs.levels("rowsum_flat", np.float32, 33800, "parts") == 6
    assert xs.levels("rowsum_flat", np.float32, 17000, "parts") == 5
    assert xs.levels("mfree_round_flat", np.float32, 6144, "piece") == 3 + 9
    assert xs.levels("split_flat_round", np.float32, 6144, "parts", col0=1000, col1=3000) == 3 + 1


@pytest.mark.parametrize("dt", DTYPES)
def test_oracle_within_its_levels(orc, dt):
    """|e| <= levels + 1 ulps for the oracle's row sums on every shape of the
    GPU tests (the bound the kernels are held to, applied to the reference)."""
    for nrows, ncols in xs.SHAPES:
        a = orc.generate_c("random", ncols, xs.SEED, dt, nrows=nrows)
        e = xs.err_ulps(orc.rowsum(a), a)
        bound = xs.levels("oracle", dt, ncols) + 1
        print(f"oracle {np.dtype(dt).name} {nrows}x{ncols}: max|e| {np.abs(e).max():.3f} "
              f"rms {np.sqrt(np.mean(e * e)):.3f} bound {bound}")
        assert np.abs(e).max() <= bound, (nrows, ncols)


@pytest.mark.parametrize("n,seed", xs.CIRC_CASES)
def test_circulant_premises(orc, n, seed):
    dt = np.float32
    S = xs.circulant_sum(n, dt, seed, orc)
    assert 2048.0 <= S < 4096.0, S
    ulp = math.ldexp(1.0, 11 - 23)
    assert abs(float(xs.EPS_F32) / ulp - 4.1) < 0.01           # EPS = 1e-3f is 4.10 ulps
    a = xs.circulant(n, dt, seed, orc=orc)
    x = a[0]
    assert a.shape == (n, n) and a[1, 0] == x[-1] and a[n - 1, 0] == x[1]
    assert np.array_equal(a[5], np.roll(x, 5))
    s0 = orc.rowsum(a)
    e = xs.err_ulps_of(s0, np.full(n, S), dt)
    spread = e.max() - e.min()
    print(f"circulant {n} seed {seed}: S {S!r} oracle e in [{e.min():.3f}, {e.max():.3f}]")
    assert spread <= 2.0, spread
    assert np.abs(e).max() <= xs.levels("oracle", dt, n) + 1
    for sem, count in ((orc.SEM_SYCL, 0), (orc.SEM_MAINPY, 1)):
        r = orc.similarity_transform(a, sem, trace=True)
        assert (r.iter_count, r.rounds_evaluated) == (count, 1), (sem, r.iter_count)
        assert np.array_equal(r.row_sums[0], s0) and r.eigen_val == s0[0]


@pytest.mark.parametrize("dt", DTYPES)
def test_circulant_blocks_have_equal_sums(orc, dt):
    for n, seed in ((257, 1), (4099, 2), (6144, 1)):
        x = orc.random_matrix(n, seed, dt, nrows=1)[0]
        S = math.fsum(x.tolist())
        assert xs.circulant_sum(n, dt, seed, orc) == S
        for row0, nrows in ((0, 3), (n // 2, 64), (n - 20, 40)):   # the last wraps to row 0
            b = xs.circulant(n, dt, seed, rows=(row0, nrows), orc=orc)
            assert b.shape == (nrows, n) and b.dtype == np.dtype(dt)
            for i, row in enumerate(b):
                assert np.array_equal(row, np.roll(x, (row0 + i) % n))
            assert fsum_rows(b) == [S] * nrows
            assert np.abs(xs.err_ulps_of(xs.exact_rowsum(b).astype(np.float64),
                                         np.full(nrows, S), dt)).max() < 2.0 ** -9
