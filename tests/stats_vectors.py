"""Row-sum vectors with a known stop decision and a known maximum.

TEST INFRASTRUCTURE (imported by tests/ only; plain numpy, no device).

Every round kernel folds m_k = max(0, max s_k) and stop_k = all
|s_i - s_{i+1}| < eps into its own sweep of s_k, and in that sweep a pair
(i, i+1) can straddle a vector, a lane, a wave, an unroll step, the
main-loop / tail split, a column piece, a split round's local range or the
cyclic wrap (n-1, 0).  The builders here put the ONE pair that decides the
stop test (or the one element that is the maximum) at a chosen position p,
so that a kernel which drops that pair or that element gives the wrong
answer:

  one_fail    exactly one failing pair, the one starting at p
  all_pass    the same shape with a jump of eps / 2: no pair fails
  exact_eps   a jump of exactly eps = 2^-10 at p ("fail": `<` is strict)
              or one ulp less ("pass")
  max_at      the maximum at p alone (optionally next to a NaN and a
              negative entry, which find_max - it starts at 0 - ignores)
  nan_at      constant with one NaN: the stop test fails, the maximum stands

`positions` lists the boundary positions p for a given chunk width;
`split_rows` turns an fp32 vector into three pieces that a 16-bit storage
format holds exactly and that add up to 1024 times the vector, for the
kernels that sum the rows of a 16-bit matrix themselves.

`eps` is cast to the vector's dtype, as the kernels take it.  The cyclic
forms need n >= 9 (one_fail / all_pass) or n >= 3 (exact_eps); the open
forms need p < n - 1.  tests/test_stats_vectors.py checks every
construction against numpy and the oracle before any kernel sees it.
"""
from __future__ import annotations

import numpy as np

EPS = 1e-3            # the reference's EPS (similarity_transform.hpp:4, main.py:6)
EXACT_EPS = 2.0 ** -10  # exact in fp32 and fp64, with 1 + e and 1 + e / 2

# the sizes the position sweeps use: 9 (one lane), 257 and 1031 (no multiple
# of the vector width: the element-wide path), 1032 / 2056 (one 8 KB fp64 /
# fp32 piece plus 8 columns), 4104 and 8200 (several pieces plus 8 columns)
SIZES = (9, 257, 1031, 1032, 2056, 4104, 8200)


def _ramp(n: int, p: int, dt, jump: float) -> np.ndarray:
    """s[(p+1+j) % n] = 1 + jump (1 - j / (n-1)): up by `jump` at the pair
    starting at p, down by jump / (n-1) at every other pair of the cycle."""
    assert n >= 9 and 0 <= p < n
    j = np.arange(n, dtype=np.float64)
    s = np.empty(n, dtype=dt)
    s[(p + 1 + np.arange(n)) % n] = (1.0 + jump * (1.0 - j / (n - 1))).astype(dt)
    return s


def _step(n: int, p: int, dt, hi) -> np.ndarray:
    assert 0 <= p < n - 1
    s = np.ones(n, dtype=dt)
    s[p + 1:] = hi
    return s


def one_fail(n: int, p: int, dt, eps=EPS, cyclic: bool = True) -> np.ndarray:
    e = float(np.dtype(dt).type(eps))
    return _ramp(n, p, dt, 4.0 * e) if cyclic else _step(n, p, dt, 1.0 + 4.0 * e)


def all_pass(n: int, p: int, dt, eps=EPS, cyclic: bool = True) -> np.ndarray:
    e = float(np.dtype(dt).type(eps))
    return _ramp(n, p, dt, 0.5 * e) if cyclic else _step(n, p, dt, 1.0 + 0.5 * e)


def exact_eps(n: int, p: int, dt, variant: str, cyclic: bool = True) -> np.ndarray:
    """The pair starting at p differs by exactly EXACT_EPS ("fail") or by one
    ulp less ("pass"); pass EXACT_EPS to the kernel as eps.  The cyclic form
    returns to 1 in two exact half steps, at the pair starting at p + n // 2
    and at the pair before p."""
    assert variant in ("fail", "pass")
    T = np.dtype(dt).type
    one, top = T(1), T(1) + T(EXACT_EPS)
    if variant == "pass":
        top = np.nextafter(top, T(0))
    if not cyclic:
        return _step(n, p, dt, top)
    assert n >= 3 and 0 <= p < n
    base = np.empty(n, dtype=dt)          # built for p = 0, then rotated
    base[0] = one
    base[1:n // 2 + 1] = top
    base[n // 2 + 1:] = T(1) + T(EXACT_EPS / 2)
    return np.roll(base, p)


def max_at(n: int, p: int, dt, eps=EPS, decoys: bool = False) -> np.ndarray:
    """1 everywhere, 1 + eps / 4 at p (every pair passes); with `decoys` a
    NaN before p and -7 after it, neither of which may win the maximum."""
    assert 0 <= p < n
    T = np.dtype(dt).type
    s = np.ones(n, dtype=dt)
    s[p] = T(1) + T(eps) / T(4)
    if decoys:
        if p >= 1:
            s[p - 1] = np.nan
        if p + 1 < n:
            s[p + 1] = T(-7)
    return s


def nan_at(n: int, p: int, dt) -> np.ndarray:
    assert 0 <= p < n
    s = np.ones(n, dtype=dt)
    s[p] = np.nan
    return s


def positions(n: int, dt, cyclic: bool = True, nrandom: int = 8, w=None) -> list:
    """Pair positions p to sweep: the vector, lane, wave, workgroup-stride
    (256 lanes), epilogue-block, 8 KB piece, tail and wrap boundaries that
    lie in the valid range (p < n cyclic, p < n - 1 open), and `nrandom`
    seeded ones.  `w` is the number of columns a lane takes per chunk: by
    default one 16-byte vector of `dt`; 8 for the 16-bit-storage kernels,
    whose vectors are fp32 but whose chunk is 8 columns (st_half.h)."""
    if w is None:
        w = 16 // np.dtype(dt).itemsize
    cls = {0, 1, w - 1, w, 2 * w - 1, 63, 64, 64 * w - 1, 64 * w, 255, 256,
           256 * w - 1, 256 * w, 1023, 1024, 2047, 2048, 4095, 4096,
           n - w - 1, n - w, n - 2, n - 1}
    last = n if cyclic else n - 1
    rng = np.random.default_rng(1000003 * n + 2 * w + int(cyclic))
    cls |= {int(x) for x in rng.integers(0, last, size=nrandom)}
    return sorted(p for p in cls if 0 <= p < last)


def split_rows(S: np.ndarray, storage_bits: int):
    """1024 * S (fp32) as three fp32 pieces p0, p1, p2, each exactly
    representable in a 16-bit storage format of `storage_bits` significant
    bits (8: bfloat16, 11: binary16): p0 is 1024 * S truncated to that many
    bits, p1 the remainder truncated likewise, p2 what is left (3 * 8 = 24
    bits cover an fp32 significand).  The pieces are disjoint runs of the
    bits of 1024 * S, so they - and any two of them - add up exactly in fp32
    in any order: a matrix row holding them and zeros has the row sum
    1024 * S bit for bit whatever the kernel's association.  The factor 1024
    (a power of two: comparisons and quotients are unchanged) lifts the last
    bit of an S near 1, 2^-23, to 2^-13 - above binary16's smallest normal
    number 2^-14, so no piece is subnormal.  A NaN goes into p0 alone."""
    assert storage_bits in (8, 11)
    S = np.asarray(S)
    assert S.dtype == np.float32
    keep = np.uint32(0xffffffff ^ ((1 << (24 - storage_bits)) - 1))

    def trunc(x):
        return (x.view(np.uint32) & keep).view(np.float32)

    nan = np.isnan(S)
    t = np.where(nan, np.float32(0), S) * np.float32(1024)
    p0 = trunc(t)
    r = t - p0
    p1 = trunc(r)
    p2 = r - p1
    assert np.array_equal(trunc(p2), p2) and np.array_equal(p0 + r, t)
    return np.where(nan, np.float32(np.nan), p0).astype(np.float32), p1, p2


def failing_pairs(s: np.ndarray, eps, cyclic: bool) -> list:
    """Start indices of the pairs that fail the stop test, computed in s's
    dtype as the kernels and orc_stop do: !(|s_i - s_{i+1}| < eps), so a NaN
    fails."""
    e = s.dtype.type(eps)
    nxt = np.roll(s, -1)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(s - nxt) < e)
    if not cyclic:
        bad = bad[:-1]
    return [int(i) for i in np.nonzero(bad)[0]]


def find_max(s: np.ndarray):
    """max(0, max s) ignoring NaN (find_max starts at 0, cpp:185), in s's dtype."""
    return s.dtype.type(np.fmax.reduce(s, initial=s.dtype.type(0)))
