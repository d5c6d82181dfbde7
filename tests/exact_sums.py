"""Row sums against an exact sum, in ulps.

TEST INFRASTRUCTURE (imported by tests/ and tools/rowsum_error.py only).

The stop test compares neighbouring row sums with EPS, and for fp32 sums in
[2048, 4096) EPS = 1e-3f is 4.1 ulps, so the rounding of a row sum decides
when a solve stops.  This module measures that rounding for any computed
row sum s of a STORED fp32 / fp64 matrix:

  exact_rowsum(a)   the true row sums, in a wider type
  err_ulps(s, a)    (s - exact) / ulp(exact), signed, per row
  circulant(...)    matrices whose exact row sums are all one number, so
                    only the summation order differs from row to row
  levels(...)       the number L of rounding additions on the longest path
                    from an element to the row sum, for every summation
                    structure of the library and for the oracle's order

The bound that goes with L: for non-negative data every addition errs by at
most half an ulp of its own partial sum, ulp(p) <= 2u p (u the unit
roundoff), and the partial sums of one level of the structure add up to at
most the row sum S; so a level contributes less than u S < ulp(S) in total
and |s - S| <= L ulp(S).  The tests allow L + 1: the extra ulp covers the
second-order terms and an exact sum that sits next to a binade edge, where
the spacing of the computed sum is twice that of the exact one.
"""
from __future__ import annotations

import math

import numpy as np

NMANT = {np.dtype(np.float32): 23, np.dtype(np.float64): 52}

# nrows x ncols of the step-level cases: small, each crossing one structural
# boundary of the kernels
SHAPES = [
    (5, 3), (37, 1001), (257, 257),          # tails; one piece
    (1031, 4099),                            # element-wide path; 5 pieces, ragged last
    (2050, 4096),                            # vector path; k_round's row groups + remainder
    (512, 6144), (333, 8200), (64, 12288),   # 6 / 9 / 12 pieces: k_parts_seg<16>
    (40, 17000),                             # 17 pieces: k_parts_seg<32>
    (24, 33800),                             # 34 pieces: k_parts, one wave per row
]
SEED = 7                                     # orc.random_matrix seed of those cases

# equal-sum inputs: fp32 circulants whose one row sum S lies in [2048, 4096),
# where EPS = 1e-3f is 4.1 ulps; (8192, seed 2) has S ~ 4099, the next binade
CIRC_CASES = [(n, seed) for n in (4352, 6144, 7000, 8192) for seed in (1, 2)
              if (n, seed) != (8192, 2)]
EPS_F32 = np.float32(1e-3)

# the kernels' workgroup: kBlock lanes in waves of 64 (st_device.h:40-41)
BLOCK = 256
WAVE = 64
WAVES = BLOCK // WAVE


def _wide(dtype):
    """The accumulation type for a matrix dtype, or None for math.fsum."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.float64
    if dtype == np.float64:
        return np.longdouble if np.finfo(np.longdouble).nmant >= 63 else None
    raise TypeError(f"float32 / float64 matrix required, got {dtype}")


def exact_rowsum(a: np.ndarray) -> np.ndarray:
    """Row sums of a stored fp32 / fp64 matrix (or one row), far below one
    ulp of its dtype, returned in the wide type (never rounded back).

    fp32 accumulates in fp64: every add errs by at most 2^-53 relative, so
    the sum is within n 2^-53 of the truth - under 2^-16 of an fp32 ulp for
    n <= 65536.  fp64 accumulates in the 64-bit-significand long double
    (numpy's pairwise order: about log2(n) + 20 roundings of 2^-64 on the
    longest path, under 0.01 fp64 ulp for any n here); where long double is
    no wider than that, math.fsum per row (exact, slow)."""
    a = np.atleast_2d(np.asarray(a))
    wide = _wide(a.dtype)
    if wide is None:
        return np.array([math.fsum(r) for r in a], dtype=np.longdouble)
    if wide is np.longdouble:
        assert np.finfo(np.longdouble).nmant >= 63
    out = np.empty(a.shape[0], dtype=wide)
    step = max(1, (1 << 22) // max(1, a.shape[1]))    # bounded temporaries
    for r in range(0, a.shape[0], step):
        out[r:r + step] = np.ascontiguousarray(a[r:r + step]).astype(wide).sum(axis=1)
    return out


def ulp_of(exact, dtype):
    """Spacing of `dtype` at |exact| (exact in a wide type): 2^(e - nmant) for
    2^e <= |exact| < 2^(e + 1)."""
    x = np.abs(np.asarray(exact))
    _, e = np.frexp(x)                                  # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(np.ones_like(x), e - 1 - NMANT[np.dtype(dtype)])


def err_ulps_of(s, exact, dtype) -> np.ndarray:
    """(s - exact) / ulp(exact) for given exact sums (wide type)."""
    exact = np.asarray(exact)
    d = np.asarray(s).astype(exact.dtype) - exact
    return np.asarray(d / ulp_of(exact, dtype), dtype=np.float64)


def err_ulps(s, a) -> np.ndarray:
    """Signed error per row of the computed row sums `s` of the stored matrix
    `a`, in ulps of a's dtype at the exact sum."""
    a = np.atleast_2d(np.asarray(a))
    return err_ulps_of(np.atleast_1d(s), exact_rowsum(a), a.dtype)


def circulant(n: int, dtype, seed: int, rows=None, orc=None) -> np.ndarray:
    """A[r][c] = x[(c - r) mod n] with x = orc.random_matrix(n, seed, dtype,
    nrows=1)[0]: every row holds the same numbers, rotated, so every exact
    row sum is fsum(x).  `rows` = (row0, nrows) selects the rows row0 ...
    row0 + nrows - 1, taken mod n (a block may run over the last row into
    row 0).  A sliding window over x x: no n x n index array."""
    if orc is None:
        from oracle import oracle as orc
    x = orc.random_matrix(n, seed, dtype, nrows=1)[0]
    row0, nrows = (0, n) if rows is None else rows
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([x, x]), n)
    r = (row0 + np.arange(nrows)) % n
    return np.ascontiguousarray(win[n - r])              # win[i] = (x x)[i : i + n]


def circulant_sum(n: int, dtype, seed: int, orc=None) -> float:
    """The one exact row sum of circulant(n, dtype, seed): fsum(x)."""
    if orc is None:
        from oracle import oracle as orc
    return math.fsum(orc.random_matrix(n, seed, dtype, nrows=1)[0].tolist())


# --------------------------------------------------------------------------
# levels: rounding additions on the longest path, per summation structure
# --------------------------------------------------------------------------
# An addition whose one operand is an exact zero - the first add into a zeroed
# accumulator, a tree step that meets a lane holding 0 - is exact and is not
# counted.

def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


def _tree(active: int, width: int = WAVE) -> int:
    """Levels of the DPP tree over `width` lanes of which the first `active`
    hold data and the rest 0 (wave_sum_l63, st_device.h:120-131: lanes l ^ 1,
    l ^ 2, the quads of a row of 16, its halves, the rows of a half-wave, the
    half-waves - step i joins groups of 2^i neighbouring lanes)."""
    active = min(active, width)
    return 0 if active <= 1 else math.ceil(math.log2(active))


def _wave_combine(active_lanes: int) -> int:
    """Serial add of the workgroup's wave partials in wave order (`t =
    red[0]; t += red[w]`, st_device.h:398-403, 559-563, 1331-1336, 1418-1423,
    1687-1691): the first wave's partial passes one add per further wave
    that holds data."""
    return max(0, min(WAVES, _ceil_div(active_lanes, WAVE)) - 1)


def _vec_width(dtype, ncols: int, *also) -> int:
    """W of the launchers: 16-byte vectors when ncols (and a split round's
    col0 / col1) are whole vectors, else one element (launch_vec,
    st_kernels.hip:443-451; round_dispatch 501-502; launch_round_split
    892-895; launch_round_flat 984-985; launch_rowsum_flat 1560-1561).  The
    tests' tensors are 16-byte aligned."""
    w = 16 // np.dtype(dtype).itemsize
    return w if all(x % w == 0 for x in (ncols, *also)) else 1


def _sweep_levels(w: int, nvec: int, fma: bool) -> int:
    """A workgroup's sum of `nvec` vectors of w elements, lane l taking the
    vectors l, l + 256, ... in column order (k_fused st_device.h:374-386,
    round_group 528-539, mfree_group 1660-1676; the unroll U only groups the
    loads, 121-126 of st_kernels.hip): per lane hsum's w - 1 adds (62-66)
    then one add per further chunk - or, matrix-free, one fused multiply-add
    per element, w * chunks - 1 past the first - then the wave tree and the
    wave combine."""
    if nvec <= 0:
        return 0
    chunks = _ceil_div(nvec, BLOCK)
    lane = (w * chunks - 1) if fma else (w - 1) + (chunks - 1)
    return lane + _tree(nvec) + _wave_combine(nvec)


def piece_cols(dtype, nt: bool = False) -> int:
    """Columns per flat piece, from the library's launch policy
    (st_launch_policy_query's piece_bytes): the cached form's below 2 GiB,
    the non-temporal form's (`nt`) from 2 GiB."""
    from eigen_value_amd import _lib
    dt = "f64" if np.dtype(dtype) == np.float64 else "f32"
    n = 32768 if nt else 8192                            # 8 / 4 GiB; 512 / 256 MiB
    p = _lib.launch_policy(dt, n, n, _lib.ST_FORM_ROUND)
    return int(p["piece_bytes"]) // np.dtype(dtype).itemsize


def pieces_per_row(dtype, ncols: int, nt: bool = False) -> int:
    """ppr (flat_pieces, st_kernels.hip:372-376, called with W * U)."""
    return _ceil_div(ncols, piece_cols(dtype, nt))


def _piece_levels(w: int, cols: int, fma: bool) -> int:
    """One flat piece of `cols` columns (k_flat st_device.h:1283-1337,
    k_flat_sum 1394-1424): lane l holds the vectors l, l + 256, ... of the
    piece, `acc = hsum(y_0)` then `acc + hsum(y_u)` for the piece's further
    chunks (1260, 1306, 1401) - matrix-free, a fused multiply-add per element
    (1286-1295) - then the wave tree (wave_sum_pair / wave_sum_l63: the adds
    of wave_sum, 164-187) and the wave combine."""
    return _sweep_levels(w, _ceil_div(cols, w), fma)


def _parts_levels(ppr: int) -> int:
    """A row's `ppr` piece partials summed by one wave - or a 16 / 32 lane
    segment of one, bitwise the same (k_parts st_device.h:1554-1559,
    k_parts_seg 1505-1511, k_mparts 1468-1472; launch_parts
    st_kernels.hip:350-369): lane l adds the partials l, l + 64, ... in
    order, then the tree over the lanes that hold one."""
    if ppr <= 0:
        return 0
    return (_ceil_div(ppr, WAVE) - 1) + _tree(ppr)


def _oracle_levels(n: int) -> int:
    """numpy's pairwise order as oracle/st_oracle.c restates it (62-94):
    buffers of 8192 elements added to a running result (88-93), a buffer
    halved down to blocks of at most 128 (82-86), a block as 8 interleaved
    chains, their 3-level tree and a serial tail (70-81), fewer than 8
    elements serially (65-69)."""
    def rec(m: int) -> int:
        if m < 8:
            return max(0, m - 1)
        if m <= 128:
            return (m // 8 - 1) + 3 + m % 8
        h = m // 2
        h -= h % 8
        return 1 + max(rec(h), rec(m - h))
    nbuf = _ceil_div(n, 8192)
    return rec(min(n, 8192)) + (nbuf - 1)


FUSED = ("rowsum", "scale_rowsum", "fused_round")            # k_fused, k_round
FLAT = ("rowsum_flat", "flat_round", "flat_round_deferred")  # k_flat_sum / k_flat + k_parts
KERNELS = ("oracle",) + FUSED + ("split_round", "mfree_round") + FLAT + (
    "split_flat_round", "mfree_round_flat")


def levels(kernel: str, dtype, ncols: int, stage: str = "total", *, col0: int = 0,
           col1: int = 0, nt: bool = False) -> int:
    """L for `kernel` (a name of eigen_value_amd.device's step-level calls, or
    "oracle") on rows of `ncols` columns.

    stage (flat forms): "piece" - a piece's partial sum, the longest piece;
    "parts" - the row sum from the stored partials; "total" - both.
    col0 / col1: the local column range of the split rounds.
    nt: the non-temporal flat form of blocks from 2 GiB (another piece size
    for fp64; not reachable at test sizes, tests/test_gpu_fullsize.py runs
    it)."""
    if kernel == "oracle":
        return _oracle_levels(ncols)
    if kernel in FUSED or kernel == "mfree_round":
        w = _vec_width(dtype, ncols)
        return _sweep_levels(w, ncols // w, kernel == "mfree_round")
    if kernel == "split_round":
        # the local half sums the vectors [q0, q1) into part, the remote half
        # the rest - [0, q0) then [q1, nv) in one lane accumulator - and adds
        # `part + t` (round_group, st_device.h:541-548, 564-569); with
        # nothing remote s_next = part + 0 (608-616)
        w = _vec_width(dtype, ncols, col0, col1)
        nv, q0, q1 = ncols // w, col0 // w, col1 // w
        local = _sweep_levels(w, q1 - q0, False)
        if q0 == 0 and q1 == nv:
            return local
        ch = _ceil_div(q0, BLOCK) + _ceil_div(nv - q1, BLOCK)
        act = max(min(q0, BLOCK), min(nv - q1, BLOCK))
        remote = (w - 1) + (ch - 1) + _tree(act) + _wave_combine(act)
        return max(local, remote) + (1 if q1 > q0 else 0)
    pc = piece_cols(dtype, nt)
    ppr = _ceil_div(ncols, pc)
    if kernel in FLAT or kernel == "mfree_round_flat":
        w = _vec_width(dtype, ncols)
        piece = _piece_levels(w, min(pc, ncols), kernel == "mfree_round_flat")
        parts = _parts_levels(ppr)
        return {"piece": piece, "parts": parts, "total": piece + parts}[stage]
    if kernel == "split_flat_round":
        # both halves run k_flat over whole pieces with the lanes of the
        # other half idle (st_device.h:1093-1097, 1264-1266): no piece sums
        # more than a whole one.  k_parts sums the remote launch's partials,
        # then the local launch's, and adds the two (1556-1566;
        # launch_split_flat_cfg, st_kernels.hip:1398-1437)
        w = _vec_width(dtype, ncols, col0, col1)
        piece = _piece_levels(w, min(pc, ncols), False)
        npl = (_ceil_div(col1, pc) - col0 // pc) if col1 > col0 else 0
        parts = max(_parts_levels(ppr), _parts_levels(npl)) + (1 if npl else 0)
        return {"piece": piece, "parts": parts, "total": piece + parts}[stage]
    raise ValueError(f"unknown kernel {kernel!r}")
