"""A host model of the summation order of the dense kernels, exact to the bit.

TEST INFRASTRUCTURE (numpy only; no device).

exact_sums.py describes the order of every dense row sum in words and counts
its levels.  This module restates that order from the kernels' code
(st_device.h, st_half.h) in IEEE arithmetic, so that a device result can be
compared with tobytes().  One function per structure; each takes the matrix
the kernel summed - the STORED matrix where a kernel transforms - and returns
the sums in the kernel's dtype:

  fused(a)                    k_fused, round_group over the full span
  mfree_sum / mfree           mfree_group; w = 8 on a widened matrix: half_group
  flat_pieces(a)              k_flat, k_flat_sum: part[r][p]
  mfree_flat_pieces           k_flat<MF>
  parts / parts_split         k_parts, k_parts_seg<16|32>, k_mparts
  split_round(a, col0, col1)  round_group local and remote
  split_flat(a, col0, col1)   k_flat<SPLIT 1|2> and k_parts with two buffers

The order, once for all of them.  A workgroup has 256 lanes in 4 waves.  A
row (or a piece of it, or a column range) is cut into vectors of W elements,
W = 16 bytes of elements when every boundary is a whole number of vectors,
else 1; lane l takes the vectors l, l + 256, ... in column order.  Add-only
kernels add a vector's elements serially, ((y0 + y1) + y2) + y3, and add that
to the lane's one accumulator; matrix-free kernels run one fused multiply-add
per element, in column order, against x = v * s rounded once.  Each wave sums
its 64 lanes in the balanced tree over the lane index (pairs, quads, the
quads of a row of 16, the rows), lanes without data holding +0; the four wave
sums are added serially in wave order.  A flat row sum adds its pieces'
partials: lane l of one wave adds the partials l, l + 64, ... in order, then
the same tree.  How many rows share a workgroup, the unroll, the walk order
and the cache policy do not enter.

The add-only structures are plain numpy in the dtype, vectorised over the
rows: numpy's elementwise fp32 / fp64 add is IEEE, subnormals included.  The
fused multiply-add is csr_order_model's exact integer chain for fp64 (slow:
callers model a subset of the rows, `subset_rows`) and, for fp32, `fma32`: the
exact product in fp64, an error-free sum, rounding to odd, rounding to fp32
(test_dense_order_model.py proves it equal to csr_order_model.fma).

Inputs are nonnegative; the sign of a zero is not modelled (every zero is +0).
`Order` holds the steps, so that the tests can swap one for a wrong one.

The second half builds the case set: exact_sums.SHAPES and two more, in four
value regimes.
"""
from __future__ import annotations

import dataclasses
import hashlib

import numpy as np

import exact_sums as xs
from csr_order_model import FORMAT, _chain, _split, _value, block_sum, fma, round_fraction, tree

__all__ = ["fma", "round_fraction", "tree", "block_sum"]     # re-exported for the tests

BLOCK, WAVE = xs.BLOCK, xs.WAVE
HALF_W = 8             # kHalfW: columns per lane and chunk of the 16-bit kernels
F32 = np.dtype(np.float32)


# ---------------------------------------------------------------------------
# the steps
# ---------------------------------------------------------------------------
def strided(v):
    """Vectors v [rows, nvec, w] as the lanes hold them: y [rows, chunks, 256,
    w], lane l of chunk u holding vector u * 256 + l, +0 past the data."""
    rows, nvec, w = v.shape
    chunks = max(1, -(-nvec // BLOCK))
    y = np.zeros((rows, chunks * BLOCK, w), dtype=v.dtype)
    y[:, :nvec] = v
    return y.reshape(rows, chunks, BLOCK, w)


def hsum(y):
    """A vector's elements, serially: ((y0 + y1) + y2) + y3 (last axis)."""
    t = y[..., 0]
    for k in range(1, y.shape[-1]):
        t = t + y[..., k]
    return t


def lane_adds(y, o):
    """The lane accumulators [rows, 256] of an add-only sweep: acc = hsum(y_0),
    then acc + hsum(y_u), chunk by chunk (k_fused starts from 0: 0 + h = h)."""
    h = o.hsum(y)
    acc = h[:, 0]
    for u in range(1, h.shape[1]):
        acc = acc + h[:, u]
    return acc


def fma32(a, x, acc):
    """fp32 a * x + acc with one rounding, elementwise (nonnegative or
    non-finite operands): the product is exact in fp64; the fp64 sum s and its
    exact error (two-sum) give the sum rounded to odd - when inexact, the
    neighbour of the two whose last bit is set; 53 >= 24 + 2 bits, so rounding
    that to fp32 is the single rounding of the exact sum."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(a, dtype=np.float64) * np.asarray(x, dtype=np.float64)
        c = np.asarray(acc, dtype=np.float64)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
        fix = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        # s > 0 here; the exact sum lies on err's side of s
        bits = np.where(fix, np.where(err > 0, bits + 1, bits - 1), bits)
        return bits.view(np.float64).astype(np.float32)


_CHAINS = {}           # chain_lanes' results, by dtype, shapes and a 256-bit digest of the bytes


def _digest(a):
    return hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=32).digest()


def chain_lanes(y, x):
    """fp64 (or fp32) lane accumulators by the exact integer chain: lane l =
    fma chain from 0 over its elements in order (y [rows, chunks, 256, w], x
    [chunks, 256, w])."""
    dt = y.dtype
    rows, chunks, _, w = y.shape
    n = chunks * w
    key = (y.dtype.str, y.shape, x.shape, _digest(y), _digest(x))
    if key in _CHAINS:                                    # the same sweep under another tree
        return _CHAINS[key].copy()
    xm, xe = _split(x.transpose(1, 0, 2).reshape(BLOCK, n))
    out = np.zeros((rows, BLOCK), dtype=dt)
    idx = range(n)
    for r in range(rows):
        yr = y[r].transpose(1, 0, 2).reshape(BLOCK, n)
        am, ae = _split(yr)
        live = yr != 0                                    # fma(0, x, acc) = acc
        for l in np.flatnonzero(live.any(axis=1)):
            sel = idx if live[l].all() else np.flatnonzero(live[l]).tolist()
            out[r, l] = _value(*_chain(am[l], ae[l], xm[l], xe[l], sel, FORMAT[dt]), dt)
    if len(_CHAINS) >= 2048:
        _CHAINS.clear()
    _CHAINS[key] = out.copy()
    return out


def fma_lanes(y, x):
    """Lane accumulators of acc = fma(y, x, acc) over a lane's elements in
    order: fma32 vectorised over rows and lanes, the integer chain for fp64."""
    if y.dtype != F32:
        return chain_lanes(y, x)
    acc = np.zeros((y.shape[0], BLOCK), dtype=np.float32)
    for u in range(y.shape[1]):
        for i in range(y.shape[3]):
            acc = fma32(y[:, u, :, i], x[None, u, :, i], acc)
    return acc


def lane_fmas(y, vy, sy, o):
    """The lane accumulators of a matrix-free sweep: x = v * s rounded once in
    the dtype, one fused multiply-add per element."""
    return fma_lanes(y, vy * sy)


def wave_sum(v):
    """wave_sum of 64 lanes (last axis): block_sum's tree with the other three
    waves at +0, whose sums the serial combine then adds exactly."""
    pad = np.zeros(v.shape[:-1] + (BLOCK - WAVE,), dtype=v.dtype)
    return block_sum(np.concatenate([v, pad], axis=-1))


@dataclasses.dataclass(frozen=True)
class Order:
    """The steps of the order; the tests replace one to get a wrong order."""
    width: object = xs._vec_width     # (dtype, ncols, *also) -> W
    layout: object = strided          # vectors -> lanes
    hsum: object = hsum
    lane: object = lane_adds          # (y, order) -> [rows, 256]
    lane_fma: object = lane_fmas      # (y, vy, sy, order) -> [rows, 256]
    block: object = block_sum         # [.., 256] -> the workgroup's sum
    wave: object = wave_sum           # [.., 64] -> the wave's sum
    piece: object = lambda dtype, w: xs.piece_cols(dtype)   # columns per piece


ORDER = Order()


def _vectors(a, w):
    a = np.atleast_2d(a)
    assert a.shape[1] % w == 0
    return a.reshape(a.shape[0], a.shape[1] // w, w)


# ---------------------------------------------------------------------------
# the structures
# ---------------------------------------------------------------------------
def sweep(a, w, o=ORDER):
    """The workgroup's sum of the columns of a [rows, cols] (cols % w == 0)."""
    return o.block(o.lane(o.layout(_vectors(a, w)), o))


def fused(a, o=ORDER):
    """k_fused (rowsum, scale_rowsum) and round_group over the full span
    (fused_round): the row sums of the stored matrix a."""
    a = np.atleast_2d(a)
    return sweep(a, o.width(a.dtype, a.shape[1]), o)


def _pad_cols(a, w):
    a = np.atleast_2d(a)
    pad = -a.shape[1] % w
    if pad:
        a = np.concatenate([a, np.zeros((a.shape[0], pad), dtype=a.dtype)], axis=1)
    return a


def mfree_sum(a, s_prev, v_prev, o=ORDER, w=None, rows=None):
    """mfree_group's sum of a[r][c] x[c] before the division, for the rows
    `rows` of a (all when None).  w = HALF_W with the 16-bit matrix widened to
    fp32: half_group (columns past the row are zeros of both factors)."""
    a = np.atleast_2d(a)
    ncols = a.shape[1]
    if rows is not None:
        a = a[np.asarray(rows, dtype=np.int64)]
    if w is None:
        w = o.width(a.dtype, ncols)
    y = o.layout(_vectors(_pad_cols(a, w), w))
    vy = o.layout(_vectors(_pad_cols(v_prev[:ncols], w), w))[0]
    sy = o.layout(_vectors(_pad_cols(s_prev[:ncols], w), w))[0]
    return o.block(o.lane_fma(y, vy, sy, o))


def _quotient(t, s_prev, v_prev, row0, nrows, rows):
    r = row0 + (np.arange(nrows) if rows is None else np.asarray(rows, dtype=np.int64))
    with np.errstate(invalid="ignore", divide="ignore"):
        return t / (v_prev[r] * s_prev[r])


def mfree(a, s_prev, v_prev, row0=0, o=ORDER, w=None, rows=None):
    """s_next of mfree_round (mfree_round_half with w = HALF_W): the sum, then
    one IEEE division by v_prev[r] * s_prev[r]."""
    t = mfree_sum(a, s_prev, v_prev, o, w, rows)
    return _quotient(t, s_prev, v_prev, row0, np.atleast_2d(a).shape[0], rows)


def half_rowsum(a, o=ORDER):
    """rowsum_half: half_group with x == 1 - fma(a, 1, acc), an element-serial
    add in fp32 - on the widened matrix."""
    one = np.ones(np.atleast_2d(a).shape[1], dtype=np.float32)
    return mfree_sum(a, one, one, o, HALF_W)


def _pieces(ncols, pc):
    return [(c, min(c + pc, ncols)) for c in range(0, ncols, pc)]


def flat_pieces(a, o=ORDER, w=None):
    """part[r][p] of k_flat / k_flat_sum: every piece of `piece` columns swept
    like a row of its own."""
    a = np.atleast_2d(a)
    if w is None:
        w = o.width(a.dtype, a.shape[1])
    pieces = _pieces(a.shape[1], o.piece(a.dtype, w))
    return np.stack([sweep(a[:, lo:hi], w, o) for lo, hi in pieces], axis=1)


def mfree_flat_pieces(a, s_prev, v_prev, o=ORDER, rows=None):
    """part[r][p] of k_flat<MF>: the fma sweep of every piece."""
    a = np.atleast_2d(a)
    ncols = a.shape[1]
    w = o.width(a.dtype, ncols)
    return np.stack([mfree_sum(a[:, lo:hi], s_prev[lo:hi], v_prev[lo:hi], o, w, rows)
                     for lo, hi in _pieces(ncols, o.piece(a.dtype, w))], axis=1)


def parts(part, o=ORDER):
    """A row's partials [rows, ppr] summed by one wave (k_parts; k_parts_seg
    and k_mparts bitwise the same): lane l adds the partials l, l + 64, ... in
    order, then the tree."""
    part = np.atleast_2d(part)
    rows, ppr = part.shape
    chunks = max(1, -(-ppr // WAVE))
    y = np.zeros((rows, chunks * WAVE), dtype=part.dtype)
    y[:, :ppr] = part
    y = y.reshape(rows, chunks, WAVE)
    acc = y[:, 0]
    for u in range(1, chunks):
        acc = acc + y[:, u]
    return o.wave(acc)


def parts_split(part, skip0, nskip, part2, o=ORDER):
    """k_parts of a split flat round: `part` without [skip0, skip0 + nskip),
    then the second buffer's wave_sum added last."""
    part = np.array(part, copy=True)
    part[:, skip0:skip0 + nskip] = 0                     # not added: + 0 is exact
    return parts(part, o) + parts(part2, o)


def mparts(part, s_prev, v_prev, row0=0, o=ORDER, rows=None):
    """k_mparts: parts, then the division of mfree."""
    part = np.atleast_2d(part)
    return _quotient(parts(part, o), s_prev, v_prev, row0, part.shape[0], rows)


def split_round(a, col0, col1, o=ORDER):
    """(part, s) of round_group's two passes on the stored matrix: local sums
    the vectors [q0, q1) into part; remote sweeps [0, q0) and then [q1, nv)
    into ONE lane accumulator and stores part + t (nothing remote: t = 0)."""
    a = np.atleast_2d(a)
    w = o.width(a.dtype, a.shape[1], col0, col1)
    v = _vectors(a, w)
    q0, q1 = col0 // w, col1 // w
    part = o.block(o.lane(o.layout(v[:, q0:q1]), o))
    y = np.concatenate([o.layout(v[:, :q0]), o.layout(v[:, q1:])], axis=1)
    return part, part + o.block(o.lane(y, o))


def split_flat_layout(dtype, ncols, col0, col1, o=ORDER):
    """launch_split_flat_cfg: (w, pc, ppr, p_lo, npl, pa, nfull) - the local
    launch covers the npl pieces from p_lo; k_parts skips the nfull pieces from
    pa of the remote buffer (those wholly inside [col0, col1))."""
    w = o.width(dtype, ncols, col0, col1)
    pc = o.piece(dtype, w)
    ppr = -(-ncols // pc)
    p_lo = col0 // pc
    npl = -(-col1 // pc) - p_lo if col1 > col0 else 0
    pa = -(-col0 // pc)
    pb = ppr if col1 >= ncols else col1 // pc
    return w, pc, ppr, p_lo, npl, pa, max(pb - pa, 0)


def split_flat(a, col0, col1, o=ORDER):
    """(remote [rows, ppr], local [rows, npl], s) of the split flat round on
    the stored matrix: both launches sum whole pieces with the lanes of the
    other half idle; k_parts adds the remote partials, then the local sum."""
    a = np.atleast_2d(a)
    w, pc, ppr, p_lo, npl, pa, nfull = split_flat_layout(a.dtype, a.shape[1], col0, col1, o)
    rem, loc = a.copy(), np.zeros_like(a)
    rem[:, col0:col1] = 0
    loc[:, col0:col1] = a[:, col0:col1]
    remote = flat_pieces(rem, o, w)
    local = flat_pieces(loc, o, w)[:, p_lo:p_lo + npl]
    return remote, local, parts_split(remote, pa, nfull, local, o)


def scaled(a, s_cur, row0, sem_mainpy, inv=None):
    """The element update of one round on the host, numpy's single IEEE
    operations in the kernel's operand order: a * (inv[r] * s[c]) (the
    reference's order) or (inv[r] * a) * s[c] (main.py's), inv = 1 / s."""
    nrows, ncols = a.shape
    if inv is None:
        inv = a.dtype.type(1) / s_cur
    ir = inv[row0:row0 + nrows, None]
    sc = s_cur[None, :ncols]
    return (ir * a) * sc if sem_mainpy else a * (ir * sc)


# ---------------------------------------------------------------------------
# the case set: shapes, rows to model, value regimes
# ---------------------------------------------------------------------------
# exact_sums.SHAPES, and: more than 64 partials per row (65 pieces of 1024
# columns: the second trip of k_parts' lane 0); a last piece of one vector
# (element-wide, so for both dtypes), and its vector-path neighbour; one piece
# on the vector path, with lanes that hold nothing, and on the element-wide
# path with 4 chunks per lane (exact_sums.SHAPES has neither)
SHAPES = list(xs.SHAPES) + [(8, 65540), (63, 4097), (48, 2052), (192, 1000), (256, 999)]
REGIMES = ("A", "B", "C", "D")


def subset_rows(nrows, ncols=0):
    """The rows the fp64 fma model is run on: for row groups of 2, 4 and 8 the
    first and last row of the first, a middle and the last full group; every
    remainder row; rows 0 .. 3 and the last full group of 8's last four (both
    members of four pairs that share a tree); and rows spread over the block,
    96 of them up to 4100 columns, 24 and fewer on longer rows.  All rows of a
    short or small block."""
    if nrows <= 16 or nrows * ncols <= 1 << 18:
        return list(range(nrows))
    spread = 96 if ncols <= 4100 else max(1, min(24, (1 << 18) // ncols))
    rows = set(range(4)) | set(range(0, nrows, max(1, nrows // spread)))
    for g in (2, 4, 8):
        full = nrows // g
        for grp in (0, full // 2, full - 1):
            rows |= {grp * g, grp * g + g - 1}
        rows |= set(range(full * g, nrows))
    last8 = (nrows // 8 - 1) * 8
    rows |= set(range(last8 + 4, last8 + 8))
    return sorted(rows)


def _rng(regime, dtname, shape, salt=0):
    return np.random.default_rng([REGIMES.index(regime), int(dtname == "float64"), shape[0],
                                  shape[1], salt])


# Regime B, per storage type: (lo, span, hi).  A background of significands in
# [1, 2) times 2^k, k in [lo, lo + span], and in every row a few HOT elements,
# k in [hi - 3, hi], far enough above that their sum exceeds the background's
# at 65540 columns.  With one flat range the few largest elements of a row sit
# at unrelated places and decide every bit of the sum: no order shows.  So
# each row puts its hot elements where ONE level of the order combines them
# (row r: kind r % 6, `_hot_columns`), operands of different magnitude at
# every add; the sixth kind is the flat range.  No partial sum overflows; for
# the 16-bit types every element is a normal number of the storage type.
B_RANGE = {"float32": (-30, 6, 8), "float64": (-60, 6, 8), "float16": (-14, 6, 11),
           "bfloat16": (-30, 6, 8)}
PIECE = 1024           # columns per flat piece of the cached form, both dtypes
# C, add-only kernels: around the smallest normal (2^-126 / 2^-1022), elements
# on both sides of it (and every third row deep below, see `matrix`); 16-bit:
# stored subnormals (fp16 below 2^-14, bf16 below 2^-126)
C_ADD_RANGE = {"float32": (-138, -124), "float64": (-1040, -1020), "float16": (-24, -13),
               "bfloat16": (-133, -122)}
# C, fma kernels: with x = v * s ~ 2^-40 / 2^-60 the products are subnormal
C_FMA_RANGE = {"float32": (-100, -84), "float64": (-1000, -960)}
C_SCALE_EXP = {"float32": -20, "float64": -30}          # s and v of the fma kernels in C


def _wide(rng, shape, lo, hi, dt):
    m = 1.0 + rng.random(shape)
    return np.ldexp(m, rng.integers(lo, hi + 1, size=shape)).astype(dt)


def _hot_columns(rng, kind, ncols, w):
    """The columns of a row's hot elements (vectors of w columns, lane l =
    (column // w) % 256, chunk = column // (256 w), piece = column // 1024):
      0  one vector and its neighbour: the serial hsum, the first tree step
      1  every chunk of one lane: the lane's accumulator
      2  chunk 0 of the 64 lanes of one wave (and its second chunk): the tree
      3  one vector in each wave, in two chunks: the wave combine
      4  the last vector of every piece and the first of the next: the piece
         boundaries, the partials' order"""
    nvec = -(-ncols // w)
    col = np.arange(ncols)
    vec, lane = col // w, (col // w) % BLOCK
    if kind == 0:
        v0 = int(rng.integers(0, max(1, nvec - 1)))
        return (vec == v0) | (vec == v0 + 1)
    if kind == 1:
        return lane == int(rng.integers(0, min(nvec, BLOCK)))
    if kind == 2:
        w0 = int(rng.integers(0, max(1, min(nvec, BLOCK) // WAVE))) * WAVE
        return (lane >= w0) & (lane < w0 + WAVE) & (vec < 2 * BLOCK) & (col % w == 0)
    if kind == 3:
        off = int(rng.integers(0, WAVE))
        return (lane % WAVE == off) & (vec < 2 * BLOCK)
    edge = col % PIECE
    return (edge < w) | (edge >= PIECE - w) | (col >= ncols - w)


def _regime_b(rng, shape, dt, store, w):
    nrows, ncols = shape
    lo, span, hi = B_RANGE[store]
    a = _wide(rng, shape, lo, lo + span, np.float64)
    for r in range(nrows):
        kind = r % 6
        if kind == 5:                                    # the flat range
            a[r] = _wide(rng, ncols, hi - 3 - dt.itemsize * 4, hi, np.float64)
        else:
            hot = _hot_columns(rng, kind, ncols, w)
            a[r, hot] = _wide(rng, int(hot.sum()), hi - 3, hi, np.float64)
    return a.astype(dt)


def matrix(regime, dtname, shape, base, *, fma=False, zero_row=True, store=None, w=None):
    """The input matrix of one regime.  base: regime A's matrix (the library's
    random generator, uniform in [0, 1)).  fma: regime C
    for a kernel that multiplies by x (subnormal products, not elements).
    store: the 16-bit storage type's name, whose ranges B and C then fit.
    w: the vector width the hot elements of B are laid out for (the dtype's
    path on this row length; 8 for the 16-bit kernels).
    Returns fp32 / fp64; the caller narrows for the 16-bit kernels."""
    dt = np.dtype(dtname)
    nrows, ncols = shape
    rng = _rng(regime, dtname, shape)
    if regime == "A":
        return np.array(base, dtype=dt)
    if regime == "B":
        if w is None:
            w = HALF_W if store else xs._vec_width(dt, ncols)
        return _regime_b(rng, shape, dt, store or dtname, w)
    if regime == "C":
        rngs = C_ADD_RANGE[store or dtname] if (store or not fma) else C_FMA_RANGE[dtname]
        with np.errstate(under="ignore"):
            a = _wide(rng, shape, *rngs, np.float64)
            if not store and not fma:
                # every third row from the smallest subnormal up: lane sums, wave
                # sums and (up to some 4000 columns) row sums stay subnormal
                qmin = FORMAT[dt][1]
                deep = np.arange(nrows) % 3 == 1
                a[deep] = _wide(rng, (int(deep.sum()), ncols), qmin, qmin + 9, np.float64)
            return a.astype(dt)
    # D: B's values (an order shows in few rows of thinned uniform data) with
    # most of them zeroed: 9 of 10 background elements, a tenth of the hot ones
    if w is None:
        w = HALF_W if store else xs._vec_width(dt, ncols)
    a = _regime_b(rng, shape, dt, store or dtname, w)
    hot = a >= np.ldexp(1.0, B_RANGE[store or dtname][2] - 3)
    a[rng.random(shape) < np.where(hot, 0.1, 0.9)] = 0
    wv = 16 // dt.itemsize
    pc = PIECE
    col = np.arange(ncols)
    if nrows > 1:                                        # whole vectors
        a[1, np.repeat(rng.random(-(-ncols // wv)) < 0.5, wv)[:ncols]] = 0
    if nrows > 2:                                        # whole lanes
        a[2, np.isin((col // wv) % BLOCK, rng.choice(BLOCK, 100, replace=False))] = 0
    if nrows > 3:                                        # whole pieces, the first included
        a[3, (col // pc) % 2 == 0] = 0
    if nrows > 4 and zero_row:
        a[4] = 0
    return a


def narrow(a, store):
    """fp32 values rounded to nearest even into the 16-bit storage type and
    widened again (exact): what the 16-bit kernels sum.  Finite input."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if store == "float16":
        with np.errstate(under="ignore"):
            return a.astype(np.float16).astype(np.float32)
    assert store == "bfloat16"
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def half_case(regime, store, shape, base):
    """The matrix of the 16-bit kernels in one regime, as fp32 values that the
    storage type holds exactly: regime's values fitted to `store`, hot elements
    laid out for 8 columns per lane, narrowed.  The GPU tests and the power
    check share it."""
    return narrow(matrix(regime, "float32", shape, base, store=store, w=HALF_W), store)


def scale_vector(orc, n, dtname, seed, regime="A", fma=False):
    """A scale vector as the step tests make it, `random + 0.5` (the oracle's
    generator); for the fma kernels in regime C times 2^-20 / 2^-30, so that
    x = v * s is near 2^-40 / 2^-60."""
    dt = np.dtype(dtname).type
    s = (orc.random_matrix(n, seed, dt, nrows=1)[0] + dt(0.5)).astype(dt)
    if regime == "C" and fma:
        s = np.ldexp(s, C_SCALE_EXP[dtname]).astype(dt)
    return np.ascontiguousarray(s)
