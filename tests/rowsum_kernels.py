"""Drivers of every step-level kernel that computes row sums, for the exact-
sum checks (tests/test_gpu_rowsum_exact.py, tools/rowsum_error.py) and the
byte comparison with the order model (tests/test_gpu_dense_order.py).

TEST INFRASTRUCTURE.  Each driver runs one kernel of eigen_value_amd.device
on a host matrix and returns what the kernel stored and summed:

  stored  the matrix the row sums are sums of (the output matrix of a
          transforming kernel, the input of a read-only one)
  s       the kernel's row sums of it
  part    (flat forms with the layout part[r * ppr + p]) the piece partials,
          shape (nrows, ppr)

`measure` turns that into errors in ulps per stage, next to the oracle's
errors on the same stored matrix.
"""
from __future__ import annotations

import numpy as np
import torch

import exact_sums as xs
from eigen_value_amd import _lib
from eigen_value_amd import device as dev

DEV = "cuda:0"
TD = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}
SYCL, MAINPY = _lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY

# variant -> (the summation structure `exact_sums.levels` knows it by, whether
# it transforms (and so runs under both semantics), whether it needs the row
# block inside the s vector, whether `part` has the flat layout)
VARIANTS = {
    "rowsum": ("rowsum", False, False, False),
    "rowsum_flat": ("rowsum_flat", False, False, True),
    "scale_rowsum": ("scale_rowsum", True, False, False),
    "fused_round": ("fused_round", True, True, False),
    "flat_round": ("flat_round", True, True, True),
    "flat_round_deferred_np0": ("flat_round_deferred", True, True, True),
    "flat_round_deferred_np3": ("flat_round_deferred", True, True, True),
    "split_round": ("split_round", True, True, False),
    "split_flat_round": ("split_flat_round", True, True, False),
    "mfree_round": ("mfree_round", False, True, False),
    "mfree_round_flat": ("mfree_round_flat", False, True, True),
}


def cases():
    """(variant, semantics) pairs: transforming kernels under both."""
    out = []
    for name, (_, transforms, _, _) in VARIANTS.items():
        out += [(name, SYCL), (name, MAINPY)] if transforms else [(name, SYCL)]
    return out


def fits(variant: str, nrows: int, ncols: int) -> bool:
    return nrows <= ncols or not VARIANTS[variant][2]


def block_row0(nrows: int, ncols: int) -> int:
    """Where the step tests put a row block inside the s vector: the middle,
    on a 16-byte boundary."""
    return max(0, (ncols - nrows) // 2) & ~3


def to_np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def scales(orc, n: int, dt, seed: int, unit: bool):
    """A positive scale vector, `random + 0.5` as the step tests use - or all
    ones, which leave the matrix as it is: x * ((1 / 1) * 1) = x."""
    if unit:
        return np.ones(n, dtype=dt)
    return np.ascontiguousarray((orc.random_matrix(n, seed, dt, nrows=1)[0] + dt(0.5)).astype(dt))


HALF = ("rowsum_half", "mfree_round_half")     # on a float16 / bfloat16 torch tensor


def _run_half(variant: str, a, row0: int, s_prev, v_prev):
    """The 16-bit kernels on the torch tensor `a` (float16 / bfloat16, on the
    host): fp32 sums; `stored` is the matrix widened to fp32 (exact)."""
    nrows, ncols = a.shape
    ta = a.contiguous().to(DEV)
    out = dict(part=None, col0=0, col1=0, stored=a.float().numpy())
    if variant == "rowsum_half":
        out["s"] = to_np(dev.rowsum_half(ta))
        return out
    assert row0 + nrows <= ncols
    ones = np.ones(ncols, dtype=np.float32)
    s_next = torch.full((nrows,), -1.0, dtype=torch.float32, device=DEV)
    v_cur = torch.empty(ncols, dtype=torch.float32, device=DEV)
    dev.mfree_round_half(ta, _dev(ones if s_prev is None else s_prev), s_next,
                         _dev(ones if v_prev is None else v_prev), v_cur, dev.new_state(DEV),
                         row0=row0, eps=0.0, k=1, semantics=SYCL)
    out["s"] = to_np(s_next)
    return out


def run(orc, variant: str, a: np.ndarray, sem: int = SYCL, row0: int = 0, unit: bool = False, *,
        s_prev=None, v_prev=None, scale=None, rounds: bool = False):
    """Run `variant` on the host matrix `a` (nrows x ncols) as rows row0 ...
    of the s vector.  Returns dict(stored, s, part, col0, col1).

    scale: the scale vector s_cur instead of `scales(orc, ...)` (the deferred
    variants: the list of their npend + 1 vectors).  s_prev / v_prev: those of
    the matrix-free variants instead of ones.  rounds (deferred variants):
    also s_rounds / part_rounds, every round's s_next and partials, and
    pend_s / pend_inv, the rounds' scales and the reciprocals the device made
    of them.  split_flat_round also returns split_part, its whole scratch (the
    remote partials, then the local ones: device.split_flat_scratch).  The
    variants of HALF take a float16 / bfloat16 torch tensor."""
    if variant in HALF:
        return _run_half(variant, a, row0, s_prev, v_prev)
    dt = a.dtype.type
    tdt = TD[a.dtype]
    nrows, ncols = a.shape
    n_full = max(ncols, row0 + nrows)
    ta = _dev(a)
    s_next = torch.full((nrows,), -1.0, dtype=tdt, device=DEV)
    out = dict(part=None, col0=0, col1=0)
    kw = dict(row0=row0, eps=0.0, semantics=sem)          # eps = 0: no round stops
    if variant == "rowsum":
        s_next = dev.rowsum(ta)
    elif variant == "rowsum_flat":
        part = dev.flat_scratch(nrows, ncols, tdt, DEV)
        dev.rowsum_flat(ta, s_next, part)
        out["part"] = part
    elif variant == "scale_rowsum":
        dev.scale_rowsum(ta, _dev(scales(orc, n_full, dt, 9, unit) if scale is None else scale),
                         s_next, row0=row0, semantics=sem)
    else:
        assert row0 + nrows <= ncols
        deferred = variant.startswith("flat_round_deferred")
        ts = None
        if not deferred:
            ts = _dev(scales(orc, ncols, dt, 9, unit) if scale is None else scale)
        tv = torch.ones(ncols, dtype=tdt, device=DEV)
        state = dev.new_state(DEV)
        if variant == "fused_round":
            dev.fused_round(ta, ts, s_next, tv, state, k=0, **kw)
        elif variant == "flat_round":
            part = dev.flat_scratch(nrows, ncols, tdt, DEV)
            dev.flat_round(ta, ts, s_next, part, tv, state, k=0, **kw)
            out["part"] = part
        elif deferred:
            # as tests/test_gpu_deferred_step.py drives it: `npend` read-only
            # rounds from A_0, then the storing round; ta ends at A_{npend+1}
            npend = int(variant[-1])
            part = dev.flat_scratch(nrows, ncols, tdt, DEV)
            s = [_dev(scales(orc, ncols, dt, 9 + k, unit) if scale is None else scale[k])
                 for k in range(npend + 1)]
            inv = [torch.empty_like(x) for x in s]
            for x, y in zip(s, inv):
                dev.recip(x, y)
            inv_next = torch.empty_like(s_next)
            for k in range(npend + 1):
                dev.flat_round_deferred(ta, s[k], inv[k], s_next, inv_next, part, tv, state,
                                        s[:k], inv[:k], store=k == npend, k=k, **kw)
                if rounds:
                    out.setdefault("s_rounds", []).append(to_np(s_next))
                    out.setdefault("part_rounds", []).append(to_np(part))
            if rounds:
                out.update(pend_s=[to_np(x) for x in s], pend_inv=[to_np(x) for x in inv])
            out["part"] = part
        elif variant in ("split_round", "split_flat_round"):
            col0, col1 = row0, row0 + nrows                # the block's own rows
            out.update(col0=col0, col1=col1)
            if variant == "split_round":
                fn, part = dev.split_round, torch.empty(nrows, dtype=tdt, device=DEV)
            else:
                fn = dev.split_flat_round
                part = dev.split_flat_scratch(nrows, ncols, col0, col1, tdt, DEV)
            fn(ta, ts, None, part, None, state, span=dev.SPAN_LOCAL, col0=col0, col1=col1, k=0,
               **kw)
            fn(ta, ts, s_next, part, tv, state, span=dev.SPAN_REMOTE, col0=col0, col1=col1, k=0,
               **kw)
            if variant == "split_flat_round":              # both partial buffers, as laid out
                out["split_part"] = to_np(part)
        elif variant in ("mfree_round", "mfree_round_flat"):
            # launch k = 1 with s_prev = v_prev = 1: x = v s = 1, every product
            # A_0[r][c] x[c] is exact and s_next = (sum) / 1 a pure row sum of A_0
            # (or the caller's s_prev / v_prev: a rounded x)
            ones = torch.ones(ncols, dtype=tdt, device=DEV)
            tsp = ones if s_prev is None else _dev(s_prev)
            tvp = tv if v_prev is None else _dev(v_prev)
            v_cur = torch.empty_like(ones)
            if variant == "mfree_round":
                dev.mfree_round(ta, tsp, s_next, tvp, v_cur, state, k=1, **kw)
            else:
                part = dev.flat_scratch(nrows, ncols, tdt, DEV)
                dev.mfree_round_flat(ta, tsp, s_next, tvp, v_cur, part, state, k=1, **kw)
                out["part"] = part
        else:
            raise ValueError(variant)
    out["s"] = to_np(s_next)
    out["stored"] = to_np(ta)
    if out["part"] is not None:
        ppr = xs.pieces_per_row(a.dtype, ncols)
        out["part"] = to_np(out["part"])[:nrows * ppr].reshape(nrows, ppr)
        if rounds and "part_rounds" in out:
            out["part_rounds"] = [p[:nrows * ppr].reshape(nrows, ppr) for p in out["part_rounds"]]
    return out


def stats(e) -> dict:
    e = np.asarray(e, dtype=np.float64).ravel()
    return dict(max=float(np.abs(e).max()), rms=float(np.sqrt(np.mean(e * e))),
                mean=float(e.mean()))


def measure(orc, variant: str, a: np.ndarray, sem: int = SYCL, row0: int = 0,
            unit: bool = False) -> dict:
    """Errors in ulps of `variant`'s row sums of the matrix it stored, per
    stage, with each stage's `levels`, and the oracle's errors on the same
    stored matrix: {stage: dict(e, levels)} for stage in total / oracle and,
    for the flat forms, piece / parts."""
    r = run(orc, variant, a, sem, row0, unit)
    base = VARIANTS[variant][0]
    dt, ncols = a.dtype, a.shape[1]
    lv = dict(col0=r["col0"], col1=r["col1"])
    exact = xs.exact_rowsum(r["stored"])
    out = {"total": dict(e=xs.err_ulps_of(r["s"], exact, dt), levels=xs.levels(base, dt, ncols, **lv)),
           "oracle": dict(e=xs.err_ulps_of(orc.rowsum(r["stored"]), exact, dt),
                          levels=xs.levels("oracle", dt, ncols))}
    if r["part"] is not None:
        pc = xs.piece_cols(dt)
        ppr = r["part"].shape[1]
        # (a) every piece partial against the exact sum of that piece of the
        # stored row: lane, chunks, wave tree, wave combine
        ep = np.stack([xs.err_ulps(r["part"][:, p], r["stored"][:, p * pc:(p + 1) * pc])
                       for p in range(ppr)], axis=1)
        out["piece"] = dict(e=ep, levels=xs.levels(base, dt, ncols, "piece"))
        # (b) the row sum against the exact sum of the stored partials
        out["parts"] = dict(e=xs.err_ulps(r["s"], r["part"]),
                            levels=xs.levels(base, dt, ncols, "parts"))
    out["stored"] = r["stored"]
    out["s"] = r["s"]
    return out
