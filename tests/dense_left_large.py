"""The sizes, the modelled columns and the host-built slabs of the dense
left-vector tests past n = 2049.

TEST INFRASTRUCTURE (numpy; no device).

The rows per block RB and the kind of load are step functions of n, so the
smallest matrices that reach the tall blocks and the non-temporal loads are
large (up to 16388^2, 2 GiB in fp64) and cannot be drawn on the host as
dense_left_order_model.regime draws them.  A column's sum depends on that
column and x only, so a test fills the matrix on the device with values it
never compares, overwrites `cols` with slab(name, dt, n, cols) and gives
the host model the slab.

  facts(dt, n)            what the kernels branch on at this n, from the library
  sizes(dt)               {role: n}: the sizes, derived from the library's
                          table and threshold (nothing retyped)
  model_columns(dt, n)    at most 16 columns: the boundary ones first
  slab(name, dt, n, cols) (slab [n, len(cols)], s [n], v [n]) of one value regime
  unseen(name, dt, n)     the wrong orders that fewer than MIN_COLUMNS of the
                          slab's columns tell from the library's order
  digest(dt, n, value)    the model's expected bytes of a size in one hash

tests/golden/dense_left_large_order.json holds, per (dtype, n), that hash
("order") and the number of the draw each regime's slab is ("draw").  Why a
draw is chosen: sixteen long columns of positive numbers do not always show
every wrong order three times.  The sum's last place lies far above a
product's, so multiply-then-add changes the sum of about one such column in
four, and in the wide-exponent regime a few entries carry the sum, so the
last row or the order inside a block changes few of them.  The draw recorded
is the first whose slab shows every wrong order of dlm.WRONG and every other
value of the table in MIN_COLUMNS columns, in launch 0 and launch 1;
test_dense_left_model.py checks exactly that of the recorded draw, so the file
can claim nothing the test does not verify.

Run as a program it rewrites that file from the built library - after a
change of the table, once the cases that fail are the ones meant to.
"""
from __future__ import annotations

import functools
import hashlib
import json
import math
import os

import numpy as np

import dense_left_order_model as dlm

DTYPES = ("float32", "float64")
COLUMNS = 16                     # modelled columns of one matrix
MIN_COLUMNS = 3                  # columns that must tell a wrong order from the model
PINNED = 3                       # slab columns whose expected bytes the golden file pins
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "dense_left_large_order.json")
ZERO_AT, SUBNORMAL_AT = -2, -1   # slab positions of regime D's / C's special column: the last two


def _code(dtname):
    from eigen_value_amd import _lib
    return _lib.DTYPE_F64 if np.dtype(dtname) == np.float64 else _lib.DTYPE_F32


def facts(dtname, n):
    """What a launch on an aligned n x n matrix of dtname derives from n: rb,
    nrb, last (rows of the last block), w (columns per lane: the library's
    when n is a multiple of it, else 1), strip, nstrips, nt, in_flight."""
    from eigen_value_amd import _lib
    sh = _lib.left_shape(_code(dtname), int(n))
    rb = sh["rows"]
    w = sh["w"] if n % sh["w"] == 0 else 1
    strip = sh["block"] * w
    return {"rb": rb, "nrb": -(-n // rb), "last": n - (-(-n // rb) - 1) * rb, "w": w,
            "strip": strip, "nstrips": -(-n // strip), "nt": sh["nt"],
            "in_flight": sh["rows_in_flight"], "table": sh["rows_table"],
            "from": sh["rows_from"], "combine": sh["combine"], "lanes": sh["w"]}


def first_nt(dtname):
    """The smallest n whose sweeps load non-temporally."""
    from eigen_value_amd import _lib
    sh = _lib.left_shape(_code(dtname), 1)
    elems = (sh["nt_from_mib"] << 20) // np.dtype(dtname).itemsize
    n = math.isqrt(elems - 1) + 1                       # the smallest n with n * n >= elems
    assert facts(dtname, n)["nt"] and not facts(dtname, n - 1)["nt"], (dtname, n)
    return n


def nt_edge(dtname):
    """{(nt, w): n}: the last cached and the first non-temporal size of each
    lane width."""
    from eigen_value_amd import _lib
    w = _lib.left_shape(_code(dtname), 1)["w"]
    n0 = first_nt(dtname)
    below_w = (n0 - 1) // w * w
    below_1 = n0 - 1 if (n0 - 1) % w else n0 - 2
    above_w = -(-n0 // w) * w
    above_1 = n0 if n0 % w else n0 + 1
    return {(False, w): below_w, (False, 1): below_1, (True, 1): above_1, (True, w): above_w}


def short_last_block(dtname, lo):
    """The first size from lo on that is a multiple of every lane width, whose
    last row block is shorter than the rows in flight and whose last strip is
    partial."""
    every_w = max(facts(d, 1)["lanes"] for d in DTYPES)  # the wider lane; the other divides it
    n = -(-(lo + 1) // every_w) * every_w
    while True:
        f = facts(dtname, n)
        if f["w"] > 1 and 0 < n % f["rb"] < f["in_flight"] and n % f["strip"]:
            return n
        n += every_w


STEPS = 3                         # steps of the table (the sizes test holds it to the library's)
ROLES = tuple(f"{what}{i}" for i in range(1, STEPS + 1) for what in ("below", "on", "short")) + \
    ("lanes0", f"odd{STEPS}", "cached_w", "cached_1", "nt_1", "nt_w")


@functools.lru_cache(maxsize=None)
def sizes(dtname):
    """{role: n}, the roles in the order of ROLES - named without the library,
    so that a test module can list its cases before anything is loaded:
    below<i> / on<i>    one below and one on step i of the table
    short<i>            short_last_block of the class that begins there
    lanes0, odd<last>   16-byte lanes in the first class, element-wide in the
                        last (every other class has both from the above)
    cached_w, cached_1, nt_1, nt_w   nt_edge: both sides of the non-temporal
                        threshold in both lane widths"""
    f = facts(dtname, 1)
    assert len(f["from"]) == STEPS + 1, f["from"]
    out = {}
    for i, step in enumerate(f["from"][1:], 1):
        out[f"below{i}"], out[f"on{i}"] = step - 1, step
        out[f"short{i}"] = short_last_block(dtname, step)
    out["lanes0"] = (f["from"][1] - 1) // f["lanes"] * f["lanes"]
    last = f["from"][-1] + 1
    out[f"odd{STEPS}"] = last if last % f["lanes"] else last + 1
    for (nt, w), n in nt_edge(dtname).items():
        out[("nt_" if nt else "cached_") + ("w" if w > 1 else "1")] = n
    assert tuple(out) == ROLES
    return out


def model_columns(dtname, n, limit=COLUMNS, seed=dlm.SEED):
    """The columns a large test models, `limit` at the most: where a lane's
    tail, a strip boundary or the last strip would show, then seeded ones."""
    f = facts(dtname, n)
    w, strip = f["w"], f["strip"]
    edge = [0, w - 1, w, strip - 1, strip, strip + 1, (f["nstrips"] - 1) * strip, n - w - 1,
            n - w, n - 1]
    cols = sorted({c for c in edge if 0 <= c < n})
    rng = np.random.default_rng(seed + n)
    while len(cols) < limit:
        c = int(rng.integers(0, n))
        if c not in cols:
            cols.append(c)
    return sorted(cols)


def _mant(rng, shape_):
    return 1.0 - 0.5 * rng.random(shape_)                 # (0.5, 1]


def _pow2(rng, lo, hi, shape_):
    return np.ldexp(1.0, rng.integers(lo, hi + 1, size=shape_))


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=16)
def slab(name, dtname, n, cols, draw=None, seed=dlm.SEED):
    """(slab [n, k], s_prev [n], v_prev [n]) of one regime in dtype dtname for
    the k = len(cols) columns `cols` (a tuple) of an n x n matrix, read-only
    and a function of (name, dtname, n, k, draw) alone - where the columns go
    does not enter - in the value ranges dense_left_order_model.regime
    documents for A, B, C and D.  C's column of subnormal entries is slab
    column SUBNORMAL_AT and D's all-zero column is slab column ZERO_AT; B's
    last row is at the top of its range of exponents (a few large entries
    carry a column's sum there, and a sweep that stops one row early must
    still show).
    draw None: the one the golden file records for (dtname, n, name)."""
    k = len(cols)
    assert k >= 3 and all(0 <= c < n for c in cols) and len(set(cols)) == k
    if draw is None:
        draw = golden()[str(np.dtype(dtname))][str(n)]["draw"][name]
    dt = np.dtype(dtname)
    f32 = dt == np.float32
    rng = np.random.default_rng([seed, dlm.REGIMES.index(name), 0 if f32 else 1, n, k, draw])
    if name in ("A", "D"):
        S = 1.0 - rng.random((n, k))
        s = 0.5 + 1.5 * rng.random(n)
        v = 0.5 + 1.5 * rng.random(n)
        if name == "D":
            S[rng.random((n, k)) < 0.1] = 0.0
            S[:, ZERO_AT] = 0.0
    elif name == "B":
        lo, hi = (-20, 20) if f32 else (-200, 200)
        S = _pow2(rng, lo, hi, (n, k)) * _mant(rng, (n, k))
        S[n - 1] = np.ldexp(_mant(rng, k), hi)            # see the docstring
        s = _pow2(rng, -5, 5, n) * _mant(rng, n)
        v = _pow2(rng, -5, 5, n) * _mant(rng, n)
    else:
        S = _pow2(rng, *((-100, -80) if f32 else (-1000, -956)), (n, k)) * _mant(rng, (n, k))
        h = -20 if f32 else -30
        s = np.ldexp(0.5 + 1.5 * rng.random(n), h)
        v = np.ldexp(0.5 + 1.5 * rng.random(n), h)
        S[:, SUBNORMAL_AT] = np.ldexp(_mant(rng, n), -140 if f32 else -1040)
    S, s, v = np.ascontiguousarray(S.astype(dt)), s.astype(dt), v.astype(dt)
    for arr in (S, s, v):
        arr.setflags(write=False)
    return S, s, v


def unseen(name, dtname, n, draw=None, model=None):
    """[(launch, rival, columns that differ)] of the rivals that fewer than
    MIN_COLUMNS of the slab's columns tell from the model with the library's
    rows per block: each wrong order of dlm.WRONG (multiply-then-add is launch
    0's own arithmetic and is left out there) and the model run with each
    OTHER value of the table - what an edit of the table would compute.  The
    columns are tried in slab order and a rival is done with once MIN_COLUMNS
    of them differ (the model costs ~1.6 us per row).  model: a dict the
    model's values are left in, {(launch, j): value}."""
    f = facts(dtname, n)
    rb, comb = f["rb"], f["combine"]
    others = [o for o in f["table"] if o != rb]
    assert len(others) == len(f["table"]) - 1
    cols = tuple(model_columns(dtname, n))
    S, s, v = slab(name, dtname, n, cols, draw)
    model = {} if model is None else model
    out = []
    for launch in (1, 0):
        x = v * s if launch else None

        def want(j):
            if (launch, j) not in model:
                model[launch, j] = dlm.column(S[:, j], x, dtname, rb, comb)
            return model[launch, j]

        rivals = [(kind, lambda j, kind=kind: dlm.wrong_column(kind, S[:, j], x, dtname, rb, comb))
                  for kind in dlm.WRONG if launch or kind != "mul_add"]
        rivals += [(f"rows={o}", lambda j, o=o: dlm.column(S[:, j], x, dtname, o, comb))
                   for o in others]
        for tag, rival in rivals:
            differ = 0
            for j in range(len(cols)):
                differ += rival(j).tobytes() != want(j).tobytes()
                if differ >= MIN_COLUMNS:
                    break
            if differ < MIN_COLUMNS:
                out.append((launch, tag, differ))
        for j in range(PINNED):
            want(j)
    return out


def digest(dtname, n, value):
    """sha256 over the model's sums, in the library's order, of the first
    PINNED slab columns of every regime, launch 0 then launch 1;
    value[name][launch, j] as unseen leaves them."""
    h = hashlib.sha256()
    for name in dlm.REGIMES:
        for launch in (0, 1):
            for j in range(PINNED):
                h.update(np.dtype(dtname).type(value[name][launch, j]).tobytes())
    return h.hexdigest()


def choose(dtname, n, limit=64):
    """{"order": the hash, "draw": {regime: the first draw nothing is unseen in}}."""
    draws, value = {}, {}
    for name in dlm.REGIMES:
        for draw in range(limit):
            value[name] = {}
            if not unseen(name, dtname, n, draw, value[name]):
                draws[name] = draw
                break
        else:
            raise RuntimeError(f"no draw below {limit} for {dtname} {n} {name}")
    return {"order": digest(dtname, n, value), "draw": draws}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    doc ={dt: {str(n): choose(dt, n) for n in sorted(set(sizes(dt).values()))}
           for dt in DTYPES}
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", GOLDEN)
