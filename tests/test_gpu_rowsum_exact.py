"""GPU: the row sums of every kernel against an exact sum, in ulps.

The row sum decides when a solve stops: for fp32 sums in [2048, 4096)
EPS = 1e-3f is 4.1 ulps.  The other tests hold a kernel's row sums to the
same-precision oracle at 2e-6 / 1e-13 relative (17-34 fp32 ulps, 450-900
fp64 ulps); here every step-level kernel that sums rows is measured against
the exact sums (tests/exact_sums.py) of the matrix it actually stored or
read, per stage:

  1. hard bound: |e| <= levels + 1 ulps for every row, kernel, shape, dtype
     and stage (levels: the rounding additions on the longest path, written
     from the kernels' code in exact_sums.levels);
  2. no wider than the reference: over all rows of all shapes, max|e_gpu| <=
     max|e_oracle| + 1 ulp, the oracle summing the same stored matrix.  The
     1 is one step of the grid computed sums live on - two faithful sums of
     one row can land on neighbouring numbers - not a measured allowance;
  3. equal-sum inputs: on row blocks of circulant matrices (every exact row
     sum is the same number, only the order of the terms differs) the
     spread max e - min e over the rows is at most the oracle's + 1 ulp.
     MEASURED: 62 of the 648 cases miss it, each with a spread of 3 ulps
     on a block where the oracle's happens to be 1 (KNOWN_WIDER below,
     expected failures, strict);
  4. the consequence: fp32 circulant solves with S in [2048, 4096), where
     the oracle stops in round 0 (tests/test_exact_sums.py), stop in round 0
     through the drop-in and the device solver in every form, with lambda
     within levels + 1 ulps of S.  No straddle rule applies: the exact row
     sums are equal, so a solve that runs on is carried by its own rounding
     spread alone.

The flat forms' split rounds keep their partials in another layout (remote
pieces, then the local range's); they are checked on the row sums only.
The one-launch small and batched kernels expose no row sums and are tied
bit for bit to k_round by their own tests.  Seeds and shapes are fixed: a
failing case is a finding, not a reason to pick another seed.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import eigen_value_amd as ev  # noqa: E402
import exact_sums as xs  # noqa: E402
import rowsum_kernels as rk  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402

DTYPES = [np.float32, np.float64]
CASES = rk.cases()
CASE_IDS = [f"{v}-sem{s}" for v, s in CASES]
STAGES = ("total", "piece", "parts")

_INPUT, _MEASURED, _BLOCK = {}, {}, {}


def random_input(orc, dt, shape):
    """orc.random_matrix of the shape (the C generator: the same bits), once."""
    key = (np.dtype(dt).name, shape)
    if key not in _INPUT:
        _INPUT[key] = orc.generate_c("random", shape[1], xs.SEED, dt, nrows=shape[0])
        _INPUT[key].setflags(write=False)
    return _INPUT[key]


def measured(orc, variant, sem, dt, shape):
    """Errors per stage of one (kernel, semantics, dtype, shape), once; the
    stored matrix is dropped."""
    key = (variant, sem, np.dtype(dt).name, shape)
    if key not in _MEASURED:
        nrows, ncols = shape
        row0 = rk.block_row0(nrows, ncols) if rk.VARIANTS[variant][2] else 0
        m = rk.measure(orc, variant, random_input(orc, dt, shape), sem, row0)
        _MEASURED[key] = {k: v for k, v in m.items() if k not in ("stored", "s")}
    return _MEASURED[key]


# a call that needs the row block inside the s vector keeps the shapes with
# nrows <= ncols
BOUND_CASES = [(v, s, shape) for v, s in CASES for shape in xs.SHAPES if rk.fits(v, *shape)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("variant,sem,shape", BOUND_CASES,
                         ids=[f"{v}-sem{s}-{n}x{c}" for v, s, (n, c) in BOUND_CASES])
def test_hard_bound(orc, variant, sem, dt, shape):
    """Assertion 1: every row and stage within levels + 1 ulps of the exact sum."""
    m = measured(orc, variant, sem, dt, shape)
    bad = []
    for stage in STAGES:
        if stage in m:
            st = rk.stats(m[stage]["e"])
            print(f"{variant} sem{sem} {np.dtype(dt).name} {shape} {stage}: max|e| "
                  f"{st['max']:.3f} rms {st['rms']:.3f} mean {st['mean']:+.3f} "
                  f"levels {m[stage]['levels']}")
            if st["max"] > m[stage]["levels"] + 1:
                bad.append((stage, st["max"], m[stage]["levels"]))
    assert not bad, bad


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("variant,sem", CASES, ids=CASE_IDS)
def test_no_wider_than_the_oracle(orc, variant, sem, dt):
    """Assertion 2: pooled over all rows of all shapes, max|e_gpu| <=
    max|e_oracle| + 1 ulp (the oracle on the same stored matrices)."""
    gpu, ref = [], []
    for shape in xs.SHAPES:
        if rk.fits(variant, *shape):
            m = measured(orc, variant, sem, dt, shape)
            gpu.append(np.abs(m["total"]["e"]))
            ref.append(np.abs(m["oracle"]["e"]))
    gpu, ref = np.concatenate(gpu), np.concatenate(ref)
    print(f"{variant} sem{sem} {np.dtype(dt).name}: pooled max|e| gpu {gpu.max():.3f} oracle "
          f"{ref.max():.3f}; rms gpu {np.sqrt(np.mean(gpu * gpu)):.3f} oracle "
          f"{np.sqrt(np.mean(ref * ref)):.3f} over {gpu.size} rows")
    assert gpu.max() <= ref.max() + 1.0, (gpu.max(), ref.max())


CIRC_BLOCKS = [(ncols, seed, row0) for ncols in (4099, 6144, 8200) for seed in (1, 2)
               for row0 in (0, 1000, ncols - 128)]         # the last runs over into row 0
CIRC_ROWS = 256


def circulant_block(orc, dt, ncols, seed, row0):
    """A circulant row block, its one exact row sum per row and the oracle's
    errors on it, once."""
    key = (np.dtype(dt).name, ncols, seed, row0)
    if key not in _BLOCK:
        a = xs.circulant(ncols, dt, seed, rows=(row0, CIRC_ROWS), orc=orc)
        S = np.full(CIRC_ROWS, xs.circulant_sum(ncols, dt, seed, orc))
        _BLOCK[key] = (a, S, xs.err_ulps_of(orc.rowsum(a), S, dt))
    return _BLOCK[key]


# Blocks on which a kernel's spread is 3 ulps where the oracle's is 1, as
# measured on an MI355X with every kernel of this list: (dtype, ncols, seed,
# row0) -> the kernels.  On all 648 (kernel, semantics, dtype, block) cases
# both spreads are 1, 2 or 3 ulps; these 62 are the ones that pair a 3 with a
# 1.  No stage stands out: on random inputs the piece partials carry rms 0.50 -
# 0.52 ulp against the exact piece sums and the sums over the partials 0.39 -
# 0.57, the row sums 0.50 - 0.54 in all against the oracle's 0.47 - 0.50
# (profiles/rowsum_exact_error.json).  Kept failing, strictly: a summation
# order that narrows one of them must take it off this list.
KNOWN_WIDER = {
    ("float32", 4099, 2, 1000): ["flat_round", "flat_round_deferred_np0",
                                 "flat_round_deferred_np3", "mfree_round_flat", "rowsum_flat"],
    ("float32", 6144, 1, 0): ["split_flat_round", "split_round"],
    ("float32", 6144, 1, 1000): ["mfree_round", "split_flat_round", "split_round"],
    ("float32", 6144, 1, 6016): ["split_round"],
    ("float64", 4099, 1, 1000): ["flat_round", "flat_round_deferred_np0",
                                 "flat_round_deferred_np3", "fused_round", "mfree_round",
                                 "mfree_round_flat", "rowsum", "rowsum_flat", "scale_rowsum",
                                 "split_flat_round", "split_round"],
    ("float64", 4099, 1, 3971): ["fused_round", "mfree_round", "rowsum", "scale_rowsum",
                                 "split_flat_round", "split_round"],
    ("float64", 6144, 1, 0): ["split_flat_round", "split_round"],
    ("float64", 6144, 1, 1000): ["fused_round", "rowsum", "scale_rowsum", "split_round"],
    ("float64", 6144, 1, 6016): ["split_flat_round", "split_round"],
}


def _equal_sum_cases():
    out = []
    for variant, sem in CASES:
        for dt in DTYPES:
            for blk in CIRC_BLOCKS:
                name = np.dtype(dt).name
                marks = ()
                if variant in KNOWN_WIDER.get((name, *blk), ()):
                    marks = pytest.mark.xfail(strict=True, reason=(
                        "row-sum stage (total): spread 3 ulps on this block where the "
                        "oracle's is 1; measured, see KNOWN_WIDER"))
                out.append(pytest.param(variant, sem, dt, blk, marks=marks,
                                        id=f"{variant}-sem{sem}-{name}-{blk[0]}-seed{blk[1]}-"
                                           f"row{blk[2]}"))
    return out


@pytest.mark.parametrize("variant,sem,dt,blk", _equal_sum_cases())
def test_equal_sum_inputs(orc, variant, sem, dt, blk):
    """Assertion 3: a circulant row block, unit scales (a transforming kernel
    stores the block as it is): spread_gpu <= spread_oracle + 1 ulp.  (Where
    the sums lie in [2048, 4096) - the 6144-column blocks - the oracle at <= 2
    and EPS at 4.1 ulps then put every adjacent |ds| below EPS.)"""
    ncols, seed, row0 = blk
    a, S, eo = circulant_block(orc, dt, ncols, seed, row0)
    r = rk.run(orc, variant, a, sem, 0, unit=True)
    assert np.array_equal(r["stored"], a)
    eg = xs.err_ulps_of(r["s"], S, dt)
    sg, so = eg.max() - eg.min(), eo.max() - eo.min()
    print(f"{variant} sem{sem} {np.dtype(dt).name} circulant {ncols} seed {seed} row0 {row0}: "
          f"spread gpu {sg:.3f} oracle {so:.3f}; e gpu [{eg.min():+.3f}, {eg.max():+.3f}]")
    levels = xs.levels(rk.VARIANTS[variant][0], dt, ncols, col0=r["col0"], col1=r["col1"])
    assert np.abs(eg).max() <= levels + 1
    assert sg <= so + 1.0, (float(sg), float(so))


# ---------------------------------------------------------------------------
# 4. whole solves of fp32 circulants: one right answer, round 0
# ---------------------------------------------------------------------------
FORMS = {"deferred": {}, "every": dict(write_every_round=True), "mfree": dict(matrix_free=True)}
SOLVES = [(n, seed, form) for n, seed in xs.CIRC_CASES
          for form in (FORMS if n in (6144, 7000) else ("deferred",))]
_CIRC = {}


def circulant_case(orc, n, seed):
    """The matrix, S and the oracle's solves of one (n, seed); the last one is kept."""
    if (n, seed) not in _CIRC:
        _CIRC.clear()
        a = xs.circulant(n, np.float32, seed, orc=orc)
        ref = {sem: orc.similarity_transform(a, sem) for sem in (rk.SYCL, rk.MAINPY)}
        _CIRC[n, seed] = (a, xs.circulant_sum(n, np.float32, seed, orc), ref)
    return _CIRC[n, seed]


@pytest.fixture(scope="module")
def eigen():
    e = ev.EigenValue()
    yield e
    e.close()


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(rk.DEV)
    yield s
    s.close()


@pytest.mark.parametrize("sem", [rk.SYCL, rk.MAINPY])
@pytest.mark.parametrize("n,seed,form", SOLVES, ids=[f"{n}-seed{s}-{f}" for n, s, f in SOLVES])
def test_circulant_solves_stop_in_round_0(orc, eigen, solver, n, seed, form, sem):
    """Assertion 4: the drop-in and the device solver stop where the oracle
    stops - round 0: count 0 (cyclic) / 1 (open), one round evaluated - and
    lambda = s_0[0] lies within levels + 1 ulps of S (K0 is st_rowsum below
    the flat threshold, st_rowsum_flat from it)."""
    a, S, ref = circulant_case(orc, n, seed)
    want = (ref[sem].iter_count, ref[sem].rounds_evaluated)
    assert want == ((0, 1) if sem == rk.SYCL else (1, 1))
    k0 = "rowsum_flat" if dev.flat_round_pays(n, n, torch.float32) else "rowsum"
    assert (k0 == "rowsum_flat") == (n >= 6144)
    bound = xs.levels(k0, np.float32, n) + 1
    got = {}
    lam, _, _, it, st = eigen.similarity_transform_ex(a, semantics=sem, **FORMS[form])
    got["drop-in ex"] = (float(lam), it, st["rounds"])
    if sem == rk.SYCL and form == "deferred":       # the reference's own call
        lam, _, _, it = eigen.similarity_transform(a)
        got["drop-in"] = (float(lam), it, 1)
    lam, _, it, st = solver.solve(torch.from_numpy(a).to(rk.DEV), semantics=sem, **FORMS[form])
    got["device"] = (float(lam), it, st["rounds"])
    bad = []
    for path, (lam, it, rounds) in got.items():
        e = float(xs.err_ulps_of(np.float32(lam), np.float64(S), np.float32))
        print(f"circulant {n} seed {seed} {form} sem{sem} {path}: count {it} rounds {rounds} "
              f"lambda {lam!r} e {e:+.3f} ulps (bound {bound})")
        if (it, rounds) != want or abs(e) > bound:
            bad.append((path, it, rounds, e))
    assert not bad, (bad, want)
