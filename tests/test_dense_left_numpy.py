"""GPU: EigenValue.similarity_transform_left from numpy against numpy's own
eigenvalues of the transposed matrix, and the return shapes and types of the
similarity_transform_* family next to it.

eps: the stop test compares neighbouring column sums, so lambda is known to
about eps when it passes; the bounds here (1e-5 / 1e-10 relative) need eps
well below the default 1e-3.  1e-6 (fp32) and 1e-12 (fp64) lie at or below the
rounding noise of the sums, where the loop may run out of rounds instead of
stopping - lambda is then converged to that noise, which is what is checked;
max_itr = 100 bounds the time."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import eigen_value_amd as ev                      # noqa: E402

pytestmark = pytest.mark.gpu

EPS = {np.float32: 1e-6, np.float64: 1e-12}
TOL = {np.float32: 1e-5, np.float64: 1e-10}


@pytest.fixture(scope="module")
def eigen():
    e = ev.EigenValue()
    yield e


def _hilbert(n, dt):
    i = np.arange(n, dtype=np.float64)
    return (1.0 / (i[:, None] + i[None, :] + 1.0)).astype(dt)


def _random(n, dt):
    # not symmetric: the left and the right vectors differ
    return (np.random.default_rng(513).random((n, n)) + 0.05).astype(dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind,n", [("hilbert", 128), ("random", 513)])
def test_left_vector_against_numpy_eig_of_the_transpose(eigen, kind, n, dt):
    mat = _hilbert(n, dt) if kind == "hilbert" else _random(n, dt)
    keep = mat.copy()
    lam, u, ts, itr, st = eigen.similarity_transform_left(mat, eps=EPS[dt], max_itr=100)
    assert isinstance(lam, dt) and u.shape == (n,) and u.dtype == dt
    assert isinstance(ts, int) and isinstance(itr, int) and isinstance(st, dict)
    assert st["rounds"] >= 1 and np.array_equal(mat, keep)
    w, vecs = np.linalg.eig(mat.astype(np.float64).T)
    top = int(np.argmax(w.real))
    assert abs(float(lam) - w[top].real) <= TOL[dt] * w[top].real, (float(lam), w[top].real)
    ref = np.abs(vecs[:, top].real)
    got = u.astype(np.float64)
    assert (got > 0).all()
    assert np.max(np.abs(got / got.max() - ref / ref.max())) <= (1e-3 if dt == np.float32 else 1e-7)
    # u A = lambda u in fp64 arithmetic
    resid = np.abs(got @ mat.astype(np.float64) - float(lam) * got)
    assert resid.max() <= (1e-4 if dt == np.float32 else 1e-9) * float(lam) * got.max()


def test_left_traces_and_times(eigen):
    mat = _random(300, np.float64)
    lam, u, ts, itr, st = eigen.similarity_transform_left(mat, trace_sums=True, time_kernels=True)
    sums = eigen.last_round_sums()
    assert sums.shape == (st["rounds"], 300) and sums.dtype == np.float64
    assert np.allclose(sums[0], mat.sum(axis=0), rtol=1e-13)       # round 0: the column sums
    assert st["fused_launches"] == st["rounds"]
    lam2, u2, _, itr2, _ = eigen.similarity_transform_left(mat, semantics=ev._lib.ST_SEM_MAINPY)
    assert abs(lam2 - lam) <= 1e-3 * lam


def test_return_shapes_of_the_family(eigen):
    n = 64
    m32, m64 = _random(n, np.float32), _random(n, np.float64)
    lam, v, ts, itr = eigen.similarity_transform(m32)               # the reference's 4-tuple
    assert isinstance(lam, np.float32) and v.shape == (n,) and v.dtype == np.float32
    assert isinstance(ts, int) and isinstance(itr, int)
    lam, v, ts, itr = eigen.similarity_transform(m64)
    assert isinstance(lam, np.float64) and v.dtype == np.float64
    out = eigen.similarity_transform_ex(m64, matrix_free=True)
    assert len(out) == 5 and isinstance(out[4], dict) and out[1].shape == (n,)
    out = eigen.similarity_transform_left(m32)
    assert len(out) == 5 and isinstance(out[0], np.float32) and out[1].dtype == np.float32
    assert isinstance(out[4], dict) and "rounds" in out[4]
    lam, v, ts, itr = eigen.similarity_transform_half(m32.astype(np.float16))
    assert isinstance(lam, np.float32) and v.shape == (n,) and v.dtype == np.float32
    lams, vs, ts, its = eigen.similarity_transform_batched(np.stack([m32, m32 + 1]))
    assert lams.shape == (2,) and vs.shape == (2, n) and its.dtype == np.uint32
    lams, vl, ts, its = eigen.similarity_transform_vbatched([m64, m64[:9, :9].copy()])
    assert lams.shape == (2,) and [x.shape for x in vl] == [(n,), (9,)] and its.shape == (2,)
