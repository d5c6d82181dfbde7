"""GPU: the flat round with deferred writes, one launch at a time.

st_round_flat_deferred is what the headline solve runs, and the header
promises that every value it produces - s_{k+1}, 1 / s_{k+1}, v, the state
and the matrix it finally stores - is bit-identical to st_round_flat storing
every round.  The whole-solve tests run it only on square, vector-aligned
matrices of 144 MiB and more; here each of its launches (NP = 0 ... 5
pending rounds, storing or not, the flush) runs on small row blocks with
ragged last row groups (13 and 37 rows are ragged for 1 / 2 / 4 / 8 rows
per workgroup), a ragged last piece (1032 / 2056 columns: one or two 1024-
column pieces and 8 columns), columns that are no multiple of the vector
width (257: W = 1) and row0 > 0, against

  * st_round_flat on a matrix stored every round (s, v, state, matrix),
  * the oracle's compute_next chain (matrix),
  * numpy division in the dtype and st_recip (the reciprocals),

all with equality - there is no tolerance in this file.

Not reachable at sizes a quick test can afford: the non-temporal
instantiations (flat_round_nt: blocks of 2 GiB and more), which the
full-size solve tests cover, and the dispatch on pointer misalignment.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import eigen_value_amd as ev  # noqa: E402
from eigen_value_amd import _lib  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402

DEV = "cuda:0"
TD = {np.float64: torch.float64, np.float32: torch.float32}
SEMS = [_lib.ST_SEM_SYCL, _lib.ST_SEM_MAINPY]
BLOCKS = [(1, 1, 0), (3, 3, 0), (13, 257, 100), (13, 1032, 3), (37, 2056, 11),
          (64, 4096, 1024)]
MAX_ITR = 1000


def to_np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def raw_state(state):
    torch.cuda.synchronize()
    return _lib.st_state.from_buffer_copy(state.cpu().numpy().tobytes())


def state_of(state):
    """The round's record and the flat kernels' scratch words (zero between
    launches)."""
    r = raw_state(state)
    assert r.arrivals == 0 and r.max_bits == 0 and r.fail == 0
    return dev.read_state(state)


class Block:
    """One row block's inputs and the every-round reference run."""

    def __init__(self, orc, dt, sem, nrows, ncols, row0, eps=0.0):
        self.orc, self.dt, self.sem = orc, dt, sem
        self.nrows, self.ncols, self.row0, self.eps = nrows, ncols, row0, eps
        self.tdt = TD[dt]
        self.m = dev.defer_rounds(nrows, ncols, self.tdt)
        assert self.m == 6
        self.order = 0 if sem == _lib.ST_SEM_SYCL else 1
        self.rows = slice(row0, row0 + nrows)
        self.a0 = orc.random_matrix(ncols, 3, dt, nrows=nrows)
        self.v0 = orc.random_matrix(ncols, 5, dt, nrows=1)[0]
        # s_0, and what s_1 ... s_m hold outside the block's slot (another
        # rank's rows): fixed positive vectors, so both runs see the same
        self.fill = [np.ascontiguousarray((orc.random_matrix(ncols, 9 + k, dt, nrows=1)[0]
                                           + dt(0.5)).astype(dt)) for k in range(self.m + 1)]
        self.part = dev.flat_scratch(nrows, ncols, self.tdt, DEV)
        self.reference()

    def dev_(self, x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)

    def next_full(self, k, s_next):
        """s_{k+1}: the block's slot from the launch, the rest as given."""
        s = self.dev_(self.fill[k + 1])
        s[self.rows] = s_next
        return s

    def reference(self):
        """st_round_flat for k = 0 ... m-1, the matrix stored every round:
        A_{k+1}, the full s_{k+1}, v and the state after each round, and the
        oracle's matrices."""
        a, v = self.dev_(self.a0), self.dev_(self.v0)
        s = self.dev_(self.fill[0])
        state = dev.new_state(DEV)
        self.A, self.s, self.v, self.st = [self.a0], [to_np(s)], [], []
        chain = self.a0
        for k in range(self.m):
            s_next = torch.empty(self.nrows, dtype=self.tdt, device=DEV)
            dev.flat_round(a, s, s_next, self.part, v, state, row0=self.row0, eps=self.eps, k=k,
                           max_itr=MAX_ITR, semantics=self.sem)
            chain = self.orc.compute_next(chain, self.s[k], row0=self.row0, order=self.order)
            s = self.next_full(k, s_next)
            self.A.append(to_np(a)), self.s.append(to_np(s)), self.v.append(to_np(v))
            self.st.append(state_of(state))
            assert np.array_equal(self.A[-1], chain), k        # the oracle's A_{k+1}
            if self.st[-1]["done"]:
                break
        self.rounds = len(self.st)

    def deferred(self, stores, flush_at=None):
        """The same rounds through st_round_flat_deferred, storing A_{k+1} in
        the rounds of `stores` (a store starts a new group of pending
        rounds); everything is compared with the reference after every
        round.  `flush_at`: after that (non-storing) round, flush and end."""
        dt = self.dt
        a, v = self.dev_(self.a0), self.dev_(self.v0)
        s = [self.dev_(self.fill[0])]
        inv = [torch.empty_like(s[0])]
        dev.recip(s[0], inv[0])
        state = dev.new_state(DEV)
        j0 = 0                                     # the matrix in `a` is A_j0
        for k in range(self.rounds):
            npend, store = k - j0, k in stores
            s_next = torch.full((self.nrows,), -1.0, dtype=self.tdt, device=DEV)
            inv_next = torch.full((self.nrows,), -1.0, dtype=self.tdt, device=DEV)
            args = (a, s[k], inv[k], s_next, inv_next, self.part, v, state, s[j0:k], inv[j0:k])
            kw = dict(row0=self.row0, eps=self.eps, k=k, max_itr=MAX_ITR, semantics=self.sem)
            dev.flat_round_deferred(*args, store=store, **kw)
            tag = (k, npend, store)
            assert np.array_equal(to_np(s_next), self.s[k + 1][self.rows]), tag
            assert np.array_equal(to_np(v), self.v[k]), tag
            assert state_of(state) == self.st[k], tag
            # 1 / s_{k+1}: k_parts' quotient, st_recip's and numpy's, the same bits
            r = torch.empty_like(s_next)
            dev.recip(s_next, r)
            assert np.array_equal(to_np(inv_next), to_np(r)), tag
            assert np.array_equal(to_np(inv_next), dt(1) / self.s[k + 1][self.rows]), tag
            # the matrix: the last stored one until this round stores
            j0 = k + 1 if store else j0
            assert np.array_equal(to_np(a), self.A[j0]), tag
            stopped = self.st[k]["done"] == 1
            if (flush_at == k or stopped) and not store:
                keep = (s_next.clone(), inv_next.clone(), v.clone(), state.clone())
                dev.flat_round_deferred(*args, store=True, flush=True, **kw)
                assert np.array_equal(to_np(a), self.A[k + 1]), ("flush", tag)
                now = (s_next, inv_next, v, state)
                assert all(torch.equal(x, y) for x, y in zip(keep, now)), ("flush", tag)
                state_of(state)
                return
            if stopped:
                return
            full = self.next_full(k, s_next)
            finv = torch.empty_like(full)
            dev.recip(full, finv)
            finv[self.rows] = inv_next               # the launch's own reciprocals
            s.append(full), inv.append(finv)


_BLOCKS = {}


def block(orc, dt, sem, shape):
    """Inputs and the reference run, computed once per (dtype, semantics, block)."""
    key = (np.dtype(dt).name, sem, shape)
    if key not in _BLOCKS:
        _BLOCKS[key] = Block(orc, dt, sem, *shape)
    return _BLOCKS[key]


@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_deferred_chain(orc, dt, sem, shape):
    """NP = 0 ... 4 read-only, NP = 5 storing: the group the solve runs."""
    b = block(orc, dt, sem, shape)
    # eps = 0: no round stops (but a 1-long s in the open semantics, which
    # has no pair to fail: round 0 stops, and the flush stores A_1)
    assert b.rounds == (1 if (shape[1] == 1 and sem == _lib.ST_SEM_MAINPY) else b.m)
    b.deferred(stores={b.m - 1})


@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_deferred_early_store(orc, dt, sem, shape):
    """A store with 2 pending (the storing NP = 2 instantiation) leaves A_3;
    a fresh group goes on from there (NP = 0, 1 and a storing NP = 2)."""
    b = block(orc, dt, sem, shape)
    b.deferred(stores={2, 5})


@pytest.mark.parametrize("npend", [0, 3])
@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_deferred_flush(orc, dt, sem, shape, npend):
    """flush = 1 after a read-only round with `npend` pending stores A_{k+1}
    and leaves s_{k+1}, 1 / s_{k+1}, v and the state as they were."""
    b = block(orc, dt, sem, shape)
    b.deferred(stores=set(), flush_at=min(npend, b.rounds - 1))


@pytest.mark.parametrize("sem", SEMS)
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_deferred_gating(orc, dt, sem):
    """Once a round has stopped, a later deferred round - storing or not -
    is a no-op: A, v and s_next stand, the scratch words stay zero."""
    nrows, n, row0 = 13, 1032, 3
    tdt = TD[dt]
    a = torch.from_numpy(orc.random_matrix(n, 1, dt, nrows=nrows)).to(DEV)
    s = torch.full((n,), 4.0, dtype=tdt, device=DEV)             # constant: stops
    inv = torch.empty_like(s)
    dev.recip(s, inv)
    s_next, inv_next = torch.empty(nrows, dtype=tdt, device=DEV), torch.empty(nrows, dtype=tdt,
                                                                             device=DEV)
    v = torch.ones(n, dtype=tdt, device=DEV)
    part = dev.flat_scratch(nrows, n, tdt, DEV)
    state = dev.new_state(DEV)
    kw = dict(row0=row0, eps=1e-3, max_itr=MAX_ITR, semantics=sem)
    dev.flat_round_deferred(a, s, inv, s_next, inv_next, part, v, state, store=False, k=0, **kw)
    st = state_of(state)
    assert st["stop"] == 1 and st["done"] == 1 and st["end"] == 1
    keep = [x.clone() for x in (a, v, s_next, inv_next, state)]
    s2, inv2 = s * 2.0, inv * 0.5
    for k, store in ((1, False), (2, True), (2, False)):
        pend = ([s, s2][:k], [inv, inv2][:k])
        dev.flat_round_deferred(a, s2, inv2, s_next, inv_next, part, v, state, *pend,
                                store=store, k=k, **kw)
        assert all(torch.equal(x, y) for x, y in zip(keep, (a, v, s_next, inv_next, state))), k
        assert state_of(state) == st


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_deferred_rejected_calls(orc, dt):
    """npend = m, and npend = m - 1 without a store, are errors of the C
    entry point itself (the Python wrapper's own assertions are bypassed);
    nothing is launched."""
    nrows, n, row0 = 13, 1032, 3
    tdt, sfx = TD[dt], "f64" if dt == np.float64 else "f32"
    m = dev.defer_rounds(nrows, n, tdt)
    a = torch.from_numpy(orc.random_matrix(n, 1, dt, nrows=nrows)).to(DEV)
    s = torch.from_numpy(orc.random_matrix(n, 2, dt, nrows=1)[0] + dt(0.5)).to(DEV)
    inv = torch.empty_like(s)
    dev.recip(s, inv)
    s_next = torch.full((nrows,), -1.0, dtype=tdt, device=DEV)
    inv_next = s_next.clone()
    v = torch.ones(n, dtype=tdt, device=DEV)
    part = dev.flat_scratch(nrows, n, tdt, DEV)
    state = dev.new_state(DEV)
    keep = [x.clone() for x in (a, v, s_next, inv_next, state)]
    L = _lib.load()
    fn = getattr(L, f"st_round_flat_deferred_{sfx}")
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call(npend, store):
        ps = (ctypes.c_void_p * m)(*[s.data_ptr()] * m)
        pi = (ctypes.c_void_p * m)(*[inv.data_ptr()] * m)
        return fn(a.data_ptr(), s.data_ptr(), inv.data_ptr(), s_next.data_ptr(),
                  inv_next.data_ptr(), part.data_ptr(), v.data_ptr(), nrows, n, row0, 1e-3, m,
                  MAX_ITR, _lib.ST_SEM_SYCL, ps, pi, npend, int(store), 0, state.data_ptr(),
                  stream)

    for npend, store, msg in ((m, True, "pending rounds"), (m, False, "pending rounds"),
                              (m - 1, False, "without a store")):
        rc = call(npend, store)
        assert rc < 0
        with pytest.raises(ev.EigenValueError, match=msg):
            _lib.check(rc, "round_flat_deferred")
        assert all(torch.equal(x, y) for x, y in zip(keep, (a, v, s_next, inv_next, state)))
    # the wrapper refuses the same calls before the library sees them
    with pytest.raises(AssertionError):
        dev.flat_round_deferred(a, s, inv, s_next, inv_next, part, v, state, [s] * (m - 1),
                                [inv] * (m - 1), store=False)
    # and the group's storing round, m - 1 pending, is accepted
    assert call(m - 1, True) == 0
    torch.cuda.synchronize()
    assert not torch.equal(a, keep[0])


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 3, 257, 4100])
def test_recip_bitwise(orc, dt, n):
    """st_recip: the correctly rounded quotient, numpy's bits."""
    s = (orc.random_matrix(max(n, 2), 21, dt, nrows=1)[0][:n] * dt(3) + dt(1e-3)).astype(dt)
    ts = torch.from_numpy(np.ascontiguousarray(s)).to(DEV)
    inv = torch.full((n + 2,), -1.0, dtype=TD[dt], device=DEV)
    dev.recip(ts, inv)
    got = to_np(inv)
    assert np.array_equal(got[:n], dt(1) / s) and np.all(got[n:] == -1)   # nothing past n
