"""GPU: the counted round loop of the three batched forms - rounds enqueued
`batch_rounds` at a time, the count of finished entries mirrored to the host
once per batch - on one tiny input each:

  dense   solve_batched(round_loop=True) on 3 x 130^2 fp64
  csrb    solve_csr_batched on the three table matrices as one batch
  multi   solve_csr_multi, C = 3, K = 1, on table matrix 0

A  the rounds per host check (1, 3, the default 8) change no bit of lambda, v,
   the counts or the converged flags, and rounds <= fused_launches
B  eps = 0, max_itr = 7 at 3 rounds per check: the last batch is cut to one
   round (fused_launches == 7), every entry ends unconverged with count 7
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no HIP device", allow_module_level=True)

import csr_terms_cases as tc  # noqa: E402
from eigen_value_amd import device as dev  # noqa: E402
from test_gpu_csr import DEV, csr_of, table_case, up  # noqa: E402
from test_gpu_csr_batch import batch_of  # noqa: E402

PATHS = ["dense", "csrb", "multi"]


@pytest.fixture(scope="module")
def solver():
    s = dev.DeviceSolver(DEV)
    yield s
    s.close()


@pytest.fixture(scope="module")
def runners(solver, orc):
    """path -> run(per_check, **options) -> (lambda, v, counts, converged,
    stats), everything on the host but v; the inputs are made once."""
    mats = np.stack([orc.random_matrix(130, 0, np.float64), orc.random_matrix(130, 1, np.float64),
                     orc.hilbert(130, np.float64)])
    d_mats = up(mats)
    bt = batch_of(solver, [table_case(i)[1:] for i in range(3)], np.float64)
    n, ip, ix, da = table_case(0)
    m = csr_of(solver, ip, ix, da, n)
    u, w = tc.term_vectors(n, 3, 3)
    mt = dev.CsrMultiTerms(m, up(u), up(w), solver=solver)   # [C, n]: K = 1
    assert (mt.C, mt.K) == (3, 1)

    def dense(per_check, **kw):
        lam, v, it, st = solver.solve_batched(d_mats, round_loop=True, batch=per_check, **kw)
        return lam.numpy(), v, it.numpy(), st["converged_each"], st

    def csrb(per_check, **kw):
        return solver.solve_csr_batched(bt, batch_rounds=per_check, **kw)

    def multi(per_check, **kw):
        return solver.solve_csr_multi(m, mt, batch_rounds=per_check, **kw)

    yield {"dense": dense, "csrb": csrb, "multi": multi}
    mt.close()
    m.close()
    bt.close()


@pytest.mark.parametrize("path", PATHS)
def test_rounds_per_check_change_no_bit(runners, path):
    run = runners[path]
    lam0, v0, it0, conv0, st0 = run(0)
    assert len(lam0) == 3 and st0["rounds"] >= int(max(it0)) >= 1
    assert st0["rounds"] <= st0["fused_launches"] and st0["fused_launches"] % 8 == 0
    for per_check in (1, 3):
        lam, v, it, conv, st = run(per_check)
        print(f"{path} per_check={per_check}: counts {[int(x) for x in it]}, rounds {st['rounds']}, "
              f"round launches {st['fused_launches']}")
        assert lam.tobytes() == lam0.tobytes() and torch.equal(v, v0)
        assert np.array_equal(it, it0) and np.array_equal(conv, conv0)
        assert (st["rounds"], st["converged"]) == (st0["rounds"], st0["converged"])
        assert st["rounds"] <= st["fused_launches"]


@pytest.mark.parametrize("path", PATHS)
def test_a_partial_last_batch_stops_at_max_itr(runners, path):
    lam, v, it, conv, st = runners[path](3, eps=0.0, max_itr=7)
    print(f"{path}: counts {[int(x) for x in it]}, converged {[int(x) for x in conv]}, "
          f"rounds {st['rounds']}, round launches {st['fused_launches']}")
    assert st["fused_launches"] == 7
    assert [int(x) for x in conv] == [0, 0, 0] and [int(x) for x in it] == [7, 7, 7]
    assert st["converged"] == 0 and st["rounds"] == 7
