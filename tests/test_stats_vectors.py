"""tests/stats_vectors.py does what it says (CPU; numpy and the oracle).

The position sweeps on the GPU (test_gpu_stats_positions.py) are only as good
as their inputs: a vector meant to have ONE failing pair at p that has two,
or none, would let a kernel drop that pair unnoticed.  So every construction
is checked here at every size, dtype, semantics and position the sweeps use:
the failing pairs in plain numpy (in the vector's dtype) and the decision and
the maximum through the oracle's orc_stop / orc_find_max.
"""
import numpy as np
import pytest

import stats_vectors as sv


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("cyclic", [True, False])
@pytest.mark.parametrize("n", sv.SIZES)
def test_constructions(orc, dt, cyclic, n):
    eps, ee = dt(sv.EPS), dt(sv.EXACT_EPS)
    pos = sv.positions(n, dt, cyclic)
    assert pos and pos[0] == 0 and pos[-1] == (n - 1 if cyclic else n - 2)
    for p in pos:
        s = sv.one_fail(n, p, dt, eps, cyclic)
        assert s.dtype == dt and s.shape == (n,)
        assert sv.failing_pairs(s, eps, cyclic) == [p]
        assert not orc.stop(s, eps, cyclic)
        s = sv.all_pass(n, p, dt, eps, cyclic)
        assert sv.failing_pairs(s, eps, cyclic) == []
        assert orc.stop(s, eps, cyclic)
        s = sv.exact_eps(n, p, dt, "fail", cyclic)
        assert s.dtype == dt and abs(s[p] - s[(p + 1) % n]) == ee
        assert sv.failing_pairs(s, ee, cyclic) == [p]
        assert not orc.stop(s, ee, cyclic)
        s = sv.exact_eps(n, p, dt, "pass", cyclic)
        assert abs(s[p] - s[(p + 1) % n]) == np.nextafter(dt(1) + ee, dt(0)) - dt(1)
        assert sv.failing_pairs(s, ee, cyclic) == []
        assert orc.stop(s, ee, cyclic)
    # the maximum and the NaN sit on an element, not a pair: every index class
    for p in sv.positions(n, dt, True):
        s = sv.max_at(n, p, dt, eps)
        assert s[p] > 1 and np.count_nonzero(s != 1) == 1
        assert orc.find_max(s) == s[p] == sv.find_max(s) == s.max()
        assert orc.stop(s, eps, cyclic) and sv.failing_pairs(s, eps, cyclic) == []
        s = sv.max_at(n, p, dt, eps, decoys=True)
        assert orc.find_max(s) == s[p] == sv.find_max(s)
        assert np.isnan(s).sum() == (p >= 1) and (s == -7).sum() == (p + 1 < n)
        assert not orc.stop(s, eps, cyclic)           # -7 or the NaN fails a pair
        s = sv.nan_at(n, p, dt)
        assert np.isnan(s[p]) and np.isnan(s).sum() == 1
        assert orc.find_max(s) == 1 == sv.find_max(s)
        assert not orc.stop(s, eps, cyclic) and sv.failing_pairs(s, eps, cyclic)


def test_positions_hold_every_boundary_class():
    """Both sides of each boundary, where the size reaches it."""
    for dt, w in ((np.float64, 2), (np.float32, 4)):
        pos = set(sv.positions(8200, dt, True))
        for b in (w, 64, 64 * w, 256, 256 * w, 1024, 2048, 4096, 8200 - w):
            assert {b - 1, b} <= pos, (dt, b)
        assert {0, 1, 8198, 8199} <= pos
        assert 8199 not in sv.positions(8200, dt, False)       # open: no wrap pair
        assert set(sv.positions(9, dt, True)) >= {0, 1, w - 1, w, 7, 8}
        assert sv.positions(8200, dt, True) == sv.positions(8200, dt, True)   # seeded
