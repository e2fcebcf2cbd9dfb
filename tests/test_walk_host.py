"""The closed form of the leaf update (leaf_eval in icp-variants_amd/csrc/dev_bvh.hpp) against the sequential scan it replaces, both
restated in NumPy float32 (tests/walk_restatement.py): the six outputs agree bitwise on 10^5 leaves of every category, ties included.
tests/test_gpu_walk_steps.py compares the device code with the same restatement.  No GPU needed."""
import numpy as np
import pytest
import walk_restatement as wr
from support import raw_bits as bits

N = 100_000


@pytest.mark.parametrize("category", wr.CATEGORIES)
def test_closed_form_equals_the_sequential_scan_bitwise(category):
    case = wr.leaf_cases(category, N, seed=1)
    seq = wr.leaf_update_sequential(**case)
    *closed, rare = wr.leaf_update_closed(**case)
    for name, a, b in zip(("best", "bi", "bpos", "b2", "l2", "b3"), seq, closed):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), (category, name, int((bits(a) != bits(b)).sum()))
    dd = wr.leaf_distances(case["C"], case["P"])
    assert not np.isnan(dd).any()
    m = np.minimum(dd.min(axis=1), wr.FLT_MAX)
    heavy = m <= case["best"]
    assert not (rare & ~heavy).any()
    # the categories do what their names say: no tie at all in continuous coordinates, nothing but ties where the running best is an
    # equal distance at another index, plenty of both on the grids
    if category in ("continuous", "seed_inside"):
        assert not rare.any()
    if category in ("tie_lower_elsewhere", "tie_higher_elsewhere"):
        assert rare.all()
        won = seq[1] != case["bi"]                         # the leaf's point wins the tie iff its index is the lower one
        assert won.all() == (category == "tie_higher_elsewhere") and won.any() == (category == "tie_higher_elsewhere")
    if category in ("grid2", "grid4"):
        assert 0.05 * N < rare.sum() and 0.05 * N < (heavy & ~rare).sum()
    if category == "unseeded":
        assert heavy.all() and (seq[1] >= 0).all() and not rare.any()
    if category == "padded":
        empty = (case["IDX"] < 0).all(axis=1)
        assert empty.any() and np.array_equal(seq[1][empty], case["bi"][empty])
    if category == "huge":
        assert np.isinf(dd).any() and np.isfinite(dd).any()


def test_quad_bounds_of_the_restatement():
    """Inside a box the bound is +0, an empty child as the builder stores it (+inf, +inf) gives +inf, and a degenerate box is a point distance."""
    LO = np.zeros((3, 3, 4), np.float32); HI = np.ones((3, 3, 4), np.float32)
    LO[1] = HI[1] = 0.5
    LO[2] = HI[2] = np.inf
    P = np.array([[0.25, 0.5, 1.0], [0.5, 0.5, 2.5], [0.0, 0.0, 0.0]], np.float32)
    b = wr.quad_bounds(LO, HI, P)
    assert np.array_equal(b[0], np.zeros(4, np.float32)) and not np.signbit(b[0]).any()
    assert np.array_equal(b[1], np.full(4, 4.0, np.float32))
    assert np.isposinf(b[2]).all()
