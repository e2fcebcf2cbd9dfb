"""The crafted neighbourhood clouds (tests/neighbourhood_cases.py) on the restatements alone: every case reaches what it is named for, the
caps that tests/test_gpu_neighbourhood_cases.py relies on hold for the reference by itself, and the reference's neighbour lists -- which
take a shortcut through a k-d tree -- equal a plain O(n^2) restatement on every case."""
import numpy as np
import pytest

import colored_restatement as CR
import gicp_restatement as G
import neighbourhood_cases as NC
import support as S

f32 = np.float32
LATTICES = ("plane", "plane tilted", "block", "block shuffled")
# share of points whose K-th and (K+1)-th fp32 distances are equal.  Plane, K = 5: an interior point's 5th neighbour is the last of four at
# distance 1 and its 6th the first at sqrt 2, so only the 156 points on the rim tie (9.75 %); every other (lattice, K) ties in the interior.
TIE_FLOOR = {("plane", 5): 0.09, ("plane tilted", 5): 0.09}


@pytest.fixture(scope="module")
def brute():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = NC.brute_neighbours(NC.CASES[name][0], max(NC.KS) + 1)
        return cache[name]
    return get


def test_sizes_follow_the_kernels_block():
    assert NC.BLOCK == 256 or {NC.BLOCK - 1, NC.BLOCK, NC.BLOCK + 1} <= set(NC.SIZES)
    assert {3, 4, 255, 256, 257, 4097} | {k + d for k in NC.KS for d in (-1, 0, 1)} <= set(NC.SIZES)
    assert all("uniform %d" % n in NC.CASES for n in NC.SIZES)
    assert max(len(c[0]) for c in NC.CASES.values()) <= 4100
    assert set(NC.FAMILY.values()) == {"lattice", "sizes", "repeats", "holes", "normals and colours", "scale", "threshold"}


@pytest.mark.parametrize("name", NC.NAMES)
def test_neighbour_lists_equal_brute_force(name, brute):
    """gicp_restatement.neighbours (k + 8 candidates of a cKDTree, a ball query where that is not provably complete) against the lexsort of
    all fp32 distances by (d2, index): the same lists, in the same order, for every K."""
    pts = NC.CASES[name][0]
    ids, _ = brute(name)
    n_finite = int(np.isfinite(pts).all(1).sum())
    for k in NC.KS:
        nb = NC.reference(name, k)["nb"]
        m = min(k, n_finite)
        assert nb.shape == (len(pts), m)
        want = ids[:, :m] if n_finite >= 3 else np.full((len(pts), m), -1)
        bad = np.nonzero((nb != want).any(1))[0]
        assert len(bad) == 0, "%s k=%d: %d lists differ, first at point %d: %s, brute force %s" % (name, k, len(bad), bad[0], nb[bad[0]], want[bad[0]])


@pytest.mark.parametrize("name", LATTICES)
def test_lattices_tie_at_the_kth_neighbour(name, brute):
    ids, d2 = brute(name)
    for k in NC.KS:
        share = float((d2[:, k - 1] == d2[:, k]).mean())
        print("%s k=%d: %.4f of the points tie at the K-th neighbour" % (name, k, share))
        assert share >= TIE_FLOOR.get((name, k), 0.8), (name, k, share)


def test_shuffled_block_tells_lowest_from_highest_index(brute):
    """The tie rule is visible: with "highest index wins" the neighbour SET of some point differs, for every K."""
    pts = NC.CASES["block shuffled"][0]
    low, _ = brute("block shuffled")
    high, _ = NC.brute_neighbours(pts, max(NC.KS), highest_index_wins=True)
    for k in NC.KS:
        differ = (np.sort(low[:, :k], 1) != np.sort(high[:, :k], 1)).any(1)
        assert differ.sum() > 0.5 * len(pts), (k, int(differ.sum()))


@pytest.mark.parametrize("name", NC.NAMES)
def test_threshold_band_is_capped(name):
    """The reference alone: at most 2 % of a crafted cloud has det / threshold inside (1e-2, 1e4), where a kernel's determinant may
    land visibly elsewhere than numpy's."""
    n = len(NC.CASES[name][0])
    for k in NC.KS:
        r = NC.reference(name, k)
        band = NC.in_band(r["margin"])
        with np.errstate(invalid="ignore"):
            near = (r["margin"] > S.GRAD_NEAR[0]) & (r["margin"] < S.GRAD_NEAR[1])
        print("%s k=%d: %d of %d in the band, %d within 2x of the threshold" % (name, k, band.sum(), n, near.sum()))
        assert band.sum() <= NC.BAND_CAP * n, (name, k, int(band.sum()), n)
    assert NC.BAND == S.GRAD_BAND and NC.BAND_CAP == S.GRAD_SHARE_CAP


def ungapped_share(name, k):
    r = NC.reference(name, k)
    fin = ~np.isnan(r["nrm"]).any(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = (r["ev"][fin, 1] - r["ev"][fin, 0]) / r["ev"][fin, 2]
    return float((~((gap >= S.GICP_GAP) | (r["ev"][fin, 2] == 0))).mean())


def test_cases_reach_what_they_are_named_for():
    # neighbourhoods without a usable eigen-gap, which the Rayleigh-quotient rule has to judge
    assert all(ungapped_share("line", k) == 1.0 for k in NC.KS)
    assert 0.6 <= ungapped_share("block", 20) <= 0.66 and ungapped_share("block", 5) == 0.0
    # fewer than K points: every finite point is a neighbour; fewer than 3: nothing is solved
    for n in NC.SIZES:
        for k in NC.KS:
            r = NC.reference("uniform %d" % n, k)
            assert r["nb"].shape[1] == min(n, k) and np.isfinite(r["nrm"]).all() and np.isfinite(r["grad"]).all()
    for k in NC.KS:
        r = NC.reference("one point", k)
        assert (r["nrm"] == f32([1, 0, 0])).all() and (r["grad"] == 0).all() and (r["nb"] == np.arange(k)).all()
        r = NC.reference("pairs", k)
        pts = NC.CASES["pairs"][0]
        assert (pts[r["nb"][:, 0]] == pts[r["nb"][:, 1]]).all() and (r["nb"][:, 0] < r["nb"][:, 1]).all()       # a point and its twin lead every list
        r = NC.reference("two finite", k)
        assert np.isnan(r["nrm"]).all() and (r["grad"][[10, 200]] == 0).all() and np.isnan(np.delete(r["grad"], [10, 200], 0)).all()
        r = NC.reference("three finite", k)
        assert np.isfinite(r["nrm"][[7, 150, 299]]).all() and np.isnan(r["nrm"]).any(1).sum() == 297 and (r["grad"][[7, 150, 299]] != 0).any()
        for n in (1, 2, 3, 1000):
            r = NC.reference("all NaN %d" % n, k)
            assert np.isnan(r["nrm"]).all() and np.isnan(r["grad"]).all()
        r = NC.reference("holes", k)
        holes = NC.CASES["holes"][0]
        fin = np.isfinite(holes).all(1)
        assert 2550 <= fin.sum() < 2700 and np.isnan(holes).any(1).sum() == 300 and np.isposinf(holes).any() and np.isneginf(holes).any()
        assert np.array_equal(np.isnan(r["nrm"]).any(1), ~fin) and np.array_equal(np.isnan(r["grad"]).any(1), ~fin)
        assert fin[r["nb"][fin]].all()


def test_normals_and_colours_of_the_gradient():
    pts, nrm, rgba = NC.CASES["bad normals"]
    ln = np.linalg.norm(nrm.astype(np.float64), axis=1)
    bad = ~np.isfinite(nrm).all(1) | (ln == 0)
    with np.errstate(invalid="ignore"):
        assert bad.sum() == 15 and (nrm == 0).all(1).sum() == 5 and np.isnan(nrm).any(1).sum() == 5 and np.isinf(nrm).any(1).sum() == 5
        assert ((ln > 0.9e-3) & (ln < 1.1e-3)).sum() == 5 and ((ln > 0.9e3) & (ln < 1.1e3)).sum() == 5
    unit = nrm.copy()
    unit[~bad] = (nrm[~bad] / ln[~bad, None]).astype(f32)
    for k in NC.KS:
        r = NC.reference("bad normals", k)
        assert np.array_equal(np.isnan(r["grad"]).any(1), bad) and np.isfinite(r["nrm"]).all()
        g1, _ = CR.gradients(pts, unit, rgba, k, nb=r["nb"])                 # a normal's length does not matter
        scaled = ~bad & (np.abs(ln - 1) > 0.5)
        assert np.abs(g1[scaled].astype(np.float64) - r["grad"][scaled]).max() <= 1e-5 * max(1.0, np.abs(g1[scaled]).max())
        r = NC.reference("one colour", k)
        assert (r["grad"] == 0).all() and (r["margin"] > 1e4).all()
        # intensity linear in position: the gradient in closed form, the reference within an fp32 rounding of it
        r = NC.reference("linear intensity", k)
        want = NC.linear_gradient(NC.CASES["linear intensity"][1])
        assert np.abs(r["grad"] - want).max() <= 1e-9 and (r["margin"] > 1e4).all()
    assert {tuple(x) for x in NC.CASES["linear intensity"][1]} == {(0.0, 0.0, 1.0), NC.TILTED}
    assert np.abs(want[:, 2]).max() > 1e-3                                    # the tilted normals' gradients leave the lattice's plane


def test_scale_and_threshold_cases():
    tight = NC.MARKS["tight"]
    for k in NC.KS:
        r = NC.reference("mixed scales", k)
        # the contract as written: the constraint row (m - 1) n is not scaled with the cloud, so a neighbourhood 1e-4 across falls below
        # 1e-12 (tr / 3)^3 and its gradient is zero; the clusters 1 across are solved
        assert (r["grad"][tight] == 0).all() and (r["margin"][tight] < 1e-2).all()
        assert (r["grad"][~tight] != 0).any(1).all() and (r["margin"][~tight] > 1e4).all()
        assert np.isfinite(r["nrm"]).all()
        r = NC.reference("offset 1e4", k)
        assert (r["margin"] > 1e4).all() and np.abs(NC.CASES["offset 1e4"][0]).min() > 9e3
    lo, hi = NC.ladder_window(5)
    assert NC.ladder_window(10) is None and NC.ladder_window(20) is None     # (m / (m - 1))^4 < 2: no such interval for the larger K
    m = NC.reference("threshold ladder", 5)["margin"][NC.MARKS["ladder"]]
    assert NC.MARKS["ladder"].sum() == 60 and ((m > lo) & (m < hi)).sum() >= 12, np.sort(m)
    assert ((m > S.GRAD_NEAR[0]) & (m < S.GRAD_NEAR[1])).sum() >= 1           # and the either-side-is-right rule is exercised
