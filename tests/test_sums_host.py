"""What the bound of tests/test_gpu_sums.py can see, measured on its own reference (no GPU).

The device tests accept |sum - reference| <= 1e-9 of the sum of the absolute terms.  For every source size of tests/sums_cases.py, metrics
0, 1, 2 and weighting 0, 1, the valid pair that contributes LEAST to the 33 sums is left out, or counted twice: at least one sum must move
by more than 100 x 1e-9 of its absolute sum -- a lane dropped at a block tail or a partial folded twice cannot hide under the bound.  A
condition on the inputs: a shape that fails it needs another cloud, not another factor.

Measured (test_resolution_of_the_bound prints the figures): the smallest move of a dropped or doubled pair, over all sizes, metrics and
weightings, is 1.06e-5 of an absolute sum (n = 131 073, point-to-point, constant weights; the largest size is the hardest: about 1 / n
of a sum), 10 600 times the bound; at n = 257 it is 4.4e-3, at n = 65 537 2.8e-5.  One weight scaled by 1 + 2^-23 -- one unit in the
last place of an fp32 weight -- moves a sum by 1.2e-7 .. 4.1e-7 of its absolute sum at n = 1, by 2.6e-10 (the least-contributing pair)
.. 1.7e-8 (the most-contributing one) at n = 511, by 3.3e-12 .. 2.1e-10 at n = 65 281 and by 1.3e-12 .. 8.5e-11 at n = 131 073.  That
is BELOW the bound of 1e-9 for some pairs from about 500 pairs on and for every pair at the three largest sizes: there the sum tests
do not resolve a last-place error of ONE weight.  The weights are held by the record comparison instead (bit-equal to the oracle's
where the route keeps records); a wrong weight on every pair of a wave moves the sums by a wave's share, far above the bound.  The
figure decides nothing."""
import math

import numpy as np
import pytest

import sums_cases as S

f32 = np.float32


def reference_terms(orc, n, metric, weighting, rejection=1):
    """The reference of one shape with finite normals: sums, absolute sums, per-pair terms, the positions of the valid pairs, and what is
    needed to restate one pair (q, qn, records, means)."""
    tgt = S.target(False)
    pts, nrm, rgba, cluster, nan_pt = S.source(n, False, edges=n > 2)
    T = S.pose()
    q, qn = S.moved(orc, (pts, nrm), T)
    raw = S.matcher(orc, "knn3", tgt)(q)
    recs = S.records(orc, weighting, rejection, q, qn, rgba, tgt, raw)
    means = None
    if metric == 2:
        s0, _ = S.sums(0, q, qn, tgt, recs)
        means = (f32(s0[1:4] / s0[0]), f32(s0[4:7] / s0[0]))
    out, ab, X, at = S.R.sums(metric, q, tgt[0], recs, tgt_nrm=tgt[1], src_nrm_t=qn, means=means, terms=True)
    S.check_inputs(pts, cluster, nan_pt, S.valid_mask(q, tgt, recs), "n %d" % n)
    return dict(out=out, ab=ab, X=X, at=at, q=q, qn=qn, recs=recs, means=means, tgt=tgt)


def moves(r, metric):
    """(move of the sums when the least-contributing pair is dropped or doubled, moves when the weight of the least- / most-contributing
    pair grows by one unit in the last place), each the largest over the 33 sums, relative to the absolute sums."""
    share = (np.abs(r["X"][:, 1:34]) / (r["ab"][1:34] + 1e-300)).max(1)       # a pair's largest share of any sum
    out = [float(share.min())]
    for k in (int(np.argmin(share)), int(np.argmax(share))):
        i = r["at"][k]
        one = r["recs"][i:i + 1].copy()
        one["weight"] = (one["weight"] * f32(1 + 2.0 ** -23)).astype(f32)
        _, _, X1, _ = S.R.sums(metric, r["q"][i:i + 1], r["tgt"][0], one, tgt_nrm=r["tgt"][1], src_nrm_t=r["qn"][i:i + 1], means=r["means"], terms=True)
        out.append(float((np.abs(X1[0, 1:34] - r["X"][k, 1:34]) / (r["ab"][1:34] + 1e-300)).max()))
    return out


@pytest.mark.parametrize("n", S.SIZES)
def test_resolution_of_the_bound(orc, n):
    for metric in (0, 1, 2):
        for weighting in (0, 1):
            r = reference_terms(orc, n, metric, weighting)
            assert len(r["at"]) >= 1 and r["out"][0] == len(r["at"])
            pair, ulp_least, ulp_most = moves(r, metric)
            print("n %6d metric %d weighting %d: %6d valid, a dropped / doubled pair moves a sum by >= %.3g, one weight ulp by %.3g .. %.3g"
                  % (n, metric, weighting, len(r["at"]), pair, ulp_least, ulp_most))
            assert pair > 100 * S.TOL, (n, metric, weighting, pair)


def test_reference_fold_against_fsum(orc):
    """The reference folds its terms with numpy's sum over the first axis: a running sum per column, whose error is at most n 2^-53 of
    the absolute sum (7.3e-12 at n = 65 537, a hundredth of the bound).  math.fsum is exact."""
    n = 65537
    r = reference_terms(orc, n, 1, 1)
    X, out, ab = r["X"], r["out"], r["ab"]
    for a in range(34):
        exact = math.fsum(X[:, a].tolist())
        assert abs(out[a] - exact) <= len(X) * 2.0 ** -53 * ab[a], a
        assert abs(ab[a] - math.fsum(np.abs(X[:, a]).tolist())) <= len(X) * 2.0 ** -53 * ab[a], a
    assert out[0] == len(X)


def test_compare_rejects_what_it_should():
    """The comparison itself: a slot off by 2e-9 of its absolute sum, a wrong count and a NaN against a number all fail; the same kind of
    non-finite value passes only where it is allowed."""
    ref = np.zeros(34); ab = np.zeros(34)
    ref[0] = 10; ref[1:34] = np.linspace(-1, 1, 33); ab[1:34] = 4.0
    S.compare(ref.copy(), 10, ref, ab, "equal")
    for slot, delta in ((7, 8e-9), (33, -8e-9)):
        d = ref.copy(); d[slot] += delta
        with pytest.raises(AssertionError):
            S.compare(d, 10, ref, ab, "off")
    d = ref.copy(); d[5] += 3e-9
    assert S.compare(d, 10, ref, ab, "within") <= S.TOL
    with pytest.raises(AssertionError):
        S.compare(ref.copy(), 9, ref, ab, "count")
    d = ref.copy(); d[9] = np.nan
    with pytest.raises(AssertionError):
        S.compare(d, 10, ref, ab, "nan on the device", allow_nonfinite=True)
    rn = ref.copy(); rn[9] = np.nan; rn[10] = np.inf
    with pytest.raises(AssertionError):
        S.compare(rn.copy(), 10, rn, ab, "not allowed")
    S.compare(rn.copy(), 10, rn, ab, "same kind", allow_nonfinite=True)
    d = rn.copy(); d[10] = -np.inf
    with pytest.raises(AssertionError):
        S.compare(d, 10, rn, ab, "other infinity", allow_nonfinite=True)
