"""The projective matcher's crafted cases on the host: the oracle's orc_projective equals tests/projective_restatement.py bit for bit on
every size and threshold, and the cases contain what they claim -- every clipped window width at every alignment, exact two- and four-way
ties, queries exactly on the threshold, holes by x alone under a query.  The conditions are about the inputs and the two references; the
device meets the same records in tests/test_gpu_projective.py.  Run with -s for the counts per size."""
import collections

import numpy as np
import pytest

import projective_restatement as P
from support import bits

f32 = np.float32
BIG = (37, 29)


def oracle_records(orc, c, thr):
    return orc.projective(c["queries"], c["tgt"], c["W"], c["H"], c["K"], thr)


def test_query_count():
    assert sum(len(P.case(W, H)["queries"]) for W, H in P.SIZES) == 38424
    assert all(len(P.case(W, H)["queries"]) % 256 for W, H in P.SIZES)            # no size fills its last block of 256 threads


@pytest.mark.parametrize("size", P.SIZES, ids=lambda s: "%dx%d" % s)
def test_oracle_equals_restatement_and_the_cases_hold(orc, size):
    W, H = size
    c = P.case(W, H)
    q, tgt = c["queries"], c["tgt"]
    best, bi, info = P.case_scan(W, H)
    recs = {}
    for thr in P.THRESHOLDS:
        m, d2 = P.records(best, bi, info, thr)
        mo, do = oracle_records(orc, c, thr)
        assert np.array_equal(mo["idx"], m["idx"]) and np.array_equal(bits(mo["weight"]), bits(m["weight"])) and np.array_equal(bits(do), bits(d2)), (size, thr)
        recs[thr] = mo
    lo, mid, hi = (recs[t] for t in P.THRESHOLDS)
    ran = info["ran"]
    cols = collections.Counter(info["cols"][ran].tolist())
    rows = collections.Counter(info["rows"][ran].tolist())
    align = collections.Counter((info["u0"][ran] % 4).tolist())
    ties = collections.Counter(info["ties"][info["ties"] > 0].tolist())
    on_thr = best == f32(P.HALF_PIXEL_D2)
    print("%d x %d: %d queries, %d windows, matched %s at thresholds %s" % (W, H, len(q), ran.sum(), [int((recs[t]["weight"] > 0).sum()) for t in P.THRESHOLDS], list(P.THRESHOLDS)))
    print("  column counts %s" % sorted(cols.items()))
    print("  row counts %s" % sorted(rows.items()))
    print("  u0 mod 4 %s" % sorted(align.items()))
    print("  ties by multiplicity %s, d2 == 2^-14: %d" % (sorted(ties.items()), on_thr.sum()))

    # every clipped width, every alignment of the first column
    assert set(cols) == set(range(1, min(W, 25) + 1)), size
    if W >= 12:
        assert set(align) == {0, 1, 2, 3}, size
    # a tie resolves to the lowest linear index of the tied pixels: the window's distances once more in fp64 (exact on this lattice)
    for i in np.flatnonzero(info["ties"] > 1):
        us = info["u0"][i] + np.arange(info["cols"][i]); vs = info["v0"][i] + np.arange(info["rows"][i])
        js = (vs[:, None] * W + us[None, :]).ravel()
        with np.errstate(invalid="ignore", over="ignore"):
            d = ((q[i].astype(np.float64) - tgt[js].astype(np.float64)) ** 2).sum(1)
        d[tgt[js, 0] == P.MINF] = np.nan
        same = js[d == np.nanmin(d)]
        assert len(same) == info["ties"][i] and hi["idx"][i] == same.min() and float(best[i]) == np.nanmin(d), (size, i)
    # exactly on the threshold: matched at 2^-14, not at 1e-9
    assert (mid["weight"][on_thr] == 1).all() and (mid["idx"][on_thr] >= 0).all() and (lo["idx"][on_thr] == -1).all(), size
    # a hole by x alone (y and z finite) under a query: never the match, although its y and z would make it the nearest pixel
    x_only = np.zeros(W * H, bool); x_only[c["defects"]["x_only"]] = True
    whole = ran & (c["hu"] % 1 == 0) & (c["hv"] % 1 == 0) & (c["hu"] < W) & (c["hv"] < H)
    pix = np.where(whole, c["hv"] * W + c["hu"], 0).astype(np.int64)
    over_hole = whole & x_only[pix]
    for m in (lo, mid, hi):
        matched = m["weight"] > 0
        assert not (tgt[m["idx"][matched], 0] == P.MINF).any(), size
        assert not (m["idx"][over_hole] == pix[over_hole]).any(), size
    assert (lo["idx"][over_hole] == -1).all() and (hi["idx"][over_hole] >= 0).all(), size
    if W * H > 50:
        assert len(c["defects"]["x_only"]) == int(round(0.025 * W * H)) > 0 and np.isfinite(tgt[c["defects"]["x_only"], 1:]).all(), size
    # the odd queries: Match{0, 0.f} for x == -inf; no window for the rest, but for the denormal depth (0, 0, 1e-40): 0 / 1e-40 = 0
    # projects it to the principal point, a unit away from the plane, where an image of 25 columns and rows or more has a window
    odd = hi[-P.N_ODD:]; rest = np.array([1, 2, 3, 4, 6, 7, 8])
    assert (odd["idx"][0], odd["weight"][0]) == (0, 0.0) and (odd["idx"][rest] == -1).all() and not ran[-P.N_ODD:][rest].any(), size
    assert bool(ran[-P.N_ODD + 5]) == (W >= 25 and H >= 25) == bool(odd["idx"][5] >= 0), size
    # the underflow quirk and the far edge: uf < 12 never matches, uf = W + 12 and beyond has no window
    assert not ran[(c["hu"] < 11.5) | (c["hv"] < 11.5)].any() and not ran[(c["hu"] >= W + 11.5) | (c["hv"] >= H + 11.5)].any(), size

    if size == BIG:
        assert over_hole.sum() > 0
        assert ties[2] >= 1000 and ties[4] >= 200, ties
        assert on_thr.sum() >= 500, on_thr.sum()
        assert len(rows) == 25 and set(cols) == set(range(1, 26))
    if size == (25, 3):
        assert set(rows) == {1, 2, 3} and len(cols) == 25
    if size == (12, 5):
        assert (hi["weight"] > 0).sum() > 200            # an image narrower than the window, reached from uf >= 12
    if size == (1, 1):
        assert (hi["idx"] >= 0).sum() == 5 and (hi["weight"] > 0).sum() == 4      # (the fifth: Match{0, 0.f}; all four 11.5 or 12 pixels away)


def test_restatement_rounds_half_away_from_zero():
    for a, r in ((0.5, 1.0), (1.5, 2.0), (2.5, 3.0), (-0.5, -1.0), (-2.5, -3.0), (0.49999997, 0.0), (8388609.0, 8388609.0), (12.4999, 12.0)):
        assert P.round_half_away(f32(a)) == f32(r), a
    assert np.isnan(P.round_half_away(f32(np.nan))) and P.round_half_away(f32(np.inf)) == np.inf


def test_wavy_pair_is_usable(orc):
    """The pair of the one-iteration device test: a full-rank problem with the defects and odd queries in the source."""
    d = P.wavy_pair()
    W, H = d["W"], d["H"]
    assert len(d["tgt_pts"]) == W * H and len(d["src_pts"]) == W * H + P.N_ODD
    assert np.isfinite(d["tgt_pts"]).all() and np.isfinite(d["tgt_nrm"]).all() and np.isfinite(d["src_nrm"]).all()
    assert (d["src_pts"][:, 0] == P.MINF).sum() >= 2 * int(round(0.025 * W * H))
    m, _ = orc.projective(d["src_pts"], d["tgt_pts"], W, H, d["K"], 0.01)
    assert 100 < (m["weight"] > 0).sum() < W * H
