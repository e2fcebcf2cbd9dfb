"""Inputs and the fp64 reference of the sum tests (tests/test_gpu_sums.py on the device, tests/test_sums_host.py on the host).  Test
infrastructure only; needs the oracle, no GPU.

  SIZES                      the source sizes, each at an edge of a fold ("the accumulation routes")
  pair()                     the target frame of the depth/8 pair of tests/test_gpu_robust.py, 80 x 60, compacted and organised
  target(hostile)            the compacted target (a few thousand points); hostile: one infinite normal on a point that is matched
  organised_target(hostile)  the same frame as the 80 x 60 grid the projective matcher needs
  source(n, hostile)         n source points: the target's points tiled with jitter, NaN points on the wave / block edges, a compact far
                             cluster of cluster_size(n) points (n >= 1054), and with hostile a zero and a NaN normal
  reference(...)             oracle matcher -> orc.apply_weights -> orc.prune -> robust_restatement.sums: records, sums, absolute sums
  check_inputs(...)          what a case must satisfy to prove anything: the cluster empties a block, half of the rest is valid
  compare(...)               the three assertions of every comparison

Non-finite normals and the sums.  The validity filter of the loop (ICPOptimizer.h:596-598) looks at the points only, and a normal that is
not finite makes the rejection angle NaN, which keeps the pair.  Such a pair enters the point-to-plane rows (target normal) or the symmetric
rows (both normals) and every one of the 27 metric sums becomes NaN or infinite, on the device as in the reference.  The hostile normals are
therefore checked where they leave finite sums (point-to-point, every weighting and rejection: all 33 sums) and in kind elsewhere (the same
slots non-finite, of the same kind; count, sum s and sum d exact / to the bound); the point-to-plane and symmetric sums themselves are checked
on the same points with finite normals (the zero normal stays: it is finite)."""
import functools

import numpy as np

import robust_restatement as R

f32 = np.float32
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1054, 65281, 65537, 131073)
SMALL = (65, 257, 1054)           # the sizes of the 6-D and projective matchers
SEL = (257, 1054)                 # the sizes of the sel-indexed path
TOL = 1e-9                        # of |sum - reference| / (sum of the absolute terms), tests/test_gpu_robust.py's bound for the same quantity
MAX_DIST = 0.01
BLOCK = 256


def cluster_size(n):
    """Points of the far cluster, enough to empty one whole block of the fused routes wherever the run starts.  A grid of fewer than
    128 blocks gives a block 256 consecutive queries of the Morton order: 600 > 2 * 256 - 1.  From 128 blocks on (n > 32 512) the four
    waves of a block take stretches of 64 queries that lie 128 stretches (8 192 queries) apart (fused_wave_slot, dev_fused.hpp): the run
    must span three such steps and a stretch, wherever it starts.  tests/test_gpu_sums.py asserts with the library's own mapping
    (icp_debug_wave_slot) that a block ends up empty."""
    return 0 if n < 1054 else 600 if n <= 127 * BLOCK else 3 * 8192 + 600


K8 = np.array([[525.0 / 8, 0, 319.5 / 8], [0, 525.0 / 8, 239.5 / 8], [0, 0, 1]])
INF_TARGET = 2000                 # (compacted index) the target point whose normal is infinite in the hostile variant
NAN_POINTS = (0, 63, 64)          # and n - 1
ZERO_NORMAL, NAN_NORMAL = 5, 11
HITS_INF = 7                      # the source point made from target point INF_TARGET


def pose():
    from icp_amd import synth
    return synth.make_pose((0.002, -0.003, 0.0025), (0.002, -0.003, 0.001)).astype(f32)


@functools.lru_cache(maxsize=None)
def pair():
    from icp_amd import synth
    d = synth.rgbd_pair(0, width=80, height=60, K=K8)
    tp, tn, tc = synth.compact_valid(d["tgt_pts"], d["tgt_nrm"], d["tgt_rgba"])
    ok = np.isfinite(d["tgt_pts"]).all(1) & np.isfinite(d["tgt_nrm"]).all(1)
    return dict(tgt=(tp.astype(f32), tn.astype(f32), tc),
                organised=(d["tgt_pts"].astype(f32), d["tgt_nrm"].astype(f32), d["tgt_rgba"]), organised_of=np.flatnonzero(ok))


def target(hostile):
    tp, tn, tc = pair()["tgt"]
    tn = tn.copy()
    if hostile:
        tn[INF_TARGET, 1] = np.inf
    return tp, tn, tc


def organised_target(hostile):
    tp, tn, tc = pair()["organised"]
    tn = tn.copy()
    if hostile:
        tn[pair()["organised_of"][INF_TARGET], 1] = np.inf
    return tp, tn, tc


@functools.lru_cache(maxsize=None)
def _source(n, edges):
    sp, sn, sc = pair()["tgt"]           # the target's own points, jittered: S.pose() moves them by a few centimetres, well inside MAX_DIST
    m = len(sp)
    rng = np.random.default_rng(1000 + n)
    pick = (np.arange(n, dtype=np.int64) * 7919 + 13) % m
    if n > HITS_INF:
        pick[HITS_INF] = INF_TARGET
    pts = (sp[pick] + rng.normal(0, 2e-3, (n, 3))).astype(f32)
    nrm = (sn[pick] + rng.normal(0, 0.05, (n, 3))).astype(f32)
    nrm[4::9] = -nrm[4::9]                 # every ninth normal faces away: the rejection has something to remove
    rgba = sc[pick].copy(); rgba[:, :3] += rng.integers(-6, 7, (n, 3)).astype(np.uint8)      # (uint8 wrap-around, as weighting.h:28 has it)
    cluster = np.zeros(n, bool)
    if n >= 1054:
        # far beyond the rest on every axis: the rest keeps to the lower third of the bounding box, so whatever the axis order of a Morton
        # code over that box the cluster is one run at the end of the finite points (check_inputs asserts the premise)
        lo, hi = pts.min(0), pts.max(0)
        cluster[n - 20 - cluster_size(n):n - 20] = True
        pts[cluster] = (hi + 2 * (hi - lo) + 1 + rng.normal(0, 1e-3, (cluster_size(n), 3))).astype(f32)
    nan_pt = np.zeros(n, bool)
    if edges:
        for i in NAN_POINTS + (n - 1,):
            if i < n:
                nan_pt[i] = True
        pts[nan_pt] = np.nan
    return pts, nrm, rgba, cluster, nan_pt


def source(n, hostile, edges=True):
    """(points, normals, rgba, cluster mask, NaN-point mask).  edges=False (n <= 2 only needs it): no NaN points, so that the smallest
    sizes are also seen with every pair valid -- with them, index 0 and n - 1 leave nothing."""
    pts, nrm, rgba, cluster, nan_pt = _source(n, bool(edges))
    nrm = nrm.copy()
    if n > NAN_NORMAL:
        nrm[ZERO_NORMAL] = 0
        if hostile:
            nrm[NAN_NORMAL, 2] = np.nan
    return pts, nrm, rgba, cluster, nan_pt


def matcher(orc, kind, tgt, src_rgba=None):
    """q -> records of the oracle's matcher: "knn3", "knn6" (colour features) or "projective" (tgt: the organised target)."""
    tp, tn, tc = tgt
    if kind == "knn3":
        return lambda q: orc.knn3(q, tp, MAX_DIST)[0]
    if kind == "knn6":
        return lambda q: orc.knn6(q, src_rgba, tp, tc, MAX_DIST)[0]
    return lambda q: orc.projective(q, tp, 80, 60, K8, MAX_DIST)[0]


def moved(orc, src, T):
    return orc.transform_points(src[0], T), orc.transform_normals(src[1], T)


def records(orc, weighting, rejection, q, qn, src_rgba, tgt, raw):
    """The oracle's chain behind its matcher (oracle_post of tests/test_gpu_parity.py)."""
    tp, tn, tc = tgt
    m = orc.apply_weights(weighting, MAX_DIST, q, tp, qn, tn, src_rgba, tc, raw)
    return orc.prune(qn, tn, m) if rejection == 1 else m


def sums(metric, q, qn, tgt, recs, means=None):
    with np.errstate(invalid="ignore", over="ignore"):      # (the hostile normals)
        return R.sums(metric, q, tgt[0], recs, tgt_nrm=tgt[1], src_nrm_t=qn, means=means)


def valid_mask(q, tgt, recs):
    j = np.maximum(recs["idx"], 0)
    return (recs["idx"] >= 0) & np.isfinite(q).all(1) & np.isfinite(tgt[0][j]).all(1)


def check_inputs(q_src, cluster, nan_pt, valid, label):
    """From the reference alone: the cluster has no valid pair and lies in the upper half of the finite points' bounding box on every axis
    while every other finite point lies in the lower half -- the top bit of each axis of a Morton code over that box (k_query_keys) then
    separates them, and the cluster is ONE run of consecutive queries that starts behind the other finite points; and at least half of
    the other queries are valid."""
    rest = ~cluster & ~nan_pt
    if cluster.any():
        assert cluster.sum() == cluster_size(len(cluster)) and not valid[cluster].any(), label
        fin = np.isfinite(q_src).all(1)
        mid = (q_src[fin].min(0).astype(np.float64) + q_src[fin].max(0).astype(np.float64)) / 2
        assert (q_src[cluster] > mid).all() and (q_src[rest & fin] < mid).all(), label
    if rest.sum() >= 8:
        assert valid[rest].sum() * 2 >= rest.sum(), (label, int(valid[rest].sum()), int(rest.sum()))


def compare(dev_sums, dev_nv, ref, ref_abs, label, allow_nonfinite=False, means_unused=False):
    """Count exact; sums[1:34] within TOL of the reference relative to its sums of absolute terms.  allow_nonfinite: a slot the reference
    has as NaN / +inf / -inf must be the same kind on the device (the rest as above); otherwise every reference slot must be finite.
    means_unused: the fused matcher's point-to-plane epilogue (fused_block_epilogue, dev_fused.hpp) does not fold sum s and sum d --
    they feed only the means, which that metric never reads -- and stores exact zeros in slots 1..6: asserted as such, the other 27 compared."""
    assert dev_sums[0] == ref[0] and dev_nv == int(ref[0]), (label, dev_sums[0], dev_nv, ref[0])
    r, d, a = ref[1:34].copy(), np.asarray(dev_sums[1:34]), ref_abs[1:34]
    if means_unused:
        assert not d[:6].any() and not np.signbit(d[:6]).any(), (label, "sum s / sum d of the fused point-to-plane route are not +0", d[:6])
        r[:6] = 0.0
    fin = np.isfinite(r)
    assert allow_nonfinite or fin.all(), (label, "the reference is not finite")
    with np.errstate(invalid="ignore"):
        assert np.array_equal(np.isnan(r), np.isnan(d)) and np.array_equal(r[~fin & ~np.isnan(r)], d[~fin & ~np.isnan(r)]), (label, "non-finite slots differ")
        err = np.where(fin, np.abs(d - r) / (a + 1e-300), 0.0)
    k = int(np.argmax(err))
    assert err.max(initial=0.0) <= TOL, (label, "sum %d: %r against %r, off by %.3g of its absolute sum %r" % (k + 1, d[k], r[k], err.max(), a[k]))
    return float(err.max(initial=0.0))
