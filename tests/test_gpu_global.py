"""Global registration on the device (icp_register_global: FPFH features, feature matching, RANSAC) against the numpy restatement of its
contract (tests/global_restatement.py), stage by stage and teacher-forced: each stage's restatement is fed what the device produced for
the stage before, so every comparison is exact or has a bound that follows from the contract."""
import numpy as np
import pytest

import global_cases as gc
import global_restatement as gr
from conftest import pose_error
from support import bits

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-5
EXCLUDE_MARGIN, EXCLUDE_GAP = 1e-6, 1e-9      # a point may be left out of the SPFH comparison only inside these (bin units; ||a1| - |a2||)


def ulps(a, b):
    """distance in fp32 units in the last place between finite arrays of equal sign structure (FPFH values are >= 0)"""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def configure(ctx, knn_backend=1, metric=1, n_iterations=20, max_distance=0.0003):          # not support.configure: the backend comes first and
                                                                                            # the selection fields are left as they are
    p = ctx.params
    p.metric = metric; p.matching = 0; p.weighting = 0; p.rejection = 1; p.color_icp = 0; p.multires = 0
    p.n_iterations = n_iterations; p.max_distance = max_distance; p.knn_backend = knn_backend
    ctx.push_params()


def load(ctx, b, knn_backend=1):                              # not support.load: configures too, and loads no colours
    configure(ctx, knn_backend)
    ctx.set_target(b["tgt_pts"], b["tgt_nrm"])
    ctx.set_source(b["src_pts"], b["src_nrm"])


_REST = {}


def restated(bunny, which, k):
    """the restatement's features of a bunny cloud, computed once per (cloud, k) and shared"""
    if (which, k) not in _REST:
        p, n = (bunny["src_pts"], bunny["src_nrm"]) if which == "source" else (bunny["tgt_pts"], bunny["tgt_nrm"])
        _REST[(which, k)] = gr.features(p, n, k)
    return _REST[(which, k)]


@pytest.mark.parametrize("knn_backend", [0, 1])
@pytest.mark.parametrize("k", [5, 10, 20])
def test_neighbours_equal_a_brute_force_sort(gpu_ctx_factory, bunny, k, knn_backend):
    """knn_backend 1: the target's lists come from its own tree, 0: from the scratch tree (the source's always do)."""
    ctx = gpu_ctx_factory()
    load(ctx, bunny, knn_backend)
    ctx.set_global_options(k=k)
    for which in ("source", "target"):
        idx, d2 = ctx.feature_neighbours(which)
        r = restated(bunny, which, k)
        assert np.array_equal(idx, r["idx"]), which
        assert np.array_equal(bits(d2), bits(r["d2"])), which


@pytest.mark.parametrize("k", [5, 10, 20])
def test_spfh_equals_restatement(gpu_ctx_factory, bunny, k):
    ctx = gpu_ctx_factory()
    load(ctx, bunny)
    ctx.set_global_options(k=k)
    for which in ("source", "target"):
        counts, pairs = ctx.spfh(which)
        r = restated(bunny, which, k)
        excluded = (r["margin"] < EXCLUDE_MARGIN) | (r["gap"] < EXCLUDE_GAP)
        print("%s k=%d: min margin %.3g bin units, min ||a1|-|a2|| %.3g, excluded %d" % (which, k, r["margin"].min(), r["gap"].min(), excluded.sum()))
        assert not excluded.any()                      # none on the bunny (measured on the CPU); the contract would allow 0.1 %
        assert np.array_equal(pairs, r["pairs"]), which
        assert np.array_equal(counts, r["counts"]), which


def handmade_cloud():
    """40 points: 30 scattered ones with unit normals, then the special cases (indices in the comments)."""
    rng = np.random.default_rng(42)
    p = rng.uniform(-0.05, 0.05, (40, 3)).astype(np.float32)
    n = rng.normal(size=(40, 3)); n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(np.float32)
    p[30] = [np.nan, 0.0, 0.0]                                   # NaN position
    p[31] = [0.01, np.inf, 0.0]                                  # Inf position
    n[32] = [0.0, np.nan, 0.0]                                   # NaN normal
    n[33] = [0.0, 0.0, 0.0]                                      # zero normal
    p[34] = p[0]; p[35] = p[0]                                   # coincident points (d2 = 0: listed, no pair)
    p[36] = [0.2, 0.0, 0.0]; p[37] = [0.2 + 2.0 ** -9, 0.0, 0.0]   # far from the rest, nearest to each other ...
    n[36] = [1.0, 0.0, 0.0]; n[37] = [1.0, 0.0, 0.0]             # ... with normals parallel to dp: |dp x n1| = 0 exactly, the pair skipped
    n[38] = [0.0, 0.0, -np.inf]                                  # Inf normal
    return p, n


def test_handmade_cloud(gpu_ctx_factory):
    p, n = handmade_cloud()
    ctx = gpu_ctx_factory()
    configure(ctx)
    ctx.set_target(p, n); ctx.set_source(p, n)
    for k in (5, 10):
        ctx.set_global_options(k=k)
        r = gr.features(p, n, k)
        fin = np.isfinite(r["margin"])
        assert r["margin"][fin].min() > EXCLUDE_MARGIN and r["gap"][np.isfinite(r["gap"])].min() > EXCLUDE_GAP      # (the comparison below is exact: no pair near a boundary)
        for which in ("source", "target"):
            idx, d2 = ctx.feature_neighbours(which)
            counts, pairs = ctx.spfh(which)
            F = ctx.features(which)
            assert np.array_equal(idx, r["idx"]) and np.array_equal(bits(d2), bits(r["d2"]))
            assert np.array_equal(counts, r["counts"]) and np.array_equal(pairs, r["pairs"])
            assert np.array_equal(np.isnan(F), np.isnan(r["F"]))
            ok = ~np.isnan(F)
            assert ulps(F[ok], r["F"][ok]).max() <= 2
        # what the special points must show
        assert (r["idx"][30] == -1).all() and (r["idx"][31] == -1).all() and r["pairs"][30] == 0 and r["pairs"][31] == 0
        assert r["pairs"][32] == 0 and np.isnan(r["F"][[30, 31, 32, 38]]).all()
        assert set(r["idx"][0][:3]) == {0, 34, 35} and (r["d2"][0][:3] == 0).all()
        assert r["idx"][36][1] == 37 and r["pairs"][36] == k - 2                     # the parallel pair is skipped, the other neighbours count


def test_two_valid_points(gpu_ctx_factory):
    """A cloud of 2 valid points (and a NaN one): each has one pair; registration has fewer than 3 correspondences: a status code."""
    from icp_amd import binding
    p = np.array([[0, 0, 0], [np.nan, 0, 0], [0.01, 0.002, 0]], np.float32)
    n = np.array([[0, 0, 1], [0, 0, 1], [0, 0.6, 0.8]], np.float32)
    ctx = gpu_ctx_factory()
    configure(ctx)
    ctx.set_target(p, n); ctx.set_source(p, n)
    ctx.set_global_options(k=5)
    r = gr.features(p, n, 5)
    counts, pairs = ctx.spfh("source")
    assert pairs.tolist() == [1, 0, 1] and np.array_equal(counts, r["counts"]) and np.array_equal(pairs, r["pairs"])
    F = ctx.features("target")
    assert np.array_equal(np.isnan(F), np.isnan(r["F"])) and np.isnan(F[1]).all() and not np.isnan(F[[0, 2]]).any()
    si, ti = ctx.match_features()
    es, et = gr.correspondences(F, F, 1, True)          # (the two rows are equal: both match row 0, the mutual test keeps (0, 0) only)
    assert np.array_equal(si, es) and np.array_equal(ti, et) and len(si) < 3
    poses, recs, rc = ctx.register_global(check=False)
    assert rc == binding.ERR_NO_CORRESPONDENCES and poses == [] and len(recs) == 0
    with pytest.raises(binding.IcpError):
        ctx.register_global()


@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("k", [5, 20])
def test_fpfh_values(gpu_ctx_factory, bunny, k, stride):
    """Device F against the restatement fed the device's own SPFH and neighbour lists: the same fp64 sums in the same order, so 0 or 1 ulp
    (fp64 division and sqrt are correctly rounded on both sides); 2 ulp asserted."""
    ctx = gpu_ctx_factory()
    load(ctx, bunny)
    ctx.set_global_options(k=k, feature_stride=stride)
    for which, p, n in (("source", bunny["src_pts"], bunny["src_nrm"]), ("target", bunny["tgt_pts"], bunny["tgt_nrm"])):
        idx, d2 = ctx.feature_neighbours(which)
        counts, pairs = ctx.spfh(which)
        F = ctx.features(which)
        R = gr.fpfh(p, n, idx, d2, counts, pairs, stride)
        assert F.shape == R.shape == ((len(p) + stride - 1) // stride, 33)
        assert not np.isnan(F).any() and not np.isnan(R).any()
        u = ulps(F, R)
        print("%s k=%d stride=%d: max |F - restatement| = %d ulp (%d of %d values differ)" % (which, k, stride, u.max(), (u > 0).sum(), u.size))
        assert u.max() <= 2


def matcher_clouds(bunny, case):
    sp, sn, tp, tn = bunny["src_pts"], bunny["src_nrm"], bunny["tgt_pts"], bunny["tgt_nrm"]
    if case == "1x1":                               # one keypoint on either side (stride beyond the cloud), a valid feature each
        return sp[:63], sn[:63], tp[:65], tn[:65], 100
    if case == "63x65":
        return sp[:63], sn[:63], tp[:65], tn[:65], 1
    if case == "257x256":
        return sp[:257], sn[:257], tp[:256], tn[:256], 1
    if case == "full":
        return sp, sn, tp, tn, 1
    if case == "full_stride3":
        return sp, sn, tp, tn, 3
    if case == "duplicates":                        # every target point twice: rows i and i + 300 are equal bit for bit, the lower index must win
        return sp[:300], sn[:300], np.concatenate([tp[:300], tp[:300]]), np.concatenate([tn[:300], tn[:300]]), 1
    if case == "nan_rows":
        sn = sn[:400].copy(); tn = tn[:500].copy()
        sn[::7] = np.nan; tn[::5] = np.nan; tn[3] = np.nan
        return sp[:400], sn, tp[:500], tn, 1
    raise ValueError(case)


@pytest.mark.parametrize("mutual", [1, 0])
@pytest.mark.parametrize("case", ["1x1", "63x65", "257x256", "full", "full_stride3", "duplicates", "nan_rows"])
def test_matcher_equals_restatement(gpu_ctx_factory, bunny, case, mutual):
    sp, sn, tp, tn, stride = matcher_clouds(bunny, case)
    ctx = gpu_ctx_factory()
    configure(ctx)
    ctx.set_target(tp, tn); ctx.set_source(sp, sn)
    ctx.set_global_options(k=10, feature_stride=stride, mutual=mutual)
    si, ti = ctx.match_features()
    Fs, Ft = ctx.features("source"), ctx.features("target")
    es, et = gr.correspondences(Fs, Ft, stride, bool(mutual))
    assert np.array_equal(si, es) and np.array_equal(ti, et)
    assert (np.diff(si) > 0).all()
    if case == "1x1":
        assert Fs.shape == (1, 33) and Ft.shape == (1, 33) and si.tolist() == [0] and ti.tolist() == [0]
    if case == "duplicates":
        assert np.array_equal(bits(Ft[:300]), bits(Ft[300:])) and (ti < 300).all() and len(ti) > 0
        if mutual:                                  # (the backward match of a duplicated row is the same for both copies: the pairs survive)
            assert len(si) > 30
    if case == "nan_rows":
        assert np.isnan(Fs[::7]).all() and np.isnan(Ft[::5]).all()
        assert not np.isin(si, np.arange(0, 400, 7)).any() and not np.isin(ti, np.arange(0, 500, 5)).any() and 3 not in ti
    if case == "full" and not mutual:
        assert len(si) == len(sp)


@pytest.mark.parametrize("seed", [0, 7])
def test_ransac_teacher_forced(gpu_ctx_factory, bunny, seed):
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    load(ctx, bunny)
    H = 4096
    ctx.set_global_options(k=20, mutual=1, n_hypotheses=H, edge_similarity=0.9, inlier_distance=0.005, seed=seed, n_best=16)
    poses, recs, rc = ctx.register_global()
    hyp = ctx.global_hypotheses()
    si, ti = ctx.match_features()
    cs, ct = bunny["src_pts"][si], bunny["tgt_pts"][ti]
    assert rc == 0 and len(hyp) == H and len(si) >= 3
    dr = gr.draws(seed, H, len(si))
    assert np.array_equal(hyp["draw"], dr)
    status, rposes = gr.ransac_fit(cs, ct, dr, 0.9)
    assert np.array_equal(hyp["status"] == gr.REPEATED, status == gr.REPEATED)
    assert np.array_equal(hyp["status"] == gr.EDGES, status == gr.EDGES)
    assert np.array_equal(hyp["status"], status)
    valid = status == gr.VALID
    assert valid.sum() > 100
    err = np.abs(hyp["pose"][valid] - rposes[valid]).max()
    print("seed %d: M = %d, %d valid hypotheses, max |pose - restatement| = %.3g" % (seed, len(si), valid.sum(), err))
    assert err < POSE_TOL
    eye = np.eye(4, dtype=np.float32).reshape(16)
    assert (hyp["pose"][~valid] == eye).all() and (hyp["n_inliers"][~valid] == 0).all() and (hyp["sum_d2"][~valid] == 0).all()
    n_in, sums = gr.ransac_score(hyp["pose"], hyp["status"], cs, ct, 0.005)      # scored at the DEVICE's fp32 poses
    assert np.array_equal(hyp["n_inliers"], n_in)
    assert np.allclose(hyp["sum_d2"], sums, rtol=1e-12, atol=0.0)
    order = gr.ranking(hyp["status"], hyp["n_inliers"], hyp["sum_d2"])            # a host re-sort of the device's records
    assert len(poses) == 16 and len(recs) == 16
    assert np.array_equal(recs, hyp[order[:16]])
    for r in range(16):
        assert np.array_equal(binding.pose_to_c(poses[r]), hyp["pose"][order[r]])
    poses2, recs2, _ = ctx.register_global()                                      # two runs agree bit for bit
    assert hyp.tobytes() == ctx.global_hypotheses().tobytes() and recs.tobytes() == recs2.tobytes()


# ---- the feature pass beyond the bunny's shapes: exact ties, sizes around K / the block / a tree level, a deeper tree, coincident points ----
def load_same(ctx, p, nr, k, knn_backend=1):
    """one cloud as target and source: the target's lists come from its own tree (knn_backend 1) or the scratch tree (0), the source's
    always from the scratch tree"""
    configure(ctx, knn_backend)
    ctx.set_target(p, nr); ctx.set_source(p, nr)
    ctx.set_global_options(k=k)


def assert_features(ctx, which, p, nr, r, rows=None, label=""):
    """The device's lists and SPFH of `which` bit for bit against the restatement r (of the points `rows`, default all), its F within 2 ulp
    of the restatement fed the device's own lists and SPFH (every row), the NaN rows the same.  Returns the largest ulp distance of F."""
    idx, d2 = ctx.feature_neighbours(which); counts, pairs = ctx.spfh(which); F = ctx.features(which)
    k = r["idx"].shape[1]
    assert idx.shape == d2.shape == (len(p), k) and counts.shape == (len(p), 33) and pairs.shape == (len(p),) and F.shape == (len(p), 33), label
    at = slice(None) if rows is None else rows
    assert np.array_equal(idx[at], r["idx"]), (label, which)
    assert np.array_equal(bits(d2[at]), bits(r["d2"])), (label, which)
    excluded = (r["margin"] < EXCLUDE_MARGIN) | (r["gap"] < EXCLUDE_GAP)
    assert not excluded.any(), (label, r["margin"].min(), r["gap"].min())      # (a condition on the inputs: tests/test_global_host.py)
    assert np.array_equal(pairs[at], r["pairs"]), (label, which)
    assert np.array_equal(counts[at], r["counts"]), (label, which)
    R = gr.fpfh(p, nr, idx, d2, counts, pairs)
    assert np.array_equal(np.isnan(F), np.isnan(R)), (label, which)
    assert np.array_equal(np.isnan(F).any(axis=1), np.isnan(F).all(axis=1))
    ok = ~np.isnan(F)
    u = int(ulps(F[ok], R[ok]).max()) if ok.any() else 0
    assert u <= 2, (label, which, u)
    return u


_CASES = {}


def restated_case(name, k, make):
    if (name, k) not in _CASES:
        p, nr = make()
        _CASES[(name, k)] = (p, nr, gr.features(p, nr, k))
    return _CASES[(name, k)]


@pytest.mark.parametrize("knn_backend", [0, 1])
@pytest.mark.parametrize("k", [5, 10, 20])
def test_exact_ties_on_lattices(gpu_ctx_factory, k, knn_backend):
    """Integer lattices: every neighbour list holds an exact fp32 distance tie (tests/test_global_host.py), decided by the lowest index."""
    ctx = gpu_ctx_factory()
    for name in ("plane", "block"):
        p, nr, r = restated_case(name, k, lambda: gc.lattices()[name])
        load_same(ctx, p, nr, k, knn_backend)
        for which in ("source", "target"):
            u = assert_features(ctx, which, p, nr, r, label="%s k=%d backend=%d" % (name, k, knn_backend))
            print("lattice %s k=%d backend %d %s: max |F - restatement| = %d ulp" % (name, k, knn_backend, which, u))


@pytest.mark.parametrize("k", [5, 20])
def test_sizes_around_k_the_block_and_a_tree_level(gpu_ctx_factory, k):
    ctx = gpu_ctx_factory()
    for n in gc.SIZES(k):
        p, nr = gc.uniform_cloud(n, 1000 * k + n)
        r = gr.features(p, nr, k)
        load_same(ctx, p, nr, k)
        for which in ("source", "target"):
            u = assert_features(ctx, which, p, nr, r, label="n=%d k=%d" % (n, k))
            print("uniform n=%d k=%d %s: max |F - restatement| = %d ulp" % (n, k, which, u))
            idx, d2 = ctx.feature_neighbours(which); _, pairs = ctx.spfh(which); F = ctx.features(which)
            assert ((idx >= 0).sum(axis=1) == min(n, k)).all() and (idx[:, 0] == np.arange(n)).all() and (d2[:, 0] == 0).all()
            assert (pairs == min(n, k) - 1).all()
            if n == 1:                                   # the point itself, no pair, no feature
                assert idx[0].tolist() == [0] + [-1] * (k - 1) and np.isinf(d2[0, 1:]).all() and pairs[0] == 0 and np.isnan(F).all()
            if n == 2:                                   # one pair each
                assert idx[:, :2].tolist() == [[0, 1], [1, 0]] and (idx[:, 2:] == -1).all() and pairs.tolist() == [1, 1] and not np.isnan(F).any()


@pytest.mark.parametrize("k", [10, 20])
def test_a_deeper_tree_on_a_sample_of_rows(gpu_ctx_factory, k):
    """A 40 800-point scan: lists and SPFH of 2 000 rows against the rows form of the restatement, F of every row against the restatement
    fed the device's lists and SPFH, the shapes and the NaN pattern of the whole output."""
    p, nr = gc.deep_scan()
    assert len(p) == 40800 and np.isfinite(p).all() and np.isfinite(nr).all()
    rows = gc.deep_rows(len(p))
    idx, d2 = gr.neighbour_lists(p, k, rows=rows)
    counts, pairs, margin, gap = gr.spfh(p, nr, idx, d2, rows=rows)
    r = dict(idx=idx, d2=d2, counts=counts, pairs=pairs, margin=margin, gap=gap)
    ctx = gpu_ctx_factory()
    load_same(ctx, p, nr, k)
    for which in ("source", "target"):
        u = assert_features(ctx, which, p, nr, r, rows=rows, label="scan k=%d" % k)
        print("scan k=%d %s: max |F - restatement| = %d ulp" % (k, which, u))
        _, dev_pairs = ctx.spfh(which)
        assert np.array_equal(np.isnan(ctx.features(which)).all(axis=1), dev_pairs == 0)


def test_more_coincident_points_than_k(gpu_ctx_factory):
    """25 copies of one point, k = 20: a copy's list is the 20 lowest-index copies at d2 = 0, it has no pair and no feature."""
    p, nr, copies = gc.coincident_cloud()
    r = gr.features(p, nr, 20)
    ctx = gpu_ctx_factory()
    load_same(ctx, p, nr, 20)
    for which in ("source", "target"):
        assert_features(ctx, which, p, nr, r, label="coincident")
        idx, d2 = ctx.feature_neighbours(which); _, pairs = ctx.spfh(which); F = ctx.features(which)
        assert (d2[copies] == 0).all() and (idx[copies] == copies[:20]).all()
        assert (pairs[copies] == 0).all()
        assert np.isnan(F[copies]).all() and not np.isnan(np.delete(F, copies, axis=0)).any()


# ---- RANSAC beyond H in {512, 4096} and M ~ 655 ----
def teacher_forced_ransac(ctx, src_pts, tgt_pts, seed, H, n_best, edge_similarity=0.9, inlier_distance=0.005, label=""):
    """test_ransac_teacher_forced's comparisons after ctx.set_global_options(...): draws, statuses, poses, counts, sums, ranking, the
    number of records, two runs byte for byte.  Returns (hyp, status of the restatement, the ranking, poses, recs, rc)."""
    from icp_amd import binding
    poses, recs, rc = ctx.register_global(check=False)
    hyp = ctx.global_hypotheses()
    si, ti = ctx.match_features()
    cs, ct = src_pts[si], tgt_pts[ti]
    assert len(hyp) == H and len(si) >= 3, label
    dr = gr.draws(seed, H, len(si))
    assert np.array_equal(hyp["draw"], dr), label
    status, rposes = gr.ransac_fit(cs, ct, dr, edge_similarity)
    assert np.array_equal(hyp["status"], status), (label, np.bincount(hyp["status"], minlength=4), np.bincount(status, minlength=4))
    valid = status == gr.VALID
    err = float(np.abs(hyp["pose"][valid] - rposes[valid]).max()) if valid.any() else 0.0
    eye = np.eye(4, dtype=np.float32).reshape(16)
    assert (hyp["pose"][~valid] == eye).all() and (hyp["n_inliers"][~valid] == 0).all() and (hyp["sum_d2"][~valid] == 0).all(), label
    assert (hyp["reserved"] == 0).all()
    n_in, sums = gr.ransac_score(hyp["pose"], hyp["status"], cs, ct, inlier_distance)      # scored at the DEVICE's fp32 poses
    rel = float((np.abs(hyp["sum_d2"] - sums) / np.where(sums > 0, sums, 1.0)).max())
    print("%s: M = %d, H = %d, statuses %s, max |pose - restatement| = %.3g, max relative sum_d2 error = %.3g"
          % (label, len(si), H, np.bincount(status, minlength=4).tolist(), err, rel))
    assert err < POSE_TOL, (label, err)
    assert np.array_equal(hyp["n_inliers"], n_in), label
    assert np.allclose(hyp["sum_d2"], sums, rtol=1e-12, atol=0.0), label
    order = gr.ranking(hyp["status"], hyp["n_inliers"], hyp["sum_d2"])            # a host re-sort of the device's records
    want = min(n_best, len(order))
    assert rc == (0 if want else binding.ERR_NO_CORRESPONDENCES), label
    assert len(poses) == want and len(recs) == want, label
    assert np.array_equal(recs, hyp[order[:want]]), label
    for r in range(want):
        assert np.array_equal(binding.pose_to_c(poses[r]), hyp["pose"][order[r]]), label
    _, recs2, rc2 = ctx.register_global(check=False)                              # two runs agree byte for byte
    assert rc2 == rc and hyp.tobytes() == ctx.global_hypotheses().tobytes() and recs.tobytes() == recs2.tobytes(), label
    return hyp, status, order, poses, recs, rc


def test_line_cloud_every_hypothesis_degenerate_or_repeated(gpu_ctx_factory):
    from icp_amd import binding
    p, nr = gc.line_cloud()
    ctx = gpu_ctx_factory()
    for mutual in (1, 0):
        load_same(ctx, p, nr, 10)
        ctx.set_global_options(k=10, mutual=mutual, n_hypotheses=gc.LINE_H, seed=gc.LINE_SEED)
        hyp, status, order, poses, recs, rc = teacher_forced_ransac(ctx, p, p, gc.LINE_SEED, gc.LINE_H, 16, label="line mutual=%d" % mutual)
        assert np.isin(hyp["status"], (gr.REPEATED, gr.DEGENERATE)).all() and (hyp["status"] == gr.DEGENERATE).sum() > 400
        assert rc == binding.ERR_NO_CORRESPONDENCES and poses == [] and len(recs) == 0
        assert "no valid hypothesis" in ctx.lib.icp_last_error(ctx.h).decode()
        assert (hyp["pose"] == np.eye(4, dtype=np.float32).reshape(16)).all() and (hyp["n_inliers"] == 0).all() and (hyp["sum_d2"] == 0).all()


def test_ribbon_cloud_on_both_sides_of_the_collinearity_threshold(gpu_ctx_factory):
    p, nr = gc.ribbon_cloud()
    ctx = gpu_ctx_factory()
    load_same(ctx, p, nr, 10)
    ctx.set_global_options(k=10, mutual=1, n_hypotheses=gc.RIBBON_H, seed=gc.RIBBON_SEED)
    hyp, status, order, poses, recs, rc = teacher_forced_ransac(ctx, p, p, gc.RIBBON_SEED, gc.RIBBON_H, 16, label="ribbon")
    count = np.bincount(hyp["status"], minlength=4)
    assert rc == 0 and count[gr.VALID] >= 50 and count[gr.DEGENERATE] >= 50 and count[gr.EDGES] == 0, count


@pytest.mark.parametrize("n,start,H", gc.EDGE_CASES)
def test_edges_of_h_and_m(gpu_ctx_factory, bunny, n, start, H):
    """M = n correspondences (n source points, no mutual test: tests/test_global_host.py) and H hypotheses, with and without the edge test."""
    sp, sn, tp, tn = gc.sub_clouds(bunny, n, start)
    seed = gc.edge_seed(n, start, H)
    ctx = gpu_ctx_factory()
    configure(ctx)
    ctx.set_target(tp, tn); ctx.set_source(sp, sn)
    for es in gc.EDGE_SIMILARITIES:
        ctx.set_global_options(k=gc.SUB_K, mutual=0, n_hypotheses=H, edge_similarity=es, seed=seed, n_best=16)
        hyp, status, _, _, _, _ = teacher_forced_ransac(ctx, sp, tp, seed, H, 16, edge_similarity=es, label="M=%d (from %d) H=%d es=%.1f" % (n, start, H, es))
        assert len(ctx.match_features()[0]) == n
        assert 0 <= int(hyp["draw"].min()) and int(hyp["draw"].max()) < n
        if es == 0.0 and H >= 63 and (n, start) not in ((3, 0), (4, 0)):
            assert (status == gr.VALID).sum() > H // 8


def test_n_best_above_the_valid_count_and_the_hand_over_to_multistart(gpu_ctx_factory, bunny):
    """n_best = 256 with fewer valid hypotheses: every valid one comes back, in the restatement's ranking; then all of them as the starts of
    one icp_run_multistart -- more than one 64-start block of its score fold -- each against icp_run."""
    from support import assert_matches_icp_run, expected_best
    ctx = gpu_ctx_factory()
    configure(ctx, knn_backend=1, metric=1, n_iterations=5, max_distance=0.0003)
    ctx.set_target(bunny["tgt_pts"], bunny["tgt_nrm"]); ctx.set_source(bunny["src_pts"], bunny["src_nrm"])
    ctx.set_global_options(k=gc.N_BEST_K, mutual=1, n_hypotheses=gc.N_BEST_H, seed=0, n_best=256)
    hyp, status, order, poses, recs, rc = teacher_forced_ransac(ctx, bunny["src_pts"], bunny["tgt_pts"], 0, gc.N_BEST_H, 256, label="n_best")
    count = int((status == gr.VALID).sum())
    assert rc == 0 and 65 <= count <= 255
    assert len(poses) == len(recs) == count == len(order)
    assert np.array_equal(recs, hyp[order])
    res, _, best = assert_matches_icp_run(ctx, poses)
    assert len(res) == count and best == expected_best(res)


def rigid_fit(a, b):
    """the rigid pose taking points a onto b (fp64 Kabsch)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    am, bm = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((b - bm).T @ (a - am))
    R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = bm - R @ am
    return T


def moved_source(bunny, trial):
    """the bunny source under the seeded motion of a trial, and the true pose that takes it onto the target"""
    rng = np.random.default_rng(trial)
    axis = rng.normal(size=3); angle = rng.uniform(1, 3); tr = 0.1 * rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    Mv = np.eye(4); Mv[:3, :3] = R; Mv[:3, 3] = tr
    p = (bunny["src_pts"].astype(np.float64) @ R.T + tr).astype(np.float32)
    n = (bunny["src_nrm"].astype(np.float64) @ R.T).astype(np.float32)
    T0 = rigid_fit(bunny["src_pts"][bunny["gt_src_idx"]], bunny["tgt_pts"][bunny["gt_tgt_idx"]])
    return p, n, T0 @ np.linalg.inv(Mv)


# The largest difference between globalreg.align's pose and the pose icp_run reaches from the true pose, over the four trials, as measured
# on an MI355X (4.88e-5 / 4.88e-5 / 4.89e-5 / 4.88e-5 rad and 7.75e-6 / 5.36e-6 / 4.77e-6 / 6.31e-6 m); the test asserts 10 x these, and they must stay below 0.01 rad and 1 mm: beyond that it is another minimum.
E2E_MEASURED_RAD, E2E_MEASURED_M = 4.89e-5, 7.75e-6


@pytest.mark.parametrize("trial", [0, 1, 2, 3])
def test_end_to_end_from_an_unknown_pose(gpu_ctx_factory, bunny, trial):
    from icp_amd import globalreg
    p, n, truth = moved_source(bunny, trial)
    ctx = gpu_ctx_factory()
    configure(ctx, knn_backend=1, metric=1, n_iterations=20, max_distance=0.0003)
    ctx.set_target(bunny["tgt_pts"], bunny["tgt_nrm"]); ctx.set_source(p, n)
    pose, results, records, best = globalreg.align(ctx, k=20, mutual=1, n_hypotheses=4096, inlier_distance=0.005, n_best=16)
    ref, _, rc = ctx.run(truth.astype(np.float32))
    plain, _, _ = ctx.run(np.eye(4, dtype=np.float32), check=False)
    ang, dist = pose_error(pose, ref)
    print("trial %d: |align - run(truth)| = %.3g rad, %.3g m; RANSAC best vs truth %s; run(truth) vs truth %s; plain icp_run from identity ends %s from run(truth)"
          % (trial, ang, dist, "%.3g rad %.3g m" % pose_error(binding_pose(records[0]), truth), "%.3g rad %.3g m" % pose_error(ref, truth), "%.3g rad %.3g m" % pose_error(plain, ref)))
    assert rc == 0 and len(results) == 16 and results[best]["status"] == 0
    assert E2E_MEASURED_RAD <= 0.001 and E2E_MEASURED_M <= 0.0001          # 10 x must not exceed 0.01 rad and 1 mm
    assert ang <= 10 * E2E_MEASURED_RAD and dist <= 10 * E2E_MEASURED_M, (ang, dist)


def binding_pose(rec):
    return np.asarray(rec["pose"], np.float32).reshape(4, 4).T


def test_eth_align_with_a_global_start(gpu_ctx_factory, bunny):
    """eth.align(initial="global"): the run starts from RANSAC's best pose instead of the identity and ends where the run from the true pose ends."""
    from icp_amd import eth
    p, n, truth = moved_source(bunny, 1)
    ctx = gpu_ctx_factory()
    configure(ctx)
    pair = dict(src_pts=p, src_nrm=n, tgt_pts=bunny["tgt_pts"], tgt_nrm=bunny["tgt_nrm"])
    pose, recs, rc = eth.align(ctx, pair, initial="global", k=20, inlier_distance=0.005)
    ref, _, _ = ctx.run(truth.astype(np.float32))
    ang, dist = pose_error(pose, ref)
    print("eth.align(initial='global'): %.3g rad, %.3g m from run(truth)" % (ang, dist))
    assert rc == 0 and len(recs) == 20
    assert ang <= 10 * E2E_MEASURED_RAD and dist <= 10 * E2E_MEASURED_M, (ang, dist)
    with pytest.raises(ValueError):
        eth.align(ctx, pair, initial="nowhere")
    with pytest.raises(TypeError):
        eth.align(ctx, pair, k=20)


def test_refusals_and_statuses(gpu_ctx_factory, bunny):
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    configure(ctx)

    def code(fn, *a, **kw):
        with pytest.raises(binding.IcpError) as e:
            fn(*a, **kw)
        return e.value.code
    assert code(ctx.compute_features, "target") == 3 and code(ctx.features, "source") == 4           # no clouds yet
    ctx.set_target(bunny["tgt_pts"], bunny["tgt_nrm"]); ctx.set_source(bunny["src_pts"])               # a source without normals
    assert code(ctx.compute_features, "source") == 1 and code(ctx.compute_features, "both") == 1
    assert code(ctx.match_features) == 1 and code(ctx.register_global) == 1
    ctx.compute_features("target")
    ctx.set_source(bunny["src_pts"], bunny["src_nrm"])
    before = ctx.global_options()
    for bad in (dict(k=7), dict(k=0), dict(feature_stride=0), dict(mutual=2), dict(n_hypotheses=0), dict(n_hypotheses=65537), dict(n_best=0), dict(n_best=257),
                dict(edge_similarity=1.5), dict(inlier_distance=0.0), dict(inlier_distance=float("nan"))):
        assert code(ctx.set_global_options, **bad) == 1, bad
    after = ctx.global_options()
    assert (before.k, before.n_hypotheses, before.n_best) == (after.k, after.n_hypotheses, after.n_best)
    assert ctx.lib.icp_compute_features(ctx.h, 3) == 1 and ctx.lib.icp_get_features(ctx.h, 2, None, 0, None) == 1
    # every hypothesis invalid: edge_similarity = 1 on the pairs of two different scans (no two edges have equal fp64 lengths)
    ctx.set_global_options(k=10, edge_similarity=1.0, n_hypotheses=512)
    poses, recs, rc = ctx.register_global(check=False)
    hyp = ctx.global_hypotheses()
    assert rc == binding.ERR_NO_CORRESPONDENCES and poses == [] and len(hyp) == 512
    assert np.isin(hyp["status"], (gr.REPEATED, gr.EDGES)).all() and (hyp["status"] == gr.EDGES).sum() > 400
    assert "no valid hypothesis" in ctx.lib.icp_last_error(ctx.h).decode()
    # and the context still works
    ctx.set_global_options(k=10, n_hypotheses=512)
    poses, recs, rc = ctx.register_global()
    assert rc == 0 and len(poses) == 16


def test_cache_follows_the_clouds_and_the_options(gpu_ctx_factory, bunny):
    ctx = gpu_ctx_factory()
    load(ctx, bunny)
    ctx.set_global_options(k=10)
    Fa = ctx.features("source"); Ta = ctx.features("target")
    assert np.array_equal(bits(Fa), bits(ctx.features("source")))               # served from the cache
    sub = slice(0, 700)
    ctx.set_source(bunny["src_pts"][sub][::-1].copy(), bunny["src_nrm"][sub][::-1].copy())
    Fb = ctx.features("source")
    fresh = gpu_ctx_factory()
    configure(fresh)
    fresh.set_target(bunny["tgt_pts"], bunny["tgt_nrm"]); fresh.set_source(bunny["src_pts"][sub][::-1].copy(), bunny["src_nrm"][sub][::-1].copy())
    fresh.set_global_options(k=10)
    assert Fb.shape == (700, 33) and np.array_equal(bits(Fb), bits(fresh.features("source")))
    assert np.array_equal(bits(Ta), bits(ctx.features("target")))               # the target's stay
    ctx.set_target(bunny["tgt_pts"][:900], bunny["tgt_nrm"][:900])
    assert ctx.features("target").shape == (900, 33)
    ctx.set_global_options(k=5, feature_stride=2)                              # new options: both recomputed
    assert ctx.features("source").shape == (350, 33) and ctx.feature_neighbours("target")[0].shape == (900, 5)
    fresh.set_global_options(k=5, feature_stride=2)
    assert np.array_equal(bits(ctx.features("source")), bits(fresh.features("source")))
