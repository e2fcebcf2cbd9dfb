"""Multi-start ICP (icp_run_multistart, dev_multi.hpp): K initial poses of one pair in one set of launches per iteration.  Every start must
follow icp_run from its pose bit for bit (records and final pose), the score must be the 3-D match of the full-resolution source at the
final pose, and the best start must follow the tie rules."""
import ctypes as C
import numpy as np
import pytest
from conftest import pose_error
from support import assert_matches_icp_run, expected_best

pytestmark = pytest.mark.gpu
LBVH = 1


def make(factory, clouds, **params):
    c = factory()
    c.params.knn_backend = LBVH
    for k, v in params.items():
        setattr(c.params, k, v)
    c.push_params()
    sp, sn, sc, tp, tn, tc = clouds
    c.set_target(tp, tn, tc)
    c.set_source(sp, sn, sc)
    return c


def bunny_clouds(bunny):
    return tuple(bunny[k] for k in ("src_pts", "src_nrm", "src_rgba", "tgt_pts", "tgt_nrm", "tgt_rgba"))


def bunny_starts(bunny, k=5):
    from icp_amd.multistart import start_poses
    return start_poses(np.eye(4), yaw_deg=[0.0, 4.0, -4.0, 8.0, -8.0][:k], axis=(0, 1, 0), points=bunny["src_pts"])


def ulp_distance(a, b):
    """fp32 units in the last place between two positive floats"""
    return abs(int(np.float32(a).view(np.uint32)) - int(np.float32(b).view(np.uint32)))


RMSE_ULPS = []          # the inlier_rmse ulp distances seen by check_score (reported, not asserted beyond the bound of 1)


def check_score(orc, clouds, max_distance, res, c_plain=None):
    """n_inliers / fitness / inlier_rmse of every start against the CPU oracle's 3-D match of the source at the final pose: the count equal,
    fitness bit-equal (two exact integers divided in fp64, rounded once), inlier_rmse within 1 ulp (both fp64 sums are exact to ~1e-16
    relative: the one fp32 rounding can differ only at a rounding boundary).  c_plain: also against icp_match on that context (one
    without colour ICP), as before."""
    src, tgt = clouds[0], clouds[3]
    n_finite = int(np.isfinite(src).all(axis=1).sum())
    for k, r in enumerate(res):
        m, d2 = orc.knn3(orc.transform_points(src, r["pose"]), tgt, max_distance)
        ok = m["idx"] >= 0
        n = int(ok.sum())
        assert r["n_inliers"] == n, k
        want = np.float32(n / n_finite) if n_finite else np.float32(0.0)
        assert np.float32(r["fitness"]).view(np.uint32) == want.view(np.uint32), (k, r["fitness"], want)
        if n:
            ref = np.float32(np.sqrt(d2[ok].astype(np.float64).sum() / n))
            RMSE_ULPS.append(ulp_distance(r["inlier_rmse"], ref))
            assert RMSE_ULPS[-1] <= 1, (k, r["inlier_rmse"], ref)
        else:
            assert r["inlier_rmse"] == -1.0, k
        if c_plain is not None:
            m, d2 = c_plain.match(r["pose"])
            ok = m["idx"] >= 0
            n = int(ok.sum())
            assert r["n_inliers"] == n, k
            assert r["fitness"] == pytest.approx(n / n_finite, rel=1e-6), k
            if n:
                assert r["inlier_rmse"] == pytest.approx(np.sqrt(d2[ok].astype(np.float64).sum() / n), rel=1e-6), k
            else:
                assert r["inlier_rmse"] == -1.0


BUNNY_CASES = [(m, w, r) for m in (0, 1, 2) for w in (0, 2) for r in (0, 1)]


@pytest.mark.parametrize("metric,weighting,rejection", BUNNY_CASES)
def test_bunny_starts_follow_icp_run_and_the_oracle(gpu_ctx_factory, bunny, orc, metric, weighting, rejection):
    clouds = bunny_clouds(bunny)
    c = make(gpu_ctx_factory, clouds, metric=metric, weighting=weighting, rejection=rejection, max_distance=0.0003, n_iterations=20)
    starts = bunny_starts(bunny)
    res, _, best = assert_matches_icp_run(c, starts)
    assert best == expected_best(res)
    prm = orc.make_params(metric=metric, weighting=weighting, rejection=rejection, n_iterations=20, max_distance=0.0003, solver_mode=1)
    for k, s in enumerate(starts):
        po, _ = orc.estimate_pose(prm, *clouds, s)
        assert float(np.abs(res[k]["pose"] - po).max()) < 1e-5, k
    check_score(orc, clouds, 0.0003, res, c)


@pytest.mark.parametrize("kw", [dict(multires=1, max_distance=0.001), dict(selection=1, selection_proba=0.5, selection_seed=1234, max_distance=0.0003)],
                         ids=["multires", "random_sampling"])
def test_bunny_multires_and_random_sampling(gpu_ctx_factory, bunny, orc, kw):
    clouds = bunny_clouds(bunny)
    c = make(gpu_ctx_factory, clouds, metric=1, n_iterations=20, **kw)
    starts = bunny_starts(bunny)
    res, stats, _ = assert_matches_icp_run(c, starts)
    prm = orc.make_params(metric=1, n_iterations=20, solver_mode=1, **kw)
    for k, s in enumerate(starts):
        po, _ = orc.estimate_pose(prm, *clouds, s)
        assert float(np.abs(res[k]["pose"] - po).max()) < 1e-5, k
    check_score(orc, clouds, kw["max_distance"], res, c)


def test_single_start(gpu_ctx_factory, bunny):
    c = make(gpu_ctx_factory, bunny_clouds(bunny), metric=1, max_distance=0.0003, n_iterations=20)
    res, _, best = assert_matches_icp_run(c, bunny_starts(bunny, 1))
    assert best == 0 and res[0]["n_inliers"] > 0


def depth_cloud():
    from icp_amd import synth
    r = synth.rgbd_pair(0)
    sp, sn, sc = synth.compact_valid(r["src_pts"][::8], r["src_nrm"][::8], r["src_rgba"][::8])
    tp, tn, tc = synth.compact_valid(r["tgt_pts"][::8], r["tgt_nrm"][::8], r["tgt_rgba"][::8])
    return (sp, sn, sc, tp, tn, tc), r["gt"]


def test_color_icp_on_a_depth_frame(gpu_ctx_factory, orc):
    from icp_amd.multistart import start_poses
    clouds, _ = depth_cloud()
    c = make(gpu_ctx_factory, clouds, metric=1, color_icp=1, weighting=3, max_distance=0.1, n_iterations=15)
    starts = start_poses(np.eye(4), yaw_deg=[0, 3, -3, 6], axis=(0, 1, 0), points=clouds[0])
    res, _, best = assert_matches_icp_run(c, starts)
    assert best == expected_best(res)
    plain = make(gpu_ctx_factory, clouds, metric=1, max_distance=0.1)
    check_score(orc, clouds, 0.1, res, plain)


def test_fullsize_eth_pair(gpu_ctx_factory):
    from icp_amd import synth
    from icp_amd.multistart import start_poses
    p = synth.eth_like_pair(0)
    clouds = tuple(p[k] for k in ("src_pts", "src_nrm", "src_rgba", "tgt_pts", "tgt_nrm", "tgt_rgba"))
    assert len(clouds[0]) == 370488
    c = make(gpu_ctx_factory, clouds, metric=1, max_distance=10.0, n_iterations=10)
    starts = start_poses(np.eye(4), yaw_deg=[0, 2, -2, 5], points=clouds[0])
    res, _, best = assert_matches_icp_run(c, starts)
    assert best == expected_best(res)


def test_recovery_from_a_wrong_minimum(gpu_ctx_factory, bunny, orc):
    """The target against itself turned by 130 degrees about its centroid: from the identity ICP settles upside down; a yaw grid of
    twelve starts contains one that converges, and the best start is it."""
    from icp_amd.multistart import rotation, start_poses
    tp, tn, tc = bunny["tgt_pts"], bunny["tgt_nrm"], bunny["tgt_rgba"]
    cen = tp.mean(axis=0).astype(np.float64)
    R = rotation((0, 1, 0), 130.0)
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = cen - R @ cen
    sp = (tp @ R.T + T[:3, 3]).astype(np.float32); sn = (tn @ R.T).astype(np.float32)
    gt = np.linalg.inv(T)
    clouds = (sp, sn, tc, tp, tn, tc)
    prm = orc.make_params(metric=1, n_iterations=20, max_distance=0.0003, solver_mode=1)
    p0, _ = orc.estimate_pose(prm, *clouds, np.eye(4, dtype=np.float32))
    a0, t0 = pose_error(p0, gt)
    assert np.degrees(a0) > 10.0                                         # the case keeps its meaning: identity fails
    c = make(gpu_ctx_factory, clouds, metric=1, max_distance=0.0003, n_iterations=20)
    starts = start_poses(np.eye(4), yaw_deg=np.arange(0, 360, 30), axis=(0, 1, 0), points=sp)
    res, _, best = c.run_multistart(starts)
    assert best != 0 and best == expected_best(res)
    ab, tb = pose_error(res[best]["pose"], gt)
    assert np.degrees(ab) < 1.0 and tb < 1e-3
    a, t = pose_error(res[0]["pose"], gt)
    assert not (np.degrees(a) < 1.0 and t < 1e-3)


def test_isolation_determinism_and_icp_run_untouched(gpu_ctx_factory, bunny):
    c = make(gpu_ctx_factory, bunny_clouds(bunny), metric=1, max_distance=0.0003, n_iterations=20)
    a, b = bunny_starts(bunny, 3)[1:]
    far = np.eye(4, dtype=np.float32); far[:3, 3] = (100.0, 0.0, 0.0)       # nothing within max_distance: every iteration empty
    before, recs_before, _ = c.run(a)
    r2, s2, _ = c.run_multistart([a, b])
    r3, s3, best3 = c.run_multistart([a, far, b])
    assert r3[1]["status"] == 8 and np.array_equal(r3[1]["pose"], far) and r3[1]["n_inliers"] == 0 and r3[1]["inlier_rmse"] == -1.0
    assert all(s["status"] == 8 and s["n_valid"] == 0 for s in s3[1])
    pf, _, rcf = c.run(far, check=False)
    assert rcf == 8 and np.array_equal(pf, far)
    for x, y, sx, sy in ((r2[0], r3[0], s2[0], s3[0]), (r2[1], r3[2], s2[1], s3[2])):
        assert np.array_equal(x["pose"], y["pose"]) and (x["n_inliers"], x["fitness"], x["inlier_rmse"]) == (y["n_inliers"], y["fitness"], y["inlier_rmse"])
        assert all(np.array_equal(u["pose"], v["pose"]) and u["n_valid"] == v["n_valid"] for u, v in zip(sx, sy))
    assert best3 != 1
    r4, s4, best4 = c.run_multistart([a, far, b])                        # a second call: the same, bit for bit
    assert best4 == best3
    for x, y in zip(r3, r4):
        assert np.array_equal(x["pose"], y["pose"]) and (x["n_inliers"], x["inlier_rmse"], x["status"]) == (y["n_inliers"], y["inlier_rmse"], y["status"])
    after, recs_after, _ = c.run(a)
    assert np.array_equal(before, after)
    assert all(np.array_equal(u["pose"], v["pose"]) for u, v in zip(recs_before, recs_after))


# ---- the score on more than one pass of its 64 x 256 grid, with non-finite source points ----
SCORE_MAX_DISTANCE = 0.001          # (squared metres) after 3 iterations about three quarters of the 40 800 points are inliers (asserted below)


@pytest.fixture(scope="module")
def scan_pair():
    from icp_amd import synth
    p = synth.eth_like_pair(0, n_tilt=120, n_beam=340)
    clouds = tuple(p[k] for k in ("src_pts", "src_nrm", "src_rgba", "tgt_pts", "tgt_nrm", "tgt_rgba"))
    assert len(clouds[0]) == len(clouds[3]) == 40800
    return clouds


def with_holes(pts, seed, every=False):
    """about 2 % of the rows (at least three; every: all of them) made non-finite: NaN, +inf in one coordinate, -inf in one coordinate"""
    rng = np.random.default_rng(seed)
    p = pts.copy()
    rows = np.arange(len(p)) if every else rng.choice(len(p), max(3, len(p) // 50), replace=False)
    for j, i in enumerate(rows):
        if j % 3 == 0:
            p[i] = np.nan
        else:
            p[i, rng.integers(0, 3)] = np.inf if j % 3 == 1 else -np.inf
    return p, len(rows)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 16383, 16384, 16385, 40800])
def test_score_against_the_oracle_around_the_score_grid(gpu_ctx_factory, orc, scan_pair, n):
    """k_score_multi takes 64 x 256 = 16 384 positions per pass: one block, a ragged block, one pass exactly, a second pass begun, and two
    and a half passes; the finite source points counted apart from n."""
    from icp_amd.multistart import start_poses
    sp, sn, sc = (a[:n] for a in scan_pair[:3])
    holes = 0
    if n >= 255:
        sp, holes = with_holes(sp, n)
    clouds = (sp, sn, sc) + scan_pair[3:]
    n_finite = int(np.isfinite(sp).all(axis=1).sum())
    assert n_finite == n - holes and (holes >= 3 or n == 1)
    c = make(gpu_ctx_factory, clouds, metric=1, max_distance=SCORE_MAX_DISTANCE, n_iterations=3)
    starts = start_poses(np.eye(4), yaw_deg=[0, 2, -2], points=scan_pair[0])
    res, _, best = assert_matches_icp_run(c, starts, max_stats=3)
    assert best == expected_best(res)
    check_score(orc, clouds, SCORE_MAX_DISTANCE, res, c)
    print("n = %d (%d finite): fitness %s, inlier_rmse ulp distances so far: max %d" % (n, n_finite, [r["fitness"] for r in res], max(RMSE_ULPS, default=0)))
    if n == 40800:
        assert 0.1 < res[0]["fitness"] < 0.9


def test_score_of_a_source_without_a_finite_point(gpu_ctx_factory, orc, scan_pair):
    """icp_run_multistart does not refuse such a source (check_ready asks for points, not finite ones): every start loses its
    correspondences, keeps its pose, and scores 0 inliers -- fitness 0 (0 / 0 finite points), inlier_rmse -1."""
    from icp_amd.multistart import start_poses
    sp, holes = with_holes(scan_pair[0][:300], 300, every=True)
    assert holes == 300 and not np.isfinite(sp).all(axis=1).any()
    clouds = (sp, scan_pair[1][:300], scan_pair[2][:300]) + scan_pair[3:]
    c = make(gpu_ctx_factory, clouds, metric=1, max_distance=SCORE_MAX_DISTANCE, n_iterations=3)
    starts = start_poses(np.eye(4), yaw_deg=[0, 2, -2], points=scan_pair[0])
    res, stats, best = assert_matches_icp_run(c, starts, max_stats=3)
    check_score(orc, clouds, SCORE_MAX_DISTANCE, res)
    assert best == 0
    for r, s, rec in zip(res, starts, stats):
        assert r["status"] == 8 and np.array_equal(r["pose"], s) and r["n_inliers"] == 0 and r["fitness"] == 0.0 and r["inlier_rmse"] == -1.0
        assert len(rec) == 3 and all(x["status"] == 8 and x["n_valid"] == 0 for x in rec)


# ---- as many starts as the contract allows ----
def many_starts(bunny, K):
    """a yaw grid of K starts, start 0 again at index 5 and at index K - 1, and in the middle a start with nothing within max_distance"""
    from icp_amd.multistart import start_poses
    starts = start_poses(np.eye(4), yaw_deg=np.linspace(-12.0, 12.0, K), axis=(0, 1, 0), points=bunny["src_pts"])
    starts[5] = starts[0].copy(); starts[K - 1] = starts[0].copy()
    far = np.eye(4, dtype=np.float32); far[:3, 3] = (100.0, 0.0, 0.0)
    starts[K // 2] = far
    return starts, far


@pytest.mark.parametrize("K,metric", [(63, 1), (64, 1), (65, 1), (256, 1), (256, 2)])
def test_start_counts_around_the_fold_block(gpu_ctx_factory, bunny, orc, K, metric):
    """k_score_fold runs 64 starts per block and every per-start slice is addressed as stride * blockIdx.y: K around 64 and the largest
    allowed, each start against icp_run and against the oracle's score.  (metric 2: four launches per iteration on the (x, K) grid.)"""
    clouds = bunny_clouds(bunny)
    c = make(gpu_ctx_factory, clouds, metric=metric, max_distance=0.0003, n_iterations=8)
    starts, far = many_starts(bunny, K)
    res, stats, best = assert_matches_icp_run(c, starts, max_stats=8)
    check_score(orc, clouds, 0.0003, res)
    print("K = %d, metric %d: best %d, inlier_rmse ulp distances so far: max %d over %d scores" % (K, metric, best, max(RMSE_ULPS, default=0), len(RMSE_ULPS)))
    assert best == expected_best(res) and best not in (5, K - 1, K // 2)
    for twin in (5, K - 1):
        assert np.array_equal(res[twin]["pose"], res[0]["pose"])
        assert (res[twin]["n_inliers"], res[twin]["fitness"], res[twin]["inlier_rmse"], res[twin]["status"]) == (res[0]["n_inliers"], res[0]["fitness"], res[0]["inlier_rmse"], res[0]["status"])
    r = res[K // 2]
    assert r["status"] == 8 and np.array_equal(r["pose"], far) and r["n_inliers"] == 0 and r["inlier_rmse"] == -1.0
    assert all(s["status"] == 8 and s["n_valid"] == 0 for s in stats[K // 2])
    assert res[best]["status"] == 0 and res[best]["n_inliers"] > 0


# ---- switches that never ran under multi-start, on a size that is no multiple of any block ----
@pytest.mark.parametrize("weighting", [1, 3])
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_weightings_and_the_walk_without_verify_and_skip(gpu_ctx_factory, metric, weighting):
    from icp_amd.multistart import start_poses
    full, _ = depth_cloud()
    clouds = tuple(a[:4097] for a in full[:3]) + full[3:]
    assert len(clouds[0]) == 4097
    c = make(gpu_ctx_factory, clouds, metric=metric, weighting=weighting, color_icp=1 if weighting == 3 else 0, max_distance=0.1, n_iterations=8)
    starts = start_poses(np.eye(4), yaw_deg=[0, 3, -3, 6], axis=(0, 1, 0), points=clouds[0])
    out = {}
    for inc in (0, 1):
        c.params.knn_incremental = inc
        c.push_params()
        res, stats, best = assert_matches_icp_run(c, starts, max_stats=8)
        assert best == expected_best(res) and any(r["status"] == 0 and r["n_inliers"] > 0 for r in res)
        out[inc] = (res, stats, best)
    (ra, sa, ba), (rb, sb, bb) = out[0], out[1]
    assert ba == bb
    for x, y, sx, sy in zip(ra, rb, sa, sb):
        assert np.array_equal(x["pose"], y["pose"])
        assert (x["status"], x["n_inliers"], x["fitness"], x["inlier_rmse"]) == (y["status"], y["n_inliers"], y["fitness"], y["inlier_rmse"])
        assert len(sx) == len(sy) == 8
        assert all(np.array_equal(u["pose"], v["pose"]) and (u["n_src"], u["n_valid"], u["status"]) == (v["n_src"], v["n_valid"], v["status"]) for u, v in zip(sx, sy))


# ---- fewer records than iterations ----
def raw_multistart(c, starts, max_stats, with_stats=True):
    """icp_run_multistart through ctypes: (return code, results as tuples, records [K][max_stats] or None, n_iterations_run, best)"""
    from icp_amd import binding
    K = len(starts)
    ps = np.ascontiguousarray(np.stack([binding.pose_to_c(p) for p in starts]), dtype=np.float32)
    res = (binding.IcpStartResult * K)(); n_run = C.c_int32(-1); best = C.c_int32(-1)
    st = (binding.IcpIterStats * max(K * max_stats, 1))() if with_stats else None
    rc = c.lib.icp_run_multistart(c.h, ps.ctypes.data_as(C.c_void_p), C.c_int32(K), res, st, C.c_int32(max_stats), C.byref(n_run), C.byref(best))
    results = [(bytes(np.frombuffer(r, np.uint8, 64)), r.status, r.n_inliers, r.fitness, r.inlier_rmse) for r in res]
    recs = None
    if with_stats:
        recs = [[(st[k * max_stats + i].n_src, st[k * max_stats + i].n_valid, st[k * max_stats + i].status, binding.pose_from_c(st[k * max_stats + i].pose))
                 for i in range(max_stats)] for k in range(K)]
    return rc, results, recs, n_run.value, best.value


def test_fewer_records_than_iterations(gpu_ctx_factory, bunny):
    """max_stats = 5 on a 20-iteration run: five records per start, the first five of icp_run, at a stride of five; n_iterations_run 20;
    the results those of a call with room for every record, and of one without records."""
    from icp_amd import binding
    c = make(gpu_ctx_factory, bunny_clouds(bunny), metric=1, max_distance=0.0003, n_iterations=20)
    starts = bunny_starts(bunny)
    rc20, res20, rec20, n20, best20 = raw_multistart(c, starts, 20)
    rc5, res5, rec5, n5, best5 = raw_multistart(c, starts, 5)
    rc0, res0, _, n0, best0 = raw_multistart(c, starts, 0, with_stats=False)
    assert (rc20, rc5, rc0) == (0, 0, 0) and (n20, n5, n0) == (20, 20, 20) and best20 == best5 == best0
    assert res20 == res5 == res0
    for k, s in enumerate(starts):
        pose, recs, rcs = c.run(s, max_stats=512, check=False)
        assert len(recs) == 20 and res5[k][1] == rcs and res5[k][0] == binding.pose_to_c(pose).tobytes()
        for i in range(5):
            for got in (rec5[k][i], rec20[k][i]):
                assert got[:3] == (recs[i]["n_src"], recs[i]["n_valid"], recs[i]["status"]) and np.array_equal(got[3], recs[i]["pose"]), (k, i)
        for i in range(5, 20):
            assert rec20[k][i][:3] == (recs[i]["n_src"], recs[i]["n_valid"], recs[i]["status"]) and np.array_equal(rec20[k][i][3], recs[i]["pose"]), (k, i)


def call(c, poses, n):
    from icp_amd import binding
    res = (binding.IcpStartResult * 257)(); n_run = C.c_int32(0); best = C.c_int32(0)
    ptr = None if poses is None else poses.ctypes.data_as(C.c_void_p)
    return c.lib.icp_run_multistart(c.h, ptr, C.c_int32(n), res, None, C.c_int32(0), C.byref(n_run), C.byref(best))


def test_invalid_arguments_and_unsupported_configurations(gpu_ctx_factory, bunny):
    clouds = bunny_clouds(bunny)
    poses = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (257, 1))
    c = make(gpu_ctx_factory, clouds, metric=1)
    assert call(c, poses, 1) == 0
    for n in (0, 257):
        assert call(c, poses, n) == 1
    assert call(c, None, 2) == 1
    for field, value in (("matching", 1), ("knn_backend", 0), ("record_rmse", 1)):
        d = make(gpu_ctx_factory, clouds, metric=1, **{field: value})
        assert call(d, poses, 2) == 1 and d.lib.icp_last_error(d.h)
    d = make(gpu_ctx_factory, clouds, metric=1)
    d.set_optimizer(True)
    assert call(d, poses, 2) == 1
    d.set_optimizer(None)
    assert call(d, poses, 2) == 0
    e = gpu_ctx_factory()
    e.params.knn_backend = LBVH; e.push_params()
    assert call(e, poses, 2) == 3                                         # ICP_ERR_NO_TARGET
    e.set_target(clouds[3], clouds[4], clouds[5])
    assert call(e, poses, 2) == 4                                         # ICP_ERR_NO_SOURCE
