"""Multi-start ICP (icp_run_multistart, dev_multi.hpp): K initial poses of one pair in one set of launches per iteration.  Every start must
follow icp_run from its pose bit for bit (records and final pose), the score must be the 3-D match of the full-resolution source at the
final pose, and the best start must follow the tie rules."""
import ctypes as C
import numpy as np
import pytest
from conftest import pose_error

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


def assert_matches_icp_run(c, starts, max_stats=512):
    """Every start of ONE multistart call against icp_run from that start on the same context: records and pose, bit for bit."""
    res, stats, best = c.run_multistart(starts, max_stats=max_stats)
    assert len(res) == len(starts)
    for k, s in enumerate(starts):
        pose, recs, rc = c.run(s, max_stats=max_stats, check=False)
        assert res[k]["status"] == rc, k
        assert np.array_equal(res[k]["pose"], pose), k
        assert len(stats[k]) == len(recs), k
        for i, (a, b) in enumerate(zip(stats[k], recs)):
            assert (a["n_src"], a["n_valid"], a["status"]) == (b["n_src"], b["n_valid"], b["status"]), (k, i)
            assert np.array_equal(a["pose"], b["pose"]), (k, i)
            assert a["rmse"] == -1.0 and a["benchmark_error"] == -1.0
    return res, stats, best


def expected_best(res):
    best = 0
    for k, r in enumerate(res):
        b = res[best]
        if r["n_inliers"] > b["n_inliers"] or (r["n_inliers"] == b["n_inliers"] and r["inlier_rmse"] < b["inlier_rmse"]):
            best = k
    return best


def check_score(c_plain, res, n_src_finite):
    """n_inliers / fitness / inlier_rmse against icp_match at the final pose on a context without colour ICP."""
    for k, r in enumerate(res):
        m, d2 = c_plain.match(r["pose"])
        ok = m["idx"] >= 0
        n = int(ok.sum())
        assert r["n_inliers"] == n, k
        assert r["fitness"] == pytest.approx(n / n_src_finite, rel=1e-6), k
        if n:
            ref = np.sqrt(d2[ok].astype(np.float64).sum() / n)
            assert r["inlier_rmse"] == pytest.approx(ref, rel=1e-6), k
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
    check_score(c, res, int(np.isfinite(bunny["src_pts"]).all(axis=1).sum()))


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
    check_score(c, res, len(bunny["src_pts"]))


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


def test_color_icp_on_a_depth_frame(gpu_ctx_factory):
    from icp_amd.multistart import start_poses
    clouds, _ = depth_cloud()
    c = make(gpu_ctx_factory, clouds, metric=1, color_icp=1, weighting=3, max_distance=0.1, n_iterations=15)
    starts = start_poses(np.eye(4), yaw_deg=[0, 3, -3, 6], axis=(0, 1, 0), points=clouds[0])
    res, _, best = assert_matches_icp_run(c, starts)
    assert best == expected_best(res)
    plain = make(gpu_ctx_factory, clouds, metric=1, max_distance=0.1)
    check_score(plain, res, len(clouds[0]))


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
