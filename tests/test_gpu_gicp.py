"""Generalized-ICP (params.metric = ICP_METRIC_GICP) on the device against the fp64 restatement tests/gicp_restatement.py: the GICP
normals on every point, teacher-forced iterations on the device's own records, free-running runs iteration by iteration, convergence to
a known pose, the batch and tracking entry points, the refusals, and metrics 0-2 untouched by a GICP run on the same context."""
import ctypes
import functools
import numpy as np
import pytest

import gicp_restatement as G
import support as S
from conftest import pose_error
from support import load

pytestmark = pytest.mark.gpu
f32 = np.float32
EPS = S.GICP_EPS


configure = functools.partial(S.configure, metric=3)          # this file's default metric: GICP
check_normals = S.check_gicp_normals                          # every finite point, none skipped


@pytest.fixture(scope="module")
def depth_pair():
    from icp_amd import synth
    return synth.compact_rgbd_pair()


@pytest.fixture(scope="module")
def eth_pair():
    from icp_amd import synth
    return synth.eth_like_pair(0)


@pytest.mark.parametrize("k", [5, 10, 20])
def test_normals_every_point(gpu_ctx_factory, bunny, depth_pair, eth_pair, k):
    ctx = gpu_ctx_factory()
    ctx.set_gicp_options(EPS, k)
    for label, pts, nrm in (("bunny", bunny["tgt_pts"], bunny["tgt_nrm"]), ("depth/8", depth_pair["tgt_pts"], depth_pair["tgt_nrm"]),
                            ("eth 50k", eth_pair["tgt_pts"][:50000], eth_pair["tgt_nrm"][:50000])):
        ref = G.normals(pts, k, cov=True)
        n_finite = int(np.isfinite(pts).all(1).sum())
        for knn_backend in (1, 0):                        # the target's own tree / a scratch tree
            configure(ctx, knn_backend=knn_backend)
            ctx.set_target(pts, nrm)
            st = check_normals(ctx.gicp_normals("target"), pts, k, label + " target", ref)
            assert st["gapped"] > 0 and st["gapped"] + st["ungapped"] == n_finite
        ctx.set_source(pts, nrm)
        st = check_normals(ctx.gicp_normals("source"), pts, k, label + " source", ref)
        assert st["gapped"] > 0 and st["gapped"] + st["ungapped"] == n_finite
        print("gicp normals %s k=%d: %s" % (label, k, st))
    # a replaced cloud drops the cache; k = 0 gives the cloud's own normals
    ctx.set_target(bunny["src_pts"], bunny["src_nrm"])
    check_normals(ctx.gicp_normals("target"), bunny["src_pts"], k, "replaced target")
    ctx.set_gicp_options(EPS, 0)
    assert np.array_equal(ctx.gicp_normals("target").view(np.uint32), np.ascontiguousarray(bunny["src_nrm"], f32).view(np.uint32))


def test_normals_degenerate_clouds(gpu_ctx_factory):
    ctx = gpu_ctx_factory()
    configure(ctx)
    ctx.set_gicp_options(EPS, 5)
    pts = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 1, 0]], f32)
    ctx.set_target(pts, np.ones_like(pts))
    check_normals(ctx.gicp_normals("target"), pts, 5, "4 points")
    two = np.array([[0, 0, 0], [1, 0, 0], [np.inf, 0, 0]], f32)
    ctx.set_target(two, np.ones_like(two))
    assert np.isnan(ctx.gicp_normals("target")).all()
    same = np.zeros((6, 3), f32)                              # coincident: zero covariance -> Jacobi's first axis
    ctx.set_target(same, np.ones_like(same))
    assert np.array_equal(ctx.gicp_normals("target"), np.tile(f32([1, 0, 0]), (6, 1)))


def teacher_forced(ctx, d, pose, k):
    """icp_correspond at `pose` against the restatement on the device's own records; then icp_iterate's pose against the restatement's step."""
    recs, sums, nv = ctx.correspond(pose)
    p = ctx.transform_points(d["src_pts"], pose)
    tg, sg = ctx.gicp_normals("target"), ctx.gicp_normals("source")
    b = ctx.transform_normals(sg, pose)
    idx = recs["idx"]; j = np.maximum(idx, 0)
    q = np.asarray(d["tgt_pts"], f32)[j]
    valid = (idx >= 0) & np.isfinite(p).all(1) & np.isfinite(q).all(1)
    s_ref, sa = G.sums(p, q, tg[j], b, recs["weight"], EPS, valid)
    assert nv == int(s_ref[0]) and sums[0] == s_ref[0] and nv > 0
    err = np.abs(sums[1:34] - s_ref[1:34]) / (sa[1:34] + 1e-300)
    assert err.max() <= 1e-9, (int(np.argmax(err)) + 1, sums[1:34], s_ref[1:34])
    pose_dev, st = ctx.iterate(pose)
    pose_ref = G.compose(G.solve(s_ref), pose)
    assert st["n_valid"] == nv and st["status"] == 0
    assert np.abs(pose_dev - pose_ref).max() <= 1e-5, (pose_dev, pose_ref)
    return pose_dev


CASES = [  # (covariance_k, weighting, rejection, color_icp, knn_backend)
    (20, 0, 1, 0, 1), (0, 0, 1, 0, 1), (10, 1, 0, 0, 1), (20, 2, 1, 0, 0), (5, 3, 1, 1, 1), (20, 0, 0, 1, 0), (0, 3, 0, 0, 0), (20, 1, 1, 1, 1)]


@pytest.mark.parametrize("k,weighting,rejection,color_icp,knn_backend", CASES)
def test_teacher_forced_iteration(gpu_ctx_factory, bunny, depth_pair, k, weighting, rejection, color_icp, knn_backend):
    from icp_amd import synth
    ctx = gpu_ctx_factory()
    configure(ctx, weighting=weighting, rejection=rejection, color_icp=color_icp, knn_backend=knn_backend)
    ctx.set_gicp_options(EPS, k)
    load(ctx, bunny)
    for pose in (np.eye(4, dtype=f32), synth.make_pose((0.01, -0.015, 0.02), (0.002, -0.003, 0.001)).astype(f32)):
        teacher_forced(ctx, bunny, pose, k)
    configure(ctx, weighting=weighting, rejection=rejection, color_icp=color_icp, knn_backend=knn_backend, max_distance=0.01)
    load(ctx, depth_pair)
    teacher_forced(ctx, depth_pair, np.eye(4, dtype=f32), k)


def free_running(ctx, d, n_iter):
    pose0 = np.eye(4, dtype=f32)
    pose, recs, rc = ctx.run(pose0)
    assert rc == 0 and len(recs) == n_iter
    prev = pose0
    for i, r in enumerate(recs):
        recs_i, sums, nv = ctx.correspond(prev)
        p = ctx.transform_points(d["src_pts"], prev)
        tg, sg = ctx.gicp_normals("target"), ctx.gicp_normals("source")
        b = ctx.transform_normals(sg, prev)
        idx = recs_i["idx"]; j = np.maximum(idx, 0)
        q = np.asarray(d["tgt_pts"], f32)[j]
        valid = (idx >= 0) & np.isfinite(p).all(1) & np.isfinite(q).all(1)
        s_ref, _ = G.sums(p, q, tg[j], b, recs_i["weight"], EPS, valid)
        assert r["n_valid"] == int(s_ref[0]), i
        ref = G.compose(G.solve(s_ref), prev)
        assert np.abs(r["pose"] - ref).max() <= 1e-5, (i, r["pose"], ref)
        prev = r["pose"]
    pose2, recs2, _ = ctx.run(pose0)
    assert np.array_equal(pose.view(np.uint32), pose2.view(np.uint32))
    assert all(np.array_equal(a["pose"].view(np.uint32), b["pose"].view(np.uint32)) and a["n_valid"] == b["n_valid"] for a, b in zip(recs, recs2))
    return pose, recs


def test_free_running_against_restatement(gpu_ctx_factory, bunny, depth_pair, eth_pair):
    ctx = gpu_ctx_factory()
    for d, md, n_iter in ((bunny, 0.0003, 8), (depth_pair, 0.01, 8), (eth_pair, 10.0, 5)):
        configure(ctx, n_iterations=n_iter, max_distance=md)
        load(ctx, d, colors=False)
        free_running(ctx, d, n_iter)


@pytest.mark.parametrize("multires,selection", [(1, 0), (0, 1), (1, 1)])
def test_multires_and_sampling_deterministic(gpu_ctx_factory, bunny, depth_pair, multires, selection):
    """Multires levels and random samples: two runs are bit-identical, every iteration has valid pairs, and the final pose is within
    0.02 rad / 0.01 of the full-resolution run's.  Nothing here shows WHICH points' GICP normals a level read (a multires run ends at full
    resolution): that is tests/test_gpu_query_sets.py, iteration by iteration against the restatement."""
    ctx = gpu_ctx_factory()
    for d, md in ((bunny, 0.0003), (depth_pair, 0.01)):
        configure(ctx, n_iterations=10, multires=multires, selection=selection, proba=0.5, max_distance=md)
        load(ctx, d)
        eye = np.eye(4, dtype=f32)
        a, ra, rc = ctx.run(eye)
        b, rb, _ = ctx.run(eye)
        assert rc == 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert [r["n_valid"] for r in ra] == [r["n_valid"] for r in rb] and all(r["n_valid"] > 0 for r in ra)
        configure(ctx, n_iterations=10, max_distance=md)
        full, _, _ = ctx.run(eye)
        ang, tr = pose_error(a, full)
        assert ang < 0.02 and tr < 0.01, (ang, tr)


def test_convergence_to_known_pose(gpu_ctx_factory, bunny):
    from icp_amd import synth
    T = synth.make_pose(np.deg2rad((1.2, -1.0, 1.2)), (0.003, -0.003, 0.0025))
    ang0 = pose_error(T, np.eye(4))[0]
    assert abs(ang0 - np.deg2rad(2.0)) < np.deg2rad(0.3) and abs(np.linalg.norm(T[:3, 3]) - 0.005) < 1e-3
    tp, tn = np.ascontiguousarray(bunny["tgt_pts"], f32), np.ascontiguousarray(bunny["tgt_nrm"], f32)
    sp, sn = synth.apply_pose(T, tp, tn)
    ctx = gpu_ctx_factory()
    for k in (20, 0):
        configure(ctx, n_iterations=30)
        ctx.set_gicp_options(EPS, k)
        ctx.set_target(tp, tn); ctx.set_source(sp, sn)
        pose, recs, rc = ctx.run(np.eye(4, dtype=f32))
        ang, tr = pose_error(pose, np.linalg.inv(T))
        assert rc == 0 and ang < 1e-4 and tr < 1e-5, (k, ang, tr)


def test_batch_and_align_equal_per_pair_runs(gpu_ctx_factory):
    from icp_amd import binding, eth, synth
    scans = [tuple(np.ascontiguousarray(a, f32) for a in synth.laser_scan(synth.scan_pose(k), 40 + k, n_tilt=43, n_beam=135)[:2]) for k in range(3)]
    pairs = [dict(src_pts=scans[k + 1][0], src_nrm=scans[k + 1][1], tgt_pts=scans[k][0], tgt_nrm=scans[k][1]) for k in range(2)]
    pairs.append(dict(src_pts=scans[0][0], src_nrm=scans[0][1], tgt_pts=scans[2][0], tgt_nrm=scans[2][1]))
    ctxs = [gpu_ctx_factory(), gpu_ctx_factory()]
    for c in ctxs:
        configure(c, n_iterations=12, max_distance=0.05)
        c.set_gicp_options(EPS, 10)
    poses, status, rc = binding.batch_run(ctxs, pairs)
    ref = gpu_ctx_factory()
    configure(ref, n_iterations=12, max_distance=0.05)
    ref.set_gicp_options(EPS, 10)
    for i, d in enumerate(pairs):
        pose, recs, st = eth.align(ref, d, check=False)
        assert st == status[i]
        assert np.array_equal(binding.pose_to_c(pose).view(np.uint32), poses[i].view(np.uint32)), i


def test_track_depth_frames_equals_frame_by_frame(gpu_ctx_factory):
    from icp_amd import binding, synth
    W, H = 80, 60
    K = np.array([[525.0 / 8, 0, 319.5 / 8], [0, 525.0 / 8, 239.5 / 8], [0, 0, 1]], f32)
    depth = []
    for k in range(3):
        pts, _, _ = synth.depth_frame(synth.camera_pose(k), K.astype(np.float64), W, H, 0x7A11 + k)
        depth.append(pts[:, 2].reshape(H, W).copy())
    depth = np.stack(depth)
    cam = binding.depth_camera(K, W, H)
    to, so = binding.depth_options(False, 1), binding.depth_options(False, 2)
    a = gpu_ctx_factory()
    configure(a, n_iterations=15, max_distance=0.01)
    a.set_gicp_options(EPS, 10)
    _, recs, rc = a.track_depth_frames(depth, None, cam, to, so)
    b = gpu_ctx_factory()
    configure(b, n_iterations=15, max_distance=0.01)
    b.set_gicp_options(EPS, 10)
    b.set_target_depth(depth[0], None, cam, to)
    pose = np.eye(4, dtype=f32)
    for k in range(1, 3):
        b.set_source_depth(depth[k], None, cam, so)
        pose, _, st = b.run(pose, check=False)
        assert recs[k - 1]["status"] == st
        assert np.array_equal(recs[k - 1]["pose"].view(np.uint32), pose.view(np.uint32)), k


def test_refusals(gpu_ctx_factory, bunny):
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    lib, h = ctx.lib, ctx.h
    for k, e in ((7, EPS), (-1, EPS), (20, 0.0), (20, 1.5), (20, float("nan"))):
        with pytest.raises(binding.IcpError) as ei:
            ctx.set_gicp_options(e, k)
        assert ei.value.code == 1
    ctx.set_gicp_options(EPS, 20)
    configure(ctx)
    load(ctx, bunny)
    eye = np.eye(4, dtype=f32)
    # projective matching (an organised-size camera so that only the metric is in the way)
    p = ctx.params
    p.matching, p.width, p.height, p.fx, p.fy, p.cx, p.cy = 1, len(bunny["tgt_pts"]), 1, 500.0, 500.0, 0.0, 0.0
    ctx.push_params()
    assert ctx.run(eye, check=False)[2] == 1 and "projective" in lib.icp_last_error(h).decode()
    configure(ctx)
    ctx.set_optimizer(True)
    assert ctx.run(eye, check=False)[2] == 1 and "non-linear" in lib.icp_last_error(h).decode()
    ctx.set_optimizer(None)
    with pytest.raises(binding.IcpError) as ei:
        ctx.run_multistart([eye])
    assert ei.value.code == 1
    with pytest.raises(binding.IcpError) as ei:
        ctx.match_seeded([eye])
    assert ei.value.code == 1
    ctx.set_gicp_options(EPS, 0)                          # covariance_k = 0 without normals
    ctx.set_target(bunny["tgt_pts"])
    with pytest.raises(binding.IcpError) as ei:
        ctx.gicp_normals("target")
    assert ei.value.code == 1
    assert ctx.run(eye, check=False)[2] == 1
    assert lib.icp_get_gicp_normals(h, 2, None, 0, None) == 1
    # the loop still runs after the refusals
    ctx.set_gicp_options(EPS, 20)
    load(ctx, bunny)
    assert ctx.run(eye)[2] == 0


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_other_metrics_untouched(gpu_ctx_factory, bunny, metric):
    a = gpu_ctx_factory()
    configure(a, n_iterations=6)
    load(a, bunny)
    a.run(np.eye(4, dtype=f32))
    configure(a, metric=metric, n_iterations=6)
    pa, ra, rca = a.run(np.eye(4, dtype=f32), check=False)
    b = gpu_ctx_factory()
    configure(b, metric=metric, n_iterations=6)
    load(b, bunny)
    pb, rb, rcb = b.run(np.eye(4, dtype=f32), check=False)
    assert rca == rcb and np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert all(np.array_equal(x["pose"].view(np.uint32), y["pose"].view(np.uint32)) and x["n_valid"] == y["n_valid"] for x, y in zip(ra, rb))
