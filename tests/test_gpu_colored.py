"""Colored ICP (params.metric = ICP_METRIC_COLORED) on the device against the fp64 restatement tests/colored_restatement.py: the colour
gradients on every point, teacher-forced sums on the device's own records, lambda = 1, free-running runs iteration by iteration, robust
mode, the textured plane that geometry alone cannot align, the batch and tracking entry points, the refusals, and metrics 0-3 untouched
by colored options on the same context."""
import functools
import numpy as np
import pytest

import colored_restatement as CR
import support as S
from conftest import pose_error
from support import load

pytestmark = pytest.mark.gpu
f32 = np.float32
LAM = 0.968


configure = functools.partial(S.configure, metric=4, max_distance=0.01)          # this file's defaults: the colored metric, 1 cm


@pytest.fixture(scope="module")
def depth_pair():
    from icp_amd import synth
    return synth.compact_rgbd_pair()


@pytest.fixture(scope="module")
def eth_pair():
    from icp_amd import synth
    return synth.eth_like_pair(0)


def check_gradients(dev, d, k, label, n=None, ref=None):
    """The natural-cloud form of support.check_color_gradients: the points within 2x of the determinant threshold are left out, at most
    2 % of the cloud.  ref: the restatement's result when the caller has it."""
    pts, nrm, rgba = (np.asarray(d[key])[:n] for key in ("tgt_pts", "tgt_nrm", "tgt_rgba"))
    st = S.check_color_gradients(dev, pts, nrm, rgba, k, label, ref)
    print("colour gradients %s k=%d: %s" % (label, k, st))
    return st["checked"]


@pytest.mark.parametrize("k", [5, 10, 20])
def test_gradients_every_point(gpu_ctx_factory, depth_pair, eth_pair, k):
    ctx = gpu_ctx_factory()
    ctx.set_colored_options(LAM, k)
    for label, d, n in (("depth/8", depth_pair, None), ("eth 50k", eth_pair, 50000)):      # (each replaced target drops the cache)
        ref = CR.gradients(np.asarray(d["tgt_pts"])[:n], np.asarray(d["tgt_nrm"])[:n], np.asarray(d["tgt_rgba"])[:n], k, full=True)
        for knn_backend in (1, 0):                            # the target's own tree / a scratch tree
            configure(ctx, knn_backend=knn_backend)
            ctx.set_target(np.asarray(d["tgt_pts"])[:n], np.asarray(d["tgt_nrm"])[:n], np.asarray(d["tgt_rgba"])[:n])
            assert check_gradients(ctx.color_gradients(), d, k, label, n, ref) > 0


def teacher_forced(ctx, d, pose, lam):
    recs, sums, nv = ctx.correspond(pose)
    s_ref, sa = CR.record_sums(recs, pose, d["src_pts"], d["tgt_pts"], d["tgt_nrm"], ctx.color_gradients(), d["src_rgba"], d["tgt_rgba"], lam)
    assert nv == int(s_ref[0]) and sums[0] == s_ref[0] and nv > 0
    err = np.abs(sums[1:34] - s_ref[1:34]) / (sa[1:34] + 1e-300)
    assert err.max() <= 1e-9, (int(np.argmax(err)) + 1, sums[1:34], s_ref[1:34])
    pose_dev, st = ctx.iterate(pose)
    pose_ref = CR.compose(CR.solve(s_ref), pose)
    assert st["n_valid"] == nv and st["status"] == 0
    assert np.abs(pose_dev - pose_ref).max() <= 1e-5, (pose_dev, pose_ref)
    return sums, s_ref, sa


CASES = [  # (weighting, rejection, color_icp, knn_backend, lambda)
    (0, 1, 0, 1, LAM), (1, 0, 0, 1, 0.5), (2, 1, 0, 0, LAM), (3, 1, 1, 1, 0.5), (0, 0, 1, 0, LAM), (1, 1, 1, 1, LAM), (3, 0, 0, 0, 0.5)]


@pytest.mark.parametrize("weighting,rejection,color_icp,knn_backend,lam", CASES)
def test_teacher_forced_sums(gpu_ctx_factory, depth_pair, weighting, rejection, color_icp, knn_backend, lam):
    from icp_amd import synth
    ctx = gpu_ctx_factory()
    configure(ctx, weighting=weighting, rejection=rejection, color_icp=color_icp, knn_backend=knn_backend)
    ctx.set_colored_options(lam, 10)
    load(ctx, depth_pair)
    for pose in (np.eye(4, dtype=f32), synth.make_pose((0.01, -0.015, 0.02), (0.002, -0.003, 0.001)).astype(f32)):
        teacher_forced(ctx, depth_pair, pose, lam)


def test_lambda_one_is_the_plane_term(gpu_ctx_factory, depth_pair):
    """lambda = 1: the photometric term adds exact zeros; the sums are the plane rows' w^2 j_G^T j_G, w^2 j_G^T r_G alone."""
    ctx = gpu_ctx_factory()
    configure(ctx)
    ctx.set_colored_options(1.0, 20)
    load(ctx, depth_pair)
    eye = np.eye(4, dtype=f32)
    recs, sums, nv = ctx.correspond(eye)
    p = CR.transform(eye, depth_pair["src_pts"]); j = np.maximum(recs["idx"], 0)
    valid = (recs["idx"] >= 0) & np.isfinite(p).all(1)
    ok, H, g, jG, rG, *_ = CR.pair_terms(p[valid], depth_pair["tgt_pts"][j][valid], depth_pair["tgt_nrm"][j][valid],
                                         ctx.color_gradients()[j][valid], np.zeros(valid.sum()), recs["weight"][valid], 1.0)
    W2 = recs["weight"][valid][ok].astype(np.float64) ** 2
    Hg = np.einsum("m,mi,mj->ij", W2, jG, jG); gg = np.einsum("m,mi,m->i", W2, jG, rG)
    Ha = np.einsum("m,mi,mj->ij", W2, np.abs(jG), np.abs(jG)); ga = np.einsum("m,mi,m->i", W2, np.abs(jG), np.abs(rG))
    Hd, gd = CR.unpack(sums)
    assert nv == ok.sum()
    assert (np.abs(Hd - Hg) <= 1e-12 * Ha + 1e-300).all() and (np.abs(gd - gg) <= 1e-12 * ga + 1e-300).all()


def test_free_running_against_restatement(gpu_ctx_factory, depth_pair):
    ctx = gpu_ctx_factory()
    configure(ctx, n_iterations=10)
    load(ctx, depth_pair)
    pose0 = np.eye(4, dtype=f32)
    pose, recs, rc = ctx.run(pose0)
    assert rc == 0 and len(recs) == 10
    grad = ctx.color_gradients()
    prev = pose0
    for i, r in enumerate(recs):
        recs_i, _, _ = ctx.correspond(prev)
        s_ref, _ = CR.record_sums(recs_i, prev, depth_pair["src_pts"], depth_pair["tgt_pts"], depth_pair["tgt_nrm"], grad,
                                  depth_pair["src_rgba"], depth_pair["tgt_rgba"], LAM)
        assert r["n_valid"] == int(s_ref[0]), i
        ref = CR.compose(CR.solve(s_ref), prev)
        assert np.abs(r["pose"] - ref).max() <= 1e-5, (i, r["pose"], ref)
        prev = r["pose"]


@pytest.mark.parametrize("multires,selection", [(1, 0), (0, 1), (1, 1)])
def test_multires_and_sampling_deterministic(gpu_ctx_factory, depth_pair, multires, selection):
    """Multires levels and random samples: two runs are bit-identical and every iteration has valid pairs.  What a sub-sampled iteration
    computes (which points' colours it read) is checked in tests/test_gpu_query_sets.py, iteration by iteration against the restatement."""
    ctx = gpu_ctx_factory()
    configure(ctx, n_iterations=10, multires=multires, selection=selection, proba=0.5)
    load(ctx, depth_pair)
    eye = np.eye(4, dtype=f32)
    a, ra, rc = ctx.run(eye)
    b, rb, _ = ctx.run(eye)
    assert rc == 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert [r["n_valid"] for r in ra] == [r["n_valid"] for r in rb] and all(r["n_valid"] > 0 for r in ra)


def test_robust_mode(gpu_ctx_factory, depth_pair):
    """Huber with overlap 0.8: the sums are the restatement's on the records the chain kept (weights already reweighted)."""
    ctx = gpu_ctx_factory()
    configure(ctx, weighting=1)
    ctx.set_robust_options("huber", overlap=0.8)
    load(ctx, depth_pair)
    eye = np.eye(4, dtype=f32)
    recs, sums, nv = ctx.correspond(eye)
    s_ref, sa = CR.record_sums(recs, eye, depth_pair["src_pts"], depth_pair["tgt_pts"], depth_pair["tgt_nrm"], ctx.color_gradients(),
                               depth_pair["src_rgba"], depth_pair["tgt_rgba"], LAM)
    st = ctx.robust_stats()
    assert nv == int(s_ref[0]) and 0 < nv <= st[0]["n_kept"] < st[0]["n_entering"]
    assert (np.abs(sums[1:34] - s_ref[1:34]) / (sa[1:34] + 1e-300)).max() <= 1e-9
    pose, recs_run, rc = ctx.run(eye)
    assert rc == 0 and np.isfinite(pose).all()


def test_textured_plane_capability(gpu_ctx_factory):
    """The capability: geometry does not constrain the in-plane pose, colour does.  Colored ICP reaches the true pose, point-to-plane
    stays where it started."""
    d = CR.textured_plane()
    out = {}
    for metric in (4, 1):
        ctx = gpu_ctx_factory()
        configure(ctx, metric=metric, n_iterations=40, max_distance=0.01, knn_backend=1)
        load(ctx, d)
        pose, recs, rc = ctx.run(np.eye(4, dtype=f32), check=False)
        assert rc == 0
        out[metric] = pose_error(pose, d["gt"])
    assert out[4][0] < 1e-3 and out[4][1] < 1e-3, out
    assert out[1][1] > 0.02, out


def test_batch_and_align_equal_per_pair_runs(gpu_ctx_factory):
    from icp_amd import binding, eth, synth
    scans = [tuple(np.ascontiguousarray(a) for a in synth.laser_scan(synth.scan_pose(k), 40 + k, n_tilt=43, n_beam=135)[:3]) for k in range(3)]
    pairs = [dict(src_pts=scans[k + 1][0], src_nrm=scans[k + 1][1], src_rgba=scans[k + 1][2], tgt_pts=scans[k][0], tgt_nrm=scans[k][1],
                  tgt_rgba=scans[k][2]) for k in range(2)]
    pairs.append(dict(src_pts=scans[0][0], src_nrm=scans[0][1], src_rgba=scans[0][2], tgt_pts=scans[2][0], tgt_nrm=scans[2][1], tgt_rgba=scans[2][2]))
    ctxs = [gpu_ctx_factory(), gpu_ctx_factory()]
    for c in ctxs:
        configure(c, n_iterations=12, max_distance=0.05)
        c.set_colored_options(LAM, 10)
    poses, status, rc = binding.batch_run(ctxs, pairs)
    ref = gpu_ctx_factory()
    configure(ref, n_iterations=12, max_distance=0.05)
    ref.set_colored_options(LAM, 10)
    for i, d in enumerate(pairs):
        pose, recs, st = eth.align(ref, d, check=False)
        assert st == status[i]
        assert np.array_equal(binding.pose_to_c(pose).view(np.uint32), poses[i].view(np.uint32)), i


def test_track_depth_frames_equals_frame_by_frame(gpu_ctx_factory):
    """Frame 0 is the target; frames 1 and 2 are aligned to it, as with icp_set_target_depth / icp_set_source_depth / icp_run.  The
    context first ran on another target: its gradient cache must be dropped by the tracker's icp_set_target_depth path."""
    from icp_amd import binding, synth
    W, H = 80, 60
    K = np.array([[525.0 / 8, 0, 319.5 / 8], [0, 525.0 / 8, 239.5 / 8], [0, 0, 1]], f32)
    depth, rgbx = [], []
    for k in range(3):
        pts, _, rgba = synth.depth_frame(synth.camera_pose(k), K.astype(np.float64), W, H, 0x7A11 + k)
        depth.append(pts[:, 2].reshape(H, W).copy()); rgbx.append(rgba)
    depth, rgbx = np.stack(depth), np.stack(rgbx)
    cam = binding.depth_camera(K, W, H)
    to, so = binding.depth_options(False, 1), binding.depth_options(False, 2)
    a = gpu_ctx_factory()
    configure(a, n_iterations=15)
    a.set_colored_options(LAM, 10)
    a.set_target_depth(depth[2], rgbx[2], cam, to); a.set_source_depth(depth[1], rgbx[1], cam, so)
    assert a.run(np.eye(4, dtype=f32), check=False)[2] == 0                             # gradients of frame 2 cached
    _, recs, rc = a.track_depth_frames(depth, rgbx, cam, to, so)
    b = gpu_ctx_factory()
    configure(b, n_iterations=15)
    b.set_colored_options(LAM, 10)
    b.set_target_depth(depth[0], rgbx[0], cam, to)
    pose = np.eye(4, dtype=f32)
    for k in range(1, 3):
        b.set_source_depth(depth[k], rgbx[k], cam, so)
        pose, _, st = b.run(pose, check=False)
        assert recs[k - 1]["status"] == st == 0
        assert np.array_equal(recs[k - 1]["pose"].view(np.uint32), pose.view(np.uint32)), k


def test_refusals(gpu_ctx_factory, depth_pair):
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    lib, h = ctx.lib, ctx.h
    for lam, k in ((LAM, 7), (LAM, 0), (-0.1, 20), (1.5, 20), (float("nan"), 20)):
        with pytest.raises(binding.IcpError) as ei:
            ctx.set_colored_options(lam, k)
        assert ei.value.code == 1
    o = ctx.colored_options()
    assert o.lambda_geometric == f32(LAM) and o.gradient_k == 20
    configure(ctx)
    load(ctx, depth_pair)
    eye = np.eye(4, dtype=f32)
    p = ctx.params
    p.matching, p.width, p.height, p.fx, p.fy, p.cx, p.cy = 1, len(depth_pair["tgt_pts"]), 1, 500.0, 500.0, 0.0, 0.0
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
    ctx.set_source(depth_pair["src_pts"], depth_pair["src_nrm"])                       # no source colours
    assert ctx.run(eye, check=False)[2] == 1 and "colours" in lib.icp_last_error(h).decode()
    load(ctx, depth_pair)
    ctx.set_target(depth_pair["tgt_pts"], depth_pair["tgt_nrm"])                       # no target colours
    assert ctx.run(eye, check=False)[2] == 1 and "colours" in lib.icp_last_error(h).decode()
    ctx.set_target(depth_pair["tgt_pts"], None, depth_pair["tgt_rgba"])                # no target normals
    assert ctx.run(eye, check=False)[2] == 1 and "normals" in lib.icp_last_error(h).decode()
    with pytest.raises(binding.IcpError) as ei:
        ctx.color_gradients()
    assert ei.value.code == 1
    load(ctx, depth_pair)                                                               # the loop still runs after the refusals
    assert ctx.run(eye)[2] == 0


@pytest.mark.parametrize("metric", [0, 1, 2, 3])
def test_other_metrics_untouched(gpu_ctx_factory, depth_pair, metric):
    a = gpu_ctx_factory()
    a.set_colored_options(0.5, 5)
    configure(a, n_iterations=6)
    load(a, depth_pair)
    a.run(np.eye(4, dtype=f32))
    configure(a, metric=metric, n_iterations=6)
    pa, ra, rca = a.run(np.eye(4, dtype=f32), check=False)
    b = gpu_ctx_factory()
    configure(b, metric=metric, n_iterations=6)
    load(b, depth_pair)
    pb, rb, rcb = b.run(np.eye(4, dtype=f32), check=False)
    assert rca == rcb and np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert all(np.array_equal(x["pose"].view(np.uint32), y["pose"].view(np.uint32)) and x["n_valid"] == y["n_valid"] for x, y in zip(ra, rb))
