"""The ray-cast of the hashed TSDF volume on the device (icp_tsdf_raycast_hashed, icp_set_target_tsdf_hashed, icp_track_depth_model_hashed):
against the numpy restatement of its contract (tests/htsdf_raycast_restatement.py) bit for bit on every case and camera size; against
icp_tsdf_raycast on the densified volume; independence of where the blocks sit in the pool; the model as target against the host route; the
tracking loop against a composition of public calls, also while the pool grows; the volume and the context left as they were; the refusals;
the path through tum; and the outcome on the 41-frame pan."""
import ctypes as C
import functools
import json
import os
import numpy as np
import pytest

import htsdf_cases as HC
import htsdf_raycast_cases as RC
import htsdf_raycast_outcome_fixture as ROF
import support as S
import tsdf_outcome_fixture as OF
import tsdf_restatement as TS
import tsdf_shape_cases as SC
from icp_amd.synth import camera_sequence, tum_K
from support import bits, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)
ERR_INVALID_ARG, ERR_NO_TARGET, ERR_NO_SOURCE = 1, 3, 4
configure = functools.partial(S.configure, n_iterations=35, max_distance=0.1, seed=0)
ROOM = dict(origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)


def hashed_ctx(factory, case, capacity=1 << 12, order=None):
    """A context whose hashed volume holds the case's blocks (uploaded in the given order)."""
    name, opts, c, t, w, _ = case
    ctx = factory()
    ctx.tsdf_create_hashed(block_capacity=capacity, **{k: v for k, v in opts.items() if k != "dims"})
    o = np.arange(len(c)) if order is None else order
    ctx.tsdf_upload_blocks(c[o], t[o], w[o])
    return ctx


def assert_same_cast(got, want, what):
    """(depth, vertices, normals, hits) twice: NaN-safe bit comparison of the three arrays, the hit counts equal."""
    assert got[3] == want[3], (what, got[3], want[3])
    for a, b, which in zip(got[:3], want[:3], ("depth", "vertices", "normals")):
        assert a.shape == b.shape and same_bits(a, b), (what, which, int((bits(a) != bits(b)).sum()))
    d = got[0].reshape(-1)
    assert int((d != MINF).sum()) == got[3] and ((got[1] == MINF).all(1) == (d == MINF)).all() and ((got[2] == MINF).all(1) == (d == MINF)).all(), what


@pytest.mark.parametrize("ci", range(len(RC.all_cases())), ids=[c[0] for c in RC.all_cases()])
def test_device_equals_restatement(gpu_ctx_factory, ci):
    """Every case at every camera size (1 x 1, 7 x 5, 16 x 16, 17 x 33, 64 x 48) and every pose: depth, vertices, normals and the hit count."""
    case = RC.all_cases()[ci]
    ctx = hashed_ctx(gpu_ctx_factory, case)
    total = 0
    for si, (w, h) in enumerate(RC.SIZES):
        cam = RC.camera(w, h)[0]
        for pi, P in enumerate(case[5]):
            got = ctx.tsdf_raycast_hashed(cam, P)
            assert_same_cast(got, RC.restated(ci, si, pi), (case[0], w, h, pi))
            total += got[3]
    print("%s: %d hits over %d casts" % (case[0], total, len(RC.SIZES) * len(case[5])))
    assert total > 100


@pytest.mark.parametrize("ci", range(len(RC.dense_equality_cases())), ids=[c[0] for c in RC.dense_equality_cases()])
def test_device_equals_the_dense_raycast(gpu_ctx_factory, ci):
    """P, and A - D moved to non-negative coordinates: icp_tsdf_raycast_hashed against icp_tsdf_raycast on the volume densified from voxel
    (0, 0, 0) with the same origin, bit for bit, array for array."""
    case = RC.dense_equality_cases()[ci]
    name, opts, c, t, w, poses = case
    d_opts, T, W = RC.dense_lo0(opts, c, t, w)
    hashed, dense = hashed_ctx(gpu_ctx_factory, case), gpu_ctx_factory()
    dense.tsdf_create(**d_opts)
    dense.tsdf_upload(T, W)
    total = 0
    for cw, ch in RC.SIZES:
        cam = RC.camera(cw, ch)[0]
        for pi, P in enumerate(poses):
            got, want = hashed.tsdf_raycast_hashed(cam, P), dense.tsdf_raycast(cam, P)
            assert_same_cast(got, want, (name, cw, ch, pi))
            total += got[3]
    assert total > 100


def test_pool_order_does_not_matter(gpu_ctx_factory):
    """G: P's blocks uploaded in key order and reversed, and P fused on the device from frames into a pool that starts with one block and
    grows: identical arrays, equal to the restatement's."""
    cam, _ = HC.camera()
    ci = 0
    case = RC.all_cases()[ci]
    assert case[0] == "P"
    n = len(case[2])
    ctxs = [hashed_ctx(gpu_ctx_factory, case), hashed_ctx(gpu_ctx_factory, case, order=np.arange(n)[::-1].copy())]
    for cap in (1, 1 << 12):
        g = gpu_ctx_factory()
        g.tsdf_create_hashed(block_capacity=cap, **HC.BOX)
        for d, P in zip(HC.frames(), HC.POSES):
            g.tsdf_integrate(d, cam, P)
        ctxs.append(g)
    info = ctxs[2].tsdf_blocks()[0]
    assert info["n_grown"] > 3 and info["n_blocks"] == n
    for pi, P in enumerate(case[5]):
        want = RC.restated(ci, len(RC.SIZES) - 1, pi)
        for k, ctx in enumerate(ctxs):
            assert_same_cast(ctx.tsdf_raycast_hashed(cam, P), want, ("pool order", k, pi))


def test_empty_cases_and_null_outputs(gpu_ctx_factory):
    """An empty volume and a pose looking away: all holes and no hit.  min_depth > max_depth is no volume the library creates (the options
    are refused), so the march without a sample exists in the restatement alone.  Any output may be NULL."""
    from icp_amd import binding
    case = RC.all_cases()[0]
    cam = RC.camera(17, 33)[0]
    empty = gpu_ctx_factory()
    empty.tsdf_create_hashed(**HC.BOX)
    away = RC.pose((0.0, np.pi, 0.0), (0.0, 0.0, -1.0))
    ctx = hashed_ctx(gpu_ctx_factory, case)
    for what, c, P in (("empty", empty, case[5][0]), ("away", ctx, away)):
        d, v, n, hits = c.tsdf_raycast_hashed(cam, P)
        assert hits == 0 and (d == MINF).all() and (v == MINF).all() and (n == MINF).all(), what
        assert c.set_target_tsdf_hashed(cam, P, check=False) == (0, ERR_NO_TARGET), what
        assert "hits nothing" in c.lib.icp_last_error(c.h).decode()
    bad = binding.tsdf_options(**dict(HC.BOX, min_depth=3.0, max_depth=2.4))
    assert ctx.lib.icp_tsdf_create_hashed(ctx.h, C.byref(bad), 16) == ERR_INVALID_ARG and "min_depth" in ctx.lib.icp_last_error(ctx.h).decode()
    # outputs one at a time
    P = case[5][0]
    full = ctx.tsdf_raycast_hashed(cam, P)
    npx = cam.width * cam.height
    p = binding.pose_to_c(P); hits = C.c_int32(0)
    assert ctx.lib.icp_tsdf_raycast_hashed(ctx.h, C.byref(cam), binding._ptr(p), None, None, None, C.byref(hits)) == 0 and hits.value == full[3] > 0
    for k, shape in enumerate(((npx,), (npx, 3), (npx, 3))):
        buf = np.full(shape, 7, f32)
        args = [None, None, None]; args[k] = binding._ptr(buf)
        assert ctx.lib.icp_tsdf_raycast_hashed(ctx.h, C.byref(cam), binding._ptr(p), *args, None) == 0
        assert same_bits(buf.reshape(full[k].shape), full[k]), k


@pytest.mark.parametrize("backend", [0, 1], ids=["brute", "lbvh"])
def test_model_target_on_stale_planes(gpu_ctx_factory, backend):
    """icp_set_target_tsdf_hashed on a 17 x 33 frame (561 points, 15 padded entries) in a context whose target planes held 4096 copies of
    the source as it lies at both poses, so planes beyond W H that were not rewritten with +inf would give zero-distance matches; against
    a fresh context on the host route (icp_tsdf_raycast_hashed's arrays through icp_set_target).  n_points equals n_hits; icp_correspond at
    both poses: equal indices, weights and sums, no index >= W H; icp_run: the same pose bits, records and status."""
    case = RC.all_cases()[0]
    w, h = 17, 33
    n = w * h
    assert SC.padded(n) > n
    cam = RC.camera(w, h)[0]
    a, b = hashed_ctx(gpu_ctx_factory, case), hashed_ctx(gpu_ctx_factory, case)
    for c in (a, b):
        S.configure(c, knn_backend=backend, n_iterations=10, max_distance=0.1, seed=0)
    target_pose, source_pose = case[5][0], case[5][0] @ S.pose_of((0.01, 0.02, 0.0), (-0.03, 0.02, 0.03))
    _, sv, sn, _ = b.tsdf_raycast_hashed(cam, source_pose)
    keep = sv[:, 2] != MINF
    sp, sn = np.ascontiguousarray(sv[keep]), np.ascontiguousarray(sn[keep])
    rel = (np.linalg.inv(target_pose.astype(np.float64)) @ source_pose.astype(np.float64)).astype(f32)      # aligns the source with the target
    poses = (np.eye(4, dtype=f32), rel)
    rgba = np.zeros((len(sp), 4), np.uint8)
    stale = SC.stale_cloud([(a.transform_points(sp, p), a.transform_normals(sn, p), rgba) for p in poses])
    a.set_target(stale[0], stale[1])
    hits = a.set_target_tsdf_hashed(cam, target_pose)
    d, v, nr, all_hits = b.tsdf_raycast_hashed(cam, target_pose)
    b.set_target(v, nr)
    assert hits == all_hits == RC.restated(0, RC.SIZES.index((w, h)), 0)[3] and 0 < hits < n
    for c in (a, b):
        c.set_source(sp, sn)
    for pose in poses:
        ma, sa, na = a.correspond(pose); mb, sb, nb = b.correspond(pose)
        print("target backend %d: %d hits, %d matched of %d, largest idx %d" % (backend, hits, na, len(sp), ma["idx"].max()))
        assert (ma["idx"] < n).all(), int(ma["idx"].max())
        assert na == nb and np.array_equal(ma["idx"], mb["idx"]) and same_bits(ma["weight"], mb["weight"])
        assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
    assert na > 50
    pa, ra, rca = a.run(np.eye(4, dtype=f32), check=False); pb, rb, rcb = b.run(np.eye(4, dtype=f32), check=False)
    assert rca == rcb and same_bits(pa, pb) and len(ra) == len(rb) > 0
    S.assert_same_run(ra, rb)


def python_loop(ctx, K, depth, gt, cam, so):
    """icp_track_depth_model_hashed as a composition of public calls (the volume exists)."""
    W, H = cam.width, cam.height
    eye = np.eye(4, dtype=f32)
    pose = eye.copy()
    ctx.tsdf_integrate(depth[0], cam, pose)
    recs = []
    for k in range(1, len(depth)):
        r = dict(n_src=0, iterations=0, status=0, initial_rmse=-1.0, final_rmse=-1.0)
        _, trc = ctx.set_target_tsdf_hashed(cam, pose, check=False)
        r["n_src"], src_rc = ctx.set_source_depth(depth[k], None, cam, so, check=False)
        if trc or src_rc:
            r["status"] = trc or src_rc
        else:
            if gt is not None:
                xyz, _, _, valid = ctx.backproject_depth(depth[k], None, K, max_distance=so.max_distance)
                idx = np.arange(0, W * H, so.downsample_factor)
                sp = xyz[idx][valid[idx]]
                ctx.set_convergence_reference(sp, ctx.transform_points(sp, TS.gt_in_camera(pose, gt[k - 1])))
                r["initial_rmse"] = ctx.rmse(eye)
            dT, its, rc = ctx.run(eye, check=False)
            r["iterations"], r["status"] = len(its), rc
            if gt is not None:
                r["final_rmse"] = ctx.rmse(dT)
            if rc == 0:
                pose = TS.compose_pose(pose, dT)
                ctx.tsdf_integrate(depth[k], cam, pose)
        r["pose"] = pose.copy()
        recs.append(r)
    return pose, recs


@pytest.mark.parametrize("capacity,with_gt", [(16, True), (1, False)], ids=["16 blocks, gt", "1 block"])
def test_track_depth_model_hashed_matches_composition_of_public_calls(gpu_ctx_factory, capacity, with_gt):
    """5 frames of 40 x 30 of the synthetic room, frame 2 all MINF, on a hashed volume that starts with 16 blocks, and with ONE, so that
    the pool grows inside the loop: records, poses and the blocks bit for bit; the empty frame carried and skipped with its status."""
    from icp_amd import binding
    W, H = 40, 30
    K, depth, _, gt = camera_sequence(5, W, H)
    depth[2][:] = MINF
    cam = binding.depth_camera(K, W, H)
    so = binding.depth_options(False, 1, SC.TRACK_MAX_DISTANCE)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        configure(c, max_distance=0.3)
        c.tsdf_create_hashed(block_capacity=capacity, **ROOM)
    g = gt if with_gt else None
    pose, recs, rc = a.track_depth_model_hashed(depth, cam, so, gt=g)
    ref_pose, ref = python_loop(b, K, depth, g, cam, so)
    print("track_depth_model_hashed (capacity %d): statuses %s, iterations %s, n_src %s" % (capacity, [r["status"] for r in recs], [r["iterations"] for r in recs], [r["n_src"] for r in recs]))
    assert len(recs) == 4 and rc == ERR_NO_SOURCE
    for k, (r, h) in enumerate(zip(recs, ref)):
        assert (r["n_src"], r["iterations"], r["status"]) == (h["n_src"], h["iterations"], h["status"]), k
        assert same_bits(r["pose"], h["pose"]), k
        assert bits(f32(r["initial_rmse"])) == bits(f32(h["initial_rmse"])) and bits(f32(r["final_rmse"])) == bits(f32(h["final_rmse"])), k
    assert same_bits(pose, ref_pose) and same_bits(pose, recs[-1]["pose"])
    assert [r["status"] for r in recs] == [0, ERR_NO_SOURCE, 0, 0] and same_bits(recs[1]["pose"], recs[0]["pose"]) and recs[1]["n_src"] == 0
    ai, ac, at, aw = a.tsdf_blocks(); bi, bc, bt, bw = b.tsdf_blocks()
    assert np.array_equal(ac, bc) and same_bits(at, bt) and same_bits(aw, bw)
    assert aw.max() == 4 and ai["n_grown"] == bi["n_grown"] > 0 and ai["n_unplaced"] == 0      # frames 0, 1, 3, 4: the empty one was not fused
    if with_gt:
        assert recs[0]["final_rmse"] < recs[0]["initial_rmse"] and recs[1]["initial_rmse"] == -1
    else:
        assert all(r["initial_rmse"] == -1 and r["final_rmse"] == -1 for r in recs)
    for r, gk in zip(recs, gt):
        if r["status"] == 0:
            e = OF.pose_error(r["pose"], gk)
            assert e[0] < 0.05 and e[1] < 0.1, e


def test_a_raycast_leaves_volume_and_context_as_they_were(gpu_ctx_factory):
    """Context a ray-casts (AoS) between every step, context b never does: the blocks stay bit-identical, a further integrate, an
    icp_tsdf_align_depth and a tsdf_mesh_hashed equal b's, and an icp_run before and after the ray-cast is unchanged."""
    from icp_amd import binding
    cam, _ = HC.camera()
    case = RC.all_cases()[0]
    a, b = hashed_ctx(gpu_ctx_factory, case), hashed_ctx(gpu_ctx_factory, case)
    K, depth, _, gt = camera_sequence(2, 80, 60)
    cam2 = binding.depth_camera(K, 80, 60)
    for c in (a, b):
        S.configure(c, n_iterations=10, max_distance=0.1, seed=0)
        c.set_target_depth(depth[0], None, cam2, binding.depth_options(False, 1))
        c.set_source_depth(depth[1], None, cam2, binding.depth_options(False, 4))
    before = a.tsdf_blocks()
    prm_before = binding.IcpParams(); a.lib.icp_get_params(a.h, C.byref(prm_before))
    pose_0, recs_0, _ = a.run(np.eye(4))
    for P in case[5]:
        assert a.tsdf_raycast_hashed(cam, P)[3] > 100
    after = a.tsdf_blocks()
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and same_bits(after[2], before[2]) and same_bits(after[3], before[3])
    prm_after = binding.IcpParams(); a.lib.icp_get_params(a.h, C.byref(prm_after))
    assert bytes(prm_before) == bytes(prm_after)
    pose_1, recs_1, _ = a.run(np.eye(4))
    assert same_bits(pose_0, pose_1) and len(recs_0) == len(recs_1) > 0
    S.assert_same_run(recs_0, recs_1)
    # what follows equals a context that never ray-cast
    d = HC.frames()[1]
    assert a.tsdf_integrate(d, cam, HC.POSES[1]) == b.tsdf_integrate(d, cam, HC.POSES[1]) > 1000
    a.tsdf_raycast_hashed(cam, case[5][1])
    (pa, ra, rca), (pb, rb, rcb) = (c.tsdf_align_depth(HC.frames()[2], cam, HC.POSES[2], stride=1, n_iterations=6) for c in (a, b))
    assert rca == rcb == 0 and same_bits(pa, pb) and ra["n_valid_last"] == rb["n_valid_last"] > 500
    a.tsdf_raycast_hashed(cam, case[5][0])
    ma, mb = a.tsdf_mesh_hashed(), b.tsdf_mesh_hashed()
    assert len(ma[2]) > 1000 and all(np.array_equal(S.raw_bits(x), S.raw_bits(y)) for x, y in zip(ma, mb))
    ab, bb = a.tsdf_blocks(), b.tsdf_blocks()
    assert ab[0] == bb[0] and np.array_equal(ab[1], bb[1]) and same_bits(ab[2], bb[2]) and same_bits(ab[3], bb[3])


def test_refusals(gpu_ctx_factory):
    """The three new calls without a volume and on a dense one: ICP_ERR_INVALID_ARG with a message that names the call, nothing touched; the
    loop's colour and GICP refusals and the projective camera check; the old calls still refuse a hashed volume with the message they had."""
    from icp_amd import binding
    W, H = 40, 30
    K, depth, _, gt = camera_sequence(3, W, H)
    cam = binding.depth_camera(K, W, H)
    so = binding.depth_options(False, 1, SC.TRACK_MAX_DISTANCE)
    ctx = gpu_ctx_factory()
    configure(ctx)
    lib, h = ctx.lib, ctx.h
    eye = np.eye(4, dtype=f32)
    p = binding.pose_to_c(eye); n = C.c_int32(5); out = (binding.IcpTrackFrame * 2)()
    d = np.ascontiguousarray(depth, f32)
    buf = np.full(W * H * 3, 7, f32)
    P, B = binding._ptr, C.byref
    msg = lambda: lib.icp_last_error(h).decode()
    new = {
        "icp_tsdf_raycast_hashed": lambda cm=cam: lib.icp_tsdf_raycast_hashed(h, B(cm), P(p), P(buf), None, None, B(n)),
        "icp_set_target_tsdf_hashed": lambda cm=cam: lib.icp_set_target_tsdf_hashed(h, B(cm), P(p), B(n)),
        "icp_track_depth_model_hashed": lambda cm=cam: lib.icp_track_depth_model_hashed(h, P(d), C.c_int32(3), B(cm), B(so), None, P(p), out),
    }
    for name, call in new.items():
        assert call() == ERR_INVALID_ARG and "no volume" in msg() and name in msg(), (name, msg())
    dense_opts = dict(dims=(71, 35, 89), **ROOM)
    ctx.tsdf_create(**dense_opts)
    ctx.tsdf_integrate(depth[0], cam, eye)
    t0, w0 = ctx.tsdf_volume()
    for name, call in new.items():
        assert call() == ERR_INVALID_ARG and "dense" in msg() and name in msg(), (name, msg())
    t1, w1 = ctx.tsdf_volume()
    assert same_bits(t0, t1) and same_bits(w0, w1) and (buf == 7).all() and same_bits(binding.pose_from_c(p), eye)
    # a hashed volume: bad camera, non-identity extrinsics
    ctx.tsdf_create_hashed(**ROOM)
    ctx.tsdf_integrate(depth[0], cam, eye)
    before = ctx.tsdf_blocks()
    moved = binding.depth_camera(K, W, H, S.pose_of((0, 0, 0), (0.1, 0, 0)))
    for name, call in new.items():
        assert call(moved) == ERR_INVALID_ARG and "extrinsics" in msg() and name in msg(), name
    assert lib.icp_tsdf_raycast_hashed(h, None, P(p), None, None, None, None) == ERR_INVALID_ARG
    # what needs target colours, GICP, another projective camera
    track = new["icp_track_depth_model_hashed"]
    for kw in (dict(color_icp=1), dict(weighting=3), dict(metric=4), dict(metric=3)):
        configure(ctx, **kw)
        assert track() == ERR_INVALID_ARG and "icp_track_depth_model_hashed" in msg() and len(msg()) > 40, kw
    configure(ctx, matching=1, knn_backend=0, K=K * np.array([[1.01], [1], [1]], f32), width=W, height=H)
    assert track() == ERR_INVALID_ARG and "camera" in msg()
    configure(ctx)
    after = ctx.tsdf_blocks()
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and same_bits(after[2], before[2]) and same_bits(after[3], before[3])
    # the dense volume's calls keep refusing the hashed one, with their message
    old = {
        "icp_tsdf_raycast": lambda: lib.icp_tsdf_raycast(h, B(cam), P(p), P(buf), None, None, B(n)),
        "icp_set_target_tsdf": lambda: lib.icp_set_target_tsdf(h, B(cam), P(p), B(n)),
        "icp_track_depth_model": lambda: lib.icp_track_depth_model(h, P(d), C.c_int32(3), B(cam), B(so), None, P(p), out),
    }
    for name, call in old.items():
        assert call() == ERR_INVALID_ARG and "not supported on a hashed volume (icp_tsdf_create_hashed): it needs the dense box of icp_tsdf_create" in msg() and msg().startswith(name + ":"), name
    # and the loop runs with the options icp_run accepts: projective matching, robust mode, reciprocal rejection, the convergence stop
    configure(ctx, matching=1, knn_backend=0, K=K, width=W, height=H)
    assert track() in (0, 8)
    configure(ctx, selection=1, selection_proba=0.8, selection_seed=7)
    ctx.set_robust_options("huber"); ctx.set_reciprocal_options(True); ctx.set_convergence_options(rotation=1e-4, translation=1e-4)
    ctx.tsdf_reset()
    assert track() in (0, 8)
    ctx.set_robust_options("none"); ctx.set_reciprocal_options(False); ctx.set_convergence_options(None)


def test_through_tum(tmp_path, gpu_ctx_factory):
    """tum.track(model=dict(hashed=True, raycast=True, ...)) equals Context.track_depth_model_hashed with the options it chooses, and
    tum.reconstruct_room writes the hashed model's mesh in place after tracking against its ray-cast."""
    pytest.importorskip("PIL")
    from icp_amd import binding, meshio, tum
    W, H = 80, 60
    K = tum_K(W)
    d = str(tmp_path / "seq")
    tum.write_synthetic_sequence(d, 4, width=W, height=H, K=K)
    seq = tum.load_sequence(d, frame_step=1, K=K)
    model = dict(hashed=True, raycast=True, block_capacity=64, **ROOM)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    poses, recs, rc = tum.track(a, seq, model=model)
    b.params = tum.reconstruct_room_params(b.params, K, W, H); b.push_params()
    b.tsdf_create_hashed(block_capacity=64, **ROOM)
    cam = binding.depth_camera(K, W, H)
    _, ref, rcb = b.track_depth_model_hashed(seq["depth"], cam, tum.reconstruct_room_options(b.params)[1], gt=seq["gt"])
    print("tum.track on the hashed ray-cast: statuses %s, iterations %s" % ([r["status"] for r in recs], [r["iterations"] for r in recs]))
    assert rc == rcb and len(recs) == len(ref) == 3 and len(poses) == 4
    for x, y in zip(recs, ref):
        assert (x["n_src"], x["iterations"], x["status"]) == (y["n_src"], y["iterations"], y["status"]) and same_bits(x["pose"], y["pose"])
    assert recs[0]["status"] == 0 and a.tsdf_blocks()[3].max() >= 2
    out = str(tmp_path / "out")
    c = gpu_ctx_factory()
    _, recs_c, _, paths = tum.reconstruct_room(c, seq, out_dir=out, model=model, model_mesh="m.ply", densify=False)
    assert sorted(os.listdir(out)) == ["m.ply", "mesh_0.off", "mesh_1.off", "mesh_2.off", "mesh_3.off"] and len(paths) == 4
    v, n, t = meshio.load_ply_mesh(os.path.join(out, "m.ply"))
    dv, dn, dt = c.tsdf_mesh_hashed()
    assert len(dt) > 100 and np.array_equal(bits(v), bits(dv)) and np.array_equal(t, dt)
    for x, y in zip(recs_c, recs):
        assert x["status"] == y["status"] and same_bits(x["pose"], y["pose"])
    # the ray-cast's depth image is a valid input of depth_mesh
    depth, _, _, hits = c.tsdf_raycast_hashed(cam, np.eye(4, dtype=f32))
    mv, mc, mt = c.depth_mesh(depth, None, cam, np.eye(4, dtype=f32), 0.1)
    assert hits > 1000 and len(mt) > 0 and (depth.reshape(-1)[mt.reshape(-1).astype(np.int64)] != MINF).all()      # triangles between hits only


def test_outcome_on_the_pan(gpu_ctx_factory):
    """The 41-frame, 60 degree pan of tests/tsdf_outcome_fixture.py through tum.track on a HASHED model tracked against its ray-cast, at that
    fixture's voxel size (5 cm), truncation (0.25 m) and ray step (truncation / 2), with its matcher and source options.  Figures (worst
    frame, rotation [rad] / translation [m]):
      restatement loop on the CPU (restated hashed integrate and ray-cast, the oracle's ICP; tests/golden/htsdf_raycast_outcome.json):
        0.0187 rad / 0.0702 m, 1181 blocks
      dense box, the same loop (tests/golden/tsdf_outcome.json): 0.0187 rad / 0.0702 m -- the band-only model gave the same targets
      device: printed below next to the bounds (one MI355X: 0.0187 rad / 0.0702 m, 1181 blocks)
    The bound is TWICE the restatement's worst frame with status 0 on every frame -- section 6m's margin, for its reason: a 40-frame chain
    through the model is not bit-reproducible between the oracle's ICP and the device's."""
    from icp_amd import binding, tum
    with open(ROF.GOLDEN) as f:
        ref = json.load(f)
    with open(OF.GOLDEN) as f:
        dense_ref = json.load(f)
    K, depth, gt = OF.fixture()
    seq = dict(depth=depth, rgbx=None, gt=gt, K=K, width=OF.W, height=OF.H)
    ctx = gpu_ctx_factory()
    configure(ctx, metric=1, matching=0, knn_backend=1, weighting=0, rejection=1)
    poses, recs, rc = tum.track(ctx, seq, with_gt=False, model=ROF.hashed_model(), options=(binding.depth_options(False, 1), binding.depth_options(False, OF.SOURCE_FACTOR)))
    rot, tr, last = OF.worst_errors([np.eye(4)] + [r["pose"] for r in recs], gt)
    info = ctx.tsdf_blocks()[0]
    print("restatement: worst %.4f rad / %.4f m, %d blocks (dense box: %.4f / %.4f); device on the hashed ray-cast: worst %.4f rad / %.4f m (bound %.4f / %.4f), "
          "last %.4f rad / %.4f m, status %d, %d blocks (capacity %d, %d growths), iterations %s"
          % (ref["worst_rotation_rad"], ref["worst_translation_m"], ref["n_blocks"], dense_ref["worst_rotation_rad"], dense_ref["worst_translation_m"], rot, tr,
             2 * ref["worst_rotation_rad"], 2 * ref["worst_translation_m"], last[0], last[1], rc, info["n_blocks"], info["capacity"], info["n_grown"], [r["iterations"] for r in recs]))
    assert rc == 0 and all(r["status"] == 0 for r in recs) and len(recs) == OF.N_FRAMES - 1
    assert rot < 2 * ref["worst_rotation_rad"] and tr < 2 * ref["worst_translation_m"]
    assert info["n_unplaced"] == 0 and info["n_out_of_range"] == 0
