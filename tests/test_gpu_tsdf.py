"""Frame-to-model tracking on the device (icp_tsdf_*, icp_set_target_tsdf, icp_track_depth_model): integrate and ray-cast against the numpy
restatement of the contract (tests/tsdf_restatement.py) bit for bit, the model target against the host route it replaces, the tracking
loop against a composition of public calls, the refusals, and the outcome on a pan that frame-to-frame-0 tracking cannot follow."""
import ctypes as C
import functools
import json
import numpy as np
import pytest

import support as S
import tsdf_restatement as TS
import tsdf_outcome_fixture as OF
from icp_amd.synth import camera_sequence, tum_K, wavy_depth
from support import bits, same_bits, pose_of

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)
ERR_INVALID_ARG, ERR_NO_TARGET, ERR_NO_SOURCE = 1, 3, 4


# this file's defaults: 35 iterations, max_distance 0.1, selection seed 0 (the library's default)
configure = functools.partial(S.configure, n_iterations=35, max_distance=0.1, seed=0)


def test_integrate_matches_restatement_bit_for_bit(gpu_ctx_factory):
    """Volume 37 x 21 x 29 (no multiple of the 64 x 4 x 16 thread tile on any axis, more than one block along z), frame 40 x 30 holding every
    kind of depth the contract names; two frames from different poses (the running average), one frame three times with max_weight = 2 (the
    clamp); part of the volume lies behind the camera and part outside the image: those voxels -- NaNs with a payload among them -- keep
    their bits."""
    from icp_amd import binding
    W, H = 40, 30
    K = tum_K(W)
    cam, rcam = binding.depth_camera(K, W, H), TS.Camera(K, W, H)
    opts = dict(dims=(37, 21, 29), origin=(-1.8, -1.0, -0.5), voxel_size=0.1, truncation=0.3, max_weight=2.0, min_depth=0.3, max_depth=2.4)
    ctx = gpu_ctx_factory()
    ctx.tsdf_create(**opts)
    vol = TS.Volume(**opts)
    t, w = ctx.tsdf_volume()
    assert t.shape == (29, 21, 37) and not t.any() and not w.any()
    # a crafted start: arbitrary values and weights, and NaNs with a payload where no pose below can reach (behind every camera)
    rng = np.random.default_rng(3)
    t0 = rng.uniform(-1, 1, t.shape).astype(f32); w0 = rng.choice(np.array([0, 1, 1.5], f32), t.shape)
    marked = np.zeros(t.shape, bool); marked[:3] = True                       # world z <= -0.3
    t0.view(np.uint32)[marked] = 0x7FC12345; w0.view(np.uint32)[marked] = 0xFFC54321
    ctx.tsdf_upload(t0, w0)
    vol.tsdf, vol.weight = t0.copy(), w0.copy()
    d1 = wavy_depth(W, H)
    d1[0, :6] = [MINF, np.nan, np.inf, 0.0, -1.0, 2.5]                        # 2.5 > max_depth
    d1[10:14, 20:24] = MINF
    d2 = wavy_depth(W, H, base=1.4); d2[5, 5] = np.nan
    poses = [np.eye(4, dtype=f32), pose_of((0.1, -0.25, 0.05), (0.3, -0.1, 0.2))]      # the second: part of the band leaves the image
    total = 0
    for depth, pose in [(d1, poses[0]), (d2, poses[1]), (d1, poses[0]), (d1, poses[0])]:
        n_dev = ctx.tsdf_integrate(depth, cam, pose)
        n_ref = TS.integrate(vol, depth, rcam, pose)
        t, w = ctx.tsdf_volume()
        print("integrate: %d voxels written (restatement %d)" % (n_dev, n_ref))
        assert n_dev == n_ref and 500 < n_ref < t.size - marked.sum()
        assert same_bits(t, vol.tsdf) and same_bits(w, vol.weight)
        total += n_ref
    assert (bits(t)[marked] == 0x7FC12345).all() and (bits(w)[marked] == 0xFFC54321).all()
    untouched = (bits(t) == bits(t0)) & (bits(w) == bits(w0))
    assert untouched.sum() > marked.sum() + 1000                               # outside the image and behind the band too
    assert (w == 2).sum() > 500 and (w <= 2)[~marked].all()                    # the clamp
    ctx.tsdf_reset()
    t, w = ctx.tsdf_volume()
    assert not bits(t).any() and not bits(w).any()


RAY_OPTS = dict(dims=(48, 40, 56), origin=(-1.9, -1.6, -0.4), voxel_size=0.08, truncation=0.32, max_weight=64.0, min_depth=0.3, max_depth=4.0)


def check_raycast(ctx, vol, cam, rcam, pose, what):
    d, v, n, hits = ctx.tsdf_raycast(cam, pose)
    rd, rv, rn, rhits = TS.raycast(vol, rcam, pose)
    holes = int((rd == MINF).sum())
    print("ray-cast %s: %d hits, %d holes" % (what, rhits, holes))
    assert hits == rhits, what
    assert same_bits(d, rd) and same_bits(v, rv) and same_bits(n, rn), what
    assert ((rd == MINF) == (rv[:, 2].reshape(rd.shape) == MINF)).all() and ((rd == MINF) == (rn[:, 0].reshape(rd.shape) == MINF)).all()
    return rhits, holes


def first_valid_field(vol, rcam, pose):
    """The field at the first valid sample of every ray (NaN: no valid sample), through the restatement's `field`."""
    P = np.asarray(pose, f32)
    uu, vv = np.meshgrid(np.arange(rcam.width, dtype=f32), np.arange(rcam.height, dtype=f32))
    a = (uu.reshape(-1) - rcam.cx) / rcam.fx; b = (vv.reshape(-1) - rcam.cy) / rcam.fy
    dw = [P[r, 0] * a + (P[r, 1] * b + P[r, 2] * f32(1)) for r in range(3)]
    first = np.full(len(a), np.nan, f32); found = np.zeros(len(a), bool)
    k = 0
    while True:
        z = f32(vol.min_d + f32(k) * vol.step)
        if not (z <= vol.max_d):
            return first
        valid, F = TS.field(vol, *[P[r, 3] + z * dw[r] for r in range(3)])
        new = valid & ~found
        first[new] = F[new]; found |= valid
        k += 1


def test_raycast_matches_restatement_bit_for_bit(gpu_ctx_factory):
    """Volume 48 x 40 x 56, frame 40 x 30 (no multiple of the 16 x 16 block tile: partial tiles on both axes).  The volume is fused on the
    device, downloaded, and handed to the restatement, so this compares the ray-cast alone."""
    from icp_amd import binding
    W, H = 40, 30
    K = tum_K(W)
    cam, rcam = binding.depth_camera(K, W, H), TS.Camera(K, W, H)
    ctx = gpu_ctx_factory()
    ctx.tsdf_create(**RAY_OPTS)
    d1 = wavy_depth(W, H, base=1.6); d1[8:11, 30:34] = MINF
    ctx.tsdf_integrate(d1, cam, np.eye(4, dtype=f32))
    ctx.tsdf_integrate(wavy_depth(W, H, base=1.55), cam, pose_of((0.02, 0.12, -0.03), (-0.2, 0.05, 0.1)))
    vol = TS.Volume(**RAY_OPTS)
    vol.tsdf, vol.weight = ctx.tsdf_volume()
    n = W * H
    # the camera inside the volume, at an integrated pose and between the two
    hits, holes = check_raycast(ctx, vol, cam, rcam, np.eye(4, dtype=f32), "inside")
    assert hits > 0.5 * n and holes > 0                    # (holes: the MINF block and cells next to unobserved voxels)
    check_raycast(ctx, vol, cam, rcam, pose_of((0.01, 0.06, 0.0), (-0.1, 0.02, 0.05)), "inside, between the poses")
    # outside, looking in: 1.2 m behind the volume's front face
    hits, holes = check_raycast(ctx, vol, cam, rcam, pose_of((0, 0, 0), (0.0, 0.0, -1.6)), "outside looking in")
    assert hits > 0.1 * n
    # turned away: most rays leave through the side or never enter
    hits, holes = check_raycast(ctx, vol, cam, rcam, pose_of((0, 1.0, 0), (0.0, 0.0, 0.0)), "turned away")
    assert holes > 0.5 * n
    hits, holes = check_raycast(ctx, vol, cam, rcam, pose_of((0, 3.0, 0), (0.0, 0.0, -1.0)), "missing the volume")
    assert hits == 0 and holes == n
    # starting behind the surface: the first valid sample is <= 0
    behind = pose_of((0, 0, 0), (0.0, 0.0, 1.45))
    hits, holes = check_raycast(ctx, vol, cam, rcam, behind, "behind the surface")
    first = first_valid_field(vol, rcam, behind)
    rd = TS.raycast(vol, rcam, behind)[0].reshape(-1)
    assert (first <= 0).sum() > 0.2 * n and (rd[first <= 0] == MINF).all()
    # crafted: a surface on a voxel plane with samples on voxel planes -- an exact 0 at a sample
    z = (np.arange(56, dtype=f32) * f32(0.08) + f32(-0.4))[:, None, None]
    crafted = np.broadcast_to(np.clip((f32(1.2) - z) / f32(0.32), -1, 1), (56, 40, 48)).astype(f32)
    vol.tsdf, vol.weight = crafted.copy(), np.ones_like(crafted)
    ctx.tsdf_upload(vol.tsdf, vol.weight)
    ctx2 = gpu_ctx_factory()
    o2 = dict(RAY_OPTS, origin=(-1.875, -1.5, -0.5), voxel_size=0.125, truncation=0.25, min_depth=0.25)      # dyadic: samples at 0.25 + 0.125 k land on voxel planes
    ctx2.tsdf_create(**o2)
    vol2 = TS.Volume(**o2)
    z2 = (np.arange(56, dtype=f32) * f32(0.125) + f32(-0.5))[:, None, None]
    vol2.tsdf = np.broadcast_to(np.clip((f32(1.0) - z2) / f32(0.25), -1, 1), (56, 40, 48)).astype(f32).copy(); vol2.weight = np.ones_like(vol2.tsdf)
    assert (vol2.tsdf[12] == 0).all()                      # the plane z = 1.0 holds exact zeros
    ctx2.tsdf_upload(vol2.tsdf, vol2.weight)
    d, _, _, _ = ctx2.tsdf_raycast(cam, np.eye(4, dtype=f32))
    hits, holes = check_raycast(ctx2, vol2, cam, rcam, np.eye(4, dtype=f32), "exact zero at a sample")
    assert hits == n and (d == 1.0).all()
    check_raycast(ctx, vol, cam, rcam, pose_of((0.1, -0.2, 0.05), (0.1, 0.0, 0.1)), "crafted plane, oblique")
    # NaNs in the volume: a slab in front of the surface and scattered ones; and unobserved cells
    rng = np.random.default_rng(9)
    vol.tsdf[14] = np.nan
    vol.tsdf[rng.random(vol.tsdf.shape) < 0.01] = np.nan
    vol.weight[rng.random(vol.tsdf.shape) < 0.02] = 0
    vol.weight[:, :, 20] = 0
    ctx.tsdf_upload(vol.tsdf, vol.weight)
    hits, holes = check_raycast(ctx, vol, cam, rcam, np.eye(4, dtype=f32), "NaNs and unobserved cells")
    assert holes > 0
    check_raycast(ctx, vol, cam, rcam, pose_of((0.1, -0.2, 0.05), (0.1, 0.0, 0.1)), "NaNs and unobserved cells, oblique")


ROOM_OPTS = dict(dims=(71, 35, 89), origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)


@pytest.mark.parametrize("variant", ["knn_brute", "knn_lbvh", "projective"])
def test_model_target_matches_host_arrays(gpu_ctx_factory, variant):
    """icp_set_target_tsdf then icp_correspond == icp_set_target with icp_tsdf_raycast's arrays then icp_correspond, record for record and
    sum for sum; a source, params and a convergence reference set before stay as they were."""
    from icp_amd import binding
    W, H = 160, 120
    K, depth, _, gt = camera_sequence(2, W, H)
    cam = binding.depth_camera(K, W, H)
    kw = dict(knn_brute=dict(knn_backend=0), knn_lbvh=dict(knn_backend=1), projective=dict(matching=1, knn_backend=0, K=K, width=W, height=H))[variant]
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    so = binding.depth_options(False, 4)
    eye = np.eye(4, dtype=f32)
    for c in (a, b):
        configure(c, **kw)
        c.tsdf_create(**ROOM_OPTS)
        c.tsdf_integrate(depth[0], cam, eye)
    # a: source and convergence reference first, then the model target
    n_src = a.set_source_depth(depth[1], None, cam, so)
    xyz, _, _, valid = a.backproject_depth(depth[1], None, K)
    sp = xyz[np.arange(0, W * H, 4)][valid[np.arange(0, W * H, 4)]]
    assert len(sp) == n_src
    a.set_convergence_reference(sp, a.transform_points(sp, gt[0]))
    rmse_before = a.rmse(eye)
    prm_before = bytes(a.params)
    hits = a.set_target_tsdf(cam, eye)
    # b: the host route
    d, v, n, hits_b = b.tsdf_raycast(cam, eye)
    assert hits == hits_b and hits > 0.3 * W * H
    b.set_target(v, n)
    b.set_source_depth(depth[1], None, cam, so)
    for pose in (eye, gt[0]):
        ma, sa, na = a.correspond(pose); mb, sb, nb = b.correspond(pose)
        assert na == nb and np.array_equal(ma["idx"], mb["idx"]) and same_bits(ma["weight"], mb["weight"]), variant
        assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64)), variant
    assert na > 100
    got = binding.IcpParams(); a._ck(a.lib.icp_get_params(a.h, C.byref(got)))
    assert bytes(got) == prm_before
    assert bits(f32(a.rmse(eye))) == bits(f32(rmse_before))
    pa, ra, rca = a.run(eye, check=False); pb, rb, rcb = b.run(eye, check=False)
    assert rca == rcb and same_bits(pa, pb)


def python_loop(ctx, K, depth, gt, cam, so, opts):
    """icp_track_depth_model as a composition of public calls."""
    W, H = cam.width, cam.height
    eye = np.eye(4, dtype=f32)
    ctx.tsdf_create(**opts)
    pose = eye.copy()
    ctx.tsdf_integrate(depth[0], cam, pose)
    recs = []
    for k in range(1, len(depth)):
        r = dict(n_src=0, iterations=0, status=0, initial_rmse=-1.0, final_rmse=-1.0)
        _, trc = ctx.set_target_tsdf(cam, pose, check=False)
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


@pytest.mark.parametrize("case", ["no_gt", "gt", "gt_empty_frame"])
def test_track_depth_model_matches_composition_of_public_calls(gpu_ctx_factory, case):
    from icp_amd import binding
    W, H = 80, 60
    K, depth, _, gt = camera_sequence(4, W, H)
    if case == "gt_empty_frame":
        depth[2][:] = MINF
    cam = binding.depth_camera(K, W, H)
    so = binding.depth_options(False, 2)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    configure(a); configure(b)
    g = None if case == "no_gt" else gt
    a.tsdf_create(**ROOM_OPTS)
    pose, recs, rc = a.track_depth_model(depth, cam, so, gt=g)
    ref_pose, ref = python_loop(b, K, depth, g, cam, so, ROOM_OPTS)
    print("track_depth_model %s: statuses %s, iterations %s" % (case, [r["status"] for r in recs], [r["iterations"] for r in recs]))
    assert rc == next((r["status"] for r in ref if r["status"]), 0)
    assert len(recs) == 3
    for k, (r, h) in enumerate(zip(recs, ref)):
        assert (r["n_src"], r["iterations"], r["status"]) == (h["n_src"], h["iterations"], h["status"]), k
        assert same_bits(r["pose"], h["pose"]), k
        assert bits(f32(r["initial_rmse"])) == bits(f32(h["initial_rmse"])) and bits(f32(r["final_rmse"])) == bits(f32(h["final_rmse"])), k
    assert same_bits(pose, ref_pose) and same_bits(pose, recs[-1]["pose"])
    ta, wa = a.tsdf_volume(); tb, wb = b.tsdf_volume()
    assert same_bits(ta, tb) and same_bits(wa, wb)
    assert recs[0]["status"] == 0 and wa.max() >= 2                        # a frame was aligned and fused
    if case == "no_gt":
        assert all(r["initial_rmse"] == -1 and r["final_rmse"] == -1 for r in recs)
    else:
        assert recs[0]["final_rmse"] < recs[0]["initial_rmse"]
    if case == "gt_empty_frame":
        assert rc == ERR_NO_SOURCE and recs[1]["status"] == ERR_NO_SOURCE and recs[1]["n_src"] == 0 and recs[1]["initial_rmse"] == -1
        assert same_bits(recs[1]["pose"], recs[0]["pose"])
        assert recs[2]["status"] == 0 and wa.max() == 3                   # frames 0, 1 and 3: the empty one was not fused


def test_refusals_and_untouched_frame0_path(gpu_ctx_factory):
    from icp_amd import binding, tum
    W, H = 80, 60
    K, depth, _, gt = camera_sequence(3, W, H)
    cam = binding.depth_camera(K, W, H)
    so = binding.depth_options(False, 2)
    eye = np.eye(4, dtype=f32)
    a = gpu_ctx_factory()
    configure(a)
    p = binding.pose_to_c(eye); n = C.c_int32(0); out = (binding.IcpTrackFrame * 2)()
    d = np.ascontiguousarray(depth, f32)
    track = lambda cm=cam: a.lib.icp_track_depth_model(a.h, binding._ptr(d), C.c_int32(3), C.byref(cm), C.byref(so), None, binding._ptr(p), out)
    msg = lambda: a.lib.icp_last_error(a.h).decode()
    # no volume
    assert a.lib.icp_tsdf_reset(a.h) == ERR_INVALID_ARG and "no volume" in msg()
    assert a.lib.icp_tsdf_release(a.h) == ERR_INVALID_ARG
    assert a.lib.icp_tsdf_download(a.h, None, None) == ERR_INVALID_ARG
    assert a.lib.icp_tsdf_integrate(a.h, binding._ptr(d), C.byref(cam), binding._ptr(p), C.byref(n)) == ERR_INVALID_ARG
    assert a.lib.icp_tsdf_raycast(a.h, C.byref(cam), binding._ptr(p), None, None, None, C.byref(n)) == ERR_INVALID_ARG
    assert a.lib.icp_set_target_tsdf(a.h, C.byref(cam), binding._ptr(p), C.byref(n)) == ERR_INVALID_ARG
    assert track() == ERR_INVALID_ARG and "no volume" in msg()
    # bad options, with a message
    bad = binding.tsdf_options(dims=(1, 8, 8), origin=(0, 0, 0))
    assert a.lib.icp_tsdf_create(a.h, C.byref(bad)) == ERR_INVALID_ARG and "dimension" in msg()
    a.tsdf_create(**ROOM_OPTS)
    # non-identity depth extrinsics
    moved = binding.depth_camera(K, W, H, pose_of((0, 0, 0), (0.1, 0, 0)))
    assert a.lib.icp_tsdf_integrate(a.h, binding._ptr(d), C.byref(moved), binding._ptr(p), C.byref(n)) == ERR_INVALID_ARG and "extrinsics" in msg()
    assert a.lib.icp_set_target_tsdf(a.h, C.byref(moved), binding._ptr(p), C.byref(n)) == ERR_INVALID_ARG
    assert track(moved) == ERR_INVALID_ARG
    # an empty model: no hits
    assert a.set_target_tsdf(cam, eye, check=False) == (0, ERR_NO_TARGET)
    # what needs target colours, and GICP
    for kw in (dict(color_icp=1), dict(weighting=3), dict(metric=4), dict(metric=3)):
        configure(a, **kw)
        assert track() == ERR_INVALID_ARG and "icp_track_depth_model" in msg() and len(msg()) > 30, kw
    # projective matching with another camera in the params
    configure(a, matching=1, knn_backend=0, K=K * np.array([[1.01], [1], [1]], f32), width=W, height=H)
    assert track() == ERR_INVALID_ARG and "camera" in msg()
    configure(a, matching=1, knn_backend=0, K=K, width=W, height=H)
    assert track() in (0, 8)
    # accepted with the options icp_run accepts: robust mode, reciprocal rejection, the convergence stop, a selection
    configure(a, selection=1, selection_proba=0.8, selection_seed=7)
    a.set_robust_options("huber"); a.set_reciprocal_options(True); a.set_convergence_options(rotation=1e-4, translation=1e-4)
    a.tsdf_reset()
    assert track() in (0, 8)
    a.set_robust_options("none"); a.set_reciprocal_options(False); a.set_convergence_options(None)
    # the frame-0 path after all that, against a context that never made a TSDF call
    a.tsdf_release()
    b = gpu_ctx_factory()
    rgbx = np.zeros((3, W * H, 4), np.uint8)
    res = []
    for c in (a, b):
        configure(c)
        to, so8 = tum.reconstruct_room_options(c.params)
        res.append(c.track_depth_frames(depth, rgbx, cam, to, so8, gt=gt))
    (pa, ra, rca), (pb, rb, rcb) = res
    assert rca == rcb and same_bits(pa, pb)
    for x, y in zip(ra, rb):
        assert (x["n_src"], x["iterations"], x["status"]) == (y["n_src"], y["iterations"], y["status"]) and same_bits(x["pose"], y["pose"])
        assert bits(f32(x["initial_rmse"])) == bits(f32(y["initial_rmse"])) and bits(f32(x["final_rmse"])) == bits(f32(y["final_rmse"]))


def test_outcome_on_a_pan_frame0_tracking_cannot_follow(gpu_ctx_factory):
    """The 60 degree pan of tests/tsdf_outcome_fixture.py, 41 frames of 320 x 240, through tum.track with model=None and with the model.
    Figures (worst frame, rotation [rad] / translation [m]):
      restatement loop on the CPU (numpy ray-cast and integrate, the oracle's ICP; tests/golden/tsdf_outcome.json): 0.0187 rad / 0.0702 m
      device, frame-to-model and frame-to-frame-0: printed below, not recorded here yet (CPU prototype of the frame-0 loop: ends 1.23 m off)
    The model loop's worst frame must stay below TWICE the restatement's (a 40-frame chain through the model is not bit-reproducible
    between the oracle's ICP and the device's); the frame-0 loop must end more than 0.5 m from the truth."""
    from icp_amd import binding, tum
    with open(OF.GOLDEN) as f:
        ref = json.load(f)
    K, depth, gt = OF.fixture()
    seq = dict(depth=depth, rgbx=None, gt=gt, K=K, width=OF.W, height=OF.H)
    ctx = gpu_ctx_factory()

    def run(model):
        configure(ctx, metric=1, matching=0, knn_backend=1, weighting=0, rejection=1)
        poses, recs, rc = tum.track(ctx, seq, with_gt=False, model=model, options=(binding.depth_options(False, 1), binding.depth_options(False, OF.SOURCE_FACTOR)))
        return [r["pose"] for r in recs], recs, rc
    frame0, recs0, _ = run(None)
    model, recs, rc = run(OF.VOLUME)
    e0 = OF.pose_error(frame0[-1], gt[-1])
    rot, tr, last = OF.worst_errors([np.eye(4)] + model, gt)
    print("restatement: worst %.4f rad / %.4f m; device model loop: worst %.4f rad / %.4f m, last %.4f rad / %.4f m, status %d; frame-0 loop ends %.4f rad / %.4f m off, statuses %s"
          % (ref["worst_rotation_rad"], ref["worst_translation_m"], rot, tr, last[0], last[1], rc, e0[0], e0[1], sorted(set(r["status"] for r in recs0))))
    assert e0[1] > 0.5
    assert rc == 0 and all(r["status"] == 0 for r in recs)
    # the bound: twice the restatement's worst frame, 2 x 0.0187 rad and 2 x 0.0702 m (tests/golden/tsdf_outcome.json, written by
    # tests/tsdf_outcome_fixture.py); the frame-0 loop's 0.5 m is the issue's, against 1.23 m on the CPU prototype
    assert rot < 2 * ref["worst_rotation_rad"] and tr < 2 * ref["worst_translation_m"]
