"""The coloured model on the device (icp_tsdf_color_*, icp_tsdf_integrate_color, icp_tsdf_raycast_color, icp_set_target_tsdf_color,
icp_track_depth_model_color, icp_tsdf_mesh_color): integrate, ray-cast and mesh colours against the numpy restatement of the contract
(tests/tsdf_color_restatement.py) bit for bit, the coloured target against the host route it replaces, the coloured tracking loop against a
composition of public calls, the refusals, the geometry-only paths on a volume that has colours against one that never had, and the
outcome on a flat textured wall, whose geometry leaves the lateral pose free."""
import ctypes as C
import functools
import json
import numpy as np
import pytest

import support as S
import tsdf_color_outcome_fixture as CF
import tsdf_color_restatement as TC
import tsdf_mesh_restatement as TM
import tsdf_restatement as TS
from icp_amd.synth import camera_sequence as rgbd_frames, tum_K, wavy_depth
from support import bits, same_bits, pose_of

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = f32(-np.inf)
ERR_INVALID_ARG, ERR_NO_TARGET, ERR_NO_SOURCE = 1, 3, 4
MODES = dict(colour_weighting=dict(weighting=3), colour_icp=dict(color_icp=1), colored_metric=dict(metric=4))


# this file's defaults: 35 iterations, max_distance 0.1, selection seed 0 (the library's default)
configure = functools.partial(S.configure, n_iterations=35, max_distance=0.1, seed=0)
upload = functools.partial(S.upload, color=True)

INT_OPTS = dict(dims=(37, 21, 29), origin=(-1.8, -1.0, -0.5), voxel_size=0.1, truncation=0.3, max_weight=2.0, min_depth=0.3, max_depth=2.4)


def integrate_case():
    """The frames and poses of test_integrate_matches_restatement_bit_for_bit, a seeded random colour frame for each, and a crafted start
    for both arrays with NaN payloads where no pose reaches (world z <= -0.3: behind every camera)."""
    W, H = 40, 30
    K = tum_K(W)
    rng = np.random.default_rng(3)
    shape = (29, 21, 37)
    t0 = rng.uniform(-1, 1, shape).astype(f32); w0 = rng.choice(np.array([0, 1, 1.5], f32), shape)
    c0 = rng.uniform(0, 255, shape + (3,)).astype(f32); wc0 = rng.choice(np.array([0, 1, 1.5], f32), shape)
    marked = np.zeros(shape, bool); marked[:3] = True
    t0.view(np.uint32)[marked] = 0x7FC12345; w0.view(np.uint32)[marked] = 0xFFC54321
    c0.view(np.uint32)[marked] = 0x7FC0BEEF; wc0.view(np.uint32)[marked] = 0xFFC0FACE
    d1 = wavy_depth(W, H)
    d1[0, :6] = [MINF, np.nan, np.inf, 0.0, -1.0, 2.5]
    d1[10:14, 20:24] = MINF
    d2 = wavy_depth(W, H, base=1.4); d2[5, 5] = np.nan
    poses = [np.eye(4, dtype=f32), pose_of((0.1, -0.25, 0.05), (0.3, -0.1, 0.2))]
    rgbx = [rng.integers(0, 256, (W * H, 4), dtype=np.uint8) for _ in range(2)]
    steps = [(d1, rgbx[0], poses[0]), (d2, rgbx[1], poses[1]), (d1, rgbx[1], poses[0]), (d1, rgbx[0], poses[0])]
    return K, W, H, (t0, w0, c0, wc0), marked, steps


def test_integrate_color_matches_restatement_bit_for_bit(gpu_ctx_factory):
    """Volume 37 x 21 x 29, frame 40 x 30, four integrations with max_weight = 2 (the clamp of Wc too).  After each: colour and Wc against
    the restatement bit for bit, both counts, and (tsdf, weight) bit-equal to a second context running plain icp_tsdf_integrate."""
    from icp_amd import binding
    K, W, H, (t0, w0, c0, wc0), marked, steps = integrate_case()
    cam, rcam = binding.depth_camera(K, W, H), TS.Camera(K, W, H)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    a.tsdf_create(color=True, **INT_OPTS); b.tsdf_create(**INT_OPTS)
    rgb, wc = a.tsdf_color_volume()
    assert rgb.shape == (29, 21, 37, 3) and wc.shape == (29, 21, 37) and not bits(rgb).any() and not bits(wc).any()
    vol = TC.add_color(TS.Volume(**INT_OPTS))
    a.tsdf_upload(t0, w0); b.tsdf_upload(t0, w0); a.tsdf_color_upload(c0, wc0)
    vol.tsdf, vol.weight, vol.rgb, vol.wc = t0.copy(), w0.copy(), c0.copy(), wc0.copy()
    rgb, wc = a.tsdf_color_volume()
    assert same_bits(rgb, c0) and same_bits(wc, wc0)                            # the slabs keep every bit, NaN payloads included
    for depth, rgbx, pose in steps:
        ok, paint, _, _ = TC.integrate_masks(vol, depth, rcam, pose)          # from the inputs alone
        assert (ok & ~paint).sum() > 200 and paint.sum() > 200 and not (paint & ~ok).any() and not (ok & marked).any()
        n_dev, c_dev = a.tsdf_integrate(depth, cam, pose, rgbx=rgbx)
        n_ref, c_ref = TC.integrate_color(vol, depth, rgbx, rcam, pose)
        n_plain = b.tsdf_integrate(depth, cam, pose)
        print("integrate_color: %d voxels written, %d coloured (restatement %d, %d; plain integrate %d)" % (n_dev, c_dev, n_ref, c_ref, n_plain))
        assert (n_dev, c_dev) == (n_ref, c_ref) and n_dev == n_plain and c_ref == paint.sum()
        t, w = a.tsdf_volume(); tb, wb = b.tsdf_volume(); rgb, wc = a.tsdf_color_volume()
        assert same_bits(t, tb) and same_bits(w, wb) and same_bits(t, vol.tsdf) and same_bits(w, vol.weight)
        assert same_bits(rgb, vol.rgb) and same_bits(wc, vol.wc)
    assert (bits(rgb)[marked] == 0x7FC0BEEF).all() and (bits(wc)[marked] == 0xFFC0FACE).all()
    assert (bits(t)[marked] == 0x7FC12345).all() and (bits(w)[marked] == 0xFFC54321).all()
    assert (wc == 2).sum() > 200 and (wc <= 2)[~marked].all()                  # the clamp
    # plain integrate on a volume with colours leaves the colour array alone; reset clears both; create again clears the colours
    a.tsdf_integrate(steps[1][0], cam, steps[1][2])
    rgb2, wc2 = a.tsdf_color_volume()
    assert same_bits(rgb2, rgb) and same_bits(wc2, wc)
    a.tsdf_reset()
    assert not any(bits(x).any() for x in a.tsdf_volume() + a.tsdf_color_volume())
    a.tsdf_color_upload(c0, wc0); a.tsdf_color_create()
    assert not any(bits(x).any() for x in a.tsdf_color_volume())


RAY_OPTS = dict(dims=(48, 40, 56), origin=(-1.9, -1.6, -0.4), voxel_size=0.08, truncation=0.32, max_weight=64.0, min_depth=0.3, max_depth=4.0)
RAY_POSES = [np.eye(4, dtype=f32), pose_of((0.01, 0.06, 0.0), (-0.1, 0.02, 0.05))]


def raycast_case(ctx, cam, W, H):
    """The fused volume of test_raycast_matches_restatement_bit_for_bit with colours, fused on the device; a slab of Wc = 0 cuts the
    visible surface.  Returns the restatement's volume holding the device's arrays."""
    rng = np.random.default_rng(8)
    d1 = wavy_depth(W, H, base=1.6); d1[8:11, 30:34] = MINF
    ctx.tsdf_integrate(d1, cam, np.eye(4, dtype=f32), rgbx=rng.integers(0, 256, (W * H, 4), dtype=np.uint8))
    ctx.tsdf_integrate(wavy_depth(W, H, base=1.55), cam, pose_of((0.02, 0.12, -0.03), (-0.2, 0.05, 0.1)), rgbx=rng.integers(0, 256, (W * H, 4), dtype=np.uint8))
    vol = TC.add_color(TS.Volume(**RAY_OPTS))
    vol.tsdf, vol.weight = ctx.tsdf_volume()
    vol.rgb, vol.wc = ctx.tsdf_color_volume()
    vol.wc[:, :, 18:23] = 0; vol.wc[:, 14:17, :] = 0
    ctx.tsdf_color_upload(vol.rgb, vol.wc)
    return vol


def test_raycast_color_matches_restatement_bit_for_bit(gpu_ctx_factory):
    """Volume 48 x 40 x 56, frame 40 x 30.  rgba, hits and the coloured count against the restatement from two poses, the other three arrays
    bit-equal to icp_tsdf_raycast; the restatement shows at least 50 pixels on each colour path (eight corners, nearest corner, none)."""
    from icp_amd import binding
    W, H = 40, 30
    K = tum_K(W)
    cam, rcam = binding.depth_camera(K, W, H), TS.Camera(K, W, H)
    ctx = gpu_ctx_factory()
    ctx.tsdf_create(color=True, **RAY_OPTS)
    vol = raycast_case(ctx, cam, W, H)
    seen = np.zeros(4, np.int64)
    for pose in RAY_POSES:
        d, v, n, rgba, hits, ncol = ctx.tsdf_raycast_color(cam, pose)
        rd, rv, rn, rrgba, rhits, rncol, path = TC.raycast_color(vol, rcam, pose)
        counts = np.bincount(path, minlength=4)
        print("raycast_color: %d hits, %d coloured; holes %d, no colour %d, nearest corner %d, eight corners %d" % ((rhits, rncol) + tuple(counts)))
        assert (counts[1:] >= 50).all()
        assert (hits, ncol) == (rhits, rncol)
        assert np.array_equal(rgba, rrgba)
        pd, pv, pn, phits = ctx.tsdf_raycast(cam, pose)
        assert phits == hits and same_bits(d, pd) and same_bits(v, pv) and same_bits(n, pn) and same_bits(d, rd)
        seen += counts
    # any output may be NULL
    hits2, ncol2 = C.c_int32(0), C.c_int32(0)
    ctx._ck(ctx.lib.icp_tsdf_raycast_color(ctx.h, C.byref(cam), binding._ptr(binding.pose_to_c(RAY_POSES[0])), None, None, None, None, C.byref(hits2), C.byref(ncol2)))
    assert hits2.value > 0 and ncol2.value > 0


@pytest.mark.parametrize("mode", list(MODES))
def test_coloured_model_target_matches_host_arrays(gpu_ctx_factory, mode):
    """icp_set_target_tsdf_color then icp_run == icp_set_target with icp_tsdf_raycast_color's arrays, uncoloured hits masked to holes, then
    icp_run: iteration records bit-equal under colour weighting, colour ICP and the colored metric."""
    from icp_amd import binding
    W, H = 80, 60
    K, depth, rgbx, gt = rgbd_frames(2, W, H)
    cam = binding.depth_camera(K, W, H)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    so = binding.depth_options(False, 2, fix_color_index=True)
    eye = np.eye(4, dtype=f32)
    for c in (a, b):
        configure(c, **MODES[mode])
        c.tsdf_create(color=True, **ROOM_OPTS)
        c.tsdf_integrate(depth[0], cam, eye, rgbx=rgbx[0])
    # uncoloured voxels in the band, so that some hits have no colour
    rgb, wc = b.tsdf_color_volume()
    wc[:, :, 30:33] = 0
    for c in (a, b):
        c.tsdf_color_upload(rgb, wc)
    n_a = a.set_target_tsdf(cam, eye, color=True)
    d, v, n, rgba, hits, ncol = b.tsdf_raycast_color(cam, eye)
    drop = (rgba[:, 3] == 0) & (v[:, 2] != MINF)
    print("coloured target (%s): %d hits, %d coloured, %d dropped" % (mode, hits, ncol, drop.sum()))
    assert n_a == ncol and drop.sum() == hits - ncol and drop.sum() > 20 and ncol > 0.3 * W * H
    v = v.copy(); n = n.copy(); v[drop] = MINF; n[drop] = MINF
    b.set_target(v, n, rgba)
    for c in (a, b):
        assert c.set_source_depth(depth[1], rgbx[1], cam, so) > 100
    pa, ra, rca = a.run(eye, check=False); pb, rb, rcb = b.run(eye, check=False)
    assert rca == rcb == 0 and same_bits(pa, pb) and len(ra) == len(rb) > 0
    for x, y in zip(ra, rb):
        assert (x["n_src"], x["n_valid"], x["status"]) == (y["n_src"], y["n_valid"], y["status"]) and same_bits(x["pose"], y["pose"])
        assert bits(f32(x["rmse"])) == bits(f32(y["rmse"]))
    assert ra[0]["n_valid"] > 100
    # no coloured hit at all: an empty target
    a.tsdf_color_create()
    assert a.set_target_tsdf(cam, eye, check=False, color=True) == (0, ERR_NO_TARGET)
    assert a.set_target_tsdf(cam, eye) > 0.3 * W * H                       # the geometry is still there


ROOM_OPTS = dict(dims=(71, 35, 89), origin=(-3.3, -1.7, -1.6), voxel_size=0.1, truncation=0.4)


def python_loop(ctx, K, depth, rgbx, gt, cam, so):
    """icp_track_depth_model_color as a composition of public calls (the volume exists)."""
    W, H = cam.width, cam.height
    eye = np.eye(4, dtype=f32)
    pose = eye.copy()
    ctx.tsdf_integrate(depth[0], cam, pose, rgbx=rgbx[0])
    recs = []
    for k in range(1, len(depth)):
        r = dict(n_src=0, iterations=0, status=0, initial_rmse=-1.0, final_rmse=-1.0)
        _, trc = ctx.set_target_tsdf(cam, pose, check=False, color=True)
        r["n_src"], src_rc = ctx.set_source_depth(depth[k], rgbx[k], cam, so, check=False)
        if trc or src_rc:
            r["status"] = trc or src_rc
        else:
            xyz, _, _, valid = ctx.backproject_depth(depth[k], None, K, max_distance=so.max_distance)
            idx = np.arange(0, W * H, so.downsample_factor)
            sp = xyz[idx][valid[idx]]
            ctx.set_convergence_reference(sp, ctx.transform_points(sp, TS.gt_in_camera(pose, gt[k - 1])))
            r["initial_rmse"] = ctx.rmse(eye)
            dT, its, rc = ctx.run(eye, check=False)
            r["iterations"], r["status"] = len(its), rc
            r["final_rmse"] = ctx.rmse(dT)
            if rc == 0:
                pose = TS.compose_pose(pose, dT)
                ctx.tsdf_integrate(depth[k], cam, pose, rgbx=rgbx[k])
        r["pose"] = pose.copy()
        recs.append(r)
    return pose, recs


@pytest.mark.parametrize("mode", list(MODES))
def test_track_depth_model_color_matches_composition_of_public_calls(gpu_ctx_factory, mode):
    from icp_amd import binding
    W, H = 80, 60
    K, depth, rgbx, gt = rgbd_frames(4, W, H)
    cam = binding.depth_camera(K, W, H)
    so = binding.depth_options(False, 2, fix_color_index=True)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()
    for c in (a, b):
        configure(c, **MODES[mode])
        c.tsdf_create(color=True, **ROOM_OPTS)
    pose, recs, rc = a.track_depth_model(depth, cam, so, gt=gt, rgbx_frames=rgbx)
    ref_pose, ref = python_loop(b, K, depth, rgbx, gt, cam, so)
    print("track_depth_model_color %s: statuses %s, iterations %s" % (mode, [r["status"] for r in recs], [r["iterations"] for r in recs]))
    assert rc == next((r["status"] for r in ref if r["status"]), 0) == 0
    assert len(recs) == 3
    for k, (r, h) in enumerate(zip(recs, ref)):
        assert (r["n_src"], r["iterations"], r["status"]) == (h["n_src"], h["iterations"], h["status"]), k
        assert same_bits(r["pose"], h["pose"]), k
        assert bits(f32(r["initial_rmse"])) == bits(f32(h["initial_rmse"])) and bits(f32(r["final_rmse"])) == bits(f32(h["final_rmse"])), k
    assert same_bits(pose, ref_pose) and same_bits(pose, recs[-1]["pose"])
    for x, y in zip(a.tsdf_volume() + a.tsdf_color_volume(), b.tsdf_volume() + b.tsdf_color_volume()):
        assert same_bits(x, y)
    assert a.tsdf_volume()[1].max() == 4 and a.tsdf_color_volume()[1].max() == 4      # every frame was aligned and fused, with its colours
    assert recs[0]["final_rmse"] < recs[0]["initial_rmse"]


def test_refusals(gpu_ctx_factory):
    from icp_amd import binding
    W, H = 80, 60
    K, depth, rgbx, gt = rgbd_frames(3, W, H)
    cam = binding.depth_camera(K, W, H)
    so = binding.depth_options(False, 2, fix_color_index=True)
    eye = np.eye(4, dtype=f32)
    a = gpu_ctx_factory()
    configure(a)
    lib = a.lib
    p = binding.pose_to_c(eye); n = C.c_int32(0); m = C.c_int32(0); out = (binding.IcpTrackFrame * 2)()
    p0 = lambda: binding._ptr(binding.pose_to_c(eye))                          # the loops write their pose back: a fresh one for every call
    d = np.ascontiguousarray(depth, f32); col = np.ascontiguousarray(rgbx, np.uint8)
    msg = lambda: lib.icp_last_error(a.h).decode()
    P = binding._ptr

    def track(cols=col, opt=so):
        return lib.icp_track_depth_model_color(a.h, P(d), None if cols is None else P(cols), C.c_int32(3), C.byref(cam), C.byref(opt), None, p0(), out)
    plain = lambda: lib.icp_track_depth_model(a.h, P(d), C.c_int32(3), C.byref(cam), C.byref(so), None, p0(), out)
    nv, nt = C.c_int32(0), C.c_int32(0)
    colour_calls = {
        "icp_tsdf_color_release": lambda: lib.icp_tsdf_color_release(a.h),
        "icp_tsdf_color_download": lambda: lib.icp_tsdf_color_download(a.h, None, None),
        "icp_tsdf_color_upload": lambda: lib.icp_tsdf_color_upload(a.h, P(d), P(d)),
        "icp_tsdf_integrate_color": lambda: lib.icp_tsdf_integrate_color(a.h, P(d), P(col), C.byref(cam), P(p), C.byref(n), C.byref(m)),
        "icp_tsdf_raycast_color": lambda: lib.icp_tsdf_raycast_color(a.h, C.byref(cam), P(p), None, None, None, None, C.byref(n), C.byref(m)),
        "icp_set_target_tsdf_color": lambda: lib.icp_set_target_tsdf_color(a.h, C.byref(cam), P(p), C.byref(n)),
        "icp_track_depth_model_color": track,
        "icp_tsdf_mesh_color": lambda: lib.icp_tsdf_mesh_color(a.h, C.c_float(0), 0, 0, None, None, None, None, C.byref(nv), C.byref(nt)),
    }
    # no volume at all
    assert lib.icp_tsdf_color_create(a.h) == ERR_INVALID_ARG and "no volume" in msg()
    for name, call in colour_calls.items():
        assert call() == ERR_INVALID_ARG and name in msg() and "no volume" in msg(), name
    # a volume without a colour array: every colour call refuses with a message; the plain ones work
    a.tsdf_create(**ROOM_OPTS)
    for name, call in colour_calls.items():
        assert call() == ERR_INVALID_ARG and name in msg() and "colour array" in msg(), name
    with pytest.raises(binding.IcpError):
        a.tsdf_integrate(depth[0], cam, eye, rgbx=rgbx[0])
    assert a.tsdf_integrate(depth[0], cam, eye) > 0
    # with one: the loop's own refusals
    a.tsdf_color_create()
    assert track(cols=None) == ERR_INVALID_ARG and "colour frames" in msg()
    assert track(opt=binding.depth_options(False, 2)) == ERR_INVALID_ARG and "fix_color_index" in msg()
    configure(a, metric=3)
    assert track() == ERR_INVALID_ARG and "GICP" in msg()
    assert lib.icp_tsdf_integrate_color(a.h, P(d), None, C.byref(cam), P(p), C.byref(n), C.byref(m)) == ERR_INVALID_ARG and "null" in msg()
    # icp_track_depth_model itself keeps refusing what needs target colours, colour array or not
    for kw in MODES.values():
        configure(a, **kw)
        assert plain() == ERR_INVALID_ARG and "icp_track_depth_model:" in msg() and "no colours" in msg(), kw
        a.tsdf_reset()
        assert track() == 0, kw
    # released: the colour calls refuse again, the volume lives on
    a.tsdf_color_release()
    assert colour_calls["icp_tsdf_raycast_color"]() == ERR_INVALID_ARG and "colour array" in msg()
    configure(a)
    a.tsdf_reset()
    assert plain() == 0
    # release and create (replacing a volume) free the colour array with it
    a.tsdf_color_create()
    a.tsdf_create(**ROOM_OPTS)
    assert colour_calls["icp_tsdf_color_download"]() == ERR_INVALID_ARG and "colour array" in msg()
    a.tsdf_color_create(); a.tsdf_release()
    assert colour_calls["icp_tsdf_color_download"]() == ERR_INVALID_ARG and "no volume" in msg()


def test_plain_paths_untouched_on_a_volume_with_colours(gpu_ctx_factory):
    """Context a has a colour array (cleared, then filled), context b never had one: icp_tsdf_integrate, icp_tsdf_raycast,
    icp_set_target_tsdf + icp_run, icp_track_depth_model and icp_tsdf_mesh give the same bits in both; an icp_run on a plain pair gives
    the same records before any colour call and after all of them."""
    from icp_amd import binding
    W, H = 80, 60
    K, depth, rgbx, gt = rgbd_frames(4, W, H)
    cam = binding.depth_camera(K, W, H)
    so = binding.depth_options(False, 2)
    eye = np.eye(4, dtype=f32)
    a, b = gpu_ctx_factory(), gpu_ctx_factory()

    def plain_run(c):
        configure(c)
        c.set_target_depth(depth[0], rgbx[0], cam, binding.depth_options(False, 1)); c.set_source_depth(depth[1], rgbx[1], cam, so)
        pose, recs, rc = c.run(eye, check=False)
        return pose, [(r["n_valid"], r["status"], bits(r["pose"]).tobytes(), bits(f32(r["rmse"])).tobytes()) for r in recs], rc
    before = plain_run(a)
    assert before[2] == 0 and plain_run(b)[1] == before[1]
    a.tsdf_create(color=True, **ROOM_OPTS); b.tsdf_create(**ROOM_OPTS)
    for k in range(2):
        assert a.tsdf_integrate(depth[k], cam, eye if k == 0 else gt[0]) == b.tsdf_integrate(depth[k], cam, eye if k == 0 else gt[0])
    assert all(same_bits(x, y) for x, y in zip(a.tsdf_volume(), b.tsdf_volume()))
    assert not any(bits(x).any() for x in a.tsdf_color_volume())               # plain integrate writes no colour
    a.tsdf_integrate(depth[0], cam, eye, rgbx=rgbx[0]); b.tsdf_integrate(depth[0], cam, eye)
    ra, rb = a.tsdf_raycast(cam, eye), b.tsdf_raycast(cam, eye)
    assert ra[3] == rb[3] > 0 and all(same_bits(x, y) for x, y in zip(ra[:3], rb[:3]))
    for c in (a, b):
        configure(c)
        c.set_target_tsdf(cam, eye); c.set_source_depth(depth[1], None, cam, so)
    (pa, recs_a, rca), (pb, recs_b, rcb) = a.run(eye, check=False), b.run(eye, check=False)
    assert rca == rcb == 0 and same_bits(pa, pb) and len(recs_a) == len(recs_b)
    ma, mb = a.tsdf_mesh(), b.tsdf_mesh()
    assert len(ma[0]) > 100 and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ma, mb))
    for c in (a, b):
        c.tsdf_reset()
    (pa, recs_a, rca), (pb, recs_b, rcb) = a.track_depth_model(depth, cam, so, gt=gt), b.track_depth_model(depth, cam, so, gt=gt)
    assert rca == rcb == 0 and same_bits(pa, pb)
    for x, y in zip(recs_a, recs_b):
        assert (x["n_src"], x["iterations"], x["status"]) == (y["n_src"], y["iterations"], y["status"]) and same_bits(x["pose"], y["pose"])
        assert bits(f32(x["final_rmse"])) == bits(f32(y["final_rmse"]))
    assert all(same_bits(x, y) for x, y in zip(a.tsdf_volume(), b.tsdf_volume()))
    assert not any(bits(x).any() for x in a.tsdf_color_volume())               # the geometric loop writes no colour either
    # the coloured calls, then the plain pair again
    a.tsdf_integrate(depth[0], cam, eye, rgbx=rgbx[0]); a.tsdf_raycast_color(cam, eye); a.set_target_tsdf(cam, eye, color=True); a.tsdf_mesh(colors=True)
    after = plain_run(a)
    assert after[2] == 0 and after[1] == before[1] and same_bits(after[0], before[0])


def check_mesh(ctx, vol, min_weight, what):
    v, n, t, col = ctx.tsdf_mesh(min_weight, colors=True)
    pv, pn, pt = ctx.tsdf_mesh(min_weight)
    want = TC.mesh_colors(vol, min_weight)
    print("mesh colours %s: %d vertices, %d without colour" % (what, len(want), (want[:, 3] == 0).sum()))
    assert len(v) == len(want) > 0
    assert np.array_equal(col, want), what
    for x, y in zip((v, n, t), (pv, pn, pt)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), what
    return v, n, t, col


def test_mesh_colors_match_restatement_bit_for_bit(gpu_ctx_factory):
    """The 37 x 21 x 29 sphere with holes and a crafted colour array (Wc = 0 scattered and in a slab, NaN and out-of-range channels), the
    fused volume of the integrate test, and a many-block volume (70 x 66 x 230: 1038 blocks): colours against the restatement bit for bit,
    the other arrays equal to icp_tsdf_mesh's; colors_out = NULL and the counting call."""
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    vol = TC.crafted_sphere()
    upload(ctx, vol)
    v, n, t, col = check_mesh(ctx, vol, 0.0, "sphere with holes")
    assert (col[:, 3] == 0).sum() > 20 and (col[:, 3] == 255).sum() > 500
    check_mesh(ctx, vol, 1.0, "sphere with holes, min_weight 1")
    # colors_out = NULL: the other arrays as ever; the counting call
    nv, nt = C.c_int32(0), C.c_int32(0)
    ctx._ck(ctx.lib.icp_tsdf_mesh_color(ctx.h, C.c_float(0), 0, 0, None, None, None, None, C.byref(nv), C.byref(nt)))
    assert (nv.value, nt.value) == (len(v), len(t))
    v2 = np.empty_like(v); n2 = np.empty_like(n); t2 = np.empty_like(t)
    ctx._ck(ctx.lib.icp_tsdf_mesh_color(ctx.h, C.c_float(0), nv, nt, binding._ptr(v2), binding._ptr(n2), None, binding._ptr(t2), C.byref(nv), C.byref(nt)))
    assert np.array_equal(v2.view(np.uint32), v.view(np.uint32)) and np.array_equal(n2.view(np.uint32), n.view(np.uint32)) and np.array_equal(t2, t)
    assert ctx.lib.icp_tsdf_mesh_color(ctx.h, C.c_float(0), C.c_int32(nv.value - 1), nt, binding._ptr(v2), None, None, binding._ptr(t2), C.byref(nv), C.byref(nt)) == ERR_INVALID_ARG
    # the fused volume of the integrate test
    K, W, H, (t0, w0, c0, wc0), marked, steps = integrate_case()
    cam = binding.depth_camera(K, W, H)
    ctx.tsdf_create(color=True, **INT_OPTS)
    for depth, rgbx, pose in steps:
        ctx.tsdf_integrate(depth, cam, pose, rgbx=rgbx)
    fused = TC.add_color(TS.Volume(**INT_OPTS))
    fused.tsdf, fused.weight = ctx.tsdf_volume(); fused.rgb, fused.wc = ctx.tsdf_color_volume()
    check_mesh(ctx, fused, 0.0, "fused volume")
    # many blocks
    stretched = lambda P: TM.torus((0.0, 0.0, 0.0), 1.1, 0.45)(P * np.array([1.0, 1.0, 0.3]))      # a torus drawn out along z
    big = TC.add_color(TM.analytic_volume(stretched, dims=(70, 66, 230), s=0.05, origin=(-1.72, -1.63, -5.7)))
    rng = np.random.default_rng(21)
    big.rgb = rng.uniform(0, 255, big.rgb.shape).astype(f32); big.wc = rng.choice(np.array([0, 1, 7], f32), big.wc.shape, p=[0.2, 0.4, 0.4])
    upload(ctx, big)
    vb = check_mesh(ctx, big, 0.0, "many blocks")[0]
    assert len(vb) > 20000


def test_reconstruct_room_writes_a_coloured_model_mesh(gpu_ctx_factory, tmp_path):
    """tum.reconstruct_room with model=dict(..., color=True) on a short synthetic sequence: it passes the colour frames, sets
    fix_color_index itself, and writes model_mesh as a coloured PLY whose colours are ctx.tsdf_mesh(colors=True)'s."""
    from icp_amd import meshio, tum
    W, H = 80, 60
    K, depth, rgbx, gt = rgbd_frames(3, W, H)
    seq = dict(depth=depth, rgbx=rgbx, gt=gt, K=K, width=W, height=H, frames=list(range(3)))
    ctx = gpu_ctx_factory()
    configure(ctx, **MODES["colour_weighting"])
    poses, recs, rc, paths = tum.reconstruct_room(ctx, seq, out_dir=str(tmp_path), model=dict(ROOM_OPTS, color=True), model_mesh="model.ply")
    assert rc == 0 and len(paths) == 3 and all(r["status"] == 0 for r in recs)
    v, n, t, col = meshio.load_ply_mesh(str(tmp_path / "model.ply"), colors=True)
    mv, mn, mt, mcol = ctx.tsdf_mesh(colors=True)
    assert len(v) > 1000 and np.array_equal(col, mcol) and np.array_equal(v.view(np.uint32), mv.view(np.uint32)) and np.array_equal(t, mt)
    assert (col[:, 3] == 255).sum() > 0.5 * len(col) and len(np.unique(col[:, :3], axis=0)) > 3
    assert ctx.tsdf_color_volume()[1].max() == 3
    # without color=True the mesh stays the plain 3-tuple PLY
    configure(ctx)
    tum.reconstruct_room(ctx, seq, out_dir=str(tmp_path), model=dict(ROOM_OPTS), model_mesh="plain.ply")
    assert meshio.load_ply_mesh(str(tmp_path / "plain.ply"), colors=True)[3] is None


def test_outcome_on_a_textured_wall_geometry_cannot_follow(gpu_ctx_factory):
    """The fixture of tests/tsdf_color_outcome_fixture.py: a camera facing a flat textured wall squarely slides 1 cm per frame, 12 frames
    of 160 x 120, through tum.track with the coloured model under the colored metric and with the geometric model under point-to-plane.
    Figures (translation error [m]):
      restatement loops on the CPU (tests/golden/tsdf_color_outcome.json): coloured worst frame 0.0021, geometric ends 0.1098 off (it stays
      where it started; the travel is 0.11)
      device (MI355X): coloured worst frame 0.0021 (last 0.0019, status 0), geometric ends 0.1098 off with status 0 on every frame; printed below
    The coloured loop's worst frame must stay below TWICE the restatement's (the precedent of the geometric outcome test); the geometric
    loop must end more than half the lateral travel from the truth."""
    from icp_amd import binding, tum
    with open(CF.GOLDEN) as f:
        ref = json.load(f)
    K, depth, rgbx, gt = CF.fixture()
    seq = dict(depth=depth, rgbx=rgbx, gt=gt, K=K, width=CF.W, height=CF.H)
    ctx = gpu_ctx_factory()
    ctx.set_colored_options(CF.LAMBDA, CF.GRADIENT_K)
    opts = (binding.depth_options(False, 1), binding.depth_options(False, CF.SOURCE_FACTOR))

    def run(metric, model):
        configure(ctx, metric=metric)
        _, recs, rc = tum.track(ctx, seq, with_gt=False, model=model, options=opts)
        return CF.translation_errors([np.eye(4)] + [r["pose"] for r in recs], gt), recs, rc
    ec, recs_c, rc_c = run(4, dict(CF.VOLUME, color=True))
    eg, recs_g, rc_g = run(1, dict(CF.VOLUME))
    travel = CF.STEP_M * (CF.N_FRAMES - 1)
    print("restatement: coloured worst %.4f m, geometric ends %.4f m off; device: coloured worst %.4f m (last %.4f, status %d), geometric ends %.4f m off (statuses %s); travel %.2f m"
          % (ref["colored_worst_translation_m"], ref["geometric_last_translation_m"], max(ec), ec[-1], rc_c, eg[-1], sorted(set(r["status"] for r in recs_g)), travel))
    assert ref["lateral_travel_m"] == travel and 2 * ref["colored_worst_translation_m"] < travel / 2 < ref["geometric_last_translation_m"]
    assert rc_c == 0 and all(r["status"] == 0 for r in recs_c)
    assert max(ec) < 2 * ref["colored_worst_translation_m"]
    assert eg[-1] > travel / 2
