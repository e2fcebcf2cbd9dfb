"""The depth mesh of reconstructRoom on the device (icp_depth_mesh: SimpleMesh(sensor, cameraPose, edgeThreshold), SimpleMesh.h:36-119)
against the numpy restatement tests/depth_mesh_restatement.py, bit for bit: vertices, colours and the triangle list in addFace order.
Also the edge cases, the context it leaves alone, and tum.reconstruct_room end to end (saveRoomToFile, utils.h:179-193)."""
import ctypes as C
import os
import numpy as np
import pytest

from depth_mesh_restatement import mesh_spec
from icp_amd.synth import camera_sequence as synth_frames, tum_K
from support import pose_of as make_pose

pytestmark = pytest.mark.gpu
f32 = np.float32
MINF = -np.inf


def check(ctx, depth, rgbx, K, pose, thr, color=None):
    """Device vs restatement, bit for bit; returns the restatement's floored colour columns."""
    from icp_amd import binding
    h, w = depth.shape
    cam = binding.depth_camera(K, w, h)
    ccam = None if color is None else binding.color_camera(color[0], color[2], color[3], color[1])
    v, c, t = ctx.depth_mesh(depth, rgbx, cam, pose, thr, color_cam=ccam)
    sv, sc, st, fu, fv = mesh_spec(depth, rgbx, K, pose, thr, color=color, details=True)
    assert np.array_equal(v.view(np.uint32), sv.view(np.uint32)), "vertices"
    if rgbx is None:
        assert c is None
    else:
        assert np.array_equal(c, sc), ("colours", int((c != sc).any(axis=1).sum()))
    assert t.dtype == np.uint32 and t.shape == st.shape and np.array_equal(t, st), ("triangles", len(t), len(st))
    return fu, fv, st


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()


@pytest.fixture(scope="module")
def tracked_poses(gpu_ctx_factory):
    """The camera poses tum.track returns on a 3-frame synthetic sequence (point-to-plane, LBVH k-NN)."""
    from icp_amd import binding, tum
    K, depth, rgbx, gt = synth_frames(3, 160, 120)
    seq = dict(frames=[0, 1, 2], depth=depth, rgbx=rgbx, gt=gt, K=K, width=160, height=120)
    p = binding.default_params(); p.metric = 1; p.knn_backend = 1
    poses, _, rc = tum.track(gpu_ctx_factory(), seq, p)
    assert rc == 0 and len(poses) == 3
    return poses


FAR = make_pose((0.1, 0.2, -0.3), (3.0e6, -2.0e6, 1.0e6))


def other_color_camera(w, h, seed):
    """A colour camera that is not the depth camera: other intrinsics, rotated and shifted, on a frame of its own size."""
    wc, hc = w // 2 + 3, h // 2 + 1
    Kc = np.array([[0.7 * w, 0, wc / 2.0 - 1.5], [0, 0.7 * w, hc / 2.0 + 2.0], [0, 0, 1]], f32)
    Ec = make_pose((0.02, -0.05, 0.01), (0.04, -0.03, 0.02))
    rgbx = np.random.default_rng(seed).integers(0, 256, (wc * hc, 4), dtype=np.uint8)
    return rgbx, (Kc, Ec, wc, hc)


@pytest.mark.parametrize("w,h", [(160, 120), (320, 240), (640, 480)])
def test_mesh_bit_exact(ctx, tracked_poses, w, h):
    K, depth, rgbx, _ = synth_frames(2, w, h)
    cases = [("identity", np.eye(4, dtype=f32), depth[0], rgbx[0], None)]
    cases += [("tracked%d" % k, P, depth[k % 2], rgbx[k % 2], None) for k, P in enumerate(tracked_poses[1:], 1)]
    cases += [("far", FAR, depth[1], rgbx[1], None)]
    orgbx, color = other_color_camera(w, h, w)
    cases += [("color_cam", tracked_poses[-1], depth[1], orgbx, color)]
    for name, P, d, c, col in cases:
        for thr in (0.01, 0.1, 0.0, np.inf):
            fu, fv, st = check(ctx, d, c, K, P, thr, col)
            if thr == 0.0:
                assert len(st) == 0
            if thr == np.inf:
                assert len(st) > 0, name
        ok = d.reshape(-1) != MINF
        wc = w if col is None else col[2]
        if name == "far":                                   # re-projections leave the colour frame
            assert ((fu[ok] < 0) | (fu[ok] >= wc)).any()
    # without colours: the same vertices and triangles
    check(ctx, depth[0], None, K, tracked_poses[1], 0.1)


def test_left_neighbour_colours_at_identity(ctx):
    """640x480, identity pose: some pixels take their colour from the left / upper neighbour (the round trip lands on u - eps), and the
    device agrees with the restatement on every one of them."""
    K, depth, rgbx, _ = synth_frames(1, 640, 480)
    fu, fv, _ = check(ctx, depth[0], rgbx[0], K, np.eye(4), 0.1)
    ok = depth[0].reshape(-1) != MINF
    v, u = np.divmod(np.arange(640 * 480), 640)
    assert ((fu - u)[ok] == -1).sum() > 0 and ((fv - v)[ok] == -1).sum() > 0


def test_edge_cases(ctx):
    from icp_amd import binding
    K = np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]], f32)
    for shape in ((1, 1), (1, 9), (9, 1)):
        d = np.linspace(1, 2, shape[0] * shape[1]).astype(f32).reshape(shape)
        col = np.full((d.size, 4), 5, np.uint8)
        v, c, t = ctx.depth_mesh(d, col, binding.depth_camera(K, shape[1], shape[0]), np.eye(4), np.inf)
        assert len(t) == 0 and v.shape == (d.size, 3)
        check(ctx, d, col, K, np.eye(4), np.inf)
    hole = np.full((6, 7), MINF, f32)
    v, c, t = ctx.depth_mesh(hole, np.full((42, 4), 9, np.uint8), binding.depth_camera(K, 7, 6), np.eye(4), np.inf)
    assert np.all(v == MINF) and np.all(c == 0) and len(t) == 0
    v, c, t = ctx.depth_mesh(np.ones((2, 2), f32), None, binding.depth_camera(K, 2, 2), np.eye(4), 2.0)
    assert t.tolist() == [[0, 2, 1], [2, 3, 1]] and c is None
    # an all-valid 640x480 frame at threshold inf: every quad gives two triangles (1196 blocks: the scan's carry between chunks)
    Kt = tum_K(640)
    flat = np.full((480, 640), 1.5, f32)
    v, c, t = ctx.depth_mesh(flat, None, binding.depth_camera(Kt, 640, 480), np.eye(4), np.inf)
    assert len(t) == 2 * 639 * 479 == 612162
    check(ctx, flat, None, Kt, np.eye(4), np.inf)
    # NaN and +inf depths go through the arithmetic (not holes); the colours of NaN pixels come from column 0
    K8, depth, rgbx, _ = synth_frames(1, 160, 120)
    d = depth[0].copy().reshape(-1)
    rng = np.random.default_rng(3)
    k = rng.permutation(d.size)
    d[k[:300]] = np.nan; d[k[300:600]] = np.inf
    d = d.reshape(120, 160)
    for P in (np.eye(4, dtype=f32), make_pose((0.1, 0.0, 0.2), (0.5, 0.1, -0.3))):
        for thr in (0.1, np.inf):
            check(ctx, d, rgbx[0], K8, P, thr)
            v, c, _ = ctx.depth_mesh(d, rgbx[0], binding.depth_camera(K8, 160, 120), P, thr)
            assert np.isnan(v[k[:300]]).all(axis=1).any() and not np.isfinite(v[k[300:600]]).all(axis=1).any()


def test_bad_arguments(ctx):
    from icp_amd import binding
    lib = ctx.lib
    K = tum_K(160)
    cam = binding.depth_camera(K, 16, 12)
    d = np.ones(16 * 12, f32); cols = np.zeros((16 * 12, 4), np.uint8)
    v = np.empty((16 * 12, 3), f32); t = np.empty((2 * 15 * 11, 3), np.uint32); n = C.c_int32(-1)
    p = binding.pose_to_c(np.eye(4)); P = binding._ptr

    def call(depth=P(d), rgbx=P(cols), cam_=C.byref(cam), ccam=None, pose=P(p), vo=P(v), co=P(cols), to=P(t), no=C.byref(n)):
        return lib.icp_depth_mesh(ctx.h, depth, rgbx, cam_, ccam, pose, C.c_float(0.1), vo, co, to, no)
    assert call() == 0 and n.value > 0
    assert call(rgbx=None) == 1                     # colours without a colour frame
    assert call(rgbx=None, co=None) == 0
    for kw in (dict(depth=None), dict(cam_=None), dict(pose=None), dict(vo=None), dict(to=None), dict(no=None)):
        assert call(**kw) == 1, kw
    for w, h in ((0, 12), (16, -1), (1 << 16, 1 << 16), (40000, 40000)):       # the last: 2 (w - 1)(h - 1) > INT32_MAX
        bad = binding.depth_camera(K, w, h)
        assert call(cam_=C.byref(bad)) == 1
    assert call(ccam=C.byref(binding.color_camera(K, 0, 5))) == 1
    bad = binding.depth_camera(K, 16, 12); bad.fx = float("nan")
    assert call(cam_=C.byref(bad)) == 1


def test_context_left_alone(gpu_ctx_factory):
    """icp_run on the resident pair gives bit-identical poses before and after icp_depth_mesh; the params do not change."""
    from icp_amd import binding
    ctx = gpu_ctx_factory()
    K, depth, rgbx, gt = synth_frames(2, 160, 120)
    cam = binding.depth_camera(K, 160, 120)
    p = ctx.params; p.metric = 1; p.knn_backend = 1; p.n_iterations = 10; p.max_distance = 0.1
    ctx.push_params()
    ctx.set_target_depth(depth[0], rgbx[0], cam, binding.depth_options(False, 1))
    ctx.set_source_depth(depth[1], rgbx[1], cam, binding.depth_options(False, 4))
    src = np.ones((64, 3), f32)
    ctx.set_convergence_reference(src, src)
    before = binding.IcpParams(); ctx.lib.icp_get_params(ctx.h, C.byref(before))
    pose_a, recs_a, _ = ctx.run(np.eye(4))
    rmse_a = ctx.rmse(pose_a)
    K6, d6, c6, _ = synth_frames(1, 640, 480, seed=5)
    ctx.depth_mesh(d6[0], c6[0], binding.depth_camera(K6, 640, 480), FAR, 0.1)
    after = binding.IcpParams(); ctx.lib.icp_get_params(ctx.h, C.byref(after))
    assert bytes(before) == bytes(after)
    pose_b, recs_b, _ = ctx.run(np.eye(4))
    assert np.array_equal(pose_a.view(np.uint32), pose_b.view(np.uint32)) and len(recs_a) == len(recs_b)
    assert np.float32(ctx.rmse(pose_b)) == np.float32(rmse_a)


def test_reconstruct_room_end_to_end(tmp_path, gpu_ctx_factory):
    pytest.importorskip("PIL")
    from icp_amd import binding, meshio, tum
    d = str(tmp_path / "seq")
    tum.write_synthetic_sequence(d, 21)
    seq = tum.load_sequence(d)
    assert seq["frames"] == [0, 10, 20] and seq["width"] == 640

    def params():
        p = binding.default_params(); p.metric = 1; p.knn_backend = 1
        return p
    out = str(tmp_path / "out")
    poses, recs, rc, paths = tum.reconstruct_room(gpu_ctx_factory(), seq, params(), out_dir=out)
    want_poses, want_recs, want_rc = tum.track(gpu_ctx_factory(), seq, params())
    assert rc == want_rc and len(poses) == 3
    for a, b in zip(poses, want_poses):
        assert np.array_equal(np.asarray(a, f32).view(np.uint32), np.asarray(b, f32).view(np.uint32))
    assert sorted(os.listdir(out)) == ["mesh_0.off", "mesh_10.off", "mesh_20.off"]
    assert paths == [os.path.join(out, "mesh_%d.off" % k) for k in (0, 10, 20)]
    for k, P in enumerate(poses):
        mesh = meshio.join_meshes(mesh_spec(seq["depth"][k], seq["rgbx"][k], seq["K"], P, 0.1), meshio.camera_glyph(P, 0.0015))
        ref = str(tmp_path / ("ref_%d.off" % k))
        meshio.write_off(ref, *mesh)
        assert open(paths[k], "rb").read() == open(ref, "rb").read(), k
    # without out_dir: the meshes themselves
    _, _, _, meshes = tum.reconstruct_room(gpu_ctx_factory(), seq, params())
    assert len(meshes) == 3 and meshes[0][0].shape == (640 * 480 + 8, 3) and len(meshes[0][2]) > 0
