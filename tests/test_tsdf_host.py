"""Frame-to-model tracking on the host side: the numpy restatement of the TSDF contract (tests/tsdf_restatement.py) against plain fp64
geometry on a plane and on the synthetic box room, the pose compositions, option validation through the library without a device, the
new symbols, and the resource record of the three kernels (compile only)."""
import ctypes
import os
import re
import numpy as np

import tsdf_restatement as TS
from device_asm import device_asm, kernel_resources
from icp_amd.synth import tum_K as small_K

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
MINF = f32(-np.inf)


def voxel_centres(vol):
    """World positions of the voxel centres in fp64, (nz, ny, nx, 3)."""
    o = vol.o.astype(np.float64); s = float(vol.s)
    z, y, x = np.meshgrid(np.arange(vol.nz), np.arange(vol.ny), np.arange(vol.nx), indexing="ij")
    return np.stack([o[0] + x * s, o[1] + y * s, o[2] + z * s], -1)


def test_plane_field_and_raycast():
    """A fronto-parallel plane at depth z0 seen from a moved camera: every pixel reads z0, so the signed distance along z of a voxel is
    z0 - z_c whichever pixel it projects to.  The only error is fp32 rounding of the world -> camera map and of the running average:
    a few ulp of the coordinates (|p| < 4 m: ulp 2.4e-7 m, under ten operations) -- bound 1e-5 m, far below the voxel size, so a wrong
    voxel, axis or sign cannot hide in it.  The ray-cast of a field that is linear along z interpolates exactly: depth z0 within the same
    bound (times the few more operations of the march), and the normal is the plane's."""
    W, H = 40, 30
    cam = TS.Camera(small_K(W), W, H)
    from icp_amd import synth
    pose = synth.make_pose((0.05, -0.1, 0.02), (0.3, -0.2, 0.1)).astype(f32)
    z0 = 2.0
    vol = TS.Volume((48, 40, 56), (-1.9, -1.6, -0.3), voxel_size=0.08, truncation=0.4, max_weight=8)
    depth = np.full((H, W), z0, f32)
    for _ in range(3):                                      # the running average of equal samples stays put
        n_upd = TS.integrate(vol, depth, cam, pose)
    assert n_upd > 1000
    Pi = np.linalg.inv(pose.astype(np.float64))
    pc = voxel_centres(vol) @ Pi[:3, :3].T + Pi[:3, 3]
    sdf = z0 - pc[..., 2]
    seen = vol.weight > 0
    assert (vol.weight[seen] == 3).all()
    band = seen & (np.abs(sdf) < 0.4)
    assert band.sum() > 1000
    assert np.abs(vol.tsdf[band] * 0.4 - sdf[band]).max() < 1e-5 * 4
    front = seen & (sdf >= 0.4)
    assert (vol.tsdf[front] == 1).all() and front.sum() > 1000
    assert not (seen & (sdf < -0.4 - 1e-5)).any()            # nothing behind the band is written
    # voxels behind the camera or outside the image keep their bits
    u = float(cam.fx) * pc[..., 0] / pc[..., 2] + float(cam.cx)
    outside = (pc[..., 2] <= 0) | (u < -1) | (u > W)
    assert outside.sum() > 100 and (vol.weight[outside] == 0).all()
    d, vert, nrm, hits = TS.raycast(vol, cam, pose)
    ok = np.isfinite(d)
    assert hits == ok.sum() and hits > 0.8 * W * H
    assert np.abs(d[ok] - z0).max() < 1e-4
    n_ok = nrm[ok.reshape(-1)]
    assert np.abs(n_ok - np.array([0, 0, 1], f32)).max() < 1e-3   # away from the camera, as the depth normals (-du, -dv, 1)
    v_ok = vert[ok.reshape(-1)]
    assert np.array_equal(v_ok[:, 2], d[ok])


def test_room_field_and_raycast():
    """The box room from two known poses.  A voxel takes the depth of the NEAREST pixel, not of its own ray: where the depth varies by less
    than one voxel size s over the 5 x 5 pixels around it (selected below from the analytic scene), the sample differs from the depth along
    the voxel's own ray by less than s, plus half the sensor's quantisation step (1e-4).  Bound on the field: (s + 1e-4) / truncation.
    Fronto-parallel surface (the back wall from camera 0): the samples a ray-cast interpolates all lie within the quantisation of the wall's
    depth, and lerps are convex combinations: bound 2e-4 + fp32 slack on the depth."""
    from icp_amd import synth
    W, H = 80, 60
    K = small_K(W)
    cam = TS.Camera(K, W, H)
    T0 = synth.camera_pose(0)
    s, trunc = 0.1, 0.4
    vol = TS.Volume((71, 35, 89), (-3.3, -1.7, -1.6), voxel_size=s, truncation=trunc)
    poses = [np.eye(4), np.linalg.inv(T0) @ T0 @ synth.make_pose((0, np.deg2rad(6), 0), (0.05, 0, 0))]
    for k, Pk in enumerate(poses):
        pts, _, _ = synth.depth_frame(T0 @ Pk, K.astype(np.float64), W, H, 0x7A11 + k, 0.05)
        depth = pts[:, 2].reshape(H, W)
        before = vol.weight.copy()
        TS.integrate(vol, depth, cam, Pk.astype(f32))
        if k == 0:                                         # (the ray-cast of frame 0 alone: the second camera sees the wall at a slant)
            first_depth, tsdf0 = depth, vol.tsdf.copy()
            d, vert, nrm, hits = TS.raycast(vol, cam, np.eye(4, dtype=f32))
    assert (vol.weight == 2).sum() > 1000 and (vol.weight <= 2).all() and np.array_equal(before > 0, before == 1)
    # the analytic depth along every voxel's own ray from camera 0, against the field as frame 0 alone left it
    pw = voxel_centres(vol)
    zc = pw[..., 2]
    once = before == 1
    sel = np.nonzero(once.reshape(-1))[0]
    dirs_c = pw.reshape(-1, 3)[sel] / zc.reshape(-1, 1)[sel]
    th, _, _ = synth.raycast(T0[:3, 3], dirs_c @ T0[:3, :3].T)
    # smoothness of the scene over the 5 x 5 pixels around the voxel's pixel
    u = np.floor(K[0, 0] * dirs_c[:, 0] + K[0, 2] + 0.5).astype(int); v = np.floor(K[1, 1] * dirs_c[:, 1] + K[1, 2] + 0.5).astype(int)
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dc = np.stack([(uu - K[0, 2]) / K[0, 0], (vv - K[1, 2]) / K[1, 1], np.ones_like(uu)], -1).reshape(-1, 3)
    clean = synth.raycast(T0[:3, 3], dc @ T0[:3, :3].T)[0].reshape(H, W)
    pad = np.pad(clean, 2, mode="edge")
    win = np.stack([pad[a:a + H, b:b + W] for a in range(5) for b in range(5)])
    smooth = (win.max(0) - win.min(0)) < s
    inner = (u >= 2) & (u < W - 2) & (v >= 2) & (v < H - 2)
    keep = inner & smooth[np.clip(v, 0, H - 1), np.clip(u, 0, W - 1)]
    sdf = th - zc.reshape(-1)[sel]
    band = keep & (np.abs(sdf) < trunc - s)
    assert band.sum() > 500
    got = tsdf0.reshape(-1)[sel]
    assert np.abs(got[band] - sdf[band] / trunc).max() < (s + 1e-4) / trunc
    far = keep & (sdf > trunc + s)
    assert far.sum() > 500 and (got[far] == 1).all()
    # the ray-cast from camera 0 against the input depth on the back wall (world y = 4: depth 6.8 from camera 0, fronto-parallel)
    wall = (np.abs(win - 6.8).max(0) < 1e-9) & np.isfinite(d) & np.isfinite(first_depth)
    assert wall.sum() > 100
    assert np.abs(d[wall] - first_depth[wall]).max() < 2e-4 + 1e-5
    assert np.abs(nrm.reshape(H, W, 3)[wall] - np.array([0, 0, 1], f32)).max() < 1e-2
    assert hits == np.isfinite(d).sum() and hits > 0.25 * W * H          # (5 % holes in one coarse frame leave many cells with an unobserved corner)


def test_march_rules_on_crafted_volumes():
    """The rules of the march that geometry does not exercise: a ray that starts behind a surface is a hole, an exact 0 at a sample ends the
    ray there with z* = that sample's depth, a NaN never ends a ray and leaves a hole behind it, unobserved corners invalidate a cell."""
    W, H = 8, 6
    cam = TS.Camera(np.array([[10, 0, 3.5], [0, 10, 2.5], [0, 0, 1]], f32), W, H)
    eye = np.eye(4, dtype=f32)

    def volume(fn):
        vol = TS.Volume((24, 24, 24), (-1.0, -1.0, 0.0), voxel_size=0.125, truncation=0.25, min_depth=0.25, max_depth=2.5)
        z = (np.arange(24, dtype=f32) * f32(0.125))[:, None, None]
        vol.tsdf = np.broadcast_to(fn(z), (24, 24, 24)).astype(f32).copy(); vol.weight = np.ones((24, 24, 24), f32)
        return vol
    # the surface at z = 1.0: samples every 0.125 from 0.25, all on voxel planes -- sample 6 (z = 1.0) holds an exact 0
    vol = volume(lambda z: np.clip((1.0 - z) / 0.25, -1, 1))
    d, _, n, hits = TS.raycast(vol, cam, eye)
    assert hits == W * H and (d == 1.0).all() and np.abs(n - np.array([0, 0, 1], f32)).max() < 1e-6
    # the camera behind the surface: the first valid sample is <= 0
    d, _, _, hits = TS.raycast(volume(lambda z: np.clip((0.125 - z) / 0.25, -1, 1)), cam, eye)
    assert hits == 0 and (d == MINF).all()
    # a NaN slab in front of the surface: the ray goes on, and the crossing behind it has no valid positive sample in front of it
    nan_vol = volume(lambda z: np.where(np.abs(z - 0.875) < 0.01, np.nan, np.clip((1.0 - z) / 0.25, -1, 1)))
    d, _, _, hits = TS.raycast(nan_vol, cam, eye)
    assert hits == 0
    # unobserved corners: the column of cells around x = 0 is invalid, rays through it are holes, the others hit
    vol = volume(lambda z: np.clip((1.0 - z) / 0.25, -1, 1))
    vol.weight[:, :, 8] = 0
    d, _, _, hits = TS.raycast(vol, cam, eye)
    x_at_surface = (np.arange(W) - 3.5) / 10
    cut = (x_at_surface > -0.125) & (x_at_surface < 0.125)
    assert cut.any() and (d[:, cut] == MINF).all() and (d[:, ~cut] == 1.0).all() and hits == (~cut).sum() * H


def test_pose_compositions():
    from icp_amd import synth
    P = synth.make_pose((0.3, -0.2, 0.5), (0.5, -1.0, 2.0)).astype(f32)
    D = synth.make_pose((0.01, 0.02, -0.01), (0.01, 0.0, -0.02)).astype(f32)
    out = TS.compose_pose(P, D)
    assert out.dtype == f32 and np.abs(out - P.astype(np.float64) @ D.astype(np.float64)).max() < 2.4e-7
    assert np.array_equal(out[3], [0, 0, 0, 1])
    Ri, ti = TS.invert_affine(P)
    assert np.abs(Ri @ P[:3, :3].astype(np.float64) - np.eye(3)).max() < 1e-12 and np.abs(Ri @ P[:3, 3] + ti).max() < 1e-12
    G = TS.gt_in_camera(P, P)
    assert np.abs(G - np.eye(4)).max() < 1e-6
    assert np.array_equal(TS.compose_pose(np.eye(4), D), D)


def options(**kw):
    from icp_amd import binding
    base = dict(dims=(16, 16, 16), origin=(0, 0, 0))
    base.update(kw)
    return binding.tsdf_options(**base)


def test_option_validation_without_a_device():
    from icp_amd import binding
    lib = binding.load_library()
    chk = lambda o: lib.icp_tsdf_options_check(ctypes.byref(o))
    assert chk(options()) == 0
    assert lib.icp_tsdf_options_check(None) == 1
    assert chk(binding.tsdf_options()) == 1                                  # the defaults leave the dimensions to the caller
    inf, nan = float("inf"), float("nan")
    bad = [dict(dims=(1, 16, 16)), dict(dims=(16, 16, 0)), dict(dims=(2048, 2048, 512)), dict(origin=(0, nan, 0)), dict(voxel_size=0.0), dict(voxel_size=-1.0),
           dict(voxel_size=nan), dict(truncation=0.0), dict(truncation=inf), dict(max_weight=0.5), dict(max_weight=nan), dict(min_depth=0.0), dict(min_depth=9.0),
           dict(max_depth=inf), dict(ray_step=-0.1), dict(ray_step=0.3), dict(ray_step=nan), dict(truncation=1e-6, voxel_size=1e-6)]
    for kw in bad:
        assert chk(options(**kw)) == 1, kw
    good = [dict(dims=(2, 2, 2)), dict(dims=(2047, 1024, 1024)), dict(ray_step=0.25), dict(ray_step=0.01), dict(max_weight=1.0)]
    for kw in good:
        assert chk(options(**kw)) == 0, kw
    o = options()
    assert lib.icp_tsdf_options_default(None) == 1
    assert (o.voxel_size, o.truncation, o.max_weight, o.ray_step) == (f32(0.05), f32(0.25), 64.0, 0.0) and (f32(o.min_depth), o.max_depth) == (f32(0.3), 8.0)
    # every entry point refuses a null context
    cam = binding.depth_camera(small_K(40), 40, 30); p = binding.pose_to_c(np.eye(4)); n = ctypes.c_int32(0)
    so = binding.depth_options(False, 8)
    assert lib.icp_tsdf_create(None, ctypes.byref(o)) == 1 and lib.icp_tsdf_reset(None) == 1 and lib.icp_tsdf_release(None) == 1
    assert lib.icp_tsdf_download(None, None, None) == 1 and lib.icp_tsdf_upload(None, None, None) == 1
    assert lib.icp_tsdf_integrate(None, None, ctypes.byref(cam), binding._ptr(p), ctypes.byref(n)) == 1
    assert lib.icp_tsdf_raycast(None, ctypes.byref(cam), binding._ptr(p), None, None, None, ctypes.byref(n)) == 1
    assert lib.icp_set_target_tsdf(None, ctypes.byref(cam), binding._ptr(p), ctypes.byref(n)) == 1
    assert lib.icp_track_depth_model(None, None, 1, ctypes.byref(cam), ctypes.byref(so), None, binding._ptr(p), None) == 1


def test_structs_symbols_and_python_surface():
    from icp_amd import binding, tum
    assert ctypes.sizeof(binding.IcpTsdfOptions) == 12 + 12 + 6 * 4
    assert binding.IcpTsdfOptions.voxel_size.offset == 24 and binding.IcpTsdfOptions.ray_step.offset == 44
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for name in ("icp_tsdf_options_default", "icp_tsdf_options_check", "icp_tsdf_create", "icp_tsdf_reset", "icp_tsdf_release", "icp_tsdf_download", "icp_tsdf_upload",
                 "icp_tsdf_integrate", "icp_tsdf_raycast", "icp_set_target_tsdf", "icp_track_depth_model"):
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    for m in ("tsdf_create", "tsdf_reset", "tsdf_release", "tsdf_integrate", "tsdf_raycast", "set_target_tsdf", "tsdf_volume", "tsdf_upload", "track_depth_model"):
        assert hasattr(binding.Context, m), m
    import inspect
    for fn in (tum.track, tum.reconstruct_room):
        assert inspect.signature(fn).parameters["model"].default is None, fn


def test_kernel_resource_record():
    """The three kernels from the compiled code object: no scratch.  k_tsdf_integrate is a streaming pass: 20 VGPRs recorded, budget 32 (full
    occupancy with room to spare).  k_tsdf_raycast (to the host's arrays, and to the target's planes) holds a ray, eight corners in flight and
    the march state: 48 VGPRs recorded, budget 64 (8 waves per SIMD, what the latency-bound gather wants).  Static LDS is the block sum (16 B).
    Recorded: see DESIGN.md section 6m."""
    text = device_asm()
    seen = kernel_resources(text)
    budget = {"_ZN6icpdev16k_tsdf_integrate": 32, "_ZN6icpdev14k_tsdf_raycastILb0E": 64, "_ZN6icpdev14k_tsdf_raycastILb1E": 64}
    for prefix, cap in budget.items():
        ks = {n: f for n, f in seen.items() if n.startswith(prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        (name, f), = ks.items()
        desc = text[text.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        print("%s: %d VGPRs, %d AGPRs, scratch %d B, static LDS %d B" % (prefix, f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"], lds))
        assert f["private_seg_size"] == 0, f
        assert f["num_vgpr"] <= cap and f.get("num_agpr", 0) == 0, f
        assert lds <= 16, lds
