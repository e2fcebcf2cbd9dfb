"""Host side of the RGB-D tracking runner (reference: VirtualSensor.h and reconstructRoom, main.cpp:183-341).

Pure host logic over `formats.py`; the tracking itself is one library call (`icp_track_depth_frames`):
  seq            = load_sequence(tum_dir)                     # VirtualSensor(frameStep).init + processFrameIndex(0, (i+1) * step, ...)
  tgt_o, src_o   = reconstruct_room_options(params)           # the reference's choice of clouds, 35 iterations, max distance 0.1
  poses, recs    = track(ctx, seq, params)                    # estimatedPoses (currentCameraToWorld^-1 per frame) + per-frame records
  reconstruct_room(ctx, seq, params, out_dir)                 # track + saveRoomToFile per frame: mesh_<frame>.off (utils.h:179-193)
  reconstruct_room(..., model=..., model_mesh="model.ply")     # frame-to-model tracking, and the fused volume as one mesh
  reconstruct_room(..., model=..., sdf=dict(stride=2))         # the same model, every frame aligned to the volume itself (direct SDF tracking)
  reconstruct_room(..., model=dict(color=True, ...), sdf=dict(stride=4, color_weight=0.1))   # ... with the photometric term from the colour array
Layout on disk, as the reference expects it under Data/: <tum_dir>/depth.txt, rgb.txt, groundtruth.txt and the PNGs they list (TUM RGB-D).
`write_synthetic_sequence` writes that layout from `synth.depth_frame` / `synth.camera_pose`, for the tests and for rehearsing a real
freiburg1_xyz run offline.
"""
import os
import numpy as np

from . import binding, formats, meshio, synth, tsdf_local

TUM_K = np.array([[525.0, 0.0, 319.5], [0.0, 525.0, 239.5], [0.0, 0.0, 1.0]], np.float32)     # VirtualSensor.h:44-46
TUM_WIDTH, TUM_HEIGHT = 640, 480


def frame_schedule(n_frames, frame_step=10, i_max=10):
    """Frame indices reconstructRoom processes: 0, then (i + 1) * frame_step while that frame exists and i <= i_max (main.cpp:278-281)."""
    out = [0]
    i = 0
    while (i + 1) * frame_step < n_frames and i <= i_max:
        out.append((i + 1) * frame_step)
        i += 1
    return out


def load_sequence(tum_dir, frame_step=10, i_max=10, K=None):
    """Depth (MINF holes), RGBX bytes and ground-truth pose of every scheduled frame.  Returns a dict with
    frames (indices), depth (n, h, w) float32, rgbx (n, h*w, 4) uint8, trajectory (n 4x4: the nearest-timestamp pose, stored inverted as
    readTrajectoryFile does), gt ((n - 1) 4x4: targetTrajectory * trajectory_k^-1, main.cpp:298-300), K, width, height."""
    d_ts, d_names = formats.read_tum_file_list(os.path.join(tum_dir, "depth.txt"))
    c_ts, c_names = formats.read_tum_file_list(os.path.join(tum_dir, "rgb.txt"))
    t_ts, t_poses = formats.read_tum_trajectory(os.path.join(tum_dir, "groundtruth.txt"))
    if len(d_names) != len(c_names):
        raise ValueError("depth.txt and rgb.txt list different numbers of frames (VirtualSensor.h:35)")
    frames = frame_schedule(len(c_names), frame_step, i_max)
    depth, rgbx, traj = [], [], []
    for k in frames:
        d, c = formats.load_tum_frame(tum_dir, d_names[k], c_names[k])
        depth.append(d); rgbx.append(c)
        traj.append(np.asarray(formats.nearest_pose(t_ts, t_poses, d_ts[k]), np.float32))
    h, w = depth[0].shape
    target_traj = traj[0]
    gt = [(target_traj @ np.linalg.inv(T)).astype(np.float32) for T in traj[1:]]
    return dict(frames=frames, depth=np.stack(depth), rgbx=np.stack(rgbx), trajectory=traj, gt=gt,
                K=np.asarray(TUM_K if K is None else K, np.float32), width=w, height=h)


def reconstruct_room_options(params):
    """(target, source) icp_depth_options of reconstructRoom for the given icp_params: target keepOriginalSize = projective matching,
    factor 1 (main.cpp:201-207); source (true, 1) with multi-resolution, else (false, 8) (main.cpp:287-292); maxDistance 0.1 (PointCloud.h:78)."""
    tgt = binding.depth_options(keep_original_size=params.matching == 1, downsample_factor=1)
    src = binding.depth_options(keep_original_size=True, downsample_factor=1) if params.multires else binding.depth_options(False, 8)
    return tgt, src


def reconstruct_room_params(params, K=TUM_K, width=TUM_WIDTH, height=TUM_HEIGHT):
    """The optimizer settings reconstructRoom adds on top of the chosen variant: 35 iterations, setMatchingMaxDistance(0.1), and the
    depth camera for projective matching (main.cpp:227-250).  Modifies and returns `params`."""
    params.n_iterations = 35
    params.max_distance = 0.1
    if params.matching == 1:
        K = np.asarray(K, np.float32)
        params.fx, params.fy, params.cx, params.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
        params.width, params.height = int(width), int(height)
    return params


def track(ctx, seq, params=None, with_gt=True, nonlinear=None, convergence=None, reciprocal=None, model=None, options=None, sdf=None, depth_filter=None):
    """reconstructRoom's loop on the device.  params: the variant's icp_params (metric, matching, colour ICP, weighting, multires, ...;
    ctx.params when None); reconstruct_room_params then sets what reconstructRoom sets on top of them -- 35 iterations, max distance 0.1
    and, for projective matching, the sequence's camera.  Returns (camera poses: the identity for frame 0, then currentCameraToWorld^-1
    after every frame (main.cpp:267-269,318-320), per-frame records, status).  nonlinear: True (or an IcpLmOptions) tracks with the
    non-linear optimiser -- USE_LINEAR_ICP 0 (main.cpp:26) --, False with the linear one, None keeps the context's choice.
    convergence: dict(rotation=..., translation=...[, min_iterations, patience]) stops every frame's run on a converged pose
    (Context.set_convergence_options; the records' `iterations` say where), False turns that off, None keeps the context's setting.
    reciprocal: True keeps only mutual nearest-neighbour pairs in every frame's run (Context.set_reciprocal_options), False turns that off,
    None keeps the context's setting.
    model: None tracks every frame against frame 0, as the reference does.  A dict of `binding.tsdf_options` arguments (dims, origin,
    voxel_size, truncation, ...) tracks frame-to-model instead (icp_track_depth_model): the frames are fused into a TSDF volume created
    from those options, in frame 0's camera coordinates, and every frame is aligned to a ray-cast of it -- the track survives the camera
    turning away from frame 0.  The colour frames are not used on that path unless the dict also holds color=True: the volume then gets its
    colour array and the frames are tracked with their colour frames (icp_track_depth_model_color), so the params may ask for colour ICP,
    colour weighting or the colored metric.  That path sets fix_color_index on (a copy of) the source options itself, whatever the caller
    or reconstruct_room_options chose: the model holds each pixel's own bytes, and the library refuses a source with the reference's
    shifted ones.
    options: (target, source) icp_depth_options instead of reconstruct_room_options' choice (the model path uses the source's only).
    sdf: None leaves every path above as it is.  With `model`, a dict of `binding.sdf_options` arguments (stride, n_iterations, min_valid,
    huber, stop_rotation, stop_translation; an empty dict for the defaults) tracks every frame directly against the volume instead
    (icp_track_depth_sdf): no ray-cast, no source cloud, no search, so the params, `options`, `with_gt` and the optimiser choices play no
    part and the records are icp_sdf_frame's; with color=True in `model` the colour frames are fused as well.  `sdf` without `model` is a
    ValueError.  The dict may also hold color_weight (> 0) and color_huber: every frame is then aligned with the photometric term read from
    the colour array as well (icp_track_depth_sdf_color; the records are icp_sdf_color_frame's), which holds the pose where the geometry
    leaves it free; that needs color=True in `model`, else it is a ValueError.
    model=dict(hashed=True, origin=..., voxel_size=..., ...[, block_capacity=...]) together with `sdf` tracks against a HASHED volume
    (Context.tsdf_create_hashed): no dims, no extent, blocks allocated around the surface as the frames come, so the
    trajectory need not be known beforehand.  model=dict(hashed=True, raycast=True, origin=..., ...) with sdf=None tracks frame-to-model on
    the hashed volume instead (icp_track_depth_model_hashed): every frame against a ray-cast of the blocks, with the
    params' matcher, the optimiser, convergence and reciprocal choices and `with_gt` as on the dense model path.  hashed=True without `sdf`
    and without raycast=True, or with dims, is a ValueError; so is raycast=True together with `sdf` or without hashed=True.
    model=dict(hashed=True, color=True, ...) with `sdf` gives the blocks colours (Context.tsdf_create_hashed(color=True), DESIGN.md section
    6zb): the colour frames are fused, and sdf=dict(..., color_weight=w) aligns every frame with the photometric term as on the dense
    coloured model; it goes together with keep_radius.  color=True with raycast=True is a ValueError (the geometric ray-cast loop reads no
    colours: raycast="color" is the coloured one), and so is color=True on a sequence without colour frames.
    model=dict(hashed=True, color=True, raycast="color", ...) with sdf=None tracks against the COLOURED ray-cast of the blocks
    (icp_track_depth_model_color_hashed): the colour frames are fused and the params may ask for colour ICP, colour
    weighting or the colored metric; fix_color_index is set on (a copy of) the source options, as on the dense coloured model path.
    raycast="color" without color=True, without hashed=True, with `sdf` or with keep_radius is a ValueError.
    model=dict(hashed=True, keep_radius=R, ...) with `sdf` keeps only the blocks within R metres of the camera on the device and streams
    the rest to the host and back (tsdf_local.track_depth_sdf_local): the poses and records are those of the
    unbounded run, the stored blocks are left in ctx.tsdf_store (tsdf_local.restore(ctx, ctx.tsdf_store) puts the whole model back).
    keep_radius without hashed=True, or together with raycast=True, is a ValueError; keep_radius=None, the default, changes nothing.
    depth_filter: a dict of `Context.set_depth_filter` arguments (radius, sigma_space, sigma_range) tracks with the bilateral depth filter
     set that way for this call -- every frame is aligned as filtered and fused as it came -- and puts the
    context's previous setting back; None, the default, touches nothing."""
    if depth_filter is not None:
        with binding.depth_filter_scope(ctx, depth_filter):
            return track(ctx, seq, params, with_gt, nonlinear, convergence, reciprocal, model, options, sdf)
    hashed = bool(model is not None and model.get("hashed"))
    raycast = bool(model is not None and model.get("raycast"))
    keep_radius = model.get("keep_radius") if model is not None else None
    if keep_radius is not None and not hashed:
        raise ValueError("keep_radius streams the blocks of a hashed model: pass hashed=True as well")
    if keep_radius is not None and raycast:
        raise ValueError("keep_radius streams the directly tracked hashed model (sdf=dict(...)): the ray-cast loop has no streaming")
    if raycast and not hashed:
        raise ValueError("raycast=True selects the ray-cast loop of a hashed model: pass hashed=True as well (a dense model is ray-cast as it is)")
    color_cast = model is not None and isinstance(model.get("raycast"), str) and model.get("raycast") == "color"
    if raycast and not color_cast and model.get("raycast") is not True:
        raise ValueError("raycast is True (the geometric ray-cast loop) or \"color\" (the coloured one)")
    if color_cast and not model.get("color"):
        raise ValueError("raycast=\"color\" tracks against the coloured ray-cast of a coloured hashed model: pass color=True as well")
    if raycast and sdf is not None:
        raise ValueError("raycast=True tracks against a ray-cast of the hashed model, sdf=dict(...) directly against it: pass one of them")
    if hashed:
        if sdf is None and not raycast:
            raise ValueError("a hashed model is tracked directly (sdf=dict(...)) or against its ray-cast (raycast=True in model): pass one of them")
        if model.get("dims") is not None:
            raise ValueError("a hashed model has no extent: leave dims out")
        if model.get("color") and raycast and not color_cast:
            raise ValueError("the ray-cast loop of a hashed model reads no colours: leave color out, track directly (sdf=dict(...)), or pass raycast=\"color\" for the coloured ray-cast loop")
        if model.get("color") and seq.get("rgbx") is None:
            raise ValueError("a coloured hashed model fuses the sequence's colour frames: the sequence has none (rgbx)")
    if sdf is not None and model is None:
        raise ValueError("sdf tracking needs a model: pass model=dict(dims=..., origin=..., ...) as well")
    if sdf is not None and sdf.get("color_weight", 0.0) != 0 and not model.get("color"):
        raise ValueError("sdf tracking with color_weight needs a coloured model: pass color=True in model")
    binding.select_optimizer(ctx, nonlinear)
    binding.select_convergence(ctx, convergence)
    binding.select_reciprocal(ctx, reciprocal)
    if params is not None:
        ctx.params = params
    reconstruct_room_params(ctx.params, seq["K"], seq["width"], seq["height"])
    ctx.push_params()
    cam = binding.depth_camera(seq["K"], seq["width"], seq["height"])
    tgt_o, src_o = reconstruct_room_options(ctx.params) if options is None else options
    if hashed:
        ctx.tsdf_create_hashed(color=bool(model.get("color")), **{k: v for k, v in model.items() if k not in ("hashed", "raycast", "color", "dims", "keep_radius")})
        ctx.tsdf_store = None
        rgbx = seq["rgbx"] if model.get("color") else None
        if color_cast:
            src_o = binding.depth_options(bool(src_o.keep_original_size), int(src_o.downsample_factor), float(src_o.max_distance), fix_color_index=True)
            _, recs, rc = ctx.track_depth_model_hashed(seq["depth"], cam, src_o, gt=seq["gt"] if with_gt else None, rgbx_frames=rgbx)
        elif raycast:
            _, recs, rc = ctx.track_depth_model_hashed(seq["depth"], cam, src_o, gt=seq["gt"] if with_gt else None)
        elif keep_radius is not None:
            _, recs, rc, _, ctx.tsdf_store = tsdf_local.track_depth_sdf_local(ctx, seq["depth"], cam, keep_radius, rgbx_frames=rgbx, **sdf)
        else:
            _, recs, rc = ctx.track_depth_sdf(seq["depth"], cam, rgbx_frames=rgbx, **sdf)
        poses = [np.eye(4, dtype=np.float32)] + [np.linalg.inv(r["pose"].astype(np.float64)).astype(np.float32) for r in recs]
        return poses, recs, rc
    if model is not None:
        ctx.tsdf_create(**model)
        rgbx = None
        if model.get("color"):
            rgbx = seq["rgbx"]
        if sdf is not None:
            _, recs, rc = ctx.track_depth_sdf(seq["depth"], cam, rgbx_frames=rgbx, **sdf)
            poses = [np.eye(4, dtype=np.float32)] + [np.linalg.inv(r["pose"].astype(np.float64)).astype(np.float32) for r in recs]
            return poses, recs, rc
        if model.get("color"):
            src_o = binding.depth_options(bool(src_o.keep_original_size), int(src_o.downsample_factor), float(src_o.max_distance), fix_color_index=True)
        _, recs, rc = ctx.track_depth_model(seq["depth"], cam, src_o, gt=seq["gt"] if with_gt else None, rgbx_frames=rgbx)
        poses = [np.eye(4, dtype=np.float32)] + [np.linalg.inv(r["pose"].astype(np.float64)).astype(np.float32) for r in recs]
        return poses, recs, rc
    _, recs, rc = ctx.track_depth_frames(seq["depth"], seq["rgbx"], cam, tgt_o, src_o, gt=seq["gt"] if with_gt else None)
    poses = [np.eye(4, dtype=np.float32)] + [np.linalg.inv(r["pose"].astype(np.float64)).astype(np.float32) for r in recs]
    return poses, recs, rc


def reconstruct_room(ctx, seq, params=None, out_dir=None, with_gt=True, edge_threshold=0.1, camera_scale=0.0015, nonlinear=None, convergence=None, reciprocal=None, model=None, model_mesh=None, sdf=None, densify=True, depth_filter=None, mesh_cluster=None):
    """reconstructRoom end to end: `track`, then saveRoomToFile (utils.h:179-193) for every scheduled frame k --
    joinMeshes(SimpleMesh(sensor, pose_k, edge_threshold) on the device, SimpleMesh::camera(pose_k, camera_scale), identity) with pose_k
    the camera pose `track` returned (the identity for frame 0).  With out_dir the meshes are written as mesh_<frame index>.off
    (getCurrentFrameCnt, VirtualSensor.h:142-144).  model: as `track` (frame-to-model tracking; the meshes stay per-frame depth meshes).
    model_mesh: with `model` and `out_dir`, a file name: the fused volume's zero level set (Context.tsdf_mesh, in frame 0's camera coordinates) is
    written there as a binary PLY after the last frame -- the reconstructed room as ONE mesh, with per-vertex colours when the model has them
    (color=True in `model`); None writes nothing more.  A hashed model (hashed=True in `model`) is densified over the bounding box of its
    blocks first (`densify_hashed_model`, which carries a coloured hashed model's colours: the mesh then has them), which raises when that box
    does not fit a dense volume; densify=False meshes it in place instead
    (Context.tsdf_mesh_hashed, DESIGN.md sections 6y and 6zc; with per-vertex colours when the model has them): nothing but the mesh crosses to the host, no box is built and the context keeps its hashed volume.
    densify=False with a model that is not hashed is a ValueError.  sdf: as `track` (direct SDF tracking against the model); a hashed model
    with raycast=True and no `sdf` is tracked against its ray-cast instead, as `track` says.  depth_filter: as `track` (the per-frame depth meshes are built from the raw frames).
    mesh_cluster: a cell size in metres -- the model's mesh is clustered to that resolution on the device before it crosses to the host
    (Context.tsdf_mesh / tsdf_mesh_hashed with cluster=; ctx.mesh_cluster_info() has the counts); without a mesh
    to write (model, model_mesh and out_dir) it is a ValueError; None changes nothing.  Returns (poses, records, status, the meshes -- or their paths with out_dir)."""
    if not densify and not (model is not None and model.get("hashed")):
        raise ValueError("densify=False meshes a hashed model in place: pass model=dict(hashed=True, ...)")
    if mesh_cluster is not None and not (model is not None and model_mesh is not None and out_dir is not None):
        raise ValueError("mesh_cluster needs a mesh to write: pass model, model_mesh and out_dir")
    poses, recs, rc = track(ctx, seq, params, with_gt=with_gt, nonlinear=nonlinear, convergence=convergence, reciprocal=reciprocal, model=model, sdf=sdf, depth_filter=depth_filter)
    cam = binding.depth_camera(seq["K"], seq["width"], seq["height"])
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    out = []
    for k, pose in enumerate(poses):
        depth_mesh = ctx.depth_mesh(seq["depth"][k], seq["rgbx"][k], cam, pose, edge_threshold)
        mesh = meshio.join_meshes(depth_mesh, meshio.camera_glyph(pose, camera_scale))
        if out_dir is None:
            out.append(mesh)
        else:
            path = os.path.join(out_dir, "mesh_%d.off" % seq["frames"][k])
            meshio.write_off(path, *mesh)
            out.append(path)
    if model is not None and model_mesh is not None and out_dir is not None:
        if model.get("hashed") and getattr(ctx, "tsdf_store", None) is not None:
            tsdf_local.restore(ctx, ctx.tsdf_store)     # (a streamed model: the union of the resident and the stored blocks)
        if model.get("hashed") and not densify:
            if model.get("color"):
                v, n, t, col = ctx.tsdf_mesh_hashed(colors=True, cluster=mesh_cluster)
                meshio.write_ply_mesh(os.path.join(out_dir, model_mesh), v, n, t, colors=col)
            else:
                meshio.write_ply_mesh(os.path.join(out_dir, model_mesh), *ctx.tsdf_mesh_hashed(cluster=mesh_cluster))
            return poses, recs, rc, out
        if model.get("hashed"):
            densify_hashed_model(ctx)
        if model.get("color"):
            v, n, t, col = ctx.tsdf_mesh(colors=True, cluster=mesh_cluster)
            meshio.write_ply_mesh(os.path.join(out_dir, model_mesh), v, n, t, colors=col)
        else:
            meshio.write_ply_mesh(os.path.join(out_dir, model_mesh), *ctx.tsdf_mesh(cluster=mesh_cluster))
    return poses, recs, rc, out


def densify_hashed_model(ctx):
    """Replaces the context's hashed volume by a dense one over the bounding box of its blocks, with the same contents (for
    Context.tsdf_mesh or tsdf_raycast, which need the dense box).  The dense origin is origin + lo * voxel_size, rounded once per axis.
    A coloured hashed volume becomes a dense coloured one (Context.tsdf_color_upload): `tsdf_mesh(colors=True)`, `tsdf_raycast_color` and
    `track_depth_model(..., rgbx_frames=...)` are reachable from a finished hashed coloured model by this route.
    Raises ValueError when the volume has no block or the box has more than INT32_MAX voxels."""
    colored = ctx.tsdf_has_color()
    info, coords, t, w, *col = ctx.tsdf_blocks(colors=True) if colored else ctx.tsdf_blocks()
    if len(coords) == 0:
        raise ValueError("the hashed model holds no block: nothing to densify")
    lo = coords.min(0).astype(np.int64) * 8
    dims = (coords.max(0).astype(np.int64) + 1) * 8 - lo
    if int(dims[0]) * int(dims[1]) * int(dims[2]) > 0x7FFFFFFF:
        raise ValueError("the bounding box of the hashed model's blocks, %d x %d x %d voxels, does not fit a dense volume" % tuple(dims))
    o = ctx.tsdf_hashed_options
    T, W = binding.tsdf_blocks_to_dense(coords, t, w, lo, dims)
    origin = [float(np.float32(np.float32(o.origin[a]) + np.float32(lo[a]) * np.float32(o.voxel_size))) for a in range(3)]
    ctx.tsdf_create(dims=tuple(int(d) for d in dims), origin=origin, voxel_size=o.voxel_size, truncation=o.truncation, max_weight=o.max_weight,
                    min_depth=o.min_depth, max_depth=o.max_depth, ray_step=o.ray_step)
    ctx.tsdf_upload(T, W)
    if colored:
        ctx.tsdf_color_create()
        ctx.tsdf_color_upload(*binding.tsdf_block_colors_to_dense(coords, col[0], col[1], lo, dims))


def _write_list(path, header, rows):
    with open(path, "w") as f:
        f.write("# %s\n# file: synthetic\n# timestamp filename\n" % header)
        for r in rows:
            f.write(r + "\n")


def write_synthetic_sequence(tum_dir, n_frames, width=TUM_WIDTH, height=TUM_HEIGHT, K=None, seed=0x7A11, hole_frac=0.05, dt=1.0 / 30):
    """Writes frames 0 .. n_frames-1 of `synth.camera_pose` in the TUM RGB-D layout: 16-bit depth PNGs (metres x 5000, 0 = hole),
    RGB PNGs, depth.txt / rgb.txt and groundtruth.txt ('t tx ty tz qx qy qz qw' of the camera-to-world pose, which
    read_tum_trajectory stores inverted).  Returns dict(depth=(n, h, w) float32 metres as written, with MINF holes, poses=camera-to-world)."""
    from PIL import Image
    K = np.asarray(TUM_K if K is None else K, np.float64)
    os.makedirs(os.path.join(tum_dir, "depth"), exist_ok=True)
    os.makedirs(os.path.join(tum_dir, "rgb"), exist_ok=True)
    d_rows, c_rows, g_rows, depths, poses = [], [], [], [], []
    for k in range(n_frames):
        T = synth.camera_pose(k, seed)
        pts, _, rgba = synth.depth_frame(T, K, width, height, seed + k, hole_frac)
        z = pts[:, 2].astype(np.float64)
        raw = np.where(np.isfinite(z), np.round(z * 5000.0), 0.0)
        raw = np.clip(raw, 0, 65535).astype(np.uint16).reshape(height, width)
        ts = 1000.0 + k * dt
        dn, cn = "depth/%.6f.png" % ts, "rgb/%.6f.png" % ts
        Image.fromarray(raw).save(os.path.join(tum_dir, dn))
        Image.fromarray(rgba[:, :3].reshape(height, width, 3)).save(os.path.join(tum_dir, cn))
        d_rows.append("%.6f %s" % (ts, dn)); c_rows.append("%.6f %s" % (ts, cn))
        q = _rot_to_quat(T[:3, :3])
        g_rows.append("%.6f %.9f %.9f %.9f %.9f %.9f %.9f %.9f" % ((ts,) + tuple(T[:3, 3]) + tuple(q)))
        depths.append(formats.decode_tum_depth(raw)); poses.append(T)
    _write_list(os.path.join(tum_dir, "depth.txt"), "depth maps", d_rows)
    _write_list(os.path.join(tum_dir, "rgb.txt"), "color images", c_rows)
    with open(os.path.join(tum_dir, "groundtruth.txt"), "w") as f:
        f.write("# ground truth trajectory\n# file: synthetic\n# timestamp tx ty tz qx qy qz qw\n")
        for r in g_rows:
            f.write(r + "\n")
    return dict(depth=np.stack(depths), poses=poses)


def _rot_to_quat(R):
    """(qx, qy, qz, qw) of a rotation matrix, qw >= 0."""
    R = np.asarray(R, np.float64)
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    x = np.copysign(x, R[2, 1] - R[1, 2]); y = np.copysign(y, R[0, 2] - R[2, 0]); z = np.copysign(z, R[1, 0] - R[0, 1])
    q = np.array([x, y, z, w])
    return q / np.linalg.norm(q)
