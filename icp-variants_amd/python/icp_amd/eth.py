"""Host side of the ETH benchmark runner (reference: ETHDataLoader.h:11-107 and alignETH, main.cpp:343-514).

Pure host logic over `formats.py` plus the two device steps in front of the loop (k = 5 normals, `icp_estimate_normals`):
  rows      = load_rows(eth_dir, csv_name)                 # CSVReader + ETHDataLoader ctor
  src, tgt  = load_scans(eth_dir, csv_name, row)           # loadPCDFile<PointXYZ> x 2          (ETHDataLoader.h:66-98)
  pair      = prepare_pair(ctx, src, tgt, row["pose"])     # PointCloud(pcl) normals k = 5       (PointCloud.h:41-76)
                                                           # + pose_scaling 0.1 and change_pose  (main.cpp:420-429, PointCloud.h:277-282)
  pose      = align(ctx, pair, nonlinear=...)              # estimatePose (main.cpp:457), USE_LINEAR_ICP 0 -> nonlinear=True
`pair` has the keys of `synth.eth_like_pair` (src_pts, src_nrm, tgt_pts, tgt_nrm, src_unperturbed, gt), so the bench and the
tests drive real files and synthetic scans through the same code.
Layout on disk, as the reference expects it under Data/: <eth_dir>/<name>_global.csv and <eth_dir>/<name>/<scan>.pcd.
PCL is absent here: the normals are this repo's exact k-NN + fp64 PCA (parity with pcl::NormalEstimation unpinned).
"""
import functools
import os
import numpy as np

from . import formats


def dataset_name(csv_name):
    """ETHDataLoader.h:20-23: three find_last_not_of / erase calls on the file name (character SETS, not suffixes)."""
    name = csv_name.rstrip(".csv")
    name = name.rstrip("_local")
    name = name.rstrip("_global")
    return name


def load_rows(eth_dir, csv_name):
    return formats.read_pose_csv(os.path.join(eth_dir, csv_name))


def load_scans(eth_dir, csv_name, row):
    base = os.path.join(eth_dir, dataset_name(csv_name))
    src = formats.read_pcd(os.path.join(base, row["source"]))
    tgt = formats.read_pcd(os.path.join(base, row["target"]))
    return src, tgt


def change_pose(pose, pts, nrm):
    """PointCloud::change_pose (PointCloud.h:277-282): p <- (T [p,1]).head(3), n <- (T [n,0]).head(3), fp32."""
    T = np.asarray(pose, np.float32)
    R, t = T[:3, :3], T[:3, 3]
    return (pts @ R.T + t).astype(np.float32), (nrm @ R.T).astype(np.float32)


def prepare_pair(ctx, src_xyz, tgt_xyz, benchmark_pose, pose_scaling=0.1, k=5):
    """What alignETH does between getItem and estimatePose (main.cpp:413-429), with the normals on the device."""
    src_xyz = np.ascontiguousarray(src_xyz, np.float32); tgt_xyz = np.ascontiguousarray(tgt_xyz, np.float32)
    src_nrm, _ = ctx.estimate_normals(src_xyz, k=k)                     # viewpoint (0,0,0): PCL's default
    tgt_nrm, _ = ctx.estimate_normals(tgt_xyz, k=k)
    S = formats.scaled_initial_pose(benchmark_pose, pose_scaling)
    moved, moved_nrm = change_pose(S, src_xyz, src_nrm)
    rgba = np.tile(np.array([255, 255, 255, 1], np.uint8), (len(src_xyz), 1))        # PointCloud.h:73
    return dict(src_pts=moved, src_nrm=moved_nrm, src_rgba=rgba, src_unperturbed=src_xyz,
                tgt_pts=tgt_xyz, tgt_nrm=tgt_nrm, tgt_rgba=np.tile(np.array([255, 255, 255, 1], np.uint8), (len(tgt_xyz), 1)),
                gt=np.linalg.inv(np.asarray(S, np.float64)), initial=S)


def align(ctx, pair, nonlinear=None, check=True, convergence=None, initial="identity", reciprocal=None, vgicp=None, **global_options):
    """estimatePose of alignETH (main.cpp:457) on a prepared pair with the context's params: the optimiser the reference's
    USE_LINEAR_ICP picks (main.cpp:26) -- nonlinear True (or an IcpLmOptions): CeresICPOptimizer, False: LinearICPOptimizer, None: the
    context's current choice.  convergence: dict(rotation=..., translation=...[, min_iterations, patience]) stops the run on a converged
    pose (Context.set_convergence_options), False turns that off, None keeps the context's setting.
    reciprocal: True keeps only mutual nearest-neighbour pairs (Context.set_reciprocal_options), False turns that off, None keeps the
    context's setting.
    initial: "identity" starts the run from the identity, as the reference does; "global" starts it from the best pose of the global
    registration (Context.register_global with **global_options: FPFH features, feature matching, RANSAC), for pairs whose initial pose
    is not roughly known.  (globalreg.align refines several RANSAC poses at once instead, where multi-start ICP is available.)
    vgicp: None aligns through icp_run, every path as it was; dict(voxel_size=..., ...) (the fields of binding.vgicp_options) aligns the
    source to a voxel grid of the target instead (Context.vgicp_align: voxelized GICP with the context's GICP options, no index walk, no
    search) and returns (4x4 pose, [the alignment's record], status); with check, a failed alignment raises.
    Returns (4x4 pose, per-iteration records, status)."""
    from . import binding
    if initial not in ("identity", "global"):
        raise ValueError("initial must be 'identity' or 'global'")
    if initial == "identity" and global_options:
        raise TypeError("global registration options need initial='global'")
    binding.select_optimizer(ctx, nonlinear)
    binding.select_convergence(ctx, convergence)
    binding.select_reciprocal(ctx, reciprocal)
    ctx.push_params()
    ctx.set_target(pair["tgt_pts"], pair["tgt_nrm"], pair.get("tgt_rgba"))
    ctx.set_source(pair["src_pts"], pair["src_nrm"], pair.get("src_rgba"))
    start = np.eye(4, dtype=np.float32)
    if initial == "global":
        ctx.set_global_options(**global_options)
        start = ctx.register_global()[0][0]
    if vgicp is not None:
        pose, rec, rc = ctx.vgicp_align(start, options=binding.vgicp_options(**vgicp))
        if check and rc != binding.ICP_OK:
            raise binding.IcpError(rc, ctx.lib.icp_last_error(ctx.h).decode())
        return pose, [rec], rc
    return ctx.run(start, check=check)


def track_map(ctx, scans, start_pose, voxel_size=0.25, extent=None, margin=2.0, hashed=False, capacity=1 << 16, keep_radius=None, **vgicp_options):
    """Scan-to-map tracking of a laser sequence (Context.track_scans_vmap): `scans` is a list of (xyz, normals) in the sensor frame
    (normals None where the context's GICP options compute them, covariance_k > 0), `start_pose` the 4x4 pose of scan 0.  A voxel map of
    `voxel_size` metres is created over `extent` = (lo, dims) in cells (binding.voxel_map_extent); extent None: the bounds of scan 0's
    finite points at the start pose, grown by `margin` metres on every side.  Scan 0 is fused at the start pose; every later scan is
    aligned to the map built so far (voxelized GICP with **vgicp_options, the fields of binding.vgicp_options) and fused at the pose
    found; a scan that fails is skipped and carries the pose.  Returns (poses: one 4x4 per scan, records: one per scan after the first,
    status: the first per-scan error, or 0).  The map stays in the context (Context.voxel_map).
    hashed=True: the map is a hash table of cells of at least `capacity` slots that grows as it fills (Context.voxel_map_create_hashed):
    it has no extent, so a trajectory cannot leave it; `extent` and `margin` are not used, and passing an extent is a ValueError.  The
    map is then read with Context.voxel_map_hashed.
    keep_radius (metres, either storage): the map is kept LOCAL -- after every scan is fused, the cells further than keep_radius from
    the scan's position are forgotten (Context.voxel_map_prune), so the map's size follows the sensor's range and not the length of the
    trajectory; a fourth value is then returned, the prune info of every scan."""
    from . import binding
    start = np.asarray(start_pose, np.float32)

    def run():
        out = ctx.track_scans_vmap(scans, start, keep_radius=keep_radius, options=binding.vgicp_options(voxel_size=voxel_size, **vgicp_options))
        return ([start.copy()] + [r["pose"] for r in out[1]], out[1]) + tuple(out[2:])
    if hashed:
        if extent is not None:
            raise ValueError("a hashed map has no extent")
        ctx.voxel_map_create_hashed(voxel_size, capacity)
        return run()
    if extent is None:
        p0 = np.asarray(scans[0][0], np.float64)
        p0 = p0[np.isfinite(p0).all(1)]
        if len(p0) == 0:
            raise ValueError("scan 0 has no finite point to take the extent from")
        w = p0 @ start[:3, :3].astype(np.float64).T + start[:3, 3].astype(np.float64)
        extent = binding.voxel_map_extent(w.min(0) - margin, w.max(0) + margin, voxel_size)
    ctx.voxel_map_create(voxel_size, *extent)
    return run()


def _carving(run):
    """Gives a runner the keyword `carve`: None (the default) calls it as it is; dict(distance=..., min_range=...) -- the arguments of
    Context.set_tsdf_carve -- sets the context's carve options for the call and puts the previous setting back behind it, as
    tum.track(..., depth_filter=...) does for the depth filter.  The runner's own signature stays what it was."""
    @functools.wraps(run)
    def with_carve(ctx, *args, carve=None, **kw):
        if carve is None:
            return run(ctx, *args, **kw)
        from . import binding
        with binding.tsdf_carve_scope(ctx, carve):
            return run(ctx, *args, **kw)
    return with_carve


def _colouring(coloured):
    """Gives a runner the keyword `colors`: None (the default) calls it as it is; one rgba (n, 4) uint8 array per scan calls
    `coloured(ctx, colors, ...)` with the runner's own arguments -- the same run on a volume with colours, every scan fused with its
    colours (Context.tsdf_integrate_cloud(color=True), Context.track_scans_sdf(colors=...)).  The runner's own
    signature stays what it was."""
    def give(run):
        @functools.wraps(run)
        def with_colors(ctx, *args, colors=None, **kw):
            if colors is None:
                return run(ctx, *args, **kw)
            return coloured(ctx, colors, *args, **kw)
        return with_colors
    return give


def _scan_colors(scans, colors):
    if len(colors) != len(scans):
        raise ValueError("one colour array per scan")
    return [np.ascontiguousarray(c, np.uint8) for c in colors]


def _fuse_scans(ctx, colors, scans, poses, voxel_size=0.05, truncation=None, origin=(0.0, 0.0, 0.0), max_range=30.0, block_capacity=1 << 14, hashed=True, dims=None):
    """fuse_scans behind its docstring; colors: None, or one rgba array per scan."""
    if len(scans) != len(poses):
        raise ValueError("one pose per scan")
    cols = None if colors is None else _scan_colors(scans, colors)
    _tsdf_volume(ctx, voxel_size, truncation, origin, max_range, block_capacity, hashed, dims, color=cols is not None)
    infos = []
    for k, (s, T) in enumerate(zip(scans, poses)):
        xyz = s[0] if isinstance(s, (tuple, list)) else s
        if cols is None:
            ctx.set_source(np.ascontiguousarray(xyz, np.float32))
            infos.append(ctx.tsdf_integrate_cloud("source", pose=np.asarray(T, np.float32)))
        else:
            ctx.set_source(np.ascontiguousarray(xyz, np.float32), None, cols[k])
            infos.append(ctx.tsdf_integrate_cloud("source", pose=np.asarray(T, np.float32), color=True))
    return infos


@_carving
@_colouring(_fuse_scans)
def fuse_scans(ctx, scans, poses, voxel_size=0.05, truncation=None, origin=(0.0, 0.0, 0.0), max_range=30.0, block_capacity=1 << 14, hashed=True, dims=None):
    """Laser scans fused into a TSDF volume (Context.tsdf_integrate_cloud): `scans` as track_map takes them (a list
    of (xyz, normals) in the sensor frame; a bare xyz array will do, the normals are not used), `poses` one 4x4 sensor -> world per scan.
    A volume of `voxel_size` metres is created -- hashed by default (Context.tsdf_create_hashed with `block_capacity`; it has no extent),
    or, with hashed=False, the dense box of `dims` voxels whose voxel (0, 0, 0) is centred on `origin` -- with `truncation` (None: 4
    voxels) and max_depth = `max_range`: a return beyond it is not fused.  Every scan becomes the resident source and is integrated from
    the sensor's position, one observation per scan.  Nothing is carved in front of the surfaces unless carving is on: carve=dict(distance=...,
    min_range=...) (keyword only; the arguments of Context.set_tsdf_carve) fuses with free space carved and puts the
    context's previous setting back; None changes nothing.  colors (keyword only): one rgba (n, 4) uint8 array per scan -- the volume is
    created with colours and every scan is fused with its colours (each info dict gains n_colored); None changes
    nothing.  Returns the info dict of every scan; the volume stays in the context
    (Context.tsdf_sample, Context.tsdf_mesh_hashed, Context.tsdf_blocks)."""
    return _fuse_scans(ctx, None, scans, poses, voxel_size, truncation, origin, max_range, block_capacity, hashed, dims)


def _tsdf_volume(ctx, voxel_size, truncation, origin, max_range, block_capacity, hashed, dims, color=False):
    """The volume fuse_scans and track_tsdf create: hashed, or the dense box of `dims` voxels."""
    if not hashed and dims is None:
        raise ValueError("a dense volume needs dims")
    if hashed and dims is not None:
        raise ValueError("a hashed volume has no extent")
    opts = dict(origin=tuple(float(x) for x in origin), voxel_size=float(voxel_size), truncation=4.0 * float(voxel_size) if truncation is None else float(truncation),
                max_depth=float(max_range))
    colour = dict(color=True) if color else {}
    if hashed:
        ctx.tsdf_create_hashed(block_capacity=block_capacity, **colour, **opts)
    else:
        ctx.tsdf_create(dims=dims, **colour, **opts)


def _track_tsdf(ctx, colors, scans, start_pose, voxel_size=0.05, truncation=None, origin=(0.0, 0.0, 0.0), max_range=30.0, block_capacity=1 << 14, hashed=True, dims=None,
                **sdf_options):
    """track_tsdf behind its docstring; colors: None, or one rgba array per scan."""
    if float(sdf_options.get("color_weight", 0.0)) > 0.0 and colors is None:
        raise ValueError("color_weight > 0 needs colors: one rgba array per scan")
    cols = None if colors is None else _scan_colors(scans, colors)
    _tsdf_volume(ctx, voxel_size, truncation, origin, max_range, block_capacity, hashed, dims, color=cols is not None)
    if cols is None:
        return ctx.track_scans_sdf(scans, np.asarray(start_pose, np.float32), **sdf_options)
    return ctx.track_scans_sdf(scans, np.asarray(start_pose, np.float32), colors=cols, **sdf_options)


@_carving
@_colouring(_track_tsdf)
def track_tsdf(ctx, scans, start_pose, voxel_size=0.05, truncation=None, origin=(0.0, 0.0, 0.0), max_range=30.0, block_capacity=1 << 14, hashed=True, dims=None,
               **sdf_options):
    """Tracking of a laser sequence against the TSDF volume the scans are fused into (Context.track_scans_sdf):
    one model, no voxel map beside it, every scan uploaded once.  `scans` as fuse_scans takes them, `start_pose` the 4x4 pose of scan 0;
    the volume is created as fuse_scans creates it.  Scan 0 is fused at the start pose; every later scan is aligned to the volume built
    so far (direct SDF alignment with **sdf_options, the fields of binding.sdf_options) and fused at the pose found; a scan that fails is
    skipped and carries the pose.  Unless carving is on (carve=dict(distance=..., min_range=...) as fuse_scans takes it: set for the call, the
    previous setting put back; None changes nothing) nothing is carved in front of the surfaces, so the field exists only within `truncation` of them:
    that band is the basin of convergence, and the part of the motion between two scans that is normal to the surfaces has to stay
    inside it (the default is 4 voxels; a faster sensor needs a wider truncation or coarser voxels).  Returns (poses: one 4x4 per scan, records:
    one per scan after the first, infos: the fuse info of every scan, status: the first per-scan error, or 0).  colors (keyword only): one
    rgba (n, 4) uint8 array per scan -- the volume is created with colours, every scan goes up with its colours and every fuse is the
    coloured one (Context.track_scans_sdf(colors=...)); poses, records and infos are what they are without, and a
    fifth value is returned, n_colored of every scan; None changes nothing.  color_weight, color_huber (among **sdf_options): with colors,
    a positive weight aligns every scan with the photometric term as well (Context.track_scans_sdf(colors=..., color_weight=...), DESIGN.md
    section 6zj) and the records are the colour records; without colors it raises ValueError.  The volume stays in the
    context (Context.tsdf_sample, Context.tsdf_mesh_hashed, Context.tsdf_blocks)."""
    return _track_tsdf(ctx, None, scans, start_pose, voxel_size, truncation, origin, max_range, block_capacity, hashed, dims, **sdf_options)


def _reconstruct(ctx, colors, scans, start_pose, tsdf_voxel_size=0.05, truncation=None, origin=(0.0, 0.0, 0.0), max_range=30.0, block_capacity=1 << 14, min_weight=0.0,
                 mesh_path=None, tracker="map", mesh_cluster=None, **track_map_options):
    """reconstruct behind its docstring; colors: None, or one rgba array per scan."""
    from . import meshio
    if tracker not in ("map", "sdf"):
        raise ValueError("tracker must be 'map' or 'sdf'")
    if mesh_cluster is not None and mesh_path is None:
        raise ValueError("mesh_cluster needs a mesh to write: pass mesh_path")
    if float(track_map_options.get("color_weight", 0.0)) > 0.0:
        if tracker != "sdf":
            raise ValueError("color_weight > 0 needs tracker='sdf' (the voxel-map tracker has no photometric term)")
        if colors is None:
            raise ValueError("color_weight > 0 needs colors: one rgba array per scan")
    coloured = {} if colors is None else dict(colors=colors)
    if tracker == "sdf":
        poses, records, _, status = track_tsdf(ctx, scans, start_pose, voxel_size=tsdf_voxel_size, truncation=truncation, origin=origin, max_range=max_range,
                                               block_capacity=block_capacity, **coloured, **track_map_options)[:4]
    else:
        if "keep_radius" in track_map_options and track_map_options["keep_radius"] is not None:
            raise ValueError("reconstruct tracks against the whole map (keep_radius is not supported)")
        poses, records, status = track_map(ctx, scans, start_pose, **track_map_options)
        fuse_scans(ctx, scans, poses, voxel_size=tsdf_voxel_size, truncation=truncation, origin=origin, max_range=max_range, block_capacity=block_capacity, **coloured)
    if colors is None:
        mesh = ctx.tsdf_mesh_hashed(min_weight=min_weight, cluster=mesh_cluster)
        if mesh_path is not None:
            meshio.write_ply_mesh(mesh_path, *mesh)
        return poses, records, status, mesh
    v, n, t, c = ctx.tsdf_mesh_hashed(min_weight=min_weight, colors=True, cluster=mesh_cluster)
    if mesh_path is not None:
        meshio.write_ply_mesh(mesh_path, v, n, t, colors=c)
    return poses, records, status, (v, n, t, c)


@_carving
@_colouring(_reconstruct)
def reconstruct(ctx, scans, start_pose, tsdf_voxel_size=0.05, truncation=None, origin=(0.0, 0.0, 0.0), max_range=30.0, block_capacity=1 << 14, min_weight=0.0,
                mesh_path=None, tracker="map", mesh_cluster=None, **track_map_options):
    """A surface from a laser sequence, the laser counterpart of tum.reconstruct_room: the scans tracked against the voxel map
    (`track_map` with **track_map_options; its voxel_size is the MAP's), fused at the tracked poses into a hashed TSDF volume of
    `tsdf_voxel_size` (`fuse_scans`), the zero level set extracted on the device (Context.tsdf_mesh_hashed with `min_weight`) and, with
    mesh_path, written as a PLY (meshio.write_ply_mesh).  Returns (poses, records, status, (vertices, normals, triangles)).
    tracker="sdf": the scans are tracked against the TSDF volume itself (`track_tsdf`; **track_map_options are then the fields of
    binding.sdf_options) and that same volume is meshed: one model, one upload of every scan, no second fuse.  carve: as fuse_scans
    takes it -- the fuses of either tracker carve free space for the call; None changes nothing.  colors (keyword only): one rgba (n, 4)
    uint8 array per scan -- the model is fused with the scans' colours, meshed with
    Context.tsdf_mesh_hashed(colors=True), written with meshio.write_ply_mesh(..., colors=...), and the mesh returned is (vertices,
    normals, triangles, colours (V, 4) uint8: alpha 255 on a coloured vertex); None changes nothing.  color_weight (among the options):
    with tracker="sdf" and colors, the photometric tracker of track_tsdf; with tracker="map" or without colors it raises ValueError.
    mesh_cluster: a cell size in metres -- the mesh is clustered to that resolution on the device before it crosses to the host
    (Context.tsdf_mesh_hashed with cluster=; ctx.mesh_cluster_info() has the counts), returned and written that
    way; without mesh_path it is a ValueError; None changes nothing."""
    return _reconstruct(ctx, None, scans, start_pose, tsdf_voxel_size, truncation, origin, max_range, block_capacity, min_weight, mesh_path, tracker, mesh_cluster,
                        **track_map_options)


def write_synthetic_dataset(eth_dir, csv_name, pairs, binary=True):
    """Writes synthetic scans in the reference's on-disk layout (used by the tests and for rehearsing --eth-dir offline):
    `pairs` = list of dicts with src_unperturbed, tgt_pts and a benchmark `pose` (unscaled perturbation)."""
    base = os.path.join(eth_dir, dataset_name(csv_name))
    os.makedirs(base, exist_ok=True)
    rows = []
    for i, p in enumerate(pairs):
        s, t = "Hokuyo_%d_src.pcd" % i, "Hokuyo_%d_tgt.pcd" % i
        formats.write_pcd(os.path.join(base, s), p["src_unperturbed"], binary=binary)
        formats.write_pcd(os.path.join(base, t), p["tgt_pts"], binary=binary)
        rows.append(dict(id=str(i), source=s, target=t, pose=p["pose"]))
    formats.write_pose_csv(os.path.join(eth_dir, csv_name), rows)
    return rows
