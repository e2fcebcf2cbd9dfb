"""ctypes binding of the C ABI in include/icp_hip.h (libicp_hip.so) plus a thin optimizer facade.

This is harness code for tests/ and bench.py; the product is the shared library.  It fails loudly
(ImportError / IcpError) when the HIP library is missing or no GPU is usable -- there is no CPU path.

`LinearICPOptimizer` keeps the setter names of the reference's ICPOptimizer (ICPOptimizer.h:41-95)
so the parity tests read like the reference's drivers (main.cpp:43-181, 343-514).
"""
import ctypes as C
import functools
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.abspath(os.path.join(_HERE, "..", ".."))            # icp-variants_amd/
LIB_PATH = os.environ.get("ICP_HIP_LIB") or os.path.join(PKG_ROOT, "lib", "libicp_hip.so")     # ICP_HIP_LIB: development A/B builds

MATCH_DTYPE = np.dtype([("idx", np.int32), ("weight", np.float32)])

ICP_OK = 0
ERR_NAMES = {1: "INVALID_ARG", 2: "HIP", 3: "NO_TARGET", 4: "NO_SOURCE", 5: "NO_CAMERA", 6: "TARGET_SIZE",
             7: "COLOR_MISMATCH", 8: "NO_CORRESPONDENCES", 9: "NO_DEVICE", 10: "COMM"}
ERR_NO_CORRESPONDENCES = 8
ERR_NO_SOURCE = 4
ERR_NO_TARGET = 3


class IcpError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("icp_hip error %d (%s): %s" % (code, ERR_NAMES.get(code, "?"), msg))
        self.code = code


class IcpParams(C.Structure):
    _fields_ = [("metric", C.c_int32), ("matching", C.c_int32), ("weighting", C.c_int32), ("rejection", C.c_int32),
                ("color_icp", C.c_int32), ("multires", C.c_int32), ("n_iterations", C.c_int32), ("max_distance", C.c_float),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("width", C.c_int32), ("height", C.c_int32), ("knn_backend", C.c_int32),
                ("selection", C.c_int32), ("selection_proba", C.c_float), ("selection_seed", C.c_uint32),
                ("knn_incremental", C.c_int32), ("record_rmse", C.c_int32)]


class IcpIterStats(C.Structure):
    _fields_ = [("n_src", C.c_int32), ("n_valid", C.c_int32), ("pose", C.c_float * 16), ("rmse", C.c_float), ("benchmark_error", C.c_float),
                ("status", C.c_int32)]


class IcpStartResult(C.Structure):
    _fields_ = [("pose", C.c_float * 16), ("status", C.c_int32), ("n_inliers", C.c_int32), ("fitness", C.c_float), ("inlier_rmse", C.c_float)]


class IcpTiming(C.Structure):
    _fields_ = [("match_ms", C.c_double), ("weight_reject_build_ms", C.c_double), ("solve_ms", C.c_double),
                ("total_ms", C.c_double), ("iterations", C.c_int32), ("sampled_iterations", C.c_int32)]


class IcpPair(C.Structure):
    _fields_ = [("src_xyz", C.c_void_p), ("src_normals", C.c_void_p), ("src_rgba", C.c_void_p), ("n_src", C.c_int32),
                ("tgt_xyz", C.c_void_p), ("tgt_normals", C.c_void_p), ("tgt_rgba", C.c_void_p), ("n_tgt", C.c_int32),
                ("initial_pose", C.c_float * 16)]


class IcpDepthCamera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("width", C.c_int32), ("height", C.c_int32),
                ("extrinsics", C.c_float * 16)]


class IcpDepthOptions(C.Structure):
    _fields_ = [("keep_original_size", C.c_int32), ("downsample_factor", C.c_int32), ("max_distance", C.c_float), ("fix_color_index", C.c_int32)]


class IcpTrackFrame(C.Structure):
    _fields_ = [("n_src", C.c_int32), ("iterations", C.c_int32), ("status", C.c_int32), ("initial_rmse", C.c_float), ("final_rmse", C.c_float),
                ("pose", C.c_float * 16)]


class IcpTsdfOptions(C.Structure):
    _fields_ = [("dims", C.c_int32 * 3), ("origin", C.c_float * 3), ("voxel_size", C.c_float), ("truncation", C.c_float), ("max_weight", C.c_float),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("ray_step", C.c_float)]


def tsdf_options(dims=None, origin=None, **kw):
    """icp_tsdf_options: icp_tsdf_options_default (voxel 0.05, truncation 0.25, max weight 64, depth range 0.3 .. 8, ray step truncation / 2)
    with dims (nx, ny, nz), origin (the centre of voxel (0, 0, 0)) and any other field overridden by name."""
    o = IcpTsdfOptions()
    rc = load_library().icp_tsdf_options_default(C.byref(o))
    if rc != ICP_OK:
        raise IcpError(rc, "icp_tsdf_options_default")
    if dims is not None:
        o.dims[:] = [int(d) for d in dims]
    if origin is not None:
        o.origin[:] = [float(x) for x in origin]
    for k, v in kw.items():
        if k in ("dims", "origin") or not any(k == f[0] for f in IcpTsdfOptions._fields_):
            raise TypeError("icp_tsdf_options has no field %r" % k)
        setattr(o, k, v)
    return o


class IcpTsdfHashedInfo(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("capacity", C.c_int32), ("n_grown", C.c_int32), ("n_unplaced", C.c_int32), ("n_out_of_range", C.c_int64)]


class IcpTsdfCloudInfo(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_rays", C.c_int32), ("n_updated", C.c_int32), ("n_blocks", C.c_int32), ("n_samples", C.c_int64),
                ("n_outside", C.c_int64)]


class IcpTsdfCarveOptions(C.Structure):
    _fields_ = [("distance", C.c_float), ("min_range", C.c_float)]


class IcpTsdfCarveInfo(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("reserved", C.c_int32), ("n_carved", C.c_int64), ("n_carved_total", C.c_int64)]


class IcpTsdfStreamInfo(C.Structure):
    _fields_ = [("n_evicted", C.c_int32), ("n_blocks", C.c_int32), ("n_moved", C.c_int32), ("capacity", C.c_int32), ("n_held", C.c_int32),
                ("n_inserted", C.c_int32), ("n_present", C.c_int32), ("n_grown", C.c_int32)]


def tsdf_view_reach(cam, options):
    """The farthest a block that a frame of `cam` can touch, update or sample has its centre from the camera, with a block diagonal of
    slack: (max_depth + truncation) * sqrt(1 + a_max^2 + b_max^2) + 8 * voxel_size * sqrt(3), with
    a_max = max(|0 - cx|, |width - 1 - cx|) / fx and b_max likewise with cy, fy and the height.  `options`: an IcpTsdfOptions, or a dict of
    `tsdf_options`' arguments.  Infinite when max_depth is.  A coloured hashed volume has the same reach: its
    colour is read and written only in cells and voxels the geometry touches."""
    o = options if isinstance(options, IcpTsdfOptions) else tsdf_options(**{k: v for k, v in dict(options).items() if k != "dims"})
    a = max(abs(0.0 - cam.cx), abs(cam.width - 1.0 - cam.cx)) / abs(cam.fx)
    b = max(abs(0.0 - cam.cy), abs(cam.height - 1.0 - cam.cy)) / abs(cam.fy)
    return (float(o.max_depth) + float(o.truncation)) * float(np.sqrt(1.0 + a * a + b * b)) + 8.0 * float(o.voxel_size) * float(np.sqrt(3.0))


def tsdf_blocks_to_dense(coords, tsdf, weight, lo, dims):
    """The blocks of a hashed volume (`Context.tsdf_blocks`) as the two dense arrays (nz, ny, nx) `Context.tsdf_upload` takes, on the host:
    dense voxel (0, 0, 0) is global voxel `lo` (three integers), so the dense volume's origin is origin + lo * voxel_size; voxels no block
    covers are (0, 0), unobserved, and what lies outside `dims` = (nx, ny, nz) is dropped."""
    lo = np.asarray(lo, np.int64).reshape(3); nx, ny, nz = (int(d) for d in dims)
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    tsdf = np.asarray(tsdf, np.float32).reshape(-1, 8, 8, 8); weight = np.asarray(weight, np.float32).reshape(-1, 8, 8, 8)
    if not (len(coords) == len(tsdf) == len(weight)):
        raise ValueError("coords (B, 3), tsdf and weight (B, 8, 8, 8) must agree in B")
    T = np.zeros((nz, ny, nx), np.float32); W = np.zeros((nz, ny, nx), np.float32)
    for b, t, w in zip(coords, tsdf, weight):
        x0, y0, z0 = (int(v) for v in b * 8 - lo)
        xs, ys, zs = (slice(max(0, -a), min(8, n - a)) for a, n in ((x0, nx), (y0, ny), (z0, nz)))
        if xs.start >= xs.stop or ys.start >= ys.stop or zs.start >= zs.stop:
            continue
        T[z0 + zs.start:z0 + zs.stop, y0 + ys.start:y0 + ys.stop, x0 + xs.start:x0 + xs.stop] = t[zs, ys, xs]
        W[z0 + zs.start:z0 + zs.stop, y0 + ys.start:y0 + ys.stop, x0 + xs.start:x0 + xs.stop] = w[zs, ys, xs]
    return T, W


def tsdf_block_colors_to_dense(coords, rgb, cweight, lo, dims):
    """The colours of a coloured hashed volume's blocks (`Context.tsdf_blocks(colors=True)`) as the two dense arrays `Context.tsdf_color_upload`
    takes, rgb (nz, ny, nx, 3) and weight (nz, ny, nx), by `tsdf_blocks_to_dense`'s rule: dense voxel (0, 0, 0) is global voxel `lo`, voxels
    no block covers are (0, 0, 0, 0), uncoloured, and what lies outside `dims` = (nx, ny, nz) is dropped."""
    lo = np.asarray(lo, np.int64).reshape(3); nx, ny, nz = (int(d) for d in dims)
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    rgb = np.asarray(rgb, np.float32).reshape(-1, 8, 8, 8, 3); cweight = np.asarray(cweight, np.float32).reshape(-1, 8, 8, 8)
    if not (len(coords) == len(rgb) == len(cweight)):
        raise ValueError("coords (B, 3), rgb (B, 8, 8, 8, 3) and cweight (B, 8, 8, 8) must agree in B")
    Cd = np.zeros((nz, ny, nx, 3), np.float32); W = np.zeros((nz, ny, nx), np.float32)
    for b, c, w in zip(coords, rgb, cweight):
        x0, y0, z0 = (int(v) for v in b * 8 - lo)
        xs, ys, zs = (slice(max(0, -a), min(8, n - a)) for a, n in ((x0, nx), (y0, ny), (z0, nz)))
        if xs.start >= xs.stop or ys.start >= ys.stop or zs.start >= zs.stop:
            continue
        Cd[z0 + zs.start:z0 + zs.stop, y0 + ys.start:y0 + ys.stop, x0 + xs.start:x0 + xs.stop] = c[zs, ys, xs]
        W[z0 + zs.start:z0 + zs.stop, y0 + ys.start:y0 + ys.stop, x0 + xs.start:x0 + xs.stop] = w[zs, ys, xs]
    return Cd, W


class IcpSdfOptions(C.Structure):
    _fields_ = [("stride", C.c_int32), ("n_iterations", C.c_int32), ("min_valid", C.c_int32), ("huber", C.c_float), ("stop_rotation", C.c_float),
                ("stop_translation", C.c_float)]


class IcpSdfIter(C.Structure):
    _fields_ = [("n_valid", C.c_int32), ("status", C.c_int32), ("cost", C.c_double), ("pose", C.c_float * 16)]


class IcpSdfFrame(C.Structure):
    _fields_ = [("n_depth", C.c_int32), ("n_valid_first", C.c_int32), ("n_valid_last", C.c_int32), ("iterations", C.c_int32), ("status", C.c_int32),
                ("cost_first", C.c_double), ("cost_last", C.c_double), ("pose", C.c_float * 16)]


def sdf_options(**kw):
    """icp_sdf_options: icp_sdf_options_default (stride 1, 20 iterations, min_valid 64, huber off, stops 1e-5 rad / 1e-5 m) with any field
    overridden by name."""
    o = IcpSdfOptions()
    rc = load_library().icp_sdf_options_default(C.byref(o))
    if rc != ICP_OK:
        raise IcpError(rc, "icp_sdf_options_default")
    for k, v in kw.items():
        if not any(k == f[0] for f in IcpSdfOptions._fields_):
            raise TypeError("icp_sdf_options has no field %r" % k)
        setattr(o, k, v)
    return o


class IcpVgicpOptions(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("min_points", C.c_int32), ("n_iterations", C.c_int32), ("min_valid", C.c_int32), ("stop_rotation", C.c_float),
                ("stop_translation", C.c_float)]


class IcpVoxelGridInfo(C.Structure):
    _fields_ = [("lo", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("n_occupied", C.c_int32), ("n_points", C.c_int32)]


def vgicp_options(**kw):
    """icp_vgicp_options: icp_vgicp_options_default (voxel 0.25 m, min_points 1, 30 iterations, min_valid 64, stops 1e-5 rad / 1e-5 m) with
    any field overridden by name."""
    o = IcpVgicpOptions()
    rc = load_library().icp_vgicp_options_default(C.byref(o))
    if rc != ICP_OK:
        raise IcpError(rc, "icp_vgicp_options_default")
    for k, v in kw.items():
        if not any(k == f[0] for f in IcpVgicpOptions._fields_):
            raise TypeError("icp_vgicp_options has no field %r" % k)
        setattr(o, k, v)
    return o


class IcpVoxelMapOptions(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("lo", C.c_int32 * 3), ("dims", C.c_int32 * 3)]


class IcpVoxelMapInsertInfo(C.Structure):
    _fields_ = [("n_considered", C.c_int32), ("n_entered", C.c_int32), ("n_outside", C.c_int32), ("n_cells_touched", C.c_int32), ("n_cells_new", C.c_int32),
                ("n_occupied", C.c_int32)]


class IcpVoxelMapInfo(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("lo", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("n_occupied", C.c_int32)]


class IcpVoxelHashMapInfo(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("capacity", C.c_int32), ("n_occupied", C.c_int32), ("n_grown", C.c_int32), ("n_unplaced", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class IcpVoxelMapPruneInfo(C.Structure):
    _fields_ = [("n_removed", C.c_int32), ("n_occupied", C.c_int32), ("n_vacated", C.c_int32), ("n_compacted", C.c_int32), ("capacity", C.c_int32),
                ("reserved", C.c_int32), ("n_points_removed", C.c_int64)]


def _prune_info(info):
    return {k: int(getattr(info, k)) for k, _ in info._fields_ if k != "reserved"}


def voxel_map_options(voxel_size, lo, dims):
    """icp_voxel_map_options: the voxel size in metres and the extent in cells (lowest cell, cells per axis)."""
    o = IcpVoxelMapOptions()
    o.voxel_size = voxel_size
    o.lo = (C.c_int32 * 3)(*[int(v) for v in lo]); o.dims = (C.c_int32 * 3)(*[int(v) for v in dims])
    return o


def voxel_map_extent(lower, upper, voxel_size):
    """(lo, dims) of the smallest voxel map that holds the box lower .. upper (metres), by the library's cell rule:
    c = (int)clamp(floorf(p / voxel_size), -2^30, 2^30) in fp32, lo = c(lower), dims = c(upper) - lo + 1."""
    vs = np.float32(voxel_size)
    cell = lambda p: np.clip(np.floor(np.asarray(p, np.float32) / vs), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    lo = cell(lower); hi = cell(upper)
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo + 1)


class IcpDepthFilterOptions(C.Structure):
    _fields_ = [("radius", C.c_int32), ("sigma_space", C.c_float), ("sigma_range", C.c_float)]


DEPTH_FILTER_TILE = (32, 8)              # ICP_DEPTH_FILTER_TILE_W x ICP_DEPTH_FILTER_TILE_H: the pixels of one block of the filter kernel


def depth_filter_options(**kw):
    """icp_depth_filter_options: icp_depth_filter_options_default (radius 0 = off, sigma_space 4.5 pixels, sigma_range 0.03 m) with any field
    overridden by name."""
    o = IcpDepthFilterOptions()
    rc = load_library().icp_depth_filter_options_default(C.byref(o))
    if rc != ICP_OK:
        raise IcpError(rc, "icp_depth_filter_options_default")
    for k, v in kw.items():
        if not any(k == f[0] for f in IcpDepthFilterOptions._fields_):
            raise TypeError("icp_depth_filter_options has no field %r" % k)
        setattr(o, k, v)
    return o


def depth_filter_tables(options=None, **kw):
    """icp_depth_filter_tables: the tables the device filters with under `options` (an IcpDepthFilterOptions, or `depth_filter_options`'
    arguments): (spatial (2r + 1, 2r + 1) fp32, range (256,) fp32, inv_bin as an np.float32).  Needs no device."""
    o = options if options is not None else depth_filter_options(**kw)
    w = 2 * min(max(int(o.radius), 0), 4) + 1          # (bad options are the library's to refuse)
    S =np.zeros((w, w), np.float32); R = np.zeros(256, np.float32); ib = C.c_float(0)
    rc = load_library().icp_depth_filter_tables(C.byref(o), _ptr(S), _ptr(R), C.byref(ib))
    if rc != ICP_OK:
        raise IcpError(rc, "icp_depth_filter_tables: bad options")
    return S, R, np.float32(ib.value)


class depth_filter_scope:
    """The runners' `depth_filter=` argument: the context's depth filter set from a dict of `Context.set_depth_filter` arguments inside
    the `with` block, the previous setting put back behind it."""

    def __init__(self, ctx, depth_filter):
        self.ctx, self.new = ctx, dict(depth_filter)

    def __enter__(self):
        self.old = self.ctx.depth_filter_options()
        self.ctx.set_depth_filter(**self.new)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.set_depth_filter(self.old.radius, self.old.sigma_space, self.old.sigma_range)
        return False


class tsdf_carve_scope:
    """The runners' `carve=` argument: the context's carve options set from a dict of `Context.set_tsdf_carve` arguments inside the
    `with` block, the previous setting put back behind it."""

    def __init__(self, ctx, carve):
        self.ctx, self.new = ctx, dict(carve)

    def __enter__(self):
        self.old = self.ctx.tsdf_carve_options()
        self.ctx.set_tsdf_carve(**self.new)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.set_tsdf_carve(self.old.distance, self.old.min_range)
        return False


def _colouring(name, colored):
    """Gives a method the keyword `name`: None or False (the default) calls it as it is; anything else calls `colored(self, value, ...)`
    with the method's own arguments.  The method's own signature stays what it was, as eth._carving keeps a runner's."""
    def give(plain):
        @functools.wraps(plain)
        def method(self, *args, **kw):
            value = kw.pop(name, None)
            if value is None or value is False:
                return plain(self, *args, **kw)
            return colored(self, value, *args, **kw)
        return method
    return give


def _clustering(*names):
    """Gives a mesh method the keywords `cluster` (a cell size in metres) and `cluster_origin`: cluster=None (the default) calls it as it
    is; otherwise icp_tsdf_mesh_clustered returns the same tuple with the mesh clustered on the device, the grid's
    origin at cluster_origin (the volume's by default).  names: the method's parameters after min_weight (`normals`, where there is one,
    and `colors`).  The method's own signature stays what it was."""
    def give(plain):
        @functools.wraps(plain)
        def method(self, min_weight=0.0, *args, **kw):
            cluster, origin = kw.pop("cluster", None), kw.pop("cluster_origin", None)
            if cluster is None:
                return plain(self, min_weight, *args, **kw)
            par = dict(zip(names, args), **kw)
            return self._tsdf_mesh_clustered(min_weight, bool(par.get("normals", True)), bool(par.get("colors", False)), cluster, origin)
        return method
    return give


def _color_term(kw):
    """Takes color_weight and color_huber (0.0 each by default) out of a keyword dict: None for a weight of zero -- the geometric call,
    made exactly as without the keywords -- or the icp_sdf_color_options of the photometric one."""
    weight, huber = float(kw.pop("color_weight", 0.0)), float(kw.pop("color_huber", 0.0))
    if not (np.isfinite(weight) and weight >= 0.0 and np.isfinite(huber) and huber >= 0.0):
        raise ValueError("color_weight and color_huber must be finite and >= 0")
    return IcpSdfColorOptions(weight, huber) if weight > 0.0 else None


def _photometric(colored):
    """Gives a method the keywords color_weight and color_huber: a weight of zero (the default) calls it as it is; a positive one calls
    `colored(self, colour options, ...)` with the method's own arguments.  The method's own signature stays what it was."""
    def give(plain):
        @functools.wraps(plain)
        def method(self, *args, **kw):
            copt = _color_term(kw)
            return plain(self, *args, **kw) if copt is None else colored(self, copt, *args, **kw)
        return method
    return give


def _tsdf_cloud_system_color(self, copt, which="source", pose=None, huber=0.0):
    w = _cloud(which)
    p = _pose_in(np.eye(4, dtype=np.float32) if pose is None else pose)
    o = sdf_options(huber=huber)
    sums = np.empty(29, np.float64); cnt = (C.c_int32 * 3)()
    self._ck(self.lib.icp_tsdf_cloud_system_color(self.h, C.c_int32(w), _ptr(p), C.byref(o), C.byref(copt), _ptr(sums), cnt))
    return sums, (cnt[0], cnt[1], cnt[2])


def _tsdf_align_cloud_color(self, copt, which="source", pose=None, n_iterations=20, huber=0.0, min_valid=64, stop_rotation=1e-5, stop_translation=1e-5, trace=False):
    w = _cloud(which)
    p = _pose_in(np.eye(4, dtype=np.float32) if pose is None else pose)
    o = sdf_options(n_iterations=n_iterations, huber=huber, min_valid=min_valid, stop_rotation=stop_rotation, stop_translation=stop_translation)
    rec = IcpSdfColorFrame(); tr = (IcpSdfColorIter * o.n_iterations)() if trace else None
    rc = self.lib.icp_tsdf_align_cloud_color(self.h, C.c_int32(w), C.byref(o), C.byref(copt), _ptr(p), C.byref(rec), tr)
    if rc not in (ICP_OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # the alignment's outcome: reported in the record
        self._ck(rc)
    r = _record(rec)
    if trace:
        return pose_from_c(p), r, rc, [_record(tr[i]) for i in range(r["iterations"])]
    return pose_from_c(p), r, rc


def _cloud_fuse_in(which, pose, sensor_origin):
    w = _cloud(which)
    p = _pose_in(np.eye(4, dtype=np.float32) if pose is None else pose)
    e = None
    if sensor_origin is not None:
        e = _f32(sensor_origin).reshape(-1)
        if e.size != 3:
            raise ValueError("sensor_origin must hold three numbers")
    return w, p, e


def _integrate_cloud_color(self, _, which="source", pose=None, sensor_origin=None):
    w, p, e = _cloud_fuse_in(which, pose, sensor_origin)
    info = IcpTsdfCloudInfo(); nc = C.c_int32(0)
    self._ck(self.lib.icp_tsdf_integrate_cloud_color(self.h, C.c_int32(w), _ptr(p), _ptr(e), C.byref(info), C.byref(nc)))
    return dict(_record(info), n_colored=nc.value)


def _scans_in(scans):
    pts = [_f32(s[0] if isinstance(s, (tuple, list)) else s) for s in scans]
    if any(a.ndim != 2 or a.shape[1] != 3 for a in pts):
        raise ValueError("a scan is xyz (n, 3)")
    return pts


def _track_scans_sdf(self, colors, scans, pose=None, **options):
    """Context.track_scans_sdf behind its docstring; colors: None, or one (n, 4) uint8 array per scan (icp_track_scans_sdf_color, or with
    color_weight > 0 among the options icp_track_scans_sdf_photometric)."""
    copt = _color_term(options)
    if copt is not None and colors is None:
        raise ValueError("color_weight > 0 needs colors: one rgba array per scan")
    o = sdf_options(**options)
    ns = len(scans)
    pts = _scans_in(scans)
    xp = (C.c_void_p * max(ns, 1))(*[_ptr(a) for a in pts])
    cnt = (C.c_int32 * max(ns, 1))(*[len(a) for a in pts])
    p = _pose_in(np.eye(4, dtype=np.float32) if pose is None else pose)
    start = pose_from_c(p)
    out = ((IcpSdfFrame if copt is None else IcpSdfColorFrame) * max(ns - 1, 1))(); infos = (IcpTsdfCloudInfo * max(ns, 1))()
    if colors is None:
        rc = self.lib.icp_track_scans_sdf(self.h, xp, cnt, C.c_int32(ns), C.byref(o), _ptr(p), out, infos)
    else:
        if len(colors) != ns:
            raise ValueError("one colour array per scan")
        cols = [np.ascontiguousarray(c, dtype=np.uint8) for c in colors]
        if any(c.shape != (len(a), 4) for c, a in zip(cols, pts)):
            raise ValueError("a scan's colours are rgba (n, 4) bytes, one row per point")
        cp = (C.c_void_p * max(ns, 1))(*[_ptr(c) for c in cols])
        ncol = (C.c_int32 * max(ns, 1))()
        if copt is None:
            rc = self.lib.icp_track_scans_sdf_color(self.h, xp, cp, cnt, C.c_int32(ns), C.byref(o), _ptr(p), out, infos, ncol)
        else:
            rc = self.lib.icp_track_scans_sdf_photometric(self.h, xp, cp, cnt, C.c_int32(ns), C.byref(o), C.byref(copt), _ptr(p), out, infos, ncol)
    if rc not in (ICP_OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # per-scan outcomes: reported in the records
        self._ck(rc)
    recs = [_record(out[i]) for i in range(ns - 1)]
    res = ([start] + [r["pose"] for r in recs], recs, [_record(infos[i]) for i in range(ns)], rc)
    return res if colors is None else res + ([ncol[i] for i in range(ns)],)


class IcpSdfColorOptions(C.Structure):
    _fields_ = [("weight", C.c_float), ("huber", C.c_float)]


class IcpSdfColorIter(C.Structure):
    _fields_ = [("n_valid", C.c_int32), ("n_color", C.c_int32), ("status", C.c_int32), ("pad", C.c_int32), ("cost", C.c_double), ("cost_color", C.c_double),
                ("pose", C.c_float * 16)]


class IcpSdfColorFrame(C.Structure):
    _fields_ = [("n_depth", C.c_int32), ("n_valid_first", C.c_int32), ("n_valid_last", C.c_int32), ("n_color_first", C.c_int32), ("n_color_last", C.c_int32),
                ("iterations", C.c_int32), ("status", C.c_int32), ("pad", C.c_int32), ("cost_first", C.c_double), ("cost_last", C.c_double),
                ("cost_color_first", C.c_double), ("cost_color_last", C.c_double), ("pose", C.c_float * 16)]


def sdf_color_options(**kw):
    """icp_sdf_color_options: icp_sdf_color_options_default (weight 0.1 m per unit of intensity, huber off) with any field overridden by name."""
    o = IcpSdfColorOptions()
    rc = load_library().icp_sdf_color_options_default(C.byref(o))
    if rc != ICP_OK:
        raise IcpError(rc, "icp_sdf_color_options_default")
    for k, v in kw.items():
        if not any(k == f[0] for f in IcpSdfColorOptions._fields_):
            raise TypeError("icp_sdf_color_options has no field %r" % k)
        setattr(o, k, v)
    return o


def _sdf_color_in(rgbx, n_pixels, color_weight, color_huber, message):
    """(colour frame(s), IcpSdfColorOptions) of a direct SDF call with color_weight > 0, (.., None) with color_weight == 0."""
    if not color_weight >= 0:
        raise ValueError("color_weight must be >= 0")
    if color_weight == 0:
        return None, None
    if rgbx is None:
        raise ValueError("color_weight > 0 needs the colour frame(s)")
    return _rgbx_in(rgbx, n_pixels, message), sdf_color_options(weight=color_weight, huber=color_huber)


class IcpLmOptions(C.Structure):
    _fields_ = [("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("max_num_iterations", C.c_int32), ("max_num_consecutive_invalid_steps", C.c_int32), ("jacobi_scaling", C.c_int32)]


class IcpLmSummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("successful_steps", C.c_int32), ("unsuccessful_steps", C.c_int32), ("invalid_steps", C.c_int32),
                ("termination", C.c_int32), ("n_residual_blocks", C.c_int32),
                ("accepted_steps_mask", C.c_uint32), ("invalid_steps_mask", C.c_uint32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("trust_region_radius", C.c_double), ("x", C.c_double * 6)]


LM_CONVERGENCE, LM_NO_CONVERGENCE, LM_FAILURE, LM_NO_RESIDUALS = 0, 1, 2, 3

METRIC_POINT_TO_POINT, METRIC_POINT_TO_PLANE, METRIC_SYMMETRIC, METRIC_GICP, METRIC_COLORED = 0, 1, 2, 3, 4


class IcpGicpOptions(C.Structure):
    _fields_ = [("epsilon", C.c_float), ("covariance_k", C.c_int32)]


class IcpColoredOptions(C.Structure):
    _fields_ = [("lambda_geometric", C.c_float), ("gradient_k", C.c_int32)]


def lm_options(**kw):
    """icp_lm_options: Ceres' defaults with configureSolver's max_num_iterations = 10 (icp_lm_options_default), fields overridden by name."""
    o = IcpLmOptions()
    rc = load_library().icp_lm_options_default(C.byref(o))
    if rc != ICP_OK:
        raise IcpError(rc, "icp_lm_options_default")
    for k, v in kw.items():
        if not any(k == f[0] for f in IcpLmOptions._fields_):
            raise TypeError("icp_lm_options has no field %r" % k)
        setattr(o, k, v)
    return o


def select_optimizer(ctx, nonlinear):
    """The runners' `nonlinear=` argument: True / an IcpLmOptions -> the non-linear optimiser, False -> the linear one, None -> unchanged."""
    if nonlinear is not None:
        ctx.set_optimizer(nonlinear)


def select_convergence(ctx, convergence):
    """The runners' `convergence=` argument: a dict of set_convergence_options' arguments -> on, False -> off, None -> unchanged."""
    if convergence is False:
        ctx.set_convergence_options(None)
    elif convergence is not None:
        ctx.set_convergence_options(**convergence)


def _camera(cls, K, width, height, extrinsics):
    K = np.asarray(K, dtype=np.float32)
    cam = cls(float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), int(width), int(height))
    E = pose_to_c(np.eye(4) if extrinsics is None else extrinsics)
    for k in range(16):
        cam.extrinsics[k] = float(E[k])
    return cam


def depth_camera(K, width, height, extrinsics=None):
    """icp_depth_camera from a 3x3 intrinsic matrix (K(0,0), K(1,1), K(0,2), K(1,2)) and an optional 4x4 depthExtrinsics."""
    return _camera(IcpDepthCamera, K, width, height, extrinsics)


class IcpRobustOptions(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("tuning", C.c_float), ("sigma", C.c_float), ("overlap", C.c_float)]


class IcpRobustStats(C.Structure):
    _fields_ = [("n_entering", C.c_int32), ("n_kept", C.c_int32), ("trim_d2", C.c_float), ("sigma", C.c_float)]


ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_TUKEY = 0, 1, 2, 3
ROBUST_KERNELS = {"none": ROBUST_NONE, "huber": ROBUST_HUBER, "cauchy": ROBUST_CAUCHY, "tukey": ROBUST_TUKEY}


class IcpReciprocalOptions(C.Structure):
    _fields_ = [("enabled", C.c_int32)]


class IcpReciprocalStats(C.Structure):
    _fields_ = [("n_matched", C.c_int32), ("n_mutual", C.c_int32)]


def select_reciprocal(ctx, reciprocal):
    """The runners' `reciprocal=` argument: True -> reciprocal (mutual nearest-neighbour) rejection on, False -> off, None -> unchanged."""
    if reciprocal is not None:
        ctx.set_reciprocal_options(enabled=bool(reciprocal))


class IcpConvergenceOptions(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("rotation_eps", C.c_float), ("translation_eps", C.c_float), ("min_iterations", C.c_int32), ("patience", C.c_int32)]


class IcpConvergenceStep(C.Structure):
    _fields_ = [("rotation", C.c_float), ("translation", C.c_float), ("eligible", C.c_int32), ("streak", C.c_int32)]


class IcpConvergenceResult(C.Structure):
    _fields_ = [("converged", C.c_int32), ("iterations_run", C.c_int32), ("iterations_planned", C.c_int32), ("rotation", C.c_float), ("translation", C.c_float)]


CONVERGENCE_STEP_DTYPE = np.dtype([("rotation", np.float32), ("translation", np.float32), ("eligible", np.int32), ("streak", np.int32)])


class IcpNssOptions(C.Structure):
    _fields_ = [("grid", C.c_int32), ("resample", C.c_int32)]


SELECT_ALL, SELECT_RANDOM, SELECT_NORMAL_SPACE = 0, 1, 2


class IcpGlobalOptions(C.Structure):
    _fields_ = [("k", C.c_int32), ("feature_stride", C.c_int32), ("mutual", C.c_int32), ("n_hypotheses", C.c_int32), ("edge_similarity", C.c_float),
                ("inlier_distance", C.c_float), ("seed", C.c_uint32), ("n_best", C.c_int32)]


class IcpGlobalHypothesis(C.Structure):
    _fields_ = [("pose", C.c_float * 16), ("n_inliers", C.c_int32), ("reserved", C.c_int32), ("sum_d2", C.c_double), ("status", C.c_int32), ("draw", C.c_int32 * 3)]


GLOBAL_HYPOTHESIS_DTYPE = np.dtype([("pose", np.float32, 16), ("n_inliers", np.int32), ("reserved", np.int32), ("sum_d2", np.float64), ("status", np.int32), ("draw", np.int32, 3)], align=True)
CLOUD_TARGET, CLOUD_SOURCE, CLOUD_BOTH = 0, 1, 2
GLOBAL_VALID, GLOBAL_REPEATED, GLOBAL_EDGES, GLOBAL_DEGENERATE = 0, 1, 2, 3
FPFH_DIM = 33
_CLOUDS = {"target": CLOUD_TARGET, "source": CLOUD_SOURCE, "both": CLOUD_BOTH}


def _cloud(which):
    return _CLOUDS[which] if isinstance(which, str) else int(which)


class IcpColorCamera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("width", C.c_int32), ("height", C.c_int32),
                ("extrinsics", C.c_float * 16)]


def color_camera(K, width, height, extrinsics=None):
    """icp_color_camera: colour intrinsics (K(0,0), K(1,1), K(0,2), K(1,2)), the RGBX frame's size and optional 4x4 colour extrinsics."""
    return _camera(IcpColorCamera, K, width, height, extrinsics)


def depth_options(keep_original_size=False, downsample_factor=1, max_distance=0.1, fix_color_index=False):
    """icp_depth_options: the constructor arguments of PointCloud(depthMap, ...) (PointCloud.h:78)."""
    return IcpDepthOptions(int(bool(keep_original_size)), int(downsample_factor), float(max_distance), int(bool(fix_color_index)))


class IcpMeshClusterOptions(C.Structure):
    _fields_ = [("cell_size", C.c_float), ("origin", C.c_float * 3)]


class IcpMeshClusterInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_vertices_in", "n_triangles_in", "n_invalid_vertices", "n_invalid_triangles", "n_cells", "n_vertices", "n_triangles",
                                         "n_degenerate", "n_duplicate")]


MESH_CLUSTER_MAX = 1 << 27


def mesh_cluster_options(cell_size, origin=(0.0, 0.0, 0.0)):
    """icp_mesh_cluster_options: the cell size (metres) and the grid's origin (a corner of cell (0, 0, 0))."""
    o = IcpMeshClusterOptions()
    o.cell_size = float(cell_size)
    o.origin[:] = [float(x) for x in origin]
    return o


COMM_ID_BYTES = 128

# every symbol include/icp_hip.h declares (tests check the library exports all of them)
EXPORTS = ["icp_ctx_create", "icp_ctx_create_on_stream", "icp_ctx_destroy", "icp_last_error", "icp_params_default",
           "icp_set_params", "icp_get_params", "icp_set_target", "icp_set_source", "icp_query_matches", "icp_match", "icp_match_seeded",
           "icp_correspond", "icp_iterate", "icp_run", "icp_run_multistart", "icp_get_timing", "icp_get_iteration_times", "icp_set_stage_timing", "icp_set_convergence_reference", "icp_rmse", "icp_benchmark_error",
           "icp_transform_points", "icp_transform_normals", "icp_version", "icp_schedule", "icp_select_hash", "icp_backproject_depth", "icp_estimate_normals",
           "icp_set_target_depth", "icp_set_source_depth", "icp_track_depth_frames", "icp_depth_mesh",
           "icp_tsdf_options_default", "icp_tsdf_options_check", "icp_tsdf_create", "icp_tsdf_reset", "icp_tsdf_release", "icp_tsdf_download", "icp_tsdf_upload",
           "icp_tsdf_integrate", "icp_tsdf_raycast", "icp_set_target_tsdf", "icp_track_depth_model", "icp_tsdf_mesh",
           "icp_tsdf_color_create", "icp_tsdf_color_release", "icp_tsdf_color_download", "icp_tsdf_color_upload", "icp_tsdf_integrate_color",
           "icp_tsdf_raycast_color", "icp_set_target_tsdf_color", "icp_track_depth_model_color", "icp_tsdf_mesh_color",
           "icp_sdf_options_default", "icp_sdf_options_check", "icp_tsdf_sample", "icp_tsdf_sdf_system", "icp_tsdf_align_depth", "icp_track_depth_sdf",
           "icp_tsdf_create_hashed", "icp_tsdf_reserve_blocks", "icp_tsdf_allocate_blocks", "icp_get_tsdf_hashed", "icp_tsdf_upload_hashed",
           "icp_tsdf_mesh_hashed", "icp_tsdf_raycast_hashed", "icp_set_target_tsdf_hashed", "icp_track_depth_model_hashed",
           "icp_tsdf_evict_blocks", "icp_tsdf_evicted_blocks", "icp_tsdf_insert_blocks", "icp_tsdf_integrate_cloud",
           "icp_tsdf_cloud_system", "icp_tsdf_align_cloud", "icp_track_scans_sdf", "icp_tsdf_integrate_cloud_color", "icp_track_scans_sdf_color",
           "icp_tsdf_cloud_system_color", "icp_tsdf_align_cloud_color", "icp_track_scans_sdf_photometric",
           "icp_tsdf_create_color_hashed", "icp_tsdf_hashed_has_color", "icp_get_tsdf_color_hashed", "icp_tsdf_upload_color_hashed",
           "icp_tsdf_evicted_blocks_color", "icp_tsdf_insert_blocks_color",
           "icp_tsdf_raycast_color_hashed", "icp_set_target_tsdf_color_hashed", "icp_track_depth_model_color_hashed", "icp_tsdf_mesh_color_hashed",
           "icp_sdf_color_options_default", "icp_sdf_color_options_check", "icp_tsdf_sample_color", "icp_tsdf_sdf_system_color", "icp_tsdf_align_depth_color",
           "icp_track_depth_sdf_color",
           "icp_depth_filter_options_default", "icp_depth_filter_options_check", "icp_set_depth_filter_options", "icp_get_depth_filter_options",
           "icp_depth_filter_tables", "icp_filter_depth",
           "icp_tsdf_carve_options_default", "icp_tsdf_carve_options_check", "icp_set_tsdf_carve_options", "icp_get_tsdf_carve_options", "icp_tsdf_carve_stats",
           "icp_vgicp_options_default", "icp_vgicp_options_check", "icp_voxelize_target", "icp_get_voxel_grid", "icp_vgicp_system", "icp_vgicp_align",
           "icp_voxel_map_options_check", "icp_voxel_map_create", "icp_voxel_map_destroy", "icp_voxel_map_insert", "icp_get_voxel_map", "icp_voxel_map_upload",
           "icp_voxel_map_system", "icp_voxel_map_align", "icp_track_scans_vmap",
           "icp_voxel_map_create_hashed", "icp_voxel_map_reserve", "icp_get_voxel_map_hashed", "icp_voxel_map_upload_hashed",
           "icp_voxel_map_prune", "icp_voxel_map_compact", "icp_track_scans_vmap_local",
           "icp_lm_options_default", "icp_set_optimizer", "icp_get_lm_summaries",
           "icp_gicp_options_default", "icp_set_gicp_options", "icp_get_gicp_options", "icp_get_gicp_normals",
           "icp_colored_options_default", "icp_set_colored_options", "icp_get_colored_options", "icp_get_color_gradients",
           "icp_robust_options_default", "icp_set_robust_options", "icp_get_robust_options", "icp_get_robust_stats",
           "icp_reciprocal_options_default", "icp_set_reciprocal_options", "icp_get_reciprocal_options", "icp_get_reciprocal_stats",
           "icp_convergence_options_default", "icp_set_convergence_options", "icp_get_convergence_options", "icp_get_convergence", "icp_get_convergence_trace",
           "icp_nss_options_default", "icp_set_nss_options", "icp_get_nss_options", "icp_get_normal_buckets", "icp_get_selection",
           "icp_global_options_default", "icp_set_global_options", "icp_get_global_options", "icp_compute_features", "icp_get_features", "icp_get_spfh",
           "icp_get_feature_neighbours", "icp_match_features", "icp_register_global", "icp_get_global_hypotheses",
           "icp_mesh_cluster", "icp_tsdf_mesh_clustered",
           "icp_batch_run", "icp_pair_owner", "icp_pairs_of_rank", "icp_comm_unique_id", "icp_comm_create", "icp_comm_destroy", "icp_gather_poses",
           "icp_comm_last_error"]

_lib = None


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libicp_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` (%s)" % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.icp_last_error.restype = C.c_char_p
        _lib.icp_version.restype = C.c_char_p
        _lib.icp_comm_last_error.restype = C.c_char_p
        _lib.icp_pair_owner.restype = C.c_int32
        _lib.icp_pairs_of_rank.restype = C.c_int32
        _lib.icp_select_hash.restype = C.c_uint32
        i32, vp = C.c_int32, C.c_void_p
        _lib.icp_mesh_cluster.argtypes = [vp, i32, i32, vp, vp, vp, vp, C.POINTER(IcpMeshClusterOptions), i32, i32, vp, vp, vp, vp, C.POINTER(IcpMeshClusterInfo)]
        _lib.icp_mesh_cluster.restype = i32
        _lib.icp_tsdf_mesh_clustered.argtypes = [vp, C.c_float, C.POINTER(IcpMeshClusterOptions), i32, i32, i32, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32),
                                                 C.POINTER(IcpMeshClusterInfo)]
        _lib.icp_tsdf_mesh_clustered.restype = i32
    return _lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pose_to_c(pose):
    """(4,4) numpy (row, col) -> 16 floats column-major == Eigen::Matrix4f::data()."""
    return np.ascontiguousarray(np.asarray(pose, dtype=np.float32).T).reshape(16).copy()


def _pose_in(pose):
    """A 4x4 pose as the 16 floats the library takes; anything else is a ValueError."""
    if np.shape(pose) != (4, 4):
        raise ValueError("the pose must be a 4x4 matrix")
    return pose_to_c(pose)


def pose_from_c(buf):
    return np.array(buf, dtype=np.float32).reshape(4, 4).T.copy()


def _record(s):
    """One record struct as a dict, keys in the order of _fields_: a 16-float `pose` as a 4x4, `x` as a float64 array, `converged` as a bool."""
    convert = {"pose": pose_from_c, "x": lambda v: np.array(v[:], np.float64), "converged": bool}
    return {k: convert[k](getattr(s, k)) if k in convert else getattr(s, k) for k, _ in s._fields_}


def _depth_in(depth, cam, sequence=False):
    """The depth frame (or the (n, h, w) frames) as contiguous fp32, checked against the camera's size."""
    d = np.ascontiguousarray(depth, dtype=np.float32)
    if sequence and d.size != d.shape[0] * cam.width * cam.height:
        raise ValueError("depth frames do not match the camera size")
    if not sequence and d.size != cam.width * cam.height:
        raise ValueError("depth frame has %d pixels, the camera %d x %d" % (d.size, cam.width, cam.height))
    return d


def _rgbx_in(rgbx, n_pixels, message="colour frame must hold 4 bytes per pixel"):
    """The RGBX frame(s) as contiguous bytes, four per pixel, or None."""
    c = None if rgbx is None else np.ascontiguousarray(rgbx, dtype=np.uint8)
    if c is not None and c.size != 4 * n_pixels:
        raise ValueError(message)
    return c


def _gt_in(gt, nf):
    """The tracking calls' ground truth: (nf - 1) 4x4 transforms as column-major rows, or None."""
    g = None if gt is None else np.ascontiguousarray(np.stack([pose_to_c(T) for T in gt]) if len(gt) else np.zeros((0, 16)), dtype=np.float32)
    if g is not None and len(g) != nf - 1:
        raise ValueError("gt needs one transform per tracked frame")
    return g


def schedule(params, n_src, max_out=4096):
    """icp_schedule: decimation factor per iteration (host logic only, needs no GPU)."""
    lib = load_library()
    buf = (C.c_int32 * max_out)(); cnt = C.c_int32(0)
    rc = lib.icp_schedule(C.byref(params), C.c_int32(n_src), buf, C.c_int32(max_out), C.byref(cnt))
    if rc != ICP_OK:
        raise IcpError(rc, "icp_schedule")
    return [buf[i] for i in range(min(cnt.value, max_out))]


def select_hash(seed, iteration, index):
    return int(load_library().icp_select_hash(C.c_uint32(seed), C.c_uint32(iteration), C.c_uint32(index)))


def default_params():
    p = IcpParams()
    load_library().icp_params_default(C.byref(p))
    return p


class Context:
    """RAII wrapper of icp_ctx."""

    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        self.h = C.c_void_p()
        rc = self.lib.icp_ctx_create_on_stream(C.c_int(device), C.c_void_p(stream) if stream else None, C.byref(self.h))
        if rc != ICP_OK:
            self.h = None
            raise IcpError(rc, "icp_ctx_create failed (is a HIP device visible?)")
        self.params = IcpParams()
        self.lib.icp_params_default(C.byref(self.params))

    def close(self):
        if getattr(self, "h", None):
            self.lib.icp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != ICP_OK:
            raise IcpError(rc, self.lib.icp_last_error(self.h).decode())

    def _counted(self, fn, lead, make, n_out=1):
        """A count-then-fill getter: fn(h, *lead, None..., 0, &n) reports the count, make(n) gives the output buffer (a tuple of n_out
        of them when n_out > 1), fn(h, *lead, buffers..., n, &n) fills them.  Returns what make gave."""
        n = C.c_int32(0)
        self._ck(fn(self.h, *lead, *([None] * n_out), C.c_int32(0), C.byref(n)))
        out = make(n.value)
        bufs = out if n_out > 1 else (out,)
        self._ck(fn(self.h, *lead, *[_ptr(b) if isinstance(b, np.ndarray) else b for b in bufs], C.c_int32(n.value), C.byref(n)))
        return out

    def _records(self, fn, struct):
        """A count-then-fill getter of record structs: one dict per record."""
        return [_record(b) for b in self._counted(fn, (), lambda n: (struct * n)())]

    def set_optimizer(self, options=True, **kw):
        """icp_set_optimizer: options True (the defaults, fields overridden by kw) or an IcpLmOptions selects the non-linear optimiser
        (CeresICPOptimizer); None / False return to the linear one."""
        if options is None or options is False:
            if kw:
                raise TypeError("set_optimizer: field overrides need the non-linear optimiser (options True)")
            self._ck(self.lib.icp_set_optimizer(self.h, None))
            return None
        if isinstance(options, IcpLmOptions):
            if kw:
                raise TypeError("set_optimizer: give either an IcpLmOptions or field overrides, not both")
            o = options
        elif options is True:
            o = lm_options(**kw)
        else:
            raise TypeError("set_optimizer: options must be True, None, False or an IcpLmOptions")
        self._ck(self.lib.icp_set_optimizer(self.h, C.byref(o)))
        return o

    def lm_summaries(self):
        """icp_get_lm_summaries: one dict per ICP iteration of the last run (Solver::Summary of its ceres::Solve), all of them."""
        return self._records(self.lib.icp_get_lm_summaries, IcpLmSummary)

    def set_gicp_options(self, epsilon=1e-3, k=20):
        """icp_set_gicp_options: the plane-to-plane regulariser and the neighbours of the GICP normals (0: the clouds' own normals)."""
        o = IcpGicpOptions(float(epsilon), int(k))
        self._ck(self.lib.icp_set_gicp_options(self.h, C.byref(o)))
        return o

    def gicp_options(self):
        o = IcpGicpOptions()
        self._ck(self.lib.icp_get_gicp_options(self.h, C.byref(o)))
        return o

    def gicp_normals(self, which="target"):
        """icp_get_gicp_normals: the per-point GICP normals of the target or the source, n x 3 fp32 in the cloud's order (NaN where undefined)."""
        w = {"target": 0, "source": 1}[which]
        return self._counted(self.lib.icp_get_gicp_normals, (C.c_int32(w),), lambda n: np.empty((n, 3), np.float32))

    def set_colored_options(self, lambda_geometric=0.968, k=20):
        """icp_set_colored_options: the weight of the geometric term and the neighbours of the target's colour gradients."""
        o = IcpColoredOptions(float(lambda_geometric), int(k))
        self._ck(self.lib.icp_set_colored_options(self.h, C.byref(o)))
        return o

    def colored_options(self):
        o = IcpColoredOptions()
        self._ck(self.lib.icp_get_colored_options(self.h, C.byref(o)))
        return o

    def color_gradients(self):
        """icp_get_color_gradients: the target's per-point colour gradients, n x 3 fp32 in the cloud's order (NaN where undefined)."""
        return self._counted(self.lib.icp_get_color_gradients, (), lambda n: np.empty((n, 3), np.float32))

    def set_robust_options(self, kernel="none", tuning=0.0, sigma=0.0, overlap=1.0):
        """icp_set_robust_options: trimmed ICP (overlap < 1) and an M-estimator ("none", "huber", "cauchy", "tukey" or ICP_ROBUST_*) with
        tuning constant c (0: the kernel's standard one) and scale sigma (0: adaptive, from the median residual)."""
        k = ROBUST_KERNELS[kernel.lower()] if isinstance(kernel, str) else int(kernel)
        o = IcpRobustOptions(k, float(tuning), float(sigma), float(overlap))
        self._ck(self.lib.icp_set_robust_options(self.h, C.byref(o)))
        return o

    def robust_options(self):
        o = IcpRobustOptions()
        self._ck(self.lib.icp_get_robust_options(self.h, C.byref(o)))
        return o

    def robust_stats(self):
        """icp_get_robust_stats: one dict per ICP iteration of the last icp_iterate / icp_run / icp_correspond (none when robust mode was off)."""
        return self._records(self.lib.icp_get_robust_stats, IcpRobustStats)

    def set_reciprocal_options(self, enabled=True):
        """icp_set_reciprocal_options: reciprocal (mutual nearest-neighbour) rejection: a pair (s, t) is kept only if s is also the nearest
        source point to t.  set_reciprocal_options(False) turns the option off."""
        o = IcpReciprocalOptions(int(bool(enabled)))
        self._ck(self.lib.icp_set_reciprocal_options(self.h, C.byref(o)))
        return o

    def reciprocal_options(self):
        o = IcpReciprocalOptions()
        self._ck(self.lib.icp_get_reciprocal_options(self.h, C.byref(o)))
        return o

    def reciprocal_stats(self):
        """icp_get_reciprocal_stats: one dict per ICP iteration of the last icp_iterate / icp_run / icp_correspond (none when the option was off)."""
        return self._records(self.lib.icp_get_reciprocal_stats, IcpReciprocalStats)

    def set_convergence_options(self, rotation=None, translation=None, min_iterations=1, patience=1):
        """icp_set_convergence_options: stop run / batch_run / track_depth_frames on the device once `patience` consecutive eligible
        iterations moved the pose by at most `rotation` (|sin theta|, ~radians) and `translation` (metres), not before `min_iterations`.
        set_convergence_options(None) turns the option off."""
        if rotation is None and translation is None:
            self._ck(self.lib.icp_set_convergence_options(self.h, None))
            return self.convergence_options()
        if rotation is None or translation is None:
            raise TypeError("set_convergence_options: give both rotation and translation, or neither (off)")
        o = IcpConvergenceOptions(1, float(rotation), float(translation), int(min_iterations), int(patience))
        self._ck(self.lib.icp_set_convergence_options(self.h, C.byref(o)))
        return o

    def convergence_options(self):
        o = IcpConvergenceOptions()
        self._ck(self.lib.icp_get_convergence_options(self.h, C.byref(o)))
        return o

    def convergence(self):
        """icp_get_convergence: the last run on the context: converged, iterations_run, iterations_planned and the measure (rotation,
        translation) of the last iteration that ran (-1 with the option off)."""
        r = IcpConvergenceResult()
        self._ck(self.lib.icp_get_convergence(self.h, C.byref(r)))
        return _record(r)

    def convergence_trace(self):
        """icp_get_convergence_trace: one (rotation, translation, eligible, streak) record per iteration that ran (none with the option off)."""
        return self._counted(self.lib.icp_get_convergence_trace, (), lambda n: np.zeros(n, CONVERGENCE_STEP_DTYPE))

    def set_nss_options(self, grid=5, resample=True):
        """icp_set_nss_options: normal-space sampling (params.selection = SELECT_NORMAL_SPACE): cells per cube-face edge (3, 5 or 7) and
        whether every iteration draws anew (True) or one draw per level is held for the run (False)."""
        o = IcpNssOptions(int(grid), int(resample))
        self._ck(self.lib.icp_set_nss_options(self.h, C.byref(o)))
        return o

    def nss_options(self):
        o = IcpNssOptions()
        self._ck(self.lib.icp_get_nss_options(self.h, C.byref(o)))
        return o

    def normal_buckets(self):
        """icp_get_normal_buckets: the normal-space bucket of every source point, uint16 in the cloud's order (0xFFFF: none)."""
        return self._counted(self.lib.icp_get_normal_buckets, (), lambda n: np.empty(n, np.uint16))

    def selection(self, iteration):
        """icp_get_selection: the query set (original source indices, increasing) of one iteration of the last run with selection 1 or 2."""
        return self._counted(self.lib.icp_get_selection, (C.c_int32(iteration),), lambda n: np.empty(n, np.int32))

    def set_global_options(self, **kw):
        """icp_set_global_options: global registration (FPFH features, feature matching, RANSAC).  Keywords: k (5, 10, 20), feature_stride,
        mutual, n_hypotheses, edge_similarity, inlier_distance (metres), seed, n_best; what is not given keeps its default."""
        o = IcpGlobalOptions()
        self.lib.icp_global_options_default(C.byref(o))
        for k, v in kw.items():
            if not hasattr(o, k):
                raise TypeError("unknown global option %r" % k)
            setattr(o, k, type(getattr(o, k))(v))
        self._ck(self.lib.icp_set_global_options(self.h, C.byref(o)))
        return o

    def global_options(self):
        o = IcpGlobalOptions()
        self._ck(self.lib.icp_get_global_options(self.h, C.byref(o)))
        return o

    def compute_features(self, which="both"):
        """icp_compute_features: the features of "target", "source" or "both" into the context's cache."""
        self._ck(self.lib.icp_compute_features(self.h, C.c_int32(_cloud(which))))

    def features(self, which="source"):
        """icp_get_features: the FPFH rows of the keypoints, (n_keypoints, 33) float32; row r is point r * feature_stride, NaN rows: no feature."""
        return self._counted(self.lib.icp_get_features, (C.c_int32(_cloud(which)),), lambda n: np.empty((n, FPFH_DIM), np.float32))

    def spfh(self, which="source"):
        """icp_get_spfh: (counts (n, 33) uint8, pairs (n,) int32) of every point."""
        return self._counted(self.lib.icp_get_spfh, (C.c_int32(_cloud(which)),),
                             lambda n: (np.empty((n, FPFH_DIM), np.uint8), np.empty(n, np.int32)), n_out=2)

    def feature_neighbours(self, which="source"):
        """icp_get_feature_neighbours: (idx (n, k) int32, d2 (n, k) float32), ascending (d2, index) per point; unfilled slots (-1, inf)."""
        k = self.global_options().k
        return self._counted(self.lib.icp_get_feature_neighbours, (C.c_int32(_cloud(which)),),
                             lambda n: (np.empty((n, k), np.int32), np.empty((n, k), np.float32)), n_out=2)

    def match_features(self):
        """icp_match_features: (src_idx, tgt_idx) int32 arrays of the feature correspondences, ascending in src_idx."""
        # at most one pair per source keypoint: buffers of that size make it one matcher run, not two
        cap = (int(getattr(self, "n_src", 0)) + self.global_options().feature_stride - 1) // self.global_options().feature_stride
        m = C.c_int32(0)
        if cap <= 0:                                        # (a source this wrapper did not upload: ask for the count first)
            self._ck(self.lib.icp_match_features(self.h, None, None, C.c_int32(0), C.byref(m)))
            cap = m.value
        si = np.empty(max(cap, 1), np.int32); ti = np.empty(max(cap, 1), np.int32)
        self._ck(self.lib.icp_match_features(self.h, _ptr(si), _ptr(ti), C.c_int32(cap), C.byref(m)))
        if m.value > cap:                                   # (the resident source is larger than n_src says: once more with room)
            cap = m.value
            si = np.empty(cap, np.int32); ti = np.empty(cap, np.int32)
            self._ck(self.lib.icp_match_features(self.h, _ptr(si), _ptr(ti), C.c_int32(cap), C.byref(m)))
        return si[:m.value].copy(), ti[:m.value].copy()

    def register_global(self, check=True):
        """icp_register_global: features, matching, RANSAC.  Returns (poses, records, status): the best poses (a list of 4 x 4, best first),
        their hypothesis records (GLOBAL_HYPOTHESIS_DTYPE) and the status code (check=False: ERR_NO_CORRESPONDENCES comes back as a code)."""
        nb = self.global_options().n_best
        poses = np.zeros((nb, 16), np.float32); recs = np.zeros(nb, GLOBAL_HYPOTHESIS_DTYPE); n = C.c_int32(0)
        rc = self.lib.icp_register_global(self.h, _ptr(poses), _ptr(recs), C.byref(n))
        if check or rc not in (ICP_OK, ERR_NO_CORRESPONDENCES):
            self._ck(rc)
        return [pose_from_c(p) for p in poses[:n.value]], recs[:n.value].copy(), rc

    def global_hypotheses(self):
        """icp_get_global_hypotheses: every hypothesis of the last register_global, in order of h (GLOBAL_HYPOTHESIS_DTYPE)."""
        return self._counted(self.lib.icp_get_global_hypotheses, (), lambda n: np.zeros(n, GLOBAL_HYPOTHESIS_DTYPE))

    def push_params(self):
        self._ck(self.lib.icp_set_params(self.h, C.byref(self.params)))

    def set_target(self, xyz, normals=None, rgba=None):
        xyz = _f32(xyz); normals = None if normals is None else _f32(normals)
        rgba = None if rgba is None else np.ascontiguousarray(rgba, dtype=np.uint8)
        self._ck(self.lib.icp_set_target(self.h, _ptr(xyz), _ptr(normals), _ptr(rgba), C.c_int32(len(xyz))))
        self.n_tgt = len(xyz)

    def set_source(self, xyz, normals=None, rgba=None):
        xyz = _f32(xyz); normals = None if normals is None else _f32(normals)
        rgba = None if rgba is None else np.ascontiguousarray(rgba, dtype=np.uint8)
        self._ck(self.lib.icp_set_source(self.h, _ptr(xyz), _ptr(normals), _ptr(rgba), C.c_int32(len(xyz))))
        self.n_src = len(xyz)

    def query_matches(self, transformed_xyz, rgba=None):
        q = _f32(transformed_xyz); rgba = None if rgba is None else np.ascontiguousarray(rgba, dtype=np.uint8)
        out = np.empty(len(q), MATCH_DTYPE)
        self._ck(self.lib.icp_query_matches(self.h, _ptr(q), _ptr(rgba), C.c_int32(len(q)), _ptr(out)))
        return out

    def match(self, pose):
        out = np.empty(self.n_src, MATCH_DTYPE); d2 = np.empty(self.n_src, np.float32)
        self._ck(self.lib.icp_match(self.h, _ptr(pose_to_c(pose)), _ptr(out), _ptr(d2)))
        return out, d2

    def match_seeded(self, poses):
        """icp_match_seeded: the fused matcher launched once per pose (first unseeded, then seeded + incremental as in the loop);
        returns the last launch's (Match records after weighting / rejection, squared distances) in source order."""
        ps = np.ascontiguousarray(np.stack([pose_to_c(p) for p in poses]), dtype=np.float32)
        out = np.empty(self.n_src, MATCH_DTYPE); d2 = np.empty(self.n_src, np.float32)
        self._ck(self.lib.icp_match_seeded(self.h, _ptr(ps), C.c_int32(len(ps)), _ptr(out), _ptr(d2)))
        return out, d2

    def correspond(self, pose):
        out = np.empty(self.n_src, MATCH_DTYPE); sums = np.zeros(64, np.float64); nv = C.c_int32(0)
        self._ck(self.lib.icp_correspond(self.h, _ptr(pose_to_c(pose)), _ptr(out), _ptr(sums), C.byref(nv)))
        return out, sums, nv.value

    def loop_sums(self, pose, form, iteration=0):
        """icp_debug_loop_sums (test hook, host_debug.hpp): the sums the loop itself reduced in iteration `iteration` of the plan icp_run
        makes, at `pose`, in the form "separate" or "merged".  Returns (sums[64], n_valid, composed pose, route) with route =
        dict(family: 0 k_post / 1 k_knn_bvh_post / 2 k_knn_bvh_post_ring, dim, wide, fault)."""
        sums = np.zeros(64, np.float64); nv = C.c_int32(0); out = np.zeros(16, np.float32); route = (C.c_int32 * 4)()
        self._ck(self.lib.icp_debug_loop_sums(self.h, _ptr(pose_to_c(pose)), C.c_int32(("separate", "merged").index(form)), C.c_int32(iteration),
                                              _ptr(sums), C.byref(nv), _ptr(out), route))
        return sums, nv.value, pose_from_c(out), dict(family=route[0], dim=route[1], wide=route[2], fault=route[3])

    def iterate(self, pose):
        p = pose_to_c(pose); st = IcpIterStats()
        self._ck(self.lib.icp_iterate(self.h, _ptr(p), C.byref(st)))
        return pose_from_c(p), _record(st)

    def run(self, pose, max_stats=512, check=True):
        p = pose_to_c(pose); st = (IcpIterStats * max_stats)(); n = C.c_int32(0)
        rc = self.lib.icp_run(self.h, _ptr(p), st, C.c_int32(max_stats), C.byref(n))
        if check:
            self._ck(rc)
        return pose_from_c(p), [_record(st[i]) for i in range(min(n.value, max_stats))], rc

    def run_multistart(self, poses, max_stats=512):
        """icp_run_multistart: ICP from every pose of `poses` (K x 4 x 4) at once.  Returns (results, stats, best): one dict per start
        (pose, status, n_inliers, fitness, inlier_rmse), the iteration records of each start (a list of record lists, as `run` gives
        them), and the index of the best start."""
        poses = list(poses)
        K = len(poses)
        ps = np.ascontiguousarray(np.stack([pose_to_c(p) for p in poses]) if K else np.zeros((0, 16)), dtype=np.float32)
        res = (IcpStartResult * max(K, 1))(); st = (IcpIterStats * max(K * max_stats, 1))(); n = C.c_int32(0); best = C.c_int32(-1)
        self._ck(self.lib.icp_run_multistart(self.h, _ptr(ps) if K else None, C.c_int32(K), res, st, C.c_int32(max_stats), C.byref(n), C.byref(best)))
        stats = [[_record(r) for r in st[k * max_stats:k * max_stats + min(n.value, max_stats)]] for k in range(K)]
        return [_record(r) for r in res[:K]], stats, best.value

    def run_raw(self, pose_c16):
        """Timed-loop entry for bench.py: pose buffer in/out (column-major float32[16]), no record marshalling."""
        n = C.c_int32(0)
        self._ck(self.lib.icp_run(self.h, _ptr(pose_c16), None, C.c_int32(0), C.byref(n)))
        return n.value

    def timing(self):
        t = IcpTiming()
        self._ck(self.lib.icp_get_timing(self.h, C.byref(t)))
        return _record(t)

    def iteration_times(self, max_out=4096):
        """Per-iteration (match, weight/reject/build, solve) device milliseconds of the last run; -1 = iteration not bracketed."""
        a = np.empty(max_out, np.float32); b = np.empty(max_out, np.float32); d = np.empty(max_out, np.float32); n = C.c_int32(0)
        self._ck(self.lib.icp_get_iteration_times(self.h, _ptr(a), _ptr(b), _ptr(d), C.c_int32(max_out), C.byref(n)))
        k = min(n.value, max_out)
        return a[:k].copy(), b[:k].copy(), d[:k].copy()

    def set_stage_timing(self, every_nth):
        """0: whole-run time only; 1: the stage times of every iteration (default); N > 1: every Nth iteration, scaled.  The merged loop
        reads the device's clock inside its launches (no cost to the run); the other forms bracket their stages with HIP events."""
        self._ck(self.lib.icp_set_stage_timing(self.h, C.c_int32(int(every_nth))))

    def set_convergence_reference(self, src_xyz, ref_xyz):
        s, r = _f32(src_xyz), _f32(ref_xyz)
        self._ck(self.lib.icp_set_convergence_reference(self.h, _ptr(s), _ptr(r), C.c_int32(len(s))))

    def rmse(self, pose):
        out = C.c_float(0)
        self._ck(self.lib.icp_rmse(self.h, _ptr(pose_to_c(pose)), C.byref(out)))
        return out.value

    def benchmark_error(self, pose):
        out = C.c_float(0)
        self._ck(self.lib.icp_benchmark_error(self.h, _ptr(pose_to_c(pose)), C.byref(out)))
        return out.value

    def backproject_depth(self, depth, rgbx, K, extrinsics=None, max_distance=0.1, fix_color_index=False):
        """PointCloud(depthMap, colorFrame, K, extrinsics, w, h, keepOriginalSize=true) on the device (PointCloud.h:78-165)."""
        depth = np.ascontiguousarray(depth, dtype=np.float32); h, w = depth.shape
        K = np.asarray(K, dtype=np.float32); E = pose_to_c(np.eye(4) if extrinsics is None else extrinsics)
        rgbx = None if rgbx is None else np.ascontiguousarray(rgbx, dtype=np.uint8)
        xyz = np.empty((h * w, 3), np.float32); nrm = np.empty((h * w, 3), np.float32)
        rgba = np.empty((h * w, 4), np.uint8) if rgbx is not None else None; valid = np.empty(h * w, np.uint8)
        self._ck(self.lib.icp_backproject_depth(self.h, _ptr(depth), _ptr(rgbx), C.c_float(K[0, 0]), C.c_float(K[1, 1]), C.c_float(K[0, 2]), C.c_float(K[1, 2]),
                                                _ptr(E), C.c_int32(w), C.c_int32(h), C.c_float(max_distance), C.c_int32(int(fix_color_index)),
                                                _ptr(xyz), _ptr(nrm), _ptr(rgba), _ptr(valid)))
        return xyz, nrm, rgba, valid.astype(bool)

    def _set_depth(self, fn, depth, rgbx, cam, opt, check):
        depth = _depth_in(depth, cam)
        rgbx = _rgbx_in(rgbx, depth.size)
        n = C.c_int32(0)
        rc = fn(self.h, _ptr(depth), _ptr(rgbx), C.byref(cam), C.byref(opt), C.byref(n))
        if check:
            self._ck(rc)
        return n.value, rc

    def set_target_depth(self, depth, rgbx, cam, opt, check=True):
        """icp_set_target_depth: PointCloud(depthMap, colorFrame, ...) (PointCloud.h:78-165) built on the device as the target.
        cam / opt: depth_camera(...) / depth_options(...).  Returns the number of kept points (and the status with check=False)."""
        n, rc = self._set_depth(self.lib.icp_set_target_depth, depth, rgbx, cam, opt, check)
        self.n_tgt = n
        return n if check else (n, rc)

    def set_source_depth(self, depth, rgbx, cam, opt, check=True):
        """icp_set_source_depth: the same constructor on the device, as the source."""
        n, rc = self._set_depth(self.lib.icp_set_source_depth, depth, rgbx, cam, opt, check)
        self.n_src = n
        return n if check else (n, rc)

    def set_depth_filter(self, radius=3, sigma_space=4.5, sigma_range=0.03):
        """icp_set_depth_filter_options: the bilateral depth filter in front of every call that aligns a depth frame (DESIGN.md section
        6zd): window (2 radius + 1)^2, radius 1 .. 4; radius=0 switches it off.  Fusion, the depth mesh and the back-projection keep
        reading the raw frame."""
        o = IcpDepthFilterOptions(int(radius), float(sigma_space), float(sigma_range))
        self._ck(self.lib.icp_set_depth_filter_options(self.h, C.byref(o)))
        return o

    def depth_filter_options(self):
        o = IcpDepthFilterOptions()
        self._ck(self.lib.icp_get_depth_filter_options(self.h, C.byref(o)))
        return o

    def filter_depth(self, depth, options=None, **kw):
        """icp_filter_depth: one depth frame (h, w) filtered on the device, host to host.  options: an IcpDepthFilterOptions, or
        `depth_filter_options`' arguments; neither: the context's options (radius 0: a copy of the frame)."""
        d = np.ascontiguousarray(depth, dtype=np.float32)
        if d.ndim != 2:
            raise ValueError("the depth frame must be a (height, width) image")
        o = options if options is not None else (depth_filter_options(**kw) if kw else None)
        out = np.empty_like(d)
        self._ck(self.lib.icp_filter_depth(self.h, _ptr(d), C.c_int32(d.shape[1]), C.c_int32(d.shape[0]), None if o is None else C.byref(o), _ptr(out)))
        return out

    def track_depth_frames(self, depth_frames, rgbx_frames, cam, target_opt, source_opt, gt=None, pose=None):
        """icp_track_depth_frames: reconstructRoom's tracking loop (main.cpp:183-341) over frames (n, h, w) [+ colours (n, h*w, 4)].
        gt: (n - 1) 4x4 transforms frame k -> frame 0, or None.  pose: initial currentCameraToWorld (identity by default).
        Returns (final pose, list of per-frame records for frames 1 .. n-1, status)."""
        d = _depth_in(depth_frames, cam, sequence=True)
        nf = d.shape[0]
        cols = _rgbx_in(rgbx_frames, d.size, "colour frames must hold 4 bytes per pixel")
        g = _gt_in(gt, nf)
        p = pose_to_c(np.eye(4) if pose is None else pose)
        out = (IcpTrackFrame * max(nf - 1, 1))()
        rc = self.lib.icp_track_depth_frames(self.h, _ptr(d), _ptr(cols), C.c_int32(nf), C.byref(cam), C.byref(target_opt), C.byref(source_opt),
                                             _ptr(g), _ptr(p), out)
        if rc not in (ICP_OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # per-frame outcomes: reported in the records
            self._ck(rc)
        return pose_from_c(p), [_record(out[i]) for i in range(nf - 1)], rc

    def depth_mesh(self, depth, rgbx, cam, camera_pose, edge_threshold=0.01, color_cam=None):
        """icp_depth_mesh: SimpleMesh(sensor, cameraPose, edgeThreshold) (SimpleMesh.h:36-119) on the device.  depth: the frame of `cam`;
        rgbx: the RGBX colour frame (color_cam's size, or the depth frame's when color_cam is None), or None for no colours;
        camera_pose: 4x4 world -> camera.  Returns (vertices (w*h, 3) f32, colours (w*h, 4) u8 or None, triangles (T, 3) u32)."""
        depth = _depth_in(depth, cam)
        n_color = (color_cam.width * color_cam.height) if color_cam is not None else depth.size
        rgbx = _rgbx_in(rgbx, n_color, "colour frame must hold 4 bytes per pixel of the colour camera")
        n = depth.size
        verts = np.empty((n, 3), np.float32)
        cols = np.empty((n, 4), np.uint8) if rgbx is not None else None
        tris = np.empty((2 * max(cam.width - 1, 0) * max(cam.height - 1, 0), 3), np.uint32)
        nt = C.c_int32(0)
        self._ck(self.lib.icp_depth_mesh(self.h, _ptr(depth), _ptr(rgbx), C.byref(cam), None if color_cam is None else C.byref(color_cam),
                                         _ptr(pose_to_c(camera_pose)), C.c_float(edge_threshold), _ptr(verts), _ptr(cols), _ptr(tris), C.byref(nt)))
        return verts, cols, tris[:nt.value]

    def tsdf_create(self, options=None, color=False, **kw):
        """icp_tsdf_create: the context's TSDF volume (frame-to-model tracking), allocated and cleared.  options: an IcpTsdfOptions, or
        the arguments of `tsdf_options` (dims, origin, voxel_size, truncation, max_weight, min_depth, max_depth, ray_step).
        color: also icp_tsdf_color_create, the colour array (16 more bytes per voxel)."""
        o = options if options is not None else tsdf_options(**kw)
        self._ck(self.lib.icp_tsdf_create(self.h, C.byref(o)))
        self._tsdf_dims = tuple(o.dims)
        self._tsdf_origin = tuple(o.origin)
        if color:
            self.tsdf_color_create()

    def tsdf_create_hashed(self, options=None, block_capacity=1 << 12, color=False, **kw):
        """icp_tsdf_create_hashed: the context's TSDF volume stored in 8 x 8 x 8 voxel blocks behind a hash table, without an extent
        (DESIGN.md section 6x); `tsdf_options`' arguments without dims (origin, voxel_size, truncation, ...).  block_capacity: blocks of 4 KiB
        the pool holds before it grows (it doubles on the device when a frame needs more).  Replaces any volume, dense or hashed.
        `tsdf_integrate`, `tsdf_sample`, `tsdf_sdf_system`, `tsdf_align_depth` and `track_depth_sdf` work on it as on a dense one.
        color: icp_tsdf_create_color_hashed, the blocks with colours (8 KiB more per block); `tsdf_integrate` with
        rgbx, `tsdf_sample_color` and the calls above with color_weight > 0 then work on it as on a dense coloured volume."""
        o = options if options is not None else tsdf_options(**kw)
        create = self.lib.icp_tsdf_create_color_hashed if color else self.lib.icp_tsdf_create_hashed
        self._ck(create(self.h, C.byref(o), C.c_int32(block_capacity)))
        self._tsdf_dims = None
        self._tsdf_origin = tuple(o.origin)
        self.tsdf_hashed_options = o

    def tsdf_has_color(self):
        """icp_tsdf_hashed_has_color: whether the context's hashed volume holds colours."""
        has = C.c_int32(0)
        self._ck(self.lib.icp_tsdf_hashed_has_color(self.h, C.byref(has)))
        return bool(has.value)

    def tsdf_reserve_blocks(self, block_capacity):
        """icp_tsdf_reserve_blocks: grows the hashed volume's table and pool ahead of time (smaller or equal: nothing happens)."""
        self._ck(self.lib.icp_tsdf_reserve_blocks(self.h, C.c_int32(block_capacity)))

    def tsdf_allocate_blocks(self, coords):
        """icp_tsdf_allocate_blocks: allocates the blocks `coords` (n, 3) of the hashed volume (allocated already: no effect)."""
        cc = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 3)
        self._ck(self.lib.icp_tsdf_allocate_blocks(self.h, C.c_int32(len(cc)), _ptr(cc)))

    def tsdf_blocks(self, colors=False):
        """icp_get_tsdf_hashed: (info dict(n_blocks, capacity, n_grown, n_unplaced, n_out_of_range), coords (B, 3) int32, tsdf (B, 8, 8, 8),
        weight (B, 8, 8, 8) float32, indexed [z, y, x]) of the allocated blocks, sorted by key (z, then y, then x of the block).
        colors: icp_get_tsdf_color_hashed, with rgb (B, 8, 8, 8, 3) and cweight (B, 8, 8, 8) of a coloured hashed volume behind them."""
        info = IcpTsdfHashedInfo()
        self._ck(self.lib.icp_get_tsdf_hashed(self.h, C.byref(info), C.c_int32(0), None, None, None))
        n = info.n_blocks
        coords = np.empty((n, 3), np.int32); t = np.empty((n, 8, 8, 8), np.float32); w = np.empty((n, 8, 8, 8), np.float32)
        if colors:
            rgb = np.empty((n, 8, 8, 8, 3), np.float32); cw = np.empty((n, 8, 8, 8), np.float32)
            self._ck(self.lib.icp_get_tsdf_color_hashed(self.h, C.byref(info), C.c_int32(n), _ptr(coords), _ptr(t), _ptr(w), _ptr(rgb), _ptr(cw)))
            return {k: getattr(info, k) for k, _ in info._fields_}, coords, t, w, rgb, cw
        self._ck(self.lib.icp_get_tsdf_hashed(self.h, C.byref(info), C.c_int32(n), _ptr(coords), _ptr(t), _ptr(w)))
        return {k: getattr(info, k) for k, _ in info._fields_}, coords, t, w

    @staticmethod
    def _blocks_in(coords, tsdf, weight, rgb, cweight):
        cc = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 3)
        t = _f32(tsdf).reshape(-1, 8, 8, 8); w = _f32(weight).reshape(-1, 8, 8, 8)
        if not (len(cc) == len(t) == len(w)):
            raise ValueError("coords (B, 3), tsdf and weight (B, 8, 8, 8) must agree in B")
        if (rgb is None) != (cweight is None):
            raise ValueError("rgb and cweight go together")
        if rgb is None:
            return cc, t, w, None, None
        c = _f32(rgb).reshape(-1, 8, 8, 8, 3); cw = _f32(cweight).reshape(-1, 8, 8, 8)
        if not (len(cc) == len(c) == len(cw)):
            raise ValueError("coords (B, 3), rgb (B, 8, 8, 8, 3) and cweight (B, 8, 8, 8) must agree in B")
        return cc, t, w, c, cw

    def tsdf_upload_blocks(self, coords, tsdf, weight, rgb=None, cweight=None):
        """icp_tsdf_upload_hashed: replaces the hashed volume's state by the blocks `coords` (B, 3) with `tsdf` and `weight` (B, 8, 8, 8).
        rgb (B, 8, 8, 8, 3) and cweight (B, 8, 8, 8): icp_tsdf_upload_color_hashed, the blocks with their colours (a coloured volume);
        without them a coloured volume's blocks are left uncoloured."""
        cc, t, w, c, cw = self._blocks_in(coords, tsdf, weight, rgb, cweight)
        if c is not None:
            self._ck(self.lib.icp_tsdf_upload_color_hashed(self.h, C.c_int32(len(cc)), _ptr(cc), _ptr(t), _ptr(w), _ptr(c), _ptr(cw)))
        else:
            self._ck(self.lib.icp_tsdf_upload_hashed(self.h, C.c_int32(len(cc)), _ptr(cc), _ptr(t), _ptr(w)))

    def tsdf_evict_blocks(self, centre, radius, hold=True):
        """icp_tsdf_evict_blocks: every block of the hashed volume whose centre lies beyond `radius` metres of `centre` leaves the device
        (DESIGN.md section 6za).  Returns (info dict(n_evicted, n_blocks, n_moved, capacity, n_held, n_inserted, n_present, n_grown),
        coords (E, 3) int32, tsdf (E, 8, 8, 8), weight (E, 8, 8, 8)): the evicted blocks sorted by key (icp_tsdf_evicted_blocks), for the
        caller to keep; with hold=False they are forgotten and the arrays are empty.  On a coloured hashed volume this returns the outbox's
        geometry; `tsdf_evict_blocks_color` returns the colours too."""
        return self._evict_blocks(centre, radius, hold, False)

    def tsdf_evict_blocks_color(self, centre, radius, hold=True):
        """`tsdf_evict_blocks` on a coloured hashed volume with the colours of the evicted blocks (icp_tsdf_evicted_blocks_color): returns
        (info, coords, tsdf, weight, rgb (E, 8, 8, 8, 3), cweight (E, 8, 8, 8)).  A volume without colours is a ValueError."""
        return self._evict_blocks(centre, radius, hold, True)

    def _evict_blocks(self, centre, radius, hold, colors):
        ce = _f32(centre).reshape(-1)
        if ce.size != 3:
            raise ValueError("centre is three numbers")
        info = IcpTsdfStreamInfo()
        self._ck(self.lib.icp_tsdf_evict_blocks(self.h, _ptr(ce), C.c_float(radius), C.c_int32(1 if hold else 0), C.byref(info)))
        n = info.n_held
        coords = np.empty((n, 3), np.int32); t = np.empty((n, 8, 8, 8), np.float32); w = np.empty((n, 8, 8, 8), np.float32)
        if colors:
            if not self.tsdf_has_color():
                raise ValueError("tsdf_evict_blocks_color needs a coloured hashed volume (tsdf_create_hashed(color=True))")
            rgb = np.zeros((n, 8, 8, 8, 3), np.float32); cw = np.zeros((n, 8, 8, 8), np.float32)
            if n:
                self._ck(self.lib.icp_tsdf_evicted_blocks_color(self.h, C.c_int32(n), _ptr(coords), _ptr(t), _ptr(w), _ptr(rgb), _ptr(cw)))
            return {k: getattr(info, k) for k, _ in info._fields_}, coords, t, w, rgb, cw
        if n:
            self._ck(self.lib.icp_tsdf_evicted_blocks(self.h, C.c_int32(n), _ptr(coords), _ptr(t), _ptr(w)))
        return {k: getattr(info, k) for k, _ in info._fields_}, coords, t, w

    def tsdf_insert_blocks(self, coords, tsdf, weight):
        """icp_tsdf_insert_blocks: ADDS the blocks `coords` (B, 3) with `tsdf` and `weight` (B, 8, 8, 8) to the hashed volume's state
        (`tsdf_upload_blocks` replaces it); a block that is resident already refuses the call.  Returns the info dict of `tsdf_evict_blocks`.
        On a coloured hashed volume the new blocks are uncoloured; `tsdf_insert_blocks_color` inserts them with their colours."""
        return self._insert_blocks(coords, tsdf, weight, None, None)

    def tsdf_insert_blocks_color(self, coords, tsdf, weight, rgb, cweight):
        """icp_tsdf_insert_blocks_color: `tsdf_insert_blocks` on a coloured hashed volume, the blocks with their colours rgb (B, 8, 8, 8, 3)
        and cweight (B, 8, 8, 8)."""
        if rgb is None or cweight is None:
            raise ValueError("tsdf_insert_blocks_color takes rgb and cweight")
        return self._insert_blocks(coords, tsdf, weight, rgb, cweight)

    def _insert_blocks(self, coords, tsdf, weight, rgb, cweight):
        cc, t, w, c, cw = self._blocks_in(coords, tsdf, weight, rgb, cweight)
        info = IcpTsdfStreamInfo()
        if c is not None:
            self._ck(self.lib.icp_tsdf_insert_blocks_color(self.h, C.c_int32(len(cc)), _ptr(cc), _ptr(t), _ptr(w), _ptr(c), _ptr(cw), C.byref(info)))
        else:
            self._ck(self.lib.icp_tsdf_insert_blocks(self.h, C.c_int32(len(cc)), _ptr(cc), _ptr(t), _ptr(w), C.byref(info)))
        return {k: getattr(info, k) for k, _ in info._fields_}

    def tsdf_color_create(self):
        """icp_tsdf_color_create: the volume's colour array, one (R, G, B, Wc) per voxel, allocated and cleared (called again: cleared)."""
        self._ck(self.lib.icp_tsdf_color_create(self.h))

    def tsdf_color_release(self):
        self._ck(self.lib.icp_tsdf_color_release(self.h))

    def tsdf_color_volume(self):
        """icp_tsdf_color_download: (rgb (nz, ny, nx, 3), weight (nz, ny, nx)), float32; rgb holds running averages of byte values 0..255."""
        shape = self._tsdf_shape()
        rgb = np.empty(shape + (3,), np.float32); w = np.empty(shape, np.float32)
        self._ck(self.lib.icp_tsdf_color_download(self.h, _ptr(rgb), _ptr(w)))
        return rgb, w

    def tsdf_color_upload(self, rgb, weight):
        """icp_tsdf_color_upload: replaces the colour array's contents (nx*ny*nz x 3 and nx*ny*nz values, x fastest)."""
        shape = self._tsdf_shape()
        c, w = _f32(rgb), _f32(weight)
        if w.size != np.prod(shape) or c.size != 3 * w.size:
            raise ValueError("the arrays must hold nx * ny * nz x 3 and nx * ny * nz values")
        self._ck(self.lib.icp_tsdf_color_upload(self.h, _ptr(c), _ptr(w)))

    def tsdf_reset(self):
        self._ck(self.lib.icp_tsdf_reset(self.h))

    def tsdf_release(self):
        self._ck(self.lib.icp_tsdf_release(self.h))
        self._tsdf_dims = None

    def _tsdf_shape(self):
        d = getattr(self, "_tsdf_dims", None)
        if d is None:
            raise IcpError(1, "no TSDF volume (tsdf_create)")
        return (d[2], d[1], d[0])

    def tsdf_volume(self):
        """icp_tsdf_download: (tsdf, weight), two float32 arrays of shape (nz, ny, nx) (x fastest)."""
        shape = self._tsdf_shape()
        t = np.empty(shape, np.float32); w = np.empty(shape, np.float32)
        self._ck(self.lib.icp_tsdf_download(self.h, _ptr(t), _ptr(w)))
        return t, w

    def tsdf_upload(self, tsdf, weight):
        """icp_tsdf_upload: replaces the volume's contents (two arrays of nx*ny*nz values, x fastest)."""
        shape = self._tsdf_shape()
        t, w = _f32(tsdf), _f32(weight)
        if t.size != np.prod(shape) or w.size != t.size:
            raise ValueError("the arrays must hold nx * ny * nz values")
        self._ck(self.lib.icp_tsdf_upload(self.h, _ptr(t), _ptr(w)))

    def tsdf_integrate(self, depth, cam, pose, rgbx=None):
        """icp_tsdf_integrate: fuses one depth frame, seen from `pose` (4x4 camera -> world), into the volume.  Returns the voxels written.
        rgbx (h*w x 4 bytes, the depth frame's size): icp_tsdf_integrate_color, the frame's colours into the colour array as well; returns
        (voxels written, voxels coloured)."""
        depth = _depth_in(depth, cam)
        n = C.c_int32(0)
        if rgbx is not None:
            cols = _rgbx_in(rgbx, depth.size, "colour frame must hold 4 bytes per pixel of the depth frame")
            nc = C.c_int32(0)
            self._ck(self.lib.icp_tsdf_integrate_color(self.h, _ptr(depth), _ptr(cols), C.byref(cam), _ptr(pose_to_c(pose)), C.byref(n), C.byref(nc)))
            return n.value, nc.value
        self._ck(self.lib.icp_tsdf_integrate(self.h, _ptr(depth), C.byref(cam), _ptr(pose_to_c(pose)), C.byref(n)))
        return n.value

    @_colouring("color", _integrate_cloud_color)
    def tsdf_integrate_cloud(self, which="source", pose=None, sensor_origin=None):
        """icp_tsdf_integrate_cloud: fuses the resident target ("target" / 0) or source ("source" / 1) -- an unorganised cloud in its sensor
        frame, a laser scan -- into the volume, dense or hashed, as one observation.  pose: 4x4 scan frame -> world
        (None: the identity); sensor_origin: the ray origin in the scan frame (None: (0, 0, 0)).  Geometry only (unless color=True, below): the colours of a coloured
        volume stay as they are.  Returns dict(n_points, n_rays, n_updated, n_blocks, n_samples, n_outside).
        color=True (keyword only): icp_tsdf_integrate_cloud_color -- the volume has colours (`tsdf_create(color=True)`,
        `tsdf_create_hashed(color=True)`) and the cloud was set with rgba; the scan's colours are fused with its geometry (DESIGN.md
        section 6zh) and the dict gains n_colored."""
        w, p, e = _cloud_fuse_in(which, pose, sensor_origin)
        info = IcpTsdfCloudInfo()
        self._ck(self.lib.icp_tsdf_integrate_cloud(self.h, C.c_int32(w), _ptr(p), _ptr(e), C.byref(info)))
        return _record(info)

    def set_tsdf_carve(self, distance=0.0, min_range=0.0):
        """icp_set_tsdf_carve_options: free space carved by every cloud fuse (`tsdf_integrate_cloud`, the fuses of `track_scans_sdf`;
        DESIGN.md section 6zg): the voxels up to `distance` metres in front of each return's band (inf: back to the sensor) are observed
        as free wherever the volume has storage; carve samples nearer to the sensor than `min_range` are skipped.  distance=0 (the
        default) switches it off.  Setting the options clears the stats."""
        o = IcpTsdfCarveOptions(float(distance), float(min_range))
        self._ck(self.lib.icp_set_tsdf_carve_options(self.h, C.byref(o)))
        return o

    def tsdf_carve_options(self):
        o = IcpTsdfCarveOptions()
        self._ck(self.lib.icp_get_tsdf_carve_options(self.h, C.byref(o)))
        return o

    def tsdf_carve_stats(self):
        """icp_tsdf_carve_stats: dict(n_steps: J of the last cloud fuse, n_carved: its applied carve observations, n_carved_total: the
        same since the options were last set)."""
        o = IcpTsdfCarveInfo()
        self._ck(self.lib.icp_tsdf_carve_stats(self.h, C.byref(o)))
        return dict(n_steps=o.n_steps, n_carved=o.n_carved, n_carved_total=o.n_carved_total)

    @_photometric(_tsdf_cloud_system_color)
    def tsdf_cloud_system(self, which="source", pose=None, huber=0.0):
        """icp_tsdf_cloud_system: the 28 sums of one direct SDF step of the resident target ("target" / 0) or source ("source" / 1) -- an
        unorganised cloud in its sensor frame -- at `pose` (4x4 scan frame -> world; None: the identity) against the volume, dense or
        hashed.  Returns (sums (28,) float64, (considered, valid)).
        color_weight, color_huber (keyword only, 0.0 each): a positive weight, in metres per unit of intensity, adds the photometric row
        of a coloured cloud against a coloured volume (icp_tsdf_cloud_system_color); the return is then
        (sums (29,), (considered, valid, colored)).  A weight of zero changes nothing."""
        w = _cloud(which)
        p = _pose_in(np.eye(4, dtype=np.float32) if pose is None else pose)
        o = sdf_options(huber=huber)
        sums = np.empty(28, np.float64); cnt = (C.c_int32 * 2)()
        self._ck(self.lib.icp_tsdf_cloud_system(self.h, C.c_int32(w), _ptr(p), C.byref(o), _ptr(sums), cnt))
        return sums, (cnt[0], cnt[1])

    @_photometric(_tsdf_align_cloud_color)
    def tsdf_align_cloud(self, which="source", pose=None, n_iterations=20, huber=0.0, min_valid=64, stop_rotation=1e-5, stop_translation=1e-5, trace=False):
        """icp_tsdf_align_cloud: the resident cloud aligned to the volume itself from `pose` (identity by default): no target cloud, no
        index, no search.  The field exists only inside the truncation band around the fused surfaces: a point that starts further
        than the truncation from all of them takes no part (the basin).  `tsdf_align_depth`'s returns: (pose, record, status), with trace=True (pose, record,
        status, the records of the iterations that ran); a failed alignment (status NO_SOURCE or NO_CORRESPONDENCES) returns the pose it
        started with.  color_weight, color_huber (keyword only, 0.0 each): a positive weight aligns a coloured cloud to a coloured volume
        with the photometric term (icp_tsdf_align_cloud_color, DESIGN.md section 6zj: what pins a scan of a flat textured wall); the
        records are then the colour records.  A weight of zero changes nothing."""
        w = _cloud(which)
        p = _pose_in(np.eye(4, dtype=np.float32) if pose is None else pose)
        o = sdf_options(n_iterations=n_iterations, huber=huber, min_valid=min_valid, stop_rotation=stop_rotation, stop_translation=stop_translation)
        rec = IcpSdfFrame(); tr = (IcpSdfIter * o.n_iterations)() if trace else None
        rc = self.lib.icp_tsdf_align_cloud(self.h, C.c_int32(w), C.byref(o), _ptr(p), C.byref(rec), tr)
        if rc not in (ICP_OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # the alignment's outcome: reported in the record
            self._ck(rc)
        r = _record(rec)
        if trace:
            return pose_from_c(p), r, rc, [_record(tr[i]) for i in range(r["iterations"])]
        return pose_from_c(p), r, rc

    @_colouring("colors", _track_scans_sdf)
    def track_scans_sdf(self, scans, pose=None, **options):
        """icp_track_scans_sdf: `scans`, a list of xyz (n, 3) arrays in the sensor frame (a (xyz, normals) pair as `track_scans_vmap`
        takes it will do, the normals are not used), tracked against the TSDF volume they are fused into: scan 0 fused at `pose`
        (identity by default), every later scan aligned to the volume built so far (**options: the fields of `sdf_options`) and, when
        that succeeds, fused at the pose found; a scan that fails is skipped and carries the pose.  Returns (poses: one 4x4 per scan,
        the records of scans 1 .., the fuse info of every scan -- all zero for a skipped one --, status: the first per-scan error, or 0).
        colors (keyword only): one rgba (n, 4) uint8 array per scan -- icp_track_scans_sdf_color on a coloured volume: every scan goes up
        with its colours and every fuse is the coloured one; poses, records and infos are the uncoloured loop's,
        and the tuple gains a fifth value, n_colored of every scan (0 for a skipped one).  color_weight, color_huber (among **options,
        0.0 each): with colors, a positive weight makes every alignment the photometric one (icp_track_scans_sdf_photometric, DESIGN.md
        section 6zj) and the records the colour records; without colors it raises ValueError.  A weight of zero changes nothing."""
        return _track_scans_sdf(self, None, scans, pose, **options)

    def tsdf_raycast(self, cam, pose):
        """icp_tsdf_raycast: the volume seen from `pose` as an organised cloud in that camera's frame.  Returns (depth (h, w), vertices
        (w*h, 3), normals (w*h, 3), number of hits); holes are MINF.  The depth image is a valid input of `depth_mesh`."""
        n = cam.width * cam.height
        d = np.empty((cam.height, cam.width), np.float32); v = np.empty((n, 3), np.float32); nr = np.empty((n, 3), np.float32); hits = C.c_int32(0)
        self._ck(self.lib.icp_tsdf_raycast(self.h, C.byref(cam), _ptr(pose_to_c(pose)), _ptr(d), _ptr(v), _ptr(nr), C.byref(hits)))
        return d, v, nr, hits.value

    def tsdf_raycast_color(self, cam, pose):
        """icp_tsdf_raycast_color: `tsdf_raycast` with the colour of every hit.  Returns (depth, vertices, normals, rgba (w*h, 4) u8, hits,
        coloured hits); a hole or a hit without colour is four zero bytes, a coloured pixel has alpha 255."""
        n = cam.width * cam.height
        d = np.empty((cam.height, cam.width), np.float32); v = np.empty((n, 3), np.float32); nr = np.empty((n, 3), np.float32)
        rgba = np.empty((n, 4), np.uint8); hits, ncol = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.icp_tsdf_raycast_color(self.h, C.byref(cam), _ptr(pose_to_c(pose)), _ptr(d), _ptr(v), _ptr(nr), _ptr(rgba), C.byref(hits), C.byref(ncol)))
        return d, v, nr, rgba, hits.value, ncol.value

    def mesh_cluster(self, vertices, triangles, cell_size, normals=None, colors=None, origin=(0, 0, 0)):
        """icp_mesh_cluster: vertex clustering of an indexed triangle mesh on the device: the vertices of one cell of
        a grid of `cell_size` with a corner at `origin` become one vertex, triangles that lose a corner are dropped, equal ones kept once.
        vertices (V, 3) f32, triangles (T, 3) u32, normals (V, 3) f32 and colors (V, 4) u8 optional.  One call with capacities V and T,
        then slices.  Returns (vertices, normals | None, colors | None, triangles, info dict)."""
        v = _f32(vertices).reshape(-1, 3); t = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        n = None if normals is None else _f32(normals).reshape(-1, 3)
        col = None if colors is None else np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 4)
        if (n is not None and len(n) != len(v)) or (col is not None and len(col) != len(v)):
            raise ValueError("normals and colors need one row per vertex")
        ov = np.empty((len(v), 3), np.float32); ot = np.empty((len(t), 3), np.uint32)
        on = None if n is None else np.empty((len(v), 3), np.float32); oc = None if col is None else np.empty((len(v), 4), np.uint8)
        info = IcpMeshClusterInfo()
        self._ck(self.lib.icp_mesh_cluster(self.h, len(v), len(t), _ptr(v), _ptr(n), _ptr(col), _ptr(t), C.byref(mesh_cluster_options(cell_size, origin)), len(v), len(t),
                                           _ptr(ov), _ptr(on), _ptr(oc), _ptr(ot), C.byref(info)))
        self._mc_info = _record(info)
        nv, nt = info.n_vertices, info.n_triangles
        return ov[:nv], None if on is None else on[:nv], None if oc is None else oc[:nv], ot[:nt], dict(self._mc_info)

    def mesh_cluster_info(self):
        """The info of the last clustering call on this context (`mesh_cluster`, or a mesh call with `cluster`), as a dict; None before one."""
        info = getattr(self, "_mc_info", None)
        return None if info is None else dict(info)

    def _tsdf_mesh_clustered(self, min_weight, normals, colors, cluster, cluster_origin):
        """icp_tsdf_mesh_clustered (a counting call, then a filling call): the tuple shape of `tsdf_mesh` / `tsdf_mesh_hashed`."""
        origin = cluster_origin if cluster_origin is not None else (getattr(self, "_tsdf_origin", None) or (0.0, 0.0, 0.0))
        opt = mesh_cluster_options(cluster, origin)
        nv, nt, info = C.c_int32(0), C.c_int32(0), IcpMeshClusterInfo()

        def call(v, n, col, t):
            self._ck(self.lib.icp_tsdf_mesh_clustered(self.h, float(min_weight), C.byref(opt), int(bool(colors)), nv.value, nt.value, _ptr(v), _ptr(n), _ptr(col), _ptr(t),
                                                      C.byref(nv), C.byref(nt), C.byref(info)))
        call(None, None, None, None)
        v = np.empty((nv.value, 3), np.float32); n = np.empty((nv.value, 3), np.float32) if normals else None; t = np.empty((nt.value, 3), np.uint32)
        col = np.empty((nv.value, 4), np.uint8) if colors else None
        if nv.value or nt.value:
            call(v, n, col, t)
        self._mc_info = _record(info)
        return (v, n, t, col) if colors else (v, n, t)

    @_clustering("colors")
    def tsdf_mesh(self, min_weight=0.0, colors=False):
        """icp_tsdf_mesh: the zero level set of the volume as an indexed triangle mesh, extracted on the device (a counting call, then a
        filling call).  min_weight: voxels below this weight count as unobserved.  Returns (vertices (V, 3) f32 in the world frame,
        normals (V, 3) f32 pointing into free space, triangles (T, 3) u32, counter-clockwise seen from free space).
        colors: icp_tsdf_mesh_color; a fourth array, (V, 4) u8 RGBA per vertex (four zero bytes where the volume holds no colour).
        cluster, cluster_origin (keyword only; cluster is a cell size in metres): icp_tsdf_mesh_clustered, the same tuple with the mesh clustered on the device (DESIGN.md section
        6zk), the grid's origin at cluster_origin (the volume's by default); `mesh_cluster_info` has the counts.  None: exactly the calls above."""
        nv, nt = C.c_int32(0), C.c_int32(0)
        fn = self.lib.icp_tsdf_mesh_color if colors else self.lib.icp_tsdf_mesh

        def call(v, n, col, t):                             # the colour array sits between the normals and the triangles
            bufs = [_ptr(v), _ptr(n)] + ([_ptr(col)] if colors else []) + [_ptr(t)]
            self._ck(fn(self.h, C.c_float(min_weight), C.c_int32(nv.value), C.c_int32(nt.value), *bufs, C.byref(nv), C.byref(nt)))
        call(None, None, None, None)
        v = np.empty((nv.value, 3), np.float32); n = np.empty((nv.value, 3), np.float32); t = np.empty((nt.value, 3), np.uint32)
        col = np.empty((nv.value, 4), np.uint8)
        if nv.value or nt.value:
            call(v, n, col, t)
        return (v, n, t, col) if colors else (v, n, t)

    @_clustering("normals", "colors")
    def tsdf_mesh_hashed(self, min_weight=0.0, normals=True, colors=False):
        """icp_tsdf_mesh_hashed: the zero level set of the HASHED volume as an indexed triangle mesh, extracted on the block pool (a counting
        call, then a filling call).  The volume stays as it is.  Returns (vertices (V, 3) f32, normals (V, 3) f32 --
        None with normals=False --, triangles (T, 3) u32); vertices in ascending (block in key order, local voxel, edge code), so the arrays
        do not depend on where the blocks sit in the pool.
        colors: icp_tsdf_mesh_color_hashed on a coloured hashed volume; a fourth array, (V, 4) u8 RGBA per vertex
        (four zero bytes where neither end of the vertex's edge holds a colour).
        cluster, cluster_origin (keyword only): as in `tsdf_mesh` -- icp_tsdf_mesh_clustered on the hashed volume, the same tuple shape."""
        min_weight = float(min_weight)
        if not (np.isfinite(min_weight) and min_weight >= 0.0):
            raise ValueError("min_weight must be finite and >= 0")
        nv, nt = C.c_int32(0), C.c_int32(0)
        fn = self.lib.icp_tsdf_mesh_color_hashed if colors else self.lib.icp_tsdf_mesh_hashed

        def call(v, n, col, t):                             # the colour array sits between the normals and the triangles
            bufs = [_ptr(v), _ptr(n)] + ([_ptr(col)] if colors else []) + [_ptr(t)]
            self._ck(fn(self.h, C.c_float(min_weight), C.c_int32(nv.value), C.c_int32(nt.value), *bufs, C.byref(nv), C.byref(nt)))
        call(None, None, None, None)
        v = np.empty((nv.value, 3), np.float32); n = np.empty((nv.value, 3), np.float32) if normals else None; t = np.empty((nt.value, 3), np.uint32)
        col = np.empty((nv.value, 4), np.uint8)
        if nv.value or nt.value:
            call(v, n, col, t)
        return (v, n, t, col) if colors else (v, n, t)

    def set_target_tsdf(self, cam, pose, check=True, color=False):
        """icp_set_target_tsdf: the ray-cast of the volume from `pose` as the target (organised, with normals).  Returns the number of hits
        (and the status with check=False).  color: icp_set_target_tsdf_color, the target with colours; hits without a colour become holes
        and the coloured hits are returned."""
        n = C.c_int32(0)
        fn = self.lib.icp_set_target_tsdf_color if color else self.lib.icp_set_target_tsdf
        rc = fn(self.h, C.byref(cam), _ptr(pose_to_c(pose)), C.byref(n))
        if check:
            self._ck(rc)
        self.n_tgt = cam.width * cam.height if rc == ICP_OK else 0
        return n.value if check else (n.value, rc)

    def track_depth_model(self, depth_frames, cam, source_opt, gt=None, pose=None, rgbx_frames=None):
        """icp_track_depth_model: frame-to-model tracking over frames (n, h, w) against the context's TSDF volume.  gt: (n - 1) 4x4 transforms
        frame k -> world, or None.  pose: the camera -> world pose of frame 0 (identity by default).  Returns (final pose, records, status).
        rgbx_frames (n, h*w, 4): icp_track_depth_model_color, the coloured model (needs the colour array and source_opt.fix_color_index)."""
        d = _depth_in(depth_frames, cam, sequence=True)
        nf = d.shape[0]
        g = _gt_in(gt, nf)
        p = pose_to_c(np.eye(4) if pose is None else pose)
        out = (IcpTrackFrame * max(nf - 1, 1))()
        if rgbx_frames is not None:
            cols = _rgbx_in(rgbx_frames, d.size, "colour frames must hold 4 bytes per pixel")
            rc = self.lib.icp_track_depth_model_color(self.h, _ptr(d), _ptr(cols), C.c_int32(nf), C.byref(cam), C.byref(source_opt), _ptr(g), _ptr(p), out)
        else:
            rc = self.lib.icp_track_depth_model(self.h, _ptr(d), C.c_int32(nf), C.byref(cam), C.byref(source_opt), _ptr(g), _ptr(p), out)
        if rc not in (ICP_OK, ERR_NO_TARGET, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # per-frame outcomes: reported in the records
            self._ck(rc)
        return pose_from_c(p), [_record(out[i]) for i in range(nf - 1)], rc

    def tsdf_raycast_hashed(self, cam, pose):
        """icp_tsdf_raycast_hashed: `tsdf_raycast` on the HASHED volume, read where the blocks lie: no dense box is
        built and the volume stays as it is.  Returns (depth (h, w), vertices (w*h, 3), normals (w*h, 3), number of hits); holes are MINF.
        The depth image is a valid input of `depth_mesh`."""
        p = _pose_in(pose)
        n = cam.width * cam.height
        d = np.empty((cam.height, cam.width), np.float32); v = np.empty((n, 3), np.float32); nr = np.empty((n, 3), np.float32); hits = C.c_int32(0)
        self._ck(self.lib.icp_tsdf_raycast_hashed(self.h, C.byref(cam), _ptr(p), _ptr(d), _ptr(v), _ptr(nr), C.byref(hits)))
        return d, v, nr, hits.value

    def tsdf_raycast_color_hashed(self, cam, pose):
        """icp_tsdf_raycast_color_hashed: `tsdf_raycast_hashed` on a coloured hashed volume with the colour of every hit (DESIGN.md section
        6zc).  Returns (depth, vertices, normals, rgba (w*h, 4) u8, hits, coloured hits); a hole or a hit without colour is four zero
        bytes, a coloured pixel has alpha 255."""
        p = _pose_in(pose)
        n = cam.width * cam.height
        d = np.empty((cam.height, cam.width), np.float32); v = np.empty((n, 3), np.float32); nr = np.empty((n, 3), np.float32)
        rgba = np.empty((n, 4), np.uint8); hits, ncol = C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.icp_tsdf_raycast_color_hashed(self.h, C.byref(cam), _ptr(p), _ptr(d), _ptr(v), _ptr(nr), _ptr(rgba), C.byref(hits), C.byref(ncol)))
        return d, v, nr, rgba, hits.value, ncol.value

    def set_target_tsdf_hashed(self, cam, pose, check=True, color=False):
        """icp_set_target_tsdf_hashed: the ray-cast of the HASHED volume from `pose` as the target (organised, with normals).  Returns the
        number of hits (and the status with check=False).  color: icp_set_target_tsdf_color_hashed, the target with colours from a coloured
        hashed volume; hits without a colour become holes and the coloured hits are returned."""
        p = _pose_in(pose)
        n = C.c_int32(0)
        fn = self.lib.icp_set_target_tsdf_color_hashed if color else self.lib.icp_set_target_tsdf_hashed
        rc = fn(self.h, C.byref(cam), _ptr(p), C.byref(n))
        if check:
            self._ck(rc)
        self.n_tgt = cam.width * cam.height if rc == ICP_OK else 0
        return n.value if check else (n.value, rc)

    def track_depth_model_hashed(self, depth_frames, cam, source_opt, gt=None, pose=None, rgbx_frames=None):
        """icp_track_depth_model_hashed: `track_depth_model` against the context's HASHED volume: every frame aligned to a ray-cast of the
        blocks and, when that succeeds, fused into them (blocks allocated as the frames come; the pool grows on the device).  Returns
        (final pose, records, status).
        rgbx_frames (n, h*w, 4): icp_track_depth_model_color_hashed, the coloured hashed model (needs a coloured hashed volume and
        source_opt.fix_color_index)."""
        d = _depth_in(depth_frames, cam, sequence=True)
        nf = d.shape[0]
        g = _gt_in(gt, nf)
        p = _pose_in(np.eye(4) if pose is None else pose)
        out = (IcpTrackFrame * max(nf - 1, 1))()
        if rgbx_frames is not None:
            cols = _rgbx_in(rgbx_frames, d.size, "colour frames must hold 4 bytes per pixel")
            rc = self.lib.icp_track_depth_model_color_hashed(self.h, _ptr(d), _ptr(cols), C.c_int32(nf), C.byref(cam), C.byref(source_opt), _ptr(g), _ptr(p), out)
        else:
            rc = self.lib.icp_track_depth_model_hashed(self.h, _ptr(d), C.c_int32(nf), C.byref(cam), C.byref(source_opt), _ptr(g), _ptr(p), out)
        if rc not in (ICP_OK, ERR_NO_TARGET, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # per-frame outcomes: reported in the records
            self._ck(rc)
        return pose_from_c(p), [_record(out[i]) for i in range(nf - 1)], rc

    def tsdf_sample(self, points):
        """icp_tsdf_sample: the volume's field and its gradient at world points (n, 3).  Returns (F (n,), G (n, 3) per voxel, valid (n,)
        bool: the point's cell lies inside the volume with all eight corners observed; elsewhere F and G read 0)."""
        p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        n = len(p)
        f = np.empty(n, np.float32); g = np.empty((n, 3), np.float32); ok = np.empty(n, np.uint8)
        self._ck(self.lib.icp_tsdf_sample(self.h, _ptr(p), C.c_int32(n), _ptr(f), _ptr(g), _ptr(ok)))
        return f, g, ok.astype(bool)

    def tsdf_sample_color(self, points):
        """icp_tsdf_sample_color: the intensity field S = R + G + B of the colour array and its gradient at world points (n, 3).  Returns
        (S (n,), H (n, 3) per voxel, valid (n,) bool: the point's cell lies inside the volume with all eight corners coloured; elsewhere S
        and H read 0)."""
        p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 3))
        n = len(p)
        f = np.empty(n, np.float32); g = np.empty((n, 3), np.float32); ok = np.empty(n, np.uint8)
        self._ck(self.lib.icp_tsdf_sample_color(self.h, _ptr(p), C.c_int32(n), _ptr(f), _ptr(g), _ptr(ok)))
        return f, g, ok.astype(bool)

    def tsdf_sdf_system(self, depth, cam, pose, options=None, rgbx=None, color_weight=0.0, color_huber=0.0, **kw):
        """icp_tsdf_sdf_system: the 28 sums of one direct SDF step of the frame at `pose` (4x4 camera -> world).  options: an
        IcpSdfOptions, or the arguments of `sdf_options`.  Returns (sums (28,) float64, (n_depth, n_valid)).
        color_weight > 0 (with rgbx, the frame's colour frame): icp_tsdf_sdf_system_color, the joint system with the photometric term of
        weight color_weight and Huber bound color_huber.  Returns (sums (29,), (n_depth, n_valid, n_color))."""
        o = options if options is not None else sdf_options(**kw)
        depth = _depth_in(depth, cam)
        cols, co = _sdf_color_in(rgbx, depth.size, color_weight, color_huber, "colour frame must hold 4 bytes per pixel")
        if co is not None:
            sums = np.empty(29, np.float64); cnt = (C.c_int32 * 3)()
            self._ck(self.lib.icp_tsdf_sdf_system_color(self.h, _ptr(depth), _ptr(cols), C.byref(cam), _ptr(pose_to_c(pose)), C.byref(o), C.byref(co), _ptr(sums), cnt))
            return sums, (cnt[0], cnt[1], cnt[2])
        sums = np.empty(28, np.float64); cnt = (C.c_int32 * 2)()
        self._ck(self.lib.icp_tsdf_sdf_system(self.h, _ptr(depth), C.byref(cam), _ptr(pose_to_c(pose)), C.byref(o), _ptr(sums), cnt))
        return sums, (cnt[0], cnt[1])

    def tsdf_align_depth(self, depth, cam, pose=None, trace=False, options=None, rgbx=None, color_weight=0.0, color_huber=0.0, **kw):
        """icp_tsdf_align_depth: one depth frame aligned to the volume itself, from `pose` (identity by default).  Returns (pose, record,
        status), with trace=True (pose, record, status, the records of the iterations that ran); a failed frame (status NO_SOURCE or
        NO_CORRESPONDENCES) returns the pose it started with.
        color_weight > 0 (with rgbx): icp_tsdf_align_depth_color, every step with the photometric term; the records are the colour ones."""
        o = options if options is not None else sdf_options(**kw)
        depth = _depth_in(depth, cam)
        p = pose_to_c(np.eye(4) if pose is None else pose)
        cols, co = _sdf_color_in(rgbx, depth.size, color_weight, color_huber, "colour frame must hold 4 bytes per pixel")
        if co is not None:
            rec = IcpSdfColorFrame(); tr = (IcpSdfColorIter * o.n_iterations)() if trace else None
            rc = self.lib.icp_tsdf_align_depth_color(self.h, _ptr(depth), _ptr(cols), C.byref(cam), C.byref(o), C.byref(co), _ptr(p), C.byref(rec), tr)
        else:
            rec = IcpSdfFrame(); tr = (IcpSdfIter * o.n_iterations)() if trace else None
            rc = self.lib.icp_tsdf_align_depth(self.h, _ptr(depth), C.byref(cam), C.byref(o), _ptr(p), C.byref(rec), tr)
        if rc not in (ICP_OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # the frame's outcome: reported in the record
            self._ck(rc)
        r = _record(rec)
        if trace:
            return pose_from_c(p), r, rc, [_record(tr[i]) for i in range(r["iterations"])]
        return pose_from_c(p), r, rc

    def track_depth_sdf(self, depth_frames, cam, pose=None, rgbx_frames=None, options=None, color_weight=0.0, color_huber=0.0, **kw):
        """icp_track_depth_sdf: direct SDF tracking over frames (n, h, w) against the context's TSDF volume: frame 0 integrated at `pose`
        (identity by default), every later frame aligned to the volume and, when that succeeds, integrated at the pose found.
        rgbx_frames (n, h*w, 4): the colours go into the volume's colour array as well.  Returns (final pose, records, status).
        color_weight > 0 (with rgbx_frames): icp_track_depth_sdf_color, every frame aligned with the photometric term as well; the records
        are the colour ones."""
        o = options if options is not None else sdf_options(**kw)
        d = _depth_in(depth_frames, cam, sequence=True)
        nf = d.shape[0]
        p = pose_to_c(np.eye(4) if pose is None else pose)
        cols, co = _sdf_color_in(rgbx_frames, d.size, color_weight, color_huber, "colour frames must hold 4 bytes per pixel")
        if co is not None:
            out = (IcpSdfColorFrame * max(nf - 1, 1))()
            rc = self.lib.icp_track_depth_sdf_color(self.h, _ptr(d), _ptr(cols), C.c_int32(nf), C.byref(cam), C.byref(o), C.byref(co), _ptr(p), out)
        else:
            cols = _rgbx_in(rgbx_frames, d.size, "colour frames must hold 4 bytes per pixel")
            out = (IcpSdfFrame * max(nf - 1, 1))()
            rc = self.lib.icp_track_depth_sdf(self.h, _ptr(d), _ptr(cols), C.c_int32(nf), C.byref(cam), C.byref(o), _ptr(p), out)
        if rc not in (ICP_OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # per-frame outcomes: reported in the records
            self._ck(rc)
        return pose_from_c(p), [_record(out[i]) for i in range(nf - 1)], rc

    def voxelize_target(self, options=None, **kw):
        """icp_voxelize_target: the voxel grid of the resident target (voxelized GICP), built on the device and kept in the context.
        options: an IcpVgicpOptions, or the arguments of `vgicp_options`.  Returns dict(lo, dims, n_occupied, n_points)."""
        o = options if options is not None else vgicp_options(**kw)
        info = IcpVoxelGridInfo()
        self._ck(self.lib.icp_voxelize_target(self.h, C.byref(o), C.byref(info)))
        self._vg_dims = tuple(info.dims)
        return dict(lo=tuple(info.lo), dims=tuple(info.dims), n_occupied=info.n_occupied, n_points=info.n_points)

    def voxel_grid(self, options=None, **kw):
        """icp_get_voxel_grid of the grid `voxelize_target` gives for these options (built if it is not current): (info, counts (n_cells,)
        int32, sums (n_cells, 9) int64, cells (n_cells, 9) float32), cell index (z dims_y + y) dims_x + x."""
        info = self.voxelize_target(options, **kw)
        n = int(np.prod(info["dims"], dtype=np.int64))
        counts = np.empty(n, np.int32); sums = np.empty((n, 9), np.int64); cells = np.empty((n, 9), np.float32)
        self._ck(self.lib.icp_get_voxel_grid(self.h, _ptr(counts), _ptr(sums), _ptr(cells)))
        return info, counts, sums, cells

    def vgicp_system(self, pose, options=None, **kw):
        """icp_vgicp_system: the 28 sums of one voxelized GICP step of the resident source at `pose`.  Returns (sums (28,) float64,
        (considered, valid))."""
        o = options if options is not None else vgicp_options(**kw)
        sums = np.empty(28, np.float64); cnt = (C.c_int32 * 2)()
        self._ck(self.lib.icp_vgicp_system(self.h, _ptr(pose_to_c(pose)), C.byref(o), _ptr(sums), cnt))
        return sums, (cnt[0], cnt[1])

    def vgicp_align(self, pose=None, trace=False, options=None, **kw):
        """icp_vgicp_align: the resident source aligned to the voxel grid of the resident target, from `pose` (identity by default).
        Returns (pose, record, status) and, with trace, the records of the steps tried.  A failed alignment (status ERR_NO_SOURCE or
        ERR_NO_CORRESPONDENCES) returns the pose it started with; every other error raises."""
        o = options if options is not None else vgicp_options(**kw)
        p = pose_to_c(np.eye(4) if pose is None else pose)
        rec = IcpSdfFrame(); tr = (IcpSdfIter * o.n_iterations)() if trace else None
        rc = self.lib.icp_vgicp_align(self.h, C.byref(o), _ptr(p), C.byref(rec), tr, C.c_int32(o.n_iterations if trace else 0))
        if rc not in (ICP_OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # the alignment's outcome: reported in the record
            self._ck(rc)
        r = _record(rec)
        if trace:
            return pose_from_c(p), r, rc, [_record(tr[i]) for i in range(r["iterations"])]
        return pose_from_c(p), r, rc

    def voxel_map_create(self, voxel_size, lo, dims):
        """icp_voxel_map_create: the context's voxel map (scan-to-map laser tracking), allocated and cleared: voxel_size in metres, the
        extent as the lowest cell `lo` and the cells per axis `dims` (see `voxel_map_extent`).  Called again: replaced."""
        o = voxel_map_options(voxel_size, lo, dims)
        self._ck(self.lib.icp_voxel_map_create(self.h, C.byref(o)))

    def voxel_map_destroy(self):
        self._ck(self.lib.icp_voxel_map_destroy(self.h))

    def voxel_map_insert(self, which, pose):
        """icp_voxel_map_insert: fuses the resident target (which = 0) or source (1) into the map at `pose`.  Returns dict(n_considered,
        n_entered, n_outside, n_cells_touched, n_cells_new, n_occupied)."""
        info = IcpVoxelMapInsertInfo()
        self._ck(self.lib.icp_voxel_map_insert(self.h, C.c_int32(which), _ptr(pose_to_c(pose)), C.byref(info)))
        return _record(info)

    def voxel_map(self):
        """icp_get_voxel_map: (info dict(voxel_size, lo, dims, n_occupied), counts (n_cells,) int32, sums (n_cells, 9) int64, cells
        (n_cells, 9) float32), cell index (z dims_y + y) dims_x + x."""
        info = IcpVoxelMapInfo()
        self._ck(self.lib.icp_get_voxel_map(self.h, C.byref(info), None, None, None))
        n = int(np.prod(tuple(info.dims), dtype=np.int64))
        counts = np.empty(n, np.int32); sums = np.empty((n, 9), np.int64); cells = np.empty((n, 9), np.float32)
        self._ck(self.lib.icp_get_voxel_map(self.h, None, _ptr(counts), _ptr(sums), _ptr(cells)))
        return dict(voxel_size=info.voxel_size, lo=tuple(info.lo), dims=tuple(info.dims), n_occupied=info.n_occupied), counts, sums, cells

    def voxel_map_upload(self, counts, sums):
        """icp_voxel_map_upload: replaces the map's integer state (counts (n_cells,), sums (n_cells, 9)) and recomputes every record."""
        info = IcpVoxelMapInfo()
        self._ck(self.lib.icp_get_voxel_map(self.h, C.byref(info), None, None, None))
        n = int(np.prod(tuple(info.dims), dtype=np.int64))
        cn = np.ascontiguousarray(counts, dtype=np.int32); sm = np.ascontiguousarray(sums, dtype=np.int64)
        if cn.size != n or sm.size != 9 * n:
            raise ValueError("the map has %d cells: counts needs %d values, sums %d" % (n, n, 9 * n))
        self._ck(self.lib.icp_voxel_map_upload(self.h, _ptr(cn), _ptr(sm)))

    def voxel_map_create_hashed(self, voxel_size, capacity=1 << 16):
        """icp_voxel_map_create_hashed: the context's voxel map stored in a hash table of cells, without an extent: at least `capacity`
        slots (rounded up to a power of two, 2^8 .. 2^26); it grows on the device when it fills.  Replaces any map, dense or hashed."""
        self._ck(self.lib.icp_voxel_map_create_hashed(self.h, C.c_float(voxel_size), C.c_int32(capacity)))

    def voxel_map_reserve(self, capacity):
        """icp_voxel_map_reserve: rehashes the hashed map into at least `capacity` slots (smaller or equal: nothing happens); slots that a prune
        vacated are dropped on the way."""
        self._ck(self.lib.icp_voxel_map_reserve(self.h, C.c_int32(capacity)))

    def voxel_map_hashed(self):
        """icp_get_voxel_map_hashed: (info dict(voxel_size, capacity, n_occupied, n_grown, n_unplaced), coords (n, 3) int32, counts (n,)
        int32, sums (n, 9) int64, cells (n, 9) float32) of the occupied cells, sorted by key (z, then y, then x)."""
        info = IcpVoxelHashMapInfo()
        self._ck(self.lib.icp_get_voxel_map_hashed(self.h, C.byref(info), C.c_int32(0), None, None, None, None))
        n = info.n_occupied
        coords = np.empty((n, 3), np.int32); counts = np.empty(n, np.int32); sums = np.empty((n, 9), np.int64); cells = np.empty((n, 9), np.float32)
        self._ck(self.lib.icp_get_voxel_map_hashed(self.h, C.byref(info), C.c_int32(n), _ptr(coords), _ptr(counts), _ptr(sums), _ptr(cells)))
        d = {k: getattr(info, k) for k, _ in info._fields_ if k != "reserved"}
        return d, coords, counts, sums, cells

    def voxel_map_upload_hashed(self, coords, counts, sums):
        """icp_voxel_map_upload_hashed: replaces the hashed map's state by the cells `coords` (n, 3) with `counts` (n,) and `sums` (n, 9),
        and computes every record."""
        cc = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 3); cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        sm = np.ascontiguousarray(sums, dtype=np.int64).reshape(-1, 9)
        if not (len(cc) == len(cn) == len(sm)):
            raise ValueError("coords (n, 3), counts (n,) and sums (n, 9) must agree in n")
        self._ck(self.lib.icp_voxel_map_upload_hashed(self.h, C.c_int32(len(cc)), _ptr(cc), _ptr(cn), _ptr(sm)))

    def voxel_map_prune(self, centre, radius):
        """icp_voxel_map_prune: every cell of the map (dense or hashed) whose centre lies beyond `radius` metres of `centre` goes back to
        the cleared state.  Returns dict(n_removed, n_occupied, n_vacated, n_compacted, capacity, n_points_removed)."""
        ce = _f32(centre).reshape(-1)
        if ce.size != 3:
            raise ValueError("centre is three numbers")
        info = IcpVoxelMapPruneInfo()
        self._ck(self.lib.icp_voxel_map_prune(self.h, _ptr(ce), C.c_float(radius), C.byref(info)))
        return _prune_info(info)

    def voxel_map_compact(self):
        """icp_voxel_map_compact: drops the slots a prune vacated from the hashed map, at its current capacity (none: nothing happens)."""
        self._ck(self.lib.icp_voxel_map_compact(self.h))

    def voxel_map_system(self, pose, options=None, **kw):
        """icp_voxel_map_system: the 28 sums of one voxelized GICP step of the resident source at `pose` against the map.  Returns (sums
        (28,) float64, (considered, valid))."""
        o = options if options is not None else vgicp_options(**kw)
        sums = np.empty(28, np.float64); cnt = (C.c_int32 * 2)()
        self._ck(self.lib.icp_voxel_map_system(self.h, _ptr(pose_to_c(pose)), C.byref(o), _ptr(sums), cnt))
        return sums, (cnt[0], cnt[1])

    def voxel_map_align(self, pose=None, trace=False, options=None, **kw):
        """icp_voxel_map_align: the resident source aligned to the map from `pose` (identity by default); `vgicp_align`'s returns."""
        o = options if options is not None else vgicp_options(**kw)
        p = pose_to_c(np.eye(4) if pose is None else pose)
        rec = IcpSdfFrame(); tr = (IcpSdfIter * o.n_iterations)() if trace else None
        rc = self.lib.icp_voxel_map_align(self.h, C.byref(o), _ptr(p), C.byref(rec), tr, C.c_int32(o.n_iterations if trace else 0))
        if rc not in (ICP_OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # the alignment's outcome: reported in the record
            self._ck(rc)
        r = _record(rec)
        if trace:
            return pose_from_c(p), r, rc, [_record(tr[i]) for i in range(r["iterations"])]
        return pose_from_c(p), r, rc

    def track_scans_vmap(self, scans, pose=None, keep_radius=None, options=None, **kw):
        """icp_track_scans_vmap: `scans`, a list of (xyz (n, 3), normals (n, 3) or None) in the sensor frame, tracked against the map:
        scan 0 inserted at `pose` (identity by default), every later scan aligned to the map and, when that succeeds, inserted at the
        pose found.  Returns (final pose, the records of scans 1 .., status: the first per-scan error, or 0).
        keep_radius (metres): icp_track_scans_vmap_local -- after every insert the map is pruned about the scan's position, so it stays
        local; then a fourth value is returned, the prune info of every scan (`voxel_map_prune`'s dict; all zero for a skipped scan)."""
        o = options if options is not None else vgicp_options(**kw)
        ns = len(scans)
        pts = [_f32(s[0]) for s in scans]
        nrm = [None if s[1] is None else _f32(s[1]) for s in scans]
        if any(a.ndim != 2 or a.shape[1] != 3 for a in pts) or any(b is not None and b.shape != a.shape for a, b in zip(pts, nrm)):
            raise ValueError("a scan is (xyz (n, 3), normals (n, 3) or None)")
        xp = (C.c_void_p * ns)(*[_ptr(a) for a in pts]); npp = (C.c_void_p * ns)(*[_ptr(b) for b in nrm])
        cnt = (C.c_int32 * ns)(*[len(a) for a in pts])
        p = pose_to_c(np.eye(4) if pose is None else pose)
        out = (IcpSdfFrame * max(ns - 1, 1))()
        if keep_radius is None:
            rc = self.lib.icp_track_scans_vmap(self.h, xp, npp, cnt, C.c_int32(ns), C.byref(o), _ptr(p), out)
        else:
            pr = (IcpVoxelMapPruneInfo * max(ns, 1))()
            rc = self.lib.icp_track_scans_vmap_local(self.h, xp, npp, cnt, C.c_int32(ns), C.byref(o), C.c_float(keep_radius), _ptr(p), out, pr)
        if rc not in (ICP_OK, ERR_NO_SOURCE, ERR_NO_CORRESPONDENCES):     # per-scan outcomes: reported in the records
            self._ck(rc)
        if keep_radius is None:
            return pose_from_c(p), [_record(out[i]) for i in range(ns - 1)], rc
        return pose_from_c(p), [_record(out[i]) for i in range(ns - 1)], rc, [_prune_info(pr[i]) for i in range(ns)]

    def estimate_normals(self, xyz, k=5, viewpoint=(0.0, 0.0, 0.0)):
        """PointCloud(pcl cloud): k-NN PCA normals flipped towards the viewpoint (PointCloud.h:41-76)."""
        x = _f32(xyz); vp = np.asarray(viewpoint, np.float32)
        nrm = np.empty_like(x); curv = np.empty(len(x), np.float32)
        self._ck(self.lib.icp_estimate_normals(self.h, _ptr(x), C.c_int32(len(x)), C.c_int32(k), _ptr(vp), _ptr(nrm), _ptr(curv)))
        return nrm, curv

    def transform_points(self, xyz, pose):
        x = _f32(xyz); out = np.empty_like(x)
        self._ck(self.lib.icp_transform_points(self.h, _ptr(x), C.c_int32(len(x)), _ptr(pose_to_c(pose)), _ptr(out)))
        return out

    def transform_normals(self, nrm, pose):
        x = _f32(nrm); out = np.empty_like(x)
        self._ck(self.lib.icp_transform_normals(self.h, _ptr(x), C.c_int32(len(x)), _ptr(pose_to_c(pose)), _ptr(out)))
        return out


def pair_owner(pair, n_ranks):
    return int(load_library().icp_pair_owner(C.c_int32(pair), C.c_int32(n_ranks)))


def pairs_of_rank(n_pairs, rank, n_ranks):
    return int(load_library().icp_pairs_of_rank(C.c_int32(n_pairs), C.c_int32(rank), C.c_int32(n_ranks)))


def batch_run(contexts, pairs, initial_poses=None):
    """icp_batch_run: aligns `pairs` (dicts with src_pts/src_nrm[/src_rgba]/tgt_pts/tgt_nrm[/tgt_rgba]) on the given contexts of
    one device, one host thread per context inside the library.  Returns ((n,16) float32 column-major poses in pair order,
    per-pair status codes, overall status)."""
    lib = load_library()
    n = len(pairs)
    keep = []                                                            # keeps the converted arrays alive for the call
    arr = (IcpPair * max(n, 1))()
    for i, d in enumerate(pairs):
        def cv(key, dt):
            a = d.get(key)
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt); keep.append(a)
            return a.ctypes.data
        arr[i].src_xyz = cv("src_pts", np.float32); arr[i].src_normals = cv("src_nrm", np.float32); arr[i].src_rgba = cv("src_rgba", np.uint8)
        arr[i].tgt_xyz = cv("tgt_pts", np.float32); arr[i].tgt_normals = cv("tgt_nrm", np.float32); arr[i].tgt_rgba = cv("tgt_rgba", np.uint8)
        arr[i].n_src = len(d["src_pts"]); arr[i].n_tgt = len(d["tgt_pts"])
        p0 = pose_to_c(np.eye(4) if initial_poses is None else initial_poses[i])
        for k in range(16):
            arr[i].initial_pose[k] = float(p0[k])
    hs = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
    poses = np.zeros((n, 16), np.float32); status = np.zeros(n, np.int32)
    rc = lib.icp_batch_run(hs, C.c_int32(len(contexts)), arr, C.c_int32(n), _ptr(poses), _ptr(status))
    return poses, status, rc


class Comm:
    """icp_comm: one RCCL communicator per process / GPU; the unique id travels through the host application."""

    def __init__(self, device, n_ranks, rank, unique_id):
        self.lib = load_library()
        self.h = C.c_void_p()
        self.n_ranks, self.rank = n_ranks, rank
        idb = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        rc = self.lib.icp_comm_create(C.c_int(device), C.c_int32(n_ranks), C.c_int32(rank), idb, C.byref(self.h))
        if rc != ICP_OK:
            self.h = None
            raise IcpError(rc, self.lib.icp_comm_last_error().decode())

    @staticmethod
    def unique_id():
        lib = load_library()
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        rc = lib.icp_comm_unique_id(buf)
        if rc != ICP_OK:
            raise IcpError(rc, lib.icp_comm_last_error().decode())
        return bytes(buf)

    def gather_poses(self, local_poses, n_pairs):
        lp = np.ascontiguousarray(np.asarray(local_poses, np.float32).reshape(-1, 16))
        out = np.zeros((n_pairs, 16), np.float32)
        rc = self.lib.icp_gather_poses(self.h, _ptr(lp) if len(lp) else None, C.c_int32(len(lp)), C.c_int32(n_pairs), _ptr(out))
        if rc != ICP_OK:
            raise IcpError(rc, self.lib.icp_comm_last_error().decode())
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.icp_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LinearICPOptimizer:
    """Python mirror of the reference's LinearICPOptimizer setter surface (ICPOptimizer.h:41-95, 489-663)."""

    def __init__(self, device=0, stream=None):
        self.ctx = Context(device, stream)

    # -- setters, same names / meaning as the reference --
    def setMatchingMaxDistance(self, d): self.ctx.params.max_distance = d                      # ICPOptimizer.h:41-44
    def setMetric(self, m): self.ctx.params.metric = m                                         # :46-48
    def enableMultiResolution(self, on): self.ctx.params.multires = int(bool(on))              # :50-52
    def enableColorICP(self, on): self.ctx.params.color_icp = int(bool(on))                    # :54-56
    def setRejectionMethod(self, r): self.ctx.params.rejection = r                             # :63-65
    def setWeightingMethod(self, w): self.ctx.params.weighting = w                             # :67-69
    def setMatchingMethod(self, m): self.ctx.params.matching = m                               # :71-78
    def setNbOfIterations(self, n): self.ctx.params.n_iterations = n                           # :84-86
    def setKnnBackend(self, b): self.ctx.params.knn_backend = b
    def setGICPOptions(self, epsilon=1e-3, k=20): self.ctx.set_gicp_options(epsilon, k)         # setMetric(METRIC_GICP) selects it
    def setColoredICPOptions(self, lambda_geometric=0.968, k=20): self.ctx.set_colored_options(lambda_geometric, k)   # setMetric(METRIC_COLORED)
    def setRobustOptions(self, kernel="none", tuning=0.0, sigma=0.0, overlap=1.0): self.ctx.set_robust_options(kernel, tuning, sigma, overlap)

    def setUseReciprocalCorrespondences(self, on): self.ctx.set_reciprocal_options(enabled=bool(on))   # PCL's name for the mutual nearest-neighbour test

    def setConvergenceCriteria(self, rotation_eps, translation_eps, min_iterations=1, patience=1):
        self.ctx.set_convergence_options(rotation_eps, translation_eps, min_iterations, patience)

    def setNormalSpaceOptions(self, grid=5, resample=True): self.ctx.set_nss_options(grid, resample)   # setSelectionMethod(SELECT_NORMAL_SPACE) selects it

    def setSelectionMethod(self, method, proba=1.0, seed=0):                                   # :58-61 (+ explicit seed)
        self.ctx.params.selection = int(method); self.ctx.params.selection_proba = float(proba); self.ctx.params.selection_seed = int(seed)

    def setCameraParamsMatchingMethod(self, K, width, height):                                 # :80-82
        K = np.asarray(K, dtype=np.float32)
        p = self.ctx.params
        p.fx, p.fy, p.cx, p.cy, p.width, p.height = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), int(width), int(height)

    def setConvergenceMeasure(self, src_xyz, ref_xyz, runBenchmark=False):                     # :93-95, ConvergenceMeasure.h:35-44
        self.ctx.set_convergence_reference(src_xyz, ref_xyz)
        self.ctx.params.record_rmse = 3 if runBenchmark else 1

    def estimatePose(self, source, target, initialPose, check=True):
        """source/target: dicts with 'pts', 'nrm', optional 'rgba'.  Returns (pose, per-iteration records)."""
        self.ctx.push_params()
        self.ctx.set_target(target["pts"], target["nrm"], target.get("rgba"))
        self.ctx.set_source(source["pts"], source["nrm"], source.get("rgba"))
        pose, recs, rc = self.ctx.run(initialPose, check=check)
        self.last_status = rc
        return pose, recs


class CeresICPOptimizer(LinearICPOptimizer):
    """The reference's CeresICPOptimizer (ICPOptimizer.h:181-483): the same setters and loop, one Levenberg-Marquardt solve per
    iteration on the device (icp_set_optimizer).  lm_options: field overrides of icp_lm_options."""

    def __init__(self, device=0, stream=None, **options):
        super().__init__(device, stream)
        self.ctx.set_optimizer(True, **options)
