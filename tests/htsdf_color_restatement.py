"""The coloured hashed TSDF volume of include/icp_hip.h restated in numpy fp32: htsdf_restatement.HVolume with
colours, colour fusion over the allocated blocks, the intensity sample, the sums of one joint step, align and track.  Written from the
contract alone, by composition: the blocks, the touch, the geometric integrate and the hashed cell are htsdf_restatement's (HR), the
colour rule is tsdf_color_restatement's (TC), the intensity field, the joint sums, the solve and the alignment are
sdf_color_restatement's (SC).  What is stated here is only what the contract adds: which voxels of the allocated blocks a frame paints,
and that a colour sample reads the colour pool through the hashed cell.  Contains no table and no device code.

Importing this module makes sdf_color_restatement._intensity_field hand a coloured HVolume to the hashed form below (a dense Volume goes
where it always went), so SC.sample_color / SC.system / SC.align take either volume."""
import numpy as np

import htsdf_restatement as HR
import sdf_color_restatement as SC
import sdf_restatement as SR
import tsdf_restatement as TS

f32 = np.float32


def add_color(vol):
    """Colours for an HR.HVolume: vol.colors {(bx, by, bz): [rgb (8, 8, 8, 3), wc (8, 8, 8)]}, float32, indexed [z, y, x]; a block without
    an entry reads (0, 0, 0, 0), uncoloured."""
    vol.colors = {}
    vol._cbox = None
    return vol


def _colors_of(vol, b):
    if b not in vol.colors:
        vol.colors[b] = [np.zeros((8, 8, 8, 3), f32), np.zeros((8, 8, 8), f32)]
    return vol.colors[b]


def sorted_colors(vol):
    """icp_get_tsdf_color_hashed's two extra arrays, in HVolume.sorted_blocks' order: rgb (B, 8, 8, 8, 3), cweight (B, 8, 8, 8)."""
    keys = sorted(vol.blocks, key=lambda b: (b[2], b[1], b[0]))
    if not keys:
        return np.zeros((0, 8, 8, 8, 3), f32), np.zeros((0, 8, 8, 8), f32)
    return np.stack([_colors_of(vol, b)[0] for b in keys]), np.stack([_colors_of(vol, b)[1] for b in keys])


def drop_colors(vol):
    """What icp_tsdf_reset, the geometry-only upload and an evict do to the colours of blocks that are gone: forgotten."""
    vol.colors = {b: c for b, c in vol.colors.items() if b in vol.blocks}
    vol._cbox = None


def block_masks(vol, keys, depth, cam, pose):
    """(updated, painted, pixel index), each (B, 8, 8, 8) indexed [block, z, y, x]: HR.integrate_allocated's decision per voxel of the
    blocks `keys` -- from the inputs alone -- with the colour rule's band: painted iff updated and !(sdf > truncation)."""
    Ri, ti = TS.invert_affine(pose)
    M = Ri.astype(f32); T = ti.astype(f32)
    depth = np.ascontiguousarray(depth, f32).reshape(-1)
    B = np.array(keys, np.int64).reshape(-1, 3)
    loc = np.arange(8, dtype=np.int64)
    gx = (B[:, 0, None] * 8 + loc).astype(f32); gy = (B[:, 1, None] * 8 + loc).astype(f32); gz = (B[:, 2, None] * 8 + loc).astype(f32)
    X = (vol.o[0] + gx * vol.s)[:, None, None, :]; Y = (vol.o[1] + gy * vol.s)[:, None, :, None]; Z = (vol.o[2] + gz * vol.s)[:, :, None, None]
    with np.errstate(all="ignore"):
        xc, yc, zc = [(M[r, 0] * X + (M[r, 1] * Y + M[r, 2] * Z)) + T[r] for r in range(3)]
        ok = zc > 0
        u = np.floor((cam.fx * (xc / zc) + cam.cx) + f32(0.5))
        v = np.floor((cam.fy * (yc / zc) + cam.cy) + f32(0.5))
        ok &= (u >= 0) & (u < f32(cam.width)) & (v >= 0) & (v < f32(cam.height))
        ui = np.where(ok, u, 0).astype(np.int64); vi = np.where(ok, v, 0).astype(np.int64)
        pix = vi * cam.width + ui
        d = depth[pix]
        ok &= np.isfinite(d) & (d > 0) & (d <= vol.max_d)
        sdf = d - zc
        ok &= ~(sdf < -vol.trunc)
        paint = ok & ~(sdf > vol.trunc)
    return ok, paint, pix


def integrate_color_allocated(vol, depth, rgbx, cam, pose):
    """The coloured integrate over every allocated block: HR.integrate_allocated for the geometry, then TC.integrate_color's colour rule on
    the painted voxels, from the pixel the geometry used.  Returns (voxels written, voxels coloured)."""
    if not vol.blocks:
        return 0, 0
    keys = list(vol.blocks)
    ok, paint, pix = block_masks(vol, keys, depth, cam, pose)
    n = HR.integrate_allocated(vol, depth, cam, pose)
    assert n == int(ok.sum())
    rgbx = np.ascontiguousarray(rgbx, np.uint8).reshape(-1, 4)
    c = rgbx[pix][..., :3].astype(f32)
    RGB = np.stack([_colors_of(vol, b)[0] for b in keys]); Wc = np.stack([_colors_of(vol, b)[1] for b in keys])
    with np.errstate(all="ignore"):
        newC = (Wc[..., None] * RGB + c) / (Wc[..., None] + f32(1))
        newWc = np.fmin(Wc + f32(1), vol.max_w)
    RGB = np.where(paint[..., None], newC, RGB).astype(f32); Wc = np.where(paint, newWc, Wc).astype(f32)
    for i, b in enumerate(keys):
        vol.colors[b] = [RGB[i], Wc[i]]
    vol._cbox = None
    return n, int(paint.sum())


def integrate_color(vol, depth, rgbx, cam, pose):
    """icp_tsdf_integrate_color on a coloured hashed volume: HR's touch, then the coloured integrate over every allocated block."""
    blocks, oor = HR.touch(vol, depth, cam, pose)
    vol.n_out_of_range += oor
    vol.allocate(sorted(blocks))
    return integrate_color_allocated(vol, depth, rgbx, cam, pose)


class _IntensityView(HR.HVolume):
    """The colour pool seen as a volume of (s, Wc) pairs with s = (R + G) + B per voxel: HR's hashed cell on it is the colour cell of the
    contract -- valid iff the cell is storable and every corner has Wc > 0 (a voxel of a block that does not exist reads Wc = 0)."""

    def __init__(self, hv):
        self.hv, self.o, self.s = hv, hv.o, hv.s

    def box(self):
        hv = self.hv
        if getattr(hv, "_cbox", None) is None:
            coords = hv.sorted_blocks()[0]
            if not len(coords):
                hv._cbox = (np.zeros(3, np.int64), np.zeros((0, 0, 0), f32), np.zeros((0, 0, 0), f32))
            else:
                rgb, wc = sorted_colors(hv)
                s = (rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]
                lo = coords.min(0).astype(np.int64) * 8
                dims = (coords.max(0).astype(np.int64) + 1) * 8 - lo
                hv._cbox = (lo,) + HR.blocks_to_dense(coords, s, wc, lo, dims)
        return hv._cbox


def _intensity_field(vol, qx, qy, qz):
    """SC._intensity_field on a coloured hashed volume: (cell storable, all eight Wc > 0, S, H_x, H_y, H_z); the interpolation is SR's."""
    all8, S, hx, hy, hz = SR._field_and_gradient(_IntensityView(vol), qx, qy, qz)
    with np.errstate(all="ignore"):
        storable = np.ones(len(qx), bool)
        for a, q in enumerate((qx, qy, qz)):
            fl = np.floor((q - vol.o[a]) / vol.s)
            storable &= (fl >= HR.CELL_LO) & (fl <= HR.CELL_HI)
    return storable, all8, S, hx, hy, hz


_dense_field = getattr(SC._intensity_field, "dense", SC._intensity_field)      # (the original, also when this module is imported a second time)


def _either_field(vol, qx, qy, qz):
    return _intensity_field(vol, qx, qy, qz) if isinstance(vol, HR.HVolume) else _dense_field(vol, qx, qy, qz)


_either_field.dense = _dense_field
SC._intensity_field = _either_field

sample_color, system, align = SC.sample_color, SC.system, SC.align


def track(vol, frames, rgbx_frames, cam, pose0, **kw):
    """icp_track_depth_sdf_color on a coloured hashed volume: SC.track with the hashed coloured integrate.  Returns (poses after every
    frame, frame 0 included; records of frames 1 ..; blocks after every frame)."""
    pose = np.asarray(pose0, f32).copy()
    integrate_color(vol, frames[0], rgbx_frames[0], cam, pose)
    poses, recs, n_blocks = [pose.copy()], [], [len(vol.blocks)]
    for k in range(1, len(frames)):
        pose, rec, _ = SC.align(vol, frames[k], rgbx_frames[k], cam, pose, **kw)
        if rec["status"] == SC.OK:
            integrate_color(vol, frames[k], rgbx_frames[k], cam, pose)
        poses.append(pose.copy()); recs.append(rec); n_blocks.append(len(vol.blocks))
    return poses, recs, n_blocks
