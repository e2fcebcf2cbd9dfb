"""The hashed TSDF volume of include/icp_hip.h restated in numpy fp32: the touch that allocates blocks from a depth
frame, the integrate over the allocated blocks, the cell, and the tracking composition.  Written from the contract alone; every fp32
operation is one numpy float32 operation in the order the contract writes it, so the device is compared bit for bit.  Blocks live in a dict
keyed by their coordinates.  Contains no table and no device code.

Field, gradient, sums, solve and alignment are sdf_restatement's: that module reads a volume through tsdf_restatement._cell alone, and
importing this module makes that function hand an HVolume to the hashed cell below (a dense Volume goes where it always went), so
sdf_restatement.sample / system / align take either volume."""
import math
import numpy as np

import tsdf_restatement as TS
import sdf_restatement as SR

f32 = np.float32
RANGE = 1 << 20                                   # storable block coordinates: -2^20 <= b < 2^20
CELL_LO, CELL_HI = f32(-(1 << 23)), f32((1 << 23) - 2)      # cells whose eight corners have storable blocks


class HVolume:
    """blocks: {(bx, by, bz): [tsdf (8, 8, 8), weight (8, 8, 8)]}, float32, indexed [z, y, x]."""

    def __init__(self, origin, voxel_size=0.05, truncation=0.25, max_weight=64.0, min_depth=0.3, max_depth=8.0, ray_step=0.0, **_):
        self.o = np.asarray(origin, f32)
        self.s, self.trunc, self.max_w = f32(voxel_size), f32(truncation), f32(max_weight)
        self.min_d, self.max_d = f32(min_depth), f32(max_depth)
        self.blocks = {}
        self.n_out_of_range = 0
        self._box = None

    def options(self):
        return dict(origin=tuple(float(x) for x in self.o), voxel_size=float(self.s), truncation=float(self.trunc), max_weight=float(self.max_w),
                    min_depth=float(self.min_d), max_depth=float(self.max_d))

    def allocate(self, coords):
        for b in np.asarray(coords, np.int64).reshape(-1, 3):
            b = tuple(int(x) for x in b)
            assert all(-RANGE <= x < RANGE for x in b), b
            if b not in self.blocks:
                self.blocks[b] = [np.zeros((8, 8, 8), f32), np.zeros((8, 8, 8), f32)]
                self._box = None

    def sorted_blocks(self):
        """icp_get_tsdf_hashed's layout: (coords (B, 3) int32, tsdf (B, 8, 8, 8), weight (B, 8, 8, 8)), sorted by key: z, then y, then x."""
        keys = sorted(self.blocks, key=lambda b: (b[2], b[1], b[0]))
        if not keys:
            return np.zeros((0, 3), np.int32), np.zeros((0, 8, 8, 8), f32), np.zeros((0, 8, 8, 8), f32)
        return np.array(keys, np.int32), np.stack([self.blocks[b][0] for b in keys]), np.stack([self.blocks[b][1] for b in keys])

    def box(self):
        """(lo (3,) voxel coordinates, tsdf, weight (nz, ny, nx)) over the bounding box of the blocks; outside it everything reads (0, 0)."""
        if self._box is None:
            if not self.blocks:
                self._box = (np.zeros(3, np.int64), np.zeros((0, 0, 0), f32), np.zeros((0, 0, 0), f32))
            else:
                coords, t, w = self.sorted_blocks()
                lo = coords.min(0).astype(np.int64) * 8
                dims = (coords.max(0).astype(np.int64) + 1) * 8 - lo
                self._box = (lo,) + blocks_to_dense(coords, t, w, lo, dims)
        return self._box


def blocks_to_dense(coords, tsdf, weight, lo, dims):
    """The blocks written into two dense arrays (nz, ny, nx) whose voxel (0, 0, 0) is global voxel `lo`; what no block covers is (0, 0),
    what lies outside the arrays is dropped."""
    lo = np.asarray(lo, np.int64); nx, ny, nz = (int(d) for d in dims)
    T = np.zeros((nz, ny, nx), f32); W = np.zeros((nz, ny, nx), f32)
    for b, t, w in zip(np.asarray(coords, np.int64).reshape(-1, 3), tsdf, weight):
        x0, y0, z0 = b * 8 - lo
        xs, ys, zs = (slice(max(0, -a), min(8, n - a)) for a, n in ((x0, nx), (y0, ny), (z0, nz)))
        if xs.start >= xs.stop or ys.start >= ys.stop or zs.start >= zs.stop:
            continue
        T[z0 + zs.start:z0 + zs.stop, y0 + ys.start:y0 + ys.stop, x0 + xs.start:x0 + xs.stop] = t[zs, ys, xs]
        W[z0 + zs.start:z0 + zs.stop, y0 + ys.start:y0 + ys.stop, x0 + xs.start:x0 + xs.stop] = w[zs, ys, xs]
    return T, W


def n_steps(vol):
    """M = ceil(2 truncation / s), in double."""
    return int(math.ceil(2.0 * float(vol.trunc) / float(vol.s)))


def touch(vol, depth, cam, pose):
    """The blocks a frame asks for: (set of block coordinates, number of samples out of range).  Allocates nothing."""
    P = np.asarray(pose, f32)
    d = np.ascontiguousarray(depth, f32).reshape(-1)
    uu, vv = np.meshgrid(np.arange(cam.width), np.arange(cam.height))
    u = uu.reshape(-1); v = vv.reshape(-1)
    out, oor = set(), 0
    with np.errstate(all="ignore"):
        usable = np.isfinite(d) & (d > 0) & (d <= vol.max_d)
        a = (u.astype(f32) - cam.cx) / cam.fx; b = (v.astype(f32) - cam.cy) / cam.fy
        z_lo = d - vol.trunc; z_hi = d + vol.trunc
        for m in range(n_steps(vol) + 1):
            z = np.fmin(z_lo + f32(m) * vol.s, z_hi)
            act = usable & (z > 0)
            x = a * z; y = b * z
            fl = [np.floor((((P[r, 0] * x + (P[r, 1] * y + P[r, 2] * z)) + P[r, 3]) - vol.o[r]) / vol.s) for r in range(3)]
            inr = np.ones(len(d), bool)
            for r in range(3):
                inr &= (fl[r] >= CELL_LO) & (fl[r] <= CELL_HI)
            oor += int((act & ~inr).sum())
            act &= inr
            cell = np.stack([fl[r][act] for r in range(3)], 1).astype(np.int64)
            for k in range(8):
                corner = (cell + np.array([k & 1, (k >> 1) & 1, k >> 2], np.int64)) >> 3
                out.update(map(tuple, np.unique(corner, axis=0).tolist()))
    return out, oor


def integrate_allocated(vol, depth, cam, pose):
    """tsdf_restatement.integrate's rule on every voxel of every allocated block, with (float)g for (float)i.  Returns the voxels written."""
    if not vol.blocks:
        return 0
    Ri, ti = TS.invert_affine(pose)
    M = Ri.astype(f32); T = ti.astype(f32)
    depth = np.ascontiguousarray(depth, f32).reshape(-1)
    keys = list(vol.blocks)
    B = np.array(keys, np.int64)
    loc = np.arange(8, dtype=np.int64)
    gx = (B[:, 0, None] * 8 + loc).astype(f32); gy = (B[:, 1, None] * 8 + loc).astype(f32); gz = (B[:, 2, None] * 8 + loc).astype(f32)
    X = (vol.o[0] + gx * vol.s)[:, None, None, :]; Y = (vol.o[1] + gy * vol.s)[:, None, :, None]; Z = (vol.o[2] + gz * vol.s)[:, :, None, None]
    D = np.stack([vol.blocks[b][0] for b in keys]); W = np.stack([vol.blocks[b][1] for b in keys])
    with np.errstate(all="ignore"):
        xc, yc, zc = [(M[r, 0] * X + (M[r, 1] * Y + M[r, 2] * Z)) + T[r] for r in range(3)]
        ok = zc > 0
        u = np.floor((cam.fx * (xc / zc) + cam.cx) + f32(0.5))
        v = np.floor((cam.fy * (yc / zc) + cam.cy) + f32(0.5))
        ok &= (u >= 0) & (u < f32(cam.width)) & (v >= 0) & (v < f32(cam.height))
        ui = np.where(ok, u, 0).astype(np.int64); vi = np.where(ok, v, 0).astype(np.int64)
        d = depth[vi * cam.width + ui]
        ok &= np.isfinite(d) & (d > 0) & (d <= vol.max_d)
        sdf = d - zc
        ok &= ~(sdf < -vol.trunc)
        f = np.fmin(f32(1), sdf / vol.trunc)
        newD = (W * D + f) / (W + f32(1))
        newW = np.fmin(W + f32(1), vol.max_w)
    D = np.where(ok, newD, D).astype(f32); W = np.where(ok, newW, W).astype(f32)
    for i, b in enumerate(keys):
        vol.blocks[b] = [D[i], W[i]]
    vol._box = None
    return int(ok.sum())


def integrate(vol, depth, cam, pose):
    """icp_tsdf_integrate on a hashed volume: the touch, then the integrate over every allocated block.  Returns the voxels written."""
    blocks, oor = touch(vol, depth, cam, pose)
    vol.n_out_of_range += oor
    vol.allocate(sorted(blocks))
    return integrate_allocated(vol, depth, cam, pose)


BOX_LIMIT = 1 << 24                               # voxels of the bounding box beyond which _cell gathers per block instead


def _cell_box(vol, qx, qy, qz):
    """_cell through the dense bounding box of the blocks."""
    lo, T, W = vol.box()
    dims = np.array(T.shape[::-1], np.int64)
    with np.errstate(all="ignore"):
        g = [(q - vol.o[a]) / vol.s for a, q in enumerate((qx, qy, qz))]
        fl = [np.floor(x) for x in g]
        ok = np.ones(len(qx), bool)
        for a in range(3):
            ok &= (fl[a] >= CELL_LO) & (fl[a] <= CELL_HI)
        t = [g[a] - fl[a] for a in range(3)]
        i = [np.where(ok, fl[a], 0).astype(np.int64) - lo[a] for a in range(3)]
        c = np.zeros((8, len(qx)), f32)
        valid = ok.copy()
        for k in range(8):
            j = [i[0] + (k & 1), i[1] + ((k >> 1) & 1), i[2] + (k >> 2)]
            inside = np.ones(len(qx), bool)
            for a in range(3):
                inside &= (j[a] >= 0) & (j[a] < dims[a])
            jj = [np.where(inside, j[a], 0) for a in range(3)]
            if T.size:
                c[k] = np.where(inside, T[jj[2], jj[1], jj[0]], f32(0))
                valid &= inside & (W[jj[2], jj[1], jj[0]] > 0)
            else:
                valid &= False
    return valid, c, t[0], t[1], t[2]


def _cell_gather(vol, qx, qy, qz):
    """_cell without a box: each of the eight corners is read from the block that holds it (g >> 3, local g & 7), found in the dict's keys;
    a corner whose block does not exist reads (0, 0).  The same g, floor, range test and fractions as _cell_box."""
    n = len(qx)
    keys = sorted(vol.blocks, key=lambda b: (b[2], b[1], b[0]))
    B = np.array(keys, np.int64).reshape(-1, 3)
    order = ((B[:, 2] + RANGE) << 42) | ((B[:, 1] + RANGE) << 21) | (B[:, 0] + RANGE)      # (ascending: the sort above is the key's order)
    T = np.stack([vol.blocks[b][0] for b in keys]).reshape(-1, 512) if keys else np.zeros((0, 512), f32)
    W = np.stack([vol.blocks[b][1] for b in keys]).reshape(-1, 512) if keys else np.zeros((0, 512), f32)
    with np.errstate(all="ignore"):
        g = [(q - vol.o[a]) / vol.s for a, q in enumerate((qx, qy, qz))]
        fl = [np.floor(x) for x in g]
        ok = np.ones(n, bool)
        for a in range(3):
            ok &= (fl[a] >= CELL_LO) & (fl[a] <= CELL_HI)
        t = [g[a] - fl[a] for a in range(3)]
        i = [np.where(ok, fl[a], 0).astype(np.int64) for a in range(3)]
    c = np.zeros((8, n), f32)
    valid = ok.copy()
    for k in range(8):
        j = [i[0] + (k & 1), i[1] + ((k >> 1) & 1), i[2] + (k >> 2)]      # (a storable cell's corners: -2^23 .. 2^23 - 1, blocks in range)
        if not keys:
            valid &= False
            continue
        key = (((j[2] >> 3) + RANGE) << 42) | (((j[1] >> 3) + RANGE) << 21) | ((j[0] >> 3) + RANGE)
        at = np.minimum(np.searchsorted(order, key), len(order) - 1)
        there = order[at] == key
        loc = (j[2] & 7) * 64 + (j[1] & 7) * 8 + (j[0] & 7)
        c[k] = np.where(there, T[at, loc], f32(0))
        valid &= there & (W[at, loc] > 0)
    return valid, c, t[0], t[1], t[2]


def box_voxels(vol):
    """The voxels of the bounding box of the blocks (a Python int); 0 for a view that brings a box of its own and no blocks."""
    if not getattr(vol, "blocks", None):
        return 0
    B = np.array(list(vol.blocks), np.int64)
    d = (B.max(0) - B.min(0) + 1) * 8
    return int(d[0]) * int(d[1]) * int(d[2])


def _cell(vol, qx, qy, qz):
    """tsdf_restatement._cell on the hashed volume: (valid, corners (8, n), tx, ty, tz).  Valid iff the cell is storable and all eight
    corner weights are > 0; a voxel of a block that does not exist reads (0, 0).  Through the dense bounding box of the blocks, or, where
    that box would hold more than BOX_LIMIT voxels (blocks at both ends of the storable range), block by block: the two agree bit for bit."""
    return _cell_gather(vol, qx, qy, qz) if box_voxels(vol) > BOX_LIMIT else _cell_box(vol, qx, qy, qz)


_dense_cell = getattr(TS._cell, "dense", TS._cell)      # (the original, also when this module is imported a second time)


def _either_cell(vol, qx, qy, qz):
    return _cell(vol, qx, qy, qz) if isinstance(vol, HVolume) else _dense_cell(vol, qx, qy, qz)


_either_cell.dense = _dense_cell
TS._cell = _either_cell

sample, system, align = SR.sample, SR.system, SR.align


def track(vol, frames, cam, pose0, **kw):
    """icp_track_depth_sdf on a hashed volume: frame 0 integrated at pose0; frame k aligned from the current pose and, on success,
    integrated at the pose found.  Returns (poses after every frame, frame 0 included; records of frames 1 ..; blocks after every frame)."""
    pose = np.asarray(pose0, f32).copy()
    integrate(vol, frames[0], cam, pose)
    poses, recs, n_blocks = [pose.copy()], [], [len(vol.blocks)]
    for k in range(1, len(frames)):
        pose, rec, _ = SR.align(vol, frames[k], cam, pose, **kw)
        if rec["status"] == SR.OK:
            integrate(vol, frames[k], cam, pose)
        poses.append(pose.copy()); recs.append(rec); n_blocks.append(len(vol.blocks))
    return poses, recs, n_blocks
