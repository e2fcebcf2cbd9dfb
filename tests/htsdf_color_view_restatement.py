"""The coloured views of the hashed TSDF volume (include/icp_hip.h) restated in numpy fp32: the coloured ray-cast,
the coloured target, the vertex colours of the mesh and the coloured model loop, on blocks with a colour pool.  Written from the contract
alone, by composition: the march and the cell are htsdf_raycast_restatement's (RR), the colour rule and the byte rule are
tsdf_color_restatement's (TC), the mesh and its vertex order htsdf_mesh_restatement's (HM), the coloured fusion htsdf_color_restatement's
(HCR).  What is stated here is only what the contract adds: that a colour corner is the colour-pool entry of the voxel at the signed global
coordinate f + d (a voxel of a block that does not exist reads (0, 0, 0, 0)).  Every fp32 operation is one numpy float32 operation in the
contract's order, so the device is compared bit for bit.  Contains no table and no device code."""
import numpy as np

import htsdf_color_restatement as HCR
import htsdf_mesh_restatement as HM
import htsdf_raycast_restatement as RR
import tsdf_color_restatement as TC
import tsdf_restatement as TS
from tsdf_mesh_restatement import _shift

f32 = np.float32
MINF = RR.MINF
PATH_HOLE, PATH_NONE, PATH_NEAREST, PATH_EIGHT = TC.PATH_HOLE, TC.PATH_NONE, TC.PATH_NEAREST, TC.PATH_EIGHT


class ColorBlocks(RR.Blocks):
    """RR.Blocks with the colour pool: rgb (B, 8, 8, 8, 3) and cweight (B, 8, 8, 8) indexed [z, y, x], in the order of coords."""

    def __init__(self, coords, tsdf, weight, rgb, cweight, origin, **opts):
        super().__init__(coords, tsdf, weight, origin, **opts)
        c = np.asarray(coords, np.int64).reshape(-1, 3)
        order = np.argsort(((c[:, 2] + RR.RANGE) << 42) | ((c[:, 1] + RR.RANGE) << 21) | (c[:, 0] + RR.RANGE))
        self.C = np.asarray(rgb, f32).reshape(-1, 512, 3)[order]
        self.Wc = np.asarray(cweight, f32).reshape(-1, 512)[order]

    def color(self, gx, gy, gz):
        """(rgb (n, 3), Wc (n,), the index of the block in key order or -1) of the voxels at signed global coordinates (int64 arrays)."""
        bx, by, bz = gx >> 3, gy >> 3, gz >> 3
        key = ((bz + RR.RANGE) << 42) | ((by + RR.RANGE) << 21) | (bx + RR.RANGE)
        if len(self.key) == 0:
            return np.zeros((len(gx), 3), f32), np.zeros(len(gx), f32), np.full(len(gx), -1, np.int64)
        at = np.minimum(np.searchsorted(self.key, key), len(self.key) - 1)
        there = self.key[at] == key
        loc = (gz & 7) * 64 + (gy & 7) * 8 + (gx & 7)
        return np.where(there[:, None], self.C[at, loc], f32(0)), np.where(there, self.Wc[at, loc], f32(0)), np.where(there, at, -1)


def block_coords(vol):
    """The block coordinates (B, 3) of a Blocks, in its (key) order."""
    m = (1 << 21) - 1
    return np.stack([(vol.key & m) - RR.RANGE, ((vol.key >> 21) & m) - RR.RANGE, (vol.key >> 42) - RR.RANGE], 1)


def blocks_of_volume(hv, ray_step=0.0):
    """The ColorBlocks of a coloured HR.HVolume (HCR.add_color) as it stands."""
    c, t, w = hv.sorted_blocks()
    rgb, wc = HCR.sorted_colors(hv)
    return ColorBlocks(c, t, w, rgb, wc, hv.o, voxel_size=hv.s, truncation=hv.trunc, min_depth=hv.min_d, max_depth=hv.max_d, ray_step=ray_step)


def raycast_color(vol, cam, pose, trace=None):
    """The coloured ray-cast of a ColorBlocks.  Returns (depth, vertices, normals, rgba (w*h, 4) u8, hits, coloured hits, path (w*h): PATH_*).
    trace (a dict, optional) receives per pixel `span` (the number of blocks the hit's cell touches, 0 for a hole) and `blocks` (w*h, 8), the
    key-order index of the block of each corner of the hit's cell (-1 for a hole)."""
    depth, vert, nrm, hits = RR.raycast(vol, cam, pose)
    P = np.asarray(pose, f32)
    n = cam.width * cam.height
    uu, vv = np.meshgrid(np.arange(cam.width, dtype=f32), np.arange(cam.height, dtype=f32))
    a = ((uu.reshape(-1) - cam.cx) / cam.fx).astype(f32); b = ((vv.reshape(-1) - cam.cy) / cam.fy).astype(f32)
    dw = [P[r, 0] * a + (P[r, 1] * b + P[r, 2] * f32(1)) for r in range(3)]
    zh = depth.reshape(-1)
    h = np.nonzero(zh != MINF)[0]
    rgba = np.zeros((n, 4), np.uint8); path = np.full(n, PATH_HOLE, np.int64)
    with np.errstate(all="ignore"):
        q = [P[r, 3] + zh[h] * dw[r][h] for r in range(3)]
        g = [(q[r] - vol.o[r]) / vol.s for r in range(3)]
        fl = [np.floor(x) for x in g]
        t = [g[r] - fl[r] for r in range(3)]
        i = [fl[r].astype(np.int64) for r in range(3)]                  # (a hit's cell is storable: the cast is exact)
        C = np.empty((8, len(h), 3), f32); Wc = np.empty((8, len(h)), f32); blk = np.empty((8, len(h)), np.int64)
        for k in range(8):
            C[k], Wc[k], blk[k] = vol.color(i[0] + (k & 1), i[1] + ((k >> 1) & 1), i[2] + (k >> 2))
        all8 = (Wc > 0).all(0)
        tx, ty, tz = [x[:, None] for x in t]
        L = RR._lerp
        lerp = L(L(L(C[0], C[1], tx), L(C[2], C[3], tx), ty), L(L(C[4], C[5], tx), L(C[6], C[7], tx), ty), tz)
        near = (t[0] >= f32(0.5)).astype(np.int64) + 2 * (t[1] >= f32(0.5)).astype(np.int64) + 4 * (t[2] >= f32(0.5)).astype(np.int64)
        ar = np.arange(len(h))
        near_ok = Wc[near, ar] > 0
        col = np.where(all8[:, None], lerp, C[near, ar])
        has = all8 | near_ok
    path[h] = np.where(all8, PATH_EIGHT, np.where(near_ok, PATH_NEAREST, PATH_NONE))
    out = np.concatenate([TC.color_byte(col), np.full((len(h), 1), 255, np.uint8)], 1)
    rgba[h[has]] = out[has]
    if trace is not None:
        span = np.zeros(n, np.int64); blocks = np.full((n, 8), -1, np.int64)
        span[h] = 1 << sum(((i[r] & 7) == 7).astype(np.int64) for r in range(3))
        blocks[h] = blk.T
        trace.update(span=span, blocks=blocks)
    return depth, vert, nrm, rgba, hits, int(has.sum()), path


def colored_target(vol, cam, pose):
    """What icp_set_target_tsdf_color_hashed makes the target: (vertices, normals, rgba, coloured hits), hits without a colour turned into holes."""
    _, vert, nrm, rgba, _, ncol, path = raycast_color(vol, cam, pose)
    vert = vert.copy(); nrm = nrm.copy()
    drop = path == PATH_NONE
    vert[drop] = MINF; nrm[drop] = MINF
    return vert, nrm, rgba, ncol


def vertex_edges(coords, tsdf, weight, min_weight=0.0):
    """(owner's signed global voxel coordinate (V, 3), code (V,)) of every vertex of HM.mesh, in its order: ascending (rank of the owner's
    block, local index, code).  The contract's rule for which edges carry a vertex, on the blocks laid over their bounding box with one
    voxel of margin (scratch of this function: the order comes from (rank, local), never from the array)."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    tsdf = np.asarray(tsdf, f32).reshape(-1, 8, 8, 8); weight = np.asarray(weight, f32).reshape(-1, 8, 8, 8)
    if len(coords) == 0:
        return np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    order = HM.sort_blocks(coords)
    coords, tsdf, weight = coords[order], tsdf[order], weight[order]
    lo = coords.min(0) * 8 - 1
    nx, ny, nz = (int(v) for v in (coords.max(0) + 1) * 8 + 1 - lo)
    F = np.zeros((nz, ny, nx), f32); W = np.zeros((nz, ny, nx), f32)
    sortkey = np.full((nz, ny, nx), -1, np.int64)
    local = np.arange(512).reshape(8, 8, 8)
    for rank, (b, t, w) in enumerate(zip(coords, tsdf, weight)):
        x0, y0, z0 = (int(v) for v in b * 8 - lo)
        F[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = t; W[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = w
        sortkey[z0:z0 + 8, y0:y0 + 8, x0:x0 + 8] = rank * 512 + local
    with np.errstate(all="ignore"):
        obs = (W > 0) & (W >= f32(min_weight)) & np.isfinite(F)
        neg = F < 0
    valid = np.ones(obs.shape, bool)
    for c in range(8):
        valid &= _shift(obs, c >> 2, (c >> 1) & 1, c & 1)
    has = np.zeros((F.size, 7), bool)
    for code in range(1, 8):
        d = (code & 1, (code >> 1) & 1, code >> 2)
        cross = neg != _shift(neg, d[2], d[1], d[0])
        cell = np.zeros(F.shape, bool)
        for off in range(8):
            if off & code:
                continue
            cell |= _shift(valid, -(off >> 2), -((off >> 1) & 1), -(off & 1))
        has[:, code - 1] = (cross & cell).reshape(-1)
    key = sortkey.reshape(-1)
    va, vc = np.nonzero(has)
    perm = np.lexsort((vc, key[va]))
    va, vc = va[perm], vc[perm] + 1
    g = np.stack([va % nx + lo[0], (va // nx) % ny + lo[1], va // (nx * ny) + lo[2]], 1)
    return g, vc


def mesh_colors(vol, min_weight=0.0, stats=None):
    """(V, 4) u8: the colour of every vertex of HM.mesh on the ColorBlocks `vol`, in its order.  Both ends of the edge v -> v + d coloured:
    C_v + t (C_(v+d) - C_v) at t = F_v / (F_v - F_(v+d)); one end: that end's colour; neither: four zero bytes.  stats (a dict, optional)
    receives the number of vertices with both ends coloured, one, neither, and of those whose far end lies in another block."""
    coords = block_coords(vol)
    g, vc = vertex_edges(coords, vol.F, vol.W, min_weight)
    d = np.stack([vc & 1, (vc >> 1) & 1, vc >> 2], 1)
    e = g + d
    Ca, Wa, _ = vol.color(g[:, 0], g[:, 1], g[:, 2]); Cb, Wb, _ = vol.color(e[:, 0], e[:, 1], e[:, 2])
    Fv = vol.voxel(g[:, 0], g[:, 1], g[:, 2])[0]; Fd = vol.voxel(e[:, 0], e[:, 1], e[:, 2])[0]
    with np.errstate(all="ignore"):
        t = (Fv / (Fv - Fd))[:, None]
        ha, hb = Wa > 0, Wb > 0
        both = Ca + t * (Cb - Ca)
        col = np.where((ha & hb)[:, None], both, np.where(ha[:, None], Ca, Cb))
    out = np.concatenate([TC.color_byte(col), np.full((len(g), 1), 255, np.uint8)], 1)
    out[~(ha | hb)] = 0
    if stats is not None:
        stats.update(both=int((ha & hb).sum()), one=int((ha ^ hb).sum()), neither=int((~(ha | hb)).sum()), far_end_in_another_block=int(((g >> 3) != (e >> 3)).any(1).sum()))
    return out


def mesh(vol, min_weight=0.0, stats=None):
    """icp_tsdf_mesh_color_hashed: HM.mesh's (vertices, normals, triangles) and the colours."""
    coords = block_coords(vol)
    v, n, t = HM.mesh(coords, vol.F, vol.W, vol.o, vol.s, min_weight)
    return v, n, t, mesh_colors(vol, min_weight, stats)


def colored_triangle_rows(vert, nrm, col, tris):
    """HM.triangle_rows with the corner colours: the mesh as a sorted multiset of triangles, each its three corners' positions, normals and
    packed colours (21 uint32), rotated so that its smallest corner comes first, the rows sorted."""
    v = np.ascontiguousarray(vert, f32).view(np.uint32).reshape(-1, 3); n = np.ascontiguousarray(nrm, f32).view(np.uint32).reshape(-1, 3)
    c = np.ascontiguousarray(col, np.uint8).reshape(-1, 4).view(np.uint32).reshape(-1, 1)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    if len(t) == 0:
        return np.zeros((0, 21), np.uint32)
    corner = np.concatenate([v[t], n[t], c[t]], 2).astype(np.int64)      # (T, 3, 7)
    rot = np.stack([np.concatenate([corner[:, (k + j) % 3] for j in range(3)], 1) for k in range(3)], 1)      # (T, 3 rotations, 21)
    best = rot[:, 0]
    for k in (1, 2):
        diff = rot[:, k] != best
        col0 = np.argmax(diff, 1)
        ar = np.arange(len(t))
        less = diff.any(1) & (rot[ar, k, col0] < best[ar, col0])
        best = np.where(less[:, None], rot[:, k], best)
    return best[np.lexsort(best.T[::-1])].astype(np.uint32)


def track(hv, frames, rgbx_frames, cam, pose0, source_of, estimate, ray_step=0.0, geometric=False):
    """icp_track_depth_model_color_hashed on a coloured HR.HVolume: TC.track with the target from the coloured ray-cast of the blocks and
    the coloured hashed integrate (the touch included).  frame 0 integrated at pose0; frame k: target = colored_target (vertices, normals,
    rgba), source = source_of(k), dT = estimate(source, target) from the identity (None: the run failed), pose <- pose dT, frame k
    integrated at the new pose.  A model without coloured hits, an empty source or a failed run carries the pose and integrates nothing.
    geometric: icp_track_depth_model_hashed on the same volume instead -- the target RR.raycast's, every hit kept, rgba None.
    Returns the pose after every frame."""
    pose = np.asarray(pose0, f32).copy()
    HCR.integrate_color(hv, frames[0], rgbx_frames[0], cam, pose)
    poses = [pose.copy()]
    for k in range(1, len(frames)):
        vol = blocks_of_volume(hv, ray_step)
        if geometric:
            _, vert, nrm, n_hit = RR.raycast(vol, cam, pose)
            rgba = None
        else:
            vert, nrm, rgba, n_hit = colored_target(vol, cam, pose)
        src = source_of(k)
        dT = estimate(src, (vert, nrm, rgba)) if n_hit > 0 and len(src[0]) > 0 else None
        if dT is not None:
            pose = TS.compose_pose(pose, dT)
            HCR.integrate_color(hv, frames[k], rgbx_frames[k], cam, pose)
        poses.append(pose.copy())
    return poses
