"""The coloured-model contract of include/icp_hip.h restated in numpy fp32: the colour array, integrate with colour,
the coloured ray-cast, the coloured target, the vertex colours of the mesh and the coloured tracking composition.  It builds on
tsdf_restatement (TS) and tsdf_mesh_restatement (TM) by import; every fp32 operation is one numpy float32 operation in the contract's
order, so the device is compared bit for bit.  Contains no device code."""
import numpy as np

import tsdf_mesh_restatement as TM
import tsdf_restatement as TS

f32 = np.float32


def add_color(vol):
    """The colour array of a TS.Volume: rgb (nz, ny, nx, 3) running averages of byte values, wc (nz, ny, nx) the colour weight; cleared."""
    vol.rgb = np.zeros((vol.nz, vol.ny, vol.nx, 3), f32)
    vol.wc = np.zeros((vol.nz, vol.ny, vol.nx), f32)
    return vol


def integrate_masks(vol, depth, cam, pose):
    """(updated, coloured, f, pixel index): which voxels one frame updates geometrically, which of them it colours (!(sdf > truncation)),
    the clamped value and the pixel each voxel projects to -- from the inputs alone, the volume's contents play no part."""
    Ri, ti = TS.invert_affine(pose)
    M = Ri.astype(f32); T = ti.astype(f32)
    depth = np.ascontiguousarray(depth, f32).reshape(-1)
    px = vol.o[0] + np.arange(vol.nx, dtype=f32) * vol.s
    py = vol.o[1] + np.arange(vol.ny, dtype=f32) * vol.s
    pz = vol.o[2] + np.arange(vol.nz, dtype=f32) * vol.s
    X, Y, Z = px[None, None, :], py[None, :, None], pz[:, None, None]
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
        f = np.fmin(f32(1), sdf / vol.trunc)
        paint = ok & ~(sdf > vol.trunc)
    return ok, paint, f.astype(f32), pix


def integrate_color(vol, depth, rgbx, cam, pose):
    """One depth frame (h, w) and its colour frame (h*w, 4) u8 fused into vol from pose.  Returns (voxels written, voxels coloured)."""
    ok, paint, f, pix = integrate_masks(vol, depth, cam, pose)
    rgbx = np.ascontiguousarray(rgbx, np.uint8).reshape(-1, 4)
    with np.errstate(all="ignore"):
        D, W = vol.tsdf, vol.weight
        newD = (W * D + f) / (W + f32(1))
        newW = np.fmin(W + f32(1), vol.max_w)
        vol.tsdf = np.where(ok, newD, D).astype(f32)
        vol.weight = np.where(ok, newW, W).astype(f32)
        c = rgbx[pix][..., :3].astype(f32)
        Wc = vol.wc
        newC = (Wc[..., None] * vol.rgb + c) / (Wc[..., None] + f32(1))
        newWc = np.fmin(Wc + f32(1), vol.max_w)
        # (a voxel that is not coloured keeps its bits, NaN payloads included: np.where copies)
        vol.rgb = np.where(paint[..., None], newC, vol.rgb).astype(f32)
        vol.wc = np.where(paint, newWc, Wc).astype(f32)
    return int(ok.sum()), int(paint.sum())


def color_byte(C):
    """(uint8_t)(int)floorf(fminf(fmaxf(C, 0), 255) + 0.5f)."""
    with np.errstate(all="ignore"):
        return np.floor(np.fmin(np.fmax(np.asarray(C, f32), f32(0)), f32(255)) + f32(0.5)).astype(np.int64).astype(np.uint8)


PATH_HOLE, PATH_NONE, PATH_NEAREST, PATH_EIGHT = 0, 1, 2, 3


def raycast_color(vol, cam, pose):
    """The coloured ray-cast.  Returns (depth, vertices, normals, rgba (w*h, 4) u8, hits, coloured hits, path (w*h): PATH_*)."""
    depth, vert, nrm, hits = TS.raycast(vol, cam, pose)
    P = np.asarray(pose, f32)
    n = cam.width * cam.height
    uu, vv = np.meshgrid(np.arange(cam.width, dtype=f32), np.arange(cam.height, dtype=f32))
    a = ((uu.reshape(-1) - cam.cx) / cam.fx).astype(f32); b = ((vv.reshape(-1) - cam.cy) / cam.fy).astype(f32)
    dw = [P[r, 0] * a + (P[r, 1] * b + P[r, 2] * f32(1)) for r in range(3)]
    zh = depth.reshape(-1)
    h = np.nonzero(zh != TS.MINF)[0]
    rgba = np.zeros((n, 4), np.uint8); path = np.full(n, PATH_HOLE, np.int64)
    with np.errstate(all="ignore"):
        q = [P[r, 3] + zh[h] * dw[r][h] for r in range(3)]
        g = [(q[r] - vol.o[r]) / vol.s for r in range(3)]
        fl = [np.floor(x) for x in g]
        t = [g[r] - fl[r] for r in range(3)]
        i = [fl[r].astype(np.int64) for r in range(3)]
        C = np.empty((8, len(h), 3), f32); Wc = np.empty((8, len(h)), f32)
        for k in range(8):
            dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
            C[k] = vol.rgb[i[2] + dz, i[1] + dy, i[0] + dx]; Wc[k] = vol.wc[i[2] + dz, i[1] + dy, i[0] + dx]
        all8 = (Wc > 0).all(0)
        tx, ty, tz = [x[:, None] for x in t]
        L = TS._lerp
        lerp = L(L(L(C[0], C[1], tx), L(C[2], C[3], tx), ty), L(L(C[4], C[5], tx), L(C[6], C[7], tx), ty), tz)
        near = (t[0] >= f32(0.5)).astype(np.int64) + 2 * (t[1] >= f32(0.5)).astype(np.int64) + 4 * (t[2] >= f32(0.5)).astype(np.int64)
        ar = np.arange(len(h))
        near_ok = Wc[near, ar] > 0
        col = np.where(all8[:, None], lerp, C[near, ar])
        has = all8 | near_ok
        px = np.where(all8, PATH_EIGHT, np.where(near_ok, PATH_NEAREST, PATH_NONE))
    path[h] = px
    out = np.concatenate([color_byte(col), np.full((len(h), 1), 255, np.uint8)], 1)
    rgba[h[has]] = out[has]
    return depth, vert, nrm, rgba, hits, int(has.sum()), path


def colored_target(vol, cam, pose):
    """What icp_set_target_tsdf_color makes the target: (vertices, normals, rgba, coloured hits), hits without a colour turned into holes."""
    _, vert, nrm, rgba, _, ncol, path = raycast_color(vol, cam, pose)
    vert = vert.copy(); nrm = nrm.copy()
    drop = path == PATH_NONE
    vert[drop] = TS.MINF; nrm[drop] = TS.MINF
    return vert, nrm, rgba, ncol


def vertex_edges(vol, min_weight=0.0):
    """(owner linear index, code) of every vertex of TM.mesh(vol, min_weight), in its order: the contract's rule for which edges carry one."""
    F = vol.tsdf
    with np.errstate(all="ignore"):
        neg = F < 0
    valid = TM.valid_cells(vol, min_weight)
    has = np.zeros((F.size, 7), bool)
    for code in range(1, 8):
        d = (code & 1, (code >> 1) & 1, code >> 2)
        inside = TM._shift(np.ones(F.shape, bool), d[2], d[1], d[0])
        cross = inside & (neg != TM._shift(neg, d[2], d[1], d[0]))
        cell = np.zeros(F.shape, bool)
        for off in range(8):
            o = (off & 1, (off >> 1) & 1, off >> 2)
            if any(o[r] and d[r] for r in range(3)):
                continue
            cell |= TM._shift(valid, -o[2], -o[1], -o[0])
        has[:, code - 1] = (cross & cell).reshape(-1)
    vl, vc = np.nonzero(has)
    return vl, vc + 1


def mesh_colors(vol, min_weight=0.0):
    """(V, 4) u8: the colour of every vertex of TM.mesh(vol, min_weight).  Both ends coloured: C_v + t (C_(v+d) - C_v); one end: that end's
    colour; neither: four zero bytes."""
    vl, vc = vertex_edges(vol, min_weight)
    nx, ny = vol.nx, vol.ny
    other = vl + (vc & 1) + ((vc >> 1) & 1) * nx + (vc >> 2) * nx * ny
    Ff = vol.tsdf.reshape(-1); C = vol.rgb.reshape(-1, 3); W = vol.wc.reshape(-1)
    with np.errstate(all="ignore"):
        Fv, Fd = Ff[vl], Ff[other]
        t = (Fv / (Fv - Fd))[:, None]
        ha, hb = W[vl] > 0, W[other] > 0
        both = C[vl] + t * (C[other] - C[vl])
        col = np.where((ha & hb)[:, None], both, np.where(ha[:, None], C[vl], C[other]))
    out = np.concatenate([color_byte(col), np.full((len(vl), 1), 255, np.uint8)], 1)
    out[~(ha | hb)] = 0
    return out


def track(vol, frames, rgbx_frames, cam, pose0, source_of, estimate):
    """TS.track with a coloured target and source: frame 0 integrated with its colours at pose0; frame k: target = colored_target(vol, cam,
    pose) (vertices, normals, rgba), source = source_of(k) (points, normals, rgba: the frame's own bytes), dT = estimate(source, target)
    from the identity (None: the run failed), pose <- pose dT, frame k integrated with its colours at the new pose.  A model without
    coloured hits, an empty source or a failed run carries the pose and integrates nothing.  Returns the pose after every frame."""
    pose = np.asarray(pose0, f32).copy()
    integrate_color(vol, frames[0], rgbx_frames[0], cam, pose)
    poses = [pose.copy()]
    for k in range(1, len(frames)):
        vert, nrm, rgba, ncol = colored_target(vol, cam, pose)
        src = source_of(k)
        dT = estimate(src, (vert, nrm, rgba)) if ncol > 0 and len(src[0]) > 0 else None
        if dT is not None:
            pose = TS.compose_pose(pose, dT)
            integrate_color(vol, frames[k], rgbx_frames[k], cam, pose)
        poses.append(pose.copy())
    return poses


def crafted_sphere():
    """The 37 x 21 x 29 sphere with holes of the mesh tests and a crafted colour array."""
    vol = TM.analytic_volume(TM.sphere((0.05, 0.02, 0.7), 0.4), dims=(37, 21, 29), s=0.05, origin=(-0.9, -0.5, -0.7))
    rng = np.random.default_rng(11)
    vol.weight[:, 9, :] = 0; vol.weight[rng.random(vol.weight.shape) < 0.02] = 0
    vol.tsdf[rng.random(vol.tsdf.shape) < 0.01] = np.nan
    vol.tsdf[5, 10, 12] = np.inf; vol.tsdf[20, 8, 30] = -np.inf; vol.tsdf[14, 3:8, 4:30] = 0.0
    add_color(vol)
    vol.rgb = rng.uniform(-20, 280, vol.rgb.shape).astype(f32)                 # out-of-range channels: the clamp
    vol.rgb[rng.random(vol.rgb.shape) < 0.01] = np.nan
    vol.wc = rng.choice(np.array([0, 1, 2.5], f32), vol.wc.shape, p=[0.15, 0.5, 0.35])
    vol.wc[:, :, 20:24] = 0
    return vol
