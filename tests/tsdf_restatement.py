"""The TSDF contract of include/icp_hip.h (frame-to-model tracking) restated in numpy fp32: integrate, ray-cast, and the pose
compositions of the tracking loop.  Written from the contract alone; every fp32 operation is one numpy float32 operation, in the order
the contract writes it, so the device is compared bit for bit.  Contains no tree and no device code."""
import numpy as np

f32 = np.float32
MINF = f32(-np.inf)


class Camera:
    def __init__(self, K, width, height):
        K = np.asarray(K, f32)
        self.fx, self.fy, self.cx, self.cy = f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])
        self.width, self.height = int(width), int(height)


class Volume:
    """tsdf / weight: (nz, ny, nx) float32, x fastest."""

    def __init__(self, dims, origin, voxel_size=0.05, truncation=0.25, max_weight=64.0, min_depth=0.3, max_depth=8.0, ray_step=0.0):
        self.nx, self.ny, self.nz = (int(d) for d in dims)
        self.o = np.asarray(origin, f32)
        self.s, self.trunc, self.max_w = f32(voxel_size), f32(truncation), f32(max_weight)
        self.min_d, self.max_d = f32(min_depth), f32(max_depth)
        self.step = f32(self.trunc / f32(2)) if f32(ray_step) == 0 else f32(ray_step)
        self.tsdf = np.zeros((self.nz, self.ny, self.nx), f32)
        self.weight = np.zeros((self.nz, self.ny, self.nx), f32)

    def options(self):
        return dict(dims=(self.nx, self.ny, self.nz), origin=tuple(float(x) for x in self.o), voxel_size=float(self.s), truncation=float(self.trunc),
                    max_weight=float(self.max_w), min_depth=float(self.min_d), max_depth=float(self.max_d), ray_step=float(self.step))


def invert_affine(pose):
    """The affine inverse of a 4x4 (row, col) float32 pose in fp64, by cofactors: (R^-1 3x3, t^-1 = -R^-1 t), in the library's operation order."""
    m = np.asarray(pose, f32).astype(np.float64)
    R = [m[r, k] for r in range(3) for k in range(3)]
    t = [m[r, 3] for r in range(3)]
    det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6])
    q = [(R[4] * R[8] - R[5] * R[7]) / det, (R[2] * R[7] - R[1] * R[8]) / det, (R[1] * R[5] - R[2] * R[4]) / det,
         (R[5] * R[6] - R[3] * R[8]) / det, (R[0] * R[8] - R[2] * R[6]) / det, (R[2] * R[3] - R[0] * R[5]) / det,
         (R[3] * R[7] - R[4] * R[6]) / det, (R[1] * R[6] - R[0] * R[7]) / det, (R[0] * R[4] - R[1] * R[3]) / det]
    ti = [-(q[r * 3] * t[0] + q[r * 3 + 1] * t[1] + q[r * 3 + 2] * t[2]) for r in range(3)]
    return np.array(q, np.float64).reshape(3, 3), np.array(ti, np.float64)


def compose_pose(P, D):
    """pose <- pose dT: the fp64 product, each element ((P_r0 D_0c + P_r1 D_1c) + P_r2 D_2c) + P_r3 D_3c, rounded once."""
    P = np.asarray(P, f32).astype(np.float64); D = np.asarray(D, f32).astype(np.float64)
    out = np.empty((4, 4), f32)
    for r in range(4):
        for c in range(4):
            out[r, c] = f32(((P[r, 0] * D[0, c] + P[r, 1] * D[1, c]) + P[r, 2] * D[2, c]) + P[r, 3] * D[3, c])
    return out


def gt_in_camera(pose_before, gt):
    """pose_before^-1 gt (both affine), composed in fp64 and rounded once: the transform that moves frame k's source onto its convergence reference."""
    Ri, ti = invert_affine(pose_before)
    g = np.asarray(gt, f32).astype(np.float64)
    G = np.zeros((4, 4), f32); G[3, 3] = 1
    for r in range(3):
        for c in range(3):
            G[r, c] = f32((Ri[r, 0] * g[0, c] + Ri[r, 1] * g[1, c]) + Ri[r, 2] * g[2, c])
        G[r, 3] = f32(((Ri[r, 0] * g[0, 3] + Ri[r, 1] * g[1, 3]) + Ri[r, 2] * g[2, 3]) + ti[r])
    return G


def integrate(vol, depth, cam, pose):
    """One depth frame (h, w) fused into vol from pose (4x4 camera -> world).  Returns the number of voxels written."""
    Ri, ti = invert_affine(pose)
    M = Ri.astype(f32); T = ti.astype(f32)
    depth = np.ascontiguousarray(depth, f32).reshape(-1)
    px = vol.o[0] + np.arange(vol.nx, dtype=f32) * vol.s
    py = vol.o[1] + np.arange(vol.ny, dtype=f32) * vol.s
    pz = vol.o[2] + np.arange(vol.nz, dtype=f32) * vol.s
    X, Y, Z = px[None, None, :], py[None, :, None], pz[:, None, None]
    with np.errstate(all="ignore"):
        cc = [(M[r, 0] * X + (M[r, 1] * Y + M[r, 2] * Z)) + T[r] for r in range(3)]
        xc, yc, zc = cc
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
        D, W = vol.tsdf, vol.weight
        newD = (W * D + f) / (W + f32(1))
        newW = np.fmin(W + f32(1), vol.max_w)
    vol.tsdf = np.where(ok, newD, D).astype(f32)
    vol.weight = np.where(ok, newW, W).astype(f32)
    return int(ok.sum())


def _lerp(a, b, t):
    return a + t * (b - a)


def _cell(vol, qx, qy, qz):
    """The cell of world points q: (valid, corners c[dx + 2 dy + 4 dz] (8, n), tx, ty, tz)."""
    with np.errstate(all="ignore"):
        g = [(q - vol.o[a]) / vol.s for a, q in enumerate((qx, qy, qz))]
        fl = [np.floor(x) for x in g]
        ok = np.ones(len(qx), bool)
        for a, n in enumerate((vol.nx, vol.ny, vol.nz)):
            ok &= (fl[a] >= 0) & (fl[a] <= f32(n - 2))
        t = [g[a] - fl[a] for a in range(3)]
        i = [np.where(ok, fl[a], 0).astype(np.int64) for a in range(3)]
        c = np.empty((8, len(qx)), f32)
        valid = ok.copy()
        for k in range(8):
            dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
            c[k] = vol.tsdf[i[2] + dz, i[1] + dy, i[0] + dx]
            valid &= vol.weight[i[2] + dz, i[1] + dy, i[0] + dx] > 0
    return valid, c, t[0], t[1], t[2]


def field(vol, qx, qy, qz):
    """(valid, F) at world points: the nested lerp along x, then y, then z."""
    valid, c, tx, ty, tz = _cell(vol, np.asarray(qx, f32), np.asarray(qy, f32), np.asarray(qz, f32))
    with np.errstate(all="ignore"):
        e0 = _lerp(_lerp(c[0], c[1], tx), _lerp(c[2], c[3], tx), ty)
        e1 = _lerp(_lerp(c[4], c[5], tx), _lerp(c[6], c[7], tx), ty)
        return valid, _lerp(e0, e1, tz)


def raycast(vol, cam, pose):
    """The volume seen from pose (4x4 camera -> world).  Returns (depth (h, w), vertices (w*h, 3), normals (w*h, 3), hits); holes MINF."""
    P = np.asarray(pose, f32)
    n = cam.width * cam.height
    uu, vv = np.meshgrid(np.arange(cam.width, dtype=f32), np.arange(cam.height, dtype=f32))
    a = ((uu.reshape(-1) - cam.cx) / cam.fx).astype(f32); b = ((vv.reshape(-1) - cam.cy) / cam.fy).astype(f32)
    dw = [P[r, 0] * a + (P[r, 1] * b + P[r, 2] * f32(1)) for r in range(3)]
    alive = np.ones(n, bool); prev_valid = np.zeros(n, bool); ended = np.zeros(n, bool)
    f_prev = np.zeros(n, f32); z_prev = np.zeros(n, f32); f_end = np.zeros(n, f32)
    k = 0
    with np.errstate(all="ignore"):
        while alive.any():
            z = f32(vol.min_d + f32(k) * vol.step)
            if not (z <= vol.max_d):
                break
            idx = np.nonzero(alive)[0]
            valid, F = field(vol, *[P[r, 3] + z * dw[r][idx] for r in range(3)])
            end = valid & (F <= 0)
            ended[idx[end]] = True; f_end[idx[end]] = F[end]; alive[idx[end]] = False
            go = ~end
            prev_valid[idx[go]] = valid[go]
            upd = go & valid
            f_prev[idx[upd]] = F[upd]; z_prev[idx[upd]] = z
            k += 1
        cand = np.nonzero(ended & prev_valid & (f_prev > 0))[0]
        depth = np.full(n, MINF, f32); vert = np.full((n, 3), MINF, f32); nrm = np.full((n, 3), MINF, f32)
        fp, fe = f_prev[cand], f_end[cand]
        zh = z_prev[cand] + vol.step * (fp / (fp - fe))
        valid, c, tx, ty, tz = _cell(vol, *[P[r, 3] + zh * dw[r][cand] for r in range(3)])
        gx = _lerp(_lerp(c[1] - c[0], c[3] - c[2], ty), _lerp(c[5] - c[4], c[7] - c[6], ty), tz)
        gy = _lerp(_lerp(c[2] - c[0], c[3] - c[1], tx), _lerp(c[6] - c[4], c[7] - c[5], tx), tz)
        gz = _lerp(_lerp(c[4] - c[0], c[5] - c[1], tx), _lerp(c[6] - c[2], c[7] - c[3], tx), ty)
        nc = [-(P[0, r] * gx + (P[1, r] * gy + P[2, r] * gz)) for r in range(3)]
        sq = nc[0] * nc[0] + (nc[1] * nc[1] + nc[2] * nc[2])
        ln = np.sqrt(sq)
        m = [x / ln for x in nc]
        hit = valid & np.isfinite(m[0]) & np.isfinite(m[1]) & np.isfinite(m[2])
        h = cand[hit]
        depth[h] = zh[hit]
        vert[h, 0] = (a[h] * zh[hit]); vert[h, 1] = (b[h] * zh[hit]); vert[h, 2] = zh[hit]
        for r in range(3):
            nrm[h, r] = m[r][hit]
    return depth.reshape(cam.height, cam.width), vert, nrm, int(len(h))


def track(vol, frames, cam, pose0, source_of, estimate):
    """The tracking composition of icp_track_depth_model with the alignment left to the caller: frame 0 integrated at pose0; frame k:
    target = raycast(vol, cam, pose), source = source_of(k), dT = estimate(source, target (vertices, normals)) from the identity (None: the
    run failed), pose <- pose dT, frame k integrated at the new pose.  A model without hits, an empty source or a failed run carries the pose
    and integrates nothing.  Returns the pose after every frame (frame 0 included)."""
    pose = np.asarray(pose0, f32).copy()
    integrate(vol, frames[0], cam, pose)
    poses = [pose.copy()]
    for k in range(1, len(frames)):
        _, vert, nrm, hits = raycast(vol, cam, pose)
        src = source_of(k)
        dT = estimate(src, (vert, nrm)) if hits > 0 and len(src[0]) > 0 else None
        if dT is not None:
            pose = compose_pose(pose, dT)
            integrate(vol, frames[k], cam, pose)
        poses.append(pose.copy())
    return poses
