"""The depth mesh of reconstructRoom (SimpleMesh(sensor, cameraPose, edgeThreshold), SimpleMesh.h:36-119) restated on the host.

`mesh_spec` is the specification the device (icp_depth_mesh, tests/test_gpu_depth_mesh.py) is held to: a vectorised numpy restatement
in fp32, in the order the kernels use, with the two matrices composed in fp64 exactly as the library composes them.  `mesh_literal` is a
per-pixel transcription of the reference loop that tests/test_depth_mesh_host.py checks it against."""
import math
import numpy as np

f32 = np.float32
MINF = -np.inf


# ------------------------------------------------------------------------------------------------------------------------------------
# fp64 compositions, operation for operation as icp_hip.hip does them (invert_affine, icp_depth_mesh)

def invert_affine(T):
    """Inverse of a 4x4 (row, col) fp32 matrix as an affine map in fp64: (R^-1 row-major, 9 floats; t^-1, 3 floats)."""
    T = np.asarray(T, f32)
    R = [float(T[r, k]) for r in range(3) for k in range(3)]
    t = [float(T[r, 3]) for r in range(3)]
    det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6])
    q = [(R[4] * R[8] - R[5] * R[7]) / det, (R[2] * R[7] - R[1] * R[8]) / det, (R[1] * R[5] - R[2] * R[4]) / det,
         (R[5] * R[6] - R[3] * R[8]) / det, (R[0] * R[8] - R[2] * R[6]) / det, (R[2] * R[3] - R[0] * R[5]) / det,
         (R[3] * R[7] - R[4] * R[6]) / det, (R[1] * R[6] - R[0] * R[7]) / det, (R[0] * R[4] - R[1] * R[3]) / det]
    ti = [-(q[r * 3] * t[0] + q[r * 3 + 1] * t[1] + q[r * 3 + 2] * t[2]) for r in range(3)]
    return q, ti


def mesh_matrices(pose, E=None, Kc=None, Ec=None, K=None):
    """(M, C): M = P^-1 E^-1 (3x3 row-major + t, 12 fp32: depth_point's layout) and C = Kc Ec P (3x4 row-major fp32), both composed in
    fp64 and rounded once.  Kc / Ec default to the depth intrinsics K and the identity (the TUM sensor)."""
    P = np.asarray(pose, f32)
    E = np.eye(4, dtype=f32) if E is None else np.asarray(E, f32)
    Ec = np.eye(4, dtype=f32) if Ec is None else np.asarray(Ec, f32)
    Kc = np.asarray(K if Kc is None else Kc, f32)
    Pi, pt = invert_affine(P)
    Ei, et = invert_affine(E)
    M = [0.0] * 12
    for r in range(3):
        for k in range(3):
            M[r * 3 + k] = (Pi[r * 3] * Ei[k] + Pi[r * 3 + 1] * Ei[3 + k]) + Pi[r * 3 + 2] * Ei[6 + k]
        M[9 + r] = ((Pi[r * 3] * et[0] + Pi[r * 3 + 1] * et[1]) + Pi[r * 3 + 2] * et[2]) + pt[r]
    Kd = [float(Kc[0, 0]), 0.0, float(Kc[0, 2]), 0.0, float(Kc[1, 1]), float(Kc[1, 2]), 0.0, 0.0, 1.0]
    A = [(((float(Ec[r, 0]) * float(P[0, k]) + float(Ec[r, 1]) * float(P[1, k])) + float(Ec[r, 2]) * float(P[2, k])) +
          float(Ec[r, 3]) * float(P[3, k])) for r in range(3) for k in range(4)]
    Cm = [(Kd[r * 3] * A[k] + Kd[r * 3 + 1] * A[4 + k]) + Kd[r * 3 + 2] * A[8 + k] for r in range(3) for k in range(4)]
    return np.array(M, np.float64).astype(f32), np.array(Cm, np.float64).astype(f32)


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement

def x86_u32(x):
    """(unsigned int) of fp32 values as gcc compiles it for x86-64: truncate to int64 (NaN and out-of-range -> INT64_MIN), low 32 bits."""
    x = np.asarray(x, f32).astype(np.float64)
    ok = (x >= -2.0 ** 63) & (x < 2.0 ** 63)
    t = np.where(ok, x, 0.0).astype(np.int64)
    t[~ok] = np.iinfo(np.int64).min
    return (t & 0xFFFFFFFF).astype(np.uint32)


def mesh_spec(depth, rgbx, K, pose, threshold, E=None, color=None, details=False):
    """SimpleMesh(sensor, pose, threshold) restated: (vertices (n,3) f32, colours (n,4) u8 or None, triangles (T,3) u32).
    depth (h, w) fp32 with MINF holes; rgbx the colour frame (nc, 4) or None; color = (Kc, Ec, width_c, height_c) or None (TUM sensor).
    details=True also returns the floored projections (column, row; fp32) of every pixel, before the cast and the clamps."""
    depth = np.asarray(depth, f32)
    h, w = depth.shape
    K = np.asarray(K, f32)
    Kc, Ec, wc, hc = (K, None, w, h) if color is None else color
    M, Cm = mesh_matrices(pose, E, Kc, Ec, K)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    d = depth.reshape(-1)
    v, u = np.divmod(np.arange(d.size), w)
    u = u.astype(f32); v = v.astype(f32)
    hole = d == MINF
    with np.errstate(all="ignore"):
        a = (u - cx) / fx * d
        b = (v - cy) / fy * d
        c = d
        p = np.stack([(M[3 * r] * a + (M[3 * r + 1] * b + M[3 * r + 2] * c)) + M[9 + r] for r in range(3)], axis=1).astype(f32)
        p[hole] = MINF
        cols = fu = fv = None
        if rgbx is not None:
            x, y, z = p[:, 0], p[:, 1], p[:, 2]
            q = [(Cm[4 * r] * x + (Cm[4 * r + 1] * y + Cm[4 * r + 2] * z)) + Cm[4 * r + 3] for r in range(3)]
            fu, fv = np.floor(q[0] / q[2]), np.floor(q[1] / q[2])
            ucol, vcol = x86_u32(fu), x86_u32(fv)
            uc = np.where(ucol >= wc, wc - 1, ucol).astype(np.int64)
            vc = np.where(vcol >= hc, hc - 1, vcol).astype(np.int64)
            cols = np.asarray(rgbx, np.uint8).reshape(-1, 4)[vc * wc + uc]
            cols[hole] = 0
        finite = np.isfinite(p).all(axis=1)
        if h < 2 or w < 2:
            tris = np.zeros((0, 3), np.uint32)
        else:
            ii, jj = np.meshgrid(np.arange(h - 1), np.arange(w - 1), indexing="ij")
            i0 = (ii * w + jj).reshape(-1)
            i1, i2 = i0 + w, i0 + 1
            i3 = i1 + 1
            thr = f32(threshold)

            def edge(s, t):
                dx, dy, dz = p[s, 0] - p[t, 0], p[s, 1] - p[t, 1], p[s, 2] - p[t, 2]
                return np.sqrt((dx * dx + dz * dz) + dy * dy)
            e12 = thr > edge(i1, i2)
            first = finite[i0] & finite[i1] & finite[i2] & e12 & (thr > edge(i0, i1)) & (thr > edge(i0, i2))
            second = finite[i1] & finite[i2] & finite[i3] & e12 & (thr > edge(i3, i1)) & (thr > edge(i3, i2))
            cand = np.stack([np.stack([i0, i1, i2], axis=1), np.stack([i1, i3, i2], axis=1)], axis=1)       # (quads, 2, 3)
            tris = cand[np.stack([first, second], axis=1)].astype(np.uint32)
    if details:
        return p, cols, tris, fu, fv
    return p, cols, tris


# ------------------------------------------------------------------------------------------------------------------------------------
# a literal transcription of SimpleMesh.h:36-119, pixel by pixel in scalar fp32, with the same fences

def _cast_u32(x):
    x = float(x)
    t = -2 ** 63 if (math.isnan(x) or not (-2.0 ** 63 <= x < 2.0 ** 63)) else int(x)
    return t & 0xFFFFFFFF


def mesh_literal(depth, rgbx, K, pose, threshold, E=None, color=None):
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    K = np.asarray(K, f32)
    Kc, Ec, Wc, Hc = (K, None, W, H) if color is None else color
    M, Cm = mesh_matrices(pose, E, Kc, Ec, K)
    fovX, fovY, cX, cY = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    colorMap = None if rgbx is None else np.asarray(rgbx, np.uint8).reshape(-1)
    pos = [None] * (W * H)
    col = [None] * (W * H)
    with np.errstate(all="ignore"):
        for v in range(H):
            for u in range(W):
                idx = v * W + u
                dep = depth[v, u]
                if dep == MINF:
                    pos[idx] = (f32(MINF),) * 3
                    col[idx] = (0, 0, 0, 0)
                    continue
                a = (f32(u) - cX) / fovX * dep
                b = (f32(v) - cY) / fovY * dep
                c = dep
                pos[idx] = tuple((M[3 * r] * a + (M[3 * r + 1] * b + M[3 * r + 2] * c)) + M[9 + r] for r in range(3))
                if colorMap is not None:
                    x, y, z = pos[idx]
                    proj = [(Cm[4 * r] * x + (Cm[4 * r + 1] * y + Cm[4 * r + 2] * z)) + Cm[4 * r + 3] for r in range(3)]
                    uCol = _cast_u32(np.floor(proj[0] / proj[2]))
                    vCol = _cast_u32(np.floor(proj[1] / proj[2]))
                    if uCol >= Wc:
                        uCol = Wc - 1
                    if vCol >= Hc:
                        vCol = Hc - 1
                    idxCol = vCol * Wc + uCol
                    col[idx] = tuple(int(colorMap[4 * idxCol + k]) for k in range(4))

        def norm(s, t):
            dx, dy, dz = s[0] - t[0], s[1] - t[1], s[2] - t[2]
            return np.sqrt((dx * dx + dz * dz) + (dy * dy + f32(0)))

        def valid(i):
            return all(np.isfinite(x) for x in pos[i])
        thr = f32(threshold)
        tris = []
        for i in range(H - 1):
            for j in range(W - 1):
                i0 = i * W + j; i1 = (i + 1) * W + j; i2 = i * W + j + 1; i3 = (i + 1) * W + j + 1
                if valid(i0) and valid(i1) and valid(i2):
                    d0, d1, d2 = norm(pos[i0], pos[i1]), norm(pos[i0], pos[i2]), norm(pos[i1], pos[i2])
                    if thr > d0 and thr > d1 and thr > d2:
                        tris.append((i0, i1, i2))
                if valid(i1) and valid(i2) and valid(i3):
                    d0, d1, d2 = norm(pos[i3], pos[i1]), norm(pos[i3], pos[i2]), norm(pos[i1], pos[i2])
                    if thr > d0 and thr > d1 and thr > d2:
                        tris.append((i1, i3, i2))
    verts = np.array(pos, f32).reshape(-1, 3)
    cols = None if colorMap is None else np.array(col, np.uint8).reshape(-1, 4)
    return verts, cols, np.array(tris, np.uint32).reshape(-1, 3)
