"""The depth mesh of reconstructRoom (SimpleMesh(sensor, cameraPose, edgeThreshold), SimpleMesh.h:36-119) on the host, no GPU needed.

`mesh_spec` is the specification the device (icp_depth_mesh, tests/test_gpu_depth_mesh.py) is held to: a vectorised numpy restatement
in fp32, in the order the kernels use, with the two matrices composed in fp64 exactly as the library composes them.  Here it is checked
against a literal per-pixel transcription of the reference loop.  Also: the COFF writer, the camera glyph and joinMeshes
(SimpleMesh.h:231-302,336-359), the entry point without a device, the ctypes layout of icp_color_camera and the kernels' register budget.
"""
import ctypes as C
import math
import os
import shutil
import subprocess
import numpy as np
import pytest
from device_asm import device_asm, kernel_resources

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
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


def make_pose(angles, t):
    from icp_amd import synth
    return synth.make_pose(angles, t).astype(f32)


def odd_depth(w, h, seed):
    """A small frame around 1 m with MINF, NaN, +inf, a depth of exactly 1 and ones just above it, and a subnormal."""
    rng = np.random.default_rng(seed)
    d = (0.8 + 0.4 * rng.random((h, w))).astype(f32)
    flat = d.reshape(-1)
    k = rng.permutation(flat.size)
    flat[k[0:4]] = MINF
    flat[k[4:6]] = np.nan
    flat[k[6:8]] = np.inf
    flat[k[8:11]] = 1.0
    flat[k[11:14]] = np.nextafter(f32(1), f32(2))
    flat[k[14]] = f32(1e-40)
    flat[k[15:25]] = flat[k[15:25]] * f32(1.003)          # a few neighbours just across a 0.01 edge
    return d


def color_cases(w, h, rng):
    """(name, rgbx, color) cases: the TUM sensor; a zoomed colour camera on a smaller frame whose projections leave it on both sides; and
    a colour camera 1 m behind the depth camera with a huge focal length, so that depths near 1 project through q2 ~ 0 (inf, NaN, and
    columns beyond 2^32 whose low 32 bits land inside the frame)."""
    wc, hc = w // 2 + 1, h // 2 + 1
    out = [("tum", rng.integers(0, 256, (w * h, 4), dtype=np.uint8), None)]
    Kz = np.array([[3.0 * w, 0, wc / 2.0], [0, 3.0 * w, hc / 2.0], [0, 0, 1]], f32)
    out.append(("zoom", rng.integers(0, 256, (wc * hc, 4), dtype=np.uint8), (Kz, make_pose((0.05, -0.1, 0.02), (0.3, -0.2, 0.1)), wc, hc)))
    Kf = np.array([[5000.0, 0, w / 2.0], [0, 5000.0, h / 2.0], [0, 0, 1]], f32)
    Eb = np.eye(4, dtype=f32); Eb[2, 3] = -1.0
    out.append(("behind", rng.integers(0, 256, (w * h, 4), dtype=np.uint8), (Kf, Eb, w, h)))
    return out


@pytest.mark.parametrize("w,h", [(9, 7), (17, 13)])
def test_restatement_matches_literal_loop(w, h):
    rng = np.random.default_rng(w * 100 + h)
    K = np.array([[w * 0.9, 0, (w - 1) / 2.0], [0, w * 0.9, (h - 1) / 2.0], [0, 0, 1]], f32)
    E = make_pose((0.01, 0.02, -0.03), (0.05, 0.0, -0.02))
    poses = [np.eye(4, dtype=f32), make_pose((0.2, -0.1, 0.3), (0.5, -1.0, 2.0))]
    depth = odd_depth(w, h, w + h)
    seen = set()
    for name, rgbx, color in color_cases(w, h, rng):
        for pose in poses:
            for thr in (0.0, 0.01, np.inf, np.nan):
                for ext in (None, E):
                    want = mesh_literal(depth, rgbx, K, pose, thr, E=ext, color=color)
                    got = mesh_spec(depth, rgbx, K, pose, thr, E=ext, color=color, details=True)
                    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (name, thr)
                    assert np.array_equal(got[1], want[1]), (name, thr)
                    assert got[2].dtype == np.uint32 and np.array_equal(got[2], want[2]), (name, thr)
                    if thr == 0.0 or np.isnan(thr):
                        assert len(got[2]) == 0
                    fu = got[3][depth.reshape(-1) != MINF]
                    wc = w if color is None else color[2]
                    with np.errstate(invalid="ignore"):
                        seen |= {"left"} if (fu < 0).any() else set()
                        seen |= {"right"} if ((fu >= wc) & (fu < 2.0 ** 32)).any() else set()
                        seen |= {"nan"} if (~np.isfinite(fu)).any() else set()
                        seen |= {"wrap"} if ((np.abs(fu) >= 2.0 ** 32) & (x86_u32(fu) < wc)).any() else set()
            # without colours the vertices and triangles are the same
            v0, c0, t0 = mesh_spec(depth, None, K, pose, 0.05)
            v1, c1, t1 = mesh_spec(depth, rgbx if color is None else None, K, pose, 0.05)
            assert c0 is None and np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and np.array_equal(t0, t1)
    assert seen == {"left", "right", "nan", "wrap"}, seen


def test_x86_cast_rule():
    vals = np.array([0, 1.9, -1, -0.0, 2.0 ** 32, 2.0 ** 32 + 2 ** 9, 2.0 ** 63, -2.0 ** 63, np.nan, np.inf, -np.inf, 3e9, -3e9], f32)
    want = [0, 1, 0xFFFFFFFF, 0, 0, 512, 0, 0, 0, 0, 0, 3000000000 & 0xFFFFFFFF, (-3000000000) & 0xFFFFFFFF]
    assert x86_u32(vals).tolist() == [w & 0xFFFFFFFF for w in want]
    assert [_cast_u32(v) for v in vals] == [w & 0xFFFFFFFF for w in want]


def test_restatement_reads_left_neighbours_at_identity():
    """At the identity pose the colour round trip lands on u - eps for some pixels of a 640x480 synthetic frame: their colour is their
    left (or upper) neighbour's, which the shortcut idxCol = idx would miss."""
    from icp_amd import synth, tum
    K = tum.TUM_K
    pts, _, rgba = synth.depth_frame(synth.camera_pose(0), K.astype(np.float64), 640, 480, 0x7A11, 0.05)
    depth = pts[:, 2].reshape(480, 640)
    _, cols, _, fu, fv = mesh_spec(depth, rgba, K, np.eye(4), 0.1, details=True)
    ok = depth.reshape(-1) != MINF
    v, u = np.divmod(np.arange(depth.size), 640)
    du, dv = (fu - u)[ok], (fv - v)[ok]
    assert set(np.unique(du)) == {-1, 0} and set(np.unique(dv)) == {-1, 0}
    assert not np.array_equal(cols[ok], rgba[ok])


def test_flat_quad_and_degenerate_frames():
    K = np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1]], f32)
    v, c, t = mesh_spec(np.ones((2, 2), f32), None, K, np.eye(4), 2.0)
    assert t.tolist() == [[0, 2, 1], [2, 3, 1]]
    for shape in ((1, 1), (1, 7), (7, 1)):
        assert len(mesh_spec(np.ones(shape, f32), None, K, np.eye(4), np.inf)[2]) == 0
    v, c, t = mesh_spec(np.full((4, 5), MINF, f32), np.full((20, 4), 9, np.uint8), K, np.eye(4), np.inf)
    assert np.all(v == MINF) and np.all(c == 0) and len(t) == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# writer, glyph, join

def test_write_off_matches_write_mesh(tmp_path):
    from icp_amd import meshio
    verts = np.array([[1e-5, -0.0, 123456789.0], [0.1, 2.5, -3.0], [np.nan, 0, 0], [MINF, MINF, MINF], [1e20, -1e-20, 100.0]], f32)
    cols = np.array([[255, 0, 7, 255], [1, 2, 3, 4], [9, 9, 9, 9], [0, 0, 0, 0], [10, 20, 30, 40]], np.uint8)
    tris = np.array([[0, 1, 4], [4, 1, 0]], np.uint32)
    path = tmp_path / "m.off"
    meshio.write_off(str(path), verts, cols, tris)
    want = ("COFF\n5 2 0\n"
            "1e-05 -0 1.23457e+08 255 0 7 255\n"
            "0.1 2.5 -3 1 2 3 4\n"
            "0.0 0.0 0.0 0 0 0 0\n"
            "0.0 0.0 0.0 0 0 0 0\n"
            "1e+20 -1e-20 100 10 20 30 40\n"
            "3 0 1 4\n3 4 1 0\n")
    assert path.read_bytes() == want.encode()
    v, c, t = meshio.load_off(str(path))
    fin = np.isfinite(verts).all(axis=1)
    assert np.array_equal(v[fin], np.array([[1e-5, -0.0, 1.23457e8], [0.1, 2.5, -3], [1e20, -1e-20, 100]], f32))
    assert np.all(v[~fin] == 0) and np.all(c[~fin] == 0) and np.array_equal(c[fin], cols[fin]) and np.array_equal(t, tris)
    meshio.write_off(str(tmp_path / "e.off"), np.zeros((0, 3), f32), np.zeros((0, 4), np.uint8), np.zeros((0, 3), np.uint32))
    assert (tmp_path / "e.off").read_bytes() == b"COFF\n0 0 0\n"


def test_camera_glyph_follows_simple_mesh_camera():
    from icp_amd import meshio
    pose = make_pose((0.3, -0.2, 0.9), (1.5, -2.0, 0.25))
    v, c, t = meshio.camera_glyph(pose)
    assert v.shape == (8, 3) and v.dtype == f32 and c.shape == (8, 4) and t.shape == (12, 3) and t.dtype == np.uint32
    assert np.all(c == np.array([255, 0, 0, 255], np.uint8))
    assert t.reshape(-1).tolist() == [1, 2, 3, 2, 0, 3, 2, 5, 4, 4, 0, 2, 5, 6, 7, 7, 4, 5, 6, 1, 7, 1, 3, 7, 3, 0, 4, 7, 3, 4, 5, 2, 1, 5, 1, 6]
    local = 0.0015 * np.array(meshio.CAMERA_VERTICES, np.float64).reshape(8, 3)
    want = (np.linalg.inv(pose.astype(np.float64)) @ np.c_[local, np.ones(8)].T).T[:, :3]
    assert np.abs(v - want).max() < 1e-6
    v2, c2, _ = meshio.camera_glyph(np.eye(4), scale=2.0, color=(1, 2, 3, 4))
    assert np.array_equal(v2, 2.0 * np.array(meshio.CAMERA_VERTICES, f32).reshape(8, 3)) and np.all(c2 == [1, 2, 3, 4])


def test_join_meshes_offsets_the_second_mesh():
    from icp_amd import meshio
    m1 = (np.array([[0, 0, 0], [1, 0, 0], [MINF, MINF, MINF]], f32), np.full((3, 4), 7, np.uint8), np.array([[0, 1, 2]], np.uint32))
    m2 = meshio.camera_glyph(np.eye(4))
    v, c, t = meshio.join_meshes(m1, m2)
    assert v.shape == (11, 3) and c.shape == (11, 4) and t.shape == (13, 3) and t.dtype == np.uint32
    assert np.array_equal(v[:3].view(np.uint32), m1[0].view(np.uint32)) and np.array_equal(v[3:], m2[0])
    assert np.array_equal(t[0], [0, 1, 2]) and np.array_equal(t[1:], m2[2] + 3) and np.all(c[3:] == [255, 0, 0, 255])
    T = make_pose((0, 0, np.pi / 2), (1, 2, 3))
    v, _, _ = meshio.join_meshes(m1, m2, T)
    assert np.abs(v[1] - (T[:3, :3] @ [1, 0, 0] + T[:3, 3])).max() < 1e-6 and not np.isfinite(v[2]).any()


# ------------------------------------------------------------------------------------------------------------------------------------
# library without a device, struct layout, register budget

def test_depth_mesh_without_device_or_context():
    from icp_amd import binding
    lib = binding.load_library()
    h = C.c_void_p()
    rc = lib.icp_ctx_create(0, C.byref(h))
    if rc == 0:
        lib.icp_ctx_destroy(h)
        pytest.skip("a HIP device is visible")
    assert rc == 9                                                  # ICP_ERR_NO_DEVICE
    cam = binding.depth_camera(np.eye(3), 4, 3); ccam = binding.color_camera(np.eye(3), 4, 3)
    d = np.zeros(12, f32); p = binding.pose_to_c(np.eye(4)); v = np.empty(36, f32); cols = np.empty(48, np.uint8)
    t = np.empty(36, np.uint32); n = C.c_int32(-1)
    assert lib.icp_depth_mesh(None, binding._ptr(d), binding._ptr(cols), C.byref(cam), C.byref(ccam), binding._ptr(p), C.c_float(0.1),
                              binding._ptr(v), binding._ptr(cols), binding._ptr(t), C.byref(n)) == 1
    assert lib.icp_depth_mesh(None, binding._ptr(d), None, C.byref(cam), None, binding._ptr(p), C.c_float(0.1),
                              binding._ptr(v), None, binding._ptr(t), C.byref(n)) == 1


C_LAYOUT = r"""
#include <stdio.h>
#include <stddef.h>
#include "icp_hip.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m));
int main(void) {
    printf("icp_color_camera %zu\n", sizeof(icp_color_camera));
    F(icp_color_camera, fx) F(icp_color_camera, fy) F(icp_color_camera, cx) F(icp_color_camera, cy) F(icp_color_camera, width)
    F(icp_color_camera, height) F(icp_color_camera, extrinsics)
    return 0;
}
"""


def test_color_camera_struct_matches_the_c_header(tmp_path):
    from icp_amd import binding
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"; src.write_text(C_LAYOUT); exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    facts = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())
    assert int(facts["icp_color_camera"]) == C.sizeof(binding.IcpColorCamera)
    for field, _ in binding.IcpColorCamera._fields_:
        assert int(facts["icp_color_camera.%s" % field]) == getattr(binding.IcpColorCamera, field).offset, field
    cam = binding.color_camera(np.array([[2, 0, 3], [0, 4, 5], [0, 0, 1]]), 7, 6, make_pose((0, 0, 0), (1, 2, 3)))
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height) == (2, 4, 3, 5, 7, 6) and list(cam.extrinsics)[12:15] == [1, 2, 3]


def test_mesh_kernels_register_budget():
    """The three mesh kernels: no scratch and at most 32 VGPRs (full occupancy for a memory-bound pass).  Compiled: k_mesh_vertices 13,
    k_mesh_count 22, k_mesh_scatter 21."""
    seen = kernel_resources(device_asm())
    for prefix in ("15k_mesh_vertices", "12k_mesh_count", "14k_mesh_scatter"):
        ks = {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev" + prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        for name, f in ks.items():
            assert f["num_vgpr"] <= 32 and f["private_seg_size"] == 0, (name, f)
