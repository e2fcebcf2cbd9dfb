"""OFF/COFF mesh reader and writer, mesh -> point-cloud conversion, and the camera glyph reconstructRoom adds (host-side data model).

Follows SimpleMesh::loadMesh (reference SimpleMesh.h:161-229) and PointCloud(const SimpleMesh&)
(PointCloud.h:12-39): vertex normals are the normalised fp32 sum of un-normalised face normals,
accumulated in file order; colours of mesh-derived clouds are all zero (PointCloud.h:26).
Pre-processing outside the timed ICP loop -- plain numpy, fp32.
write_off / camera_glyph / join_meshes follow writeMesh, camera and joinMeshes (SimpleMesh.h:231-302,336-359): the output side of
saveRoomToFile (utils.h:179-193).  A mesh is a tuple (vertices (V,3) f32, colors (V,4) u8, triangles (T,3) u32).
write_ply_mesh / load_ply_mesh: the mesh of the fused model (Context.tsdf_mesh: vertices, normals, triangles, optionally colours) as a binary PLY.
"""
import numpy as np


def load_off(path):
    """Returns (vertices (V,3) f32, colors (V,4) u8, triangles (T,3) i32)."""
    with open(path, "r") as f:
        tok = f.read().split()
    kind = tok[0]
    if kind not in ("OFF", "COFF"):
        raise ValueError("Incorrect mesh file type.")            # SimpleMesh.h:210-212
    nv, nt = int(tok[1]), int(tok[2])
    pos = 4
    stride = 7 if kind == "COFF" else 3
    body = tok[pos:pos + nv * stride]
    verts = np.array([np.float32(float(body[i * stride + k])) for i in range(nv) for k in range(3)], dtype=np.float32).reshape(nv, 3)
    if kind == "COFF":
        cols = np.array([int(body[i * stride + 3 + k]) & 0xFF for i in range(nv) for k in range(4)], dtype=np.uint8).reshape(nv, 4)
    else:
        cols = np.tile(np.array([0, 0, 0, 255], np.uint8), (nv, 1))
    pos += nv * stride
    tris = np.empty((nt, 3), np.int32)
    for i in range(nt):
        if int(tok[pos]) != 3:
            raise ValueError("We can only read triangular mesh.")   # SimpleMesh.h:220
        tris[i] = [int(tok[pos + 1]), int(tok[pos + 2]), int(tok[pos + 3])]
        pos += 4
    return verts, cols, tris


def mesh_to_cloud(verts, tris):
    """PointCloud(const SimpleMesh&): returns (points, normals, colors) with colours all zero."""
    f32 = np.float32
    pts = verts.astype(np.float32).copy()
    nrm = np.zeros_like(pts)
    for t in tris:
        a = pts[t[1]] - pts[t[0]]
        b = pts[t[2]] - pts[t[0]]
        fn = np.array([f32(a[1] * b[2]) - f32(a[2] * b[1]), f32(a[2] * b[0]) - f32(a[0] * b[2]), f32(a[0] * b[1]) - f32(a[1] * b[0])], dtype=np.float32)
        nrm[t[0]] += fn; nrm[t[1]] += fn; nrm[t[2]] += fn
    for i in range(len(nrm)):
        v = nrm[i]
        z = f32(v[0] * v[0]) + (f32(v[1] * v[1]) + f32(v[2] * v[2]))     # Eigen squaredNorm tree
        if z > 0:
            nrm[i] = v / np.sqrt(z, dtype=np.float32)
    cols = np.zeros((len(pts), 4), np.uint8)
    return pts, nrm, cols


# SimpleMesh::camera (SimpleMesh.h:336-359): eight corners of a frustum and its twelve faces.
CAMERA_VERTICES = (25, 25, 0, -50, 50, 100, 49.99986, 49.9922, 99.99993, -24.99998, 25.00426, 0.005185,
                   25.00261, -25.00023, 0.004757, 49.99226, -49.99986, 99.99997, -50, -50, 100, -25.00449, -25.00492, 0.019877)
CAMERA_FACES = (1, 2, 3, 2, 0, 3, 2, 5, 4, 4, 0, 2, 5, 6, 7, 7, 4, 5, 6, 1, 7, 1, 3, 7, 3, 0, 4, 7, 3, 4, 5, 2, 1, 5, 1, 6)


def _affine_apply(T, v):
    """Matrix4f * Vector4f(x, y, z, 1) in fp32 for every row of v: ((c0 x + c1 y) + c2 z) + c3, the columns c of T."""
    T = np.asarray(T, np.float32)
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    return ((T[:3, 0] * x + T[:3, 1] * y) + T[:3, 2] * z) + T[:3, 3]


def camera_glyph(camera_pose, scale=0.0015, color=(255, 0, 0, 255)):
    """SimpleMesh::camera(cameraPose, scale, color): the frustum moved by cameraPose^-1 (inverted in fp64, rounded once to fp32)."""
    to_world = np.linalg.inv(np.asarray(camera_pose, np.float64)).astype(np.float32)
    local = np.float32(scale) * np.array(CAMERA_VERTICES, np.float64).astype(np.float32).reshape(8, 3)
    verts = _affine_apply(to_world, local).astype(np.float32)
    cols = np.tile(np.array(color, np.uint8), (8, 1))
    return verts, cols, np.array(CAMERA_FACES, np.uint32).reshape(12, 3)


def join_meshes(m1, m2, pose1to2=None):
    """SimpleMesh::joinMeshes(mesh1, mesh2, pose1to2): mesh1's vertices moved by pose1to2 (left as they are when None, the identity),
    then mesh2's; mesh2's triangles offset by the vertex count of mesh1 (unsigned arithmetic)."""
    v1, c1, t1 = m1
    v2, c2, t2 = m2
    v1 = np.asarray(v1, np.float32)
    if pose1to2 is not None:
        with np.errstate(invalid="ignore"):
            v1 = _affine_apply(pose1to2, v1).astype(np.float32)
    verts = np.concatenate([v1, np.asarray(v2, np.float32)]).reshape(-1, 3)
    cols = np.concatenate([np.asarray(c1, np.uint8), np.asarray(c2, np.uint8)]).reshape(-1, 4)
    tris = np.concatenate([np.asarray(t1, np.uint32), np.asarray(t2, np.uint32) + np.uint32(len(v1))]).reshape(-1, 3)
    return verts, cols, tris


def write_off(path, vertices, colors, triangles):
    """SimpleMesh::writeMesh (SimpleMesh.h:231-259), byte for byte: 'COFF', 'nv nt 0', one line per vertex -- the floats as
    std::ostream prints them by default (%g, 6 significant digits) and the colour bytes as integers, or '0.0 0.0 0.0 0 0 0 0' for a
    vertex that is not finite -- then '3 a b c' per triangle."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    c = np.asarray(colors, np.uint8).reshape(-1, 4)
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    finite = np.isfinite(v).all(axis=1)
    line = np.where(finite, "%g %g %g %d %d %d %d\n", "0.0 0.0 0.0 0 0 0 0\n")
    values = np.concatenate([v[finite].astype(np.float64), c[finite].astype(np.float64)], axis=1).ravel().tolist()
    with open(path, "w") as f:
        f.write("COFF\n%d %d 0\n" % (len(v), len(t)))
        f.write("".join(line.tolist()) % tuple(values))
        f.write(("3 %d %d %d\n" * len(t)) % tuple(t.ravel().tolist()))


PLY_MESH_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                   "property float nx\nproperty float ny\nproperty float nz\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n")
_PLY_FACE = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])


PLY_COLOR_MESH_HEADER = PLY_MESH_HEADER.replace("property float nz\n", "property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n")
_PLY_COLOR_VERTEX = np.dtype([("vn", "<f4", (6,)), ("rgba", "u1", (4,))])


def write_ply_mesh(path, vertices, normals, triangles, colors=None):
    """A triangle mesh with per-vertex normals as a binary little-endian PLY: `float` x y z nx ny nz per vertex, a `uchar int` index list per face.
    colors ((V, 4) u8, Context.tsdf_mesh(colors=True)): `uchar` red green blue alpha follow the normal of every vertex."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    n = np.asarray(normals, np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.uint32).reshape(-1, 3)
    if len(n) != len(v):
        raise ValueError("one normal per vertex")
    if len(t) and int(t.max()) > 0x7FFFFFFF:
        raise ValueError("a vertex index does not fit the PLY's int")
    faces = np.empty(len(t), _PLY_FACE)
    faces["n"] = 3; faces["idx"] = t.astype("<i4")
    if colors is None:
        header, body = PLY_MESH_HEADER, np.concatenate([v, n], axis=1).astype("<f4")
    else:
        c = np.asarray(colors, np.uint8).reshape(-1, 4)
        if len(c) != len(v):
            raise ValueError("one colour per vertex")
        header, body = PLY_COLOR_MESH_HEADER, np.empty(len(v), _PLY_COLOR_VERTEX)
        body["vn"] = np.concatenate([v, n], axis=1); body["rgba"] = c
    with open(path, "wb") as f:
        f.write((header % (len(v), len(t))).encode("ascii"))
        f.write(body.tobytes())
        f.write(faces.tobytes())


def load_ply_mesh(path, colors=False):
    """Reads what write_ply_mesh writes.  Returns (vertices (V,3) f32, normals (V,3) f32, triangles (T,3) u32); with colors=True a fourth
    array, (V, 4) u8, or None for a file without colours."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError("not a binary little-endian PLY")
    nv = nt = None
    for ln in lines:
        if ln.startswith("element vertex "):
            nv = int(ln.split()[2])
        elif ln.startswith("element face "):
            nt = int(ln.split()[2])
    head = data[:end].decode("ascii")
    if head == PLY_COLOR_MESH_HEADER % (nv, nt):
        rec = np.frombuffer(data, _PLY_COLOR_VERTEX, nv, end)
        vn, cols, stride = rec["vn"], rec["rgba"].copy(), 28
    elif head == PLY_MESH_HEADER % (nv, nt):
        vn, cols, stride = np.frombuffer(data, "<f4", nv * 6, end).reshape(nv, 6), None, 24
    else:
        raise ValueError("not the layout write_ply_mesh writes")
    faces = np.frombuffer(data, _PLY_FACE, nt, end + nv * stride)
    if nt and not (faces["n"] == 3).all():
        raise ValueError("We can only read triangular mesh.")
    out = (vn[:, :3].astype(np.float32), vn[:, 3:].astype(np.float32), faces["idx"].astype(np.uint32).reshape(nt, 3))
    return out + (cols,) if colors else out
