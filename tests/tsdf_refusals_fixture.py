"""The refusals of the TSDF family's public calls, state by state (tests/test_gpu_tsdf_refusals.py): which check wins and what it says.
Five contexts -- no volume, a dense volume, a dense volume with the colour array, a hashed volume, a hashed volume with colours -- and in
each one every call of TABLE through the C ABI: the ray-casts, the targets, the samples, the SDF systems, alignments and tracking loops and
the meshes, each with valid arguments and with every bad argument of VARIANTS that applies to it.  The status and the whole
icp_last_error string of every call are what tests/golden/tsdf_refusals.json holds.

Shapes: a 16 x 16 x 16 dense volume, a hashed one created for 64 blocks, a 16 x 12 camera, 2 frames of a gently curved wall about 1 m
away (enough for the valid calls to find a surface), n_iterations = 2.

The golden file is a record of what the library DID before its host drivers were folded into shared bodies: run as a script on a GPU,
with ICP_HIP_LIB pointing at a library built from commit 9cecfae (the parent of the fold), this module writes it.  It is never written
from the tree under test; the test and this script walk the same TABLE through the same `record`."""
import ctypes as C
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "tsdf_refusals.json")
PRODUCED_BY = "9cecfae"
f32 = np.float32
W, H = 16, 12
N_FRAMES = 2
VOLUME = dict(origin=(-0.75, -0.75, 0.45), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=2.4)
DIMS = (16, 16, 16)
HASHED_BLOCKS = 64
SDF = dict(stride=1, n_iterations=2, min_valid=6)
CONTEXTS = ("none", "dense", "dense_color", "hashed", "hashed_color")

RAY = ("valid", "extrinsics")
GEO = ("valid", "null_depth", "extrinsics", "stride0")
COL = ("valid", "null_depth", "null_color", "extrinsics", "stride0", "weight0")
MESH = ("valid", "min_weight", "too_small")
# (function, kind, the variants that apply to it); the order is the order of the calls -- the tracking loops, which fuse frames, come last
TABLE = [(fn, kind, variants) for kind, variants, fns in (
    ("raycast", RAY, ("icp_tsdf_raycast", "icp_tsdf_raycast_hashed")),
    ("raycast_color", RAY, ("icp_tsdf_raycast_color", "icp_tsdf_raycast_color_hashed")),
    ("target", RAY, ("icp_set_target_tsdf", "icp_set_target_tsdf_color", "icp_set_target_tsdf_hashed", "icp_set_target_tsdf_color_hashed")),
    ("sample", ("valid",), ("icp_tsdf_sample", "icp_tsdf_sample_color")),
    ("system", GEO, ("icp_tsdf_sdf_system",)),
    ("system_color", COL, ("icp_tsdf_sdf_system_color",)),
    ("align", GEO, ("icp_tsdf_align_depth",)),
    ("align_color", COL, ("icp_tsdf_align_depth_color",)),
    ("mesh", MESH, ("icp_tsdf_mesh", "icp_tsdf_mesh_hashed")),
    ("mesh_color", MESH, ("icp_tsdf_mesh_color", "icp_tsdf_mesh_color_hashed")),
    ("track", GEO + ("color_frames", "n_frames0"), ("icp_track_depth_sdf",)),
    ("track_color", COL + ("n_frames0",), ("icp_track_depth_sdf_color",)),
) for fn in fns]


def keys():
    return ["%s/%s" % (fn, v) for fn, _, variants in TABLE for v in variants]


def frames():
    """(depth (2, H, W) float32, rgbx (2, W*H, 4) bytes): the curved wall and a smooth colour pattern, the same in both frames."""
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    z = (1.0 + 0.1 * np.sin(u * 0.5) + 0.08 * np.cos(v * 0.6)).astype(f32)
    byte = lambda a: np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)
    rgbx = np.stack([byte(60 + 10 * u), byte(200 - 12 * v), byte(90 + 5 * u + 4 * v), np.full((H, W), 255, np.uint8)], -1).reshape(W * H, 4)
    return np.ascontiguousarray(np.stack([z] * N_FRAMES)), np.ascontiguousarray(np.stack([rgbx] * N_FRAMES))


def make_context(factory, name):
    """A context in state `name`: the volume created and both frames fused at the identity (with their colours where it holds colours)."""
    from icp_amd import binding
    from icp_amd.synth import tum_K
    ctx = factory()
    depth, rgbx = frames()
    cam = binding.depth_camera(tum_K(W), W, H)
    eye = np.eye(4, dtype=f32)
    color = name.endswith("_color")
    if name.startswith("dense"):
        ctx.tsdf_create(color=color, dims=DIMS, **VOLUME)
    elif name.startswith("hashed"):
        ctx.tsdf_create_hashed(block_capacity=HASHED_BLOCKS, color=color, **VOLUME)
    if name != "none":
        for k in range(N_FRAMES):
            ctx.tsdf_integrate(depth[k], cam, eye, rgbx=rgbx[k] if color else None)
    return ctx


def record(ctx):
    """Every call of TABLE on `ctx`, in order: {"function/variant": {"status", "error"}} (error: icp_last_error after a status != 0)."""
    from icp_amd import binding as B
    from icp_amd.synth import tum_K
    lib, h, ptr = ctx.lib, ctx.h, B._ptr
    depth, rgbx = frames()
    n = W * H
    shifted = np.eye(4, dtype=f32); shifted[0, 3] = 0.25
    out = {}

    def call(fn, kind, variant):
        cam = B.depth_camera(tum_K(W), W, H, shifted if variant == "extrinsics" else None)
        pose = B.pose_to_c(np.eye(4, dtype=f32))
        opt = B.sdf_options(**dict(SDF, stride=0 if variant == "stride0" else SDF["stride"]))
        copt = B.sdf_color_options(weight=0.0 if variant == "weight0" else 0.1)
        d = None if variant == "null_depth" else depth
        col = None if variant == "null_color" else rgbx
        nf = C.c_int32(0 if variant == "n_frames0" else N_FRAMES)
        i0, i1 = C.c_int32(0), C.c_int32(0)
        img = np.empty(n, f32); v3 = np.empty((n, 3), f32); n3 = np.empty((n, 3), f32); rgba = np.empty((n, 4), np.uint8)
        if kind == "raycast":
            return getattr(lib, fn)(h, C.byref(cam), ptr(pose), ptr(img), ptr(v3), ptr(n3), C.byref(i0))
        if kind == "raycast_color":
            return getattr(lib, fn)(h, C.byref(cam), ptr(pose), ptr(img), ptr(v3), ptr(n3), ptr(rgba), C.byref(i0), C.byref(i1))
        if kind == "target":
            return getattr(lib, fn)(h, C.byref(cam), ptr(pose), C.byref(i0))
        if kind == "sample":
            pts = np.ascontiguousarray(np.array([[0.0, 0.0, 1.0], [0.1, -0.2, 1.1], [5.0, 5.0, 5.0]], f32))
            ok = np.empty(3, np.uint8)
            return getattr(lib, fn)(h, ptr(pts), C.c_int32(3), ptr(img), ptr(v3), ptr(ok))
        if kind == "system":
            sums = np.empty(28, np.float64); cnt = (C.c_int32 * 2)()
            return getattr(lib, fn)(h, ptr(None if d is None else d[1]), C.byref(cam), ptr(pose), C.byref(opt), ptr(sums), cnt)
        if kind == "system_color":
            sums = np.empty(29, np.float64); cnt = (C.c_int32 * 3)()
            return getattr(lib, fn)(h, ptr(None if d is None else d[1]), ptr(None if col is None else col[1]), C.byref(cam), ptr(pose), C.byref(opt), C.byref(copt), ptr(sums), cnt)
        if kind == "align":
            rec = B.IcpSdfFrame()
            return getattr(lib, fn)(h, ptr(None if d is None else d[1]), C.byref(cam), C.byref(opt), ptr(pose), C.byref(rec), None)
        if kind == "align_color":
            rec = B.IcpSdfColorFrame()
            return getattr(lib, fn)(h, ptr(None if d is None else d[1]), ptr(None if col is None else col[1]), C.byref(cam), C.byref(opt), C.byref(copt), ptr(pose), C.byref(rec), None)
        if kind == "track":
            recs = (B.IcpSdfFrame * N_FRAMES)()
            return getattr(lib, fn)(h, ptr(d), ptr(col if variant == "color_frames" else None), nf, C.byref(cam), C.byref(opt), ptr(pose), recs)
        if kind == "track_color":
            recs = (B.IcpSdfColorFrame * N_FRAMES)()
            return getattr(lib, fn)(h, ptr(d), ptr(col), nf, C.byref(cam), C.byref(opt), C.byref(copt), ptr(pose), recs)
        assert kind in ("mesh", "mesh_color")
        min_weight = C.c_float(-1.0 if variant == "min_weight" else 0.0)
        f = getattr(lib, fn)

        def mesh(nv, nt, v, nr, cl, t):                     # the colour array sits between the normals and the triangles
            bufs = [ptr(v), ptr(nr)] + ([ptr(cl)] if kind == "mesh_color" else []) + [ptr(t)]
            return f(h, min_weight, C.c_int32(nv), C.c_int32(nt), *bufs, C.byref(i0), C.byref(i1))
        mesh(0, 0, None, None, None, None)                  # the counting call sizes the arrays (0 and 0 where it is refused)
        V, T = i0.value, i1.value
        v = np.empty((max(V, 1), 3), f32); nr = np.empty((max(V, 1), 3), f32); cl = np.empty((max(V, 1), 4), np.uint8); t = np.empty((max(T, 1), 3), np.uint32)
        return mesh(V - 1 if variant == "too_small" else V, T, v, nr, cl, t)

    for fn, kind, variants in TABLE:
        for variant in variants:
            rc = int(call(fn, kind, variant))
            out["%s/%s" % (fn, variant)] = dict(status=rc, error=lib.icp_last_error(h).decode() if rc != 0 else "")
    return out


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from icp_amd import binding
    assert os.environ.get("ICP_HIP_LIB"), "set ICP_HIP_LIB to a library built from commit %s: the golden file is never written from the tree under test" % PRODUCED_BY
    made = []

    def factory():
        made.append(binding.Context(0))
        return made[-1]
    result = dict(produced_by=PRODUCED_BY, contexts={name: record(make_context(factory, name)) for name in CONTEXTS})
    for c in made:
        c.close()
    for name in CONTEXTS:
        assert list(result["contexts"][name]) == keys(), name
    path = sys.argv[sys.argv.index("--write") + 1] if "--write" in sys.argv else None
    text = json.dumps(result, indent=1) + "\n"
    if path:
        with open(path, "w") as f:
            f.write(text)
    else:
        print(text)
