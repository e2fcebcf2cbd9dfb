"""The depth mesh of reconstructRoom (SimpleMesh(sensor, cameraPose, edgeThreshold), SimpleMesh.h:36-119) on the host, no GPU needed.

`mesh_spec` (tests/depth_mesh_restatement.py) is the specification the device (icp_depth_mesh, tests/test_gpu_depth_mesh.py) is held
to.  Here it is checked against a literal per-pixel transcription of the reference loop.  Also: the COFF writer, the camera glyph and joinMeshes
(SimpleMesh.h:231-302,336-359), the entry point without a device, the ctypes layout of icp_color_camera and the kernels' register budget.
"""
import ctypes as C
import os
import shutil
import subprocess
import numpy as np
import pytest
from depth_mesh_restatement import mesh_spec, mesh_literal, x86_u32, _cast_u32
from device_asm import device_asm, kernel_resources
from support import pose_of as make_pose

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
MINF = -np.inf


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
