"""The coloured model without a device: the numpy restatement of its contract (tests/tsdf_color_restatement.py) against the geometry
restatements it builds on and against an analytic texture, the three colour paths of the ray-cast and the vertex-colour rule on crafted
volumes, argument validation through the library, symbols and the Python surface, the coloured PLY, the compiled kernels' resource record
and the vertex-colour kernel's own source in lockstep on the host."""
import ctypes
import inspect
import os
import re
import subprocess
import numpy as np

import tsdf_color_restatement as TC
import tsdf_mesh_restatement as TM
import tsdf_restatement as TS
from device_asm import device_asm, kernel_resources
from icp_amd.synth import tum_K as small_K, wavy_depth
from support import bits
from tsdf_color_restatement import crafted_sphere

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32
MINF = f32(-np.inf)


def test_restated_geometry_equals_the_geometry_restatements():
    """integrate_color leaves (tsdf, weight) and the count of TS.integrate; raycast_color returns TS.raycast's arrays; vertex_edges lists
    the vertices of TM.mesh in its order (their positions, recomputed from owner, code and t, have TM.mesh's bits)."""
    from icp_amd import synth
    W, H = 40, 30
    cam = TS.Camera(small_K(W), W, H)
    opts = dict(dims=(37, 21, 29), origin=(-1.8, -1.0, -0.5), voxel_size=0.1, truncation=0.3, max_weight=2.0, min_depth=0.3, max_depth=2.4)
    rng = np.random.default_rng(1)
    a = TC.add_color(TS.Volume(**opts)); b = TS.Volume(**opts)
    poses = [np.eye(4, dtype=f32), synth.make_pose((0.1, -0.25, 0.05), (0.3, -0.1, 0.2)).astype(f32)]
    for k in range(4):
        d = wavy_depth(W, H, 1.5 - 0.05 * (k & 1)); d[3, 3] = np.nan; d[10:14, 20:24] = MINF
        rgbx = rng.integers(0, 256, (W * H, 4), dtype=np.uint8)
        na, nc = TC.integrate_color(a, d, rgbx, cam, poses[k & 1])
        nb = TS.integrate(b, d, cam, poses[k & 1])
        assert na == nb and 0 < nc < na
        assert np.array_equal(bits(a.tsdf), bits(b.tsdf)) and np.array_equal(bits(a.weight), bits(b.weight))
        assert (a.wc <= a.weight).all() and ((a.wc > 0) <= (a.weight > 0)).all()
    assert a.wc.max() == 2 and (a.rgb >= 0).all() and (a.rgb <= 255).all()
    for pose in poses:
        got = TC.raycast_color(a, cam, pose); want = TS.raycast(b, cam, pose)
        assert got[4] == want[3] > 100
        for x, y in zip(got[:3], want[:3]):
            assert np.array_equal(bits(x), bits(y))
        assert ((got[6] == TC.PATH_HOLE) == (want[0].reshape(-1) == MINF)).all()
        assert got[5] == int((got[3][:, 3] == 255).sum()) == int((got[6] >= TC.PATH_NEAREST).sum())
    vol = TM.analytic_volume(TM.sphere((0.05, 0.02, 0.7), 0.4), dims=(37, 21, 29), s=0.05, origin=(-0.9, -0.5, -0.7))
    vol.weight[:, 9, :] = 0
    vert, _, _ = TM.mesh(vol)
    vl, vc = TC.vertex_edges(vol)
    assert len(vl) == len(vert) > 500
    Ff = vol.tsdf.reshape(-1)
    other = vl + (vc & 1) + ((vc >> 1) & 1) * vol.nx + (vc >> 2) * vol.nx * vol.ny
    ts = (Ff[vl] / (Ff[vl] - Ff[other])) * vol.s
    i = [vl % vol.nx, (vl // vol.nx) % vol.ny, vl // (vol.nx * vol.ny)]
    for r in range(3):
        base = vol.o[r] + i[r].astype(f32) * vol.s
        assert np.array_equal(bits(np.where(((vc >> r) & 1) == 1, base + ts, base)), bits(vert[:, r]))


def texture(x, y):
    """A smooth colour field on the plane, in byte units, per channel (fp64)."""
    return np.stack([128 + 100 * np.sin(2 * np.pi * x / 1.0) * np.cos(2 * np.pi * y / 1.3),
                     128 + 90 * np.cos(2 * np.pi * (x + 0.3 * y) / 1.1),
                     100 + 80 * np.sin(2 * np.pi * (y - 0.2 * x) / 0.9)], -1)


# the largest gradient norm of a channel of `texture`, byte units per metre: amplitude x the norm of the phase's gradient, per channel
TEXTURE_GRADIENT = max(100 * 2 * np.pi * np.hypot(1 / 1.0, 1 / 1.3), 90 * 2 * np.pi * np.hypot(1, 0.3) / 1.1, 80 * 2 * np.pi * np.hypot(1, 0.2) / 0.9)


def test_plane_texture_through_integrate_and_raycast():
    """A fronto-parallel textured plane at z0 = 1.5 fused from two poses (the camera moved sideways) and ray-cast from a third: the colour of
    a hit against the analytic texture at the hit point.  The cap is the half byte of the output's quantisation plus the texture's change
    over one voxel, TEXTURE_GRADIENT x s: a voxel takes the colour of the pixel nearest its centre's projection (half a pixel's footprint,
    0.011 m = 0.23 s here), a voxel up to one s off the plane sees the plane through its own ray (a lateral shift of at most s tan(27 deg) =
    0.5 s at the image's edge), the trilinear interpolant of a field that smooth adds curvature terms of (2 pi s / wavelength)^2 / 8 of the
    amplitude (1.5 byte), and the input's own quantisation half a byte: together below one voxel of texture.  A wrong voxel, axis or
    pixel is an error of the texture's amplitude, several times the cap.  Both numbers are printed."""
    W, H = 80, 60
    K = small_K(W)
    cam = TS.Camera(K, W, H)
    z0, s = 1.5, 0.05
    vol = TC.add_color(TS.Volume((72, 56, 24), (-1.8, -1.4, 0.95), voxel_size=s, truncation=0.2, max_weight=8))

    def frame(tx):
        u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        x = (u - float(cam.cx)) / float(cam.fx) * z0 + tx; y = (v - float(cam.cy)) / float(cam.fy) * z0
        c = np.clip(np.floor(texture(x, y) + 0.5), 0, 255).astype(np.uint8).reshape(-1, 3)
        return np.full((H, W), z0, f32), np.concatenate([c, np.full((W * H, 1), 77, np.uint8)], 1)
    for tx in (-0.1, 0.15):
        pose = np.eye(4, dtype=f32); pose[0, 3] = tx
        d, rgbx = frame(tx)
        n_upd, n_col = TC.integrate_color(vol, d, rgbx, cam, pose)
        assert 0 < n_col < n_upd
    assert vol.wc.max() == 2
    pose = np.eye(4, dtype=f32); pose[0, 3] = 0.03; pose[1, 3] = -0.02
    depth, vert, _, rgba, hits, ncol, path = TC.raycast_color(vol, cam, pose)
    ok = path == TC.PATH_EIGHT
    assert ok.sum() > 0.8 * W * H and (rgba[ok][:, 3] == 255).all()
    want = texture(vert[ok, 0].astype(np.float64) + 0.03, vert[ok, 1].astype(np.float64) - 0.02)
    err = np.abs(rgba[ok][:, :3].astype(np.float64) - want).max()
    cap = 0.5 + TEXTURE_GRADIENT * s
    print("plane texture: worst channel error %.2f bytes over %d pixels, cap %.2f (0.5 + %.1f / m x %.2f m); amplitude 100" % (err, ok.sum(), cap, TEXTURE_GRADIENT, s))
    assert err <= cap
    assert np.abs(want - want.mean(0)).max() > 2 * cap                    # the texture varies by far more than the cap over the image


def plane_volume(wc_edit):
    """A surface on the plane z = 1.0 (all weights 1), colours linear in the voxel index along x and y, Wc = 1 but where wc_edit zeroes it."""
    opts = dict(dims=(24, 20, 20), origin=(-1.15, -0.95, 0.05), voxel_size=0.1, truncation=0.2, max_weight=8.0, min_depth=0.3, max_depth=3.0)
    vol = TC.add_color(TS.Volume(**opts))
    z = (np.arange(20, dtype=f32) * f32(0.1) + f32(0.05))[:, None, None]
    vol.tsdf = np.broadcast_to(np.clip((f32(1.0) - z) / f32(0.2), -1, 1), (20, 20, 24)).astype(f32).copy()
    vol.weight = np.ones_like(vol.tsdf)
    i = np.arange(24, dtype=f32)[None, None, :]; j = np.arange(20, dtype=f32)[None, :, None]
    vol.rgb[..., 0] = 10 + 8 * i; vol.rgb[..., 1] = 20 + 10 * j; vol.rgb[..., 2] = 250 - 4 * i - 3 * j
    vol.wc[:] = 1
    wc_edit(vol.wc)
    return vol


def test_three_colour_paths_on_a_crafted_volume():
    """Eight corners: the lerp of a colour field linear in the index reproduces it at the hit (to the byte).  A slab of Wc = 0: cells next to
    it take the nearest corner's colour when that corner lies outside the slab; cells inside it, and cells whose nearest corner is in it,
    have no colour: four zero bytes on a pixel that has a depth."""
    W, H = 32, 24
    cam = TS.Camera(small_K(W), W, H)
    eye = np.eye(4, dtype=f32)

    def edit(wc):
        wc[:, :, 10:14] = 0
    vol = plane_volume(edit)
    depth, vert, nrm, rgba, hits, ncol, path = TC.raycast_color(vol, cam, eye)
    assert hits == W * H and np.abs(depth - 1.0).max() < 1e-5
    n8, nn, n0 = [(path == p).sum() for p in (TC.PATH_EIGHT, TC.PATH_NEAREST, TC.PATH_NONE)]
    print("crafted paths: eight %d, nearest %d, none %d" % (n8, nn, n0))
    assert n8 > 100 and nn > 20 and n0 > 20 and n8 + nn + n0 == hits and ncol == n8 + nn
    gx = (vert[:, 0].astype(np.float64) + 1.15) / 0.1; gy = (vert[:, 1].astype(np.float64) + 0.95) / 0.1
    want = np.stack([10 + 8 * gx, 20 + 10 * gy, 250 - 4 * gx - 3 * gy], 1)
    e = path == TC.PATH_EIGHT
    assert np.abs(rgba[e][:, :3] - want[e]).max() <= 0.5 + 1e-3 and (rgba[e][:, 3] == 255).all()
    # nearest: the colour of the voxel nearest the hit in x and y (z: both planes hold the same colours), which lies outside the slab
    ne = path == TC.PATH_NEAREST
    ix = np.floor(gx[ne] + 0.5); iy = np.floor(gy[ne] + 0.5)
    assert ((ix < 10) | (ix > 13)).all()
    assert np.array_equal(rgba[ne][:, :3], np.stack([10 + 8 * ix, 20 + 10 * iy, 250 - 4 * ix - 3 * iy], 1).astype(np.uint8))
    no = path == TC.PATH_NONE
    assert not rgba[no].any() and np.isfinite(depth.reshape(-1)[no]).all()
    ixn = np.floor(gx[no] + 0.5)
    assert ((ixn >= 10) & (ixn <= 13)).all()
    # the coloured target drops exactly the uncoloured hits
    tv, tn, trgba, tcnt = TC.colored_target(vol, cam, eye)
    assert tcnt == ncol and ((tv[:, 2] == MINF) == no).all() and ((tn[:, 0] == MINF) == no).all() and np.array_equal(trgba, rgba)
    # the byte rule: clamp, round half up, NaN to 0
    assert list(TC.color_byte(np.array([-3, 0.49999, 0.5, 254.5, 300, np.nan], f32))) == [0, 0, 1, 255, 255, 0]


def test_vertex_colour_rule():
    """Both ends coloured: the lerp at the vertex's t; one end: that end's colour; neither: four zero bytes -- on the plane volume, whose
    surface z = 1.0 crosses the edges between the voxel planes k = 9 (F = 0.25) and k = 10 (F = -0.25): t = 0.5 on every edge."""
    def edit(wc):
        wc[10, :, 8:] = 0             # upper ends uncoloured from i = 8
        wc[9, :, 16:] = 0             # both ends uncoloured from i = 16
    vol = plane_volume(edit)
    vert, nrm, tris = TM.mesh(vol)
    col = TC.mesh_colors(vol)
    vl, vc = TC.vertex_edges(vol)
    assert len(col) == len(vert) > 0 and (vl // (24 * 20) == 9).all() and ((vc >> 2) == 1).all()
    i = vl % 24; j = (vl // 24) % 20
    i2 = i + (vc & 1); j2 = j + ((vc >> 1) & 1)
    lo = lambda a, b: np.stack([10 + 8 * a, 20 + 10 * b, 250 - 4 * a - 3 * b], 1).astype(np.float64)
    both = (i < 16) & (i2 < 8); one = (i < 16) & (i2 >= 8); none = (i >= 16)
    assert both.sum() > 50 and one.sum() > 50 and none.sum() > 50
    assert np.array_equal(col[both][:, :3], np.floor(0.5 * (lo(i, j) + lo(i2, j2))[both] + 0.5).astype(np.uint8)) and (col[both][:, 3] == 255).all()
    assert np.array_equal(col[one][:, :3], lo(i, j)[one].astype(np.uint8)) and (col[one][:, 3] == 255).all()
    assert not col[none].any()
    # the lower end uncoloured, the upper one coloured: the upper end's colour
    vol2 = plane_volume(lambda wc: wc.__setitem__((9, slice(None), slice(None)), 0))
    col2 = TC.mesh_colors(vol2)
    assert np.array_equal(col2[:, :3], lo(i2, j2).astype(np.uint8)) and (col2[:, 3] == 255).all()


def test_argument_validation_without_a_device():
    """Every new entry point refuses a null context with ICP_ERR_INVALID_ARG before it touches anything."""
    from icp_amd import binding
    lib = binding.load_library()
    n = ctypes.c_int32(7)
    assert lib.icp_tsdf_color_create(None) == 1 and lib.icp_tsdf_color_release(None) == 1
    assert lib.icp_tsdf_color_download(None, None, None) == 1 and lib.icp_tsdf_color_upload(None, None, None) == 1
    assert lib.icp_tsdf_integrate_color(None, None, None, None, None, None, None) == 1
    assert lib.icp_tsdf_raycast_color(None, None, None, None, None, None, None, None, None) == 1
    assert lib.icp_set_target_tsdf_color(None, None, None, None) == 1
    assert lib.icp_track_depth_model_color(None, None, None, 0, None, None, None, None, None) == 1
    assert lib.icp_tsdf_mesh_color(None, ctypes.c_float(0), 0, 0, None, None, None, None, ctypes.byref(n), ctypes.byref(n)) == 1


NEW_SYMBOLS = ["icp_tsdf_color_create", "icp_tsdf_color_release", "icp_tsdf_color_download", "icp_tsdf_color_upload", "icp_tsdf_integrate_color",
               "icp_tsdf_raycast_color", "icp_set_target_tsdf_color", "icp_track_depth_model_color", "icp_tsdf_mesh_color"]


def test_symbols_header_and_python_surface():
    from icp_amd import binding, meshio, tum
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in binding.EXPORTS and hasattr(lib, name) and re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    assert "2 GiB" in hdr                                                   # the header says what the colour array costs at 512^3
    assert ctypes.sizeof(binding.IcpTsdfOptions) == 12 + 12 + 6 * 4         # the options keep their layout
    sig = lambda f: inspect.signature(f).parameters
    Ctx = binding.Context
    assert sig(Ctx.tsdf_create)["color"].default is False and list(sig(Ctx.tsdf_create))[:3] == ["self", "options", "color"]
    assert sig(Ctx.tsdf_integrate)["rgbx"].default is None and list(sig(Ctx.tsdf_integrate)) == ["self", "depth", "cam", "pose", "rgbx"]
    assert sig(Ctx.set_target_tsdf)["color"].default is False and list(sig(Ctx.set_target_tsdf)) == ["self", "cam", "pose", "check", "color"]
    assert sig(Ctx.track_depth_model)["rgbx_frames"].default is None and list(sig(Ctx.track_depth_model))[:6] == ["self", "depth_frames", "cam", "source_opt", "gt", "pose"]
    assert sig(Ctx.tsdf_mesh)["colors"].default is False and sig(Ctx.tsdf_mesh)["min_weight"].default == 0.0
    for name in ("tsdf_color_create", "tsdf_color_release", "tsdf_color_volume", "tsdf_color_upload", "tsdf_raycast_color"):
        assert hasattr(Ctx, name), name
    assert sig(meshio.write_ply_mesh)["colors"].default is None and sig(meshio.load_ply_mesh)["colors"].default is False
    assert "fix_color_index" in tum.track.__doc__ and "color=True" in tum.track.__doc__


def test_coloured_ply_round_trip(tmp_path):
    from icp_amd import meshio
    rng = np.random.default_rng(4)
    v = rng.normal(size=(11, 3)).astype(f32); n = rng.normal(size=(11, 3)).astype(f32); t = rng.integers(0, 11, (7, 3)).astype(np.uint32)
    c = rng.integers(0, 256, (11, 4), dtype=np.uint8)
    p = str(tmp_path / "c.ply")
    meshio.write_ply_mesh(p, v, n, t, colors=c)
    head = open(p, "rb").read(400).decode("ascii", "ignore")
    assert "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n" in head
    got = meshio.load_ply_mesh(p, colors=True)
    assert len(got) == 4 and all(np.array_equal(a, b) for a, b in zip(got, (v, n, t, c)))
    old = meshio.load_ply_mesh(p)
    assert len(old) == 3 and all(np.array_equal(a, b) for a, b in zip(old, (v, n, t)))           # the default keeps the 3-tuple
    q = str(tmp_path / "g.ply")
    meshio.write_ply_mesh(q, v, n, t)
    assert len(meshio.load_ply_mesh(q)) == 3 and meshio.load_ply_mesh(q, colors=True)[3] is None
    assert "red" not in open(q, "rb").read(400).decode("ascii", "ignore")


def test_kernel_resource_record():
    """The new kernels from the compiled code object: no scratch, no AGPRs, static LDS no more than their block sums (two counters of four
    waves for the two TSDF kernels, one for the mesh colours).  VGPRs recorded in DESIGN.md section 6p: k_tsdf_integrate_color 34,
    k_tsdf_raycast_color 55 in both forms, k_tm_colors 31 -- each pinned at 64, the first occupancy step at or above it."""
    text = device_asm()
    seen = kernel_resources(text)
    budget = {"_ZN6icpdev22k_tsdf_integrate_color": (64, 32), "_ZN6icpdev20k_tsdf_raycast_colorILb0E": (64, 32),
              "_ZN6icpdev20k_tsdf_raycast_colorILb1E": (64, 32), "_ZN6icpdev11k_tm_colors": (64, 16)}
    for prefix, (cap, lds_cap) in budget.items():
        ks = {n: f for n, f in seen.items() if n.startswith(prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        (name, f), = ks.items()
        desc = text[text.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        print("%s: %d VGPRs, %d AGPRs, scratch %d B, static LDS %d B" % (prefix, f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"], lds))
        assert f["private_seg_size"] == 0, f
        assert f["num_vgpr"] <= cap and f.get("num_agpr", 0) == 0, f
        assert lds <= lds_cap, lds


def test_vertex_colour_kernel_in_lockstep_on_the_host(tmp_path):
    """k_tm_colors' own source (dev_tsdf_mesh_color.hpp) run on the host, a thread per lane with ballots as wave barriers
    (tests/tsdf_mesh_color_lockstep.cpp), against the restatement bit for bit: the sphere with unobserved voxels, NaN, inf and exact zeros
    in a 37 x 21 x 29 volume (23 blocks, a partial last run) with a crafted colour array (Wc = 0 scattered and in a slab, NaN and
    out-of-range channels), and a random field with every case of every tetrahedron."""
    exe = str(tmp_path / "lockstep")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-w", "-I", os.path.join(ROOT, "icp-variants_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "tsdf_mesh_color_lockstep.cpp")], timeout=300)

    def run(vol, mw):
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([vol.nx, vol.ny, vol.nz], np.int32).tobytes())
            f.write(np.array([vol.o[0], vol.o[1], vol.o[2], vol.s, mw], f32).tobytes())
            f.write(np.stack([vol.tsdf.reshape(-1), vol.weight.reshape(-1)], 1).astype(f32).tobytes())
            f.write(np.concatenate([vol.rgb.reshape(-1, 3), vol.wc.reshape(-1, 1)], 1).astype(f32).tobytes())
        subprocess.check_call([exe, src, dst], timeout=300)
        d = open(dst, "rb").read()
        nv = int(np.frombuffer(d, np.int32, 1)[0])
        got = np.frombuffer(d, np.uint8, nv * 4, 4).reshape(nv, 4)
        want = TC.mesh_colors(vol, mw)
        assert nv == len(want) == len(TM.mesh(vol, mw)[0]) and nv > 0
        assert np.array_equal(got, want)
        return want
    vol = crafted_sphere()
    want = run(vol, 0.0)
    assert (want[:, 3] == 0).sum() > 20 and (want[:, 3] == 255).sum() > 500
    rng = np.random.default_rng(11)
    rnd = TC.add_color(TM.Volume((19, 11, 13), (-1.8, -1.0, -0.5), voxel_size=0.1))
    rnd.tsdf = rng.uniform(-1, 1, (13, 11, 19)).astype(f32); rnd.weight = rng.choice(np.array([0, 1, 1.5], f32), (13, 11, 19), p=[0.1, 0.3, 0.6])
    rnd.rgb = rng.uniform(0, 255, (13, 11, 19, 3)).astype(f32); rnd.wc = rng.choice(np.array([0, 1, 3], f32), (13, 11, 19), p=[0.3, 0.4, 0.3])
    run(rnd, 0.0); run(rnd, 1.5)


def test_outcome_fixture_and_its_golden_file():
    """The wall fixture is what DESIGN.md section 6p says: 12 frames of 160 x 120, 1 cm per frame, a texture that is not constant along the
    travel, a volume that holds the field of view plus the travel; and the golden file records the separation of the two restatement loops
    (written by tests/tsdf_color_outcome_fixture.py, which refuses to write it otherwise)."""
    import json
    import tsdf_color_outcome_fixture as CF
    K, depth, rgbx, gt = CF.fixture()
    assert depth.shape == (12, 120, 160) and rgbx.shape == (12, 160 * 120, 4) and len(gt) == 11
    assert np.abs(depth - CF.WALL_Z).max() < 5 * CF.SIGMA + 1e-4 and len(np.unique(depth)) > 10
    assert [float(g[0, 3]) for g in gt] == [float(f32(CF.STEP_M * k)) for k in range(1, 12)]
    # the shortest wavelength of the texture (the phase's gradient norm) is at least 8 voxels
    shortest = min(0.61 / np.hypot(1, 0.31), 0.43 / np.hypot(0.45, 1), 0.37 / np.hypot(1, 0.22), 0.79 / np.hypot(0.3, 1), 0.53 / np.hypot(0.8, 0.6), 0.97 / np.hypot(1, 0.1))
    assert shortest >= 8 * CF.VOLUME["voxel_size"]
    a, b = rgbx[0].reshape(120, 160, 4)[:, :, :3].astype(int), rgbx[11].reshape(120, 160, 4)[:, :, :3].astype(int)
    assert np.abs(a - b).mean() > 10                                         # 11 cm of travel is visible in the colours
    half_w = 80 / float(K[0, 0]) * CF.WALL_Z
    o, d, s = CF.VOLUME["origin"], CF.VOLUME["dims"], CF.VOLUME["voxel_size"]
    assert o[0] < -half_w and o[0] + (d[0] - 1) * s > half_w + 0.11 and o[2] < CF.WALL_Z - CF.VOLUME["truncation"] and o[2] + (d[2] - 1) * s > CF.WALL_Z + CF.VOLUME["truncation"]
    ref = json.load(open(CF.GOLDEN))
    assert ref["frames"] == CF.N_FRAMES and ref["lateral_travel_m"] == CF.STEP_M * (CF.N_FRAMES - 1)
    assert 2 * ref["colored_worst_translation_m"] < ref["lateral_travel_m"] / 2 < ref["geometric_last_translation_m"]
