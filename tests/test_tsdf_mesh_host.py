"""icp_tsdf_mesh on the host side: properties of the numpy restatement of the contract (tests/tsdf_mesh_restatement.py) on analytic
volumes -- closed, consistently oriented, the right topology, volume and normals --, its behaviour on partly unobserved volumes, exact
zeros and non-finite values, the device's case table against the generated one, the resource record of the five kernels (compile only)
and the PLY round trip."""
import ctypes
import os
import re
import numpy as np

import tsdf_mesh_restatement as TM
from device_asm import device_asm, kernel_resources

f32 = np.float32
CENTRE = np.array([0.013, -0.021, 0.034])                        # off the grid


analytic_volume = TM.analytic_volume
sphere = TM.sphere(CENTRE, 0.6)
torus = TM.torus(CENTRE, 0.55, 0.25)


def check_manifold(vert, tris, closed):
    """Shared checks; returns the per-undirected-edge triangle counts."""
    t = tris.astype(np.int64)
    assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()      # no degenerate index triple
    assert t.min() >= 0 and t.max() < len(vert)
    assert len(np.unique(t)) == len(vert)                      # every vertex is referenced
    uc, twice = TM.edge_counts(tris)
    assert twice == 0                                           # no directed edge appears twice
    if closed:
        assert (uc == 2).all()
    else:
        assert uc.max() <= 2
    return uc


def test_closed_surfaces_sphere_and_torus():
    for name, fn, euler in (("sphere", sphere, 2), ("torus", torus, 0)):
        vol = analytic_volume(fn)
        vert, nrm, tris = TM.mesh(vol)
        uc = check_manifold(vert, tris, closed=True)
        chi = len(vert) - len(uc) + len(tris)
        print("%s: V %d, T %d, Euler characteristic %d" % (name, len(vert), len(tris), chi))
        assert len(tris) > 1000 and chi == euler
        if name == "sphere":
            vol_mesh, vol_true = TM.signed_volume(vert, tris), 4.0 / 3.0 * np.pi * 0.6 ** 3
            dist = np.abs(np.linalg.norm(vert - CENTRE, axis=1) - 0.6).max()
            print("sphere: signed volume %.4f (analytic %.4f), max vertex distance from the sphere %.4f" % (vol_mesh, vol_true, dist))
            assert vol_mesh > 0 and abs(vol_mesh - vol_true) < 0.03 * vol_true
            assert dist < 0.01                                   # a tenth of a voxel: the linear crossing of a field with curvature 1 / 0.6
            radial = vert - CENTRE
        else:
            q = vert - CENTRE
            ring = np.concatenate([q[:, :2] / np.linalg.norm(q[:, :2], axis=1, keepdims=True) * 0.55, np.zeros((len(q), 1))], 1)
            radial = q - ring                                    # outward from the torus' centre circle
            assert TM.signed_volume(vert, tris) > 0
        assert (np.einsum("ij,ij->i", nrm.astype(np.float64), radial) > 0).all()
        assert np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_partly_unobserved_volumes():
    """A slab and a small block of zero weights; and min_weight > 0 on mixed weights: the mesh opens (boundary edges), stays consistently
    oriented, references every vertex and takes no triangle from an invalid cell."""
    vol = analytic_volume(sphere)
    vol.weight[:, 9, :] = 0                                     # a slab through the middle
    vol.weight[3:6, 12:15, 8:11] = 0                           # a block on the surface (z index 3..5 cuts the lower cap)
    mixed = analytic_volume(sphere)
    mixed.weight = np.random.default_rng(4).choice(np.array([1, 2, 3], f32), mixed.weight.shape, p=[0.03, 0.47, 0.5])
    full = TM.mesh(analytic_volume(sphere))
    for what, v, mw in (("zero weights", vol, 0.0), ("min_weight 2 on mixed weights", mixed, 2.0)):
        vert, nrm, tris = TM.mesh(v, mw)
        uc = check_manifold(vert, tris, closed=False)
        print("%s: V %d, T %d, boundary edges %d" % (what, len(vert), len(tris), int((uc == 1).sum())))
        assert (uc == 1).sum() > 0 and 0 < len(tris) < len(full[2])
        # every triangle lies inside one valid cell: its vertices fit a unit cell whose eight corners are observed
        valid = TM.valid_cells(v, mw)
        g = (vert.astype(np.float64) - v.o.astype(np.float64)) / float(v.s)
        tri_g = g[tris.astype(np.int64)]                       # (T, 3, 3)
        cell = np.floor(tri_g.mean(axis=1) + 1e-9).astype(int)
        cell = np.clip(cell, 0, [v.nx - 2, v.ny - 2, v.nz - 2])
        assert (np.abs(tri_g - (cell[:, None, :] + 0.5)).max(axis=(1, 2)) <= 0.5 + 1e-4).all()
        assert valid[cell[:, 2], cell[:, 1], cell[:, 0]].all()
    assert np.array_equal(TM.mesh(mixed, 0.0)[2], full[2])      # at min_weight 0 the mixed weights change nothing
    # nothing observed: an empty mesh
    vol.weight[:] = 0
    vert, nrm, tris = TM.mesh(vol)
    assert vert.shape == (0, 3) and nrm.shape == (0, 3) and tris.shape == (0, 3)


def test_exact_zeros_and_non_finite_values():
    # a plane through voxel centres: F = z - 0.5 on dyadic coordinates has exact zeros on one layer
    vol = TM.Volume((9, 8, 10), (0.0, 0.0, 0.0), voxel_size=0.125)
    z = (np.arange(10, dtype=f32) * f32(0.125))[:, None, None]
    vol.tsdf = np.broadcast_to(z - f32(0.5), (10, 8, 9)).astype(f32).copy(); vol.weight = np.ones_like(vol.tsdf)
    assert (vol.tsdf[4] == 0).all()
    vert, nrm, tris = TM.mesh(vol)
    uc = check_manifold(vert, tris, closed=False)              # distinct indices throughout
    assert (vert[:, 2] == 0.5).all()                           # t is 1 on every crossing edge (from z = 0.375 up to the zero layer)
    assert len(np.unique(vert, axis=0)) < len(vert)            # coincident vertices ...
    area = np.linalg.norm(np.cross(vert[tris[:, 1]] - vert[tris[:, 0]], vert[tris[:, 2]] - vert[tris[:, 0]]), axis=1)
    assert (area == 0).any() and (area > 0).any()              # ... and zero-area triangles, kept
    assert np.array_equal(nrm, np.tile(np.array([0, 0, 1], f32), (len(nrm), 1)))
    # NaN and +-inf: their cells are invalid and nothing non-finite reaches an output
    base = analytic_volume(sphere)
    full = TM.mesh(base)
    for bad in (np.nan, np.inf, -np.inf):
        vol = analytic_volume(sphere)
        vol.tsdf[4, 10, 10] = bad; vol.tsdf[10, 4, 9] = bad; vol.tsdf[0, 0, 0] = bad
        vert, nrm, tris = TM.mesh(vol)
        uc = check_manifold(vert, tris, closed=False)
        assert np.isfinite(vert).all() and np.isfinite(nrm).all() and (uc == 1).sum() > 0 and len(tris) < len(full[2])
        same = TM.Volume((vol.nx, vol.ny, vol.nz), vol.o, voxel_size=float(vol.s))
        same.tsdf = base.tsdf.copy(); same.weight = np.where(np.isfinite(vol.tsdf), 1, 0).astype(f32)
        for a, b in zip(TM.mesh(same), (vert, nrm, tris)):      # exactly the mesh of the volume with those voxels unobserved
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_generated_table_shape():
    """What the rule implies, on the generated table: every case with corners on both sides gives one or two triangles, a case and its
    complement give the same edges in the opposite order, and the six tetrahedra share the corners (0,0,0) and (1,1,1)."""
    T = TM.tet_table()
    Q = TM.tet_corners()
    assert [tuple(p) for p in TM.PERMS] == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    assert (Q[:, 0] == 0).all() and (Q[:, 3] == 1).all() and (np.diff(Q, axis=1).sum(axis=2) == 1).all()
    for p in range(6):
        assert T[p][0] == [] and T[p][15] == []
        for m in range(1, 15):
            n_neg = bin(m).count("1")
            assert len(T[p][m]) == (2 if n_neg == 2 else 1)
            edges = {e for t in T[p][m] for e in t}
            assert edges == {r for r, (a, b) in enumerate(TM.EDGES) if ((m >> a) & 1) != ((m >> b) & 1)}
            assert {e for t in T[p][15 - m] for e in t} == edges
            if len(T[p][m]) == 1:
                e = T[p][m][0]
                assert T[p][15 - m] == [(e[0], e[2], e[1])]
            else:
                (e0, e1, e2), (_, _, e3) = T[p][m]
                assert T[p][15 - m] == [(e0, e3, e2), (e0, e2, e1)]
            assert T[p][m][0][0] == min(edges)


def test_device_table_equals_generated_table():
    from icp_amd import binding
    lib = binding.load_library()
    table = (ctypes.c_int32 * (6 * 16 * 7))(); corners = (ctypes.c_int32 * 24)()
    assert lib.icp_debug_tsdf_mesh_table(table, corners) == 0
    assert lib.icp_debug_tsdf_mesh_table(None, corners) == 1
    table = np.array(table).reshape(6, 16, 7); corners = np.array(corners).reshape(6, 4)
    T = TM.tet_table()
    Q = TM.tet_corners()
    assert np.array_equal(corners, Q @ np.array([1, 2, 4]))
    for p in range(6):
        for m in range(16):
            want = [len(T[p][m])] + [e for t in T[p][m] for e in t]
            want += [-1] * (7 - len(want))
            assert table[p, m].tolist() == want, (p, m)


def test_kernel_source_in_lockstep_on_the_host(tmp_path):
    """The kernels' own source (dev_tsdf_mesh.hpp) run on the host, a thread per lane with ballots as wave barriers
    (tests/tsdf_mesh_lockstep.cpp), against the restatement bit for bit: a sphere with unobserved voxels, NaN, inf and exact zeros in a
    37 x 21 x 29 volume (23 blocks, a partial last run), and a random field with weights in {0, 1, 1.5} (every case of every tetrahedron)
    at min_weight 0 and 1.5."""
    import subprocess
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    exe = str(tmp_path / "lockstep")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-ffp-contract=off", "-pthread", "-w", "-I", os.path.join(root, "icp-variants_amd", "csrc"),
                           "-o", exe, os.path.join(root, "tests", "tsdf_mesh_lockstep.cpp")], timeout=300)

    def run(vol, mw):
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            f.write(np.array([vol.nx, vol.ny, vol.nz], np.int32).tobytes())
            f.write(np.array([vol.o[0], vol.o[1], vol.o[2], vol.s, mw], f32).tobytes())
            f.write(np.stack([vol.tsdf.reshape(-1), vol.weight.reshape(-1)], 1).astype(f32).tobytes())
        subprocess.check_call([exe, src, dst], timeout=300)
        d = open(dst, "rb").read()
        nv, nt = (int(x) for x in np.frombuffer(d, np.int32, 2))
        got = (np.frombuffer(d, np.uint32, nv * 3, 8).reshape(nv, 3), np.frombuffer(d, np.uint32, nv * 3, 8 + nv * 12).reshape(nv, 3),
               np.frombuffer(d, np.uint32, nt * 3, 8 + nv * 24).reshape(nt, 3))
        want = TM.mesh(vol, mw)
        assert (nv, nt) == (len(want[0]), len(want[2])) and nt > 0
        for a, b in zip(got, want):
            assert np.array_equal(a, b.view(np.uint32))
    vol = analytic_volume(TM.sphere(CENTRE, 0.4), dims=(37, 21, 29), s=0.05, origin=(-0.9, -0.5, -0.7))
    rng = np.random.default_rng(11)
    vol.weight[:, 9, :] = 0; vol.weight[rng.random(vol.weight.shape) < 0.02] = 0
    vol.tsdf[rng.random(vol.tsdf.shape) < 0.01] = np.nan
    vol.tsdf[5, 10, 12] = np.inf; vol.tsdf[20, 8, 30] = -np.inf; vol.tsdf[14, 3:8, 4:30] = 0.0
    run(vol, 0.0)
    rnd = TM.Volume((19, 11, 13), (-1.8, -1.0, -0.5), voxel_size=0.1)
    rnd.tsdf = rng.uniform(-1, 1, (13, 11, 19)).astype(f32); rnd.weight = rng.choice(np.array([0, 1, 1.5], f32), (13, 11, 19), p=[0.1, 0.3, 0.6])
    run(rnd, 0.0); run(rnd, 1.5)


def test_symbols_and_python_surface():
    import inspect
    from icp_amd import binding, meshio, tum
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    lib = binding.load_library()
    hdr = open(os.path.join(root, "include", "icp_hip.h")).read()
    assert "icp_tsdf_mesh" in binding.EXPORTS and hasattr(lib, "icp_tsdf_mesh") and re.search(r"^int icp_tsdf_mesh\(", hdr, flags=re.M)
    assert hasattr(lib, "icp_debug_tsdf_mesh_time") and "icp_debug_tsdf_mesh" not in hdr
    assert hasattr(binding.Context, "tsdf_mesh") and hasattr(meshio, "write_ply_mesh") and hasattr(meshio, "load_ply_mesh")
    assert inspect.signature(tum.reconstruct_room).parameters["model_mesh"].default is None
    n = ctypes.c_int32(7)
    assert lib.icp_tsdf_mesh(None, ctypes.c_float(0), 0, 0, None, None, None, ctypes.byref(n), ctypes.byref(n)) == 1     # a null context


def test_kernel_resource_record():
    """The five kernels from the compiled code object: no scratch, no AGPRs, and VGPR budgets pinned at the next occupancy step (8 waves
    per SIMD up to 64 registers, 7 up to 72, 6 up to 80, 5 up to 96, 4 up to 128) above what the compiler reports.  Recorded (DESIGN.md
    section 6n): k_tm_classify 14, k_tm_cells 30, k_tm_count 51, k_tm_vertices 44, k_tm_triangles 44 -- all within 64, full occupancy, what
    passes that wait on memory want.  Static LDS is the wave counts (at most 32 B)."""
    text = device_asm()
    seen = kernel_resources(text)
    for kernel in ("k_tm_classify", "k_tm_cells", "k_tm_count", "k_tm_vertices", "k_tm_triangles"):
        prefix = "_ZN6icpdev%d%s" % (len(kernel), kernel)
        ks = {n: f for n, f in seen.items() if n.startswith(prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        (name, f), = ks.items()
        desc = text[text.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        print("%s: %d VGPRs, %d AGPRs, scratch %d B, static LDS %d B" % (kernel, f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"], lds))
        assert f["private_seg_size"] == 0, f
        assert f["num_vgpr"] <= 64 and f.get("num_agpr", 0) == 0, f
        assert lds <= 32, lds


def test_ply_mesh_round_trip(tmp_path):
    from icp_amd import meshio
    vert, nrm, tris = TM.mesh(analytic_volume(sphere))
    path = str(tmp_path / "sphere.ply")
    meshio.write_ply_mesh(path, vert, nrm, tris)
    v2, n2, t2 = meshio.load_ply_mesh(path)
    assert v2.dtype == f32 and n2.dtype == f32 and t2.dtype == np.uint32
    assert np.array_equal(v2.view(np.uint32), vert.view(np.uint32)) and np.array_equal(n2.view(np.uint32), nrm.view(np.uint32)) and np.array_equal(t2, tris)
    with open(path, "rb") as f:
        head = f.read(260).decode("ascii", "replace")
    assert head.startswith("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n" % len(vert))
    assert "property float nz\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(tris) in head
    assert os.path.getsize(path) == len(meshio.PLY_MESH_HEADER % (len(vert), len(tris))) + 24 * len(vert) + 13 * len(tris)
    empty = str(tmp_path / "empty.ply")
    meshio.write_ply_mesh(empty, np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros((0, 3), np.uint32))
    v0, n0, t0 = meshio.load_ply_mesh(empty)
    assert v0.shape == (0, 3) and n0.shape == (0, 3) and t0.shape == (0, 3)
