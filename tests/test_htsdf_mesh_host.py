"""icp_tsdf_mesh_hashed on the host side: the numpy restatement of the contract (tests/htsdf_mesh_restatement.py) against the dense
restatement on the blocks' bounding box as a multiset of triangles, closedness, the classes of cells and vertices the cases must contain,
the order rule on a hand-made example, the wrappers' argument checks, the symbols, and the resource record of the new kernels (compile only)."""
import ctypes
import os
import re
import numpy as np
import pytest

import htsdf_mesh_cases as MC
import htsdf_mesh_restatement as HM
import tsdf_mesh_restatement as TM
from device_asm import device_asm, kernel_resources

f32 = np.float32
KERNELS = ("k_htm_neighbours", "k_htm_classify", "k_htm_cells", "k_htm_count", "k_htm_vertices", "k_htm_triangles")


def dense_mesh(coords, t, w, opts, min_weight=0.0):
    d_opts, T, W = MC.dense_of(coords, t, w, opts)
    vol = TM.Volume(d_opts["dims"], d_opts["origin"], voxel_size=d_opts["voxel_size"])
    vol.tsdf = T; vol.weight = W
    return TM.mesh(vol, min_weight)


CASES = [("A", MC.case_a, 0.0), ("B", MC.case_b, 0.0), ("C without (0,0,0)", lambda: MC.case_c((0, 0, 0)), 0.0),
         ("C without (-1,-1,-1)", lambda: MC.case_c((-1, -1, -1)), 0.0), ("D", MC.case_d, 0.0), ("D at min_weight 1.5", MC.case_d, 1.5), ("E", MC.case_e, 0.0)]


@pytest.mark.parametrize("name,make,mw", CASES, ids=[c[0] for c in CASES])
def test_restatement_equals_the_dense_restatement_as_a_multiset(name, make, mw):
    coords, t, w = make()
    got = HM.mesh(coords, t, w, MC.OPTS["origin"], MC.OPTS["voxel_size"], mw)
    want = dense_mesh(coords, t, w, MC.OPTS, mw)
    print("%s: V %d, T %d" % (name, len(got[0]), len(got[2])))
    assert len(got[2]) > 0 and (len(got[0]), len(got[2])) == (len(want[0]), len(want[2]))
    assert np.array_equal(HM.triangle_rows(*got), HM.triangle_rows(*want))
    assert got[2].max() == len(got[0]) - 1 and len(np.unique(got[2])) == len(got[0])      # every vertex is referenced


def test_fused_volume_equals_the_dense_restatement_as_a_multiset():
    opts, coords, t, w = MC.case_h_host("NEG")
    got = HM.mesh(coords, t, w, opts["origin"], opts["voxel_size"])
    want = dense_mesh(coords, t, w, opts)
    print("H(NEG): %d blocks, V %d, T %d" % (len(coords), len(got[0]), len(got[2])))
    assert len(got[2]) > 1000 and (len(got[0]), len(got[2])) == (len(want[0]), len(want[2]))
    assert np.array_equal(HM.triangle_rows(*got), HM.triangle_rows(*want))


def test_closed_and_open_meshes():
    for name, case, closed in (("A", MC.case_a(), True), ("B", MC.case_b(), True), ("C", MC.case_c((0, 0, 0)), False), ("C'", MC.case_c((-1, -1, -1)), False)):
        vert, nrm, tris = HM.mesh(*case, MC.OPTS["origin"], MC.OPTS["voxel_size"])
        uc, twice = TM.edge_counts(tris)
        chi = len(vert) - len(uc) + len(tris)
        print("%s: V %d, T %d, boundary edges %d, Euler characteristic %d" % (name, len(vert), len(tris), int((uc == 1).sum()), chi))
        assert twice == 0                                       # no directed edge occurs twice
        if closed:
            assert (uc == 2).all() and chi == 2
        else:
            assert uc.max() <= 2 and (uc == 1).sum() > 0
    full = HM.mesh(*MC.case_b(), MC.OPTS["origin"], MC.OPTS["voxel_size"])
    for missing in ((0, 0, 0), (-1, -1, -1)):
        assert 0 < len(HM.mesh(*MC.case_c(missing), MC.OPTS["origin"], MC.OPTS["voxel_size"])[2]) < len(full[2])


def test_the_cases_contain_every_class():
    """Crossing cells whose corners lie in 1, 2, 4 and 8 blocks, and vertices whose holding cell lies in a lower neighbour: each class must
    occur, per case where the case is there for it, so a case that lost its point fails loudly."""
    total = {1: 0, 2: 0, 4: 0, 8: 0}
    held = 0
    per = {}
    for name, case, opts in (("A", MC.case_a(), MC.OPTS), ("B", MC.case_b(), MC.OPTS), ("C", MC.case_c((0, 0, 0)), MC.OPTS), ("D", MC.case_d(), MC.OPTS), ("E", MC.case_e(), MC.OPTS),
                             ("H", MC.case_h_host("NEG")[1:], MC.case_h_host("NEG")[0])):
        st = {}
        HM.mesh(*case, opts["origin"], opts["voxel_size"], stats=st)
        print(name, st)
        per[name] = st
        for k in total:
            total[k] += st["cells_spanning"][k]
        held += st["vertices_held_below"]
    for k in total:
        assert total[k] > 0, k
    assert held > 0
    assert per["A"]["cells_spanning"] == {1: per["A"]["cells_spanning"][1], 2: 0, 4: 0, 8: 0} and per["A"]["vertices_held_below"] == 0
    for k in (1, 2, 4):                                          # B's surface crosses the block planes and their edges (the shared corner lies inside the sphere)
        assert per["B"]["cells_spanning"][k] > 0, k
    assert per["E"]["cells_spanning"][8] > 0 and per["H"]["cells_spanning"][8] > 0
    assert per["D"]["vertices_held_below"] > 0 and per["H"]["vertices_held_below"] > 0      # (the cell of the owner itself is invalid there)


def test_order_rule_on_two_blocks():
    """A plane x = 7.5 voxels between the blocks (0,0,0) and (1,0,0), given in reverse key order: every vertex is owned by a voxel with local
    x = 7 of block (0,0,0), rank 0 -- an axis edge (code 1) or a diagonal into block (1,0,0) --, ascending in (local index, code); the triangles
    ascend in the local index of their cell; and the arrays do not depend on the order the blocks are given in."""
    l = np.arange(8, dtype=np.float64)
    blocks = {}
    for b in ((1, 0, 0), (0, 0, 0)):
        x = np.broadcast_to(b[0] * 8 + l, (8, 8, 8))
        blocks[b] = (np.clip((x - 7.5) / 4.0, -1, 1).astype(f32), np.ones((8, 8, 8), f32))
    o, s = (0.0, 0.0, 0.0), 0.125
    vert, nrm, tris = HM.mesh_blocks(blocks, o, s)
    # owners: local x = 7, y and z 0 .. 7; the cells that hold the edges are y, z in 0 .. 6
    assert (vert[:, 0] == f32(7.5 * 0.125)).all() and np.array_equal(nrm, np.tile(np.array([1, 0, 0], f32), (len(nrm), 1)))
    want = []
    for z in range(8):
        for y in range(8):
            for code in (1, 3, 5, 7):
                dy, dz = (code >> 1) & 1, code >> 2
                if y + dy > 7 or z + dz > 7:
                    continue                                     # the far end lies in a block that does not exist
                if not any(0 <= y - oy <= 6 and 0 <= z - oz <= 6 for oy in ((0,) if dy else (0, 1)) for oz in ((0,) if dz else (0, 1))):
                    continue
                want.append((z * 64 + y * 8 + 7, code, y, z))
    assert len(want) == len(vert)
    t = 0.5
    for (loc, code, y, z), p in zip(want, vert):
        dy, dz = (code >> 1) & 1, code >> 2
        assert tuple(p) == (f32(0.9375), f32((y + t * dy) * 0.125), f32((z + t * dz) * 0.125)), (loc, code)
    # triangles: the 7 x 7 cells (7, y, z) in ascending local index; a triangle's cell is where the lowest of its corners lies
    g = vert[tris.astype(np.int64)].astype(np.float64) / s       # (T, 3, 3) in voxel units
    cell = np.floor(g[:, :, 2].min(1)).astype(int) * 64 + np.floor(g[:, :, 1].min(1)).astype(int) * 8 + 7
    assert (np.diff(cell) >= 0).all()
    assert sorted(set(cell.tolist())) == [z * 64 + y * 8 + 7 for z in range(7) for y in range(7)]
    same = HM.mesh_blocks({b: blocks[b] for b in sorted(blocks)}, o, s)
    for a, b in zip((vert, nrm, tris), same):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # key order is z, then y, then x: with a second pair of blocks at y = -1 those come first
    more = dict(blocks)
    for b in ((0, -1, 0), (1, -1, 0)):
        more[b] = blocks[(b[0], 0, 0)]
    v2, _, _ = HM.mesh_blocks(more, o, s)
    first_y = v2[:len(v2) // 2, 1]
    assert (first_y < 0).all() and (v2[len(v2) // 2 + 8:, 1] >= 0).all()


def test_wrapper_argument_checks():
    from icp_amd import binding, tum
    for bad in (float("nan"), -1.0, float("inf")):
        with pytest.raises(ValueError):
            binding.Context.tsdf_mesh_hashed(object(), min_weight=bad)
    seq = dict(K=np.eye(3), width=4, height=4, depth=[], rgbx=[], frames=[], gt=[])
    with pytest.raises(ValueError, match="hashed"):
        tum.reconstruct_room(None, seq, model=dict(dims=(8, 8, 8), origin=(0, 0, 0)), densify=False)
    with pytest.raises(ValueError, match="hashed"):
        tum.reconstruct_room(None, seq, densify=False)


def test_symbols_and_python_surface():
    import inspect
    from icp_amd import binding, tum
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    lib = binding.load_library()
    hdr = open(os.path.join(root, "include", "icp_hip.h")).read()
    assert "icp_tsdf_mesh_hashed" in binding.EXPORTS and hasattr(lib, "icp_tsdf_mesh_hashed") and re.search(r"^int icp_tsdf_mesh_hashed\(", hdr, flags=re.M)
    assert hasattr(lib, "icp_debug_htsdf_mesh_time") and "icp_debug_htsdf_mesh" not in hdr
    assert hasattr(binding.Context, "tsdf_mesh_hashed")
    assert inspect.signature(tum.reconstruct_room).parameters["densify"].default is True
    n = ctypes.c_int32(7)
    assert lib.icp_tsdf_mesh_hashed(None, ctypes.c_float(0), 0, 0, None, None, None, ctypes.byref(n), ctypes.byref(n)) == 1     # a null context


def test_kernel_resource_record():
    """The six kernels from the compiled code object: no scratch, no AGPRs, at most 64 VGPRs -- the first occupancy step, where the dense
    passes are pinned (tests/test_tsdf_mesh_host.py)."""
    text = device_asm()
    seen = kernel_resources(text)
    for kernel in KERNELS:
        prefix = "_ZN6icpdev%d%s" % (len(kernel), kernel)
        ks = {n: f for n, f in seen.items() if n.startswith(prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        (name, f), = ks.items()
        print("%s: %d VGPRs, %d AGPRs, scratch %d B" % (kernel, f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"]))
        assert f["private_seg_size"] == 0, f
        assert f["num_vgpr"] <= 64 and f.get("num_agpr", 0) == 0, f
