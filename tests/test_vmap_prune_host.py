"""The local voxel map on the host side: the new struct, symbols, signatures and Python surface, the refusals that need no device, the
prune predicate on cases that are exact in fp32, the identity the feature rests on (insert everything, then prune == insert only the
points whose cell survives, bit for bit) in the numpy restatement for both storages, the compaction rule on a scripted sequence, and the
resource record of the three new kernels (compile only)."""
import ctypes
import inspect
import os
import re
import numpy as np
import pytest

import vgicp_restatement as VR
import vmap_restatement as MR
import hmap_restatement as HR
import vmap_prune_restatement as PR
import vmap_outcome_fixture as MF
from device_asm import device_asm, kernel_resources
from support import pose_of

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32, f64 = np.float32, np.float64
EYE = np.eye(4, dtype=f32)
POSE_A = ((0.05, -0.04, 0.3), (0.4, -0.3, 0.2))
POSE_B = ((-0.1, 0.08, -0.25), (-0.35, 0.2, 0.1))


def test_struct_symbols_and_python_surface():
    from icp_amd import binding, eth
    T = binding.IcpVoxelMapPruneInfo
    assert ctypes.sizeof(T) == 32 and T.n_points_removed.offset == 24 and T.capacity.offset == 16
    assert [f[0] for f in T._fields_] == ["n_removed", "n_occupied", "n_vacated", "n_compacted", "capacity", "reserved", "n_points_removed"]
    assert ctypes.sizeof(binding.IcpVoxelHashMapInfo) == 32      # (keeps its layout)
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    sig = {"icp_voxel_map_prune": r"icp_ctx\* ctx, const float centre\[3\], float radius, icp_voxel_map_prune_info\* info_out",
           "icp_voxel_map_compact": r"icp_ctx\* ctx",
           "icp_track_scans_vmap_local": r"icp_ctx\* ctx, const float\* const\* xyz, const float\* const\* normals, const int32_t\* n, int32_t n_scans,\s+"
                                         r"const icp_vgicp_options\* opt, float keep_radius, float pose_inout\[16\], icp_vgicp_record\* out,\s+icp_voxel_map_prune_info\* prune_out"}
    for name, args in sig.items():
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(%s\);" % (name, args), hdr, flags=re.M), name
    assert re.search(r"^\} icp_voxel_map_prune_info;", hdr, flags=re.M) and "static_assert(sizeof(icp_voxel_map_prune_info) == 32" in hdr
    for m in ("voxel_map_prune", "voxel_map_compact"):
        assert hasattr(binding.Context, m), m
    assert list(inspect.signature(binding.Context.voxel_map_prune).parameters) == ["self", "centre", "radius"]
    par = inspect.signature(binding.Context.track_scans_vmap).parameters
    assert list(par)[:4] == ["self", "scans", "pose", "keep_radius"] and par["keep_radius"].default is None
    assert inspect.signature(eth.track_map).parameters["keep_radius"].default is None
    assert tuple(PR.PRUNE_INFO) == tuple(f[0] for f in T._fields_ if f[0] != "reserved")


def test_refusals_without_a_device():
    """A null context is refused by every new entry point; the restatement refuses what the contract refuses."""
    from icp_amd import binding
    lib = binding.load_library()
    ce = np.zeros(3, f32); p = binding.pose_to_c(np.eye(4)); o = binding.vgicp_options()
    assert lib.icp_voxel_map_prune(None, binding._ptr(ce), ctypes.c_float(1.0), None) == 1
    assert lib.icp_voxel_map_compact(None) == 1
    assert lib.icp_track_scans_vmap_local(None, None, None, None, 1, ctypes.byref(o), ctypes.c_float(1.0), binding._ptr(p), None, None) == 1
    m = MR.create(0.25, (0, 0, 0), (2, 2, 2))
    for centre, radius in (((np.nan, 0, 0), 1.0), ((0, np.inf, 0), 1.0), ((0, 0, 0), -1.0), ((0, 0, 0), np.nan), ((0, 0, 0), np.inf)):
        with pytest.raises(PR.BadOptions):
            PR.prune(m, centre, radius)
    for r in (0.0, -2.0, np.nan, np.inf):
        with pytest.raises(PR.BadOptions):
            PR.track_local(m, [], EYE, 1e-3, r)


def block9(hashed):
    """Voxel 0.25, the 9 x 9 x 9 block of cells 0 .. 8 with one point each at the cell's centre (exact in fp32)."""
    g = np.arange(9)
    cc = np.stack([a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij")], 1)
    pts = ((cc + 0.5) * 0.25).astype(f32)
    assert np.array_equal(pts.astype(f64), (cc + 0.5) * 0.25)
    nrm = np.tile(np.array([[0.6, 0.0, 0.8]], f32), (len(pts), 1))
    m = HR.create(0.25, 256) if hashed else MR.create(0.25, (0, 0, 0), (9, 9, 9))
    PR.insert(m, pts, nrm, EYE)
    return m, cc, pts, nrm


CENTRE9 = (1.125, 1.125, 1.125)                     # the centre of cell (4, 4, 4)


@pytest.mark.parametrize("hashed", [False, True])
def test_predicate_on_exact_cases(hashed):
    """Radius 0.75 = three cells: the kept set is exactly dx^2 + dy^2 + dz^2 <= 9 in cells, the cells ON the sphere included ((+-3, 0, 0),
    (2, 2, 1) and their kin); radius 0 keeps the centre cell alone; radius 2e19 (r2 infinite) removes nothing."""
    m, cc, _, _ = block9(hashed)
    info = PR.prune(m, CENTRE9, 0.75)
    want = {tuple(int(v) for v in c) for c in cc if ((c - 4) ** 2).sum() <= 9}
    got = {tuple(int(v) for v in c) for c in PR.entries(m)[0]}
    assert got == want and len(want) == 123 and {(7, 4, 4), (1, 4, 4), (4, 4, 7), (6, 6, 5), (2, 2, 3), (5, 6, 6)} <= got and (7, 5, 4) not in got
    assert info["n_removed"] == 729 - 123 == info["n_points_removed"] and info["n_occupied"] == 123
    assert info["n_vacated"] == (606 if hashed else 0) and info["capacity"] == (2048 if hashed else 729) and info["n_compacted"] == 0
    again = PR.prune(m, CENTRE9, 0.75)
    assert again["n_removed"] == 0 and again["n_points_removed"] == 0 and again["n_occupied"] == 123 and again["n_vacated"] == info["n_vacated"]
    m0 = block9(hashed)[0]
    zero = PR.prune(m0, CENTRE9, 0.0)
    assert zero["n_occupied"] == 1 and [tuple(c) for c in PR.entries(m0)[0]] == [(4, 4, 4)]
    m1 = block9(hashed)[0]
    before = PR.entries(m1)
    huge = PR.prune(m1, CENTRE9, 2e19)
    assert huge["n_removed"] == 0 and huge["n_occupied"] == 729 and all(np.array_equal(a, b) for a, b in zip(before, PR.entries(m1)))
    with np.errstate(over="ignore"):
        assert PR.kept([[4, 4, 4]], 0.25, CENTRE9, 3e38).all() and not np.isfinite(f32(2e19) * f32(2e19))


def identity_clouds():
    from test_gpu_hmap import crafted
    sc = MF.scans(6, (43, 135))
    return [("crafted", crafted()), ("scan 1", sc[1]), ("scan 4", sc[4])]


def surviving(pts, nrm, pose, vs, centre, radius):
    """The points that enter and whose cell the prune keeps."""
    pt = VR.transform_points(pose, pts); nt = VR.transform_normals(pose, nrm)
    ok = np.isfinite(np.asarray(pts, f32)).all(1) & np.isfinite(pt).all(1) & np.isfinite(nt).all(1)
    idx = np.nonzero(ok)[0]
    keep = PR.kept(VR.cell_coords(pt[idx], vs), vs, centre, radius)
    return idx[keep]


def same_entries(a, b, what=""):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), what
    assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)), what


def fresh_map(hashed, vs, lo=(-64, -64, -64), dims=(128, 128, 128)):
    return HR.create(vs, 256) if hashed else MR.create(vs, lo, dims)


@pytest.mark.parametrize("vs", [0.25, 0.3])
def test_prune_equals_never_inserted(vs):
    """The identity that carries the feature: for the crafted cloud and two of the small scans, at the identity and two poses, dense and
    hashed, "insert everything, then prune" equals, bit for bit (counts, sums, records), "insert only the points whose cell survives"
    into a fresh map; and the hashed map equals the dense one."""
    for name, (pts, nrm) in identity_clouds():
        for pose in (EYE, pose_of(*POSE_A), pose_of(*POSE_B)):
            world = VR.transform_points(pose, pts)
            centre = np.nanmedian(np.where(np.isfinite(world), world, np.nan), axis=0).astype(f32)
            radius = 0.9
            idx = surviving(pts, nrm, pose, vs, centre, radius)
            both = []
            for hashed in (False, True):
                full = fresh_map(hashed, vs); PR.insert(full, pts, nrm, pose)
                n_before = len(PR.entries(full)[0]); pts_before = int(PR.entries(full)[1].sum())
                info = PR.prune(full, centre, radius)
                part = fresh_map(hashed, vs); PR.insert(part, pts[idx], nrm[idx], pose)
                same_entries(PR.entries(full), PR.entries(part), (name, vs, hashed))
                assert 0 < info["n_occupied"] == len(PR.entries(part)[0]) < n_before and info["n_removed"] == n_before - info["n_occupied"], (name, info)
                assert info["n_points_removed"] == pts_before - int(PR.entries(part)[1].sum()) > 0 and pts_before - info["n_points_removed"] == len(idx), (name, info)
                both.append(PR.entries(full))
            same_entries(*both, (name, vs, "hashed against dense"))


def line_cells(first, n):
    """n single-point cells (first .. first + n - 1, 0, 0) at 0.25 m: points at the cells' centres."""
    cc = np.stack([np.arange(first, first + n), np.zeros(n, np.int64), np.zeros(n, np.int64)], 1)
    return ((cc + 0.5) * 0.25).astype(f32), np.tile(np.array([[0.0, 0.6, 0.8]], f32), (n, 1))


SCRIPT = [("insert", (0, 100)), ("prune", ((500.0, 0.0, 0.0), 0.0)), ("insert", (1000, 20)), ("insert", (1020, 10)), ("prune", ((256.375, 0.125, 0.125), 1.3)),
          ("insert", (2000, 90)), ("insert", (2090, 30)), ("insert", (3000, 150))]
# after each step: (capacity, n_occupied, n_vacated, n_compacted, n_grown), worked out from the rule by hand:
#   insert 100: 2 (0 + 0 + 100) = 200 <= 256.  prune all: 100 vacated.  insert 20: 2 (0 + 100 + 20) = 240 <= 256.
#   insert 10: 2 (20 + 100 + 10) = 260 > 256, vacated > 0: compaction; 2 (20 + 10) = 60 <= 0.75 x 256: the capacity stays.
#   prune about cell 1025 with 1.3 m (cells 1020 .. 1029 + 0.5 within 5.2 cells of 1025.5: all ten kept), cells 1000 .. 1019 leave: 20 vacated.
#   insert 90: 2 (10 + 20 + 90) = 240 <= 256.  insert 30: 2 (100 + 20 + 30) = 300 > 256: compaction; 2 x 130 = 260 > 192: 512 slots (<= 384).
#   insert 150: 2 (130 + 0 + 150) = 560 > 512, nothing vacated: growth to 1024.
SCRIPT_STATE = [(256, 100, 0, 0, 0), (256, 0, 100, 0, 0), (256, 20, 100, 0, 0), (256, 30, 0, 1, 0), (256, 10, 20, 1, 0), (256, 100, 20, 1, 0), (512, 130, 0, 2, 1),
                (1024, 280, 0, 2, 2)]


def run_script(step, m):
    kind, arg = step
    if kind == "insert":
        PR.insert(m, *line_cells(*arg), EYE)
    else:
        PR.prune(m, *arg)
    return (m["capacity"], len(m["cells"]), m.get("n_vacated", 0), m.get("n_compacted", 0), m["n_grown"])


def test_compaction_rule_on_a_scripted_sequence():
    m = HR.create(0.25, 256)
    for k, (step, want) in enumerate(zip(SCRIPT, SCRIPT_STATE)):
        assert run_script(step, m) == want, (k, step)
    # the hysteresis: 2 (occupied + n) = 200 would fit 256 slots, but not 0.75 of them
    h = HR.create(0.25, 256)
    PR.insert(h, *line_cells(0, 60), EYE); PR.prune(h, (500.0, 0.0, 0.0), 0.0); PR.insert(h, *line_cells(100, 50), EYE)
    assert (h["capacity"], h["n_vacated"], h.get("n_compacted", 0)) == (256, 60, 0)
    PR.insert(h, *line_cells(200, 50), EYE)
    assert (h["capacity"], h["n_vacated"], h["n_compacted"], h["n_grown"], len(h["cells"])) == (512, 0, 1, 1, 100)
    # reserve and compact
    r = HR.create(0.25, 256)
    PR.insert(r, *line_cells(0, 60), EYE); PR.reserve(r, 512)
    assert (r["capacity"], r["n_grown"], r.get("n_compacted", 0)) == (512, 1, 0)
    PR.prune(r, (0.125, 0.125, 0.125), 1.0)
    kept = len(r["cells"])
    assert kept == 5 and r["n_vacated"] == 55
    PR.reserve(r, 300); PR.compact(HR.create(0.25, 256))
    assert (r["capacity"], r["n_vacated"], r.get("n_compacted", 0)) == (512, 55, 0)
    PR.reserve(r, 1024)
    assert (r["capacity"], r["n_vacated"], r["n_compacted"], r["n_grown"], len(r["cells"])) == (1024, 0, 1, 2, 5)
    PR.prune(r, (0.125, 0.125, 0.125), 0.0); PR.compact(r)
    assert (r["capacity"], r["n_vacated"], r["n_compacted"], r["n_grown"], len(r["cells"])) == (1024, 0, 2, 2, 1)
    PR.compact(r)
    assert r["n_compacted"] == 2
    big = HR.create(0.25, 1 << 26); big["n_vacated"] = 1
    with pytest.raises(PR.BadOptions):
        PR.room(big, 1 << 25)


def test_kernel_resource_record():
    """The three new kernels from the compiled code object: no scratch, no AGPRs, no static LDS, VGPRs within the budget of eight waves per
    SIMD (64), as the kernels they stand beside.  Recorded: DESIGN.md section 6v."""
    text = device_asm()
    seen = kernel_resources(text)
    for prefix in ("_ZN6icpdev12k_vmap_prune", "_ZN6icpdev12k_hmap_prune", "_ZN6icpdev14k_hmap_compact"):
        ks = {n: f for n, f in seen.items() if n.startswith(prefix)}
        assert len(ks) == 1, (prefix, list(ks))
        (name, f), = ks.items()
        desc = text[text.index(".amdhsa_kernel " + name):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", desc).group(1))
        print("%s: %d VGPRs, %d AGPRs, scratch %d B, static LDS %d B" % (prefix, f["num_vgpr"], f.get("num_agpr", 0), f["private_seg_size"], lds))
        assert f["private_seg_size"] == 0 and f.get("num_agpr", 0) == 0 and lds == 0, f
        assert f["num_vgpr"] <= 64, f
    for prefix in ("_ZN6icpdev13k_hmap_rehash", "_ZN6icpdev13k_hmap_insert", "_ZN6icpdev13k_vmap_insert"):
        assert len([n for n in seen if n.startswith(prefix)]) == 1, prefix
