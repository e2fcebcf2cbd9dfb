"""Scan-to-map laser tracking on the host side: option validation through the library without a device, the new structs, symbols and Python
surface, the numpy restatement of the contract (tests/vmap_restatement.py) against plain loops and against voxelized GICP's grid, the
resource record of the new kernels (compile only), and the recorded outcome of the CPU loops."""
import ctypes
import inspect
import json
import os
import re
import numpy as np
import pytest

import vgicp_restatement as VR
import vmap_restatement as MR
import vmap_outcome_fixture as MF
from device_asm import device_asm, kernel_resources
from support import pose_of

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32, f64 = np.float32, np.float64
POSE_A = ((0.3, -0.2, 0.5), (0.4, -0.3, 0.2))
POSE_B = ((-0.1, 0.25, -0.4), (-0.2, 0.1, 0.3))


def small_cloud(n=200, seed=5):
    r = np.random.default_rng(seed)
    pts = r.uniform(-0.5, 0.7, (n, 3)).astype(f32)
    pts[:20] = (pts[:20] * 8).round() / 8                       # dyadic, several exactly on cell faces
    nrm = r.normal(size=(n, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    pts[3] = (np.nan, 0, 0); nrm[7] = (0, np.inf, 0); pts[9] = (0, -np.inf, 1); nrm[11] = (np.nan, 0, 0)
    return pts, nrm


def test_option_validation_without_a_device():
    from icp_amd import binding
    lib = binding.load_library()
    chk = lambda o: lib.icp_voxel_map_options_check(ctypes.byref(o))
    mk = binding.voxel_map_options
    assert chk(mk(0.25, (-14, -18, -2), (29, 37, 15))) == 0 and lib.icp_voxel_map_options_check(None) == 1
    inf, nan = float("inf"), float("nan")
    bad = [mk(0.0, (0, 0, 0), (1, 1, 1)), mk(-0.25, (0, 0, 0), (1, 1, 1)), mk(nan, (0, 0, 0), (1, 1, 1)), mk(inf, (0, 0, 0), (1, 1, 1)),
           mk(0.25, (0, 0, 0), (0, 1, 1)), mk(0.25, (0, 0, 0), (4, -1, 4)), mk(0.25, (0, 0, 0), (256, 256, 257)), mk(0.25, (0, 0, 0), (1 << 24, 2, 1)),
           mk(0.25, (0, 0, 0), (1 << 30, 1 << 30, 4)), mk(0.25, (-(1 << 30) - 1, 0, 0), (1, 1, 1)), mk(0.25, (0, (1 << 30) + 1, 0), (1, 1, 1))]
    for o in bad:
        assert chk(o) == 1, (o.voxel_size, tuple(o.lo), tuple(o.dims))
    good = [mk(1e-3, (0, 0, 0), (1, 1, 1)), mk(100.0, (-5, 7, 0), (256, 256, 256)), mk(0.25, (0, 0, 0), (1 << 24, 1, 1)), mk(0.25, (-(1 << 30), 1 << 30, 0), (2, 2, 2))]
    for o in good:
        assert chk(o) == 0, (o.voxel_size, tuple(o.lo), tuple(o.dims))
    for kw in (dict(voxel_size=0.0, lo=(0, 0, 0), dims=(1, 1, 1)), dict(voxel_size=0.25, lo=(0, 0, 0), dims=(0, 1, 1)), dict(voxel_size=0.25, lo=(0, 0, 0), dims=(256, 256, 257))):
        with pytest.raises(MR.BadOptions):
            MR.create(**kw)
    # every entry point refuses a null context
    p = binding.pose_to_c(np.eye(4)); o = binding.vgicp_options(); m = mk(0.25, (0, 0, 0), (1, 1, 1))
    assert lib.icp_voxel_map_create(None, ctypes.byref(m)) == 1 and lib.icp_voxel_map_destroy(None) == 1
    assert lib.icp_voxel_map_insert(None, 0, binding._ptr(p), None) == 1
    assert lib.icp_get_voxel_map(None, None, None, None, None) == 1 and lib.icp_voxel_map_upload(None, None, None) == 1
    assert lib.icp_voxel_map_system(None, binding._ptr(p), ctypes.byref(o), None, None) == 1
    assert lib.icp_voxel_map_align(None, ctypes.byref(o), binding._ptr(p), None, None, 0) == 1
    assert lib.icp_track_scans_vmap(None, None, None, None, 1, ctypes.byref(o), binding._ptr(p), None) == 1
    # the extent by the cell rule: the library's rule in fp32, both ends inclusive
    assert binding.voxel_map_extent((-3.5, -4.5, -0.5), (3.5, 4.5, 3.1), 0.25) == ((-14, -18, -2), (29, 37, 15))
    assert binding.voxel_map_extent((0, 0, 0), (0.3, 0.299, 1e12), 0.3) == ((0, 0, 0), (2, 1, (1 << 30) + 1))
    lo, dims = MR.extent((-3.5, -4.5, -0.5), (3.5, 4.5, 3.1), 0.25)
    assert tuple(lo) == (-14, -18, -2) and tuple(dims) == (29, 37, 15)


def test_structs_symbols_and_python_surface():
    from icp_amd import binding, eth
    assert ctypes.sizeof(binding.IcpVoxelMapOptions) == 28 and binding.IcpVoxelMapOptions.lo.offset == 4 and binding.IcpVoxelMapOptions.dims.offset == 16
    assert ctypes.sizeof(binding.IcpVoxelMapInsertInfo) == 24 and [f[0] for f in binding.IcpVoxelMapInsertInfo._fields_] == list(MR.INFO)
    assert ctypes.sizeof(binding.IcpVoxelMapInfo) == 32 and binding.IcpVoxelMapInfo.n_occupied.offset == 28
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    sig = {"icp_voxel_map_options_check": r"const icp_voxel_map_options\* opt",
           "icp_voxel_map_create": r"icp_ctx\* ctx, const icp_voxel_map_options\* opt",
           "icp_voxel_map_destroy": r"icp_ctx\* ctx",
           "icp_voxel_map_insert": r"icp_ctx\* ctx, int32_t which, const float pose\[16\], icp_voxel_map_insert_info\* info_out",
           "icp_get_voxel_map": r"icp_ctx\* ctx, icp_voxel_map_info\* info_out, int32_t\* counts_out, int64_t\* sums_out, float\* cells_out",
           "icp_voxel_map_upload": r"icp_ctx\* ctx, const int32_t\* counts, const int64_t\* sums",
           "icp_voxel_map_system": r"icp_ctx\* ctx, const float pose\[16\], const icp_vgicp_options\* opt, double\* sums_out, int32_t\* counts_out",
           "icp_voxel_map_align": r"icp_ctx\* ctx, const icp_vgicp_options\* opt, float pose_inout\[16\], icp_vgicp_record\* rec_out, icp_vgicp_iter\* trace_out,\s+int32_t max_trace",
           "icp_track_scans_vmap": r"icp_ctx\* ctx, const float\* const\* xyz, const float\* const\* normals, const int32_t\* n, int32_t n_scans,\s+const icp_vgicp_options\* opt, float pose_inout\[16\], icp_vgicp_record\* out"}
    for name, args in sig.items():
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(%s\);" % (name, args), hdr, flags=re.M), name
    for struct in ("icp_voxel_map_options", "icp_voxel_map_insert_info", "icp_voxel_map_info"):
        assert re.search(r"^\} %s;" % struct, hdr, flags=re.M), struct
    for m in ("voxel_map_create", "voxel_map_destroy", "voxel_map_insert", "voxel_map", "voxel_map_upload", "voxel_map_system", "voxel_map_align", "track_scans_vmap"):
        assert hasattr(binding.Context, m), m
    par = inspect.signature(eth.track_map).parameters
    assert par["voxel_size"].default == 0.25 and par["extent"].default is None and "margin" in par
    assert list(inspect.signature(binding.voxel_map_extent).parameters) == ["lower", "upper", "voxel_size"]


def loop_insert(cells, pts, nrm, pose, vs, lo, dims):
    """One Python loop per point with Python integers: the contract's insert into the dict `cells` (cell coordinates -> [count, nine sums]).
    Returns (considered, entered, outside)."""
    v = f32(vs); P = np.asarray(pose, f32); N = VR.normal_matrix(pose)
    considered = entered = outside = 0
    for p, n in zip(pts, nrm):
        if not np.isfinite(p).all():
            continue
        considered += 1
        with np.errstate(all="ignore"):
            pt = [f32(f32(f32(f32(P[r, 0] * p[0]) + f32(P[r, 1] * p[1])) + f32(P[r, 2] * p[2])) + P[r, 3]) for r in range(3)]
            nt = [f32(f32(f32(N[r, 0] * n[0]) + f32(N[r, 1] * n[1])) + f32(N[r, 2] * n[2])) for r in range(3)]
        if not (np.isfinite(pt).all() and np.isfinite(nt).all()):
            continue
        entered += 1
        c = tuple(int(np.floor(f32(pt[a] / v))) for a in range(3))
        if not all(lo[a] <= c[a] < lo[a] + dims[a] for a in range(3)):
            outside += 1
            continue
        q = [int(np.rint(min(max(f32(f32(f32(pt[a] - f32(f32(f32(c[a]) + f32(0.5)) * v)) / v) * f32(65536.0)), f32(-32768)), f32(32768)))) for a in range(3)]
        m = [int(np.rint(f32(min(max(nt[a], f32(-2.0)), f32(2.0)) * f32(16384.0)))) for a in range(3)]
        acc = cells.setdefault(c, [0] * 10)
        acc[0] += 1
        for a in range(3):
            acc[1 + a] += q[a]
        for k, (a, b) in enumerate(VR.PAIRS):
            acc[4 + k] += m[a] * m[b]
    return considered, entered, outside


def test_restatement_insert_against_a_plain_loop():
    """200 points (dyadic ones, points on cell faces, negative coordinates, four that must stay out) inserted at two poses into a map smaller
    than the moved clouds: the restatement's counts, sums, records and info against one Python loop per point with Python integers."""
    pts, nrm = small_cloud()
    vs, lo, dims = 0.25, (-2, -1, -1), (4, 3, 4)
    m = MR.create(vs, lo, dims)
    cells = {}
    occupied = 0
    for pose in (pose_of(*POSE_A), pose_of(*POSE_B)):
        N = VR.normal_matrix(pose)
        assert np.abs(N - np.linalg.inv(pose[:3, :3].astype(f64)).T).max() < 1e-6      # the normal matrix is (R^-1)^T
        before = {c: a[0] for c, a in cells.items()}
        considered, entered, outside = loop_insert(cells, pts, nrm, pose, vs, lo, dims)
        info = MR.insert(m, pts, nrm, pose)
        touched = [c for c, a in cells.items() if a[0] != before.get(c, 0)]
        new = [c for c in touched if c not in before]
        occupied += len(new)
        assert info == dict(n_considered=considered, n_entered=entered, n_outside=outside, n_cells_touched=len(touched), n_cells_new=len(new), n_occupied=occupied)
        assert considered == 198 and entered == 196 and 0 < outside < entered and len(new) > 0
        assert int(m["counts"].sum()) == sum(a[0] for a in cells.values()) and m["n_occupied"] == len(cells) == int((m["counts"] > 0).sum())
        for c, acc in cells.items():
            i = ((c[2] - lo[2]) * dims[1] + (c[1] - lo[1])) * dims[0] + (c[0] - lo[0])
            assert m["counts"][i] == acc[0] and list(m["sums"][i]) == acc[1:], c
            mu = [(c[a] + 0.5) * f64(f32(vs)) + (acc[1 + a] / acc[0]) * (f64(f32(vs)) / 65536.0) for a in range(3)]
            assert np.array_equal(m["cells"][i, :3], np.array(mu, f64).astype(f32))
            tr = acc[4] + acc[7] + acc[9]
            assert tr > 0 and np.array_equal(m["cells"][i, 3:], (np.array(acc[4:], f64) / f64(tr)).astype(f32))
        empty = m["counts"] == 0
        assert not m["cells"][empty].any() and not m["sums"][empty].any()
    assert len(touched) < len(cells) or len(new) == len(cells)


def test_order_independence_and_upload():
    """A then B equals B then A, bytes for bytes; a shuffled cloud gives the same map; upload of the integer state reproduces the records."""
    pts, nrm = small_cloud(300, seed=8)
    A, B = pose_of(*POSE_A), pose_of(*POSE_B)
    make = lambda: MR.create(0.3, (-3, -3, -3), (7, 6, 7))
    ab, ba, sh = make(), make(), make()
    MR.insert(ab, pts, nrm, A); iab = MR.insert(ab, pts[:150], nrm[:150], B)
    MR.insert(ba, pts[:150], nrm[:150], B); iba = MR.insert(ba, pts, nrm, A)
    perm = np.random.default_rng(1).permutation(300)
    MR.insert(sh, pts[perm], nrm[perm], A); MR.insert(sh, pts[:150][::-1], nrm[:150][::-1], B)
    for other in (ba, sh):
        assert np.array_equal(ab["counts"], other["counts"]) and np.array_equal(ab["sums"], other["sums"])
        assert np.array_equal(ab["cells"].view(np.uint32), other["cells"].view(np.uint32)) and ab["n_occupied"] == other["n_occupied"]
    assert iab["n_occupied"] == iba["n_occupied"] and (iab["n_cells_touched"], iab["n_cells_new"]) != (iba["n_cells_touched"], iba["n_cells_new"])
    up = make()
    MR.upload(up, ab["counts"], ab["sums"])
    assert np.array_equal(up["cells"].view(np.uint32), ab["cells"].view(np.uint32)) and up["n_occupied"] == ab["n_occupied"]


def test_identity_insert_equals_the_grid():
    """At the identity pose, with lo and dims taken from vgicp_restatement.grid, the map is that grid: counts, sums and records bit for bit."""
    pts, nrm = small_cloud()
    for vs in (0.25, 0.3):
        g = VR.grid(pts, nrm, vs)
        m = MR.create(vs, g["lo"], g["dims"])
        info = MR.insert(m, pts, nrm, np.eye(4, dtype=f32))
        assert np.array_equal(m["counts"], g["counts"]) and m["counts"].dtype == g["counts"].dtype and np.array_equal(m["sums"], g["sums"])
        assert np.array_equal(m["cells"].view(np.uint32), g["cells"].view(np.uint32))
        assert info == dict(n_considered=198, n_entered=g["n_points"], n_outside=0, n_cells_touched=g["n_occupied"], n_cells_new=g["n_occupied"], n_occupied=g["n_occupied"])
        # and a step against the map is a step against the grid
        src = (pts * f32(1.1)).astype(f32)
        a = MR.system(m, src, nrm, pose_of(*POSE_B), 1e-3); b = VR.system(g, src, nrm, pose_of(*POSE_B), 1e-3)
        assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_kernel_resource_record():
    """The new kernels from the compiled code object: no scratch, no AGPRs.  k_vmap_insert is k_vg_cells_add's segmented shuffle sum over
    ten values of which six are 64-bit (55 VGPRs there) with the moved point, two more atomics' results and four ballots in front and
    behind, none of them live across the sum: 50 recorded, budget 64 (eight waves per SIMD; the kernel is bound by its atomics, not by
    occupancy).  k_vmap_records is k_vg_finalise's nine fp64 divisions behind one indirection: 56 recorded, budget 64.  Static LDS: the 16
    floats of the pose and the nine of the normal matrix for k_vmap_insert (100 bytes), none for k_vmap_records.  Recorded: DESIGN.md
    section 6t."""
    text = device_asm()
    seen = kernel_resources(text)
    budget = {"_ZN6icpdev13k_vmap_insert": (64, 25 * 4), "_ZN6icpdev14k_vmap_records": (64, 0)}
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
    # the alignment against the map adds no kernel: one k_vgicp_accumulate, one k_sdf_solve, as before
    assert len([n for n in seen if n.startswith("_ZN6icpdev18k_vgicp_accumulate")]) == 1 and len([n for n in seen if n.startswith("_ZN6icpdev11k_sdf_solve")]) == 1


def test_recorded_outcome_is_present_and_consistent():
    """tests/golden/vmap_outcome.json (written by tests/vmap_outcome_fixture.py): the fixture's own parameters, every scan aligned, and the
    map loop's final and worst errors at most half the pair chain's -- what the map is for.  Close to the fp64 prototype's figures (map
    final 1.0e-3 rad / 3.2e-3 m, chain final 3.6e-3 rad / 8.9e-3 m: within a factor of two either way)."""
    with open(MF.GOLDEN) as f:
        o = json.load(f)
    mp, ch = o["map"], o["chain"]
    print("map: final %.3g rad / %.3g m, worst %.3g rad / %.3g m; chain: final %.3g rad / %.3g m, worst %.3g rad / %.3g m" % (
        mp["final_rotation_rad"], mp["final_translation_m"], mp["worst_rotation_rad"], mp["worst_translation_m"],
        ch["final_rotation_rad"], ch["final_translation_m"], ch["worst_rotation_rad"], ch["worst_translation_m"]))
    lo, dims = MF.extent()
    assert (o["n_scans"], o["points"], o["voxel_size"], o["epsilon"], o["n_iterations"]) == (MF.N_SCANS, 86 * 270, MF.VOXEL, MF.EPSILON, MF.OPTIONS["n_iterations"])
    assert o["lo"] == [int(x) for x in lo] and o["dims"] == [29, 37, 15] == [int(x) for x in dims]
    assert o["status"] == 0 and o["chain_status"] == 0 and len(o["iterations"]) == MF.N_SCANS - 1 and all(1 <= i <= 30 for i in o["iterations"])
    assert 0 < o["n_occupied"] <= 29 * 37 * 15
    for k in ("final_rotation_rad", "final_translation_m", "worst_rotation_rad", "worst_translation_m"):
        assert 0 < mp[k] <= 0.5 * ch[k], k
        assert mp["worst" + k[5:]] >= mp["final" + k[5:]] and ch["worst" + k[5:]] >= ch["final" + k[5:]]
    assert 0.5e-3 < mp["final_rotation_rad"] < 2.0e-3 and 1.6e-3 < mp["final_translation_m"] < 6.4e-3
    assert 1.8e-3 < ch["final_rotation_rad"] < 7.2e-3 and 4.45e-3 < ch["final_translation_m"] < 17.8e-3
