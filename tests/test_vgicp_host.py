"""Voxelized GICP on the host side: option validation through the library without a device, the new structs, symbols and Python surface,
the numpy restatement of the contract (tests/vgicp_restatement.py) against plain loops, the positive definiteness the contract promises,
the resource record of the new kernels (compile only), and the recorded outcome of the CPU loop."""
import ctypes
import inspect
import json
import os
import re
import numpy as np
import pytest

import vgicp_restatement as VR
import vgicp_outcome_fixture as VF
from device_asm import device_asm, kernel_resources
from support import pose_of

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32, f64 = np.float32, np.float64


def small_clouds(n=200, seed=5):
    r = np.random.default_rng(seed)
    pts = r.uniform(-0.5, 0.7, (n, 3)).astype(f32)
    pts[:20] = (pts[:20] * 8).round() / 8                       # dyadic, several exactly on cell faces
    nrm = r.normal(size=(n, 3)); nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    pts[3] = (np.nan, 0, 0); nrm[7] = (0, np.inf, 0); pts[9] = (0, -np.inf, 1)
    return pts, nrm


def test_option_validation_without_a_device():
    from icp_amd import binding
    lib = binding.load_library()
    chk = lambda o: lib.icp_vgicp_options_check(ctypes.byref(o))
    o = binding.vgicp_options()
    assert chk(o) == 0 and lib.icp_vgicp_options_check(None) == 1 and lib.icp_vgicp_options_default(None) == 1
    assert (o.voxel_size, o.min_points, o.n_iterations, o.min_valid, o.stop_rotation, o.stop_translation) == (0.25, 1, 30, 64, f32(1e-5), f32(1e-5))
    assert {k: (f32(v) if isinstance(v, float) else v) for k, v in VR.DEFAULTS.items()} == {k: getattr(o, k) for k, _ in binding.IcpVgicpOptions._fields_}
    inf, nan = float("inf"), float("nan")
    bad = [dict(voxel_size=0.0), dict(voxel_size=-0.25), dict(voxel_size=nan), dict(voxel_size=inf), dict(min_points=0), dict(min_points=-3),
           dict(n_iterations=0), dict(n_iterations=1001), dict(min_valid=5), dict(stop_rotation=-1e-6), dict(stop_rotation=nan),
           dict(stop_translation=-1.0), dict(stop_translation=inf)]
    for kw in bad:
        assert chk(binding.vgicp_options(**kw)) == 1, kw
    good = [dict(voxel_size=1e-3), dict(voxel_size=100.0), dict(min_points=1000), dict(n_iterations=1), dict(n_iterations=1000), dict(min_valid=6),
            dict(stop_rotation=0.0), dict(stop_translation=0.0)]
    for kw in good:
        assert chk(binding.vgicp_options(**kw)) == 0, kw
    with pytest.raises(TypeError):
        binding.vgicp_options(voxel=0.5)
    # every entry point refuses a null context
    p = binding.pose_to_c(np.eye(4))
    assert lib.icp_voxelize_target(None, ctypes.byref(o), None) == 1
    assert lib.icp_get_voxel_grid(None, None, None, None) == 1
    assert lib.icp_vgicp_system(None, binding._ptr(p), ctypes.byref(o), None, None) == 1
    assert lib.icp_vgicp_align(None, ctypes.byref(o), binding._ptr(p), None, None, 0) == 1


def test_structs_symbols_and_python_surface():
    from icp_amd import binding, eth
    assert ctypes.sizeof(binding.IcpVgicpOptions) == 24 and binding.IcpVgicpOptions.min_points.offset == 4 and binding.IcpVgicpOptions.stop_rotation.offset == 16
    assert ctypes.sizeof(binding.IcpVoxelGridInfo) == 32 and binding.IcpVoxelGridInfo.dims.offset == 12 and binding.IcpVoxelGridInfo.n_occupied.offset == 24
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    sig = {"icp_vgicp_options_default": r"icp_vgicp_options\* opt", "icp_vgicp_options_check": r"const icp_vgicp_options\* opt",
           "icp_voxelize_target": r"icp_ctx\* ctx, const icp_vgicp_options\* opt, icp_voxel_grid_info\* info_out",
           "icp_get_voxel_grid": r"icp_ctx\* ctx, int32_t\* counts_out, int64_t\* sums_out, float\* cells_out",
           "icp_vgicp_system": r"icp_ctx\* ctx, const float pose\[16\], const icp_vgicp_options\* opt, double\* sums_out, int32_t\* counts_out",
           "icp_vgicp_align": r"icp_ctx\* ctx, const icp_vgicp_options\* opt, float pose_inout\[16\], icp_vgicp_record\* rec_out, icp_vgicp_iter\* trace_out,\s+int32_t max_trace"}
    for name, args in sig.items():
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(%s\);" % (name, args), hdr, flags=re.M), name
    for struct in ("icp_vgicp_options", "icp_voxel_grid_info"):
        assert re.search(r"^\} %s;" % struct, hdr, flags=re.M), struct
    assert "typedef icp_sdf_iter icp_vgicp_iter;" in hdr and "typedef icp_sdf_frame icp_vgicp_record;" in hdr
    for m in ("voxelize_target", "voxel_grid", "vgicp_system", "vgicp_align"):
        assert hasattr(binding.Context, m), m
    assert inspect.signature(eth.align).parameters["vgicp"].default is None


def test_restatement_grid_against_a_plain_loop():
    """200 points (dyadic ones, points on cell faces, negative coordinates, three that must stay out): the restatement's vectorised integer
    sums, counts and extent against one Python loop per point with Python integers, at both voxel sizes of the device test."""
    pts, nrm = small_clouds()
    for vs in (0.25, 0.3):
        g = VR.grid(pts, nrm, vs)
        v = f32(vs)
        cells = {}
        for p, n in zip(pts, nrm):
            if not (np.isfinite(p).all() and np.isfinite(n).all()):
                continue
            c = tuple(int(np.floor(f32(p[a] / v))) for a in range(3))
            q = [int(np.rint(min(max(f32(f32(f32(p[a] - f32(f32(f32(c[a]) + f32(0.5)) * v)) / v) * f32(65536.0)), f32(-32768)), f32(32768)))) for a in range(3)]
            m = [int(np.rint(f32(n[a] * f32(16384.0)))) for a in range(3)]
            acc = cells.setdefault(c, [0] * 10)
            acc[0] += 1
            for a in range(3):
                acc[1 + a] += q[a]
            for k, (a, b) in enumerate(VR.PAIRS):
                acc[4 + k] += m[a] * m[b]
        keys = np.array(list(cells))
        lo = keys.min(0); dims = keys.max(0) - lo + 1
        assert np.array_equal(lo, g["lo"]) and np.array_equal(dims, g["dims"])
        assert g["n_points"] == 197 and g["n_occupied"] == len(cells) and int(g["counts"].sum()) == 197
        for c, acc in cells.items():
            i = ((c[2] - lo[2]) * dims[1] + (c[1] - lo[1])) * dims[0] + (c[0] - lo[0])
            assert g["counts"][i] == acc[0] and list(g["sums"][i]) == acc[1:], (vs, c)
            mu = [(c[a] + 0.5) * f64(v) + (acc[1 + a] / acc[0]) * (f64(v) / 65536.0) for a in range(3)]
            assert np.array_equal(g["cells"][i, :3], np.array(mu, f64).astype(f32))
            tr = acc[4] + acc[7] + acc[9]
            assert np.array_equal(g["cells"][i, 3:], (np.array(acc[4:], f64) / f64(tr)).astype(f32))
            assert abs(f64(g["cells"][i, 3]) + f64(g["cells"][i, 6]) + f64(g["cells"][i, 8]) - 1) < 1e-6
        empty = g["counts"] == 0
        assert not g["cells"][empty].any() and not g["sums"][empty].any()
        # the mean of a cell is the mean of its points to the quantisation: half a step of voxel / 65536, and the fp32 rounding of mu
        ok = VR.entering(pts, nrm)
        cc, _, _ = VR.quantise(pts[ok], nrm[ok], vs)
        idx = ((cc[:, 2] - lo[2]) * dims[1] + (cc[:, 1] - lo[1])) * dims[0] + (cc[:, 0] - lo[0])
        for i in np.unique(idx):
            mean = pts[ok][idx == i].astype(f64).mean(0)
            assert np.abs(g["cells"][i, :3] - mean).max() < 0.5 * vs / 65536 + 4 * 2.0 ** -24 * 2.0
    with pytest.raises(VR.GridTooLarge):
        VR.grid(np.array([[0, 0, 0], [1e6, 0, 0]], f32), np.array([[0, 0, 1], [0, 0, 1]], f32), 0.01)
    with pytest.raises(VR.NoTarget):
        VR.grid(np.array([[np.nan, 0, 0]], f32), np.array([[0, 0, 1]], f32), 0.25)


def test_sigma_is_positive_definite_at_the_smallest_epsilon():
    """S = sum m m^T / trace over 1 .. 40 quantised unit normals (aligned ones too: the worst case is S = b b^T), rounded to fp32 as the record
    is; Sigma = 2I - (1 - eps)(S + b b^T) at eps = 1e-6.  lambda_max(S) <= 1 up to the fp32 rounding of its six entries (3 x 2^-24), so
    lambda_min(Sigma) >= 2 eps - (1 - eps) 3 x 2^-24 - rounding: positive, and at least 1e-6 here."""
    r = np.random.default_rng(11)
    eps = f64(f32(1e-6))
    worst = np.inf
    for trial in range(400):
        k = int(r.integers(1, 41))
        if trial % 4 == 0:
            base = r.normal(size=3); n = np.tile(base / np.linalg.norm(base), (k, 1)) + r.normal(size=(k, 3)) * 1e-4
        else:
            n = r.normal(size=(k, 3))
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
        m = np.rint(n * f32(16384.0)).astype(np.int64)
        mm = np.einsum("ka,kb->ab", m, m)
        S = (mm.astype(f64) / f64(np.trace(mm))).astype(f32).astype(f64)
        b = n[0].astype(f64) if trial % 2 == 0 else r.normal(size=3)
        b = b / np.linalg.norm(b)
        Sigma = 2.0 * np.eye(3) - (1.0 - eps) * (S + np.outer(b, b))
        lam = np.linalg.eigvalsh(Sigma)
        worst = min(worst, lam[0])
        assert lam[0] > 0 and np.linalg.det(Sigma) > 0
    print("smallest eigenvalue of Sigma over 400 trials at eps = 1e-6: %.3g" % worst)
    assert worst >= 1e-6


def test_restatement_system_against_rows():
    """The restatement's 28 sums on the 200-point clouds against N J^T M J, N J^T M r and N r^T M r assembled point by point, row by row,
    with numpy's own inverse of Sigma; the counts against the classes the pose produces (outside, empty cell, below min_points)."""
    pts, nrm = small_clouds()
    g = VR.grid(pts, nrm, 0.3)
    src, sn = small_clouds(260, seed=9)
    src = (src * f32(1.3)).astype(f32)                           # some points leave the grid
    sn[11] = (0, 0, 0); sn[12] = (np.nan, 0, 0)
    pose = pose_of((0.03, -0.02, 0.05), (0.05, 0.02, -0.04))
    for min_points in (1, 3):
        (nc, nv), s, a = VR.system(g, src, sn, pose, 1e-3, min_points)
        t = VR.point_terms(g, src, sn, pose, 1e-3, min_points)
        assert nc == int(np.isfinite(src).all(1).sum()) == 258 and nv == len(t["index"]) and 20 < nv < nc
        H = np.zeros((6, 6)); b = np.zeros(6); cost = 0.0
        for k in range(nv):
            p = t["p"][k].astype(f64); r = t["r"][k]; N = t["N"][k]
            assert N >= min_points and N == g["counts"][t["cell"][k]]
            M = np.linalg.inv(t["Sigma"][k])
            assert np.abs(M - t["M"][k]).max() < 1e-12 * np.abs(M).max()
            A = np.array([[0.0, p[2], -p[1]], [-p[2], 0.0, p[0]], [p[1], -p[0], 0.0]])      # -[p]x
            J = np.hstack([A, np.eye(3)])
            for row in range(3):
                for col in range(3):
                    H += N * M[row, col] * np.outer(J[row], J[col])
                    b += N * M[row, col] * J[row] * r[col]
                    cost += N * M[row, col] * r[row] * r[col]
        k = 0
        for i in range(6):
            for j in range(i, 6):
                assert abs(s[k] - H[i, j]) <= 1e-9 * a[k] + 1e-12, (i, j); k += 1
        assert np.abs(s[21:27] - b).max() <= 1e-9 * a[21:27].max() and abs(s[27] - cost) <= 1e-9 * a[27]
        # the step reduces the cost: the sums describe a descent direction of the objective they sum
        new, x = VR.step(s, (nc, nv), pose, min_valid=6)
        assert new is not None and np.isfinite(x).all()
    n1 = VR.system(g, src, sn, pose, 1e-3, 1)[0][1]; n3 = VR.system(g, src, sn, pose, 1e-3, 3)[0][1]
    assert n3 < n1
    # the Jacobian's sign and scale: sums[21..26] = -1/2 d/dx of sum N r(x)^T M r(x), r(x) = mu - dT(x) p with cells and M held fixed, against
    # central differences (h = 1e-6; the objective is quadratic in t and smooth in the angles, so what is left is O(h^2) and fp64 rounding of
    # a difference of sums of size sum |term| / h: bound 1e-6 sum |term| of the cost)
    (nc, nv), s, a = VR.system(g, src, sn, pose, 1e-3, 1)
    t = VR.point_terms(g, src, sn, pose, 1e-3, 1)
    P = t["p"].astype(f64); mu = t["r"] + P

    def cost(x):
        ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
        Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]); Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
        r = mu - (P @ (Rx @ Ry @ Rz).T + x[3:])
        return float((t["N"] * np.einsum("na,nab,nb->n", r, t["M"], r)).sum())
    assert abs(cost(np.zeros(6)) - s[27]) <= 1e-12 * a[27]
    h = 1e-6
    for i in range(6):
        e = np.zeros(6); e[i] = h
        fd = (cost(e) - cost(-e)) / (2 * h)
        assert abs(-0.5 * fd - s[21 + i]) <= 1e-6 * a[27] and abs(s[21 + i]) > 1e-3 * a[21 + i], (i, fd, s[21 + i])


def test_kernel_resource_record():
    """The new kernels from the compiled code object: no scratch, no AGPRs.  k_vgicp_accumulate keeps a lane's 28 fp64 sums (56 registers)
    live across the second point's 3 x 3 inverse and products: 126 VGPRs recorded, budget 128 (four waves per SIMD; its grid is one block
    per 512 points, 724 blocks = 2.8 waves per SIMD at 370 488 points, so registers do not limit what is resident).  k_vg_cells_add, the
    segmented shuffle sum over ten values of which six are 64-bit: 55 recorded, budget 64.  k_vg_finalise, nine fp64 divisions per cell: 58
    recorded, budget 64.  k_vg_bounds: 17 recorded, budget 24.  k_vg_box_init: 3 recorded, budget 8.  Static LDS: the block fold's
    4 x 28 x 17 doubles, 8 ints and the nine floats of the normal matrix (padded to 16) for k_vgicp_accumulate; 4 x 6 ints for k_vg_bounds.
    Recorded: see DESIGN.md section 6s."""
    text = device_asm()
    seen = kernel_resources(text)
    budget = {"_ZN6icpdev18k_vgicp_accumulate": (128, 4 * 28 * 17 * 8 + 32 + 64), "_ZN6icpdev14k_vg_cells_add": (64, 0), "_ZN6icpdev13k_vg_finalise": (64, 0),
              "_ZN6icpdev11k_vg_bounds": (24, 4 * 6 * 4), "_ZN6icpdev13k_vg_box_init": (8, 0)}
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


def test_recorded_outcome_is_present_and_consistent():
    """tests/golden/vgicp_outcome.json (written by tests/vgicp_outcome_fixture.py): the fixture's own parameters, a run that used all its
    iterations and succeeded, an end below a tenth of the identity's error, and close to the fp64 prototype's 2.8e-4 rad / 1.9 mm (within a
    factor of two either way: the prototype shares the method, not the quantised grid)."""
    with open(VF.GOLDEN) as f:
        o = json.load(f)
    print("restatement: %.3g rad / %.3g m from %.3g rad / %.3g m" % (o["rotation_rad"], o["translation_m"], o["identity_rotation_rad"], o["identity_translation_m"]))
    assert (o["points"], o["voxel_size"], o["epsilon"], o["n_iterations"]) == (86 * 270, VF.OPTIONS["voxel_size"], VF.EPSILON, VF.OPTIONS["n_iterations"])
    assert o["status"] == 0 and o["iterations"] == 30 and o["cost_last"] < o["cost_first"] and o["n_valid_last"] >= o["n_valid_first"] > 64
    assert abs(o["identity_rotation_rad"] - 0.056) < 1e-3 and abs(o["identity_translation_m"] - 0.042) < 1e-3
    assert o["rotation_rad"] < 0.1 * o["identity_rotation_rad"] and o["translation_m"] < 0.1 * o["identity_translation_m"]
    assert 1.4e-4 < o["rotation_rad"] < 5.6e-4 and 0.95e-3 < o["translation_m"] < 3.8e-3
    assert int(np.prod(o["dims"])) >= o["n_occupied"] > 0
