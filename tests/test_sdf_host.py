"""Direct SDF tracking on the host side: the numpy restatement of the contract (tests/sdf_restatement.py) against finite differences,
option validation through the library without a device, the new structs, symbols and Python surface, the resource record of the new
kernels (compile only), and the recorded outcome of the CPU loop against the ray-cast model loop's."""
import ctypes
import inspect
import json
import os
import re
import numpy as np
import pytest

import sdf_restatement as SR
import tsdf_restatement as TS
import tsdf_outcome_fixture as OF
import sdf_outcome_fixture as SF
from device_asm import device_asm, kernel_resources
from icp_amd.synth import tum_K, wavy_depth
from support import pose_of

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32, f64 = np.float32, np.float64
SMALL = dict(dims=(37, 21, 29), origin=(-1.8, -1.0, -0.5), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=2.4)


def small_model(W=40, H=30):
    cam = TS.Camera(tum_K(W), W, H)
    vol = TS.Volume(**SMALL)
    for _ in range(2):
        TS.integrate(vol, wavy_depth(W, H), cam, np.eye(4, dtype=f32))
    return vol, cam


def field64(vol, q):
    """truncation x the trilinear interpolant of the cell of q, everything in fp64: (r, fractions)."""
    g = (q - vol.o.astype(f64)) / f64(vol.s)
    i = np.floor(g).astype(int); t = g - i
    c = vol.tsdf[i[2]:i[2] + 2, i[1]:i[1] + 2, i[0]:i[0] + 2].astype(f64)      # [dz, dy, dx]
    cz = c[0] * (1 - t[2]) + c[1] * t[2]
    cy = cz[0] * (1 - t[1]) + cz[1] * t[1]
    return f64(vol.trunc) * (cy[0] * (1 - t[0]) + cy[1] * t[0]), t


def increment64(x):
    """dT = [Rx Ry Rz | t] in fp64."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]); Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    D = np.eye(4); D[:3, :3] = Rx @ Ry @ Rz; D[:3, 3] = x[3:]
    return D


def test_jacobian_against_finite_differences():
    """J = (q x g, g) against central differences of r(dT q) in the six components of a left-multiplied increment, h = 1e-6, on pixels whose
    point stays in its cell (fractions in [0.01, 0.99]; the point moves by h (1 + |q|) < 4e-6 m = 4e-5 voxels).  Inside a cell r is a
    polynomial with bounded third derivatives, so the central difference is exact to O(h^2); what is left is the fp32 rounding of the
    restatement's gradient: six operations on corner differences of magnitude <= 2, 6 x 2 x 2^-24 = 7e-7 per voxel, x truncation /
    voxel_size = 3 per metre, x |q| <= 3 m in the rotational columns: bound 1e-5 on every component."""
    vol, cam = small_model()
    pose = pose_of((0.02, -0.015, 0.01), (0.03, -0.02, 0.02))
    t = SR.pixel_terms(vol, wavy_depth(40, 30), cam, pose)
    J = SR.jacobian(t["q"], t["g"])
    h, checked, worst = 1e-6, 0, 0.0
    for k in np.nonzero(t["valid"])[0]:
        q = t["q"][k].astype(f64)
        r0, fr = field64(vol, q)
        if not ((fr > 0.01) & (fr < 0.99)).all():
            continue
        assert abs(r0 - t["r"][k]) < 1e-6                   # the same cell, the same field
        assert np.linalg.norm(q) < 3.0
        fd = np.empty(6)
        for a in range(6):
            x = np.zeros(6); x[a] = h
            qp = increment64(x)[:3, :3] @ q + increment64(x)[:3, 3]; qm = increment64(-x)[:3, :3] @ q + increment64(-x)[:3, 3]
            fd[a] = (field64(vol, qp)[0] - field64(vol, qm)[0]) / (2 * h)
        worst = max(worst, float(np.abs(fd - J[k]).max()))
        checked += 1
    print("Jacobian against finite differences: %d pixels, worst |J - fd| = %.3g" % (checked, worst))
    assert checked > 300 and worst < 1e-5
    assert np.abs(J).max() > 0.5                            # the columns are not all near zero


def test_restatement_system_and_align():
    """The restatement on the small model: the sums are the terms' sums in the contract's layout, the Huber weight only lowers the cost, and
    Gauss-Newton from two starts reaches one minimum (which is not the identity at 10 cm voxels)."""
    vol, cam = small_model()
    d = wavy_depth(40, 30); d[0, :6] = [-np.inf, np.nan, np.inf, 0.0, -1.0, 2.5]
    pose = pose_of((0.02, -0.015, 0.01), (0.03, -0.02, 0.02))
    (nd, nv), s, a = SR.system(vol, d, cam, pose)
    assert nd == 1200 - 6 and 500 < nv < nd
    t = SR.pixel_terms(vol, d, cam, pose)
    J = SR.jacobian(t["q"][t["valid"]], t["g"][t["valid"]]); r = t["r"][t["valid"]]
    H = J.T @ J; b = -(J.T @ r)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            assert abs(s[k] - H[i, j]) <= nv * 2.0 ** -52 * a[k]; k += 1
    assert np.abs(s[21:27] - b).max() <= nv * 2.0 ** -52 * a[21:27].max() and abs(s[27] - r @ r) <= nv * 2.0 ** -52 * a[27]
    _, sh, _ = SR.system(vol, d, cam, pose, huber=0.05)
    assert sh[27] < s[27] and (np.abs(r) > 0.05).any()
    ends = []
    for start in (pose, pose_of((0.05, 0.04, -0.03), (0.06, 0.05, -0.04))):
        p, rec, tr = SR.align(vol, d, cam, start, n_iterations=8, stop_rotation=0.0, stop_translation=0.0)
        assert rec["status"] == 0 and rec["iterations"] == 8 and len(tr) == 8 and rec["cost_last"] < rec["cost_first"]
        ends.append(p)
    e0, e1 = OF.pose_error(pose, np.eye(4)), OF.pose_error(ends[0], np.eye(4))
    assert e1[0] < 0.5 * e0[0] and e1[1] < 0.5 * e0[1]
    assert np.abs(ends[0] - ends[1]).max() < 1e-3
    p, rec, tr = SR.align(vol, d, cam, pose, stop_rotation=1e-4, stop_translation=1e-4)
    assert rec["iterations"] < 20 and np.array_equal(p, tr[-1]["pose"])
    away = pose_of((0, 3.0, 0), (0, 0, -1.0))
    p, rec, tr = SR.align(vol, d, cam, away)
    assert rec["status"] == SR.ERR_NO_CORRESPONDENCES and np.array_equal(p, away) and rec["iterations"] == 1
    p, rec, tr = SR.align(vol, np.full((30, 40), -np.inf, f32), cam, pose)
    assert rec["status"] == SR.ERR_NO_SOURCE and rec["n_depth"] == 0 and np.array_equal(p, pose)


def test_option_validation_without_a_device():
    from icp_amd import binding
    lib = binding.load_library()
    chk = lambda o: lib.icp_sdf_options_check(ctypes.byref(o))
    o = binding.sdf_options()
    assert chk(o) == 0 and lib.icp_sdf_options_check(None) == 1 and lib.icp_sdf_options_default(None) == 1
    assert (o.stride, o.n_iterations, o.min_valid, o.huber, o.stop_rotation, o.stop_translation) == (1, 20, 64, 0.0, f32(1e-5), f32(1e-5))
    inf, nan = float("inf"), float("nan")
    bad = [dict(stride=0), dict(stride=-1), dict(n_iterations=0), dict(n_iterations=1001), dict(min_valid=5), dict(huber=-0.1), dict(huber=nan), dict(huber=inf),
           dict(stop_rotation=-1e-6), dict(stop_rotation=nan), dict(stop_translation=-1.0), dict(stop_translation=inf)]
    for kw in bad:
        assert chk(binding.sdf_options(**kw)) == 1, kw
    good = [dict(stride=16), dict(n_iterations=1), dict(n_iterations=1000), dict(min_valid=6), dict(huber=0.05), dict(stop_rotation=0.0), dict(stop_translation=0.0)]
    for kw in good:
        assert chk(binding.sdf_options(**kw)) == 0, kw
    with pytest.raises(TypeError):
        binding.sdf_options(iterations=3)
    # every entry point refuses a null context
    cam = binding.depth_camera(tum_K(40), 40, 30); p = binding.pose_to_c(np.eye(4))
    assert lib.icp_tsdf_sample(None, None, 0, None, None, None) == 1
    assert lib.icp_tsdf_sdf_system(None, None, ctypes.byref(cam), binding._ptr(p), ctypes.byref(o), None, None) == 1
    assert lib.icp_tsdf_align_depth(None, None, ctypes.byref(cam), ctypes.byref(o), binding._ptr(p), None, None) == 1
    assert lib.icp_track_depth_sdf(None, None, None, 1, ctypes.byref(cam), ctypes.byref(o), binding._ptr(p), None) == 1


def test_structs_symbols_and_python_surface():
    from icp_amd import binding, tum
    assert ctypes.sizeof(binding.IcpSdfOptions) == 24 and binding.IcpSdfOptions.huber.offset == 12
    assert ctypes.sizeof(binding.IcpSdfIter) == 80 and binding.IcpSdfIter.cost.offset == 8 and binding.IcpSdfIter.pose.offset == 16
    assert ctypes.sizeof(binding.IcpSdfFrame) == 104 and binding.IcpSdfFrame.cost_first.offset == 24 and binding.IcpSdfFrame.pose.offset == 40
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for name in ("icp_sdf_options_default", "icp_sdf_options_check", "icp_tsdf_sample", "icp_tsdf_sdf_system", "icp_tsdf_align_depth", "icp_track_depth_sdf"):
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    for struct in ("icp_sdf_options", "icp_sdf_iter", "icp_sdf_frame"):
        assert re.search(r"^\} %s;" % struct, hdr, flags=re.M), struct
    for m in ("tsdf_sample", "tsdf_sdf_system", "tsdf_align_depth", "track_depth_sdf"):
        assert hasattr(binding.Context, m), m
    for fn in (tum.track, tum.reconstruct_room):
        assert inspect.signature(fn).parameters["sdf"].default is None, fn
    with pytest.raises(ValueError):
        tum.track(None, dict(), sdf=dict(stride=4))          # refused before anything is touched


def test_kernel_resource_record():
    """The new kernels from the compiled code object: no scratch, no AGPRs.  k_sdf_accumulate holds a pixel's 28 fp64 terms (56 registers)
    next to eight corners in flight: 85 VGPRs recorded, budget 96 (five waves per SIMD, above the four an iteration's latency-bound gather
    asks for; its grid is at most a few blocks per CU).  k_sdf_solve, one block: 94 recorded, budget 96.  k_tsdf_sample, a streaming pass: 32
    recorded, budget 40.  k_sdf_init: 6 recorded, budget 16.  Static LDS: the block fold's 4 x 28 x 17 doubles and 8 ints for
    k_sdf_accumulate, the solver's workspaces for k_sdf_solve (4 KiB bound).  Recorded: see DESIGN.md section 6q."""
    text = device_asm()
    seen = kernel_resources(text)
    budget = {"_ZN6icpdev16k_sdf_accumulate": (96, 4 * 28 * 17 * 8 + 32), "_ZN6icpdev11k_sdf_solve": (96, 4096), "_ZN6icpdev13k_tsdf_sample": (40, 0),
              "_ZN6icpdev10k_sdf_init": (16, 0)}
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


def test_recorded_outcome_beats_the_raycast_model_loop():
    """tests/golden/sdf_outcome.json (the restatement's loop at stride 4, 20 iterations; written by tests/sdf_outcome_fixture.py) against
    tests/golden/tsdf_outcome.json (the ray-cast model loop with the oracle's ICP) on the same 41-frame pan: the worst rotation and the
    worst translation are both lower.  Prototype: 0.0075 < 0.0187 rad and 0.039 < 0.070 m."""
    with open(SF.GOLDEN) as f:
        sdf = json.load(f)
    with open(OF.GOLDEN) as f:
        ray = json.load(f)
    print("SDF loop: worst %.4f rad / %.4f m; ray-cast model loop: worst %.4f rad / %.4f m" % (sdf["worst_rotation_rad"], sdf["worst_translation_m"],
                                                                                              ray["worst_rotation_rad"], ray["worst_translation_m"]))
    assert sdf["frames"] == ray["frames"] == OF.N_FRAMES and (sdf["stride"], sdf["n_iterations"]) == (4, 20) and sdf["statuses"] == [0]
    assert sdf["worst_rotation_rad"] < ray["worst_rotation_rad"] and sdf["worst_translation_m"] < ray["worst_translation_m"]
