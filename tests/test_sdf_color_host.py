"""Direct SDF tracking with the photometric term on the host side: the numpy restatement of the contract (tests/sdf_color_restatement.py)
against finite differences and against a densely assembled J^T J, its geometric half against sdf_restatement bit for bit, option
validation through the library without a device, the new structs, symbols and Python surface, the resource record of the new kernels
(compile only), and the recorded outcome of the two CPU loops on the textured wall."""
import ctypes
import inspect
import json
import os
import re
import numpy as np
import pytest

import sdf_color_restatement as SC
import sdf_restatement as SR
import tsdf_color_restatement as TC
import tsdf_restatement as TS
import sdf_color_outcome_fixture as CO
from device_asm import device_asm, kernel_resources
from icp_amd.synth import tum_K, wavy_depth
from support import pose_of

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32, f64 = np.float32, np.float64
SMALL = dict(dims=(37, 21, 29), origin=(-1.8, -1.0, -0.5), voxel_size=0.1, truncation=0.3, max_weight=64.0, min_depth=0.3, max_depth=2.4)
W, H = 40, 30
NEAR = ((0.02, -0.015, 0.01), (0.03, -0.02, 0.02))


def small_model():
    cam = TS.Camera(tum_K(W), W, H)
    vol = TS.Volume(**SMALL)
    for _ in range(2):
        TS.integrate(vol, wavy_depth(W, H), cam, np.eye(4, dtype=f32))
    rgbx = np.random.default_rng(3).integers(0, 256, (W * H, 4), dtype=np.uint8)
    return SC.smooth_colors(vol), cam, rgbx


def intensity64(vol, q):
    """The trilinear interpolant of s = (R + G) + B (the fp32 corner values) in the cell of q over 765, everything else in fp64:
    (value, fractions, the largest corner difference along an edge)."""
    g = (q - vol.o.astype(f64)) / f64(vol.s)
    i = np.floor(g).astype(int); t = g - i
    c = vol.rgb[i[2]:i[2] + 2, i[1]:i[1] + 2, i[0]:i[0] + 2]
    s = ((c[..., 0] + c[..., 1]) + c[..., 2]).astype(f64)                         # [dz, dy, dx]
    edge = max(np.abs(np.diff(s, axis=a)).max() for a in range(3))
    cz = s[0] * (1 - t[2]) + s[1] * t[2]
    cy = cz[0] * (1 - t[1]) + cz[1] * t[1]
    return (cy[0] * (1 - t[0]) + cy[1] * t[0]) / 765.0, t, edge


def increment64(x):
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]); Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]]); Rz = np.array([[cg, -sg, 0], [sg, cg, 0], [0, 0, 1]])
    D = np.eye(4); D[:3, :3] = Rx @ Ry @ Rz; D[:3, 3] = x[3:]
    return D


def test_color_jacobian_against_finite_differences():
    """J_c = (q x h, h) against central differences of r_c(dT q) in the six components of a left-multiplied increment, step 1e-6, on
    coloured pixels whose point stays in its cell (fractions in [0.01, 0.99]; the point moves by less than 4e-5 voxels).  I_p does not
    move with the pose, and inside a cell S is a polynomial, so the central difference is exact to O(step^2).  What is left is the fp32
    rounding of the restatement's gradient H: six operations on corner differences of magnitude <= 64 (asserted), 6 x 64 x 2^-24 = 2.3e-5
    per voxel in byte units, / (765 x voxel_size 0.1) = 3.0e-7 per metre in intensity, x |q| <= 3 m in the rotational columns = 9e-7:
    bound 1e-6 on every component (test_sdf_host.py's derivation, with this field's magnitudes)."""
    vol, cam, rgbx = small_model()
    pose = pose_of(*NEAR)
    t = SC.pixel_terms(vol, wavy_depth(W, H), rgbx, cam, pose)
    Jc = SR.jacobian(t["q"], t["h"])
    px = rgbx[t["v"] * W + t["u"]].astype(np.int64)
    step, checked, worst = 1e-6, 0, 0.0
    for k in np.nonzero(t["colored"])[0]:
        q = t["q"][k].astype(f64)
        s0, fr, edge = intensity64(vol, q)
        if not ((fr > 0.01) & (fr < 0.99)).all():
            continue
        assert edge <= 64.0 and np.linalg.norm(q) < 3.0
        assert abs((s0 - px[k, :3].sum() / 765.0) - t["r_c"][k]) < 1e-6          # the same cell, the same field, the pixel's own bytes
        fd = np.empty(6)
        for a in range(6):
            x = np.zeros(6); x[a] = step
            Dp, Dm = increment64(x), increment64(-x)
            fd[a] = (intensity64(vol, Dp[:3, :3] @ q + Dp[:3, 3])[0] - intensity64(vol, Dm[:3, :3] @ q + Dm[:3, 3])[0]) / (2 * step)
        worst = max(worst, float(np.abs(fd - Jc[k]).max()))
        checked += 1
    print("colour Jacobian against finite differences: %d pixels, worst |J_c - fd| = %.3g" % (checked, worst))
    assert checked > 300 and worst < 1e-6
    assert np.abs(Jc[t["colored"]]).max() > 0.1                   # the columns are not all near zero


def test_sums_against_dense_assembly():
    """The 29 sums against J^T W J + J_c^T W_c J_c, the right-hand side and the two costs assembled densely from the per-pixel terms, with
    both Huber weights on: within (n_valid + n_color) 2^-52 sum(|geometric term| + |photometric term|)."""
    vol, cam, rgbx = small_model()
    vol.wc[:, :, 20:] = 0                                         # a part of the frame valid but uncoloured
    d = wavy_depth(W, H); d[0, :6] = [-np.inf, np.nan, np.inf, 0.0, -1.0, 2.5]
    pose = pose_of(*NEAR)
    kw = dict(huber=0.05, weight=0.25, color_huber=0.2)
    (nd, nv, nc), s, a = SC.system(vol, d, rgbx, cam, pose, **kw)
    assert nd == W * H - 6 and 0 < nc < nv < nd
    t = SC.pixel_terms(vol, d, rgbx, cam, pose)
    m, c = t["valid"], t["colored"]
    J = SR.jacobian(t["q"][m], t["g"][m]); r = t["r"][m]; w = np.where(np.abs(r) <= f64(f32(0.05)), 1.0, f64(f32(0.05)) / np.abs(r))
    Jc = SR.jacobian(t["q"][c], t["h"][c]); rc = t["r_c"][c]
    wc = f64(f32(0.25)) ** 2 * np.where(np.abs(rc) <= f64(f32(0.2)), 1.0, f64(f32(0.2)) / np.abs(rc))
    assert (w < 1).any() and (wc < wc.max()).any()
    Hd = J.T @ (w[:, None] * J) + Jc.T @ (wc[:, None] * Jc)
    b = -(J.T @ (w * r)) - Jc.T @ (wc * rc)
    bound = (nv + nc) * 2.0 ** -52 * a
    k = 0
    for i in range(6):
        for j in range(i, 6):
            assert abs(s[k] - Hd[i, j]) <= bound[k], (i, j); k += 1
    assert (np.abs(s[21:27] - b) <= bound[21:27]).all()
    assert abs(s[27] - (r @ (w * r) + rc @ (wc * rc))) <= bound[27] and abs(s[28] - rc @ (wc * rc)) <= bound[28] and 0 < s[28] < s[27]
    # the restatement's alignment runs on the joint system
    p, rec, tr = SC.align(vol, d, rgbx, cam, pose, n_iterations=8, stop_rotation=0.0, stop_translation=0.0, **kw)
    assert rec["status"] == 0 and rec["iterations"] == 8 and len(tr) == 8 and rec["n_color_last"] > 0 and rec["cost_color_last"] > 0


def test_uncoloured_volume_reduces_to_the_geometric_system():
    """With every Wc zeroed the entries 0 .. 27 are sdf_restatement.system's bit for bit, n_color is 0 and entry 28 is 0."""
    vol, cam, rgbx = small_model()
    vol.wc[:] = 0
    d = wavy_depth(W, H); d[0, :6] = [-np.inf, np.nan, np.inf, 0.0, -1.0, 2.5]
    for pose in (np.eye(4, dtype=f32), pose_of(*NEAR)):
        for stride, huber in ((1, 0.0), (3, 0.05)):
            (nd, nv, nc), s, a = SC.system(vol, d, rgbx, cam, pose, stride=stride, huber=huber, weight=0.5)
            (gd, gv), gs, ga = SR.system(vol, d, cam, pose, stride=stride, huber=huber)
            assert (nd, nv, nc) == (gd, gv, 0) and nv > 50
            assert np.array_equal(s[:28].view(np.uint64), gs.view(np.uint64)) and np.array_equal(a[:28].view(np.uint64), ga.view(np.uint64))
            assert s[28] == 0 and a[28] == 0
    # and a corner colour that is not finite takes the pixel's photometric row out, not its geometric one
    vol.wc[:] = 1
    full = SC.system(vol, d, rgbx, cam, np.eye(4, dtype=f32))[0]
    t = SC.pixel_terms(vol, d, rgbx, cam, np.eye(4, dtype=f32))
    q = t["q"][np.nonzero(t["colored"])[0][400]].astype(f64)
    i = np.floor((q - vol.o.astype(f64)) / f64(vol.s)).astype(int)
    vol.rgb[i[2], i[1], i[0], 1] = np.nan                          # the low corner of a coloured pixel's cell
    nan = SC.system(vol, d, rgbx, cam, np.eye(4, dtype=f32))
    assert nan[0][1] == full[1] and nan[0][2] < full[2] and np.isfinite(nan[1]).all()


def test_option_validation_without_a_device():
    from icp_amd import binding
    lib = binding.load_library()
    chk = lambda o: lib.icp_sdf_color_options_check(ctypes.byref(o))
    o = binding.sdf_color_options()
    assert chk(o) == 0 and lib.icp_sdf_color_options_check(None) == 1 and lib.icp_sdf_color_options_default(None) == 1
    assert (o.weight, o.huber) == (f32(0.1), 0.0)
    inf, nan = float("inf"), float("nan")
    for kw in (dict(weight=0.0), dict(weight=-0.1), dict(weight=nan), dict(weight=inf), dict(huber=-0.1), dict(huber=nan), dict(huber=inf)):
        assert chk(binding.sdf_color_options(**kw)) == 1, kw
    for kw in (dict(weight=1e-3), dict(weight=10.0), dict(huber=0.05), dict(huber=0.0)):
        assert chk(binding.sdf_color_options(**kw)) == 0, kw
    with pytest.raises(TypeError):
        binding.sdf_color_options(color_weight=0.1)
    # every entry point refuses a null context
    cam = binding.depth_camera(tum_K(W), W, H); p = binding.pose_to_c(np.eye(4)); so = binding.sdf_options()
    assert lib.icp_tsdf_sample_color(None, None, 0, None, None, None) == 1
    assert lib.icp_tsdf_sdf_system_color(None, None, None, ctypes.byref(cam), binding._ptr(p), ctypes.byref(so), ctypes.byref(o), None, None) == 1
    assert lib.icp_tsdf_align_depth_color(None, None, None, ctypes.byref(cam), ctypes.byref(so), ctypes.byref(o), binding._ptr(p), None, None) == 1
    assert lib.icp_track_depth_sdf_color(None, None, None, 1, ctypes.byref(cam), ctypes.byref(so), ctypes.byref(o), binding._ptr(p), None) == 1


def test_structs_symbols_and_python_surface():
    from icp_amd import binding, tum
    assert ctypes.sizeof(binding.IcpSdfOptions) == 24                             # icp_sdf_options keeps its layout
    assert ctypes.sizeof(binding.IcpSdfColorOptions) == 8 and binding.IcpSdfColorOptions.huber.offset == 4
    assert ctypes.sizeof(binding.IcpSdfColorIter) == 96 and binding.IcpSdfColorIter.cost.offset == 16 and binding.IcpSdfColorIter.cost_color.offset == 24 \
        and binding.IcpSdfColorIter.pose.offset == 32
    assert ctypes.sizeof(binding.IcpSdfColorFrame) == 128 and binding.IcpSdfColorFrame.cost_first.offset == 32 and binding.IcpSdfColorFrame.cost_color_last.offset == 56 \
        and binding.IcpSdfColorFrame.pose.offset == 64
    lib = binding.load_library()
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    for name in ("icp_sdf_color_options_default", "icp_sdf_color_options_check", "icp_tsdf_sample_color", "icp_tsdf_sdf_system_color", "icp_tsdf_align_depth_color",
                 "icp_track_depth_sdf_color"):
        assert name in binding.EXPORTS and hasattr(lib, name), name
        assert re.search(r"^int %s\(" % name, hdr, flags=re.M), name
    for struct, size in (("icp_sdf_color_options", 8), ("icp_sdf_color_iter", 96), ("icp_sdf_color_frame", 128)):
        assert re.search(r"^\} %s;" % struct, hdr, flags=re.M), struct
        assert re.search(r"^static_assert\(sizeof\(%s\) == %d," % (struct, size), hdr, flags=re.M), struct
    assert "alignment never reads the colour array" not in hdr
    assert hasattr(binding.Context, "tsdf_sample_color") and callable(binding.sdf_color_options)
    for m in ("tsdf_sdf_system", "tsdf_align_depth"):
        prm = inspect.signature(getattr(binding.Context, m)).parameters
        assert prm["rgbx"].default is None and prm["color_weight"].default == 0.0 and prm["color_huber"].default == 0.0, m
    prm = inspect.signature(binding.Context.track_depth_sdf).parameters
    assert prm["rgbx_frames"].default is None and prm["color_weight"].default == 0.0 and prm["color_huber"].default == 0.0
    # refused before anything is touched: a colour weight without colour frames, or without a coloured model
    with pytest.raises(ValueError):
        binding._sdf_color_in(None, 12, 0.1, 0.0, "")
    assert binding._sdf_color_in(None, 12, 0.0, 0.0, "") == (None, None)
    for model in (dict(dims=(8, 8, 8), origin=(0, 0, 0)), dict(dims=(8, 8, 8), origin=(0, 0, 0), color=False)):
        for fn in (tum.track, tum.reconstruct_room):
            with pytest.raises(ValueError):
                fn(None, dict(), model=model, sdf=dict(stride=4, color_weight=0.1))
    with pytest.raises(ValueError):
        tum.track(None, dict(), sdf=dict(stride=4, color_weight=0.1))


def test_kernel_resource_record():
    """The new kernels from the compiled code object: no scratch, no AGPRs.  k_sdf_accumulate_color holds a pixel's 29 fp64 sums (58
    registers) next to eight 16-byte colour corners in flight and adds the photometric row into the registers of the geometric one: 98
    VGPRs recorded, budget 128 (four waves per SIMD, what an iteration's latency-bound gather asks for).  k_sdf_solve_color, one block:
    106 recorded, budget 128.  k_tsdf_sample_color, a streaming pass with eight float4 in flight: 44 recorded, budget 48.
    k_sdf_init_color: 6 recorded, budget 16.  Static LDS: the block fold's 4 x 29 x 17 doubles and 12 ints for k_sdf_accumulate_color,
    the solver's workspaces for k_sdf_solve_color (4 KiB bound).  Recorded: see DESIGN.md section 6r."""
    text = device_asm()
    seen = kernel_resources(text)
    budget = {"_ZN6icpdev22k_sdf_accumulate_color": (128, 4 * 29 * 17 * 8 + 48), "_ZN6icpdev17k_sdf_solve_color": (128, 4096),
              "_ZN6icpdev19k_tsdf_sample_color": (48, 0), "_ZN6icpdev16k_sdf_init_color": (16, 0)}
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


def test_recorded_outcome_separates_the_two_trackers():
    """tests/golden/sdf_color_outcome.json (written by tests/sdf_color_outcome_fixture.py: the textured wall at stride 2, 20 iterations,
    default stops, weight 0.1) holds both CPU loops: twice the coloured loop's worst translation error stays below half the lateral travel,
    and the geometric loop ends more than half the travel away.  Recorded: 2 x 0.0018 = 0.0036 < 0.055 < 0.088."""
    with open(CO.GOLDEN) as f:
        g = json.load(f)
    travel = g["lateral_travel_m"]
    print("coloured SDF loop: worst %.4f m, last %.4f m, iterations %s; geometric SDF loop: worst %.4f m, last %.4f m; travel %.2f m"
          % (g["colored_worst_translation_m"], g["colored_last_translation_m"], g["colored_iterations"], g["geometric_worst_translation_m"],
             g["geometric_last_translation_m"], travel))
    assert (g["stride"], g["n_iterations"], g["weight"], g["frames"]) == (2, 20, 0.1, 12) and g["colored_statuses"] == [0]
    assert 2 * g["colored_worst_translation_m"] < travel / 2 < g["geometric_last_translation_m"]
