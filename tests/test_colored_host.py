"""Colored ICP on the host side: the options record, the new symbols, the entry points without a device, the numpy restatement
(tests/colored_restatement.py) against independent derivations and on the textured-plane fixture, and the register / scratch budget of
the new kernels (compile only)."""
import ctypes
import os
import re
import numpy as np
from scipy.spatial import cKDTree

import colored_restatement as CR
from device_asm import device_asm, kernel_resources

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32


def test_options_layout_and_defaults():
    from icp_amd import binding
    assert ctypes.sizeof(binding.IcpColoredOptions) == 8
    assert binding.IcpColoredOptions.gradient_k.offset == 4 and binding.METRIC_COLORED == 4
    assert ctypes.sizeof(binding.IcpParams) == 80
    o = binding.IcpColoredOptions()
    lib = binding.load_library()
    assert lib.icp_colored_options_default(ctypes.byref(o)) == 0
    assert o.lambda_geometric == f32(0.968) and o.gradient_k == 20
    assert lib.icp_colored_options_default(None) == 1


def test_new_symbols_exported():
    from icp_amd import binding
    lib = binding.load_library()
    for name in ("icp_colored_options_default", "icp_set_colored_options", "icp_get_colored_options", "icp_get_color_gradients"):
        assert name in binding.EXPORTS and hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    assert "ICP_METRIC_COLORED = 4" in hdr and "int icp_get_color_gradients(icp_ctx* ctx" in hdr
    assert "int setColoredICPOptions(float lambda_geometric, unsigned k)" in open(os.path.join(ROOT, "include", "icp_hip_adaptor.hpp")).read()
    assert hasattr(binding.LinearICPOptimizer, "setColoredICPOptions") and hasattr(binding.Context, "color_gradients")


def test_null_context_refused():
    from icp_amd import binding
    lib = binding.load_library()
    o = binding.IcpColoredOptions(0.968, 20)
    out = np.zeros((4, 3), np.float32); n = ctypes.c_int32(0)
    assert lib.icp_set_colored_options(None, ctypes.byref(o)) == 1
    assert lib.icp_set_colored_options(None, None) == 1
    assert lib.icp_get_colored_options(None, ctypes.byref(o)) == 1
    assert lib.icp_get_color_gradients(None, out.ctypes.data_as(ctypes.c_void_p), 4, ctypes.byref(n)) == 1


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])


def test_jacobians_match_central_differences():
    """With x = (alpha, beta, gamma, tx, ty, tz) and p(x) = Rx Ry Rz p + t: d/dx of the exact geometric residual n.(q - p(x)) is -j_G and
    d/dx of the exact photometric residual I_s - I_q - u.(p(x) - q) is -j_C at x = 0; the gradient of the exact objective
    1/2 sum w^2 (lambda r_G^2 + (1 - lambda) r_C^2) is -g."""
    rng = np.random.default_rng(5)
    m, lam = 40, 0.7
    p = rng.normal(size=(m, 3)).astype(f32); q = (p + 0.01 * rng.normal(size=(m, 3))).astype(f32)
    n = rng.normal(size=(m, 3)).astype(f32); d = rng.normal(size=(m, 3)).astype(f32)
    di = rng.normal(size=m) * 0.1; w = rng.uniform(0.2, 1, m).astype(f32)
    ok, H, g, jG, rG, jC, rC = CR.pair_terms(p, q, n, d, di, w, lam)
    assert ok.all()
    P, Q = p.astype(np.float64), q.astype(np.float64)
    nu = n / np.linalg.norm(n.astype(np.float64), axis=1, keepdims=True)
    u = d - nu * np.sum(nu * d, 1, keepdims=True)
    lam = float(f32(lam))

    def moved(x):
        return P @ _rot(*x[:3]).T + x[3:6]

    def res_g(x):
        return np.sum(nu * (Q - moved(x)), 1)

    def res_c(x):
        return di - np.sum(u * (moved(x) - Q), 1)

    def energy(x):
        return 0.5 * np.sum(w.astype(np.float64) ** 2 * (lam * res_g(x) ** 2 + (1 - lam) * res_c(x) ** 2))
    assert np.allclose(res_g(np.zeros(6)), rG, atol=1e-12) and np.allclose(res_c(np.zeros(6)), rC, atol=1e-12)
    h = 1e-6
    for k in range(6):
        e = np.zeros(6); e[k] = h
        assert np.allclose((res_g(e) - res_g(-e)) / (2 * h), -jG[:, k], atol=1e-8), k
        assert np.allclose((res_c(e) - res_c(-e)) / (2 * h), -jC[:, k], atol=1e-8), k
        de = (energy(e) - energy(-e)) / (2 * h)
        assert abs(de + g.sum(0)[k]) <= 1e-6 * (np.abs(g).sum() + 1e-12), k
    # H is the Gauss-Newton matrix of that objective
    Jg = np.stack([-(res_g(np.eye(6)[k] * h) - res_g(-np.eye(6)[k] * h)) / (2 * h) for k in range(6)], 1)
    Jc = np.stack([-(res_c(np.eye(6)[k] * h) - res_c(-np.eye(6)[k] * h)) / (2 * h) for k in range(6)], 1)
    W2 = w.astype(np.float64) ** 2
    Href = np.einsum("m,mi,mj->ij", W2 * lam, Jg, Jg) + np.einsum("m,mi,mj->ij", W2 * (1 - lam), Jc, Jc)
    assert np.allclose(H.sum(0), Href, rtol=1e-6, atol=1e-8)


def test_gradients_recover_a_linear_ramp():
    """On a plane whose intensity is a linear function of position, the gradient is that function's in-plane gradient (up to uint8
    quantisation); degenerate points give NaN / zero as the contract says."""
    ax = np.arange(-0.1, 0.1001, 0.005)
    X, Y = np.meshgrid(ax, ax, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size)], 1).astype(f32)
    nrm = np.tile(f32([0, 0, 1]), (len(pts), 1))
    gval = np.clip(np.round(255 * (0.5 + 1.0 * pts[:, 0] - 0.5 * pts[:, 1])), 0, 255).astype(np.uint8)
    rgba = np.stack([gval, gval, gval, np.full_like(gval, 255)], 1)
    pts[7] = np.nan; nrm[11] = 0.0; nrm[13] = np.inf
    grad, margin = CR.gradients(pts, nrm, rgba, 20)
    assert np.isnan(grad[[7, 11, 13]]).all()
    inner = (np.abs(pts[:, 0]) < 0.07) & (np.abs(pts[:, 1]) < 0.07)
    assert np.abs(grad[inner] - f32([1.0, -0.5, 0.0])).max() < 0.12 and np.abs(np.median(grad[inner], 0) - [1.0, -0.5, 0.0]).max() < 0.02
    assert (margin[inner] > 2).all()
    # fewer than 3 finite points: zeros for the live ones
    few = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0]], f32)
    g2, _ = CR.gradients(few, np.tile(f32([0, 0, 1]), (3, 1)), np.zeros((3, 4), np.uint8), 5)
    assert np.array_equal(g2[:2], np.zeros((2, 3), f32)) and np.isnan(g2[2]).all()


def _run(d, lam, iters, k=20, max_d2=0.01):
    """The restatement's free-running loop on the fixture: nearest-neighbour matching (d^2 <= max_d2), constant weights."""
    grad, _ = CR.gradients(d["tgt_pts"], d["tgt_nrm"], d["tgt_rgba"], k)
    tree = cKDTree(d["tgt_pts"].astype(np.float64))
    pose = np.eye(4, dtype=f32)
    for _ in range(iters):
        p = CR.transform(pose, d["src_pts"])
        dist, j = tree.query(p.astype(np.float64))
        keep = dist ** 2 <= max_d2
        pose, s = CR.step(pose, d["src_pts"][keep], d["tgt_pts"][j[keep]], d["tgt_nrm"][j[keep]], grad[j[keep]], d["src_rgba"][keep],
                          d["tgt_rgba"][j[keep]], np.ones(keep.sum(), f32), lam, lstsq=lam == 1.0)
    return pose


def _pose_error(a, b):
    R = np.asarray(a, np.float64)[:3, :3] @ np.asarray(b, np.float64)[:3, :3].T
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    return ang, np.linalg.norm(np.asarray(a, np.float64)[:3, 3] - np.asarray(b, np.float64)[:3, 3])


def test_step_recovers_textured_plane_pose():
    """The capability in numpy: on the textured plane lambda = 0.968 reaches the true pose, lambda = 1 (geometry only) stays put."""
    d = CR.textured_plane(n_src=8000)
    ang, tr = _pose_error(_run(d, 0.968, 40), d["gt"])
    assert ang < 1e-3 and tr < 1e-3, (ang, tr)
    ang1, tr1 = _pose_error(_run(d, 1.0, 10), d["gt"])
    assert tr1 > 0.02, (ang1, tr1)


def test_new_kernels_register_budget():
    """k_color_gradients<5|10|20>: no scratch, at most 128 VGPRs; k_post_colored: no scratch, at most 136 VGPRs (it holds 34 fp64
    accumulators and two Jacobian rows)."""
    seen = kernel_resources(device_asm())
    grads = {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev17k_color_gradientsILi")}
    assert sorted(re.search(r"ILi(\d+)E", n).group(1) for n in grads) == ["10", "20", "5"], list(grads)
    post = {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev14k_post_colored")}
    assert len(post) == 1, list(post)
    for name, f in grads.items():
        assert f["private_seg_size"] == 0 and f["num_vgpr"] <= 128, (name, f)
    for name, f in post.items():
        assert f["private_seg_size"] == 0 and f["num_vgpr"] <= 136, (name, f)
