"""Generalized-ICP on the host side: the options record, the new symbols, the entry points without a device, the numpy restatement
(tests/gicp_restatement.py) against independent derivations, and the register / scratch budget of the new kernels (compile only)."""
import ctypes
import os
import re
import numpy as np

import gicp_restatement as G
from device_asm import device_asm, kernel_resources

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_options_layout_and_defaults():
    from icp_amd import binding
    assert ctypes.sizeof(binding.IcpGicpOptions) == 8
    assert binding.IcpGicpOptions.covariance_k.offset == 4 and binding.METRIC_GICP == 3
    o = binding.IcpGicpOptions()
    assert binding.load_library().icp_gicp_options_default(ctypes.byref(o)) == 0
    assert o.epsilon == np.float32(1e-3) and o.covariance_k == 20
    assert binding.load_library().icp_gicp_options_default(None) == 1


def test_new_symbols_exported():
    from icp_amd import binding
    lib = binding.load_library()
    for name in ("icp_gicp_options_default", "icp_set_gicp_options", "icp_get_gicp_options", "icp_get_gicp_normals"):
        assert name in binding.EXPORTS and hasattr(lib, name), name
    hdr = open(os.path.join(ROOT, "include", "icp_hip.h")).read()
    assert "ICP_METRIC_GICP = 3" in hdr and "int icp_get_gicp_normals(icp_ctx* ctx" in hdr


def test_null_context_refused():
    from icp_amd import binding
    lib = binding.load_library()
    o = binding.IcpGicpOptions(1e-3, 20)
    out = np.zeros((4, 3), np.float32); n = ctypes.c_int32(0)
    assert lib.icp_set_gicp_options(None, ctypes.byref(o)) == 1
    assert lib.icp_get_gicp_options(None, ctypes.byref(o)) == 1
    assert lib.icp_get_gicp_normals(None, 0, out.ctypes.data_as(ctypes.c_void_p), 4, ctypes.byref(n)) == 1


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])


def test_jacobian_matches_central_differences():
    """d r / d x of the exact residual r(x) = q - (Rx Ry Rz p + t) at x = 0 is -J, and the gradient of the exact objective
    1/2 sum w^2 r^T M r (M at the linearisation point) is -g."""
    rng = np.random.default_rng(5)
    m = 40
    p = rng.normal(size=(m, 3)).astype(np.float32); q = (p + 0.01 * rng.normal(size=(m, 3))).astype(np.float32)
    a = rng.normal(size=(m, 3)).astype(np.float32); b = rng.normal(size=(m, 3)).astype(np.float32); w = rng.uniform(0.2, 1, m).astype(np.float32)
    ok, H, g, S, M, J, r = G.pair_terms(p, q, a, b, w, 1e-3)
    assert ok.all()
    P, Q = p.astype(np.float64), q.astype(np.float64)

    def resid(x):
        return Q - (P @ _rot(*x[:3]).T + x[3:6])

    def energy(x):
        rr = resid(x)
        return 0.5 * np.sum(w.astype(np.float64) ** 2 * np.einsum("mi,mij,mj->m", rr, M, rr))
    h = 1e-6
    for k in range(6):
        e = np.zeros(6); e[k] = h
        dr = (resid(e) - resid(-e)) / (2 * h)
        assert np.allclose(dr, -J[:, :, k], atol=1e-8), k
        de = (energy(e) - energy(-e)) / (2 * h)
        assert abs(de + g.sum(0)[k]) <= 1e-6 * (np.abs(g).sum() + 1e-12), k
    # Sigma: the two plane covariances, |Sigma^-1 Sigma - I| tiny, eigenvalues >= 2 eps
    an = a / np.linalg.norm(a, axis=1, keepdims=True); bn = b / np.linalg.norm(b, axis=1, keepdims=True)
    assert np.allclose(S, G.plane_cov(an, 1e-3) + G.plane_cov(bn, 1e-3), atol=1e-15)
    assert np.allclose(np.einsum("mij,mjk->mik", M, S), np.eye(3), atol=1e-9)
    assert np.linalg.eigvalsh(S).min() >= 2e-3 * (1 - 1e-12)


def test_step_reaches_a_known_pose():
    """The step iterated on exact correspondences (points on five planes, each cloud with its own normals) recovers the pose."""
    rng = np.random.default_rng(11)
    pts, nrm = [], []
    for _ in range(5):
        n = rng.normal(size=3); n /= np.linalg.norm(n)
        u = np.cross(n, [1.0, 0, 0]); u /= np.linalg.norm(u); v = np.cross(n, u)
        c = rng.normal(size=3)
        st = rng.uniform(-0.5, 0.5, size=(200, 2))
        pts.append(c + st[:, :1] * u + st[:, 1:] * v); nrm.append(np.broadcast_to(n, (200, 3)))
    tgt = np.concatenate(pts).astype(np.float32); tn = np.concatenate(nrm).astype(np.float32)
    T = np.eye(4); T[:3, :3] = _rot(0.03, -0.02, 0.04); T[:3, 3] = (0.02, -0.01, 0.015)
    Ti = np.linalg.inv(T)
    src = (tgt.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    sn = (tn.astype(np.float64) @ Ti[:3, :3].T).astype(np.float32)
    pose = np.eye(4, dtype=np.float32)
    for _ in range(12):
        pose, s = G.step(pose, src, tgt, sn, tn, np.ones(len(src), np.float32), 1e-3)
        assert s[0] == len(src)
    R = pose[:3, :3].astype(np.float64) @ T[:3, :3].T
    ang = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    assert ang < 2e-6 and np.abs(pose[:3, 3] - T[:3, 3]).max() < 2e-6, (ang, pose, T)


def test_covariance_equals_eigendecomposition_form():
    """I - (1 - eps) n n^T with the restatement's normal equals V diag(eps, 1, 1) V^T of each neighbourhood's full eigendecomposition."""
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(300, 3)) * (1.0, 0.6, 0.05)
    pts = pts.astype(np.float32)
    pts[17] = np.nan
    k, eps = 10, 1e-3
    nrm, ev = G.normals(pts, k)
    assert np.isnan(nrm[17]).all() and np.isfinite(np.delete(nrm, 17, 0)).all()
    nb = G.neighbours(pts, k)
    for i in range(0, 300, 7):
        if i == 17:
            continue
        X = pts[nb[i]].astype(np.float64)
        D = X - X.mean(0)
        w, V = np.linalg.eigh(D.T @ D / len(X))
        ref = V @ np.diag([eps, 1.0, 1.0]) @ V.T
        assert np.allclose(G.plane_cov(nrm[i], eps), ref, atol=1e-6), i
        # the neighbour set is the k smallest (fp32 d2, index) pairs: brute force over every finite point
        fin = np.nonzero(np.isfinite(pts).all(1))[0]
        d2 = G._d2_f32(pts[i][None, :], pts[fin])
        o = np.lexsort((fin, d2))
        assert np.array_equal(nb[i], fin[o][:k])


def test_new_kernels_register_budget():
    """k_gicp_normals<5|10|20> and k_post_gicp: no scratch; k_post_gicp within 128 VGPRs (4 waves per SIMD)."""
    seen = kernel_resources(device_asm())
    normals = {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev14k_gicp_normalsILi")}
    assert sorted(re.search(r"ILi(\d+)E", n).group(1) for n in normals) == ["10", "20", "5"], list(normals)
    for name, f in normals.items():
        assert f["private_seg_size"] == 0, (name, f)
    post = {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev11k_post_gicp")}
    assert len(post) == 1, list(post)
    for name, f in post.items():
        assert f["private_seg_size"] == 0 and f["num_vgpr"] <= 128, (name, f)
