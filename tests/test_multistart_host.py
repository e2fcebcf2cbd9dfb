"""Multi-start ICP on the host side: the result record's layout, the entry point without a device, the start poses, and the register
budget of the new kernels (compile only; no GPU needed)."""
import ctypes
import os
import numpy as np
from device_asm import device_asm, kernel_resources

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_start_result_layout():
    from icp_amd import binding
    assert ctypes.sizeof(binding.IcpStartResult) == 64 + 4 * 4
    assert binding.IcpStartResult.n_inliers.offset == 68 and binding.IcpStartResult.inlier_rmse.offset == 76
    assert "icp_run_multistart" in binding.EXPORTS


def test_entry_point_without_a_device_or_context():
    """No CPU path: without a GPU there is no context (ICP_ERR_NO_DEVICE from icp_ctx_create); a NULL context is refused either way."""
    from icp_amd import binding
    lib = binding.load_library()
    h = ctypes.c_void_p()
    rc = lib.icp_ctx_create(0, ctypes.byref(h))
    if rc == 0:
        lib.icp_ctx_destroy(h)
    else:
        assert rc == 9 and not h.value
    res = (binding.IcpStartResult * 1)()
    pose = np.eye(4, dtype=np.float32).reshape(16)
    assert lib.icp_run_multistart(None, pose.ctypes.data_as(ctypes.c_void_p), 1, res, None, 0, None, None) == 1


def test_start_poses():
    from icp_amd.multistart import rotation, start_poses
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(500, 3)).astype(np.float32) + np.float32([1.0, -2.0, 0.5])
    pts[7] = np.nan
    init = np.eye(4); init[:3, 3] = (0.3, 0.1, -0.2)
    yaws = (0.0, 90.0, -45.0, 180.0)
    P = start_poses(init, yaw_deg=yaws, axis=(0, 0, 1), points=pts)
    assert len(P) == 4 and all(p.dtype == np.float32 and p.shape == (4, 4) for p in P)
    assert np.array_equal(P[0], init.astype(np.float32))
    c = np.nanmean(pts, axis=0).astype(np.float64) + init[:3, 3]          # centroid of the finite points, moved by the initial pose
    for p, yaw in zip(P, yaws):
        R = p[:3, :3].astype(np.float64)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-6) and np.linalg.det(R) > 0
        assert np.allclose(R, rotation((0, 0, 1), yaw), atol=1e-6)
        moved = (p.astype(np.float64) @ np.append(c - init[:3, 3], 1.0))[:3]      # the centroid of the source itself lands on c
        assert np.allclose(moved, c, atol=1e-5)
    R90 = rotation((0, 0, 1), 90.0)
    assert np.allclose(R90 @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], atol=1e-12)
    Q = start_poses(np.eye(4), yaw_deg=(30.0,), axis=(1, 0, 0), center=(0.0, 0.0, 0.0))
    assert np.allclose(Q[0][:3, :3], rotation((1, 0, 0), 30.0), atol=1e-6) and np.allclose(Q[0][:3, 3], 0.0)


def test_new_kernels_register_budget():
    """k_knn_bvh_post_multi<3, .> keeps its single-start sibling's budget (80 VGPRs: 6 waves per SIMD, no scratch); the colour matcher,
    the stand-alone matcher, the post stages and k_reduce_solve_multi have no scratch either."""
    seen = kernel_resources(device_asm())

    def kernels(prefix):
        return {n: f for n, f in seen.items() if n.startswith("_ZN6icpdev" + prefix)}
    ks = kernels("20k_knn_bvh_post_multiILi3ELb")
    assert len(ks) == 2, list(ks)
    for name, f in ks.items():
        assert f["num_vgpr"] <= 80 and f["private_seg_size"] == 0, (name, f)
    for prefix, count in (("20k_knn_bvh_post_multiILi6ELb", 2), ("15k_knn_bvh_multiILi", 2), ("20k_reduce_solve_multi", 1), ("12k_post_multi", 1),
                          ("22k_sym_accumulate_multi", 1), ("13k_score_multi", 1)):
        ks = kernels(prefix)
        assert len(ks) == count, (prefix, list(ks))
        for name, f in ks.items():
            assert f["private_seg_size"] == 0, (name, f)
