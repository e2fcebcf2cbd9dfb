"""The outcome fixture of the coloured model (tests/test_gpu_tsdf_color.py): a camera that faces a flat textured wall
squarely and slides sideways, 1 cm per frame, 12 frames of 160 x 120.  The wall's geometry leaves the lateral pose free; its texture does
not.  `fixture()` builds the frames; run as a script (CPU only, about a minute) it tracks them twice with the numpy restatements -- the
coloured model loop (tsdf_color_restatement.track with colored_restatement.step) and the geometric one (tsdf_restatement.track with the
oracle's point-to-plane ICP) -- and writes the worst translation error of both to tests/golden/tsdf_color_outcome.json: the reference the
device's bound is twice of, and the check that the fixture separates the two loops before any device sees it."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
N_FRAMES, W, H = 12, 160, 120
STEP_M, WALL_Z, SIGMA = 0.01, 1.5, 0.001
# just large enough: the wall seen through 160 x 120 at 1.5 m is 1.83 m x 1.37 m, the camera travels 0.11 m along x; the band is 4 voxels
VOLUME = dict(dims=(58, 40, 13), origin=(-1.0, -0.78, 1.26), voxel_size=0.04, truncation=0.16, max_weight=64.0, min_depth=1.0, max_depth=2.0, ray_step=0.0)
SOURCE_FACTOR = 4
ITERATIONS, MAX_DISTANCE, LAMBDA, GRADIENT_K = 35, 0.1, 0.968, 20
GOLDEN = os.path.join(HERE, "golden", "tsdf_color_outcome.json")


def texture(x, y):
    """The wall's colour at (x, y) [m], bytes per channel: smooth, deterministic, and not periodic over the field of view (incommensurate
    wavelengths along oblique directions); the shortest wavelength is 0.37 m, more than 9 voxels of 0.04 m."""
    r = 128 + 60 * np.sin(2 * np.pi * (x + 0.31 * y) / 0.61) + 50 * np.sin(2 * np.pi * (0.45 * x - y) / 0.43)
    g = 120 + 70 * np.cos(2 * np.pi * (x - 0.22 * y) / 0.37) + 40 * np.sin(2 * np.pi * (0.3 * x + y) / 0.79)
    b = 110 + 55 * np.sin(2 * np.pi * (0.8 * x + 0.6 * y) / 0.53 + 1.0) + 45 * np.cos(2 * np.pi * (x + 0.1 * y) / 0.97)
    return np.stack([r, g, b], -1)


def fixture(n_frames=N_FRAMES):
    """(K, depth (n, H, W), rgbx (n, W*H, 4), gt: n - 1 transforms frame k -> frame 0).  The depth carries the sensor's noise (sigma 1 mm,
    seeded) and its 1/5000 m quantisation, so that no linear system is exactly singular."""
    from icp_amd import synth
    K = synth.tum_K(W)
    fx, fy, cx, cy = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    depth, rgbx, gt = [], [], []
    for k in range(n_frames):
        rng = np.random.Generator(np.random.MT19937(0xC010 + k))
        tx = STEP_M * k
        d = np.round((WALL_Z + rng.normal(0.0, SIGMA, (H, W))) * 5000.0) / 5000.0
        x = (u - cx) / fx * WALL_Z + tx; y = (v - cy) / fy * WALL_Z
        c = np.clip(np.floor(texture(x, y) + 0.5), 0, 255).astype(np.uint8).reshape(-1, 3)
        depth.append(d.astype(f32)); rgbx.append(np.concatenate([c, np.full((W * H, 1), 255, np.uint8)], 1))
        if k:
            T = np.eye(4, dtype=f32); T[0, 3] = tx
            gt.append(T)
    return K, np.stack(depth), np.stack(rgbx), gt


def translation_errors(poses, gt):
    """Per frame 1 .. n - 1 the translation error [m] against the truth."""
    return [float(np.linalg.norm(np.asarray(P, np.float64)[:3, 3] - np.asarray(G, np.float64)[:3, 3])) for P, G in zip(poses[1:], gt)]


def restatement_tracks(orc):
    """(poses of the coloured model loop, poses of the geometric model loop, gt), both on the CPU."""
    import colored_restatement as CR
    import tsdf_color_restatement as TC
    import tsdf_restatement as TS
    from scipy.spatial import cKDTree
    K, depth, rgbx, gt = fixture()
    cam = TS.Camera(K, W, H)
    eye = np.eye(4, dtype=f32)
    idx = np.arange(0, W * H, SOURCE_FACTOR)

    def source_of(k):
        xyz, nrm, rgba, valid = orc.backproject(depth[k], rgbx[k], K, max_distance=MAX_DISTANCE, fix_color_index=True)
        sel = idx[valid[idx]]
        return xyz[sel], nrm[sel], rgba[sel]

    def estimate_colored(src, tgt):
        """The colored metric's free-running loop: 3-D nearest neighbour within MAX_DISTANCE, the 60 degree normal rejection, constant weights."""
        tp, tn, tc = tgt
        ok = np.isfinite(tp).all(1) & np.isfinite(tn).all(1)
        tp, tn, tc = tp[ok], tn[ok], tc[ok]
        grad, _ = CR.gradients(tp, tn, tc, GRADIENT_K)
        tree = cKDTree(tp.astype(np.float64))
        pose = eye.copy()
        for _ in range(ITERATIONS):
            p = CR.transform(pose, src[0])
            dist, j = tree.query(p.astype(np.float64))
            sn = src[1].astype(np.float64) @ pose[:3, :3].astype(np.float64).T
            keep = (dist <= MAX_DISTANCE) & ((sn * tn[j]).sum(1) > 0.5)
            if keep.sum() < 6:
                return None
            pose, _ = CR.step(pose, src[0][keep], tp[j[keep]], tn[j[keep]], grad[j[keep]], src[2][keep], tc[j[keep]], np.ones(keep.sum(), f32), LAMBDA)
            if not np.isfinite(pose).all():
                return None
        return pose
    poses_c = TC.track(TC.add_color(TS.Volume(**VOLUME)), depth, rgbx, cam, eye, source_of, estimate_colored)

    prm = orc.make_params(metric=1, matching=0, weighting=0, rejection=1, n_iterations=ITERATIONS, max_distance=MAX_DISTANCE, solver_mode=1, knn_kdtree=1)

    def estimate_plane(src, tgt):
        ok = np.isfinite(tgt[0]).all(1) & np.isfinite(tgt[1]).all(1)
        try:
            dT, _ = orc.estimate_pose(prm, src[0], src[1], None, tgt[0][ok], tgt[1][ok], None, eye)
        except RuntimeError:
            return None
        return dT if np.isfinite(dT).all() else None
    poses_g = TS.track(TS.Volume(**VOLUME), depth, cam, eye, lambda k: source_of(k)[:2], estimate_plane)
    return poses_c, poses_g, gt


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle import oracle
    oracle.build()
    poses_c, poses_g, gt = restatement_tracks(oracle)
    ec, eg = translation_errors(poses_c, gt), translation_errors(poses_g, gt)
    travel = STEP_M * (N_FRAMES - 1)
    out = dict(colored_worst_translation_m=max(ec), colored_last_translation_m=ec[-1], geometric_worst_translation_m=max(eg),
               geometric_last_translation_m=eg[-1], lateral_travel_m=travel, frames=N_FRAMES, width=W, height=H)
    print(json.dumps(out))
    print("coloured loop per frame:", " ".join("%.4f" % e for e in ec))
    print("geometric loop per frame:", " ".join("%.4f" % e for e in eg))
    assert 2 * max(ec) < travel / 2 < eg[-1], "the fixture does not separate the two loops"
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
