"""The outcome fixture of the coloured hashed model loop (tests/test_gpu_htsdf_color_view.py): the textured wall of
tests/tsdf_color_outcome_fixture.py (CF) -- a camera that faces a flat textured wall squarely and slides sideways, 1 cm per frame, 12
frames of 160 x 120 -- tracked on a HASHED volume with that fixture's voxel size, truncation and depth range and no extent.  Run as a script
(CPU only, a few minutes) it tracks the frames twice with the numpy restatements -- the coloured hashed model loop
(htsdf_color_view_restatement.track under the colored metric, CF's estimate_colored) and the geometric hashed ray-cast loop (the same
composition with the target of htsdf_raycast_restatement.raycast under the oracle's point-to-plane ICP) -- and writes the translation errors
of both to tests/golden/htsdf_color_view_outcome.json: the reference the device's bound is twice of, and the check that the fixture
separates the two loops before any device sees it.  The dense golden is not reused: the hashed volume allocates blocks past the dense
box's upper faces, so the two loops are not bit-equal there."""
import json
import os
import sys
import numpy as np

import tsdf_color_outcome_fixture as CF

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32
GOLDEN = os.path.join(HERE, "golden", "htsdf_color_view_outcome.json")
VOLUME = {k: v for k, v in CF.VOLUME.items() if k != "dims"}
BLOCK_CAPACITY = 256


def hashed_model(color=True):
    """The `model` argument of tum.track for the fixture: the coloured ray-cast loop, or the geometric one."""
    return dict(VOLUME, hashed=True, block_capacity=BLOCK_CAPACITY, **(dict(color=True, raycast="color") if color else dict(raycast=True)))


def restatement_tracks(orc):
    """(poses of the coloured hashed model loop, poses of the geometric hashed ray-cast loop, gt, blocks at the end of the coloured loop)."""
    import colored_restatement as CR
    import htsdf_color_restatement as HCR
    import htsdf_color_view_restatement as VR
    import htsdf_restatement as HR
    import tsdf_restatement as TS
    from scipy.spatial import cKDTree
    K, depth, rgbx, gt = CF.fixture()
    cam = TS.Camera(K, CF.W, CF.H)
    eye = np.eye(4, dtype=f32)
    idx = np.arange(0, CF.W * CF.H, CF.SOURCE_FACTOR)

    def source_of(k):
        xyz, nrm, rgba, valid = orc.backproject(depth[k], rgbx[k], K, max_distance=CF.MAX_DISTANCE, fix_color_index=True)
        sel = idx[valid[idx]]
        return xyz[sel], nrm[sel], rgba[sel]

    def estimate_colored(src, tgt):
        """CF's: the colored metric's free-running loop -- 3-D nearest neighbour within MAX_DISTANCE, the 60 degree normal rejection, constant weights."""
        tp, tn, tc = tgt
        ok = np.isfinite(tp).all(1) & np.isfinite(tn).all(1)
        tp, tn, tc = tp[ok], tn[ok], tc[ok]
        grad, _ = CR.gradients(tp, tn, tc, CF.GRADIENT_K)
        tree = cKDTree(tp.astype(np.float64))
        pose = eye.copy()
        for _ in range(CF.ITERATIONS):
            p = CR.transform(pose, src[0])
            dist, j = tree.query(p.astype(np.float64))
            sn = src[1].astype(np.float64) @ pose[:3, :3].astype(np.float64).T
            keep = (dist <= CF.MAX_DISTANCE) & ((sn * tn[j]).sum(1) > 0.5)
            if keep.sum() < 6:
                return None
            pose, _ = CR.step(pose, src[0][keep], tp[j[keep]], tn[j[keep]], grad[j[keep]], src[2][keep], tc[j[keep]], np.ones(keep.sum(), f32), CF.LAMBDA)
            if not np.isfinite(pose).all():
                return None
        return pose

    prm = orc.make_params(metric=1, matching=0, weighting=0, rejection=1, n_iterations=CF.ITERATIONS, max_distance=CF.MAX_DISTANCE, solver_mode=1, knn_kdtree=1)

    def estimate_plane(src, tgt):
        ok = np.isfinite(tgt[0]).all(1) & np.isfinite(tgt[1]).all(1)
        try:
            dT, _ = orc.estimate_pose(prm, src[0], src[1], None, tgt[0][ok], tgt[1][ok], None, eye)
        except RuntimeError:
            return None
        return dT if np.isfinite(dT).all() else None

    hv = HCR.add_color(HR.HVolume(**VOLUME))
    poses_c = VR.track(hv, depth, rgbx, cam, eye, source_of, estimate_colored, ray_step=VOLUME["ray_step"])
    hg = HCR.add_color(HR.HVolume(**VOLUME))
    poses_g = VR.track(hg, depth, rgbx, cam, eye, lambda k: source_of(k)[:2], estimate_plane, ray_step=VOLUME["ray_step"], geometric=True)
    return poses_c, poses_g, gt, len(hv.blocks)


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle import oracle
    oracle.build()
    poses_c, poses_g, gt, n_blocks = restatement_tracks(oracle)
    ec, eg = CF.translation_errors(poses_c, gt), CF.translation_errors(poses_g, gt)
    travel = CF.STEP_M * (CF.N_FRAMES - 1)
    out = dict(colored_worst_translation_m=max(ec), colored_last_translation_m=ec[-1], geometric_worst_translation_m=max(eg),
               geometric_last_translation_m=eg[-1], lateral_travel_m=travel, frames=CF.N_FRAMES, width=CF.W, height=CF.H, n_blocks=n_blocks)
    print(json.dumps(out))
    print("coloured hashed loop per frame:", " ".join("%.4f" % e for e in ec))
    print("geometric hashed loop per frame:", " ".join("%.4f" % e for e in eg))
    assert 2 * max(ec) < travel / 2 < eg[-1], "the fixture does not separate the two loops"
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
