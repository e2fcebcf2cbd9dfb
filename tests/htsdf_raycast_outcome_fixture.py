"""The outcome fixture of frame-to-model tracking on the HASHED volume (tests/test_gpu_htsdf_raycast.py): the
41-frame, 60 degree pan of tests/tsdf_outcome_fixture.py, which frame-0 tracking loses and a short dense box loses silently, tracked on
the CPU by the loop of icp_track_depth_model_hashed -- the hashed restatement's touch and integrate (tests/htsdf_restatement.py), the
restated ray-cast of the blocks (tests/htsdf_raycast_restatement.py) and the oracle's ICP with tsdf_outcome_fixture's parameters -- on a
hashed volume with that fixture's origin, voxel size, truncation and ray step, and no extent.  Run as a script (CPU only, a few minutes)
it writes the worst-frame and last-frame rotation and translation errors and the block count to tests/golden/htsdf_raycast_outcome.json:
the reference the device's bound is twice of."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "htsdf_raycast_outcome.json")
f32 = np.float32


def hashed_model():
    """tum.track's model dict: the dense fixture's options without its dims, tracked against the ray-cast of the blocks."""
    import tsdf_outcome_fixture as OF
    m = {k: v for k, v in OF.VOLUME.items() if k != "dims"}
    m.update(hashed=True, raycast=True)
    return m


def restatement_track(orc):
    """tsdf_restatement.track's composition on the hashed volume.  Returns (poses, gt, blocks after every frame, hits of every ray-cast)."""
    import htsdf_raycast_restatement as RR
    import htsdf_restatement as HR
    import tsdf_restatement as TS
    import tsdf_outcome_fixture as OF
    K, depth, gt = OF.fixture()
    cam = TS.Camera(K, OF.W, OF.H)
    opts = {k: v for k, v in OF.VOLUME.items() if k != "dims"}
    vol = HR.HVolume(**opts)
    prm = orc.make_params(metric=1, matching=0, weighting=0, rejection=1, n_iterations=35, max_distance=0.1, solver_mode=1, knn_kdtree=1)
    eye = np.eye(4, dtype=f32)
    pose = eye.copy()
    HR.integrate(vol, depth[0], cam, pose)
    poses, n_blocks, hits_of = [pose.copy()], [len(vol.blocks)], []
    for k in range(1, len(depth)):
        _, vert, nrm, hits = RR.raycast(RR.Blocks(*vol.sorted_blocks(), **opts), cam, pose)
        xyz, snr, _, valid = orc.backproject(depth[k], None, K, max_distance=0.1)
        idx = np.arange(0, OF.W * OF.H, OF.SOURCE_FACTOR)
        sel = idx[valid[idx]]
        dT = None
        if hits > 0 and len(sel) > 0:
            ok = np.isfinite(vert).all(1) & np.isfinite(nrm).all(1)
            try:
                dT, _ = orc.estimate_pose(prm, xyz[sel], snr[sel], None, vert[ok], nrm[ok], None, eye)
            except RuntimeError:
                dT = None
            if dT is not None and not np.isfinite(dT).all():
                dT = None
        if dT is not None:
            pose = TS.compose_pose(pose, dT)
            HR.integrate(vol, depth[k], cam, pose)
        poses.append(pose.copy()); n_blocks.append(len(vol.blocks)); hits_of.append(int(hits))
        print("frame %d: %d hits, %d blocks, error %s" % (k, hits, len(vol.blocks), OF.pose_error(pose, gt[k - 1])), file=sys.stderr)
    return poses, gt, n_blocks, hits_of, vol


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle import oracle
    import tsdf_outcome_fixture as OF
    oracle.build()
    poses, gt, n_blocks, hits_of, vol = restatement_track(oracle)
    rot, tr, last = OF.worst_errors(poses, gt)
    out = dict(worst_rotation_rad=rot, worst_translation_m=tr, last_rotation_rad=last[0], last_translation_m=last[1], frames=OF.N_FRAMES, width=OF.W, height=OF.H,
               voxel_size=OF.VOLUME["voxel_size"], truncation=OF.VOLUME["truncation"], ray_step=OF.VOLUME["ray_step"], n_blocks=n_blocks[-1],
               n_blocks_first=n_blocks[0], min_hits=min(hits_of), n_out_of_range=vol.n_out_of_range)
    print(json.dumps(out))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
