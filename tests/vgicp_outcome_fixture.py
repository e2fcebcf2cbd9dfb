"""The outcome fixture of voxelized GICP (tests/test_gpu_vgicp.py): synth.eth_like_pair(0, 86, 270) (23 220 points,
1 cm range noise) aligned by the numpy restatement (tests/vgicp_restatement.py) from the identity with the clouds' own normals
(covariance_k = 0), epsilon 1e-3, voxel 0.25 m, 30 iterations, stops off.  Run as a script (CPU only, under a minute) it writes the final
rotation and translation error against the pair's truth to tests/golden/vgicp_outcome.json -- the reference the device's bound is twice of."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "vgicp_outcome.json")
PAIR = (0, 86, 270)
EPSILON = 1e-3
OPTIONS = dict(voxel_size=0.25, min_points=1, n_iterations=30, min_valid=64, stop_rotation=0.0, stop_translation=0.0)


def pose_error(A, B):
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64)
    R = A[:3, :3] @ B[:3, :3].T
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(s, (np.trace(R) - 1) / 2)), float(np.linalg.norm(A[:3, 3] - B[:3, 3]))


def pair():
    from icp_amd import synth
    return synth.eth_like_pair(*PAIR)


def restatement_align(d):
    import vgicp_restatement as VR
    g = VR.grid(d["tgt_pts"], d["tgt_nrm"], OPTIONS["voxel_size"])
    pose, rec, trace = VR.align(g, d["src_pts"], d["src_nrm"], np.eye(4, dtype=np.float32), EPSILON, **OPTIONS)
    return g, pose, rec, trace


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    d = pair()
    g, pose, rec, trace = restatement_align(d)
    rot, tr = pose_error(pose, d["gt"])
    rot0, tr0 = pose_error(np.eye(4), d["gt"])
    out = dict(rotation_rad=rot, translation_m=tr, identity_rotation_rad=rot0, identity_translation_m=tr0, points=int(len(d["src_pts"])),
               voxel_size=OPTIONS["voxel_size"], epsilon=EPSILON, n_iterations=OPTIONS["n_iterations"], iterations=rec["iterations"], status=rec["status"],
               n_valid_first=rec["n_valid_first"], n_valid_last=rec["n_valid_last"], cost_first=rec["cost_first"], cost_last=rec["cost_last"],
               dims=[int(x) for x in g["dims"]], n_occupied=g["n_occupied"])
    print(json.dumps(out))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
