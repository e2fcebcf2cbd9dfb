"""The outcome fixture of laser scans tracked against the TSDF volume they are fused into (tests/test_gpu_sdf_cloud.py, DESIGN.md section
6zf): the twelve synthetic scans of tests/tsdf_cloud_outcome_fixture.py (imported, not edited: 10 cm voxels, truncation 0.4 m, steps of
0.40 m and 0.03 to 0.11 rad, 1 cm range noise), scan 0 fused at its true pose and every later scan aligned to the model built so far and fused
at the pose found, all by the numpy restatement (tests/sdf_cloud_restatement.py).  What makes the outcome worth comparing with is asserted
here, on the CPU: every scan aligns, the worst scan ends within MAX_ROT rad and MAX_TRANS m (half a voxel) of its true pose, and the model
the TRACKED poses built passes that fixture's own assert_surface."""
import functools
import numpy as np

import tsdf_cloud_outcome_fixture as CF

f32 = np.float32
N_ITERATIONS = 30
MAX_ROT, MAX_TRANS = 0.02, 0.5 * CF.VOXEL
SDF_OPTIONS = dict(n_iterations=N_ITERATIONS)


def pose_error(T, truth):
    """(rotation angle [rad], translation distance [m]) between two 4x4 poses, in fp64."""
    A, B = np.asarray(T, np.float64), np.asarray(truth, np.float64)
    R = A[:3, :3] @ B[:3, :3].T
    s = 0.5 * np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])      # (atan2: well conditioned near 0, unlike arccos of the trace)
    return float(np.arctan2(s, (np.trace(R) - 1.0) / 2.0)), float(np.linalg.norm(A[:3, 3] - B[:3, 3]))


def worst(poses):
    """The largest rotation and the largest translation error over the scans."""
    errs = [pose_error(T, G) for T, G in zip(poses, CF.scans()[1])]
    return max(e[0] for e in errs), max(e[1] for e in errs)


@functools.lru_cache(maxsize=None)
def tracked():
    """(the restatement's HVolume after the track, poses, records, infos, status).  Shared: do not modify."""
    import sdf_cloud_restatement as SC
    clouds, poses, _ = CF.scans()
    vol = SC.HVolume(**CF.options())
    return (vol,) + SC.track(vol, clouds, poses[0], **SDF_OPTIONS)


def assert_outcome(poses, records, status):
    rot, trans = worst(poses)
    print("tracked against the TSDF: status %d, worst scan %.4f rad and %.4f m from its true pose; valid points %d (scan 1) .. %d (scan %d)"
          % (status, rot, trans, records[0]["n_valid_first"], records[-1]["n_valid_first"], len(records)))
    assert status == 0 and all(r["status"] == 0 for r in records) and len(records) == CF.N_SCANS - 1
    assert rot <= MAX_ROT, rot
    assert trans <= MAX_TRANS, trans
    return rot, trans


if __name__ == "__main__":
    import os
    import sys
    import time
    here = os.path.dirname(os.path.abspath(__file__)); root = os.path.abspath(os.path.join(here, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    t0 = time.time()
    vol, poses, recs, infos, status = tracked()
    print("%.1f s; iterations %s" % (time.time() - t0, [r["iterations"] for r in recs]))
    assert_outcome(poses, recs, status)
    CF.assert_surface(vol)
