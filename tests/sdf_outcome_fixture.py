"""The outcome fixture of direct SDF tracking (tests/test_gpu_sdf.py): the 41-frame, 60 degree pan of
tests/tsdf_outcome_fixture.py tracked by the numpy restatement (tests/sdf_restatement.py) at stride 4 with 20 iterations and the default
stops.  Run as a script (CPU only, well under a minute) it writes the worst rotation and translation error to tests/golden/sdf_outcome.json,
in the shape of tsdf_outcome.json -- the reference the device's bound is twice of."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sdf_outcome.json")
OPTIONS = dict(stride=4, n_iterations=20)


def restatement_track():
    import sdf_restatement as SR
    import tsdf_restatement as TS
    import tsdf_outcome_fixture as OF
    K, depth, gt = OF.fixture()
    poses, recs = SR.track(TS.Volume(**OF.VOLUME), depth, TS.Camera(K, OF.W, OF.H), np.eye(4, dtype=np.float32), **OPTIONS)
    return poses, recs, gt


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import tsdf_outcome_fixture as OF
    poses, recs, gt = restatement_track()
    rot, tr, last = OF.worst_errors(poses, gt)
    out = dict(worst_rotation_rad=rot, worst_translation_m=tr, last_rotation_rad=last[0], last_translation_m=last[1], frames=OF.N_FRAMES, width=OF.W, height=OF.H,
               stride=OPTIONS["stride"], n_iterations=OPTIONS["n_iterations"], statuses=sorted(set(r["status"] for r in recs)),
               iterations=[r["iterations"] for r in recs])
    print(json.dumps(out))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
