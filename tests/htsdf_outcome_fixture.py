"""The outcome fixture of direct SDF tracking on the HASHED volume (tests/test_gpu_htsdf.py): the 41-frame, 60 degree
pan of tests/tsdf_outcome_fixture.py tracked by the numpy restatement (tests/htsdf_restatement.py) at stride 4 with 20 iterations, with
that fixture's origin, voxel size and truncation and no extent.  Run as a script (CPU only, a few minutes) it writes the worst rotation
and translation error and the number of blocks after every frame to tests/golden/htsdf_outcome.json -- the reference the device's bound
is twice of, and whose block counts the device must meet exactly.  It also tracks the pan with the DENSE restatement in a box cut to
CUT_DIMS at the same origin, which the pan walks out of, and records where that ends: the silent failure the hashed volume removes."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "htsdf_outcome.json")
OPTIONS = dict(stride=4, n_iterations=20)
CUT_DIMS = (100, 69, 177)


def hashed_model():
    """tum.track's model dict for the hashed run: the dense fixture's options without its dims."""
    import tsdf_outcome_fixture as OF
    m = {k: v for k, v in OF.VOLUME.items() if k != "dims"}
    m["hashed"] = True
    return m


def cut_model():
    import tsdf_outcome_fixture as OF
    return dict(OF.VOLUME, dims=CUT_DIMS)


def restatement_track():
    import htsdf_restatement as HR
    import tsdf_restatement as TS
    import tsdf_outcome_fixture as OF
    K, depth, gt = OF.fixture()
    vol = HR.HVolume(**{k: v for k, v in OF.VOLUME.items() if k != "dims"})
    poses, recs, n_blocks = HR.track(vol, depth, TS.Camera(K, OF.W, OF.H), np.eye(4, dtype=np.float32), **OPTIONS)
    return poses, recs, n_blocks, vol, gt


def restatement_track_cut():
    import sdf_restatement as SR
    import tsdf_restatement as TS
    import tsdf_outcome_fixture as OF
    K, depth, gt = OF.fixture()
    poses, recs = SR.track(TS.Volume(**cut_model()), depth, TS.Camera(K, OF.W, OF.H), np.eye(4, dtype=np.float32), **OPTIONS)
    return poses, recs, gt


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import tsdf_outcome_fixture as OF
    poses, recs, n_blocks, vol, gt = restatement_track()
    rot, tr, last = OF.worst_errors(poses, gt)
    cposes, crecs, _ = restatement_track_cut()
    crot, ctr, clast = OF.worst_errors(cposes, gt)
    out = dict(worst_rotation_rad=rot, worst_translation_m=tr, last_rotation_rad=last[0], last_translation_m=last[1], frames=OF.N_FRAMES, width=OF.W, height=OF.H,
               stride=OPTIONS["stride"], n_iterations=OPTIONS["n_iterations"], statuses=sorted(set(r["status"] for r in recs)),
               iterations=[r["iterations"] for r in recs], n_blocks=n_blocks, n_out_of_range=vol.n_out_of_range,
               cut_dims=list(CUT_DIMS), cut_last_rotation_rad=clast[0], cut_last_translation_m=clast[1], cut_worst_rotation_rad=crot, cut_worst_translation_m=ctr,
               cut_statuses=sorted(set(r["status"] for r in crecs)))
    print(json.dumps(out))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
