"""The outcome fixture of direct SDF tracking with the photometric term (tests/test_gpu_sdf_color.py): the textured
wall of tests/tsdf_color_outcome_fixture.py -- 12 frames of 160 x 120, the camera sliding 1 cm per frame along a flat wall whose geometry
leaves the lateral pose free -- tracked at stride 2 with 20 iterations, the default stops, weight 0.1 and the colour Huber off.  Run as a
script (CPU only) it tracks the frames twice with the numpy restatements, once coloured (sdf_color_restatement.track) and once with
sdf_restatement alone, asserts that the fixture separates the two and writes tests/golden/sdf_color_outcome.json: the reference the
device's bound is twice of."""
import json
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sdf_color_outcome.json")
OPTIONS = dict(stride=2, n_iterations=20)
COLOR_OPTIONS = dict(weight=0.1, huber=0.0)


def restatement_tracks():
    """(poses and records of the coloured loop, poses and records of the geometric loop, gt), both on the CPU."""
    import sdf_color_restatement as SC
    import sdf_restatement as SR
    import tsdf_color_restatement as TC
    import tsdf_restatement as TS
    import tsdf_color_outcome_fixture as CF
    K, depth, rgbx, gt = CF.fixture()
    cam = TS.Camera(K, CF.W, CF.H)
    eye = np.eye(4, dtype=np.float32)
    colored = SC.track(TC.add_color(TS.Volume(**CF.VOLUME)), depth, rgbx, cam, eye, weight=COLOR_OPTIONS["weight"], color_huber=COLOR_OPTIONS["huber"], **OPTIONS)
    geometric = SR.track(TS.Volume(**CF.VOLUME), depth, cam, eye, **OPTIONS)
    return colored, geometric, gt


if __name__ == "__main__":
    root = os.path.abspath(os.path.join(HERE, ".."))
    for p in (root, os.path.join(root, "icp-variants_amd", "python"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import tsdf_color_outcome_fixture as CF
    (poses_c, recs_c), (poses_g, recs_g), gt = restatement_tracks()
    ec, eg = CF.translation_errors(poses_c, gt), CF.translation_errors(poses_g, gt)
    travel = CF.STEP_M * (CF.N_FRAMES - 1)
    out = dict(colored_worst_translation_m=max(ec), colored_last_translation_m=ec[-1], geometric_worst_translation_m=max(eg),
               geometric_last_translation_m=eg[-1], lateral_travel_m=travel, frames=CF.N_FRAMES, width=CF.W, height=CF.H,
               stride=OPTIONS["stride"], n_iterations=OPTIONS["n_iterations"], weight=COLOR_OPTIONS["weight"],
               colored_statuses=sorted(set(r["status"] for r in recs_c)), colored_iterations=[r["iterations"] for r in recs_c],
               geometric_iterations=[r["iterations"] for r in recs_g])
    print(json.dumps(out))
    print("coloured loop per frame:", " ".join("%.4f" % e for e in ec))
    print("geometric loop per frame:", " ".join("%.4f" % e for e in eg))
    assert 2 * max(ec) < travel / 2 < eg[-1], "the fixture does not separate the two trackers"
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
